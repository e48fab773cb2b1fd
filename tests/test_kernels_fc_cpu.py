"""The FC kernel cases of tests/fc_check.py on the executable specification (fake_t3d.FakeLib): the same functions
tests/test_kernels_fc_gpu.py runs on the device, so the cases (inputs, guard bands, padding columns, refusals, pairs) are validated without
one -- plus what only the host can check: that every backward case keeps its activation margin, that the K = 1096 reduction stays far
inside the tolerance with a float32 accumulator, that the case tables catch deliberately wrong libraries, and the specification itself
against autograd in fp64."""
import os

import pytest

import fc_check as fc
from fake_t3d import FakeLib


@pytest.fixture
def env():
    return fc.Env(FakeLib(), 'cpu')


# ---- 1. the FC kernels at their edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.CASE_IDS)
def test_fc_against_spec(env, cid):
    fc.check_case(env, cid)


def test_every_backward_case_keeps_its_activation_margin():
    assert sum(fc.check_margins(cid) for cid in fc.CASE_IDS) >= 40      # (the relu / leaky_relu backward cases were looked at)


def test_the_margin_check_sees_a_violation():
    case = fc.make('bwd-rows-B33')
    f = dict(case.facts)
    y = f['y'].copy()
    y[3, 5] = f['mean'][5] - f['beta'][5] / (f['gamma'][5] * f['invstd'][5])      # z = 0 up to rounding
    assert fc.margin_violations(y, f['mean'], f['invstd'], f['gamma'], f['beta'], True)[3, 5]
    assert not fc.margin_violations(fc.nudge_margin(y, f['mean'], f['invstd'], f['gamma'], f['beta'], True), f['mean'], f['invstd'], f['gamma'],
                                    f['beta'], True).any()


@pytest.mark.parametrize('B', fc.FORM_B)
def test_long_reduction_stays_inside_the_tolerance_in_float32(B):
    fc.check_long_reduction_in_float32(B)


@pytest.mark.parametrize('rid', fc.REFUSAL_IDS)
def test_fc_refusals(env, rid):
    fc.check_refusal(env, rid)


def test_fc_null_struct(env):
    fc.check_null_struct(env)


@pytest.mark.parametrize('mutant', list(fc.MUTANTS), ids=lambda m: m.__name__)
def test_a_wrong_library_is_caught(mutant):
    must, must_not = fc.MUTANTS[mutant]
    for cid in must:
        assert fc.caught(mutant, cid), '%s is not caught by %s' % (mutant.__name__, cid)
    for cid in must_not:
        assert not fc.caught(mutant, cid), '%s: %s fails although the mutation does not reach its shape' % (mutant.__name__, cid)


@pytest.mark.parametrize('form', fc.AUTOGRAD_FORMS)
def test_spec_against_autograd(form):
    fc.check_spec_against_autograd(form)


# ---- 2. the rider form ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.RIDER_IDS)
def test_fc_rider_form(env, cid):
    fc.check_rider(env, cid)


# ---- 3. t3d_small_pair ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', fc.PAIRED_IDS)
def test_fc_case_in_a_pair(env, cid):
    fc.check_case_in_a_pair(env, cid)


@pytest.mark.parametrize('pid', fc.PAIR_IDS)
def test_small_pair(env, pid):
    fc.check_pair_id(env, pid)


@pytest.mark.parametrize('rid', fc.PAIR_REFUSAL_IDS)
def test_small_pair_refusals(env, rid):
    fc.check_pair_refusal(env, rid)


@pytest.mark.parametrize('dense', [1, 0])
def test_bn_bwd_frozen_with_null_statistics(env, dense):
    fc.check_bn_bwd_frozen(env, dense)


def test_gpu_module_docstring_carries_the_form_table():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_kernels_fc_gpu.py')).read()
    assert fc.forms_text() in text, 'tests/test_kernels_fc_gpu.py: its FORM COVERAGE table is not fc_check.forms_text()'
