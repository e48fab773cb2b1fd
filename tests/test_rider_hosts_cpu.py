"""The rider cases of tests/rider_check.py on the executable specification (fake_t3d.FakeLib): each rider kind as a set of its own, the
mixed dependent chains, the hand-built `depends` patterns, the `_r` entry points on forms that do not host, and the refusals -- the same
functions tests/test_rider_hosts_gpu.py runs on the device, so the cases (inputs, guard bands, barrier-word rule) are validated without one."""
import ctypes as C

import pytest

import rider_check as rc
from fake_t3d import FakeLib
from transferable3d_amd import abi


@pytest.fixture
def env():
    return rc.Env(FakeLib(), 'cpu')


@pytest.mark.parametrize('case_id,factory,args', rc.KIND_CASES, ids=[c[0] for c in rc.KIND_CASES])
def test_each_rider_kind_as_a_set_of_its_own(env, case_id, factory, args):
    rs = rc.check_set_alone(env, factory(*args), what=case_id)
    assert rs.n_ops == 1 and 1 <= rs.n_wg <= rc.RIDER_MAX_WG


@pytest.mark.parametrize('M,K,N,rpf', rc.MID_SHAPES)
def test_wide_rider_pool_bwd_mid(env, M, K, N, rpf):
    rc.check_wide_rider(env, M, K, N, rpf)


@pytest.mark.parametrize('n_ops', [abi.RIDER_MAX_OPS, 2])
def test_dependent_chain_of_mixed_kinds(env, n_ops):
    rc.check_set_alone(env, rc.fc_head_bwd_case(n_ops), what='head backward, %d ops' % n_ops)


@pytest.mark.parametrize('pattern', [(0, 0, 0, 0), (0, 1, 0, 1)], ids=['independent', '0101'])
def test_hand_built_sets_without_barriers(env, pattern):
    rc.check_set_alone(env, rc.independent_case(pattern), depends=list(pattern), what='depends=%s' % (pattern,))


@pytest.mark.parametrize('name', [n[0] for n in rc.NON_HOSTING if n[4]])
def test_r_call_on_a_form_that_does_not_host(env, name):
    rc.check_non_hosting(env, name)


def test_riders_plan_refusals(env):
    rc.check_plan_refusals(env)


def test_run_riders_and_r_launcher_refusals(env):
    rc.check_launch_refusals(env)


def test_hosts_riders_queries_refuse_what_the_launchers_refuse(env):
    rc.check_query_refusals(env)


def test_design_md_carries_the_generated_table():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'DESIGN.md')).read()
    assert rc.forms_markdown() in text, 'DESIGN.md: regenerate the rider-form table (python tools/rider_forms_table.py)'
