"""CPU: the rescoring entry points through the NumPy specification (tests/fake_rescore.py) -- the cases and checkers of
tests/rescore_check.py that tests/test_rescore_gpu.py runs through libt3d.so -- and what needs no device at all: the specification's own
statistics, the model file, the option checks, the header's constants."""
import os
import re

import numpy as np
import pytest

import fake_rescore as FR
import rescore_check as RK
from transferable3d_amd import abi
from transferable3d_amd import rescore as RS
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def rt():
    return Runtime(device='cpu', lib=FR.FakeRescoreLib())


def test_header_constants_and_struct_fields_match_the_bindings():
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    const = lambda name: int(re.search(r'#define %s (\d+)' % name, h).group(1))
    assert const('T3D_RESCORE_MAX_FEATURES') == abi.RESCORE_MAX_FEATURES and const('T3D_RESCORE_SLICE') == abi.RESCORE_SLICE
    assert const('T3D_RESCORE_MAX_HALVINGS') == abi.RESCORE_MAX_HALVINGS and const('T3D_RESCORE_N_FEATURES') == len(abi.RESCORE_FEATURES)
    for k, name in enumerate(abi.RESCORE_FEATURES):
        assert const('T3D_RESCORE_F_%s' % name.upper()) == 1 << k
    for bit, name in abi.RESCORE_STATUS.items():
        assert const('T3D_RESCORE_%s' % name.upper()) == bit
    import ctypes as C
    for cname, cls in (('rescore_features_args', abi.RescoreFeaturesArgs), ('rescore_fit_args', abi.RescoreFitArgs),
                       ('rescore_apply_args', abi.RescoreApplyArgs)):
        assert const('T3D_V2_SIZE_%s' % cname) == C.sizeof(cls)
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*t3d_%s;' % cname, h).group(1), flags=re.S)
        names = [re.findall(r'(\w+)\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
        assert names == [f[0].rstrip('_') for f in cls._fields_], cname
    assert abi.rescore_fit_workspace_bytes(1) == (128 + 368) * 8 and abi.rescore_fit_workspace_bytes(abi.RESCORE_SLICE + 1) == (128 + 2 * 368) * 8
    assert abi.rescore_fit_workspace_bytes(0) == 128 * 8


def test_features(rt):
    RK.check_features(rt)


def test_apply(rt):
    RK.check_apply(rt)


def test_fit_every_shape(rt):
    RK.check_fit_shapes(rt)


def test_equal_bytes(rt):
    RK.check_equal_bytes(rt)


def test_zero_weight_rows_move_the_slice_cuts_not_the_model(rt):
    RK.check_slice_cut(rt)


def test_collinear_columns(rt):
    RK.check_collinear(rt)


def test_status_cases(rt):
    RK.check_status_cases(rt)


def test_refusals():
    RK.check_refusals(FR.FakeRescoreLib())


def test_the_specification_recovers_a_known_model():
    """The seeds of the recovery test pass on the specification alone (so a failure on the device is the device's)."""
    RK.check_recovery(lambda X, y, r, lam: FR.fit(X, y, r, lam))


def test_recovery_through_the_entry_point(rt):
    RK.check_recovery(lambda X, y, r, lam: RK.call_fit(rt, X, y, r, lam))


def test_model_saved_and_reloaded_gives_the_same_bytes(rt, tmp_path):
    RK.check_model_round_trip(rt, tmp_path)


def test_the_halving_rule_is_taken_and_the_losses_never_increase(rt):
    RK.check_halving(rt)


def test_option_checks():
    assert RS.feature_mask(RS.FEATURES) == 127 and RS.feature_mask(('score', 'logit_prob')) == 3
    assert RS.ordered(('log_mask', 'score')) == ['score', 'log_mask']
    for bad in ((), ('score', 'score'), ('nope',)):
        with pytest.raises(ValueError):
            RS.feature_mask(bad)
    assert RS.check_min_rescore(None) is None and RS.check_min_rescore(0.25) == 0.25
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='min_rescore'):
            RS.check_min_rescore(bad)
    assert RS.status_names(abi.RESCORE_NOT_CONVERGED | abi.RESCORE_CONSTANT_COLUMN) == ['constant_column', 'not_converged']
    with pytest.raises(ValueError):
        RS.Model(('score',), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        RS.Model(('score',), [1.0, 2.0], target='iou')


def test_detect_with_a_model_records_legends_rows_and_result_files(rt, tmp_path):
    RK.check_detect_flow(rt, tmp_path)


def test_min_rescore_rejects_before_the_groups_and_the_suppression_ranks_by_the_model(rt, tmp_path):
    RK.check_accept_and_ranking(rt, tmp_path)


def test_autolabel_with_the_two_flags(rt, tmp_path):
    RK.check_autolabel_flow(rt, tmp_path)


def test_rescore_fit_command_line(rt, tmp_path):
    RK.check_fit_command(rt, tmp_path)


def test_constructed_case_background_has_low_reproj_iou(rt):
    RK.check_constructed_case(rt)
