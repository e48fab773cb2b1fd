"""GPU: the rescoring entry points through libt3d.so (t3d_rescore_features, t3d_rescore_fit, t3d_rescore_apply): the cases and checkers
of tests/rescore_check.py that tests/test_rescore_cpu.py runs through the NumPy specification (tests/fake_rescore.py).  Every bound and
where it comes from is written down at the head of tests/rescore_check.py; the one measured number, the worst difference of the
standardised coefficients against the specification, is `rescore_check.MEASURED_WORST`."""
import pytest

import rescore_check as RK
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def test_features(rt):
    RK.check_features(rt)


def test_apply(rt):
    RK.check_apply(rt)


def test_fit_every_shape(rt):
    """n from 1 over the wave, the workgroup and the slice to three slices and five rows, F in {1, 3, 7, 15}, ld > F with NaN in the padding
    columns, a third of the weights 0 and a third fractions."""
    RK.check_fit_shapes(rt)


def test_equal_bytes(rt):
    RK.check_equal_bytes(rt)


def test_zero_weight_rows_move_the_slice_cuts_not_the_model(rt):
    RK.check_slice_cut(rt)


def test_collinear_columns(rt):
    RK.check_collinear(rt)


def test_the_halving_rule_is_taken_and_the_losses_never_increase(rt):
    RK.check_halving(rt)


def test_status_cases(rt):
    RK.check_status_cases(rt)


def test_refusals(hip_lib):
    RK.check_refusals(hip_lib)


def test_recovery_of_a_known_model(rt):
    RK.check_recovery(lambda X, y, r, lam: RK.call_fit(rt, X, y, r, lam))


def test_model_saved_and_reloaded_gives_the_same_bytes(rt, tmp_path):
    RK.check_model_round_trip(rt, tmp_path)


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
