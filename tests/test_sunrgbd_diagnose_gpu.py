"""GPU: the detection-error diagnosis through libt3d.so (t3d_sunrgbd_diagnose): the cases of tests/sunrgbd_diagnose_check.py that
tests/test_sunrgbd_diagnose_cpu.py runs through the NumPy specification (tests/fake_sunrgbd_diagnose.py) -- the hand case, the generated
cases against the specification, the properties, the edge cases, the refusals and both command lines.

Tolerance of other_overlap and ap_fixed against the specification: both go through code that tests/test_sunrgbd_eval_gpu.py bounds with
min(8 x measured worst, 1e-9) -- the two fp64 clips (boundary integral on the device, Sutherland-Hodgman vertex list in the restatement)
and the AP sum in another order.  MEASURED_WORST is the larger of the worst |other_overlap difference| and the worst |ap_fixed
difference| on the generated cases on the MI355X (docs/EXPERIMENTS.md); the bound is 8 times it, capped at 1e-9.  The discrete
outputs get no tolerance."""
import pytest

import sunrgbd_diagnose_check as DK
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MEASURED_WORST = 7.105e-15      # |other_overlap difference| of the small case; large: 6.5e-15; the worst |ap_fixed difference| was 1.7e-16
BOUND = 1e-9 if MEASURED_WORST is None else min(8.0 * MEASURED_WORST, 1e-9)


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def test_hand_case(rt):
    DK.check_hand_case(rt)


def test_hand_case_logged_lines_json_and_curves(rt, tmp_path):
    DK.check_hand_lines(rt, tmp_path)


def test_generated_small_equals_the_specification(rt):
    """300 images, 3 000 boxes, 9 000 detections over ten classes: about 900 detections per class, the curve kernel runs with empty threads."""
    DK.check_conditions('small')
    DK.check_against_spec(rt, 'small', BOUND)


def test_generated_large_class_equals_the_specification(rt):
    """One class of 1 500 images, 15 000 boxes, 45 000 detections: ragged chunks of more than one element in the curve kernel."""
    DK.check_conditions('large')
    DK.check_against_spec(rt, 'large', BOUND)


def test_properties(rt):
    DK.check_properties(rt, BOUND)


def test_edge_cases(rt):
    DK.check_edge_cases(rt)


def test_refusals(hip_lib):
    DK.check_refusals(hip_lib)


def test_command_line_adds_exactly_the_new_lines(rt, tmp_path):
    DK.check_command_line(rt, tmp_path)


def test_detect_official_eval_diagnose_end_to_end(rt, tmp_path):
    print('\n'.join(DK.check_detect_official_eval_diagnose(rt, tmp_path)))
