"""GPU: the split of the localisation errors through libt3d.so (t3d_sunrgbd_locparts): the cases of tests/sunrgbd_locparts_check.py that
tests/test_sunrgbd_locparts_cpu.py runs through the NumPy specification (tests/fake_sunrgbd_locparts.py) -- the hand case, the generated
cases against the specification, the properties, the edge cases, the refusals and both command lines.

Tolerance of part_overlap, loc_error and ap_part against the specification, by the convention of tests/test_sunrgbd_diagnose_gpu.py:
min(8 x measured worst, 1e-9).  part_overlap goes through the two fp64 clips (boundary integral on the device, Sutherland-Hodgman vertex
list in the restatement), ap_part through the AP sum in another order, loc_error through hypot, log and atan2 of two libraries.
MEASURED_WORST is the largest |difference| of the three on the generated cases on the MI355X against the specification
(docs/EXPERIMENTS.md).  The discrete outputs get no tolerance."""
import pytest

import sunrgbd_locparts_check as LK
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu

MEASURED_WORST = 1.732e-14     # |part_overlap difference| of the large class; small: 1.654e-14; loc_error 2.2e-16 and ap_part 1.7e-16 at worst
BOUND = 1e-9 if MEASURED_WORST is None else min(8.0 * MEASURED_WORST, 1e-9)


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


def test_hand_case(rt):
    LK.check_hand_case(rt)


def test_hand_case_logged_lines_json_and_curves(rt, tmp_path):
    LK.check_hand_lines(rt, tmp_path)


def test_generated_small_equals_the_specification(rt):
    """The ten classes of the diagnosis' small case, about 900 detections each: several 256-thread blocks of (detection, part) lanes and a
    ragged last one."""
    LK.check_conditions('small')
    LK.check_against_spec(rt, 'small', BOUND)


def test_generated_large_class_equals_the_specification(rt):
    """One class of the diagnosis' large case, P > 2048 and no multiple of 1024: ragged chunks of more than one element where the new
    tp_of / fp_of meet the curve's chunking."""
    LK.check_conditions('large')
    LK.check_against_spec(rt, 'large', BOUND)


def test_properties(rt):
    LK.check_properties(rt, BOUND)


def test_edge_cases(rt):
    LK.check_edge_cases(rt)


def test_refusals(hip_lib):
    LK.check_refusals(hip_lib)


def test_command_line_adds_exactly_the_new_lines(rt, tmp_path):
    LK.check_command_line(rt, tmp_path)


def test_detect_official_eval_diagnose_parts_end_to_end(rt, tmp_path):
    print('\n'.join(LK.check_detect_official_eval_diagnose_parts(rt, tmp_path)))
