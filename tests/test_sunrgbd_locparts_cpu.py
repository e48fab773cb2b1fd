"""The split of the localisation errors (t3d_sunrgbd_locparts, evaluate_sunrgbd.diagnose_class(parts=True), --diagnose_parts of
evaluate_sunrgbd and detect) without a GPU, through the NumPy specification of the entry point (tests/fake_sunrgbd_locparts.py): the
hand case worked out on paper, the generated cases and their conditions, the properties, the edge cases, the refusals (of the
specification and, without a launch, of libt3d.so), both command lines and the ABI mirror.  tests/sunrgbd_locparts_check.py holds the
cases; tests/test_sunrgbd_locparts_gpu.py runs the same ones on the device."""
import ctypes as C
import os
import subprocess

import pytest

import sunrgbd_locparts_check as LK
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_sunrgbd_locparts import FakeSunrgbdLocPartsLib
from test_sunrgbd_eval_cpu import _header_fields
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_case():
    LK.check_hand_case(LK.spec_rt())


def test_hand_case_logged_lines_json_and_curves(tmp_path):
    LK.check_hand_lines(LK.spec_rt(), tmp_path)


def test_generated_cases_satisfy_their_conditions():
    """Every part repairs at least 20 detections at the small size, two parts differ in the boxes they win, no part overlap within 1e-6
    of t_f and no pairing within 1e-9 of a tie; the large class runs ragged chunks."""
    print('small: repaired per part', list(LK.check_conditions('small')))
    print('large: repaired per part', list(LK.check_conditions('large')))


def test_generated_cases_reproduce():
    """The comparison the GPU file makes with libt3d.so, here of the specification with a second run of itself: exact."""
    assert LK.check_against_spec(LK.spec_rt(), 'small', 0.0) == (0.0, 0.0, 0.0)


def test_properties():
    LK.check_properties(LK.spec_rt(), LK.SPEC_BOUND)


def test_edge_cases():
    LK.check_edge_cases(LK.spec_rt())


def test_refusals_of_the_specification_library():
    LK.check_refusals(FakeSunrgbdLocPartsLib())


def test_refusals_of_the_library_come_before_any_launch():
    LK.check_refusals(abi.load())


def test_command_line_adds_exactly_the_new_lines(tmp_path):
    LK.check_command_line(LK.spec_rt(), tmp_path)


def test_parser_errors(tmp_path):
    LK.check_parser_errors(LK.spec_rt(), tmp_path)


def test_parts_need_a_diagnosis():
    det, gt_all = LK.hand_case()
    with pytest.raises(ValueError):
        LK.ES._eval_prepare(det, gt_all, None, LK.T_F, LK.spec_rt(), parts=True)


class SpecLib(DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdLocPartsLib):
    pass


def test_detect_official_eval_diagnose_parts_end_to_end(tmp_path):
    print('\n'.join(LK.check_detect_official_eval_diagnose_parts(Runtime(device='cpu', lib=SpecLib()), tmp_path)))


def test_ctypes_struct_follows_the_header(tmp_path):
    assert _header_fields('t3d_sunrgbd_locparts_args') == [f[0] for f in abi.SunrgbdLocPartsArgs._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void){printf("%zu %d %llu %d %d %d %d %d\\n", sizeof(t3d_sunrgbd_locparts_args), '
                   'T3D_V2_SIZE_sunrgbd_locparts_args, (unsigned long long)T3D_SUNRGBD_LOCPARTS_WORKSPACE_BYTES(1000, 300), '
                   'T3D_LOCPART_XY, T3D_LOCPART_Z, T3D_LOCPART_CENTRE, T3D_LOCPART_SIZE, T3D_LOCPART_HEADING);return 0;}\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 's')])
    size, v2, ws, *parts = [int(v) for v in subprocess.check_output([str(tmp_path / 's')], text=True).split()]
    assert size == v2 == C.sizeof(abi.SunrgbdLocPartsArgs) and abi.SunrgbdLocPartsArgs().struct_size == size
    assert ws == abi.sunrgbd_locparts_workspace_bytes(1000, 300)
    assert parts == [abi.LOC_PARTS.index(k) for k in ('xy', 'z', 'centre', 'size', 'heading')] == list(range(5))
    args = abi.ENTRY_POINTS['t3d_sunrgbd_locparts']
    assert args[0]._type_ is abi.SunrgbdEvalArgs and args[1]._type_ is abi.SunrgbdDiagnoseArgs and args[2]._type_ is abi.SunrgbdLocPartsArgs
