"""The detection-error diagnosis (t3d_sunrgbd_diagnose, evaluate_sunrgbd.diagnose_class, --diagnose of evaluate_sunrgbd and detect)
without a GPU, through the NumPy specification of the entry point (tests/fake_sunrgbd_diagnose.py): the hand case worked out on paper,
the generated cases and their conditions, the properties, the edge cases, the refusals (of the specification and, without a launch, of
libt3d.so), both command lines and the ABI mirror.  tests/sunrgbd_diagnose_check.py holds the cases; tests/test_sunrgbd_diagnose_gpu.py
runs the same ones on the device."""
import ctypes as C
import os
import subprocess

import sunrgbd_diagnose_check as DK
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_sunrgbd_diagnose import FakeSunrgbdDiagnoseLib
from test_sunrgbd_eval_cpu import _header_fields
from transferable3d_amd import abi
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_case():
    DK.check_hand_case(DK.spec_rt())


def test_hand_case_logged_lines_json_and_curves(tmp_path):
    DK.check_hand_lines(DK.spec_rt(), tmp_path)


def test_generated_cases_satisfy_their_conditions():
    """Every kind at least 100 times at the small size, every decision at least 1e-6 off its boundary; the large class runs ragged chunks."""
    print('small: detections per kind', list(DK.check_conditions('small')))
    print('large: detections per kind', list(DK.check_conditions('large')))


def test_generated_cases_reproduce():
    """The comparison the GPU file makes with libt3d.so, here of the specification with a second run of itself: exact."""
    assert DK.check_against_spec(DK.spec_rt(), 'small', 0.0) == (0.0, 0.0)


def test_properties():
    DK.check_properties(DK.spec_rt(), DK.SPEC_BOUND)


def test_edge_cases():
    DK.check_edge_cases(DK.spec_rt())


def test_refusals_of_the_specification_library():
    DK.check_refusals(FakeSunrgbdDiagnoseLib())


def test_refusals_of_the_library_come_before_any_launch():
    DK.check_refusals(abi.load())


def test_command_line_adds_exactly_the_new_lines(tmp_path):
    DK.check_command_line(DK.spec_rt(), tmp_path)


def test_parser_errors(tmp_path):
    DK.check_parser_errors(DK.spec_rt(), tmp_path)


class SpecLib(DetectDecodeSpec, FakeFrustumLib, FakeSunrgbdDiagnoseLib):
    pass


def test_detect_official_eval_diagnose_end_to_end(tmp_path):
    print('\n'.join(DK.check_detect_official_eval_diagnose(Runtime(device='cpu', lib=SpecLib()), tmp_path)))


def test_ctypes_struct_follows_the_header(tmp_path):
    assert _header_fields('t3d_sunrgbd_diagnose_args') == [f[0] for f in abi.SunrgbdDiagnoseArgs._fields_]
    src = tmp_path / 's.c'
    src.write_text('#include <stdio.h>\n#include "t3d.h"\nint main(void){printf("%zu %d %llu %d %d %d %d\\n", sizeof(t3d_sunrgbd_diagnose_args), '
                   'T3D_V2_SIZE_sunrgbd_diagnose_args, (unsigned long long)T3D_SUNRGBD_DIAGNOSE_WORKSPACE_BYTES(1000, 300, 2500), '
                   'T3D_DIAG_TP, T3D_DIAG_BKG, T3D_DIAG_FIX_CLS, T3D_DIAG_FIX_FN);return 0;}\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 's')])
    size, v2, ws, tp, bkg, fix_cls, fix_fn = [int(v) for v in subprocess.check_output([str(tmp_path / 's')], text=True).split()]
    assert size == v2 == C.sizeof(abi.SunrgbdDiagnoseArgs) and abi.SunrgbdDiagnoseArgs().struct_size == size
    assert ws == abi.sunrgbd_diagnose_workspace_bytes(1000, 300, 2500)
    assert (tp, bkg) == (abi.DIAG_KINDS.index('tp'), abi.DIAG_KINDS.index('bkg')) and (fix_cls, fix_fn) == (abi.DIAG_FIXES.index('cls'), abi.DIAG_FIXES.index('fn'))
    args = abi.ENTRY_POINTS['t3d_sunrgbd_diagnose']
    assert args[0]._type_ is abi.SunrgbdEvalArgs and args[1]._type_ is abi.SunrgbdDiagnoseArgs and abi.ABI_VERSION == 3
