"""GPU: transferable3d_amd/detect.py through libt3d.so on the golden scenes (B = 4, N = 256 -- the smallest the Box-PC
kernel of --refine 1 takes --, refine 1, the graph's initial weights): its
<class>_pred.txt files equal, as text, those of sunrgbd_data -> pickle -> semisup_infer --from_rgb_detection --device_decode; against
the same route with the host decode the classes and the structure are equal and every printed number agrees within the kernel's bound
plus the 1e-6 of two %f roundings (five digits behind the point); the detection of fewer than 5 points is in neither; Detector.detect
returns the records the command line wrote."""
import pytest

import detect_check as DC
from test_detect_decode_gpu import BOUND
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


def test_detect_equals_the_two_step_route(hip_lib, tmp_path):
    print('\n'.join(DC.check_scene_flow(Runtime(lib=hip_lib), tmp_path, BOUND)))
