"""GPU: every stage behind t3d_detect_decode in one `Detector.decode_all` call through libt3d.so -- the order of the entry points, what
each stage was handed, the records and the log lines (tests/stages_check.py); the specification is met within the bounds of
ensemble_check and fuse_check."""
import pytest

import stages_check as SC
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


def test_every_stage_in_one_call_is_handed_what_the_stage_before_it_wrote(hip_lib, tmp_path):
    print('\n'.join(SC.check_flow(Runtime(lib=hip_lib), tmp_path, exact=False)))
