"""CPU: every stage behind t3d_detect_decode in one `Detector.decode_all` call on the NumPy specification libraries -- the order of the
entry points, what each stage was handed, the records, the log lines and the number of copies back (tests/stages_check.py)."""
import fake_consistency as FK
import fake_ensemble as FE
import fake_fuse as FF
import fake_nms as FN
import stages_check as SC
from fake_detect import DetectDecodeSpec
from fake_frustum import FakeFrustumLib
from fake_render import RenderSpec
from transferable3d_amd.engine import Runtime


class SpecLib(FE.DetectEnsembleSpec, FK.ConsistencySpec, RenderSpec, FF.DetectFuseSpec, FN.DetectNmsSpec, DetectDecodeSpec, FakeFrustumLib):
    pass


def test_every_stage_in_one_call_is_handed_what_the_stage_before_it_wrote(tmp_path):
    print('\n'.join(SC.check_flow(Runtime(device='cpu', lib=SpecLib()), tmp_path, exact=True)))
