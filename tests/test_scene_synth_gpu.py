"""GPU: t3d_scene_raycast (csrc/scene_synth.hip) and transferable3d_amd/synth_scenes.py through libt3d.so: the cases and checkers of
tests/scene_check.py that tests/test_scene_synth_cpu.py runs through the NumPy specification (tests/fake_scene.py).  Every bound and
where it comes from is written down at the head of tests/scene_check.py; none is measured."""
import pytest

import scene_check as SK
from transferable3d_amd.engine import Runtime

pytestmark = pytest.mark.gpu


@pytest.fixture
def rt(hip_lib):
    return Runtime(lib=hip_lib)


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('name', sorted(SK.BATCHES))
def test_against_the_specification(rt, name, stride):
    """hit, image, scene_offsets, point_pixel, visible, vis_box and the noise-free rows, bit for bit."""
    SK.check_against_specification(rt, name, stride, 0.0)


@pytest.mark.parametrize('name,stride', [('three_a', 3), ('one_65', 1)])
def test_noisy_points(rt, name, stride):
    """The rows with noise within the bound t3d.h derives from the ulp errors of log, sqrt and cos."""
    SK.check_against_specification(rt, name, stride, 0.002)


def test_without_point_pixel(rt):
    SK.check_without_point_pixel(rt)


def test_zero_direction_components(rt):
    SK.check_zero_components(rt)


def test_coincident_parts_the_lower_index_wins(rt):
    SK.check_coincident_parts(rt)


def test_camera_inside_a_part_and_a_part_behind_the_camera(rt):
    SK.check_camera_inside_and_behind(rt)


def test_p_drop_one_emits_nothing(rt):
    SK.check_drop_everything(rt)


def test_max_range_below_every_hit(rt):
    SK.check_range_below_every_hit(rt)


def test_round_trip_through_the_extractors_projection(rt):
    SK.check_round_trip(rt)


def test_batch_independence_and_repeatability(rt):
    SK.check_batch_independence_and_repeatability(rt)


def test_refusals(hip_lib):
    SK.check_refusals(hip_lib)


def test_through_the_extractor(rt, tmp_path):
    SK.check_through_the_extractor(rt, tmp_path)


def test_command_line_flow(rt, tmp_path):
    SK.check_command_line(rt, tmp_path)


def test_frustum_dir_from_memory(rt, tmp_path):
    SK.check_frustum_dir(rt, tmp_path)


def test_detector_options(rt):
    SK.check_detector_options(rt)
