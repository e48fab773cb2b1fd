"""CPU: t3d_scene_raycast and transferable3d_amd/synth_scenes.py through the NumPy specification (tests/fake_scene.py) -- the cases and
checkers of tests/scene_check.py that tests/test_scene_synth_gpu.py runs through libt3d.so -- and what needs no device: the header
against the bindings, the layout's properties, the argument checks of the library (they come before any launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fake_scene as FS
import scene_check as SK
from transferable3d_amd import abi
from transferable3d_amd import synth_scenes as SS
from transferable3d_amd.engine import Runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rt():
    return Runtime(device='cpu', lib=FS.FakeSceneLib())


def test_header_constants_and_struct_fields_match_the_bindings():
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    const = lambda name: re.search(r'#define %s \(?(-?[\d.]+)\)?\s' % name, h).group(1)
    assert int(const('T3D_SCENE_MAX_PARTS')) == abi.SCENE_MAX_PARTS and int(const('T3D_SCENE_MAX_OBJECTS')) == abi.SCENE_MAX_OBJECTS
    assert int(const('T3D_SCENE_BLOCK_PIXELS')) == abi.SCENE_BLOCK_PIXELS and float(const('T3D_SCENE_ROOM_COLOUR')) == abi.SCENE_ROOM_COLOUR
    assert int(const('T3D_SCENE_HIT_ROOM')) == abi.SCENE_HIT_ROOM and int(const('T3D_SCENE_HIT_INVALID')) == abi.SCENE_HIT_INVALID
    shades = re.search(r'#define T3D_SCENE_SHADES \{([^}]*)\}', h).group(1)
    assert tuple(float(v) for v in shades.split(',')) == abi.SCENE_SHADES
    assert int(const('T3D_V2_SIZE_scene_raycast_args')) == C.sizeof(abi.SceneRaycastArgs)
    for cname, cls in (('scene_raycast_args', abi.SceneRaycastArgs), ('scene_part', abi.ScenePart)):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*t3d_%s;' % cname, h).group(1), flags=re.S)
        names = [re.findall(r'(\w+)(?:\[\d+\])?\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
        assert names == [f[0] for f in cls._fields_], cname
    assert SS.PART_DTYPE.itemsize == C.sizeof(abi.ScenePart) == 96 and SS.PART_DTYPE.names == tuple(f[0] for f in abi.ScenePart._fields_)
    for f in abi.ScenePart._fields_:
        assert SS.PART_DTYPE.fields[f[0]][1] == getattr(abi.ScenePart, f[0]).offset
    assert abi.scene_blocks(SK.H, SK.W) == 3 and abi.scene_workspace_bytes(3, SK.H, SK.W) == 3 * 3 * 16
    assert abi.scene_blocks(32, 32) == 1 and abi.scene_blocks(32, 33) == 2
    for name in ('0x9E3779B97F4A7C15', '0xC2B2AE3D27D4EB4F', '0x94D049BB133111EB', '0xBF58476D1CE4E5B9'):      # the hash's own key constants
        assert name in h


def test_the_library_and_the_specification_refuse_alike():
    """The argument checks come before any launch: the built library answers them without a device."""
    SK.check_refusals(FS.FakeSceneLib())
    SK.check_refusals(abi.load())


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('name', sorted(SK.BATCHES))
def test_against_the_specification(rt, name, stride):
    SK.check_against_specification(rt, name, stride, 0.0)


def test_noisy_points(rt):
    SK.check_against_specification(rt, 'three_a', 3, 0.002)


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


def test_the_specifications_hash_is_the_frustum_finaliser_on_its_own_keys():
    u = FS.uniforms(5, 7, np.arange(4096), 0)
    assert 0.0 < u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.03
    assert not np.array_equal(u, FS.uniforms(5, 8, np.arange(4096), 0)) and not np.array_equal(u, FS.uniforms(6, 7, np.arange(4096), 0))
    assert not np.array_equal(u, FS.uniforms(5, 7, np.arange(4096), 1))
    g = FS.normal(FS.uniforms(5, 7, np.arange(1 << 16), 1), FS.uniforms(5, 7, np.arange(1 << 16), 2))
    assert abs(g.mean()) < 0.02 and abs(g.std() - 1.0) < 0.02


def test_layout_properties():
    SK.check_layout_properties()


def test_through_the_extractor(tmp_path):
    import fake_frustum

    class Both(FS.FakeSceneLib, fake_frustum.FakeFrustumLib):
        pass
    SK.check_through_the_extractor(Runtime(device='cpu', lib=Both()), tmp_path)


def test_command_line_flow(tmp_path):
    import fake_sunrgbd_eval

    class Both(FS.FakeSceneLib, fake_sunrgbd_eval.FakeSunrgbdEvalLib):
        pass
    SK.check_command_line(Runtime(device='cpu', lib=Both()), tmp_path)


def test_frustum_dir_from_memory(tmp_path):
    import fake_frustum

    class Both(FS.FakeSceneLib, fake_frustum.FakeFrustumLib):
        pass
    SK.check_frustum_dir(Runtime(device='cpu', lib=Both()), tmp_path)


def test_detector_options(rt):
    SK.check_detector_options(rt)
