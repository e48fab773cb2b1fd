"""GPU: t3d_frustum_extract at kernel level (tests/frustum_kernel_check.py).  Every case of tests/test_kernels_frustum_cpu.py through
libt3d.so on guarded device tensors, against the NumPy specification on the host: integer outputs, box2d_out and out_points bit for
bit over the whole [J, num_points] arrays, frustum_angle within 1e-12, inputs unchanged, no store outside the scratch and the outputs,
every output element written, two runs equal; the ragged batch also one launch per scene."""
import pytest

import frustum_kernel_check as KC
import test_kernels_frustum_cpu as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('detection', [False, True])
def test_ragged_batch(hip_lib, detection):
    c = KC.ragged_case(detection)
    out = KC.check_on_device(c, hip_lib, DEV)
    T.check_ragged(c, out)
    KC.check_split(c, out, hip_lib, DEV)


@pytest.mark.parametrize('NP', KC.CUT_NP)
def test_the_cut_at_num_points(hip_lib, NP):
    c = KC.cut_case(NP)
    T.check_cut(c, KC.check_on_device(c, hip_lib, DEV))


def test_the_cut_at_the_largest_num_points(hip_lib):
    c = KC.cut_big_case()
    T.check_cut(c, KC.check_on_device(c, hip_lib, DEV))


@pytest.mark.parametrize('i', range(len(KC.TIES)))
def test_threshold_tie_keeps_the_lower_rank(hip_lib, i):
    T.check_tie(i, KC.check_on_device(KC.tie_case(i), hip_lib, DEV))


def test_exact_boundaries_against_the_hand_table(hip_lib):
    T.check_boundary_table(KC.check_on_device(KC.boundary_case(), hip_lib, DEV))


def test_injected_choice_edge_cases(hip_lib):
    c = KC.choice_case()
    T.check_choice(c, KC.check_on_device(c, hip_lib, DEV))


@pytest.mark.parametrize('C_src,C_out', KC.CHANNELS)
def test_fewer_channels_than_the_source(hip_lib, C_src, C_out):
    KC.check_on_device(KC.channels_case(C_src, C_out), hip_lib, DEV)


@pytest.mark.parametrize('given', [True, False])
def test_perturbed_boxes_across_a_job_tile(hip_lib, given):
    KC.check_on_device(KC.perturb_case(given), hip_lib, DEV)


def test_refusals(hip_lib):
    KC.check_refusals(hip_lib, DEV)
