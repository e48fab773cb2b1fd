"""t3d_frustum_extract at kernel level without a GPU (tests/frustum_kernel_check.py): the cases of tests/test_kernels_frustum_gpu.py
through the NumPy specification (tests/fake_frustum.py) on guarded host arrays, the specification against the independent restatement
of the reference (tests/ref_frustum.py, Delaunay labels, injected draws), the hand-written table of the exact boundaries, and the
assertion that the three hash ties still straddle their cut."""
from fractions import Fraction

import numpy as np
import pytest

import frustum_kernel_check as KC
from fake_frustum import FakeFrustumLib, job_base, rank_keys


def spec(c):
    out = KC.run(c, FakeFrustumLib())
    KC.check_against_restatement(c, out)
    return out


def check_ragged(c, out):
    """the case reaches what it is for: both sides of both job-tile boundaries hold boxes with different contents, some of them
    subsampled; the point-less scene's jobs are empty"""
    sj = np.concatenate([[0], np.cumsum(KC.RAGGED_JOBS)])
    n = out['n_in_box']
    assert (out['count'] == np.minimum(n, c.NP)).all()
    big = n[sj[7]:sj[8]]                                                    # 1000 points, 300 jobs: three tiles
    for lo, hi in ((0, 128), (128, 256), (256, 300)):
        assert len(set(big[lo:hi].tolist())) > 8 and (big[lo:hi] > c.NP).any() and (big[lo:hi] == 0).any()
    assert big[127] != big[128] and big[255] != big[256]
    assert not n[sj[1]:sj[2]].any() and (out['index'][sj[1]:sj[2]] == -1).all()
    for s in (3, 5, 6):                                                     # 64, 255 and 256 points: every point in some box
        assert n[sj[s]:sj[s + 1]].max() == KC.RAGGED_POINTS[s]


@pytest.mark.parametrize('detection', [False, True])
def test_ragged_batch(detection):
    c = KC.ragged_case(detection)
    out = spec(c)
    check_ragged(c, out)
    KC.check_split(c, out, FakeFrustumLib())


def check_cut(c, out):
    assert out['n_in_box'].tolist() == [j['n'] for j in c.jobs]
    for i, j in enumerate(c.jobs):
        k = min(j['n'], c.NP)
        idx = out['index'][i]
        assert (idx[:k] >= 0).all() and len(np.unique(idx[:k])) == k and (np.diff(idx[:k]) > 0).all() and (idx[k:] == -1).all()


@pytest.mark.parametrize('NP', KC.CUT_NP)
def test_the_cut_at_num_points(NP):
    c = KC.cut_case(NP)
    check_cut(c, spec(c))


def test_the_cut_at_the_largest_num_points():
    c = KC.cut_big_case()
    check_cut(c, spec(c))


@pytest.mark.parametrize('i', range(len(KC.TIES)))
def test_the_hash_ties_straddle_the_cut(i):
    """If the hash ever changes this fails: search the seeds again on the host and replace KC.TIES."""
    seed, n, NP, kept, dropped = KC.TIES[i]
    keys = rank_keys(job_base(seed, KC.TIE_KEY), n)
    order = np.lexsort((np.arange(n), keys))
    assert keys[order[NP - 1]] == keys[order[NP]] and (order[NP - 1], order[NP]) == (kept, dropped) and kept < dropped
    assert NP < 2 or keys[order[NP - 2]] < keys[order[NP - 1]]             # exactly one of the tied ranks is inside


def check_tie(i, out):
    seed, n, NP, kept, dropped = KC.TIES[i]
    idx = out['index'][0]
    assert out['n_in_box'][0] == n and out['count'][0] == NP                # every point is in the box: rank = index
    assert kept in idx and dropped not in idx and len(np.unique(idx)) == NP and (np.diff(idx) > 0).all()


@pytest.mark.parametrize('i', range(len(KC.TIES)))
def test_threshold_tie_keeps_the_lower_rank(i):
    check_tie(i, spec(KC.tie_case(i)))


# The hand-written table of KC.boundary_case(): per 2-D box the points inside it, in the cloud's order.  Points 0 .. 4 project to
# (384, 256), (128, 256), (256, 128), (256, 384), (256, 256); 5 .. 7 are the NaN and the two zero-depth points (in no box); point 8 lies
# behind the camera and is left to the specification; 9 .. 22 are the points of the 3-D box (all left of the image).
BEHIND = 8
MEMBERS = [[1, 2, 4],                       # [128, 384) x [128, 384): u = 128 and v = 128 are in, u = 384 and v = 384 are out
           [0, 1, 2, 3, 4],                 # right and lower edge one ulp further
           [4],                             # left and upper edge one ulp further
           [4],                             # [256, 257)^2
           [],                              # [255, 256)^2
           [0, 1, 2, 3, 4] + list(range(9, 23))]
# labels of points 9 .. 22: centre; then on the face / one ulp outside it for x = -2, x = -4, y = 2, y = 4, z = 4, z = 3; far outside
LABELS_3D = [1, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0]


def check_boundary_table(out):
    for j, want in enumerate(MEMBERS):
        k = int(out['count'][j])
        keep = out['index'][j, :k] != BEHIND
        assert out['index'][j, :k][keep].tolist() == want, (j, out['index'][j, :k])
        assert out['n_in_box'][j] == k and k - len(want) in (0, 1)
        lab = out['label'][j, :k][keep].tolist()
        assert lab == [0] * len(want) if j < 5 else lab == [0] * 5 + LABELS_3D, (j, lab)


def test_boundary_case_is_exact_arithmetic():
    """the table speaks of real numbers; here: the fp64 operations of the projection and of the face test are exact on these inputs"""
    want_uv = [(384, 256), (128, 256), (256, 128), (256, 384), (256, 256)]
    for (x, y, z), (u, v) in zip(KC.BOUNDARY_UV, want_uv):
        assert (x * 512.0 + y * 256.0) / y == u and (-z * 512.0 + y * 256.0) / y == v
        assert Fraction(x) * 512 / Fraction(y) + 256 == u and -Fraction(z) * 512 / Fraction(y) + 256 == v
    corner1, edges = (-2.0, 2.0, 4.0), ((0, 0, -1.0), (0, 2.0, 0), (-2.0, 0, 0))       # to corners 2, 5 and 0
    for p, lab in zip(KC.BOUNDARY_CAM, LABELS_3D):
        inside = True
        for e in edges:
            q = [Fraction(float(a)) - Fraction(b) for a, b in zip(p, corner1)]
            assert all(Fraction(float(a) - b) == f for a, b, f in zip(p, corner1, q))          # the subtraction is exact
            dv, dd = sum(a * Fraction(b) for a, b in zip(q, e)), sum(Fraction(b) ** 2 for b in e)
            assert Fraction(float(dv)) == dv
            inside &= 0 <= dv <= dd
        assert inside == bool(lab), p


def test_exact_boundaries_against_the_hand_table():
    check_boundary_table(spec(KC.boundary_case()))


def check_choice(c, out):
    n = out['n_in_box']
    assert n[0] == n[1] == n[3] == n[4] == 300 and 0 < n[2] <= c.NP
    assert (out['count'] == [c.NP, c.NP, n[2], c.NP, c.NP]).all()
    bad = out['index'][3]
    assert bad[5] == -1 and bad[9] == -1 and (np.delete(bad, [5, 9]) >= 0).all()
    assert not out['out_points'][3, [5, 9]].any() and not out['label'][3, [5, 9]].any()
    assert np.array_equal(out['index'][0], c.jobs[0]['choice']) and (np.diff(out['index'][1]) > 0).all()      # every point is in the box
    assert np.array_equal(out['index'][2, :n[2]], np.sort(out['index'][2, :n[2]])) and out['index'][4, 0] == 299


def test_injected_choice_edge_cases():
    c = KC.choice_case()
    check_choice(c, spec(c))


@pytest.mark.parametrize('C_src,C_out', KC.CHANNELS)
def test_fewer_channels_than_the_source(C_src, C_out):
    c = KC.channels_case(C_src, C_out)
    out = spec(c)
    assert out['out_points'].shape[2] == C_out and (out['n_in_box'] > 0).sum() >= 4


@pytest.mark.parametrize('given', [True, False])
def test_perturbed_boxes_across_a_job_tile(given):
    c = KC.perturb_case(given)
    out = spec(c)
    box = np.array([j['box2d'] for j in c.jobs])
    assert (out['box2d_out'] != box).any(1).all() and len(np.unique(out['box2d_out'], axis=0)) == len(c.jobs)


def test_refusals_of_the_specification():
    KC.check_refusals(FakeFrustumLib())


def test_refusals_of_the_library_without_a_launch():
    """the real launcher refuses (and answers a call without jobs) before it touches the device: host arrays serve"""
    from transferable3d_amd import abi
    KC.check_refusals(abi.load(), then_launch=False)
