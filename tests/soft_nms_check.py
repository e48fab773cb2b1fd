"""Shared cases of the t3d_detect_soft_nms tests: the CPU tests run them through the NumPy specification library (fake_soft_nms), the GPU
tests through libt3d.so, and both compare with fake_soft_nms.soft_nms.

The cases are deep copies of nms_check's (the cached originals are never touched), one set per pass (metric, method, threshold, sigma,
floor) of PASSES.

How close is close enough.  The kernel takes its IoUs in fp32, the specification in fp64, and the project holds the device IoU to EPS =
2e-5 of the specification's (nms_check, tests/test_dataset_gpu.py).  A decay multiplies the working score s by a factor f(IoU); with the IoU
off by e, |e| <= EPS, the factor is off by df:
    gaussian   f = exp(-IoU^2 / sigma):  exp(-(IoU + e)^2 / sigma) = f exp(-(2 IoU e + e^2) / sigma), so df / f <= (2 IoU EPS + EPS^2) / sigma
               to first order (the exponent is about 1e-4: the second order is 1e-8 of f);
    linear     f = 1 - IoU:              df <= EPS, i.e. df / f <= EPS / (1 - IoU);
and a score that carried the absolute error E before the decay carries E f + s df behind it, plus the fp32 arithmetic of the decay: the
rounding of IoU^2, of the division by sigma (an error of 2 * 2^-24 * IoU^2 / sigma <= 5e-7 in the exponent for sigma >= 0.25), expf's own
2 ulps and the product's half ulp -- under 8 ulps = 8 * 2^-23 of the new score, which is what fake_soft_nms.ULPS allows (for linear, 1 -
IoU is exact above IoU 0.5 and within half an ulp below, so the same allowance holds).  In relative terms E' / s' = E / s + df / f + ULPS:
the relative bounds of the decays of a box add up.  The bound is carried in absolute form so that it stays finite where 1 - IoU is 0.
`score_out` must lie within TWICE that bound (the factor two pays for the first-order step and for the bound being evaluated at the
specification's scores); a box nothing decayed has bound 0 and must hold its input bits.  keep, suppressed_by and n_decays are compared
exactly, so a case is usable only where no decision can flip inside the bound (fake_soft_nms.soft_nms reports the offenders):
    at every selection, no live box that the selected box decays has a working score within twice the two boxes' bounds of the selected
    one's (near ties between boxes that do not decay each other only swap two commuting steps);
    no decayed score lies within twice its bound of the floor;
    linear: no IoU within nms_check.MARGIN of the threshold (nms_check's repair, which the copies inherit);
A box that breaks one of these gets its score redrawn from the case's own generator; at most nms_check.MAX_REDRAWN of a case's boxes may
be redrawn (the hand-built cases must be usable as they are).
Gaussian has a threshold too, 0, and it cannot be repaired that way: the IoUs of jittered copies pile up at 0 -- slivers between
neighbours, 18 boxes of the 130-box group meet one below EPS -- and an IoU the specification finds in (0, EPS) may be 0 on the device,
as one it finds 0 between boxes that all but touch may be positive there; either changes n_decays.  Redrawing those boxes afterwards
makes new slivers as fast as it removes them.  So the gaussian passes do not take nms_check's boxes as they are: `settle` walks every
group in list order and draws a box again, from the case's own generator and the object it copies, until it forms no such pair with
the boxes before it -- no IoU in (0, EPS), and no IoU of 0 that turns positive when the box is blown up by 1e-3 about its centre (a gap
under a millimetre; real gaps are centimetres).  That is the generator with a rejection step, not a repair: `settled` counts the boxes
it drew again and the CPU test prints it; nothing bounds it.  The specification still reports a sliver decay as unsafe, so a case that
kept one would not build.  With that n_decays is compared exactly, like keep and suppressed_by.
A random case of more than one box must decay, keep and -- at the 0.05 floor -- prune something.  Two boxes prune only if the lower
score lies below 0.05 / factor, and size_2, whose drawn scores do under gaussian, sigma 0.25, does not under linear above 0.5; the 5 %
budget allows no redraw of a two-box case.  A case that prunes nothing at a pass's 0.05 floor therefore runs under a floor of its own,
twice the smallest score the specification decays it to at the pass's floor (`floor_raised`; only size_2 under the last pass).
"""
import copy
import functools

import numpy as np
import torch

import fake_nms as FN
import fake_soft_nms as FS
import nms_check as NC
from transferable3d_amd import nms as NMS

EPS = 2e-5
# (metric, method, threshold, sigma, floor)
PASSES = (('3d', 'gaussian', None, 0.5, 0.001), ('bev', 'gaussian', None, 0.25, 0.05), ('3d', 'linear', 0.25, None, 0.001),
          ('bev', 'linear', 0.5, None, 0.05))
BIG_PASSES = (0, 3)                        # the passes group_1024 runs under
FILL = (-3.5, 7, -7, -9)                   # (score_out, keep, suppressed_by, n_decays) before a launch: an unlisted box must still hold it
HAND = ('chain', 'ties_nan', 'identical', 'zero_volume')


def blown_up(k, by=1e-3):
    c = k.mean(0)
    return c + (k - c) * (1.0 + by)


def on_the_edge(ka, kb, metric):
    """Whether the decision IoU > 0 of the two boxes, either way round, could flip inside the IoU error: 0 < IoU < EPS, or 0 with the
    boxes all but touching (the gap is the same whichever box is blown up)."""
    v, w = NC.memo_iou(ka, kb)[metric], NC.memo_iou(kb, ka)[metric]
    if v != v or w != w or (v >= EPS and w >= EPS):
        return False
    return v > 0.0 or w > 0.0 or FN.iou_corners(ka, blown_up(kb))[metric] > 0.0


class SoftCase:
    """A copy of an nms_check.Case under one pass."""

    def __init__(self, case, pass_id):
        self.c, self.pass_id = copy.deepcopy(case), pass_id
        self.metric, self.method, self.threshold, self.sigma, self.floor = PASSES[pass_id]
        self.name, self.hand_built, self.groups = case.name, case.hand_built, self.c.groups
        self.redrawn, self.settled, self.floor_raised, self.cache, self.want = 0, 0, False, {}, None

    @property
    def n(self):
        return self.c.n

    def arrays(self):
        return self.c.arrays()

    def spec(self, fill=FILL):
        corners, score, offsets, members = self.arrays()
        return FS.soft_nms(corners, score, offsets, members, self.method, self.threshold, self.sigma or 0.5, self.floor, NC.METRIC_ID[self.metric],
                           fill=fill, cache=self.cache, iou=NC.memo_iou, eps=EPS)

    @property
    def want_at_pass_floor(self):
        """`want` under the pass's own floor: what a call that holds several cases (`moved`) runs every one of them under."""
        if not self.floor_raised:
            return self.want
        corners, score, offsets, members = self.arrays()
        r = FS.soft_nms(corners, score, offsets, members, self.method, self.threshold, self.sigma or 0.5, PASSES[self.pass_id][4],
                        NC.METRIC_ID[self.metric], fill=FILL, cache=self.cache, iou=NC.memo_iou, eps=EPS)
        assert not r.unsafe and not r.slivers, self.name
        return r

    def edge_pairs(self, group, upto=None, k=None):
        """The pairs (earlier, later) of a group, both ways round, whose gaussian decision lies on the edge (on_the_edge); upto: only
        the pairs of the box at that list position with the boxes before it."""
        c, m = self.c, NC.METRIC_ID[self.metric]
        k = k or {b: NC.corners_of(c.boxes[b]).astype(np.float64) for b in group}
        centre, half = {b: k[b].mean(0) for b in group}, {b: 0.5 * np.linalg.norm(k[b][0] - k[b][6]) for b in group}
        out = []
        for t in (range(1, len(group)) if upto is None else [upto]):
            kt = k[group[t]]
            before = np.asarray(group[:t])
            far = np.linalg.norm(np.stack([centre[b] for b in before]) - centre[group[t]], axis=1) > (np.asarray([half[b] for b in before]) + half[group[t]]) * 1.01 + 1e-6
            for b in before[~far]:                # (the others cannot touch, blown up or not)
                kb = k[b]
                if on_the_edge(kb, kt, m):
                    out.append((b, group[t]))
        return out

    def settle(self):
        """Gaussian passes: the module docstring's rejection step."""
        c = self.c
        for g in self.groups:
            k = {b: NC.corners_of(c.boxes[b]).astype(np.float64) for b in g}
            for t in range(1, len(g)):
                drawn = False
                while self.edge_pairs(g[:t + 1], upto=t, k=k):
                    j = g[t]
                    c.boxes[j] = NC.draw_copy(c.r, c.parent[j]) if c.parent[j] is not None else NC.draw_object(c.r)
                    k[j] = NC.corners_of(c.boxes[j]).astype(np.float64)
                    drawn = True
                self.settled += drawn

    def repair(self):
        """The usability conditions of the module docstring; asserts the redraw budget."""
        c = self.c
        if self.method == 'gaussian' and not self.hand_built:
            self.settle()
        listed = [b for g in self.groups for b in g]
        while True:
            r = self.spec()
            if r.unsafe or r.slivers:
                assert not self.hand_built and not r.slivers, (self.name, PASSES[self.pass_id], sorted(r.unsafe), sorted(r.slivers))
                for j in r.unsafe:
                    c.scores[j] = c.r.uniform(0, 1)
                self.redrawn += len(r.unsafe)
            elif not self.hand_built and len(listed) > 1 and self.floor >= 0.05 and not self.floor_raised and r.keep[listed].min() != 0:
                self.floor, self.floor_raised = float(np.float32(2.0 * r.score_out[listed][r.n_decays[listed] > 0].min())), True
            else:
                break
        assert self.redrawn <= NC.MAX_REDRAWN * self.n, '%s %s: %d of %d boxes redrawn' % (self.name, PASSES[self.pass_id], self.redrawn, self.n)
        self.want = r
        for a in (r.score_out, r.keep, r.suppressed_by, r.n_decays, r.bound):
            a.setflags(write=False)
        if not self.hand_built and len(listed) > 1:       # a case that decays nothing, keeps nothing or (at the 0.05 floor) prunes nothing checks little
            assert r.n_decays[listed].max() > 0 and r.keep[listed].max() == 1, (self.name, PASSES[self.pass_id])
            assert self.floor < 0.05 or r.keep[listed].min() == 0, (self.name, PASSES[self.pass_id])
        return self


def base_cases(pass_id):
    metric, _, threshold, _, _ = PASSES[pass_id]
    return metric, (threshold if threshold is not None else 0.5)      # gaussian has no threshold: any repaired set serves


@functools.lru_cache(maxsize=None)
def cases(pass_id):
    """name -> SoftCase, repaired and with `.want` (fake_soft_nms.Result, read-only); built once per process."""
    return {name: SoftCase(c, pass_id).repair() for name, c in NC.cases(*base_cases(pass_id)).items()}


@functools.lru_cache(maxsize=None)
def big_case(pass_id):
    return SoftCase(NC.big_case(*base_cases(pass_id)), pass_id).repair()


def run_with(rt, corners, score, offsets, members, method, threshold, sigma, floor, metric, fill=FILL, dev=None):
    """nms.DeviceSoftNms on NumPy arrays, outputs pre-filled with `fill` -> (score_out, keep, suppressed_by, n_decays) as NumPy arrays."""
    dev = dev or NMS.DeviceSoftNms(rt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)
    k = up(corners.reshape(-1, 24)) if len(corners) else rt.zeros(0, 24)
    s = up(score) if len(score) else rt.zeros(0)
    out = dev.run(k, s, offsets, members, method, threshold, sigma or 0.5, floor, metric, fill=fill)
    return tuple(t.cpu().numpy().copy() for t in out)


def run(rt, corners, score, offsets, members, pass_id, fill=FILL, floor=None, dev=None):
    """`run_with` under the options of a pass (floor: another floor than the pass's)."""
    metric, method, threshold, sigma, fl = PASSES[pass_id]
    return run_with(rt, corners, score, offsets, members, method, threshold, sigma, fl if floor is None else floor, metric, fill, dev)


def run_case(rt, c):
    return run(rt, *c.arrays(), c.pass_id, floor=c.floor)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_case(got, c, what=None, want=None):
    """got: (score_out, keep, suppressed_by, n_decays) of an implementation on case c, unlisted boxes at FILL."""
    want, what = want or c.want, what or c.name
    for k, g, w in zip(('keep', 'suppressed_by', 'n_decays'), got[1:], (want.keep, want.suppressed_by, want.n_decays)):
        assert np.array_equal(g, w), (what, k, np.nonzero(g != w)[0][:8], g[g != w][:8], w[g != w][:8])
    s = got[0].astype(np.float64)
    exact = want.bound == 0                      # never decayed (or unlisted): the input bits (the fill)
    assert np.array_equal(bits(got[0])[exact], bits(want.score_out)[exact]), (what, 'score_out bits of undecayed boxes')
    err, tol = np.abs(s[~exact] - want.score_out[~exact]), 2.0 * want.bound[~exact]
    print('%s: %d decayed boxes, largest |score_out - spec| / bound %.3g, largest relative bound %.3g' % (
        what, int((~exact).sum()), float((err / want.bound[~exact]).max()) if err.size else 0.0,
        float((want.bound[~exact] / np.maximum(np.abs(want.score_out[~exact]), 1e-300)).max()) if err.size else 0.0))
    assert (err <= tol).all(), (what, 'score_out', np.nonzero(~exact)[0][err > tol][:8], err[err > tol][:8], tol[err > tol][:8])


def hard_equal(got, hard, score, listed, what):
    """Consequence (a): with linear at T and a floor above every score, keep and suppressed_by are t3d_detect_nms's at T, byte for byte,
    for every listed box that takes part -- a box whose score is not a finite number above 0 ranks behind all of those in
    t3d_detect_nms, so it changes nothing for them, and Soft-NMS returns it kept by rule."""
    part = np.zeros(len(score), bool)
    part[listed] = True
    part &= np.isfinite(score) & (score > 0)
    assert np.array_equal(got[1][part], hard[0][part]) and np.array_equal(got[2][part], hard[1][part]), what
    rest = np.zeros(len(score), bool)
    rest[listed] = True
    rest &= ~part
    assert (got[1][rest] == 1).all() and (got[2][rest] == -1).all(), what


def moved(rt, names, pass_id, seed=0):
    """nms_check.moved for Soft-NMS: the groups of the cases `names` in one larger call, at permuted box indices, in reversed group order
    and with unlisted boxes in between, all under the pass's floor -> per case, the outputs mapped back to the case's own indices
    (compare with `want_at_pass_floor`)."""
    cs = [cases(pass_id)[k] for k in names]
    r = np.random.RandomState(seed)
    total = sum(c.n for c in cs) + 9
    perm = r.permutation(total)
    corners, score = np.zeros((total, 8, 3), np.float32), np.zeros(total, np.float32)
    groups, where, at = [], [], 0
    for c in cs:
        k, s, _, _ = c.arrays()
        new = np.sort(perm[at:at + c.n])          # ascending, so that equal scores tie as before
        at += c.n
        if c.n:
            corners[new], score[new] = k, s
        where.append(new)
        groups = [sorted(int(new[b]) for b in g) for g in c.groups] + groups
    for j in perm[at:]:
        corners[j] = NC.corners_of(NC.draw_object(r))
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    members = np.asarray([b for g in groups for b in g], np.int32)
    out, keep, sup, dec = run(rt, corners, score, offsets, members, pass_id)
    assert all(out[j] == FILL[0] and keep[j] == FILL[1] and sup[j] == FILL[2] and dec[j] == FILL[3] for j in perm[at:])
    back = np.full(total, -1, np.int64)
    res = []
    for c, new in zip(cs, where):
        back[:] = -1
        back[new] = np.arange(c.n)
        s = sup[new]
        listed = np.zeros(c.n, bool)
        listed[[b for g in c.groups for b in g]] = True
        res.append((out[new], keep[new], np.where(listed & (s >= 0), back[np.clip(s, 0, total - 1)], s).astype(np.int32), dec[new]))
    return res


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
def records_soft(ids, records, method, threshold=None, sigma=0.5, floor=0.001, metric='3d'):
    """fake_soft_nms.soft_nms over the records of a plain Detector.detect -> (the records that are not pruned, each a copy with 'soft_prob'
    and 'decays'; the Result)."""
    from transferable3d_amd.constants import type2class
    flat = [(s, r) for s, recs in zip(ids, records) for r in recs]
    corners = np.stack([r['corners'] for _, r in flat]).astype(np.float32)
    prob = np.asarray([r['prob'] for _, r in flat], np.float32)
    offsets, members = NMS.groups_of([s for s, _ in flat], [type2class[r['class']] for _, r in flat])
    res = FS.soft_nms(corners, prob, offsets, members, method, threshold, sigma, floor, NC.METRIC_ID[metric])
    kept, i = [], 0
    for recs in records:
        kept.append([dict(r, soft_prob=float(np.float32(res.score_out[i + k])), decays=int(res.n_decays[i + k]))
                     for k, r in enumerate(recs) if res.keep[i + k]])
        i += len(recs)
    return kept, res


FLOW_CONFIGS = (('gaussian', None, 0.5, 0.2, '3d'), ('linear', NC.FLOW_T, None, 0.2, 'bev'))      # (method, threshold, sigma, floor, metric)


def flow_flags(method, threshold, sigma, floor, metric):
    return (['--soft_nms', method, '--soft_nms_min_prob', repr(floor), '--nms_metric', metric]
            + (['--soft_nms_sigma', repr(sigma)] if sigma is not None else []) + (['--nms_iou', repr(threshold)] if threshold is not None else []))


def held_of(ids, kept):
    """The official evaluation's boxes of spec-applied records, as detect.main holds them: ranked by 'soft_prob'."""
    import types
    from transferable3d_amd import evaluate_sunrgbd as ES, semisup_infer as SI
    flat = [(s, r) for s, recs in zip(ids, kept) for r in recs]
    p = SI.Predictions([None] * 14)
    p[3], p[9], p[11] = [None] * len(flat), [r['soft_prob'] for _, r in flat], [s for s, _ in flat]
    p.decoded = types.SimpleNamespace(label=np.stack([r['label'] for _, r in flat]))
    names = [r['class'] for _, r in flat]
    return ES.official_predictions(sorted(set(ES.CLASS_NAMES['AB']) | set(names)), p, names)


def check_flow(rt, root, exact=True):
    """detect --soft_nms on nms_check.write_duplicated's scenes against the specification applied to the plain run's records: the
    records, the result files' last column, the log line, --official_eval (exact only), the two-step route and Detector.detect.  exact:
    the runtime's library is the specification itself, so every byte agrees; otherwise keep and decays agree exactly, soft_prob within
    twice the specification's bound and the files' last column within that plus the half unit of its sixth decimal.  -> report lines."""
    import os
    import detect_check as DC
    from transferable3d_amd import detect as DT, evaluate_sunrgbd as ES, semisup_infer as SI, sunrgbd_data as SD, test_semisup as TS
    from transferable3d_amd.dataset import save_zipped_pickle
    quiet = lambda *a: None
    ids, folder, idx, dets = NC.write_duplicated(root)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS
    res = lambda name: os.path.join(str(root), name)
    DT.main(base + ['--result_dir', res('plain')], rt=rt, log=quiet)
    plain = DC.read_results(res('plain'))
    scenes = DC.load_scenes(root, ids)
    records = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt).detect(scenes, dets, scene_ids=ids)
    lines = DC.record_lines(ids, records)
    assert all(lines.get(c, '') == t for c, t in plain.items()), 'without the flags: the files are the records, all of them'
    assert not any('soft_prob' in r or 'decays' in r for recs in records for r in recs), 'without the flags a record has no soft keys'
    lists = SD.extract_roi_seg_from_rgb_detection(folder, str(root), valid_id_list=ids, seed=3, rt=rt)
    path = res('val_det_dup.zip.pickle')
    save_zipped_pickle(lists, path)
    report = []
    for cfg in FLOW_CONFIGS:
        method, threshold, sigma, floor, metric = cfg
        kept, spec = records_soft(ids, records, method, threshold, sigma or 0.5, floor, metric)
        n_all, n_kept, n_dec = sum(len(r) for r in records), sum(len(k) for k in kept), int((spec.n_decays > 0).sum())
        assert 0 < n_kept < n_all and n_dec > n_all - n_kept, (cfg, n_all, n_kept, n_dec)      # something pruned, something decayed and kept
        want = DC.record_lines(ids, [[dict(r, prob=r['soft_prob']) for r in recs] for recs in kept])
        flags, logged = flow_flags(*cfg), []
        DT.main(base + ['--result_dir', res(method), '--official_eval'] + flags, rt=rt, log=logged.append)
        got = DC.read_results(res(method))
        assert any('soft-nms (%s' % method in l and 'kept %d of %d detections, decayed %d' % (n_kept, n_all, n_dec) in l for l in logged), logged
        det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, soft_nms=method, nms_iou=threshold, soft_nms_sigma=sigma, soft_nms_min_prob=floor,
                          nms_metric=metric)
        recs = det.detect(scenes, dets, scene_ids=ids)
        assert [len(r) for r in recs] == [len(k) for k in kept]
        bound = iter(spec.bound[spec.keep != 0])
        for r, w in ((r, w) for rs, ws in zip(recs, kept) for r, w in zip(rs, ws)):
            b = next(bound)
            assert r['class'] == w['class'] and r['prob'] == w['prob'] and r['decays'] == w['decays'] and np.array_equal(r['corners'], w['corners'])
            assert r['soft_prob'] == w['soft_prob'] if exact or b == 0 else abs(r['soft_prob'] - w['soft_prob']) <= 2 * b, (r['soft_prob'], w['soft_prob'], b)
        if exact:
            assert all(want.get(c, '') == t for c, t in got.items()) and set(want) <= set(got), 'detect --soft_nms differs from the specification on the plain run'
            assert DC.record_lines(ids, [[dict(r, prob=r['soft_prob']) for r in rs] for rs in recs]) == want
            official = []
            ES.evaluate(None, str(root), idx, 'AB', rt=rt, log=official.append, predictions=held_of(ids, kept))
            assert official and all(l in logged for l in official), (official, logged)
        else:
            tol = 2 * float(spec.bound.max()) + 0.5000001e-6
            for c in set(want) | set(got):
                g, w = got.get(c, '').splitlines(), want.get(c, '').splitlines()
                assert len(g) == len(w), c
                for a, b in zip(g, w):
                    assert a.split()[:-1] == b.split()[:-1] and abs(float(a.split()[-1]) - float(b.split()[-1])) <= tol, (a, b)
        for c, t in got.items():              # the lines of the plain run but for the last column, minus the pruned ones, in its order
            left = iter(l.rsplit(' ', 1)[0] for l in plain[c].splitlines())
            assert all(any(l.rsplit(' ', 1)[0] == m for m in left) for l in t.splitlines()), c
        p = SI.test(SI.build_flags(DC.MODEL_FLAGS + ['--from_rgb_detection', '--data_path', path, '--result_dir', res('two_step_' + method),
                                                     '--device_decode'] + flags), rt=rt, log=quiet)
        assert DC.read_results(res('two_step_' + method)) == got, 'semisup_infer --device_decode --soft_nms differs from detect --soft_nms'
        assert len(p[3]) == len(p.decoded) == n_kept and p.decoded.keep.all() and list(p[9]) == [float(v) for v in p.decoded.soft_prob]
        report.append('%s: %d of %d detections kept, %d decayed, largest bound %.3g' % (' '.join(flags), n_kept, n_all, n_dec, float(spec.bound.max())))
    return report


def check_stages(rt, root):
    """--soft_nms beside the other stages, on nms_check.write_duplicated's scenes: with --tta 2 --tta_flip and --consistency the
    decayed confidences, keep and decays equal the specification applied to the run's own final corners and confidences; the --vis_dir
    legends (with --vis_suppressed) and the --consistency_json rows carry 'soft_prob' / 'decays' beside an unchanged 'prob', the pruned
    detections are drawn as 'suppressed' and named by the box that pruned them.  -> report lines."""
    import json
    import os
    import detect_check as DC
    from transferable3d_amd import detect as DT, test_semisup as TS
    from transferable3d_amd.constants import type2class
    method, threshold, sigma, floor, metric = FLOW_CONFIGS[0]
    ids, folder, idx, dets = NC.write_duplicated(root)
    scenes = DC.load_scenes(root, ids)
    det = DT.Detector(TS.build_flags(DC.MODEL_FLAGS), rt=rt, soft_nms=method, soft_nms_sigma=sigma, soft_nms_min_prob=floor, nms_metric=metric,
                      tta=2, tta_flip=True, consistency=True)
    parts = [det.extract(scenes, dets, ids)]
    meta, d = det.decode_all(parts)
    prob = np.asarray([m.prob for m in meta], np.float32)
    offsets, members = NMS.groups_of([m.image for m in meta], [type2class[m.name] for m in meta])
    want = FS.soft_nms(d.corners.astype(np.float32), prob, offsets, members, method, threshold, sigma, floor, NC.METRIC_ID[metric], eps=EPS)
    assert d.view_iou is not None and d.reproj_iou is not None and d.soft_prob is not None
    assert np.array_equal(d.keep, want.keep != 0) and np.array_equal(d.n_decays, want.n_decays) and 0 < d.keep.sum() < len(meta)
    assert np.array_equal(d.suppressed_by, want.suppressed_by)
    assert (np.abs(d.soft_prob - want.score_out) <= 2 * want.bound + 1e-12).all() and np.array_equal(bits(d.soft_prob)[want.bound == 0], bits(prob)[want.bound == 0])
    recs = det.detect(scenes, dets, scene_ids=ids)
    assert all({'soft_prob', 'decays', 'view_iou', 'reproj_iou'} <= set(r) for rs in recs for r in rs) and sum(len(r) for r in recs) == int(d.keep.sum())
    # the command line: pictures with the pruned boxes, and the per-detection rows
    vis, rows_path, logged = os.path.join(str(root), 'vis'), os.path.join(str(root), 'rows.json'), []
    DT.main(['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder] + DC.MODEL_FLAGS + flow_flags(*FLOW_CONFIGS[0])
            + ['--vis_dir', vis, '--vis_suppressed', '--consistency', '--consistency_json', rows_path], rt=rt, log=logged.append)
    rows = json.load(open(rows_path))
    assert len(rows) == len(meta) and all({'prob', 'soft_prob', 'decays', 'kept'} <= set(r) for r in rows)
    assert all(r['kept'] == (r['soft_prob'] >= floor or r['decays'] == 0) for r in rows) and 0 < sum(r['kept'] for r in rows) < len(rows)
    assert all(r['prob'] == float(m.prob) for r, m in zip(rows, meta)) and any(r['decays'] > 0 and r['kept'] for r in rows)
    assert any('soft-nms (%s' % method in l and 'kept %d of %d' % (sum(r['kept'] for r in rows), len(rows)) in l for l in logged), logged
    boxes = [b for f in sorted(os.listdir(vis)) if f.endswith('.json') for b in json.load(open(os.path.join(vis, f)))['boxes']]
    drawn = [b for b in boxes if b['kind'] in ('kept', 'suppressed')]
    assert drawn and all({'prob', 'soft_prob', 'decays'} <= set(b) for b in drawn)
    gone = [b for b in drawn if b['kind'] == 'suppressed']
    assert len(gone) == sum(not r['kept'] for r in rows) and all(b['soft_prob'] < floor and b['decays'] > 0 and b['suppressed_by'] is not None and not b['kept'] for b in gone)
    assert all(b['soft_prob'] <= b['prob'] + 1e-6 for b in drawn)
    with np.testing.assert_raises(ValueError):
        DT.Vis(vis, vis_suppressed=True, nms=False)
    return ['--tta 2 --tta_flip --consistency --soft_nms %s: %d of %d detections kept, %d decayed' % (method, int(d.keep.sum()), len(meta), int((d.n_decays > 0).sum())),
            '--vis_dir --vis_suppressed: %d boxes drawn, %d of them pruned; %d rows in --consistency_json' % (len(drawn), len(gone), len(rows))]
