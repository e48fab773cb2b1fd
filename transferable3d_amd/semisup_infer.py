#!/usr/bin/env python3
"""test_semisup with the detections decoded on the device (t3d_detect_decode, csrc/detect.hip).

    python -m transferable3d_amd.semisup_infer --device_decode <test_semisup's flags>
    python -m transferable3d_amd.semisup_infer --device_decode --from_rgb_detection --nms_iou 0.25 [--nms_metric bev] [--nms_score score] ...

test_semisup's `inference` fetches every batch's logits and six head tensors and decodes them in fp64 NumPy, and its result writers
loop over the detections.  `inference(decode='device')` here follows a batch's graph with one t3d_detect_decode launch on the same
stream, fetches nothing in between, and copies the decoded records (plus the uint8 masks where the caller needs them) back once at
the end.  `test` is test_semisup's driver run with that inference (device_decode_driver); without --device_decode every function
here hands over to test_semisup's, so nothing that exists changes its numbers.

--nms_iou T (with --from_rgb_detection): before the copy back, t3d_detect_nms (nms.py) suppresses, per image and class, every box that
overlaps a better-ranked kept box by more than T; the suppressed detections are absent from the 14-list, the result files and --evaluate.
--nms_fuse [--nms_fuse_iou V] (with --nms_iou): t3d_detect_fuse follows on the same buffers; every kept box is written with the weighted
mean geometry of the boxes it suppressed (nms.DeviceFuse).  Which boxes are kept, and every score, stay.
--soft_nms {gaussian,linear} (with --from_rgb_detection): t3d_detect_soft_nms (nms.DeviceSoftNms) runs in place of t3d_detect_nms; the
confidence of a box that overlaps a better one is decayed and is what the 14-list, the result files and --evaluate then carry; a
detection whose confidence falls below --soft_nms_min_prob is absent like a suppressed one.

What runs behind the decode, and in which order, is written down in one place: `DeviceStages`.  `inference` builds one from its requests
(nms, consistency, views); per batch it decodes every view and then measures the consistency of view 0, after the last batch it runs
the ensemble of the views, the floor stage, the visibility stage, the rescoring, the accept rule (one loop over the run's tests of `TESTS`),
the suppression and the box voting, and fetches everything as one `Decoded`.  It holds the boxes on the device as the stages so far left them, so nothing behind it asks which stage ran.
`DeviceDecode` is the buffers of t3d_detect_decode alone; `report` writes a run's log lines and `kept` drops the rows that were not
kept, for every caller.
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import torch

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import abi, nms as NMS, test_semisup as TS       # noqa: E402
from transferable3d_amd.abi import fptr, iptr                            # noqa: E402
from transferable3d_amd import consistency as CS, ensemble as EN, floor as FL, rescore as RS, visibility as VS      # noqa: E402
from transferable3d_amd.consistency import ConsistencyRequest, DeviceConsistency      # noqa: E402
from transferable3d_amd.constants import type2class                     # noqa: E402

# Every test that can reject a detection (consistency.Test, each stated beside the stage that takes its measure), in the order the
# `consistency:` line prints them.  DeviceStages.accept_rows, `report` and autolabel's counts all run over this tuple.
TESTS = CS.TESTS + (EN.TEST, RS.TEST, FL.TEST, VS.TEST)
# the stages that need the device-decoded boxes: the keyword of `inference`, what it refuses them with under decode='host', and how
# DeviceStages names a request whose length is not the number of detections
REQUESTS = (('nms', "nms runs on the device-decoded boxes: decode='device'", None),
            ('consistency', "the consistency measures are taken on the device-decoded boxes: decode='device'", '%d detections in the consistency request, %d decoded'),
            ('rescore', "the rescoring reads the device-decoded records: decode='device'", '%d confidences in the rescore request, %d decoded'),
            ('floor', "the floor stage reads the device-decoded boxes: decode='device'", '%d detections in the floor request, %d decoded'),
            ('visibility', "the visibility stage reads the device-decoded boxes: decode='device'", '%d detections in the visibility request, %d decoded'))


def active_tests(*holders):
    """[(test, limit, parameters)] of the tests of TESTS that are on: one of `holders` -- the requests of a run, or a Detector and its
    checked floor and visibility options; None counts for nothing -- carries a limit under the flag's name, and the test's parameters
    are attributes of that holder's `options`."""
    return [(t, getattr(h, t.flag), {k: getattr(h.options, k) for k in t.parameters})
            for t in TESTS for h in holders if getattr(h, t.flag, None) is not None]


def build_flags(argv=None):
    """test_semisup.build_flags plus --device_decode (test_semisup's parser is built inside its build_flags and refuses a flag it does
    not declare, so the flag is taken out of argv here)."""
    argv = list(sys.argv[1:] if argv is None else argv)
    device = '--device_decode' in argv
    import argparse
    own = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    NMS.add_arguments(own)
    nms, rest = own.parse_known_args([a for a in argv if a != '--device_decode'])
    FLAGS = TS.build_flags(rest)
    FLAGS.device_decode = device
    FLAGS.suppression = s = NMS.suppression(**vars(nms))
    FLAGS.nms_iou, FLAGS.nms_metric, FLAGS.nms_score, FLAGS.nms_fuse, FLAGS.nms_fuse_iou, FLAGS.soft_nms = s
    if s.on and not (device and FLAGS.from_rgb_detection):
        raise ValueError('--%s runs on the device-decoded boxes of a detection file: it needs --device_decode and --from_rgb_detection'
                         % ('nms_iou' if s.soft is None else 'soft_nms'))
    return FLAGS


class NmsRequest:
    """What `inference(decode='device', nms=...)` needs to run t3d_detect_nms on its decoded corners: the threshold, the metric ('3d' /
    'bev'), what ranks ('prob': the 2-D detection confidences given here; 'score': the decoded network score) and, per detection, the
    image id and the class id that make its group.  fuse: t3d_detect_fuse follows (box voting: a kept box takes the weighted mean
    geometry of the boxes it suppressed); a suppressed box votes above the IoU vote_threshold (default: the threshold, so all of them do)
    with the weight that ranked it -- `prob`, or exp(score) for score='score' (the decoded score is a sum of logs).
    soft ('gaussian' / 'linear'; sigma, min_prob): t3d_detect_soft_nms runs in place of t3d_detect_nms (nms.suppression checks them all: 'linear'
    takes the threshold, 'gaussian' none; the confidences `prob` are decayed, nothing is fused).  `of` takes the checked options as they are."""
    soft = None

    def __init__(self, threshold, metric, score, image_ids, class_ids, prob=None, fuse=False, vote_threshold=None, soft=None, sigma=None,
                 min_prob=None):
        self._set(NMS.suppression(soft, sigma, min_prob, threshold, metric, score, fuse, vote_threshold), image_ids, class_ids, prob)

    @classmethod
    def of(cls, suppression, image_ids, class_ids, prob):
        """The request of a nms.Suppression that is on, as the drivers hold it."""
        req = cls.__new__(cls)
        req._set(suppression, image_ids, class_ids, prob)
        return req

    def _set(self, s, image_ids, class_ids, prob):
        if not s.on:
            raise ValueError('an NMS request needs a threshold')
        self.soft, self.threshold = s.soft, s.nms_iou if s.soft is None else s.soft.threshold
        self.metric, self.score, self.fuse, self.vote_threshold = s.nms_metric, s.nms_score, s.nms_fuse, s.nms_fuse_iou
        self.image_ids, self.class_ids = np.asarray(image_ids, np.int64), np.asarray(class_ids, np.int64)
        self.prob = None if prob is None else np.asarray(prob, np.float32)
        if self.score == 'prob' and (self.prob is None or len(self.prob) != len(self.image_ids)):
            raise ValueError("ranking by 'prob' needs one detection confidence per detection")


class Decoded:
    """The records of t3d_detect_decode in host memory, one row per detection: score, mask_count, heading_cls, size_cls, center [n,3],
    heading_res, size_res [n,3], label [n,7] = (h, w, l, tx, ty, tz, ry) as from_prediction_to_label_format, corners [n,8,3] as
    get_3d_box in the camera frame.  It travels beside the 14-list; write_detection_results, evaluate_sunrgbd.official_predictions and
    eval_det.evaluate_predictions read label / corners from it instead of looping over the detections.
    keep [n] bool and suppressed_by [n] (-1: kept; else the row of the better-ranked box that suppressed this one) are what t3d_detect_nms
    answered, or None where no suppression was asked for.  A sliced Decoded carries its rows' values; suppressed_by keeps naming rows of
    the unsliced run.
    reproj_rect [n,4], reproj_iou, n_mask, n_box, n_both, flags, mask_in_box, seg_box_iou are what t3d_detect_consistency measured
    (consistency.py); None where no consistency request was made.  accept [n] bool: whether none of the run's tests (TESTS) rejects
    the detection -- True for the rows that pad a last batch, which are no detections -- or None where the run measured no
    consistency and had no test with a limit.
    With a fusion (NmsRequest(fuse=True)) label and corners hold what t3d_detect_fuse wrote -- for a kept box with voters the fused
    geometry, for every other box what the decode wrote -- raw_label / raw_corners what the decode wrote, and n_votes [n] the number of
    voters of a kept box (-1: suppressed; 0: nothing to fuse, or listed in no group); None without.  center, heading_cls, heading_res,
    size_cls and size_res are NOT fused: they keep what the decode wrote and describe the raw box.
    With views (inference(views=...), ensemble.py) label and corners hold what t3d_detect_ensemble wrote (and, with a fusion, what
    t3d_detect_fuse made of that: raw_label / raw_corners are then the ensemble's output); view_label [V,n,7] and view_score [V,n] what
    the decode wrote per view, view_iou [n] the mean and view_min_iou [n] the smallest pairwise IoU of a detection's views, anchor_view
    [n] the view the fused box was built around (-1: no view with a finite label) and n_views_voted [n] the views that voted beside it;
    None without.  score, mask_count, the heads and the consistency measures stay those of view 0.
    With Soft-NMS (NmsRequest(soft=...)) soft_prob [n] is the confidence t3d_detect_soft_nms left of every detection -- the 2-D
    detector's where nothing decayed it -- and n_decays [n] the number of better boxes that decayed it; keep is False for a detection
    whose confidence fell below the floor and suppressed_by names the box whose decay took it there; None without.
    With a rescoring model (RescoreRequest, rescore.py) rescore_prob [n] is the confidence t3d_rescore_apply gave every detection from
    its measures; the suppression stages then rank by it where they rank by 'prob' (and soft_prob is what Soft-NMS left of it); None
    without.
    With a floor request (floor.FloorRequest) floor_gap [n] is how far the floor of the detection's scene lies below the bottom of its
    box (positive: the box floats; negative: it sinks; NaN: no floor is known) and floor_flags [n] the bits t3d_detect_floor set, both
    measured on the box the stage read: the ensemble's where views ran.  Where the request snaps, label and corners hold what the stage
    wrote (and a fusion's raw_label / raw_corners with them) and unsnapped_label / unsnapped_corners what it read; None without.
    With a visibility request (visibility.VisibilityRequest) see_through, occluded and support [n] are what t3d_detect_visibility
    measured of the box the stage read (the floor stage's where it snapped), visibility_flags [n] the bits it set and visibility_profile
    [n, 6] the counts behind them (abi.VIS_PROFILE: rays, unknown, front, inside, through, graze); None without."""
    FIELDS = ('score', 'mask_count', 'heading_cls', 'size_cls', 'center', 'heading_res', 'size_res', 'label', 'corners')
    OPTIONAL = ('keep', 'suppressed_by', 'reproj_rect', 'reproj_iou', 'n_mask', 'n_box', 'n_both', 'flags', 'mask_in_box', 'seg_box_iou', 'accept',
                'raw_label', 'raw_corners', 'n_votes', 'view_label', 'view_score', 'view_iou', 'view_min_iou', 'anchor_view', 'n_views_voted',
                'soft_prob', 'n_decays', 'rescore_prob', 'floor_gap', 'floor_flags', 'unsnapped_label', 'unsnapped_corners', 'see_through', 'occluded',
                'support', 'visibility_flags', 'visibility_profile')
    VIEW_MAJOR = ('view_label', 'view_score')              # [V, n, ...]: the detection is the second axis

    def __init__(self, **fields):
        for k in self.FIELDS:
            setattr(self, k, fields[k])
        for k in self.OPTIONAL:
            setattr(self, k, fields.get(k))

    def __len__(self):
        return len(self.score)

    def __getitem__(self, sel):
        """Rows `sel` (a slice or an index array)."""
        return Decoded(**{k: getattr(self, k)[sel] for k in self.FIELDS},
                       **{k: getattr(self, k)[:, sel] if k in self.VIEW_MAJOR else getattr(self, k)[sel]
                          for k in self.OPTIONAL if getattr(self, k) is not None})

    def confidence(self, prob):
        """What the result files write and the evaluation rank by, per detection: what Soft-NMS left where it ran, else the rescored
        confidence (either as Python floats), else `prob`, the 2-D detector's, as it is."""
        best = self.soft_prob if self.soft_prob is not None else self.rescore_prob
        return prob if best is None else [float(v) for v in best]


class Predictions(list):
    """test_semisup's 14-list; `.decoded` (Decoded or None) holds the device-decoded records of the same detections."""
    decoded = None


class InferenceResult(tuple):
    """The 7-tuple of `inference`; `.decoded` as above; `.device` the DeviceStages of the run, whose buffers still hold the records on the
    device: `.device.corners` [n, 24] are the boxes after every stage that ran, `.device.score` [n] the decoded scores."""
    decoded = None
    device = None


class DeviceDecode:
    """Output buffers of t3d_detect_decode for `n` frustums (planar sections of one fp32 and one int32 allocation, so that everything
    comes back in two copies) and the launch of one batch of them."""
    WIDTH = (('score', 1), ('center', 3), ('heading_res', 1), ('size_res', 3), ('label', 7), ('corners', 24))
    INTS = ('mask_count', 'heading_cls', 'size_cls')

    def __init__(self, rt, n, num_point, want_seg=False):
        self.rt, self.n, self.N = rt, n, num_point
        self.f = rt.zeros(n * sum(w for _, w in self.WIDTH))
        self.i = rt.zeros(n * len(self.INTS), dtype=torch.int32)
        self.seg = rt.zeros(n, num_point, dtype=torch.uint8) if want_seg else None
        self.sec, o = {}, 0
        for k, w in self.WIDTH:
            self.sec[k] = self.f[o:o + n * w].view(n, w)
            o += n * w
        for j, k in enumerate(self.INTS):
            self.sec[k] = self.i[j * n:(j + 1) * n]

    def launch(self, first, B, n_valid, logits, box_out, stage1_center, total_delta=None, fit_prob=None, rot_angle=None):
        """Decode the batch whose frustums are rows first .. first + B - 1 of the outputs; the first `n_valid` of them are real."""
        assert 0 <= first and first + B <= self.n and logits.numel() == B * self.N * 2
        o = {k: v[first:first + B] for k, v in self.sec.items()}
        a = abi.DetectDecodeArgs(B, self.N, int(n_valid), int(box_out.stride(0)), fptr(logits), fptr(box_out), fptr(stage1_center),
                                 fptr(total_delta), fptr(fit_prob), fptr(rot_angle), abi.u8ptr(None if self.seg is None else self.seg[first:]),
                                 fptr(o['score']), iptr(o['mask_count']), iptr(o['heading_cls']), iptr(o['size_cls']), fptr(o['center']),
                                 fptr(o['heading_res']), fptr(o['size_res']), fptr(o['label']), fptr(o['corners']))
        abi.check(self.rt.lib.t3d_detect_decode(C.byref(a), self.rt.stream()), 't3d_detect_decode')

    def fetch(self):
        """-> (Decoded, masks [n, N] uint8 or None): the copies back."""
        f, i = self.f.cpu().numpy().astype(np.float64), self.i.cpu().numpy().astype(np.int64)
        n, out, o = self.n, {}, 0
        for k, w in self.WIDTH:
            out[k] = f[o:o + n * w].reshape((n, w) if w > 1 else (n,))
            o += n * w
        out['corners'] = out['corners'].reshape(n, 8, 3)
        for j, k in enumerate(self.INTS):
            out[k] = i[j * n:(j + 1) * n]
        return Decoded(**out), (None if self.seg is None else self.seg.cpu().numpy())


class DeviceStages:
    """The stages behind t3d_detect_decode of one `inference(decode='device')` run over `n` frustums, the first `total` of them real, and
    the one place that says in which order they run.  Per batch (`launch`): the decode of every view, then -- behind view 0's -- the
    consistency measures.  After the last batch (`finish`): the ensemble of the views, the floor stage, the visibility stage, the rescoring, the accept rows, the
    suppression, the box voting, and the one fetch of everything as a Decoded.

    label [n, 7], corners [n, 24]: the boxes on the device as the stages so far left them -- a stage that rewrites boxes (the ensemble,
    the floor stage where it snaps, the box voting) reads them and puts its output in their place, so neither a later stage nor a caller asks which stage ran; score [n]:
    where view 0's decode wrote it.  tests: the tests of TESTS for which a request carries a limit (`active_tests`); accept [n] bool
    (None: nothing was asked that could reject): the detections none of them rejects; below: per flag of `tests`, how many of the real
    detections its test rejects (`report`).  rescore_out (rescore.DeviceRescore, None without a request): its out32 [n] is the
    rescored confidence on the device, which `nms` ranks by in the place of the request's `prob`."""

    def __init__(self, rt, n, total, num_point, want_seg=False, nms=None, consistency=None, views=None, rescore=None, floor=None, visibility=None):
        if nms is not None and len(nms.image_ids) != total:
            raise ValueError('%d image ids for %d detections' % (len(nms.image_ids), total))
        requests = dict(consistency=consistency, rescore=rescore, floor=floor, visibility=visibility)
        for name, _, message in REQUESTS:
            if requests.get(name) is not None and len(requests[name]) != total:
                raise ValueError(message % (len(requests[name]), total))
        if rescore is not None:
            names = rescore.model.features
            if 'view_iou' in names and views is None:
                raise ValueError('the rescoring model reads view_iou, the agreement of the augmented views: it needs --tta')
            if consistency is None and any(k in names for k in ('reproj_iou', 'mask_in_box', 'seg_box_iou', 'log_mask')):
                raise ValueError('the rescoring model reads the consistency measures: it needs a consistency request')
        self.rt, self.n, self.total, self.nms_request, self.views = rt, n, total, nms, views
        self.rescore_request, self.rescore_out = rescore, None
        self.floor_request, self.floor_out, self.floor_in, self.floor_host = floor, None, None, None
        self.visibility_request, self.visibility_out, self.visibility_host = visibility, None, None
        self.decodes = [DeviceDecode(rt, n, num_point, want_seg=want_seg and v == 0) for v in range(1 if views is None else len(views))]
        self.consistency = None if consistency is None else DeviceConsistency(rt, n, num_point, consistency)
        self.rot_angle = None if views is None else rt.zeros(n)      # every batch's angles: the ensemble mirrors back with them
        sec = self.decodes[0].sec
        self.label, self.corners, self.score = sec['label'], sec['corners'], sec['score'].view(-1)
        self.tests = active_tests(consistency, views, rescore, floor, visibility)
        self.accept, self.below = None, {}
        self.measures = self.ensemble_out = self.nms_out = self.fuse_out = None

    def launch(self, view, first, B, n_valid, heads, rot_angle=None, xyz=None):
        """Behind the graph's run of one view of a batch (a batch's view 0 runs last): t3d_detect_decode on `heads` (`decode_sources`)
        into the view's rows first .. first + B - 1 and, behind view 0's, t3d_detect_consistency on the points xyz [B * N, ld] the network
        read, the logits and the corners just written."""
        self.decodes[view].launch(first, B, n_valid, *heads, rot_angle)
        if view == 0 and self.rot_angle is not None:
            self.rot_angle[first:first + B].copy_(rot_angle.view(-1)[:B])
        if view == 0 and self.consistency is not None:
            self.consistency.launch(first, B, n_valid, xyz, int(xyz.stride(0)), heads[0], self.corners[first:], rot_angle)

    def finish(self):
        """After the last batch -> (Decoded, masks [n, N] uint8 or None)."""
        if self.views is not None:
            self.ensemble()
        if self.floor_request is not None:
            self.floor()
        if self.visibility_request is not None:
            self.visibility()
        if self.rescore_request is not None:
            self.rescore()
        self.accept_rows()
        if self.nms_request is not None:
            self.nms()
        return self.fetch()

    def ensemble(self):
        """t3d_detect_ensemble over all rows of the views' decodes: a view's weight is exp of its decoded score (what `nms` votes with
        for score='score')."""
        req, self.ensemble_out = self.views, EN.DeviceEnsemble(self.rt)
        out = self.ensemble_out.run([d.sec['label'] for d in self.decodes], [torch.exp(d.sec['score'].view(-1)) for d in self.decodes],
                                    self.corners, req.flip_mask, self.rot_angle, req.vote_threshold, req.metric)
        self.label, self.corners = out[0], out[1]

    def floor(self):
        """t3d_detect_floor on the current boxes: the gap between every box's bottom and its scene's floor and, where the request snaps,
        the boxes standing on it in the place of the ones it read (`floor_in`)."""
        self.floor_out = FL.DeviceFloorStage(self.rt)
        out = self.floor_out.run(self.label, self.corners, self.floor_request, self.n)
        if out is not None:
            self.floor_in = (self.label, self.corners)
            self.label, self.corners = out

    def visibility(self):
        """t3d_detect_visibility on the current boxes: every box against the range map of its scene.  It moves no box."""
        self.visibility_out = VS.DeviceVisibilityStage(self.rt)
        self.visibility_out.run(self.label, self.corners, self.visibility_request, self.n)

    def rescore(self):
        """t3d_rescore_features on the buffers the stages so far wrote -- the 2-D confidences, view 0's decoded score, the consistency
        kernel's rectangle and counts, the ensemble's agreement -- and t3d_rescore_apply of the request's model over the real rows."""
        req, total = self.rescore_request, self.total
        out = self.rescore_out = RS.DeviceRescore(self.rt, self.n, req.model.features)
        prob = self.rt.zeros(self.n)
        prob[:total] = torch.from_numpy(req.prob).to(self.rt.device)
        con, ens = self.consistency, self.ensemble_out
        out.features(prob, self.score, None if con is None else con.reproj, None if con is None else con.counts,
                     None if ens is None else ens.agreement)
        out.load(req.model)
        out.apply(n_valid=total)

    def accept_rows(self):
        """The one accept rule: a detection is rejected where one of the run's tests (`tests`, of TESTS) rejects it; `below` counts,
        per flag, the real detections it rejects.  The rows that pad a last batch are no detections: every test accepts them.  Copies
        the consistency outputs, the agreement, the rescored confidence and the floor and visibility measures back -- the small copies
        in front of the group building."""
        total, host = self.total, {}
        if self.consistency is not None:
            self.measures = self.consistency.fetch()
            host.update(self.measures)
        if self.views is not None and self.views.min_view_iou is not None:
            host['view_iou'] = self.ensemble_out.agreement[:self.n].cpu().numpy().astype(np.float64)
        if self.rescore_request is not None and self.rescore_request.min_rescore is not None:
            host['rescore_prob'] = self.rescore_out.out[:self.n].cpu().numpy()
        if self.floor_out is not None:
            self.floor_host = (self.floor_out.gap[:self.n].cpu().numpy(), self.floor_out.flags[:self.n].cpu().numpy().astype(np.int64))
            host['floor_gap'], host['floor_flags'] = self.floor_host
        if self.visibility_out is not None:
            h = self.visibility_host = self.visibility_out.fetch(self.n)
            host.update(see_through=h['measures'][:, 0], visibility_evidence=VS.evidence(h['profile']), visibility_flags=h['flags'])
        if not self.tests and self.consistency is None:
            return
        self.accept = np.ones(self.n, bool)
        for test, limit, parameters in self.tests:
            bad = test.rejected(*(host[k][:total] for k in test.fields), limit, **parameters)
            self.below[test.flag] = int(bad.sum())
            self.accept[:total] &= ~bad

    def nms(self):
        """t3d_detect_nms over the real rows, on the current corners.  A rejected detection is listed in no group, so it suppresses
        nothing and comes back as kept (`accept` says it is rejected).  With a request that fuses, t3d_detect_fuse follows directly on the
        same buffers (a row in no group neither votes nor is fused) and its output becomes the current boxes.  With a soft request
        t3d_detect_soft_nms runs in its place, on the same groups: a row in no group keeps its confidence.  Where the rescoring stage
        ran, 'prob' is the confidence it left on the device, not the request's."""
        req, total = self.nms_request, self.total
        rows = np.arange(total) if self.accept is None else np.nonzero(self.accept[:total])[0]
        offsets, members = NMS.groups_of(req.image_ids[rows], req.class_ids[rows])
        score = self.score
        if req.score == 'prob' and self.rescore_out is not None:
            score = self.rescore_out.out32                        # the rescored confidence, where the stage wrote it
        elif req.score == 'prob':
            score = self.rt.zeros(self.n)
            score[:total] = torch.from_numpy(req.prob).to(self.rt.device)
        if req.soft is not None:
            self.nms_out = NMS.DeviceSoftNms(self.rt)
            self.nms_out.run(self.corners, score, offsets, rows[members].astype(np.int32), req.soft.method, req.soft.threshold, req.soft.sigma,
                             req.soft.min_prob, req.soft.metric)
            return
        self.nms_out = NMS.DeviceNms(self.rt)
        self.nms_out.run(self.corners, score, offsets, rows[members].astype(np.int32), req.threshold, req.metric)
        if req.fuse:
            self.fuse_out = NMS.DeviceFuse(self.rt)
            out = self.fuse_out.run(self.nms_out, self.label, self.corners, score if req.score == 'prob' else torch.exp(score), req.vote_threshold)
            self.label, self.corners = out[0], out[1]

    def fetch(self):
        """-> (Decoded, masks): the copies back of the decode's records and of what every stage that ran added to them (Decoded)."""
        n = self.n
        d, seg = self.decodes[0].fetch()
        host = lambda t, dtype=np.float64: t[:n].cpu().numpy().astype(dtype)
        if self.nms_out is not None:
            d.keep, d.suppressed_by = host(self.nms_out.keep, bool), host(self.nms_out.suppressed_by, np.int64)
            if self.nms_request.soft is not None:
                d.soft_prob, d.n_decays = host(self.nms_out.score_out), host(self.nms_out.n_decays, np.int64)
        if self.ensemble_out is not None:
            e = self.ensemble_out
            d.view_label = np.stack([host(v.sec['label']) for v in self.decodes])
            d.view_score = np.stack([host(v.sec['score'].view(-1)) for v in self.decodes])
            d.label, d.corners = host(e.label), host(e.corners).reshape(n, 8, 3)
            d.view_iou, d.view_min_iou = host(e.agreement), host(e.min_iou)
            d.anchor_view, d.n_views_voted = host(e.anchor, np.int64), host(e.n_votes, np.int64)
        if self.floor_out is not None:
            d.floor_gap, d.floor_flags = self.floor_host
            if self.floor_in is not None:
                d.unsnapped_label, d.unsnapped_corners = d.label, d.corners
                d.label, d.corners = host(self.floor_out.label_out), host(self.floor_out.corners_out).reshape(n, 8, 3)
        if self.visibility_out is not None:
            h = self.visibility_host
            d.see_through, d.occluded, d.support = (h['measures'][:, k].copy() for k in range(3))
            d.visibility_flags, d.visibility_profile = h['flags'], h['profile']
        if self.fuse_out is not None:
            d.raw_label, d.raw_corners = d.label, d.corners
            d.label, d.corners = host(self.label), host(self.corners).reshape(n, 8, 3)
            d.n_votes = host(self.fuse_out.n_votes, np.int64)
        for k, v in (self.measures or {}).items():
            if k in Decoded.OPTIONAL:
                setattr(d, k, v)
        if self.rescore_out is not None:
            d.rescore_prob = host(self.rescore_out.out)
        d.accept = self.accept
        return d, seg


def decode_sources(ops, prefix, use_boxpc_fit_prob=False):
    """The device buffers behind the heads `prefix` of an inference graph: (logits, box_out [B, >= 67], stage1_center, total_delta or
    None, fit_prob or None).  The F2_ heads are the F_ heads minus the accumulated Box-PC deltas (semisup_v1_sunrgbd.get_semi_model_final)."""
    ep = ops['end_points']
    box = ep[prefix + 'heading_scores'].src                 # semisup_models.BoxHeads slices the [B, 67] head output
    delta = None
    src = getattr(ep[prefix + 'center'], 'src', None)
    if src is not box:                                      # a refined centre: its source is the accumulated deltas
        if getattr(src, 'name', None) != 'total_delta':
            raise NotImplementedError('decode on the device: the %s heads are not a head output minus total_delta' % prefix)
        delta = src.buf
    fit = ep['boxpc_fit_prob'].buf if use_boxpc_fit_prob else None
    bufs = (ops['logits'].buf, box.buf, ep['stage1_center'].buf, delta, fit)
    if any(t is not None and t.element_size() < 4 for t in bufs):
        raise NotImplementedError('decode on the device reads fp32 logits and heads')
    return bufs


def inference(sess, ops, pc, one_hot_vec, batch_size, prefix='', use_boxpc_fit_prob=False, source=None, n_batches=None, oracle_mask=None,
              decode='host', want_seg=True, nms=None, consistency=None, views=None, rescore=None, floor=None, visibility=None):
    """test_semisup.inference with `decode`: 'host' is that function; 'device' runs t3d_detect_decode behind every batch's graph and
    returns the same 7-tuple (InferenceResult; the records as `.decoded`; the mask entry is None unless `want_seg`).  The rows of a
    padded last batch are zeros.  nms (NmsRequest, decode='device' only): t3d_detect_nms runs on the decoded corners before anything is
    copied back; `.decoded.keep` / `.suppressed_by` hold its answer (None without it).  Nothing is removed here: the callers drop the rows.
    With nms.fuse, t3d_detect_fuse follows it and `.decoded.label` / `.corners` hold the fused boxes (Decoded).
    consistency (ConsistencyRequest, decode='device' only): t3d_detect_consistency follows every batch's decode on the points the network
    read, the logits, the corners just written and the batch's rotation angles; `.decoded.reproj_iou`, `.n_mask`, ... `.accept` hold what
    it measured.  Its outputs are copied back before the NMS groups are built: a detection below a threshold of the request is listed
    in no group, so a box the filter rejects cannot suppress a good one (its `keep` stays True; `accept` says it is rejected).
    views (ensemble.EnsembleRequest, decode='device' with a `source` only): every batch is assembled, run and decoded once per view --
    view 0 is `source` itself, view v its `source.view(seed, mirrored)` -- each into a DeviceDecode of its own; the consistency kernel
    still follows view 0's decode.  After the last batch one t3d_detect_ensemble call fuses the views of every detection; the NMS, the
    box voting and `.decoded.label` / `.corners` then read its output, `.decoded.view_*` / `.anchor_view` / `.n_views_voted` say what
    it found (Decoded), and a detection whose view_iou lies below views.min_view_iou is rejected as one below a consistency threshold.
    rescore (rescore.RescoreRequest, decode='device' only): behind the ensemble, t3d_rescore_features and t3d_rescore_apply give every
    detection one confidence from its measures (`.decoded.rescore_prob`); a detection below rescore.min_rescore is rejected like one below
    a consistency threshold, and an nms request that ranks by 'prob' ranks by the rescored confidence.
    floor (floor.FloorRequest, decode='device' only): behind the ensemble, t3d_detect_floor measures every box against the floor plane of
    its scene (`.decoded.floor_gap` / `.floor_flags`), stands it on the floor where the request snaps, and a detection whose |floor_gap|
    exceeds floor.max_floor_gap is rejected like one below a consistency threshold.
    visibility (visibility.VisibilityRequest, decode='device' only): behind the floor stage, t3d_detect_visibility holds every box against
    the range map of its scene (`.decoded.see_through` / `.occluded` / `.support` / `.visibility_flags`), and a detection whose
    see_through exceeds visibility.max_see_through on enough rays is rejected like one below a consistency threshold.
    The stages and their order are DeviceStages'; this function loads and runs the graph and says when a view of a batch is ready."""
    requests = dict(nms=nms, consistency=consistency, rescore=rescore, floor=floor, visibility=visibility)
    for name, message, _ in REQUESTS:
        if decode == 'host' and requests[name] is not None:
            raise ValueError(message)
    if views is not None and (decode != 'device' or source is None):
        raise ValueError("views are further draws of a device-resident source: decode='device' and a source")
    if decode == 'host':
        return TS.inference(sess, ops, pc, one_hot_vec, batch_size, prefix=prefix, use_boxpc_fit_prob=use_boxpc_fit_prob, source=source,
                            n_batches=n_batches, oracle_mask=oracle_mask)
    if decode != 'device':
        raise ValueError("decode is 'host' or 'device'")
    if source is not None:
        n, npts = n_batches * batch_size, sess.g.engine.rpf
    else:
        assert pc.shape[0] % batch_size == 0
        n, npts = pc.shape[0], pc.shape[1]
    heads = decode_sources(ops, prefix, use_boxpc_fit_prob)
    total = source.ds.F if source is not None else n                 # the frustums past it pad the last batch
    rot = sess.g.inputs.rot_frust if source is not None else None    # written by t3d_batch_assemble; fed frustums are in their centre view
    xyz = sess.g.inputs.pc if consistency is not None else None      # [B * N, ld] where the network read the batch
    stages = DeviceStages(sess.g.rt, n, total, npts, want_seg=want_seg, views=views, **requests)
    sources = [source] + ([] if views is None else [source.view(seed, flip) for seed, flip in views.views[1:]])
    for i in range(n // batch_size):
        sl = slice(i * batch_size, (i + 1) * batch_size)
        for v in range(len(sources) - 1, -1, -1):                    # view 0 last: the consistency kernel reads its points and logits
            if sources[v] is not None:
                sources[v].load(i, labels=False)
                sess.run([])
            else:
                feed = {ops['pc_pl']: pc[sl], ops['one_hot_vec_pl']: one_hot_vec[sl]}
                if oracle_mask is not None:
                    feed[ops['y_seg_pl']] = np.asarray(oracle_mask[sl], np.int32)
                sess.run([], feed_dict=feed)
            stages.launch(v, sl.start, batch_size, max(0, min(batch_size, total - sl.start)), heads, rot, xyz)
    d, seg = stages.finish()
    res = InferenceResult((None if seg is None else seg.astype(np.int64), d.center, d.heading_cls, d.heading_res, d.size_cls, d.size_res,
                           d.score))
    res.decoded = d
    res.device = stages
    return res


def write_detection_results(result_dir, test_classes, predictions, class_names):
    """test_semisup.write_detection_results; predictions that carry decoded records are written from their label rows."""
    decoded = getattr(predictions, 'decoded', None)
    if decoded is None:
        return TS.write_detection_results(result_dir, test_classes, predictions, class_names)
    os.makedirs(result_dir, exist_ok=True)
    files = {c: open(os.path.join(result_dir, c + '_pred.txt'), 'w') for c in test_classes}
    score_l, id_l, box2d_l = predictions[9], predictions[11], predictions[12]
    for i in range(len(decoded)):
        box2d = box2d_l[i] if box2d_l is not None else (0.0, 0.0, 0.0, 0.0)
        files[class_names[i]].write('%d %s -1 -1 -10 %f %f %f %f %f %f %f %f %f %f %f %f\n' % (
            (int(id_l[i]), class_names[i], box2d[0], box2d[1], box2d[2], box2d[3]) + tuple(decoded.label[i]) + (float(score_l[i]),)))
    for f in files.values():
        f.close()


def report(log, stages, d):
    """What a run says of its stages, one line each through `log` and in their order: `consistency:` (how many detections the accept rule
    kept, how many lie below each threshold), `tta:` (the views) and `nms ...` (how many of the accepted detections were kept and, with
    a fusion, how many kept boxes changed, from how many votes); `floor:` (floor.log_line) follows `tta:` and `visibility:` (visibility.log_line) follows that.  stages: the run's DeviceStages; d: the records of its real detections."""
    if d.accept is not None:
        log(CS.log_line(d.accept, stages.below, [limit for _, limit, _ in stages.tests], [test for test, _, _ in stages.tests]))
    if stages.views is not None:
        log(EN.log_line(stages.views, d))
    if stages.floor_request is not None:
        log(FL.log_line(stages.floor_request, d.floor_gap, d.floor_flags))
    if stages.visibility_request is not None:
        host = dict(measures=np.stack([d.see_through, d.occluded, d.support], 1), profile=d.visibility_profile, flags=d.visibility_flags)
        log(VS.log_line(stages.visibility_request, host))
    req = stages.nms_request
    if req is not None:
        kept, offered = (d.keep, len(d)) if d.accept is None else (d.keep & d.accept, int(d.accept.sum()))
        if req.soft is not None:
            o = req.soft
            how = 'sigma %g' % o.sigma if o.method == 'gaussian' else 'IoU > %g' % o.threshold
            log('soft-nms (%s, %s, %s IoU, floor %g): kept %d of %d detections, decayed %d'
                % (o.method, how, o.metric, o.min_prob, int(kept.sum()), offered, int((d.n_decays > 0).sum())))
            return
        line = 'nms (%s IoU > %g, ranked by %s): kept %d of %d detections' % (req.metric, req.threshold, req.score, int(kept.sum()), offered)
        if d.n_votes is not None:
            v = d.n_votes[d.n_votes > 0]
            line += ', fused %d boxes from %d votes' % (len(v), int(v.sum()))
        log(line)


def kept(d, *lists):
    """The records `d` (Decoded or None) and the per-detection lists that run beside them (None stays None) without the rows that were
    not kept (d.keep) -> (d, *lists); as they are where nothing was asked for that drops a row."""
    if d is None or d.keep is None:
        return (d,) + lists
    rows = np.nonzero(d.keep)[0]
    return (d[rows],) + tuple(l if l is None else [l[i] for i in rows] for l in lists)


@contextlib.contextmanager
def device_decode_driver(FLAGS):
    """test_semisup's driver functions (`test`, `test_on_frustum_file`) look three names up at the moment they call them: `inference` and
    `write_detection_results` in their own module, `evaluate_predictions` in eval_det.  For the length of one run those names are bound
    to the versions that decode on the device and that read the decoded records; everything else of the driver -- weights, batches, the
    14-list, the ground truth of --evaluate, --gt_path, --output -- is test_semisup's own code, run once, not copied.  Yields the
    function that attaches the run's records to its 14-list.  One run at a time per process: the binding is module-wide."""
    from transferable3d_amd import eval_det
    run = {}

    def attach(predictions):
        d = run.get('decoded')
        if d is not None and len(predictions[3]) != len(d):       # the rows t3d_detect_nms suppressed are dropped already
            lists, d = predictions, kept(d)[0]
        else:
            d, *lists = kept(d, *predictions)
        p = Predictions(lists)
        if d is not None:                                         # the confidence the files and the evaluation rank by
            p[9] = d.confidence(p[9])
        p.decoded = d
        return p

    def infer(sess, ops, pc, one_hot_vec, batch_size, **kw):
        source = kw.get('source')
        s = getattr(FLAGS, 'suppression', None)                   # (FLAGS of test_semisup.build_flags have none)
        req = None
        if s is not None and s.on:
            req = NmsRequest.of(s, source.ds.image_ids, [type2class[t] for t in source.ds.class_names], source.ds.prob)
        res = inference(sess, ops, pc, one_hot_vec, batch_size, decode='device', want_seg=source is None or bool(FLAGS.output), nms=req, **kw)
        run['decoded'] = res.decoded[slice(0, res.device.total)]                     # without the padding
        report(run.get('log') or print, res.device, run['decoded'])
        seg = res[0] if res[0] is not None else np.full(len(res.decoded), None)      # (no --output: the masks stayed on the device)
        return (seg,) + tuple(res[1:])

    real_evaluate = eval_det.evaluate_predictions
    saved = (TS.inference, TS.write_detection_results)
    TS.inference = infer
    TS.write_detection_results = lambda d, classes, predictions, names: write_detection_results(d, classes, attach(predictions),
                                                                                                kept(run.get('decoded'), names)[1])
    eval_det.evaluate_predictions = lambda predictions, *a, **kw: real_evaluate(attach(predictions), *a, **kw)
    attach.run = run
    try:
        yield attach
    finally:
        TS.inference, TS.write_detection_results = saved
        eval_det.evaluate_predictions = real_evaluate


def test(FLAGS, rt=None, log=print):
    """test_semisup.test -> Predictions (its 14-list; with FLAGS.device_decode the decoded records as `.decoded`)."""
    if not getattr(FLAGS, 'device_decode', False):
        return Predictions(TS.test(FLAGS, rt=rt, log=log))
    with device_decode_driver(FLAGS) as attach:
        attach.run['log'] = log
        return attach(TS.test(FLAGS, rt=rt, log=log))


if __name__ == '__main__':
    test(build_flags())
