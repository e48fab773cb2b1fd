#!/usr/bin/env python3
"""Scenes and 2-D detections in, 3-D boxes out, in one process and without a frustum file.

    python -m transferable3d_amd.detect --dataset_dir D --idx_path I --rgb_detection_path DETS --model_path M [--boxpc_model_path P] \
        --result_dir R [--official_eval [--diagnose [--diagnose_bg 0.1] [--diagnose_json FILE] [--diagnose_parts]]]
        # + test_semisup's model flags (--semi_type, --refine, --pred_prefix, --num_point, ...)
        [--nms_iou T [--nms_metric {3d,bev}] [--nms_score {prob,score}] [--nms_fuse] [--nms_fuse_iou V]]
        [--soft_nms gaussian [--soft_nms_sigma S] | --soft_nms linear --nms_iou T] [--soft_nms_min_prob F] [--nms_metric {3d,bev}]
        [--vis_dir DIR [--vis_max N] [--vis_gt] [--vis_suppressed]]
        [--consistency] [--min_reproj_iou T] [--min_mask_in_box F] [--min_seg_box_iou F] [--consistency_json FILE]
        [--tta K [--tta_flip] [--tta_vote_iou V] [--min_view_iou A]]
        [--sweep [--sweep_nms_iou V ..] [--sweep_min_reproj_iou V ..] [--sweep_min_mask_in_box V ..] [--sweep_min_seg_box_iou V ..]
                 [--sweep_json FILE] [--sweep_top N]]
        [--bootstrap R [--bootstrap_seed S] [--bootstrap_level L] [--bootstrap_json FILE]]
        [--rescore MODEL.json [--min_rescore P]]
        [--rescore_fit MODEL.json [--rescore_classes C ..] [--rescore_target {overlap,tp}] [--rescore_lambda L] [--rescore_holdout H]
                       [--rescore_features NAME ..]]
        [--floor] [--snap_floor {shift,stretch} [--snap_floor_max M]] [--max_floor_gap G] [--floor_json FILE]
        [--floor_bin B] [--floor_range LO HI] [--floor_min_share F] [--floor_band D] [--floor_max_tilt DEG]
        [--visibility] [--visibility_cell PX] [--visibility_margin M] [--visibility_min_chord M]
        [--max_see_through F [--visibility_min_rays N]]

What `sunrgbd_data --option rgb_detection` followed by `semisup_infer --from_rgb_detection --device_decode` computes, with the frustum
points staying where t3d_frustum_extract wrote them: extraction -> DeviceFrustumSet.from_device -> DeviceEvalSource -> the network ->
t3d_detect_decode.  Two things cross to the host: the per-job point counts of every extraction launch (the reference drops a frustum
of fewer than 5 points, sunrgbd_data.py:313-315) and the decoded records at the end.

As in test_semisup, a frustum's N points are drawn by a hash of (seed, batch, slot): its boxes depend on its position among the
frustums of the call.  One call over the scenes of a run therefore equals the two-step route over the same detections, and a call over
a part of them does not.

--nms_iou T: a 2-D detector reports one object several times, every report becomes a 3-D box, and the evaluation counts all but one of
them as false positives.  With the flag, t3d_detect_nms (nms.py) suppresses, per image and class, every box whose IoU with a
better-ranked kept box exceeds T, on the decoded corners where they lie; the suppressed detections are absent from everything this
module hands out.  Without it nothing changes.

--nms_fuse (with --nms_iou): box voting.  The suppressed boxes of a kept box are further estimates of the same object, each from a frustum
and a point sample of its own; t3d_detect_fuse (nms.DeviceFuse) writes every kept box with the weighted mean geometry of its cluster
(weights: what ranked, times the IoU with the kept box; headings and the l / w exchange aligned to the kept box first).  Which boxes are
kept, and every score, stay; a kept box without a suppressed box stays byte for byte.  --nms_fuse_iou V (in [T, 1], implies --nms_fuse)
lets only the suppressed boxes above IoU V vote.  Records and --vis_dir legends gain 'votes'.  Without --nms_fuse every output is what
it was, byte for byte.

--soft_nms {gaussian,linear}: Soft-NMS in place of the suppression (t3d_detect_soft_nms, nms.DeviceSoftNms; Bodla et al., ICCV 2017).
Neighbouring true objects overlap in 3-D, so a threshold that removes duplicates removes neighbours; here a box that overlaps a better
one of its image and class keeps its place and its confidence is multiplied by exp(-IoU^2 / sigma) (gaussian; --soft_nms_sigma, default
0.5) or, above --nms_iou T, by 1 - IoU (linear).  The decayed confidence is what the result files' last column, --official_eval and the
14-list carry; in records, legends and --consistency_json rows 'prob' stays the 2-D detector's and 'soft_prob' / 'decays' say what
became of it.  A detection that falls below --soft_nms_min_prob (default 0.001) is dropped like a suppressed one.  It does not go with
--nms_score score, --nms_fuse or --sweep.  Without the flag every output is what it was, byte for byte.

--vis_dir DIR: for each of the first --vis_max scenes (default 50) with at least one detection, DIR/<id>.png -- the camera image with the
kept 3-D boxes in class colours and their 2-D rectangles, beside a bird's-eye panel of the scene's points with the same boxes -- and
DIR/<id>.json, the legend (there is no text in the pictures).  t3d_render (render.py) paints them from the corners where the decode
wrote them and from the device copy of the points the extraction made; only the finished panels come back.  --vis_gt adds the label
boxes in green, --vis_suppressed (with --nms_iou or --soft_nms) the boxes that were dropped in grey.  Nothing else changes with these flags.

--consistency: t3d_detect_consistency (consistency.py) follows every batch's decode and measures, without ground truth, how well each 3-D
box agrees with what it was predicted from: reproj_iou (its reprojection against its 2-D box; the image size, read from the JPEG's
header, clips the reprojection), mask_in_box and seg_box_iou (the segmented points against the points inside the box).  Records,
--vis_dir legends and --consistency_json FILE (one row per detection) carry the numbers.  --min_reproj_iou / --min_mask_in_box /
--min_seg_box_iou (each implies --consistency) reject a detection below the threshold: it is absent from everything this module hands
out, and it is rejected BEFORE --nms_iou runs -- it is listed in no NMS group, so a box the filter rejects cannot suppress a good one.
Without these flags every output is byte for byte what it was.

--tta K (2..8): test-time augmentation (ensemble.py).  Every frustum goes through the network K times: view 0 is the run without the
flag, view v redraws the frustum's points with a seed derived from (--seed, v), and with --tta_flip the odd views are mirrored in the
centre view.  Behind the last decode one t3d_detect_ensemble call brings the mirrored boxes back, measures how far the K boxes of a
detection overlap (view_iou: the mean pairwise IoU under --nms_metric, view_min_iou: the smallest) and writes their weighted mean around
the view that agrees best with the others (weights: exp of a view's score, times its IoU with that anchor view; a view votes above
--tta_vote_iou, default 0).  --nms_iou, --nms_fuse, the records, the result files and --vis_dir then work on the fused boxes.
--min_view_iou A rejects a detection whose view_iou lies below A where the --min_* thresholds reject: before the NMS groups are built,
and counted in the `consistency:` line.  Records, --vis_dir legends and --consistency_json rows gain view_iou, view_min_iou, views_voted
and anchor_view; score, prob and the consistency measures stay those of view 0.  K views cost K passes of the network.  Without --tta
every output is byte for byte what it was.  The views are not swept: --tta does not go with --sweep.

--sweep: which --nms_iou and --min_* to pass.  The pipeline runs once, without thresholds and without suppression (the consistency
measures are taken iff a --sweep_min_* is given); then every combination of the values given -- numbers the flag of that name accepts, or
the word off; an omitted flag is off -- is scored by the official AP of --test_on on the device (sweep.py: t3d_detect_nms_sweep computes
each pair's IoU once for all of them, t3d_sunrgbd_eval_sweep the footprints, ranks and overlaps).  --nms_metric / --nms_score hold for
every combination.  The log: the size of the grid, the baseline (everything off: the AP --official_eval prints for the plain run), the
best --sweep_top rows (default 10) by mean AP with their per-class AP and the detections they keep, and `best: <the flags to pass>`;
--sweep_json FILE takes every row.  No result files, pictures or other reports are written.  Box voting (--nms_fuse) moves the kept
boxes, so its overlaps differ per combination: it is not swept.

--bootstrap R [--bootstrap_seed S] [--bootstrap_level L] [--bootstrap_json FILE] (with --official_eval or --sweep; bootstrap.py): how far
an AP moves when the validation images are redrawn.  R redraws of the image list with replacement are scored on the device
(t3d_sunrgbd_eval_bootstrap: the matching of the point evaluation, a weighted curve per redraw).  --official_eval gains an `AP interval`
line behind every AP line and a `Mean AP interval` line; --sweep gains, on each of the --sweep_top rows, the paired interval of the row's
mean AP minus the baseline's and minus the best row's (the same redraws for every row), a line `indistinguishable from best at 95 %:
rows ...` behind `best:`, and the intervals in --sweep_json (which is where they go: --bootstrap_json is --official_eval's).  Without
--bootstrap every output is what it was, byte for byte.

--rescore MODEL.json [--min_rescore P]: one confidence per detection from its label-free measures (rescore.py: t3d_rescore_features and
t3d_rescore_apply behind the ensemble, in front of the accept rule).  The records, the legends of --vis_dir and the rows of
--consistency_json gain rescore_prob ('prob' stays the 2-D detector's); the suppression ranks by it where it ranks by 'prob', and the
last column of the result files, --official_eval, --diagnose and --bootstrap use it (with --soft_nms: what Soft-NMS leaves of it);
--min_rescore rejects a detection below P as the min_* thresholds do.  It implies --consistency; a model that reads view_iou needs --tta.
--rescore_fit MODEL.json fits such a model (rescore.fit_parts): the pipeline runs once as for --sweep, the classes with ground truth are
evaluated on the device, the images are split by --seed, and the held-out part reports the AP by prob against the AP by rescore_prob.
It does not go with --rescore, --sweep, a suppression or a threshold.  Without these flags every output is what it was, byte for byte.

--floor: the one measure that looks at the whole scene (floor.py).  All evaluated classes stand on the floor, and a frustum seldom shows
the floor under its object: the bottom of a box and its height are guesses of the size head.  Behind every extraction launch
t3d_scene_floor fits the floor plane of each scene to the depth points the launch left on the device -- the lowest peak of a height
histogram (--floor_bin, --floor_range) that holds --floor_min_share of the points, then a plane through the points within --floor_band
of it, taken as level where it would tilt by more than --floor_max_tilt or the floor shows as a strip.  Behind the ensemble of the views
and in front of the rescoring, t3d_detect_floor measures floor_gap, the distance from the bottom of every box down to that plane
(positive: the box floats, negative: it sinks); records, legends and --consistency_json rows gain floor_gap and floor_flags.
--snap_floor shift moves a box onto the floor, --snap_floor stretch moves its bottom face there and keeps its top; a box further than
--snap_floor_max (default 0.3 m) from the floor is left alone.  The suppression, the records, the result files and --vis_dir then work
on the snapped boxes; the consistency measures stay those of the box as decoded.  --max_floor_gap G rejects a detection whose
|floor_gap| -- measured before any snapping -- exceeds G, where the --min_* thresholds reject; a scene without a floor snaps and rejects
nothing.  --floor_json FILE takes one row per scene: its plane, the share of its points on it, their rms distance from it and the
flags.  The floor flags do not go with --sweep or --rescore_fit.  Measured: the synthetic recipe (README).  Not measured: real SUN-RGBD.
Without these flags every output is what it was, byte for byte.

--visibility: the free space of the scene (visibility.py).  Every pixel of a depth image says that the space between the camera and its
return is empty: a box pulled towards the camera has the wall behind it visible through it, a box pushed away has every return in front
of it, a background box in mid-air is seen through entirely.  Behind every extraction launch t3d_scene_range keeps, per cell of
--visibility_cell pixels (default 4), the nearest return of the points the launch left on the device -- a few KB per scene, which stay
when the points go.  Behind the floor stage and in front of the rescoring, t3d_detect_visibility casts a ray through every cell a box
covers and asks where the cell's return lies: in front of the box, inside it (within --visibility_margin, default 0.05 m) or behind it;
a ray that crosses less than --visibility_min_chord (default 0.1 m) of the box counts nowhere.  Records, legends and --consistency_json
rows gain see_through = through / (through + inside), occluded = front / rays, support = inside / rays and visibility_flags.
--max_see_through F rejects a detection whose see_through exceeds F on at least --visibility_min_rays (default 16) rays, where the
--min_* thresholds reject.  The stage moves no box: the kernel's slide along the viewing ray (t3d.h, mode 1) is offered by no flag,
because on clean label boxes it brought back fewer than half of the displaced ones (README).  Every default is an option, not a tuned
value.  The flags do not go with --sweep or --rescore_fit.  Measured: the synthetic recipe (README).  Not
measured: real SUN-RGBD.  Without these flags every output is what it was, byte for byte.

Where things live: the stages behind the decode (views, consistency, the accept rule, NMS, box voting) and their order belong to
semisup_infer.DeviceStages, which `Detector.decode_all` reaches through `inference` and keeps as `Detector.stages` -- its `corners` are the
boxes on the device after every stage that ran, which `Vis.write` draws and `sweep_parts` suppresses.  What rejects a detection is
semisup_infer.TESTS, one entry beside each stage's measure.  semisup_infer.report writes the `consistency:` / `tta:` / `nms` lines, semisup_infer.kept drops the rows that were not kept.  Here: what the host knows of a detection
(`Detection`), the extraction, the requests, the records and reports with the fields every stage adds to them (`FIELD_GROUPS`), and
`main`, which checks its own flags, lets `Detector` check the rest (`STAGE_KEYWORDS`), and turns either's ValueError into an argument
error in one place, before a model is built.
"""
import argparse
import collections
import json
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import bootstrap as BS, consistency as CS, ensemble as EN, floor as FL, nms as NMS, render as RD, rescore as RS, semisup_infer as SI, sunrgbd_data as SD, sweep as SW, test_semisup as TS, visibility as VS      # noqa: E402
from transferable3d_amd.constants import type2class                        # noqa: E402
from transferable3d_amd.dataset import DeviceEvalSource, DeviceFrustumSet   # noqa: E402
from transferable3d_amd.tf_checkpoint import load_state                    # noqa: E402

MIN_POINTS = 5
# what the host knows of a detection: its scene's position in the extraction launch, the image id, the class name, the 2-D box, the confidence
Detection = collections.namedtuple('Detection', 'scene image name box2d prob')


def flags_from_keywords(**kw):
    """test_semisup's FLAGS from keyword arguments: semi_type='F', refine=1, use_one_hot=True, SUNRGBD_SEMI_TEST_CLS=[...], ..."""
    argv = []
    for k, v in kw.items():
        if isinstance(v, bool):
            argv += ['--' + k] if v else []
        elif isinstance(v, (list, tuple)):
            argv += ['--' + k] + [str(x) for x in v]
        elif v is not None:
            argv += ['--' + k, str(v)]
    return TS.build_flags(argv)


class Vis:
    """detect --vis_dir: which scenes are drawn, what is kept of them between the extraction and the decode, and the pictures."""
    SCENES_PER_CALL = 8          # scenes painted by one t3d_render call (two views each)

    def __init__(self, vis_dir, vis_max=50, vis_gt=False, vis_suppressed=False, nms=False):
        if vis_suppressed and not nms:
            raise ValueError('--vis_suppressed shows what --nms_iou / --soft_nms dropped: it needs one of them')
        if int(vis_max) < 0:
            raise ValueError('--vis_max must not be negative')
        self.dir, self.max, self.gt, self.suppressed = vis_dir, int(vis_max), bool(vis_gt), bool(vis_suppressed)
        self.taken = 0
        self.written = []

    def take(self, rt, part, scenes, scene_ids, last_scene):
        """After an extraction launch: keep, for the scenes of this part that have a frustum (so will have a detection), the device
        copy of their points as fp32 upright camera coordinates, until the budget of --vis_max is spent."""
        import torch
        part['vis'] = {}
        if last_scene is None:
            return
        points, offsets = last_scene
        for s in sorted(set(m.scene for m in part['meta'])):
            if self.taken >= self.max:
                break
            p = points[int(offsets[s]):int(offsets[s + 1])]
            xyz = torch.stack([p[:, 0], -p[:, 2], p[:, 1]], 1).to(torch.float32).contiguous()          # upright depth -> upright camera
            rgb = p[:, 3:6].to(torch.float32).contiguous() if p.shape[1] >= 6 else None
            host = SD.flip_axis_to_camera(np.asarray(scenes[s]['points'], np.float64)[:, :3])
            part['vis'][s] = dict(id=scene_ids[s], xyz=xyz, rgb=rgb, ranges=RD.ranges_of(host), Rtilt=scenes[s]['Rtilt'], K=scenes[s]['K'],
                                  image=scenes[s].get('image'), gt=scenes[s].get('gt_corners'), gt_classes=scenes[s].get('gt_classes'))
            self.taken += 1

    def write(self, rt, parts, d, corners):
        """parts as Detector.decode_all took them, d its Decoded (every detection in its place), corners [n, 24] the boxes on the device
        after every stage of that run (Detector.stages.corners: with nms_fuse the fused corners of a kept box and copies of the unfused
        ones for every other, so --vis_suppressed still shows the raw boxes).  -> the scene ids written."""
        os.makedirs(self.dir, exist_ok=True)
        todo, i = [], 0
        for p in parts:
            rows = {}
            for m in p['meta']:
                rows.setdefault(m.scene, []).append((i, m))
                i += 1
            for s, rec in sorted(p.get('vis', {}).items()):
                rec['rows'] = rows.get(s, [])
                if any(d.keep is None or d.keep[r] for r, _ in rec['rows']):
                    todo.append(rec)
        ren = RD.Renderer(rt)
        k3 = corners.view(-1, 8, 3)
        for lo in range(0, len(todo), self.SCENES_PER_CALL):
            batch = todo[lo:lo + self.SCENES_PER_CALL]
            views, legends = [], []
            for rec in batch:
                v, legend = self.views_of(rec, d, k3)
                views += v
                legends.append(legend)
            panels = ren.render(views)
            for k, (rec, legend) in enumerate(zip(batch, legends)):
                RD.write_png(os.path.join(self.dir, '%06d.png' % rec['id']), RD.side_by_side(panels[2 * k:2 * k + 2]))
                with open(os.path.join(self.dir, '%06d.json' % rec['id']), 'w') as fh:
                    json.dump(legend, fh, indent=1)
                self.written.append(rec['id'])
        for p in parts:
            p.pop('vis', None)
        return self.written

    def views_of(self, rec, d, k3):
        """-> ([image view, bird's-eye view], legend) of one scene."""
        K = np.asarray(rec['K'], np.float64).reshape(3, 3)
        image = rec['image']
        H, W = image.shape[:2] if image is not None else (int(2 * K[1, 2] + 0.5), int(2 * K[0, 2] + 0.5))
        cam = RD.image_view(rec['Rtilt'], K, H, W, image=image)
        xr, yr, zr = rec['ranges']
        bev = RD.bev_view(xr, zr, H, H, y_top=yr[0], bg_colour=RD._rgb(20, 20, 24))
        if image is None:
            cam.points(rec['xyz'], rgb=rec['rgb'])
        bev.points(rec['xyz'], rgb=rec['rgb'])
        legend = {'scene': int(rec['id']), 'panels': {'image': [int(H), int(W)], 'bev': [int(H), int(H)]}, 'boxes': []}
        byte = lambda c: [int(v * 255.0 + 0.5) for v in c]
        if self.gt and rec['gt'] is not None and len(rec['gt']):
            gt = np.asarray(rec['gt'], np.float32).reshape(-1, 8, 3)
            for v in (cam, bev):
                v.boxes(gt, RD.GT_COLOUR, thickness=1)
            names = rec['gt_classes'] or [None] * len(gt)
            legend['boxes'] += [{'kind': 'gt', 'class': n, 'colour': byte(RD.GT_COLOUR)} for n in names]
        rows = rec['rows']
        local = {r: j for j, (r, _) in enumerate(rows)}
        kept = [(r, m) for r, m in rows if d.keep is None or d.keep[r]]
        dropped = [(r, m) for r, m in rows if not (d.keep is None or d.keep[r])] if self.suppressed else []
        for group, kind in ((dropped, 'suppressed'), (kept, 'kept')):              # the kept boxes lie over the suppressed ones
            if not group:
                continue
            colours = [RD.SUPPRESSED_COLOUR if kind == 'suppressed' else RD.class_colour(m.name) for _, m in group]
            for v in (cam, bev):
                v.boxes(k3, colours, thickness=1 if kind == 'suppressed' else 2, index=[r for r, _ in group])
            cam.rects([m.box2d for _, m in group], colours, thickness=1)
            for (r, m), c in zip(group, colours):
                entry = {'kind': kind, 'detection': local[r], 'class': m.name, 'prob': float(m.prob), 'score': float(d.score[r]),
                         'box2d': [float(x) for x in m.box2d], 'colour': byte(c), 'kept': kind == 'kept'}
                if kind == 'suppressed':
                    entry['suppressed_by'] = local.get(int(d.suppressed_by[r]), None)
                entry.update(fields_of(d, r, RECORD_GROUPS, as_lists=True))
                if d.accept is not None and not d.accept[r]:
                    entry['kind'] = 'rejected'
                legend['boxes'].append(entry)
        return [cam, bev], legend


def consistency_fields(d, i, as_lists=False):
    """What a record (or a legend / JSON entry: as_lists) says of detection i's consistency measures."""
    rect = d.reproj_rect[i]
    return {'reproj_iou': float(d.reproj_iou[i]), 'reproj_rect': [float(v) for v in rect] if as_lists else rect,
            'mask_in_box': float(d.mask_in_box[i]), 'seg_box_iou': float(d.seg_box_iou[i]), 'flags': int(d.flags[i])}


def soft_fields(d, i, as_lists=False):
    """What a record (or a legend / JSON entry) says of what Soft-NMS left of detection i's confidence ('prob' stays the 2-D detector's)."""
    return {'soft_prob': float(d.soft_prob[i]), 'decays': int(d.n_decays[i])}


def view_fields(d, i, as_lists=False):
    """What a record (or a legend / JSON entry) says of how detection i's views agreed (detect --tta)."""
    return {'view_iou': float(d.view_iou[i]), 'view_min_iou': float(d.view_min_iou[i]), 'views_voted': int(d.n_views_voted[i]),
            'anchor_view': int(d.anchor_view[i])}


def visibility_fields(d, i, as_lists=False):
    """What a record (or a legend / JSON entry) says of how detection i stands in the free space of its scene (detect --visibility)."""
    return {'see_through': float(d.see_through[i]), 'occluded': float(d.occluded[i]), 'support': float(d.support[i]),
            'visibility_flags': int(d.visibility_flags[i])}


# The optional fields of a detection, one group per stage that adds some: the Decoded attribute that says the stage ran, and the fields
# it contributes to a record (as_lists: to a legend entry or a JSON row).  A writer names the groups it carries, in its own order.
FIELD_GROUPS = {
    'votes': ('n_votes', lambda d, i, as_lists=False: {'votes': int(d.n_votes[i])}),
    'rescore': ('rescore_prob', lambda d, i, as_lists=False: {'rescore_prob': float(d.rescore_prob[i])}),
    'soft': ('soft_prob', soft_fields),
    'views': ('view_iou', view_fields),
    'consistency': ('reproj_iou', consistency_fields),
    'floor': ('floor_gap', lambda d, i, as_lists=False: {'floor_gap': float(d.floor_gap[i]), 'floor_flags': int(d.floor_flags[i])}),
    'visibility': ('see_through', visibility_fields),
}
RECORD_GROUPS = ('votes', 'rescore', 'soft', 'views', 'consistency', 'visibility', 'floor')     # the records of `Detector.detect` and the legends of --vis_dir
ROW_GROUPS = ('consistency', 'rescore', 'soft', 'views', 'visibility', 'floor')              # the rows of --consistency_json
# the options of the stages as `Detector` takes them, under the names of the flags (the module docstring describes them)
SCENE_FLAGS = FL.FLAGS + ('floor_json',) + VS.FLAGS          # the flags of the stages that look at the whole scene: not for --sweep or --rescore_fit
STAGE_KEYWORDS = ('nms_iou', 'nms_metric', 'nms_score', 'nms_fuse', 'nms_fuse_iou', 'soft_nms', 'soft_nms_sigma', 'soft_nms_min_prob', 'consistency',
                  'min_reproj_iou', 'min_mask_in_box', 'min_seg_box_iou', 'tta', 'tta_flip', 'tta_vote_iou', 'min_view_iou', 'rescore', 'min_rescore') + FL.FLAGS + VS.FLAGS


def scene_rows(parts):
    """-> (per detection of `parts`, in order, the row of its scene among the scenes of all parts; the number of those rows).  A part's
    meta names its scenes by their position in the part; every part has one row per scene, with or without a frustum.  The consistency,
    floor and visibility requests all index their per-scene tables by it."""
    index, n_rows = [], 0
    for p in parts:
        index += [n_rows + m.scene for m in p['meta']]
        n_rows += p['n_scenes']
    return index, n_rows


def fields_of(d, i, groups, as_lists=False):
    """The fields the stages that ran (Decoded `d`) add for detection i, of the groups named, in that order."""
    out = {}
    for present, fields in (FIELD_GROUPS[g] for g in groups):
        if getattr(d, present) is not None:
            out.update(fields(d, i, as_lists))
    return out


class Detector:
    """The test_semisup inference graph, built once; `detect` runs scenes through it.  `stages`: the semisup_infer.DeviceStages of the
    last `decode_all` (None where it had no detection)."""
    stages = None

    def __init__(self, FLAGS=None, model_path=None, boxpc_model_path=None, rt=None, type_whitelist=SD.TYPE_WHITELIST,
                 num_points=SD.NUM_POINTS, nms_iou=None, nms_metric=None, nms_score=None, log=None, consistency=False,
                 min_reproj_iou=None, min_mask_in_box=None, min_seg_box_iou=None, nms_fuse=False, nms_fuse_iou=None, tta=None, tta_flip=False,
                 tta_vote_iou=None, min_view_iou=None, soft_nms=None, soft_nms_sigma=None, soft_nms_min_prob=None, rescore=None, min_rescore=None,
                 floor=False, snap_floor=None, snap_floor_max=None, max_floor_gap=None, floor_bin=None, floor_range=None, floor_min_share=None,
                 floor_band=None, floor_max_tilt=None, visibility=False, visibility_cell=None, visibility_margin=None, visibility_min_chord=None,
                 max_see_through=None, visibility_min_rays=None, **keywords):
        """FLAGS: test_semisup.build_flags(...), or keyword arguments of the same names.  model_path / boxpc_model_path: state dicts
        (.npz) or TensorFlow checkpoint prefixes (default: FLAGS'; neither: the graph's initial weights).  num_points: the cap of a
        frustum's points at extraction (the frustum files': 2048); the network draws FLAGS.num_point of them per batch.  log: a
        function that takes the lines a run says of its stages (semisup_infer.report).
        The options of the stages (STAGE_KEYWORDS) carry the names, the values and the defaults of the flags the module docstring
        describes, None or False where a flag is not given; consistency: measure every detection (a threshold and rescore imply it);
        rescore: a rescore.Model or the path of one.  They are checked here, before a model is built, and kept under their names:
        nms_iou, nms_metric, nms_score, nms_fuse, nms_fuse_iou and soft_nms (its nms.SoftOptions) as `suppression` (nms.Suppression)
        holds them -- with soft_nms, nms_iou is None -- thresholds, consistency, tta, tta_flip, tta_vote_iou, min_view_iou, rescore (the
        Model), min_rescore, `floor` (floor.Floor: on, snap, snap_max, max_floor_gap and the estimator's FloorOptions) and `visibility`
        (visibility.Visibility: on, max_see_through and the kernels' VisibilityOptions)."""
        self.floor = FL.check_options(floor, snap_floor, snap_floor_max, max_floor_gap, floor_bin, floor_range, floor_min_share, floor_band, floor_max_tilt)
        self.visibility = VS.check_options(visibility, visibility_cell, visibility_margin, visibility_min_chord, max_see_through, visibility_min_rays)
        self.min_rescore = RS.check_min_rescore(min_rescore)
        if self.min_rescore is not None and rescore is None:
            raise ValueError('--min_rescore rejects by the rescored confidence: it needs --rescore')
        self.rescore = None if rescore is None else RS.Model.of(rescore)
        self.tta, self.tta_flip, self.tta_vote_iou, self.min_view_iou = EN.check_options(tta, tta_flip, tta_vote_iou, min_view_iou)
        self.suppression = NMS.suppression(soft_nms, soft_nms_sigma, soft_nms_min_prob, nms_iou, nms_metric, nms_score, nms_fuse, nms_fuse_iou)
        self.nms_iou, self.nms_metric, self.nms_score, self.nms_fuse, self.nms_fuse_iou, self.soft_nms = self.suppression
        self.thresholds = CS.check_thresholds(min_reproj_iou, min_mask_in_box, min_seg_box_iou)
        self.min_reproj_iou, self.min_mask_in_box, self.min_seg_box_iou = self.thresholds
        self.consistency = bool(consistency) or any(t is not None for t in self.thresholds) or self.rescore is not None
        if self.rescore is not None and 'view_iou' in self.rescore.features and self.tta is None:
            raise ValueError('the rescoring model reads view_iou, the agreement of the augmented views: it needs --tta')
        self.log = log
        self.FLAGS = FLAGS = FLAGS if FLAGS is not None else flags_from_keywords(**keywords)
        model_path = model_path or FLAGS.model_path
        boxpc_model_path = boxpc_model_path or FLAGS.boxpc_model_path
        sd = load_state(model_path) if model_path else None
        if boxpc_model_path:
            sd = dict(sd or {})
            sd.update({'D_boxpc_branch/' + k: v for k, v in load_state(boxpc_model_path).items()})
        self.B = FLAGS.batch_size
        self.sess, self.ops = TS.get_model(FLAGS, self.B, FLAGS.num_point, FLAGS.NUM_CHANNELS, rt=rt, state_dict=sd)
        self.rt = self.ops['graph'].rt
        self.extractor = SD.FrustumExtractor(self.rt, num_points, FLAGS.seed)
        self.floor_estimator = FL.DeviceFloor(self.rt, self.floor.options) if self.floor.on else None
        self.range_builder = VS.DeviceRange(self.rt, self.visibility.options) if self.visibility.on else None
        self.whitelist = list(type_whitelist)
        self.classes = list(FLAGS.SUNRGBD_SEMI_TEST_CLS) or None

    def extract(self, scenes, detections, scene_ids=None, vis=None):
        """One t3d_frustum_extract launch over `scenes`; -> a part for `decode` (device tensors + what the host knows of the kept jobs).
        vis (Vis): the scenes it will draw keep their points on the device.  With the floor stage, t3d_scene_floor follows the launch on
        the points it left there: part['floor'] = the planes and counts of the part's scenes on the device, the counts on the host, the ids.
        With the visibility stage, t3d_scene_range follows it alike: part['range'] = the range maps of the part's scenes on the device and,
        on the host, their grids, calibration rows and counts (visibility.DeviceRange.build)."""
        scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
        jobs, meta = [], []
        for s, dets in enumerate(detections):
            for o, (name, box2d, prob) in enumerate(dets):          # the ordinal counts every detection of the image (sunrgbd_data)
                if name not in self.whitelist or (self.classes is not None and name not in self.classes):
                    continue
                jobs.append({'scene': s, 'box2d': np.asarray(box2d, np.float64), 'box3d': None, 'key': (scene_ids[s], o, 0), 'choice': None})
                meta.append(Detection(s, scene_ids[s], name, np.asarray(box2d, np.float64), float(prob)))
        want_scene = vis is not None and vis.taken < vis.max
        out = self.extractor.run(scenes, jobs, on_device=True, keep_scene=want_scene or self.floor.on or self.visibility.on)
        calib = [CS.calib_row(sc['Rtilt'], sc['K'], sc.get('image_wh')) for sc in scenes] if self.consistency else []
        if out is None:
            return dict(out=None, keep=[], counts=[], meta=[], n_scenes=len(scenes), calib=calib)
        counts = out['count'].cpu().numpy()                          # the one copy back of this launch
        keep = np.nonzero(counts >= MIN_POINTS)[0]
        part = dict(out=out, keep=keep, counts=counts[keep], meta=[meta[j] for j in keep], n_scenes=len(scenes), calib=calib)
        if self.floor.on:
            plane, floor_counts, floor_counts_host = self.floor_estimator.estimate(*self.extractor.last_scene)
            part['floor'] = dict(plane=plane, counts=floor_counts, counts_host=floor_counts_host, ids=scene_ids)
        if self.visibility.on:
            part['range'] = self.range_builder.build(*self.extractor.last_scene, scenes)
        if want_scene:
            vis.take(self.rt, part, scenes, scene_ids, self.extractor.last_scene)
        self.extractor.last_scene = None          # (the points go unless Vis took what it draws)
        return part

    def decode(self, parts):
        """The network and t3d_detect_decode over the frustums of `parts` (in order) -> (meta, semisup_infer.Decoded); with nms_iou, of
        the detections t3d_detect_nms kept."""
        meta, d = self.decode_all(parts)
        d, meta = SI.kept(d, meta)
        return meta, d

    def decode_all(self, parts):
        """`decode` with every detection in its place: the records say which ones t3d_detect_nms kept (Decoded.keep; None without nms_iou).
        With thresholds, Decoded.accept says which ones passed them, and Decoded.keep is False for the others too.  `self.stages` holds
        the run's semisup_infer.DeviceStages (None without a detection): its `corners` [n, 24] are the boxes on the device after every
        stage that ran (what `Vis.write` draws and `sweep_parts` suppresses), its `score` [n] the decoded scores."""
        FLAGS = self.FLAGS
        meta = [m for p in parts for m in p['meta']]
        self.stages = None
        if not meta:
            return meta, None
        live = [p for p in parts if len(p['keep'])]
        classes = [type2class[m.name] for m in meta]
        ds = DeviceFrustumSet.from_device(self.rt, [p['out'] for p in live], [p['keep'] for p in live], [p['counts'] for p in live], classes)
        source = DeviceEvalSource(self.ops['graph'], dataset=ds, seed=FLAGS.seed)
        nms = con = views = rescore = floor = visibility = None
        if self.visibility.on:
            visibility = VS.VisibilityRequest(*self.visibility_rows(parts), options=self.visibility.options,
                                              max_see_through=self.visibility.max_see_through)
        if self.rescore is not None:
            rescore = RS.RescoreRequest(self.rescore, [m.prob for m in meta], self.min_rescore)
        if self.suppression.on:
            nms = SI.NmsRequest.of(self.suppression, [m.image for m in meta], classes, [m.prob for m in meta])
        if self.consistency:
            con = SI.ConsistencyRequest([m.box2d for m in meta], [row for p in parts for row in p.get('calib', [])], scene_rows(parts)[0], *self.thresholds)
        if self.floor.on:
            floor = FL.FloorRequest(*self.floor_rows(parts), snap=self.floor.snap, snap_max=self.floor.snap_max, max_floor_gap=self.floor.max_floor_gap)
        if self.tta is not None:
            views = EN.EnsembleRequest(EN.views_of(self.tta, self.tta_flip, FLAGS.seed), self.nms_metric, self.tta_vote_iou, self.min_view_iou)
        res = SI.inference(self.sess, self.ops, None, None, self.B, prefix=FLAGS.pred_prefix, use_boxpc_fit_prob=FLAGS.use_boxpc_fit_prob,
                           source=source, n_batches=(ds.F + self.B - 1) // self.B, decode='device', want_seg=False, nms=nms, consistency=con,
                           views=views, rescore=rescore, floor=floor, visibility=visibility)
        self.stages = res.device
        d = res.decoded[slice(0, ds.F)]
        if self.log:
            SI.report(self.log, res.device, d)
        if d.accept is not None and not d.accept.all():          # a rejected detection is dropped wherever a suppressed one is
            d.keep = d.accept.copy() if d.keep is None else d.keep & d.accept
        return meta, d

    def floor_rows(self, parts):
        """The planes [S, 8] and counts [S, 4] of the parts' scenes on the device (a part without a frustum was not estimated: its scenes
        have no floor) and per detection the row of its scene (`scene_rows`)."""
        import torch
        planes, counts = [], []
        for p in parts:
            if p.get('floor') is not None:
                planes.append(p['floor']['plane'])
                counts.append(p['floor']['counts'])
            else:
                planes.append(torch.zeros(p['n_scenes'], 8, dtype=torch.float64, device=self.rt.device))
                counts.append(torch.tensor([[0, 0, -1, FL.NONE]] * p['n_scenes'], dtype=torch.int32, device=self.rt.device).view(-1, 4))
        return torch.cat(planes), torch.cat(counts), scene_rows(parts)[0]

    def visibility_rows(self, parts):
        """The calibration rows [S, 20], grids (dims [S, 2], offsets [S + 1]) and range maps (one int32 tensor on the device) of the parts'
        scenes (a part without a frustum built no map: its scenes have a grid of no cells and so no scene) and per detection the row of
        its scene (`scene_rows`)."""
        import torch
        calib, dims, maps = [], [], []
        for p in parts:
            if p.get('range') is not None:
                calib.append(p['range']['calib'])
                dims.append(p['range']['dims'])
                maps.append(p['range']['range'])
            else:
                calib.append(np.zeros((p['n_scenes'], 20)))
                dims.append(np.zeros((p['n_scenes'], 2), np.int32))
        dims = np.concatenate(dims).reshape(-1, 2)
        offsets = np.concatenate([[0], np.cumsum(dims[:, 0].astype(np.int64) * dims[:, 1])]).astype(np.int64)
        range_ = torch.cat(maps) if maps else torch.zeros(0, dtype=torch.int32, device=self.rt.device)
        return np.concatenate(calib).reshape(-1, 20), dims, offsets, range_, scene_rows(parts)[0]

    def floor_json_rows(self, parts):
        """--floor_json: one row per estimated scene of `parts` (floor.scene_rows)."""
        rows = []
        for p in parts:
            if p.get('floor') is not None:
                rows += FL.scene_rows(p['floor']['ids'], p['floor']['plane'].cpu().numpy(), p['floor']['counts_host'])
        return rows

    def detect(self, scenes, detections, scene_ids=None, batch_scenes=16, vis_dir=None, vis_max=50, vis_gt=False, vis_suppressed=False):
        """scenes: [{'points' (n, C) fp64 upright depth, 'Rtilt', 'K'}] (FrustumExtractor.run); detections[s]: [(class name, box2d
        (xmin, ymin, xmax, ymax), prob)] of scene s.  -> per scene, a list of {'class', 'box2d', 'prob', 'score', 'label' (7,) = (h, w, l,
        tx, ty, tz, ry), 'corners' (8, 3)} in detection order; a detection whose frustum holds fewer than 5 points, or whose class is
        not whitelisted (or not among FLAGS.SUNRGBD_SEMI_TEST_CLS), or which t3d_detect_nms suppressed, has no entry.  (With nms_iou,
        scenes that share a scene id share their groups: give distinct ids.)
        vis_dir: write <id>.png / <id>.json of the first vis_max scenes with a detection there (module docstring); a scene may carry
        'image' (uint8 [H,W,3], RGB) for the camera panel, and 'gt_corners' [g,8,3] (upright camera) / 'gt_classes' for vis_gt.  The
        records do not depend on it.
        A stage that ran adds its fields to the records (FIELD_GROUPS, in the order of RECORD_GROUPS; the module docstring says what they
        mean): nms_fuse 'votes', the number of suppressed boxes that voted (0: the box is what the decode wrote); rescore
        'rescore_prob'; soft_nms 'soft_prob' and 'decays'; tta 'view_iou', 'view_min_iou', 'views_voted' and 'anchor_view'; consistency
        'reproj_iou', 'reproj_rect' (4,), 'mask_in_box', 'seg_box_iou' and 'flags'; visibility 'see_through', 'occluded', 'support' and 'visibility_flags'; floor 'floor_gap' and
        'floor_flags'.  'prob' stays the 2-D detector's.  'label' and
        'corners' are the box after every stage that ran: what t3d_detect_ensemble made of the views, snap_floor of that, and nms_fuse of that; 'score'
        and the consistency measures stay those of view 0's unfused box.  A detection that a threshold rejected, or whose confidence
        Soft-NMS took below soft_nms_min_prob, has no entry.  With consistency a scene may carry 'image_wh' = (W, H), to which the
        reprojected rectangle is then clipped (without it: no clipping)."""
        vis = None if vis_dir is None else Vis(vis_dir, vis_max, vis_gt, vis_suppressed, nms=self.suppression.on)
        if len(scenes) != len(detections):
            raise ValueError('%d scenes, detections of %d' % (len(scenes), len(detections)))
        scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
        parts, first = [], []
        for lo in range(0, len(scenes), batch_scenes):
            hi = min(lo + batch_scenes, len(scenes))
            parts.append(self.extract(scenes[lo:hi], detections[lo:hi], scene_ids[lo:hi], vis=vis))
            first.append(lo)
        meta, d = self.decode_all(parts)
        out = [[] for _ in scenes]
        if d is None:
            return out
        if vis is not None:
            vis.write(self.rt, parts, d, self.stages.corners)
        i = 0
        for lo, p in zip(first, parts):
            for m in p['meta']:
                if d.keep is None or d.keep[i]:
                    out[lo + m.scene].append(self.record(m.name, m.box2d, m.prob, d, i))
                i += 1
        return out

    def sweep(self, scenes, detections, grid, dataset_dir, idx_list, test_on='AB', scene_ids=None, batch_scenes=16, threshold=0.25,
              bootstrap=None, top=10):
        """Which thresholds to use: the scenes go through the pipeline once, as in `detect`, and every configuration of `grid`
        (sweep.Grid) is scored by the official AP of the class set `test_on` against the label files of dataset_dir for the images
        idx_list (ids, or the path of an index file) -> sweep.Result.  The detector must have been built without nms_iou and without
        thresholds, and with consistency=True when the grid sweeps a min_* threshold.
        bootstrap: None, the number of replicates, or {'R', 'seed', 'level'}: the `top` best rows gain the paired bootstrap intervals of
        their mean AP against the baseline row and against the best row (sweep.Result.bootstrap_rows)."""
        if len(scenes) != len(detections):
            raise ValueError('%d scenes, detections of %d' % (len(scenes), len(detections)))
        scene_ids = list(range(len(scenes))) if scene_ids is None else list(scene_ids)
        parts = [self.extract(scenes[lo:lo + batch_scenes], detections[lo:lo + batch_scenes], scene_ids[lo:lo + batch_scenes])
                 for lo in range(0, len(scenes), batch_scenes)]
        return self.sweep_parts(parts, grid, dataset_dir, idx_list, test_on, threshold, bootstrap, top)

    def sweep_parts(self, parts, grid, dataset_dir, idx_list, test_on='AB', threshold=0.25, bootstrap=None, top=10):
        """`sweep` on extracted parts (what `main` holds)."""
        from transferable3d_amd import evaluate_sunrgbd as ES
        import torch
        if self.suppression.on or any(t is not None for t in self.thresholds):
            raise ValueError('a sweep starts from the plain run: the detector has nms_iou, soft_nms or a min_* threshold')
        if self.tta is not None:
            raise ValueError('the views of tta are not swept: the detector has tta')
        if self.rescore is not None:
            raise ValueError('a sweep starts from the plain run: the detector has a rescoring model')
        if self.floor.on:
            raise ValueError('a sweep starts from the plain run: the detector has the floor stage')
        if self.visibility.on:
            raise ValueError('a sweep starts from the plain run: the detector has the visibility stage')
        if grid.consistency and not self.consistency:
            raise ValueError('the grid sweeps a min_* threshold: the detector needs consistency=True')
        meta, d = self.decode_all(parts)
        if d is None:
            raise ValueError('no detections to sweep')
        n, names = len(meta), [m.name for m in meta]
        if grid.score == 'prob':
            score = torch.from_numpy(np.asarray([m.prob for m in meta], np.float32)).to(self.rt.device)
        else:
            score = self.stages.score[:n]
        held = ES.official_predictions(sorted(set(ES.CLASS_NAMES[test_on]) | set(names)), self.predictions(meta, d), names)
        det_index = {c: np.nonzero(np.asarray([x == c for x in names], bool))[0].astype(np.int32) for c in ES.CLASS_NAMES[test_on]}
        measures = {k: getattr(d, k) for k in CS.MEASURES} if grid.consistency else None
        return SW.run(self.rt, grid, self.stages.corners[:n], score, [m.image for m in meta], [type2class[m.name] for m in meta], measures, held,
                      det_index, dataset_dir, idx_list, test_on, threshold,
                      bootstrap=({'R': int(bootstrap)} if bootstrap is not None and not isinstance(bootstrap, dict) else bootstrap), top=top)

    @staticmethod
    def record(name, box2d, prob, d, i):
        r = {'class': name, 'box2d': box2d, 'prob': prob, 'score': float(d.score[i]), 'label': d.label[i], 'corners': d.corners[i]}
        r.update(fields_of(d, i, RECORD_GROUPS))
        return r

    def predictions(self, meta, d):
        """test_semisup's 14-list of a detection run (the entries it fills for --from_rgb_detection; the rotation angles stayed on the
        device, the label rows carry them) with the decoded records attached.  Its confidence entry -- what the result files write and
        the evaluation ranks by -- is semisup_infer.Decoded.confidence."""
        n = len(meta)
        if d is None:
            return SI.Predictions([None, None, [], [], [], [], [], [], [], [], [], [], [], None])
        p = SI.Predictions([None, None, [None] * n, list(d.center), list(d.heading_cls), list(d.heading_res), list(d.size_cls),
                            list(d.size_res), [None] * n, d.confidence([m.prob for m in meta]), [type2class[m.name] for m in meta], [m.image for m in meta], [m.box2d for m in meta], None])
        p.decoded = d
        return p


def scene_pictures(dataset, idx, with_gt, type_whitelist):
    """What --vis_dir reads of a scene besides its points: the image (RGB) and, for --vis_gt, the label boxes."""
    out = {'image': np.ascontiguousarray(dataset.get_image(idx)[:, :, ::-1])}
    if with_gt:
        objs = [o for o in dataset.get_label_objects(idx) if o.classname in type_whitelist]
        out['gt_corners'] = np.stack([SD.compute_box_3d(o) for o in objs]) if objs else np.zeros((0, 8, 3))
        out['gt_classes'] = [o.classname for o in objs]
    return out


def write_consistency_json(path, meta, d):
    """One row per detection of a run, in detection order, the rejected and the suppressed ones included."""
    rows = []
    for i, m in enumerate(meta):
        row = {'image': int(m.image), 'class': m.name, 'box2d': [float(v) for v in m.box2d], 'prob': float(m.prob), 'score': float(d.score[i]),
               'n_mask': int(d.n_mask[i]), 'n_box': int(d.n_box[i]), 'n_both': int(d.n_both[i]), 'accepted': bool(d.accept[i]),
               'kept': bool(d.keep is None or d.keep[i])}
        row.update(fields_of(d, i, ROW_GROUPS, as_lists=True))
        rows.append(row)
    with open(path, 'w') as fh:
        json.dump(rows, fh, indent=1)


def parser():
    p = argparse.ArgumentParser(description='3-D detections from SUN-RGBD scenes and 2-D detections, on the device', allow_abbrev=False)
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (<dir>/training/{image,calib,depth,label_dimension})')
    p.add_argument('--idx_path', required=True, help='index file of the images to run, e.g. mysunrgbd/training/val_data_idx.txt')
    p.add_argument('--rgb_detection_path', required=True, help='folder of 2-D detection files (sunrgbd_data --rgb_detection_path)')
    p.add_argument('--type_whitelist', nargs='+', default=list(SD.TYPE_WHITELIST), help='classes of detections to take')
    p.add_argument('--official_eval', action='store_true', help='print the lines of script_3Deval.m for the detections (evaluate_sunrgbd)')
    p.add_argument('--test_on', default='AB', choices=['A', 'B', 'AB'], help='set of classes --official_eval scores')
    from transferable3d_amd.evaluate_sunrgbd import add_diagnose_arguments
    add_diagnose_arguments(p)                 # with --official_eval: the kinds of errors behind every AP (evaluate_sunrgbd --diagnose)
    NMS.add_arguments(p)
    p.add_argument('--vis_dir', default=None, help='write <id>.png (camera image + bird\'s-eye panel with the 3-D boxes) and <id>.json (legend) of detected scenes here')
    p.add_argument('--vis_max', type=int, default=50, help='how many scenes --vis_dir draws (the first ones with a detection)')
    p.add_argument('--vis_gt', action='store_true', help='--vis_dir: add the label boxes of label_dimension in green')
    p.add_argument('--vis_suppressed', action='store_true', help='--vis_dir: add the boxes --nms_iou (or --soft_nms) dropped, in grey')
    CS.add_arguments(p)
    p.add_argument('--consistency_json', default=None, help='write one row per detection (rejected ones included) with its consistency measures here')
    EN.add_arguments(p)
    SW.add_arguments(p)
    BS.add_arguments(p)                       # with --official_eval or --sweep: intervals behind the APs (bootstrap.py)
    RS.add_arguments(p)
    RS.add_fit_arguments(p)
    FL.add_arguments(p)
    p.add_argument('--floor_json', default=None, help='write one row per scene with its floor plane, the share of its points on it, their rms and the flags here')
    VS.add_arguments(p)
    return p


def sweep_options(args):
    """The sweep.Grid of parsed flags (None without --sweep); ValueError where they contradict."""
    given = [f for f in SW.FLAGS if getattr(args, 'sweep_' + f) is not None]
    if not args.sweep:
        if given or args.sweep_json is not None or args.sweep_top is not None:
            raise ValueError('--sweep_* flags need --sweep')
        return None
    single = [f for f in SW.FLAGS if getattr(args, f) is not None] + [f for f in ('nms_fuse', 'diagnose') if getattr(args, f)]
    single += ['nms_fuse_iou'] if args.nms_fuse_iou is not None else []
    single += ['soft_nms'] if args.soft_nms is not None else []      # (the scores differ per configuration: ranks cannot be shared)
    single += [f for f in EN.FLAGS if getattr(args, f) not in (None, False)]
    single += [f for f in ('rescore', 'min_rescore', 'rescore_fit') if getattr(args, f) is not None]
    single += [f for f in SCENE_FLAGS if getattr(args, f) not in (None, False)]
    if single:
        raise ValueError('--sweep starts from the plain run and chooses the thresholds itself: it does not go with %s' % ' '.join('--' + f for f in single))
    if args.vis_dir or args.consistency_json:
        raise ValueError('--sweep writes no pictures and no per-detection report: it does not go with --vis_dir / --consistency_json')
    if args.sweep_top is not None and args.sweep_top < 0:
        raise ValueError('--sweep_top must not be negative')
    return SW.Grid.from_args(args)


def scene_batches(dataset, ids, batch_scenes=16, workers=8, image_wh=None, pictures=None, also=None):
    """The scenes `ids` of a sunrgbd_object as `Detector.extract` takes them, loaded by `workers` threads one batch ahead -> per batch,
    (its ids, [{'points', 'Rtilt', 'K'}]).  image_wh: None, or a function from the path of a scene's JPEG to its (W, H) (None: unknown)
    for the scenes' 'image_wh'; pictures: None, or a function from a scene's id to what --vis_dir reads of it (`scene_pictures`; {} once
    enough are drawn), asked as the batch is handed out; also: None, or a function of the id that is called where the scene is loaded."""
    def load(idx):
        if also is not None:
            also(idx)
        return dataset.get_calibration(idx), dataset.get_depth(idx)

    for batch in SD._scenes_in_batches(load, ids, batch_scenes, workers):
        scenes = []
        for idx, (calib, depth) in batch:
            scene = {'points': depth, 'Rtilt': calib.Rtilt, 'K': calib.K}
            wh = None if image_wh is None else image_wh(dataset._path('image', idx, 'jpg'))
            if wh is not None:
                scene['image_wh'] = wh
            if pictures is not None:
                scene.update(pictures(idx))
            scenes.append(scene)
        yield [idx for idx, _ in batch], scenes


def main(argv=None, rt=None, log=print):
    """Every flag this parser does not know is test_semisup's (--seed serves the extraction and the network alike)."""
    from transferable3d_amd import evaluate_sunrgbd as ES
    p = parser()
    args, rest = p.parse_known_args(argv)
    FLAGS = TS.build_flags(list(rest))
    try:                                         # (Detector checks its options before it builds a model)
        grid = sweep_options(args)
        diagnose = ES.diagnose_options(p, args)
        if diagnose is not None and not args.official_eval:
            raise ValueError('--diagnose breaks down the score of --official_eval: it needs --official_eval')
        bootstrap = BS.options(p, args)
        if bootstrap is not None and not (args.official_eval or grid is not None):
            raise ValueError('--bootstrap puts intervals behind the APs of --official_eval or --sweep: it needs one of them')
        if bootstrap is not None and grid is not None and bootstrap['json']:
            raise ValueError('--sweep writes its intervals to --sweep_json: it does not go with --bootstrap_json')
        fit = RS.fit_options(args)
        if args.min_rescore is not None and args.rescore is None:                # (Detector's own check would come behind the ones below)
            raise ValueError('--min_rescore rejects by the rescored confidence: it needs --rescore')
        # (of the features to fit: Detector checks the ones a model of --rescore reads)
        if fit is not None and fit['features'] is not None and 'view_iou' in fit['features'] and args.tta is None:
            raise ValueError('the feature view_iou is the agreement of the augmented views: it needs --tta')
        if fit is not None:
            other = [f for f in SW.FLAGS if getattr(args, f) is not None] + [f for f in ('nms_fuse', 'official_eval') if getattr(args, f)]
            other += [f for f in ('nms_fuse_iou', 'soft_nms', 'min_view_iou', 'vis_dir', 'consistency_json') if getattr(args, f) is not None]
            other += [f for f in SCENE_FLAGS if getattr(args, f) not in (None, False)]
            if other:
                raise ValueError('--rescore_fit starts from the plain run, as --sweep does: it does not go with %s' % ' '.join('--' + f for f in other))
        floor = FL.check_options(**{k: getattr(args, k) for k in FL.FLAGS})
        if args.floor_json and not floor.on:
            raise ValueError('--floor_json writes the floor planes: it needs --floor, --snap_floor or --max_floor_gap')
        visibility = VS.check_options(**{k: getattr(args, k) for k in VS.FLAGS})
        if (args.vis_gt or args.vis_suppressed) and not args.vis_dir:
            raise ValueError('--vis_gt / --vis_suppressed need --vis_dir')
        consistency = args.consistency or any(getattr(args, t) is not None for t in CS.THRESHOLDS) or (grid is not None and grid.consistency)
        consistency = consistency or args.rescore is not None or fit is not None
        if args.consistency_json and not consistency:
            raise ValueError('--consistency_json writes the consistency measures: it needs --consistency or a --min_* threshold')
        # (the flags as given, not Detector.suppression.on: an error of --vis_* is reported before one of the options Detector checks)
        vis = Vis(args.vis_dir, args.vis_max, args.vis_gt, args.vis_suppressed, nms=args.nms_iou is not None or args.soft_nms is not None) if args.vis_dir else None
        stage = dict({k: getattr(args, k) for k in STAGE_KEYWORDS}, consistency=consistency)
        if grid is not None:                     # (--nms_metric / --nms_score hold for every combination of the sweep, not for its plain run)
            stage.update(nms_metric=None, nms_score=None)
        det = Detector(FLAGS, rt=rt, type_whitelist=args.type_whitelist, log=log, **stage)
    except ValueError as e:
        p.error(str(e))
    valid = set(int(line.rstrip()) for line in open(args.idx_path))
    det_id, det_type, det_box2d, det_prob = SD.read_det_folder(args.rgb_detection_path)
    per_scene = collections.OrderedDict()
    for d, idx in enumerate(det_id):
        per_scene.setdefault(idx, []).append((det_type[d], det_box2d[d], det_prob[d]))
    ids = [i for i in per_scene if i in valid]
    dataset = SD.sunrgbd_object(args.dataset_dir, 'training')
    pictures = None if vis is None else (lambda idx: scene_pictures(dataset, idx, args.vis_gt, args.type_whitelist) if vis.taken < vis.max else {})
    parts = [det.extract(scenes, [per_scene[idx] for idx in batch], batch, vis=vis)
             for batch, scenes in scene_batches(dataset, ids, image_wh=CS.image_size if consistency or visibility.on else None, pictures=pictures)]
    if fit is not None:
        return RS.fit_parts(det, parts, args.dataset_dir, args.idx_path, args.test_on, seed=FLAGS.seed, log=log, **fit)
    if grid is not None:
        top = 10 if args.sweep_top is None else args.sweep_top
        result = det.sweep_parts(parts, grid, args.dataset_dir, args.idx_path, args.test_on, bootstrap=bootstrap, top=top)
        for line in result.lines(top):
            log(line)
        if args.sweep_json:
            result.write_json(args.sweep_json)
            log('sweep of %d configurations written to %s' % (len(grid), args.sweep_json))
        return result
    if args.floor_json:
        rows = det.floor_json_rows(parts)
        FL.write_json(args.floor_json, rows)
        log('floor planes of %d scenes written to %s' % (len(rows), args.floor_json))
    meta, d = det.decode_all(parts)
    if args.consistency_json:                                    # the two reports that need every row, then the rows go
        write_consistency_json(args.consistency_json, meta, d)
        log('consistency measures of %d detections written to %s' % (len(meta), args.consistency_json))
    if vis is not None and d is not None:
        log('%d scenes drawn to %s' % (len(vis.write(det.rt, parts, d, det.stages.corners)), args.vis_dir))
    d, meta = SI.kept(d, meta)
    predictions = det.predictions(meta, d)
    names = [m.name for m in meta]
    log('%d detections of %d images' % (len(meta), len(ids)))
    if FLAGS.result_dir:
        SI.write_detection_results(FLAGS.result_dir, det.classes or sorted(set(names)), predictions, names)
        log('detection results written to %s' % FLAGS.result_dir)
    if args.official_eval:
        held = ES.official_predictions(sorted(set(ES.CLASS_NAMES[args.test_on]) | set(names)), predictions, names)
        ES.evaluate(None, args.dataset_dir, args.idx_path, args.test_on, rt=det.rt, log=log, predictions=held, diagnose=diagnose, bootstrap=bootstrap)
    return predictions


if __name__ == '__main__':
    main()
