#!/usr/bin/env python3
"""The two modes of the reference's viewer.py that matter on a server, as files instead of a vtk window.

    python -m transferable3d_amd.viewer --vis pred3d --pred_files P [P ...] --gt_file G [--num 10] [--filenums N ...] [--seed S] [--out_dir vis]
    python -m transferable3d_amd.viewer --vis fpc --filenum N [--rgb_detection] [--dataset_dir mysunrgbd] [--rgb_detection_path DETS] [--out_dir vis]

pred3d reads `test_semisup --output` pickles (the 14-list: points, ground-truth masks, predicted masks, centres, heading class and
residual, size class and residual, rotation angles, scores, classes, file numbers, 2-D boxes, 3-D label boxes) and the ground-truth
frustum file.  It picks --num frustums spread over the classes as viewer.py:343-360 does (an equal share per class in order of first
appearance, the shares shuffled, drawn without replacement; here from RandomState(--seed)) and writes, per prediction file, one contact
sheet OUT/pred3d_<name>.png with its legend OUT/pred3d_<name>.json.  A frustum is one tile: a bird's-eye view and a side view of its
points, the label box in green and the predicted box in white.  Where the pickle holds the points the network saw and their masks, the
points are coloured by predicted against ground-truth mask (neither, predicted only, ground truth only, both); where it does not
(test_semisup leaves both out for a frustum file: its batches are drawn on the device), the points and the mask are the ground-truth
file's, in two colours.  It logs what the reference shows as text: `Mean Box IOU` (t3d_box3d_iou_corners over every prediction against
its label box) and `Mean Seg IOU` (get_seg_iou, viewer.py:507-516) per file, and evaluate.get_ap_info's block through eval_det.

fpc draws OUT/fpc_<N>.png: the scene's image with, per labelled object (--rgb_detection: per 2-D detection), the points of its frustum
in the object's colour and its 2-D box.  The frustums come from FrustumExtractor (t3d_frustum_extract).

Everything is painted by t3d_render (render.py); there is no text in the pictures.  The other modes of viewer.py (pc, seg_box, box_pc,
pred2d) parse and exit with a message.
"""
import argparse
import json
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transferable3d_amd import render as RD, sunrgbd_data as SD                  # noqa: E402
from transferable3d_amd.constants import MEAN_DIMS_ARR, NUM_HEADING_BIN, class2type      # noqa: E402
from transferable3d_amd.dataset import load_zipped_pickle                        # noqa: E402
from transferable3d_amd.eval_det import box3d_iou_batch, evaluate_predictions, get_3d_box, get_ap_info      # noqa: E402

SUPPORTED = ('pred3d', 'fpc')
MODES = ('pc', 'fpc', 'seg_box', 'box_pc', 'pred2d', 'pred3d')
TILE = 160                    # a tile is two TILE x TILE panels side by side
COLUMNS = 5


def get_seg_iou(seg_gt, seg_pred, num_seg_classes=2):
    """viewer.py:507-516: the mean over the classes of |gt = l and pred = l| / |gt = l or pred = l|.  (A class in neither mask makes the
    reference stop on an assertion; here it counts 1, the value the line behind the assertion would have appended.)"""
    seg_gt, seg_pred = np.asarray(seg_gt), np.asarray(seg_pred)
    ious = []
    for l in range(num_seg_classes):
        union = np.sum((seg_gt == l) | (seg_pred == l))
        ious.append(1.0 if union == 0 else np.sum((seg_gt == l) & (seg_pred == l)) / float(union))
    return float(np.mean(ious))


def rotate_along_y(pc, angle):
    """roi_seg_box3d_dataset.rotate_pc_along_y on a copy."""
    pc = np.array(pc, np.float64)
    c, s = np.cos(angle), np.sin(angle)
    pc[:, [0, 2]] = np.stack([c * pc[:, 0] - s * pc[:, 2], s * pc[:, 0] + c * pc[:, 2]], 1)
    return pc


def y_max_face_first(k):
    """A label box with its y-max face in rows 0-3, the order get_3d_box gives a predicted one (evaluate.py:49-52)."""
    k = np.asarray(k, np.float64)
    return k if k[0, 1] >= k[4, 1] else k[[4, 5, 6, 7, 0, 1, 2, 3]]


def predicted_boxes(predictions):
    """[n,8,3]: class2angle / class2size / get_3d_box in the centre view, rotated back by -rot_angle (evaluate.py:56-72)."""
    _, _, _, center_l, hcls_l, hres_l, scls_l, sres_l, rot_l = predictions[:9]
    out = []
    for i in range(len(center_l)):
        heading = int(hcls_l[i]) * (2 * np.pi / NUM_HEADING_BIN) + float(hres_l[i])
        if heading > np.pi:
            heading -= 2 * np.pi
        k = get_3d_box(MEAN_DIMS_ARR[int(scls_l[i])] + np.asarray(sres_l[i], np.float64), heading, np.asarray(center_l[i], np.float64).reshape(3))
        out.append(rotate_along_y(k, -float(rot_l[i])))
    return np.stack(out) if out else np.zeros((0, 8, 3))


def choose(cls_l, file_l, num, seed, filenums=None):
    """viewer.py:343-360: `num` prediction indices spread over the whitelisted classes."""
    options, order = {}, []
    for i, c in enumerate(cls_l):
        if class2type[int(c)] not in SD.TYPE_WHITELIST or (filenums is not None and int(file_l[i]) not in filenums):
            continue
        if int(c) not in options:
            order.append(int(c))
        options.setdefault(int(c), []).append(i)
    if not options:
        return []
    r = np.random.RandomState(seed)
    shares = [len(g) for g in np.array_split([1] * num, len(order))]
    r.shuffle(shares)
    picked = []
    for c, share in zip(order, shares):
        picked += [int(i) for i in r.choice(options[c], min(share, len(options[c])), replace=False)]
    return picked


def match_ground_truth(predictions, gt):
    """Per prediction, the index of its frustum in the ground-truth file: the one with the same file number and the same label box
    (predictions without label boxes: the k-th prediction of an image and class is its k-th frustum)."""
    file_l, cls_l, box3d_l = predictions[11], predictions[10], predictions[13]
    by_box, by_order = {}, {}
    for j in range(len(gt[0])):
        by_box.setdefault((int(gt[0][j]), np.asarray(gt[2][j], np.float64).tobytes()), j)
        by_order.setdefault((int(gt[0][j]), gt[6][j]), []).append(j)
    out, seen = [], {}
    for i in range(len(file_l)):
        j = None
        if box3d_l is not None and box3d_l[i] is not None:
            j = by_box.get((int(file_l[i]), np.asarray(box3d_l[i], np.float64).tobytes()))
        if j is None:
            key = (int(file_l[i]), class2type[int(cls_l[i])])
            k = seen.get(key, 0)
            seen[key] = k + 1
            j = by_order.get(key, [None] * (k + 1))[k] if k < len(by_order.get(key, [])) else None
        out.append(j)
    return out


def frustum_views(xyz, colours, label, gt_box, pred_box):
    """[bird's-eye view, side view] of one frustum, everything in upright camera coordinates."""
    boxes = np.stack([gt_box, pred_box]).astype(np.float32)
    xr, yr, zr = RD.ranges_of(np.concatenate([np.asarray(xyz, np.float64)[:, :3], boxes.reshape(-1, 3)]))
    ext = max(yr[1] - yr[0], zr[1] - zr[0])                    # the side view shows y and z at one scale
    ymid = 0.5 * (yr[0] + yr[1])
    views = [RD.bev_view(xr, zr, TILE, TILE, y_top=yr[0], bg_colour=RD._rgb(12, 12, 16)),
             RD.side_view((zr[0], zr[0] + ext), (ymid - 0.5 * ext, ymid + 0.5 * ext), TILE, TILE, x_near=xr[0], bg_colour=RD._rgb(12, 12, 16))]
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    for v in views:
        if colours is not None:
            v.points(xyz, rgb=colours, splat=3)
        else:
            v.points(xyz, label=label, colour0=RD.MASK_COLOURS[0], colour1=RD.MASK_COLOURS[1], splat=3)
        v.boxes(boxes, [RD.GT_COLOUR, RD.PRED_COLOUR], thickness=1)
    return views


def vis_predictions3d(pred_files, gt_file, num, filenums, seed, out_dir, rt, log):
    """-> per prediction file {'mean_box_iou', 'mean_seg_iou' (None without masks), 'ap', 'mean_ap', 'sheet', 'chosen'}"""
    gt = load_zipped_pickle(gt_file)
    classes = [class2type[i] for i in range(len(class2type))]
    gt_all = {}
    for img, name, k in zip(gt[0], gt[6], gt[2]):
        gt_all.setdefault(int(img), []).append((name, y_max_face_first(k)))
    os.makedirs(out_dir, exist_ok=True)
    ren = RD.Renderer(rt)
    results, chosen = [], None
    for pred_file in pred_files:
        predictions = load_zipped_pickle(pred_file)
        if not isinstance(predictions, (list, tuple)) or len(predictions) != 14:
            raise ValueError('%s is no test_semisup --output file (a list of 14 lists)' % pred_file)
        ps_l, seg_gt_l, seg_pred_l = predictions[0], predictions[1], predictions[2]
        cls_l, file_l, box3d_l = predictions[10], predictions[11], predictions[13]
        n = len(predictions[3])
        if chosen is None:                                     # the choice of the first file serves all of them (viewer.py:342)
            chosen = choose(cls_l, file_l, num, seed, None if not filenums else set(int(f) for f in filenums))
            log('Number of objects in whitelist: %d' % len(set(int(cls_l[i]) for i in range(n) if class2type[int(cls_l[i])] in SD.TYPE_WHITELIST)))
        where = match_ground_truth(predictions, gt)
        label_box = [y_max_face_first(box3d_l[i]) if box3d_l is not None and box3d_l[i] is not None
                     else (y_max_face_first(gt[2][where[i]]) if where[i] is not None else None) for i in range(n)]
        if any(b is None for b in label_box):
            raise ValueError('%s: a prediction has no label box in the file and no frustum in %s' % (pred_file, gt_file))
        pred_box = predicted_boxes(predictions)
        log('==== Computing overall statistics for %s ====' % pred_file)
        _, _, ap, mean_ap = evaluate_predictions(predictions, gt_all, classes, rt=rt)
        log(get_ap_info(ap, mean_ap))
        box_iou = box3d_iou_batch(np.stack(label_box), pred_box, rt)[0].astype(np.float64)
        mean_box_iou = float(box_iou.mean())
        with_masks = seg_gt_l is not None and seg_pred_l is not None
        mean_seg_iou = float(np.mean([get_seg_iou(seg_gt_l[i], seg_pred_l[i]) for i in range(n)])) if with_masks else None
        log('Mean Box IOU: %f' % mean_box_iou)
        log('Mean Seg IOU: %f' % mean_seg_iou if with_masks else 'Mean Seg IOU: not available (the prediction file holds no masks of its points)')
        views, tiles = [], []
        for i in chosen:
            if i >= n:
                continue
            rot = float(predictions[8][i])
            if ps_l is not None and with_masks:
                xyz = rotate_along_y(np.asarray(ps_l[i], np.float64)[:, :3], -rot)          # the network's points, back from the centre view
                code = 2 * (np.asarray(seg_gt_l[i]) != 0).astype(np.int64) + (np.asarray(seg_pred_l[i]) != 0)
                views += frustum_views(xyz, np.asarray(RD.MASK_AGREEMENT, np.float32)[code], None, label_box[i], pred_box[i])
                seg_iou = get_seg_iou(seg_gt_l[i], seg_pred_l[i])
            else:
                j = where[i]
                if j is None:
                    raise ValueError('%s: prediction %d has no frustum in %s' % (pred_file, i, gt_file))
                views += frustum_views(np.asarray(gt[4][j])[:, :3], None, np.asarray(gt[5][j]), label_box[i], pred_box[i])
                seg_iou = None
            tiles.append({'prediction': int(i), 'class': class2type[int(cls_l[i])], 'file_num': int(file_l[i]), 'box_iou': float(box_iou[i]),
                          'seg_iou': seg_iou})
        name = os.path.basename(pred_file).split('.')[0]
        sheet = os.path.join(out_dir, 'pred3d_%s.png' % name)
        if views:
            panels = ren.render(views)
            RD.write_png(sheet, RD.contact_sheet([RD.side_by_side(panels[2 * k:2 * k + 2], gap=2) for k in range(len(tiles))], columns=COLUMNS))
        legend = {'pred_file': pred_file, 'gt_file': gt_file, 'mean_box_iou': mean_box_iou, 'mean_seg_iou': mean_seg_iou,
                  'ap': {k: float(v) for k, v in ap.items()}, 'mean_ap': mean_ap, 'tile': [TILE, 2 * TILE + 2], 'columns': COLUMNS, 'tiles': tiles,
                  'colours': {'gt_box': list(RD.GT_COLOUR), 'pred_box': list(RD.PRED_COLOUR)}}
        with open(os.path.join(out_dir, 'pred3d_%s.json' % name), 'w') as fh:
            json.dump(legend, fh, indent=1)
        log('%d tiles written to %s' % (len(tiles), sheet))
        results.append(dict(mean_box_iou=mean_box_iou, mean_seg_iou=mean_seg_iou, ap=ap, mean_ap=mean_ap, sheet=sheet, chosen=list(chosen)))
    return results


def vis_fpc(filenum, rgb_detection, dataset_dir, det_folder, out_dir, rt, log):
    """The scene's image with every frustum's points in its object's colour and the 2-D boxes -> (path, objects drawn)."""
    dataset = SD.sunrgbd_object(dataset_dir, 'training')
    calib = dataset.get_calibration(filenum)
    image = np.ascontiguousarray(dataset.get_image(filenum)[:, :, ::-1])
    if rgb_detection:
        if not det_folder:
            raise ValueError('--rgb_detection needs --rgb_detection_path')
        lists = SD.extract_roi_seg_from_rgb_detection(det_folder, dataset_dir, valid_id_list=[filenum], rt=rt)
        objects = [(t, b, p) for t, b, p in zip(lists[4], lists[1], lists[3])]
    else:
        lists = SD.extract_roi_seg(dataset_dir, [filenum], rt=rt)
        objects = [(t, b, p) for t, b, p in zip(lists[6], lists[1], lists[4])]
    view = RD.image_view(calib.Rtilt, calib.K, image.shape[0], image.shape[1], image=image)
    legend = []
    for k, (name, box2d, pts) in enumerate(objects):
        colour = RD.CLASS_PALETTE[k % len(RD.CLASS_PALETTE)]                 # one colour per object: two chairs stay apart
        view.points(np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3]), colour0=colour, splat=3)
        view.rects([box2d], colour, thickness=2)
        legend.append({'object': k, 'class': name, 'box2d': [float(v) for v in box2d], 'points': int(len(pts)), 'colour': list(colour)})
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'fpc_%06d.png' % filenum)
    RD.write_png(path, RD.Renderer(rt).render([view])[0])
    with open(os.path.join(out_dir, 'fpc_%06d.json' % filenum), 'w') as fh:
        json.dump({'scene': int(filenum), 'rgb_detection': bool(rgb_detection), 'objects': legend}, fh, indent=1)
    log('%d frustums of scene %d drawn to %s' % (len(objects), filenum, path))
    return path, legend


def parser():
    p = argparse.ArgumentParser(description='viewer.py without a display: pictures of predictions and frustums, painted on the device', allow_abbrev=False)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--vis', required=True, choices=MODES, help='type of visualisation (built: %s)' % ', '.join(SUPPORTED))
    p.add_argument('--filename', type=str, help='file name to show (modes that are not built)')
    p.add_argument('--filenum', type=int, help='file number to show (fpc)')
    p.add_argument('--filenums', nargs='+', type=int, help='only show these file numbers (pred3d)')
    p.add_argument('--pred_files', nargs='+', type=str, help='prediction files (test_semisup --output)')
    p.add_argument('--gt_file', type=str, help='ground-truth frustum file for pred3d')
    p.add_argument('--num', type=int, default=10, help='number to show')
    p.add_argument('--rgb_detection', action='store_true')
    p.add_argument('--out_dir', default='vis', help='where the pictures go')
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (fpc)')
    p.add_argument('--rgb_detection_path', default=None, help='folder of 2-D detection files (fpc --rgb_detection)')
    return p


def main(argv=None, rt=None, log=print):
    args = parser().parse_args(argv)
    if args.vis not in SUPPORTED:
        raise SystemExit('--vis %s needs a display and is not built: the modes without one are %s' % (args.vis, ' and '.join(SUPPORTED)))
    if args.vis == 'pred3d' and (not args.pred_files or not args.gt_file):
        parser().error('--vis pred3d needs --pred_files and --gt_file')
    if args.vis == 'fpc' and args.filenum is None:
        parser().error('--vis fpc needs --filenum')
    if rt is None:
        from transferable3d_amd.engine import Runtime
        rt = Runtime()
    if args.vis == 'pred3d':
        return vis_predictions3d(args.pred_files, args.gt_file, args.num, args.filenums, args.seed, args.out_dir, rt, log)
    return vis_fpc(args.filenum, args.rgb_detection, args.dataset_dir, args.rgb_detection_path, args.out_dir, rt, log)


if __name__ == '__main__':
    main()
