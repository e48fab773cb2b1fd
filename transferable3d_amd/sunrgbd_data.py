"""Frustum files from SUN-RGBD scenes: sunrgbd/sunrgbd_data/sunrgbd_data.py of the reference, with the per-box geometry on the device.

    python -m transferable3d_amd.sunrgbd_data --dataset_dir D --output_dir O                 # the five roi_seg files of the reference
    python -m transferable3d_amd.sunrgbd_data --option rgb_detection --test_data val --rgb_detection_path DET --dataset_dir D --output_dir O

The scene readers follow the reference's layout (utils.py:12-77, 174-184); the projection, the frustum test, the subsample and the 3-D
box labels run in csrc/frustum.hip (t3d_frustum_extract) on a batch of scenes per launch, while a host thread pool parses the next
scenes.  The output is the reference's gzip'd pickle of 13 (roi_seg) or 7 (detections) lists, read as it is by
DeviceFrustumSet.from_pickle / from_detection_pickle and by the reference's own loaders.

Random draws: where the reference calls np.random (random_shift_box2d's 4 uniforms, np.random.choice of num_points of a frustum's n > num_points
points) the device draws from a counter-based hash keyed by (seed, scene id, job ordinal within the scene, augmentation index), so a
job's draws do not depend on the batch it runs in.  `draws` injects them instead: {'perturb': {key: 4 uniforms}, 'choice': {key: ranks}},
key = (scene id, ordinal, augmentation index); the ordinal is the object's line in its label file, or the detection's position among
its image's detections.  Generated subsamples keep the points in the cloud's order; injected ones keep the order given.

One deliberate difference: detection files are read in file-name order (the reference's os.listdir order is arbitrary).
"""
import argparse
import collections
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import abi
from .dataset import save_zipped_pickle

TYPE_WHITELIST = ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']
NUM_POINTS = 2048
MAX_WORKERS = 16


class SUNObject3d:
    """One line of label_dimension/%06d.txt (utils.py:12-36)."""

    def __init__(self, line):
        data = line.split(' ')
        data[1:] = [float(x) for x in data[1:]]
        self.classname = data[0]
        self.xmin, self.ymin = data[1], data[2]
        self.xmax, self.ymax = data[1] + data[3], data[2] + data[4]
        self.box2d = np.array([self.xmin, self.ymin, self.xmax, self.ymax])
        self.centroid = np.array([data[5], data[6], data[7]])
        self.w, self.l, self.h = data[8], data[9], data[10]
        self.orientation = np.zeros((3,))
        self.orientation[0] = data[15]
        self.orientation[1] = data[16]
        self.heading_angle = -1 * np.arctan2(self.orientation[1], self.orientation[0])


class Calibration:
    """calib/%06d.txt: Rtilt and K, column-major (utils.py:67-76)."""

    def __init__(self, path):
        lines = [line.rstrip() for line in open(path)]
        self.Rtilt = np.reshape(np.array([float(x) for x in lines[0].split(' ')]), (3, 3), order='F')
        self.K = np.reshape(np.array([float(x) for x in lines[1].split(' ')]), (3, 3), order='F')


def flip_axis_to_camera(pc):
    """upright depth (X right, Y forward, Z up) -> upright camera (X right, Y down, Z forward) (utils.py:78-85)."""
    pc2 = np.copy(pc)
    pc2[:, [0, 1, 2]] = pc2[:, [0, 2, 1]]
    pc2[:, 1] *= -1
    return pc2


def load_depth_points(path):
    """depth/%06d.txt, N x 6: the float64 values np.loadtxt gives (both round every decimal string correctly), a few times faster."""
    with open(path, 'rb') as fh:
        text = fh.read()
    first = text.split(b'\n', 1)[0].split()
    return np.array(text.split(), dtype=np.float64).reshape(-1, len(first))


def load_image(path):
    """image/%06d.jpg as cv2.imread gives it: H x W x 3 uint8, BGR."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def read_sunrgbd_label(path):
    return [SUNObject3d(line.rstrip()) for line in open(path)]


class sunrgbd_object:
    """The reference's data set layout (sunrgbd_data.py:23-62): <root>/<split>/{image,calib,depth,label_dimension}/%06d.*"""

    def __init__(self, root_dir, split='training'):
        self.split_dir = os.path.join(root_dir, split)
        self.split = split

    def _path(self, sub, idx, ext):
        return os.path.join(self.split_dir, sub, '%06d.%s' % (idx, ext))

    def get_image(self, idx):
        return load_image(self._path('image', idx, 'jpg'))

    def get_depth(self, idx):
        return load_depth_points(self._path('depth', idx, 'txt'))

    def get_calibration(self, idx):
        return Calibration(self._path('calib', idx, 'txt'))

    def get_label_objects(self, idx):
        assert self.split == 'training'
        return read_sunrgbd_label(self._path('label_dimension', idx, 'txt'))


def read_det_folder(det_folder):
    """Detection files (sunrgbd_data.py:221-239), in file-name order: lines `type -1 -10 -10 xmin ymin xmax ymax ... prob`."""
    id_list, type_list, prob_list, box2d_list = [], [], [], []
    for filename in sorted(os.listdir(det_folder)):
        img_id = int(filename[0:6])
        for line in open(os.path.join(det_folder, filename), 'r'):
            t = line.rstrip().split(' ')
            id_list.append(img_id)
            type_list.append(t[0])
            prob_list.append(float(t[-1]))
            box2d_list.append(np.array([float(t[i]) for i in range(4, 8)]))
    return id_list, type_list, box2d_list, prob_list


def compute_box_3d(obj):
    """The 8 corners of the object's box in upright camera coordinates (utils.compute_box_3d, then
    project_upright_depth_to_upright_camera), with the reference's operations."""
    c, s = np.cos(-1 * obj.heading_angle), np.sin(-1 * obj.heading_angle)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    l, w, h = obj.l, obj.w, obj.h
    corners = np.dot(R, np.vstack([[-l, l, l, -l, -l, l, l, -l], [w, w, -w, -w, w, w, -w, -w], [h, h, h, h, -h, -h, -h, -h]]))
    corners[0, :] += obj.centroid[0]
    corners[1, :] += obj.centroid[1]
    corners[2, :] += obj.centroid[2]
    return flip_axis_to_camera(np.transpose(corners))


def _runtime(rt):
    if rt is not None:
        return rt
    from .engine import Runtime
    return Runtime()


class FrustumExtractor:
    """t3d_frustum_extract over a batch of scenes: one launch sequence, one copy back."""

    def __init__(self, rt, num_points=NUM_POINTS, seed=0):
        self.rt, self.num_points, self.seed = rt, num_points, seed
        self.last_kernel_ms = None
        self.last_scene = None

    def run(self, scenes, jobs, perturb_box2d=False, timed=False, on_device=False, keep_scene=False):
        """scenes: [{'points': (N, C) fp64 upright depth, 'Rtilt', 'K'}]; jobs (grouped by scene, in scene order): [{'scene': batch index,
        'box2d', 'box3d': (8,3) or None, 'key': (scene id, ordinal, aug), 'perturb': 4 uniforms or None, 'choice': ranks or None}].
        Returns per job {'box2d', 'frustum_angle', 'n', 'index', 'points', 'label'}.  on_device=True: nothing is copied back; returns the
        device tensors of the launch instead ({'box2d_out' [J,4], 'frustum_angle' [J], 'n_in_box' [J], 'count' [J], 'index' [J,NP],
        'out_points' [J,NP,C] fp64, 'label' [J,NP]}; DeviceFrustumSet.from_device takes them), None for no jobs.  keep_scene=True:
        `last_scene` = (the device copy of the scenes' points [sum N, C] fp64, the scenes' row offsets) of this launch, for a caller
        that goes on reading them there (detect --vis_dir)."""
        dev, NP, J, S = self.rt.device, self.num_points, len(jobs), len(scenes)
        if J == 0:
            return None if on_device else []
        sc = np.array([j['scene'] for j in jobs])
        if np.any(np.diff(sc) < 0) or sc.min() < 0 or sc.max() >= S:
            raise ValueError('jobs must be grouped by scene, in scene order')
        counts = np.array([len(s['points']) for s in scenes], np.int64)
        Csrc = scenes[0]['points'].shape[1]
        if any(s['points'].shape[1] != Csrc for s in scenes) or Csrc < 3:
            raise ValueError('every scene needs the same number (>= 3) of channels')
        scene_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        scene_jobs = np.searchsorted(sc, np.arange(S + 1), side='left').astype(np.int32)
        segs = (counts[sc] + 63) // 64
        mask_offsets = np.concatenate([[0], np.cumsum(segs)]).astype(np.int64)
        with_box3d = jobs[0]['box3d'] is not None
        if any((j['box3d'] is not None) != with_box3d for j in jobs):
            raise ValueError('a launch is either all roi_seg jobs (3-D boxes) or all detections')
        with_perturb = perturb_box2d and jobs[0].get('perturb') is not None
        if perturb_box2d and any((j.get('perturb') is not None) != with_perturb for j in jobs):
            raise ValueError('perturbation draws are given for every job of a launch or for none')
        choice = np.full((J, NP), -1, np.int32)
        for i, j in enumerate(jobs):
            if j.get('choice') is not None:
                if len(j['choice']) != NP:
                    raise ValueError('an injected choice holds num_points ranks')
                choice[i] = j['choice']
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(dev)
        t = dict(points=up(np.concatenate([s['points'] for s in scenes]), torch.float64), scene_offsets=up(scene_offsets, torch.int64),
                 rtilt=up(np.stack([np.asarray(s['Rtilt'], np.float64).reshape(9) for s in scenes]), torch.float64),
                 K=up(np.stack([np.asarray(s['K'], np.float64).reshape(9) for s in scenes]), torch.float64),
                 scene_jobs=up(scene_jobs, torch.int32), box2d=up(np.stack([np.asarray(j['box2d'], np.float64) for j in jobs]), torch.float64),
                 job_key=up(np.array([j['key'] for j in jobs], np.int64).astype(np.int32), torch.int32),
                 mask_offsets=up(mask_offsets, torch.int64))
        if keep_scene:
            self.last_scene = (t['points'], scene_offsets)
        if with_perturb:
            t['perturb_draws'] = up(np.array([j['perturb'] for j in jobs], np.float64), torch.float64)
        if with_box3d:
            t['box3d'] = up(np.stack([np.asarray(j['box3d'], np.float64) for j in jobs]), torch.float64)
        if (choice[:, 0] >= 0).any():
            t['choice'] = up(choice, torch.int32)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        nseg = int(mask_offsets[-1])
        o = dict(masks=z((max(nseg, 1),), torch.int64), seg_prefix=z((max(nseg, 1),), torch.int32), box2d_out=z((J, 4), torch.float64),
                 frustum_angle=z((J,), torch.float64), n_in_box=z((J,), torch.int32), count=z((J,), torch.int32),
                 index=z((J, NP), torch.int32), out_points=z((J, NP, Csrc), torch.float64), label=z((J, NP), torch.int32))
        ptr = lambda x, T: C.cast(C.c_void_p(0 if x is None else x.data_ptr()), C.POINTER(T))
        g = lambda k, T: ptr(t.get(k), T)
        a = abi.FrustumExtractArgs(g('points', C.c_double), g('scene_offsets', C.c_int64), g('rtilt', C.c_double), g('K', C.c_double),
                                   g('scene_jobs', C.c_int32), S, int(counts.max()), Csrc, Csrc, J, NP, g('box2d', C.c_double),
                                   int(bool(perturb_box2d)), g('perturb_draws', C.c_double), g('box3d', C.c_double), g('job_key', C.c_int32),
                                   self.seed & 0xFFFFFFFF, g('choice', C.c_int32), g('mask_offsets', C.c_int64),
                                   ptr(o['masks'], C.c_uint64), ptr(o['seg_prefix'], C.c_int32), ptr(o['box2d_out'], C.c_double),
                                   ptr(o['frustum_angle'], C.c_double), ptr(o['n_in_box'], C.c_int32), ptr(o['count'], C.c_int32),
                                   ptr(o['index'], C.c_int32), ptr(o['out_points'], C.c_double),
                                   ptr(o['label'] if with_box3d else None, C.c_int32))
        cuda = dev.type == 'cuda'
        if cuda and timed:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        abi.check(self.rt.lib.t3d_frustum_extract(C.byref(a), self.rt.stream()), 't3d_frustum_extract')
        if cuda and timed:
            ev[1].record()
        if on_device:
            return {k: v for k, v in o.items() if k not in ('masks', 'seg_prefix')}
        h = {k: v.cpu().numpy() for k, v in o.items() if k not in ('masks', 'seg_prefix')}     # the one copy back (synchronises)
        if cuda and timed:
            self.last_kernel_ms = ev[0].elapsed_time(ev[1])
        out = []
        for i in range(J):
            c = int(h['count'][i])
            out.append({'box2d': h['box2d_out'][i], 'frustum_angle': np.float64(h['frustum_angle'][i]), 'n': int(h['n_in_box'][i]),
                        'index': h['index'][i, :c], 'points': h['out_points'][i, :c],
                        'label': h['label'][i, :c].astype(np.float64) if with_box3d else None})
        return out


def _scenes_in_batches(load, ids, batch_scenes, workers):
    """(ids, loaded scenes) of consecutive batches; a pool of at most MAX_WORKERS threads parses ahead of the device."""
    workers = max(1, min(int(workers), MAX_WORKERS))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        window = collections.deque()
        it = iter(ids)
        for idx in it:
            window.append((idx, pool.submit(load, idx)))
            if len(window) >= 2 * batch_scenes + workers:
                break
        batch = []
        while window:
            idx, fut = window.popleft()
            batch.append((idx, fut.result()))
            nxt = next(it, None)
            if nxt is not None:
                window.append((nxt, pool.submit(load, nxt)))
            if len(batch) == batch_scenes or not window:
                yield batch
                batch = []


def _job_draws(draws, key):
    if not draws:
        return None, None
    p = draws.get('perturb', {}).get(tuple(key))
    c = draws.get('choice', {}).get(tuple(key))
    return (None if p is None else np.asarray(p, np.float64)), (None if c is None else np.asarray(c, np.int32))


def extract_roi_seg(dataset_dir, idx_list, split='training', augmentX=1, perturb_box2d=False, type_whitelist=TYPE_WHITELIST,
                    num_points=NUM_POINTS, seed=0, rt=None, draws=None, batch_scenes=16, workers=8, timings=None, dataset=None):
    """sunrgbd_data.extract_roi_seg (sunrgbd_data.py:130-195) on the device.  idx_list: scene ids, or the path of an index file.
    Returns the reference's 13 lists: [id, box2d, box3d, image crop, points, label, type, heading, box3d size, Rtilt, K,
    frustum angle, img_dims].  dataset: an object with sunrgbd_object's four getters (synth_scenes.SceneSet.dataset(): scenes held in
    memory) in place of the files under dataset_dir."""
    if isinstance(idx_list, str):
        idx_list = [int(line.rstrip()) for line in open(idx_list)]
    ex = FrustumExtractor(_runtime(rt), num_points, seed)
    if dataset is None:
        dataset = sunrgbd_object(dataset_dir, split)

    def load(idx):
        calib = dataset.get_calibration(idx)
        return calib, dataset.get_label_objects(idx), dataset.get_depth(idx), dataset.get_image(idx)

    lists = [[] for _ in range(13)]
    for batch in _scenes_in_batches(load, idx_list, batch_scenes, workers):
        scenes, jobs, meta = [], [], []
        for b, (idx, (calib, objects, depth, img)) in enumerate(batch):
            scenes.append({'points': depth, 'Rtilt': calib.Rtilt, 'K': calib.K})
            for oi, obj in enumerate(objects):
                if obj.classname not in type_whitelist:
                    continue
                corners = compute_box_3d(obj)
                for aug in range(augmentX):
                    key = (idx, oi, aug)
                    pu, ch = _job_draws(draws, key)
                    jobs.append({'scene': b, 'box2d': obj.box2d, 'box3d': corners, 'key': key, 'perturb': pu, 'choice': ch})
                    meta.append((idx, obj, calib, img, corners))
        res = ex.run(scenes, jobs, perturb_box2d=perturb_box2d, timed=timings is not None)
        if timings is not None and ex.last_kernel_ms is not None:
            timings.append(ex.last_kernel_ms)
        for r, (idx, obj, calib, img, corners) in zip(res, meta):
            if np.sum(r['label']) < 5:                # reject objects with too few points (sunrgbd_data.py:168-170)
                continue
            xmin, ymin, xmax, ymax = [float(v) for v in r['box2d']]
            h, w, _ = img.shape
            for lst, v in zip(lists, (idx, np.array([xmin, ymin, xmax, ymax]), corners, img[int(ymin):int(ymax), int(xmin):int(xmax), :],
                                      r['points'], r['label'], obj.classname, obj.heading_angle,
                                      np.array([2 * obj.l, 2 * obj.w, 2 * obj.h]), calib.Rtilt, calib.K, r['frustum_angle'], [h, w])):
                lst.append(v)
    return lists


def extract_roi_seg_from_rgb_detection(det_folder, dataset_dir, split='training', valid_id_list=None, type_whitelist=TYPE_WHITELIST,
                                       seed=0, rt=None, draws=None, num_points=NUM_POINTS, batch_scenes=16, workers=8, timings=None,
                                       dataset=None):
    """sunrgbd_data.extract_roi_seg_from_rgb_detection (sunrgbd_data.py:242-326) on the device.  Returns the reference's 7 lists:
    [id, box2d, image crop, points, type, frustum angle, prob].  dataset: as for extract_roi_seg."""
    det_id, det_type, det_box2d, det_prob = read_det_folder(det_folder)
    valid = None if valid_id_list is None else set(valid_id_list)
    ex = FrustumExtractor(_runtime(rt), num_points, seed)
    if dataset is None:
        dataset = sunrgbd_object(dataset_dir, split)
    ordinal = collections.Counter()
    per_scene = collections.OrderedDict()         # scene id -> [(det index, ordinal)], scenes in order of their first detection
    for d, idx in enumerate(det_id):
        o = ordinal[idx]
        ordinal[idx] += 1
        if valid is not None and idx not in valid:
            continue
        if det_type[d] not in type_whitelist:
            continue
        per_scene.setdefault(idx, []).append((d, o))

    def load(idx):
        return dataset.get_calibration(idx), dataset.get_depth(idx), dataset.get_image(idx)

    kept = {}
    for batch in _scenes_in_batches(load, list(per_scene), batch_scenes, workers):
        scenes, jobs, meta = [], [], []
        for b, (idx, (calib, depth, img)) in enumerate(batch):
            scenes.append({'points': depth, 'Rtilt': calib.Rtilt, 'K': calib.K})
            for d, o in per_scene[idx]:
                key = (idx, o, 0)
                _, ch = _job_draws(draws, key)
                jobs.append({'scene': b, 'box2d': det_box2d[d], 'box3d': None, 'key': key, 'choice': ch})
                meta.append((d, img))
        res = ex.run(scenes, jobs, timed=timings is not None)
        if timings is not None and ex.last_kernel_ms is not None:
            timings.append(ex.last_kernel_ms)
        for r, (d, img) in zip(res, meta):
            if len(r['points']) < 5:                  # sunrgbd_data.py:313-315
                continue
            xmin, ymin, xmax, ymax = det_box2d[d]
            kept[d] = (img[int(ymin):int(ymax), int(xmin):int(xmax), :], r['points'], r['frustum_angle'])
    lists = [[] for _ in range(7)]
    for d in sorted(kept):
        crop, pts, angle = kept[d]
        for lst, v in zip(lists, (det_id[d], det_box2d[d], crop, pts, det_type[d], angle, det_prob[d])):
            lst.append(v)
    return lists


def get_box3d_dim_statistics(dataset_dir, idx_list, output_path, type_whitelist=TYPE_WHITELIST):
    """sunrgbd_data.py:197-219: three pickles (types, [l, w, h], heading) in one file."""
    import pickle
    dataset = sunrgbd_object(dataset_dir)
    dims, types, ry = [], [], []
    for idx in idx_list:
        for obj in dataset.get_label_objects(idx):
            if obj.classname not in type_whitelist:
                continue
            dims.append(np.array([obj.l, obj.w, obj.h]))
            types.append(obj.classname)
            ry.append(-1 * np.arctan2(obj.orientation[1], obj.orientation[0]))
    with open(output_path, 'wb') as fp:
        pickle.dump(types, fp, 2)
        pickle.dump(dims, fp, 2)
        pickle.dump(ry, fp, 2)


# --option '': the reference's five files (sunrgbd_data.py:354-367): (index file, output file, augmentX)
ROI_SEG_FILES = [('train_mini_data_idx.txt', 'train_mini.zip.pickle', 1), ('train_data_idx.txt', 'train_aug5x.zip.pickle', 5),
                 ('val_data_idx.txt', 'val.zip.pickle', 1), ('trainval_data_idx.txt', 'trainval_aug5x.zip.pickle', 5),
                 ('test_data_idx.txt', 'test.zip.pickle', 1)]


def parser():
    p = argparse.ArgumentParser()
    p.add_argument('--option', default='', choices=['', 'stats', 'rgb_detection'],
                   help='To visualize, to retrieve the statistics or to extract the rois with 2D predictions.')
    p.add_argument('--test_data', default='', choices=['train', 'val', 'trainval', 'test'], help='Dataset to use for testing.')
    p.add_argument('--rgb_detection_path', default=None, help='Path for the 2D detection results')
    p.add_argument('--output_filename', default=None, help='Name for the output pickle filename')
    p.add_argument('--dataset_dir', default='mysunrgbd', help='SUN-RGBD root (<dir>/training/{image,calib,depth,label_dimension})')
    p.add_argument('--output_dir', default='frustums', help='where the .zip.pickle files are written')
    p.add_argument('--seed', type=int, default=0, help='seed of the device draws (box perturbation, subsampling)')
    return p


def main(argv=None):
    FLAGS = parser().parse_args(argv)
    idx_file = lambda name: os.path.join(FLAGS.dataset_dir, 'training', name)
    read_ids = lambda path: [int(line.rstrip()) for line in open(path)]
    os.makedirs(FLAGS.output_dir, exist_ok=True)
    written = []
    if FLAGS.option == 'stats':
        path = os.path.join(FLAGS.output_dir, 'box3d_dimensions.pickle')
        get_box3d_dim_statistics(FLAGS.dataset_dir, read_ids(idx_file('train_data_idx.txt')), path)
        written.append(path)
    elif FLAGS.option == 'rgb_detection':
        if FLAGS.rgb_detection_path is None:
            raise Exception('Please provide an 2D detection path.')
        if FLAGS.output_filename is None:
            FLAGS.output_filename = FLAGS.rgb_detection_path.split('/')[-1]
        assert FLAGS.test_data in ['train', 'val', 'trainval', 'test']
        valid = read_ids(idx_file('%s_data_idx.txt' % FLAGS.test_data))
        lists = extract_roi_seg_from_rgb_detection(FLAGS.rgb_detection_path, FLAGS.dataset_dir, 'training', valid_id_list=valid, seed=FLAGS.seed)
        path = os.path.join(FLAGS.output_dir, '%s_%s.zip.pickle' % (FLAGS.test_data, FLAGS.output_filename))
        save_zipped_pickle(lists, path)
        written.append(path)
    else:
        rt = _runtime(None)
        for idx_name, out_name, augmentX in ROI_SEG_FILES:
            lists = extract_roi_seg(FLAGS.dataset_dir, idx_file(idx_name), 'training', augmentX=augmentX, seed=FLAGS.seed, rt=rt)
            path = os.path.join(FLAGS.output_dir, out_name)
            save_zipped_pickle(lists, path)
            n = sum(len(p) for p in lists[4])
            print('%s: %d frustums, average pos ratio %.4f' % (path, len(lists[0]), sum(float(np.sum(l)) for l in lists[5]) / max(n, 1)))
            written.append(path)
    return written


if __name__ == '__main__':
    main()
