"""Shared pieces of the detection-decode tests (t3d_detect_decode, semisup_infer.inference(decode='device'), transferable3d_amd/detect.py)
for the CPU tests (NumPy specification libraries) and the GPU tests (libt3d.so)."""
import os

import numpy as np
import torch

import fake_detect as FD
import frustum_check as FC
from transferable3d_amd import constants as K
from transferable3d_amd import detect as DT
from transferable3d_amd import sunrgbd_data as SD
from transferable3d_amd import semisup_infer as SI
from transferable3d_amd import test_semisup as TS
from transferable3d_amd.dataset import save_zipped_pickle
from transferable3d_amd.engine import Runtime

NH, NS = K.NUM_HEADING_BIN, K.NUM_SIZE_CLUSTER
FLOATS = ('score', 'center', 'heading_res', 'size_res', 'label', 'corners')
INTS = ('mask_count', 'heading_cls', 'size_cls')


class WideRuntime(Runtime):
    """A host runtime whose float buffers are fp64, for FakeDetectLib(wide=True)."""

    def zeros(self, *shape, dtype=torch.float64):
        return Runtime.zeros(self, *shape, dtype=dtype)


def golden_vectors():
    return np.load(os.path.join(FC.GOLDEN, 'reference_vectors.npz'))


def golden_net(V):
    """infer/net/* as the entry point's inputs: (logits [12,32,2], box_out [12,67] in BoxHeads order, stage1_center = 0, fit_prob)."""
    net = {k: V['infer/net/' + k] for k in ('logits', 'center', 'hs', 'hr', 'ss', 'sr', 'fit')}
    B = len(net['center'])
    box = np.zeros((B, FD.BOX))
    box[:, 0:3], box[:, 3:3 + NH], box[:, 3 + NH:3 + 2 * NH] = net['center'], net['hs'], net['hr'] / (np.pi / NH)
    box[:, 3 + 2 * NH:3 + 2 * NH + NS] = net['ss']
    box[:, 3 + 2 * NH + NS:] = (net['sr'] / K.MEAN_DIMS_ARR[None]).reshape(B, 3 * NS)
    return net['logits'], box, np.zeros((B, 3)), net['fit']


def random_case(seed, B, N):
    r = np.random.RandomState(seed)
    return dict(logits=r.normal(0, 2.0, (B, N, 2)), box_out=r.normal(0, 1.0, (B, FD.BOX)) * 0.5, stage1_center=r.normal(0, 2.0, (B, 3)),
                total_delta=r.normal(0, 0.1, (B, 7)), fit_prob=r.uniform(0, 1, B), rot_angle=r.uniform(-np.pi, np.pi, B))


def cases():
    """name -> fp32 inputs of the kernel tests: the golden network outputs, random cases at sizes around the block (1 point, one more than a
    wave, no multiple of 256, eight strides of the block), all-background and all-foreground frustums, exact ties, headings on both
    sides of pi."""
    out = {}
    lg, box, s1, fit = golden_net(golden_vectors())
    g = random_case(1, len(box), lg.shape[1])
    g.update(logits=lg, box_out=box, stage1_center=s1, fit_prob=fit)
    out['golden'] = g
    for B, N in ((1, 1), (5, 65), (3, 1000), (4, 2048)):
        out['random_%dx%d' % (B, N)] = random_case(100 + N, B, N)
    c = random_case(7, 2, 300)
    c['logits'][0, :, 0], c['logits'][0, :, 1] = 3.0, -2.0          # all background: the "+ 1" denominator alone
    c['logits'][1, :, 0], c['logits'][1, :, 1] = -1.5, 2.5          # all foreground
    out['all_bg_all_fg'] = c
    c = random_case(8, 3, 130)
    c['logits'][0, ::3, 1] = c['logits'][0, ::3, 0]                 # l1 == l0: background
    c['box_out'][:, 3:3 + NH] = np.round(c['box_out'][:, 3:3 + NH] * 4) / 4
    c['box_out'][0, 3 + 2], c['box_out'][0, 3 + 7], c['box_out'][0, 3 + 9] = 5.0, 5.0, 5.0            # heading tie: 2 wins
    c['box_out'][1, 3:3 + NH] = 0.25                                                                 # all equal: 0 wins
    c['box_out'][0, 27 + 4], c['box_out'][0, 27 + 8] = 4.0, 4.0                                      # size tie: 4 wins
    c['box_out'][2, 27:27 + NS] = -1.0
    out['ties'] = c
    c = random_case(9, 6, 64)
    c['box_out'][:, 3:3 + NH] = 0.0
    c['total_delta'][:, 6] = 0.0
    for b, (k, res) in enumerate(((6, -0.2), (6, 0.2), (5, 0.5), (5, 0.55), (11, 0.26), (0, -0.26))):   # 6 * 30 deg = pi: -0.2 stays, +0.2 wraps
        c['box_out'][b, 3 + k] = 3.0
        c['box_out'][b, 3 + NH + k] = res / (np.pi / NH)
    out['around_pi'] = c
    return {k: {n: np.ascontiguousarray(a, np.float32) for n, a in v.items()} for k, v in out.items()}


def run_decode(rt, c, with_delta=True, with_fit=True, with_rot=True, pad=0, n_valid=None, sentinel=None):
    """t3d_detect_decode through semisup_infer.DeviceDecode on the case's arrays; `pad`: that many more frustums (copies of the first)
    in front of and behind the case, so that the same frustums sit in a batch of another size at other block indices.
    -> (Decoded of the case's rows, masks)."""
    B, N = c['logits'].shape[:2]
    grow = lambda a: np.concatenate([np.repeat(a[:1], pad, 0), a, np.repeat(a[:1], pad, 0)]) if pad else a
    up = lambda k, on=True: torch.as_tensor(grow(c[k])).to(rt.device) if on else None
    dec = SI.DeviceDecode(rt, B + 2 * pad, N, want_seg=True)
    if sentinel is not None:
        dec.f.fill_(sentinel)
        dec.i.fill_(int(sentinel))
        dec.seg.fill_(int(sentinel))
    keep = (up('logits'), up('box_out'), up('stage1_center'), up('total_delta', with_delta), up('fit_prob', with_fit), up('rot_angle', with_rot))
    dec.launch(0, B + 2 * pad, B + 2 * pad if n_valid is None else n_valid, *keep)
    d, seg = dec.fetch()
    return d[slice(pad, pad + B)], seg[pad:pad + B]


def spec(c, with_delta=True, with_fit=True, with_rot=True):
    return FD.decode(c['logits'], c['box_out'], c['stage1_center'], c['total_delta'] if with_delta else None,
                     c['fit_prob'] if with_fit else None, c['rot_angle'] if with_rot else None)


def worst_errors(d, seg, want):
    """Integer outputs and masks exactly; -> {float output: worst |difference| from the fp64 spec}."""
    assert np.array_equal(seg, want['seg'])
    for k in INTS:
        assert np.array_equal(getattr(d, k), want[k]), k
    return {k: float(np.abs(getattr(d, k) - want[k]).max()) for k in FLOATS}


# ---- scene-level flow ---------------------------------------------------------------------------------------------------------------
# N = 256, not 128: t3d_boxpc_rep (the Box-PC net of --refine 1) takes frustums of a multiple of 256 points only
MODEL_FLAGS = ['--semi_type', 'F', '--use_one_hot', '--num_point', '256', '--batch_size', '4', '--refine', '1', '--pred_prefix', 'F2_',
               '--seed', '3', '--test', 'AB', '--SUNRGBD_SEMI_TEST_CLS'] + list(SD.TYPE_WHITELIST)
SPARSE = ('chair', (1.0, 1.0, 1.5, 1.5), 0.5)       # a detection whose frustum holds fewer than 5 points


def write_data_set(root):
    """The golden scenes as a data set directory, and a detection folder made from their label boxes (prob by position) plus, in the first
    scene, one detection of a quarter of a pixel.  -> (ids, detection folder, index file, detections per scene)."""
    ids, _, _ = FC.write_golden_scenes(root)
    ds = SD.sunrgbd_object(str(root))
    folder = os.path.join(str(root), 'det_from_labels')
    os.makedirs(folder)
    dets = []
    for k, s in enumerate(ids):
        rows = [(o.classname, tuple(float(v) for v in o.box2d), 0.95 - 0.05 * i) for i, o in enumerate(ds.get_label_objects(s))]
        if k == 0:
            rows.insert(1, SPARSE)
        dets.append(rows)
        with open(os.path.join(folder, '%06d.txt' % s), 'w') as fh:
            for name, b, p in rows:
                fh.write('%s -1 -10 -10 %r %r %r %r -1 -1 -1 -1000 -1000 -1000 -10 %r\n' % ((name,) + b + (p,)))
    idx = os.path.join(str(root), 'idx.txt')
    with open(idx, 'w') as fh:
        fh.write(''.join('%d\n' % i for i in ids))
    return ids, folder, idx, dets


def two_step(rt, root, ids, folder, out_name, device_decode):
    """sunrgbd_data's detection frustums -> pickle -> test_semisup --from_rgb_detection --result_dir; -> {class: text of its file}."""
    lists = SD.extract_roi_seg_from_rgb_detection(folder, str(root), valid_id_list=ids, seed=3, rt=rt)
    path = os.path.join(str(root), 'val_det.zip.pickle')
    save_zipped_pickle(lists, path)
    res = os.path.join(str(root), out_name)
    flags = SI.build_flags(MODEL_FLAGS + ['--from_rgb_detection', '--data_path', path, '--result_dir', res] + (['--device_decode'] if device_decode else []))
    predictions = SI.test(flags, rt=rt, log=lambda *a: None)
    return read_results(res), lists, predictions


def read_results(res):
    return {f[:-len('_pred.txt')]: open(os.path.join(res, f)).read() for f in sorted(os.listdir(res))}


def record_lines(ids, records):
    """The lines write_detection_results writes for the records Detector.detect returned, per class."""
    out = {}
    for s, recs in zip(ids, records):
        for r in recs:
            out.setdefault(r['class'], []).append('%d %s -1 -1 -10 %f %f %f %f %f %f %f %f %f %f %f %f\n' % (
                (s, r['class']) + tuple(r['box2d']) + tuple(r['label']) + (r['prob'],)))
    return {c: ''.join(l) for c, l in out.items()}


def load_scenes(root, ids):
    ds = SD.sunrgbd_object(str(root))
    return [{'points': ds.get_depth(s), 'Rtilt': ds.get_calibration(s).Rtilt, 'K': ds.get_calibration(s).K} for s in ids]


def check_scene_flow(rt, root, bound):
    """The issue's four comparisons on the golden scenes; -> lines of what was compared."""
    ids, folder, idx, dets = write_data_set(root)
    a, lists, pa = two_step(rt, root, ids, folder, 'res_two_step_device', True)
    b, _, pb = two_step(rt, root, ids, folder, 'res_two_step_host', False)
    # eval_det.predictions_to_boxes: the kernel's corners (rot_angle != 0 here) against the host loop over the same 14-list, and over the
    # host-decoded one
    from transferable3d_amd import eval_det as E
    classes = [K.class2type[i] for i in range(K.NUM_CLASS)]
    assert pa.decoded is not None and pb.decoded is None and min(abs(float(r)) for r in pa[8]) > 1e-3
    dev_boxes, loop_boxes, host_boxes = E.predictions_to_boxes(pa, classes), E.predictions_to_boxes(list(pa), classes), E.predictions_to_boxes(pb, classes)
    assert sorted(dev_boxes) == sorted(loop_boxes) == sorted(host_boxes)
    # the host loops start from fp32 records: beside `bound`, half an ulp of a coordinate below 8 (2^-22) for the stored corner, as much for
    # the centre they read, and less than that again for the size and heading residuals (each below 4, entering halved)
    tol, worst_k = bound + 3 * 2.0 ** -22, 0.0
    for img in dev_boxes:
        for (n1, k1, s1), (n2, k2, s2), (n3, k3, s3) in zip(dev_boxes[img], loop_boxes[img], host_boxes[img]):
            assert n1 == n2 == n3 and s1 == s2 == s3 and k1.shape == (8, 3)
            worst_k = max(worst_k, np.abs(k1 - k2).max(), np.abs(k1 - k3).max())
            assert worst_k <= tol and np.abs(k1).max() < 8.0, (img, n1, worst_k)
    res = os.path.join(str(root), 'res_detect')
    DT.main(['--dataset_dir', str(root), '--idx_path', idx, '--rgb_detection_path', folder, '--result_dir', res] + MODEL_FLAGS, rt=rt,
            log=lambda *a: None)
    c = read_results(res)
    n = sum(len(t.splitlines()) for t in a.values())
    assert n == len(lists[0]) > 4 and SPARSE in dets[0] and n < sum(len(d) for d in dets)
    assert a == c, 'detect differs from sunrgbd_data + test_semisup --device_decode'
    sparse = '%f %f %f %f' % SPARSE[1]
    assert all(sparse not in t for t in list(a.values()) + list(c.values()))
    # host decode: the same detections, every number within the kernel's bound of the fp64 host arithmetic, as two values printed at %f
    # can show it: each is rounded to 1e-6, so they differ by at most bound + 1e-6 -- five digits behind the point are compared
    assert sorted(a) == sorted(b)
    worst = 0.0
    for cname in a:
        la, lb = a[cname].splitlines(), b[cname].splitlines()
        assert len(la) == len(lb)
        for x, y in zip(la, lb):
            x, y = x.split(), y.split()
            assert x[:5] == y[:5] and len(x) == len(y) == 17
            worst = max(worst, max(abs(float(p) - float(q)) for p, q in zip(x[5:], y[5:])))
    assert worst <= bound + 1e-6, worst
    records = DT.Detector(TS.build_flags(MODEL_FLAGS), rt=rt).detect(load_scenes(root, ids), dets, scene_ids=ids)
    lines = record_lines(ids, records)
    assert set(lines) <= set(c) and all(lines.get(cname, '') == text for cname, text in c.items())      # (a class without detections: an empty file)
    assert all(r['corners'].shape == (8, 3) and np.isfinite(r['score']) for recs in records for r in recs)
    return ['%d detections, %d classes; device decode against host decode as printed: worst |difference| %.3e; corners against the host loops: %.3e (tolerance %.3e)'
            % (n, len(a), worst, worst_k, tol)]
