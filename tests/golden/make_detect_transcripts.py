"""Generates tests/golden/detect_transcripts.json: what `detect.main`, `Detector.detect` and the two-step route of semisup_infer DO behind
t3d_detect_decode, seen from outside, on the CPU with the NumPy specification library (`python tests/golden/make_detect_transcripts.py`).
Recorded at the commit BEFORE the stages' options and record fields got one owner each (nms.suppression, NmsRequest.of,
Decoded.confidence, detect.FIELD_GROUPS); tests/test_detect_transcripts_cpu.py replays the recording with no tolerance, so the file is
regenerated only when the behaviour is changed on purpose -- never to make a refactor pass.

Every run goes through the golden scenes of detect_check.write_data_set, Runtime(device='cpu', lib=fake_rescore.FakeRescoreLib()) and
detect_check.MODEL_FLAGS.  But for the plain run every detection is reported a second time as stages_check.doubled does, so that every
(image, class) group holds a pair and a suppression has something to do.  The three thresholds (--min_reproj_iou of `consistency`,
--min_view_iou of `tta`, --min_rescore of `rescore`) are midpoints between order statistics of runs without thresholds, as in stages_check.

Per run of RUNS (detect.main): every line given to `log`, the text of every result file, of --consistency_json and of every legend
<id>.json, a SHA-256 of every <id>.png.  Per run of DETECT (Detector.detect with keywords): every record as its keys in order with the
repr of its scalars and a SHA-256 of its arrays.  Per run of TWO_STEP (semisup_infer.build_flags + test on the frustum file of
detect_check.two_step): the log, the result files, entries 9 .. 12 of the 14-list and len(.decoded).  A text of more than LONG
characters is kept as its SHA-256, its length and its head (key order is part of what is compared: texts, not parsed objects).
The directory of the data set reads <root> everywhere, a run's own <out>.

`errors`: for every argv of ERRORS, what detect.main ends with (the message argparse's `error` prints) and what
semisup_infer.build_flags does with it behind --device_decode --from_rgb_detection; for every argv of BUILD_FLAGS_ERRORS the latter alone.
Which of two simultaneous errors is reported is behaviour.  `attributes`: the option attributes of a Detector per keyword form of
KEYWORDS, and of the namespace of semisup_infer.build_flags per argv of NAMESPACES, each as [type name, value].
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402

OUT = os.path.join(HERE, 'detect_transcripts.json')
LONG = 1500
NMS_IOU = '0.05'                                   # stages_check.NMS_IOU
MODEL = {'features': ['score', 'reproj_iou'], 'coef': [0.05, 6.0, -2.0]}       # written by hand: features that need no --tta

# detect.main: name -> (detections doubled, argv; <T>, <A>, <P>, <model>, <json>, <vis>, <res> are filled in per run)
RUNS = {
    'plain': (False, ['--official_eval']),
    'fuse': (True, ['--nms_iou', NMS_IOU, '--nms_fuse']),
    'bev_score_vote': (True, ['--nms_iou', NMS_IOU, '--nms_metric', 'bev', '--nms_score', 'score', '--nms_fuse_iou', '0.5']),
    'soft_gaussian': (True, ['--soft_nms', 'gaussian', '--soft_nms_sigma', '0.3']),
    'soft_linear': (True, ['--soft_nms', 'linear', '--nms_iou', NMS_IOU, '--soft_nms_min_prob', '0.05']),
    'consistency': (True, ['--consistency', '--min_reproj_iou', '<T>', '--consistency_json', '<json>', '--vis_dir', '<vis>', '--vis_gt',
                           '--vis_suppressed', '--nms_iou', NMS_IOU]),
    # (--consistency: --consistency_json needs it, and --min_view_iou does not imply it)
    'tta': (True, ['--tta', '2', '--tta_flip', '--min_view_iou', '<A>', '--nms_iou', NMS_IOU, '--nms_fuse', '--consistency', '--consistency_json',
                   '<json>', '--vis_dir', '<vis>']),
    'rescore': (True, ['--rescore', '<model>', '--min_rescore', '<P>', '--soft_nms', 'gaussian', '--consistency_json', '<json>',
                       '--vis_dir', '<vis>']),
}
# the keyword forms of the runs above ('<A>', '<P>' and '<model>' as there)
KEYWORDS = {
    'fuse': dict(nms_iou=0.05, nms_fuse=True),
    'bev_score_vote': dict(nms_iou=0.05, nms_metric='bev', nms_score='score', nms_fuse_iou=0.5),
    'soft_gaussian': dict(soft_nms='gaussian', soft_nms_sigma=0.3),
    'soft_linear': dict(soft_nms='linear', nms_iou=0.05, soft_nms_min_prob=0.05),
    'tta': dict(tta=2, tta_flip=True, min_view_iou='<A>', nms_iou=0.05, nms_fuse=True, consistency=True),
    'rescore': dict(rescore='<model>', min_rescore='<P>', soft_nms='gaussian'),
}
DETECT = ('fuse', 'soft_linear', 'tta', 'rescore')         # Detector(**KEYWORDS[name]).detect(...)
TWO_STEP = {'fuse': ['--nms_iou', NMS_IOU, '--nms_fuse'], 'soft_gaussian': ['--soft_nms', 'gaussian']}
ATTRIBUTES = ('nms_iou', 'nms_metric', 'nms_score', 'nms_fuse', 'nms_fuse_iou', 'soft_nms', 'thresholds', 'consistency', 'tta', 'tta_flip',
              'tta_vote_iou', 'min_view_iou', 'min_rescore')
FLAG_ATTRIBUTES = ('soft_nms', 'nms_iou', 'nms_metric', 'nms_score', 'nms_fuse', 'nms_fuse_iou', 'device_decode')
DEV = ['--device_decode', '--from_rgb_detection']
NAMESPACES = [[], DEV] + [DEV + RUNS[k][1] for k in ('fuse', 'bev_score_vote', 'soft_gaussian', 'soft_linear')]

_SWEEP = ['--sweep', '--sweep_nms_iou', '0.25']
_FIT = ['--rescore_fit', '<root>/m.json']
# the argv of the flag-error tests: test_detect_soft_nms_cpu, test_detect_nms_cpu, test_detect_fuse_cpu, test_detect_ensemble_cpu,
# test_detect_sweep_cpu, rescore_check.check_flag_errors (test_rescore_cpu), then the ones that hold two errors at once
ERRORS = [
    ['--soft_nms', 'gaussian', '--nms_iou', '0.3'], ['--soft_nms', 'linear'], ['--soft_nms', 'gaussian', '--nms_score', 'score'],
    ['--soft_nms', 'gaussian', '--nms_fuse'], ['--soft_nms', 'linear', '--nms_iou', '0.3', '--nms_fuse_iou', '0.5'],
    ['--soft_nms_sigma', '0.5'], ['--soft_nms_min_prob', '0.01'], ['--soft_nms', 'gaussian', '--soft_nms_sigma', '0'],
    ['--soft_nms', 'gaussian', '--soft_nms_min_prob', '1'], ['--soft_nms', 'cosine'],
    ['--soft_nms', 'gaussian', '--sweep'], ['--soft_nms', 'linear', '--nms_iou', '0.3', '--sweep'],
    ['--nms_metric', 'bev'], ['--nms_score', 'score'], ['--nms_iou', '0'], ['--nms_iou', '1.01'], ['--nms_iou', '0.3', '--nms_metric', 'xy'],
    ['--nms_fuse'], ['--nms_fuse_iou', '0.5'], ['--nms_iou', '0.3', '--nms_fuse_iou', '0.25'],
    ['--nms_iou', '0.3', '--nms_fuse', '--nms_fuse_iou', '1.01'],
    ['--tta', '1'], ['--tta', '9'], ['--tta_flip'], ['--tta_vote_iou', '0.5'], ['--min_view_iou', '0.5'], ['--tta', '3', '--min_view_iou', '1.5'],
    ['--tta', '3', '--tta_vote_iou', '-1'], ['--tta', '3', '--sweep', '--sweep_nms_iou', '0.25'], ['--tta', 'x'],
    ['--sweep'], ['--sweep_nms_iou', '0.25'], ['--sweep_json', 'x.json'], ['--sweep_top', '3'],
    _SWEEP + ['--nms_iou', '0.3'], _SWEEP + ['--nms_fuse'], _SWEEP + ['--nms_fuse_iou', '0.5'], _SWEEP + ['--min_reproj_iou', '0.5'],
    _SWEEP + ['--min_mask_in_box', '0.5'], _SWEEP + ['--min_seg_box_iou', '0.5'], _SWEEP + ['--official_eval', '--diagnose'],
    _SWEEP + ['--vis_dir', '<root>'], _SWEEP + ['--consistency_json', 'x.json'], _SWEEP + ['--sweep_top', '-1'],
    ['--sweep', '--sweep_nms_iou', '0'], ['--sweep', '--sweep_nms_iou', 'of'], ['--sweep', '--sweep_min_reproj_iou', '1.5'],
    ['--sweep', '--sweep_min_reproj_iou', '0.5', '--nms_metric', 'bev'],
    ['--sweep', '--sweep_nms_iou'] + ['%g' % (0.01 * k) for k in range(1, 18)],
    ['--sweep', '--sweep_nms_iou'] + ['%g' % (0.05 * k) for k in range(1, 17)] + ['--sweep_min_reproj_iou'] + ['%g' % (0.01 * k) for k in range(65)]
    + ['--sweep_min_mask_in_box'] + ['%g' % (0.01 * k) for k in range(64)],
    ['--min_rescore', '0.5'], ['--rescore', '<model>'] + _FIT, ['--rescore', '<model>', '--sweep', '--sweep_nms_iou', 'off', '0.25'],
    _FIT + ['--sweep', '--sweep_nms_iou', 'off', '0.25'], ['--rescore_lambda', '0.1'], ['--rescore_features', 'score'], ['--rescore_target', 'tp'],
    ['--rescore_holdout', '0.2'], ['--rescore_classes', 'chair'], ['--rescore', '<model>', '--min_rescore', '1.5'],
    ['--rescore', '<model>', '--min_rescore', '-0.1'], _FIT + ['--rescore_holdout', '1.0'], _FIT + ['--rescore_lambda', '0'],
    _FIT + ['--nms_iou', '0.25'], _FIT + ['--rescore_features', 'view_iou'],
    ['--min_rescore', '0.5', '--vis_gt'], ['--min_rescore', '0.5', '--soft_nms', 'cosine'], _FIT + ['--rescore_features', 'view_iou', '--nms_fuse'],
    ['--vis_dir', '<root>/v', '--vis_suppressed', '--nms_metric', 'bev'], ['--rescore', '<views>'], ['--tta', '1', '--nms_metric', 'bev'],
]
# what the same tests give semisup_infer.build_flags as it stands
BUILD_FLAGS_ERRORS = [
    ['--soft_nms', 'gaussian'], ['--from_rgb_detection', '--soft_nms', 'gaussian'], ['--device_decode', '--soft_nms', 'gaussian'],
    ['--nms_iou', '0.3'], ['--from_rgb_detection', '--nms_iou', '0.3'], ['--device_decode', '--nms_iou', '0.3'], DEV + ['--nms_metric', 'bev'],
    DEV + ['--nms_iou', '7'], ['--nms_iou', '0.3', '--nms_fuse'], DEV + ['--tta', '3'],
]


def sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else data.encode()).hexdigest()


def text_of(text):
    """A text as it is, or -- a long one -- its hash, its length and its head."""
    return text if len(text) <= LONG else {'sha256': sha(text), 'chars': len(text), 'head': text[:400]}


def plain(v):
    """A value as json writes it: tuples (named ones too) and arrays as lists, NumPy scalars as Python's."""
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return plain(v.tolist())
    return v.item() if isinstance(v, np.generic) else v


def typed(v):
    return [type(v).__name__, plain(v)]


def runtime():
    import fake_rescore
    from transferable3d_amd.engine import Runtime
    return Runtime(device='cpu', lib=fake_rescore.FakeRescoreLib())


class World:
    """The data set of every run under one directory, and the three thresholds."""

    def __init__(self, root):
        import consistency_check as CC
        import detect_check as DC
        import stages_check as SC
        from transferable3d_amd import detect as DT, rescore as RS, test_semisup as TS
        self.root = str(root)
        self.ids, self.folder, self.idx, self.dets = DC.write_data_set(self.root)
        self.doubled = SC.doubled(self.dets)
        self.folder2 = os.path.join(self.root, 'det_doubled')
        os.makedirs(self.folder2)
        for s, rows in zip(self.ids, self.doubled):              # (the lines of detect_check.write_data_set)
            with open(os.path.join(self.folder2, '%06d.txt' % s), 'w') as fh:
                for name, b, p in rows:
                    fh.write('%s -1 -10 -10 %r %r %r %r -1 -1 -1 -1000 -1000 -1000 -10 %r\n' % ((name,) + tuple(float(v) for v in b) + (p,)))
        self.model = os.path.join(self.root, 'hand.json')
        RS.Model(MODEL['features'], MODEL['coef']).save(self.model)
        self.views = os.path.join(self.root, 'views.json')
        RS.Model(('score', 'view_iou'), [1.0, 1.0, 0.0]).save(self.views)
        self.scenes = CC.scenes_with_sizes(_Path(self.root), self.ids)
        self.flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
        first = DT.Detector(self.flags(), rt=runtime(), tta=2, tta_flip=True, consistency=True)
        _, d0 = first.decode_all([first.extract(self.scenes, self.doubled, self.ids)])
        self.n = len(d0)
        self.T, self.A = between(d0.reproj_iou, self.n // 3), between(d0.view_iou, self.n // 3)
        first = DT.Detector(self.flags(), rt=runtime(), rescore=self.model)
        self.P = between(first.decode_all([first.extract(self.scenes, self.doubled, self.ids)])[1].rescore_prob, self.n // 3)

    def fill(self, v, out=None):
        """An argv entry or keyword value with its placeholder filled in."""
        if not isinstance(v, str):
            return v
        if v in ('<A>', '<P>') and out is None:                 # (a keyword)
            return self.A if v == '<A>' else self.P
        for k, w in (('<T>', repr(self.T)), ('<A>', repr(self.A)), ('<P>', repr(self.P)), ('<model>', self.model), ('<views>', self.views), ('<root>', self.root)):
            v = v.replace(k, w)
        for k in ('res', 'json', 'vis'):
            v = v.replace('<%s>' % k, os.path.join(out or self.root, k))
        return v

    def argv(self, doubled=True):
        import detect_check as DC
        return ['--dataset_dir', self.root, '--idx_path', self.idx, '--rgb_detection_path', self.folder2 if doubled else self.folder] + DC.MODEL_FLAGS

    def tidy(self, line, out=None):
        line = str(line) if out is None else str(line).replace(out, '<out>')
        return line.replace(self.root, '<root>')


class _Path(str):
    """str with the `/` of pathlib, which consistency_check.scenes_with_sizes uses."""

    def __truediv__(self, other):
        return _Path(os.path.join(self, str(other)))


def between(values, k):
    """The midpoint between two neighbouring order statistics from rank k on that differ: some values lie below it and not all."""
    v = np.sort(np.asarray(values, np.float64))
    while v[k - 1] == v[k]:
        k += 1
    return float((v[k - 1] + v[k]) / 2.0)


_WORLD = []


def world():
    """One World per process (the directory lives as long as the process)."""
    if not _WORLD:
        tmp = tempfile.TemporaryDirectory()
        _WORLD.extend([World(tmp.name), tmp])
    return _WORLD[0]


def files_of(w, out):
    """What a run wrote under its directory `out`."""
    got = {}
    res, cj, vis = (os.path.join(out, k) for k in ('res', 'json', 'vis'))
    if os.path.isdir(res):
        got['results'] = {f: text_of(open(os.path.join(res, f)).read()) for f in sorted(os.listdir(res))}
    if os.path.exists(cj):
        got['consistency_json'] = text_of(open(cj).read())
    if os.path.isdir(vis):
        names = sorted(os.listdir(vis))
        got['legends'] = {f: text_of(open(os.path.join(vis, f)).read()) for f in names if f.endswith('.json')}
        got['png'] = {f: sha(open(os.path.join(vis, f), 'rb').read()) for f in names if f.endswith('.png')}
    return got


def record_main(name):
    """detect.main with RUNS[name] and --result_dir."""
    from transferable3d_amd import detect as DT
    w = world()
    doubled, argv = RUNS[name]
    out = tempfile.mkdtemp(dir=w.root)
    lines = []
    DT.main(w.argv(doubled) + [w.fill(a, out) for a in ['--result_dir', '<res>'] + argv], rt=runtime(), log=lambda line: lines.append(w.tidy(line, out)))
    return dict(files_of(w, out), log=lines)


def keywords_of(name):
    w = world()
    return {k: w.fill(v) for k, v in KEYWORDS[name].items()}


def record_of(r):
    """A record of Detector.detect as one line: its keys in order, each with the repr of its value -- of 'label' and 'corners' the dtype,
    the shape and the head of the SHA-256 of the bytes, of any other array its dtype and its values."""
    def value(k, v):
        if isinstance(v, np.ndarray):
            return '%s%s %s' % (v.dtype, list(v.shape), sha(np.ascontiguousarray(v).tobytes())[:16] if k in ('label', 'corners') else v.tolist())
        return '%s %r' % (type(v).__name__, plain(v))
    return '; '.join('%s: %s' % (k, value(k, v)) for k, v in r.items())


def record_detect(name):
    """Detector(**KEYWORDS[name]).detect(...) on the doubled detections -> its attributes and, per scene, its records."""
    from transferable3d_amd import detect as DT
    w = world()
    lines = []
    det = DT.Detector(w.flags(), rt=runtime(), log=lambda line: lines.append(w.tidy(line)), **keywords_of(name))
    got = {'attributes': attributes_of(det)}
    if name in DETECT:
        got['records'] = [[record_of(r) for r in recs] for recs in det.detect(w.scenes, w.doubled, scene_ids=w.ids)]
        got['log'] = lines
    return got


def attributes_of(obj, names=ATTRIBUTES):
    return {k: typed(getattr(obj, k)) for k in names}


def record_two_step(name):
    """semisup_infer.build_flags + test behind --device_decode --from_rgb_detection on the frustum file of detect_check.two_step; 'plain'
    is two_step's own run."""
    import detect_check as DC
    from transferable3d_amd import semisup_infer as SI
    w = world()
    path = os.path.join(w.root, 'val_det.zip.pickle')
    if name == 'plain' or not os.path.exists(path):
        texts, _, p = DC.two_step(runtime(), w.root, w.ids, w.folder2, 'res_two_step', True)
    lines = []
    if name != 'plain':
        res = tempfile.mkdtemp(dir=w.root)
        flags = SI.build_flags(DC.MODEL_FLAGS + DEV + ['--data_path', path, '--result_dir', res] + TWO_STEP[name])
        p = SI.test(flags, rt=runtime(), log=lambda line: lines.append(w.tidy(line, res)))
        texts = DC.read_results(res)
    return {'log': lines, 'results': {c: text_of(t) for c, t in texts.items()}, 'decoded': len(p.decoded),
            'entries': {str(k): text_of(json.dumps(plain(list(p[k])))) for k in (9, 10, 11, 12)}}


def error_of(call):
    """What a call that must refuse its arguments ends with."""
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            call()
    except SystemExit:
        return 'argument error: ' + err.getvalue().strip().split('error: ', 1)[-1]
    except ValueError as e:
        return 'ValueError: %s' % e
    except Exception as e:                                      # (accepted by the checks; it failed on the files that are not there)
        return 'accepted, then %s' % type(e).__name__
    return 'accepted'


def record_errors():
    from transferable3d_amd import detect as DT, semisup_infer as SI
    w = world()
    needed = ['--dataset_dir', w.root, '--idx_path', 'none', '--rgb_detection_path', 'none']
    out = {'detect': [], 'build_flags': []}
    for argv in ERRORS:
        real = [w.fill(a) for a in argv]
        out['detect'].append([' '.join(argv), w.tidy(error_of(lambda: DT.main(needed + real, log=lambda *a: None)))])
        out['build_flags'].append([' '.join(DEV + argv), w.tidy(error_of(lambda: SI.build_flags(DEV + real)))])
    for argv in BUILD_FLAGS_ERRORS:
        out['build_flags'].append([' '.join(argv), w.tidy(error_of(lambda: SI.build_flags(list(argv))))])
    return out


def record_namespaces():
    from transferable3d_amd import semisup_infer as SI
    return [[' '.join(argv), attributes_of(SI.build_flags(list(argv)), FLAG_ATTRIBUTES)] for argv in NAMESPACES]


def main():
    w = world()
    out = {'thresholds': {'T': repr(w.T), 'A': repr(w.A), 'P': repr(w.P), 'n': w.n}, 'main': {}, 'detect': {}, 'two_step': {}}
    for name in RUNS:
        out['main'][name] = record_main(name)
        print('main %s: %d log lines' % (name, len(out['main'][name]['log'])))
        for line in out['main'][name]['log'][:4]:
            print('   ', line)
    for name in KEYWORDS:
        out['detect'][name] = record_detect(name)
        print('detect %s: %s records' % (name, sum(len(r) for r in out['detect'][name].get('records', []))))
    for name in ['plain'] + list(TWO_STEP):
        out['two_step'][name] = record_two_step(name)
        print('two-step %s: %d decoded' % (name, out['two_step'][name]['decoded']))
    out['errors'] = record_errors()
    out['namespaces'] = record_namespaces()
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
