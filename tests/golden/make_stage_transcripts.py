"""Generates tests/golden/stage_transcripts.json: what `detect.main`, `Detector.detect` and `autolabel.main` DO with the floor stage, the
visibility stage and all seven rejecting tests at once, seen from outside, on the CPU with the NumPy specification libraries
(`python tests/golden/make_stage_transcripts.py`).  detect_transcripts.json was made before the floor and visibility stages existed and
covers neither of them, nor autolabel; this recording stands beside it.  Recorded at the commit BEFORE each rejecting test was stated
once (consistency.Test, semisup_infer.TESTS); tests/test_stage_transcripts_cpu.py replays it with no tolerance, so the file is regenerated
only when the behaviour is changed on purpose -- never to make a refactor pass.

The recorder (text_of, record_of, between, files_of, error_of, World.tidy) is make_detect_transcripts.py's.  The scenes are the four
ray-cast ones of the `world` fixtures of test_floor_cpu.py and test_visibility_cpu.py (scene_check.scene_set: floors and walls), written
out as a data set and read back as `detect.main` reads them; every detection is reported a second time as stages_check.doubled does.
The runtime's library composes the specification mixins under tests/: VisibilitySpec and FloorSpec on fake_rescore.FakeRescoreLib, with
FakeSceneLib for the ray caster.

The seven limits are midpoints between neighbouring order statistics (`between`) of one run that measures everything and rejects
nothing.  `conditions` in the file says what they were chosen for: in `all_seven` every test rejects a detection, one detection is
rejected by two tests, one is accepted, and one exceeds --max_see_through or --max_floor_gap as a bare number and is spared by the rule
of its test (too few rays, a flag of visibility.UNMEASURED, an unknown floor).

Per run of RUNS (detect.main): the log, the result files, --consistency_json, --floor_json, the legends and a SHA-256 of every picture.
Per run of KEYWORDS (Detector(**keywords).detect): the log and every record.  `autolabel`: autolabel.main with the flags of all_seven
plus --score_against_labels --floor_json: every log line, the texts of autolabel.json (key order is part of it), of every label file,
of autolabel_idx.txt and of the floor JSON, and every entry of '_records' as its keys in order with their values.  `errors`: what
detect.main and autolabel.parse end with for every argv of ERRORS.
"""
import importlib.util
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

_spec = importlib.util.spec_from_file_location('make_detect_transcripts', os.path.join(HERE, 'make_detect_transcripts.py'))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)
text_of, record_of, between = D.text_of, D.record_of, D.between

OUT = os.path.join(HERE, 'stage_transcripts.json')
NMS_IOU = D.NMS_IOU
MIN_RAYS = 4
SCENES = 4                                          # scene_check.scene_set(rt, 4, ...): the fixtures' scenes
SEVEN = ['--min_reproj_iou', '<T>', '--min_mask_in_box', '<M>', '--min_seg_box_iou', '<S>', '--tta', '2', '--tta_flip', '--min_view_iou', '<A>',
         '--rescore', '<model>', '--min_rescore', '<P>', '--max_floor_gap', '<G>', '--max_see_through', '<F>', '--visibility_min_rays', str(MIN_RAYS)]

# detect.main: name -> argv (<T> ... <F>, <model>, <json>, <floor>, <vis>, <res> are filled in per run)
RUNS = {
    'floor': ['--floor', '--floor_json', '<floor>', '--consistency', '--consistency_json', '<json>'],
    'snap': ['--snap_floor', 'shift', '--max_floor_gap', '<G>', '--nms_iou', NMS_IOU, '--vis_dir', '<vis>'],
    'see_through': ['--max_see_through', '<F>', '--visibility_min_rays', str(MIN_RAYS), '--consistency', '--consistency_json', '<json>'],
    'all_seven': SEVEN + ['--nms_iou', NMS_IOU, '--nms_fuse'],
}
# the keyword forms of `snap` and `all_seven`
KEYWORDS = {
    'snap': dict(snap_floor='shift', max_floor_gap='<G>', nms_iou=0.05),
    'all_seven': dict(min_reproj_iou='<T>', min_mask_in_box='<M>', min_seg_box_iou='<S>', tta=2, tta_flip=True, min_view_iou='<A>', rescore='<model>',
                      min_rescore='<P>', max_floor_gap='<G>', max_see_through='<F>', visibility_min_rays=MIN_RAYS, nms_iou=0.05, nms_fuse=True),
}
AUTOLABEL = SEVEN + ['--score_against_labels', '--floor_json', '<floor>']

_SWEEP, _FIT = ['--sweep'], ['--rescore_fit', 'm.json']
# every floor and visibility flag with a value it takes
FLAG_ARGV = [['--floor'], ['--snap_floor', 'shift'], ['--snap_floor', 'shift', '--snap_floor_max', '0.2'], ['--max_floor_gap', '0.2'], ['--floor', '--floor_bin', '0.04'],
             ['--floor', '--floor_range', '-3', '-1'], ['--floor', '--floor_min_share', '0.1'], ['--floor', '--floor_band', '0.1'], ['--floor', '--floor_max_tilt', '3'],
             ['--floor', '--floor_json', 'x.json'], ['--visibility'], ['--visibility', '--visibility_cell', '8'], ['--visibility', '--visibility_margin', '0.1'],
             ['--visibility', '--visibility_min_chord', '0.2'], ['--max_see_through', '0.5'], ['--max_see_through', '0.5', '--visibility_min_rays', '8']]
# the argv of test_flag_errors_are_argument_errors of test_floor_cpu.py and of test_visibility_cpu.py and of the two
# test_autolabel_takes_the_flags, every flag with --sweep and with --rescore_fit, then two lines that hold two errors at once
ERRORS = [
    ['--snap_floor_max', '0.2'], ['--floor_bin', '0.02'], ['--floor_range', '-3', '-1'], ['--floor_json', 'x.json'], ['--max_floor_gap', '-0.5'],
    ['--max_floor_gap', 'nan'], ['--snap_floor', 'shift', '--snap_floor_max', '-1'], ['--floor', '--floor_band', 'nan'], ['--floor', '--sweep'],
    ['--sweep', '--snap_floor', 'stretch'], ['--sweep', '--max_floor_gap', '0.2'], ['--rescore_fit', 'm.json', '--floor'],
    ['--rescore_fit', 'm.json', '--max_floor_gap', '0.1'],
    ['--visibility_cell', '4'], ['--visibility_margin', '0.1'], ['--visibility_min_chord', '0.1'], ['--visibility', '--visibility_min_rays', '8'],
    ['--max_see_through', '1.5'], ['--max_see_through', 'nan'], ['--visibility', '--visibility_cell', '0'], ['--visibility', '--visibility_margin', 'nan'],
    ['--visibility', '--sweep'], ['--sweep', '--max_see_through', '0.5'], ['--rescore_fit', 'm.json', '--visibility'],
    ['--rescore_fit', 'm.json', '--max_see_through', '0.5'],
    ['--floor_json', 'f.json'], ['--visibility_min_rays', '8'],
] + [_SWEEP + a for a in FLAG_ARGV] + [_FIT + a for a in FLAG_ARGV] + [
    ['--floor_json', 'x.json', '--visibility_min_rays', '8'], ['--sweep', '--max_floor_gap', '-0.5', '--visibility_cell', '4'],
]


def runtime():
    import fake_floor
    import fake_rescore
    import fake_visibility
    from transferable3d_amd.engine import Runtime

    class StageLib(fake_visibility.VisibilitySpec, fake_floor.FloorSpec, fake_rescore.FakeRescoreLib, fake_floor.FakeSceneLib):
        """Everything `detect` and `autolabel` call, the floor and visibility stages included, and the ray caster."""

    return Runtime(device='cpu', lib=StageLib())


class World(D.World):
    """The data set of every run under one directory, and the seven limits.  (`tidy` is the parent's.)"""

    def __init__(self, root):
        import detect_check as DC
        import scene_check as SK
        import stages_check as SC
        from transferable3d_amd import consistency as CS, detect as DT, floor as FL, rescore as RS, sunrgbd_data as SD, test_semisup as TS, visibility as VS
        self.root = str(root)
        ss = SK.scene_set(runtime(), SCENES, det_dup=1.0, det_miss=0.0, det_confuse=0.0, det_fp_per_image=0.0)
        ss.write(self.root)
        self.ids = ss.ids
        self.idx = os.path.join(self.root, 'training', 'all_idx.txt')
        with open(self.idx, 'w') as fh:
            fh.write(''.join('%d\n' % i for i in self.ids))
        self.doubled = SC.doubled([[(name, tuple(float(v) for v in b), p) for name, b, p in s['detections']] for s in ss.scenes])
        self.folder2 = os.path.join(self.root, 'det_doubled')
        os.makedirs(self.folder2)
        for s, rows in zip(self.ids, self.doubled):              # (the lines of detect_check.write_data_set)
            with open(os.path.join(self.folder2, '%06d.txt' % s), 'w') as fh:
                for name, b, p in rows:
                    fh.write('%s -1 -10 -10 %r %r %r %r -1 -1 -1 -1000 -1000 -1000 -10 %r\n' % ((name,) + tuple(float(v) for v in b) + (p,)))
        self.classes = sorted(set(lab['object'].classname for s in ss.scenes for lab in s['labels']))
        self.model = os.path.join(self.root, 'hand.json')
        RS.Model(D.MODEL['features'], D.MODEL['coef']).save(self.model)
        self.scenes = [sc for _, scenes in DT.scene_batches(SD.sunrgbd_object(self.root, 'training'), self.ids, image_wh=CS.image_size) for sc in scenes]
        self.flags = lambda: TS.build_flags(DC.MODEL_FLAGS)
        first = DT.Detector(self.flags(), rt=runtime(), tta=2, tta_flip=True, consistency=True, rescore=self.model, floor=True, visibility=True)
        _, d = first.decode_all([first.extract(self.scenes, self.doubled, self.ids)])
        self.n = n = len(d)
        self.T, self.M, self.S = between(d.reproj_iou, n // 12), between(d.mask_in_box, n // 12), between(d.seg_box_iou, n // 12)
        self.A, self.P = between(d.view_iou, n // 10), between(d.rescore_prob, n // 10)
        known = (d.floor_flags & FL.UNKNOWN) == 0
        enough = ((d.visibility_flags & VS.UNMEASURED) == 0) & (d.visibility_profile[:, VS.THROUGH] + d.visibility_profile[:, VS.INSIDE] >= MIN_RAYS)
        self.G = between(np.abs(d.floor_gap[known]), int(known.sum()) - n // 12)
        self.F = between(d.see_through[enough], int(enough.sum()) - n // 12)
        # the conditions (module text), from the same run: the limits do not change a measure
        bad = [~(d.reproj_iou >= self.T), ~(d.mask_in_box >= self.M), ~(d.seg_box_iou >= self.S), ~(d.view_iou >= self.A), ~(d.rescore_prob >= self.P),
               known & (np.abs(d.floor_gap) > self.G), enough & (d.see_through > self.F)]
        with np.errstate(invalid='ignore'):
            spared = (~enough & (d.see_through > self.F)) | ~known
        self.conditions = {'n': n, 'rejected_by': [int(b.sum()) for b in bad], 'rejected_by_two': int((np.sum(bad, 0) >= 2).sum()),
                           'accepted': int((np.sum(bad, 0) == 0).sum()), 'spared': int(spared.sum())}

    def limits(self):
        return {'<%s>' % k: getattr(self, k) for k in 'TMSAPGF'}

    def fill(self, v, out=None):
        """An argv entry or keyword value with its placeholder filled in."""
        if not isinstance(v, str):
            return v
        if v in self.limits() and out is None:                  # (a keyword)
            return self.limits()[v]
        for k, w in list(self.limits().items()) + [('<model>', self.model), ('<root>', self.root)]:
            v = v.replace(k, w if isinstance(w, str) else repr(w))
        for k in ('res', 'json', 'vis', 'floor', 'auto'):
            v = v.replace('<%s>' % k, os.path.join(out or self.root, k))
        return v

    def argv(self):
        import detect_check as DC
        return ['--dataset_dir', self.root, '--idx_path', self.idx, '--rgb_detection_path', self.folder2] + DC.MODEL_FLAGS


_WORLD = []


def world():
    """One World per process (the directory lives as long as the process)."""
    if not _WORLD:
        tmp = tempfile.TemporaryDirectory()
        _WORLD.extend([World(tmp.name), tmp])
    return _WORLD[0]


def files_of(w, out):
    got = D.files_of(w, out)
    if os.path.exists(os.path.join(out, 'floor')):
        got['floor_json'] = text_of(open(os.path.join(out, 'floor')).read())
    return got


def record_main(name):
    """detect.main with RUNS[name] and --result_dir."""
    from transferable3d_amd import detect as DT
    w = world()
    out = tempfile.mkdtemp(dir=w.root)
    lines = []
    DT.main(w.argv() + [w.fill(a, out) for a in ['--result_dir', '<res>'] + RUNS[name]], rt=runtime(), log=lambda line: lines.append(w.tidy(line, out)))
    return dict(files_of(w, out), log=lines)


def record_detect(name):
    """Detector(**KEYWORDS[name]).detect(...) on the doubled detections -> its log and, per scene, its records."""
    from transferable3d_amd import detect as DT
    w = world()
    lines = []
    det = DT.Detector(w.flags(), rt=runtime(), log=lambda line: lines.append(w.tidy(line)), **{k: w.fill(v) for k, v in KEYWORDS[name].items()})
    return {'records': [text_of('\n'.join(record_of(r) for r in recs)) for recs in det.detect(w.scenes, w.doubled, scene_ids=w.ids)], 'log': lines}


def record_autolabel():
    from transferable3d_amd import autolabel as AL
    import detect_check as DC
    w = world()
    out = tempfile.mkdtemp(dir=w.root)
    lines = []
    argv = ['--dataset_dir', w.root, '--idx_path', w.idx, '--classes'] + w.classes + ['--out_dir', os.path.join(out, 'auto')] + [w.fill(a, out) for a in AUTOLABEL]
    s = AL.main(argv + DC.MODEL_FLAGS, rt=runtime(), log=lambda line: lines.append(w.tidy(line, out)))
    read = lambda *path: text_of(open(os.path.join(out, 'auto', *path)).read())
    folder = os.path.join(out, 'auto', 'training', 'label_dimension')
    return {'log': lines, 'autolabel_json': read('autolabel.json'), 'idx': read('training', 'autolabel_idx.txt'),
            'labels': {f: read('training', 'label_dimension', f) for f in sorted(os.listdir(folder))},
            'floor_json': text_of(open(os.path.join(out, 'floor')).read()), 'records': [record_of(hashed(r, 'label_corners')) for r in s['_records']],
            'summary_keys': list(s)}


def hashed(r, key):
    """The record with the array under `key` (where it has one) as the head of its SHA-256, in its place among the keys."""
    return dict(r, **{key: D.sha(np.ascontiguousarray(r[key]).tobytes())[:16]}) if key in r else r


def record_errors():
    from transferable3d_amd import autolabel as AL, detect as DT
    import detect_check as DC
    w = world()
    needed = ['--dataset_dir', w.root, '--idx_path', 'none', '--rgb_detection_path', 'none']
    base = ['--idx_path', 'none', '--classes', 'chair', '--out_dir', 'none']
    out = {'detect': [], 'autolabel': []}
    for argv in ERRORS:
        out['detect'].append([' '.join(argv), w.tidy(D.error_of(lambda: DT.main(needed + argv + DC.MODEL_FLAGS, log=lambda *a: None)))])
        if '--sweep' not in argv and '--rescore_fit' not in argv:          # (flags of detect alone)
            out['autolabel'].append([' '.join(argv), w.tidy(D.error_of(lambda: AL.parse(base + argv + DC.MODEL_FLAGS)))])
    return out


def thresholds_of(w):
    return dict({k: repr(getattr(w, k)) for k in 'TMSAPGF'}, conditions=w.conditions)


def main():
    w = world()
    out = {'thresholds': thresholds_of(w), 'main': {}, 'detect': {}}
    print(out['thresholds'])
    for name in RUNS:
        out['main'][name] = record_main(name)
        print('main %s:' % name)
        for line in out['main'][name]['log']:
            print('   ', line)
    for name in KEYWORDS:
        out['detect'][name] = record_detect(name)
        print('detect %s: records of %d scenes' % (name, len(out['detect'][name]['records'])))
    out['autolabel'] = record_autolabel()
    for line in out['autolabel']['log']:
        print('   ', line)
    out['errors'] = record_errors()
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
