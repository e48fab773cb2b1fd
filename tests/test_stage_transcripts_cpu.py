"""CPU: what detect.main, Detector.detect and autolabel.main write, log, return and refuse with the floor stage, the visibility stage
and all seven rejecting tests at once -- log lines, result files, --consistency_json, --floor_json, legends, pictures, records,
autolabel.json, label files, argument errors -- against the recording made before each rejecting test was stated once
(tests/golden/make_stage_transcripts.py, which also holds the runs).  The recorder and `same` are those of the detect transcripts.
No tolerance: texts and hashes are compared.  There is no GPU counterpart, for the reason given there."""
import importlib.util
import json
import os
import re

import pytest

from test_detect_transcripts_cpu import same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_stage_transcripts', os.path.join(GOLDEN, 'make_stage_transcripts.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(G.OUT) as _f:
    Z = json.load(_f)

FRAGMENTS = ('reproj_iou <', 'mask_in_box <', 'seg_box_iou <', 'view_iou <', 'rescore_prob <', '|floor_gap| >', 'see_through >')


def test_every_test_rejects_some_detections_two_reject_one_and_some_are_accepted_or_spared():
    w = G.world()
    same(G.thresholds_of(w), Z['thresholds'], 'thresholds')
    log = Z['main']['all_seven']['log']
    line = [l for l in log if l.startswith('consistency: kept')][0]
    kept, n = (int(v) for v in line.split()[2:5:2])
    parts = line[line.index('(') + 1:-1].split(', ')
    assert [p.startswith(f) for p, f in zip(parts, FRAGMENTS)] == [True] * 7 == [True] * len(parts), line      # the order of the fragments
    counts = [int(p.rsplit(': ', 1)[1]) for p in parts]
    c = Z['thresholds']['conditions']
    assert counts == c['rejected_by'] and min(counts) >= 1, line
    assert n == c['n'] == w.n and 1 <= kept == c['accepted'] < n
    assert sum(counts) > n - kept and c['rejected_by_two'] >= 1, 'a detection is rejected by two tests at once'
    assert c['spared'] >= 1, 'a box beyond a limit that its test does not reject: too few rays, not measured, or no floor'
    assert [l.split(':')[0].split(' ')[0] for l in log[:5]] == ['consistency', 'tta', 'floor', 'visibility', 'nms'], log
    assert int(re.search(r'rejected (\d+) \(', log[2]).group(1)) == counts[5] and int(log[3].rsplit('rejected ', 1)[1]) == counts[6]
    for name, fragment in (('snap', FRAGMENTS[5]), ('see_through', FRAGMENTS[6])):
        line = [l for l in Z['main'][name]['log'] if l.startswith('consistency: kept')][0]
        kept, n = (int(v) for v in line.split()[2:5:2])
        assert 0 < kept < n == w.n and fragment in line, line
    by = json.dumps(Z['autolabel']['log'])
    assert all('(%s: ' % f in by for f in ('min_reproj_iou', 'min_mask_in_box', 'min_seg_box_iou', 'min_view_iou', 'min_rescore', 'max_floor_gap', 'max_see_through'))
    assert 'rejected by --max_floor_gap' in by and 'rejected by --max_see_through' in by and 'rejected by --min_view_iou' in by


@pytest.mark.parametrize('name', sorted(G.RUNS))
def test_detect_main_reproduces_its_transcript(name):
    assert sorted(Z['main']) == sorted(G.RUNS)
    got = G.record_main(name)
    same(got, Z['main'][name], name)
    assert got['results'] and (('--vis_dir' in G.RUNS[name]) == bool(got.get('png'))) and (('--consistency_json' in G.RUNS[name]) == ('consistency_json' in got))
    assert ('--floor_json' in G.RUNS[name]) == ('floor_json' in got)


@pytest.mark.parametrize('name', sorted(G.KEYWORDS))
def test_detector_keeps_its_records(name):
    assert sorted(Z['detect']) == sorted(G.KEYWORDS)
    got = G.record_detect(name)
    same(got, Z['detect'][name], name)
    assert len(got['records']) == G.SCENES and all(got['records']) and got['log'] == Z['main'][name]['log'][:len(got['log'])]


def test_autolabel_reproduces_its_transcript():
    got = G.record_autolabel()
    same(got, Z['autolabel'], 'autolabel')
    assert got['labels'] and len(got['records']) > len(got['labels']) and 'visibility_evidence: int' in json.dumps(got['records'])


def test_argument_errors_and_which_of_two_is_reported():
    got = G.record_errors()
    for key in ('detect', 'autolabel'):
        for (argv, g), (_, w) in zip(got[key], Z['errors'][key]):
            assert g == w, (key, argv)
        assert [a for a, _ in got[key]] == [a for a, _ in Z['errors'][key]]
    assert all(m.startswith('argument error: ') for _, m in got['detect']) and len(got['detect']) == len(G.ERRORS)      # detect.main accepts none of them
