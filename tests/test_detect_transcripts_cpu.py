"""CPU: what detect.main, Detector.detect and the two-step route of semisup_infer write, log, return and refuse behind
t3d_detect_decode -- log lines, result files, --consistency_json, legends, pictures, records, the 14-list, argument errors, option
attributes -- against the recording made before the stages' options and record fields got one owner each
(tests/golden/make_detect_transcripts.py, which also holds the runs and the recorder).  No tolerance: texts and hashes are compared.
There is no GPU counterpart: the device's last bits differ from the fp64 specification's, so a CPU recording cannot be replayed there."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_detect_transcripts', os.path.join(GOLDEN, 'make_detect_transcripts.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(G.OUT) as _f:
    Z = json.load(_f)


def same(got, want, what):
    """Equal as json writes them (1 != 1.0 != true, unlike ==), reported leaf by leaf."""
    if isinstance(want, dict) and isinstance(got, dict):
        assert sorted(got) == sorted(want), what
        for k in want:
            same(got[k], want[k], '%s / %s' % (what, k))
    elif isinstance(want, list) and isinstance(got, (list, tuple)):
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, '%s / %d' % (what, i))
        assert len(got) == len(want), what
    else:
        assert json.dumps(got) == json.dumps(want), what


def test_the_thresholds_reject_some_detections_and_not_all():
    w = G.world()
    same({'T': repr(w.T), 'A': repr(w.A), 'P': repr(w.P), 'n': w.n}, Z['thresholds'], 'thresholds')
    for name, measure in (('consistency', 'reproj_iou'), ('tta', 'view_iou'), ('rescore', 'rescore_prob')):
        line = [l for l in Z['main'][name]['log'] if l.startswith('consistency: kept')][0]
        kept, n = (int(v) for v in line.split()[2:5:2])
        assert 0 < kept < n == w.n and measure + ' <' in line, line


@pytest.mark.parametrize('name', sorted(G.RUNS))
def test_detect_main_reproduces_its_transcript(name):
    assert sorted(Z['main']) == sorted(G.RUNS)
    got = G.record_main(name)
    same(got, Z['main'][name], name)
    assert got['results'] and (('--vis_dir' in G.RUNS[name][1]) == bool(got.get('png'))) and (('--consistency_json' in G.RUNS[name][1]) == ('consistency_json' in got))


@pytest.mark.parametrize('name', sorted(G.KEYWORDS))
def test_detector_keeps_its_attributes_and_its_records(name):
    assert sorted(Z['detect']) == sorted(G.KEYWORDS)
    got = G.record_detect(name)
    same(got, Z['detect'][name], name)
    assert (name in G.DETECT) == bool(got.get('records')) and sorted(got['attributes']) == sorted(G.ATTRIBUTES)


@pytest.mark.parametrize('name', ['plain'] + sorted(G.TWO_STEP))
def test_the_two_step_route_reproduces_its_transcript(name):
    assert sorted(Z['two_step']) == sorted(['plain'] + list(G.TWO_STEP))
    same(G.record_two_step(name), Z['two_step'][name], name)


def test_argument_errors_and_which_of_two_is_reported():
    got = G.record_errors()
    for key in ('detect', 'build_flags'):
        for (argv, g), (_, w) in zip(got[key], Z['errors'][key]):
            assert g == w, (key, argv)
        assert [a for a, _ in got[key]] == [a for a, _ in Z['errors'][key]]
    assert all(m.startswith('argument error: ') for _, m in got['detect'])           # detect.main accepts none of them


def test_build_flags_keeps_its_attributes():
    same(G.record_namespaces(), Z['namespaces'], 'namespaces')
