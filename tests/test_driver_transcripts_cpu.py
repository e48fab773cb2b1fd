"""CPU: the observable sequence of the three training drivers -- every Session.run (fetches, fed placeholders, the mode fed), every log
line, every file that appears in log_dir, in order -- and the namespaces their build_flags return, against the recording made before
the drivers' common parts moved into train_common.py (tests/golden/make_driver_transcripts.py, which also holds the recorder)."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_driver_transcripts', os.path.join(GOLDEN, 'make_driver_transcripts.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(G.OUT) as _f:
    Z = json.load(_f)


@pytest.mark.parametrize('name', sorted(G.RUNS))
def test_driver_reproduces_its_transcript(name):
    assert Z['runs'][name]['argv'] == G.RUNS[name][1]          # the recording is of this command line
    want, got = Z['runs'][name]['events'], G.record_run(name)
    for i, (w, g) in enumerate(zip(want, got)):
        assert w == g, 'event %d of %s' % (i, name)
    assert len(got) == len(want)
    # both halves of the run are there: training steps, an evaluation after each of the two epochs, one checkpoint (epoch 0 only)
    assert sum(e[0] == 'run' and e[3] is False for e in got) == 2
    assert [e[1] for e in got if e[0] == 'save'] == ['model_epoch_0.npz']


@pytest.mark.parametrize('d', 'abc')
def test_build_flags_accepts_the_same_flags_with_the_same_defaults_and_types(d):
    z = Z['flags'][d]
    same = lambda a, b: json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)      # (1 != 1.0 != true, unlike ==)
    for key, argv in (('default', []), ('set', z['argv'])):
        got = G.namespace_of(d, argv)
        assert sorted(got) == sorted(z[key])
        for k in got:
            assert same(got[k], z[key][k]), (key, k, got[k], z[key][k])
