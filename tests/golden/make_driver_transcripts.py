"""Generates tests/golden/driver_transcripts.json: what the three training drivers (train_semisup, train_boxpc, train_semisup_adv) DO,
seen from outside, on the CPU with the NumPy specification library (`python tests/golden/make_driver_transcripts.py`).  Recorded at the
commit BEFORE the drivers' common parts moved into train_common.py; tests/test_driver_transcripts_cpu.py replays the recording, so the
file is regenerated only when a driver's behaviour is changed on purpose -- never to make a refactor pass.

The drivers are driven through their public interface only -- `build_flags(argv)`, `train(FLAGS, rt=Runtime(device='cpu',
lib=FakeLib()), log=...)` -- with `api.Session.run` wrapped.  Per run, the ordered events:
  ['run', number of fetches, number of fed placeholders, value fed to is_training or None]
  ['log', line]
  ['save', basename]       for every file that appears in log_dir (looked for after every run and before every log line)
Log lines are normalised as little as possible: the log_dir path becomes <log_dir>; every token that holds a decimal number, and `nan`,
becomes # (losses, APs and rates can differ in the last bit between CPUs); integers -- epochs, data-set lengths, supports -- stay.

Six runs: every driver on `--device_data 64` (12 / 12 / 6 steps: both halves of every fetch predicate, stage c's two-batch alternation)
and on `--synthetic` host batches (3 / 3 / 2 steps); two epochs, so that epoch 0 saves and epoch 1 does not.

Also recorded, per driver: the namespace `build_flags([])` returns, and the namespace of one argv that sets every lower-case option
the driver's parser knows to a non-default value (the option list is taken from the parser `config.make_parser` hands the driver).
That pins "same flags, same defaults, same types".
"""
import argparse
import importlib
import json
import os
import re
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, 'driver_transcripts.json')
DRIVERS = {'a': 'transferable3d_amd.train_semisup', 'b': 'transferable3d_amd.train_boxpc', 'c': 'transferable3d_amd.train_semisup_adv'}
# the per-driver model flags of tests/test_train_cli_and_dp.py
MODEL_ARGV = {
    'a': ['--SEMI_MODEL', 'A', '--WEAK_WEIGHT_REPROJECTION', '0', '--WEAK_WEIGHT_SURFACE', '0'],
    'b': ['--BOX_PC_MASK_REPRESENTATION', 'A', '--BOXPC_WEIGHT_DELTA', '4'],
    'c': ['--SEMI_MODEL', 'F', '--BOX_PC_MASK_REPRESENTATION', 'A', '--use_one_hot', '--SEMI_TRAIN_BOX_TRAIN_CLASS_AG_TNET', '1',
          '--SEMI_TRAIN_BOX_TRAIN_CLASS_AG_BOX', '1', '--SEMI_BOXPC_FIT_ONLY_ON_2D_CLS', '1', '--WEAK_WEIGHT_INTRACLASSVAR', '2',
          '--WEAK_WEIGHT_REPROJECTION', '0', '--SEMI_MULTIPLIER_FOR_WEAK_LOSS', '0.05', '--SUNRGBD_SEMI_TEST_CLS', 'table', 'sofa',
          'dresser', 'night_stand', 'bookshelf'],
}
SMALL = ['--num_point', '128', '--batch_size', '4', '--num_channels', '4', '--max_epoch', '2', '--eval_batches', '1']
DEVICE_STEPS = {'a': 12, 'b': 12, 'c': 6}
HOST_STEPS = {'a': 3, 'b': 3, 'c': 2}
RUNS = {}
for _d in 'abc':
    RUNS[_d + '_device'] = (_d, MODEL_ARGV[_d] + SMALL + ['--device_data', '64', '--steps_per_epoch', str(DEVICE_STEPS[_d])])
    RUNS[_d + '_host'] = (_d, MODEL_ARGV[_d] + SMALL + ['--synthetic', '--steps_per_epoch', str(HOST_STEPS[_d])])

_NUMBER = re.compile(r'\S*\d\.\d\S*|\bnan\b')


def normalise(line, log_dir):
    return _NUMBER.sub('#', str(line).replace(log_dir, '<log_dir>'))


def driver(d):
    return importlib.import_module(DRIVERS[d])


def record_run(name):
    """The events of RUNS[name]: a list of lists, as json gives them back."""
    from fake_t3d import FakeLib
    from transferable3d_amd import api
    from transferable3d_amd.engine import Runtime
    d, argv = RUNS[name]
    T = driver(d)
    events, seen = [], set()
    real_run = api.Session.run

    with tempfile.TemporaryDirectory() as log_dir:
        def new_files():
            for f in sorted(set(os.listdir(log_dir)) - seen):
                seen.add(f)
                events.append(['save', f])

        def run(self, fetches, feed_dict=None):
            out = real_run(self, fetches, feed_dict)
            mode = [bool(v) for pl, v in (feed_dict or {}).items() if isinstance(pl, api.BoolPlaceholder)]
            events.append(['run', len(fetches) if isinstance(fetches, (list, tuple)) else 1, len(feed_dict or {}), mode[0] if mode else None])
            new_files()
            return out

        def log(line):
            new_files()
            events.append(['log', normalise(line, log_dir)])
        api.Session.run = run
        try:
            T.train(T.build_flags(argv + ['--log_dir', log_dir]), rt=Runtime(device='cpu', lib=FakeLib()), log=log)
        finally:
            api.Session.run = real_run
        new_files()
    return events


def namespace_of(d, argv):
    """vars(build_flags(argv)) through json: str / int / float / bool / list / None keep their types."""
    return json.loads(json.dumps(vars(driver(d).build_flags(list(argv))), sort_keys=True))


def every_lower_case_option(d):
    """One argv that sets every lower-case option of driver d's parser to a value that is not its default."""
    T = driver(d)
    parsers, real = [], T.make_parser

    def capture():
        parsers.append(real())
        return parsers[-1]
    T.make_parser = capture
    try:
        T.build_flags([])
    finally:
        T.make_parser = real
    argv = []
    for a in parsers[0]._actions:
        opt = next((o for o in a.option_strings if o.startswith('--')), None)
        if opt is None or opt == '--help' or opt != opt.lower():
            continue
        if isinstance(a, argparse._StoreTrueAction):
            argv += [opt]
        elif a.choices:
            argv += [opt, [c for c in a.choices if c != a.default][0]]
        elif a.type is int:
            argv += [opt, str((a.default or 0) + 3)]
        elif a.type is float:
            argv += [opt, '0.25']                 # (inside [-1, 1], which the probability flags demand; no float default is 0.25)
        else:
            argv += [opt, 'other_' + a.dest]
    return argv


def main():
    out = {'runs': {}, 'flags': {}}
    for name in RUNS:
        out['runs'][name] = {'argv': RUNS[name][1], 'events': record_run(name)}
        print('%s: %d events' % (name, len(out['runs'][name]['events'])))
    for d in 'abc':
        argv = every_lower_case_option(d)
        out['flags'][d] = {'default': namespace_of(d, []), 'argv': argv, 'set': namespace_of(d, argv)}
        print('%s: %d options set' % (DRIVERS[d], sum(a.startswith('--') for a in argv)))
    with open(OUT, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
