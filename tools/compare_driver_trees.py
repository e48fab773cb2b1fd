#!/usr/bin/env python3
"""Do the three training drivers of two source trees behave the same, exactly?  Every run of tests/golden/make_driver_transcripts.py
(each driver on --device_data and on --synthetic host batches) is made once per tree, each in a fresh process, and compared with no
tolerance: every log line (only the frustums/s figure and the log_dir path are masked), the returned loss, and every array of every
model_epoch_*.npz and of the returned state dict, byte for byte.  The path has no float atomics, so a difference
is a difference in the code.

  python tools/compare_driver_trees.py TREE_A TREE_B --out DIR [--cpu | --gpu]
    --cpu   the NumPy specification library (tests/fake_t3d.py of each tree); adds a two-rank stage-c run on gloo
    --gpu   the built library of each tree on the GPU, --dtype f32; adds stage a under --dtype bf16 and the three-stage hand-over
            (stage c started from the model_epoch_0.npz of the same tree's stage-a and stage-b device runs)
Every run is its own process under its own `timeout`; the first run that fails ends the comparison (nothing more is started, exit
status 2).  Exit status 0: no difference; 1: differences, listed."""
import argparse
import importlib.util
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RATE = re.compile(r'\(\S+ frustums/s')


def runs_of(mode):
    spec = importlib.util.spec_from_file_location('make_driver_transcripts', os.path.join(HERE, '..', 'tests', 'golden', 'make_driver_transcripts.py'))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    # the built library's Box-PC kernels take whole 256-row tiles per frustum (t3d_boxpc_rep): 256 points on the GPU, the recording's 128 on the CPU
    size = ['--num_point', '256'] if mode == 'gpu' else []
    runs = [(name, d, argv + size + ['--dtype', 'f32'], 1, {}) for name, (d, argv) in sorted(G.RUNS.items())]
    if mode == 'gpu':
        runs.append(('a_device_bf16', 'a', G.RUNS['a_device'][1] + size + ['--dtype', 'bf16'], 1, {}))
        runs.append(('c_handover', 'c', G.RUNS['c_device'][1] + size + ['--dtype', 'f32'], 1,
                     {'--init_class_ag_path': 'a_device', '--init_boxpc_path': 'b_device'}))
    else:
        runs.append(('c_host_2ranks', 'c', G.RUNS['c_host'][1] + ['--dtype', 'f32'], 2, {}))
    return G.DRIVERS, runs


def worker(tree, module, mode, out, argv):
    """One run in this process: out/log.json, out/loss.txt, out/final.npz, out/log_dir/."""
    tree = os.path.abspath(tree)
    sys.path[:0] = [tree, os.path.join(tree, 'tests')]
    import importlib
    T = importlib.import_module(module)
    assert os.path.abspath(T.__file__).startswith(tree + os.sep), T.__file__
    rt = None
    if mode == 'cpu':
        from fake_t3d import FakeLib
        from transferable3d_amd.engine import Runtime
        rt = Runtime(device='cpu', lib=FakeLib())
    log_dir, lines = os.path.join(out, 'log_dir'), []
    final, loss = T.train(T.build_flags(argv + ['--log_dir', log_dir]), rt=rt, log=lambda line: lines.append(str(line)))
    with open(os.path.join(out, 'log.json'), 'w') as f:
        json.dump([RATE.sub('(# frustums/s', l.replace(log_dir, '<log_dir>')) for l in lines], f, indent=0)
    with open(os.path.join(out, 'loss.txt'), 'w') as f:
        f.write(float(loss).hex() + '\n')
    np.savez(os.path.join(out, 'final.npz'), **final)


def launch(tree, module, mode, out, argv, ranks, limit):
    procs = []
    port = socket.socket()
    port.bind(('127.0.0.1', 0))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port.getsockname()[1]))
    port.close()
    for r in range(ranks):
        o = os.path.join(out, 'rank%d' % r) if ranks > 1 else out
        os.makedirs(o, exist_ok=True)
        if ranks > 1:
            env = dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(ranks))
        procs.append(subprocess.Popen(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--worker', tree, module, mode, o]
                                      + argv, env=env, stdout=subprocess.DEVNULL))
    return [p.wait() for p in procs]


def arrays_differ(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            bad.append(k)
    return len(a.files), bad


def compare(da, db):
    """(number of things compared, list of differences) of two run directories."""
    n, diffs = 0, []
    for sub in sorted(d for d in os.listdir(da) if d.startswith('rank')) or ['']:
        a, b = os.path.join(da, sub), os.path.join(db, sub)
        la, lb = json.load(open(os.path.join(a, 'log.json'))), json.load(open(os.path.join(b, 'log.json')))
        n += max(len(la), len(lb)) + 1
        diffs += ['%s log line %d: %r != %r' % (sub, i, x, y) for i, (x, y) in enumerate(zip(la, lb)) if x != y]
        if len(la) != len(lb):
            diffs.append('%s: %d log lines != %d' % (sub, len(la), len(lb)))
        if open(os.path.join(a, 'loss.txt')).read() != open(os.path.join(b, 'loss.txt')).read():
            diffs.append('%s: returned loss differs' % sub)
        fa, fb = sorted(os.listdir(os.path.join(a, 'log_dir'))), sorted(os.listdir(os.path.join(b, 'log_dir')))
        if fa != fb:
            diffs.append('%s: files in log_dir %s != %s' % (sub, fa, fb))
        for f in ['final.npz'] + [os.path.join('log_dir', f) for f in fa if f in fb and f.endswith('.npz')]:
            k, bad = arrays_differ(os.path.join(a, f), os.path.join(b, f))
            n += k
            diffs += ['%s %s: array %s differs' % (sub, f, name) for name in bad]
    return n, diffs


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--worker':
        return worker(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6:])
    p = argparse.ArgumentParser()
    p.add_argument('trees', nargs=2)
    p.add_argument('--out', required=True)
    p.add_argument('--gpu', action='store_true')
    p.add_argument('--cpu', action='store_true')
    p.add_argument('--timeout', type=int, default=240, help='seconds per run')
    a = p.parse_args()
    mode = 'gpu' if a.gpu else 'cpu'
    drivers, runs = runs_of(mode)
    total = 0
    for name, d, argv, ranks, handed in runs:
        dirs = []
        for tag, tree in zip('AB', a.trees):
            out = os.path.join(os.path.abspath(a.out), mode, tag, name)
            extra = [x for flag, src in handed.items() for x in (flag, os.path.join(os.path.dirname(out), src, 'log_dir', 'model_epoch_0.npz'))]
            codes = launch(tree, drivers[d], mode, out, argv + extra, ranks, a.timeout)
            if any(codes):
                print('%s in %s: exit status %s -- stopped, nothing more is started' % (name, tree, codes))
                sys.exit(2)
            dirs.append(out)
        n, diffs = compare(*dirs)
        total += len(diffs)
        print('%-14s %s: %4d items compared (log lines, loss, arrays), %d differ' % (name, mode, n, len(diffs)), flush=True)
        for line in diffs[:10]:
            print('    ' + line)
    print('TOTAL: %d differences' % total)
    sys.exit(1 if total else 0)


if __name__ == '__main__':
    main()
