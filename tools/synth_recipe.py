#!/usr/bin/env python3
"""The recipe on generated scenes, end to end, with a known answer: generate a training and a validation split
(transferable3d_amd.synth_scenes), extract their frustum files from memory, train stage a (train_semisup --SEMI_MODEL A, the paper's
split: 3-D labels for bed chair toilet desk bathtub, 2-D labels only for table sofa dresser night_stand bookshelf) from
--frustum_file, then run `detect --official_eval --diagnose` on the validation scenes and the simulated 2-D detections: once plain and
once each with --nms_iou 0.25, --nms_iou 0.25 --nms_fuse, --soft_nms gaussian and --tta 4; then three runs with --diagnose_parts, which
splits `loc` into xy, z, centre, size and heading: plain, --snap_floor shift, --snap_floor stretch, --visibility (which measures and
must leave every AP as the plain row has it) and --max_see_through 0.5.

Every step is a fresh child process under its own `timeout -k 10`; the tool stops at the first non-zero status and retries nothing.  The
sizes are chosen so that the whole run takes minutes and are written into the record.  Writes profiles/synth_recipe.json (`--out`): the
sizes, per run the AP of every class, the mean AP, the mean dAP per fix (dup, loc, bkg among them) and, of the runs with
--diagnose_parts, the mean dAP of `loc` per part (mean_dAP_parts), and the last evaluation lines
of the training log.  The scenes are synthetic: the numbers say what the pipeline does on a problem with a known answer, not what it does
on SUN-RGBD.

  python tools/synth_recipe.py [--work DIR] [--train_scenes 320] [--val_scenes 80] [--epochs 6]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']
RUNS = [('plain', []), ('nms', ['--nms_iou', '0.25']), ('nms_fuse', ['--nms_iou', '0.25', '--nms_fuse']), ('soft_nms', ['--soft_nms', 'gaussian']),
        ('tta4', ['--tta', '4']), ('parts', ['--diagnose_parts']), ('floor_shift', ['--snap_floor', 'shift', '--diagnose_parts']),
        ('floor_stretch', ['--snap_floor', 'stretch', '--diagnose_parts']), ('visibility', ['--visibility', '--diagnose_parts']),
        ('max_see_through', ['--max_see_through', '0.5', '--diagnose_parts'])]


def step(name, seconds, argv, log_path, steps):
    """One child process under `timeout -k 10 seconds`; its output goes to log_path.  Raises SystemExit on a non-zero status."""
    cmd = ['timeout', '-k', '10', str(int(seconds)), sys.executable, '-m'] + argv
    t0 = time.time()
    with open(log_path, 'w') as fh:
        rc = subprocess.call(cmd, cwd=ROOT, stdout=fh, stderr=subprocess.STDOUT)
    steps.append({'step': name, 'seconds': round(time.time() - t0, 1), 'limit_s': int(seconds), 'status': rc})
    print('%s: status %d after %.1f s' % (name, rc, steps[-1]['seconds']), flush=True)
    if rc != 0:
        tail = open(log_path).read().splitlines()[-15:]
        raise SystemExit('%s ended with status %d (no retry); the end of %s:\n%s' % (name, rc, log_path, '\n'.join(tail)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--work', default=os.path.join(ROOT, 'build', 'synth_recipe'), help='where the data, the logs and the checkpoints go (build/ is not tracked)')
    ap.add_argument('--train_scenes', type=int, default=320)
    ap.add_argument('--val_scenes', type=int, default=80)
    ap.add_argument('--width', type=int, default=365)
    ap.add_argument('--height', type=int, default=265)
    ap.add_argument('--stride', type=int, default=2)
    ap.add_argument('--num_point', type=int, default=512)
    ap.add_argument('--epochs', type=int, default=6, help='stage a trains this many epochs; checkpoints are written after epochs 0, 5, 10, ...')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synth_recipe.json'))
    a = ap.parse_args()
    if (a.epochs - 1) % 5 != 0:
        raise SystemExit('--epochs must be 1, 6, 11, ...: the last epoch then writes the checkpoint detect reads')
    work = os.path.abspath(a.work)
    os.makedirs(work, exist_ok=True)
    size = ['--width', str(a.width), '--height', str(a.height), '--stride', str(a.stride), '--seed', str(a.seed)]
    train, val = os.path.join(work, 'train'), os.path.join(work, 'val')
    steps, runs, failure = [], {}, None
    log_a = os.path.join(work, 'a')
    try:
        step('generate_train', 420, ['transferable3d_amd.synth_scenes', '--out', train, '--scenes', str(a.train_scenes), '--first_id', '1',
                                     '--val_share', '0', '--frustum_dir', os.path.join(train, 'frustums'), '--no_files'] + size,
             os.path.join(work, 'generate_train.log'), steps)
        step('generate_val', 300, ['transferable3d_amd.synth_scenes', '--out', val, '--scenes', str(a.val_scenes), '--first_id', '100001',
                                   '--val_share', '1', '--frustum_dir', os.path.join(val, 'frustums')] + size,
             os.path.join(work, 'generate_val.log'), steps)
        step('train_a', 600, ['transferable3d_amd.train_semisup', '--SEMI_MODEL', 'A', '--WEAK_WEIGHT_REPROJECTION', '0', '--WEAK_WEIGHT_SURFACE', '0',
                              '--frustum_file', os.path.join(train, 'frustums', 'train_aug5x.zip.pickle'),
                              '--eval_file', os.path.join(val, 'frustums', 'val.zip.pickle'), '--num_point', str(a.num_point), '--batch_size', '32',
                              '--max_epoch', str(a.epochs), '--log_dir', log_a, '--seed', str(a.seed)],
             os.path.join(work, 'train_a.log'), steps)
        model = os.path.join(log_a, 'model_epoch_%d.npz' % (a.epochs - 1))
        for name, flags in RUNS:
            dj = os.path.join(work, 'diagnose_%s.json' % name)
            step('detect_' + name, 300, ['transferable3d_amd.detect', '--dataset_dir', val, '--idx_path', os.path.join(val, 'training', 'val_data_idx.txt'),
                                         '--rgb_detection_path', os.path.join(val, 'det'), '--model_path', model, '--semi_type', 'A', '--pred_prefix', '',
                                         '--num_point', str(a.num_point), '--SUNRGBD_SEMI_TEST_CLS'] + CLASSES +
                 ['--official_eval', '--test_on', 'AB', '--diagnose', '--diagnose_json', dj, '--seed', str(a.seed)] + flags,
                 os.path.join(work, 'detect_%s.log' % name), steps)
            doc = json.load(open(dj))
            runs[name] = {'flags': flags, 'ap': {c: doc['classes'][c]['ap'] for c in CLASSES}, 'mean_ap': doc['mean_ap'], 'mean_dAP': doc['mean_dAP'],
                          'predictions': {c: doc['classes'][c]['predictions'] for c in CLASSES}}
            if 'mean_dAP_parts' in doc:
                runs[name]['mean_dAP_parts'] = doc['mean_dAP_parts']
            for stage in ('floor', 'visibility'):
                line = [l.strip() for l in open(os.path.join(work, 'detect_%s.log' % name)) if l.startswith(stage + ':')]
                if line:
                    runs[name][stage] = line[-1]
    except SystemExit as e:          # the record says how far the run came
        failure = str(e)
    train_log = os.path.join(work, 'train_a.log')
    last_eval = [l.strip() for l in (open(train_log).read().splitlines() if os.path.exists(train_log) else []) if 'eval' in l or 'Mean AP' in l][-7:]
    synth = {k: json.load(open(os.path.join(d, 'synth.json'))) for k, d in (('train', train), ('val', val)) if os.path.exists(os.path.join(d, 'synth.json'))}
    rec = {'synthetic': True, 'seed': a.seed, 'train_scenes': a.train_scenes, 'val_scenes': a.val_scenes, 'width': a.width, 'height': a.height,
           'stride': a.stride, 'num_point': a.num_point, 'epochs': a.epochs, 'classes_with_3d_labels': ['bed', 'chair', 'toilet', 'desk', 'bathtub'],
           'class_counts': {k: v['class_counts'] for k, v in synth.items()}, 'generator_flags': synth.get('val', {}).get('flags'),
           'steps': steps, 'training_last_evaluation': last_eval, 'runs': runs}
    if failure is not None:
        rec['stopped'] = failure
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(rec, fh, indent=1)
        fh.write('\n')
    print(json.dumps({'mean_ap': {k: v['mean_ap'] for k, v in runs.items()}, 'seconds': sum(s['seconds'] for s in steps)}))
    if failure is not None:
        raise SystemExit(failure)


if __name__ == '__main__':
    main()
