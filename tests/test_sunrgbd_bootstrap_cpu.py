"""CPU: the bootstrap over images (t3d_bootstrap_weights, t3d_sunrgbd_eval_bootstrap, bootstrap.py, evaluate_sunrgbd --bootstrap /
--compare_pred_dir, detect --sweep --bootstrap) on the specification library (tests/fake_bootstrap.py), whose replicates are LITERAL
expansions of the resampled data set: the argument structs, every refusal of the built library and of the specification, hand cases
whose answers need no code, `summary` and `paired` on fixed arrays, the flags, and the two flows on the golden scenes."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_check as BC
import fake_bootstrap as FB
import nms_check as NC
import sunrgbd_eval_check as SC
import sweep_check as SW
from transferable3d_amd import abi, bootstrap as BS, detect as DT, evaluate_sunrgbd as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cpu_rt = BC.spec_rt


# ---- the argument structs ------------------------------------------------------------------------------------------------------------
def header_fields(name):
    h = open(os.path.join(ROOT, 'include', 't3d.h')).read()
    body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\}\s*%s;' % name, h).group(1), flags=re.S)
    return [re.findall(r'(\w+)(?:\[\d+\])?\s*$', part.strip())[0] for decl in body.split(';') if decl.strip() for part in decl.split(',')]


def test_structs_follow_the_header_and_the_compiler(tmp_path):
    assert 't3d_bootstrap_weights' in abi.ENTRY_POINTS and 't3d_sunrgbd_eval_bootstrap' in abi.ENTRY_POINTS
    assert header_fields('t3d_bootstrap_weights_args') == [f[0] for f in abi.BootstrapWeightsArgs._fields_]
    assert header_fields('t3d_sunrgbd_bootstrap_args') == [f[0] for f in abi.SunrgbdBootstrapArgs._fields_]
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "t3d.h"\nint main(void) { printf("%zu %d %zu %d %llu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(t3d_bootstrap_weights_args), T3D_V2_SIZE_bootstrap_weights_args, sizeof(t3d_sunrgbd_bootstrap_args), '
                   'T3D_V2_SIZE_sunrgbd_bootstrap_args, (unsigned long long)T3D_SUNRGBD_BOOTSTRAP_WORKSPACE_BYTES(1001), '
                   'offsetof(t3d_bootstrap_weights_args, weights), offsetof(t3d_sunrgbd_bootstrap_args, det_col), '
                   'offsetof(t3d_sunrgbd_bootstrap_args, workspace_bytes), offsetof(t3d_sunrgbd_bootstrap_args, n_fp), '
                   'T3D_BOOTSTRAP_MAX_REPLICATES, T3D_ABI_VERSION); return 0; }\n')
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'size')])
    v = [int(x) for x in subprocess.check_output([str(tmp_path / 'size')], text=True).split()]
    assert v[0] == v[1] == C.sizeof(abi.BootstrapWeightsArgs) == abi.BootstrapWeightsArgs().struct_size
    assert v[2] == v[3] == C.sizeof(abi.SunrgbdBootstrapArgs) == abi.SunrgbdBootstrapArgs().struct_size
    assert v[4] == abi.sunrgbd_bootstrap_workspace_bytes(1001) == 4012
    assert v[5] == abi.BootstrapWeightsArgs.weights.offset and v[6] == abi.SunrgbdBootstrapArgs.det_col.offset
    assert v[7] == abi.SunrgbdBootstrapArgs.workspace_bytes.offset and v[8] == abi.SunrgbdBootstrapArgs.n_fp.offset
    assert v[9] == abi.BOOTSTRAP_MAX_REPLICATES == BS.MAX_REPLICATES == FB.MAX_REPLICATES == 65536
    assert v[10] == abi.ABI_VERSION == 3                                    # the two entry points did not move the version


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def libs(which):
    return (abi.load() if which == 'built' else cpu_rt().lib), C.c_void_p(0)


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_weights_check_before_they_launch(which):
    """No GPU needed: everything below is refused before anything is launched, with the same answers by both libraries."""
    lib, null = libs(which)
    buf = (C.c_int32 * 64)()
    args = lambda **kw: abi.BootstrapWeightsArgs(**dict(dict(seed=1, R=3, n_images=7, stride=8, weights=C.cast(buf, abi.I)), **kw))
    call = lambda a: lib.t3d_bootstrap_weights(C.byref(a), null)
    a = args()
    a.struct_size -= 8
    assert call(a) == abi.ERR_ABI
    for bad in (dict(R=0), dict(R=-1), dict(R=65537), dict(n_images=0), dict(n_images=-3)):
        assert call(args(**bad)) == -2, bad                                  # T3D_ERR_SHAPE
    for bad in (dict(stride=6), dict(weights=None)):
        assert call(args(**bad)) == -1, bad                                  # T3D_ERR_ARG
    assert not any(buf)


def boot_args_pair(buf, P=4, G=2, **kw):
    d, i, u, l = C.cast(buf, abi.D), C.cast(buf, abi.I), C.cast(buf, abi.U8), C.cast(buf, abi.L)
    a = abi.SunrgbdEvalArgs(P=P, G=G, det_centroid=d, det_basis=d, det_coeffs=d, det_confidence=d, det_image=i, gt_centroid=d, gt_basis=d, gt_coeffs=d,
                            gt_image=i, n_images=1, image_ids=i, image_gt_offsets=i, image_gt=i, threshold=0.25, workspace=C.addressof(buf),
                            workspace_bytes=abi.sunrgbd_eval_workspace_bytes(P, G), order=i, max_overlap=d, gt_idx=i, is_tp=u, is_fp=u, gt_assignment=i,
                            is_missed=u, precision=d, recall=d, ap=d)
    b = abi.SunrgbdBootstrapArgs(R=3, weights=i, weight_stride=8, det_col=i, gt_col=i, workspace=C.addressof(buf),
                                 workspace_bytes=abi.sunrgbd_bootstrap_workspace_bytes(P), ap=d, n_pos=l, n_tp=l, n_fp=l)
    for k, v in kw.items():
        setattr(a if k in ('gt_difficult', 'ap_eval') else b, 'ap' if k == 'ap_eval' else k, v)
    return a, b


@pytest.mark.parametrize('which', ['built', 'specification'])
def test_the_evaluation_bootstrap_checks_before_it_launches(which):
    lib, null = libs(which)
    call = lambda a, b: lib.t3d_sunrgbd_eval_bootstrap(C.byref(a), C.byref(b), null)
    buf = (C.c_uint64 * 512)()
    a, b = boot_args_pair(buf)
    b.struct_size -= 8
    assert call(a, b) == abi.ERR_ABI
    a, b = boot_args_pair(buf)
    a.struct_size -= 8
    assert call(a, b) == abi.ERR_ABI
    for bad in (dict(R=0), dict(R=65537), dict(weight_stride=0), dict(weight_stride=(1 << 30) + 1)):
        assert call(*boot_args_pair(buf, **bad)) == -2, bad
    for bad in (dict(weights=None), dict(ap=None), dict(n_pos=None), dict(n_tp=None), dict(n_fp=None), dict(det_col=None), dict(gt_col=None),
                dict(workspace=None), dict(workspace_bytes=abi.sunrgbd_bootstrap_workspace_bytes(4) - 8), dict(workspace=C.addressof(buf) + 4),
                dict(gt_difficult=C.cast(buf, abi.U8)), dict(ap_eval=None)):
        assert call(*boot_args_pair(buf, **bad)) == -1, bad
    assert not any(buf)


def test_python_refusals():
    rt = cpu_rt()
    for bad in (dict(R=0), dict(R=65537), dict(n_images=0), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            BS.Weights(rt, **dict(dict(n_images=5, R=3, seed=0), **bad))
    shift = lambda x: SC.box(x, 5.0, 0.0, 1.0, 1.0, 1.0)
    det, gt = SC.stack([shift(0.0)], [4], [0.9]), SC.stack([shift(0.0)], [4])
    w = BS.Weights.of(rt, np.ones((2, 2), np.int32))
    assert list(ES.bootstrap_class('table', det, gt, w, [7, 4], rt=rt)['n_pos']) == [1, 1]
    with pytest.raises(ValueError, match='a detection of image 4'):
        ES.bootstrap_class('table', det, SC.stack([], []), w, [7, 5], rt=rt)
    with pytest.raises(ValueError, match='a ground-truth box of image 4'):
        ES.bootstrap_class('table', SC.stack([], [], []), gt, w, [7, 5], rt=rt)
    with pytest.raises(ValueError, match='2 weight columns for 3 images'):
        ES.bootstrap_class('table', det, gt, w, [7, 4, 5], rt=rt)


# ---- the weights ---------------------------------------------------------------------------------------------------------------------
def test_weights_of_the_specification():
    """The hash on paper for the first draw: seed 0, replicate 0, draw 0 has key 1 * 0xD6E8FEB86659FD93."""
    x = 0xD6E8FEB86659FD93
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) % 2 ** 64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) % 2 ** 64
    x ^= x >> 33
    u = (x >> 16) % 2 ** 32
    assert FB.draw(0, 0, 0, 1000) == (u * 1000) >> 32 and 0 <= FB.draw(0, 0, 0, 1000) < 1000
    w = BS.Weights(cpu_rt(), 50, 7, seed=2).numpy()
    assert w.shape == (7, 50) and (w.sum(1) == 50).all() and w.tobytes() == FB.weights(2, 7, 50).tobytes()
    assert len({r.tobytes() for r in w}) == 7 and FB.weights(3, 7, 50).tobytes() != w.tobytes()


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
shift = lambda x: SC.box(x, 5.0, 0.0, 1.0, 1.0, 1.0)


def boot(det, gt, rows, idx_list):
    rt = cpu_rt()
    gt = dict(gt, classname=['table'] * len(gt['image']))
    return ES.bootstrap_class('table', det, gt, BS.Weights.of(rt, np.asarray(rows, np.int32)), idx_list, 0.25, rt)


def test_hand_cases():
    # one image, one box, one true positive, weight 3: three boxes, three true positives -> AP 1
    r = boot(SC.stack([shift(0.0)], [1], [0.9]), SC.stack([shift(0.0)], [1]), [[3]], [1])
    assert list(r['ap']) == [1.0] and list(r['n_pos']) == [3] and list(r['n_tp']) == [3] and list(r['n_fp']) == [0] and r['apScore'] == 1.0
    # image 1: a true positive; image 2: a box nobody finds and a false positive ranked first.  Both: fp tp, 2 boxes -> 1/2 * 1/2.
    # Without image 2 its detection and its box are gone: AP 1.  Without image 1: 0.  A row of zeros: 0, and nothing counted.
    det = SC.stack([shift(9.0), shift(0.0)], [2, 1], [0.9, 0.8])
    gt = SC.stack([shift(0.0), shift(3.0)], [1, 2])
    r = boot(det, gt, [[1, 1], [1, 0], [0, 1], [0, 0]], [1, 2])
    assert list(r['ap']) == [0.25, 1.0, 0.0, 0.0] and r['apScore'] == 0.25
    assert list(r['n_pos']) == [2, 1, 1, 0] and list(r['n_tp']) == [1, 1, 0, 0] and list(r['n_fp']) == [1, 0, 1, 0]
    # a false positive of weight 2 ahead of a true positive: fp fp tp -> precision 1/3 at recall 1
    det = SC.stack([shift(9.0), shift(0.0)], [2, 1], [0.9, 0.8])
    r = boot(det, SC.stack([shift(0.0)], [1]), [[1, 2]], [1, 2])
    assert abs(r['ap'][0] - 1.0 / 3.0) <= 1e-15 and (r['n_pos'][0], r['n_tp'][0], r['n_fp'][0]) == (1, 1, 2)


def test_literal_expansion_keeps_copies_apart():
    """Two copies of an image are two images: the copy of a detection claims the copy of its box, not the box of the other copy --
    weight 2 on a true positive gives 2 true positives, not one and a duplicate."""
    det, gt = SC.stack([shift(0.0)], [1], [0.9]), SC.stack([shift(0.0)], [1])
    d, g = FB.expand(det, gt, [0], [0], [2])
    assert list(d['image']) == [0, 1] and list(g['image']) == [0, 1] and len(d['confidence']) == 2
    r = boot(det, gt, [[2]], [1])
    assert (r['n_tp'][0], r['n_fp'][0], r['ap'][0]) == (2, 0, 1.0)


@pytest.mark.parametrize('P,G,R', [(0, 0, 1), (0, 5, 3), (1, 1, 3), (6, 0, 3), (40, 6, 5)])
def test_plumbing_on_the_specification_library(P, G, R):
    BC.check_curves(cpu_rt(), P, G, R, exact=True)
    BC.check_ones(cpu_rt(), P, G)


# ---- summary and paired ----------------------------------------------------------------------------------------------------------------
def test_summary_and_paired_on_fixed_arrays():
    a = {'x': np.arange(101) / 100.0, 'y': np.full(101, 0.5)}
    s = BS.summary(a, 0.9)
    assert s['R'] == 101 and s['level'] == 0.9
    assert abs(s['classes']['x']['mean'] - 0.5) < 1e-15 and abs(s['classes']['x']['lo'] - 0.05) < 1e-15 and abs(s['classes']['x']['hi'] - 0.95) < 1e-15
    assert abs(s['classes']['x']['se'] - np.sqrt(101 * 102 / 12.0) / 100.0) < 1e-14           # sd of 0 .. 100, ddof 1: sqrt(n (n + 1) / 12)
    assert s['classes']['y'] == {'mean': 0.5, 'se': 0.0, 'lo': 0.5, 'hi': 0.5}
    m = s['mean_ap']                                                                          # per replicate (x + 0.5) / 2
    assert abs(m['mean'] - 0.5) < 1e-15 and abs(m['lo'] - 0.275) < 1e-15 and abs(m['hi'] - 0.725) < 1e-15
    b = {'x': a['x'] + 0.1, 'y': np.where(np.arange(101) < 25, 0.4, 0.6)}
    p = BS.paired(a, b, 0.9)
    assert abs(p['classes']['x']['mean'] - 0.1) < 1e-15 and abs(p['classes']['x']['hi'] - p['classes']['x']['lo']) < 1e-15
    assert p['classes']['x']['p_le0'] == 0.0 and abs(p['classes']['y']['p_le0'] - 25 / 101.0) < 1e-15
    assert abs(p['classes']['y']['lo'] + 0.1) < 1e-15 and abs(p['classes']['y']['hi'] - 0.1) < 1e-15
    same = BS.paired(a, a, 0.95)
    assert all(v == {'mean': 0.0, 'se': 0.0, 'lo': 0.0, 'hi': 0.0, 'p_le0': 1.0} for v in list(same['classes'].values()) + [same['mean_ap']])
    for bad in (lambda: BS.summary(a, 1.0), lambda: BS.summary(a, 0.0), lambda: BS.summary({}, 0.9), lambda: BS.paired(a, {'x': a['x']}, 0.9),
                lambda: BS.summary({'x': np.zeros(3), 'y': np.zeros(4)}, 0.9)):
        with pytest.raises(ValueError):
            bad()
    assert BS.difference_text({'mean': 0.0132, 'lo': -0.0041, 'hi': 0.0302, 'p_le0': 0.07}) == '+1.32 [−0.41, +3.02], p(≤0) 0.07'
    assert BS.interval_text({'lo': 0.5, 'hi': 0.75, 'se': 0.0625}, 0.95, 200, ES.num2str) == '[50, 75] (95 %, se 6.25, 200 replicates)'


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_flag_errors(tmp_path):
    ev = ['--idx_path', 'none', '--dataset_dir', str(tmp_path), '--pred_dir', str(tmp_path)]
    for extra in (['--bootstrap_seed', '1'], ['--bootstrap_level', '0.9'], ['--bootstrap_json', 'x.json'],      # ... need --bootstrap
                  ['--bootstrap', '99'], ['--bootstrap', '65537'], ['--bootstrap', '100', '--bootstrap_level', '1'],
                  ['--bootstrap', '100', '--bootstrap_level', '0'], ['--bootstrap', '100', '--bootstrap_seed', '-1'],
                  ['--bootstrap', '100', '--diagnose'], ['--compare_pred_dir', str(tmp_path)],
                  ['--compare_pred_dir', str(tmp_path), '--bootstrap', '100', '--save_curves', str(tmp_path)]):
        with pytest.raises(SystemExit):
            ES.main(ev + extra, rt=cpu_rt(), log=lambda *a: None)
    with pytest.raises(SystemExit):
        ES.main(['--idx_path', 'none', '--official_eval', '--compare_pred_dir', str(tmp_path), '--bootstrap', '100'], rt=cpu_rt(), log=lambda *a: None)
    needed = ['--dataset_dir', str(tmp_path), '--idx_path', 'none', '--rgb_detection_path', 'none']
    sweep = ['--sweep', '--sweep_nms_iou', '0.25']
    for extra in (['--bootstrap', '100'],                                                        # needs --official_eval or --sweep
                  ['--official_eval', '--bootstrap_seed', '1'], ['--official_eval', '--bootstrap', '50'],
                  ['--official_eval', '--bootstrap', '100', '--diagnose'], sweep + ['--bootstrap', '100', '--bootstrap_json', 'x.json'],
                  sweep + ['--bootstrap_level', '0.9']):
        with pytest.raises(SystemExit):
            DT.main(needed + extra, log=lambda *a: None)
    with pytest.raises(ValueError):
        ES.evaluate(None, str(tmp_path), [], 'B', rt=cpu_rt(), predictions={}, diagnose={'bg': 0.1}, bootstrap=100)


# ---- the flows ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden(tmp_path_factory):
    import detect_check as DC
    root = tmp_path_factory.mktemp('golden')
    ids, _, idx, _ = DC.write_data_set(root)
    return root, ids, idx


def test_compare_pred_dir_flow(golden, tmp_path):
    root, ids, idx = golden
    rows_a, rows_b = BC.golden_rows(root, ids, seed=1), BC.golden_rows(root, ids, seed=1, drop=0.3)
    dir_a, dir_b = BC.write_pred_dir(str(tmp_path / 'a'), rows_a), BC.write_pred_dir(str(tmp_path / 'b'), rows_b)
    base = ['--dataset_dir', str(root), '--idx_path', idx, '--test_on', 'AB', '--bootstrap', '100', '--bootstrap_seed', '5']
    # two identical directories: dAP exactly 0 with interval [0, 0]
    lines = []
    a, b, d = ES.main(base + ['--pred_dir', dir_a, '--compare_pred_dir', dir_a], rt=cpu_rt(), log=lines.append)
    assert all(v['mean'] == v['lo'] == v['hi'] == 0.0 and v['p_le0'] == 1.0 for v in list(d['classes'].values()) + [d['mean_ap']])
    dap = [l for l in lines if l.startswith('dAP for ')]
    assert len(dap) == 10 and dap[0] == 'dAP for BED (B - A): +0.00 [+0.00, +0.00], p(≤0) 1.00' and lines[-1] == 'Mean dAP (B - A): +0.00 [+0.00, +0.00], p(≤0) 1.00'
    assert [l[3:] for l in lines if l.startswith('A: ')] == [l[3:] for l in lines if l.startswith('B: ')] and lines[0].startswith('A: Number of predictions for BED')
    # the tagged lines are those of a single run with the same flags, and --bootstrap changes none of the script's lines
    single, plain = [], []
    one = ES.main(base + ['--pred_dir', dir_a], rt=cpu_rt(), log=single.append)
    ES.main(base[:6] + ['--pred_dir', dir_a], rt=cpu_rt(), log=plain.append)
    assert single == [l[3:] for l in lines if l.startswith('A: ')]
    assert [l for l in single if ' interval' not in l] == plain and len(single) == len(plain) + 11
    assert all(np.array_equal(one[2]['ap'][c], a[2]['ap'][c]) for c in ES.CLASS_NAMES['AB'])
    # two different directories, the same redraws: the differences are those of the replicates, and the JSON holds all of it
    path = str(tmp_path / 'cmp.json')
    lines = []
    a, b, d = ES.main(base + ['--pred_dir', dir_a, '--compare_pred_dir', dir_b, '--bootstrap_json', path, '--bootstrap_level', '0.8'], rt=cpu_rt(), log=lines.append)
    assert all(np.array_equal(a[2]['ap'][c], one[2]['ap'][c]) for c in ES.CLASS_NAMES['AB']), 'the side A depends on what it is compared with'
    diff = b[2]['ap']['bed'] - a[2]['ap']['bed']
    assert np.ptp(diff) > 0.0 and abs(d['classes']['bed']['mean'] - diff.mean()) < 1e-15 and d['level'] == 0.8
    assert d['classes']['bed']['lo'] == np.percentile(diff, 10.0) and d['classes']['bed']['p_le0'] == float(np.mean(diff <= 0))
    assert '(80 %, se ' in lines[2]
    js = json.load(open(path))
    assert js['paired']['classes']['bed'] == d['classes']['bed'] and js['A']['replicates']['bed'] == [float(x) for x in a[2]['ap']['bed']]
    assert js['B']['summary']['mean_ap'] == b[2]['summary']['mean_ap'] and js['A']['R'] == 100 and js['A']['seed'] == 5


def test_detect_sweep_bootstrap_flow(tmp_path):
    """detect --sweep --bootstrap on the duplicated golden scenes: the rows' order, APs and lines are those without --bootstrap; each of
    the top rows carries the paired intervals; the baseline row against itself and the best row against itself are [0, 0]; a row's
    replicate mean APs are those of a separate detect run with that row's flags followed by evaluate --bootstrap with the same seed."""
    from transferable3d_amd.constants import class2type
    import detect_check as DC
    quiet = lambda *a: None
    rt = cpu_rt()
    ids, folder, idx, dets = NC.write_duplicated(tmp_path)
    base = ['--dataset_dir', str(tmp_path), '--idx_path', idx, '--rgb_detection_path', folder, '--test_on', 'B'] + DC.MODEL_FLAGS
    path = os.path.join(str(tmp_path), 'sweep.json')
    plain, logged = [], []
    ref = DT.main(base + SW.SWEEP_FLAGS + ['--sweep_top', '6'], rt=rt, log=plain.append)
    result = DT.main(base + SW.SWEEP_FLAGS + ['--sweep_top', '6', '--sweep_json', path, '--bootstrap', '100', '--bootstrap_seed', '2'], rt=rt, log=logged.append)
    assert ref.bootstrap is None and np.array_equal(ref.mean_ap, result.mean_ap) and ref.ranking() == result.ranking()
    rows = [l for l in logged if l[:4].strip().endswith('.')]
    assert len(rows) == 6 and [l.split(' | vs baseline ')[0] for l in logged[:-2] if 'written to' not in l] == plain
    boot, order = result.bootstrap, result.ranking()
    assert sorted(boot['rows']) == list(range(6)) and boot['R'] == 100 and boot['seed'] == 2 and boot['level'] == 0.95
    zero = {'mean': 0.0, 'se': 0.0, 'lo': 0.0, 'hi': 0.0, 'p_le0': 1.0}
    assert boot['rows'][0]['vs_baseline'] == zero and boot['rows'][order[0]]['vs_best'] == zero      # (row 0 of this grid is the baseline)
    assert rows[0].endswith(' | vs best +0.00 [+0.00, +0.00], p(≤0) 1.00')
    same = [k + 1 for k, m in enumerate(order) if k > 0 and boot['rows'][m]['vs_best']['lo'] <= 0.0 <= boot['rows'][m]['vs_best']['hi']]
    assert logged[-2] == 'indistinguishable from best at 95 %: ' + ('rows ' + ', '.join(map(str, same)) if same else 'none'), logged[-2]
    assert logged[-3] == plain[-1] and plain[-1].startswith('best: ')
    for m in range(6):
        r = boot['rows'][m]
        d = boot['replicates'][m] - boot['replicates'][0]
        assert abs(r['vs_baseline']['mean'] - d.mean()) < 1e-15 and r['vs_baseline']['p_le0'] == float(np.mean(d <= 0))
    js = json.load(open(path))
    assert js['bootstrap'] == {'R': 100, 'seed': 2, 'level': 0.95} and js['rows'][order[1]]['bootstrap']['vs_best'] == boot['rows'][order[1]]['vs_best']
    # one row against a separate run with its flags
    m = order[0]
    flags = [] if result.table()[m]['flags'] == '(no flags)' else result.table()[m]['flags'].split()
    p = DT.main(base + flags, rt=rt, log=quiet)
    names = [class2type[int(c)] for c in p[10]]
    held = ES.official_predictions(sorted(set(ES.CLASS_NAMES['B']) | set(names)), p, names)
    sep = ES.evaluate(None, str(tmp_path), idx, 'B', rt=rt, log=quiet, predictions=held, bootstrap={'R': 100, 'seed': 2})
    assert np.array_equal(BS.mean_over_classes({c: sep[2]['ap'][c] for c in ES.CLASS_NAMES['B']}), boot['replicates'][m])
