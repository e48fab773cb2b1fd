"""Generates tests/golden/label_subsets.npz (and, when needed, tests/golden/label_subset_frustums.zip.pickle) by EXECUTING the
reference's two data set constructors (run in the build container only, where /root/reference exists:
`python tests/golden/make_label_subset_vectors.py`).

What runs is the reference's own code, loaded from where it lies with the placeholder modules of make_reference_vectors.py (nothing of
it is copied here): ROISemiDataset.__init__ (roi_semi_dataset.py:196-274) under --train_data3D_keep_prob / --add3D_for_classes2D_prob
and BoxPCFitDataset.__init__ (box_pc_fit_dataset.py:47-100) under --classes_to_drop_prob, each seeding the global np.random stream
with 20 and walking the frustum file once.  Recorded, per setting: the lists the constructors built (`idx_3Dl`, `idx_2Dl`, `idx_l`)
and their `cls_to_idx_map`s.  The frustum file numbers its frustums 0..F-1 in its `idx` column, so the recorded idx lists ARE the file
positions of the kept frustums.

The frustum file is tests/golden/reference_frustums.zip.pickle when it has at least 40 frustums and two classes on either side of the
TRAIN_CLS / TEST_CLS split with `idx` = file position; otherwise (today: it has 24) a synthetic file of 96 small frustums is written
with the product's save_zipped_pickle and used.  tests/test_label_subset_cpu.py / _gpu.py replay the recording:
dataset.reference_label_subset / reference_drop_subset must give these memberships, t3d_label_subset these lists and groups.

A map is stored as three arrays: `<map>_classes` (indices into `class_names`, ascending), `<map>_offsets` [n + 1] and `<map>_positions`
(the positions within the list, class after class).
"""
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, 'label_subsets.npz')
OWN_FILE = os.path.join(HERE, 'label_subset_frustums.zip.pickle')
SEMI_SETTINGS = [(1, -1), (0.5, -1), (0.1, 0), (0.5, 0.25), (0, 1)]      # (train_data3D_keep_prob, add3D_for_classes2D_prob)
DROP_SETTINGS = [1, 0.5, 0]                                               # classes_to_drop_prob
N_OWN = 96


def tag(v):
    return ('%g' % v).replace('-', 'm')


def semi_key(keep, add):
    return 'semi/keep%s_add%s/' % (tag(keep), tag(add))


def drop_key(prob):
    return 'boxpc/drop%s/' % tag(prob)


def own_frustums(class_names, n_frustums=N_OWN, seed=5):
    """A frustum file in the 13-list layout of the reference's readers: small frustums, classes drawn uniformly after one of each."""
    from transferable3d_amd.constants import MEAN_DIMS_ARR, type2class
    from transferable3d_amd.eval_det import get_3d_box
    r = np.random.RandomState(seed)
    L = [[] for _ in range(13)]
    order = list(r.permutation(len(class_names))) * 2 + list(r.randint(0, len(class_names), size=n_frustums - 2 * len(class_names)))
    for i in range(n_frustums):
        cls = class_names[order[i]]
        npts = int(r.randint(24, 49))
        pts = np.concatenate([r.normal(size=(npts, 3)) * [0.8, 0.5, 0.8] + [0.3, 0.1, 3.0], r.uniform(size=(npts, 3))], 1).astype(np.float32)
        size = MEAN_DIMS_ARR[type2class[cls]] * r.uniform(0.8, 1.2, size=3)
        heading = float(r.uniform(-np.pi, np.pi))
        center = np.array([0.3, 0.1, 3.0]) + r.normal(size=3) * 0.2
        items = (i, r.uniform(0, 300, size=4), np.asarray(get_3d_box(size, heading, center)), None, pts,
                 (r.uniform(size=npts) < 0.4).astype(np.float64), cls, heading, size, np.eye(3) + r.normal(size=(3, 3)) * 0.01,
                 np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]]), float(r.uniform(-np.pi, 0)), np.array([480.0, 640.0]))
        for lst, it in zip(L, items):
            lst.append(it)
    return L


def usable(path, train_cls, test_cls):
    from transferable3d_amd.dataset import load_zipped_pickle
    if not os.path.exists(path):
        return False
    L = load_zipped_pickle(path)
    names = set(L[6])
    return (len(L[0]) >= 40 and len(names & set(train_cls)) >= 2 and len(names & set(test_cls)) >= 2
            and [int(i) for i in L[0]] == list(range(len(L[0]))))


def map_arrays(cmap, class_names):
    present = sorted(class_names.index(t) for t in cmap)
    groups = [np.asarray(cmap[class_names[c]], np.int32) for c in present]
    return (np.asarray(present, np.int32), np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32),
            np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, np.int32))


def main():
    spec = importlib.util.spec_from_file_location('make_reference_vectors', os.path.join(HERE, 'make_reference_vectors.py'))
    mrv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mrv)
    _, seg, semi, _, bp = mrv.reference_modules()
    from transferable3d_amd.config import make_parser
    from transferable3d_amd.dataset import load_zipped_pickle, save_zipped_pickle
    flags = make_parser().parse_special_args([])
    class_names = [seg.class2type[i] for i in range(seg.NUM_CLASS)]
    train_cls, test_cls = list(flags.SUNRGBD_SEMI_TRAIN_CLS), list(flags.SUNRGBD_SEMI_TEST_CLS)
    path = os.path.join(HERE, 'reference_frustums.zip.pickle')
    if not usable(path, train_cls, test_cls):
        save_zipped_pickle(own_frustums(class_names), OWN_FILE)
        path = OWN_FILE
        assert usable(path, train_cls, test_cls)
    file_cls = load_zipped_pickle(path)[6]
    out = {'class_names': np.array(class_names), 'classes3D': np.array(train_cls), 'classes2D': np.array(test_cls),
           'frustum_file': np.array(os.path.basename(path)), 'file_cls': np.array([class_names.index(t) for t in file_cls], np.int32),
           'semi_settings': np.array(SEMI_SETTINGS, np.float64), 'drop_settings': np.array(DROP_SETTINGS, np.float64)}
    for keep, add in SEMI_SETTINGS:
        ds = semi.ROISemiDataset(train_cls, test_cls, 128, data3D_keep_prob=keep, add3D_for_classes2D_prob=add, overwritten_data_path=path)
        k = semi_key(keep, add)
        out[k + 'idx_3Dl'], out[k + 'idx_2Dl'] = np.asarray(ds.idx_3Dl, np.int32), np.asarray(ds.idx_2Dl, np.int32)
        for name, cmap, lst in (('map3D', ds.cls_to_idx_map3D, ds.cls_type_3Dl), ('map2D', ds.cls_to_idx_map2D, ds.cls_type_2Dl)):
            out[k + name + '_classes'], out[k + name + '_offsets'], out[k + name + '_positions'] = map_arrays(cmap, class_names)
            assert all(lst[p] == t for t, ps in cmap.items() for p in ps)
        print('%s: keep %g add %g -> len3D %d, len2D %d' % (os.path.basename(path), keep, add, len(ds.idx_3Dl), len(ds.idx_2Dl)))
    for prob in DROP_SETTINGS:
        ds = bp.BoxPCFitDataset(classes=class_names, npoints=128, center_perturbation=0.8, size_perturbation=0.2, angle_perturbation=np.pi,
                                classes_to_drop=test_cls, classes_to_drop_prob=prob, overwritten_data_path=path)
        k = drop_key(prob)
        out[k + 'idx_l'] = np.asarray(ds.idx_l, np.int32)
        out[k + 'map_classes'], out[k + 'map_offsets'], out[k + 'map_positions'] = map_arrays(ds.cls_to_idx_map, class_names)
        print('%s: classes_to_drop_prob %g -> %d frustums' % (os.path.basename(path), prob, len(ds.idx_l)))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes;', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
