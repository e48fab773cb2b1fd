"""Generates tests/golden/consistency_reference.npz by EXECUTING the reference's own box construction and projection
(sunrgbd/sunrgbd_data/utils.py: SUNObject3d, compute_box_3d, SUNRGBD_Calibration.project_upright_depth_to_image) on 42 label lines drawn
here, under the calibrations of the three scenes of frustum_scenes.npz (run in the build container only, where /root/reference exists:
`python tests/golden/make_consistency_vectors.py`).

The reference runs unmodified from where it lies, with the placeholder modules make_frustum_vectors.py uses (`cv2`, `cPickle`).  A third
of the boxes sits well inside the view, a third straddles the image border (a centroid near the edge of the field of view), a third lies
behind the camera (a negative forward coordinate).  Stored per box: the calibration (Rtilt, K as the reference holds them), the 8
corners in upright depth coordinates, their pixel coordinates and camera depths.  Data only; tests/test_consistency_cpu.py projects the
same corners through tests/fake_consistency.py and compares."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
REF = '/root/reference/sunrgbd/sunrgbd_data'
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import frustum_check as FC        # noqa: E402

PER_KIND = 14


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.modules['cv2'] = types.ModuleType('cv2')
    import pickle
    sys.modules['cPickle'] = pickle
    utils = load('utils', os.path.join(REF, 'utils.py'))
    tmp = tempfile.mkdtemp()
    ids, _, _ = FC.write_golden_scenes(tmp)
    calibs = [utils.SUNRGBD_Calibration(os.path.join(tmp, 'training', 'calib', '%06d.txt' % s)) for s in ids]
    rng = np.random.RandomState(41)
    rows = {k: [] for k in ('kind', 'Rtilt', 'K', 'corners_depth', 'uv', 'depth')}
    for kind in range(3):                  # 0: inside the view, 1: across the image border, 2: behind the camera
        for i in range(PER_KIND):
            calib = calibs[(kind * PER_KIND + i) % len(calibs)]
            y = rng.uniform(1.5, 5.0) * (-1.0 if kind == 2 else 1.0)              # upright depth: y is forward
            half_view = abs(y) * calib.c_u / calib.f_u
            x = rng.uniform(-0.4, 0.4) * half_view if kind != 1 else rng.choice([-1.0, 1.0]) * rng.uniform(0.95, 1.05) * half_view
            z = rng.uniform(-1.0, 0.5)
            w, l, h = rng.uniform(0.2, 1.2, 3)
            a = rng.uniform(-np.pi, np.pi)
            line = 'table 10 20 30 40 %r %r %r %r %r %r %r %r %r %r %r %r' % tuple(
                float(t) for t in (x, y, z, w, l, h, np.cos(a), -np.sin(a), np.sin(a), np.cos(a), np.cos(a), -np.sin(a)))
            obj = utils.SUNObject3d(line)
            uv, k3 = utils.compute_box_3d(obj, calib)
            uv2, depth = calib.project_upright_depth_to_image(k3)
            assert np.array_equal(uv, uv2)
            for k, v in (('kind', kind), ('Rtilt', calib.Rtilt), ('K', calib.K), ('corners_depth', k3), ('uv', uv), ('depth', depth)):
                rows[k].append(np.asarray(v, np.float64))
    out = {k: np.stack(v) for k, v in rows.items()}
    out['kind'] = out['kind'].astype(np.int32)
    assert (out['depth'][out['kind'] == 2] < 0).all() and (out['depth'][out['kind'] != 2] > 0).all()
    path = os.path.join(HERE, 'consistency_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), out['uv'].shape)


if __name__ == '__main__':
    main()
