"""Generates tests/golden/render_reference.npz by EXECUTING the reference's own projections (sunrgbd/sunrgbd_data/utils.py:
compute_box_3d's box3d_pts_2d and SUNRGBD_Calibration.project_upright_depth_to_image) on the three scenes of frustum_scenes.npz (run in
the build container only, where /root/reference exists: `python tests/golden/make_render_vectors.py`).

The reference runs unmodified from where it lies, with the placeholder modules make_frustum_vectors.py uses (`cv2`, `cPickle`).
Stored, per scene: for every label object its class, the 8 projected corners (box3d_pts_2d, pixels) and the 8 corners in upright depth
coordinates the reference projected; a sample of 200 scene points (indices into the scene's depth rows), their pixel coordinates and
camera depths.  Data only; tests/test_render_cpu.py projects the same corners and points through render.image_view and compares."""
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

SAMPLE = 200


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    from PIL import Image
    cv2 = types.ModuleType('cv2')
    cv2.imread = lambda p: np.ascontiguousarray(np.asarray(Image.open(p).convert('RGB'))[:, :, ::-1])
    sys.modules['cv2'] = cv2
    import pickle
    sys.modules['cPickle'] = pickle
    utils = load('utils', os.path.join(REF, 'utils.py'))
    tmp = tempfile.mkdtemp()
    ids, _, _ = FC.write_golden_scenes(tmp)
    rng = np.random.RandomState(23)
    out = {'ids': np.array(ids, np.int32)}
    for s in ids:
        calib = utils.SUNRGBD_Calibration(os.path.join(tmp, 'training', 'calib', '%06d.txt' % s))
        objects = utils.read_sunrgbd_label(os.path.join(tmp, 'training', 'label_dimension', '%06d.txt' % s))
        uv, k3 = zip(*[utils.compute_box_3d(o, calib) for o in objects])
        depth = utils.load_depth_points(os.path.join(tmp, 'training', 'depth', '%06d.txt' % s))
        pick = np.sort(rng.choice(len(depth), SAMPLE, replace=False))
        puv, pd = calib.project_upright_depth_to_image(depth[pick, :3])
        out.update({'box_class_%d' % s: np.array([o.classname for o in objects]), 'box_uv_%d' % s: np.stack(uv).astype(np.float64),
                    'box_depth_corners_%d' % s: np.stack(k3).astype(np.float64), 'point_index_%d' % s: pick.astype(np.int32),
                    'point_uv_%d' % s: np.asarray(puv, np.float64), 'point_depth_%d' % s: np.asarray(pd, np.float64)})
    path = os.path.join(HERE, 'render_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
