"""TEST INFRASTRUCTURE ONLY -- a NumPy restatement of the reference's frustum extraction (sunrgbd_data.py process_object and the loop
of extract_roi_seg_from_rgb_detection; utils.py project_upright_depth_to_image, random_shift_box2d, extract_pc_in_box3d,
project_image_to_upright_camerea), one 2-D box at a time, on given draws.  Labels use Delaunay.find_simplex like the reference."""
import numpy as np


def flip_axis_to_camera(pc):
    pc2 = np.copy(pc)
    pc2[:, [0, 1, 2]] = pc2[:, [0, 2, 1]]
    pc2[:, 1] *= -1
    return pc2


def project_to_image(depth, rtilt, K):
    pc2 = flip_axis_to_camera(np.transpose(np.dot(np.transpose(rtilt), np.transpose(depth[:, 0:3]))))
    uv = np.dot(pc2, np.transpose(K))
    uv[:, 0] /= uv[:, 2]
    uv[:, 1] /= uv[:, 2]
    return uv[:, 0:2]


def shift_box2d(box2d, u, r=0.1):
    xmin, ymin, xmax, ymax = box2d
    h, w = ymax - ymin, xmax - xmin
    cx, cy = (xmin + xmax) / 2.0, (ymin + ymax) / 2.0
    cx2 = cx + w * r * (u[0] * 2 - 1)
    cy2 = cy + h * r * (u[1] * 2 - 1)
    h2 = h * (1 + u[2] * 2 * r - r)
    w2 = w * (1 + u[3] * 2 * r - r)
    return np.array([cx2 - w2 / 2.0, cy2 - h2 / 2.0, cx2 + w2 / 2.0, cy2 + h2 / 2.0])


def frustum_angle(box2d, rtilt, K):
    xmin, ymin, xmax, ymax = box2d
    uvd = np.array([[(xmin + xmax) / 2.0, (ymin + ymax) / 2.0, 20.0]])
    x = ((uvd[:, 0] - K[0, 2]) * uvd[:, 2]) / K[0, 0]
    y = ((uvd[:, 1] - K[1, 2]) * uvd[:, 2]) / K[1, 1]
    cam = np.stack([x, y, uvd[:, 2]], 1)
    depth = np.stack([cam[:, 0], cam[:, 2], -cam[:, 1]], 1)
    up = flip_axis_to_camera(np.transpose(np.dot(rtilt, np.transpose(depth))))
    return -1 * np.arctan2(up[0, 2], up[0, 0])


def in_box3d(pc, corners):
    from scipy.spatial import Delaunay
    return Delaunay(corners).find_simplex(pc[:, 0:3]) >= 0


def extract(depth, rtilt, K, box2d, corners=None, perturb=None, choice=None, num_points=2048, uv=None):
    """One job: {'box2d', 'index' (scene-local), 'points', 'label' (or None), 'frustum_angle', 'n'}.  choice: the ranks
    np.random.choice drew (required when n > num_points)."""
    if uv is None:
        uv = project_to_image(depth, rtilt, K)
    box = shift_box2d(box2d, perturb) if perturb is not None else np.array(box2d, np.float64)
    xmin, ymin, xmax, ymax = box
    inds = np.nonzero((uv[:, 0] < xmax) & (uv[:, 0] >= xmin) & (uv[:, 1] < ymax) & (uv[:, 1] >= ymin))[0]
    n = len(inds)
    pts = np.zeros_like(depth)
    pts[:, 0:3] = flip_axis_to_camera(depth[:, 0:3])
    pts[:, 3:] = depth[:, 3:]
    label = None
    if corners is not None:
        label = np.zeros(n)
        label[in_box3d(pts[inds], corners)] = 1
    if n > num_points:
        assert choice is not None and len(choice) == num_points
        inds = inds[np.asarray(choice)]
        if label is not None:
            label = label[np.asarray(choice)]
    return {'box2d': box, 'index': inds, 'points': pts[inds], 'label': label, 'frustum_angle': frustum_angle(box, rtilt, K), 'n': n}


def face_distance(pc, corners):
    """Distance of each point to the nearest face plane of the box (the band where an inclusive test and Delaunay may disagree)."""
    p1 = corners[1]
    out = np.full(len(pc), np.inf)
    for far in (2, 5, 0):
        e = corners[far] - p1
        L = np.linalg.norm(e)
        t = (pc[:, 0:3] - p1) @ (e / L)
        out = np.minimum(out, np.minimum(np.abs(t), np.abs(t - L)))
    return out
