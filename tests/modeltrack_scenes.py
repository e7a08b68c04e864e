"""Scenes for the tests of spec S34 (tests/test_modeltrack_spec.py): a small ray-plane / ray-box renderer that gives the disparity image of
a corridor (floor and two walls, optionally with four boxes standing in it) from any camera-to-world pose, pose helpers and the two
accuracy runs whose measured figures stand in the test file and in DESIGN.md 7.16.  Host only, numpy only."""
import math

import numpy as np

import np_modeltrack as T
import np_voxelmap as V

INV = V.INVALID
FLOOR_Y, WALL_X = 1.5, 3.0                       # the camera looks along +z, y points down: the floor lies 1.5 m below it, the walls 3 m to each side
# (x0, x1, y0, y1, z0, z1): four boxes standing on the floor
BOXES = ((-2.5, -1.5, 0.5, 1.5, 4.0, 5.0), (1.0, 2.2, 0.3, 1.5, 6.0, 7.0), (-1.0, -0.2, 0.5, 1.5, 9.0, 10.0), (1.8, 2.8, 0.1, 1.5, 11.0, 12.0))


def pose_of(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0, t=(0.0, 0.0, 0.0)):
    """camera-to-world 3 x 4 as 12 floats: R = Ry(yaw) Rx(pitch) Rz(roll)."""
    a, b, c = (math.radians(v) for v in (yaw_deg, pitch_deg, roll_deg))
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    R = Ry @ Rx @ Rz
    return [float(v) for v in np.hstack([R, np.asarray(t, np.float64).reshape(3, 1)]).reshape(12)]


def mat(pose):
    M = np.eye(4)
    M[:3] = np.asarray(pose, np.float64).reshape(3, 4)
    return M


def chain(a, b):
    """a then b on the right: the camera-to-world pose a composed with the relative pose b (b's frame expressed in a's)."""
    return [float(v) for v in (mat(a) @ mat(b))[:3].reshape(12)]


def pose_error(est, true):
    """-> (translation error in metres, rotation error in degrees)."""
    E, G = mat(est), mat(true)
    c = (np.trace(E[:3, :3].T @ G[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(E[:3, 3] - G[:3, 3])), math.degrees(math.acos(max(-1.0, min(1.0, c))))


def render(cam, pose, w, h, boxes=BOXES):
    """The noise-free disparity (x16, int16) of the corridor seen from `pose`: the nearest of the floor, the two walls and the boxes along
    every pixel's ray; -32768 where the ray meets nothing in front of the camera or the disparity leaves 1..32767."""
    M = mat(pose)
    y, x = np.mgrid[0:h, 0:w]
    d_cam = np.stack([(x - cam["cx"]) / cam["fx"], (y - cam["cy"]) / cam["fy"], np.ones((h, w))], -1)   # Z = 1: the ray parameter is the depth
    d = d_cam @ M[:3, :3].T
    o = M[:3, 3]
    best = np.full((h, w), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, value in ((1, FLOOR_Y), (0, -WALL_X), (0, WALL_X)):
            s = (value - o[axis]) / d[..., axis]
            best = np.where((s > 0) & (s < best), s, best)
        for b in boxes:
            lo, hi = np.array(b[0::2]), np.array(b[1::2])
            s0, s1 = (lo - o) / d, (hi - o) / d
            near, far = np.minimum(s0, s1).max(-1), np.maximum(s0, s1).min(-1)
            best = np.where((near <= far) & (near > 0) & (near < best), near, best)
        sw = np.floor(cam["fx"] * cam["baseline"] / best * 16.0 + 0.5)
    return np.where(np.isfinite(best) & (sw >= 1) & (sw <= 32767), sw, INV).astype(np.int16)


def noisy(truth, rng, holes=0.10):
    """+-1/4 pixel of uniform noise and fresh holes."""
    ok = truth != INV
    d = truth.copy()
    d[ok] += rng.integers(-4, 5, int(ok.sum())).astype(np.int16)
    d[ok & (rng.random(truth.shape) < holes)] = INV
    return d


def perturb(pose, offset, yaw_deg):
    """The pose moved by `offset` (world metres) and turned by yaw_deg about the camera's y axis."""
    P = chain(pose, pose_of(yaw_deg=yaw_deg))
    for a in range(3):
        P[4 * a + 3] += offset[a]
    return P


def single_frame_run(cam, shape, w, h, offset, yaw_deg, boxes=BOXES, seed=5, frames=6, step=0.25, p=None):
    """A model of `frames` frames integrated at their true poses (`step` metres forward each), then the next frame tracked from its true
    pose perturbed by (offset, yaw_deg).  -> (start error, end error, result record)."""
    rng = np.random.default_rng(seed)
    m = V.Map(*shape)
    for k in range(frames):
        pose = pose_of(t=(0.0, 0.0, step * k))
        m.integrate(cam, pose, noisy(render(cam, pose, w, h, boxes), rng))
    true = pose_of(t=(0.0, 0.0, step * frames))
    d = noisy(render(cam, true, w, h, boxes), rng)
    start = perturb(true, offset, yaw_deg)
    res = T.refine(m, cam, p if p is not None else T.params(), start, d)
    end = T.join([float(v) for v in res["R"][0]], [float(v) for v in res["t"][0]])
    return pose_error(start, true), pose_error(end, true), res


def chain_run(cam, shape, w, h, frames=14, seed=7, step=0.25, sigma_deg=0.15, sigma_t=0.02, boxes=BOXES, p=None):
    """Track-then-integrate over `frames` frames: the odometry is the true relative pose with Gaussian noise of sigma_deg per angle and
    sigma_t per component; the tracked chain predicts from the previous tracked pose.  -> (errors of the chained odometry per frame, errors
    of the tracked chain per frame, accepted flags)."""
    rng = np.random.default_rng(seed)
    p = p if p is not None else T.params()
    m = V.Map(*shape)
    true_prev = odo = tracked = None
    e_odo, e_trk, taken = [], [], []
    for k in range(frames):
        true = pose_of(yaw_deg=0.5 * math.sin(0.7 * k), t=(0.05 * math.sin(0.5 * k), 0.0, step * k))
        d = noisy(render(cam, true, w, h, boxes), rng)
        if k == 0:
            odo = tracked = true
            took = False
        else:
            rel = (np.linalg.inv(mat(true_prev)) @ mat(true))[:3].reshape(12)
            ang, tn = rng.normal(0.0, sigma_deg, 3), rng.normal(0.0, sigma_t, 3)
            rel = chain(rel, pose_of(yaw_deg=ang[0], pitch_deg=ang[1], roll_deg=ang[2], t=tn))
            odo = chain(odo, rel)
            pred = chain(tracked, rel)
            took, tracked = T.accept(T.refine(m, cam, p, pred, d), pred, p)
        m.integrate(cam, tracked, d)
        true_prev = true
        e_odo.append(pose_error(odo, true))
        e_trk.append(pose_error(tracked, true))
        taken.append(took)
    return e_odo, e_trk, taken
