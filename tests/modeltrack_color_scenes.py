"""Scenes for the tests of spec S38 (tests/test_modeltrack_color_spec.py): modeltrack_scenes.single_frame_run's corridor with a colour
volume integrated beside the map from the paint of tests/test_voxelcolor_spec.py, every image with uniform noise of +-3
levels.  The disparity frames are drawn from the run's generator first, in single_frame_run's order, and the image noise after them, so
that the geometry of a run is single_frame_run's own at the same seed and photo_weight = 0 reproduces S34's figures.  Host only, numpy only."""
import numpy as np

import modeltrack_scenes as MS
import np_modeltrack as T
import np_modeltrack_color as TC
import np_voxelcolor as K
import np_voxelmap as V
from test_voxelcolor_spec import paint

IMAGE_NOISE = 3              # levels of 255, uniform, on every channel of every image


def noisy_image(image, rng):
    n = rng.integers(-IMAGE_NOISE, IMAGE_NOISE + 1, image.shape)
    return np.clip(image.astype(np.int64) + n, 0, 255).astype(np.uint8)


def build(cam, shape, w, h, boxes=MS.BOXES, seed=5, frames=6, step=0.25):
    """-> (Map, Color, true pose of the tracked frame, its disparity, its image): the model of `frames` frames integrated at their true
    poses, geometry and colour, and frame `frames` to track."""
    rng = np.random.default_rng(seed)
    poses = [MS.pose_of(t=(0.0, 0.0, step * k)) for k in range(frames + 1)]
    truths = [MS.render(cam, pose, w, h, boxes) for pose in poses]
    disps = [MS.noisy(t, rng) for t in truths]
    images = [noisy_image(paint(cam, pose, t), rng) for pose, t in zip(poses, truths)]
    m = V.Map(*shape)
    c = K.Color(m)
    for k in range(frames):
        m.integrate(cam, poses[k], disps[k])
        c.integrate(cam, poses[k], disps[k], images[k])
    return m, c, poses[frames], disps[frames], images[frames]


def track(model, cam, offset, yaw_deg, p=None, cp=None):
    """The model's next frame tracked from its true pose perturbed by (offset, yaw_deg).  -> (start pose, end pose, true pose, record)."""
    m, c, true, d, im = model
    start = MS.perturb(true, offset, yaw_deg)
    res = TC.refine(m, c, cam, p if p is not None else T.params(), cp if cp is not None else TC.params(), start, d, im)
    end = T.join([float(v) for v in res["R"][0]], [float(v) for v in res["t"][0]])
    return start, end, true, res


def errors(pose, true):
    """-> (along-axis error, cross-axis error, total translation error in metres, rotation error in degrees)."""
    e = [pose[4 * a + 3] - true[4 * a + 3] for a in range(3)]
    tot, rot = MS.pose_error(pose, true)
    return abs(e[2]), float(np.hypot(e[0], e[1])), tot, rot
