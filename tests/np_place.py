"""numpy restatement of spec S27: place recognition over a ring of stored ORB frames.  The checker of cart_place_*
and of the loop_closure module; shares no code with them.  The per-query best and second-best distances come from np_match's forward
table (S22 without a gate), the verification of the module from np_match and np_ego."""
import numpy as np

import np_ego as E
import np_match as M

CANDIDATE_DTYPE = np.dtype([("slot", "<i4"), ("score", "<i4"), ("frame_id", "<u8")])   # cart_place_candidate
DEFAULTS = dict(max_distance=64, ratio=80, min_score=30, max_candidates=4, min_gap=50)   # cart_place_default_params
U64 = 1 << 64
LOOP_DTYPE = np.dtype([("detected", "<i4"), ("slot", "<i4"), ("score", "<i4"), ("reserved", "<i4"), ("keyframe_id", "<u8"), ("relative", E.RESULT_DTYPE),
                       ("pose_keyframe", "<f8", 12), ("pose_loop", "<f8", 12)])   # the module's LoopClosure record


def params(**fields):
    assert set(fields) <= set(DEFAULTS)
    return dict(DEFAULTS, **fields)


def votes(qd, td, p):
    """bool [nq]: which queries vote for a stored set (S22's forward record without a gate, then the vote rule)."""
    qd = np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
    td = np.ascontiguousarray(td, np.uint8).reshape(-1, 32)
    fwd = M.match(qd, td, M.params(use_gate=0, cross_check=0))[1].astype(np.int64)
    j1, d1, d2 = fwd[:, 0], fwd[:, 1], fwd[:, 2]
    ok = (j1 >= 0) & (d1 <= p["max_distance"])
    if p["ratio"]:
        ok &= (d2 < 0) | (100 * d1 < p["ratio"] * d2)
    return ok


class Ring:
    """The database: insert number m goes to slot m mod capacity."""

    def __init__(self, max_features, capacity):
        self.max_features, self.capacity = max_features, capacity
        self.clear()

    def clear(self):
        self.slots = [None] * self.capacity
        self.inserts = 0

    def insert(self, desc, frame_id, kp=None, landmarks=None, count=None):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = min(max(len(desc) if count is None else int(count), 0), self.max_features)
        slot = self.inserts % self.capacity
        self.slots[slot] = dict(desc=desc[:n].copy(), frame_id=int(frame_id) % U64, kp=None if kp is None else kp[:n].copy(),
                                landmarks=None if landmarks is None else np.array(landmarks[:n], np.float64))
        self.inserts += 1
        return slot

    def eligible(self, k, frame_id, min_gap):
        s = self.slots[k]
        return s is not None and s["frame_id"] + int(min_gap) < U64 and s["frame_id"] + int(min_gap) <= int(frame_id)

    def scores(self, qd, frame_id, p, count=None):
        qd = np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
        qd = qd[:min(max(len(qd) if count is None else int(count), 0), self.max_features)]
        out = np.full(self.capacity, -1, np.int32)
        for k in range(self.capacity):
            if self.eligible(k, frame_id, p["min_gap"]):
                out[k] = int(votes(qd, self.slots[k]["desc"], p).sum())
        return out

    def query(self, qd, frame_id, p=None, count=None):
        """-> (scores int32 [capacity], candidates CANDIDATE_DTYPE [n])."""
        p = params() if p is None else p
        scores = self.scores(qd, frame_id, p, count)
        ks = [k for k in range(self.capacity) if scores[k] >= 0 and scores[k] >= p["min_score"]]
        ks.sort(key=lambda k: (-int(scores[k]), self.slots[k]["frame_id"], k))
        ks = ks[:p["max_candidates"]]
        cand = np.zeros(len(ks), CANDIDATE_DTYPE)
        for r, k in enumerate(ks):
            cand[r] = (k, scores[k], self.slots[k]["frame_id"])
        return scores, cand


MODULE_DEFAULTS = dict(capacity=256, keyframe_interval=5, verify=1, min_inliers=30, seed=0)


def loop_closure(frames, cam, place=None, ego=None, max_features=5000, **options):
    """The loop_closure module over a sequence.  frames = [(frame_id, kp, desc, landmarks, pose)] in order: the left features of the
    frame, ego_motion's landmarks of it (float64 [n, 4]) and the accumulated pose under pose_key (12 doubles).  -> LOOP_DTYPE [len(frames)].
    A record without a detection is all zeros."""
    o = dict(MODULE_DEFAULTS, **options)
    assert set(o) == set(MODULE_DEFAULTS)
    place = params() if place is None else place
    ego = E.params() if ego is None else ego
    ring = Ring(max_features, o["capacity"])
    poses = [None] * o["capacity"]
    out = np.zeros(len(frames), LOOP_DTYPE)
    for f, (fid, kp, desc, lm, pose) in enumerate(frames):
        if fid % o["keyframe_interval"]:
            continue
        _, cand = ring.query(desc, fid, place)
        for c in cand[:o["verify"]]:
            s = ring.slots[int(c["slot"])]
            matches = M.match(desc, s["desc"], M.params(use_gate=0, max_distance=place["max_distance"], ratio=place["ratio"], cross_check=1))[0]
            res = E.estimate(cam, ego, lm, kp, s["landmarks"], matches, seed=o["seed"], frame_id=fid, capacity=max_features)[0]
            if int(res["status"][0]) == 1 and int(res["n_inliers"][0]) >= o["min_inliers"]:
                r = out[f]
                r["detected"], r["slot"], r["score"], r["keyframe_id"] = 1, c["slot"], c["score"], c["frame_id"]
                r["relative"] = res[0]
                r["pose_keyframe"] = poses[int(c["slot"])]
                r["pose_loop"] = E.chain(list(poses[int(c["slot"])]), res)
                break
        poses[ring.insert(desc, fid, kp, lm)] = [float(v) for v in pose]
    return out
