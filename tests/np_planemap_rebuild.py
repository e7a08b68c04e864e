"""numpy restatement of spec S30: rebuilding the plane map from stored keyframes.  Written from the spec on top of
np_planemap (votes, window_origin, empty_cells): a ring store with a host id table, and rebuild(map, store, ids, poses, window_pose),
which empties the window of window_pose and adds every stored entry's S24 votes through the entry's own pose."""
import numpy as np

import np_planemap as M


class Store:
    """cart_plane_store restated: insertion n (from 0 since create / clear) goes to slot n mod capacity; the images are kept verbatim."""

    def __init__(self, width, height, capacity):
        self.width, self.height, self.capacity = int(width), int(height), int(capacity)
        self.clear()

    def clear(self):
        self.inserted = 0
        self.ids = [None] * self.capacity
        self.frames = [None] * self.capacity

    def insert(self, frame_id, disp, planes):
        disp, planes = np.asarray(disp), np.asarray(planes)
        assert disp.shape == planes.shape == (self.height, self.width)
        slot = self.inserted % self.capacity
        self.ids[slot], self.frames[slot] = int(frame_id), (disp.astype(np.int16).copy(), planes.astype(np.uint8).copy())
        self.inserted += 1

    def size(self):
        return min(self.inserted, self.capacity), self.capacity

    def slot_of(self, frame_id):
        """Newest first, so a repeated id names its latest insertion; -1 when the id is not held."""
        for n in range(self.inserted - 1, max(self.inserted - self.capacity, 0) - 1, -1):
            if self.ids[n % self.capacity] == int(frame_id):
                return n % self.capacity
        return -1

    def contains(self, frame_id):
        return self.slot_of(frame_id) >= 0


def add_votes(cells, origin, cam, p, pose, disp, planes):
    """One frame's S24 votes into `cells` (window order, origin fixed); votes outside the window are dropped."""
    nz, nx = cells.shape
    ox, oz = origin
    gx, gz, l, q = M.votes(cam, p, pose, disp, planes)
    inside = (gx >= ox) & (gx < ox + nx) & (gz >= oz) & (gz < oz + nz)
    cx, cz = (gx[inside] - ox).astype(np.int64), (gz[inside] - oz).astype(np.int64)
    l, q = l[inside], q[inside]
    for label, field in ((0, "horizontal"), (1, "vertical")):
        count = np.zeros((nz, nx), np.int64)
        np.add.at(count, (cz[l == label], cx[l == label]), 1)
        cells[field] = ((cells[field].astype(np.int64) + count) & 0xFFFFFFFF).astype(np.uint32)
    lo, hi = cells["y_min"].astype(np.int64), cells["y_max"].astype(np.int64)
    np.minimum.at(lo, (cz[l == 1], cx[l == 1]), q[l == 1])
    np.maximum.at(hi, (cz[l == 1], cx[l == 1]), q[l == 1])
    cells["y_min"], cells["y_max"] = lo.astype(np.int32), hi.astype(np.int32)


def rebuild(m, store, ids, poses, window_pose):
    """m = np_planemap.Map.  -> used = the entries whose id the store holds.  Afterwards m is valid at the window of window_pose."""
    P = np.asarray(window_pose, np.float64).reshape(12)
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    assert len(poses) == len(ids)
    m.origin = (M.window_origin(P[3], m.p["cell_size"], m.nx), M.window_origin(P[11], m.p["cell_size"], m.nz))
    m.cells = M.empty_cells(m.nz, m.nx)
    used = 0
    for frame_id, pose in zip(ids, poses):
        slot = store.slot_of(frame_id)
        if slot < 0:
            continue
        used += 1
        add_votes(m.cells, m.origin, m.cam, m.p, pose, *store.frames[slot])
    return used
