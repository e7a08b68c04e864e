"""numpy restatement of spec S35: rebuilding the TSDF volume from stored keyframes.  Written from the spec on top of
np_voxelmap.Map, whose integrate first moves the window and then works from self.origin: a subclass whose _move does nothing while a rebuild
runs is the fixed-window integrate, with no second copy of the gates.  The store is S30's restatement (np_planemap_rebuild.Store: a ring,
ids, newest first), reused as it is."""
import numpy as np

import np_voxelmap as V
from np_planemap_rebuild import Store  # noqa: F401  (the store of S30, for the callers of this module)


class Map(V.Map):
    """np_voxelmap.Map with rebuild().  Everything else is inherited: integrate, raycast and read continue after a rebuild as after any integrate."""

    _fixed = False

    def _move(self, o):
        if not self._fixed:
            super()._move(o)

    def rebuild(self, store, ids, poses, window_pose, cam, use_mask=False):
        """-> ((ox, oy, oz), used, counts int64 [2]): the window of window_pose, emptied; then every entry whose id the store holds, in list
        order, through its own pose into that fixed window.  counts = the voxel updates over all used entries, of them with f < 1."""
        poses = np.asarray(poses, np.float64).reshape(-1, 12)
        assert len(poses) == len(ids)
        self.clear()
        self.origin = V.window_origin(window_pose, self.p, (self.nx, self.ny, self.nz))
        used, counts = 0, np.zeros(2, np.int64)
        self._fixed = True
        try:
            for frame_id, pose in zip(ids, poses):
                slot = store.slot_of(frame_id)
                if slot < 0:
                    continue
                disp, plane = store.frames[slot]
                counts += self.integrate(cam, pose, disp, plane if use_mask else None).astype(np.int64)
                used += 1
        finally:
            self._fixed = False
        return self.origin, used, counts
