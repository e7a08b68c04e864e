// engine_voxelmap.h -- the cart_voxel_map device object (spec S33), for the host translation units that read its grid: engine_voxelmap.hip,
// which owns it, and engine_modeltrack.hip (S34), which only reads the volume.  Private to csrc/.
#pragma once

#include "engine_host.h"

extern "C" {

struct cart_voxel_map : cart_amd::DeviceObject {
    using cart_amd::DeviceObject::DeviceObject;
    int n[3] = {0, 0, 0};                   // nx, ny, nz
    cart_voxel_map_params p{};
    uint32_t *voxels = nullptr;             // [nz][ny][nx], toroidal (engine_internal.h, VoxelGrid)
    int32_t *counters = nullptr;            // [kVoxelCounters]
    bool valid = false;                     // a window exists (guarded by mu)
    int64_t o[3] = {0, 0, 0};               // its origin in absolute voxels
    uint32_t *mesh_cells = nullptr;         // cart_voxel_map_mesh's workspace (S36), allocated by its first call: [nz ny nx] cell words ...
    uint32_t *mesh_blocks = nullptr;        // ... and [2][nz ny nx / kMeshBlock] per-workgroup counts
};

}  // extern "C"

namespace cart_amd {

inline int floor_mod(int64_t a, int n) { return (int)(((a % n) + n) % n); }

inline VoxelGrid grid_of(const cart_voxel_map *m) {
    return VoxelGrid{m->voxels, m->n[0], m->n[1], m->n[2], floor_mod(m->o[0], m->n[0]), floor_mod(m->o[1], m->n[1]), floor_mod(m->o[2], m->n[2]),
                     (double)m->o[0], (double)m->o[1], (double)m->o[2]};
}

}  // namespace cart_amd
