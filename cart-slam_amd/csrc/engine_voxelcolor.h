// engine_voxelcolor.h -- the cart_voxel_color device object (spec S37), for the host translation units that read its grid:
// engine_voxelcolor.hip, which owns it, and engine_modeltrack_color.hip (S38), which only reads the colour volume.  Private to csrc/.
#pragma once

#include "engine_host.h"
#include "engine_voxelmap.h"

extern "C" {

struct cart_voxel_color : cart_amd::DeviceObject {
    using cart_amd::DeviceObject::DeviceObject;
    int n[3] = {0, 0, 0};                   // nx, ny, nz: the map's
    cart_voxel_map_params p{};              // the map's, copied at create
    int max_weight = CART_VOXEL_COLOR_DEFAULT_MAX_WEIGHT;
    uint32_t *voxels = nullptr;             // [nz][ny][nx] words b | g << 8 | r << 16 | weight << 24, toroidal (engine_internal.h, VoxelGrid)
    int32_t *counters = nullptr;            // [kColorCounters]
    bool valid = false;                     // a window exists (guarded by mu)
    int64_t o[3] = {0, 0, 0};               // its origin in absolute voxels
};

}  // extern "C"

namespace cart_amd {

inline VoxelGrid color_grid(const cart_voxel_color *c) {
    return VoxelGrid{c->voxels, c->n[0], c->n[1], c->n[2], floor_mod(c->o[0], c->n[0]), floor_mod(c->o[1], c->n[1]), floor_mod(c->o[2], c->n[2]),
                     (double)c->o[0], (double)c->o[1], (double)c->o[2]};
}

}  // namespace cart_amd
