// cart_slam_amd <source.json> <modules.json> [--frames N] [--dump DIR] [--sequential 1] [--inflight N] [--timing FILE.csv]
// (--sequential 1 finishes every frame before the next starts: the cumulative plane histogram then sees the frames in id
//  order, which the reference's concurrent frame loop does not guarantee)
// Frame loop of the reference's src/main.cpp:8-63 without logging/UI; --dump writes every frame's blackboard images as
// raw little-endian files (<DIR>/<id>_<key>.bin) so that tests can compare them with the oracle.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <deque>
#include <future>
#include <fstream>
#include <iostream>
#include <vector>

#include "cartslam_amd/cartconfig.hpp"
#include "cartslam_amd/modules/depth.hpp"
#include "cartslam_amd/modules/egomotion.hpp"
#include "cartslam_amd/modules/features.hpp"
#include "cartslam_amd/modules/matches.hpp"
#include "cartslam_amd/modules/denseego.hpp"
#include "cartslam_amd/modules/fusion.hpp"
#include "cartslam_amd/modules/localba.hpp"
#include "cartslam_amd/modules/loopclosure.hpp"
#include "cartslam_amd/modules/motionseg.hpp"
#include "cartslam_amd/modules/objects.hpp"
#include "cartslam_amd/timing.hpp"
#include "cartslam_amd/modules/planefit.hpp"
#include "cartslam_amd/modules/planemap.hpp"
#include "cartslam_amd/modules/planeseg.hpp"
#include "cartslam_amd/modules/posegraph.hpp"
#include "cartslam_amd/modules/voxelmap.hpp"

namespace {
// --dump: <dir>/<id>_<name>.bin gets `bytes` bytes; what a record has beyond its first part is appended to the returned file
void append(std::ofstream &o, const void *p, size_t bytes) {
    if (bytes) o.write(static_cast<const char *>(p), (std::streamsize)bytes);
}
std::ofstream writeBin(const std::string &dir, int id, const std::string &name, const void *p, size_t bytes) {
    std::ofstream o(dir + "/" + std::to_string(id) + "_" + name + ".bin", std::ios::binary);
    append(o, p, bytes);
    return o;
}
void writeBin(const std::string &dir, int id, const std::string &name, const std::vector<uint8_t> &tight) { writeBin(dir, id, name, tight.data(), tight.size()); }
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        std::cerr << "Usage: " << argv[0] << " <data source config file> <module config file> [--frames N] [--dump DIR]\n";
        return 1;
    }
    int maxFrames = 1 << 30;
    std::string dump;
    bool sequential = false;
    for (int i = 3; i + 1 < argc; i += 2) {
        if (!std::strcmp(argv[i], "--frames")) maxFrames = std::atoi(argv[i + 1]);
        else if (!std::strcmp(argv[i], "--dump")) { dump = argv[i + 1]; setenv("CARTSLAM_PLANE_MAP_SNAPSHOT", "1", 1); }  // plane_map keeps every frame's cells
        else if (!std::strcmp(argv[i], "--sequential")) sequential = std::atoi(argv[i + 1]) != 0;
        else if (!std::strcmp(argv[i], "--inflight")) setenv("CARTSLAM_CONCURRENT_RUN_LIMIT", argv[i + 1], 1);  // frames in flight (reference: 12)
        else if (!std::strcmp(argv[i], "--timing")) cart::timing::Sink::instance().open(argv[i + 1]);
    }
    try {
        auto dataSource = cart::config::readDataSourceConfig(argv[1]);
        const size_t inflight = cart::concurrentRunLimit();
        auto system = std::make_shared<cart::System>(dataSource, std::max<size_t>(CARTSLAM_RUN_RETENTION, inflight + 8), inflight);
        cart::config::readModuleConfig(argv[2], system);
        std::deque<std::future<void>> pending;   // at most `inflight` + 1 entries: finished frames are reaped as the loop goes
        int frames = 0, failed = 0;
        auto reap = [&](bool all) {
            while (!pending.empty() && (all || pending.front().wait_for(std::chrono::seconds(0)) == std::future_status::ready)) {
                try { pending.front().get(); } catch (const std::exception &e) { std::cerr << "Error in processing: " << e.what() << "\n"; ++failed; }
                pending.pop_front();
            }
        };
        while (!dataSource->isFinished() && frames < maxFrames) {
            if (!dataSource->isNextReady()) continue;
            pending.push_back(system->run());
            if (sequential) pending.back().wait();
            ++frames;
            reap(false);
        }
        reap(true);
        if (!dump.empty()) {
            const char *keys[] = {CARTSLAM_KEY_DISPARITY, CARTSLAM_KEY_DISPARITY_DERIVATIVE, CARTSLAM_KEY_DISPARITY_DERIVATIVE_HISTOGRAM, CARTSLAM_KEY_PLANES,
                                  CARTSLAM_KEY_PLANE_COMPONENTS, CARTSLAM_KEY_DEPTH, CARTSLAM_KEY_PLANES_UNSMOOTHED, CARTSLAM_KEY_SUPERPIXELS, CARTSLAM_KEY_OPTFLOW,
                                  CARTSLAM_KEY_PLANE_COMPONENT_TABLE, CARTSLAM_KEY_PLANE_COMPONENT_COUNT, CARTSLAM_KEY_PLANES_STATIC, CARTSLAM_KEY_MOTION_COMPONENTS,
                                  CARTSLAM_KEY_MOTION_COMPONENT_TABLE, CARTSLAM_KEY_MOTION_COMPONENT_COUNT};
            for (int id = 1; id <= frames; ++id) {
                std::shared_ptr<cart::SystemRunData> run;
                try { run = system->getRunById((uint32_t)id); } catch (const std::exception &) { continue; }  // evicted (retention ring)
                if (run->hasData(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL)) {
                    const cart::contour::label_t mx = *run->getData<cart::contour::label_t>(CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL);
                    writeBin(dump, id, CARTSLAM_KEY_SUPERPIXELS_MAX_LABEL, &mx, sizeof(mx));
                }
                if (run->hasData(CARTSLAM_KEY_PLANES_EQ)) {   // planes f64 [N][4], assignments u64 [max_label + 1]
                    auto pf = run->getData<cart::plane_fit_data_t>(CARTSLAM_KEY_PLANES_EQ);
                    writeBin(dump, id, CARTSLAM_KEY_PLANES_EQ "_planes", pf->planes.data(), pf->planes.size() * sizeof(cart::Vec4d));
                    std::vector<uint64_t> as(pf->planeAssignments.begin(), pf->planeAssignments.end());
                    writeBin(dump, id, CARTSLAM_KEY_PLANES_EQ "_assignments", as.data(), as.size() * sizeof(uint64_t));
                }
                if (run->hasData(CARTSLAM_KEY_FEATURES)) {   // keypoints: 28-byte cv::KeyPoint records; descriptors: n x 32 bytes
                    auto f = run->getData<std::pair<cart::ImageFeatures, cart::ImageFeatures>>(CARTSLAM_KEY_FEATURES);
                    const std::pair<const char *, const cart::ImageFeatures *> sides[] = {{"left", &f->first}, {"right", &f->second}};
                    for (const auto &side : sides) {
                        const std::string base = std::string(CARTSLAM_KEY_FEATURES) + "_" + side.first;
                        writeBin(dump, id, base + "_keypoints", side.second->keypoints.data(), side.second->keypoints.size() * sizeof(cart::KeyPoint));
                        std::vector<uint8_t> d((size_t)side.second->descriptors.rows * CART_ORB_DESCRIPTOR_BYTES);
                        if (!d.empty()) side.second->descriptors.download(d.data(), CART_ORB_DESCRIPTOR_BYTES);
                        writeBin(dump, id, base + "_descriptors", d);
                    }
                }
                if (run->hasData(CARTSLAM_KEY_FEATURE_MATCHES)) {   // 16-byte cart_match records; an empty list gives an empty file
                    auto fm = run->getData<cart::FeatureMatches>(CARTSLAM_KEY_FEATURE_MATCHES);
                    const std::pair<const char *, const std::vector<cart::FeatureMatch> *> lists[] = {{"stereo", &fm->stereo}, {"temporal", &fm->temporal}};
                    for (const auto &list : lists)
                        writeBin(dump, id, std::string(CARTSLAM_KEY_FEATURE_MATCHES) + "_" + list.first, list.second->data(), list.second->size() * sizeof(cart::FeatureMatch));
                }
                if (run->hasData(CARTSLAM_KEY_EGO_MOTION)) {   // the 120-byte cart_ego_result, then the pose as 12 doubles
                    auto ego = run->getData<cart::EgoMotion>(CARTSLAM_KEY_EGO_MOTION);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_EGO_MOTION, &ego->result, sizeof(ego->result));
                    append(o, ego->pose, sizeof(ego->pose));
                }
                if (run->hasData(CARTSLAM_KEY_DENSE_EGO)) {   // the 136-byte cart_dense_ego_result, then the chained pose as 12 doubles
                    auto dense = run->getData<cart_dense_ego_result>(CARTSLAM_KEY_DENSE_EGO_RESULT);
                    auto chained = run->getData<cart::EgoMotion>(CARTSLAM_KEY_DENSE_EGO);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_DENSE_EGO, dense.get(), sizeof(*dense));
                    append(o, chained->pose, sizeof(chained->pose));
                }
                if (run->hasData(CARTSLAM_KEY_LOOP_CLOSURE)) {   // the 336-byte LoopClosure record
                    auto loop = run->getData<cart::LoopClosure>(CARTSLAM_KEY_LOOP_CLOSURE);
                    writeBin(dump, id, CARTSLAM_KEY_LOOP_CLOSURE, loop.get(), sizeof(*loop));
                }
                if (run->hasData(CARTSLAM_KEY_POSE_GRAPH)) {   // the 48-byte PoseGraphRecord, then the corrected pose as 12 doubles; every node's estimate on a frame that optimised
                    auto record = run->getData<cart::PoseGraphRecord>(CARTSLAM_KEY_POSE_GRAPH_RESULT);
                    auto corrected = run->getData<cart::EgoMotion>(CARTSLAM_KEY_POSE_GRAPH);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_POSE_GRAPH, record.get(), sizeof(*record));
                    append(o, corrected->pose, sizeof(corrected->pose));
                    auto nodes = run->getData<std::vector<double>>(CARTSLAM_KEY_POSE_GRAPH_NODES);
                    if (!nodes->empty()) writeBin(dump, id, CARTSLAM_KEY_POSE_GRAPH "_nodes", nodes->data(), nodes->size() * sizeof(double));
                }
                if (run->hasData(CARTSLAM_KEY_LOCAL_BA)) {   // the 80-byte LocalBARecord, the refined pose as 12 doubles, the window's ids (uint64) and poses, then the published R and t
                    auto record = run->getData<cart::LocalBARecord>(CARTSLAM_KEY_LOCAL_BA_RESULT);
                    auto refined = run->getData<cart::EgoMotion>(CARTSLAM_KEY_LOCAL_BA);
                    auto window = run->getData<cart::LocalBAWindow>(CARTSLAM_KEY_LOCAL_BA_WINDOW);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_LOCAL_BA, record.get(), sizeof(*record));
                    append(o, refined->pose, sizeof(refined->pose));
                    append(o, window->ids.data(), window->ids.size() * sizeof(uint64_t));
                    append(o, window->poses.data(), window->poses.size() * sizeof(double));
                    append(o, refined->result.R, sizeof(refined->result.R));
                    append(o, refined->result.t, sizeof(refined->result.t));
                }
                if (run->hasData(CARTSLAM_KEY_PLANE_MAP)) {   // int64 ox, oz; int32 Nx, Nz; double cell_size; the 16-byte cells; the u8 classes
                    auto pm = run->getData<cart::PlaneMap>(CARTSLAM_KEY_PLANE_MAP);
                    const int64_t origin[2] = {pm->originX, pm->originZ};
                    const int32_t shape[2] = {pm->cellsX, pm->cellsZ};
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_PLANE_MAP, origin, sizeof(origin));
                    append(o, shape, sizeof(shape));
                    append(o, &pm->cellSize, sizeof(pm->cellSize));
                    append(o, pm->cells.data(), pm->cells.size() * sizeof(cart_plane_map_cell));
                    const auto classes = pm->classes.downloadTight();
                    append(o, classes.data(), classes.size());
                    if (pm->rebuilt > 0) {   // a frame that rebuilt the grid (S30): int32 count, used; the ids as uint64
                        const int32_t counts[2] = {pm->rebuilt, pm->rebuildUsed};
                        std::ofstream r = writeBin(dump, id, CARTSLAM_KEY_PLANE_MAP "_rebuild", counts, sizeof(counts));
                        append(r, pm->rebuildIds.data(), pm->rebuildIds.size() * sizeof(uint64_t));
                    }
                }
                if (run->hasData(CARTSLAM_KEY_VOXEL_MAP)) {   // int64 origin [3]; int32 cells [3]; double voxel_size; int32 integrate counts [2], ray counts [3], width, height; the model (int16) and status (u8) images
                    auto vm = run->getData<cart::VoxelMap>(CARTSLAM_KEY_VOXEL_MAP);
                    auto rays = run->getData<cart::VoxelRayCounts>(CARTSLAM_KEY_DISPARITY_MODEL_COUNTS);
                    auto model = run->getData<cart::image_t>(CARTSLAM_KEY_DISPARITY_MODEL);
                    const int32_t shape[2] = {model->cols, model->rows};   // 0 x 0 without "raycast"
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_VOXEL_MAP, vm->origin, sizeof(vm->origin));
                    append(o, vm->cells, sizeof(vm->cells));
                    append(o, &vm->voxelSize, sizeof(vm->voxelSize));
                    append(o, vm->counts, sizeof(vm->counts));
                    append(o, rays->rays, sizeof(rays->rays));
                    append(o, shape, sizeof(shape));
                    if (!model->empty()) {
                        for (const char *k : {CARTSLAM_KEY_DISPARITY_MODEL, CARTSLAM_KEY_DISPARITY_MODEL_STATUS}) {
                            const auto bytes = run->getData<cart::image_t>(k)->downloadTight();
                            append(o, bytes.data(), bytes.size());
                        }
                    }
                    if (!vm->voxels.empty())   // with CARTSLAM_VOXEL_MAP_SNAPSHOT: the 4-byte voxels in window order
                        writeBin(dump, id, CARTSLAM_KEY_VOXEL_MAP "_voxels", vm->voxels.data(), vm->voxels.size() * sizeof(cart_voxel));
                    if (vm->rebuilt > 0) {   // a frame that rebuilt the volume (S35): int32 count, used; the ids as uint64 (the plane map's layout)
                        const int32_t counts[2] = {vm->rebuilt, vm->rebuildUsed};
                        std::ofstream r = writeBin(dump, id, CARTSLAM_KEY_VOXEL_MAP "_rebuild", counts, sizeof(counts));
                        append(r, vm->rebuildIds.data(), vm->rebuildIds.size() * sizeof(uint64_t));
                    }
                }
                if (run->hasData(CARTSLAM_KEY_VOXEL_MESH)) {   // voxel_map with "mesh", on the frames that extracted: int64 origin [3]; double voxel_size; int32 counts [4]; the written vertices (24 bytes) and quads (16 bytes)
                    auto mesh = run->getData<cart::VoxelMesh>(CARTSLAM_KEY_VOXEL_MESH);
                    if (mesh->extracted) {
                        std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_VOXEL_MESH, mesh->origin, sizeof(mesh->origin));
                        append(o, &mesh->voxelSize, sizeof(mesh->voxelSize));
                        append(o, mesh->counts, sizeof(mesh->counts));
                        append(o, mesh->vertices.data(), mesh->vertices.size() * sizeof(cart_mesh_vertex));
                        append(o, mesh->quads.data(), mesh->quads.size() * sizeof(cart_mesh_quad));
                    }
                }
                if (run->hasData(CARTSLAM_KEY_VOXEL_COLOR)) {   // voxel_map with "color": int32 integrated, colour counts [2], rendered, width, height; the model image (B, G, R) and its alpha (u8)
                    auto vc = run->getData<cart::VoxelColorFrame>(CARTSLAM_KEY_VOXEL_COLOR);
                    auto image = run->getData<cart::image_t>(CARTSLAM_KEY_IMAGE_MODEL);
                    const int32_t head[6] = {vc->integrated ? 1 : 0, vc->counts[0], vc->counts[1], vc->rendered, image->cols, image->rows};   // 0 x 0 without "raycast"
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_VOXEL_COLOR, head, sizeof(head));
                    if (!image->empty()) {
                        for (const char *k : {CARTSLAM_KEY_IMAGE_MODEL, CARTSLAM_KEY_IMAGE_MODEL_ALPHA}) {
                            const auto bytes = run->getData<cart::image_t>(k)->downloadTight();
                            append(o, bytes.data(), bytes.size());
                        }
                    }
                    if (!vc->voxels.empty()) {   // with CARTSLAM_VOXEL_MAP_SNAPSHOT: int64 origin [3], then the 4-byte colour voxels in window order
                        std::ofstream v = writeBin(dump, id, CARTSLAM_KEY_VOXEL_COLOR "_voxels", vc->origin, sizeof(vc->origin));
                        append(v, vc->voxels.data(), vc->voxels.size() * sizeof(cart_voxel_rgb));
                    }
                }
                if (run->hasData(CARTSLAM_KEY_VOXEL_MESH_COLORS)) {   // with "color" and "mesh", on the frames that extracted: int32 count, then one 4-byte (b, g, r, alpha) per written vertex
                    auto colors = run->getData<cart::VoxelMeshColors>(CARTSLAM_KEY_VOXEL_MESH_COLORS);
                    if (colors->extracted) {
                        const int32_t count = (int32_t)colors->colors.size();
                        std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_VOXEL_MESH_COLORS, &count, sizeof(count));
                        append(o, colors->colors.data(), colors->colors.size() * sizeof(cart_voxel_rgb));
                    }
                }
                if (run->hasData(CARTSLAM_KEY_MODEL_POSE)) {   // voxel_map with "track": the 136-byte cart_model_track_result, then the tracked pose as 12 doubles
                    auto record = run->getData<cart_model_track_result>(CARTSLAM_KEY_MODEL_TRACK_RESULT);
                    auto tracked = run->getData<cart::EgoMotion>(CARTSLAM_KEY_MODEL_POSE);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_MODEL_POSE, record.get(), sizeof(*record));
                    append(o, tracked->pose, sizeof(tracked->pose));
                }
                if (run->hasData(CARTSLAM_KEY_MODEL_TRACK_COLOR_RESULT)) {   // voxel_map with "track_color": the 176-byte cart_model_track_color_result
                    auto record = run->getData<cart_model_track_color_result>(CARTSLAM_KEY_MODEL_TRACK_COLOR_RESULT);
                    writeBin(dump, id, "model_track_color", record.get(), sizeof(*record));
                }
                if (run->hasData(CARTSLAM_KEY_MOTION)) {   // int32 width, height; the filtered labels, the raw labels, the residual records
                    auto labels = run->getData<cart::image_t>(CARTSLAM_KEY_MOTION);
                    const int32_t shape[2] = {labels->cols, labels->rows};
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_MOTION, shape, sizeof(shape));
                    for (const char *k : {CARTSLAM_KEY_MOTION, CARTSLAM_KEY_MOTION_UNSMOOTHED, CARTSLAM_KEY_MOTION_RESIDUAL}) {
                        const auto bytes = run->getData<cart::image_t>(k)->downloadTight();
                        append(o, bytes.data(), bytes.size());
                    }
                }
                if (run->hasData(CARTSLAM_KEY_DISPARITY_FUSED)) {   // int32 width, height; fused (int16), age, source (u8); the five int32 counts
                    auto fused = run->getData<cart::image_t>(CARTSLAM_KEY_DISPARITY_FUSED);
                    const int32_t shape[2] = {fused->cols, fused->rows};
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_DISPARITY_FUSED, shape, sizeof(shape));
                    for (const char *k : {CARTSLAM_KEY_DISPARITY_FUSED, CARTSLAM_KEY_DISPARITY_AGE, CARTSLAM_KEY_DISPARITY_SOURCE}) {
                        const auto bytes = run->getData<cart::image_t>(k)->downloadTight();
                        append(o, bytes.data(), bytes.size());
                    }
                    auto counts = run->getData<cart::FusionCounts>(CARTSLAM_KEY_DISPARITY_FUSION_COUNTS);
                    append(o, counts->pixels, sizeof(counts->pixels));
                }
                if (run->hasData(CARTSLAM_KEY_MOVING_OBJECTS)) {   // int32 counts [8]; the n_objects 192-byte cart_object records; the live 96-byte cart_track records
                    auto mo = run->getData<cart::MovingObjects>(CARTSLAM_KEY_MOVING_OBJECTS);
                    std::ofstream o = writeBin(dump, id, CARTSLAM_KEY_MOVING_OBJECTS, mo->counts, sizeof(mo->counts));
                    append(o, mo->objects.data(), mo->objects.size() * sizeof(cart_object));
                    append(o, mo->tracks.data(), mo->tracks.size() * sizeof(cart_track));
                }
                if (run->hasData(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES)) {   // f64 [max_label + 1][4]
                    auto lp = run->getData<std::vector<cart::Vec4d>>(CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES);
                    writeBin(dump, id, CARTSLAM_KEY_PLANES_EQ_LABEL_PLANES, lp->data(), lp->size() * sizeof(cart::Vec4d));
                }
                for (const char *k : keys) {
                    if (!run->hasData(k)) continue;
                    auto img = run->getData<cart::image_t>(k);
                    if (!img) continue;  // e.g. "optflow" of the first frame (optflow.cpp:126-128)
                    writeBin(dump, id, k, img->downloadTight());
                }
            }
        }
        if (!dump.empty()) {
            std::ofstream q(dump + "/Q.bin", std::ios::binary);
            const cart::CameraIntrinsics K = dataSource->getCameraIntrinsics();
            append(q, K.Q, sizeof(K.Q));
        }
        std::cout << "frames " << frames << " failed " << failed;
        for (const auto &m : system->getModules())
            if (auto d = std::dynamic_pointer_cast<cart::ImageDisparityModule>(m)) std::cout << " frames_per_launch " << d->meanFramesPerLaunch();
            else if (auto c = std::dynamic_pointer_cast<cart::SuperPixelPlaneClusterModule>(m)) std::cout << " merge_ms " << c->meanMergeMs();
        std::cout << "\n";
        return failed ? 2 : 0;
    } catch (const std::exception &e) {
        std::cerr << "fatal: " << e.what() << "\n";
        return 1;
    }
}
