// scene_demo.cpp -- a headless caller that puts moving actors into views and sweeps of a map set, through the drop-in facade and the
// C-ABI only.  `views` holds u32 n and n camera->world poses of 16 floats (they serve as the sensor's poses too); every actor is a
// map file and a pose file: u32 n, n actor->world poses of 16 floats (Eigen's column-major 4x4), n bytes of presence.  The camera
// is w x h with fx fy cx cy; the sensor is 180 x 8 at 2 degrees from -179, elevations -14 .. 0, 1 .. 60 m.
// SurfelMapping::acquireSceneImages (holes filled, depth written) and acquireSceneSweeps write <out_dir>/image, semantic, depth and
// velodyne; then the blended view is switched on and the scene call must refuse.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

static bool read_poses(const char *path, std::vector<Eigen::Matrix4f> &poses, std::vector<uint8_t> *present)
{
    FILE *f = std::fopen(path, "rb");
    uint32_t n = 0;
    if (!f || std::fread(&n, 4, 1, f) != 1) return false;
    poses.resize(n);
    for (auto &p : poses)
        if (std::fread(p.data(), 4, 16, f) != 16) return false;
    if (present) {
        present->resize(n);
        if (n && std::fread(present->data(), 1, n, f) != n) return false;
    }
    std::fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 11) {
        std::printf("usage: scene_demo max_sqrt_vertices views.bin out_dir w h fx fy cx cy n_static [static map files...] [actor.bin actor_poses.bin]...\n");
        return 2;
    }
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    const float fx = (float)std::atof(argv[6]), fy = (float)std::atof(argv[7]), cx = (float)std::atof(argv[8]), cy = (float)std::atof(argv[9]);
    Config::getInstance(fx, fy, cx, cy, w, h);
    Config::maxSqrtVertices() = std::atoi(argv[1]);
    SurfelMapping core;
    std::vector<Eigen::Matrix4f> views;
    if (!read_poses(argv[2], views, nullptr)) return 2;
    const int n_static = std::atoi(argv[10]);
    if (n_static < 0 || 11 + n_static > argc || (argc - 11 - n_static) % 2) return 2;
    std::vector<std::string> files;
    for (int i = 0; i < n_static; ++i) files.push_back(argv[11 + i]);
    std::vector<SceneActor> actors;
    for (int i = 11 + n_static; i < argc; i += 2) {
        SceneActor a;
        a.file = argv[i];
        if (!read_poses(argv[i + 1], a.poses, &a.present)) return 2;
        actors.push_back(a);
    }

    sm_lidar_sensor sn;
    if (sm_default_lidar_sensor(&sn) != SM_OK) return 1;
    const float el[8] = {-14, -12, -10, -8, -6, -4, -2, 0};
    sn.n_az = 180; sn.n_el = 8; sn.az0_deg = -179.0f; sn.az_step_deg = 2.0f; sn.el_deg = el;

    core.setFillHoles(true);
    core.setWriteDepth(true);
    if (!core.acquireSceneImages(argv[3], files, false, actors, views, w, h, fx, fy, cx, cy)) return 1;
    if (!core.acquireSceneSweeps(argv[3], files, false, actors, views, sn)) return 1;
    sm_scene_stats_t st;
    if (sm_scene_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("views %zu actors %u files %u records %llu\n", views.size(), st.actors, st.files, (unsigned long long)st.records);
    core.setBlend(true);
    if (core.acquireSceneImages(argv[3], files, false, actors, views, w, h, fx, fy, cx, cy)) return 1;
    std::printf("blend refused\n");
    return 0;
}
