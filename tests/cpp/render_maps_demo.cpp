// render_maps_demo.cpp -- load_map.cpp's job for a drive that no longer fits the model: map a sequence through the drop-in
// facade with the periodic retirement on (retire_demo.cpp's loop), then look at the WHOLE map -- the files the retirement
// wrote plus the live model -- without loading it: SurfelMapping::acquireImages with the list of map files writes the novel
// views as PNGs, GlobalModel::renderModelImage with the same list the model view.  Frames come from a raw dump (u32 W,H,n; f32
// fx,fy,cx,cy; per frame rgb|depth|sem|pose16); the novel views from views.bin (u32 n; n x f32 pose16); the model view's
// camera from camera.bin (f64 mvp[16], f64 mv[16], i32 w, h).  Writes <out_dir>/image|semantic/%06d.png and, per draw mode,
// the w*h*4 RGBA bytes of the model view.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 11) {
        std::printf("usage: render_maps_demo frames.bin max_sqrt_vertices every min_age min_distance prefix views.bin camera.bin out_dir out_images.bin\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    if (!core.setAutoRetire(std::atoi(argv[3]), argv[6], std::atoi(argv[4]), (float)std::atof(argv[5]))) return 1;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    Eigen::Matrix4f pose;
    for (int k = 0; k < n; ++k) {
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
    }
    std::fclose(f);
    // the map set: what the retirement wrote, in writing order, then the live model
    std::vector<std::string> files;
    const auto st = core.autoRetireStats();
    for (unsigned i = 0; i < st.first; ++i) {
        char name[32];
        std::snprintf(name, sizeof name, "_%06u.bin", i);
        files.push_back(std::string(argv[6]) + name);
    }
    FILE *vf = std::fopen(argv[7], "rb");
    uint32_t nv = 0;
    if (!vf || std::fread(&nv, 4, 1, vf) != 1) return 2;
    std::vector<Eigen::Matrix4f> views(nv);
    for (auto &v : views) if (std::fread(v.data(), 4, 16, vf) != 16) return 2;
    std::fclose(vf);
    if (!core.acquireImages(argv[9], files, views, W, H, intr[0], intr[1], intr[2], intr[3], 3)) return 1;
    FILE *c = std::fopen(argv[8], "rb");
    if (!c) return 2;
    pangolin::OpenGlMatrix mvp{}, mv{};
    int32_t vw = 0, vh = 0;
    if (std::fread(mvp.m, 8, 16, c) != 16 || std::fread(mv.m, 8, 16, c) != 16 || std::fread(&vw, 4, 1, c) != 1 ||
        std::fread(&vh, 4, 1, c) != 1) return 2;
    std::fclose(c);
    FILE *o = std::fopen(argv[10], "wb");
    if (!o) return 2;
    const float clear[4] = {0.2f, 0.4f, 0.6f, 1.0f};
    GlobalModel &gm = core.getGlobalModel();
    // shaded discs, semantic discs, coloured points -- and the shaded discs of the files alone
    if (!gm.renderModelImage(mvp, mv, 0.5f, true, false, false, false, false, false, n, 1, vw, vh, clear, files)) return 1;
    std::fwrite(gm.modelImageRGBA().data(), 1, gm.modelImageRGBA().size(), o);
    if (!gm.renderModelImage(mvp, mv, 0.5f, true, false, false, false, false, true, n, 1, vw, vh, clear, files)) return 1;
    std::fwrite(gm.modelImageRGBA().data(), 1, gm.modelImageRGBA().size(), o);
    if (!gm.renderModelImage(mvp, mv, 0.5f, true, false, true, true, false, false, n, 1, vw, vh, clear, files)) return 1;
    std::fwrite(gm.modelImageRGBA().data(), 1, gm.modelImageRGBA().size(), o);
    if (!gm.renderModelImage(mvp, mv, 0.5f, true, false, false, false, false, false, n, 1, vw, vh, clear, files, false)) return 1;
    std::fwrite(gm.modelImageRGBA().data(), 1, gm.modelImageRGBA().size(), o);
    std::fclose(o);
    std::printf("files %u surfels %llu count %u views %u\n", st.first, st.second, core.getGlobalModel().getModel().second, nv);
    return 0;
}
