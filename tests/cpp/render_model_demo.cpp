// render_model_demo.cpp -- a caller that builds a map through the drop-in facade (as facade_demo.cpp does) and then asks
// GlobalModel::renderModelImage for the model view in the reference's draw modes (build_map.cpp:190 passes renderModel the
// GUI's switches).  Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame rgb|depth|sem|pose16); the camera
// from a second file (f64 mvp[16], f64 mv[16], i32 w, h).  Writes the map and, per mode, the w*h*4 RGBA bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) { std::printf("usage: render_model_demo frames.bin camera.bin out_map.bin out_images.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    Config::maxSqrtVertices() = 1000;
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    for (int k = 0; k < n; ++k) {
        Eigen::Matrix4f pose;
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
    }
    std::fclose(f);
    FILE *c = std::fopen(argv[2], "rb");
    if (!c) return 2;
    pangolin::OpenGlMatrix mvp{}, mv{};
    int32_t vw = 0, vh = 0;
    if (std::fread(mvp.m, 8, 16, c) != 16 || std::fread(mv.m, 8, 16, c) != 16 || std::fread(&vw, 4, 1, c) != 1 ||
        std::fread(&vh, 4, 1, c) != 1) return 2;
    std::fclose(c);
    FILE *o = std::fopen(argv[4], "wb");
    if (!o) return 2;
    const float clear[4] = {0.2f, 0.4f, 0.6f, 1.0f};
    struct Mode { bool normals, colors, points, window, semantic; };
    const Mode modes[] = {{false, false, false, false, false}, {true, false, false, false, false}, {false, true, false, false, false},
                          {false, false, false, false, true}, {false, false, false, true, false}, {false, true, true, false, false}};
    for (const Mode &m : modes) {
        GlobalModel &gm = core.getGlobalModel();
        if (!gm.renderModelImage(mvp, mv, 0.5f, true, m.normals, m.colors, m.points, m.window, m.semantic, n, 1, vw, vh, clear)) return 1;
        std::fwrite(gm.modelImageRGBA().data(), 1, gm.modelImageRGBA().size(), o);
    }
    std::fclose(o);
    std::printf("model %u\n", core.getGlobalModel().getModel().second);
    return core.getGlobalModel().downloadMap(argv[3], 0, n - 1) ? 0 : 1;
}
