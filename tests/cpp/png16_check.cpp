// png16_check.cpp -- host only: sm_png::write16 (facade/sm_png.h) against the reader's decoder (sm_png::read, facade/KittiReader.h).
// A 16-bit grey PNG of every size in a small set -- one pixel, odd sizes, a row longer than a stored deflate block (65535 bytes) --
// is written and read back: size, bit depth, channel count and every big-endian sample must come back.  The extremes 0, 1, 255,
// 256, 65535 are in every image.  Also: write16 refuses empty sizes, and the 8-bit writer still round-trips.
// usage: png16_check <dir>; prints "ok <images>" and returns 0, or names what differs and returns 1.
#include <cstdio>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/sm_png.h"
#include "../../surfelmapping_amd/csrc/facade/KittiReader.h"

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: png16_check dir\n"); return 2; }
    const std::string dir = argv[1];
    const int sizes[][2] = {{1, 1}, {2, 2}, {7, 5}, {131, 37}, {40000, 3}, {3, 300}};
    const uint16_t edge[5] = {0, 1, 255, 256, 65535};
    int images = 0;
    for (const auto &wh : sizes) {
        const int w = wh[0], h = wh[1];
        std::vector<uint16_t> img((size_t)w * h);
        uint32_t x = 12345u + (uint32_t)w;
        for (size_t i = 0; i < img.size(); ++i) {
            x = x * 1664525u + 1013904223u;
            img[i] = i < 5 ? edge[i] : (uint16_t)(x >> 16);
        }
        const std::string path = dir + "/d" + std::to_string(images) + ".png";
        if (!sm_png::write16(path.c_str(), img.data(), w, h)) { std::printf("write16 failed: %s\n", path.c_str()); return 1; }
        sm_png::Image im;
        if (!sm_png::read(path, im)) { std::printf("read failed: %s\n", path.c_str()); return 1; }
        if (im.w != w || im.h != h || im.channels != 1 || im.depth != 16 || im.data.size() != img.size() * 2) {
            std::printf("header differs: %s\n", path.c_str());
            return 1;
        }
        for (size_t i = 0; i < img.size(); ++i)
            if ((uint16_t)((im.data[i * 2] << 8) | im.data[i * 2 + 1]) != img[i]) { std::printf("sample %zu differs: %s\n", i, path.c_str()); return 1; }
        ++images;
    }
    uint16_t one = 7;
    if (sm_png::write16((dir + "/bad.png").c_str(), &one, 0, 1) || sm_png::write16((dir + "/bad.png").c_str(), &one, 1, -1)) {
        std::printf("write16 accepted an empty size\n");
        return 1;
    }
    const uint8_t rgb[2 * 2 * 3] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 250, 251, 252};
    const std::string p8 = dir + "/c.png";
    sm_png::Image im;
    if (!sm_png::write(p8.c_str(), rgb, 2, 2, 3) || !sm_png::read(p8, im) || im.depth != 8 || im.channels != 3 ||
        im.data != std::vector<uint8_t>(rgb, rgb + 12)) {
        std::printf("8-bit round trip differs\n");
        return 1;
    }
    std::printf("ok %d\n", images);
    return 0;
}
