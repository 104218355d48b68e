// KittiReader.h -- drop-in for the reference's dataset reader (gui/DatasetReader.h:16-75,
// gui/KittiReader.{h,cpp}) without OpenCV: reads <dir>/image_2/%06d.png (RGB), <dir>/PSMNet/%06d.png (u16 depth in
// millimetres), <dir>/semantics/%06d.png (u8 train ids), calibration.txt ("fx fy cx cy" / "width height"), pose.txt
// (3x4 row-major camera->world per line, right-multiplied by the -0.06 m x-offset T20: gui/KittiReader.cpp:296-302)
// and times.txt.  With estimateDepth the reference skips PSMNet and hands on a null depth (gui/KittiReader.cpp:68,87); here the
// flag also reads the right camera's <dir>/image_3/%06d.png into rgbRight, for SurfelMapping::processFrameStereo.
// setUseLidar(true) (off by default) reads <dir>/velo_to_cam.txt (12 floats, a row-major 3 x 4: the odometry benchmark's Tr line)
// and, per frame, <dir>/velodyne/%06d.bin (x, y, z, reflectance as floats) into velodyne, for SurfelMapping::processFrameLidar; the
// frame's depth image is then not read (depth stays null).  With estimateDepth as well, both the right image and the scan are read.
// An empty scan is a frame with numPoints == 0 and velodyne not null.  setUseLidar(false) puts velodyne and numPoints back to none.
// PNG decoding: 8/16-bit grey, 8-bit RGB/RGBA, non-interlaced, all five filter types, zlib inflate (link with -lz).  Only subLevel == 0 is supported (the reference's sub-sampling branch is unused by build_map.cpp:279
// and writes the sub-sampled semantics into the depth buffer, gui/KittiReader.cpp:206).
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sm_compat.h"

namespace sm_png {

struct Image { int w = 0, h = 0, channels = 0, depth = 0; std::vector<uint8_t> data; /* rows of w*channels*(depth/8), big-endian for 16 bit */ };

inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

inline bool read(const std::string &path, Image &img)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (b.size() < 8 || std::memcmp(b.data(), sig, 8) != 0) return false;
    size_t pos = 8;
    std::vector<uint8_t> idat;
    int ctype = -1, interlace = 0;
    while (pos + 12 <= b.size()) {
        const uint32_t n = be32(&b[pos]);
        if (pos + 12 + n > b.size()) return false;
        const char *typ = (const char *)&b[pos + 4];
        const uint8_t *body = &b[pos + 8];
        if (!std::memcmp(typ, "IHDR", 4) && n >= 13) {
            img.w = (int)be32(body); img.h = (int)be32(body + 4); img.depth = body[8]; ctype = body[9]; interlace = body[12];
        } else if (!std::memcmp(typ, "IDAT", 4)) {
            idat.insert(idat.end(), body, body + n);
        } else if (!std::memcmp(typ, "IEND", 4)) {
            break;
        }
        pos += 12 + n;
    }
    if (img.w <= 0 || img.h <= 0 || interlace != 0) return false;
    img.channels = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 6 ? 4 : ctype == 4 ? 2 : 0;
    if (!img.channels || (img.depth != 8 && img.depth != 16)) return false;
    const size_t bpp = (size_t)img.channels * img.depth / 8, stride = (size_t)img.w * bpp;
    std::vector<uint8_t> raw((stride + 1) * img.h);
    uLongf outlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &outlen, idat.data(), (uLong)idat.size()) != Z_OK || outlen != raw.size()) return false;
    img.data.assign(stride * img.h, 0);
    for (int y = 0; y < img.h; ++y) {
        const uint8_t ft = raw[(stride + 1) * y];
        const uint8_t *in = &raw[(stride + 1) * y + 1];
        uint8_t *out = &img.data[stride * y];
        const uint8_t *up = y ? &img.data[stride * (y - 1)] : nullptr;
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? out[i - bpp] : 0, bb = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            int pred = 0;
            switch (ft) {
                case 0: pred = 0; break;
                case 1: pred = a; break;
                case 2: pred = bb; break;
                case 3: pred = (a + bb) >> 1; break;
                case 4: { const int p = a + bb - c, pa = std::abs(p - a), pb = std::abs(p - bb), pc = std::abs(p - c);
                          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c); break; }
                default: return false;
            }
            out[i] = (uint8_t)(in[i] + pred);
        }
    }
    return true;
}

}  // namespace sm_png

class KittiReader {
public:
    // gui/KittiReader.cpp:7-46
    KittiReader(std::string datasetDir, bool estimateDepth, bool useSemantic, int subLevel, bool groundTruth)
        : depth(nullptr), rgb(nullptr), rgbRight(nullptr), semantic(nullptr), currentFrameId(-1), time(0.0), savedFrameId(-1),
          datasetDir_(std::move(datasetDir)), estimate_depth(estimateDepth), use_semantic(useSemantic), ok_(true)
    {
        if (subLevel != 0) { std::printf("KittiReader: subLevel != 0 is not supported\n"); ok_ = false; }
        std::ifstream timesIn(datasetDir_ + "/times.txt");
        double t;
        while (timesIn >> t) times.push_back(t);
        depthDir = datasetDir_ + "/PSMNet";
        rgbDir = datasetDir_ + "/image_2";
        rgbRightDir = datasetDir_ + "/image_3";
        semanticDir = datasetDir_ + "/semantics";
        ok_ = loadCalibration() && ok_;
        if (groundTruth) ok_ = loadGroundTruth() && ok_;
    }
    bool good() const { return ok_; }

    // Read the lidar scan of every frame instead of its depth image.  false (and the reader no longer good) if the
    // lidar-to-camera transform cannot be read.
    bool setUseLidar(bool on)
    {
        use_lidar = on;
        if (!on) { velodyne = nullptr; numPoints = 0; return true; }
        depth = nullptr;                           // (a frame read before the switch no longer stands for the next ones)
        std::ifstream file(datasetDir_ + "/velo_to_cam.txt");
        int n = 0;
        for (int i = 0; i < 16; ++i) veloToCam[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        while (n < 12 && (file >> veloToCam[n])) ++n;
        if (n != 12) { std::printf("CANNOT read the lidar-to-camera transform from %s/velo_to_cam.txt\n", datasetDir_.c_str()); ok_ = false; }
        return n == 12;
    }

    bool getNext() { ++currentFrameId; return load(); }                       // gui/KittiReader.cpp:56-75
    bool getLast() { --currentFrameId; return load(); }                       // :77-96
    void saveState() { savedFrameId = currentFrameId; }
    void resumeState() { currentFrameId = savedFrameId; }
    void setState(int frameId) { currentFrameId = frameId; }                  // next getNext() yields frameId + 1 (build_map.cpp:292)

    int W() const { return width_; }
    int H() const { return height_; }
    int numPixels() const { return width_ * height_; }
    float fx() const { return fx_; }
    float fy() const { return fy_; }
    float cx() const { return cx_; }
    float cy() const { return cy_; }
    const std::vector<Eigen::Matrix4f> *getGroundTruth() const { return &groundTruth_; }
    size_t numFrames() const { return times.size(); }

    unsigned short *depth;
    unsigned char *rgb;
    unsigned char *rgbRight;                  // the right camera's image, R first; null unless estimateDepth
    unsigned char *semantic;
    const float *velodyne = nullptr;          // the frame's scan, numPoints x (x, y, z, reflectance); null unless setUseLidar(true)
    unsigned numPoints = 0;
    float veloToCam[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // lidar frame -> camera frame, row-major 4 x 4
    int currentFrameId;
    double time;
    int savedFrameId;
    Eigen::Matrix4f gtPose;

    // gui/KittiReader.cpp:239-280
    bool loadCalibration()
    {
        std::ifstream file(datasetDir_ + "/calibration.txt");
        std::string line;
        if (!file || !std::getline(file, line)) return false;
        if (std::sscanf(line.c_str(), "%f %f %f %f", &fx_, &fy_, &cx_, &cy_) != 4) return false;
        if (!std::getline(file, line)) return false;
        return std::sscanf(line.c_str(), "%d %d", &width_, &height_) == 2;
    }

    // gui/KittiReader.cpp:282-321: 3x4 row-major per line, times T20 (x offset -0.06 m)
    bool loadGroundTruth()
    {
        std::ifstream file(datasetDir_ + "/pose.txt");
        std::string line;
        groundTruth_.clear();
        while (std::getline(file, line)) {
            std::stringstream ss(line);
            float r[12];
            int n = 0;
            while (n < 12 && (ss >> r[n])) ++n;
            if (n != 12) continue;
            Eigen::Matrix4f g = Eigen::Matrix4f::Identity();
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) g(i, j) = r[4 * i + j];
            Eigen::Matrix4f out = g;                  // g * T20 with T20 = I + (-0.06) e_x e_w^T: only column 3 changes
            for (int i = 0; i < 3; ++i) out(i, 3) = g(i, 0) * -0.06f + g(i, 3);
            groundTruth_.push_back(out);
        }
        return groundTruth_.size() == times.size();
    }

private:
    bool load()
    {
        if (currentFrameId < 0 || (size_t)currentFrameId >= times.size()) return false;
        time = times[currentFrameId];
        if (!groundTruth_.empty()) gtPose = groundTruth_[currentFrameId];
        char name[32];
        std::snprintf(name, sizeof name, "/%06d.png", currentFrameId);
        const size_t P = (size_t)width_ * height_;
        sm_png::Image im;
        if (!loadRgb(rgbDir + name, im, rgbBuf_)) return false;
        rgb = rgbBuf_.data();                      // R first, as after the reference's BGR->RGB swap (gui/KittiReader.cpp:131-134)
        if (estimate_depth) {
            if (!loadRgb(rgbRightDir + name, im, rgbRightBuf_)) return false;
            rgbRight = rgbRightBuf_.data();
        } else if (!use_lidar) {
            if (!sm_png::read(depthDir + name, im) || im.w != width_ || im.h != height_ || im.channels != 1) {
                std::printf("CANNOT read depth image from %s%s", depthDir.c_str(), name);
                return false;
            }
            depthBuf_.resize(P);
            for (size_t p = 0; p < P; ++p)
                depthBuf_[p] = im.depth == 16 ? (unsigned short)((im.data[p * 2] << 8) | im.data[p * 2 + 1]) : im.data[p];
            depth = depthBuf_.data();
        }
        if (use_lidar) {
            char bin[32];
            std::snprintf(bin, sizeof bin, "/velodyne/%06d.bin", currentFrameId);
            std::ifstream f(datasetDir_ + bin, std::ios::binary);
            if (!f) { std::printf("CANNOT read the lidar scan from %s%s", datasetDir_.c_str(), bin); return false; }
            std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            if (raw.size() % 16) { std::printf("%s%s is not a whole number of points", datasetDir_.c_str(), bin); return false; }
            veloBuf_.assign(std::max<size_t>(raw.size() / 4, 4), 0.0f);      // (never empty: velodyne is not null for a frame)
            if (!raw.empty()) std::memcpy(veloBuf_.data(), raw.data(), raw.size());
            velodyne = veloBuf_.data();
            numPoints = (unsigned)(raw.size() / 16);
        }
        if (use_semantic) {
            if (!sm_png::read(semanticDir + name, im) || im.w != width_ || im.h != height_ || im.channels != 1 || im.depth != 8) {
                std::printf("CANNOT read semantic image from %s%s", semanticDir.c_str(), name);
                return false;
            }
            semBuf_.assign(im.data.begin(), im.data.end());
            semantic = semBuf_.data();
        }
        return true;
    }

    // an 8-bit colour (or grey) image of the calibration's size into buf, three bytes per pixel
    bool loadRgb(const std::string &path, sm_png::Image &im, std::vector<unsigned char> &buf)
    {
        const size_t P = (size_t)width_ * height_;
        if (!sm_png::read(path, im) || im.w != width_ || im.h != height_ || im.depth != 8) {
            std::printf("CANNOT read RGB image from %s", path.c_str());
            return false;
        }
        buf.resize(P * 3);
        for (size_t p = 0; p < P; ++p)
            for (int c = 0; c < 3; ++c) buf[p * 3 + c] = im.channels >= 3 ? im.data[p * im.channels + c] : im.data[p * im.channels];
        return true;
    }

    const std::string datasetDir_;
    std::string depthDir, rgbDir, rgbRightDir, semanticDir;
    int width_ = 0, height_ = 0;
    float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0;
    bool estimate_depth, use_semantic, ok_;
    bool use_lidar = false;
    std::vector<float> veloBuf_;
    std::vector<double> times;
    std::vector<Eigen::Matrix4f> groundTruth_;
    std::vector<unsigned char> rgbBuf_, rgbRightBuf_, semBuf_;
    std::vector<unsigned short> depthBuf_;
};
