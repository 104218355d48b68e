// SurfelMapping.h -- drop-in for src/SurfelMapping.h:18-128: same class, method names and
// argument order, backed by the HIP core through include/sm_c_api.h.
#pragma once
#include <cassert>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../../include/sm_c_api.h"
#include "Config.h"
#include "GPUTexture.h"
#include "GlobalModel.h"
#include "IndexMap.h"
#include "sm_compat.h"
#include "sm_png.h"
#include <sys/stat.h>

#include "FeedbackBuffer.h"

class Checker;          // debug aid of the reference (src/Utils/Checker.h); never constructed here

// One moving actor of a scene (sm_c_api.h "scenes"; DESIGN.md "4w. Scenes"): a map file whose records are in the actor's own frame,
// one actor->world pose per view (or sweep) and, if not empty, one byte per view: 0 = the actor is not in that view.
struct SceneActor {
    std::string file;
    std::vector<Eigen::Matrix4f> poses;
    std::vector<uint8_t> present;
};

class SurfelMapping {
public:
    // src/SurfelMapping.cpp:12-25: reads the Config singleton, which must have been initialised
    // with real values first (build_map.cpp:282-286).
    SurfelMapping() : checker(nullptr)
    {
        sm_config c;
        sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
        c.near_clip = Config::nearClip();
        c.far_clip = Config::farClip();
        c.fuse_thresh = Config::surfelFuseDistanceThreshFactor();
        c.max_sqrt_vertices = Config::maxSqrtVertices();
        const char *pre = std::getenv("SM_PREPROCESS");
        if (pre) c.preprocess = std::atoi(pre);
        // SM_FACADE_ASYNC=1: processFrame only enqueues (sm_process_frame_async: the images are staged inside the call, the copy of
        // frame f+1 overlaps frame f) and every getter waits -- the reference's processFrame ends in glFinish, so this is opt-in: a
        // device-side error is then reported by the next call that synchronises instead of by processFrame itself
        const char *as = std::getenv("SM_FACADE_ASYNC");
        async_ = as && as[0] == '1';
        ctx_ = sm_create(&c);
        if (!ctx_) throw std::runtime_error(std::string("SurfelMapping: ") + sm_last_error());
        globalModel.bind(ctx_);
        indexMap.bind(ctx_);
        rawFeedback.bind(ctx_);
        currPose = Eigen::Matrix4f::Identity();
        for (const char *n : {GPUTexture::RGB, GPUTexture::DEPTH_RAW, GPUTexture::DEPTH_FILTERED, GPUTexture::DEPTH_METRIC,
                              GPUTexture::SEMANTIC, "LAST"}) {
            textures[n] = new GPUTexture();
            textures[n]->texture->width = Config::W();
            textures[n]->texture->height = Config::H();
        }
    }
    virtual ~SurfelMapping()
    {
        for (auto &kv : textures) delete kv.second;
        sm_destroy(ctx_);
    }
    SurfelMapping(const SurfelMapping &) = delete;
    SurfelMapping &operator=(const SurfelMapping &) = delete;

    // src/SurfelMapping.h:31-34.  A null gtPose means "track" as the reference's header documents (the reference itself
    // dereferences it: src/SurfelMapping.cpp:130): the depth image is tracked against the model (sm_track_frame, constant-velocity
    // guess, default parameters) and the frame is then fused with the tracked pose.  A failed track (LOST, DEGENERATE,
    // NO_MODEL) prints one line and fuses with the guess.  With SM_FACADE_ASYNC=1 the track waits for the frames in flight; the
    // frame itself is enqueued as usual.  After setTrackColour(true) the track is sm_track_frame_rgb with the frame's own rgb
    // (default parameters): the colour term sees motion along flat ground and walls, where depth alone is DEGENERATE.
    void processFrame(const unsigned char *rgb, const unsigned short *depth = nullptr, const unsigned char *semantic = nullptr,
                      const Eigen::Matrix4f *gtPose = 0)
    {
        Eigen::Matrix4f tracked;
        if (!gtPose) {
            const unsigned short *d = depth ? depth : (textures[GPUTexture::DEPTH_RAW]->host_u16.empty()
                                                           ? nullptr : textures[GPUTexture::DEPTH_RAW]->host_u16.data());
            if (!d) { std::printf("processFrame: no gtPose and no depth image to track\n"); return; }
            const int rc = trackColour_ ? sm_track_frame_rgb(ctx_, rgb, d, nullptr, nullptr, nullptr, tracked.data(), &lastTrackInfo,
                                                             &lastTrackRgbInfo)
                                        : sm_track_frame(ctx_, d, nullptr, nullptr, tracked.data(), &lastTrackInfo);
            if (rc != SM_OK) {
                std::printf("processFrame: %s\n", sm_last_error());
                return;
            }
            static const char *const names[] = {"OK", "LOST", "DEGENERATE", "NO_MODEL"};
            if (lastTrackInfo.status != SM_TRACK_OK)
                std::printf("processFrame: tracking %s (%u inliers); using the guess\n",
                            lastTrackInfo.status >= 0 && lastTrackInfo.status <= 3 ? names[lastTrackInfo.status] : "failed",
                            lastTrackInfo.inliers);
            gtPose = &tracked;
        }
        currPose = *gtPose;
        // the reference uploads the three images into its RGB / DEPTH / SEMANTIC textures (src/SurfelMapping.cpp:122-128; a null
        // depth / semantic keeps the old one): kept here as host copies for getTexture()
        const size_t P = (size_t)Config::W() * Config::H();
        textures[GPUTexture::RGB]->host_u8.assign(rgb, rgb + P * 3);
        if (depth) textures[GPUTexture::DEPTH_RAW]->host_u16.assign(depth, depth + P);
        if (semantic) textures[GPUTexture::SEMANTIC]->host_u8.assign(semantic, semantic + P);
        int rc = async_ ? sm_process_frame_async(ctx_, rgb, depth, semantic, gtPose->data())
                        : sm_process_frame(ctx_, rgb, depth, semantic, gtPose->data());
        if (rc != SM_OK) std::printf("processFrame: %s\n", sm_last_error());
        historyPoses.push_back(currPose);
    }
    // src/SurfelMapping.cpp:496-532
    void cleanPoints(const unsigned short *depth, const unsigned char *semantic, const Eigen::Matrix4f *gtPose)
    {
        currPose = *gtPose;
        if (sm_clean_points(ctx_, depth, semantic, gtPose->data()) != SM_OK) std::printf("cleanPoints: %s\n", sm_last_error());
        beginCleanPoints = false;
    }
    void reset() { sm_reset(ctx_); historyPoses.clear(); }          // src/SurfelMapping.cpp:436-441
    void setBeginCleanPoints() { beginCleanPoints = true; }
    bool getBeginCleanPoints() { return beginCleanPoints; }
    const Eigen::Matrix4f &getCurrPose() { return currPose; }
    const std::vector<Eigen::Matrix4f> &getHistoryPoses() { return historyPoses; }
    // statistics of the last processFrame that tracked (gtPose null); zero before the first
    const sm_track_info &getLastTrackInfo() { return lastTrackInfo; }
    // track with the colour term as well (off by default); its statistics of the last processFrame that tracked with it
    void setTrackColour(bool on) { trackColour_ = on; }
    const sm_track_rgb_info &getLastTrackRgbInfo() { return lastTrackRgbInfo; }
    IndexMap &getIndexMap() { return indexMap; }
    GlobalModel &getGlobalModel() { return globalModel; }

    // src/SurfelMapping.cpp:450-456
    // The images live in the HIP context; the handle is filled when somebody asks for it (build_map.cpp:34-38 shows RGB,
    // DEPTH_METRIC and DEPTH_FILTERED every frame): the three float images are read back from the core (sm_download_depth),
    // the input images are the copies processFrame kept.  With SM_FACADE_GL the data goes into a real pangolin::GlTexture of the
    // reference's format (src/SurfelMapping.cpp:50-85); without GL the POD handle points at the host copy.
    pangolin::GlTexture *getTexture(const std::string &textureType)
    {
        auto it = textures.find(textureType);
        assert(it != textures.end() && "there is no such texture type");
        GPUTexture *t = it->second;
        const int W = Config::W(), H = Config::H();
        const int which = textureType == GPUTexture::DEPTH_METRIC ? SM_TEX_DEPTH_METRIC
                        : textureType == GPUTexture::DEPTH_FILTERED ? SM_TEX_DEPTH_FILTERED : textureType == "LAST" ? SM_TEX_LAST : -1;
        if (which >= 0) {
            t->host_f.resize((size_t)W * H);
            if (sm_download_depth(ctx_, which, t->host_f.data()) != SM_OK) std::printf("getTexture: %s\n", sm_last_error());
        }
#ifdef SM_FACADE_GL
        if (which >= 0) {
            if (!t->texture->tid) t->texture->Reinitialise(W, H, GL_R32F, false, 0, GL_RED, GL_FLOAT);
            t->texture->Upload(t->host_f.data(), GL_RED, GL_FLOAT);
        } else if (textureType == GPUTexture::RGB && !t->host_u8.empty()) {
            if (!t->texture->tid) t->texture->Reinitialise(W, H, GL_RGB32F, true, 0, GL_RGB, GL_UNSIGNED_BYTE);
            t->texture->Upload(t->host_u8.data(), GL_RGB, GL_UNSIGNED_BYTE);
        } else if (textureType == GPUTexture::DEPTH_RAW && !t->host_u16.empty()) {
            if (!t->texture->tid) t->texture->Reinitialise(W, H, GL_R16UI, false, 0, GL_RED_INTEGER, GL_UNSIGNED_SHORT);
            t->texture->Upload(t->host_u16.data(), GL_RED_INTEGER, GL_UNSIGNED_SHORT);
        } else if (textureType == GPUTexture::SEMANTIC && !t->host_u8.empty()) {
            if (!t->texture->tid) t->texture->Reinitialise(W, H, GL_R8UI, false, 0, GL_RED_INTEGER, GL_UNSIGNED_BYTE);
            t->texture->Upload(t->host_u8.data(), GL_RED_INTEGER, GL_UNSIGNED_BYTE);
        }
#elif defined(SM_COMPAT_POD_TEXTURE)
        t->texture->host = t->host_f.empty() ? nullptr : t->host_f.data();
        t->texture->host_u8 = t->host_u8.empty() ? nullptr : t->host_u8.data();
        t->texture->host_u16 = t->host_u16.empty() ? nullptr : t->host_u16.data();
#endif
        return t->texture;
    }
    // src/SurfelMapping.cpp:458-464: only "RAW" is ever created (src/SurfelMapping.cpp:88-90)
    FeedbackBuffer *getFeedbackBuffer(const std::string &feedbackType)
    {
        assert(feedbackType == FeedbackBuffer::RAW && "there is no such feedback buffer");
        (void)feedbackType;
        return &rawFeedback;
    }
    void computeFeedbackBuffers() { rawFeedback.refresh(); }                  // src/SurfelMapping.cpp:367-376

    // novel-view dump for SPADE (src/SurfelMapping.cpp:378-434): <path>/image/%06d.png (the bytes of the
    // reference's BGR cv::Mat, i.e. a correct-colour picture) and <path>/semantic/%06d.png (class + 1)
    void acquireImages(std::string path, const std::vector<Eigen::Matrix4f> &views, int w, int h, float fx, float fy, float cx,
                       float cy, int startId = 0)
    {
        if (fillHoles_ || writeDepth_ || blend_) { (void)acquireImagesEx(path, nullptr, true, views, w, h, fx, fy, cx, cy, startId); return; }
        if (path.empty() || path.back() != '/') path += "/";
        const std::string image_path = path + "image/", semantic_path = path + "semantic/";
        ::mkdir(image_path.c_str(), 0755);
        ::mkdir(semantic_path.c_str(), 0755);
        globalModel.setImageSize(w, h, fx, fy, cx, cy);
        std::vector<unsigned char> rgb((size_t)w * h * 3);
        for (const auto &v : views) {
            char name[32];
            std::snprintf(name, sizeof name, "%06d.png", startId);
            globalModel.renderImage(v);
            const std::vector<unsigned char> &bgr = globalModel.imageBGR();
            for (size_t p = 0; p < (size_t)w * h; ++p) { rgb[p * 3] = bgr[p * 3 + 2]; rgb[p * 3 + 1] = bgr[p * 3 + 1]; rgb[p * 3 + 2] = bgr[p * 3]; }
            const bool r1 = sm_png::write((image_path + name).c_str(), rgb.data(), w, h, 3);
            const bool r2 = sm_png::write((semantic_path + name).c_str(), globalModel.imageSemantic().data(), w, h, 1);
            if (!(r1 && r2)) std::printf("%s is NOT saved!\n", name);
            startId++;
        }
    }

    // The same dump of a map set: the map files `mapFiles` (downloadMap's format, the files of setAutoRetire) in that order,
    // then -- includeModel -- the live model.  One streamed call draws all views (sm_render_image_maps: every file is read once
    // per batch of views, nothing is loaded into the model); the pictures and their names are those of the overload above for a
    // model that is the concatenation of the set.
    bool acquireImages(std::string path, const std::vector<std::string> &mapFiles, const std::vector<Eigen::Matrix4f> &views, int w,
                       int h, float fx, float fy, float cx, float cy, int startId = 0, bool includeModel = true)
    {
        if (fillHoles_ || writeDepth_ || blend_) return acquireImagesEx(path, &mapFiles, includeModel, views, w, h, fx, fy, cx, cy, startId);
        if (path.empty() || path.back() != '/') path += "/";
        const std::string image_path = path + "image/", semantic_path = path + "semantic/";
        ::mkdir(image_path.c_str(), 0755);
        ::mkdir(semantic_path.c_str(), 0755);
        if (w <= 0 || h <= 0) return false;
        const size_t npix = (size_t)w * h;
        std::vector<float> v16(views.size() * 16);
        for (size_t i = 0; i < views.size(); ++i) std::memcpy(&v16[i * 16], views[i].data(), 64);
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        std::vector<unsigned char> bgr(views.size() * npix * 3), sem(views.size() * npix), rgb(npix * 3);
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_render_image_maps(ctx_, &src, v16.data(), (uint32_t)views.size(), w, h, fx, fy, cx, cy, bgr.data(), sem.data()) != SM_OK) {
            std::printf("acquireImages: %s\n", sm_last_error());
            return false;
        }
        bool ok = true;
        for (size_t i = 0; i < views.size(); ++i, ++startId) {
            char name[32];
            std::snprintf(name, sizeof name, "%06d.png", startId);
            const unsigned char *b = &bgr[i * npix * 3];
            for (size_t p = 0; p < npix; ++p) { rgb[p * 3] = b[p * 3 + 2]; rgb[p * 3 + 1] = b[p * 3 + 1]; rgb[p * 3 + 2] = b[p * 3]; }
            const bool r1 = sm_png::write((image_path + name).c_str(), rgb.data(), w, h, 3);
            const bool r2 = sm_png::write((semantic_path + name).c_str(), &sem[i * npix], w, h, 1);
            if (!(r1 && r2)) { std::printf("%s is NOT saved!\n", name); ok = false; }
        }
        return ok;
    }

    // What both acquireImages overloads add once switched on (sm_render_image_ex / sm_render_image_maps_ex; DESIGN.md "4n. Hole
    // filling").  setFillHoles: the views' holes are closed by the depth-aware push-pull completion before they are written;
    // levels, if not negative, replaces the default number of pyramid levels (3; 0..8).  setWriteDepth: each view's depth goes to
    // <path>/depth/%06d.png, a 16-bit grey PNG in millimetres (0 = empty or beyond 65.535 m), the format KittiReader reads from
    // PSMNet/.  With both off the overloads write what they always wrote.
    void setFillHoles(bool on, int levels = -1)
    {
        fillHoles_ = on;
        sm_default_fill_params(&fillParams_);
        if (levels >= 0) fillParams_.levels = levels;
    }
    void setWriteDepth(bool on) { writeDepth_ = on; }
    // setBlend (sm_render_image_blend / sm_render_image_maps_blend; DESIGN.md "4o. Blended views"): the colour of a pixel is the
    // weighted mean of the discs of its visible layer, not the nearest disc's; labels and depth stay the nearest disc's.  tol
    // (0..255, in 1/256 of the front depth) and falloff (0 box, 1 linear, 2 quadratic), if not negative, replace the defaults (13,
    // 2).  Off by default; a map set is then read twice per batch of views.
    void setBlend(bool on, int tol = -1, int falloff = -1)
    {
        blend_ = on;
        sm_default_blend_params(&blendParams_);
        if (tol >= 0) blendParams_.depth_tol_256 = tol;
        if (falloff >= 0) blendParams_.falloff = falloff;
    }

    // A drive's map made smaller (sm_simplify_maps; DESIGN.md "4p. Simplification"): the records of `mapFiles`, then (includeModel)
    // of the live model, that share a cell of voxelMm millimetres, a class and (splitNormals) a facing direction become one, and the
    // result is written as ONE map file to outPath, which may not be one of mapFiles.  The files and the model stay as they are.
    // Returns the records written, or -1 with the error printed (then outPath has not been touched).
    long simplifyMaps(const std::vector<std::string> &mapFiles, const std::string &outPath, int voxelMm = 50, bool splitNormals = true,
                      bool includeModel = false)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        sm_simplify_params p;
        sm_default_simplify_params(&p);
        p.voxel_mm = voxelMm;
        p.split_normals = splitNormals ? 1 : 0;
        sm_simplify_stats_t st;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_simplify_maps(ctx_, &src, &p, outPath.c_str()) != SM_OK || sm_simplify_stats(ctx_, &st) != SM_OK) {
            std::printf("simplifyMaps: %s\n", sm_last_error());
            return -1;
        }
        return (long)st.records_out;
    }

    // A map set sorted in space (sm_tile_maps; DESIGN.md "4s. Spatial tiling"): the records of `mapFiles`, then (withModel) of the
    // live model, verbatim, in Morton order over a world grid and cut at tile boundaries into the files "<prefix>_%06u.bin", none
    // of which may be one of mapFiles.  params null: the defaults (200 mm cells, tiles of 25.6 m, files of up to 2^20 records).
    // The files and the model stay as they are.  Returns the files written, in order; on an error it is printed, nothing has
    // been written and the list is empty (as it is for an empty set: sm_tile_stats tells the two apart).
    std::vector<std::string> tileMaps(const std::vector<std::string> &mapFiles, const std::string &prefix, bool withModel = false,
                                      const sm_tile_params *params = nullptr)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), withModel ? 1 : 0};
        sm_tile_params p;
        sm_default_tile_params(&p);
        if (params) p = *params;
        sm_tile_stats_t st;
        std::vector<std::string> written;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_tile_maps(ctx_, &src, &p, prefix.c_str()) != SM_OK || sm_tile_stats(ctx_, &st) != SM_OK) {
            std::printf("tileMaps: %s\n", sm_last_error());
            return written;
        }
        for (uint32_t i = 0; i < st.files_written; ++i) {
            char name[32];
            std::snprintf(name, sizeof name, "_%06u.bin", i);
            written.push_back(prefix + name);
        }
        return written;
    }

    // The map files `mapFiles` -- then, with withModel, the live model as one more -- written again as packed files of 20 bytes a
    // record, "<prefix>_%06u.smp" (sm_pack_maps; DESIGN.md "4aa. Packed map files"): every call that reads a map set takes them in
    // place of the plain ones.  Sources and model stay as they are.  params null: the defaults.  Returns the files written, in
    // order; none if the call was refused (the message is printed).
    std::vector<std::string> packMaps(const std::vector<std::string> &mapFiles, const std::string &prefix, bool withModel = false,
                                      const sm_pack_params *params = nullptr)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), withModel ? 1 : 0};
        sm_pack_params p;
        sm_default_pack_params(&p);
        if (params) p = *params;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_pack_maps(ctx_, &src, &p, prefix.c_str()) != SM_OK) {
            std::printf("packMaps: %s\n", sm_last_error());
            return {};
        }
        return numberedFiles(prefix, ".smp", mapFiles.size() + (withModel ? 1 : 0));
    }

    // ... and back: "<prefix>_%06u.bin", a packed file decoded, a plain one copied (sm_unpack_maps)
    std::vector<std::string> unpackMaps(const std::vector<std::string> &mapFiles, const std::string &prefix)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), 0};
        (void)sm_sync(ctx_);
        if (sm_unpack_maps(ctx_, &src, prefix.c_str()) != SM_OK) {
            std::printf("unpackMaps: %s\n", sm_last_error());
            return {};
        }
        return numberedFiles(prefix, ".bin", mapFiles.size());
    }

    // Which rigid transform takes the map set `sourceFiles` onto the set `targetFiles` (sm_register_maps; DESIGN.md "4q.
    // Registration"): two drives of one street, each in the world of its own first pose.  guess: source world -> target world, as
    // far as it is known (within about a cell of the coarsest level, 0.8 m by default); pose: the result, the guess unless the
    // status is SM_REGISTER_OK.  params (null: the defaults) should name a pivot inside the overlap.  Nothing is changed.
    // Returns the status (SM_REGISTER_*), or -1 with the error printed.
    int registerMaps(const std::vector<std::string> &sourceFiles, const std::vector<std::string> &targetFiles, const Eigen::Matrix4f &guess,
                     Eigen::Matrix4f &pose, const sm_register_params *params = nullptr, sm_register_info *info = nullptr)
    {
        std::vector<const char *> sp, tp;
        for (const std::string &f : sourceFiles) sp.push_back(f.c_str());
        for (const std::string &f : targetFiles) tp.push_back(f.c_str());
        const sm_map_source src{sp.data(), (uint32_t)sp.size(), 0}, tgt{tp.data(), (uint32_t)tp.size(), 0};
        sm_register_params p;
        sm_default_register_params(&p);
        if (params) p = *params;
        sm_register_info got;
        float out[16];
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_register_maps(ctx_, &src, &tgt, guess.data(), &p, out, &got) != SM_OK) {
            std::printf("registerMaps: %s\n", sm_last_error());
            return -1;
        }
        std::memcpy(pose.data(), out, 64);
        if (info) *info = got;
        return got.status;
    }
    // Where does the map set `sourceFiles` lie in the world of the set `targetFiles`, without a guess (sm_locate_maps; DESIGN.md
    // "4ab. Locating"): any yaw about the shared up axis, offsets of thousands of cells, a height.  params (null: the defaults)
    // should place the target window around the target's structure and source_origin near the source's middle.  pose: source
    // world -> target world, to be given to registerMaps as its guess; the identity unless the status is SM_LOCATE_OK or
    // SM_LOCATE_AMBIGUOUS.  Nothing is changed.  Returns the status (SM_LOCATE_*), or -1 with the error printed.
    int locateMaps(const std::vector<std::string> &sourceFiles, const std::vector<std::string> &targetFiles, Eigen::Matrix4f &pose,
                   const sm_locate_params *params = nullptr, sm_locate_info *info = nullptr)
    {
        std::vector<const char *> sp, tp;
        for (const std::string &f : sourceFiles) sp.push_back(f.c_str());
        for (const std::string &f : targetFiles) tp.push_back(f.c_str());
        const sm_map_source src{sp.data(), (uint32_t)sp.size(), 0}, tgt{tp.data(), (uint32_t)tp.size(), 0};
        sm_locate_params p;
        sm_default_locate_params(&p);
        if (params) p = *params;
        sm_locate_info got;
        float out[16];
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_locate_maps(ctx_, &src, &tgt, &p, out, &got) != SM_OK) {
            std::printf("locateMaps: %s\n", sm_last_error());
            return -1;
        }
        std::memcpy(pose.data(), out, 64);
        if (info) *info = got;
        return got.status;
    }
    // registerMaps, and on SM_REGISTER_OK the source files moved into the target's world (sm_warp_by_time with t0 = 0 and one
    // row, the pose): the two sets can then be viewed, swept or simplified as one.  A file none of whose records moves is left
    // alone; the live model stays.  Returns as registerMaps; -1 as well if the warp fails (the error is printed).
    int alignMaps(const std::vector<std::string> &sourceFiles, const std::vector<std::string> &targetFiles, const Eigen::Matrix4f &guess,
                  Eigen::Matrix4f &pose, const sm_register_params *params = nullptr, sm_register_info *info = nullptr)
    {
        const int status = registerMaps(sourceFiles, targetFiles, guess, pose, params, info);
        if (status != SM_REGISTER_OK || sourceFiles.empty()) return status;
        std::vector<const char *> sp;
        for (const std::string &f : sourceFiles) sp.push_back(f.c_str());
        const sm_map_source src{sp.data(), (uint32_t)sp.size(), 0};
        float corr[12];                                                  // row-major 3 x 4 of the column-major pose
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) corr[r * 4 + c] = pose.data()[c * 4 + r];
        if (sm_warp_by_time(ctx_, &src, 0, 1, corr) != SM_OK) {
            std::printf("alignMaps: %s\n", sm_last_error());
            return -1;
        }
        return status;
    }

    // Which records of the map set `queryFiles` does the set `referenceFiles` hold the surface of (sm_compare_maps; DESIGN.md "4r.
    // Change detection")?  pose: query world -> reference world (registerMaps measures it).  outPath (may be empty): the query
    // records whose label is in params->write_mask -- by default the CHANGED ones: the reference mapped the place, not this
    // surface -- as one map file, verbatim and in set order.  params: null = the defaults.  Nothing else is changed.  Returns the
    // CHANGED records, or -1 with the error printed.
    long compareMaps(const std::vector<std::string> &queryFiles, const std::vector<std::string> &referenceFiles, const Eigen::Matrix4f &pose,
                     const std::string &outPath, const sm_compare_params *params = nullptr, sm_compare_info *info = nullptr)
    {
        std::vector<const char *> qp, rp;
        for (const std::string &f : queryFiles) qp.push_back(f.c_str());
        for (const std::string &f : referenceFiles) rp.push_back(f.c_str());
        const sm_map_source qry{qp.data(), (uint32_t)qp.size(), 0}, ref{rp.data(), (uint32_t)rp.size(), 0};
        sm_compare_params p;
        sm_default_compare_params(&p);
        if (params) p = *params;
        sm_compare_info got;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_compare_maps(ctx_, &qry, &ref, pose.data(), &p, nullptr, outPath.empty() ? nullptr : outPath.c_str(), &got) != SM_OK) {
            std::printf("compareMaps: %s\n", sm_last_error());
            return -1;
        }
        if (info) *info = got;
        return (long)got.counts[SM_COMPARE_CHANGED];
    }
    // What appeared and what vanished between the map sets a (before) and b (after): compareMaps of b against a, its CHANGED
    // records -- b's surfaces that a does not hold -- to outAppeared, and of a against b to outVanished.  poseAToB: a's world to
    // b's; the first call gets its inverse, taken in double and rounded to float.  Returns false with the error printed.
    bool diffMaps(const std::vector<std::string> &aFiles, const std::vector<std::string> &bFiles, const Eigen::Matrix4f &poseAToB,
                  const std::string &outAppeared, const std::string &outVanished, const sm_compare_params *params = nullptr,
                  sm_compare_info *appeared = nullptr, sm_compare_info *vanished = nullptr)
    {
        // the inverse of [A | t], last row (0, 0, 0, 1): [A^-1 | -A^-1 t], A^-1 by cofactors
        const float *f = poseAToB.data();
        double a[3][3], c[3][3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) a[r][k] = (double)f[k * 4 + r];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k)
                c[r][k] = a[(r + 1) % 3][(k + 1) % 3] * a[(r + 2) % 3][(k + 2) % 3] - a[(r + 1) % 3][(k + 2) % 3] * a[(r + 2) % 3][(k + 1) % 3];
        const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
        Eigen::Matrix4f inv = Eigen::Matrix4f::Identity();
        for (int r = 0; r < 3; ++r) {
            double t = 0.0;
            for (int k = 0; k < 3; ++k) {
                inv.data()[k * 4 + r] = (float)(c[k][r] / det);
                t -= (c[k][r] / det) * (double)f[12 + k];
            }
            inv.data()[12 + r] = (float)t;
        }
        return compareMaps(bFiles, aFiles, inv, outAppeared, params, appeared) >= 0 &&
               compareMaps(aFiles, bFiles, poseAToB, outVanished, params, vanished) >= 0;
    }

    // The records of the map set `mapFiles`, then (withModel) of the live model, grouped into objects (sm_segment_maps; DESIGN.md
    // "4t. Segmentation"): connected components of occupied voxel cells, numbered in set order of first appearance.  components:
    // a row per numbered component (the set is segmented twice: once to count them, once to fill the vectors);
    // labels (may be null): per record of the set its component's number, or SM_SEGMENT_SMALL / SKIPPED / LOOSE.  outPath (may be
    // empty): the records whose label kind is in params->write_mask -- by default those of numbered components, so that
    // min_records N drops every speck of fewer than N records -- as one map file, verbatim and in set order.  params: null = the
    // defaults.  Nothing else is changed.  Returns the numbered components, or -1 with the error printed.
    long segmentMaps(const std::vector<std::string> &mapFiles, const std::string &outPath, const sm_segment_params *params,
                     std::vector<sm_segment_component> &components, std::vector<uint32_t> *labels = nullptr, bool withModel = false,
                     sm_segment_info *info = nullptr)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), withModel ? 1 : 0};
        sm_segment_params p;
        sm_default_segment_params(&p);
        if (params) p = *params;
        const char *out = outPath.empty() ? nullptr : outPath.c_str();
        sm_segment_info got;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        // the first call counts (it writes no row, no label and no file), the second fills vectors of the right size
        if (sm_segment_maps(ctx_, &src, &p, nullptr, nullptr, 0, nullptr, &got) != SM_OK) {
            std::printf("segmentMaps: %s\n", sm_last_error());
            return -1;
        }
        components.assign(got.components, sm_segment_component{});
        if (labels) labels->assign((size_t)got.records, 0u);
        if (sm_segment_maps(ctx_, &src, &p, labels && got.records ? labels->data() : nullptr, got.components ? components.data() : nullptr, got.components,
                            out, &got) != SM_OK) {
            std::printf("segmentMaps: %s\n", sm_last_error());
            return -1;
        }
        if (info) *info = got;
        return (long)got.components;
    }

    // The surface the records of the map set `mapFiles`, then (withModel) of the live model, lie on, as a triangle mesh
    // (sm_mesh_maps; DESIGN.md "4u. Meshing"): one plane per occupied voxel cell, a signed field at the grid's lattice points,
    // marching tetrahedra; faces counter-clockwise seen from outside, the way the surfel normals point.  plyPath (may be empty):
    // the mesh as a binary little-endian PLY with per-vertex normal, colour and class.  params: null = the defaults (100 mm cells,
    // reach 2).  vertices / faces (may be null): filled with the whole mesh, for which the set is read twice: once to count, once
    // to fill.  Nothing else is changed.  Returns the faces, or -1 with the error printed.
    long meshMaps(const std::vector<std::string> &mapFiles, const sm_mesh_params *params, const std::string &plyPath,
                  std::vector<sm_mesh_vertex> *vertices = nullptr, std::vector<uint32_t> *faces = nullptr, bool withModel = false,
                  sm_mesh_info *info = nullptr)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), withModel ? 1 : 0};
        sm_mesh_params p;
        sm_default_mesh_params(&p);
        if (params) p = *params;
        const char *out = plyPath.empty() ? nullptr : plyPath.c_str();
        sm_mesh_info got{};
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if ((vertices || faces) && sm_mesh_maps(ctx_, &src, &p, nullptr, 0, nullptr, 0, nullptr, &got) != SM_OK) {
            std::printf("meshMaps: %s\n", sm_last_error());
            return -1;
        }
        if (vertices) vertices->assign(got.vertices, sm_mesh_vertex{});
        if (faces) faces->assign((size_t)got.faces * 3, 0u);
        const uint32_t vcap = vertices ? got.vertices : 0u, fcap = faces ? got.faces : 0u;
        if (sm_mesh_maps(ctx_, &src, &p, vcap ? vertices->data() : nullptr, vcap, fcap ? faces->data() : nullptr, fcap, out, &got) != SM_OK) {
            std::printf("meshMaps: %s\n", sm_last_error());
            return -1;
        }
        if (info) *info = got;
        return (long)got.faces;
    }

    // The records of the map set `mapFiles`, then (withModel) of the live model, as a planner's ground map (sm_ground_maps; DESIGN.md
    // "4v. Ground map"): a bird's-eye raster over the window params states -- per cell the ground height, the state FREE / OBSTACLE /
    // STEP / UNKNOWN, the ground's colour and class, the tallest obstacle and the exact squared distance to the nearest blocking
    // cell.  params: null = the defaults.  Nothing else is changed.  The result's `ok` is false, with the error printed, if the call failed.
    GroundMap groundMaps(const std::vector<std::string> &mapFiles, const sm_ground_params *params = nullptr, bool withModel = false)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), withModel ? 1 : 0};
        sm_ground_params p;
        sm_default_ground_params(&p);
        if (params) p = *params;
        return GroundMap::of(ctx_, src, p, "groundMaps");
    }

    // Routes over a ground map (sm_route_ground; DESIGN.md "4ac. Routes"): for each goal set of `goals` the cost-to-go field over the
    // ground map's window -- the least cost of an 8-connected path that keeps body_cells away from blocking cells and pays more near
    // them -- and the direction of the first step; for each start (field, u, v) the cells of its path.  params: null = the defaults;
    // nu and nv are the ground map's.  Nothing is changed.  The result's `ok` is false, with the error printed, if the call failed.
    RouteField routeGround(const GroundMap &ground, const std::vector<std::vector<RouteGoal>> &goals, const std::vector<RouteStart> &starts = {},
                           const sm_route_params *params = nullptr)
    {
        sm_route_params p;
        sm_default_route_params(&p);
        if (params) p = *params;
        return RouteField::of(ctx_, ground, goals, starts, p, "routeGround");
    }

    // Routes a car can follow over a ground map (sm_route_car; DESIGN.md "4ad. Routes for a car"): for each goal set of `goals` the
    // cost-to-go over (cell, heading) -- the least weight of a sequence of steps ahead, turns of 45 degrees that take turn_cells
    // cells before and after, and steps back where reverse_weight allows them -- and the first move; for each start (field, u, v, h)
    // the words of its path, every unit cell passed.  params: null = the defaults; nu and nv are the ground map's.  Nothing is
    // changed.  The result's `ok` is false, with the error printed, if the call failed.
    CarField routeCar(const GroundMap &ground, const std::vector<std::vector<CarGoal>> &goals, const std::vector<CarStart> &starts = {},
                      const sm_route_car_params *params = nullptr)
    {
        sm_route_car_params p;
        sm_default_route_car_params(&p);
        if (params) p = *params;
        return CarField::of(ctx_, ground, goals, starts, p, "routeCar");
    }

    // The second sensor's dump: what a lidar `sensor` (sm_lidar_sensor; sm_default_lidar_sensor) at each of `poses` (sensor->world,
    // the camera's axes) measures in the live model, written as <path>/velodyne/%06d.bin next to acquireImages' folders, in KITTI's
    // velodyne layout: per return four floats, (z, -x, -y) of t*d in the sensor frame -- x forward, y left, z up -- and the
    // reflectance, the luminance ((0.299 r + 0.587 g) + 0.114 b) / 255 of the surfel's colour.  Beams without a return are left out.
    bool acquireSweeps(std::string path, const std::vector<Eigen::Matrix4f> &poses, const sm_lidar_sensor &sensor, int startId = 0)
    {
        return acquireSweeps(path, {}, poses, sensor, startId, true);
    }
    // The same dump of a map set (sm_lidar_sweep_maps): the map files in that order, then -- includeModel -- the live model, streamed.
    bool acquireSweeps(std::string path, const std::vector<std::string> &mapFiles, const std::vector<Eigen::Matrix4f> &poses,
                       const sm_lidar_sensor &sensor, int startId = 0, bool includeModel = true)
    {
        return acquireSweepsOf(path, mapFiles, poses, sensor, startId, includeModel, nullptr);
    }

    // What a list of rays hits in a map set (sm_cast_rays_maps; DESIGN.md "4x. Ray casts"): the map files in that order, then --
    // includeModel -- the live model, read once whatever the number of rays.  GlobalModel::castRays is the live model alone.
    bool castRays(const std::vector<std::string> &mapFiles, const std::vector<sm_ray> &rays, GlobalModel::RayReturns &out, bool includeModel = true,
                  const sm_rays_params *params = nullptr)
    {
        return GlobalModel::castRaysOf(ctx_, mapFiles, includeModel, rays, out, params, "castRays");
    }

    // The nearest disc of a map set to each of a list of points, within the point's reach (sm_query_points_maps; DESIGN.md "4y.
    // Point queries"): the map files in that order, then -- includeModel -- the live model, read once whatever the number of points.
    // GlobalModel::queryPoints is the live model alone.
    bool queryPoints(const std::vector<std::string> &mapFiles, const std::vector<sm_point> &points, GlobalModel::PointReturns &out,
                     bool includeModel = true, const sm_points_params *params = nullptr)
    {
        return GlobalModel::queryPointsOf(ctx_, mapFiles, includeModel, points, out, params, "queryPoints");
    }

    // Scenes (sm_render_image_scene / sm_lidar_sweep_scene; DESIGN.md "4w. Scenes"): the map set with moving actors in it.  Every
    // actor's file is read once and drawn under its pose of each view where it is present; no file is copied or rewritten.
    // acquireSceneImages writes what acquireImages writes and honours setFillHoles / setWriteDepth; the blended view draws no
    // scenes, so with setBlend on it refuses.  acquireSceneSweeps writes velodyne/%06d.bin as acquireSweeps does.
    bool acquireSceneImages(std::string path, const std::vector<std::string> &mapFiles, bool includeModel, const std::vector<SceneActor> &actors,
                            const std::vector<Eigen::Matrix4f> &views, int w, int h, float fx, float fy, float cx, float cy, int startId = 0)
    {
        if (blend_) {
            std::printf("acquireSceneImages: blended views draw no scenes (setBlend is on)\n");
            return false;
        }
        return acquireImagesEx(path, &mapFiles, includeModel, views, w, h, fx, fy, cx, cy, startId, &actors);
    }
    bool acquireSceneSweeps(std::string path, const std::vector<std::string> &mapFiles, bool includeModel, const std::vector<SceneActor> &actors,
                            const std::vector<Eigen::Matrix4f> &poses, const sm_lidar_sensor &sensor, int startId = 0)
    {
        return acquireSweepsOf(path, mapFiles, poses, sensor, startId, includeModel, &actors);
    }

    // extras of the HIP core
    sm_ctx *context() { return ctx_; }
    // The replacement of the operator's save / reset buttons (build_map.cpp:235-263) for a headless run: after every `every`-th
    // frame the surfels that fusion can no longer reach (older than Config's time delta, farther than 1.5 farClip from the
    // camera) leave the model for the map file "<prefix>_%06u.bin", which uploadMap reads (sm_set_auto_retire).  every <= 0: off.
    // minAge / minDistance, if not negative, replace those two defaults.
    bool setAutoRetire(int every, const std::string &prefix, int minAge = -1, float minDistance = -1.0f)
    {
        sm_config c;
        sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
        c.far_clip = Config::farClip();
        sm_retire_params p;
        sm_default_retire_params(&c, &p);
        if (minAge >= 0) p.min_age = minAge;
        if (minDistance >= 0.0f) p.min_distance = minDistance;
        if (sm_set_auto_retire(ctx_, &p, every, prefix.c_str()) == SM_OK) return true;
        std::printf("setAutoRetire: %s\n", sm_last_error());
        return false;
    }
    // map files written so far and the surfels in them
    std::pair<unsigned, unsigned long long> autoRetireStats()
    {
        uint32_t f = 0; uint64_t n = 0;
        sm_auto_retire_stats(ctx_, &f, &n);
        return {f, (unsigned long long)n};
    }
    // Close a loop (sm_close_loop, default parameters): `depth` is tracked against the surfels that are older than time_delta
    // frames -- what a recall has brought back -- starting from `pose`, where the caller believes the camera is; if the two
    // disagree by a plausible amount, the model, the stored poses and the map files `mapFiles` are pulled straight along a ramp
    // over the surfels' times.  Returns the corrected pose, or `pose` itself when no loop was closed; getLastLoopInfo().status
    // (SM_LOOP_*) says which, and its D is the correction that was measured.
    Eigen::Matrix4f closeLoop(const unsigned short *depth, const Eigen::Matrix4f &pose, const std::vector<std::string> &mapFiles = {})
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), 1};
        Eigen::Matrix4f out = pose;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        const int rc = loopSearch_ ? sm_close_loop_search(ctx_, nullptr, depth, pose.data(), &src, nullptr, nullptr, loopParams(), &loopSearchParams_,
                                                          out.data(), &lastLoopInfo)
                                   : sm_close_loop(ctx_, depth, pose.data(), &src, nullptr, nullptr, out.data(), &lastLoopInfo);
        if (rc != SM_OK) {
            std::printf("closeLoop: %s\n", sm_last_error());
            return pose;
        }
        return out;
    }
    // The same with the frame's rgb image: after setTrackColour(true) the loop is measured with the colour term as well
    // (sm_close_loop_rgb, default parameters), which closes on a street of flat ground and flat walls, where depth alone cannot;
    // without it this is the overload above.
    Eigen::Matrix4f closeLoop(const unsigned char *rgb, const unsigned short *depth, const Eigen::Matrix4f &pose,
                              const std::vector<std::string> &mapFiles = {})
    {
        if (!trackColour_) return closeLoop(depth, pose, mapFiles);
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), 1};
        Eigen::Matrix4f out = pose;
        (void)sm_sync(ctx_);
        const int rc = loopSearch_ ? sm_close_loop_search(ctx_, rgb, depth, pose.data(), &src, nullptr, nullptr, loopParams(), &loopSearchParams_,
                                                          out.data(), &lastLoopInfo)
                                   : sm_close_loop_rgb(ctx_, rgb, depth, pose.data(), &src, nullptr, nullptr, nullptr, out.data(), &lastLoopInfo);
        if (rc != SM_OK) {
            std::printf("closeLoop: %s\n", sm_last_error());
            return pose;
        }
        return out;
    }
    const sm_loop_info &getLastLoopInfo() { return lastLoopInfo; }
    // Measure loops by a pose search (sm_close_loop_search, sm_set_auto_loop_search): instead of one track from the believed pose,
    // which converges from a few decimetres, a grid of poses +-transHalf metres sideways and forward and +-yawHalfDeg degrees about
    // the vertical around it is scored against the old surfels, refined, and the best are tracked from -- metres of drift close.
    // Honoured by both closeLoop overloads and by setAutoLoop, before or after this call.  Negative arguments keep the defaults
    // (2 m, 3 degrees); maxTrans, if not negative, replaces the 2 m above which a measured loop is rejected (the default box
    // reaches 2.8 m).  on = false: off, and the bound is the default again.
    bool setLoopSearch(bool on, float transHalf = -1.0f, float yawHalfDeg = -1.0f, float maxTrans = -1.0f)
    {
        sm_search_params sp;
        sm_default_search_params(&sp);
        if (transHalf >= 0.0f) sp.trans_half[0] = sp.trans_half[2] = transHalf;
        if (yawHalfDeg >= 0.0f) sp.rot_half_deg[1] = yawHalfDeg;
        if (sm_set_auto_loop_search(ctx_, on ? &sp : nullptr) != SM_OK) {
            std::printf("setLoopSearch: %s\n", sm_last_error());
            return false;
        }
        loopSearch_ = on;
        loopSearchParams_ = sp;
        loopMaxTrans_ = on ? maxTrans : -1.0f;
        return true;
    }
    // Close loops unasked (sm_set_auto_loop): while on, every processFrame that tracks (null gtPose) tracks in the young map, counts
    // the surfels older than time_delta frames the tracked pose sees and, with at least minOld of them, makes one closeLoop attempt
    // before the frame is fused -- with the colour term after setTrackColour(true).  The map files `mapFiles` and those of
    // setAutoRetire move with the model.  every / rest / minOld, if not negative, replace the defaults (1, 10, 1000).  on = false: off.
    bool setAutoLoop(bool on, const std::vector<std::string> &mapFiles = {}, int every = -1, int rest = -1, long minOld = -1)
    {
        int rc;
        if (!on) rc = sm_set_auto_loop(ctx_, nullptr, nullptr);
        else {
            sm_config c;
            sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
            sm_auto_loop_params p;
            sm_default_auto_loop_params(&c, &p);
            if (every >= 0) p.every = every;
            if (rest >= 0) p.rest = rest;
            if (minOld >= 0) p.min_old = (uint32_t)minOld;
            if (loopSearch_ && loopMaxTrans_ >= 0.0f) p.loop.max_trans = loopMaxTrans_;
            std::vector<const char *> paths;
            for (const std::string &f : mapFiles) paths.push_back(f.c_str());
            const sm_map_source src{paths.data(), (uint32_t)paths.size(), 1};
            rc = sm_set_auto_loop(ctx_, &p, &src);
        }
        if (rc == SM_OK) return true;
        std::printf("setAutoLoop: %s\n", sm_last_error());
        return false;
    }
    // censuses, attempts and their outcomes so far; `last` is the last attempt's sm_loop_info
    sm_auto_loop_stats_t autoLoopStats()
    {
        sm_auto_loop_stats_t st{};
        sm_auto_loop_stats(ctx_, &st);
        return st;
    }

    // Recognise revisited places without a pose prior (sm_set_ferns, sm_set_auto_place): while on, every processFrame that tracks
    // (null gtPose) encodes the frame as a fern code, matches it against the keyframes, and where an old keyframe far from the
    // tracked pose matches, searches and tracks at that keyframe's pose and closes the loop before the frame is fused; frames unlike
    // every keyframe become keyframes.  Turning it on makes a fresh, empty database (loadKeyframes fills it from a file).  nFerns /
    // matchBelow, if not negative, replace the defaults (512, 0.3).  on = false: off, and the database is freed.
    bool setAutoPlace(bool on, int nFerns = -1, float matchBelow = -1.0f)
    {
        int rc;
        if (!on) {
            rc = sm_set_auto_place(ctx_, nullptr);
            if (rc == SM_OK) rc = sm_set_ferns(ctx_, nullptr);
        } else {
            sm_config c;
            sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
            c.near_clip = Config::nearClip();              // (the context's own clips: the ferns' depth thresholds span them)
            c.far_clip = Config::farClip();
            sm_fern_params fp;
            sm_default_fern_params(&c, &fp);
            if (nFerns >= 0) fp.n_ferns = nFerns;
            sm_auto_place_params ap;
            sm_default_auto_place_params(&c, &ap);
            if (matchBelow >= 0.0f) ap.match_below = matchBelow;
            rc = sm_set_ferns(ctx_, &fp);
            if (rc == SM_OK) rc = sm_set_auto_place(ctx_, &ap);
        }
        if (rc == SM_OK) return true;
        std::printf("setAutoPlace: %s\n", sm_last_error());
        return false;
    }
    // the keyframes (codes, poses, times) as one file, and back: of a context whose setAutoPlace used the same number of ferns
    bool saveKeyframes(const std::string &path)
    {
        if (sm_fern_save(ctx_, path.c_str()) == SM_OK) return true;
        std::printf("saveKeyframes: %s\n", sm_last_error());
        return false;
    }
    bool loadKeyframes(const std::string &path)
    {
        if (sm_fern_load(ctx_, path.c_str()) == SM_OK) return true;
        std::printf("loadKeyframes: %s\n", sm_last_error());
        return false;
    }
    // frames encoded, keyframes added, matches, attempts and their outcomes so far; `last` is the last attempt's sm_loop_info
    sm_auto_place_stats_t autoPlaceStats()
    {
        sm_auto_place_stats_t st{};
        sm_auto_place_stats(ctx_, &st);
        return st;
    }

    // Estimate depth from a rectified stereo pair (sm_set_stereo): what the reference's estimateDepth flag leaves undone.  baseline
    // (metres) / maxDisp, if not negative, replace the defaults (0.54, 128).  on = false: off, and the matcher's buffers are freed.
    bool setStereo(bool on, float baseline = -1.0f, int maxDisp = -1)
    {
        int rc;
        if (!on) {
            rc = sm_set_stereo(ctx_, nullptr);
        } else {
            sm_config c;
            sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
            sm_stereo_params sp;
            sm_default_stereo_params(&c, &sp);
            if (baseline >= 0.0f) sp.baseline = baseline;
            if (maxDisp >= 0) sp.max_disp = maxDisp;
            rc = sm_set_stereo(ctx_, &sp);
        }
        if (rc == SM_OK) return true;
        std::printf("setStereo: %s\n", sm_last_error());
        return false;
    }
    // processFrame with the depth image estimated from the pair (sm_stereo_depth; setStereo(true) first): a null gtPose tracks
    // with the estimated depth exactly as it would with a file's.  false (and nothing processed) if the estimate fails.
    bool processFrameStereo(const unsigned char *rgbLeft, const unsigned char *rgbRight, const unsigned char *semantic = nullptr,
                            const Eigen::Matrix4f *gtPose = nullptr)
    {
        stereoDepth_.resize((size_t)Config::W() * Config::H());
        if (sm_stereo_depth(ctx_, rgbLeft, rgbRight, stereoDepth_.data(), nullptr) != SM_OK) {
            std::printf("processFrameStereo: %s\n", sm_last_error());
            return false;
        }
        processFrame(rgbLeft, stereoDepth_.data(), semantic, gtPose);
        return true;
    }
    // the depth image (millimetres, 0 = invalid) of the last processFrameStereo; empty before the first
    const std::vector<unsigned short> &getLastStereoDepth() { return stereoDepth_; }

    // Make the depth image of a frame from its lidar scan (sm_set_lidar_depth).  params null: the defaults
    // (sm_default_lidar_depth_params).  on = false: off, and the stage's planes are freed.
    bool setLidarDepth(bool on, const sm_lidar_depth_params *params = nullptr)
    {
        int rc;
        if (!on) {
            rc = sm_set_lidar_depth(ctx_, nullptr);
        } else {
            sm_config c;
            sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
            sm_lidar_depth_params lp;
            sm_default_lidar_depth_params(&c, &lp);
            rc = sm_set_lidar_depth(ctx_, params ? params : &lp);
        }
        if (rc == SM_OK) return true;
        std::printf("setLidarDepth: %s\n", sm_last_error());
        return false;
    }
    // processFrame with the depth image made from the scan (sm_lidar_depth; setLidarDepth(true) first): points4 holds n points
    // (x, y, z, reflectance) in the lidar's frame, veloToCam16 the row-major 4 x 4 from there to the camera's (KittiReader's
    // velodyne, numPoints and veloToCam).  false (and nothing processed) if the stage fails.
    bool processFrameLidar(const unsigned char *rgb, const float *points4, unsigned n, const float *veloToCam16,
                           const unsigned char *semantic = nullptr, const Eigen::Matrix4f *gtPose = nullptr)
    {
        lidarDepth_.resize((size_t)Config::W() * Config::H());
        if (sm_lidar_depth(ctx_, points4, n, veloToCam16, lidarDepth_.data(), nullptr, nullptr) != SM_OK) {
            std::printf("processFrameLidar: %s\n", sm_last_error());
            return false;
        }
        processFrame(rgb, lidarDepth_.data(), semantic, gtPose);
        return true;
    }
    // the depth image (millimetres, 0 = empty) of the last processFrameLidar; empty before the first
    const std::vector<unsigned short> &getLastLidarDepth() { return lidarDepth_; }

    // With setAutoRetire on: after every retirement, the records of its map files within `radius` metres of that frame's camera
    // come back into the model and leave the files, so that a camera that returns finds what it left (sm_set_auto_recall;
    // 0 < radius <= the retirement's minDistance).  radius <= 0: off.
    bool setAutoRecall(float radius = -1.0f)
    {
        const sm_recall_params p = {radius};
        if (sm_set_auto_recall(ctx_, radius > 0.0f ? &p : nullptr) == SM_OK) return true;
        std::printf("setAutoRecall: %s\n", sm_last_error());
        return false;
    }
    // recalls the policy has made and the surfels they brought back
    std::pair<unsigned, unsigned long long> autoRecallStats()
    {
        uint32_t r = 0; uint64_t n = 0;
        sm_auto_recall_stats(ctx_, &r, &n);
        return {r, (unsigned long long)n};
    }
    // (sm_sync first: with SM_FACADE_ASYNC frames may still be in flight, and sm_get_counts returns the counters of the last wait)
    sm_counts counts() { sm_counts c{}; (void)sm_sync(ctx_); sm_get_counts(ctx_, &c); return c; }

    Checker *checker;

private:
    // "<prefix>_%06u<ext>", 0 .. n - 1: the names sm_pack_maps and sm_unpack_maps give their outputs
    static std::vector<std::string> numberedFiles(const std::string &prefix, const char *ext, size_t n)
    {
        std::vector<std::string> files;
        for (size_t i = 0; i < n; ++i) {
            char name[32];
            std::snprintf(name, sizeof name, "_%06u", (unsigned)i);
            files.push_back(prefix + name + ext);
        }
        return files;
    }
    sm_ctx *ctx_ = nullptr;
    Eigen::Matrix4f currPose;
    IndexMap indexMap;
    GlobalModel globalModel;
    FeedbackBuffer rawFeedback;
    std::map<std::string, GPUTexture *> textures;
    std::vector<Eigen::Matrix4f> historyPoses;
    sm_track_info lastTrackInfo{};
    sm_track_rgb_info lastTrackRgbInfo{};
    bool trackColour_ = false;
    sm_loop_info lastLoopInfo{};
    bool loopSearch_ = false;
    sm_search_params loopSearchParams_{};
    float loopMaxTrans_ = -1.0f;
    sm_loop_params loopParams_{};
    // the loop bounds of a searched closeLoop: the defaults, with setLoopSearch's maxTrans (null: the defaults as they are)
    const sm_loop_params *loopParams()
    {
        if (loopMaxTrans_ < 0.0f) return nullptr;
        sm_config c;
        sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
        sm_default_loop_params(&c, &loopParams_);
        loopParams_.max_trans = loopMaxTrans_;
        return &loopParams_;
    }
    bool fillHoles_ = false, writeDepth_ = false, blend_ = false;
    sm_fill_params fillParams_{};
    sm_blend_params blendParams_{};
    // acquireImages with setFillHoles, setWriteDepth or setBlend on: mapFiles null = the live model, one sm_render_image_blend per
    // view; otherwise the map set, one sm_render_image_maps_blend for all views (with blending off these are the _ex calls).  The live model's image (globalModel.imageBGR() /
    // imageSemantic(), its size) is left as the plain overload leaves it: the last view, filled if filling is on.  One difference
    // remains: a view that cannot be rendered ends the call with the error printed and no file written (false; the void overload has
    // no way to return it), where the plain live-model overload prints the error and writes the planes it has.
    // actors (with mapFiles) non-null: the scene call, sm_render_image_scene, which draws no blended views.
    bool acquireImagesEx(std::string path, const std::vector<std::string> *mapFiles, bool includeModel, const std::vector<Eigen::Matrix4f> &views,
                         int w, int h, float fx, float fy, float cx, float cy, int startId, const std::vector<SceneActor> *actors = nullptr)
    {
        if (path.empty() || path.back() != '/') path += "/";
        const std::string image_path = path + "image/", semantic_path = path + "semantic/", depth_path = path + "depth/";
        ::mkdir(image_path.c_str(), 0755);
        ::mkdir(semantic_path.c_str(), 0755);
        if (writeDepth_) ::mkdir(depth_path.c_str(), 0755);
        if (w <= 0 || h <= 0) return false;
        const size_t npix = (size_t)w * h, V = views.size();
        const sm_fill_params *fill = fillHoles_ ? &fillParams_ : nullptr;
        const sm_blend_params *blend = blend_ ? &blendParams_ : nullptr;
        std::vector<unsigned char> bgr(V * npix * 3), sem(V * npix), rgb(npix * 3);
        std::vector<unsigned short> depth(writeDepth_ ? V * npix : 0);
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        int rc = SM_OK;
        if (mapFiles) {
            std::vector<float> v16(V * 16);
            for (size_t i = 0; i < V; ++i) std::memcpy(&v16[i * 16], views[i].data(), 64);
            std::vector<const char *> paths;
            for (const std::string &f : *mapFiles) paths.push_back(f.c_str());
            const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
            SceneArgs sc;
            if (actors && !sceneArgs(*actors, V, sc, "acquireSceneImages")) return false;
            rc = actors ? sm_render_image_scene(ctx_, &src, &sc.scene, v16.data(), (uint32_t)V, w, h, fx, fy, cx, cy, fill, bgr.data(), sem.data(),
                                                writeDepth_ ? depth.data() : nullptr)
                        : sm_render_image_maps_blend(ctx_, &src, v16.data(), (uint32_t)V, w, h, fx, fy, cx, cy, blend, fill, bgr.data(), sem.data(),
                                                     writeDepth_ ? depth.data() : nullptr);
        } else {
            globalModel.setImageSize(w, h, fx, fy, cx, cy);              // as the plain overload leaves the model's image ...
            for (size_t i = 0; i < V && rc == SM_OK; ++i) {
                rc = sm_render_image_blend(ctx_, views[i].data(), w, h, fx, fy, cx, cy, blend, fill, &bgr[i * npix * 3], &sem[i * npix],
                                           writeDepth_ ? &depth[i * npix] : nullptr);
                if (rc == SM_OK) globalModel.setImage(&bgr[i * npix * 3], &sem[i * npix]);     // ... the last view, here as written
            }
        }
        if (rc != SM_OK) {
            std::printf("%s: %s\n", actors ? "acquireSceneImages" : "acquireImages", sm_last_error());
            return false;
        }
        bool ok = true;
        for (size_t i = 0; i < V; ++i, ++startId) {
            char name[32];
            std::snprintf(name, sizeof name, "%06d.png", startId);
            const unsigned char *b = &bgr[i * npix * 3];
            for (size_t p = 0; p < npix; ++p) { rgb[p * 3] = b[p * 3 + 2]; rgb[p * 3 + 1] = b[p * 3 + 1]; rgb[p * 3 + 2] = b[p * 3]; }
            const bool r1 = sm_png::write((image_path + name).c_str(), rgb.data(), w, h, 3);
            const bool r2 = sm_png::write((semantic_path + name).c_str(), &sem[i * npix], w, h, 1);
            const bool r3 = !writeDepth_ || sm_png::write16((depth_path + name).c_str(), &depth[i * npix], w, h);
            if (!(r1 && r2 && r3)) { std::printf("%s is NOT saved!\n", name); ok = false; }
        }
        return ok;
    }
    // a scene's C structs for n views: the poses as ROW-major 3x4 rows; false (a line printed) where an actor's arrays do not hold n
    struct SceneArgs { std::vector<std::vector<float>> poses; std::vector<sm_scene_actor> list; sm_scene scene{nullptr, 0}; };
    static bool sceneArgs(const std::vector<SceneActor> &actors, size_t n, SceneArgs &a, const char *who)
    {
        a.poses.resize(actors.size());
        a.list.resize(actors.size());
        for (size_t j = 0; j < actors.size(); ++j) {
            const SceneActor &act = actors[j];
            if (act.poses.size() != n || (!act.present.empty() && act.present.size() != n)) {
                std::printf("%s: actor %zu has %zu poses for %zu views\n", who, j, act.poses.size(), n);
                return false;
            }
            a.poses[j].resize(n * 12);
            for (size_t i = 0; i < n; ++i)
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 4; ++c) a.poses[j][i * 12 + r * 4 + c] = act.poses[i](r, c);
            a.list[j] = sm_scene_actor{act.file.c_str(), a.poses[j].data(), act.present.empty() ? nullptr : act.present.data()};
        }
        a.scene = sm_scene{a.list.data(), (uint32_t)a.list.size()};
        return true;
    }
    // acquireSweeps of a map set and, with actors, acquireSceneSweeps
    bool acquireSweepsOf(std::string path, const std::vector<std::string> &mapFiles, const std::vector<Eigen::Matrix4f> &poses,
                         const sm_lidar_sensor &sensor, int startId, bool includeModel, const std::vector<SceneActor> *actors)
    {
        if (path.empty() || path.back() != '/') path += "/";
        const std::string velo_path = path + "velodyne/";
        ::mkdir(velo_path.c_str(), 0755);
        if (sensor.n_az <= 0 || sensor.n_el <= 0 || (unsigned long long)sensor.n_az * (unsigned long long)sensor.n_el > SM_LIDAR_MAX_BEAMS) return false;
        const size_t nb = (size_t)sensor.n_az * sensor.n_el;
        std::vector<float> p16(poses.size() * 16), dir(nb * 3), range(poses.size() * nb);
        for (size_t i = 0; i < poses.size(); ++i) std::memcpy(&p16[i * 16], poses[i].data(), 64);
        std::vector<unsigned char> rgb(poses.size() * nb * 3);
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        SceneArgs sc;
        if (actors && !sceneArgs(*actors, poses.size(), sc, "acquireSceneSweeps")) return false;
        if (sm_lidar_directions(&sensor, dir.data()) != SM_OK ||
            (actors ? sm_lidar_sweep_scene(ctx_, &src, &sc.scene, &sensor, p16.data(), (uint32_t)poses.size(), range.data(), nullptr, rgb.data(), nullptr)
                    : sm_lidar_sweep_maps(ctx_, &src, &sensor, p16.data(), (uint32_t)poses.size(), range.data(), nullptr, rgb.data(), nullptr)) != SM_OK) {
            std::printf("%s: %s\n", actors ? "acquireSceneSweeps" : "acquireSweeps", sm_last_error());
            return false;
        }
        bool ok = true;
        std::vector<float> pts;
        for (size_t i = 0; i < poses.size(); ++i, ++startId) {
            char name[32];
            std::snprintf(name, sizeof name, "%06d.bin", startId);
            pts.clear();
            for (size_t b = 0; b < nb; ++b) {
                const float t = range[i * nb + b];
                if (!(t > 0.0f)) continue;
                const unsigned char *c = &rgb[(i * nb + b) * 3];
                const float x = t * dir[3 * b], y = t * dir[3 * b + 1], z = t * dir[3 * b + 2];
                const float lum = 0.299f * (float)c[0] + 0.587f * (float)c[1];
                pts.push_back(z); pts.push_back(-x); pts.push_back(-y);
                pts.push_back((lum + 0.114f * (float)c[2]) / 255.0f);
            }
            FILE *f = std::fopen((velo_path + name).c_str(), "wb");
            const bool w = f && std::fwrite(pts.data(), 4, pts.size(), f) == pts.size();
            if (f && std::fclose(f) != 0) ok = false;
            if (!w) { std::printf("%s is NOT saved!\n", name); ok = false; }
        }
        return ok;
    }
    std::vector<unsigned short> stereoDepth_;
    std::vector<unsigned short> lidarDepth_;
    bool beginCleanPoints = false;
    bool async_ = false;
};
