// GlobalModel.h -- drop-in for src/GlobalModel.h:16-120 over the C-ABI.  The per-pass methods
// keep the reference's names and call order (src/SurfelMapping.cpp:178-239); passes that the
// HIP core fuses into a neighbour are no-ops here (noted per method).
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/sm_c_api.h"
#include "Config.h"
#include "GPUTexture.h"
#include "sm_compat.h"

// Not in the reference: a ground map's planes (sm_ground_maps; DESIGN.md "4v. Ground map"), row-major, row = cell v, column = cell u.
struct GroundMap {
    int nu = 0, nv = 0;
    std::vector<int32_t> ground, top;  // 2^-16 m; ground: SM_GROUND_NONE without ground
    std::vector<uint8_t> state, cls;   // SM_GROUND_UNKNOWN / FREE / OBSTACLE / STEP; the ground's class, 255 without ground
    std::vector<uint8_t> bgr;          // three bytes a cell
    std::vector<uint32_t> clear2;      // squared distance in cells to the nearest blocking cell
    sm_ground_info info{};
    bool ok = false;                   // false: the call failed (the error is printed) and the planes are empty

    // the planes of nu x nv cells filled by sm_ground_maps of `src`
    static GroundMap of(sm_ctx *ctx, const sm_map_source &src, const sm_ground_params &p, const char *who)
    {
        GroundMap m;
        const size_t n = p.nu > 0 && p.nv > 0 && (long long)p.nu * p.nv <= (1ll << 24) ? (size_t)p.nu * (size_t)p.nv : 0;   // (else refused below)
        m.ground.assign(n, 0); m.top.assign(n, 0); m.state.assign(n, 0); m.cls.assign(n, 0); m.bgr.assign(n * 3, 0); m.clear2.assign(n, 0u);
        (void)sm_sync(ctx);                                              // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_ground_maps(ctx, &src, &p, m.ground.data(), m.top.data(), m.state.data(), m.cls.data(), m.bgr.data(), m.clear2.data(), &m.info) != SM_OK) {
            std::printf("%s: %s\n", who, sm_last_error());
            return GroundMap{};
        }
        m.nu = p.nu; m.nv = p.nv;
        m.ok = true;
        return m;
    }
};

// Not in the reference: the routes over a ground map (sm_route_ground; DESIGN.md "4ac. Routes"): per goal set a field of nu x nv
// cells, row-major as the ground map's planes, field after field; per start a path.
struct RouteGoal { int u, v; };
struct RouteStart { int field, u, v; };
struct RouteField {
    int nu = 0, nv = 0, fields = 0;
    std::vector<uint32_t> cost;        // SM_ROUTE_NONE without a path to a goal
    std::vector<uint8_t> next;         // the direction 0..7 of the first step, 8 at a goal, 255 without
    std::vector<std::vector<uint32_t>> paths;   // per start the cells v * nu + u of its path, the start first (truncated at max_steps + 1)
    std::vector<uint32_t> pathCost;    // per start cost[start], SM_ROUTE_NONE without a path
    std::vector<sm_route_info> info;   // per field
    bool ok = false;                   // false: the call failed (the error is printed) and everything is empty

    // the fields of the goal sets `goals` over the planes of `g`, the paths of `starts`
    static RouteField of(sm_ctx *ctx, const GroundMap &g, const std::vector<std::vector<RouteGoal>> &goals, const std::vector<RouteStart> &starts,
                         sm_route_params p, const char *who)
    {
        RouteField r;
        p.nu = g.nu; p.nv = g.nv;
        const size_t G = goals.size(), n = (size_t)g.nu * (size_t)g.nv;
        const bool fits = G >= 1 && G * n <= ((size_t)1 << 26) && p.max_steps >= 0 &&
                          starts.size() * ((size_t)p.max_steps + 1) <= ((size_t)1 << 26);             // (else refused below)
        std::vector<uint32_t> first(G + 1, 0u), path, len(starts.size(), 0u);
        std::vector<int32_t> flat, st;
        for (size_t f = 0; f < G; ++f) {
            for (const RouteGoal &q : goals[f]) { flat.push_back(q.u); flat.push_back(q.v); }
            first[f + 1] = (uint32_t)(flat.size() / 2);
        }
        for (const RouteStart &s : starts) { st.push_back(s.field); st.push_back(s.u); st.push_back(s.v); }
        const size_t row = fits ? (size_t)p.max_steps + 1 : 0;
        if (fits) { r.cost.assign(G * n, 0u); r.next.assign(G * n, 0); path.assign(starts.size() * row, 0u); r.pathCost.assign(starts.size(), 0u); }
        r.info.assign(G ? G : 1, sm_route_info{});
        (void)sm_sync(ctx);                                              // (SM_FACADE_ASYNC: frames may still be in flight)
        if (!g.ok || sm_route_ground(ctx, &p, g.state.data(), g.clear2.data(), (uint32_t)G, first.data(), flat.data(), (uint32_t)starts.size(), st.data(),
                                     fits ? r.cost.data() : nullptr, fits ? r.next.data() : nullptr, fits ? path.data() : nullptr, len.data(),
                                     fits ? r.pathCost.data() : nullptr, r.info.data()) != SM_OK) {
            std::printf("%s: %s\n", who, g.ok ? sm_last_error() : "no ground map");
            return RouteField{};
        }
        for (size_t i = 0; i < starts.size(); ++i) r.paths.emplace_back(path.begin() + i * row, path.begin() + i * row + len[i]);
        r.info.resize(G);
        r.nu = g.nu; r.nv = g.nv; r.fields = (int)G;
        r.ok = true;
        return r;
    }
};

// Not in the reference: the routes a car can follow over a ground map (sm_route_car; DESIGN.md "4ad. Routes for a car"): per goal set
// a field of 8 x nv x nu states, heading after heading, field after field; per start the path words.
struct CarGoal { int u, v, h; };       // h = -1: any heading
struct CarStart { int field, u, v, h; };
struct CarField {
    int nu = 0, nv = 0, fields = 0;
    std::vector<uint32_t> cost;        // SM_ROUTE_NONE without a way to a goal
    std::vector<uint8_t> next;         // the move SM_CAR_MOVE_* of the first step, 8 at a goal, 255 without
    std::vector<std::vector<uint32_t>> paths;   // per start the words cell | heading << 22 | reverse << 25 of its path, the start first
    std::vector<uint32_t> pathCost;    // per start cost[start], SM_ROUTE_NONE without a path
    std::vector<sm_route_car_info> info;   // per field
    bool ok = false;                   // false: the call failed (the error is printed) and everything is empty

    static uint32_t cell(uint32_t word) { return word & 0x3FFFFFu; }
    static int heading(uint32_t word) { return (int)(word >> 22 & 7u); }
    static bool reverse(uint32_t word) { return (word >> 25 & 1u) != 0; }

    // the fields of the goal sets `goals` over the planes of `g`, the paths of `starts`
    static CarField of(sm_ctx *ctx, const GroundMap &g, const std::vector<std::vector<CarGoal>> &goals, const std::vector<CarStart> &starts,
                       sm_route_car_params p, const char *who)
    {
        CarField r;
        p.nu = g.nu; p.nv = g.nv;
        const size_t G = goals.size(), n = (size_t)g.nu * (size_t)g.nv;
        const bool fits = G >= 1 && G * n <= ((size_t)1 << 23) && p.max_steps >= 0 &&
                          starts.size() * ((size_t)p.max_steps + 1) <= ((size_t)1 << 26);             // (else refused below)
        std::vector<uint32_t> first(G + 1, 0u), path, len(starts.size(), 0u);
        std::vector<int32_t> flat, st;
        for (size_t f = 0; f < G; ++f) {
            for (const CarGoal &q : goals[f]) { flat.push_back(q.u); flat.push_back(q.v); flat.push_back(q.h); }
            first[f + 1] = (uint32_t)(flat.size() / 3);
        }
        for (const CarStart &s : starts) { st.push_back(s.field); st.push_back(s.u); st.push_back(s.v); st.push_back(s.h); }
        const size_t row = fits ? (size_t)p.max_steps + 1 : 0;
        if (fits) { r.cost.assign(G * 8 * n, 0u); r.next.assign(G * 8 * n, 0); path.assign(starts.size() * row, 0u); r.pathCost.assign(starts.size(), 0u); }
        r.info.assign(G ? G : 1, sm_route_car_info{});
        (void)sm_sync(ctx);                                              // (SM_FACADE_ASYNC: frames may still be in flight)
        if (!g.ok || sm_route_car(ctx, &p, g.state.data(), g.clear2.data(), (uint32_t)G, first.data(), flat.data(), (uint32_t)starts.size(), st.data(),
                                  fits ? r.cost.data() : nullptr, fits ? r.next.data() : nullptr, fits ? path.data() : nullptr, len.data(),
                                  fits ? r.pathCost.data() : nullptr, r.info.data()) != SM_OK) {
            std::printf("%s: %s\n", who, g.ok ? sm_last_error() : "no ground map");
            return CarField{};
        }
        for (size_t i = 0; i < starts.size(); ++i) r.paths.emplace_back(path.begin() + i * row, path.begin() + i * row + len[i]);
        r.info.resize(G);
        r.nu = g.nu; r.nv = g.nv; r.fields = (int)G;
        r.ok = true;
        return r;
    }
};

class GlobalModel {
public:
    explicit GlobalModel(sm_ctx *ctx = nullptr)
        : TEXTURE_DIMENSION(Config::maxSqrtVertices()), MAX_VERTICES(TEXTURE_DIMENSION * TEXTURE_DIMENSION), ctx_(ctx) {}
    void bind(sm_ctx *ctx) { ctx_ = ctx; }

    const int TEXTURE_DIMENSION;
    const int MAX_VERTICES;

    // p2 (+p3): src/GlobalModel.cpp:396-515
    void processConflict(const Eigen::Matrix4f &pose, const int & /*time*/, GPUTexture * /*depthRaw*/, GPUTexture * /*semantic*/,
                         float minDepth, float maxDepth, float fuseThresh = Config::surfelFuseDistanceThreshFactor(), int isClean = 0)
    {
        if (sm_stage_conflict(ctx_, pose.data(), minDepth, maxDepth, fuseThresh, isClean) == SM_OK) pending_ = true;
        else std::printf("processConflict: %s\n", sm_last_error());
    }
    void updateConflict() {}                       // in-place decrement, applied by backMapping()
    // p4/p10: src/GlobalModel.cpp:517-579 (the 2nd call per frame copies nothing: fuse is in place)
    void backMapping()
    {
        if (pending_) { if (sm_stage_cull(ctx_) != SM_OK) std::printf("backMapping: %s\n", sm_last_error()); pending_ = false; }
    }
    void buildModelMap() {}                        // no mirror textures (src/GlobalModel.cpp:639-681)
    // p8 + p9 + p11: src/GlobalModel.cpp:246-394,581-637
    void dataAssociate(const Eigen::Matrix4f &pose, const int &time, GPUTexture *, GPUTexture *, GPUTexture *, GPUTexture *,
                       GPUTexture *, GPUTexture *, GPUTexture *, float depthMin, float depthMax)
    {
        int rc = sm_stage_associate_fuse(ctx_, pose.data(), time, depthMin, depthMax);
        if (rc != SM_OK) std::printf("dataAssociate: %s\n", sm_last_error());
    }
    void updateFuse() {}
    void concatenate() {}

    std::pair<GLuint, GLuint> getModel() { return {0u, counts().count}; }
    std::pair<GLuint, GLuint> getData() { return {0u, counts().data_count}; }
    std::pair<GLuint, GLuint> getConflict() { return {0u, counts().conflict_count}; }
    std::pair<GLuint, GLuint> getUnstable() { return {0u, counts().unstable_count}; }
    unsigned int getOffset() { return counts().offset; }

    // src/GlobalModel.cpp:901-1011, same file format and diagnostics
    bool downloadMap(const std::string &path, int startId, int endId)
    {
        if (sm_save_map(ctx_, path.c_str(), startId, endId) != SM_OK) { std::printf("%s\n", sm_last_error()); return false; }
        std::printf("%s is saved! Saved model count: %d\n", path.c_str(), (int)counts().count);
        return true;
    }
    bool uploadMap(const std::string &model_path, std::vector<int> &start_end_ids)
    {
        int32_t a = 0, b = 0;
        if (sm_load_map(ctx_, model_path.c_str(), &a, &b) != SM_OK) { std::printf("%s\n", sm_last_error()); return false; }
        std::printf("Load model count: %d\nRead model from %s.\n", (int)counts().count, model_path.c_str());
        start_end_ids.clear(); start_end_ids.push_back(a); start_end_ids.push_back(b);
        return true;
    }
    void resetBuffer() { sm_reset(ctx_); }

    // Not in the reference, whose operator saves the whole map and resets it when the capacity bar fills (build_map.cpp:204,
    // 235-263): moves the surfels last updated more than minAge frames ago and farther than minDistance metres from the
    // camera centre of `pose` out of the model into `out` (12 floats each, model order), the rest stays (sm_retire).
    bool retire(const Eigen::Matrix4f &pose, int minAge, float minDistance, std::vector<float> &out)
    {
        const sm_retire_params p = {minAge, minDistance};
        uint32_t n = 0;
        out.clear();
        if (sm_retire(ctx_, pose.data(), &p, nullptr, 0, &n) != SM_OK) { std::printf("retire: %s\n", sm_last_error()); return false; }
        out.resize((size_t)n * 12 + 12);             // never empty: a null destination would be a dry run
        if (sm_retire(ctx_, pose.data(), &p, out.data(), n, &n) != SM_OK) { std::printf("retire: %s\n", sm_last_error()); out.clear(); return false; }
        out.resize((size_t)n * 12);
        return true;
    }

    // A correction that is a function of a surfel's last-update time (sm_warp_by_time): every surfel of the model and of the map
    // files `mapFiles` whose time tau is >= t0 is moved by row min(int(tau - t0), rows - 1) of `corr12` (12 floats per row: a
    // row-major 3x4 world->world [R|t]); files that hold such a surfel are rewritten in place.  Returns how many surfels moved
    // (model and files together), or -1 with the error printed.
    long warpByTime(const std::vector<std::string> &mapFiles, int t0, const std::vector<float> &corr12, bool includeModel = true)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        sm_warp_stats_t st;
        if (sm_warp_by_time(ctx_, &src, t0, (uint32_t)(corr12.size() / 12), corr12.data()) != SM_OK || sm_warp_stats(ctx_, &st) != SM_OK) {
            std::printf("warpByTime: %s\n", sm_last_error());
            return -1;
        }
        return (long)(st.records_moved + st.model_moved);
    }

    // The reverse: the records of the map files `mapFiles` (downloadMap's format, the files of SurfelMapping::setAutoRetire) that
    // lie within `radius` metres of the camera centre of `pose` are appended to the model, in the order of the files and of their
    // records, and -- unless keepFiles -- taken out of the files (sm_recall).  Returns how many came back, or -1 with the error
    // printed (then neither the model nor the files have changed, but for a failed rename: see sm_c_api.h).
    long recall(const std::vector<std::string> &mapFiles, const Eigen::Matrix4f &pose, float radius, bool keepFiles = false)
    {
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), 0};
        const sm_recall_params p = {radius};
        uint32_t n = 0;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_recall(ctx_, &src, pose.data(), &p, keepFiles ? SM_RECALL_COPY : SM_RECALL_MOVE, &n) != SM_OK) {
            std::printf("recall: %s\n", sm_last_error());
            return -1;
        }
        return (long)n;
    }

    // Not in the reference: the surfels that share a cell of voxelMm millimetres of the world grid, a class and (splitNormals) a
    // facing direction become one (sm_simplify; DESIGN.md "4p. Simplification"); what is alone in its cell stays as it is.
    // Returns the surfels the model holds afterwards, or -1 with the error printed (the model is then unchanged).
    long simplify(int voxelMm = 50, bool splitNormals = true)
    {
        sm_simplify_params p;
        sm_default_simplify_params(&p);
        p.voxel_mm = voxelMm;
        p.split_normals = splitNormals ? 1 : 0;
        sm_simplify_stats_t st;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_simplify(ctx_, &p) != SM_OK || sm_simplify_stats(ctx_, &st) != SM_OK) {
            std::printf("simplify: %s\n", sm_last_error());
            return -1;
        }
        return (long)st.records_out;
    }

    // Not in the reference: the surface the model's surfels lie on as a triangle mesh (sm_mesh_maps on the live model alone;
    // DESIGN.md "4u. Meshing"), written to plyPath as a binary PLY.  voxelMm: the cell edge; reach 2 closes the holes reach 1
    // leaves where the surface clips a cell corner.  The model is unchanged.  Returns the faces, or -1 with the error printed.
    long mesh(const std::string &plyPath, int voxelMm = 100, int reach = 2, sm_mesh_info *info = nullptr)
    {
        sm_mesh_params p;
        sm_default_mesh_params(&p);
        p.voxel_mm = voxelMm;
        p.reach = reach;
        const sm_map_source src{nullptr, 0u, 1};
        sm_mesh_info got;
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_mesh_maps(ctx_, &src, &p, nullptr, 0, nullptr, 0, plyPath.empty() ? nullptr : plyPath.c_str(), &got) != SM_OK) {
            std::printf("mesh: %s\n", sm_last_error());
            return -1;
        }
        if (info) *info = got;
        return (long)got.faces;
    }

    // Not in the reference: the live model alone as a planner's ground map (sm_ground_maps; DESIGN.md "4v. Ground map"): per cell of
    // the window the ground height, the state FREE / OBSTACLE / STEP / UNKNOWN, the ground's colour and class and the squared
    // distance to the nearest blocking cell.  params: null = the defaults (100 mm cells, 256 x 256 of them at the origin, -y up).
    // The model is unchanged.
    GroundMap groundMap(const sm_ground_params *params = nullptr)
    {
        sm_ground_params p;
        sm_default_ground_params(&p);
        if (params) p = *params;
        return GroundMap::of(ctx_, sm_map_source{nullptr, 0u, 1}, p, "groundMap");
    }

    // Not in the reference: routes over a ground map (sm_route_ground; DESIGN.md "4ac. Routes"): per goal set the least cost of an
    // 8-connected path from every cell to a goal and the direction of its first step, per start the path.  params: null = the
    // defaults; nu and nv are the ground map's.  The model is neither read nor changed.
    RouteField routeGround(const GroundMap &ground, const std::vector<std::vector<RouteGoal>> &goals, const std::vector<RouteStart> &starts = {},
                           const sm_route_params *params = nullptr)
    {
        sm_route_params p;
        sm_default_route_params(&p);
        if (params) p = *params;
        return RouteField::of(ctx_, ground, goals, starts, p, "routeGround");
    }

    // Not in the reference: routes a car can follow (sm_route_car; DESIGN.md "4ad. Routes for a car"): per goal set the least weight
    // of a sequence of car moves from every (cell, heading) to a goal state and the first move, per start the path.  params: null =
    // the defaults; nu and nv are the ground map's.  The model is neither read nor changed.
    CarField routeCar(const GroundMap &ground, const std::vector<std::vector<CarGoal>> &goals, const std::vector<CarStart> &starts = {},
                      const sm_route_car_params *params = nullptr)
    {
        sm_route_car_params p;
        sm_default_route_car_params(&p);
        if (params) p = *params;
        return CarField::of(ctx_, ground, goals, starts, p, "routeCar");
    }

    // model read-back in the reference's AoS layout (12 floats / surfel, src/Config.cpp:17-32)
    std::vector<float> downloadModel()
    {
        uint32_t n = 0;
        sm_download_model_aos(ctx_, nullptr, 0, &n);
        std::vector<float> v((size_t)n * 12);
        if (n) sm_download_model_aos(ctx_, v.data(), n, &n);
        return v;
    }

    // novel views for SPADE (src/GlobalModel.cpp:772-833): rendered by the HIP core, kept on the host
    void setImageSize(int w, int h, float fx, float fy, float cx, float cy)
    {
        iw_ = w; ih_ = h; ifx_ = fx; ify_ = fy; icx_ = cx; icy_ = cy;
        imageBgr_.assign((size_t)w * h * 3, 0);
        imageSem_.assign((size_t)w * h, 0);
        imageTex_.texture->width = semTex_.texture->width = w;
        imageTex_.texture->height = semTex_.texture->height = h;
    }
    void renderImage(const Eigen::Matrix4f &view)
    {
        if (sm_render_image(ctx_, view.data(), iw_, ih_, ifx_, ify_, icx_, icy_, imageBgr_.data(), imageSem_.data()) != SM_OK)
            std::printf("renderImage: %s\n", sm_last_error());
    }
    // a view of setImageSize's size that somebody else rendered (acquireImages with hole filling or depth): kept like renderImage's
    void setImage(const unsigned char *bgr, const unsigned char *sem)
    {
        imageBgr_.assign(bgr, bgr + (size_t)iw_ * ih_ * 3);
        imageSem_.assign(sem, sem + (size_t)iw_ * ih_);
    }
    pangolin::GlTexture *getImageTex() { return imageTex_.texture; }
    pangolin::GlTexture *getSemanticTex() { return semTex_.texture; }
    const std::vector<unsigned char> &imageBGR() const { return imageBgr_; }      // h*w*3, B,G,R (FragColor = srgb.wzy)
    const std::vector<unsigned char> &imageSemantic() const { return imageSem_; } // h*w, class + 1, 0 = empty
    int imageWidth() const { return iw_; }
    int imageHeight() const { return ih_; }

    // src/GlobalModel.cpp:683-758 (signature src/GlobalModel.h:27-37).  The compute core keeps no GL buffer: the model is
    // pulled to the host when somebody looks (the reference's AoS layout, 12 floats per surfel) and, built with
    // SM_FACADE_GL, drawn as GL_POINTS; `threshold` / `time` / `timeDelta` select what the reference's shader discards
    // (confidence below threshold unless drawUnstable, last seen more than timeDelta frames ago) -- applied on the host copy.
    void renderModel(pangolin::OpenGlMatrix mvp, pangolin::OpenGlMatrix mv, float threshold, bool drawUnstable, bool drawNormals,
                     bool drawColors, bool drawPoints, bool drawWindow, bool drawSemantic, int time, int timeDelta)
    {
        (void)mv; (void)drawNormals; (void)drawColors; (void)drawPoints; (void)drawWindow; (void)drawSemantic; (void)time; (void)timeDelta;
        refreshHostModel();
        drawn_.clear();
        const size_t n = hostModel_.size() / 12;
        for (size_t k = 0; k < n; ++k) {
            const float *v = &hostModel_[k * 12];
            if (!drawUnstable && v[3] < threshold) continue;                 // draw_surface.vert: confidence gate
            drawn_.insert(drawn_.end(), v, v + 3);
        }
#ifdef SM_FACADE_GL
        glMatrixMode(GL_PROJECTION); glLoadIdentity(); glMultMatrixd(mvp.m);
        glMatrixMode(GL_MODELVIEW); glLoadIdentity();
        glEnableClientState(GL_VERTEX_ARRAY);
        glVertexPointer(3, GL_FLOAT, 0, drawn_.data());
        glDrawArrays(GL_POINTS, 0, (GLsizei)(drawn_.size() / 3));
        glDisableClientState(GL_VERTEX_ARRAY);
#else
        (void)mvp;
#endif
    }
    size_t lastDrawnCount() const { return drawn_.size() / 3; }

    // renderModel's arguments plus a viewport: the model view rendered by the HIP core (sm_render_model) into a host image --
    // the five colour modes, the confidence gate, the unstable switch, discs or points, as the reference's shaders draw them.
    // `clear` is the glClearColor of the view.  The image is RGBA8, w*h*4 bytes, GL row order (row 0 = bottom).
    bool renderModelImage(pangolin::OpenGlMatrix mvp, pangolin::OpenGlMatrix mv, float threshold, bool drawUnstable, bool drawNormals,
                          bool drawColors, bool drawPoints, bool drawWindow, bool drawSemantic, int time, int timeDelta, int w, int h,
                          const float clear[4])
    {
        sm_model_view v{};
        fillModelView(v, mvp, mv, threshold, drawUnstable, drawNormals, drawColors, drawPoints, drawWindow, drawSemantic, time, timeDelta, w, h, clear);
        modelImage_.resize((size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0) * 4);
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_render_model(ctx_, &v, modelImage_.data(), nullptr, nullptr) != SM_OK) {
            std::printf("renderModelImage: %s\n", sm_last_error());
            return false;
        }
        return true;
    }
    // The same view of a map set: the map files `mapFiles` (downloadMap's format, the files of SurfelMapping::setAutoRetire) in
    // that order, then -- includeModel -- the live model, streamed through the core without loading them
    // (sm_render_model_maps): the image equals renderModelImage of a model that is their concatenation.
    bool renderModelImage(pangolin::OpenGlMatrix mvp, pangolin::OpenGlMatrix mv, float threshold, bool drawUnstable, bool drawNormals,
                          bool drawColors, bool drawPoints, bool drawWindow, bool drawSemantic, int time, int timeDelta, int w, int h,
                          const float clear[4], const std::vector<std::string> &mapFiles, bool includeModel = true)
    {
        sm_model_view v{};
        fillModelView(v, mvp, mv, threshold, drawUnstable, drawNormals, drawColors, drawPoints, drawWindow, drawSemantic, time, timeDelta, w, h, clear);
        modelImage_.resize((size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0) * 4);
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_render_model_maps(ctx_, &src, &v, 1, modelImage_.data(), nullptr, nullptr) != SM_OK) {
            std::printf("renderModelImage: %s\n", sm_last_error());
            return false;
        }
        return true;
    }
    const std::vector<unsigned char> &modelImageRGBA() const { return modelImage_; }

    // What a lidar `sensor` at `pose` (sensor->world, the camera's axes) measures in the model (sm_lidar_sweep): per beam of the
    // n_el x n_az grid, row-major, the range (0: no return), the surfel's id (-1), its colour bytes and its class + 1 (0).
    struct LidarReturns { std::vector<float> range; std::vector<int32_t> id; std::vector<unsigned char> rgb, sem; };
    bool lidarSweep(const Eigen::Matrix4f &pose, const sm_lidar_sensor &sensor, LidarReturns &out)
    {
        const size_t nb = (size_t)(sensor.n_az > 0 ? sensor.n_az : 0) * (size_t)(sensor.n_el > 0 ? sensor.n_el : 0);
        out.range.assign(nb, 0.0f); out.id.assign(nb, -1); out.rgb.assign(nb * 3, 0); out.sem.assign(nb, 0);
        (void)sm_sync(ctx_);                                             // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_lidar_sweep(ctx_, &sensor, pose.data(), out.range.data(), out.id.data(), out.rgb.data(), out.sem.data()) != SM_OK) {
            std::printf("lidarSweep: %s\n", sm_last_error());
            return false;
        }
        return true;
    }

    // What a list of rays (sm_ray: origin, t_min, dir, t_max; world frame) hits in the model (sm_cast_rays_maps): per ray the t of the
    // nearest hitting surfel in units of |dir| (0: none), its id (-1), its colour bytes, its class + 1 (0) and its stored normal.
    struct RayReturns { std::vector<float> t; std::vector<int32_t> id; std::vector<unsigned char> rgb, sem; std::vector<float> normal; };
    bool castRays(const std::vector<sm_ray> &rays, RayReturns &out, const sm_rays_params *params = nullptr)
    {
        return castRaysOf(ctx_, {}, true, rays, out, params, "castRays");
    }
    // (SurfelMapping::castRays casts into a map set through this)
    static bool castRaysOf(sm_ctx *ctx, const std::vector<std::string> &mapFiles, bool includeModel, const std::vector<sm_ray> &rays, RayReturns &out,
                           const sm_rays_params *params, const char *who)
    {
        const size_t n = rays.size();
        out.t.assign(n, 0.0f); out.id.assign(n, -1); out.rgb.assign(n * 3, 0); out.sem.assign(n, 0); out.normal.assign(n * 3, 0.0f);
        sm_rays_params p;
        sm_default_rays_params(&p);
        if (params) p = *params;
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        (void)sm_sync(ctx);                                              // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_cast_rays_maps(ctx, &src, &p, rays.data(), (uint32_t)n, out.t.data(), out.id.data(), out.rgb.data(), out.sem.data(), out.normal.data()) != SM_OK) {
            std::printf("%s: %s\n", who, sm_last_error());
            return false;
        }
        return true;
    }

    // The nearest disc of the model to each of a list of points (sm_point: position and reach; world frame, metres) within that reach
    // (sm_query_points_maps): per point the squared distance (+inf: none), the surfel's id (-1), its centre, stored normal and
    // radius, its colour bytes and its class + 1 (0).
    struct PointReturns {
        std::vector<float> d2; std::vector<int32_t> id; std::vector<float> centre, normal, radius; std::vector<unsigned char> rgb, sem;
    };
    bool queryPoints(const std::vector<sm_point> &points, PointReturns &out, const sm_points_params *params = nullptr)
    {
        return queryPointsOf(ctx_, {}, true, points, out, params, "queryPoints");
    }
    // (SurfelMapping::queryPoints queries a map set through this)
    static bool queryPointsOf(sm_ctx *ctx, const std::vector<std::string> &mapFiles, bool includeModel, const std::vector<sm_point> &points,
                              PointReturns &out, const sm_points_params *params, const char *who)
    {
        const size_t n = points.size();
        out.d2.assign(n, std::numeric_limits<float>::infinity()); out.id.assign(n, -1); out.centre.assign(n * 3, 0.0f); out.normal.assign(n * 3, 0.0f);
        out.radius.assign(n, 0.0f); out.rgb.assign(n * 3, 0); out.sem.assign(n, 0);
        sm_points_params p;
        sm_default_points_params(&p);
        if (params) p = *params;
        std::vector<const char *> paths;
        for (const std::string &f : mapFiles) paths.push_back(f.c_str());
        const sm_map_source src{paths.data(), (uint32_t)paths.size(), includeModel ? 1 : 0};
        (void)sm_sync(ctx);                                              // (SM_FACADE_ASYNC: frames may still be in flight)
        if (sm_query_points_maps(ctx, &src, &p, points.data(), (uint32_t)n, out.d2.data(), out.id.data(), out.centre.data(), out.normal.data(),
                                 out.radius.data(), out.rgb.data(), out.sem.data()) != SM_OK) {
            std::printf("%s: %s\n", who, sm_last_error());
            return false;
        }
        return true;
    }

    // The model-aligned mirror textures (src/GlobalModel.cpp:639-681) do not exist in the compute core.  GUI::drawCapacity
    // (build_map.cpp:204) shows the fill level of the TEXTURE_DIMENSION^2 normal/radius mirror: the handle is filled lazily --
    // size TEXTURE_DIMENSION x TEXTURE_DIMENSION, and (without GL) the host copy of the plane for whoever wants to look.
    pangolin::GlTexture *getModelMapVC() { return fillMirror(mapVC_, 0); }
    pangolin::GlTexture *getModelMapCT() { return fillMirror(mapCT_, 4); }
    pangolin::GlTexture *getModelMapNR() { return fillMirror(mapNR_, 8); }
    const std::vector<float> &mirrorHost(int which) const { return mirror_[which]; }      // 0 VC, 1 CT, 2 NR: count x 4 floats

private:
    // renderModel's arguments plus a viewport as the core takes them
    static void fillModelView(sm_model_view &v, const pangolin::OpenGlMatrix &mvp, const pangolin::OpenGlMatrix &mv, float threshold,
                              bool drawUnstable, bool drawNormals, bool drawColors, bool drawPoints, bool drawWindow, bool drawSemantic,
                              int time, int timeDelta, int w, int h, const float clear[4])
    {
        double inv[16];
        invert4d(mv.m, inv);                                             // mv.Inverse() in double, as pangolin computes it
        for (int i = 0; i < 16; ++i) { v.mvp[i] = (float)mvp.m[i]; v.mv_inv[i] = (float)inv[i]; }
        v.threshold = threshold;
        v.color_type = drawNormals ? 1 : drawColors ? 2 : drawSemantic ? 3 : 0;    // src/GlobalModel.cpp:702
        v.draw_unstable = drawUnstable; v.draw_points = drawPoints; v.draw_window = drawWindow;
        v.time = time; v.time_delta = timeDelta;
        v.width = w; v.height = h;
        for (int c = 0; c < 4; ++c) {
            const float x = clear ? clear[c] : 0.0f;
            v.clear_rgba[c] = (uint8_t)std::floor((x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x) * 255.0f + 0.5f);
        }
    }
    // general 4x4 inverse by cofactors (column-major, double)
    static void invert4d(const double *m, double *o)
    {
        double c[16];
        c[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
        c[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
        c[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
        c[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
        c[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
        c[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
        c[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
        c[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
        c[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
        c[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
        c[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
        c[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
        c[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
        c[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
        c[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
        c[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
        const double det = m[0] * c[0] + m[1] * c[4] + m[2] * c[8] + m[3] * c[12];
        for (int i = 0; i < 16; ++i) o[i] = c[i] / det;
    }
    void refreshHostModel() { hostModel_ = downloadModel(); }
    pangolin::GlTexture *fillMirror(GPUTexture &t, int off)
    {
        refreshHostModel();
        std::vector<float> &m = mirror_[off / 4];
        const size_t n = hostModel_.size() / 12;
        m.resize(n * 4);
        for (size_t k = 0; k < n; ++k)
            for (int c = 0; c < 4; ++c) m[k * 4 + c] = hostModel_[k * 12 + off + c];
        if (off == 4) for (size_t k = 0; k < n; ++k) m[k * 4 + 1] = (float)k;            // map.vert:32 stores float(index) in .y
        t.texture->width = TEXTURE_DIMENSION;
        t.texture->height = TEXTURE_DIMENSION;
#ifdef SM_FACADE_GL
        if (!t.texture->tid) t.texture->Reinitialise(TEXTURE_DIMENSION, TEXTURE_DIMENSION, GL_RGBA32F, false, 0, GL_RGBA, GL_FLOAT);
        const int rows = (int)((n + TEXTURE_DIMENSION - 1) / TEXTURE_DIMENSION);
        if (rows) { m.resize((size_t)rows * TEXTURE_DIMENSION * 4, 0.0f); t.texture->Upload(m.data(), 0, 0, TEXTURE_DIMENSION, rows, GL_RGBA, GL_FLOAT); }
#endif
        return t.texture;
    }
    // (sm_sync first: with SM_FACADE_ASYNC frames may still be in flight, and sm_get_counts returns the counters of the last wait)
    sm_counts counts() { sm_counts c{}; (void)sm_sync(ctx_); sm_get_counts(ctx_, &c); return c; }
    std::vector<float> hostModel_, drawn_, mirror_[3];
    sm_ctx *ctx_;
    bool pending_ = false;
    GPUTexture mapVC_, mapCT_, mapNR_, imageTex_, semTex_;
    int iw_ = 0, ih_ = 0;
    float ifx_ = 0, ify_ = 0, icx_ = 0, icy_ = 0;
    std::vector<unsigned char> imageBgr_, imageSem_, modelImage_;
};
