// sm_mesh.hip -- a map set turned into a triangle mesh (sm_mesh_maps; DESIGN.md "4u. Meshing"): the set streamed once into a voxel
// table of cells; the cells' lattice points claimed in a second table sized from the cell count; the field summed per lattice
// point, the cubes classified, the owners of a vertex or a face sorted by key and ranked; vertices and faces written at their ranks
// and brought back in pieces while the host fills the caller's buffers and the PLY file.  Kernels: sm_k_mesh.h; the grid, the
// tables' sizes, the tally's verdict, the pair sort and the ranks: sm_voxel.h; the call's frame and the drain: sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_mesh.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
enum { EV_CLR0 = 0, EV_CLR1, EV_INS0, EV_INS1, EV_FIELD0, EV_FIELD1, EV_SORT0, EV_SORT1, EV_EMIT0, EV_EMIT1, EV_PIECE, N_EV = EV_PIECE + 2 };
static_assert(N_EV == decltype(Mesh::scratch)::N_EV, "the context holds the events of a call");
static_assert(sizeof(MeshVertex) == sizeof(sm_mesh_vertex), "a vertex leaves the device as it is");
static_assert(MESH_USED == SM_MESH_USED && MESH_SKIPPED == SM_MESH_SKIPPED && MESH_LOOSE == SM_MESH_LOOSE && MESH_OUTSIDE == SM_MESH_OUTSIDE,
              "the kinds are the entries of info->counts");

int check_params(const sm_mesh_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->voxel_mm < 10 || p->voxel_mm > 10000) return bad("voxel_mm outside 10..10000");
    if (p->reach != 1 && p->reach != 2) return bad("reach is 1 or 2");
    if (p->min_records == 0) return bad("min_records is 0");
    if (p->max_cells == 0) return bad("max_cells is 0");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    return SM_OK;
}

// The file: a binary little-endian PLY written as a temporary; whatever has not been renamed when the call ends is removed.
struct PlyFile {
    const char *who;
    std::string tmp, path;
    FILE *f = nullptr;
    std::vector<uint8_t> rows;

    explicit PlyFile(const char *who_) : who(who_) {}
    ~PlyFile()
    {
        if (f) std::fclose(f);
        if (!tmp.empty()) std::remove(tmp.c_str());
    }
    int fail() { g_err = sm_mapfile::said(who, path, " saved err!!"); return SM_E_ARG; }
    int open(const char *ply_path, uint32_t nv, uint32_t nf)
    {
        path = ply_path;
        tmp = path + ".mesh.tmp";
        if (!(f = std::fopen(tmp.c_str(), "wb"))) { tmp.clear(); return fail(); }
        const std::string h = "ply\nformat binary_little_endian 1.0\ncomment surfelmapping mesh\nelement vertex " + std::to_string(nv) +
                              "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar class\nelement face " + std::to_string(nf) +
                              "\nproperty list uchar int vertex_indices\nend_header\n";
        return std::fwrite(h.data(), 1, h.size(), f) == h.size() ? SM_OK : fail();
    }
    // m vertices: x y z nx ny nz as they are, then red, green, blue -- bytes 2, 1, 0 of the colour word -- and the class, byte 3
    int vertices(const sm_mesh_vertex *v, size_t m)
    {
        rows.resize(m * 28);
        for (size_t i = 0; i < m; ++i) {
            uint8_t *r = rows.data() + i * 28;
            memcpy(r, &v[i], 24);
            const uint32_t c = v[i].colour;
            r[24] = (uint8_t)(c >> 16); r[25] = (uint8_t)(c >> 8); r[26] = (uint8_t)c; r[27] = (uint8_t)(c >> 24);
        }
        return std::fwrite(rows.data(), 1, rows.size(), f) == rows.size() ? SM_OK : fail();
    }
    int faces(const uint32_t *v, size_t m)
    {
        rows.resize(m * 13);
        for (size_t i = 0; i < m; ++i) {
            uint8_t *r = rows.data() + i * 13;
            r[0] = 3;
            memcpy(r + 1, v + i * 3, 12);
        }
        return std::fwrite(rows.data(), 1, rows.size(), f) == rows.size() ? SM_OK : fail();
    }
    int commit()
    {
        const bool ok = std::fclose(f) == 0;
        f = nullptr;
        if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) return fail();
        tmp.clear();
        return SM_OK;
    }
};

// One call's device side: the two tables, the owners' pairs, the mesh, the launches on the context's stream.
struct MeshJob {
    sm_ctx *s;
    Mesh &me;
    const Event *ev;
    const char *who;
    const sm_mesh_params &p;
    SimplifyArgs a{};
    MeshArgs ma{};
    SimplifyTable T{};                 // key, SW, SP, SN, SC and n
    unsigned long long *cmin = nullptr;
    MeshLattice L{};
    Dev<uint8_t> cells, lattice;       // everything below is freed when the call ends
    Dev<unsigned long long> d_key[2];
    Dev<uint32_t> d_idx[2], d_hist, d_faces;
    Dev<MeshVertex> d_vert;
    RankedOutput out;                  // (for the ranks; it opens no file)
    uint32_t launches = 0;
    sm_mesh_stats_t stats{};           // this call's; the context's once the call has succeeded

    MeshJob(sm_ctx *s_, const char *who_, const sm_mesh_params &p_) : s(s_), me(s_->mesh), ev(s_->mesh.scratch.ev), who(who_), p(p_), out(s_, who_) {}

    uint32_t *tally() const { return me.scratch.d_tally.get(); }
    const uint32_t *h() const { return me.scratch.h(); }
    int read_tally() { return me.scratch.read(s); }

    int open(uint64_t records)
    {
        int rc;
        uint64_t slots;
        if ((rc = me.scratch.ensure(MESH_TALLY_WORDS)) || (rc = voxel_slots(records, p.max_cells, who, "the cell table", slots)) || (rc = out.ensure(0, 0))) return rc;
        a = voxel_args(p.voxel_mm, 0, p.origin, 0, p.max_cells);
        for (int i = 0; i < 8; ++i) ma.class_mask[i] = p.class_mask[i];
        ma.reach = p.reach;
        ma.min_records = p.min_records;
        // key, cmin (all ones) | SW, SP[3], SN[3], SC[3], n (zero)
        const size_t S = (size_t)slots;
        if ((rc = dalloc(cells, S * (MESH_CELL_ONES + MESH_CELL_ZERO)))) return rc;
        uint8_t *b = cells.get();
        T.key = (unsigned long long *)b;
        cmin = T.key + S;
        T.SW = cmin + S; T.SP = T.SW + S; T.SN = T.SP + 3 * S; T.SC = T.SN + 3 * S;
        T.n = (uint32_t *)(T.SC + 3 * S);
        T.mask = (uint32_t)(S - 1);
        T.tally = tally();
        if ((rc = mark(s, ev[EV_CLR0]))) return rc;
        HIPCK(hipMemsetAsync(b, 0xFF, S * MESH_CELL_ONES, s->stream));
        HIPCK(hipMemsetAsync(b + S * MESH_CELL_ONES, 0, S * MESH_CELL_ZERO, s->stream));
        if ((rc = me.scratch.clear(s->stream))) return rc;
        HIPCK(hipMemsetAsync(tally() + MESH_AND, 0xFF, 8, s->stream));
        return mark(s, ev[EV_CLR1]);
    }
    // the reading of n <= CHUNK records
    void insert(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        hipLaunchKernelGGL(k_mesh_insert, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, a, ma, T, cmin);
        launches++;
        stats.chunks++;
    }
    // The lattice points of `cells` cells claimed in a table of their own.  A sheet of cells shares most of its points: the table
    // begins at 8 (reach 1: 4) points a cell.  Sparse cells share none: the kernel then stops at the table's error word (no walk
    // is longer than MESH_CLAIM_WALK), and the table is doubled and claimed again; at 64 (8) a cell the count cannot pass half of it.
    int claim(uint32_t ncells)
    {
        int rc;
        const uint32_t most = p.reach == 2 ? 64u : 8u, least = p.reach == 2 ? 8u : 4u;
        for (uint32_t per_cell = least;; per_cell *= 2u) {
            const uint64_t points = (uint64_t)ncells * per_cell;
            uint64_t S = SIMP_MIN_SLOTS;
            while (S < 2 * points) S <<= 1;
            if (S > (1ull << 31)) { g_err = std::string(who) + ": the lattice table would need more than 2^31 slots"; return SM_E_CAPACITY; }
            lattice = Dev<uint8_t>();
            if ((rc = dalloc(lattice, (size_t)S * MESH_LAT_BYTES))) return rc;
            uint8_t *b = lattice.get();
            L.key = (unsigned long long *)b;
            L.F = (double *)(L.key + S);
            L.W = (unsigned long long *)(L.F + S); L.NS = L.W + S; L.CS = L.NS + 3 * S; L.cmin = L.CS + 3 * S;
            L.faces = (uint32_t *)(L.cmin + S); L.used = L.faces + S; L.vbase = L.used + S; L.fbase = L.vbase + S;
            L.mask = (uint32_t)(S - 1);
            L.tally = tally();
            HIPCK(hipMemsetAsync(L.key, 0xFF, (size_t)S * 8, s->stream));
            HIPCK(hipMemsetAsync(L.faces, 0, (size_t)S * 8, s->stream));             // faces and used
            HIPCK(hipMemsetAsync(tally() + MESH_LAT, 0, SIMP_TALLY_WORDS * 4, s->stream));
            SimplifyArgs al = a;
            al.max_cells = (uint32_t)(S / 2);
            hipLaunchKernelGGL(k_mesh_claim, dim3(T.mask / 256u + 1u), dim3(256), 0, s->stream, T, ma, al, L, per_cell == least ? 1 : 0);
            launches++;
            if ((rc = read_tally())) return rc;
            if (!h()[MESH_LAT + SIMP_ERR]) return SM_OK;
            if (per_cell >= most) { g_err = std::string(who) + ": internal: the lattice table filled at its bound"; return SM_E_HIP; }
        }
    }
    void field_and_cubes()
    {
        const dim3 grid(L.mask / 256u + 1u);
        hipLaunchKernelGGL(k_mesh_field, grid, dim3(256), 0, s->stream, a, ma, T, (const unsigned long long *)cmin, L);
        hipLaunchKernelGGL(k_mesh_cubes, grid, dim3(256), 0, s->stream, L);
        launches += 2;
    }
    // the owners among `points` lattice points listed; the tally read
    int owners(uint32_t points)
    {
        int rc;
        if ((rc = dalloc(d_key[0], points)) || (rc = dalloc(d_key[1], points)) || (rc = dalloc(d_idx[0], points)) || (rc = dalloc(d_idx[1], points)) ||
            (rc = dalloc(d_hist, pair_sort_hist_words(points))))
            return rc;
        hipLaunchKernelGGL(k_mesh_owners, dim3(L.mask / MESH_OWNERS_BLOCK + 1u), dim3(256), 0, s->stream, L, points, d_key[0].get(), d_idx[0].get());
        launches++;
        return read_tally();
    }
    // m owners sorted by key and ranked: vbase and fbase of each; the tally read
    int rank(uint32_t m)
    {
        int rc, which = 0;
        unsigned long long bits[2];
        memcpy(bits, h() + MESH_OR, 16);
        unsigned long long *const key[2] = {d_key[0].get(), d_key[1].get()};
        uint32_t *const idx[2] = {d_idx[0].get(), d_idx[1].get()};
        uint32_t passes = 0;
        if ((rc = pair_sort(s, key, idx, d_hist.get(), m, bits[0] ^ bits[1], which, launches, passes))) return rc;
        const uint32_t *sorted = d_idx[which].get();
        for (uint32_t first = 0; first < m; first += CHUNK) {                        // (a plane of block counts holds a chunk's)
            const uint32_t n = std::min(CHUNK, m - first), nblk = (n + 255) / 256;
            hipLaunchKernelGGL(k_mesh_count, dim3(nblk), dim3(256), 0, s->stream, L, sorted, first, n, out.blk_cnt(0), out.blk_cnt(1));
            launches++;
            out.scan(nblk, tally() + MESH_VRUN, -1, launches, 0);
            out.scan(nblk, tally() + MESH_FRUN, -1, launches, 1);
            hipLaunchKernelGGL(k_mesh_base, dim3(nblk), dim3(256), 0, s->stream, L, sorted, first, n, out.blk_base(0), out.blk_base(1));
            launches++;
        }
        return read_tally();
    }
    int emit(uint32_t nv, uint32_t nf)
    {
        int rc;
        if ((rc = dalloc(d_vert, nv)) || (rc = dalloc(d_faces, (size_t)nf * 3))) return rc;
        const dim3 grid(L.mask / 256u + 1u);
        if (nv) { hipLaunchKernelGGL(k_mesh_vertices, grid, dim3(256), 0, s->stream, a, L, nv, d_vert.get()); launches++; }
        if (nf) { hipLaunchKernelGGL(k_mesh_faces, grid, dim3(256), 0, s->stream, L, nf, d_faces.get()); launches++; }
        HIPCK(hipGetLastError());
        return SM_OK;
    }
};

}  // namespace

extern "C" {

int sm_default_mesh_params(sm_mesh_params *p)
{
    if (!p) { g_err = "sm_default_mesh_params: null argument"; return SM_E_ARG; }
    *p = sm_mesh_params{};
    p->voxel_mm = 100;
    p->reach = 2;
    p->min_records = 1;
    for (uint32_t &w : p->class_mask) w = 0xFFFFFFFFu;
    p->max_cells = 1u << 24;
    return SM_OK;
}

int sm_mesh_maps(sm_ctx *s, const sm_map_source *src, const sm_mesh_params *p, sm_mesh_vertex *vertices, uint32_t vcap, uint32_t *faces, uint32_t fcap,
                 const char *ply_path, sm_mesh_info *info)
{
    const char *who = "sm_mesh_maps";
    SetCall call(s, src, who);
    if (!s || !src || !p || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (!vertices && vcap) { g_err = std::string(who) + ": no vertices to hold vcap = " + std::to_string(vcap) + " rows"; return SM_E_ARG; }
    if (!faces && fcap) { g_err = std::string(who) + ": no faces to hold fcap = " + std::to_string(fcap) + " rows"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&] { return check_params(p, who); }, {ply_path}))) return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;
    const uint64_t total = call.total;

    Mesh &me = s->mesh;
    sm_mesh_info got{};
    got.records = total;

    MeshJob job(s, who, *p);
    sm_mesh_stats_t &st = job.stats;
    const Event *ev = job.ev;
    if ((rc = job.open(total)) || (rc = call.model())) return rc;
    const float4 *d_model = call.d_model;
    if ((rc = call.staging())) return rc;                // (the mesh leaves through the staging's host buffers)

    // ---- the reading: the cells
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, {&st.read_ms, &call.copy_ms, &st.table_ms}, ev[EV_INS0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.insert(d_rec, n, gid0); })))
        return rc;
    if ((rc = mark(s, ev[EV_INS1])) || (rc = job.read_tally())) return rc;
    if ((rc = add_marked(&ev[EV_CLR0], &st.table_ms)) || (rc = add_marked(&ev[EV_INS0], &st.table_ms))) return rc;
    const uint32_t *h = job.h();
    // (nothing has been written: rows, file and info follow)
    if ((rc = voxel_check_tally(h + MESH_CELL, p->max_cells, who, "cells"))) return rc;
    for (int k = 0; k < MESH_KINDS; ++k) got.counts[k] = h[MESH_COUNTS + k];
    const uint32_t table_cells = h[MESH_CELL + SIMP_CELLS];

    // ---- lattice points, field, cubes, owners; then the sort and the ranks
    uint32_t owners = 0;
    if (table_cells) {
        if ((rc = mark(s, ev[EV_FIELD0])) || (rc = job.claim(table_cells))) return rc;
        got.cells = h[MESH_EXIST];
        got.lattice_points = h[MESH_LAT + SIMP_CELLS];
        if (got.lattice_points) {
            job.field_and_cubes();
            if ((rc = mark(s, ev[EV_FIELD1])) || (rc = mark(s, ev[EV_SORT0])) || (rc = job.owners(got.lattice_points))) return rc;
            if ((rc = add_marked(&ev[EV_FIELD0], &st.field_ms))) return rc;
            got.cubes = h[MESH_CUBES];
            owners = h[MESH_OWNERS];
            if (owners > got.lattice_points) { g_err = std::string(who) + ": internal: more owners than lattice points"; return SM_E_HIP; }
            if (owners && (rc = job.rank(owners))) return rc;
            if ((rc = mark(s, ev[EV_SORT1])) || (rc = add_marked(&ev[EV_SORT0], &st.sort_ms))) return rc;
        }
    }
    unsigned long long totals[2];
    memcpy(totals, h + MESH_VTOTAL, 16);
    if (totals[0] > 0xFFFFFFFFull || totals[1] > 0xFFFFFFFFull) {
        g_err = std::string(who) + ": the mesh would have " + std::to_string(totals[0]) + " vertices and " + std::to_string(totals[1]) + " faces, more than 2^32 - 1";
        return SM_E_CAPACITY;
    }
    got.vertices = (uint32_t)totals[0];
    got.faces = (uint32_t)totals[1];
    if (got.vertices != h[MESH_VRUN + SIMP_RUN] || got.faces != h[MESH_FRUN + SIMP_RUN]) { g_err = std::string(who) + ": internal: totals and ranks differ"; return SM_E_HIP; }

    // ---- the emit; the rows come back while the host fills the buffers and the file
    if (got.vertices || got.faces) {
        if ((rc = mark(s, ev[EV_EMIT0])) || (rc = job.emit(got.vertices, got.faces)) || (rc = mark(s, ev[EV_EMIT1]))) return rc;
    }
    PlyFile ply(who);
    if (ply_path) {                                      // (the file's opening and its close count as writing)
        const double t0 = now_ms();
        rc = ply.open(ply_path, got.vertices, got.faces);
        st.write_ms += (float)(now_ms() - t0);
        if (rc) return rc;
    }
    if (got.vertices && (vcap || ply_path)) {
        rc = drain(s, job.d_vert.get(), got.vertices, sizeof(MeshVertex), &ev[EV_PIECE], &st.write_ms, true,
                   [&](int, const void *rows, size_t first, size_t m) -> int {
                       if (first < vcap) memcpy(vertices + first, rows, std::min<size_t>(m, vcap - first) * sizeof(sm_mesh_vertex));
                       return ply_path ? ply.vertices((const sm_mesh_vertex *)rows, m) : SM_OK;
                   });
        if (rc) return rc;
    }
    if (got.faces && (fcap || ply_path)) {
        rc = drain(s, job.d_faces.get(), got.faces, 12, &ev[EV_PIECE], &st.write_ms, true,
                   [&](int, const void *rows, size_t first, size_t m) -> int {
                       if (first < fcap) memcpy(faces + first * 3, rows, std::min<size_t>(m, fcap - first) * 12);
                       return ply_path ? ply.faces((const uint32_t *)rows, m) : SM_OK;
                   });
        if (rc) return rc;
    }
    HIPCK(hipStreamSynchronize(s->stream));
    if ((got.vertices || got.faces) && (rc = add_marked(&ev[EV_EMIT0], &st.emit_ms))) return rc;
    if (ply_path) {
        const double t0 = now_ms();
        rc = ply.commit();
        st.write_ms += (float)(now_ms() - t0);
        if (rc) return rc;
    }
    *info = got;
    st.launches = job.launches;
    st.total_ms = call.elapsed_ms();
    me.stats = st;                                       // (a call that fails leaves the last one's)
    me.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_mesh_stats, sm_mesh_stats_t, mesh, "sm_mesh_maps")

}  // extern "C"
