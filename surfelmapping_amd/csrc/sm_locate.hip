// sm_locate.hip -- one map set located in another without a guess (sm_locate_maps; DESIGN.md "4ab. Locating"): each set streamed
// once into top-down rasters, the source's compacted into its cell lists, the target's into occ and its max-pyramid; the coarse
// winner and the runner-up by a best-first branch and bound whose nodes the device scores in rounds and whose frontier the host
// keeps; the refinement and the height pairs by one small launch each.  Kernels: sm_k_locate.h; the call's frame: sm_set_call.h.
// Everything but the tally and the events is allocated per call and freed when it ends.
#include "sm_set_call.h"
#include "sm_k_locate.h"
#include "sm_pose.h"

#include <queue>

using namespace sm;
using sm_mapfile::now_ms;

namespace {

enum { EV_CLR0 = 0, EV_CLR1, EV_TGT0, EV_TGT1, EV_SRC0, EV_SRC1, EV_PYR0, EV_PYR1, N_EV };
static_assert(N_EV == decltype(Locate::scratch)::N_EV, "the context holds the events of a call");
static_assert(LOCATE_K_STRUCTURE == SM_LOCATE_STRUCTURE && LOCATE_K_LOOSE == SM_LOCATE_LOOSE, "the kinds are the header's");
constexpr uint32_t LOCATE_ROUND_NODES = 1u << 14;        // nodes scored per round at most (max_nodes may lower it)
constexpr uint32_t LOCATE_FIRST_PARENTS = 64;            // nodes the first round takes from the frontier; every later one four times as many
constexpr size_t LOCATE_ROUND_BYTES = (size_t)LOCATE_ROUND_NODES * (sizeof(LocateNode) + 8);
constexpr uint64_t LOCATE_EXHAUSTIVE_MAX = 1ull << 36;

int q16(int64_t mm) { return (int)((mm * 65536 + 500) / 1000); }

int check_params(const sm_locate_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->cell_mm < 50 || p->cell_mm > 4000) return bad("cell_mm outside 50..4000");
    if (p->up < 0 || p->up > 5) return bad("up outside 0..5");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k]) || !std::isfinite(p->source_origin[k])) return bad("non-finite origin or source_origin");
    if (p->nu < 1 || p->nu > 4096) return bad("nu outside 1..4096");
    if (p->nv < 1 || p->nv > 4096) return bad("nv outside 1..4096");
    if (p->max_up < 0 || p->max_up > 16384) return bad("max_up outside 0..16384");
    if (p->min_up < 0 || p->min_up > 16384) return bad("min_up outside 0..16384");
    if (p->normal_sign != 1 && p->normal_sign != -1) return bad("normal_sign is +1 or -1");
    if (p->min_records == 0) return bad("min_records is 0");
    if (p->dilate < 0 || p->dilate > 2) return bad("dilate outside 0..2");
    if (p->n_yaw < 1 || p->n_yaw > 1024) return bad("n_yaw outside 1..1024");
    if (p->refine < 1 || p->refine > 16) return bad("refine outside 1..16");
    if (p->sep_yaw < 0) return bad("sep_yaw is negative");
    if (p->min_ground < 0) return bad("min_ground is negative");
    if (p->min_overlap_256 < 0 || p->min_overlap_256 > 256) return bad("min_overlap_256 outside 0..256");
    if (p->ambiguity_256 < 0 || p->ambiguity_256 > 65536) return bad("ambiguity_256 outside 0..65536");
    if (p->max_source_cells < 1 || p->max_source_cells > (1u << 20)) return bad("max_source_cells outside 1..2^20");
    if (p->max_nodes < 4 || p->max_nodes > (1u << 24)) return bad("max_nodes outside 4..2^24");
    return SM_OK;
}

LocateArgs locate_args(const sm_locate_params &p)
{
    LocateArgs g{};
    g.C = q16(p.cell_mm);
    for (int k = 0; k < 3; ++k) { g.origin[0][k] = p.origin[k]; g.origin[1][k] = p.source_origin[k]; }
    g.a = p.up >> 1;
    g.sgn = (p.up & 1) ? -1 : 1;
    g.nsgn = g.sgn * p.normal_sign;
    g.ua = g.a == 0 ? 1 : 0;
    g.va = g.a == 2 ? 1 : 2;
    g.nu = p.nu; g.nv = p.nv;
    g.max_up = p.max_up; g.min_up = p.min_up;
    for (int i = 0; i < 8; ++i) { g.smask[i] = p.structure_mask[i]; g.gmask[i] = p.ground_mask[i]; }
    g.min_records = p.min_records;
    g.dilate = p.dilate;
    return g;
}

void rotation_table(const sm_locate_params &p, std::vector<int32_t> &t)
{
    const int n = p.n_yaw * p.refine;
    t.resize((size_t)2 * n);
    for (int j = 0; j < n; ++j) {
        const double ang = 2.0 * 3.14159265358979323846 * (double)j / (double)n;
        t[2 * j] = (int32_t)llrint(std::cos(ang) * 1073741824.0);
        t[2 * j + 1] = (int32_t)llrint(std::sin(ang) * 1073741824.0);
    }
}

// One call's device side
struct LocateJob {
    sm_ctx *s;
    Locate &lc;
    const Event *ev;
    const sm_locate_params &p;
    LocateArgs g;
    sm_locate_stats_t stats{};
    size_t Nt;
    static constexpr size_t Ns = (size_t)LOCATE_SW * LOCATE_SW;
    static constexpr uint32_t NBLK = (uint32_t)((Ns + 255) / 256);
    Dev<uint8_t> planes;               // cnt_t, Z_t | cnt_s, Z_s
    uint32_t *cnt[2] = {nullptr, nullptr};
    int *Z[2] = {nullptr, nullptr};
    Dev<uint32_t> blk, totals, S, G, rot, d_bound, d_refine;
    Dev<int> GZ, d_table, d_height;
    Dev<uint8_t> pyr;                  // occ, then the levels above it
    Dev<LocateNode> d_nodes;
    Dev<unsigned long long> d_best;
    LocateLevels lv{};
    int top = 0;                       // the roots' level
    uint32_t n_s = 0, n_g = 0, cap = 0;
    int R = 0;
    std::vector<uint32_t> h_S;
    std::vector<int32_t> table;

    LocateJob(sm_ctx *s_, const sm_locate_params &p_) : s(s_), lc(s_->locate), ev(s_->locate.scratch.ev), p(p_), g(locate_args(p_)), Nt((size_t)p_.nu * p_.nv) {}
    uint32_t *tally() const { return lc.scratch.d_tally.get(); }

    int open()
    {
        int rc;
        if ((rc = lc.scratch.ensure(LOCATE_TALLY_WORDS)) || (rc = dalloc(planes, (Nt + Ns) * 8)) || (rc = dalloc(blk, (size_t)2 * NBLK)) ||
            (rc = dalloc(totals, 2)))
            return rc;
        cnt[0] = (uint32_t *)planes.get(); cnt[1] = cnt[0] + Nt;
        Z[0] = (int *)(cnt[1] + Ns); Z[1] = Z[0] + Nt;
        if ((rc = mark(s, ev[EV_CLR0]))) return rc;
        HIPCK(hipMemsetAsync(cnt[0], 0, (Nt + Ns) * 4, s->stream));
        HIPCK(hipMemsetAsync(Z[0], 0x7F, (Nt + Ns) * 4, s->stream));
        if ((rc = lc.scratch.clear(s->stream))) return rc;
        return mark(s, ev[EV_CLR1]);
    }
    void raster(const float4 *d_rec, uint32_t n, int side)
    {
        if (!n) return;
        hipLaunchKernelGGL(k_locate_raster, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, g, side, cnt[side], Z[side], tally());
        stats.launches++;
        stats.chunks++;
    }
    // S and G from the source's planes; waits twice (the totals, then the cells of S)
    int compact()
    {
        int rc;
        hipLaunchKernelGGL(k_locate_count, dim3(NBLK), dim3(256), 0, s->stream, (const uint32_t *)cnt[1], (const int *)Z[1], (uint32_t)Ns, g.min_records, NBLK, blk.get());
        hipLaunchKernelGGL(k_locate_scan, dim3(1), dim3(1024), 0, s->stream, blk.get(), NBLK, totals.get());
        stats.launches += 2;
        uint32_t tot[2];
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(tot, totals.get(), 8, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        n_s = tot[0]; n_g = tot[1];
        if (n_s > p.max_source_cells) {
            g_err = "sm_locate_maps: the source has " + std::to_string(n_s) + " occupied cells, more than max_source_cells = " + std::to_string(p.max_source_cells);
            return SM_E_CAPACITY;
        }
        if ((rc = dalloc(S, n_s)) || (rc = dalloc(G, n_g)) || (rc = dalloc(GZ, n_g))) return rc;
        hipLaunchKernelGGL(k_locate_emit, dim3(NBLK), dim3(256), 0, s->stream, (const uint32_t *)cnt[1], (const int *)Z[1], (uint32_t)Ns, g.min_records, NBLK,
                           (const uint32_t *)blk.get(), S.get(), n_s, G.get(), GZ.get(), n_g);
        stats.launches++;
        HIPCK(hipGetLastError());
        h_S.resize(n_s);
        if (n_s) HIPCK(hipMemcpyAsync(h_S.data(), S.get(), (size_t)n_s * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        long long m = 0;
        for (uint32_t w : h_S) {
            const long long cu = (long long)(w & 0xFFFFu) - LOCATE_SPAN, cv = (long long)(w >> 16) - LOCATE_SPAN;
            m = std::max(m, std::max(std::llabs(cu * g.C + g.C / 2), std::llabs(cv * g.C + g.C / 2)));
        }
        R = (int)((3 * m / 2) / g.C + 2);
        stats.range = (uint32_t)R;
        return SM_OK;
    }
    int Wu() const { return g.nu + 2 * R; }
    int Wv() const { return g.nv + 2 * R; }
    // occ (level 0); with `levels` the pyramid above it up to the roots' level
    int pyramid(bool levels)
    {
        int rc;
        top = LOCATE_LEAF;
        while (top < LOCATE_MAX_LEVELS - 1 && (1 << top) < std::max(Wu(), Wv())) ++top;
        size_t bytes = 0, at[LOCATE_MAX_LEVELS];
        const int n_lv = levels ? top + 1 : 1;
        for (int h = 0; h < n_lv; ++h) {
            LocateLevel &L = lv.l[h];
            L.off = (1 << h) - 1;
            L.W = g.nu + L.off; L.H = g.nv + L.off;
            at[h] = bytes;
            bytes += ((size_t)L.W * L.H + 255) & ~(size_t)255;
        }
        if ((rc = dalloc(pyr, bytes))) return rc;
        for (int h = 0; h < n_lv; ++h) lv.l[h].p = pyr.get() + at[h];
        hipLaunchKernelGGL(k_locate_occ, dim3((unsigned)((Nt + 255) / 256)), dim3(256), 0, s->stream, (const uint32_t *)cnt[0], g.nu, g.nv, g.min_records, g.dilate,
                           pyr.get(), tally());
        stats.launches++;
        for (int h = 1; h < n_lv; ++h) {
            const size_t n = (size_t)lv.l[h].W * lv.l[h].H;
            hipLaunchKernelGGL(k_locate_pyramid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, lv.l[h - 1], lv.l[h], pyr.get() + at[h], 1 << (h - 1));
            stats.launches++;
        }
        stats.levels = (uint32_t)(n_lv - 1);
        HIPCK(hipGetLastError());
        return SM_OK;
    }
    // the table on the device, the rotated lists of the coarse rows, the rounds' buffers
    int prepare()
    {
        int rc;
        rotation_table(p, table);
        cap = std::min(p.max_nodes, LOCATE_ROUND_NODES);
        if (!lc.h_round) HIPCK(hipHostMalloc((void **)lc.h_round.put(), LOCATE_ROUND_BYTES, hipHostMallocDefault));
        if ((rc = dalloc(d_table, table.size())) || (rc = dalloc(rot, (size_t)p.n_yaw * n_s)) || (rc = dalloc(d_nodes, cap)) || (rc = dalloc(d_bound, cap)) ||
            (rc = dalloc(d_best, cap)) || (rc = dalloc(d_refine, (size_t)(2 * p.refine - 1) * 9)) || (rc = dalloc(d_height, n_g)))
            return rc;
        HIPCK(hipMemcpyAsync(d_table.get(), table.data(), table.size() * 4, hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_locate_rotate, dim3((n_s + 255) / 256, p.n_yaw), dim3(256), 0, s->stream, (const uint32_t *)S.get(), n_s, (const int *)d_table.get(), p.refine,
                           g.C, rot.get());
        stats.launches++;
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s->stream));          // (the table's host copy is pageable)
        return SM_OK;
    }
    LocateSearch query(const sm_locate_info *excl) const
    {
        LocateSearch q{};
        q.rot = rot.get(); q.n_s = n_s; q.R = R; q.nu = g.nu; q.nv = g.nv; q.n_yaw = p.n_yaw;
        if (excl) { q.ex_on = 1; q.ex_k = excl->coarse_k; q.ex_du = excl->coarse_du; q.ex_dv = excl->coarse_dv; q.sep_yaw = p.sep_yaw; q.sep_cells = p.sep_cells; }
        return q;
    }

    // One round: the bounds of n inner nodes, or the best candidates of n leaf nodes, to the host through the pinned buffer
    int score_nodes(const LocateSearch &q, const std::vector<LocateNode> &nodes, size_t first, uint32_t n, bool leaves, std::vector<uint32_t> &bound,
                    std::vector<unsigned long long> &best)
    {
        LocateNode *h_nodes = (LocateNode *)lc.h_round.get();
        void *h_out = lc.h_round.get() + (size_t)LOCATE_ROUND_NODES * sizeof(LocateNode);
        memcpy(h_nodes, nodes.data() + first, (size_t)n * sizeof(LocateNode));
        HIPCK(hipMemcpyAsync(d_nodes.get(), h_nodes, (size_t)n * sizeof(LocateNode), hipMemcpyHostToDevice, s->stream));
        if (leaves) {
            hipLaunchKernelGGL(k_locate_tiles, dim3((n + 3) / 4), dim3(256), 0, s->stream, q, lv.l[0], (const LocateNode *)d_nodes.get(), n, d_best.get());
            HIPCK(hipMemcpyAsync(h_out, d_best.get(), (size_t)n * 8, hipMemcpyDeviceToHost, s->stream));
            stats.leaves += (uint64_t)n * 64;
        } else {
            hipLaunchKernelGGL(k_locate_bound, dim3((n + 3) / 4), dim3(256), 0, s->stream, q, lv, (const LocateNode *)d_nodes.get(), n, d_bound.get());
            HIPCK(hipMemcpyAsync(h_out, d_bound.get(), (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
            stats.nodes += n;
        }
        stats.launches++;
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s->stream));
        if (leaves) best.assign((const unsigned long long *)h_out, (const unsigned long long *)h_out + n);
        else bound.assign((const uint32_t *)h_out, (const uint32_t *)h_out + n);
        return SM_OK;
    }

    // The largest coarse score and, of equal ones, the smallest (k, dv, du), as score << 40 | (LOCATE_KEY_MAX - key); excl: the
    // runner-up's search, whose candidates keep away from excl's winner and of which only the score counts.  Best-first: the host
    // keeps the frontier ordered by (bound, smallest key it may hold); a round scores the children of its best nodes.
    int search(const sm_locate_info *excl, unsigned long long &result)
    {
        int rc;
        const LocateSearch q = query(excl);
        const int hi_u = g.nu - 1 + R, hi_v = g.nv - 1 + R;
        unsigned long long best = 0;
        bool any = false;
        const auto min_key = [&](const LocateNode &nd) {
            return (unsigned long long)nd.k << 30 | (unsigned long long)(nd.dv0 + R) << 15 | (unsigned long long)(nd.du0 + R);
        };
        const auto priority = [&](uint32_t bound, const LocateNode &nd) { return (unsigned long long)bound << 40 | (LOCATE_KEY_MAX - min_key(nd)); };
        // (bound, -smallest key) above (best, -best's key); the runner-up's search asks for a larger score
        const auto survives = [&](unsigned long long pri) { return !any || (excl ? (pri >> 40) > (best >> 40) : pri > best); };
        const auto dropped = [&](const LocateNode &nd) {     // wholly inside the excluded box
            if (!excl) return false;
            int dk = std::abs(nd.k - q.ex_k);
            dk = std::min(dk, q.n_yaw - dk);
            const int side = (1 << nd.h) - 1;
            return dk <= q.sep_yaw && nd.du0 >= q.ex_du - q.sep_cells && nd.du0 + side <= q.ex_du + q.sep_cells && nd.dv0 >= q.ex_dv - q.sep_cells &&
                   nd.dv0 + side <= q.ex_dv + q.sep_cells;
        };
        struct Entry { unsigned long long pri; LocateNode nd; };
        const auto below = [](const Entry &a, const Entry &b) { return a.pri < b.pri; };
        std::priority_queue<Entry, std::vector<Entry>, decltype(below)> frontier(below);
        std::vector<LocateNode> inner, leaf;
        std::vector<uint32_t> bound;
        std::vector<unsigned long long> got;
        const auto add = [&](const LocateNode &nd) {
            if (nd.du0 > hi_u || nd.dv0 > hi_v || dropped(nd)) return;
            inner.push_back(nd);
        };
        for (int k = 0; k < p.n_yaw; ++k)
            for (int dv0 = -R; dv0 <= hi_v; dv0 += 1 << top)
                for (int du0 = -R; du0 <= hi_u; du0 += 1 << top) add({k, du0, dv0, top});
        // the first rounds take few nodes, so that leaves are reached -- and the frontier is cut -- before it has grown wide
        uint32_t parents = std::min(std::max(1u, cap / 4), LOCATE_FIRST_PARENTS);
        for (;; parents = std::min(std::max(1u, cap / 4), parents * 4)) {
            // the nodes waiting for their bound, a round of at most `cap` at a time; what survives joins the frontier
            for (size_t first = 0; first < inner.size(); first += cap) {
                const uint32_t n = (uint32_t)std::min<size_t>(cap, inner.size() - first);
                if ((rc = score_nodes(q, inner, first, n, false, bound, got))) return rc;
                stats.rounds++;
                for (uint32_t i = 0; i < n; ++i) {
                    const unsigned long long pri = priority(bound[i], inner[first + i]);
                    if (survives(pri)) frontier.push({pri, inner[first + i]});
                }
            }
            inner.clear();
            leaf.clear();
            // the best nodes of the frontier: leaf nodes are scored offset by offset, the others give their four children
            uint32_t taken = 0;
            while (!frontier.empty() && taken < parents) {
                const Entry e = frontier.top();
                if (!survives(e.pri)) break;             // (nor does anything behind it)
                frontier.pop();
                ++taken;
                if (e.nd.h == LOCATE_LEAF) { leaf.push_back(e.nd); continue; }
                const int h = e.nd.h - 1, half = 1 << h;
                for (int c = 0; c < 4; ++c) add({e.nd.k, e.nd.du0 + (c & 1) * half, e.nd.dv0 + (c >> 1) * half, h});
            }
            if (!taken) break;
            if (!leaf.empty()) {
                if ((rc = score_nodes(q, leaf, 0, (uint32_t)leaf.size(), true, bound, got))) return rc;
                stats.rounds++;
                for (unsigned long long b : got)
                    if (b && (!any || b > best)) { best = b; any = true; }
            }
        }
        result = any ? best : 0ull;
        return SM_OK;
    }

    // every coarse candidate, without the pyramid
    int search_all(const sm_locate_info *excl, unsigned long long &result)
    {
        const LocateSearch q = query(excl);
        HIPCK(hipMemsetAsync(d_best.get(), 0, 8, s->stream));
        const unsigned strips = (unsigned)((Wu() + 63) / 64);
        hipLaunchKernelGGL(k_locate_all, dim3((strips + 3) / 4, (unsigned)Wv(), (unsigned)p.n_yaw), dim3(256), 0, s->stream, q, lv.l[0], d_best.get());
        stats.launches++;
        stats.rounds++;
        stats.leaves += (uint64_t)Wu() * Wv() * p.n_yaw;
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(&result, d_best.get(), 8, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        return SM_OK;
    }

    int refine(sm_locate_info &out)
    {
        const int rows = 2 * p.refine - 1, n_fine = p.n_yaw * p.refine;
        hipLaunchKernelGGL(k_locate_refine, dim3(rows), dim3(64), 0, s->stream, (const uint32_t *)S.get(), n_s, (const int *)d_table.get(), n_fine, p.refine,
                           out.coarse_k, out.coarse_du, out.coarse_dv, g.C, lv.l[0], d_refine.get());
        stats.launches++;
        HIPCK(hipGetLastError());
        std::vector<uint32_t> sc((size_t)rows * 9);
        HIPCK(hipMemcpyAsync(sc.data(), d_refine.get(), sc.size() * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        bool any = false;
        // in the order (|dj|, dj, dv, du): a later candidate needs a larger score
        for (int m = 0; m < p.refine; ++m)
            for (int dj : {-m, m}) {
                if (m == 0 && dj != 0) continue;
                if (m == 0 && any) continue;
                for (int o = 0; o < 9; ++o) {
                    const uint32_t v = sc[(size_t)(dj + p.refine - 1) * 9 + o];
                    if (any && v <= out.score) continue;
                    any = true;
                    out.score = v;
                    out.row = ((out.coarse_k * p.refine + dj) % n_fine + n_fine) % n_fine;
                    out.du = out.coarse_du + o % 3 - 1;
                    out.dv = out.coarse_dv + o / 3 - 1;
                }
            }
        return SM_OK;
    }

    int height(sm_locate_info &out)
    {
        out.height_pairs = 0;
        out.dh = 0;
        if (!n_g) return SM_OK;
        hipLaunchKernelGGL(k_locate_height, dim3((n_g + 255) / 256), dim3(256), 0, s->stream, (const uint32_t *)G.get(), (const int *)GZ.get(), n_g, table[2 * out.row],
                           table[2 * out.row + 1], out.du, out.dv, g.C, g.nu, g.nv, (const int *)Z[0], d_height.get());
        stats.launches++;
        HIPCK(hipGetLastError());
        std::vector<int> d(n_g);
        HIPCK(hipMemcpyAsync(d.data(), d_height.get(), (size_t)n_g * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        d.erase(std::remove(d.begin(), d.end(), LOCATE_NO_PAIR), d.end());
        const size_t m = d.size();
        out.height_pairs = (uint32_t)m;
        if (m && m >= (size_t)p.min_ground) {
            std::nth_element(d.begin(), d.begin() + (m - 1) / 2, d.end());
            out.dh = d[(m - 1) / 2];
        }
        return SM_OK;
    }
};

void unpack_candidate(unsigned long long b, int R, uint32_t &score, int &k, int &du, int &dv)
{
    const unsigned long long key = LOCATE_KEY_MAX - (b & LOCATE_KEY_MAX);
    score = (uint32_t)(b >> 40);
    k = (int)(key >> 30);
    dv = (int)((key >> 15) & 0x7FFFu) - R;
    du = (int)(key & 0x7FFFu) - R;
}

void locate_pose(const sm_locate_params &p, const LocateArgs &g, const std::vector<int32_t> &table, const sm_locate_info &o, float *pose16)
{
    const double c = (double)table[2 * o.row] * (1.0 / 1073741824.0), sn = (double)table[2 * o.row + 1] * (1.0 / 1073741824.0);
    const double Cm = (double)g.C * (1.0 / 65536.0);
    double O[3], So[3], M[4][4] = {};
    for (int k = 0; k < 3; ++k) { O[k] = (double)p.origin[k]; So[k] = (double)p.source_origin[k]; }
    const int a = g.a, ua = g.ua, va = g.va;
    M[3][3] = 1.0;
    M[ua][ua] = c; M[ua][va] = -sn; M[va][ua] = sn; M[va][va] = c; M[a][a] = 1.0;
    M[ua][3] = (O[ua] + (double)o.du * Cm) - (c * So[ua] - sn * So[va]);
    M[va][3] = (O[va] + (double)o.dv * Cm) - (sn * So[ua] + c * So[va]);
    M[a][3] = (O[a] + (double)(g.sgn * (long long)o.dh) * (1.0 / 65536.0)) - So[a];
    for (int col = 0; col < 4; ++col)
        for (int row = 0; row < 4; ++row) pose16[col * 4 + row] = (float)M[row][col];
}

}  // namespace

extern "C" {

int sm_default_locate_params(sm_locate_params *p)
{
    if (!p) { g_err = "sm_default_locate_params: null argument"; return SM_E_ARG; }
    *p = sm_locate_params{};
    p->cell_mm = 500;
    p->up = 3;
    p->nu = p->nv = 256;
    for (uint32_t &w : p->structure_mask) w = 0xFFFFFFFFu;
    for (uint32_t &w : p->ground_mask) w = 0xFFFFFFFFu;
    p->max_up = 8192;
    p->min_up = 11585;
    p->normal_sign = -1;
    p->min_records = 2;
    p->dilate = 1;
    p->n_yaw = 360;
    p->refine = 8;
    p->sep_yaw = 10;
    p->sep_cells = 8;
    p->min_ground = 16;
    p->min_overlap_256 = 128;
    p->ambiguity_256 = 218;
    p->max_source_cells = 1u << 18;
    p->max_nodes = 1u << 20;
    return SM_OK;
}

int sm_locate_rotations(const sm_locate_params *p, int32_t *table)
{
    const char *who = "sm_locate_rotations";
    if (!p || !table) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (int rc = check_params(p, who)) return rc;
    std::vector<int32_t> t;
    rotation_table(*p, t);
    memcpy(table, t.data(), t.size() * 4);
    return SM_OK;
}

int sm_locate_maps(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const sm_locate_params *p, float *pose16_out, sm_locate_info *info)
{
    const char *who = "sm_locate_maps";
    const double t_begin = now_ms();
    if (!s || !source || !target || !p || !pose16_out || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, who)) || (rc = check_not_mid_cull(s, who))) return rc;
    sm_mapset::ReadSet sset, tset;
    if ((rc = check_sets(source, target, who)) || (rc = open_sets(source, target, who, sset, tset))) return rc;
    const sm_map_source *const srcs[2] = {source, target};
    const sm_mapset::ReadSet *const sets[2] = {&sset, &tset};
    uint32_t live[2];
    if ((rc = maps_counts(s, who, 2, srcs, sets, live))) return rc;
    const uint32_t scnt = live[0], tcnt = live[1];
    const uint64_t stotal = sset.file_total + scnt, ttotal = tset.file_total + tcnt;
    const bool exhaustive = env_is_one("SM_LOCATE_EXHAUSTIVE");

    LocateJob job(s, *p);
    sm_locate_stats_t &st = job.stats;
    st.source_records = stotal;
    st.target_records = ttotal;
    st.exhaustive = exhaustive ? 1u : 0u;
    Locate &lc = s->locate;
    const Event *ev = job.ev;
    if ((rc = job.open())) return rc;
    const float4 *d_model;
    if ((rc = maps_export(s, std::max(scnt, tcnt), d_model))) return rc;
    if (sset.jobs.size() + tset.jobs.size())
        if ((rc = maps_ensure_staging(s))) return rc;
    float copy_ms = 0.0f;
    const MapStream::Tally times = {&st.read_ms, &copy_ms, &st.raster_ms};

    // ---- one reading per set
    if ((rc = maps_feed(s, who, tset, target->paths, tcnt, d_model, times, ev[EV_TGT0], [&](const float4 *d_rec, uint32_t n, uint32_t) { job.raster(d_rec, n, 0); })))
        return rc;
    if ((rc = mark(s, ev[EV_TGT1]))) return rc;
    if ((rc = maps_feed(s, who, sset, source->paths, scnt, d_model, times, ev[EV_SRC0], [&](const float4 *d_rec, uint32_t n, uint32_t) { job.raster(d_rec, n, 1); })))
        return rc;
    if ((rc = job.compact())) return rc;
    if ((rc = mark(s, ev[EV_SRC1])) || (rc = mark(s, ev[EV_PYR0])) || (rc = job.pyramid(!exhaustive)) || (rc = mark(s, ev[EV_PYR1])) || (rc = lc.scratch.read(s))) return rc;
    for (int pair : {EV_CLR0, EV_TGT0, EV_SRC0})
        if ((rc = add_marked(&ev[pair], &st.raster_ms))) return rc;
    if ((rc = add_marked(&ev[EV_PYR0], &st.pyramid_ms))) return rc;

    const uint32_t *h = lc.scratch.h();
    sm_locate_info out{};
    uint64_t seen[2] = {0, 0};
    for (int k = 0; k < LOCATE_KINDS; ++k) {
        out.target_counts[k] = h[LOCATE_COUNTS + k];
        out.source_counts[k] = h[LOCATE_COUNTS + 8 + k];
        seen[0] += out.target_counts[k];
        seen[1] += out.source_counts[k];
    }
    if (seen[0] != ttotal || seen[1] != stotal) { g_err = std::string(who) + ": a set changed while it was read"; return SM_E_ARG; }
    out.n_s = job.n_s;
    out.target_cells = h[LOCATE_OCC];
    out.status = out.target_cells == 0 ? SM_LOCATE_NO_TARGET : out.n_s == 0 ? SM_LOCATE_NO_SOURCE : SM_LOCATE_OK;

    if (out.status == SM_LOCATE_OK) {
        if (exhaustive && (uint64_t)p->n_yaw * (uint64_t)job.Wu() * (uint64_t)job.Wv() > LOCATE_EXHAUSTIVE_MAX / job.n_s) {
            g_err = std::string(who) + ": SM_LOCATE_EXHAUSTIVE=1 would need more than 2^36 lookups";
            return SM_E_ARG;
        }
        const double t_search = now_ms();
        if ((rc = job.prepare())) return rc;
        unsigned long long best = 0, second = 0;
        if ((rc = exhaustive ? job.search_all(nullptr, best) : job.search(nullptr, best))) return rc;
        unpack_candidate(best, job.R, out.coarse_score, out.coarse_k, out.coarse_du, out.coarse_dv);
        if (p->sep_cells >= 0) {
            if ((rc = exhaustive ? job.search_all(&out, second) : job.search(&out, second))) return rc;
            out.runner_up = (uint32_t)(second >> 40);
        }
        if ((rc = job.refine(out)) || (rc = job.height(out))) return rc;
        if ((uint64_t)out.score * 256 < (uint64_t)out.n_s * (uint64_t)p->min_overlap_256) out.status = SM_LOCATE_NONE;
        else if ((uint64_t)out.runner_up * 256 > (uint64_t)out.coarse_score * (uint64_t)p->ambiguity_256) out.status = SM_LOCATE_AMBIGUOUS;
        st.search_ms = (float)(now_ms() - t_search);
    }
    if (out.status == SM_LOCATE_OK || out.status == SM_LOCATE_AMBIGUOUS) locate_pose(*p, job.g, job.table, out, pose16_out);
    else sm_pose::identity(pose16_out);
    *info = out;
    st.total_ms = (float)(now_ms() - t_begin);
    lc.stats = st;                                       // (a call that fails leaves the last one's)
    lc.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_locate_stats, sm_locate_stats_t, locate, "sm_locate_maps")

}  // extern "C"
