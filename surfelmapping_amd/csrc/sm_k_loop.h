// sm_k_loop.h -- closing loops unasked (DESIGN.md "4i. Closing loops unasked"): the per-frame census of old surfels in view.
// Included by sm_track.hip only, after sm_k_track.h.
//
//   k_loop_census         how many live surfels with m[7] <= max_time pass k_track_splat's gates at a given pose: one alive word
//                         per 64 slots, one time per slot, a position only where the lane is old; one ballot per 64 slots, the
//                         count kept in a register, one atomic per wave at the end.

#pragma once

#include "sm_k_track.h"

namespace sm {

constexpr int LOOP_CENSUS_GRID = 2048;   // 256 CUs x 8 workgroups of 256: every wave walks its share of the alive words

// tp.tinv_prev holds the inverse of the pose the census is taken at.  Wave w of the grid takes alive words 4w .. 4w + 3, then those
// 4 * waves further on, ...: the loop bound is the same for all 64 lanes, so every ballot sees the whole wave.  The four times of
// a step are loaded unconditionally, at indices clamped into the occupied range, and tested without a branch, so that the four
// loads are issued back to back and waited for with a counted wait each (in the gfx950 listing: four global_load_dword, then
// s_waitcnt vmcnt(3) .. vmcnt(0)); what a clamped index read is discarded by the range test.  The alive words are scalar loads
// issued while those are in flight.  A position is loaded under the exec mask of its old lanes as soon as that mask is known,
// behind the time loads still outstanding; the compiler waits for the first three before it issues the fourth.
__global__ __launch_bounds__(256) void k_loop_census(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ alive,
                                                     TrackParams tp, float max_time, uint32_t *__restrict__ n)
{
    const uint32_t count = st->count;
    if (count == 0u) return;
    const SurfelSet cur = M.s[st->cur];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t words = (count + 63u) >> 6;
    const uint32_t step = gridDim.x * 16u;                    // 4 waves per workgroup, 4 words per wave
    uint32_t total = 0u;                                      // the same in every lane of the wave
    for (uint32_t w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u); w0 < words; w0 += step) {
        uint64_t a[4];
        float t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = alive[min(w0 + (uint32_t)j, words - 1u)];          // (wave-uniform: scalar loads)
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = cur.time[min(((w0 + (uint32_t)j) << 6) + lane, count - 1u)];
        bool old[4];
        float4 pc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = ((w0 + (uint32_t)j) << 6) + lane;
            // (bitwise, not short-circuit: no branch may come between the loads above and their use)
            old[j] = ((uint32_t)(k < count) & (uint32_t)((a[j] >> lane) & 1ull) & (uint32_t)(t[j] <= max_time)) != 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pc[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (old[j]) pc[j] = cur.pos_conf[((w0 + (uint32_t)j) << 6) + lane];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool hit = false;
            if (old[j]) {
                const float3 c = xform3(tp.tinv_prev, pc[j].x, pc[j].y, pc[j].z);
                if (c.z > tp.near_clip && c.z < tp.far_clip) {
                    const float fu = floorf(((tp.fx * c.x) / c.z + tp.cx) + 0.5f);
                    const float fv = floorf(((tp.fy * c.y) / c.z + tp.cy) + 0.5f);
                    hit = fu >= 0.0f && fu < (float)tp.W && fv >= 0.0f && fv < (float)tp.H;
                }
            }
            total += (uint32_t)__popcll(__ballot(hit));
        }
    }
    if (lane == 0u && total) atomicAdd(n, total);
}

}  // namespace sm
