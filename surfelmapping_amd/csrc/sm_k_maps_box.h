// sm_k_maps_box.h -- what the kernels over chunks of map-file records share (sm_k_render_maps.h, sm_k_lidar.h): the chunk's SoA
// planes and the one box per 256 records that k_maps_intake (sm_k_render_maps.h) writes.  Device functions only, no kernel.
#pragma once

#include "sm_device.h"

namespace sm {

// a chunk's planes (or the live model's: the resolve reads either)
struct MapsSoA {
    float4 *pos_conf, *norm_rad;
    uint32_t *color;
    float *time;
};

constexpr int MAPS_BLOCK = 256;          // records per box = per workgroup of the splat

// One box per block of 256 records: box[2b] = (min x, min y, min z, rmax), box[2b + 1] = (max x, max y, max z, rnorm);
// rmax = the largest |radius|, rnorm = the largest |radius| * max(1, |normal|) (the model view draws with the stored normal as
// it is, see maps_reach_view).  A block with a record whose centre, radius or normal is not finite has rnorm = +inf -- a box
// with a non-finite member is never skipped.
struct MapsBox { float lx, ly, lz, rmax, hx, hy, hz, rnorm; };

__device__ __forceinline__ MapsBox maps_box_load(const float4 *__restrict__ box, uint32_t b)
{
    const float4 lo = box[2 * (size_t)b], hi = box[2 * (size_t)b + 1];
    return {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

__device__ __forceinline__ bool maps_box_finite(const MapsBox &b)
{
    const float t = ((b.lx - b.lx) + (b.ly - b.ly)) + ((b.lz - b.lz) + (b.hx - b.hx)) + ((b.hy - b.hy) + (b.hz - b.hz)) + ((b.rmax - b.rmax) + (b.rnorm - b.rnorm));
    return t == 0.0f;                                    // x - x is 0 for a finite x, NaN otherwise
}

}  // namespace sm
