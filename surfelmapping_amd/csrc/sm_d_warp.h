// sm_d_warp.h -- the row rule of sm_warp_by_time as a device function, shared by the warp's kernels (sm_k_warp.h) and the
// scenes' (sm_k_scene.h), so that a record placed in a lane has the bits the warp would have written to its file.  No kernels here.
#pragma once

#include "sm_device.h"

namespace sm {

// centre and normal under table row c = (c0 | c1 | c2), each (R row, t); confidence and radius pass through
__device__ __forceinline__ void warp_apply(const float4 &c0, const float4 &c1, const float4 &c2, float4 &pc, float4 &nr)
{
    const float x = pc.x, y = pc.y, z = pc.z, nx = nr.x, ny = nr.y, nz = nr.z;
    pc.x = ((c0.x * x + c0.y * y) + c0.z * z) + c0.w;
    pc.y = ((c1.x * x + c1.y * y) + c1.z * z) + c1.w;
    pc.z = ((c2.x * x + c2.y * y) + c2.z * z) + c2.w;
    nr.x = (c0.x * nx + c0.y * ny) + c0.z * nz;
    nr.y = (c1.x * nx + c1.y * ny) + c1.z * nz;
    nr.z = (c2.x * nx + c2.y * ny) + c2.z * nz;
}

}  // namespace sm
