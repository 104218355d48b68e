// tile_sort_yardstick.hip -- the yardstick of the tiling's radix sort (DESIGN.md "4s. Spatial tiling"; tools/tile_probe.py runs it):
// rocprim::radix_sort_pairs on the same (u64 key, u32 index) pairs, bits 0..50, median of 3 after 1 warm-up, by HIP events.  rocPRIM
// is header-only and used here alone: it is never linked into the library.
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/tile_sort_yardstick tools/tile_sort_yardstick.hip    (tile_probe.py does if it is missing)
// Run:   tools/tile_sort_yardstick keys.bin        (keys.bin: n little-endian u64)
#include <hip/hip_runtime.h>
#include <cstring>                                       // (a rocPRIM header calls memset without including it)
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: tile_sort_yardstick keys.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "%s is not open\n", argv[1]); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<uint64_t> keys(n);
    if (fread(keys.data(), 8, n, f) != n) return 1;
    fclose(f);
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    uint64_t *k_in, *k_out;
    uint32_t *v_in, *v_out;
    CK(hipMalloc(&k_in, n * 8 + 8)); CK(hipMalloc(&k_out, n * 8 + 8));
    CK(hipMalloc(&v_in, n * 4 + 4)); CK(hipMalloc(&v_out, n * 4 + 4));
    CK(hipMemcpy(k_in, keys.data(), n * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(v_in, idx.data(), n * 4, hipMemcpyHostToDevice));
    size_t tmp_bytes = 0;
    CK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, n, 0, 51));
    void *tmp;
    CK(hipMalloc(&tmp, tmp_bytes + 8));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 4; ++rep) {
        CK(hipEventRecord(e0));
        CK(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, v_out, n, 0, 51));
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (rep) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    // the result, checked on the host: ascending keys, ties in index order
    std::vector<uint32_t> got(n);
    CK(hipMemcpy(got.data(), v_out, n * 4, hipMemcpyDeviceToHost));
    bool ok = true;
    for (size_t i = 1; i < n && ok; ++i)
        ok = keys[got[i - 1]] < keys[got[i]] || (keys[got[i - 1]] == keys[got[i]] && got[i - 1] < got[i]);
    printf("rocprim radix_sort_pairs n %zu ms %.4f sorted_and_stable %d\n", n, ms[1], ok ? 1 : 0);
    return ok ? 0 : 1;
}
