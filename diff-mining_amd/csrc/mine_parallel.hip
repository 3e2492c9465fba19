// mine_parallel.hip — the two kernels that `Cluster.df_PD` (parallel-dataset/cluster.py:224-251) needs around mine.hip's selection:
//   dm = np.median(np.stack([ds[c] for c in self.countries], axis=0), axis=0)      (:231)  -> median_maps_kernel
//   ... + tuple([ds[c][i, j] for c in self.countries]) ...                         (:233)  -> gather_sets_kernel, at the winners only
// A parallel group is n_sets pooled maps of one size; "set" = country.  The selection itself is mine_select_kernel, unchanged,
// run on the median maps.
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

namespace dm {

namespace {

constexpr int kMedianThreads = 256;

// Compare-exchange without fminf / fmaxf (they drop NaNs; a NaN here leaves the pair as it is and the caller reports NaN).
// +0 and -0 compare equal and keep their places.
__device__ __forceinline__ void cswap(float& a, float& b) {
    const float lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo; b = hi;
}

// One thread per candidate, the group on blockIdx.y.  The C values are read from C streams (coalesced across candidates) into
// v[0..C), every index a compile-time constant after unrolling, so v lives in registers; an odd-even transposition network of
// C rounds sorts it (C(C-1)/2 compare-exchanges: 45 for 10 sets — the kernel is bound by its C loads per output).
//   odd C:  s[C/2];  even C: (s[C/2-1] + s[C/2]) * 0.5f  (== np.mean of the two in fp32);  any NaN among the C -> NaN.
template <int C>
__global__ __launch_bounds__(kMedianThreads)
void median_maps_kernel(const float* __restrict__ maps, const dm_mine_desc* __restrict__ desc,
                        const dm_mine_desc* __restrict__ group_desc, int kx, int ky, float* __restrict__ median) {
    const int g = blockIdx.y;
    const dm_mine_desc gd = group_desc[g];
    const int n = (gd.H - kx + 1) * (gd.W - ky + 1);
    const int p = blockIdx.x * kMedianThreads + threadIdx.x;
    if (p >= n) return;
    float v[C];
    bool has_nan = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        v[c] = maps[desc[(size_t)g * C + c].map_offset + p];
        has_nan |= v[c] != v[c];
    }
#pragma unroll
    for (int r = 0; r < C; ++r) {
#pragma unroll
        for (int i = r & 1; i + 1 < C; i += 2) cswap(v[i], v[i + 1]);
    }
    float m;
    if constexpr (C & 1) m = v[C / 2];
    else m = (v[C / 2 - 1] + v[C / 2]) * 0.5f;
    median[gd.map_offset + p] = has_nan ? __uint_as_float(0x7FC00000u) : m;
}

template <int C>
void launch_median_c(const float* maps, const dm_mine_desc* desc, const dm_mine_desc* group_desc, int n_groups, int kx, int ky,
                     int max_n, float* median, hipStream_t s) {
    hipLaunchKernelGGL(median_maps_kernel<C>, dim3((max_n + kMedianThreads - 1) / kMedianThreads, n_groups), dim3(kMedianThreads), 0, s,
                       maps, desc, group_desc, kx, ky, median);
}

// One workgroup per group, one thread per (winner r, set c): set_d[g][r][c] = set c's map at winner r's (i, j); NaN past count[g].
__global__ void gather_sets_kernel(const float* __restrict__ maps, const dm_mine_desc* __restrict__ desc, int n_sets, int ky,
                                   int k_per_image, const int32_t* __restrict__ boxes, const int32_t* __restrict__ count,
                                   float* __restrict__ set_d) {
    const int g = blockIdx.x, taken = count[g];
    for (int t = threadIdx.x; t < k_per_image * n_sets; t += blockDim.x) {
        const int r = t / n_sets, c = t - r * n_sets;
        float v = __uint_as_float(0x7FC00000u);
        if (r < taken) {
            const dm_mine_desc d = desc[(size_t)g * n_sets + c];
            const int32_t* b = boxes + ((size_t)g * k_per_image + r) * 4;
            v = maps[d.map_offset + (size_t)b[0] * (d.W - ky + 1) + b[1]];
        }
        set_d[((size_t)g * k_per_image + r) * n_sets + c] = v;
    }
}

}  // namespace

hipError_t launch_median_maps(const float* maps, const dm_mine_desc* desc, const dm_mine_desc* group_desc, int n_groups, int n_sets,
                              int kx, int ky, int max_n, float* median, hipStream_t s) {
    if (n_groups < 1 || max_n < 1) return hipErrorInvalidValue;
    switch (n_sets) {
#define DM_MEDIAN_CASE(C) case C: launch_median_c<C>(maps, desc, group_desc, n_groups, kx, ky, max_n, median, s); break;
        DM_MEDIAN_CASE(1) DM_MEDIAN_CASE(2) DM_MEDIAN_CASE(3) DM_MEDIAN_CASE(4) DM_MEDIAN_CASE(5) DM_MEDIAN_CASE(6) DM_MEDIAN_CASE(7)
        DM_MEDIAN_CASE(8) DM_MEDIAN_CASE(9) DM_MEDIAN_CASE(10) DM_MEDIAN_CASE(11) DM_MEDIAN_CASE(12) DM_MEDIAN_CASE(13)
        DM_MEDIAN_CASE(14) DM_MEDIAN_CASE(15) DM_MEDIAN_CASE(16)
#undef DM_MEDIAN_CASE
        default: return hipErrorInvalidValue;
    }
    static_assert(DM_MINE_MAX_SETS == 16, "one case per set count");
    return hipGetLastError();
}

hipError_t launch_gather_sets(const float* maps, const dm_mine_desc* desc, int n_groups, int n_sets, int ky, int k_per_image,
                              const int32_t* boxes, const int32_t* count, float* set_d, hipStream_t s) {
    if (n_groups < 1 || n_sets < 1 || k_per_image < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_sets_kernel, dim3(n_groups), dim3(256), 0, s, maps, desc, n_sets, ky, k_per_image, boxes, count, set_d);
    return hipGetLastError();
}

}  // namespace dm
