// mine.hip — the patch-mining stage between the pooled typicality maps and the patch features:
//   `Cluster.df_D` (cluster.py:184-215): one candidate per window position (i, j) of the pooled map dm [OH][OW], box
//   (x_start, y_start, x_end, y_end) = (i, j, i + kx, j + ky) with x = rows, D = dm[i, j]; `sort` by D (utils.py:82-83), then
//   `get_non_overlapping` (utils.py:94-102): take the first candidate, drop every candidate whose box touches it (inclusive
//   comparisons: |i - i*| <= kx and |j - j*| <= ky), repeat k_per_image times or until nothing is left.
// The frame, the sort and the filters never exist here: round r is one argmax over the map that skips the candidates inside
// the inclusive zone of the r winners so far.  Nothing is written to the map and there is no mask array.
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

namespace dm {

namespace {

constexpr int kMineThreads = 1024;
constexpr int kMineWaves = kMineThreads / 64;

// Order-preserving image of a non-NaN fp32 in uint32 (a < b  <=>  image(a) < image(b); -0 is folded onto +0 so that the two
// zeros tie like they do in a comparison); inverted for the ascending order.  No non-NaN value maps to 0 in either order.
__device__ __forceinline__ unsigned mine_key_bits(float v, int ascending) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ascending ? ~u : u;
}

__device__ __forceinline__ unsigned long long mine_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// One workgroup per image.  The reduction key is 64 bits: the key's order image in the high word, ~flat_index in the low word,
// so the maximum is the best key and, among equal keys, the LOWEST row-major index.  0 = "no candidate".  The key comes from
// `priority` when given (the shuffled arm: a permutation's ranks), D always from the map.  NaN keys are never selected.
__global__ __launch_bounds__(kMineThreads)
void mine_select_kernel(const float* __restrict__ maps, const float* __restrict__ priority, const dm_mine_desc* __restrict__ desc,
                        int kx, int ky, int k_per_image, int ascending, int32_t* __restrict__ boxes, float* __restrict__ d_out,
                        int32_t* __restrict__ count) {
    __shared__ unsigned long long wave_best[kMineWaves];
    __shared__ int win_i[DM_MINE_MAX_K], win_j[DM_MINE_MAX_K];
    const dm_mine_desc d = desc[blockIdx.x];
    const int OH = d.H - kx + 1, OW = d.W - ky + 1, n = OH * OW;
    const float* __restrict__ dm = maps + d.map_offset;
    const float* __restrict__ keys = priority ? priority + d.map_offset : dm;
    boxes += (size_t)blockIdx.x * k_per_image * 4;
    d_out += (size_t)blockIdx.x * k_per_image;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int taken = 0;
    for (int r = 0; r < k_per_image; ++r) {
        unsigned long long best = 0ull;
        for (int idx = tid; idx < n; idx += kMineThreads) {
            const float v = keys[idx];
            if (v != v) continue;
            const unsigned long long key = ((unsigned long long)mine_key_bits(v, ascending) << 32) | (unsigned)~(unsigned)idx;
            if (key <= best) continue;                     // the zone test only for a candidate that would lead
            const int i = idx / OW, j = idx - i * OW;
            bool is_free = true;
            for (int t = 0; t < r; ++t) {
                const int di = i - win_i[t], dj = j - win_j[t];
                if (di <= kx && di >= -kx && dj <= ky && dj >= -ky) { is_free = false; break; }
            }
            if (is_free) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                 // wave: 64 lanes, cross-lane
            const unsigned hi = __shfl_xor((unsigned)(best >> 32), o), lo = __shfl_xor((unsigned)best, o);
            best = mine_max(best, ((unsigned long long)hi << 32) | lo);
        }
        if (lane == 0) wave_best[wv] = best;
        __syncthreads();
        unsigned long long b = wave_best[0];               // waves: every thread folds the 16 partials (LDS broadcast reads)
#pragma unroll
        for (int t = 1; t < kMineWaves; ++t) b = mine_max(b, wave_best[t]);
        if (b == 0ull) break;                              // the map ran out (uniform over the workgroup)
        const int idx = (int)~(unsigned)b;
        const int i = idx / OW, j = idx - i * OW;
        if (tid == 0) {
            win_i[r] = i; win_j[r] = j;
            boxes[r * 4 + 0] = i; boxes[r * 4 + 1] = j; boxes[r * 4 + 2] = i + kx; boxes[r * 4 + 3] = j + ky;
            d_out[r] = dm[idx];
        }
        taken = r + 1;
        __syncthreads();                                   // winners visible, wave_best free for the next round
    }
    for (int t = taken + tid; t < k_per_image; t += kMineThreads) {
        boxes[t * 4 + 0] = -1; boxes[t * 4 + 1] = -1; boxes[t * 4 + 2] = -1; boxes[t * 4 + 3] = -1;
        d_out[t] = __uint_as_float(0x7FC00000u);
    }
    if (tid == 0) count[blockIdx.x] = taken;
}

}  // namespace

hipError_t launch_mine_select(const float* maps, const float* priority, const dm_mine_desc* desc, int n_images, int kx, int ky,
                              int k_per_image, int ascending, int32_t* boxes, float* d_out, int32_t* count, hipStream_t s) {
    if (n_images < 1 || k_per_image < 1 || k_per_image > DM_MINE_MAX_K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mine_select_kernel, dim3(n_images), dim3(kMineThreads), 0, s, maps, priority, desc, kx, ky, k_per_image,
                       ascending ? 1 : 0, boxes, d_out, count);
    return hipGetLastError();
}

}  // namespace dm
