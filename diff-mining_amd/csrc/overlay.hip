// overlay.hip — typicality overlays: scipy's gaussian_filter on fp32 maps, bit for bit, and the reference's alpha blend
//   T = gaussian_filter(alpha, sigma=10); T = T*(T>0); R = 0.05*I + 0.95*(T*I + (1-T)); (R*255).astype(np.uint8)
// (typicality/cluster.py:93-110, typicality/utils.py:165-214, applications/parallel-dataset/cluster.py:132-141) plus `filter_patch`
// (utils.py:104-109) on the same crops.
//
//   - gauss_pass_kernel<AXIS>: map of the table on blockIdx.y, a 32 x 32 output tile of it on blockIdx.x (a block past the map's own
//     tile count leaves at once).  The tile and its halo of `radius` elements on either side of the filtered axis are staged in LDS as
//     fp32; the reflected index (a mirror of period 2n, so a halo may wrap several times) is resolved when the element is loaded, and
//     is always inside [0, n): no load touches a float outside the map.  Each thread owns 4 outputs, 8 rows apart, and walks the taps
//     from the far pair inward in fp64: acc = a[i] w[0]; acc += (a[i-j] + a[i+j]) w[j], j = r ... 1 (multiply and add separately
//     rounded: the TU is built with -ffp-contract=off).  One cast to fp32 per axis.  Axis 0 reads the maps and writes the workspace,
//     axis 1 reads the workspace and writes the result, applying the clamp, or leaving one NaN-propagating maximum per tile.
//   - gauss_unit_kernel: the third pass of DM_GAUSS_POST_UNIT.  Every block folds its map's tile maxima (max is exact: the order of
//     the fold cannot change the value that matters) and divides and clamps its own tile in place.
//   - overlay_blend_kernel: one workgroup per row; the blend in fp64 per pixel and channel; the luminance sum as a 64-bit integer,
//     folded by shuffles and LDS.
// Nothing waits on another workgroup, nothing reads workspace this call has not written, and there is no floating-point atomic.
#include "../../include/dm_engine.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dm {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = DM_GAUSS_TILE;
constexpr int kPerThread = kTile * kTile / kThreads;          // 4 outputs per thread, kTile / kPerThread rows apart
constexpr int kRowStep = kThreads / kTile;                    // 8
constexpr int kMaxSide = 1 << 24;
static_assert(kTile * kTile % kThreads == 0 && kThreads % kTile == 0, "whole outputs per thread");
static_assert((size_t)(kTile + 2 * DM_GAUSS_MAX_RADIUS) * kTile * sizeof(float) <= 60 * 1024, "the tile and its halo stay below the 64 KiB of LDS a kernel gets unasked");

inline size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int tiles_of(int h, int w) { return ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile); }

// numpy's maximum: NaN if either is NaN
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

__device__ __forceinline__ float block_nan_max(float v, float* lds /*[kWaves]*/) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v = nan_max(v, __shfl_xor(v, m));
    __syncthreads();                                          // `lds` may still be read from an earlier fold
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = v;
    __syncthreads();
    v = lds[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v = nan_max(v, lds[k]);
    return v;
}

// `reflect` (d c b a | a b c d | d c b a): index i of the infinite extension of a line of n elements
__device__ __forceinline__ int reflect_index(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

__device__ __forceinline__ float clamp_as_numpy(float v) { return v * (v > 0.0f ? 1.0f : 0.0f); }     // T * (T > 0)

template <int AXIS>
__global__ __launch_bounds__(kThreads) void gauss_pass_kernel(const float* __restrict__ src_base, float* __restrict__ dst_base,
                                                              const dm_gauss_desc* __restrict__ desc, const double* __restrict__ wts,
                                                              int radius, int post_op, float* __restrict__ partial, int max_tiles) {
    extern __shared__ __align__(16) float tile[];             // AXIS 0: [kTile + 2 r][kTile]; AXIS 1: [kTile][kTile + 2 r]
    __shared__ float fold[kWaves];
    const dm_gauss_desc d = desc[blockIdx.y];
    const int tw = (d.W + kTile - 1) / kTile, th = (d.H + kTile - 1) / kTile;
    const int t = blockIdx.x;
    if (t >= tw * th) return;
    const int r0 = (t / tw) * kTile, c0 = (t % tw) * kTile;
    const float* __restrict__ src = src_base + (AXIS == 0 ? d.map_offset : d.work_offset);
    float* __restrict__ dst = dst_base + (AXIS == 0 ? d.work_offset : d.out_offset);
    const int r = radius;
    const int rows = AXIS == 0 ? kTile + 2 * r : kTile, cols = AXIS == 0 ? kTile : kTile + 2 * r;
    for (int idx = threadIdx.x; idx < rows * cols; idx += kThreads) {
        const int lr = idx / cols, lc = idx - lr * cols;
        int gr, gc;
        bool ok;
        if (AXIS == 0) {
            gr = reflect_index(r0 + lr - r, d.H);
            gc = c0 + lc;
            ok = gc < d.W;
        } else {
            gr = r0 + lr;
            gc = reflect_index(c0 + lc - r, d.W);
            ok = gr < d.H;
        }
        tile[idx] = ok ? src[(int64_t)gr * d.W + gc] : 0.0f;
    }
    __syncthreads();
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int step = AXIS == 0 ? cols : 1;                    // LDS distance of one tap
    int at[kPerThread];
    double acc[kPerThread];
    const double w0 = wts[r];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int lr = ty + k * kRowStep;
        at[k] = AXIS == 0 ? (lr + r) * cols + tx : lr * cols + tx + r;
        acc[k] = (double)tile[at[k]] * w0;
    }
    for (int j = r; j >= 1; --j) {
        const double wj = wts[r - j];
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const double pair = (double)tile[at[k] - j * step] + (double)tile[at[k] + j * step];
            acc[k] = acc[k] + pair * wj;
        }
    }
    float best = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int gr = r0 + ty + k * kRowStep, gc = c0 + tx;
        if (gr < d.H && gc < d.W) {
            float v = (float)acc[k];
            if (AXIS == 1 && post_op == DM_GAUSS_POST_CLAMP) v = clamp_as_numpy(v);
            dst[(int64_t)gr * d.W + gc] = v;
            best = nan_max(best, v);
        }
    }
    if (AXIS == 1 && post_op == DM_GAUSS_POST_UNIT) {
        best = block_nan_max(best, fold);
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * max_tiles + t] = best;
    }
}

__global__ __launch_bounds__(kThreads) void gauss_unit_kernel(float* __restrict__ out_base, const dm_gauss_desc* __restrict__ desc,
                                                              const float* __restrict__ partial, int max_tiles,
                                                              float* __restrict__ max_out) {
    __shared__ float fold[kWaves];
    const dm_gauss_desc d = desc[blockIdx.y];
    const int tw = (d.W + kTile - 1) / kTile, th = (d.H + kTile - 1) / kTile;
    const int t = blockIdx.x;
    if (t >= tw * th) return;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < tw * th; i += kThreads) m = nan_max(m, partial[(int64_t)blockIdx.y * max_tiles + i]);
    m = block_nan_max(m, fold);
    const bool degenerate = m == 0.0f || m != m;
    if (t == 0 && threadIdx.x == 0 && max_out) max_out[blockIdx.y] = m;
    float* __restrict__ out = out_base + d.out_offset;
    const int r0 = (t / tw) * kTile, c0 = (t % tw) * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int gr = r0 + ty + k * kRowStep, gc = c0 + tx;
        if (gr < d.H && gc < d.W) {
            const int64_t i = (int64_t)gr * d.W + gc;
            out[i] = degenerate ? 0.0f : clamp_as_numpy(out[i] / m);
        }
    }
}

__global__ __launch_bounds__(kThreads) void overlay_blend_kernel(const uint8_t* __restrict__ images, const float* __restrict__ maps,
                                                                 const float* __restrict__ map_max, const dm_overlay_row* __restrict__ rows,
                                                                 uint8_t* __restrict__ blended, uint8_t* __restrict__ plain,
                                                                 float* __restrict__ alpha, int64_t* __restrict__ lum_out,
                                                                 int32_t* __restrict__ verdict_out, int32_t* __restrict__ degenerate_out) {
    __shared__ long long fold[kWaves];
    const dm_overlay_row w = rows[blockIdx.x];
    const int bh = w.x_end - w.x_start, bw = w.y_end - w.y_start;
    const int64_t count = (int64_t)bh * bw;
    bool degenerate = false;
    if (w.variant == DM_OVERLAY_CROP && w.map_index >= 0) {
        const float m = map_max[w.map_index];
        degenerate = m == 0.0f || m != m;
    }
    const uint8_t* __restrict__ img = images + w.image_offset;
    const float* __restrict__ map = maps + w.map_offset;
    uint8_t* __restrict__ out = blended + w.out_offset;
    uint8_t* __restrict__ keep = plain + w.out_offset;
    long long lum = 0;
    for (int64_t p = threadIdx.x; p < count; p += kThreads) {
        const int i = (int)(p / bw), j = (int)(p - (int64_t)i * bw);
        const int gi = w.x_start + i, gj = w.y_start + j;
        const int mi = gi - w.map_x0, mj = gj - w.map_y0;
        float T = 0.0f;
        if (!degenerate && mi >= 0 && mi < w.map_h && mj >= 0 && mj < w.map_w) T = map[(int64_t)mi * w.map_w + mj];
        const double t = (double)T;
        const double rest = w.variant == DM_OVERLAY_CROP ? (double)(1.0f - T) : 1.0 - t;
        const uint8_t* px = img + ((int64_t)gi * w.img_w + gj) * 3;
        int c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = px[k];
            const double I = (double)c[k] / 255.0;
            const double R = 0.05 * I + 0.95 * (t * I + rest);
            const double v = fmin(fmax(R * 255.0, -2147483648.0), 2147483647.0);          // NaN -> -2^31: byte 0, as numpy on x86-64
            out[p * 3 + k] = (uint8_t)((int)v & 255);
            keep[p * 3 + k] = (uint8_t)c[k];
        }
        if (alpha) alpha[w.alpha_offset + p] = T;
        lum += (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 0x8000) >> 16;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) lum += __shfl_xor(lum, m);
    if ((threadIdx.x & (kWave - 1)) == 0) fold[threadIdx.x / kWave] = lum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int k = 0; k < kWaves; ++k) s += fold[k];
        lum_out[blockIdx.x] = s;
        const double mean = (double)s / (double)count;       // 0 / 0 = NaN for an empty crop: no verdict
        verdict_out[blockIdx.x] = (30.0 < mean && mean < 225.0) ? 1 : 0;
        degenerate_out[blockIdx.x] = degenerate ? 1 : 0;
    }
}

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

size_t dm_overlay_workspace_bytes(int n_maps, int64_t total_elements, int max_h, int max_w) {
    if (n_maps < 1 || total_elements < 1 || max_h < 1 || max_w < 1 || max_h > kMaxSide || max_w > kMaxSide) return 0;
    return round256((size_t)n_maps * tiles_of(max_h, max_w) * sizeof(float)) + (size_t)total_elements * sizeof(float);
}

int dm_gaussian_filter_maps(const void* maps_dev, const dm_gauss_desc* desc_dev, int n_maps, double sigma, const double* weights_dev,
                            int radius, int post_op, void* work_dev, size_t work_bytes, void* out_dev, float* max_out_dev,
                            void* stream) {
    if (!maps_dev || !desc_dev || !weights_dev || !work_dev || !out_dev) return 1;
    if (n_maps < 1 || n_maps > 65535 || !(sigma > 0.0) || !(sigma < 1e6)) return 1;          // the map rides on blockIdx.y
    if (radius != (int)(4.0 * sigma + 0.5) || radius < 0 || radius > DM_GAUSS_MAX_RADIUS) return 1;
    if (post_op < DM_GAUSS_POST_NONE || post_op > DM_GAUSS_POST_UNIT) return 1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<dm_gauss_desc> desc((size_t)n_maps);
    if (hipMemcpyAsync(desc.data(), desc_dev, desc.size() * sizeof(dm_gauss_desc), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return 2;
    int max_h = 0, max_w = 0;
    for (const dm_gauss_desc& d : desc) {
        if (d.H < 1 || d.W < 1 || d.H > kMaxSide || d.W > kMaxSide || (int64_t)d.H * d.W > 0x7fffffffLL) return 1;
        if (d.map_offset < 0 || d.out_offset < 0 || d.work_offset < 0) return 1;
        max_h = std::max(max_h, d.H);
        max_w = std::max(max_w, d.W);
    }
    const int max_tiles = tiles_of(max_h, max_w);
    const size_t partial_bytes = round256((size_t)n_maps * max_tiles * sizeof(float));
    if (work_bytes < partial_bytes) return 1;
    const int64_t room = (int64_t)((work_bytes - partial_bytes) / sizeof(float));
    for (const dm_gauss_desc& d : desc)
        if (d.work_offset + (int64_t)d.H * d.W > room) return 1;
    float* partial = (float*)work_dev;
    float* mid = (float*)((char*)work_dev + partial_bytes);
    const size_t lds = (size_t)(kTile + 2 * radius) * kTile * sizeof(float);
    const dim3 grid((unsigned)max_tiles, (unsigned)n_maps);
    hipLaunchKernelGGL(gauss_pass_kernel<0>, grid, dim3(kThreads), lds, s, (const float*)maps_dev, mid, desc_dev, weights_dev, radius,
                       post_op, partial, max_tiles);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(gauss_pass_kernel<1>, grid, dim3(kThreads), lds, s, (const float*)mid, (float*)out_dev, desc_dev, weights_dev,
                       radius, post_op, partial, max_tiles);
    if (hipGetLastError() != hipSuccess) return 2;
    if (post_op == DM_GAUSS_POST_UNIT) {
        hipLaunchKernelGGL(gauss_unit_kernel, grid, dim3(kThreads), 0, s, (float*)out_dev, desc_dev, (const float*)partial, max_tiles,
                           max_out_dev);
        if (hipGetLastError() != hipSuccess) return 2;
    }
    return 0;
}

int dm_overlay_blend(const void* images_dev, int64_t image_bytes, const void* maps_dev, int64_t map_elements, const float* map_max_dev,
                     int n_map_max, const dm_overlay_row* rows_dev, int n_rows, void* blended_out_dev, void* plain_out_dev,
                     int64_t out_bytes, float* alpha_out_dev, int64_t alpha_elements, int64_t* lum_out_dev, int32_t* verdict_out_dev,
                     int32_t* degenerate_out_dev, void* stream) {
    if (!images_dev || !maps_dev || !rows_dev || !blended_out_dev || !plain_out_dev || !lum_out_dev || !verdict_out_dev ||
        !degenerate_out_dev)
        return 1;
    if (n_rows < 1 || image_bytes < 0 || map_elements < 0 || out_bytes < 0 || alpha_elements < 0 || n_map_max < 0) return 1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<dm_overlay_row> rows((size_t)n_rows);
    if (hipMemcpyAsync(rows.data(), rows_dev, rows.size() * sizeof(dm_overlay_row), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return 2;
    for (const dm_overlay_row& w : rows) {
        if (w.variant < DM_OVERLAY_IMAGE || w.variant > DM_OVERLAY_STORED) return 1;
        if (w.img_h < 1 || w.img_w < 1 || w.img_h > kMaxSide || w.img_w > kMaxSide || w.image_offset < 0) return 1;
        if (w.image_offset + (int64_t)w.img_h * w.img_w * 3 > image_bytes) return 1;
        if (w.x_start < 0 || w.x_start > w.x_end || w.x_end > w.img_h || w.y_start < 0 || w.y_start > w.y_end || w.y_end > w.img_w) return 1;
        if (w.map_h < 0 || w.map_w < 0) return 1;
        if (w.map_h > 0 && w.map_w > 0) {
            if (w.map_offset < 0 || w.map_offset + (int64_t)w.map_h * w.map_w > map_elements) return 1;
            if (w.map_x0 < 0 || w.map_y0 < 0 || (int64_t)w.map_x0 + w.map_h > w.img_h || (int64_t)w.map_y0 + w.map_w > w.img_w) return 1;
        }
        if (w.map_index < -1 || w.map_index >= n_map_max || (w.map_index >= 0 && !map_max_dev)) return 1;
        const int64_t count = (int64_t)(w.x_end - w.x_start) * (w.y_end - w.y_start);
        if (w.out_offset < 0 || w.out_offset + 3 * count > out_bytes) return 1;
        if (alpha_out_dev && (w.alpha_offset < 0 || w.alpha_offset + count > alpha_elements)) return 1;
    }
    hipLaunchKernelGGL(overlay_blend_kernel, dim3((unsigned)n_rows), dim3(kThreads), 0, s, (const uint8_t*)images_dev,
                       (const float*)maps_dev, map_max_dev, rows_dev, (uint8_t*)blended_out_dev, (uint8_t*)plain_out_dev, alpha_out_dev,
                       lum_out_dev, verdict_out_dev, degenerate_out_dev);
    if (hipGetLastError() != hipSuccess) return 2;
    return 0;
}

}  // extern "C"
