// xray_eval.hip — the counting half of the X-ray application's two numbers (applications/xray/compute.py:263-284):
//   tp = np.sum(dm_flattened[x_flattened == 1] > thresholds[:, np.newaxis], axis=1)      (:275)
//   fp = np.sum(dm_flattened[x_flattened == 0] > thresholds[:, np.newaxis], axis=1)      (:276)
//   dm[bbox[1]:bbox[3], bbox[0]:bbox[2]].mean()                                          (:264; the sum, the host divides)
// The reference compares every pixel with every threshold.  The thresholds decrease strictly, so tp[k] and fp[k] are the inclusive
// prefix sums of two histograms of "first k with thresholds[k] < v": one pass over the map, one binary search per pixel.
//
//   - xray_hist_kernel: row of the table on blockIdx.y, a chunk of kChunk pixels of that row's map on blockIdx.x.  Thresholds in LDS
//     as fp64; the comparison is the reference's (fp32 value widened, fp64 threshold, strictly greater; NaN exceeds nothing: bin T).
//     Two int32 histograms per workgroup in LDS.  The end bins 0 and T — where real maps put most pixels, and a constant map all of
//     them — are counted in registers and reduced once per wave by xor-shuffles; bins between take one LDS atomic per pixel, or one
//     per wave when the whole wave agrees.  Partials leave by plain stores; nothing is zeroed in global memory and there is no
//     floating-point atomic.
//   - the pixel-to-thread map depends on the pixel's index in its map alone (group g = 4 pixels, thread g % kThreads), never on the
//     address: the fp64 box sum then has the same bits wherever the map lies.  A row whose first float is 16-byte aligned reads its
//     groups as float4; any other row reads the same groups with scalar loads.  The last, partial group of a map is always scalar.
//     No load touches a float outside [0, H W).
//   - xray_finish_kernel: one workgroup per row; adds the partials in ascending workgroup order, scans the bins, stores tp / fp.
// Nothing waits on another workgroup; nothing reads workspace this call has not written.
#include "../../include/dm_engine.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

namespace dm {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 512;                         // 8 waves
constexpr int kWaves = kThreads / kWave;
constexpr int kChunk = 16384;                         // pixels per workgroup: 8 groups of 4 per thread
constexpr int kFinishThreads = 256;
static_assert(kChunk % (4 * kThreads) == 0, "whole groups per thread");

struct XrWork {                                       // the workspace: per (row, workgroup) one box sum and two histograms
    double* sums;                                     // [n_rows][n_wg]
    int32_t* hist;                                    // [n_rows][n_wg][2][T + 1]   (0 = inside the box, 1 = outside)
    size_t bytes;
};

inline int chunks_of(int64_t pixels) { return (int)((pixels + kChunk - 1) / kChunk); }

XrWork xr_layout(void* base, int n_rows, int T, int n_wg) {
    XrWork w;
    const size_t sums = ((size_t)n_rows * n_wg * 8 + 255) & ~(size_t)255;
    w.sums = (double*)base;
    w.hist = (int32_t*)(base ? (char*)base + sums : nullptr);
    w.bytes = sums + (size_t)n_rows * n_wg * 2 * (T + 1) * 4;
    return w;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

struct XrBox { int x1, y1, x2, y2; };                 // clipped to the map

__device__ __forceinline__ XrBox clip_box(const dm_xray_desc& d) {
    XrBox b;
    b.x1 = min(d.x1, d.W); b.x2 = min(d.x2, d.W);
    b.y1 = min(d.y1, d.H); b.y2 = min(d.y2, d.H);
    return b;
}

__global__ __launch_bounds__(kThreads)
void xray_hist_kernel(const float* __restrict__ maps, const dm_xray_desc* __restrict__ desc, const double* __restrict__ thresholds,
                      int T, int n_wg, double* __restrict__ sums, int32_t* __restrict__ hist_out) {
    extern __shared__ double smem[];
    const int row = blockIdx.y, wg = blockIdx.x;
    const dm_xray_desc d = desc[row];
    const int n = d.H * d.W;
    const int c0 = wg * kChunk;
    if (c0 >= n) return;                              // this row's map is shorter than the longest: its finish reads chunks_of(n) partials only
    const int c1 = min(c0 + kChunk, n);
    double* thr = smem;                               // [T]
    int* hist = (int*)(smem + T);                     // [2][T + 1]
    __shared__ double wsum[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int k = tid; k < T; k += kThreads) thr[k] = thresholds[k];
    for (int k = tid; k < 2 * (T + 1); k += kThreads) hist[k] = 0;
    __syncthreads();

    const XrBox box = clip_box(d);
    const float* base = maps + d.map_offset;
    const double thr_hi = thr[0], thr_lo = thr[T - 1];
    int in0 = 0, inT = 0, out0 = 0, outT = 0;         // the end bins, in registers
    double sum = 0.0;

    auto pixel = [&](float f, int r, int c) {
        const double v = (double)f;
        const bool inside = r >= box.y1 && r < box.y2 && c >= box.x1 && c < box.x2;
        if (inside) sum += v;
        int key = -1;                                 // (bin, side) of a pixel that falls between the end bins
        if (v > thr_hi) {
            if (inside) ++in0; else ++out0;
        } else if (!(v > thr_lo)) {                   // NaN included
            if (inside) ++inT; else ++outT;
        } else {
            int lo = 1, hi = T - 1;                   // thr[0] >= v > thr[T - 1]: the first k with thr[k] < v lies in [1, T - 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (thr[mid] < v) hi = mid; else lo = mid + 1;
            }
            key = (inside ? 0 : T + 1) + lo;
        }
        return key;
    };
    auto count = [&](int key) {                       // called by whole waves (uniform trip counts below)
        const int first = __shfl(key, 0);
        if (__all(key == first)) {                    // a flat stretch: one atomic for the wave instead of 64 on one address
            if (lane == 0 && first >= 0) atomicAdd(&hist[first], kWave);
        } else if (key >= 0) {
            atomicAdd(&hist[key], 1);
        }
    };

    const int n_full = (c1 - c0) >> 2;                // whole groups of 4 pixels in this chunk
    const bool vec = (((uintptr_t)(base + c0)) & 15) == 0;
    const int trips = (n_full + kThreads - 1) / kThreads;
    for (int it = 0; it < trips; ++it) {
        const int g = it * kThreads + tid;
        int key[4] = {-1, -1, -1, -1};
        if (g < n_full) {
            const int p = c0 + 4 * g;
            float f[4];
            if (vec) {
                const float4 q = *(const float4*)(base + p);
                f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) f[j] = base[p + j];
            }
            int r = p / d.W, c = p - r * d.W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                key[j] = pixel(f[j], r, c);
                if (++c == d.W) { c = 0; ++r; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) count(key[j]);
    }
    {                                                 // the map's last 1 ... 3 pixels (only the last chunk of a row has any)
        const int p = c0 + 4 * n_full + tid;
        int key = -1;
        if (p < c1) {
            const int r = p / d.W;
            key = pixel(base[p], r, p - r * d.W);
        }
        if (wave == 0) count(key);
    }

    in0 = wave_sum(in0); inT = wave_sum(inT); out0 = wave_sum(out0); outT = wave_sum(outT);
    sum = wave_sum(sum);
    if (lane == 0) {
        if (in0) atomicAdd(&hist[0], in0);
        if (inT) atomicAdd(&hist[T], inT);
        if (out0) atomicAdd(&hist[T + 1], out0);
        if (outT) atomicAdd(&hist[2 * T + 1], outT);
        wsum[wave] = sum;
    }
    __syncthreads();
    int32_t* out = hist_out + ((size_t)row * n_wg + wg) * 2 * (T + 1);
    for (int k = tid; k < 2 * (T + 1); k += kThreads) out[k] = hist[k];
    if (tid == 0) {
        double s = wsum[0];
        for (int w = 1; w < kWaves; ++w) s += wsum[w];
        sums[(size_t)row * n_wg + wg] = s;
    }
}

__global__ __launch_bounds__(kFinishThreads)
void xray_finish_kernel(const dm_xray_desc* __restrict__ desc, int T, int n_wg, const double* __restrict__ sums,
                        const int32_t* __restrict__ hist, int32_t* __restrict__ tp, int32_t* __restrict__ fp,
                        int32_t* __restrict__ n_in, double* __restrict__ box_sum) {
    __shared__ int bins[2][DM_XRAY_MAX_THRESHOLDS + 1];
    __shared__ int seg[2][kFinishThreads];
    const int row = blockIdx.x, tid = threadIdx.x;
    const dm_xray_desc d = desc[row];
    const int mine = (d.H * d.W + kChunk - 1) / kChunk;              // the workgroups that wrote a partial for this row
    const int32_t* h = hist + (size_t)row * n_wg * 2 * (T + 1);
    for (int b = tid; b < 2 * (T + 1); b += kFinishThreads) {
        int s = 0;
        for (int w = 0; w < mine; ++w) s += h[(size_t)w * 2 * (T + 1) + b];
        bins[b / (T + 1)][b % (T + 1)] = s;
    }
    __syncthreads();
    // inclusive scan of bins [0, T): each thread owns `per` consecutive bins, thread 0 scans the 256 segment totals
    const int per = (T + kFinishThreads - 1) / kFinishThreads;
    const int b0 = min(tid * per, T), b1 = min(b0 + per, T);
    int s_in = 0, s_out = 0;
    for (int b = b0; b < b1; ++b) { s_in += bins[0][b]; s_out += bins[1][b]; }
    seg[0][tid] = s_in; seg[1][tid] = s_out;
    __syncthreads();
    if (tid == 0) {
        int a = 0, o = 0;
        for (int t = 0; t < kFinishThreads; ++t) {
            const int va = seg[0][t], vo = seg[1][t];
            seg[0][t] = a; seg[1][t] = o;                           // exclusive
            a += va; o += vo;
        }
        const XrBox box = clip_box(d);
        n_in[row] = max(box.y2 - box.y1, 0) * max(box.x2 - box.x1, 0);
        double s = 0.0;
        for (int w = 0; w < mine; ++w) s += sums[(size_t)row * n_wg + w];
        box_sum[row] = s;
    }
    __syncthreads();
    s_in = seg[0][tid]; s_out = seg[1][tid];
    for (int b = b0; b < b1; ++b) {
        s_in += bins[0][b]; s_out += bins[1][b];
        tp[(size_t)row * T + b] = s_in;
        fp[(size_t)row * T + b] = s_out;
    }
}

inline size_t hist_lds_bytes(int T) { return (size_t)T * 8 + (size_t)2 * (T + 1) * 4; }

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

size_t dm_xray_eval_workspace_bytes(int n_rows, int n_thresholds, int64_t max_pixels) {
    if (n_rows < 1 || n_thresholds < 1 || n_thresholds > DM_XRAY_MAX_THRESHOLDS || max_pixels < 1 || max_pixels >= (1 << 24)) return 0;
    return xr_layout(nullptr, n_rows, n_thresholds, chunks_of(max_pixels)).bytes;
}

int dm_xray_eval(const void* maps_dev, const dm_xray_desc* desc_dev, int n_rows, const double* thresholds_dev, int n_thresholds,
                 void* work_dev, int32_t* tp_out_dev, int32_t* fp_out_dev, int32_t* n_in_out_dev, double* box_sum_out_dev,
                 void* stream) {
    if (!maps_dev || !desc_dev || !thresholds_dev || !work_dev || !tp_out_dev || !fp_out_dev || !n_in_out_dev || !box_sum_out_dev)
        return DM_XRAY_E_NULL;
    if (n_rows < 1) return DM_XRAY_E_ROWS;
    const int T = n_thresholds;
    if (T < 1 || T > DM_XRAY_MAX_THRESHOLDS) return DM_XRAY_E_NTHR;
    hipStream_t s = (hipStream_t)stream;
    std::vector<dm_xray_desc> desc((size_t)n_rows);
    std::vector<double> thr((size_t)T);
    if (hipMemcpyAsync(desc.data(), desc_dev, desc.size() * sizeof(dm_xray_desc), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(thr.data(), thresholds_dev, thr.size() * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return DM_XRAY_E_HIP;
    for (int k = 0; k < T; ++k)
        if (thr[k] != thr[k] || (k > 0 && !(thr[k] < thr[k - 1]))) return DM_XRAY_E_THR_ORDER;
    int64_t max_pixels = 0;
    for (const dm_xray_desc& d : desc) {
        if (d.H < 1 || d.W < 1) return DM_XRAY_E_SIZE;
        const int64_t px = (int64_t)d.H * d.W;
        if (px >= (1 << 24)) return DM_XRAY_E_PIXELS;
        if (d.x1 < 0 || d.y1 < 0 || d.x2 < 0 || d.y2 < 0) return DM_XRAY_E_BOX;
        if (px > max_pixels) max_pixels = px;
    }
    const int n_wg = chunks_of(max_pixels);
    const XrWork w = xr_layout(work_dev, n_rows, T, n_wg);
    const size_t lds = hist_lds_bytes(T);
    if (lds > 64 * 1024 &&                                   // past the default cap a kernel has to ask (T > 4095)
        hipFuncSetAttribute((const void*)xray_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DM_XRAY_E_HIP;
    hipLaunchKernelGGL(xray_hist_kernel, dim3(n_wg, n_rows), dim3(kThreads), lds, s, (const float*)maps_dev, desc_dev, thresholds_dev,
                       T, n_wg, w.sums, w.hist);
    if (hipGetLastError() != hipSuccess) return DM_XRAY_E_HIP;
    hipLaunchKernelGGL(xray_finish_kernel, dim3(n_rows), dim3(kFinishThreads), 0, s, desc_dev, T, n_wg, (const double*)w.sums,
                       (const int32_t*)w.hist, tp_out_dev, fp_out_dev, n_in_out_dev, box_sum_out_dev);
    if (hipGetLastError() != hipSuccess) return DM_XRAY_E_HIP;
    return 0;
}

}  // extern "C"
