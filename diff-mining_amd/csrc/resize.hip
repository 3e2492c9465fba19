// PIL-exact LANCZOS rescale + `to_tensor(x) * 2 - 1` of uint8 HWC RGB images on the device (dm_resize_lanczos,
// include/dm_engine.h).  The reference resizes with `PIL.Image.resize(size, LANCZOS)` (compute.py:165-180) and feeds
// the VAE `to_tensor(img) * 2 - 1` (compute.py:126-132).  PIL's 8-bit resampler is integer arithmetic over
// per-output-pixel coefficient windows, so the device result is bit-equal when it runs the same two passes on the
// same tables: the tables (window start / length and fixed-point weights per output column and row) are built on the
// host in float64 by PIL's own formula (typicality.lanczos_axis); here
//   pass 1 (horizontal): source rows [ybox_first, ybox_first + tmp_rows) -> uint8 tmp [3][tmp_rows][out_w]
//   pass 2 (vertical)  : tmp -> uint8 -> fp32 [B][3][out_h][out_w] in [-1,1]
// each with int32 accumulators seeded with 1 << (PRECISION_BITS - 1), shifted right by PRECISION_BITS and clamped to
// [0, 255] (PIL's clip8).  One thread per output value per pass: the kernel is bandwidth-light integer work.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/dm_engine.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;        // PIL Resample.c PRECISION_BITS
constexpr int kThreads = 256;

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= kPrecisionBits;                           // arithmetic shift, as PIL's lookup index
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// `to_tensor(x) * 2 - 1` in fp32, the operation order of TypicalityScorer.load_image: x / 255 (correctly rounded fp32
// division: hipcc's default), * 2, - 1 (the build uses -ffp-contract=off, so no fma).
__device__ __forceinline__ float unit(uint8_t v) {
    return (float)v / 255.0f * 2.0f - 1.0f;
}

__global__ void __launch_bounds__(kThreads) resize_h_kernel(const uint8_t* __restrict__ src, const dm_resize_desc* __restrict__ desc,
                                                            const int32_t* __restrict__ tables, int out_w, int tmp_rows_max,
                                                            uint8_t* __restrict__ tmp) {
    const int b = blockIdx.y;
    const dm_resize_desc d = desc[b];
    const long long n = 3LL * d.tmp_rows * out_w;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % out_w);
    const int y = (int)((i / out_w) % d.tmp_rows);
    const int c = (int)(i / ((long long)out_w * d.tmp_rows));
    const int xmin = tables[d.xb_off + 2 * x], xn = tables[d.xb_off + 2 * x + 1];
    const int32_t* k = tables + d.xk_off + (long long)x * d.kx;
    int ss = 1 << (kPrecisionBits - 1);
    const int sy = d.ybox_first + y;
    // the host validated the tables; this guard only keeps a corrupt descriptor from reading outside the image
    if (xmin >= 0 && xn <= d.kx && xmin + xn <= d.src_w && sy >= 0 && sy < d.src_h) {
        const uint8_t* row = src + d.src_offset + ((long long)sy * d.src_w + xmin) * 3 + c;
        for (int t = 0; t < xn; ++t) ss += (int)row[3 * t] * k[t];
    }
    tmp[(size_t)b * 3 * tmp_rows_max * out_w + ((size_t)c * tmp_rows_max + y) * out_w + x] = clip8(ss);
}

__global__ void __launch_bounds__(kThreads) resize_v_kernel(const dm_resize_desc* __restrict__ desc, const int32_t* __restrict__ tables,
                                                            int out_w, int out_h, int tmp_rows_max, const uint8_t* __restrict__ tmp,
                                                            float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long n = 3LL * out_h * out_w;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const dm_resize_desc d = desc[b];
    const int x = (int)(i % out_w);
    const int y = (int)((i / out_w) % out_h);
    const int c = (int)(i / ((long long)out_w * out_h));
    const int ymin = tables[d.yb_off + 2 * y], yn = tables[d.yb_off + 2 * y + 1];     // ymin relative to ybox_first
    const int32_t* k = tables + d.yk_off + (long long)y * d.ky;
    int ss = 1 << (kPrecisionBits - 1);
    if (ymin >= 0 && yn <= d.ky && ymin + yn <= d.tmp_rows) {
        const uint8_t* col = tmp + (size_t)b * 3 * tmp_rows_max * out_w + ((size_t)c * tmp_rows_max + ymin) * out_w + x;
        for (int t = 0; t < yn; ++t) ss += (int)col[(size_t)t * out_w] * k[t];
    }
    out[(size_t)b * n + i] = unit(clip8(ss));
}

// no resampling (datasets without a rescale rule): uint8 HWC -> fp32 CHW in [-1,1]
__global__ void __launch_bounds__(kThreads) to_unit_kernel(const uint8_t* __restrict__ src, const dm_resize_desc* __restrict__ desc,
                                                           int out_w, int out_h, float* __restrict__ out) {
    const int b = blockIdx.y;
    const long long n = 3LL * out_h * out_w;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const dm_resize_desc d = desc[b];
    const int x = (int)(i % out_w);
    const int y = (int)((i / out_w) % out_h);
    const int c = (int)(i / ((long long)out_w * out_h));
    uint8_t v = 0;
    if (d.src_w == out_w && d.src_h == out_h) v = src[d.src_offset + ((long long)y * out_w + x) * 3 + c];
    out[(size_t)b * n + i] = unit(v);
}

}  // namespace

extern "C" int dm_resize_lanczos(const void* src_dev, const dm_resize_desc* desc_dev, const int32_t* tables_dev, int batch, int out_w,
                                 int out_h, int tmp_rows_max, void* tmp_dev, float* out_dev, void* stream) {
    if (!src_dev || !desc_dev || !out_dev || batch < 1 || batch > 65535 || out_w < 1 || out_h < 1) return 1;
    if (tables_dev && (!tmp_dev || tmp_rows_max < 1)) return 1;
    hipStream_t s = (hipStream_t)stream;
    const long long n_out = 3LL * out_h * out_w;
    const dim3 grid_out((unsigned)((n_out + kThreads - 1) / kThreads), (unsigned)batch);
    if (!tables_dev) {
        hipLaunchKernelGGL(to_unit_kernel, grid_out, dim3(kThreads), 0, s, (const uint8_t*)src_dev, desc_dev, out_w, out_h, out_dev);
        return hipGetLastError() == hipSuccess ? 0 : 2;
    }
    const long long n_tmp = 3LL * tmp_rows_max * out_w;
    const dim3 grid_tmp((unsigned)((n_tmp + kThreads - 1) / kThreads), (unsigned)batch);
    hipLaunchKernelGGL(resize_h_kernel, grid_tmp, dim3(kThreads), 0, s, (const uint8_t*)src_dev, desc_dev, tables_dev, out_w, tmp_rows_max,
                       (uint8_t*)tmp_dev);
    if (hipGetLastError() != hipSuccess) return 2;
    hipLaunchKernelGGL(resize_v_kernel, grid_out, dim3(kThreads), 0, s, desc_dev, tables_dev, out_w, out_h, tmp_rows_max,
                       (const uint8_t*)tmp_dev, out_dev);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
