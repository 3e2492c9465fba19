// clip_vision.hip — the glue kernels of the fp32 CLIP ViT-B/32 image tower (dm_f32_clip_image_features, f32_clip_nets.hip): the
// processor's preprocessing, patch rows, token assembly, the CLS gather and the L2 normalisation (the attention over the 50
// tokens is the text tower's kernel without the mask, f32_ops.hip).  Every GEMM of the tower (patch embedding, q|k|v, out_proj,
// fc1, fc2, visual_projection) runs on gemm32.  Below them, with (size, patch) as launch parameters, the glue of the configurable
// tower (dm_f32_clip_tower_*; CLIP ViT-L/14-336 of the CLIP baseline) and the text embeddings' pooling gather.
//
// Preprocessing = `CLIPImageProcessor` (PIL backend) of `Cluster.embed` (cluster.py:224-231) on uint8 HWC RGB crops:
//   * BICUBIC shortest-edge resize: PIL's 8-bit two-pass resampler (horizontal first, 8-bit intermediate, int32 accumulators
//     seeded with 1 << 21, >> 22, clamp to [0, 255]); a pass whose axis keeps its size is skipped, as PIL's need_horizontal /
//     need_vertical do.  The tables (resample.bicubic_axis, built on the host by PIL's float64 formula) cover only the 224
//     columns / rows the center crop keeps.  One thread per output value recomputes the intermediate values its vertical window
//     reads: integer arithmetic, so recomputing gives the bytes PIL's stored intermediate holds.
//   * rescale `(uint8.astype(float64) * (1 / 255)).astype(float32)` (the multiply in double) and normalise `(x - mean) / std` in
//     fp32 with an IEEE division (hipcc's default division; the build has -ffp-contract=off, so nothing is fused).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "f32_kernels.h"
#include "../../include/dm_engine.h"

namespace dm32 {
namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;        // PIL Resample.c PRECISION_BITS
constexpr int kThreads = 256;
constexpr int S = 224, PS = 32, GRID = S / PS, NPATCH = GRID * GRID, KP = 3 * PS * PS;     // 224 px, 7 x 7 patches of 3 x 32 x 32
constexpr int VT = NPATCH + 1;                    // 50 tokens

__device__ __forceinline__ int clip8(int v) {
    v >>= kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one value of the horizontal pass: crop row `row` (relative to the crop), output column x of the kept window
__device__ __forceinline__ int hpass(const uint8_t* img, const dm_clip_pre_desc& d, const int32_t* tables, int row, int x, int c) {
    const uint8_t* src = img + ((long long)(d.crop_row0 + row) * d.src_w + d.crop_col0) * 3 + c;
    if (!(d.flags & DM_CLIP_NEED_H)) return src[(d.left + x) * 3];
    const int xmin = tables[d.xb_off + 2 * x], xn = tables[d.xb_off + 2 * x + 1];
    const int32_t* k = tables + d.xk_off + (long long)x * d.kx;
    int ss = 1 << (kPrecisionBits - 1);
    if (xmin >= 0 && xn <= d.kx && xmin + xn <= d.crop_w)
        for (int t = 0; t < xn; ++t) ss += (int)src[(xmin + t) * 3] * k[t];
    return clip8(ss);
}

// layout 0: pixel_values [P][3][224][224]; layout 1: patch rows [P * 49][3 * 32 * 32], row = patch (py * 7 + px), k = (c, ky, kx)
__global__ void __launch_bounds__(kThreads) clip_pre_kernel(const uint8_t* __restrict__ images, const dm_clip_pre_desc* __restrict__ desc,
                                                            const int32_t* __restrict__ tables, int layout, float* __restrict__ out) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= 3 * S * S) return;
    const dm_clip_pre_desc d = desc[p];
    const int x = i % S, y = (i / S) % S, c = i / (S * S);
    // the host checked every descriptor; this guard only keeps a corrupt one from reading outside its image
    const bool ok = d.crop_row0 >= 0 && d.crop_col0 >= 0 && d.crop_w >= 1 && d.crop_h >= 1 && d.crop_col0 + d.crop_w <= d.src_w &&
                    d.crop_row0 + d.crop_h <= d.src_h && ((d.flags & DM_CLIP_NEED_H) || d.left + S <= d.crop_w) &&
                    ((d.flags & DM_CLIP_NEED_V) || d.top + S <= d.crop_h);
    int v = 0;
    if (ok) {
        const uint8_t* img = images + d.src_offset;
        if (d.flags & DM_CLIP_NEED_V) {
            const int ymin = tables[d.yb_off + 2 * y], yn = tables[d.yb_off + 2 * y + 1];
            const int32_t* k = tables + d.yk_off + (long long)y * d.ky;
            int ss = 1 << (kPrecisionBits - 1);
            if (ymin >= 0 && yn <= d.ky && ymin + yn <= d.crop_h)
                for (int t = 0; t < yn; ++t) ss += hpass(img, d, tables, ymin + t, x, c) * k[t];
            v = clip8(ss);
        } else {
            v = hpass(img, d, tables, d.top + y, x, c);
        }
    }
    // OPENAI_CLIP_MEAN / OPENAI_CLIP_STD: the double literals rounded to fp32 once, as np.array(mean, dtype=float32) does
    const float mean = c == 0 ? (float)0.48145466 : (c == 1 ? (float)0.4578275 : (float)0.40821073);
    const float stdv = c == 0 ? (float)0.26862954 : (c == 1 ? (float)0.26130258 : (float)0.27577711);
    const float r = (float)((double)v * (1.0 / 255.0));
    const float o = (r - mean) / stdv;
    if (layout == 0) {
        out[(size_t)p * 3 * S * S + i] = o;
    } else {
        const int row = (y / PS) * GRID + x / PS, k = (c * PS + y % PS) * PS + x % PS;
        out[((size_t)p * NPATCH + row) * KP + k] = o;
    }
}

// pixel_values [P][3][224][224] -> patch rows [P * 49][3072] (the stride-32 convolution as a dense GEMM over these rows)
__global__ void __launch_bounds__(kThreads) clip_patchify_kernel(const float* __restrict__ pix, long long total, float* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % S), y = (int)((i / S) % S), c = (int)((i / (S * S)) % 3);
    const long long p = i / (3LL * S * S);
    const int row = (y / PS) * GRID + x / PS, k = (c * PS + y % PS) * PS + x % PS;
    rows[(p * NPATCH + row) * KP + k] = pix[i];
}

// CLIPVisionEmbeddings: token 0 = class_embedding, tokens 1..49 = the patch embeddings; + position_embedding
__global__ void __launch_bounds__(kThreads) clip_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, int n, int C, float* __restrict__ x) {
    const int row = blockIdx.x;                    // p * 50 + t
    const int p = row / VT, t = row - p * VT;
    const float* a = t == 0 ? cls : pe + ((size_t)p * NPATCH + t - 1) * C;
    const float* b = pos + (size_t)t * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) x[(size_t)row * C + c] = a[c] + b[c];
}

// last_hidden_state[:, 0, :] -> [n][C] (post_layernorm runs on these rows)
__global__ void __launch_bounds__(kThreads) clip_cls_kernel(const float* __restrict__ x, int C, float* __restrict__ y) {
    const int p = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) y[(size_t)p * C + c] = x[(size_t)p * VT * C + c];
}

// features / features.norm(dim=-1, keepdim=True): one wave per row
__global__ void __launch_bounds__(64) clip_l2norm_kernel(const float* __restrict__ x, int C, float* __restrict__ y) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* a = x + (size_t)row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += a[c] * a[c];
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
    const float nrm = sqrtf(s);
    for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = a[c] / nrm;
}

// ---- the configurable tower (CLIP ViT-L/14-336 of the CLIP baseline, clipmining/ranking.py:58-70): any (image size S, patch PS) -------
// The processor there has do_center_crop = False and the engine takes square images only, so the BICUBIC shortest-edge resize maps the
// whole s x s image onto S x S: left = top = 0 and the tables cover every output column / row.  Same integer passes as clip_pre_kernel.
__device__ __forceinline__ float tower_pixel(const uint8_t* __restrict__ images, const dm_clip_pre_desc& d, const int32_t* __restrict__ tables,
                                             int S, int x, int y, int c) {
    const bool ok = d.crop_row0 >= 0 && d.crop_col0 >= 0 && d.crop_w >= 1 && d.crop_h >= 1 && d.crop_col0 + d.crop_w <= d.src_w &&
                    d.crop_row0 + d.crop_h <= d.src_h && d.left >= 0 && d.top >= 0 && ((d.flags & DM_CLIP_NEED_H) || d.left + S <= d.crop_w) &&
                    ((d.flags & DM_CLIP_NEED_V) || d.top + S <= d.crop_h);
    int v = 0;
    if (ok) {
        const uint8_t* img = images + d.src_offset;
        if (d.flags & DM_CLIP_NEED_V) {
            const int ymin = tables[d.yb_off + 2 * y], yn = tables[d.yb_off + 2 * y + 1];
            const int32_t* k = tables + d.yk_off + (long long)y * d.ky;
            int ss = 1 << (kPrecisionBits - 1);
            if (ymin >= 0 && yn <= d.ky && ymin + yn <= d.crop_h)
                for (int t = 0; t < yn; ++t) ss += hpass(img, d, tables, ymin + t, x, c) * k[t];
            v = clip8(ss);
        } else {
            v = hpass(img, d, tables, d.top + y, x, c);
        }
    }
    const float mean = c == 0 ? (float)0.48145466 : (c == 1 ? (float)0.4578275 : (float)0.40821073);
    const float stdv = c == 0 ? (float)0.26862954 : (c == 1 ? (float)0.26130258 : (float)0.27577711);
    const float r = (float)((double)v * (1.0 / 255.0));
    return (r - mean) / stdv;
}

// patch-row element i of an image -> (x, y, c) of the pixel it holds, or c = -1 for a padding column k >= 3 PS PS;
// row = patch (py * G + px), k = (c, ky, kx): the k order of patch_embedding.weight [hidden][3][PS][PS]
__device__ __forceinline__ void tower_row_elem(int i, int S, int PS, int KPAD, int* x, int* y, int* c) {
    const int G = S / PS, row = i / KPAD, k = i - row * KPAD;
    if (k >= 3 * PS * PS) { *c = -1; *x = 0; *y = 0; return; }
    const int kx = k % PS, ky = (k / PS) % PS;
    *c = k / (PS * PS);
    *y = (row / G) * PS + ky;
    *x = (row % G) * PS + kx;
}

// layout 0: pixel_values [n][3][S][S] (per = 3 S S); layout 1: patch rows [n * G^2][KPAD] (per = G^2 KPAD), columns 3 PS PS .. KPAD - 1
// written as zeros (the packed weight has zero columns there: a + 0 * 0 term changes no fp32 sum)
__global__ void __launch_bounds__(kThreads) clip_tower_pre_kernel(const uint8_t* __restrict__ images, const dm_clip_pre_desc* __restrict__ desc,
                                                                  const int32_t* __restrict__ tables, int S, int PS, int KPAD, int layout, int per,
                                                                  float* __restrict__ out) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= per) return;
    int x, y, c;
    if (layout == 0) { x = i % S; y = (i / S) % S; c = i / (S * S); }
    else tower_row_elem(i, S, PS, KPAD, &x, &y, &c);
    float o = 0.f;
    if (c >= 0) o = tower_pixel(images, desc[p], tables, S, x, y, c);
    out[(size_t)p * per + i] = o;
}

// pixel_values [n][3][S][S] -> patch rows [n * G^2][KPAD], one thread per element of the rows (padding columns = 0)
__global__ void __launch_bounds__(kThreads) clip_tower_patchify_kernel(const float* __restrict__ pix, int S, int PS, int KPAD, int per,
                                                                       float* __restrict__ rows) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= per) return;
    int x, y, c;
    tower_row_elem(i, S, PS, KPAD, &x, &y, &c);
    rows[(size_t)p * per + i] = c < 0 ? 0.f : pix[(((size_t)p * 3 + c) * S + y) * S + x];
}

// CLIPVisionEmbeddings for T = G^2 + 1 tokens: token 0 = class_embedding, tokens 1..G^2 = the patch embeddings; + position_embedding
__global__ void __launch_bounds__(kThreads) clip_tower_tokens_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                                     const float* __restrict__ pos, int T, int C, float* __restrict__ x) {
    const int row = blockIdx.x;                    // p * T + t
    const int p = row / T, t = row - p * T;
    const float* a = t == 0 ? cls : pe + ((size_t)p * (T - 1) + t - 1) * C;
    const float* b = pos + (size_t)t * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) x[(size_t)row * C + c] = a[c] + b[c];
}

// post_layernorm on last_hidden_state[:, 1:, :]: X [n][T][C] -> Y [n * (T - 1)][C] dense, the CLS rows skipped; one wave per output
// row, two-pass statistics in ln32_kernel's order (f32_ops.hip)
__global__ void __launch_bounds__(kThreads) clip_tower_patch_ln_kernel(const float* __restrict__ X, long long rows, int T, int C,
                                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                       float* __restrict__ Y) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long long p = row / (T - 1);
    const int t = (int)(row - p * (T - 1)) + 1;
    const float* x = X + (p * T + t) * C;
    float s = 0.f;
    for (int i = lane; i < C; i += 64) s += x[i];
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
    const float mean = s / (float)C;
    float q = 0.f;
    for (int i = lane; i < C; i += 64) { const float d = x[i] - mean; q += d * d; }
    for (int w = 32; w > 0; w >>= 1) q += __shfl_xor(q, w);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    float* y = Y + row * C;
    for (int i = lane; i < C; i += 64) y[i] = (x[i] - mean) * rstd * gamma[i] + beta[i];
}

// CLIPTextModelWithProjection's pooling: the hidden row at argmax(input_ids) (torch.argmax = the FIRST maximum = the EOS position)
__global__ void __launch_bounds__(kThreads) clip_eos_gather_kernel(const int32_t* __restrict__ ids, const float* __restrict__ hidden, int T, int C,
                                                                   float* __restrict__ y) {
    const int p = blockIdx.x;
    int best = 0, at = 0;
    for (int t = 0; t < T; ++t) { const int v = ids[(size_t)p * T + t]; if (t == 0 || v > best) { best = v; at = t; } }
    const float* a = hidden + ((size_t)p * T + at) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) y[(size_t)p * C + c] = a[c];
}

}  // namespace

hipError_t launch_clip_tower_preprocess(const uint8_t* images, const dm_clip_pre_desc* desc, const int32_t* tables, int n, int S, int PS, int KPAD,
                                        int layout, float* out, hipStream_t s) {
    if (n < 1 || n > 65535 || (layout != 0 && layout != 1) || S < 1 || PS < 1 || S % PS != 0 || KPAD < 3 * PS * PS) return hipErrorInvalidValue;
    const long long per = layout == 0 ? 3LL * S * S : (long long)(S / PS) * (S / PS) * KPAD;
    if (per >= (1LL << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_tower_pre_kernel, dim3((unsigned)((per + kThreads - 1) / kThreads), n), dim3(kThreads), 0, s, images, desc, tables, S, PS,
                       KPAD, layout, (int)per, out);
    return hipGetLastError();
}

hipError_t launch_clip_tower_patchify(const float* pix, int n, int S, int PS, int KPAD, float* rows, hipStream_t s) {
    if (n < 1 || n > 65535 || S < 1 || PS < 1 || S % PS != 0 || KPAD < 3 * PS * PS) return hipErrorInvalidValue;
    const long long per = (long long)(S / PS) * (S / PS) * KPAD;
    if (per >= (1LL << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_tower_patchify_kernel, dim3((unsigned)((per + kThreads - 1) / kThreads), n), dim3(kThreads), 0, s, pix, S, PS, KPAD,
                       (int)per, rows);
    return hipGetLastError();
}

hipError_t launch_clip_tower_tokens(const float* pe, const float* cls, const float* pos, int n, int T, int C, float* x, hipStream_t s) {
    if (n < 1 || T < 2 || (long long)n * T >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_tower_tokens_kernel, dim3((unsigned)(n * T)), dim3(kThreads), 0, s, pe, cls, pos, T, C, x);
    return hipGetLastError();
}

hipError_t launch_clip_tower_patch_ln(const float* X, int n, int T, int C, const float* gamma, const float* beta, float eps, float* Y, hipStream_t s) {
    if (n < 1 || T < 2 || C < 1) return hipErrorInvalidValue;
    const long long rows = (long long)n * (T - 1);
    if ((rows + 3) / 4 >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_tower_patch_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kThreads), 0, s, X, rows, T, C, gamma, beta, eps, Y);
    return hipGetLastError();
}

hipError_t launch_clip_eos_gather(const int32_t* ids, const float* hidden, int n, int T, int C, float* y, hipStream_t s) {
    if (n < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_eos_gather_kernel, dim3(n), dim3(kThreads), 0, s, ids, hidden, T, C, y);
    return hipGetLastError();
}

hipError_t launch_clip_preprocess(const uint8_t* images, const dm_clip_pre_desc* desc, const int32_t* tables, int n, int layout, float* out,
                                  hipStream_t s) {
    if (n < 1 || n > 65535 || (layout != 0 && layout != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_pre_kernel, dim3((3 * S * S + kThreads - 1) / kThreads, n), dim3(kThreads), 0, s, images, desc, tables, layout, out);
    return hipGetLastError();
}

hipError_t launch_clip_patchify(const float* pix, int n, float* rows, hipStream_t s) {
    const long long total = 3LL * S * S * n;
    hipLaunchKernelGGL(clip_patchify_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, pix, total, rows);
    return hipGetLastError();
}

hipError_t launch_clip_tokens(const float* pe, const float* cls, const float* pos, int n, int C, float* x, hipStream_t s) {
    hipLaunchKernelGGL(clip_tokens_kernel, dim3(n * VT), dim3(kThreads), 0, s, pe, cls, pos, n, C, x);
    return hipGetLastError();
}

hipError_t launch_clip_cls(const float* x, int n, int C, float* y, hipStream_t s) {
    hipLaunchKernelGGL(clip_cls_kernel, dim3(n), dim3(kThreads), 0, s, x, C, y);
    return hipGetLastError();
}

hipError_t launch_clip_l2norm(const float* x, int n, int C, float* y, hipStream_t s) {
    hipLaunchKernelGGL(clip_l2norm_kernel, dim3(n), dim3(64), 0, s, x, C, y);
    return hipGetLastError();
}

}  // namespace dm32
