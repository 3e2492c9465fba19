// sample.hip — the kernels of text-to-image sampling on the fp16 engine (reference: `Trainer.sample`, finetuning/cars.py:235-255:
// `StableDiffusionPipeline(prompt, negative_prompt, latents, num_inference_steps=50, eta=0.0, guidance_scale=7.5)` on a DDIMScheduler under
// `torch.autocast('cuda')`): the classifier-free-guidance DDIM step in torch's type promotion, the head of the VAE decoder (latent /
// scaling_factor + post_quant_conv) and its tail (GroupNorm affine + SiLU on the way into LDS, conv_out 128 -> 3 on the matrix cores, the
// pipeline's image post-processing from the same registers).
#include "dm_kernels.h"
#include <math.h>

namespace dm {

typedef _Float16 sm_half8 __attribute__((ext_vector_type(8)));
typedef float sm_floatx4 __attribute__((ext_vector_type(4)));

namespace {

inline unsigned sm_grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 * 16 ? 65536 * 16 : g));
}

__device__ __forceinline__ f16 rn16(float v) { return (f16)v; }

// One guided DDIM step with fp32 latents and an fp16 noise prediction, in the type promotion of `StableDiffusionPipeline.__call__` +
// `DDIMScheduler.step` (diffusers 0.24; eta = 0, clip_sample = False; `--mixed_precision no`: the latents stay fp32, the U-Net's output under
// autocast is fp16).  eps [2n]: the unconditional rows first (`torch.cat([negative, prompt])`).  Every elementwise op on fp16 tensors is
// an fp32 operation rounded to fp16; a Python scalar (g) and a 0-dim fp32 tensor (the scheduler's square roots) enter such an op at
// fp32 precision and do not promote its result:
//   e   = rn16(u + rn16(g * rn16(c - u)))                  noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
//   x0  = (x - rn16(c1 * e)) / c2                          fp32 - fp16 -> fp32
//   x'  = c0 * x0 + rn16(c3 * e)                           fp32 + fp16 -> fp32
// coef = one row (c0, c1, c2, c3) = (sqrt(a_prev), sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev)) of the host's table: no square root here.
// x and out carry no __restrict__: the loop runs the step in place (out == x; thread i reads x[i] before it stores out[i]).
__global__ void cfg_ddim_step_kernel(const float* x, const f16* __restrict__ eps, float g, const float* __restrict__ coef, long long n, float* out) {
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float u = (float)eps[i], c = (float)eps[n + i];
        const f16 d = rn16(__fsub_rn(c, u));
        const f16 m = rn16(__fmul_rn(g, (float)d));
        const float e = (float)rn16(__fadd_rn(u, (float)m));
        const f16 p1 = rn16(__fmul_rn(c1, e));
        const float x0 = __fdiv_rn(__fsub_rn(x[i], (float)p1), c2);
        const f16 dir = rn16(__fmul_rn(c3, e));
        out[i] = __fadd_rn(__fmul_rn(c0, x0), (float)dir);
    }
}

// The decoder's head: z = rn16(latent / scaling_factor) (the pipeline divides: a correctly rounded fp32 quotient, then autocast's cast),
// post_quant_conv (1x1, 4 -> 4) with the four exact products added in fp32 in the order i = 0..3, then the bias, rounded to fp16.
// lat NCHW fp32 [B,4,HW] -> out NHWC [B*HW][ldc]: channels 0..3, zeros up to ldc (conv_in reads the row as one 64-channel k step).
__global__ void latent_prologue_kernel(const float* __restrict__ lat, const f16* __restrict__ w, const f16* __restrict__ b, long long total,
                                       int HW, float sf, f16* __restrict__ out, int ldc) {
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= total) return;
    const long long n = pix / HW;
    const int r = (int)(pix - n * HW);
    float z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (float)rn16(__fdiv_rn(lat[((size_t)n * 4 + i) * HW + r], sf));
    sm_half8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = __fadd_rn(acc, __fmul_rn((float)w[c * 4 + i], z[i]));
        o[c] = rn16(__fadd_rn(acc, (float)b[c]));
    }
    sm_half8* dst = reinterpret_cast<sm_half8*>(out + (size_t)pix * ldc);
    dst[0] = o;
    const sm_half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 1; k < ldc / 8; ++k) dst[k] = zero;
}

// The per-(sample, channel) affine of a GroupNorm, y = x * a + b, from the partial sums of launch_gn_stats — the prologue of
// gn_apply_kernel (norm.hip) as a kernel of its own, launched with gn_apply's block size so that the slices, the order of the fp64 sums and
// with them the bits of (a, b) are the ones gn_apply forms.  ab [N][2][C] fp32.  The tail reads 1 KiB per sample instead of every
// block re-adding the `chunks` partial sums (1024 chunks x 32 groups at 512 x 512).
__global__ void gn_affine_kernel(const double* __restrict__ partial, int chunks, int G, int C, double count, float eps,
                                 const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ ab) {
    __shared__ double sh_stat[2 * 64];
    __shared__ double sh_part[2 * 1024];
    const int n = blockIdx.x, t = threadIdx.x;
    const int S = (int)blockDim.x / G, g = t % G, sl = t / G;
    double ds = 0.0, dq = 0.0;
    if (sl < S) {
        const double* in = partial + ((size_t)n * chunks * G + g) * 2;
        for (int c = sl; c < chunks; c += S) { ds += in[(size_t)c * G * 2]; dq += in[(size_t)c * G * 2 + 1]; }
        sh_part[2 * t] = ds; sh_part[2 * t + 1] = dq;
    }
    __syncthreads();
    if (t < G) {
        ds = 0.0; dq = 0.0;
        for (int k = 0; k < S; ++k) { ds += sh_part[2 * (k * G + t)]; dq += sh_part[2 * (k * G + t) + 1]; }
        const double mean = ds / count;
        double var = dq / count - mean * mean;
        var = var > 0.0 ? var : 0.0;
        sh_stat[2 * t] = mean;
        sh_stat[2 * t + 1] = 1.0 / sqrt(var + (double)eps);
    }
    __syncthreads();
    const int cpg = C / G;
    for (int c = t; c < C; c += (int)blockDim.x) {
        const int gc = c / cpg;
        const double ad = sh_stat[2 * gc + 1] * (double)gamma[c];
        ab[((size_t)n * 2 + 0) * C + c] = (float)ad;
        ab[((size_t)n * 2 + 1) * C + c] = (float)((double)beta[c] - sh_stat[2 * gc] * ad);
    }
}

// The decoder's tail.  The input of conv_out, [B,H,W,128] fp16, is the largest tensor of the path (67 MB per 512 x 512 image) and one
// 3-channel convolution reads it: its normalised copy is never written.  A block owns a tile of 8 x 16 output pixels of one sample:
//   * the 10 x 18 patch (one halo pixel all round) goes to LDS NORMALISED: fmaf(x, a, b), SiLU, rounded to fp16 — the expression and
//     the rounding point of gn_apply_kernel(silu), so the fused and the two-kernel path differ by the order of conv_out's fp32 sums only;
//     pixels outside the image are the convolution's zero padding.  An LDS row is one pixel (256 bytes = 16 chunks of 8 channels), chunk
//     q of row R at slot q ^ (R & 15): the 16 pixels of a B-fragment read, 16 consecutive rows, spread over all 64 banks.  Thread t
//     always handles chunk t & 15, so its eight (a, b) pairs stay in registers; 16 threads read one pixel's 256 contiguous bytes;
//   * the three output channels are rows 0..2 of a 16x16x32 MFMA's A operand (lanes of rows 3..15 hold zeros; the layer's weights,
//     6.9 KB, sit in LDS), sixteen pixels of one image row its columns: tap (dy, dx) of a pixel is the same B-fragment read shifted by
//     dy * 18 + dx LDS rows.  Wave w owns rows 2 w, 2 w + 1 of the tile: 2 x 36 MFMAs.  The sum runs tap 0..8, then 32-channel block
//     0..3 inside a tap, for every pixel alike: its bits depend on its own 3 x 3 x 128 inputs and on nothing else (not on the batch,
//     the tile it falls in or its neighbours);
//   * lanes 0..15 end with the channels of their pixel: + bias, fp16 = the raw sample (NCHW), and `VaeImageProcessor.postprocess`
//     op by op — (raw / 2 + 0.5).clamp(0, 1) in fp16, each operation rounded, widened to fp32, * 255, rounded half to even — as uint8
//     NHWC.  A NaN sample stays NaN in the raw output; its uint8 value, which numpy leaves undefined, is 0 here.
constexpr int DT_C = DEC_TAIL_C, DT_TH = 8, DT_TW = 16, DT_PH = DT_TH + 2, DT_PW = DT_TW + 2, DT_NPIX = DT_PH * DT_PW, DT_K = 9 * DT_C;
__global__ __launch_bounds__(256) void decoder_tail16_kernel(const f16* __restrict__ X, const float* __restrict__ ab, const f16* __restrict__ Wp,
                                                             const f16* __restrict__ bias, int H, int W, f16* __restrict__ raw,
                                                             uint8_t* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) char xs[DT_NPIX * DT_C * 2];
    __shared__ __attribute__((aligned(16))) char ws[3 * DT_K * 2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = blockIdx.z, oy0 = blockIdx.y * DT_TH, ox0 = blockIdx.x * DT_TW;
    for (int i = tid * 8; i < 3 * DT_K; i += 256 * 8)
        *reinterpret_cast<sm_half8*>(ws + i * 2) = *reinterpret_cast<const sm_half8*>(Wp + i);
    const int q = tid & 15, c8 = q * 8;
    float a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { a[k] = ab[((size_t)n * 2 + 0) * DT_C + c8 + k]; b[k] = ab[((size_t)n * 2 + 1) * DT_C + c8 + k]; }
    for (int R0 = tid >> 4; R0 < DT_NPIX; R0 += 64) {
        sm_half8 v[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {           // four independent loads in flight per thread
            const int R = R0 + 16 * u;
            const int py = R / DT_PW, px = R - py * DT_PW;
            const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
            ok[u] = R < DT_NPIX && iy >= 0 && iy < H && ix >= 0 && ix < W;
            v[u] = sm_half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) v[u] = *reinterpret_cast<const sm_half8*>(X + (((size_t)n * H + iy) * W + ix) * DT_C + c8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int R = R0 + 16 * u;
            if (R >= DT_NPIX) continue;
            sm_half8 o = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float y = fmaf((float)v[u][k], a[k], b[k]);
                    y = y / (1.0f + __expf(-y));
                    o[k] = (f16)y;
                }
            }
            *reinterpret_cast<sm_half8*>(xs + R * (DT_C * 2) + ((q ^ (R & 15)) << 4)) = o;
        }
    }
    __syncthreads();

    const int l15 = lane & 15, kg = lane >> 4;
    int r0[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) r0[f] = (wid * 2 + f) * DT_PW + l15;
    sm_floatx4 acc[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[f] = sm_floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            sm_half8 wa = sm_half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (l15 < 3) wa = *reinterpret_cast<const sm_half8*>(ws + ((l15 * DT_K + tap * DT_C + ks * 32 + kg * 8) << 1));
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const int R = r0[f] + dy * DT_PW + dx;
                const sm_half8 bv = *reinterpret_cast<const sm_half8*>(xs + R * (DT_C * 2) + (((ks * 4 + kg) ^ (R & 15)) << 4));
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, bv, acc[f], 0, 0, 0);
            }
        }
    }

    if (kg == 0) {
        float bs[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) bs[r] = (float)bias[r];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int oy = oy0 + wid * 2 + f, ox = ox0 + l15;
            if (oy < H && ox < W) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const f16 pr = (f16)__fadd_rn(acc[f][r], bs[r]);
                    if (raw) raw[(((size_t)n * 3 + r) * H + oy) * W + ox] = pr;
                    if (img) {
                        f16 t = (f16)__fadd_rn((float)(f16)__fdiv_rn((float)pr, 2.0f), 0.5f);
                        const bool nan = !(t == t);
                        t = t < (f16)0.f ? (f16)0.f : (t > (f16)1.f ? (f16)1.f : t);
                        img[(((size_t)n * H + oy) * W + ox) * 3 + r] = nan ? (uint8_t)0 : (uint8_t)(int)rintf(__fmul_rn((float)t, 255.0f));
                    }
                }
            }
        }
    }
}

}  // namespace

hipError_t launch_cfg_ddim_step(const float* x, const f16* eps, float g, const float* coef, long long n, float* out, hipStream_t s) {
    if (!x || !eps || !coef || !out || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cfg_ddim_step_kernel, dim3(sm_grid_for(n)), dim3(256), 0, s, x, eps, g, coef, n, out);
    return hipGetLastError();
}

hipError_t launch_latent_prologue(const float* lat, const f16* w, const f16* b, int B, int HW, float sf, f16* out, int ldc, hipStream_t s) {
    const long long total = (long long)B * HW;
    if (!lat || !w || !b || !out || total <= 0 || ldc < 8 || ldc % 8 || !(sf > 0.f) || (total + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(latent_prologue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, lat, w, b, total, HW, sf, out, ldc);
    return hipGetLastError();
}

hipError_t launch_gn_affine(const double* partial, int N, int HW, int C, int G, float eps, const float* gamma, const float* beta, float* ab,
                            hipStream_t s) {
    if (!partial || !gamma || !beta || !ab || N <= 0 || HW <= 0 || C % 8 || C % G || G > 64) return hipErrorInvalidValue;
    const int threads = gn_apply_threads(C, G);
    if (threads > 1024 || threads < G) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_affine_kernel, dim3(N), dim3(threads), 0, s, partial, gn_stats_chunks(HW), G, C, (double)HW * (double)(C / G), eps,
                       gamma, beta, ab);
    return hipGetLastError();
}

hipError_t launch_decoder_tail(const f16* X, const float* ab, const f16* Wp, const f16* bias, int B, int H, int W, int C, f16* raw, uint8_t* img,
                               hipStream_t s) {
    if (!X || !ab || !Wp || !bias || C != DT_C || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H + DT_TH - 1) / DT_TH > 65535 || (!raw && !img))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_tail16_kernel, dim3((W + DT_TW - 1) / DT_TW, (H + DT_TH - 1) / DT_TH, B), dim3(256), 0, s, X, ab, Wp, bias, H, W,
                       raw, img);
    return hipGetLastError();
}

}  // namespace dm
