// pnp.hip — the kernels of the parallel-dataset generator (reference: diffmining/applications/parallel-dataset/pnp.py) on the fp32 net:
// the DDIM update (inversion, reconstruction and DDIMScheduler.step are one expression with four scalars), its classifier-free-guidance
// form, the broadcast add of Plug-and-Play's feature injection, the head of the VAE decoder (latent scale + post_quant_conv) and its tail
// (GroupNorm affine + SiLU while loading, conv_out 128 -> 3, the image post-processing from the same registers).  All fp32.
#include "f32_kernels.h"
#include <math.h>

namespace dm32 {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

inline unsigned grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 * 16 ? 65536 * 16 : g));
}

// x' = c0 * ((x - c1 * eps) / c2) + c3 * eps, every operation rounded on its own (torch's elementwise kernels do not contract; pnp.py:176-177,
// :200-201 and DDIMScheduler.step with eta = 0, clip_sample = False).  CFG: eps = eps_u + g * (eps_c - eps_u) first (pnp.py:553-554).
// coef = one row (c0, c1, c2, c3) of the host's table: the device computes no square root.
template <bool CFG>
__global__ void ddim_step32_kernel(const float* x, const float* eps_u, const float* eps_c, float g, const float* coef, long long n, float* out) {
    const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float eps = eps_u[i];
        if (CFG) eps = __fadd_rn(eps, __fmul_rn(g, __fsub_rn(eps_c[i], eps)));
        const float x0 = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(c1, eps)), c2);
        out[i] = __fadd_rn(__fmul_rn(c0, x0), __fmul_rn(c3, eps));
    }
}

// Y[b] = R[b] + Hs for the samples b = 0 .. B-1 of R: `input_tensor + hidden_states` (pnp.py:357) with the source's hidden_states in
// every row (pnp.py:348-350); per = elements per sample
__global__ void bcast_add32_kernel(const float* R, const float* Hs, int B, long long per, float* Y) {
    const long long per4 = per / 4, total = (long long)B * per4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i % per4;
        const v4f a = *reinterpret_cast<const v4f*>(R + 4 * i), h = *reinterpret_cast<const v4f*>(Hs + 4 * r);
        *reinterpret_cast<v4f*>(Y + 4 * i) = a + h;
    }
}

// z = post_quant_conv(latent * scale): 1x1, 4 -> 4, NCHW in and out (pnp.py:139-140 / :533-534; `1 / 0.18215 * latents` is an fp32 product)
__global__ void decoder_head32_kernel(const float* lat, const float* w, const float* b, int B, int HW, float scale, float* z) {
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (long long)B * HW) return;
    const int n = (int)(pix / HW), r = (int)(pix - (long long)n * HW);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lat[((size_t)n * 4 + i) * HW + r] * scale;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += w[o * 4 + i] * v[i];
        z[((size_t)n * 4 + o) * HW + r] = acc + b[o];
    }
}

// The decoder's tail.  The input of conv_out is the largest tensor of the pipeline (134 MB per 512 x 512 image) and is read by one
// 3-channel convolution: it is never written.  One block = an 8 x 8 tile of output pixels.  The 10 x 10 x 128 input patch goes to LDS
// normalised: (x - mean) * rstd * gamma + beta, SiLU — the expression of gn32_apply_kernel, so the fused and the two-kernel path differ
// in the convolution's summation order only; pixels outside the image are the convolution's zero padding.  Pixel pitch 129 floats (odd, so
// the 64 lanes of a wave, which read one channel of 64 different pixels, spread over the banks; the tile's pixel indices run 0 .. 77 of the
// 10-wide patch, so about a dozen lanes still meet two-way).  Wave q sums channels 32 q .. 32 q + 31 of all nine taps for the
// tile's 64 pixels (lane = pixel); q is wave-uniform, so the weights come through the scalar cache.  The four partial sums meet in LDS
// and are added in the fixed order q = 0 .. 3, + bias.  Post-processing op by op (pnp.py:141: `(imgs / 2 + 0.5).clamp(0, 1)`; :591: `(x * 255)
// .astype(np.uint8)` truncates), each rounded on its own: torch's bits for every finite sample.  A NaN sample stays NaN in the fp32
// outputs, as torch's clamp leaves it; its uint8 value, which numpy leaves undefined, is 0 here.
constexpr int TC = 128, TG = 32, TT = 8, TP = TT + 2, TPITCH = TC + 1;
__global__ __launch_bounds__(256) void decoder_tail32_kernel(const float* __restrict__ X, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ Wp, const float* __restrict__ bias,
                                                             int H, int W, int raw, float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
    __shared__ float patch[TP * TP * TPITCH];
    __shared__ float part[4][3][64];
    const int tid = threadIdx.x, n = blockIdx.z, oy0 = blockIdx.y * TT, ox0 = blockIdx.x * TT;
    for (int i = tid; i < TP * TP * (TC / 4); i += 256) {
        const int px = i / (TC / 4), c4 = i - px * (TC / 4);       // cpg = 4: a float4 is one group
        const int iy = oy0 - 1 + px / TP, ix = ox0 - 1 + px % TP;
        v4f y = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const v4f x = *reinterpret_cast<const v4f*>(X + (((long long)n * H + iy) * W + ix) * TC + 4 * c4);
            const float mean = stats[2 * (n * TG + c4)], rstd = stats[2 * (n * TG + c4) + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = (x[j] - mean) * rstd * gamma[4 * c4 + j] + beta[4 * c4 + j];
                y[j] = v / (1.0f + expf(-v));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) patch[px * TPITCH + 4 * c4 + j] = y[j];
    }
    __syncthreads();
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, ly = lane >> 3, lx = lane & 7;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int tap = 0; tap < 9; ++tap) {
        const float* pr = patch + ((ly + tap / 3) * TP + lx + tap % 3) * TPITCH + 32 * q;
        const float* w0 = Wp + tap * TC + 32 * q;
#pragma unroll 8
        for (int c = 0; c < 32; ++c) {
            const float v = pr[c];
            acc[0] += v * w0[c];
            acc[1] += v * w0[9 * TC + c];
            acc[2] += v * w0[18 * TC + c];
        }
    }
#pragma unroll
    for (int co = 0; co < 3; ++co) part[q][co][lane] = acc[co];
    __syncthreads();
    if (tid >= 64) return;
    const int oy = oy0 + ly, ox = ox0 + lx;
    if (oy >= H || ox >= W) return;
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        const float v = ((part[0][co][lane] + part[1][co][lane]) + part[2][co][lane]) + part[3][co][lane] + bias[co];
        float img = __fadd_rn(__fdiv_rn(v, 2.0f), 0.5f);
        img = img < 0.f ? 0.f : (img > 1.f ? 1.f : img);
        if (out_f32) out_f32[(((long long)n * 3 + co) * H + oy) * W + ox] = raw ? v : img;
        if (out_u8) out_u8[(((long long)n * H + oy) * W + ox) * 3 + co] = img == img ? (uint8_t)(int)__fmul_rn(img, 255.0f) : (uint8_t)0;
    }
}

}  // namespace

hipError_t launch_ddim_step(const float* x, const float* eps_u, const float* eps_c, float g, const float* coef, long long n, float* out, hipStream_t s) {
    if (!x || !eps_u || !coef || !out || n <= 0) return hipErrorInvalidValue;
    if (eps_c) hipLaunchKernelGGL(ddim_step32_kernel<true>, dim3(grid_for(n)), dim3(256), 0, s, x, eps_u, eps_c, g, coef, n, out);
    else hipLaunchKernelGGL(ddim_step32_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, x, eps_u, eps_c, g, coef, n, out);
    return hipGetLastError();
}
hipError_t launch_bcast_add(const float* R, const float* Hs, int B, long long per, float* Y, hipStream_t s) {
    if (B <= 0 || per <= 0 || per % 4 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bcast_add32_kernel, dim3(grid_for((long long)B * (per / 4))), dim3(256), 0, s, R, Hs, B, per, Y);
    return hipGetLastError();
}
hipError_t launch_decoder_head(const float* lat, const float* w, const float* b, int B, int HW, float scale, float* z, hipStream_t s) {
    const long long total = (long long)B * HW;
    if (total <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_head32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, lat, w, b, B, HW, scale, z);
    return hipGetLastError();
}
hipError_t launch_decoder_tail(const float* X, const float* stats, const float* gamma, const float* beta, const float* Wp, const float* bias, int B,
                               int H, int W, int C, int raw, float* out_f32, uint8_t* out_u8, hipStream_t s) {
    if (C != TC || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (H + TT - 1) / TT > 65535 || (!out_f32 && !out_u8)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_tail32_kernel, dim3((W + TT - 1) / TT, (H + TT - 1) / TT, B), dim3(256), 0, s, X, stats, gamma, beta, Wp, bias, H, W, raw,
                       out_f32, out_u8);
    return hipGetLastError();
}

}  // namespace dm32
