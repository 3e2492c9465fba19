// f32_train.hip — the gradient kernels of the fp32 net's convolutional blocks (ResnetBlock2D, Downsample2D, Upsample2D), gfx950.
//
// Only what has no forward counterpart lives here.  The DATA gradient of every convolution / linear layer is gemm32 itself on
// repacked weights (train.py: dgrad_weights); this file holds
//   wgrad32        dWp[co][tap Cin + ci] = sum over output pixels of dY[pixel][co] * im2col(X)[pixel][tap][ci]  (fp32 MFMA 32x32x2)
//   colsum32       dbias / the per-sample sums that flow into time_emb_proj
//   gn32_bwd_*     GroupNorm (+ SiLU) backward over one or two concatenated sources, from the forward pass's (mean, rstd)
//   silu_bwd, zero_insert2 (stride-2 data gradient -> a mode-1 convolution), nearest_bwd (up-sampler's data gradient)
// and, for the transformer blocks (whose attention backward is f32_train_attn.hip),
//   ln32_bwd_*     LayerNorm backward, mean / rstd recomputed per row; dgamma / dbeta over row slabs in fp64
//   geglu32, geglu32_bwd   the unfused GEGLU of the training forward pass and its gradient
// Every sum has a fixed order: no floating-point atomics, the same bits from run to run.
//
// wgrad32.  The reduction runs over PIXELS; both operands lie pixel-major in NHWC (dY [pixel][Cout], X [pixel][Cin]), so one LDS
// stage of [32 pixels][channels] feeds both MFMA fragments without a transpose: A lane (c32, h32) = dY[pixel 2 kk + h32][co c32],
// B = X[pixel 2 kk + h32][ci c32], D[co][ci] as in f32_gemm.hip (registers 4 q .. 4 q + 3 = rows 8 q + 4 h32 .. + 3 of column c32).
// Block = 4 waves, tile = 128 output channels x 2 column chunks of 32 (a column chunk = 32 consecutive k = (tap, ci) of the packed
// weight row: Cin % 32 == 0 and C1 % 32 == 0, so a chunk has one tap and one source); wave w = channels 32 w .. + 31 x both chunks.
// The pixels are cut into `slabs` (wgrad_slabs: a function of the pixel count alone) across blockIdx.z; slab s writes its partial
// tile to work[s][Cout][K], and wgrad32_reduce_kernel adds the slabs in ascending order (+ what dWp holds, when accumulate).
#include "f32_kernels.h"

namespace dm32 {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int WG_CO = 128, WG_PX = 32, WG_NT = 256, WG_NC = 2;      // column chunks of 32 per block (4 measured slower at the 64^2 level: 164 VGPRs, fewer blocks per CU)

struct WgradParams {
    const float* X; const float* X2; const float* dY; float* work;
    int M, Cout, Cin, C1, H, W, OH, OW, mode, K, slab_len;
};

__global__ __launch_bounds__(WG_NT) void wgrad32_kernel(WgradParams p) {
    __shared__ __attribute__((aligned(16))) float Ds[WG_PX][WG_CO];
    __shared__ __attribute__((aligned(16))) float Xs[WG_NC][WG_PX][32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c32 = lane & 31, h32 = lane >> 5;
    const int co0 = blockIdx.y * WG_CO;
    const int nchunks = p.K / 32;
    const int p_begin = blockIdx.z * p.slab_len;
    const int p_end = min(p.M, p_begin + p.slab_len);
    const int OHW = p.OH * p.OW;
    const float sh = (float)p.H / (float)p.OH, sw = (float)p.W / (float)p.OW;

    // loader roles: X — pixel row tid / 8, 16-byte piece tid % 8 of every column chunk; dY — pieces tid + 256 i of [32][32 float4]
    const int xpx = tid >> 3, xq = tid & 7;
    const float* xbase[WG_NC]; int xcs[WG_NC], xdy[WG_NC], xdx[WG_NC]; bool xok[WG_NC];
#pragma unroll
    for (int j = 0; j < WG_NC; ++j) {
        const int chunk = blockIdx.x * WG_NC + j;
        xok[j] = chunk < nchunks;
        const int k0 = xok[j] ? chunk * 32 : 0;
        const int tap = k0 / p.Cin, c = k0 - tap * p.Cin;
        const bool second = c >= p.C1;
        xbase[j] = (second ? p.X2 + (c - p.C1) : p.X + c) + 4 * xq;
        xcs[j] = second ? p.Cin - p.C1 : p.C1;
        xdy[j] = tap / 3; xdx[j] = tap - 3 * xdy[j];
    }
    v4f xr[WG_NC], dr[4];
    auto gload = [&](int p0) {
        const int px = p0 + xpx;
        int n = 0, oy = 0, ox = px;
        if (p.mode != 0) { n = px / OHW; const int rem = px - n * OHW; oy = rem / p.OW; ox = rem - oy * p.OW; }
#pragma unroll
        for (int j = 0; j < WG_NC; ++j) {
            long long off = -1;
            if (px < p_end && xok[j]) {
                if (p.mode == 0) off = px;
                else if (p.mode == 3) {
                    const int uh = oy + xdy[j] - 1, uw = ox + xdx[j] - 1;
                    if (uh >= 0 && uh < p.OH && uw >= 0 && uw < p.OW) {
                        int ih = (int)floorf((float)uh * sh); ih = ih < p.H - 1 ? ih : p.H - 1;
                        int iw = (int)floorf((float)uw * sw); iw = iw < p.W - 1 ? iw : p.W - 1;
                        off = ((long long)n * p.H + ih) * p.W + iw;
                    }
                } else {
                    const int st = p.mode == 1 ? 1 : 2;
                    const int ih = oy * st + xdy[j] - 1, iw = ox * st + xdx[j] - 1;
                    if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W) off = ((long long)n * p.H + ih) * p.W + iw;
                }
            }
            xr[j] = off >= 0 ? *reinterpret_cast<const v4f*>(xbase[j] + off * xcs[j]) : v4f{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + WG_NT * i, r = idx >> 5, co = co0 + 4 * (idx & 31), q = p0 + r;
            dr[i] = (q < p_end && co < p.Cout) ? *reinterpret_cast<const v4f*>(p.dY + (long long)q * p.Cout + co) : v4f{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < WG_NC; ++j) *reinterpret_cast<v4f*>(&Xs[j][xpx][4 * xq]) = xr[j];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int idx = tid + WG_NT * i; *reinterpret_cast<v4f*>(&Ds[idx >> 5][4 * (idx & 31)]) = dr[i]; }
    };

    v16f acc[WG_NC];
#pragma unroll
    for (int j = 0; j < WG_NC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    if (p_begin < p_end) gload(p_begin);
    for (int p0 = p_begin; p0 < p_end; p0 += WG_PX) {
        __syncthreads();                    // the previous step's fragment reads are done
        lstore();
        __syncthreads();
        if (p0 + WG_PX < p_end) gload(p0 + WG_PX);      // the next step's global loads fly under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < WG_PX / 2; ++kk) {
            const float a = Ds[2 * kk + h32][wid * 32 + c32];
#pragma unroll
            for (int j = 0; j < WG_NC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Xs[j][2 * kk + h32][c32], acc[j], 0, 0, 0);
        }
    }

    float* out = p.work + (size_t)blockIdx.z * p.Cout * p.K;
#pragma unroll
    for (int j = 0; j < WG_NC; ++j) {
        const int chunk = blockIdx.x * WG_NC + j;
        if (chunk >= nchunks) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + wid * 32 + 8 * (r >> 2) + 4 * h32 + (r & 3);
            if (co < p.Cout) out[(size_t)co * p.K + chunk * 32 + c32] = acc[j][r];
        }
    }
}

__global__ void wgrad32_reduce_kernel(const float* work, long long n4, int slabs, int accumulate, float* dWp) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        v4f s = *reinterpret_cast<const v4f*>(work + 4 * i);
        for (int k = 1; k < slabs; ++k) s += *reinterpret_cast<const v4f*>(work + 4 * ((long long)k * n4 + i));
        if (accumulate) s = *reinterpret_cast<const v4f*>(dWp + 4 * i) + s;
        *reinterpret_cast<v4f*>(dWp + 4 * i) = s;
    }
}

// ---- column sums: out[n][c] = sum over the HW rows of sample n, fp64 accumulators, fixed order ------------------------------------
// block = (32-channel chunk, sample): 32 row lanes x 8 pieces of 16 bytes; row lane r adds rows r, r + 32, ... ; the lanes are added 0 .. 31
__global__ __launch_bounds__(256) void colsum32_kernel(const float* dY, int HW, int C, int accumulate, float* out) {
    __shared__ double part[32][33];
    const int q = threadIdx.x & 7, r = threadIdx.x >> 3, c = blockIdx.x * 32 + 4 * q, n = blockIdx.y;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < C) {
        const float* src = dY + (long long)n * HW * C + c;
        for (int row = r; row < HW; row += 32) {
            const v4f v = *reinterpret_cast<const v4f*>(src + (long long)row * C);
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += (double)v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[r][4 * q + j] = s[j];
    __syncthreads();
    if (threadIdx.x < 32) {
        const int ch = blockIdx.x * 32 + threadIdx.x;
        if (ch < C) {
            double t = 0.0;
            for (int k = 0; k < 32; ++k) t += part[k][threadIdx.x];
            float* o = out + (long long)n * C + ch;
            const float g = (float)t;
            *o = accumulate ? *o + g : g;
        }
    }
}

// ---- GroupNorm (+ SiLU) backward ---------------------------------------------------------------------------------------------------
__device__ inline float silu_grad(float z) {          // d/dz [z sigmoid(z)] = s (1 + z (1 - s))
    const float s = 1.0f / (1.0f + expf(-z));
    return s * (1.0f + z * (1.0f - s));
}

// pass 1, block = (sample, group): thread (r, j) = pixel lane r, channel j of the group; per (sample, channel) A = sum dz, B = sum dz xhat
// in fp64 (lanes added in ascending order) -> chan[n][c] = (A, B); per (sample, group) sum_j gamma_j (A_j, B_j) -> grp[n * G + g]
__global__ __launch_bounds__(256) void gn32_bwd_sums_kernel(const float* X, const float* X2, const float* dY, int HW, int C, int C1, int G,
                                                            const float* gamma, const float* beta, const float* stats, int silu,
                                                            double* chan, double* grp) {
    __shared__ double sa[256], sb[256];
    const int n = blockIdx.x / G, g = blockIdx.x - n * G, cpg = C / G, C2 = C - C1;
    const int lanes = 256 / cpg, r = threadIdx.x / cpg, j = threadIdx.x - r * cpg, ch = g * cpg + j;
    const float mean = stats[2 * blockIdx.x], rstd = stats[2 * blockIdx.x + 1];
    double a = 0.0, b = 0.0;
    if (r < lanes) {
        const float ga = gamma[ch], be = beta[ch];
        for (int px = r; px < HW; px += lanes) {
            const long long row = (long long)n * HW + px;
            const float x = ch < C1 ? X[row * C1 + ch] : X2[row * C2 + (ch - C1)];
            const float xh = (x - mean) * rstd;
            float dz = dY[row * C + ch];
            if (silu) dz *= silu_grad(xh * ga + be);
            a += (double)dz; b += (double)dz * (double)xh;
        }
    }
    sa[threadIdx.x] = a; sb[threadIdx.x] = b;
    __syncthreads();
    if ((int)threadIdx.x < cpg) {
        double ta = 0.0, tb = 0.0;
        for (int k = 0; k < lanes; ++k) { ta += sa[k * cpg + threadIdx.x]; tb += sb[k * cpg + threadIdx.x]; }
        chan[2 * ((long long)n * C + ch)] = ta; chan[2 * ((long long)n * C + ch) + 1] = tb;
        sa[threadIdx.x] = ta * (double)gamma[ch]; sb[threadIdx.x] = tb * (double)gamma[ch];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ta = 0.0, tb = 0.0;
        for (int k = 0; k < cpg; ++k) { ta += sa[k]; tb += sb[k]; }
        grp[2 * blockIdx.x] = ta; grp[2 * blockIdx.x + 1] = tb;
    }
}

// dgamma[c] = sum_n B[n][c], dbeta[c] = sum_n A[n][c], samples in ascending order
__global__ void gn32_bwd_params_kernel(const double* chan, int N, int C, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int n = 0; n < N; ++n) { a += chan[2 * ((long long)n * C + c)]; b += chan[2 * ((long long)n * C + c) + 1]; }
    dgamma[c] = (float)b; dbeta[c] = (float)a;
}

// pass 2: dx = rstd (dz gamma - mean(dz gamma) - xhat mean(dz gamma xhat)), the means over the HW * cpg elements of the (sample, group)
__global__ void gn32_bwd_apply_kernel(const float* X, const float* X2, const float* dY, long long rows, int HW, int C, int C1, int G,
                                      const float* gamma, const float* beta, const float* stats, int silu, const double* grp, float* dX, float* dX2) {
    const int cpg = C / G, C2 = C - C1;
    const long long total = rows * C;
    const double inv = 1.0 / ((double)HW * (double)cpg);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C;
        const int ch = (int)(i - row * C), n = (int)(row / HW), sg = n * G + ch / cpg;
        const float mean = stats[2 * sg], rstd = stats[2 * sg + 1];
        const float m1 = (float)(grp[2 * sg] * inv), m2 = (float)(grp[2 * sg + 1] * inv);
        const float x = ch < C1 ? X[row * C1 + ch] : X2[row * C2 + (ch - C1)];
        const float xh = (x - mean) * rstd, ga = gamma[ch];
        float dz = dY[i];
        if (silu) dz *= silu_grad(xh * ga + beta[ch]);
        const float v = rstd * (dz * ga - m1 - xh * m2);
        if (ch < C1) dX[row * C1 + ch] = v; else dX2[row * C2 + (ch - C1)] = v;
    }
}

// ---- small kernels -----------------------------------------------------------------------------------------------------------------
__global__ void silu_bwd32_kernel(const float* x, const float* dy, float* dx, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dx[i] = dy[i] * silu_grad(x[i]);
}

// Z [N,H,W,C]: Z[2 oy][2 ox] = dY[oy][ox] (dY [N,OH,OW,C], OH = (H + 1) / 2, OW = (W + 1) / 2), zero elsewhere; C % 4 == 0
__global__ void zero_insert2_kernel(const float* dY, int N, int H, int W, int C, float* Z) {
    const int c4 = C / 4, OH = (H + 1) / 2, OW = (W + 1) / 2;
    const long long total = (long long)N * H * W * c4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long px = i / c4;
        const int q = (int)(i - px * c4), x = (int)(px % W), y = (int)((px / W) % H), n = (int)(px / ((long long)W * H));
        v4f v = {0.f, 0.f, 0.f, 0.f};
        if (!(x & 1) && !(y & 1)) v = *reinterpret_cast<const v4f*>(dY + (((long long)n * OH + (y >> 1)) * OW + (x >> 1)) * C + 4 * q);
        *reinterpret_cast<v4f*>(Z + px * C + 4 * q) = v;
    }
}

// the nearest rule of gemm32's mode 3 (and of F.interpolate): src = min(floor(dst * (float)in / (float)out), in - 1); non-decreasing in dst,
// so the pre-image of `src` is the range [lo, hi)
__device__ inline int nearest_src(int dst, float scale, int in) { const int s = (int)floorf((float)dst * scale); return s < in - 1 ? s : in - 1; }
__device__ inline void nearest_range(int src, int in, int out, int& lo, int& hi) {
    const float scale = (float)in / (float)out;
    lo = (int)((float)src * ((float)out / (float)in)) - 1;
    lo = lo < 0 ? 0 : (lo > out ? out : lo);
    while (lo > 0 && nearest_src(lo - 1, scale, in) >= src) --lo;
    while (lo < out && nearest_src(lo, scale, in) < src) ++lo;
    hi = lo;
    while (hi < out && nearest_src(hi, scale, in) == src) ++hi;
}

// dS [N,H,W,C] = sum of dU [N,OH,OW,C] over each source pixel's pre-image, destination rows then columns ascending; C % 4 == 0
__global__ void nearest_bwd_kernel(const float* dU, int N, int H, int W, int OH, int OW, int C, float* dS) {
    const int c4 = C / 4;
    const long long total = (long long)N * H * W * c4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long px = i / c4;
        const int q = (int)(i - px * c4), x = (int)(px % W), y = (int)((px / W) % H), n = (int)(px / ((long long)W * H));
        int y0, y1, x0, x1;
        nearest_range(y, H, OH, y0, y1);
        nearest_range(x, W, OW, x0, x1);
        v4f s = {0.f, 0.f, 0.f, 0.f};
        for (int uy = y0; uy < y1; ++uy)
            for (int ux = x0; ux < x1; ++ux) s += *reinterpret_cast<const v4f*>(dU + (((long long)n * OH + uy) * OW + ux) * C + 4 * q);
        *reinterpret_cast<v4f*>(dS + px * C + 4 * q) = s;
    }
}

// ---- LayerNorm backward ------------------------------------------------------------------------------------------------------------
// one wave per row: mean and rstd by ln32_kernel's own expressions (f32_ops.hip: two passes, fp32, the same lane order and shuffles), kept
// in rowstats [rows][2] for the parameter sums; dx = rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)), the two means from fp64
// lane sums.  A row of zero variance has rstd = eps^-1/2 and xhat = 0.
__global__ __launch_bounds__(256) void ln32_bwd_dx_kernel(const float* X, const float* dY, int rows, int C, const float* gamma, float eps, float* rowstats,
                                                          float* dX) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* x = X + (long long)row * C;
    const float* dy = dY + (long long)row * C;
    float s = 0.f;
    for (int i = lane; i < C; i += 64) s += x[i];
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w);
    const float mean = s / (float)C;
    float q = 0.f;
    for (int i = lane; i < C; i += 64) { const float d = x[i] - mean; q += d * d; }
    for (int w = 32; w > 0; w >>= 1) q += __shfl_xor(q, w);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    double a = 0.0, b = 0.0;
    for (int i = lane; i < C; i += 64) {
        const float dg = dy[i] * gamma[i], xh = (x[i] - mean) * rstd;
        a += (double)dg; b += (double)dg * (double)xh;
    }
    for (int w = 32; w > 0; w >>= 1) { a += __shfl_xor(a, w); b += __shfl_xor(b, w); }
    const float m1 = (float)(a / (double)C), m2 = (float)(b / (double)C);
    float* dx = dX + (long long)row * C;
    for (int i = lane; i < C; i += 64) {
        const float xh = (x[i] - mean) * rstd;
        dx[i] = rstd * (dy[i] * gamma[i] - m1 - xh * m2);
    }
    if (lane == 0) { rowstats[2 * (long long)row] = mean; rowstats[2 * (long long)row + 1] = rstd; }
}

// block = (64-channel chunk, row slab): thread (r = tid / 64, j = tid % 64) adds rows r, r + 4, ... of the slab for channel j in fp64; the four
// row lanes are added 0 .. 3 -> part[slab][0][c] = sum dy xhat, part[slab][1][c] = sum dy
__global__ __launch_bounds__(256) void ln32_bwd_params_kernel(const float* X, const float* dY, int rows, int C, int slab_len, const float* rowstats,
                                                              double* part) {
    __shared__ double sa[256], sb[256];
    const int j = threadIdx.x & 63, r = threadIdx.x >> 6, ch = blockIdx.x * 64 + j;
    const int r0 = blockIdx.y * slab_len, r1 = rows < r0 + slab_len ? rows : r0 + slab_len;
    double a = 0.0, b = 0.0;
    if (ch < C)
        for (int row = r0 + r; row < r1; row += 4) {
            const float mean = rowstats[2 * (long long)row], rstd = rowstats[2 * (long long)row + 1];
            const float xh = (X[(long long)row * C + ch] - mean) * rstd, d = dY[(long long)row * C + ch];
            a += (double)d * (double)xh; b += (double)d;
        }
    sa[threadIdx.x] = a; sb[threadIdx.x] = b;
    __syncthreads();
    if (r == 0 && ch < C) {
        double ta = 0.0, tb = 0.0;
        for (int k = 0; k < 4; ++k) { ta += sa[64 * k + j]; tb += sb[64 * k + j]; }
        part[((long long)blockIdx.y * 2) * C + ch] = ta;
        part[((long long)blockIdx.y * 2 + 1) * C + ch] = tb;
    }
}

__global__ void ln32_bwd_reduce_kernel(const double* part, int slabs, int C, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < slabs; ++k) { a += part[((long long)k * 2) * C + c]; b += part[((long long)k * 2 + 1) * C + c]; }
    dgamma[c] = (float)a; dbeta[c] = (float)b;
}

// ---- GEGLU on P [M][2F] = (h | g), 16-byte accesses ----------------------------------------------------------------------------------
// gelu(g) in the GEMM epilogue's expression (f32_gemm.hip, epi = 1); gelu'(g) = Phi(g) + g phi(g), Phi = 0.5 (1 + erf(g / sqrt 2)),
// phi = exp(-g^2 / 2) / sqrt(2 pi)
__device__ inline float gelu_fwd(float g) { return 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f)); }
__device__ inline float gelu_grad(float g) {
    return 0.5f * (1.0f + erff(g * 0.70710678118654752440f)) + g * (0.39894228040143267794f * expf(-0.5f * g * g));
}

__global__ void geglu32_kernel(const float* P, long long M, int F, float* Y) {
    const int f4 = F / 4;
    const long long total = M * f4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / f4;
        const int c = 4 * (int)(i - row * f4);
        const v4f h = *reinterpret_cast<const v4f*>(P + row * 2 * F + c), g = *reinterpret_cast<const v4f*>(P + row * 2 * F + F + c);
        v4f y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = h[j] * gelu_fwd(g[j]);
        *reinterpret_cast<v4f*>(Y + row * F + c) = y;
    }
}

__global__ void geglu32_bwd_kernel(const float* P, const float* dY, long long M, int F, float* dP) {
    const int f4 = F / 4;
    const long long total = M * f4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / f4;
        const int c = 4 * (int)(i - row * f4);
        const v4f h = *reinterpret_cast<const v4f*>(P + row * 2 * F + c), g = *reinterpret_cast<const v4f*>(P + row * 2 * F + F + c);
        const v4f dy = *reinterpret_cast<const v4f*>(dY + row * F + c);
        v4f dh, dg;
#pragma unroll
        for (int j = 0; j < 4; ++j) { dh[j] = dy[j] * gelu_fwd(g[j]); dg[j] = dy[j] * h[j] * gelu_grad(g[j]); }
        *reinterpret_cast<v4f*>(dP + row * 2 * F + c) = dh;
        *reinterpret_cast<v4f*>(dP + row * 2 * F + F + c) = dg;
    }
}

inline unsigned grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 * 16 ? 65536 * 16 : g));
}

}  // namespace

// The slab partition: a function of the output pixel count M = N OH OW (mode 0: the row count) alone.  Few pixels: slabs of >= 128
// pixels, at most 4 (the layers with few pixels are the wide ones: many tiles, and a large partial each); from 8192 pixels on (the 64^2
// level of a training batch: few tiles, a long reduction) one slab per 2048 pixels, at most 16.  The slab length is a multiple of 32.
int wgrad_slabs(long long M, int* slab_len) {
    long long s = M < 8192 ? (M + 127) / 128 : M / 2048;
    const long long cap = M < 8192 ? 4 : 16;
    s = s < 1 ? 1 : (s > cap ? cap : s);
    const long long len = ((M + s - 1) / s + 31) / 32 * 32;
    if (slab_len) *slab_len = (int)len;
    return (int)s;
}

size_t wgrad_workspace_bytes(long long M, int Cout, int Cin, int mode) {
    if (M <= 0 || M > 0x7fffffffLL - 4096 || Cout <= 0 || Cin <= 0 || mode < 0 || mode > 3) return 0;
    return (size_t)wgrad_slabs(M, nullptr) * (size_t)Cout * (size_t)(mode == 0 ? 1 : 9) * (size_t)Cin * sizeof(float);
}

hipError_t launch_wgrad(const float* X, const float* X2, const float* dY, int M, int H, int W, int OH, int OW, int Cin, int C1, int Cout, int mode,
                        int accumulate, float* work, size_t work_bytes, float* dWp, hipStream_t s) {
    if (!X || !dY || !dWp || !work || mode < 0 || mode > 3 || M <= 0 || Cout <= 0 || Cin <= 0 || Cin % 32 != 0 || C1 % 32 != 0 || C1 <= 0 || C1 > Cin ||
        Cout % 4 != 0 || (C1 < Cin && !X2) || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || 9LL * Cin > (1LL << 30))
        return hipErrorInvalidValue;
    const size_t need = wgrad_workspace_bytes(M, Cout, Cin, mode);
    if (need == 0 || work_bytes < need) return hipErrorInvalidValue;
    WgradParams p;
    p.X = X; p.X2 = X2; p.dY = dY; p.work = work; p.M = M; p.Cout = Cout; p.Cin = Cin; p.C1 = C1; p.H = H; p.W = W; p.OH = OH; p.OW = OW; p.mode = mode;
    p.K = (mode == 0 ? 1 : 9) * Cin;
    const int slabs = wgrad_slabs(M, &p.slab_len);
    const int chunks = p.K / 32;
    const dim3 grid((unsigned)((chunks + WG_NC - 1) / WG_NC), (unsigned)((Cout + WG_CO - 1) / WG_CO), (unsigned)slabs);
    if (grid.y > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wgrad32_kernel, grid, dim3(WG_NT), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long n4 = (long long)Cout * p.K / 4;
    hipLaunchKernelGGL(wgrad32_reduce_kernel, dim3(grid_for(n4)), dim3(256), 0, s, (const float*)work, n4, slabs, accumulate, dWp);
    return hipGetLastError();
}

hipError_t launch_colsum(const float* dY, int N, int HW, int C, int accumulate, float* out, hipStream_t s) {
    if (!dY || !out || N <= 0 || N > 65535 || HW <= 0 || C <= 0 || C % 4 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(colsum32_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)N), dim3(256), 0, s, dY, HW, C, accumulate, out);
    return hipGetLastError();
}

size_t gn_bwd_workspace_bytes(int N, int C, int G) { return ((size_t)N * C + (size_t)N * G) * 2 * sizeof(double); }

hipError_t launch_gn_bwd(const float* X, const float* X2, const float* dY, int N, int HW, int C, int C1, int G, const float* gamma, const float* beta,
                         const float* stats, int silu, void* work, size_t work_bytes, float* dX, float* dX2, float* dgamma, float* dbeta, hipStream_t s) {
    if (!X || !dY || !gamma || !beta || !stats || !work || !dX || !dgamma || !dbeta || N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G != 0 || C / G > 256 ||
        C1 <= 0 || C1 > C || (C1 < C && (!X2 || !dX2)) || ((uintptr_t)work & 7) != 0 || work_bytes < gn_bwd_workspace_bytes(N, C, G) ||
        (long long)N * G > 0x7fffffffLL)
        return hipErrorInvalidValue;
    double* chan = (double*)work;
    double* grp = chan + 2 * (size_t)N * C;
    hipLaunchKernelGGL(gn32_bwd_sums_kernel, dim3((unsigned)(N * G)), dim3(256), 0, s, X, X2, dY, HW, C, C1, G, gamma, beta, stats, silu, chan, grp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gn32_bwd_params_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const double*)chan, N, C, dgamma, dbeta);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long rows = (long long)N * HW;
    hipLaunchKernelGGL(gn32_bwd_apply_kernel, dim3(grid_for(rows * C)), dim3(256), 0, s, X, X2, dY, rows, HW, C, C1, G, gamma, beta, stats, silu,
                       (const double*)grp, dX, dX2);
    return hipGetLastError();
}

hipError_t launch_silu_bwd(const float* x, const float* dy, float* dx, long long n, hipStream_t s) {
    if (!x || !dy || !dx || n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(silu_bwd32_kernel, dim3(grid_for(n)), dim3(256), 0, s, x, dy, dx, n);
    return hipGetLastError();
}

hipError_t launch_zero_insert2(const float* dY, int N, int H, int W, int C, float* Z, hipStream_t s) {
    if (!dY || !Z || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zero_insert2_kernel, dim3(grid_for((long long)N * H * W * (C / 4))), dim3(256), 0, s, dY, N, H, W, C, Z);
    return hipGetLastError();
}

hipError_t launch_nearest_bwd(const float* dU, int N, int H, int W, int OH, int OW, int C, float* dS, hipStream_t s) {
    if (!dU || !dS || N <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || C <= 0 || C % 4 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nearest_bwd_kernel, dim3(grid_for((long long)N * H * W * (C / 4))), dim3(256), 0, s, dU, N, H, W, OH, OW, C, dS);
    return hipGetLastError();
}

// The row slabs of LayerNorm's parameter sums: a function of the row count alone, one slab per 256 rows, at most 64
int ln_bwd_slabs(int rows, int* slab_len) {
    int s = (rows + 255) / 256;
    s = s < 1 ? 1 : (s > 64 ? 64 : s);
    if (slab_len) *slab_len = (rows + s - 1) / s;
    return s;
}

size_t ln_bwd_workspace_bytes(int rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)ln_bwd_slabs(rows, nullptr) * 2 * C * sizeof(double) + (size_t)rows * 2 * sizeof(float);
}

hipError_t launch_layernorm_bwd(const float* X, const float* dY, int rows, int C, const float* gamma, float eps, void* work, size_t work_bytes,
                                float* dX, float* dgamma, float* dbeta, hipStream_t s) {
    const size_t need = ln_bwd_workspace_bytes(rows, C);
    if (!X || !dY || !gamma || !work || !dX || !dgamma || !dbeta || need == 0 || work_bytes < need || ((uintptr_t)work & 7) != 0 || !(eps >= 0.f))
        return hipErrorInvalidValue;
    int slab_len = 0;
    const int slabs = ln_bwd_slabs(rows, &slab_len);
    double* part = (double*)work;
    float* rowstats = (float*)(part + (size_t)slabs * 2 * C);
    hipLaunchKernelGGL(ln32_bwd_dx_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, X, dY, rows, C, gamma, eps, rowstats, dX);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ln32_bwd_params_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)slabs), dim3(256), 0, s, X, dY, rows, C, slab_len,
                       (const float*)rowstats, part);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ln32_bwd_reduce_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const double*)part, slabs, C, dgamma, dbeta);
    return hipGetLastError();
}

hipError_t launch_geglu(const float* P, int M, int F, float* Y, hipStream_t s) {
    if (!P || !Y || M <= 0 || F <= 0 || F % 4 != 0 || (((uintptr_t)P | (uintptr_t)Y) & 15) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(geglu32_kernel, dim3(grid_for((long long)M * (F / 4))), dim3(256), 0, s, P, (long long)M, F, Y);
    return hipGetLastError();
}

hipError_t launch_geglu_bwd(const float* P, const float* dY, int M, int F, float* dP, hipStream_t s) {
    if (!P || !dY || !dP || M <= 0 || F <= 0 || F % 4 != 0 || (((uintptr_t)P | (uintptr_t)dY | (uintptr_t)dP) & 15) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(geglu32_bwd_kernel, dim3(grid_for((long long)M * (F / 4))), dim3(256), 0, s, P, dY, (long long)M, F, dP);
    return hipGetLastError();
}

}  // namespace dm32
