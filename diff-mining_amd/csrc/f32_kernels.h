// f32_kernels.h — launcher prototypes of the fp32 kernels (internal, C++): the arithmetic of the reference's DIFT path,
// which runs the U-Net WITHOUT autocast and without torch_dtype (diffmining/typicality/dift.py:197-199: plain fp32).
// fp32 operands, fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation), fp32 tensors in HBM (NHWC).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct dm_clip_pre_desc;          // include/dm_engine.h

namespace dm32 {

// modes as dm::IGemmMode: 0 dense, 1 conv3x3 stride 1, 2 conv3x3 stride 2 (pad 1), 3 nearest-upsample to (OH, OW) then conv3x3,
// 4 conv3x3 stride 2 with pad (0,1,0,1) (VAE downsampler), 5 Upsample2D (nearest, exact 2x) + conv3x3 as four 2x2 convolutions on the source
// grid (H = OH, W = OW = the source, M = N H W rows per parity class, Wp [4][Cout][4 Cin] pre-summed taps, Y [N][2H][2W][Cout])
struct GemmParams {
    const float* X = nullptr;     // source 1, NHWC [N,H,W,C1] (dense: [M,C1])
    const float* X2 = nullptr;    // source 2 (channel concat), NHWC [N,H,W,Cin-C1], or nullptr
    const float* Wp = nullptr;    // packed weights [Cout][taps*Cin], k = (tap, cin)
    const float* bias = nullptr;  // [Cout] or nullptr
    const float* temb = nullptr;  // per-sample channel add [N][temb_ld] (already offset) or nullptr
    const float* res = nullptr;   // residual [M][ldres] or nullptr
    float* Y = nullptr;           // [M][ldy]
    int M = 0, Cout = 0, Cin = 0, C1 = 0;
    int H = 1, W = 1, OH = 1, OW = 1;
    int mode = 0;
    int ldy = 0, ldres = 0, temb_ld = 0;
    // epi = 1: GEGLU — the weight rows are packed in quads (h0, h1, g0, g1) (value rows 2q, 2q + 1 and gate rows F + 2q, F + 2q + 1 of
    // ff.net.0.proj [2F][C], F = Cout / 2), a lane's four channels are one quad, Y [M][F] gets (h0 gelu(g0), h1 gelu(g1)) at columns 2q, 2q + 1
    int epi = 0;
};
hipError_t launch_gemm(const GemmParams& p, hipStream_t s);

struct AttnParams {
    const float* Q; const float* K; const float* V; float* O;
    int ldq, ldk, ldv, ldo;            // row strides in elements
    long long bsq, bsk, bsv, bso;      // batch strides in elements
    const int32_t* kv_slot = nullptr;  // optional: K/V batch index per sample (prompt slot), clamped to [0, n_slots)
    int n_slots = 0;
    int B, heads, Tq, Tk, D;           // D in {40, 64, 80, 160, 512}
    float scale;
};
hipError_t launch_attention(const AttnParams& p, hipStream_t s);

// GroupNorm over cat([X (C1 channels), X2 (C - C1)]) NHWC: stats [N*G][2] = (mean, rstd), then the apply (+ SiLU)
hipError_t launch_gn_stats(const float* X, const float* X2, int N, int HW, int C, int C1, int G, float eps, float* stats, hipStream_t s);
hipError_t launch_gn_apply(const float* X, const float* X2, int N, int HW, int C, int C1, int G, const float* gamma, const float* beta,
                           const float* stats, int silu, float* Y, hipStream_t s);
hipError_t launch_layernorm(const float* X, int rows, int C, const float* gamma, const float* beta, float eps, float* Y, hipStream_t s);
// CLIP tower glue (fp32): token + position embedding; attention of both towers, heads of 64 on the stacked q|k|v rows [n*T][3*heads*64]
// (q scaled by 1/8 inside): (T, causal) = (77, true) for the text tower, (50, false) for the image tower, nothing else; y * sigmoid(1.702 y)
// in place
hipError_t launch_clip_embed(const int32_t* ids, const float* tok, const float* pos, int rows, int T, int C, int vocab, float* out, hipStream_t s);
hipError_t launch_clip_attention(const float* qkv, int n, int T, int heads, bool causal, float* out, hipStream_t s);
hipError_t launch_quick_gelu(float* x, long long n, hipStream_t s);
// CLIP ViT-B/32 image tower glue (clip_vision.hip): the processor's BICUBIC resize + center crop + rescale + normalise of uint8 HWC crops
// (layout 0: [n][3][224][224], 1: patch rows [n*49][3072] with k = (c, ky, kx)); pixel_values -> patch rows; class token + patch embeddings +
// position embedding [n*50][C]; the CLS rows [n][C]; row-wise x / ||x||
hipError_t launch_clip_preprocess(const uint8_t* images, const dm_clip_pre_desc* desc, const int32_t* tables, int n, int layout, float* out,
                                  hipStream_t s);
hipError_t launch_clip_patchify(const float* pix, int n, float* rows, hipStream_t s);
hipError_t launch_clip_tokens(const float* pe, const float* cls, const float* pos, int n, int C, float* x, hipStream_t s);
hipError_t launch_clip_cls(const float* x, int n, int C, float* y, hipStream_t s);
hipError_t launch_clip_l2norm(const float* x, int n, int C, float* y, hipStream_t s);
// The configurable image tower's glue (clip_vision.hip; CLIP ViT-L/14-336: S = 336, PS = 14, T = 577): the processor WITHOUT the center
// crop on square uint8 images (layout 0: [n][3][S][S], 1: patch rows [n*G^2][KPAD], columns >= 3 PS PS written as zeros); pixel_values ->
// the same patch rows; class token + patch embeddings + positions [n*T][C]; post_layernorm of the patch tokens X [n][T][C] ->
// Y [n*(T-1)][C] (CLS skipped); text pooling: the hidden row at the first maximum of each ids row, hidden [n][T][C] -> y [n][C]
hipError_t launch_clip_tower_preprocess(const uint8_t* images, const dm_clip_pre_desc* desc, const int32_t* tables, int n, int S, int PS, int KPAD,
                                        int layout, float* out, hipStream_t s);
hipError_t launch_clip_tower_patchify(const float* pix, int n, int S, int PS, int KPAD, float* rows, hipStream_t s);
hipError_t launch_clip_tower_tokens(const float* pe, const float* cls, const float* pos, int n, int T, int C, float* x, hipStream_t s);
hipError_t launch_clip_tower_patch_ln(const float* X, int n, int T, int C, const float* gamma, const float* beta, float eps, float* Y, hipStream_t s);
hipError_t launch_clip_eos_gather(const int32_t* ids, const float* hidden, int n, int T, int C, float* y, hipStream_t s);
hipError_t launch_silu(const float* in, float* out, long long n, hipStream_t s);
// Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): out [B][dim] = [cos | sin]
hipError_t launch_timestep_embed(const int64_t* t, int B, int dim, float* out, hipStream_t s);
// conv_in: sample NCHW [B,Cin<=4,H,W] (x) 3x3 pad 1 -> NHWC [B,H,W,Cout]; w transposed [Cin*9][Cout] (k = (ci, dy, dx): consecutive
// threads = consecutive output channels read consecutive weights), bias [Cout]
hipError_t launch_conv_in(const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout, float* y, hipStream_t s);
// conv_out: NHWC [B,H,W,C] (x) 3x3 pad 1 -> NCHW [B,Cout<=8,H,W]; w packed [Cout][9*C] k = (tap, c)
hipError_t launch_conv_out(const float* x, const float* w, const float* bias, int B, int H, int W, int C, int Cout, float* y, hipStream_t s);
// scheduler.add_noise in fp32: out[b] = sa[t[b]] * x[x_index ? x_index[b] : b] + sb[t[b]] * eps[b]; `per` elements per sample
hipError_t launch_add_noise(const float* x, const int32_t* x_index, const float* eps, const int64_t* t, const float* sa, const float* sb,
                            int B, long long per, float* out, hipStream_t s);
hipError_t launch_sqerr(const float* pred, const float* eps, long long n, float* out, hipStream_t s);      // (pred - eps)^2
hipError_t launch_nhwc_to_nchw(const float* X, int N, int HW, int C, float* Y, hipStream_t s);
// quant_conv (1x1, 8 -> 8) on Hm [B*HW][8] + `draws` posterior samples per image * scaling (NCHW outputs: latent [B*draws,4,HW], moments [B,8,HW])
hipError_t launch_posterior(const float* Hm, const float* qw, const float* qb, const float* noise, int B, int draws, int HW, float scaling,
                            float* latent, float* moments, hipStream_t s);
// mean over groups of `ens` consecutive samples, NHWC -> NCHW
hipError_t launch_ensemble_mean(const float* X, int groups, int ens, int HW, int C, float* Y, hipStream_t s);
// The parallel-dataset generator's kernels (pnp.hip).  DDIM update out = c0 * ((x - c1 * eps) / c2) + c3 * eps with coef = (c0, c1, c2, c3) on
// the device, every operation rounded on its own; eps = eps_u, or eps_u + g * (eps_c - eps_u) when eps_c is given; out may be x
hipError_t launch_ddim_step(const float* x, const float* eps_u, const float* eps_c, float g, const float* coef, long long n, float* out, hipStream_t s);
// Y[b] = R[b] + Hs, b < B, `per` (a multiple of 4) elements per sample
hipError_t launch_bcast_add(const float* R, const float* Hs, int B, long long per, float* Y, hipStream_t s);
// z = post_quant_conv(latent * scale), 1x1 4 -> 4, NCHW [B,4,HW] in and out
hipError_t launch_decoder_head(const float* lat, const float* w, const float* b, int B, int HW, float scale, float* z, hipStream_t s);
// the decoder's tail on X NHWC [B,H,W,128] (the input of conv_norm_out) with its GroupNorm(32) statistics from launch_gn_stats: affine + SiLU
// while loading, conv3x3 pad 1 128 -> 3 (Wp [3][9*128], k = (tap, c)), then out_f32 NCHW [B,3,H,W] (raw ? the sample : (sample / 2 + 0.5)
// .clamp(0, 1)) and / or out_u8 NHWC [B,H,W,3] = that image * 255, truncated
hipError_t launch_decoder_tail(const float* X, const float* stats, const float* gamma, const float* beta, const float* Wp, const float* bias, int B,
                               int H, int W, int C, int raw, float* out_f32, uint8_t* out_u8, hipStream_t s);

// The gradient kernels of the convolutional blocks (f32_train.hip).  wgrad: dWp [Cout][taps*Cin] (gemm32's weight layout) = sum over the M
// output pixels of dY [M][Cout] (x) im2col(X | X2), modes 0 .. 3 as launch_gemm; the pixels are cut into wgrad_slabs(M) slabs whose partials
// go to `work` (wgrad_workspace_bytes) and are added in ascending order; accumulate: dWp += the finished gradient (one addition per element)
int wgrad_slabs(long long M, int* slab_len);
size_t wgrad_workspace_bytes(long long M, int Cout, int Cin, int mode);
hipError_t launch_wgrad(const float* X, const float* X2, const float* dY, int M, int H, int W, int OH, int OW, int Cin, int C1, int Cout, int mode,
                        int accumulate, float* work, size_t work_bytes, float* dWp, hipStream_t s);
// out [N][C] = the column sums of each sample's HW rows of dY [N*HW][C] (N = 1: dbias), fp64 accumulators in a fixed order
hipError_t launch_colsum(const float* dY, int N, int HW, int C, int accumulate, float* out, hipStream_t s);
// GroupNorm (+ SiLU) backward over cat([X, X2]) from the forward pass's stats [N*G][2]: dX [.., C1], dX2 [.., C - C1], dgamma / dbeta [C];
// work: gn_bwd_workspace_bytes, 8-byte aligned
size_t gn_bwd_workspace_bytes(int N, int C, int G);
hipError_t launch_gn_bwd(const float* X, const float* X2, const float* dY, int N, int HW, int C, int C1, int G, const float* gamma, const float* beta,
                         const float* stats, int silu, void* work, size_t work_bytes, float* dX, float* dX2, float* dgamma, float* dbeta, hipStream_t s);
hipError_t launch_silu_bwd(const float* x, const float* dy, float* dx, long long n, hipStream_t s);           // dx = dy * silu'(x)
// Z [N,H,W,C]: Z[2 oy][2 ox] = dY[oy][ox] of dY [N,(H+1)/2,(W+1)/2,C], zero elsewhere (the stride-2 data gradient as a mode-1 convolution)
hipError_t launch_zero_insert2(const float* dY, int N, int H, int W, int C, float* Z, hipStream_t s);
// dS [N,H,W,C]: every source pixel sums its pre-image of dU [N,OH,OW,C] under mode 3's nearest rule, ascending destination order
hipError_t launch_nearest_bwd(const float* dU, int N, int H, int W, int OH, int OW, int C, float* dS, hipStream_t s);

// The gradient kernels of the transformer blocks.  Attention backward (f32_train_attn.hip): Q, K, V, O, dO and dQ, dK, dV with row strides ld*
// and batch strides bs* as AttnParams (stacked q|k|v and k|v rows work in place), D in {40, 80, 160}.  `work` (16-byte aligned,
// attn_bwd_workspace_bytes) starts with the statistics [B][heads][Tq][2] = (L, Delta): L = log2 sum_k 2^(s scale log2e), Delta = dO . O;
// behind them (rounded up to 16 bytes) the dK | dV partials [slabs][B][heads][Tk][2 D] of attn_bwd_slabs(Tq, Tk) query slabs, which a reduce
// kernel adds in ascending slab order.  No floating-point atomics.
struct AttnBwdParams {
    const float* Q; const float* K; const float* V; const float* O; const float* dO;
    float* dQ; float* dK; float* dV;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    long long bsq, bsk, bsv, bso, bsdo, bsdq, bsdk, bsdv;
    int B, heads, Tq, Tk, D;
    float scale;
    void* work; size_t work_bytes;
    int phases = 15;      // bit 0 statistics, 1 dQ, 2 dK / dV partials, 3 their sum: the rate tool times them one by one (after one full run)
};
int attn_bwd_slabs(int Tq, int Tk, int* slab_len);
size_t attn_bwd_workspace_bytes(int B, int heads, int Tq, int Tk, int D);
hipError_t launch_attention_bwd(const AttnBwdParams& p, hipStream_t s);
// LayerNorm backward (f32_train.hip): mean / rstd recomputed per row as ln32_kernel does; dgamma / dbeta over ln_bwd_slabs(rows) row slabs in
// fp64, added in ascending order.  work: ln_bwd_workspace_bytes, 8-byte aligned (doubles [slabs][2][C], then floats [rows][2] = (mean, rstd))
int ln_bwd_slabs(int rows, int* slab_len);
size_t ln_bwd_workspace_bytes(int rows, int C);
hipError_t launch_layernorm_bwd(const float* X, const float* dY, int rows, int C, const float* gamma, float eps, void* work, size_t work_bytes,
                                float* dX, float* dgamma, float* dbeta, hipStream_t s);
// GEGLU on P [M][2F] = (h | g): Y [M][F] = h gelu(g) with the GEMM epilogue's expression; dP = (dY gelu(g) | dY h gelu'(g)); F % 4 == 0
hipError_t launch_geglu(const float* P, int M, int F, float* Y, hipStream_t s);
hipError_t launch_geglu_bwd(const float* P, const float* dY, int M, int F, float* dP, hipStream_t s);

}  // namespace dm32
