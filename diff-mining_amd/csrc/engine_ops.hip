// engine_ops.hip — operator-level entry points (dm_op_*): single launches for the parity tests, none of which takes an engine handle.
// The matrix kernels first (igemm tiles, attention routes, norms, conv_out), then the glue kernels around them, one entry per launch_*:
// dm_op_time_gather, dm_op_silu, dm_op_im2col_in, dm_op_nhwc_to_nchw, dm_op_ensemble_mean (misc.hip), dm_op_im2col_rgb, dm_op_posterior
// (vae.hip), dm_op_clip_embed, dm_op_clip_attention, dm_op_quick_gelu, dm_op_f16_to_f32 (clip.hip), dm_op_cfg_ddim_step, dm_op_latent_prologue,
// dm_op_decoder_tail (sample.hip).  Their fp32 counterparts are the dm_f32_op_* of f32_net.hip.
#include "../../include/dm_engine.h"
#include "dm_kernels.h"

using namespace dm;

extern "C" {

int dm_op_igemm(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb,
                const void* res, void* Y, int N, int H, int W, int C1, int C2, int Cout, int OH, int OW,
                int mode, int epi, int temb_ld) {
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = (const f16*)X2; p.Wp = (const f16*)Wp; p.bias = (const f16*)bias;
    p.temb = (const f16*)temb; p.res = (const f16*)res; p.Y = (f16*)Y;
    p.Cout = Cout; p.Cin = C1 + C2; p.C1 = C1; p.mode = mode; p.epi = epi;
    p.ldy = (epi == EPI_GEGLU) ? Cout / 2 : Cout; p.ldres = Cout; p.temb_ld = temb_ld;
    if (mode == IG_DENSE) { p.M = N * H * W; p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; }
    else { p.M = N * OH * OW; p.H = H; p.W = W; p.OH = OH; p.OW = OW; }
    return launch_igemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_ln_stats(void* stream, const void* X, int rows, int C, float eps, void* stats_f32) {
    return launch_ln_stats((const f16*)X, rows, C, eps, (float*)stats_f32, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_igemm_ln(void* stream, const void* X, const void* Wp_folded, const void* ln_s, const void* ln_t, const void* stats,
                   void* Y, int M, int Cin, int Cout, int epi) {
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = nullptr; p.Wp = (const f16*)Wp_folded; p.bias = nullptr; p.temb = nullptr; p.res = nullptr;
    p.Y = (f16*)Y; p.Cout = Cout; p.Cin = Cin; p.C1 = Cin; p.mode = IG_DENSE; p.epi = epi;
    p.ldy = (epi == EPI_GEGLU) ? Cout / 2 : Cout; p.ldres = 0; p.temb_ld = 0;
    p.M = M; p.H = 1; p.W = M; p.OH = 1; p.OW = M;
    p.ln_stats = (const float*)stats; p.ln_s = (const float*)ln_s; p.ln_t = (const float*)ln_t;
    return launch_igemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_igemm_splitk(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb,
                       const void* res, void* Y, int N, int H, int W, int C1, int C2, int Cout, int OH, int OW, int mode,
                       int temb_ld, int ksplit, void* workspace_f32) {
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = (const f16*)X2; p.Wp = (const f16*)Wp; p.bias = (const f16*)bias;
    p.temb = (const f16*)temb; p.res = (const f16*)res; p.Y = (f16*)Y;
    p.Cout = Cout; p.Cin = C1 + C2; p.C1 = C1; p.mode = mode; p.epi = EPI_PLAIN;
    p.ldy = Cout; p.ldres = Cout; p.temb_ld = temb_ld;
    if (mode == IG_DENSE) { p.M = N * H * W; p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; }
    else { p.M = N * OH * OW; p.H = H; p.W = W; p.OH = OH; p.OW = OW; }
    p.ksplit = ksplit; p.partial = (float*)workspace_f32;
    return launch_igemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_attention512(void* stream, const void* Q, const void* K, const void* V, void* O, int B, int T, int ld, int ldo,
                       float scale) {
    return launch_attention512((const f16*)Q, (const f16*)K, (const f16*)V, (f16*)O, B, T, ld, ldo, scale, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_igemm_tile(int M, int Cin, int Cout, int mode) {
    IGemmParams p{};
    p.M = M; p.Cin = Cin; p.C1 = Cin; p.Cout = Cout; p.mode = mode; p.epi = EPI_PLAIN;
    p.OH = 1; p.OW = M > 511 ? 256 : (M > 0 ? M : 1);      // spatial extent unknown here: any value inside the kernel's coordinate range
    return igemm_tile_choice(p);
}

int dm_op_igemm_pers_max_source_channels(void) { return IGEMM_PERS_MAX_SRC_C; }

int dm_op_igemm_head_rows(int M, int spatial, int Cin, int Cout, int mode) {
    IGemmParams p{};
    p.M = M; p.Cin = Cin; p.C1 = Cin; p.Cout = Cout; p.mode = mode; p.epi = EPI_PLAIN;
    p.OH = 1; p.OW = mode == IG_DENSE ? (M > 0 ? M : 1) : (spatial > 0 ? spatial : 1);
    p.H = 1; p.W = p.OW;
    return igemm_head_rows(p);
}

int dm_op_attention_slots(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv,
                          int ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot, int slot_div, int n_slots,
                          int q_mod, int B, int heads, int Tq, int Tk, int D, float scale) {
    AttnParams a;
    a.Q = (const f16*)Q; a.K = (const f16*)K; a.V = (const f16*)V; a.O = (f16*)O;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.bsq = bsq; a.bsk = bsk; a.bsv = bsv; a.bso = bso;
    a.kv_slot = kv_slot; a.slot_div = slot_div; a.n_slots = n_slots; a.q_mod = q_mod;
    a.B = B; a.heads = heads; a.Tq = Tq; a.Tk = Tk; a.D = D; a.scale = scale;
    return launch_attention(a, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_attention(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv,
                    int ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot,
                    int B, int heads, int Tq, int Tk, int D, float scale) {
    return dm_op_attention_slots(stream, Q, K, V, O, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, kv_slot, 0, 0, 0, B, heads, Tq, Tk, D, scale);
}

int dm_op_attention_route(int B, int heads, int Tq, int Tk, int D, int q_mod) {
    AttnParams a{};
    a.B = B; a.heads = heads; a.Tq = Tq; a.Tk = Tk; a.D = D; a.q_mod = q_mod;
    return (int)attention_route(a);
}

int dm_op_groupnorm(void* stream, const void* X, const void* X2, int N, int HW, int C, int C1, int G, float eps,
                    const float* gamma, const float* beta, int silu, void* Y) {
    hipStream_t s = (hipStream_t)stream;
    double* partial = nullptr;
    const int chunks = gn_stats_chunks(HW);
    if (hipMalloc((void**)&partial, (size_t)N * chunks * G * 2 * sizeof(double)) != hipSuccess) return 1;
    hipError_t r = launch_gn_stats((const f16*)X, (const f16*)X2, N, HW, C, C1, G, partial, s);
    if (r == hipSuccess) r = launch_gn_apply((const f16*)X, (const f16*)X2, N, HW, C, C1, G, eps, gamma, beta, partial, silu, (f16*)Y, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(partial);
    return r == hipSuccess ? 0 : 1;
}

int dm_op_conv_temb_gn_blocks(void* stream, const void* X, const void* Wp, const void* bias, const void* temb, void* Y, int N, int H, int W,
                              int Cin, int Cout, int temb_ld, float* blocks, int* rows_done) {
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = nullptr; p.Wp = (const f16*)Wp; p.bias = (const f16*)bias; p.temb = (const f16*)temb; p.res = nullptr;
    p.Y = (f16*)Y; p.Cout = Cout; p.Cin = Cin; p.C1 = Cin; p.mode = IG_CONV3; p.epi = EPI_PLAIN; p.ldy = Cout; p.ldres = 0; p.temb_ld = temb_ld;
    p.M = N * H * W; p.H = H; p.W = W; p.OH = H; p.OW = W;
    p.gn_blocks = blocks;
    if (rows_done) *rows_done = igemm_gn_rows(p);
    return launch_igemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_conv_out(void* stream, const void* Xn, const void* w, const void* bias, const float* eps, int B, int H, int W, int C0, float* loss,
                   void* pred) {
    return launch_conv_out((const f16*)Xn, (const f16*)w, (const f16*)bias, eps, 1, B, H, W, C0, loss, (f16*)pred, B, B, 0, 0,
                           (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_gn_blocks(void* stream, const void* X, int rows, int C, int row0, float* blocks) {
    return launch_gn_blocks((const f16*)X, rows, C, row0, blocks, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_groupnorm_blocks(void* stream, const void* X, const float* blocks, int N, int HW, int C, int G, float eps, const float* gamma,
                           const float* beta, int silu, void* Y) {
    hipStream_t s = (hipStream_t)stream;
    double* partial = nullptr;
    if (hipMalloc((void**)&partial, (size_t)N * G * 2 * sizeof(double)) != hipSuccess) return 1;
    hipError_t r = launch_gn_blocks_final(blocks, N, HW, C, G, partial, s);
    if (r == hipSuccess) r = launch_gn_apply((const f16*)X, nullptr, N, HW, C, C, G, eps, gamma, beta, partial, silu, (f16*)Y, s, 1);
    (void)hipStreamSynchronize(s);
    (void)hipFree(partial);
    return r == hipSuccess ? 0 : 1;
}

int dm_op_igemm_shortcut(void* stream, const void* X, const void* X3, const void* X4, const void* Wp, const void* bias, const void* res,
                         void* Y, int N, int H, int W, int Cin, int C3, int C4, int Cout, int mode) {
    if (mode != IG_CONV3 && mode != IG_DENSE) return 1;
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = nullptr; p.Wp = (const f16*)Wp; p.bias = (const f16*)bias; p.temb = nullptr; p.res = (const f16*)res;
    p.Y = (f16*)Y; p.Cout = Cout; p.Cin = Cin; p.C1 = Cin; p.mode = mode; p.epi = EPI_PLAIN;
    p.ldy = Cout; p.ldres = Cout; p.temb_ld = 0; p.M = N * H * W;
    if (mode == IG_DENSE) { p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; } else { p.H = H; p.W = W; p.OH = H; p.OW = W; }
    p.X3 = (const f16*)X3; p.X4 = (const f16*)X4; p.C3 = C3; p.Csc = C3 + C4;
    return launch_igemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_fold_upconv_weights(const void* w_oihw_f16_host, int Cout, int Cin, void* out_f16_host) {
    if (!w_oihw_f16_host || !out_f16_host || Cout <= 0 || Cin <= 0) return 1;
    fold_upconv_weights((const f16*)w_oihw_f16_host, Cout, Cin, (f16*)out_f16_host);
    return 0;
}

int dm_op_upconv_folded(void* stream, const void* X, const void* W4, const void* bias, void* Y, int N, int H, int W, int Cin, int Cout) {
    if (!igemm_up4_ok(N, H, W, Cin, Cout)) return 1;
    IGemmParams p;
    p.X = (const f16*)X; p.X2 = nullptr; p.Wp = (const f16*)W4; p.bias = (const f16*)bias; p.temb = nullptr; p.res = nullptr; p.Y = (f16*)Y;
    p.Cout = Cout; p.Cin = Cin; p.C1 = Cin; p.mode = IG_CONV2_UP4; p.epi = EPI_PLAIN; p.ldy = Cout; p.ldres = 0; p.temb_ld = 0;
    p.M = N * H * W; p.H = H; p.W = W; p.OH = H; p.OW = W;
    return launch_igemm_pers_up4(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_groupnorm_conv1x1(void* stream, const void* X, int N, int HW, int C, int G, float eps, const float* gamma,
                            const float* beta, const void* W, const void* bias, int Cout, void* Y) {
    hipStream_t s = (hipStream_t)stream;
    double* partial = nullptr; f16* wn = nullptr; float* tn = nullptr;
    const int chunks = gn_stats_chunks(HW);
    if (hipMalloc((void**)&partial, (size_t)N * chunks * G * 2 * sizeof(double)) != hipSuccess) return 1;
    if (hipMalloc((void**)&wn, (size_t)N * Cout * C * sizeof(f16)) != hipSuccess) { (void)hipFree(partial); return 1; }
    if (hipMalloc((void**)&tn, (size_t)N * Cout * sizeof(float)) != hipSuccess) { (void)hipFree(partial); (void)hipFree(wn); return 1; }
    hipError_t r = launch_gn_stats((const f16*)X, nullptr, N, HW, C, C, G, partial, s);
    if (r == hipSuccess) r = launch_gn_fold(partial, N, HW, C, G, eps, gamma, beta, (const f16*)W, (const f16*)bias, Cout, wn, tn, s);
    if (r == hipSuccess) {
        IGemmParams p;
        p.X = (const f16*)X; p.X2 = nullptr; p.Wp = wn; p.bias = nullptr; p.temb = nullptr; p.res = nullptr; p.Y = (f16*)Y;
        p.M = N * HW; p.Cout = Cout; p.Cin = C; p.C1 = C; p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M;
        p.mode = IG_DENSE; p.epi = EPI_PLAIN; p.ldy = Cout; p.ldres = 0; p.temb_ld = 0;
        p.ln_s = tn; p.ln_t = tn; p.w_sample_stride = (long long)Cout * C; p.rows_per_sample = HW;
        r = launch_igemm(p, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(partial); (void)hipFree(wn); (void)hipFree(tn);
    return r == hipSuccess ? 0 : 1;
}

int dm_op_layernorm(void* stream, const void* X, int rows, int C, const float* gamma, const float* beta, float eps,
                    void* Y) {
    return launch_layernorm((const f16*)X, rows, C, gamma, beta, eps, (f16*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

// ---- the glue kernels one by one (tests/test_gpu_glue.py): each entry wraps ONE launch_* and adds no arithmetic.  A null required pointer, a
// non-positive extent or a violated precondition of the kernel returns 1 before anything is launched.
int dm_op_time_gather(void* stream, const void* table, const int64_t* t, int B, int dim, void* out) {
    if (!table || !t || !out || B <= 0 || dim <= 0 || (long long)B * dim > 0x7fffffffLL - 255) return 1;
    return launch_time_gather((const f16*)table, t, B, dim, (f16*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_silu(void* stream, const void* in, void* out, int64_t n) {
    if (!in || !out || n <= 0) return 1;
    return launch_silu((const f16*)in, (f16*)out, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_im2col_in(void* stream, const void* x, const int32_t* x_index, const void* eps, const int64_t* t, const void* sa, const void* sb,
                    int latent_f32, int B, int H, int W, void* out) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 1;
    if ((sa == nullptr) != (sb == nullptr)) return 1;
    if (sa && (!eps || !t)) return 1;
    return launch_im2col_in(x, x_index, eps, t, sa, sb, latent_f32 ? 1 : 0, B, H, W, (f16*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_nhwc_to_nchw(void* stream, const void* X, int N, int HW, int C, void* Y) {
    if (!X || !Y || N <= 0 || HW <= 0 || C <= 0 || N > 65535 || (C + 31) / 32 > 65535) return 1;
    return launch_nhwc_to_nchw((const f16*)X, N, HW, C, (f16*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_ensemble_mean(void* stream, const void* X, int groups, int ens, int HW, int C, float* Y) {
    if (!X || !Y || groups <= 0 || ens < 1 || HW <= 0 || C <= 0 || groups > 65535 || (C + 31) / 32 > 65535) return 1;
    return launch_ensemble_mean((const f16*)X, groups, ens, HW, C, Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_im2col_rgb(void* stream, const void* x, int B, int H, int W, void* out) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 1;
    return launch_im2col_rgb((const f16*)x, B, H, W, (f16*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_posterior(void* stream, const void* Hm, int ldh, const void* qw, const void* qb, const void* noise, int B, int draws, int HW,
                    float scaling, void* latent16, float* latent32, float* moments) {
    if (!Hm || !qw || !qb || B <= 0 || HW <= 0 || draws < 1 || ldh < 8 || ldh % 8) return 1;
    if (!latent16 && !latent32 && !moments) return 1;
    return launch_posterior((const f16*)Hm, ldh, (const f16*)qw, (const f16*)qb, (const f16*)noise, B, draws, HW, scaling, (f16*)latent16,
                            latent32, moments, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, int rows, int T, int C, int vocab, void* out) {
    if (!ids || !tok || !pos || !out || rows <= 0 || T < 1 || C <= 0 || C % 8 || vocab < 1) return 1;
    return launch_clip_embed(ids, (const f16*)tok, (const f16*)pos, rows, T, C, vocab, (f16*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_clip_attention(void* stream, const void* qkv, int n, int T, int heads, void* out) {
    if (!qkv || !out || n <= 0 || n > 65535 || T <= 0 || heads < 1) return 1;
    return launch_clip_attention((const f16*)qkv, n, T, heads, (f16*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;      // T > 80: refused there
}

int dm_op_quick_gelu(void* stream, void* x, int64_t n) {
    if (!x || n <= 0) return 1;
    return launch_quick_gelu((f16*)x, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;                            // n % 8: refused there
}

int dm_op_f16_to_f32(void* stream, const void* x, float* y, int64_t n) {
    if (!x || !y || n <= 0) return 1;
    return launch_f16_to_f32((const f16*)x, y, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

// ---- the kernels of text-to-image sampling (sample.hip), one by one
int dm_op_cfg_ddim_step(void* stream, const float* x_f32, const void* eps_f16, const float* coef4_dev, float g, int64_t n, float* out_f32) {
    if (!x_f32 || !eps_f16 || !coef4_dev || !out_f32 || n <= 0) return 1;
    return launch_cfg_ddim_step(x_f32, (const f16*)eps_f16, g, coef4_dev, (long long)n, out_f32, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_op_latent_prologue(void* stream, const float* latent_f32, const void* w_f16, const void* b_f16, int B, int HW, float scaling_factor,
                          void* out_f16, int ldc) {
    if (!latent_f32 || !w_f16 || !b_f16 || !out_f16 || B <= 0 || HW <= 0) return 1;
    return launch_latent_prologue(latent_f32, (const f16*)w_f16, (const f16*)b_f16, B, HW, scaling_factor, (f16*)out_f16, ldc,
                                  (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

// bytes of the statistics' partial sums [B][chunks][G][2] fp64, which the affine [B][2][C] fp32 follows
static size_t decoder_tail_partial_bytes(int B, int H, int W) {
    return (size_t)B * gn_stats_chunks(H * W) * DEC_TAIL_G * 2 * sizeof(double);
}

size_t dm_op_decoder_tail_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) return 0;
    return decoder_tail_partial_bytes(B, H, W) + (size_t)B * 2 * DEC_TAIL_C * sizeof(float);
}

int dm_op_decoder_tail(void* stream, const void* X, const float* gamma, const float* beta, const void* Wp, const void* bias, int B, int H, int W,
                       float eps, void* work, size_t work_bytes, void* raw_f16_out, void* image_u8_out) {
    if (!X || !gamma || !beta || !Wp || !bias || !work || (!raw_f16_out && !image_u8_out)) return 1;
    const size_t need = dm_op_decoder_tail_workspace_bytes(B, H, W);
    if (need == 0 || work_bytes < need || ((uintptr_t)work & 7)) return 1;
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)work;
    float* ab = (float*)((char*)work + decoder_tail_partial_bytes(B, H, W));
    hipError_t r = launch_gn_stats((const f16*)X, nullptr, B, H * W, DEC_TAIL_C, DEC_TAIL_C, DEC_TAIL_G, partial, s);
    if (r == hipSuccess) r = launch_gn_affine(partial, B, H * W, DEC_TAIL_C, DEC_TAIL_G, eps, gamma, beta, ab, s);
    if (r == hipSuccess) r = launch_decoder_tail((const f16*)X, ab, (const f16*)Wp, (const f16*)bias, B, H, W, DEC_TAIL_C, (f16*)raw_f16_out,
                                                 (uint8_t*)image_u8_out, s);
    return r == hipSuccess ? 0 : 1;
}

}  // extern "C"
