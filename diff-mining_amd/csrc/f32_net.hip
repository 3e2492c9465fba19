// f32_net.hip — the handle of the fp32 net (create, destroy, last error), its profiler and memory report, and the dm_f32_op_* operator
// entries of the parity tests.  The weight sets behind the handle: f32_pack.hip; what runs on them: f32_forward.hip (the U-Net and
// its loops), f32_vae.hip, f32_clip_nets.hip.
#include "f32_impl.h"

#include <cstdlib>

using namespace dm32;

static thread_local std::string g_create_error32;

extern "C" {

int dm_f32_create(int device, dm_f32_net** out) {
    if (!out) return 1;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { g_create_error32 = "no such HIP device"; return 1; }
    dm_f32_net* e = new dm_f32_net();
    e->device = device;
    *out = e;
    return 0;
}

void dm_f32_destroy(dm_f32_net* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (float* slab : {e->w_unet.slab, e->w_vae.slab, e->w_vaed.slab, e->w_clip.slab, e->w_clipv.slab, e->w_clipt.slab}) if (slab) (void)hipFree(slab);
    if (e->loop_buf) (void)hipFree(e->loop_buf);
    if (e->sched_tab) (void)hipFree(e->sched_tab);
    if (e->score_tmp) (void)hipFree(e->score_tmp);
    if (e->arena_base) (void)hipFree(e->arena_base);
    for (float* p : e->kv_cache) if (p) (void)hipFree(p);
    for (auto& ev : e->evs) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    for (hipEvent_t h : e->ev_pool) (void)hipEventDestroy(h);
    delete e;
}

const char* dm_f32_last_error(dm_f32_net* e) { return e ? e->err.c_str() : g_create_error32.c_str(); }

int dm_f32_prof_enable(dm_f32_net* e, int on) {
    if (!e) return 1;
    e->prof = on != 0;
    return 0;
}

int dm_f32_prof_read(dm_f32_net* e, double* gemm_ms, double* gemm_flops, int64_t* gemm_launches, double* attn_ms, double* attn_flops,
                     int64_t* attn_launches) {
    if (!e) return 1;
    DM_HIP(e, hipSetDevice(e->device));
    FILE* dump = nullptr;          // DM_PROF_DUMP=<file>: one line per timed launch (kind M N K mode flops ms) for tools/prof_shapes.py
    if (const char* dp = getenv("DM_PROF_DUMP")) dump = fopen(dp, "a");
    for (auto& ev : e->evs) {
        DM_HIP(e, hipEventSynchronize(ev.b));
        float ms = 0.f;
        DM_HIP(e, hipEventElapsedTime(&ms, ev.a, ev.b));
        if (dump) fprintf(dump, "%d %d %d %d %d %.0f %.6f\n", ev.kind, ev.M, ev.N, ev.K, ev.mode, ev.flops, ms);
        e->prof_ms[ev.kind] += ms; e->prof_flops[ev.kind] += ev.flops; e->prof_n[ev.kind] += 1;
        e->ev_pool.push_back(ev.a); e->ev_pool.push_back(ev.b);
    }
    if (dump) fclose(dump);
    e->evs.clear();
    if (gemm_ms) *gemm_ms = e->prof_ms[0];
    if (gemm_flops) *gemm_flops = e->prof_flops[0];
    if (gemm_launches) *gemm_launches = e->prof_n[0];
    if (attn_ms) *attn_ms = e->prof_ms[1];
    if (attn_flops) *attn_flops = e->prof_flops[1];
    if (attn_launches) *attn_launches = e->prof_n[1];
    for (int k = 0; k < 2; ++k) { e->prof_ms[k] = 0; e->prof_flops[k] = 0; e->prof_n[k] = 0; }
    return 0;
}

int dm_f32_memory(dm_f32_net* e, size_t* weights_bytes, size_t* arena_bytes) {
    if (!e) return 1;
    if (weights_bytes) *weights_bytes = e->w_unet.bytes + e->w_vae.bytes + e->w_vaed.bytes + e->w_clip.bytes + e->w_clipv.bytes + e->w_clipt.bytes;
    if (arena_bytes) *arena_bytes = e->arena_cap;
    return 0;
}

/* operator-level entry points of the parity tests (tests/test_gpu_f32.py) */
int dm_f32_op_gemm(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb, const void* res, void* Y,
                   int N, int H, int W, int OH, int OW, int Cin, int C1, int Cout, int mode, int temb_ld) {
    GemmParams p;
    p.X = (const float*)X; p.X2 = (const float*)X2; p.Wp = (const float*)Wp; p.bias = (const float*)bias; p.temb = (const float*)temb;
    p.res = (const float*)res; p.Y = (float*)Y; p.Cout = Cout; p.Cin = Cin; p.C1 = C1; p.mode = mode; p.ldy = Cout; p.ldres = Cout; p.temb_ld = temb_ld;
    if (mode == 0) { p.M = N * H * W; p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; }
    else { p.M = N * OH * OW; p.H = H; p.W = W; p.OH = OH; p.OW = OW; }
    return launch_gemm(p, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_attention(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo,
                        int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot, int n_slots, int B, int heads, int Tq,
                        int Tk, int D, float scale) {
    AttnParams a;
    a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V; a.O = (float*)O; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.bsq = bsq; a.bsk = bsk; a.bsv = bsv; a.bso = bso; a.kv_slot = kv_slot; a.n_slots = n_slots; a.B = B; a.heads = heads; a.Tq = Tq; a.Tk = Tk;
    a.D = D; a.scale = scale;
    return launch_attention(a, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_groupnorm(void* stream, const void* X, const void* X2, int N, int HW, int C, int C1, int G, float eps, const float* gamma,
                        const float* beta, int silu, void* stats_work, void* Y) {
    hipStream_t s = (hipStream_t)stream;
    if (launch_gn_stats((const float*)X, (const float*)X2, N, HW, C, C1, G, eps, (float*)stats_work, s) != hipSuccess) return 1;
    return launch_gn_apply((const float*)X, (const float*)X2, N, HW, C, C1, G, gamma, beta, (const float*)stats_work, silu, (float*)Y, s) == hipSuccess ? 0 : 1;
}

/* the kernels of the parallel-dataset generator (pnp.hip), one by one */
int dm_f32_op_ddim_step(void* stream, const void* x, const void* eps, const float* coef4, int64_t n, void* out) {
    return launch_ddim_step((const float*)x, (const float*)eps, nullptr, 0.f, coef4, (long long)n, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_ddim_step_cfg(void* stream, const void* x, const void* eps_u, const void* eps_c, float g, const float* coef4, int64_t n, void* out) {
    if (!eps_c) return 1;
    return launch_ddim_step((const float*)x, (const float*)eps_u, (const float*)eps_c, g, coef4, (long long)n, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_bcast_add(void* stream, const void* R, const void* Hs, int B, int64_t per, void* Y) {
    return launch_bcast_add((const float*)R, (const float*)Hs, B, (long long)per, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_decoder_tail(void* stream, const void* X, const void* stats, const float* gamma, const float* beta, const void* Wp, const float* bias,
                           int B, int H, int W, int C, int raw, void* out_f32, void* out_u8) {
    return launch_decoder_tail((const float*)X, (const float*)stats, gamma, beta, (const float*)Wp, bias, B, H, W, C, raw, (float*)out_f32, (uint8_t*)out_u8,
                               (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

/* conv_out of the two-kernel tail (X NHWC [B,H,W,C] already normalised, Wp [Cout <= 8][9 C], Y NCHW): what the fused tail is measured against */
int dm_f32_op_conv_out(void* stream, const void* X, const void* Wp, const float* bias, int B, int H, int W, int C, int Cout, void* Y) {
    return launch_conv_out((const float*)X, (const float*)Wp, bias, B, H, W, C, Cout, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_layernorm(void* stream, const void* X, int rows, int C, const float* gamma, const float* beta, float eps, void* Y) {
    return launch_layernorm((const float*)X, rows, C, gamma, beta, eps, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

/* the patch-token head's first half: LayerNorm of rows 1 .. T-1 of every image, X [n][T][C] -> Y [n*(T-1)][C] */
int dm_f32_op_clip_patch_ln(void* stream, const void* X, int n, int T, int C, const float* gamma, const float* beta, float eps, void* Y) {
    return launch_clip_tower_patch_ln((const float*)X, n, T, C, gamma, beta, eps, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

/* the glue kernels of f32_ops.hip one by one (tests/test_gpu_glue.py): one launch each, no arithmetic of their own; a null required pointer, a
 * non-positive extent or a violated precondition of the kernel returns 1 before anything is launched */
int dm_f32_op_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, int rows, int T, int C, int vocab, void* out) {
    if (!ids || !tok || !pos || !out || rows <= 0 || T < 1 || C <= 0 || vocab < 1) return 1;
    return launch_clip_embed(ids, (const float*)tok, (const float*)pos, rows, T, C, vocab, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_clip_attention(void* stream, const void* qkv, int n, int T, int heads, int causal, void* out) {
    if (!qkv || !out || n <= 0 || heads < 1 || heads > 65535) return 1;
    return launch_clip_attention((const float*)qkv, n, T, heads, causal != 0, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;   // (T, causal): refused there
}

int dm_f32_op_quick_gelu(void* stream, void* x, int64_t n) {
    if (!x || n <= 0) return 1;
    return launch_quick_gelu((float*)x, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_silu(void* stream, const void* in, void* out, int64_t n) {
    if (!in || !out || n <= 0) return 1;
    return launch_silu((const float*)in, (float*)out, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_timestep_embed(void* stream, const int64_t* t, int B, int dim, void* out) {
    if (!t || !out || B <= 0 || dim < 2 || dim % 2 || (long long)B * (dim / 2) > 0x7fffffffLL - 255) return 1;
    return launch_timestep_embed(t, B, dim, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_conv_in(void* stream, const void* x, const void* w, const float* bias, int B, int Cin, int H, int W, int Cout, void* y) {
    if (!x || !w || !bias || !y || B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 1;
    return launch_conv_in((const float*)x, (const float*)w, bias, B, Cin, H, W, Cout, (float*)y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_add_noise(void* stream, const void* x, const int32_t* x_index, const void* eps, const int64_t* t, const float* sa, const float* sb, int B,
                        int64_t per, void* out) {
    if (!x || !eps || !t || !sa || !sb || !out || B <= 0 || per <= 0) return 1;
    return launch_add_noise((const float*)x, x_index, (const float*)eps, t, sa, sb, B, (long long)per, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_sqerr(void* stream, const void* pred, const void* eps, int64_t n, void* out) {
    if (!pred || !eps || !out || n <= 0) return 1;
    return launch_sqerr((const float*)pred, (const float*)eps, (long long)n, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_nhwc_to_nchw(void* stream, const void* X, int N, int HW, int C, void* Y) {
    if (!X || !Y || N <= 0 || HW <= 0 || C <= 0) return 1;
    return launch_nhwc_to_nchw((const float*)X, N, HW, C, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_ensemble_mean(void* stream, const void* X, int groups, int ens, int HW, int C, void* Y) {
    if (!X || !Y || groups <= 0 || ens < 1 || HW <= 0 || C <= 0) return 1;
    return launch_ensemble_mean((const float*)X, groups, ens, HW, C, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_posterior(void* stream, const void* Hm, const void* qw, const void* qb, const void* noise, int B, int draws, int HW, float scaling,
                        void* latent, void* moments) {
    if (!Hm || !qw || !qb || B <= 0 || draws < 1 || HW <= 0 || (!latent && !moments)) return 1;
    return launch_posterior((const float*)Hm, (const float*)qw, (const float*)qb, (const float*)noise, B, draws, HW, scaling, (float*)latent,
                            (float*)moments, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

/* the gradient operators of the convolutional blocks (f32_train.hip; tests/test_gpu_train_ops.py): a null required pointer, a channel count
 * the kernel cannot take, a workspace that is too small or a mode outside 0 .. 3 returns 1 before anything is launched */
static long long wgrad_rows(int N, int H, int W, int OH, int OW, int mode) {
    if (N <= 0 || H <= 0 || W <= 0 || (mode != 0 && (OH <= 0 || OW <= 0))) return 0;
    return mode == 0 ? (long long)N * H * W : (long long)N * OH * OW;
}

size_t dm_f32_op_gemm_wgrad_workspace(int N, int H, int W, int OH, int OW, int Cin, int Cout, int mode) {
    if (mode < 0 || mode > 3) return 0;
    return wgrad_workspace_bytes(wgrad_rows(N, H, W, OH, OW, mode), Cout, Cin, mode);
}

int dm_f32_op_gemm_wgrad(void* stream, const void* X, const void* X2, const void* dY, void* dWp, void* work, size_t work_bytes, int N, int H, int W,
                         int OH, int OW, int Cin, int C1, int Cout, int mode, int accumulate) {
    if (mode < 0 || mode > 3) return 1;
    const long long M = wgrad_rows(N, H, W, OH, OW, mode);
    if (M <= 0 || M > 0x7fffffffLL - 4096) return 1;
    if (mode == 2 && (OH != (H + 1) / 2 || OW != (W + 1) / 2)) return 1;
    if (mode == 1 && (OH != H || OW != W)) return 1;
    return launch_wgrad((const float*)X, (const float*)X2, (const float*)dY, (int)M, mode == 0 ? 1 : H, mode == 0 ? (int)M : W, mode == 0 ? 1 : OH,
                        mode == 0 ? (int)M : OW, Cin, C1, Cout, mode, accumulate != 0, (float*)work, work_bytes, (float*)dWp, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_colsum(void* stream, const void* dY, int N, int HW, int C, int accumulate, void* out) {
    return launch_colsum((const float*)dY, N, HW, C, accumulate != 0, (float*)out, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_groupnorm_bwd(void* stream, const void* X, const void* X2, const void* dY, int N, int HW, int C, int C1, int G, const float* gamma,
                            const float* beta, const void* stats, int silu, void* work, size_t work_bytes, void* dX, void* dX2, void* dgamma,
                            void* dbeta) {
    return launch_gn_bwd((const float*)X, (const float*)X2, (const float*)dY, N, HW, C, C1, G, gamma, beta, (const float*)stats, silu != 0, work, work_bytes,
                         (float*)dX, (float*)dX2, (float*)dgamma, (float*)dbeta, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_silu_bwd(void* stream, const void* x, const void* dy, void* dx, int64_t n) {
    return launch_silu_bwd((const float*)x, (const float*)dy, (float*)dx, (long long)n, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_zero_insert2(void* stream, const void* dY, int N, int H, int W, int C, void* Z) {
    return launch_zero_insert2((const float*)dY, N, H, W, C, (float*)Z, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_nearest_bwd(void* stream, const void* dU, int N, int H, int W, int OH, int OW, int C, void* dS) {
    return launch_nearest_bwd((const float*)dU, N, H, W, OH, OW, C, (float*)dS, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

/* the gradient operators of the transformer blocks (f32_train_attn.hip, f32_train.hip; tests/test_gpu_train_tfm_ops.py) */
size_t dm_f32_op_attention_bwd_workspace(int B, int heads, int Tq, int Tk, int D) { return attn_bwd_workspace_bytes(B, heads, Tq, Tk, D); }

int dm_f32_op_attention_bwd_slabs(int Tq, int Tk) { return Tq > 0 && Tk > 0 ? attn_bwd_slabs(Tq, Tk, nullptr) : 0; }

int dm_f32_op_attention_bwd_phases(void* stream, const void* Q, const void* K, const void* V, const void* O, const void* dO, void* dQ, void* dK, void* dV,
                                   const int32_t* ld8, const int64_t* bs8, const int32_t* kv_slot, int B, int heads, int Tq, int Tk, int D, float scale,
                                   void* work, size_t work_bytes, int phases) {
    if (!ld8 || !bs8 || kv_slot) return 1;
    AttnBwdParams a;
    a.Q = (const float*)Q; a.K = (const float*)K; a.V = (const float*)V; a.O = (const float*)O; a.dO = (const float*)dO;
    a.dQ = (float*)dQ; a.dK = (float*)dK; a.dV = (float*)dV;
    a.ldq = ld8[0]; a.ldk = ld8[1]; a.ldv = ld8[2]; a.ldo = ld8[3]; a.lddo = ld8[4]; a.lddq = ld8[5]; a.lddk = ld8[6]; a.lddv = ld8[7];
    a.bsq = bs8[0]; a.bsk = bs8[1]; a.bsv = bs8[2]; a.bso = bs8[3]; a.bsdo = bs8[4]; a.bsdq = bs8[5]; a.bsdk = bs8[6]; a.bsdv = bs8[7];
    a.B = B; a.heads = heads; a.Tq = Tq; a.Tk = Tk; a.D = D; a.scale = scale; a.work = work; a.work_bytes = work_bytes; a.phases = phases;
    return launch_attention_bwd(a, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_attention_bwd(void* stream, const void* Q, const void* K, const void* V, const void* O, const void* dO, void* dQ, void* dK, void* dV,
                            const int32_t* ld8, const int64_t* bs8, const int32_t* kv_slot, int B, int heads, int Tq, int Tk, int D, float scale,
                            void* work, size_t work_bytes) {
    return dm_f32_op_attention_bwd_phases(stream, Q, K, V, O, dO, dQ, dK, dV, ld8, bs8, kv_slot, B, heads, Tq, Tk, D, scale, work, work_bytes, 15);
}

size_t dm_f32_op_layernorm_bwd_workspace(int rows, int C) { return ln_bwd_workspace_bytes(rows, C); }

int dm_f32_op_layernorm_bwd(void* stream, const void* X, const void* dY, int rows, int C, const float* gamma, float eps, void* work, size_t work_bytes,
                            void* dX, void* dgamma, void* dbeta) {
    return launch_layernorm_bwd((const float*)X, (const float*)dY, rows, C, gamma, eps, work, work_bytes, (float*)dX, (float*)dgamma, (float*)dbeta,
                                (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_geglu(void* stream, const void* P, int M, int F, void* Y) {
    return launch_geglu((const float*)P, M, F, (float*)Y, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

int dm_f32_op_geglu_bwd(void* stream, const void* P, const void* dY, int M, int F, void* dP) {
    return launch_geglu_bwd((const float*)P, (const float*)dY, M, F, (float*)dP, (hipStream_t)stream) == hipSuccess ? 0 : 1;
}

}  // extern "C"
