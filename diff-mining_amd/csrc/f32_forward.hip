// f32_forward.hip — the SDv1.5 U-Net in plain fp32 on the fp32 matrix cores: the arithmetic of the reference's DIFT featuriser.
//
// `SDFeaturizer.__init__` (diffmining/typicality/dift.py:197-199) builds `OneStepSDPipeline.from_pretrained(sd_id, unet=unet,
// safety_checker=None)` with NO torch_dtype and calls the U-Net with NO autocast (dift.py:191): every tensor and every product
// of that path is fp32.  The fp16 engine (engine*.hip) reproduces the autocast arithmetic of the typicality path
// (compute.py:98-101); the fp32 net (f32_*.hip, f32_impl.h) is the second arithmetic the reference uses, behind its own C-ABI handle
// (include/dm_engine.h, dm_f32_*): fp32 weights, fp32 NHWC activations, v_mfma_f32_16x16x4_f32 GEMMs (f32_gemm.hip) and attention
// (f32_ops.hip).  It runs the whole U-Net (dm_f32_unet_forward) or the early exit after up_blocks[i] (dm_f32_dift), so it is also
// the full-size fp32 ground truth on the GPU that the CPU oracle is too slow for.
//
// This file: the operators (Fwd32) every fp32 schedule is written in; the U-Net's schedule = MyUNet2DConditionModel.forward (dift.py:24-169) op
// by op, nothing folded or fused beyond the GEMM epilogue (bias, time embedding, residual), cross-attention K/V projected once per
// registered prompt; its chunked runner and entry points; the DDIM and Plug-and-Play loops over it.
#include "f32_impl.h"

#include <cmath>

using namespace dm32;
using namespace sd15;
using namespace dm::f32;

int Fwd32::alloc(T32* t, int N, int H, int W, int C) {
    t->N = N; t->H = H; t->W = W; t->C = C;
    const size_t bytes = (size_t)N * H * W * C * sizeof(float);
    t->off = e->arena.alloc(bytes);
    if (t->off == NONE) DM_FAIL(e, "fp32 workspace arena exhausted (%zu bytes requested)", bytes);
    t->p = reinterpret_cast<float*>(e->arena_base + t->off);
    return 0;
}
void Fwd32::free(T32& t) { if (t.off != NONE) { e->arena.release(t.off); t.off = NONE; t.p = nullptr; } }
int Fwd32::prof_begin(int kind, double flops, int M, int N, int K, int mode) {
    if (!e->prof || dry) return 0;
    Ev ev; ev.flops = flops; ev.kind = kind; ev.M = M; ev.N = N; ev.K = K; ev.mode = mode;
    for (hipEvent_t* h : {&ev.a, &ev.b}) {
        if (!e->ev_pool.empty()) { *h = e->ev_pool.back(); e->ev_pool.pop_back(); }
        else DM_HIP(e, hipEventCreate(h));
    }
    DM_HIP(e, hipEventRecord(ev.a, s));
    e->evs.push_back(ev);
    return 0;
}
int Fwd32::prof_end() { if (e->prof && !dry) DM_HIP(e, hipEventRecord(e->evs.back().b, s)); return 0; }

int Fwd32::gemm(const Conv& cv, int mode, const T32& x, const T32* x2, int OH, int OW, const float* temb, int temb_ld, const T32* res, T32* y, int epi) {
    const int cin = x.C + (x2 ? x2->C : 0);
    if (cin != cv.cin) DM_FAIL(e, "gemm32: channel mismatch %d vs %d", cin, cv.cin);
    const int cy = epi == 1 ? cv.cout / 2 : cv.cout;
    DM_TRY(alloc(y, x.N, OH, OW, cy));
    if (dry) return 0;
    GemmParams p;
    p.epi = epi;
    p.X = x.p; p.X2 = x2 ? x2->p : nullptr; p.Wp = P(cv.w); p.bias = P(cv.b); p.temb = temb; p.res = res ? res->p : nullptr; p.Y = y->p;
    p.Cout = cv.cout; p.Cin = cin; p.C1 = x.C; p.mode = mode; p.ldy = cy; p.ldres = res ? res->C : 0; p.temb_ld = temb_ld;
    if (mode == 0) { p.M = (int)x.rows(); p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; }
    else { p.M = x.N * OH * OW; p.H = x.H; p.W = x.W; p.OH = OH; p.OW = OW; }
    DM_TRY(prof_begin(0, 2.0 * (double)p.M * cv.cout * (double)((mode == 0 ? 1 : 9) * cin), p.M, cv.cout, (mode == 0 ? 1 : 9) * cin, mode));
    DM_HIP(e, launch_gemm(p, s));
    return prof_end();
}
int Fwd32::upconv4(const Conv& cv, const T32& x, T32* y) {      // FLOPs booked = executed (4 taps)
    if (x.C != cv.cin) DM_FAIL(e, "upconv4 (fp32): channel mismatch %d vs %d", x.C, cv.cin);
    DM_TRY(alloc(y, x.N, 2 * x.H, 2 * x.W, cv.cout));
    if (dry) return 0;
    GemmParams p;
    p.X = x.p; p.Wp = P(cv.w); p.bias = P(cv.b); p.Y = y->p;
    p.Cout = cv.cout; p.Cin = x.C; p.C1 = x.C; p.mode = 5; p.ldy = cv.cout;
    p.M = x.N * x.H * x.W; p.H = x.H; p.W = x.W; p.OH = x.H; p.OW = x.W;
    DM_TRY(prof_begin(0, 2.0 * 4.0 * (double)p.M * cv.cout * 4.0 * (double)x.C, 4 * p.M, cv.cout, 4 * x.C, 5));
    DM_HIP(e, launch_gemm(p, s));
    return prof_end();
}
int Fwd32::groupnorm(const Norm& nw, const T32& x, const T32* x2, float eps, bool silu, T32* y) {
    const int C = x.C + (x2 ? x2->C : 0);
    if (C != nw.c) DM_FAIL(e, "groupnorm32: channel mismatch %d vs %d", C, nw.c);
    T32 st;
    DM_TRY(alloc(&st, 1, 1, x.N * GROUPS, 2));
    DM_TRY(alloc(y, x.N, x.H, x.W, C));
    if (!dry) {
        DM_HIP(e, launch_gn_stats(x.p, x2 ? x2->p : nullptr, x.N, x.H * x.W, C, x.C, GROUPS, eps, st.p, s));
        DM_HIP(e, launch_gn_apply(x.p, x2 ? x2->p : nullptr, x.N, x.H * x.W, C, x.C, GROUPS, P(nw.g), P(nw.b), st.p, silu ? 1 : 0, y->p, s));
    }
    free(st);
    return 0;
}
int Fwd32::layernorm(const Norm& nw, const T32& x, T32* y) {
    DM_TRY(alloc(y, x.N, x.H, x.W, x.C));
    if (!dry) DM_HIP(e, launch_layernorm(x.p, (int)x.rows(), x.C, P(nw.g), P(nw.b), LN_EPS, y->p, s));
    return 0;
}
// ResnetBlock2D.  inject (Plug-and-Play's feature injection, pnp.py:345-350; sample 0 = the source): norm1 .. conv2 run for the source
// alone, and every sample's output is shortcut(x_n) + h_src — one addition, `input_tensor + hidden_states` (pnp.py:357); for the source
// that is the sum the fused epilogue forms ((acc + bias) + residual), so its row does not change
int Fwd32::resnet(const Res& r, const T32& x, const T32* x2, const float* tproj, T32* out, bool inject) {
    T32 n1, h1, n2, sc, xs = x, x2s;
    if (inject) { xs.N = 1; if (x2) { x2s = *x2; x2s.N = 1; } }
    const T32& xa = inject ? xs : x;
    const T32* x2a = (inject && x2) ? &x2s : x2;
    DM_TRY(groupnorm(r.n1, xa, x2a, res_eps, true, &n1));
    DM_TRY(gemm(r.c1, 1, n1, nullptr, x.H, x.W, tproj ? tproj + r.temb_off : nullptr, e->tproj_total, nullptr, &h1));
    free(n1);
    DM_TRY(groupnorm(r.n2, h1, nullptr, res_eps, true, &n2));
    free(h1);
    const T32* resid = &x;
    if (r.has_sc) { DM_TRY(dense(r.sc, x, x2, nullptr, &sc)); resid = &sc; }
    else if (x2) DM_FAIL(e, "resnet32: concat input without shortcut conv");
    if (!inject) DM_TRY(gemm(r.c2, 1, n2, nullptr, x.H, x.W, nullptr, 0, resid, out));
    else {
        T32 hs;
        DM_TRY(gemm(r.c2, 1, n2, nullptr, x.H, x.W, nullptr, 0, nullptr, &hs));
        DM_TRY(alloc(out, x.N, x.H, x.W, r.c2.cout));
        if (!dry) DM_HIP(e, launch_bcast_add(resid->p, hs.p, x.N, (long long)x.H * x.W * r.c2.cout, out->p, s));
        free(hs);
    }
    free(n2);
    if (r.has_sc) free(sc);
    return 0;
}
// bsk < 0: K shares V's batch stride (every caller but the self-attention injection)
int Fwd32::attention(const float* Q, int ldq, long long bsq, const float* K, const float* V, int ldkv, long long bskv, const int32_t* slots,
              int B, int Tq, int Tk, int C, float* O, int heads, long long bsk) {
    AttnParams a;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = C;
    a.bsq = bsq; a.bsk = bsk < 0 ? bskv : bsk; a.bsv = bskv; a.bso = (long long)Tq * C;
    a.kv_slot = slots; a.n_slots = e->n_prompts; a.B = B; a.heads = heads; a.Tq = Tq; a.Tk = Tk; a.D = C / heads;
    a.scale = 1.0f / sqrtf((float)a.D);
    DM_TRY(prof_begin(1, 4.0 * B * heads * (double)Tq * Tk * a.D, B * Tq, Tk, a.D, Tq == Tk ? 100 : 101));
    DM_HIP(e, launch_attention(a, s));
    return prof_end();
}
// Transformer2DModel + BasicTransformerBlock.  src_qk (Plug-and-Play's self-attention injection, pnp.py:424-432): every sample attends with
// the queries and keys of sample 0 (the source) and its own values — batch strides of 0 for Q and K, no copy
int Fwd32::transformer(const Tfm& t, const T32& x, const int32_t* slots, T32* out, bool src_qk) {
    const int C = t.c, T = x.H * x.W, B = x.N;
    T32 n, t0, ln, qkv, a, t1, q, t2, ff, t3;
    DM_TRY(groupnorm(t.gn, x, nullptr, ATTN_GN_EPS, false, &n));
    DM_TRY(dense(t.proj_in, n, nullptr, nullptr, &t0));
    free(n);
    DM_TRY(layernorm(t.ln1, t0, &ln));
    DM_TRY(dense(t.qkv, ln, nullptr, nullptr, &qkv));
    free(ln);
    DM_TRY(alloc(&a, B, x.H, x.W, C));
    if (!dry) DM_TRY(attention(qkv.p, 3 * C, src_qk ? 0 : (long long)T * 3 * C, qkv.p + C, qkv.p + 2 * C, 3 * C, (long long)T * 3 * C, nullptr, B, T, T, C, a.p,
                               HEADS, src_qk ? 0 : -1));
    free(qkv);
    DM_TRY(dense(t.o1, a, nullptr, &t0, &t1));
    free(a); free(t0);
    DM_TRY(layernorm(t.ln2, t1, &ln));
    DM_TRY(dense(t.q2, ln, nullptr, nullptr, &q));
    free(ln);
    DM_TRY(alloc(&a, B, x.H, x.W, C));
    if (!dry) {
        const float* kv = e->kv_cache[t.layer];
        DM_TRY(attention(q.p, C, (long long)T * C, kv, kv + C, 2 * C, (long long)CTX_LEN * 2 * C, slots, B, T, CTX_LEN, C, a.p));
    }
    free(q);
    DM_TRY(dense(t.o2, a, nullptr, &t1, &t2));
    free(a); free(t1);
    DM_TRY(layernorm(t.ln3, t2, &ln));
    DM_TRY(gemm(t.ff1, 0, ln, nullptr, x.H, x.W, nullptr, 0, nullptr, &ff, 1));        // GEGLU in the epilogue: [tokens][4C]
    free(ln);
    DM_TRY(dense(t.ff2, ff, nullptr, &t2, &t3));
    free(ff); free(t2);
    DM_TRY(dense(t.proj_out, t3, nullptr, &x, out));
    free(t3);
    return 0;
}
// CLIPEncoderLayer of width H (heads of H / heads, MLP of Fi) on n sequences of T tokens, x [n * T][H] replaced by the layer's output:
// LN1 -> q|k|v -> attention -> out_proj + residual -> LN2 -> fc1 -> quick_gelu -> fc2 + residual.  The attention over the stacked q|k|v
// rows runs a whole sequence per block (the text tower, causal, and ViT-B/32), or on the MFMA flash kernel (attn32_kernel<64>; heads of
// 64, scale 1/8 exact): a sequence-per-block kernel does not hold the configurable tower's 577 tokens
int Fwd32::clip_layer(const ClipLayer32& L, int n, int T, int H, int heads, int Fi, ClipAttn attn, T32* x) {
    const int M = n * T;
    T32 h, qkv, a, x1, f, x2;
    DM_TRY(layernorm(L.ln1, *x, &h));
    DM_TRY(dense(L.qkv, h, nullptr, nullptr, &qkv));
    free(h);
    DM_TRY(alloc(&a, 1, 1, M, H));
    if (!dry) {
        if (attn == CLIP_ATTN_FLASH) DM_TRY(attention(qkv.p, 3 * H, (long long)T * 3 * H, qkv.p + H, qkv.p + 2 * H, 3 * H, (long long)T * 3 * H, nullptr, n, T, T, H, a.p, heads));
        else DM_HIP(e, launch_clip_attention(qkv.p, n, T, heads, attn == CLIP_ATTN_SEQ_CAUSAL, a.p, s));
    }
    free(qkv);
    DM_TRY(dense(L.o, a, nullptr, x, &x1));
    free(a); free(*x);
    DM_TRY(layernorm(L.ln2, x1, &h));
    DM_TRY(dense(L.fc1, h, nullptr, nullptr, &f));
    free(h);
    if (!dry) DM_HIP(e, launch_quick_gelu(f.p, (long long)M * Fi, s));
    DM_TRY(dense(L.fc2, f, nullptr, &x1, &x2));
    free(f); free(x1);
    *x = x2;
    return 0;
}

int dm::f32::run_forward32(dm_f32_net* e, const Args32& A, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_unet.slab};
    const int B = A.B;
    T32 te0, e1, e1s, emb, embs, tproj;
    DM_TRY(F.alloc(&te0, 1, 1, B, BOC[0]));
    if (!dry) DM_HIP(e, launch_timestep_embed(A.t, B, BOC[0], te0.p, s));
    DM_TRY(F.dense(e->time1, te0, nullptr, nullptr, &e1));
    F.free(te0);
    DM_TRY(F.alloc(&e1s, 1, 1, B, TEMB));
    if (!dry) DM_HIP(e, launch_silu(e1.p, e1s.p, (long long)B * TEMB, s));
    F.free(e1);
    DM_TRY(F.dense(e->time2, e1s, nullptr, nullptr, &emb));
    F.free(e1s);
    DM_TRY(F.alloc(&embs, 1, 1, B, TEMB));
    if (!dry) DM_HIP(e, launch_silu(emb.p, embs.p, (long long)B * TEMB, s));
    F.free(emb);
    DM_TRY(F.dense(e->tproj_all, embs, nullptr, nullptr, &tproj));
    F.free(embs);

    T32 h;
    DM_TRY(F.alloc(&h, B, A.H, A.W, BOC[0]));
    if (!dry) DM_HIP(e, launch_conv_in(A.x, F.P(e->conv_in.w), F.P(e->conv_in.b), B, 4, A.H, A.W, BOC[0], h.p, s));
    std::vector<T32> skips;
    skips.push_back(h);
    T32 cur = h;                     // aliases the newest skip (not freed here)
    for (int i = 0; i < NB; ++i) {
        const DownB& d = e->down[i];
        for (int j = 0; j < LAYERS; ++j) {
            T32 r;
            DM_TRY(F.resnet(d.res[j], cur, nullptr, tproj.p, &r));
            if (d.attn) { T32 a; DM_TRY(F.transformer(d.tf[j], r, A.slots, &a)); F.free(r); r = a; }
            skips.push_back(r);
            cur = r;
        }
        if (d.has_down) {
            T32 dn;
            DM_TRY(F.gemm(d.down, 2, cur, nullptr, (cur.H + 1) / 2, (cur.W + 1) / 2, nullptr, 0, nullptr, &dn));
            skips.push_back(dn);
            cur = dn;
        }
    }
    T32 m0, m1, m2;
    DM_TRY(F.resnet(e->mid_res[0], cur, nullptr, tproj.p, &m0, (A.conv_mask >> 12) & 1));
    DM_TRY(F.transformer(e->mid_tf, m0, A.slots, &m1, (A.attn_mask >> 12) & 1));
    F.free(m0);
    DM_TRY(F.resnet(e->mid_res[1], m1, nullptr, tproj.p, &m2, (A.conv_mask >> 13) & 1));
    F.free(m1);
    cur = m2;                        // owned from here on
    const bool fwd_up_size = (A.H % 8 != 0) || (A.W % 8 != 0);          // dift.py:54-56
    for (int i = 0; i < NB; ++i) {
        if (A.up_ft_index >= 0 && i > A.up_ft_index) break;
        const UpB& u = e->up[i];
        for (int j = 0; j < LAYERS + 1; ++j) {
            T32 skip = skips.back(); skips.pop_back();
            T32 r;
            DM_TRY(F.resnet(u.res[j], cur, &skip, tproj.p, &r, (A.conv_mask >> (3 * i + j)) & 1));
            F.free(cur); F.free(skip);
            if (u.attn) { T32 a; DM_TRY(F.transformer(u.tf[j], r, A.slots, &a, (A.attn_mask >> (3 * i + j)) & 1)); F.free(r); r = a; }
            cur = r;
        }
        if (u.has_up) {
            int OH = cur.H * 2, OW = cur.W * 2;
            if (fwd_up_size && !skips.empty()) { OH = skips.back().H; OW = skips.back().W; }
            T32 upc;
            // exact 2x: four 2x2 convolutions on the source grid (4/9 of the MACs; option up_fold, as the fp16 engine)
            if (dm::option(dm::OPT_UP_FOLD) && u.has_up4 && OH == 2 * cur.H && OW == 2 * cur.W) DM_TRY(F.upconv4(u.up4, cur, &upc));
            else DM_TRY(F.gemm(u.up, 3, cur, nullptr, OH, OW, nullptr, 0, nullptr, &upc));
            F.free(cur);
            cur = upc;
        }
        if (A.up_ft_index == i && !dry) {
            if (A.feat) DM_HIP(e, launch_nhwc_to_nchw(cur.p, cur.N, cur.H * cur.W, cur.C, A.feat, s));
            if (A.feat_mean) DM_HIP(e, launch_ensemble_mean(cur.p, cur.N / A.ensemble, A.ensemble, cur.H * cur.W, cur.C, A.feat_mean, s));
        }
    }
    if (A.up_ft_index < 0) {
        T32 nrm;
        DM_TRY(F.groupnorm(e->norm_out, cur, nullptr, GN_EPS, true, &nrm));
        if (!dry) DM_HIP(e, launch_conv_out(nrm.p, F.P(e->conv_out.w), F.P(e->conv_out.b), B, A.H, A.W, BOC[0], 4, A.out, s));
        F.free(nrm);
    }
    F.free(cur);
    for (auto& sk : skips) F.free(sk);
    F.free(tproj);
    return 0;
}

namespace {

// samples per run: the widest intermediate is the GEGLU projection ([tokens][8 C] fp32 = 42 MB per sample at a 64 x 64 latent)
int chunk32(int h, int w) {
    const long long area = (long long)h * w;
    long long c = 64LL * 4096 / (area > 0 ? area : 1);
    return (int)(c < 1 ? 1 : (c > 1024 ? 1024 : c));
}

// a loop's tables -> its buffer: the timestep of step i for each of `rows` samples, t_dev [n_steps][rows], and coef [n_steps][4]
int loop_tables32(dm_f32_net* e, hipStream_t s, const int64_t* t_host, const float* coef_host, int n_steps, int rows, int64_t* t_dev, float* coef) {
    std::vector<int64_t> tt((size_t)n_steps * rows);
    for (int i = 0; i < n_steps; ++i) for (int b = 0; b < rows; ++b) tt[(size_t)i * rows + b] = t_host[i];
    // the loop buffer is shared by every loop of this net: an earlier loop queued on `s` may still read its tables, and the blocking copy
    // runs on the null stream, which a non-blocking `s` is not ordered with — so the queue drains first (once, before the loop)
    DM_HIP(e, hipStreamSynchronize(s));
    DM_HIP(e, hipMemcpy(t_dev, tt.data(), tt.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    DM_HIP(e, hipMemcpy(coef, coef_host, (size_t)n_steps * 4 * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
// the arena sized for A, then (`run`) the forward; the loops size theirs before they start
int run32(dm_f32_net* e, const Args32& A, hipStream_t s, bool run = true) {
    const std::vector<long long> key = {KEY_UNET, A.B, A.H, A.W, A.up_ft_index, A.conv_mask};
    auto fwd = [&](bool dry) { return run_forward32(e, A, s, dry); };
    return run ? run_sized32(e, s, key, fwd) : ensure_arena_for32(e, s, key, fwd);
}
// the buffer of the DDIM / PnP loops (predictions, the per-step timestep rows and coefficients); grows before a loop starts, never inside one
int loop_reserve32(dm_f32_net* e, hipStream_t s, size_t bytes) {
    if (bytes <= e->loop_bytes) return 0;
    if (e->loop_buf) { DM_HIP(e, hipStreamSynchronize(s)); DM_HIP(e, hipFree(e->loop_buf)); e->loop_buf = nullptr; e->loop_bytes = 0; }
    DM_HIP(e, hipMalloc((void**)&e->loop_buf, bytes));
    e->loop_bytes = bytes;
    return 0;
}

int run_chunked32(dm_f32_net* e, const Args32& full, void* stream) {
    if (!e->finalized) DM_FAIL(e, "fp32 net not finalized");
    if (e->n_prompts <= 0) DM_FAIL(e, "dm_f32_set_prompts must be called first");
    if (full.B <= 0 || full.H < 1 || full.W < 1) DM_FAIL(e, "bad batch / latent size");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int chunk = chunk32(full.H, full.W);
    if (full.feat_mean) {                       // an ensemble never straddles two runs
        if (full.ensemble <= 0 || full.B % full.ensemble != 0) DM_FAIL(e, "batch %d is not a multiple of ensemble %d", full.B, full.ensemble);
        chunk = chunk >= full.ensemble ? chunk / full.ensemble * full.ensemble : full.ensemble;
    }
    int c_out = 0, oh = 0, ow = 0;
    if (full.up_ft_index >= 0 && dm_dift_shape(full.H, full.W, full.up_ft_index, &c_out, &oh, &ow)) DM_FAIL(e, "bad up_ft_index %d", full.up_ft_index);
    for (int b0 = 0; b0 < full.B; b0 += chunk) {
        Args32 C = full;
        C.B = (full.B - b0 < chunk) ? full.B - b0 : chunk;
        C.x = at(full.x, b0, (size_t)4 * full.H * full.W);
        C.t = at(full.t, b0);
        C.slots = at(full.slots, b0);
        C.out = at(full.out, b0, (size_t)4 * full.H * full.W);
        C.feat = at(full.feat, b0, (size_t)c_out * oh * ow);
        C.feat_mean = at(full.feat_mean, b0 / full.ensemble, (size_t)c_out * oh * ow);
        DM_TRY(run32(e, C, s));
    }
    return 0;
}

}  // namespace

extern "C" {

/* ctx_dev [n_prompts][77][768] fp32: cross-attention K/V of the 16 transformer blocks for every prompt */
int dm_f32_set_prompts(dm_f32_net* e, const void* ctx_dev, int n_prompts, void* stream) {
    if (!e || !ctx_dev || n_prompts <= 0) return 1;
    if (!e->finalized) DM_FAIL(e, "set_prompts before finalize");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (n_prompts > e->kv_capacity) {
        DM_HIP(e, hipStreamSynchronize(s));
        for (float* p : e->kv_cache) if (p) DM_HIP(e, hipFree(p));
        int cap = e->kv_capacity > 0 ? e->kv_capacity : 4;
        while (cap < n_prompts) cap *= 2;
        e->kv_cache.assign(e->n_tf, nullptr);
        for (int l = 0; l < e->n_tf; ++l) DM_HIP(e, hipMalloc((void**)&e->kv_cache[l], (size_t)cap * CTX_LEN * 2 * e->tfs[l]->c * sizeof(float)));
        e->kv_capacity = cap;
    }
    e->n_prompts = n_prompts;
    const int M = n_prompts * CTX_LEN;
    for (int l = 0; l < e->n_tf; ++l) {
        const Conv& kv = e->tfs[l]->kv2;
        GemmParams p;
        p.X = (const float*)ctx_dev; p.Wp = e->w_unet.slab + kv.w; p.Y = e->kv_cache[l];
        p.M = M; p.Cout = kv.cout; p.Cin = CTX_DIM; p.C1 = CTX_DIM; p.H = 1; p.W = M; p.OH = 1; p.OW = M; p.mode = 0; p.ldy = kv.cout;
        DM_HIP(e, launch_gemm(p, s));
    }
    return 0;
}

int dm_f32_unet_forward(dm_f32_net* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
                        void* out_dev, void* stream) {
    if (!e || !sample_dev || !t_dev || !slot_dev || !out_dev) return 1;
    Args32 A{(const float*)sample_dev, t_dev, slot_dev, batch, h, w, -1, (float*)out_dev, nullptr, nullptr, 1};
    return run_chunked32(e, A, stream);
}

/* SD.compute_loss in plain fp32 — what compute.py:95-102 computes WITHOUT its autocast: noisy = add_noise(x[x_index[b]], eps[b], t[b]);
 * eps_hat = UNet(noisy, t, prompt[slot[b]]); loss = (eps_hat - eps)^2 -> loss_out_dev [batch,4,h,w] fp32.  The exact-arithmetic yardstick
 * of the fp16 engine's dm_score (bench.py's score_deviation leg, tools/t_deviation_gpu.py). */
int dm_f32_score(dm_f32_net* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev, const int64_t* t_dev,
                 const int32_t* slot_dev, int batch, int n_x, int h, int w, void* loss_out_dev, void* stream) {
    if (!e || !x_dev || !eps_dev || !t_dev || !slot_dev || !loss_out_dev || batch <= 0 || n_x <= 0) return 1;
    if (!e->finalized) DM_FAIL(e, "fp32 net not finalized");
    if (!x_index_dev && n_x != batch) DM_FAIL(e, "x has %d rows for a batch of %d and no x_index", n_x, batch);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const long long per = 4LL * h * w;
    const size_t need = (size_t)2 * batch * per;
    if (need > e->score_tmp_floats) {
        if (e->score_tmp) { DM_HIP(e, hipStreamSynchronize(s)); DM_HIP(e, hipFree(e->score_tmp)); e->score_tmp = nullptr; e->score_tmp_floats = 0; }
        DM_HIP(e, hipMalloc((void**)&e->score_tmp, need * sizeof(float)));
        e->score_tmp_floats = need;
    }
    float* noisy = e->score_tmp;
    float* pred = e->score_tmp + (size_t)batch * per;
    DM_HIP(e, launch_add_noise((const float*)x_dev, x_index_dev, (const float*)eps_dev, t_dev, e->sched_tab, e->sched_tab + 1000, batch, per, noisy, s));
    Args32 A{noisy, t_dev, slot_dev, batch, h, w, -1, pred, nullptr, nullptr, 1};
    DM_TRY(run_chunked32(e, A, stream));
    DM_HIP(e, launch_sqerr(pred, (const float*)eps_dev, (long long)batch * per, (float*)loss_out_dev, s));
    return 0;
}

int dm_f32_dift(dm_f32_net* e, const void* noisy_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
                int up_ft_index, void* feat_out_dev, void* mean_out_dev, int ensemble, void* stream) {
    if (!e || !noisy_dev || !t_dev || !slot_dev || (!feat_out_dev && !mean_out_dev)) return 1;
    if (up_ft_index < 0 || up_ft_index >= NB) DM_FAIL(e, "up_ft_index %d out of range", up_ft_index);
    Args32 A{(const float*)noisy_dev, t_dev, slot_dev, batch, h, w, up_ft_index, nullptr, (float*)feat_out_dev, (float*)mean_out_dev,
             ensemble > 0 ? ensemble : 1};
    return run_chunked32(e, A, stream);
}

/* One U-Net forward with Plug-and-Play's injection (pnp.py:345-350, :424-432): sample 0 is the source; masks of 0 = dm_f32_unet_forward */
int dm_f32_unet_forward_inject(dm_f32_net* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
                               int conv_mask, int attn_mask, void* out_dev, void* stream) {
    if (!e || !sample_dev || !t_dev || !slot_dev || !out_dev) return 1;
    if (conv_mask < 0 || attn_mask < 0 || conv_mask >= (1 << 14) || attn_mask >= (1 << 13)) DM_FAIL(e, "dm_f32_unet_forward_inject: bad layer mask");
    if ((conv_mask || attn_mask) && batch > chunk32(h, w))
        DM_FAIL(e, "dm_f32_unet_forward_inject: %d samples do not fit one run (%d at %d x %d): the source must share a run with its targets", batch, chunk32(h, w), h, w);
    Args32 A{(const float*)sample_dev, t_dev, slot_dev, batch, h, w, -1, (float*)out_dev, nullptr, nullptr, 1};
    A.conv_mask = (unsigned)conv_mask; A.attn_mask = (unsigned)attn_mask;
    return run_chunked32(e, A, stream);
}

/* n_steps DDIM updates on the device queue (pnp.py:156-203): eps = UNet(x, t_i, prompt[slot]); x = step(x, eps, coef_i); optionally
 * traj[save_row[i]] = x.  No host synchronisation inside the loop; tables uploaded and the arena sized before it. */
int dm_f32_ddim_run(dm_f32_net* e, void* x_dev, const int64_t* t_host, const float* coef_host, const int32_t* slot_dev, const int32_t* save_row_host,
                    void* traj_dev, int B, int h, int w, int n_steps, void* stream) {
    if (!e) return 1;
    if (n_steps <= 0) DM_FAIL(e, "dm_f32_ddim_run: n_steps %d", n_steps);
    if (!x_dev || !t_host || !coef_host || !slot_dev) DM_FAIL(e, "dm_f32_ddim_run: bad argument");
    if (save_row_host && !traj_dev) DM_FAIL(e, "dm_f32_ddim_run: save rows without a trajectory buffer");
    if (!e->finalized) DM_FAIL(e, "fp32 net not finalized");
    if (e->n_prompts <= 0) DM_FAIL(e, "dm_f32_set_prompts must be called first");
    if (B <= 0 || h < 1 || w < 1) DM_FAIL(e, "dm_f32_ddim_run: bad batch / latent size");
    if (B > chunk32(h, w)) DM_FAIL(e, "dm_f32_ddim_run: batch %d over the %d samples of one run at %d x %d", B, chunk32(h, w), h, w);
    for (int i = 0; i < n_steps; ++i) if (t_host[i] < 0 || t_host[i] > 999) DM_FAIL(e, "dm_f32_ddim_run: timestep %lld out of range", (long long)t_host[i]);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t per = (size_t)4 * h * w, n = (size_t)B * per;
    const size_t off_t = (n * sizeof(float) + 255) & ~(size_t)255, off_c = off_t + (((size_t)n_steps * B * sizeof(int64_t) + 255) & ~(size_t)255);
    DM_TRY(loop_reserve32(e, s, off_c + (size_t)n_steps * 4 * sizeof(float)));
    float* eps = (float*)e->loop_buf;
    int64_t* t_dev = (int64_t*)(e->loop_buf + off_t);
    float* coef = (float*)(e->loop_buf + off_c);
    DM_TRY(loop_tables32(e, s, t_host, coef_host, n_steps, B, t_dev, coef));
    Args32 A{(const float*)x_dev, t_dev, slot_dev, B, h, w, -1, eps, nullptr, nullptr, 1};
    DM_TRY(run32(e, A, s, false));
    for (int i = 0; i < n_steps; ++i) {
        A.t = t_dev + (size_t)i * B;
        DM_TRY(run32(e, A, s));                       // its arena: a map lookup, the dry run and the allocation happened before the loop
        DM_HIP(e, launch_ddim_step((const float*)x_dev, eps, nullptr, 0.f, coef + 4 * i, (long long)n, (float*)x_dev, s));
        if (save_row_host && save_row_host[i] >= 0)
            DM_HIP(e, hipMemcpyAsync((float*)traj_dev + (size_t)save_row_host[i] * n, x_dev, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

/* Plug-and-Play sampling (pnp.py:538-577) for B targets of one source: per step the batch [source_i, x (uncond slots), x (cond slots)], the
 * injected forward, classifier-free guidance and DDIMScheduler.step.  The reference repeats the source B times; its rows are identical. */
int dm_f32_pnp_run(dm_f32_net* e, void* x_dev, const void* src_dev, const int64_t* t_host, const float* coef_host, const uint8_t* conv_on_host,
                   const uint8_t* attn_on_host, int conv_mask, int attn_mask, const int32_t* slot_dev, int B, int h, int w, int n_steps,
                   float guidance_scale, void* stream) {
    if (!e) return 1;
    if (n_steps <= 0) DM_FAIL(e, "dm_f32_pnp_run: n_steps %d", n_steps);
    if (!x_dev || !src_dev || !t_host || !coef_host || !conv_on_host || !attn_on_host || !slot_dev) DM_FAIL(e, "dm_f32_pnp_run: bad argument");
    if (conv_mask < 0 || attn_mask < 0 || conv_mask >= (1 << 14) || attn_mask >= (1 << 13)) DM_FAIL(e, "dm_f32_pnp_run: bad layer mask");
    if (!e->finalized) DM_FAIL(e, "fp32 net not finalized");
    if (e->n_prompts <= 0) DM_FAIL(e, "dm_f32_set_prompts must be called first");
    if (B <= 0 || h < 1 || w < 1) DM_FAIL(e, "dm_f32_pnp_run: bad batch / latent size");
    const int N = 1 + 2 * B;
    if (N > chunk32(h, w))
        DM_FAIL(e, "dm_f32_pnp_run: 1 + 2 * %d samples over the %d of one run at %d x %d: the source must share a run with its targets", B, chunk32(h, w), h, w);
    for (int i = 0; i < n_steps; ++i) if (t_host[i] < 0 || t_host[i] > 999) DM_FAIL(e, "dm_f32_pnp_run: timestep %lld out of range", (long long)t_host[i]);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t per = (size_t)4 * h * w, nb = (size_t)B * per;
    const size_t in_bytes = ((size_t)N * per * sizeof(float) + 255) & ~(size_t)255;
    const size_t off_t = 2 * in_bytes, off_c = off_t + (((size_t)n_steps * N * sizeof(int64_t) + 255) & ~(size_t)255);
    DM_TRY(loop_reserve32(e, s, off_c + (size_t)n_steps * 4 * sizeof(float)));
    float* in = (float*)e->loop_buf;
    float* eps = (float*)(e->loop_buf + in_bytes);
    int64_t* t_dev = (int64_t*)(e->loop_buf + off_t);
    float* coef = (float*)(e->loop_buf + off_c);
    DM_TRY(loop_tables32(e, s, t_host, coef_host, n_steps, N, t_dev, coef));
    Args32 A{in, t_dev, slot_dev, N, h, w, -1, eps, nullptr, nullptr, 1};
    for (int pass = 0; pass < 2; ++pass) {            // both arena sizes (with and without the feature injection) before the loop
        A.conv_mask = pass ? (unsigned)conv_mask : 0;
        DM_TRY(run32(e, A, s, false));
    }
    for (int i = 0; i < n_steps; ++i) {
        DM_HIP(e, hipMemcpyAsync(in, (const float*)src_dev + (size_t)i * per, per * sizeof(float), hipMemcpyDeviceToDevice, s));
        DM_HIP(e, hipMemcpyAsync(in + per, x_dev, nb * sizeof(float), hipMemcpyDeviceToDevice, s));
        DM_HIP(e, hipMemcpyAsync(in + per + nb, x_dev, nb * sizeof(float), hipMemcpyDeviceToDevice, s));
        A.t = t_dev + (size_t)i * N;
        A.conv_mask = conv_on_host[i] ? (unsigned)conv_mask : 0;
        A.attn_mask = attn_on_host[i] ? (unsigned)attn_mask : 0;
        DM_TRY(run32(e, A, s));
        DM_HIP(e, launch_ddim_step((const float*)x_dev, eps + per, eps + per + nb, guidance_scale, coef + 4 * i, (long long)nb, (float*)x_dev, s));
    }
    return 0;
}

}  // extern "C"
