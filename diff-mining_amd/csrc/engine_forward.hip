// engine_forward.hip — the fp16 engine's schedules: the op vocabulary (`Fwd`: arena tensors in, launches out) and the four
// networks written in it (U-Net, VAE encoder, VAE decoder, CLIP text tower), issued as hand-written gfx950 kernels on one HIP stream.
//
// Replaces, for diff-mining's hot path:  scheduler.add_noise + unet(...) + mse_loss at
// diffmining/typicality/compute.py:99-101 and MyUNet2DConditionModel.forward at dift.py:24-169.
// The block order below restates diffusers-0.24 `UNet2DConditionModel` for the public SDv1.5
// config; it is checked against the CPU oracle in tests/.
#include "engine_impl.h"

#include <cmath>

using namespace dm;
using namespace dm::eng;
using namespace sd15;

namespace dm { thread_local LaunchTimer* g_launch_timer = nullptr; }

namespace {

// ------------------------------------------------------------------------------------------------
// forward helpers
// ------------------------------------------------------------------------------------------------
struct Fwd {
    dm_engine* e;
    hipStream_t s;
    bool dry;
    float res_eps = GN_EPS;   // GroupNorm eps of the ResNet blocks (U-Net 1e-5, VAE 1e-6)
    struct SkipStat { size_t off = (size_t)-1; const double* p = nullptr; int N = 0, C = 0, HW = 0; };
    std::vector<SkipStat> skip_stats;      // by Tensor::sid
    void free_skip_stat(int sid) {
        if (sid >= 0 && sid < (int)skip_stats.size() && skip_stats[sid].off != (size_t)-1) { e->arena.release(skip_stats[sid].off); skip_stats[sid] = SkipStat(); }
    }

    int alloc(Tensor* t, int N, int H, int W, int C) {
        t->N = N; t->H = H; t->W = W; t->C = C;
        const size_t bytes = (size_t)N * H * W * C * sizeof(f16);
        t->off = e->arena.alloc(bytes);
        if (t->off == (size_t)-1) DM_FAIL(e, "workspace arena exhausted (%zu bytes requested)", bytes);
        t->p = reinterpret_cast<f16*>(e->arena_base + t->off);
        return 0;
    }
    int alloc_raw(size_t bytes, size_t* off, void** p) {
        *off = e->arena.alloc(bytes);
        if (*off == (size_t)-1) DM_FAIL(e, "workspace arena exhausted (%zu bytes requested)", bytes);
        *p = e->arena_base + *off;
        return 0;
    }
    void free(Tensor& t) { if (!t.view && t.off != (size_t)-1) { e->arena.release(t.off); t.off = (size_t)-1; t.p = nullptr; } }
    void free_raw(size_t off) { e->arena.release(off); }

    // live roofline events (dm_prof_enable): the launchers' dispatches between prof_begin and prof_end carry their own (start, stop)
    // event pairs (dm::launch_timed) — no hipEventRecord barrier packets between the kernels
    LaunchTimer timer;
    ~Fwd() { if (g_launch_timer == &timer) g_launch_timer = nullptr; }       // an error return between begin and end must not leave it installed
    int prof_begin(int kind, double flops, int M = 0, int N = 0, int K = 0, int mode = 0) {
        if (!e->prof || dry) return 0;
        ProfEv ev; ev.flops = flops; ev.kind = kind; ev.M = M; ev.N = N; ev.K = K; ev.mode = mode;
        e->prof_ev.push_back(std::move(ev));
        timer.pool = &e->ev_pool; timer.pairs.clear(); timer.err = hipSuccess;
        g_launch_timer = &timer;
        return 0;
    }
    int prof_end() {
        if (!e->prof || dry) return 0;
        g_launch_timer = nullptr;
        e->prof_ev.back().pairs.swap(timer.pairs);
        DM_HIP(e, timer.err);
        return 0;
    }

    // Y = igemm(X [, X2]) with fused epilogue.  Output spatial dims given by (OH, OW).
    int igemm(const ConvW& cv, int mode, const Tensor& x, const Tensor* x2, int OH, int OW,
              const f16* temb, int temb_ld, const Tensor* res, int epi, Tensor* y, const LnFold* ln = nullptr,
              const float* ln_stats = nullptr, const Tensor* x3 = nullptr, const Tensor* x4 = nullptr, float* gn_blocks = nullptr,
              int* gn_rows = nullptr, bool has_temb = false) {
        const int cin = x.C + (x2 ? x2->C : 0);
        if (cin != cv.cin) DM_FAIL(e, "igemm: channel mismatch %d vs %d", cin, cv.cin);
        const int cout_y = (epi == EPI_GEGLU) ? cv.cout / 2 : cv.cout;
        if (y->view) {                                 // pre-placed output (first_slot() of a stacked tensor): write in place
            if (y->N != x.N || y->H != OH || y->W != OW || y->C != cout_y) DM_FAIL(e, "igemm: pre-placed output has the wrong shape");
        } else DM_TRY(alloc(y, x.N, OH, OW, cout_y));
        IGemmParams p;
        p.X = x.p; p.X2 = x2 ? x2->p : nullptr; p.Wp = cv.w; p.bias = cv.b; p.temb = temb;
        p.res = res ? res->p : nullptr; p.Y = y->p;
        p.Cout = cv.cout; p.Cin = cin; p.C1 = x.C;
        p.mode = mode; p.epi = epi; p.ldy = cout_y; p.ldres = res ? res->C : 0; p.temb_ld = temb_ld;
        p.has_temb = has_temb || temb != nullptr;
        if (mode == IG_DENSE) { p.M = (int)x.rows(); p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; }
        else { p.M = x.N * OH * OW; p.H = x.H; p.W = x.W; p.OH = OH; p.OW = OW; }
        if (ln) { p.ln_stats = ln_stats; p.ln_s = ln->s; p.ln_t = ln->t; p.ln_eps = LN_EPS; }
        if (x3) {             // a ResNet block's conv_shortcut folded into this conv2: extra k steps on cat([x3, x4])
            if (cv.csc != x3->C + (x4 ? x4->C : 0) || (mode != IG_CONV3 && mode != IG_DENSE) || temb) DM_FAIL(e, "igemm: bad folded second GEMM");
            p.X3 = x3->p; p.X4 = x4 ? x4->p : nullptr; p.C3 = x3->C; p.Csc = cv.csc;
        }
        p.tile_ctr = e->tile_ctr;
        // small-M layers: split-K through an fp32 workspace (also accounted for in the dry run)
        const int parts = (ln || x3) ? 1 : igemm_splitk_parts(p, OH * OW);
        size_t poff = (size_t)-1;
        if (parts > 1) {
            void* pp;
            DM_TRY(alloc_raw((size_t)parts * p.M * cv.cout * sizeof(float), &poff, &pp));
            p.ksplit = parts; p.partial = (float*)pp;
        }
        // GroupNorm block sums of the output from the epilogue: *gn_rows = the leading rows that get them (the rest is the caller's)
        p.gn_blocks = gn_blocks;
        if (gn_rows) *gn_rows = igemm_gn_layer(p) ? igemm_gn_rows(p) : -1;      // -1: a layer that never gets them (the caller's r04 pass)
        if (!dry) {
            const double flops = 2.0 * (double)p.M * cv.cout * (double)((mode == IG_DENSE ? 1 : 9) * cin + p.Csc);
            DM_TRY(prof_begin(0, flops, p.M, cv.cout, (mode == IG_DENSE ? 1 : 9) * cin + p.Csc, mode + 10 * epi));
            DM_HIP(e, launch_igemm(p, s));
            DM_TRY(prof_end());
        }
        if (parts > 1) free_raw(poff);
        return 0;
    }
    // Upsample2D (nearest 2x) + conv3x3 as four 2x2 convolutions on x's own grid (igemm_pers_up.hip): y [N][2H][2W][cout].
    // The FLOPs booked are the EXECUTED ones (4 taps): 4/9 of the layer's nominal count.
    int upconv4(const ConvW& cv, const Tensor& x, Tensor* y) {
        if (x.C != cv.cin) DM_FAIL(e, "upconv4: channel mismatch %d vs %d", x.C, cv.cin);
        DM_TRY(alloc(y, x.N, 2 * x.H, 2 * x.W, cv.cout));
        IGemmParams p;
        p.X = x.p; p.X2 = nullptr; p.Wp = cv.w; p.bias = cv.b; p.temb = nullptr; p.res = nullptr; p.Y = y->p;
        p.Cout = cv.cout; p.Cin = x.C; p.C1 = x.C; p.mode = IG_CONV2_UP4; p.epi = EPI_PLAIN; p.ldy = cv.cout; p.ldres = 0; p.temb_ld = 0;
        p.M = x.N * x.H * x.W; p.H = x.H; p.W = x.W; p.OH = x.H; p.OW = x.W;
        p.tile_ctr = e->tile_ctr;
        if (!dry) {
            DM_TRY(prof_begin(0, 2.0 * 4.0 * (double)p.M * cv.cout * 4.0 * (double)x.C, 4 * p.M, cv.cout, 4 * x.C, IG_CONV2_UP4));
            if (e->prof) e->prof_ev.back().folded = 2.0 * 4.0 * (double)p.M * cv.cout * 5.0 * (double)x.C;     // 9 - 4 taps
            DM_HIP(e, launch_igemm_pers_up4(p, s));
            DM_TRY(prof_end());
        }
        return 0;
    }
    int dense(const ConvW& cv, const Tensor& x, const Tensor* x2, const Tensor* res, int epi, Tensor* y) {
        return igemm(cv, IG_DENSE, x, x2, x.H, x.W, nullptr, 0, res, epi, y);
    }

    int groupnorm(const NormW& nw, const Tensor& x, const Tensor* x2, float eps, bool silu, Tensor* y) {
        const int C = x.C + (x2 ? x2->C : 0);
        if (C != nw.c) DM_FAIL(e, "groupnorm: channel mismatch %d vs %d", C, nw.c);
        const int HW = x.H * x.W;
        const int chunks = gn_stats_chunks(HW);
        // the skip half of a concatenated input was summed once already, for the GroupNorm that read the skip alone in the down path: sum x
        // only (in the concatenation's group width) and merge — one read of the skip tensor less.  Which layers do this is a property of the
        // network (channel counts, which skips a down-path norm1 reads), never of the batch.
        if (x2 && x2->sid >= 0 && x2->sid < (int)skip_stats.size() && skip_stats[x2->sid].off != (size_t)-1) {
            const SkipStat& st = skip_stats[x2->sid];
            const int cpg = C / GROUPS, cpg2 = x2->C / GROUPS;
            if (st.C == x2->C && st.HW == HW && C % GROUPS == 0 && x2->C % GROUPS == 0 && x.C % cpg == 0 && cpg % cpg2 == 0 && x.N % st.N == 0 && x.C % 8 == 0) {
                const int G1 = x.C / cpg, m = cpg / cpg2;
                size_t poff, moff; void *pp, *mp;
                DM_TRY(alloc_raw((size_t)x.N * chunks * G1 * 2 * sizeof(double), &poff, &pp));
                DM_TRY(alloc_raw((size_t)x.N * GROUPS * 2 * sizeof(double), &moff, &mp));
                DM_TRY(alloc(y, x.N, x.H, x.W, C));
                if (!dry) {
                    DM_HIP(e, launch_gn_stats(x.p, nullptr, x.N, HW, x.C, x.C, G1, (double*)pp, s));
                    DM_HIP(e, launch_gn_merge_skip((const double*)pp, st.p, x.N, st.N, chunks, GROUPS, G1, m, (double*)mp, s));
                    DM_HIP(e, launch_gn_apply(x.p, x2->p, x.N, HW, C, x.C, GROUPS, eps, nw.g, nw.b, (const double*)mp, silu ? 1 : 0, y->p, s, 1));
                }
                free_raw(poff); free_raw(moff);
                return 0;
            }
        }
        size_t poff; void* pp;
        DM_TRY(alloc_raw((size_t)x.N * chunks * GROUPS * 2 * sizeof(double), &poff, &pp));
        DM_TRY(alloc(y, x.N, x.H, x.W, C));
        if (!dry) {
            DM_HIP(e, launch_gn_stats(x.p, x2 ? x2->p : nullptr, x.N, HW, C, x.C, GROUPS, (double*)pp, s));
            DM_HIP(e, launch_gn_apply(x.p, x2 ? x2->p : nullptr, x.N, HW, C, x.C, GROUPS, eps, nw.g, nw.b, (const double*)pp,
                                      silu ? 1 : 0, y->p, s));
        }
        // a skip tensor read alone: keep its partial sums for the up path (released with the skip)
        if (!x2 && x.sid >= 0 && x.sid < (int)skip_stats.size() && skip_stats[x.sid].off == (size_t)-1 && option(OPT_GN_SKIP) != 0) {
            SkipStat& st = skip_stats[x.sid];
            st.off = poff; st.p = (const double*)pp; st.N = x.N; st.C = C; st.HW = HW;
            return 0;
        }
        free_raw(poff);
        return 0;
    }
    // GroupNorm whose statistics arrive as per-(64-row block, channel pair) sums (r05): the producing GEMM's epilogue wrote the
    // blocks of the first `rows_done` rows; the rest comes from the tensor (same arithmetic, same bits), then the fixed-order fp64 combine.
    static bool gn_blocks_ok(int HW, int C) { return option(OPT_GN_EPI) != 0 && HW % 64 == 0 && C % 16 == 0 && (C / GROUPS) % 2 == 0 && 256 % GROUPS == 0; }
    int groupnorm_blocks(const NormW& nw, const Tensor& x, float* blocks, int rows_done, float eps, bool silu, Tensor* y) {
        const int C = x.C, HW = x.H * x.W;
        if (C != nw.c) DM_FAIL(e, "groupnorm: channel mismatch %d vs %d", C, nw.c);
        size_t poff; void* pp;
        DM_TRY(alloc_raw((size_t)x.N * GROUPS * 2 * sizeof(double), &poff, &pp));
        DM_TRY(alloc(y, x.N, x.H, x.W, C));
        if (!dry) {
            DM_HIP(e, launch_gn_blocks(x.p, (int)x.rows(), C, rows_done, blocks, s));
            DM_HIP(e, launch_gn_blocks_final(blocks, x.N, HW, C, GROUPS, (double*)pp, s));
            DM_HIP(e, launch_gn_apply(x.p, nullptr, x.N, HW, C, C, GROUPS, eps, nw.g, nw.b, (const double*)pp, silu ? 1 : 0, y->p, s, 1));
        }
        free_raw(poff);
        return 0;
    }
    // GroupNorm (no activation) folded into the following 1x1 convolution (Transformer2D.norm -> proj_in): statistics as in
    // groupnorm(), then per-sample weights W diag(a_n) and bias rows W b_n + bias, then the GEMM on the RAW x — the normalised
    // tensor (one write + one read of the residual stream) never exists.  Pays while the per-sample weights (N x C x C) are
    // small next to the tensor (the rule below: Cout * 8 <= H * W): at a 64x64 latent that is the 320-channel level only — the
    // 640-channel level (32x32 positions) would spend 62 % of what it saves on the weights, C = 1280 five times as much.
    bool gn_fold_ok(const Tensor& x, const ConvW& cv) const {
        const int HW = x.H * x.W;
        return option(OPT_GN_FOLD) != 0 && cv.k == 1 && cv.cin == x.C && x.C <= 640 && cv.cout % 160 == 0 && HW % 128 == 0 &&
               (long long)x.C * cv.cout * 8 <= (long long)HW * x.C;      // weights per sample <= 1/8 of the sample's activations
    }
    int gn_dense(const NormW& nw, const ConvW& cv, const Tensor& x, float eps, Tensor* y) {
        const int C = x.C, HW = x.H * x.W;
        const int chunks = gn_stats_chunks(HW);
        size_t poff, woff, toff; void *pp, *wp, *tp;
        DM_TRY(alloc_raw((size_t)x.N * chunks * GROUPS * 2 * sizeof(double), &poff, &pp));
        DM_TRY(alloc_raw((size_t)x.N * cv.cout * C * sizeof(f16), &woff, &wp));
        DM_TRY(alloc_raw((size_t)x.N * cv.cout * sizeof(float), &toff, &tp));
        DM_TRY(alloc(y, x.N, x.H, x.W, cv.cout));
        if (!dry) {
            DM_HIP(e, launch_gn_stats(x.p, nullptr, x.N, HW, C, C, GROUPS, (double*)pp, s));
            DM_HIP(e, launch_gn_fold((const double*)pp, x.N, HW, C, GROUPS, eps, nw.g, nw.b, cv.w, cv.b, cv.cout, (f16*)wp, (float*)tp, s));
            IGemmParams p;
            p.X = x.p; p.X2 = nullptr; p.Wp = (const f16*)wp; p.bias = nullptr; p.temb = nullptr; p.res = nullptr; p.Y = y->p;
            p.M = (int)x.rows(); p.Cout = cv.cout; p.Cin = C; p.C1 = C; p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M;
            p.mode = IG_DENSE; p.epi = EPI_PLAIN; p.ldy = cv.cout; p.ldres = 0; p.temb_ld = 0;
            p.ln_s = (const float*)tp; p.ln_t = (const float*)tp; p.w_sample_stride = (long long)cv.cout * C; p.rows_per_sample = HW;
            p.tile_ctr = e->tile_ctr;
            DM_TRY(prof_begin(0, 2.0 * (double)p.M * cv.cout * C, p.M, cv.cout, C, 0));
            DM_HIP(e, launch_igemm(p, s));
            DM_TRY(prof_end());
        }
        free_raw(poff); free_raw(woff); free_raw(toff);
        return 0;
    }
    // LayerNorm folded into the following Linear: per-row (mean, rstd), then the GEMM on the raw tokens with
    // the correction in its epilogue (saves writing and re-reading the normalised token matrix)
    int ln_dense(const LnFold& f, const Tensor& x, int epi, Tensor* y) {
        // ln_inkernel: 0 = statistics kernel + GEMM; 2 = the GEMM takes the row statistics itself everywhere; 1 = where that is
        // cheaper: every channel tile of a row re-derives the statistics (N / 320 tiles x C / 64 k steps of extra LDS reads
        // and dot2s against one C-wide read by the statistics kernel), measured per shape at the bench batch (tools/ab_igemm.py
        // ln_inkernel 0 1): to_q 0.96, to_q/k/v 0.93 / 0.99 / 1.04 (C = 320 / 640 / 1280), GEGLU projection 0.98 / 1.04 / 1.08
        // => in the GEMM up to N = 2560
        const int ink = option(OPT_LN_INKERNEL);
        if (ink == 2 || (ink == 1 && f.w.cout <= 2560)) {
            return igemm(f.w, IG_DENSE, x, nullptr, x.H, x.W, nullptr, 0, nullptr, epi, y, &f, nullptr);
        }
        size_t soff; void* sp;
        DM_TRY(alloc_raw((size_t)x.rows() * 2 * sizeof(float), &soff, &sp));
        if (!dry) DM_HIP(e, launch_ln_stats(x.p, (int)x.rows(), x.C, LN_EPS, (float*)sp, s));
        const int rc = igemm(f.w, IG_DENSE, x, nullptr, x.H, x.W, nullptr, 0, nullptr, epi, y, &f, (const float*)sp);
        free_raw(soff);
        return rc;
    }
    static bool ln_fold_enabled() {
        return option(OPT_LN_FOLD) != 0;
    }
    int layernorm(const NormW& nw, const Tensor& x, Tensor* y) {
        DM_TRY(alloc(y, x.N, x.H, x.W, x.C));
        if (!dry) DM_HIP(e, launch_layernorm(x.p, (int)x.rows(), x.C, nw.g, nw.b, LN_EPS, y->p, s));
        return 0;
    }

    // `tproj`: the stacked time-embedding projections (the U-Net's ResNets) or nullptr (the VAE's).  A Tensor*, not its data pointer:
    // in the dry run every data pointer is arena offset + 0, so "is there a time embedding" must not be read off a pointer
    int resnet(const ResW& r, const Tensor& x, const Tensor* x2, const Tensor* tproj, Tensor* out) {
        Tensor n1, h1, n2, sc;
        const bool has_temb = tproj != nullptr;
        const f16* temb = has_temb ? tproj->p + r.temb_off : nullptr;
        DM_TRY(groupnorm(r.n1, x, x2, res_eps, true, &n1));
        // norm2's statistics: block sums out of conv1's epilogue where the persistent kernels run it, from h1 where they do not
        if (has_temb && gn_blocks_ok(x.H * x.W, r.c1.cout)) {       // (only time-embedding layers ever emit block sums: igemm_gn_layer)
            size_t boff; void* bp; int rows_done = 0;
            DM_TRY(alloc_raw((size_t)x.N * (x.H * x.W / 64) * r.c1.cout * sizeof(float), &boff, &bp));
            DM_TRY(igemm(r.c1, IG_CONV3, n1, nullptr, x.H, x.W, temb, e->tproj_total, nullptr, EPI_PLAIN, &h1,
                         nullptr, nullptr, nullptr, nullptr, (float*)bp, &rows_done, has_temb));
            free(n1);
            if (rows_done < 0) { free_raw(boff); DM_TRY(groupnorm(r.n2, h1, nullptr, res_eps, true, &n2)); }
            else { DM_TRY(groupnorm_blocks(r.n2, h1, (float*)bp, rows_done, res_eps, true, &n2)); free_raw(boff); }
        } else {
            DM_TRY(igemm(r.c1, IG_CONV3, n1, nullptr, x.H, x.W, temb, e->tproj_total, nullptr, EPI_PLAIN, &h1,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, has_temb));
            free(n1);
            DM_TRY(groupnorm(r.n2, h1, nullptr, res_eps, true, &n2));
        }
        free(h1);
        // conv_shortcut folded into conv2 (extra k steps on the block's input instead of a GEMM whose output conv2 reads back as its
        // residual) wherever conv2 runs unsplit (more than 64 positions per sample: the split-K layers keep the pair)
        if (r.has_sc && r.c2sc.w && option(OPT_SC_FOLD) && x.H * x.W > 64) {
            DM_TRY(igemm(r.c2sc, IG_CONV3, n2, nullptr, x.H, x.W, nullptr, 0, nullptr, EPI_PLAIN, out, nullptr, nullptr, &x, x2));
            free(n2);
            return 0;
        }
        const Tensor* resid = &x;
        if (r.has_sc) { DM_TRY(dense(r.sc, x, x2, nullptr, EPI_PLAIN, &sc)); resid = &sc; }
        else if (x2) DM_FAIL(e, "resnet: concat input without shortcut conv");
        DM_TRY(igemm(r.c2, IG_CONV3, n2, nullptr, x.H, x.W, nullptr, 0, resid, EPI_PLAIN, out));
        free(n2);
        if (r.has_sc) free(sc);
        return 0;
    }

    int slot_div = 0;       // shared-draw mode: prompt slot of sample b is b / slot_div (no slot array)

    int attention(const f16* Q, int ldq, long long bsq, const f16* K, const f16* V, int ldkv, long long bskv,
                  const int32_t* slots, int B, int Tq, int Tk, int C, f16* O) {
        AttnParams a;
        a.Q = Q; a.K = K; a.V = V; a.O = O;
        a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = C;
        a.bsq = bsq; a.bsk = bskv; a.bsv = bskv; a.bso = (long long)Tq * C;
        a.kv_slot = slots; a.slot_div = 0; a.B = B; a.heads = HEADS; a.Tq = Tq; a.Tk = Tk; a.D = C / HEADS;
        a.scale = 1.0f / sqrtf((float)a.D);
        DM_TRY(prof_begin(1, 4.0 * B * HEADS * (double)Tq * Tk * a.D, B * Tq, Tk, a.D, 100));
        DM_HIP(e, launch_attention(a, s));
        DM_TRY(prof_end());
        return 0;
    }

    // Transformer2D, first half: GroupNorm, proj_in, LayerNorm, self-attention, to_out + residual.
    // Nothing here depends on the prompt.
    int transformer_pre(const TfmW& t, const Tensor& x, Tensor* t1) {
        const int C = t.c, T = x.H * x.W, B = x.N;
        Tensor n, t0, ln, qkv, a;
        if (gn_fold_ok(x, t.proj_in)) DM_TRY(gn_dense(t.gn, t.proj_in, x, ATTN_GN_EPS, &t0));
        else {
            DM_TRY(groupnorm(t.gn, x, nullptr, ATTN_GN_EPS, false, &n));
            DM_TRY(dense(t.proj_in, n, nullptr, nullptr, EPI_PLAIN, &t0));
            free(n);
        }
        if (ln_fold_enabled()) DM_TRY(ln_dense(t.qkv_ln, t0, EPI_PLAIN, &qkv));
        else {
            DM_TRY(layernorm(t.ln1, t0, &ln));
            DM_TRY(dense(t.qkv, ln, nullptr, nullptr, EPI_PLAIN, &qkv));
            free(ln);
        }
        DM_TRY(alloc(&a, B, x.H, x.W, C));
        if (!dry) DM_TRY(attention(qkv.p, 3 * C, (long long)T * 3 * C, qkv.p + C, qkv.p + 2 * C, 3 * C, (long long)T * 3 * C,
                                   nullptr, B, T, T, C, a.p));
        free(qkv);
        DM_TRY(dense(t.o1, a, nullptr, &t0, EPI_PLAIN, t1));
        free(a); free(t0);
        return 0;
    }
    // second half: cross-attention against the per-prompt K/V cache, GEGLU feed-forward, proj_out + x.
    // Consumes (frees) t1.
    // LN2 -> attn2.to_q
    int cross_q(const TfmW& t, const Tensor& t1, Tensor* q) {
        Tensor ln;
        if (ln_fold_enabled()) return ln_dense(t.q2_ln, t1, EPI_PLAIN, q);
        DM_TRY(layernorm(t.ln2, t1, &ln));
        DM_TRY(dense(t.q2, ln, nullptr, nullptr, EPI_PLAIN, q));
        free(ln);
        return 0;
    }
    // `qU` (optional, consumed): the queries of the first q_mod samples, shared by every block of q_mod samples (shared-draw prefix).
    // `rep` > 1 (shared-draw prefix, with qU): x and t1 hold ONE block of x.N samples that every one of the `rep` prompt blocks shares —
    // the batch is rep * x.N samples, and the two GEMMs that read x / t1 as their residual run once per prompt block against the
    // shared rows instead of reading stacked copies (r05: the copies were 3 x 210 MB per step; bit-identical: a sample's bits do not
    // depend on its position in a launch)
    int transformer_post(const TfmW& t, const Tensor& x, Tensor& t1, const int32_t* slots, Tensor* out, Tensor* qU = nullptr, int q_mod = 0,
                         int rep = 1) {
        const int C = t.c, T = x.H * x.W, B = x.N * rep;
        if (rep > 1 && !qU) DM_FAIL(e, "transformer_post: shared residual rows need the shared queries");
        Tensor ln, a, q, t2, ff, t3;
        if (qU) q = *qU;
        else DM_TRY(cross_q(t, t1, &q));
        DM_TRY(alloc(&a, B, x.H, x.W, C));
        if (!dry) {
            const f16* kv = e->kv_cache[t.layer];
            AttnParams ap;
            ap.Q = q.p; ap.K = kv; ap.V = kv + C; ap.O = a.p;
            ap.ldq = C; ap.ldk = 2 * C; ap.ldv = 2 * C; ap.ldo = C;
            ap.bsq = (long long)T * C; ap.bsk = (long long)CTX_LEN * 2 * C; ap.bsv = ap.bsk; ap.bso = (long long)T * C;
            ap.kv_slot = slot_div > 0 ? nullptr : slots; ap.slot_div = slot_div; ap.n_slots = e->n_prompts;
            ap.q_mod = qU ? q_mod : 0;
            ap.B = B; ap.heads = HEADS; ap.Tq = T; ap.Tk = CTX_LEN; ap.D = C / HEADS;
            ap.scale = 1.0f / sqrtf((float)ap.D);
            DM_TRY(prof_begin(1, 4.0 * B * HEADS * (double)T * CTX_LEN * ap.D, B * T, CTX_LEN, ap.D, 101));
            DM_HIP(e, launch_attention(ap, s));
            DM_TRY(prof_end());
        }
        free(q);
        if (rep > 1) {
            DM_TRY(alloc(&t2, B, x.H, x.W, C));
            for (int k = 0; k < rep; ++k) {
                const Tensor ak = slot_view(a, k, rep);
                Tensor t2k = slot_view(t2, k, rep);
                DM_TRY(dense(t.o2, ak, nullptr, &t1, EPI_PLAIN, &t2k));
            }
        } else DM_TRY(dense(t.o2, a, nullptr, &t1, EPI_PLAIN, &t2));
        free(a); free(t1);
        if (ln_fold_enabled()) DM_TRY(ln_dense(t.ff1_ln, t2, EPI_GEGLU, &ff));
        else {
            DM_TRY(layernorm(t.ln3, t2, &ln));
            DM_TRY(dense(t.ff1, ln, nullptr, nullptr, EPI_GEGLU, &ff));
            free(ln);
        }
        if (option(OPT_FF_FOLD) && t.ffp.w) {
            // ff.net.2 + residual + proj_out as one GEMM over [ff | t2] (+ x): the [tokens x C] intermediate is never written or read
            if (rep > 1) {
                DM_TRY(alloc(out, B, x.H, x.W, t.ffp.cout));
                for (int k = 0; k < rep; ++k) {
                    const Tensor ffk = slot_view(ff, k, rep), t2k = slot_view(t2, k, rep);
                    Tensor ok = slot_view(*out, k, rep);
                    DM_TRY(igemm(t.ffp, IG_DENSE, ffk, nullptr, x.H, x.W, nullptr, 0, &x, EPI_PLAIN, &ok, nullptr, nullptr, &t2k, nullptr));
                }
            } else DM_TRY(igemm(t.ffp, IG_DENSE, ff, nullptr, x.H, x.W, nullptr, 0, &x, EPI_PLAIN, out, nullptr, nullptr, &t2, nullptr));
            free(ff); free(t2);
            return 0;
        }
        DM_TRY(dense(t.ff2, ff, nullptr, &t2, EPI_PLAIN, &t3));
        free(ff); free(t2);
        if (rep > 1) {
            DM_TRY(alloc(out, B, x.H, x.W, t.proj_out.cout));
            for (int k = 0; k < rep; ++k) {
                const Tensor t3k = slot_view(t3, k, rep);
                Tensor ok = slot_view(*out, k, rep);
                DM_TRY(dense(t.proj_out, t3k, nullptr, &x, EPI_PLAIN, &ok));
            }
        } else DM_TRY(dense(t.proj_out, t3, nullptr, &x, EPI_PLAIN, out));
        free(t3);
        return 0;
    }
    int transformer(const TfmW& t, const Tensor& x, const int32_t* slots, Tensor* out) {
        Tensor t1;
        DM_TRY(transformer_pre(t, x, &t1));
        return transformer_post(t, x, t1, slots, out);
    }
    // n_cond stacked copies of a [U, ...] tensor, out[k*U + i] = in[i], without copying slot 0: the producer writes the
    // first slot of the stacked tensor in place (first_slot() as its output), fill_slots() copies it to the others
    static Tensor first_slot(const Tensor& stacked, int n_cond) {
        Tensor v; v.p = stacked.p; v.off = (size_t)-1; v.view = true; v.N = stacked.N / n_cond; v.H = stacked.H; v.W = stacked.W; v.C = stacked.C;
        return v;
    }
    // block k of n_cond equal sample blocks of a stacked tensor, as a pre-placed window (null in the dry run, like every pointer there)
    static Tensor slot_view(const Tensor& stacked, int k, int n_cond) {
        Tensor v = first_slot(stacked, n_cond);
        if (stacked.p) v.p = stacked.p + (size_t)k * (size_t)(stacked.rows() / n_cond) * stacked.C;
        return v;
    }
    int fill_slots(const Tensor& stacked, int n_cond) {
        if (!dry) {
            const size_t bytes = (size_t)(stacked.rows() / n_cond) * stacked.C * sizeof(f16);
            for (int k = 1; k < n_cond; ++k)
                DM_HIP(e, hipMemcpyAsync((char*)stacked.p + (size_t)k * bytes, stacked.p, bytes, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    }
};

}  // namespace

int dm::eng::run_forward(dm_engine* e, const FwdArgs& A, hipStream_t s, bool dry) {
    Fwd F{e, s, dry};
    const int B = A.B;
    const int NC = A.n_cond > 1 ? A.n_cond : 1;
    const int U = B / NC;                 // distinct (x, t, eps) draws; every draw is scored under NC prompts
    F.slot_div = (NC > 1 && !A.slots) ? U : 0;       // shared-draw mode without a slot table: prompt k for every draw of block k
    // the persistent igemm kernel leaves its tile hand-out counters at zero — unless a launch faulted or was aborted; a run
    // starts from a known state either way (1 KB, stream-ordered)
    if (!dry && e->tile_ctr) DM_HIP(e, hipMemsetAsync(e->tile_ctr, 0, IGEMM_TILE_CTR_INTS * sizeof(int), s));
    // ---- time embedding: sinusoid row -> MLP -> SiLU -> all 22 time_emb_proj in one GEMM --------
    Tensor te0, e1, e1s, emb, embs, tprojU, tproj;
    DM_TRY(F.alloc(&te0, 1, 1, U, BOC[0]));
    if (!dry) DM_HIP(e, launch_time_gather(e->sin_table, A.t, U, BOC[0], te0.p, s));
    DM_TRY(F.dense(e->time1, te0, nullptr, nullptr, EPI_PLAIN, &e1));
    F.free(te0);
    DM_TRY(F.alloc(&e1s, 1, 1, U, TEMB));
    if (!dry) DM_HIP(e, launch_silu(e1.p, e1s.p, (long long)U * TEMB, s));
    F.free(e1);
    DM_TRY(F.dense(e->time2, e1s, nullptr, nullptr, EPI_PLAIN, &emb));
    F.free(e1s);
    DM_TRY(F.alloc(&embs, 1, 1, U, TEMB));
    if (!dry) DM_HIP(e, launch_silu(emb.p, embs.p, (long long)U * TEMB, s));
    F.free(emb);
    if (NC > 1) {
        DM_TRY(F.alloc(&tproj, NC, 1, U, e->tproj_total));
        tprojU = Fwd::first_slot(tproj, NC);
    }
    DM_TRY(F.dense(e->tproj_all, embs, nullptr, nullptr, EPI_PLAIN, &tprojU));
    F.free(embs);
    if (NC > 1) DM_TRY(F.fill_slots(tproj, NC)); else tproj = tprojU;

    // ---- conv_in (+ fused add_noise) ------------------------------------------------------------
    Tensor h, hB;
    if (NC > 1) {                  // the stacked skip tensor; conv_in writes its first slot
        DM_TRY(F.alloc(&hB, U * NC, A.H, A.W, BOC[0]));
        hB.sid = 0;                 // skip 0: its statistics are taken on the per-draw rows (the copies of a draw share them)
        h = Fwd::first_slot(hB, NC);
        h.sid = 0;
    } else h.sid = 0;
    F.skip_stats.assign(3 * NB + 4, Fwd::SkipStat());
    {
        Tensor col;
        DM_TRY(F.alloc(&col, U, A.H, A.W, 64));
        const void* sa = A.latent_f32 ? (const void*)e->sa32_tab : (const void*)e->sa_tab;
        const void* sb = A.latent_f32 ? (const void*)e->sb32_tab : (const void*)e->sb_tab;
        if (!dry) DM_HIP(e, launch_im2col_in(A.x, A.x_index, A.eps, A.t, A.add_noise ? sa : nullptr,
                                             A.add_noise ? sb : nullptr, A.latent_f32, U, A.H, A.W, col.p, s));
        DM_TRY(F.dense(e->conv_in, col, nullptr, nullptr, EPI_PLAIN, &h));
        F.free(col);
    }
    std::vector<Tensor> skips;
    Tensor cur;
    int j_start = 0;
    if (NC > 1) {
        // Shared prefix: conv_in, down_blocks[0].resnets[0] and the prompt-independent half of its
        // transformer (up to the self-attention residual) run ONCE per draw; their outputs are then
        // stacked NC times and the per-prompt half continues on the full batch.  Bit-identical to
        // running every (draw, prompt) pair separately (the kernels are batch-position invariant).
        const DownBlockW& d = e->down[0];
        Tensor rU, t1U, rB, t1B, a;
        // the cross-attention queries of the first transformer depend on the draw only: projected once per draw, read modulo U
        const bool q_once = option(OPT_Q_ONCE) != 0;
        // ... and with the queries shared, the only other readers of the stacked ResNet output and of t1 are two residual reads:
        // those GEMMs can run once per prompt block against the per-draw rows, and two stacking copies disappear (q_once = 2; measured +-0:
        // 139.00 vs 139.05 ms/step over three alternating pairs, profiles/r05_ab_q_once.txt — the copies cost what the extra launches do)
        const bool share = q_once && option(OPT_Q_ONCE) == 2;
        if (share) {
            DM_TRY(F.resnet(d.res[0], h, nullptr, &tprojU, &rU));
            DM_TRY(F.transformer_pre(d.tf[0], rU, &t1U));
            Tensor qU;
            DM_TRY(F.cross_q(d.tf[0], t1U, &qU));
            DM_TRY(F.fill_slots(hB, NC));
            DM_TRY(F.transformer_post(d.tf[0], rU, t1U, A.slots, &a, &qU, U, NC));
            F.free(rU);
        } else {
            DM_TRY(F.alloc(&rB, U * NC, A.H, A.W, d.res[0].cout));
            rU = Fwd::first_slot(rB, NC);
            DM_TRY(F.resnet(d.res[0], h, nullptr, &tprojU, &rU));
            DM_TRY(F.alloc(&t1B, U * NC, A.H, A.W, d.tf[0].c));
            t1U = Fwd::first_slot(t1B, NC);
            DM_TRY(F.transformer_pre(d.tf[0], rU, &t1U));
            Tensor qU;
            if (q_once) DM_TRY(F.cross_q(d.tf[0], t1U, &qU));
            DM_TRY(F.fill_slots(hB, NC));
            DM_TRY(F.fill_slots(rB, NC));
            DM_TRY(F.fill_slots(t1B, NC));
            DM_TRY(F.transformer_post(d.tf[0], rB, t1B, A.slots, &a, q_once ? &qU : nullptr, U));
            F.free(rB);
        }
        skips.push_back(hB);
        a.sid = (int)skips.size();
        skips.push_back(a);
        cur = a;
        j_start = 1;
    } else {
        skips.push_back(h);
        cur = h;                    // `cur` aliases the newest skip (never freed here)
    }
    // ---- down -----------------------------------------------------------------------------------
    for (int i = 0; i < NB; ++i) {
        const DownBlockW& d = e->down[i];
        for (int j = (i == 0 ? j_start : 0); j < LAYERS; ++j) {
            Tensor r;
            DM_TRY(F.resnet(d.res[j], cur, nullptr, &tproj, &r));
            if (d.attn) {
                Tensor a;
                DM_TRY(F.transformer(d.tf[j], r, A.slots, &a));
                F.free(r);
                r = a;
            }
            r.sid = (int)skips.size();
            skips.push_back(r);
            cur = r;
        }
        if (d.has_down) {
            Tensor dn;
            DM_TRY(F.igemm(d.down, IG_CONV3_S2, cur, nullptr, (cur.H + 1) / 2, (cur.W + 1) / 2, nullptr, 0, nullptr, EPI_PLAIN, &dn));
            dn.sid = (int)skips.size();
            skips.push_back(dn);
            cur = dn;
        }
    }
    // ---- mid ------------------------------------------------------------------------------------
    Tensor m0, m1, m2;
    DM_TRY(F.resnet(e->mid_res[0], cur, nullptr, &tproj, &m0));
    DM_TRY(F.transformer(e->mid_tf, m0, A.slots, &m1));
    F.free(m0);
    DM_TRY(F.resnet(e->mid_res[1], m1, nullptr, &tproj, &m2));
    F.free(m1);
    cur = m2;                       // owned from here on
    // ---- up -------------------------------------------------------------------------------------
    const bool fwd_up_size = (A.H % 8 != 0) || (A.W % 8 != 0);
    for (int i = 0; i < NB; ++i) {
        if (A.up_ft_index >= 0 && i > A.up_ft_index) break;
        const UpBlockW& u = e->up[i];
        for (int j = 0; j < LAYERS + 1; ++j) {
            Tensor skip = skips.back(); skips.pop_back();
            Tensor r;
            DM_TRY(F.resnet(u.res[j], cur, &skip, &tproj, &r));
            F.free(cur); F.free(skip); F.free_skip_stat(skip.sid);
            if (u.attn) {
                Tensor a;
                DM_TRY(F.transformer(u.tf[j], r, A.slots, &a));
                F.free(r);
                r = a;
            }
            cur = r;
        }
        if (u.has_up) {
            int OH = cur.H * 2, OW = cur.W * 2;
            if (fwd_up_size && !skips.empty()) { OH = skips.back().H; OW = skips.back().W; }
            Tensor upc;
            // exact 2x (every latent whose side is a multiple of 8): four 2x2 convolutions on the source grid, 4/9 of the MACs
            // (option up_fold; a property of the layer and the sample geometry, never of the batch)
            if (option(OPT_UP_FOLD) != 0 && u.up4.w && OH == 2 * cur.H && OW == 2 * cur.W && igemm_up4_ok(cur.N, cur.H, cur.W, cur.C, u.up4.cout))
                DM_TRY(F.upconv4(u.up4, cur, &upc));
            else
                DM_TRY(F.igemm(u.up, IG_CONV3_UP, cur, nullptr, OH, OW, nullptr, 0, nullptr, EPI_PLAIN, &upc));
            F.free(cur);
            cur = upc;
        }
        if (A.up_ft_index == i) {
            if (!dry) {
                if (A.feat) DM_HIP(e, launch_nhwc_to_nchw(cur.p, cur.N, cur.H * cur.W, cur.C, A.feat, s));
                if (A.feat_mean) DM_HIP(e, launch_ensemble_mean(cur.p, cur.N / A.ensemble, A.ensemble, cur.H * cur.W, cur.C, A.feat_mean, s));
            }
        }
    }
    if (A.up_ft_index < 0) {
        Tensor nrm;
        DM_TRY(F.groupnorm(e->norm_out, cur, nullptr, GN_EPS, true, &nrm));
        if (!dry) DM_HIP(e, launch_conv_out(nrm.p, e->conv_out.w, e->conv_out.b, A.loss ? A.eps : nullptr, A.latent_f32, B, A.H, A.W, BOC[0],
                                            A.loss, A.pred, U, (NC > 1) ? U : B, (NC > 1) ? A.out_stride : 0,
                                            (NC > 1) ? A.out_off : 0, s));
        F.free(nrm);
    }
    F.free(cur);
    for (auto& sk : skips) { F.free(sk); F.free_skip_stat(sk.sid); }
    F.free(tproj);
    return 0;
}

// ---- VAE encoder: image -> moments -> latent (compute.py:91-93) ---------------------------------
int dm::eng::run_vae(dm_engine* e, const VaeArgs& A, hipStream_t s, bool dry) {
    Fwd F{e, s, dry};
    F.res_eps = VAE_EPS;
    const VaeW& v = e->vae;
    Tensor cur;
    {
        Tensor col;
        DM_TRY(F.alloc(&col, A.B, A.H, A.W, 64));
        if (!dry) DM_HIP(e, launch_im2col_rgb(A.image, A.B, A.H, A.W, col.p, s));
        DM_TRY(F.dense(v.conv_in, col, nullptr, nullptr, EPI_PLAIN, &cur));
        F.free(col);
    }
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 2; ++j) {
            Tensor r;
            DM_TRY(F.resnet(v.down[i][j], cur, nullptr, nullptr, &r));
            F.free(cur);
            cur = r;
        }
        if (i != VNB - 1) {
            Tensor dn;      // Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + conv3x3 stride 2
            DM_TRY(F.igemm(v.ds[i], IG_CONV3_S2P0, cur, nullptr, cur.H / 2, cur.W / 2, nullptr, 0, nullptr, EPI_PLAIN, &dn));
            F.free(cur);
            cur = dn;
        }
    }
    {
        Tensor m0, n, qkv, a, m1, m2;
        DM_TRY(F.resnet(v.mid[0], cur, nullptr, nullptr, &m0));
        F.free(cur);
        const int C = VBOC[VNB - 1], T = m0.H * m0.W;
        DM_TRY(F.groupnorm(v.attn_gn, m0, nullptr, VAE_EPS, false, &n));
        DM_TRY(F.dense(v.qkv, n, nullptr, nullptr, EPI_PLAIN, &qkv));
        F.free(n);
        DM_TRY(F.alloc(&a, m0.N, m0.H, m0.W, C));
        if (!dry) {
            DM_TRY(F.prof_begin(1, 4.0 * m0.N * (double)T * T * C));
            DM_HIP(e, launch_attention512(qkv.p, qkv.p + C, qkv.p + 2 * C, a.p, m0.N, T, 3 * C, C, 1.0f / sqrtf((float)C), s));
            DM_TRY(F.prof_end());
        }
        F.free(qkv);
        DM_TRY(F.dense(v.o, a, nullptr, &m0, EPI_PLAIN, &m1));
        F.free(a); F.free(m0);
        DM_TRY(F.resnet(v.mid[1], m1, nullptr, nullptr, &m2));
        F.free(m1);
        cur = m2;
    }
    Tensor nrm, co;
    DM_TRY(F.groupnorm(v.norm_out, cur, nullptr, VAE_EPS, true, &nrm));
    F.free(cur);
    DM_TRY(F.igemm(v.conv_out, IG_CONV3, nrm, nullptr, nrm.H, nrm.W, nullptr, 0, nullptr, EPI_PLAIN, &co));
    F.free(nrm);
    if (!dry) DM_HIP(e, launch_posterior(co.p, co.C, v.qw, v.qb, A.noise, A.B, A.draws, co.H * co.W, A.scaling, A.latent16, A.latent32,
                                         A.moments, s));
    F.free(co);
    return 0;
}

// ---- VAE decoder: latent -> sample / image (`vae.decode(latents / scaling_factor)` + `VaeImageProcessor.postprocess` of the pipeline
//      `Trainer.sample` runs under autocast, finetuning/cars.py:235-255) --------------------------------------------------------------
int dm::eng::run_vae_dec(dm_engine* e, const VaeDecArgs& A, hipStream_t s, bool dry) {
    Fwd F{e, s, dry};
    F.res_eps = VAE_EPS;
    const VaeDecW& v = e->vaed;
    Tensor cur;
    {
        Tensor z;       // post_quant_conv's output at the head of 64-channel rows: conv_in is one 3x3 igemm with a single k step per tap
        DM_TRY(F.alloc(&z, A.B, A.h, A.w, 64));
        if (!dry) DM_HIP(e, launch_latent_prologue(A.latent, v.pqw, v.pqb, A.B, A.h * A.w, A.scaling, z.p, 64, s));
        DM_TRY(F.igemm(v.conv_in, IG_CONV3, z, nullptr, A.h, A.w, nullptr, 0, nullptr, EPI_PLAIN, &cur));
        F.free(z);
    }
    {
        Tensor m0, n, qkv, a, m1, m2;
        DM_TRY(F.resnet(v.mid[0], cur, nullptr, nullptr, &m0));
        F.free(cur);
        const int C = VBOC[VNB - 1], T = m0.H * m0.W;
        DM_TRY(F.groupnorm(v.attn_gn, m0, nullptr, VAE_EPS, false, &n));
        DM_TRY(F.dense(v.qkv, n, nullptr, nullptr, EPI_PLAIN, &qkv));
        F.free(n);
        DM_TRY(F.alloc(&a, m0.N, m0.H, m0.W, C));
        if (!dry) {
            DM_TRY(F.prof_begin(1, 4.0 * m0.N * (double)T * T * C));
            DM_HIP(e, launch_attention512(qkv.p, qkv.p + C, qkv.p + 2 * C, a.p, m0.N, T, 3 * C, C, 1.0f / sqrtf((float)C), s));
            DM_TRY(F.prof_end());
        }
        F.free(qkv);
        DM_TRY(F.dense(v.o, a, nullptr, &m0, EPI_PLAIN, &m1));
        F.free(a); F.free(m0);
        DM_TRY(F.resnet(v.mid[1], m1, nullptr, nullptr, &m2));
        F.free(m1);
        cur = m2;
    }
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 3; ++j) {
            Tensor r;
            DM_TRY(F.resnet(v.up[i][j], cur, nullptr, nullptr, &r));
            F.free(cur);
            cur = r;
        }
        if (i != VNB - 1) {
            Tensor up;      // Upsample2D: nearest 2x, then conv3x3 (the 64-channel-wave tiles: 512 / 256 output channels)
            DM_TRY(F.igemm(v.us[i], IG_CONV3_UP, cur, nullptr, 2 * cur.H, 2 * cur.W, nullptr, 0, nullptr, EPI_PLAIN, &up));
            F.free(cur);
            cur = up;
        }
    }
    // conv_norm_out + SiLU + conv_out + post-processing: the statistics pass as everywhere, then one kernel (sample.hip)
    const int C = cur.C, HW = cur.H * cur.W;
    if (C != v.norm_out.c) DM_FAIL(e, "vae decoder: channel mismatch %d vs %d", C, v.norm_out.c);
    size_t poff, aoff; void *pp, *ap;
    DM_TRY(F.alloc_raw((size_t)cur.N * gn_stats_chunks(HW) * GROUPS * 2 * sizeof(double), &poff, &pp));
    DM_TRY(F.alloc_raw((size_t)cur.N * 2 * C * sizeof(float), &aoff, &ap));
    if (!dry) {
        DM_HIP(e, launch_gn_stats(cur.p, nullptr, cur.N, HW, C, C, GROUPS, (double*)pp, s));
        DM_HIP(e, launch_gn_affine((const double*)pp, cur.N, HW, C, GROUPS, VAE_EPS, v.norm_out.g, v.norm_out.b, (float*)ap, s));
        DM_HIP(e, launch_decoder_tail(cur.p, (const float*)ap, v.conv_out.w, v.conv_out.b, cur.N, cur.H, cur.W, C, A.raw, A.image, s));
    }
    F.free_raw(poff); F.free_raw(aoff);
    F.free(cur);
    return 0;
}

// ---- CLIP text tower: token ids -> last_hidden_state (compute.py:39-51) -------------------------
int dm::eng::run_clip(dm_engine* e, const int32_t* ids, int n, f16* out16, float* out32, hipStream_t s, bool dry) {
    Fwd F{e, s, dry};
    const ClipW& c = e->clip;
    const int M = n * CL_T;
    Tensor x;
    DM_TRY(F.alloc(&x, 1, 1, M, CL_H));
    if (!dry) DM_HIP(e, launch_clip_embed(ids, c.tok, c.pos, M, CL_T, CL_H, CL_VOCAB, x.p, s));
    for (int l = 0; l < CL_LAYERS; ++l) {
        const ClipLayerW& L = c.layer[l];
        Tensor h, qkv, a, x1, f, x2;
        DM_TRY(F.layernorm(L.ln1, x, &h));
        DM_TRY(F.dense(L.qkv, h, nullptr, nullptr, EPI_PLAIN, &qkv));
        F.free(h);
        DM_TRY(F.alloc(&a, 1, 1, M, CL_H));
        if (!dry) DM_HIP(e, launch_clip_attention(qkv.p, n, CL_T, CL_HEADS, a.p, s));
        F.free(qkv);
        DM_TRY(F.dense(L.o, a, nullptr, &x, EPI_PLAIN, &x1));
        F.free(a); F.free(x);
        DM_TRY(F.layernorm(L.ln2, x1, &h));
        DM_TRY(F.dense(L.fc1, h, nullptr, nullptr, EPI_PLAIN, &f));
        F.free(h);
        if (!dry) DM_HIP(e, launch_quick_gelu(f.p, (long long)M * CL_F, s));
        DM_TRY(F.dense(L.fc2, f, nullptr, &x1, EPI_PLAIN, &x2));
        F.free(f); F.free(x1);
        x = x2;
    }
    Tensor y;
    DM_TRY(F.layernorm(c.final_ln, x, &y));
    F.free(x);
    if (!dry) {
        if (out16) DM_HIP(e, hipMemcpyAsync(out16, y.p, (size_t)M * CL_H * sizeof(f16), hipMemcpyDeviceToDevice, s));
        if (out32) DM_HIP(e, launch_f16_to_f32(y.p, out32, (long long)M * CL_H, s));
    }
    F.free(y);
    return 0;
}
