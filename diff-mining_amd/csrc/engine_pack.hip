// engine_pack.hip — weight intake of the fp16 engine: the staged state dicts (diffusers names) packed into the MFMA-friendly HBM
// layout of one slab per network (U-Net, VAE encoder, VAE decoder, CLIP text tower), and the scheduler / sinusoid tables.
#include "engine_impl.h"

#include <cmath>
#include <cstring>

using namespace dm;
using namespace dm::eng;
using namespace sd15;

namespace {

using HostTensor = dm::HostTensorT<f16>;

// ------------------------------------------------------------------------------------------------
// host-side scheduler / sinusoid tables (also exported for the CPU test tier)
// ------------------------------------------------------------------------------------------------
void host_alphas_cumprod(int n, float beta_start, float beta_end, float* out) {
    // torch.linspace(sqrt(bs), sqrt(be), n, dtype=float32) ** 2 ; cumprod(1 - betas)
    // (linspace: symmetric fp32 evaluation; CPU cumprod accumulates in double, emits fp32)
    const float start = (float)std::sqrt((double)beta_start), end = (float)std::sqrt((double)beta_end);
    const float step = (end - start) / (float)(n - 1);
    const int half = n / 2;
    double acc = 1.0;
    for (int i = 0; i < n; ++i) {
        const float v = (i < half) ? (start + step * (float)i) : (end - step * (float)(n - i - 1));
        const float beta = v * v;
        const float alpha = 1.0f - beta;
        acc *= (double)alpha;
        out[i] = (float)acc;
    }
}

void host_sinusoid(int t, int dim, float* out) {
    const int half = dim / 2;
    const float ln1e4 = (float)std::log(10000.0);
    for (int k = 0; k < half; ++k) {
        const float exponent = (-ln1e4 * (float)k) / (float)half;
        const float f = expf(exponent);
        const float a = (float)t * f;
        out[k] = cosf(a);
        out[half + k] = sinf(a);
    }
}

// ------------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------------
struct Packer {             // one finalize: reads the staged tensors of `set`, owns the host image of its slab
    dm_engine* e;
    dm::WeightSet<f16>& set;
    std::vector<char> blob;
    std::vector<char> scratch;                             // operands needed only while finalize runs (freed afterwards)
    size_t put_scratch(const void* src, size_t bytes) {
        size_t off = (scratch.size() + 255) & ~(size_t)255;
        scratch.resize(off + bytes);
        memcpy(scratch.data() + off, src, bytes);
        return off;
    }
    size_t put(const void* src, size_t bytes) {
        size_t off = (blob.size() + 255) & ~(size_t)255;
        blob.resize(off + bytes);
        memcpy(blob.data() + off, src, bytes);
        return off;
    }
    HostTensor* get(const std::string& name, std::initializer_list<int64_t> shape) { return set.get(name, shape, e->err); }
    int finish(const char* what, size_t expected) {
        DM_TRY(set.finish(blob.data(), blob.size(), what, expected, e->err));
        ++e->n_device_allocs;
        return 0;
    }
};

// offsets are stored in the pointer fields during packing and rebased after upload
inline const f16* as_ptr(size_t off) { return reinterpret_cast<const f16*>(off + 1); }   // +1: keep 0 = null
inline const float* as_fptr(size_t off) { return reinterpret_cast<const float*>(off + 1); }

int pack_bias(Packer& P, const std::string& name, int c, const f16** out) {
    HostTensor* b = P.get(name + ".bias", {c});
    if (!b) return 1;
    *out = as_ptr(P.put(b->data.data(), (size_t)c * 2));
    return 0;
}

int pack_conv3(Packer& P, const std::string& name, int cout, int cin, ConvW* o) {
    HostTensor* w = P.get(name + ".weight", {cout, cin, 3, 3});
    if (!w) return 1;
    std::vector<f16> pk((size_t)cout * 9 * cin);
    const f16* src = w->data.data();
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap)
                pk[((size_t)co * 9 + tap) * cin + ci] = src[((size_t)co * cin + ci) * 9 + tap];
    o->w = as_ptr(P.put(pk.data(), pk.size() * 2));
    o->cin = cin; o->cout = cout; o->k = 3;
    return pack_bias(P, name, cout, &o->b);
}

// Upsample2D.conv folded onto the source grid: four 2x2 kernels (dm_kernels.h); shares the bias of the packed 3x3 layer `full`
int pack_upconv4(Packer& P, const std::string& name, int cout, int cin, const ConvW& full, ConvW* o) {
    HostTensor* w = P.get(name + ".weight", {cout, cin, 3, 3});
    if (!w) return 1;
    std::vector<f16> pk((size_t)16 * cout * cin);
    fold_upconv_weights(w->data.data(), cout, cin, pk.data());
    o->w = as_ptr(P.put(pk.data(), pk.size() * 2));
    o->cin = cin; o->cout = cout; o->k = 2; o->b = full.b;
    return 0;
}

int pack_dense(Packer& P, const std::string& name, int cout, int cin, bool conv1x1, bool bias, ConvW* o) {
    HostTensor* w = conv1x1 ? P.get(name + ".weight", {cout, cin, 1, 1}) : P.get(name + ".weight", {cout, cin});
    if (!w) return 1;
    o->w = as_ptr(P.put(w->data.data(), (size_t)cout * cin * 2));
    o->cin = cin; o->cout = cout; o->k = 1; o->b = nullptr;
    return bias ? pack_bias(P, name, cout, &o->b) : 0;
}

int pack_norm(Packer& P, const std::string& name, int c, NormW* o) {
    HostTensor* g = P.get(name + ".weight", {c});
    HostTensor* b = P.get(name + ".bias", {c});
    if (!g || !b) return 1;
    std::vector<float> fg(c), fb(c);
    for (int i = 0; i < c; ++i) { fg[i] = (float)g->data[i]; fb[i] = (float)b->data[i]; }
    o->g = as_fptr(P.put(fg.data(), (size_t)c * 4));
    o->b = as_fptr(P.put(fb.data(), (size_t)c * 4));
    o->c = c;
    return 0;
}

// several [rows_i, cin] matrices stacked along rows (fused QKV / cross K,V)
int pack_stack(Packer& P, const std::vector<std::string>& names, int rows_each, int cin, ConvW* o) {
    std::vector<f16> pk((size_t)names.size() * rows_each * cin);
    for (size_t i = 0; i < names.size(); ++i) {
        HostTensor* w = P.get(names[i] + ".weight", {rows_each, cin});
        if (!w) return 1;
        memcpy(pk.data() + i * (size_t)rows_each * cin, w->data.data(), (size_t)rows_each * cin * 2);
    }
    o->w = as_ptr(P.put(pk.data(), pk.size() * 2));
    o->cin = cin; o->cout = (int)names.size() * rows_each; o->k = 1; o->b = nullptr;
    return 0;
}

// the biases [c] of the stacked layers, concatenated (the caller puts them: CLIP scales the q part first)
int stack_bias(Packer& P, const std::vector<std::string>& names, int c, std::vector<f16>* out) {
    for (const std::string& n : names) {
        HostTensor* b = P.get(n + ".bias", {c});
        if (!b) return 1;
        out->insert(out->end(), b->data.begin(), b->data.end());
    }
    return 0;
}

// GEGLU projection [8C, C]: rows permuted so that every MFMA lane holds (h0,h1,g0,g1) quads:
// packed row rho = 16F + 4q + r  <-  r<2 ? hidden 8F+2q+r : gate 4C + 8F+2q+(r-2)
int pack_geglu(Packer& P, const std::string& name, int c, ConvW* o) {
    HostTensor* w = P.get(name + ".weight", {8 * c, c});
    HostTensor* b = P.get(name + ".bias", {8 * c});
    if (!w || !b) return 1;
    std::vector<f16> pk((size_t)8 * c * c), pb((size_t)8 * c);
    for (int rho = 0; rho < 8 * c; ++rho) {
        const int F = rho >> 4, q = (rho & 15) >> 2, r = rho & 3;
        const int srcr = (r < 2) ? (8 * F + 2 * q + r) : (4 * c + 8 * F + 2 * q + (r - 2));
        memcpy(pk.data() + (size_t)rho * c, w->data.data() + (size_t)srcr * c, (size_t)c * 2);
        pb[rho] = b->data[srcr];
    }
    o->w = as_ptr(P.put(pk.data(), pk.size() * 2));
    o->b = as_ptr(P.put(pb.data(), pb.size() * 2));
    o->cin = c; o->cout = 8 * c; o->k = 1;
    return 0;
}

// LayerNorm(gamma, beta) followed by Linear(W [rows][c], bias): W' = fp16(W * gamma) (row order given by `perm`, the
// GEGLU quad interleave, or identity), s[n] = sum_k W'[n][k], t[n] = sum_k W[n][k] beta[k] + bias[n]  (fp32).
int pack_ln_fold(Packer& P, const std::string& ln, const std::vector<std::string>& mats, int rows_each, int c,
                 const std::string& bias_name, bool geglu, LnFold* o) {
    HostTensor* g = P.get(ln + ".weight", {c});
    HostTensor* b = P.get(ln + ".bias", {c});
    if (!g || !b) return 1;
    const int rows = (int)mats.size() * rows_each;
    std::vector<f16> wp((size_t)rows * c);
    std::vector<float> sv(rows), tv(rows);
    HostTensor* bias = bias_name.empty() ? nullptr : P.get(bias_name, {rows});
    if (!bias_name.empty() && !bias) return 1;
    for (int rho = 0; rho < rows; ++rho) {
        int srcr = rho;
        if (geglu) {            // packed row rho = 16F + 4q + r  <-  r<2 ? hidden 8F+2q+r : gate rows/2 + 8F+2q+(r-2)
            const int F = rho >> 4, q = (rho & 15) >> 2, r = rho & 3;
            srcr = (r < 2) ? (8 * F + 2 * q + r) : (rows / 2 + 8 * F + 2 * q + (r - 2));
        }
        HostTensor* w = P.get(mats[srcr / rows_each] + ".weight", {rows_each, c});
        if (!w) return 1;
        const f16* wr = w->data.data() + (size_t)(srcr % rows_each) * c;
        double ss = 0.0, tt = 0.0;
        for (int k = 0; k < c; ++k) {
            const f16 wf = (f16)((float)wr[k] * (float)g->data[k]);
            wp[(size_t)rho * c + k] = wf;
            ss += (double)(float)wf;
            tt += (double)(float)wr[k] * (double)(float)b->data[k];
        }
        sv[rho] = (float)ss;
        tv[rho] = (float)(tt + (bias ? (double)(float)bias->data[srcr] : 0.0));
    }
    o->w.w = as_ptr(P.put(wp.data(), wp.size() * 2));
    o->w.b = nullptr; o->w.cin = c; o->w.cout = rows; o->w.k = 1;
    o->s = as_fptr(P.put(sv.data(), sv.size() * 4));
    o->t = as_fptr(P.put(tv.data(), tv.size() * 4));
    return 0;
}

int pack_vae_resnet(Packer& P, const std::string& name, int cin, int cout, ResW* r) {
    r->cin = cin; r->cout = cout;
    DM_TRY(pack_norm(P, name + ".norm1", cin, &r->n1));
    DM_TRY(pack_conv3(P, name + ".conv1", cout, cin, &r->c1));
    DM_TRY(pack_norm(P, name + ".norm2", cout, &r->n2));
    DM_TRY(pack_conv3(P, name + ".conv2", cout, cout, &r->c2));
    r->has_sc = (cin != cout);
    if (r->has_sc) DM_TRY(pack_dense(P, name + ".conv_shortcut", cout, cin, true, true, &r->sc));
    return 0;
}

// the U-Net's ResnetBlock2D = the VAE's + a time-embedding projection (rows to tw / tb, not to the blob) + conv2 with the shortcut folded in
int pack_resnet(Packer& P, const std::string& name, int cin, int cout, ResW* r, std::vector<f16>& tw, std::vector<f16>& tb) {
    HostTensor* w = P.get(name + ".time_emb_proj.weight", {cout, TEMB});
    HostTensor* b = P.get(name + ".time_emb_proj.bias", {cout});
    if (!w || !b) return 1;
    r->temb_off = (int)tb.size();
    tw.insert(tw.end(), w->data.begin(), w->data.end());
    tb.insert(tb.end(), b->data.begin(), b->data.end());
    DM_TRY(pack_vae_resnet(P, name, cin, cout, r));
    if (r->has_sc && cin % 64 == 0) {
        // conv2 with the shortcut folded in (igemm_pers_tile.h, SC): weight rows [9 * cout (tap, c) | cin], bias = b2 + b_sc
        HostTensor* w2 = P.get(name + ".conv2.weight", {cout, cout, 3, 3});
        HostTensor* b2 = P.get(name + ".conv2.bias", {cout});
        HostTensor* ws = P.get(name + ".conv_shortcut.weight", {cout, cin, 1, 1});
        HostTensor* bs = P.get(name + ".conv_shortcut.bias", {cout});
        if (!w2 || !b2 || !ws || !bs) return 1;
        const size_t K = (size_t)9 * cout + cin;
        std::vector<f16> pk((size_t)cout * K), pb(cout);
        for (int co = 0; co < cout; ++co) {
            for (int ci = 0; ci < cout; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    pk[(size_t)co * K + (size_t)tap * cout + ci] = w2->data[((size_t)co * cout + ci) * 9 + tap];
            memcpy(pk.data() + (size_t)co * K + (size_t)9 * cout, ws->data.data() + (size_t)co * cin, (size_t)cin * 2);
            pb[co] = (f16)((float)b2->data[co] + (float)bs->data[co]);
        }
        r->c2sc.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        r->c2sc.b = as_ptr(P.put(pb.data(), pb.size() * 2));
        r->c2sc.cin = cout; r->c2sc.cout = cout; r->c2sc.k = 3; r->c2sc.csc = cin;
    }
    return 0;
}

int pack_tfm(Packer& P, const std::string& name, int c, TfmW* t, dm_engine* e) {
    t->c = c; t->layer = e->n_tf++;
    e->tfs.push_back(t);
    DM_TRY(pack_norm(P, name + ".norm", c, &t->gn));
    DM_TRY(pack_dense(P, name + ".proj_in", c, c, true, true, &t->proj_in));
    const std::string b = name + ".transformer_blocks.0";
    DM_TRY(pack_norm(P, b + ".norm1", c, &t->ln1));
    DM_TRY(pack_stack(P, {b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"}, c, c, &t->qkv));
    DM_TRY(pack_dense(P, b + ".attn1.to_out.0", c, c, false, true, &t->o1));
    DM_TRY(pack_norm(P, b + ".norm2", c, &t->ln2));
    DM_TRY(pack_dense(P, b + ".attn2.to_q", c, c, false, false, &t->q2));
    DM_TRY(pack_stack(P, {b + ".attn2.to_k", b + ".attn2.to_v"}, c, CTX_DIM, &t->kv2));
    DM_TRY(pack_dense(P, b + ".attn2.to_out.0", c, c, false, true, &t->o2));
    DM_TRY(pack_norm(P, b + ".norm3", c, &t->ln3));
    DM_TRY(pack_geglu(P, b + ".ff.net.0.proj", c, &t->ff1));
    DM_TRY(pack_dense(P, b + ".ff.net.2", c, 4 * c, false, true, &t->ff2));
    DM_TRY(pack_dense(P, name + ".proj_out", c, c, true, true, &t->proj_out));
    {
        // ff.net.2 -> (+ residual) -> proj_out is a linear chain: out = Wp (W2 f + b2 + t2) + bp + x = (Wp W2) f + Wp t2 + (Wp b2 + bp) + x.
        // One GEMM over [f | t2] with weight rows [(Wp W2)[o] | Wp[o]] (igemm SC variant, dense mode).  The product is formed on
        // the GPU at finalize from W2^T (fp32 accumulation, one rounding to fp16); here: W2^T, Wp's columns, the bias.
        HostTensor* w2 = P.get(b + ".ff.net.2.weight", {c, 4 * c});
        HostTensor* b2 = P.get(b + ".ff.net.2.bias", {c});
        HostTensor* wp = P.get(name + ".proj_out.weight", {c, c, 1, 1});
        HostTensor* bp = P.get(name + ".proj_out.bias", {c});
        if (!w2 || !b2 || !wp || !bp) return 1;
        std::vector<f16> w2t((size_t)4 * c * c);
        for (int o = 0; o < c; ++o)
            for (int j = 0; j < 4 * c; ++j) w2t[(size_t)j * c + o] = w2->data[(size_t)o * 4 * c + j];
        t->w2t_off = P.put_scratch(w2t.data(), w2t.size() * 2);      // dead after finalize: not in the weight slab
        const size_t K = (size_t)5 * c;
        std::vector<f16> pk((size_t)c * K, (f16)0.f), pb(c);
        for (int o = 0; o < c; ++o) {
            memcpy(pk.data() + (size_t)o * K + (size_t)4 * c, wp->data.data() + (size_t)o * c, (size_t)c * 2);
            double acc = (double)(float)bp->data[o];
            for (int k = 0; k < c; ++k) acc += (double)(float)wp->data[(size_t)o * c + k] * (double)(float)b2->data[k];
            pb[o] = (f16)(float)acc;
        }
        t->ffp.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        t->ffp.b = as_ptr(P.put(pb.data(), pb.size() * 2));
        t->ffp.cin = 4 * c; t->ffp.cout = c; t->ffp.k = 1; t->ffp.csc = c;
    }
    // the three LayerNorm -> Linear pairs, folded (the unfused weights above stay for DM_LN_FOLD=0)
    DM_TRY(pack_ln_fold(P, b + ".norm1", {b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"}, c, c, "", false, &t->qkv_ln));
    DM_TRY(pack_ln_fold(P, b + ".norm2", {b + ".attn2.to_q"}, c, c, "", false, &t->q2_ln));
    DM_TRY(pack_ln_fold(P, b + ".norm3", {b + ".ff.net.0.proj"}, 8 * c, c, b + ".ff.net.0.proj.bias", true, &t->ff1_ln));
    return 0;
}

template <typename T> void rebase(const T*& p, char* base) {
    if (p) p = reinterpret_cast<const T*>(base + (reinterpret_cast<size_t>(p) - 1));
}
void rebase_conv(ConvW& c, char* base) { rebase(c.w, base); rebase(c.b, base); }
void rebase_norm(NormW& n, char* base) { rebase(n.g, base); rebase(n.b, base); }
void rebase_res(ResW& r, char* base) {
    rebase_norm(r.n1, base); rebase_norm(r.n2, base); rebase_conv(r.c1, base); rebase_conv(r.c2, base); rebase_conv(r.sc, base);
    rebase_conv(r.c2sc, base);
}
void rebase_tfm(TfmW& t, char* base) {
    rebase_norm(t.gn, base); rebase_norm(t.ln1, base); rebase_norm(t.ln2, base); rebase_norm(t.ln3, base);
    rebase_conv(t.proj_in, base); rebase_conv(t.proj_out, base); rebase_conv(t.qkv, base); rebase_conv(t.o1, base);
    rebase_conv(t.q2, base); rebase_conv(t.kv2, base); rebase_conv(t.o2, base); rebase_conv(t.ff1, base); rebase_conv(t.ff2, base);
    rebase_conv(t.ffp, base);
    for (LnFold* f : {&t.qkv_ln, &t.q2_ln, &t.ff1_ln}) { rebase_conv(f->w, base); rebase(f->s, base); rebase(f->t, base); }
}

}  // namespace

namespace dm {

void fold_upconv_weights(const f16* w, int cout, int cin, f16* out) {
    // parity class p (0 / 1) of an output coordinate, 2x2 tap a (0 / 1): the 3x3 taps d whose up-sampled coordinate 2 y + p + d - 1
    // falls on source coordinate y - 1 + p + a.   p = 0: a = 0 <- {0}, a = 1 <- {1, 2};   p = 1: a = 0 <- {0, 1}, a = 1 <- {2}
    static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            f16* o = out + (size_t)(py * 2 + px) * cout * 4 * cin;
            for (int co = 0; co < cout; ++co)
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b)
                        for (int ci = 0; ci < cin; ++ci) {
                            const f16* k9 = w + ((size_t)co * cin + ci) * 9;
                            float acc = 0.f;                  // <= 4 fp16 terms: exact in fp32
                            for (int dy = lo[py][a]; dy <= hi[py][a]; ++dy)
                                for (int dx = lo[px][b]; dx <= hi[px][b]; ++dx) acc += (float)k9[dy * 3 + dx];
                            o[(size_t)co * 4 * cin + (size_t)(a * 2 + b) * cin + ci] = (f16)acc;
                        }
        }
}

}  // namespace dm

extern "C" {

int dm_scheduler_alphas_cumprod(int n, float beta_start, float beta_end, float* out) {
    if (n < 2 || !out) return 1;
    host_alphas_cumprod(n, beta_start, beta_end, out);
    return 0;
}

int dm_timestep_sinusoid(int t, int dim, float* out) {
    if (dim < 2 || (dim & 1) || !out) return 1;
    host_sinusoid(t, dim, out);
    return 0;
}

int dm_engine_load_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->finalized) DM_FAIL(e, "load_weight after finalize");
    return dm::stage_tensor(e->w_unet.host, name, host_ptr, dtype, shape, ndim, e->err);
}

int dm_engine_finalize(dm_engine* e) {
    if (!e) return 1;
    if (e->finalized) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer P{e, e->w_unet};
    std::vector<f16> tw, tb;
    e->n_tf = 0; e->tfs.clear();
    // conv_in as a dense GEMM over the im2col rows: [C0][64], k = c*9 + ky*3 + kx (PyTorch order), zero padded
    {
        HostTensor* w = P.get("conv_in.weight", {BOC[0], 4, 3, 3});
        if (!w) return 1;
        std::vector<f16> pk((size_t)BOC[0] * 64, (f16)0.f);
        for (int co = 0; co < BOC[0]; ++co)
            for (int k = 0; k < 36; ++k) pk[(size_t)co * 64 + k] = w->data[(size_t)co * 36 + k];
        e->conv_in.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        e->conv_in.cin = 64; e->conv_in.cout = BOC[0]; e->conv_in.k = 1;
        DM_TRY(pack_bias(P, "conv_in", BOC[0], &e->conv_in.b));
    }
    DM_TRY(pack_dense(P, "time_embedding.linear_1", TEMB, BOC[0], false, true, &e->time1));
    DM_TRY(pack_dense(P, "time_embedding.linear_2", TEMB, TEMB, false, true, &e->time2));
    int cin = BOC[0];
    for (int i = 0; i < NB; ++i) {
        DownBlockW& d = e->down[i];
        d.attn = DOWN_ATTN[i];
        const int cout = BOC[i];
        for (int j = 0; j < LAYERS; ++j) {
            const std::string rn = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
            DM_TRY(pack_resnet(P, rn, j == 0 ? cin : cout, cout, &d.res[j], tw, tb));
            if (d.attn) DM_TRY(pack_tfm(P, "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), cout, &d.tf[j], e));
        }
        d.has_down = (i != NB - 1);
        if (d.has_down) DM_TRY(pack_conv3(P, "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", cout, cout, &d.down));
        cin = cout;
    }
    DM_TRY(pack_resnet(P, "mid_block.resnets.0", BOC[NB - 1], BOC[NB - 1], &e->mid_res[0], tw, tb));
    DM_TRY(pack_tfm(P, "mid_block.attentions.0", BOC[NB - 1], &e->mid_tf, e));
    DM_TRY(pack_resnet(P, "mid_block.resnets.1", BOC[NB - 1], BOC[NB - 1], &e->mid_res[1], tw, tb));
    {
        int rev[NB];
        for (int i = 0; i < NB; ++i) rev[i] = BOC[NB - 1 - i];
        int prev = rev[0];
        for (int i = 0; i < NB; ++i) {
            UpBlockW& u = e->up[i];
            u.attn = UP_ATTN[i];
            const int o = rev[i];
            const int inp = rev[i + 1 < NB ? i + 1 : NB - 1];
            for (int j = 0; j < LAYERS + 1; ++j) {
                const int skip = (j == LAYERS) ? inp : o;
                const int rin = (j == 0) ? prev : o;
                const std::string rn = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
                DM_TRY(pack_resnet(P, rn, rin + skip, o, &u.res[j], tw, tb));
                if (u.attn) DM_TRY(pack_tfm(P, "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), o, &u.tf[j], e));
            }
            u.has_up = (i != NB - 1);
            if (u.has_up) {
                DM_TRY(pack_conv3(P, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", o, o, &u.up));
                if (o % 320 == 0) DM_TRY(pack_upconv4(P, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", o, o, u.up, &u.up4));
            }
            prev = o;
        }
    }
    DM_TRY(pack_norm(P, "conv_norm_out", BOC[0], &e->norm_out));
    {
        // conv_out packed [4][tap*C0 + c]
        HostTensor* w = P.get("conv_out.weight", {4, BOC[0], 3, 3});
        if (!w) return 1;
        std::vector<f16> pk((size_t)4 * 9 * BOC[0]);
        for (int co = 0; co < 4; ++co)
            for (int ci = 0; ci < BOC[0]; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    pk[((size_t)co * 9 + tap) * BOC[0] + ci] = w->data[((size_t)co * BOC[0] + ci) * 9 + tap];
        e->conv_out.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        e->conv_out.cin = BOC[0]; e->conv_out.cout = 4; e->conv_out.k = 3;
        DM_TRY(pack_bias(P, "conv_out", 4, &e->conv_out.b));
    }
    // all time_emb_proj stacked: [sum Cout][1280]
    e->tproj_total = (int)tb.size();
    e->tproj_all.w = as_ptr(P.put(tw.data(), tw.size() * 2));
    e->tproj_all.b = as_ptr(P.put(tb.data(), tb.size() * 2));
    e->tproj_all.cin = TEMB; e->tproj_all.cout = e->tproj_total; e->tproj_all.k = 1;

    DM_TRY(P.finish("U-Net", 686));
    char* base = (char*)e->w_unet.slab;
    rebase_conv(e->conv_in, base); rebase_conv(e->conv_out, base); rebase_conv(e->time1, base); rebase_conv(e->time2, base);
    rebase_conv(e->tproj_all, base); rebase_norm(e->norm_out, base);
    for (int i = 0; i < NB; ++i) {
        for (int j = 0; j < LAYERS; ++j) { rebase_res(e->down[i].res[j], base); if (e->down[i].attn) rebase_tfm(e->down[i].tf[j], base); }
        rebase_conv(e->down[i].down, base);
        for (int j = 0; j < LAYERS + 1; ++j) { rebase_res(e->up[i].res[j], base); if (e->up[i].attn) rebase_tfm(e->up[i].tf[j], base); }
        rebase_conv(e->up[i].up, base); rebase_conv(e->up[i].up4, base);
    }
    rebase_res(e->mid_res[0], base); rebase_res(e->mid_res[1], base); rebase_tfm(e->mid_tf, base);
    // (Wp W2) of every transformer block into the first 4C columns of its fused rows: Y[o][j] = sum_c Wp[o][c] W2^T[j][c];
    // the W2^T operands live in a temporary buffer
    char* scratch = nullptr;
    DM_HIP(e, hipMalloc((void**)&scratch, P.scratch.size() ? P.scratch.size() : 256));
    DM_HIP(e, hipMemcpy(scratch, P.scratch.data(), P.scratch.size(), hipMemcpyHostToDevice));
    for (TfmW* t : e->tfs) {
        IGemmParams p;
        p.X = t->proj_out.w; p.X2 = nullptr; p.Wp = reinterpret_cast<const f16*>(scratch + t->w2t_off); p.bias = nullptr; p.temb = nullptr;
        p.res = nullptr; p.Y = const_cast<f16*>(t->ffp.w); p.M = t->c; p.Cout = 4 * t->c; p.Cin = t->c; p.C1 = t->c;
        p.H = 1; p.W = p.M; p.OH = 1; p.OW = p.M; p.mode = IG_DENSE; p.epi = EPI_PLAIN; p.ldy = 5 * t->c; p.ldres = 0; p.temb_ld = 0;
        DM_HIP(e, launch_igemm(p, nullptr));
    }
    DM_HIP(e, hipDeviceSynchronize());
    DM_HIP(e, hipFree(scratch));

    // scheduler + sinusoid tables
    {
        std::vector<float> acp(NTRAIN);
        host_alphas_cumprod(NTRAIN, 0.00085f, 0.012f, acp.data());
        std::vector<f16> sa(NTRAIN), sb(NTRAIN);
        for (int t = 0; t < NTRAIN; ++t) {
            const f16 a16 = (f16)acp[t];                        // table cast to fp16 FIRST (R3)
            sa[t] = (f16)sqrtf((float)a16);                     // fp16 pow(0.5): fp32 compute, fp16 result
            const f16 om = (f16)(1.0f - (float)a16);            // fp16 subtraction
            sb[t] = (f16)sqrtf((float)om);
        }
        DM_MALLOC(e, &e->sa_tab, NTRAIN * 2);
        DM_MALLOC(e, &e->sb_tab, NTRAIN * 2);
        DM_HIP(e, hipMemcpy(e->sa_tab, sa.data(), NTRAIN * 2, hipMemcpyHostToDevice));
        DM_HIP(e, hipMemcpy(e->sb_tab, sb.data(), NTRAIN * 2, hipMemcpyHostToDevice));
        // fp32 flow: `alphas_cumprod[t] ** 0.5`, `(1 - alphas_cumprod[t]) ** 0.5` on the fp32 table
        std::vector<float> sa32(NTRAIN), sb32(NTRAIN);
        for (int t = 0; t < NTRAIN; ++t) { sa32[t] = sqrtf(acp[t]); sb32[t] = sqrtf(1.0f - acp[t]); }
        DM_MALLOC(e, &e->sa32_tab, NTRAIN * 4);
        DM_MALLOC(e, &e->sb32_tab, NTRAIN * 4);
        DM_HIP(e, hipMemcpy(e->sa32_tab, sa32.data(), NTRAIN * 4, hipMemcpyHostToDevice));
        DM_HIP(e, hipMemcpy(e->sb32_tab, sb32.data(), NTRAIN * 4, hipMemcpyHostToDevice));
        std::vector<f16> tab((size_t)NTRAIN * BOC[0]);
        std::vector<float> row(BOC[0]);
        for (int t = 0; t < NTRAIN; ++t) {
            host_sinusoid(t, BOC[0], row.data());
            for (int k = 0; k < BOC[0]; ++k) tab[(size_t)t * BOC[0] + k] = (f16)row[k];
        }
        DM_MALLOC(e, &e->sin_table, tab.size() * 2);
        DM_HIP(e, hipMemcpy(e->sin_table, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));
    }
    e->kv_cache.assign(e->n_tf, nullptr);
    // tile hand-out counters of the persistent igemm kernel: this engine's own (8 XCD counters 128 B apart + a completion
    // counter), so two engines / streams on one device never share them; a launch leaves them at zero
    DM_MALLOC(e, &e->tile_ctr, IGEMM_TILE_CTR_INTS * sizeof(int));
    DM_HIP(e, hipMemset(e->tile_ctr, 0, IGEMM_TILE_CTR_INTS * sizeof(int)));
    e->finalized = true;
    return 0;
}

int dm_engine_load_vae_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_vae.ready) DM_FAIL(e, "load_vae_weight after finalize_vae");
    std::string nm(name);
    if (nm.rfind("vae.", 0) == 0) nm = nm.substr(4);
    if (nm.rfind("decoder.", 0) == 0 || nm.rfind("post_quant_conv.", 0) == 0) return 0;     // not on the path
    // pre-0.15 diffusers names of the mid-block attention
    static const char* legacy[4][2] = {{".query.", ".to_q."}, {".key.", ".to_k."}, {".value.", ".to_v."}, {".proj_attn.", ".to_out.0."}};
    for (auto& l : legacy) { const size_t at = nm.find(l[0]); if (at != std::string::npos) nm.replace(at, strlen(l[0]), l[1]); }
    // legacy checkpoints store the attention projections as 1x1 convs [C, C, 1, 1]: staged as [C, C]
    if (nm.find(".attentions.0.to_") != std::string::npos && ndim == 4 && shape[2] == 1 && shape[3] == 1) ndim = 2;
    return dm::stage_tensor(e->w_vae.host, nm, host_ptr, dtype, shape, ndim, e->err);
}

int dm_engine_finalize_vae(dm_engine* e) {
    if (!e) return 1;
    if (e->w_vae.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer P{e, e->w_vae};
    VaeW& v = e->vae;
    {
        HostTensor* w = P.get("encoder.conv_in.weight", {VBOC[0], 3, 3, 3});
        if (!w) return 1;
        std::vector<f16> pk((size_t)VBOC[0] * 64, (f16)0.f);
        for (int co = 0; co < VBOC[0]; ++co)
            for (int k = 0; k < 27; ++k) pk[(size_t)co * 64 + k] = w->data[(size_t)co * 27 + k];
        v.conv_in.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        v.conv_in.cin = 64; v.conv_in.cout = VBOC[0]; v.conv_in.k = 1;
        DM_TRY(pack_bias(P, "encoder.conv_in", VBOC[0], &v.conv_in.b));
    }
    int cin = VBOC[0];
    for (int i = 0; i < VNB; ++i) {
        const int cout = VBOC[i];
        const std::string bn = "encoder.down_blocks." + std::to_string(i);
        for (int j = 0; j < 2; ++j)
            DM_TRY(pack_vae_resnet(P, bn + ".resnets." + std::to_string(j), j == 0 ? cin : cout, cout, &v.down[i][j]));
        if (i != VNB - 1) DM_TRY(pack_conv3(P, bn + ".downsamplers.0.conv", cout, cout, &v.ds[i]));
        cin = cout;
    }
    const int C = VBOC[VNB - 1];
    DM_TRY(pack_vae_resnet(P, "encoder.mid_block.resnets.0", C, C, &v.mid[0]));
    {
        const std::string a = "encoder.mid_block.attentions.0";
        DM_TRY(pack_norm(P, a + ".group_norm", C, &v.attn_gn));
        DM_TRY(pack_stack(P, {a + ".to_q", a + ".to_k", a + ".to_v"}, C, C, &v.qkv));
        std::vector<f16> qb;
        DM_TRY(stack_bias(P, {a + ".to_q", a + ".to_k", a + ".to_v"}, C, &qb));
        v.qkv.b = as_ptr(P.put(qb.data(), qb.size() * 2));
        DM_TRY(pack_dense(P, a + ".to_out.0", C, C, false, true, &v.o));
    }
    DM_TRY(pack_vae_resnet(P, "encoder.mid_block.resnets.1", C, C, &v.mid[1]));
    DM_TRY(pack_norm(P, "encoder.conv_norm_out", C, &v.norm_out));
    {
        // conv_out 512 -> 8, rows zero-padded to one 128-channel igemm tile: [128][tap*C + c]
        HostTensor* w = P.get("encoder.conv_out.weight", {8, C, 3, 3});
        HostTensor* b = P.get("encoder.conv_out.bias", {8});
        if (!w || !b) return 1;
        std::vector<f16> pk((size_t)128 * 9 * C, (f16)0.f), pb(128, (f16)0.f);
        for (int co = 0; co < 8; ++co) {
            for (int ci = 0; ci < C; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    pk[((size_t)co * 9 + tap) * C + ci] = w->data[((size_t)co * C + ci) * 9 + tap];
            pb[co] = b->data[co];
        }
        v.conv_out.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        v.conv_out.b = as_ptr(P.put(pb.data(), pb.size() * 2));
        v.conv_out.cin = C; v.conv_out.cout = 128; v.conv_out.k = 3;
        HostTensor* qw = P.get("quant_conv.weight", {8, 8, 1, 1});
        HostTensor* qb = P.get("quant_conv.bias", {8});
        if (!qw || !qb) return 1;
        v.qw = as_ptr(P.put(qw->data.data(), 64 * 2));
        v.qb = as_ptr(P.put(qb->data.data(), 8 * 2));
    }
    DM_TRY(P.finish("VAE", 108));
    char* base = (char*)e->w_vae.slab;
    rebase_conv(v.conv_in, base); rebase_conv(v.qkv, base); rebase_conv(v.o, base); rebase_conv(v.conv_out, base);
    rebase_norm(v.attn_gn, base); rebase_norm(v.norm_out, base);
    rebase(v.qw, base); rebase(v.qb, base);
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 2; ++j) rebase_res(v.down[i][j], base);
        if (i != VNB - 1) rebase_conv(v.ds[i], base);
    }
    rebase_res(v.mid[0], base); rebase_res(v.mid[1], base);
    return 0;
}

int dm_engine_load_vae_decoder_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_vaed.ready) DM_FAIL(e, "load_vae_decoder_weight after finalize_vae_decoder");
    std::string nm(name);
    if (nm.rfind("vae.", 0) == 0) nm = nm.substr(4);
    if (nm.rfind("encoder.", 0) == 0 || nm.rfind("quant_conv.", 0) == 0) return 0;          // the encoder's half
    // the encoder loader's name rules: pre-0.15 attention names, [C, C, 1, 1] projections staged as [C, C]
    static const char* legacy[4][2] = {{".query.", ".to_q."}, {".key.", ".to_k."}, {".value.", ".to_v."}, {".proj_attn.", ".to_out.0."}};
    for (auto& l : legacy) { const size_t at = nm.find(l[0]); if (at != std::string::npos) nm.replace(at, strlen(l[0]), l[1]); }
    if (nm.find(".attentions.0.to_") != std::string::npos && ndim == 4 && shape[2] == 1 && shape[3] == 1) ndim = 2;
    return dm::stage_tensor(e->w_vaed.host, nm, host_ptr, dtype, shape, ndim, e->err);
}

int dm_engine_finalize_vae_decoder(dm_engine* e) {
    if (!e) return 1;
    if (e->w_vaed.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer P{e, e->w_vaed};
    VaeDecW& v = e->vaed;
    const int C = VBOC[VNB - 1];
    {
        HostTensor* qw = P.get("post_quant_conv.weight", {4, 4, 1, 1});
        HostTensor* qb = P.get("post_quant_conv.bias", {4});
        HostTensor* w = P.get("decoder.conv_in.weight", {C, 4, 3, 3});
        if (!qw || !qb || !w) return 1;
        v.pqw = as_ptr(P.put(qw->data.data(), 16 * 2));
        v.pqb = as_ptr(P.put(qb->data.data(), 4 * 2));
        // conv_in as a 3x3 igemm over 64-channel rows: [C][tap * 64 + c], c < 4 (the latent prologue writes zeros into the other 60)
        std::vector<f16> pk((size_t)C * 9 * 64, (f16)0.f);
        for (int co = 0; co < C; ++co)
            for (int ci = 0; ci < 4; ++ci)
                for (int tap = 0; tap < 9; ++tap) pk[((size_t)co * 9 + tap) * 64 + ci] = w->data[((size_t)co * 4 + ci) * 9 + tap];
        v.conv_in.w = as_ptr(P.put(pk.data(), pk.size() * 2));
        v.conv_in.cin = 64; v.conv_in.cout = C; v.conv_in.k = 3;
        DM_TRY(pack_bias(P, "decoder.conv_in", C, &v.conv_in.b));
    }
    DM_TRY(pack_vae_resnet(P, "decoder.mid_block.resnets.0", C, C, &v.mid[0]));
    {
        const std::string a = "decoder.mid_block.attentions.0";
        DM_TRY(pack_norm(P, a + ".group_norm", C, &v.attn_gn));
        DM_TRY(pack_stack(P, {a + ".to_q", a + ".to_k", a + ".to_v"}, C, C, &v.qkv));
        std::vector<f16> qb;
        DM_TRY(stack_bias(P, {a + ".to_q", a + ".to_k", a + ".to_v"}, C, &qb));
        v.qkv.b = as_ptr(P.put(qb.data(), qb.size() * 2));
        DM_TRY(pack_dense(P, a + ".to_out.0", C, C, false, true, &v.o));
    }
    DM_TRY(pack_vae_resnet(P, "decoder.mid_block.resnets.1", C, C, &v.mid[1]));
    int cin = C;
    for (int i = 0; i < VNB; ++i) {
        const int cout = VBOC[VNB - 1 - i];
        const std::string bn = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j < 3; ++j) DM_TRY(pack_vae_resnet(P, bn + ".resnets." + std::to_string(j), j == 0 ? cin : cout, cout, &v.up[i][j]));
        if (i != VNB - 1) DM_TRY(pack_conv3(P, bn + ".upsamplers.0.conv", cout, cout, &v.us[i]));
        cin = cout;
    }
    DM_TRY(pack_norm(P, "decoder.conv_norm_out", VBOC[0], &v.norm_out));
    DM_TRY(pack_conv3(P, "decoder.conv_out", 3, VBOC[0], &v.conv_out));         // [3][tap * 128 + c]: the tail's A operand rows
    DM_TRY(P.finish("VAE decoder", 140));
    char* base = (char*)e->w_vaed.slab;
    rebase(v.pqw, base); rebase(v.pqb, base);
    rebase_conv(v.conv_in, base); rebase_conv(v.qkv, base); rebase_conv(v.o, base); rebase_conv(v.conv_out, base);
    rebase_norm(v.attn_gn, base); rebase_norm(v.norm_out, base);
    rebase_res(v.mid[0], base); rebase_res(v.mid[1], base);
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 3; ++j) rebase_res(v.up[i][j], base);
        if (i != VNB - 1) rebase_conv(v.us[i], base);
    }
    return 0;
}

int dm_engine_load_clip_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_clip.ready) DM_FAIL(e, "load_clip_weight after finalize_clip");
    std::string nm(name);
    for (const char* pre : {"text_encoder.", "text_model."}) if (nm.rfind(pre, 0) == 0) nm = nm.substr(strlen(pre));
    if (nm.size() >= 12 && nm.compare(nm.size() - 12, 12, "position_ids") == 0) return 0;          // index buffer
    return dm::stage_tensor(e->w_clip.host, nm, host_ptr, dtype, shape, ndim, e->err);
}

int dm_engine_finalize_clip(dm_engine* e) {
    if (!e) return 1;
    if (e->w_clip.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer P{e, e->w_clip};
    ClipW& c = e->clip;
    {
        HostTensor* tok = P.get("embeddings.token_embedding.weight", {CL_VOCAB, CL_H});
        HostTensor* pos = P.get("embeddings.position_embedding.weight", {CL_T, CL_H});
        if (!tok || !pos) return 1;
        c.tok = as_ptr(P.put(tok->data.data(), tok->data.size() * 2));
        c.pos = as_ptr(P.put(pos->data.data(), pos->data.size() * 2));
    }
    for (int l = 0; l < CL_LAYERS; ++l) {
        ClipLayerW& L = c.layer[l];
        const std::string b = "encoder.layers." + std::to_string(l);
        DM_TRY(pack_norm(P, b + ".layer_norm1", CL_H, &L.ln1));
        // q/k/v stacked; the attention scale d^-0.5 = 1/8 (exact in fp16) is folded into q_proj
        const std::vector<std::string> qkv = {b + ".self_attn.q_proj", b + ".self_attn.k_proj", b + ".self_attn.v_proj"};
        DM_TRY(pack_stack(P, qkv, CL_H, CL_H, &L.qkv));
        {
            std::vector<f16> qb;
            DM_TRY(stack_bias(P, qkv, CL_H, &qb));
            for (int i = 0; i < CL_H; ++i) qb[i] = (f16)((float)qb[i] * 0.125f);
            f16* w = reinterpret_cast<f16*>(P.blob.data() + (reinterpret_cast<size_t>(L.qkv.w) - 1));
            for (size_t i = 0; i < (size_t)CL_H * CL_H; ++i) w[i] = (f16)((float)w[i] * 0.125f);
            L.qkv.b = as_ptr(P.put(qb.data(), qb.size() * 2));
        }
        DM_TRY(pack_dense(P, b + ".self_attn.out_proj", CL_H, CL_H, false, true, &L.o));
        DM_TRY(pack_norm(P, b + ".layer_norm2", CL_H, &L.ln2));
        DM_TRY(pack_dense(P, b + ".mlp.fc1", CL_F, CL_H, false, true, &L.fc1));
        DM_TRY(pack_dense(P, b + ".mlp.fc2", CL_H, CL_F, false, true, &L.fc2));
    }
    DM_TRY(pack_norm(P, "final_layer_norm", CL_H, &c.final_ln));
    DM_TRY(P.finish("CLIP text", 196));
    char* base = (char*)e->w_clip.slab;
    rebase(c.tok, base); rebase(c.pos, base); rebase_norm(c.final_ln, base);
    for (int l = 0; l < CL_LAYERS; ++l) {
        ClipLayerW& L = c.layer[l];
        rebase_norm(L.ln1, base); rebase_norm(L.ln2, base);
        rebase_conv(L.qkv, base); rebase_conv(L.o, base); rebase_conv(L.fc1, base); rebase_conv(L.fc2, base);
    }
    return 0;
}

}  // extern "C"
