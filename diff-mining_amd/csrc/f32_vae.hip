// f32_vae.hip — the SDv1.5 AutoencoderKL's two halves on the fp32 net, each a weight set of its own: their schedules in the operators of
// f32_forward.hip, and the chunked entry points dm_f32_vae_encode / dm_f32_vae_decode.
#include "f32_impl.h"

using namespace dm32;
using namespace sd15;
using namespace dm::f32;

// the mid block of either half (resnet, one-head attention over the 512 channels, resnet): *cur replaced by its output
static int vae_mid32(Fwd32& F, const Res (&mid)[2], const VaeAttn32& att, T32* cur) {
    T32 m0, n, qkv, a, m1, m2;
    DM_TRY(F.resnet(mid[0], *cur, nullptr, nullptr, &m0));
    F.free(*cur);
    const int C = VBOC[VNB - 1], T = m0.H * m0.W;
    DM_TRY(F.groupnorm(att.gn, m0, nullptr, VAE_EPS, false, &n));
    DM_TRY(F.dense(att.qkv, n, nullptr, nullptr, &qkv));
    F.free(n);
    DM_TRY(F.alloc(&a, m0.N, m0.H, m0.W, C));
    if (!F.dry) DM_TRY(F.attention(qkv.p, 3 * C, (long long)T * 3 * C, qkv.p + C, qkv.p + 2 * C, 3 * C, (long long)T * 3 * C, nullptr,
                                   m0.N, T, T, C, a.p, 1));
    F.free(qkv);
    DM_TRY(F.dense(att.o, a, nullptr, &m0, &m1));
    F.free(a); F.free(m0);
    DM_TRY(F.resnet(mid[1], m1, nullptr, nullptr, &m2));
    F.free(m1);
    *cur = m2;
    return 0;
}

// ---- VAE encoder: image -> moments -> latent (dift.py:187: `pipe.vae.encode(img).latent_dist.sample() * scaling_factor`, fp32) ----
int dm::f32::run_vae32(dm_f32_net* e, const VaeArgs32& A, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_vae.slab};
    F.res_eps = VAE_EPS;
    const Vae32& v = e->vae;
    T32 cur;
    DM_TRY(F.alloc(&cur, A.B, A.H, A.W, VBOC[0]));
    if (!dry) DM_HIP(e, launch_conv_in(A.image, F.P(v.conv_in.w), F.P(v.conv_in.b), A.B, 3, A.H, A.W, VBOC[0], cur.p, s));
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 2; ++j) {
            T32 r;
            DM_TRY(F.resnet(v.down[i][j], cur, nullptr, nullptr, &r));
            F.free(cur);
            cur = r;
        }
        if (i != VNB - 1) {      // Downsample2D(padding=0): F.pad(x, (0,1,0,1)) + conv3x3 stride 2
            T32 dn;
            DM_TRY(F.gemm(v.ds[i], 4, cur, nullptr, cur.H / 2, cur.W / 2, nullptr, 0, nullptr, &dn));
            F.free(cur);
            cur = dn;
        }
    }
    DM_TRY(vae_mid32(F, v.mid, v.attn, &cur));
    T32 nrm, co;
    DM_TRY(F.groupnorm(v.norm_out, cur, nullptr, VAE_EPS, true, &nrm));
    F.free(cur);
    DM_TRY(F.gemm(v.conv_out, 1, nrm, nullptr, nrm.H, nrm.W, nullptr, 0, nullptr, &co));
    F.free(nrm);
    if (!dry) DM_HIP(e, launch_posterior(co.p, F.P(v.qw), F.P(v.qb), A.noise, A.B, A.draws, co.H * co.W, A.scaling, A.latent, A.moments, s));
    F.free(co);
    return 0;
}

// ---- VAE decoder: latent -> image (pnp.py:137-142 / :531-536: `vae.decode(1 / 0.18215 * latents).sample`, `(imgs / 2 + 0.5).clamp(0, 1)`, fp32) ----
// post_quant_conv; conv_in 4 -> 512; mid block (resnet, one-head attention, resnet); four up blocks of three resnets (512, 512, 256, 128),
// blocks 0-2 followed by nearest-2x + conv3x3; conv_norm_out + SiLU + conv_out 128 -> 3 and the post-processing in one kernel (pnp.hip)
int dm::f32::run_vae_dec32(dm_f32_net* e, const VaeDecArgs32& A, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_vaed.slab};
    F.res_eps = VAE_EPS;
    const VaeDec32& v = e->vaed;
    const int C = VBOC[VNB - 1];
    T32 z, cur;
    DM_TRY(F.alloc(&z, A.B, 1, 1, 4 * A.h * A.w));
    if (!dry) DM_HIP(e, launch_decoder_head(A.latent, F.P(v.pqw), F.P(v.pqb), A.B, A.h * A.w, A.scale, z.p, s));
    DM_TRY(F.alloc(&cur, A.B, A.h, A.w, C));
    if (!dry) DM_HIP(e, launch_conv_in(z.p, F.P(v.conv_in.w), F.P(v.conv_in.b), A.B, 4, A.h, A.w, C, cur.p, s));
    F.free(z);
    DM_TRY(vae_mid32(F, v.mid, v.attn, &cur));
    for (int i = 0; i < VNB; ++i) {
        for (int j = 0; j < 3; ++j) {
            T32 r;
            DM_TRY(F.resnet(v.up[i][j], cur, nullptr, nullptr, &r));
            F.free(cur);
            cur = r;
        }
        if (i != VNB - 1) {
            T32 upc;
            if (dm::option(dm::OPT_UP_FOLD)) DM_TRY(F.upconv4(v.us4[i], cur, &upc));
            else DM_TRY(F.gemm(v.us[i], 3, cur, nullptr, 2 * cur.H, 2 * cur.W, nullptr, 0, nullptr, &upc));
            F.free(cur);
            cur = upc;
        }
    }
    T32 st;
    DM_TRY(F.alloc(&st, 1, 1, cur.N * GROUPS, 2));
    if (!dry) {
        DM_HIP(e, launch_gn_stats(cur.p, nullptr, cur.N, cur.H * cur.W, cur.C, cur.C, GROUPS, VAE_EPS, st.p, s));
        DM_HIP(e, launch_decoder_tail(cur.p, st.p, F.P(v.norm_out.g), F.P(v.norm_out.b), F.P(v.conv_out.w), F.P(v.conv_out.b), cur.N, cur.H, cur.W, cur.C,
                                      A.raw, A.out_f32, A.out_u8, s));
    }
    F.free(st);
    F.free(cur);
    return 0;
}

extern "C" {

/* `vae.encode(image).latent_dist.sample() * scaling_factor` in fp32 (dift.py:187; the featuriser's pipeline is fp32, dift.py:197-199):
 * image_dev [batch,3,H,W] fp32 in [-1,1]; noise_dev [batch*draws,4,H/8,W/8] fp32 N(0,1) draws or NULL (posterior mode);
 * latent_dev [batch*draws,4,H/8,W/8] fp32 and / or moments_dev [batch,8,H/8,W/8] fp32 */
int dm_f32_vae_encode(dm_f32_net* e, const void* image_dev, const void* noise_dev, int batch, int draws_per_image, int H, int W,
                      float scaling_factor, void* latent_dev, void* moments_dev, void* stream) {
    if (!e || !image_dev || (!latent_dev && !moments_dev)) return 1;
    if (!e->w_vae.ready) DM_FAIL(e, "no VAE weights (dm_f32_load_vae_weight / dm_f32_finalize_vae)");
    if (batch <= 0 || H < 8 || W < 8 || draws_per_image < 1) DM_FAIL(e, "bad batch / image size");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const int h = H / 8, w = W / 8;
    const long long area = (long long)H * W;
    long long chunk = 8LL * 512 * 512 / area;                 // ~0.6 GB of fp32 activations per 512 x 512 image
    chunk = chunk < 1 ? 1 : chunk;
    for (int b0 = 0; b0 < batch; b0 += (int)chunk) {
        VaeArgs32 A;
        A.B = batch - b0 < chunk ? batch - b0 : (int)chunk; A.draws = draws_per_image; A.H = H; A.W = W; A.scaling = scaling_factor;
        A.image = at((const float*)image_dev, b0, (size_t)3 * H * W);
        A.noise = at((const float*)noise_dev, b0, (size_t)draws_per_image * 4 * h * w);
        A.latent = at((float*)latent_dev, b0, (size_t)draws_per_image * 4 * h * w);
        A.moments = at((float*)moments_dev, b0, (size_t)8 * h * w);
        DM_TRY(run_sized32(e, s, {KEY_VAE, A.B, A.H, A.W, 0}, [&](bool dry) { return run_vae32(e, A, s, dry); }));
    }
    return 0;
}

/* `vae.decode(latent * latent_scale).sample` in fp32 and the reference's post-processing (pnp.py:137-142, :531-536, :590-591) */
int dm_f32_vae_decode(dm_f32_net* e, const void* latent_dev, int batch, int h, int w, float latent_scale, int raw, void* out_f32_dev,
                      void* out_u8_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_vaed.ready) DM_FAIL(e, "dm_f32_vae_decode: no VAE decoder weights (dm_f32_load_vae_decoder_weight / dm_f32_finalize_vae_decoder)");
    if (!latent_dev || (!out_f32_dev && !out_u8_dev)) DM_FAIL(e, "dm_f32_vae_decode: bad argument");
    if (batch <= 0 || h < 1 || w < 1 || h > 8192 || w > 8192) DM_FAIL(e, "dm_f32_vae_decode: bad batch / latent size");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const long long area = 64LL * h * w;
    long long chunk = 2LL * 512 * 512 / area;                 // ~1.2 GB of fp32 activations per 512 x 512 image (four live [512,512,256] tensors in a resnet)
    chunk = chunk < 1 ? 1 : chunk;
    for (int b0 = 0; b0 < batch; b0 += (int)chunk) {
        VaeDecArgs32 A;
        A.B = batch - b0 < chunk ? batch - b0 : (int)chunk; A.h = h; A.w = w; A.scale = latent_scale; A.raw = raw != 0;
        A.latent = at((const float*)latent_dev, b0, (size_t)4 * h * w);
        A.out_f32 = at((float*)out_f32_dev, b0, (size_t)3 * area);
        A.out_u8 = at((uint8_t*)out_u8_dev, b0, (size_t)3 * area);
        DM_TRY(run_sized32(e, s, {KEY_VAE_DEC, A.B, A.h, A.w, dm::option(dm::OPT_UP_FOLD) ? 1 : 0}, [&](bool dry) { return run_vae_dec32(e, A, s, dry); }));
    }
    return 0;
}

}  // extern "C"
