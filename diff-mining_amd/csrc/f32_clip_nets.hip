// f32_clip_nets.hip — the fp32 net's three CLIP towers, each a weight set of its own: the ViT-L/14 text tower, the ViT-B/32 image tower and
// the configurable image tower.  Their schedules in the operators of f32_forward.hip (one encoder layer, Fwd32::clip_layer, for all
// three), their chunked runners and the dm_f32_clip_* entry points; the glue kernels are those of f32_ops.hip and clip_vision.hip.
#include "f32_impl.h"

using namespace dm32;
using namespace sd15;
using namespace dm::f32;

// ---- CLIP text tower: token ids -> last_hidden_state, CLIPTextTransformer op by op in fp32 ---------------------------------------------
// (embeddings; 12 x [LN1 -> q|k|v -> causal attention -> out_proj + residual -> LN2 -> fc1 -> quick_gelu -> fc2 + residual]; final LN)
// out: last_hidden_state [n][77][768], or nullptr; embeds: `CLIPTextModelWithProjection.text_embeds` [n][768] (the final-LN row at the first
// maximum of the ids = the EOS token, times text_projection^T, optionally / ||.||), or nullptr
int dm::f32::run_clip32(dm_f32_net* e, const int32_t* ids, int n, float* out, float* embeds, int normalize, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_clip.slab};
    const Clip32& c = e->clip;
    const int M = n * CL_T;
    T32 x;
    DM_TRY(F.alloc(&x, 1, 1, M, CL_H));
    if (!dry) DM_HIP(e, launch_clip_embed(ids, F.P(c.tok), F.P(c.pos), M, CL_T, CL_H, CL_VOCAB, x.p, s));
    for (int l = 0; l < CL_LAYERS; ++l) DM_TRY(F.clip_layer(c.layer[l], n, CL_T, CL_H, CL_HEADS, CL_F, CLIP_ATTN_SEQ_CAUSAL, &x));
    T32 y;
    DM_TRY(F.layernorm(c.final_ln, x, &y));
    F.free(x);
    if (out && !dry) DM_HIP(e, hipMemcpyAsync(out, y.p, (size_t)M * CL_H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (embeds) {
        T32 pooled, emb;
        DM_TRY(F.alloc(&pooled, 1, 1, n, CL_H));
        if (!dry) DM_HIP(e, launch_clip_eos_gather(ids, y.p, n, CL_T, CL_H, pooled.p, s));
        DM_TRY(F.dense(c.tproj, pooled, nullptr, nullptr, &emb));
        F.free(pooled);
        if (!dry) {
            if (normalize) DM_HIP(e, launch_clip_l2norm(emb.p, n, c.tproj.cout, embeds, s));
            else DM_HIP(e, hipMemcpyAsync(embeds, emb.p, (size_t)n * c.tproj.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        F.free(emb);
    }
    F.free(y);
    return 0;
}

// ---- the configurable image tower: pixel_values (or square uint8 images) -> projected patch tokens ------------------------------------
// CLIPVisionModel op by op in fp32, then `visual_projection(post_layernorm(last_hidden_state[:, 1:, :]))` (ranking.py:66-70): patch rows
// (KPAD wide) -> patch embedding GEMM; class token + positions; pre_layrnorm; layers x [LN1 -> q|k|v -> flash attention over T tokens ->
// out_proj + residual -> LN2 -> fc1 -> quick_gelu -> fc2 + residual]; post_layernorm of rows 1..G^2 -> visual_projection
int dm::f32::run_tower32(dm_f32_net* e, const ImageArgs32& A, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_clipt.slab};
    const ClipTower32& c = e->clipt;
    const int n = A.n, G2 = c.G * c.G, H = c.cfg.hidden, M = n * c.T;
    T32 rows, pe, x, x0;
    DM_TRY(F.alloc(&rows, 1, 1, n * G2, c.KPAD));
    if (!dry) {
        if (A.pix) DM_HIP(e, launch_clip_tower_patchify(A.pix, n, c.cfg.image_size, c.cfg.patch_size, c.KPAD, rows.p, s));
        else DM_HIP(e, launch_clip_tower_preprocess(A.images, A.desc, A.tables, n, c.cfg.image_size, c.cfg.patch_size, c.KPAD, 1, rows.p, s));
    }
    DM_TRY(F.dense(c.patch, rows, nullptr, nullptr, &pe));          // the stride-PS convolution, no bias
    F.free(rows);
    DM_TRY(F.alloc(&x, 1, 1, M, H));
    if (!dry) DM_HIP(e, launch_clip_tower_tokens(pe.p, F.P(c.cls), F.P(c.pos), n, c.T, H, x.p, s));
    F.free(pe);
    DM_TRY(F.layernorm(c.pre_ln, x, &x0));
    F.free(x);
    x = x0;
    for (const ClipLayer32& L : c.layer) DM_TRY(F.clip_layer(L, n, c.T, H, c.cfg.heads, c.cfg.intermediate, CLIP_ATTN_FLASH, &x));
    if (A.hidden && !dry) DM_HIP(e, hipMemcpyAsync(A.hidden, x.p, (size_t)M * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (A.out) {
        T32 pl, emb;
        DM_TRY(F.alloc(&pl, 1, 1, n * G2, H));
        if (!dry) DM_HIP(e, launch_clip_tower_patch_ln(x.p, n, c.T, H, F.P(c.post_ln.g), F.P(c.post_ln.b), LN_EPS, pl.p, s));
        DM_TRY(F.dense(c.proj, pl, nullptr, nullptr, &emb));
        F.free(pl);
        if (!dry) DM_HIP(e, hipMemcpyAsync(A.out, emb.p, (size_t)n * G2 * c.cfg.projection_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
        F.free(emb);
    }
    F.free(x);
    return 0;
}

// ---- CLIP ViT-B/32 image tower: pixel_values (or uint8 crops) -> image embeds, CLIPVisionModelWithProjection op by op in fp32 -------------
// (patch rows -> patch embedding GEMM; class token + positions; pre_layrnorm; 12 x [LN1 -> q|k|v -> attention over 50 tokens -> out_proj
// + residual -> LN2 -> fc1 -> quick_gelu -> fc2 + residual]; CLS row -> post_layernorm -> visual_projection [-> / ||.||])
int dm::f32::run_clipvis32(dm_f32_net* e, const ImageArgs32& A, hipStream_t s, bool dry) {
    Fwd32 F{e, s, dry, e->w_clipv.slab};
    const ClipTower32& c = e->clipv;             // at CV_CONFIG
    const int n = A.n, M = n * CV_T;
    T32 rows, pe, x, x0;
    DM_TRY(F.alloc(&rows, 1, 1, n * CV_NPATCH, CV_KP));
    if (!dry) {
        if (A.pix) DM_HIP(e, launch_clip_patchify(A.pix, n, rows.p, s));
        else DM_HIP(e, launch_clip_preprocess(A.images, A.desc, A.tables, n, 1, rows.p, s));
    }
    DM_TRY(F.dense(c.patch, rows, nullptr, nullptr, &pe));          // the stride-32 convolution, no bias
    F.free(rows);
    DM_TRY(F.alloc(&x, 1, 1, M, CL_H));
    if (!dry) DM_HIP(e, launch_clip_tokens(pe.p, F.P(c.cls), F.P(c.pos), n, CL_H, x.p, s));
    F.free(pe);
    DM_TRY(F.layernorm(c.pre_ln, x, &x0));
    F.free(x);
    x = x0;
    for (const ClipLayer32& L : c.layer) DM_TRY(F.clip_layer(L, n, CV_T, CL_H, CL_HEADS, CL_F, CLIP_ATTN_SEQ, &x));
    if (A.hidden && !dry) DM_HIP(e, hipMemcpyAsync(A.hidden, x.p, (size_t)M * CL_H * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (A.out) {
        T32 cls, pooled, emb;
        DM_TRY(F.alloc(&cls, 1, 1, n, CL_H));
        if (!dry) DM_HIP(e, launch_clip_cls(x.p, n, CL_H, cls.p, s));
        DM_TRY(F.layernorm(c.post_ln, cls, &pooled));
        F.free(cls);
        DM_TRY(F.dense(c.proj, pooled, nullptr, nullptr, &emb));
        F.free(pooled);
        if (!dry) {
            if (A.normalize) DM_HIP(e, launch_clip_l2norm(emb.p, n, CV_PROJ, A.out, s));
            else DM_HIP(e, hipMemcpyAsync(A.out, emb.p, (size_t)n * CV_PROJ * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        F.free(emb);
    }
    F.free(x);
    return 0;
}

namespace {

// An image tower's call in runs of at most CV_CHUNK (ViT-B/32) or CT_CHUNK (`tower`: the configurable one) images, so that the workspace is
// bounded whatever the call's size (the fc1 output alone is 614 KB per ViT-B/32 image, 9.5 MB per L/14-336 image); rows of different images
// meet in no sum, so the split does not change a bit
int run_images_chunked32(dm_f32_net* e, bool tower, const ImageArgs32& full, void* stream, const char* what) {
    if (tower && !e->w_clipt.ready) DM_FAIL(e, "%s: CLIP tower weights not loaded (dm_f32_load_clip_tower_weight / dm_f32_finalize_clip_tower)", what);
    if (!tower && !e->w_clipv.ready) DM_FAIL(e, "%s: CLIP vision weights not loaded (dm_f32_load_clip_vision_weight / dm_f32_finalize_clip_vision)", what);
    if (full.n <= 0) DM_FAIL(e, "%s: bad image count %d", what, full.n);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const ClipTower32& c = tower ? e->clipt : e->clipv;
    const int chunk = tower ? CT_CHUNK : CV_CHUNK;
    const size_t S = (size_t)c.cfg.image_size, per_out = tower ? (size_t)c.G * c.G * c.cfg.projection_dim : (size_t)CV_PROJ;
    for (int n0 = 0; n0 < full.n; n0 += chunk) {
        ImageArgs32 C = full;
        C.n = (full.n - n0 < chunk) ? full.n - n0 : chunk;
        C.pix = at(full.pix, n0, 3 * S * S);
        C.desc = at(full.desc, n0);
        C.out = at(full.out, n0, per_out);
        C.hidden = at(full.hidden, n0, (size_t)c.T * c.cfg.hidden);
        DM_TRY(run_sized32(e, s, {tower ? KEY_CLIP_TOWER : KEY_CLIP_VISION, C.n, C.pix ? 1 : 0, C.hidden ? 1 : 0, C.out ? 1 : 0},
                           [&](bool dry) { return tower ? run_tower32(e, C, s, dry) : run_clipvis32(e, C, s, dry); }));
    }
    return 0;
}

// the text tower in runs of at most CLIP_TEXT_CHUNK prompts: last_hidden_state [n][77][768] (out) or text_embeds [n][768] (embeds)
int run_clip_chunked32(dm_f32_net* e, const int32_t* ids, int n_prompts, float* out, float* embeds, int normalize, void* stream) {
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    for (int n0 = 0; n0 < n_prompts; n0 += CLIP_TEXT_CHUNK) {
        const int n = (n_prompts - n0 < CLIP_TEXT_CHUNK) ? (n_prompts - n0) : CLIP_TEXT_CHUNK;
        DM_TRY(run_sized32(e, s, {KEY_CLIP_TEXT, n, embeds ? 1 : 0, 0, 0}, [&](bool dry) {
            return run_clip32(e, at(ids, n0, CL_T), n, at(out, n0, (size_t)CL_T * CL_H), at(embeds, n0, CL_H), normalize, s, dry); }));
    }
    return 0;
}

}  // namespace

extern "C" {

/* `text_encoder(input_ids)[0]` in fp32 — what `pipe.encode_prompt` of the featuriser's fp32 pipeline returns (dift.py:222-226):
 * input_ids_dev [n_prompts, 77] int32 (tokenizer output, padding="max_length"); out_f32_dev [n_prompts, 77, 768] fp32 */
int dm_f32_clip_encode(dm_f32_net* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_clip.ready) DM_FAIL(e, "dm_f32_clip_encode: CLIP text weights not loaded (dm_f32_load_clip_weight / dm_f32_finalize_clip)");
    if (!input_ids_dev || !out_f32_dev || n_prompts <= 0) DM_FAIL(e, "dm_f32_clip_encode: bad argument");
    if (seq_len != CL_T) DM_FAIL(e, "dm_f32_clip_encode: seq_len must be %d (padding=\"max_length\")", CL_T);
    return run_clip_chunked32(e, input_ids_dev, n_prompts, (float*)out_f32_dev, nullptr, 0, stream);
}

int dm_f32_clip_preprocess(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                           int n_patches, void* out_pixel_values_dev, void* stream) {
    if (!e) return 1;
    if (!images_u8_dev || !descs_dev || !tables_dev || !out_pixel_values_dev || n_patches <= 0) DM_FAIL(e, "dm_f32_clip_preprocess: bad argument");
    DM_HIP(e, hipSetDevice(e->device));
    for (int n0 = 0; n0 < n_patches; n0 += 65535) {
        const int n = (n_patches - n0 < 65535) ? n_patches - n0 : 65535;
        DM_HIP(e, launch_clip_preprocess((const uint8_t*)images_u8_dev, descs_dev + n0, tables_dev, n, 0,
                                        (float*)out_pixel_values_dev + (size_t)n0 * CV_KP * CV_NPATCH, (hipStream_t)stream));
    }
    return 0;
}

int dm_f32_clip_image_features(dm_f32_net* e, const void* pixel_values_dev, int n, int normalize, void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!pixel_values_dev || !out_f32_dev) DM_FAIL(e, "dm_f32_clip_image_features: bad argument");
    ImageArgs32 A;
    A.pix = (const float*)pixel_values_dev; A.n = n; A.normalize = normalize != 0; A.out = (float*)out_f32_dev;
    return run_images_chunked32(e, false, A, stream, "dm_f32_clip_image_features");
}

int dm_f32_clip_vision_hidden(dm_f32_net* e, const void* pixel_values_dev, int n, void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!pixel_values_dev || !out_f32_dev) DM_FAIL(e, "dm_f32_clip_vision_hidden: bad argument");
    ImageArgs32 A;
    A.pix = (const float*)pixel_values_dev; A.n = n; A.hidden = (float*)out_f32_dev;
    return run_images_chunked32(e, false, A, stream, "dm_f32_clip_vision_hidden");
}

int dm_f32_clip_patch_features(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                               int n_patches, int normalize, void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!images_u8_dev || !descs_dev || !tables_dev || !out_f32_dev) DM_FAIL(e, "dm_f32_clip_patch_features: bad argument");
    ImageArgs32 A;
    A.images = (const uint8_t*)images_u8_dev; A.desc = descs_dev; A.tables = tables_dev;
    A.n = n_patches; A.normalize = normalize != 0; A.out = (float*)out_f32_dev;
    return run_images_chunked32(e, false, A, stream, "dm_f32_clip_patch_features");
}

/* `CLIPTextModelWithProjection(input_ids).text_embeds` in fp32 (ranking.py:58-64): the text tower, the final-LN row at the first position of the
 * largest id (`argmax(input_ids)`: the EOS token, which both of transformers' pooling rules pick), text_projection, optionally / ||.||.
 * input_ids_dev [n, 77] int32; out_f32_dev [n, 768].  The reference pads with padding=True and the engine takes 77 ids: the tower is causal,
 * so the EOS row does not see what follows it. */
int dm_f32_clip_text_embeds(dm_f32_net* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, int normalize, void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_clip.ready) DM_FAIL(e, "dm_f32_clip_text_embeds: CLIP text weights not loaded (dm_f32_load_clip_weight / dm_f32_finalize_clip)");
    if (!e->clip.has_tproj) DM_FAIL(e, "dm_f32_clip_text_embeds: the CLIP text weights were loaded without text_projection.weight");
    if (!input_ids_dev || !out_f32_dev || n_prompts <= 0) DM_FAIL(e, "dm_f32_clip_text_embeds: bad argument");
    if (seq_len != CL_T) DM_FAIL(e, "dm_f32_clip_text_embeds: seq_len must be %d", CL_T);
    return run_clip_chunked32(e, input_ids_dev, n_prompts, nullptr, (float*)out_f32_dev, normalize != 0, stream);
}

/* The tower's processor on square uint8 images, bit-equal to `CLIPImageProcessor(size={"shortest_edge": S}, do_center_crop=False)` (PIL
 * backend): layout 0 -> pixel_values [n][3][S][S]; layout 1 -> the patch rows of the embedding GEMM [n*G^2][KPAD] (KPAD = 3 PS^2 rounded up to
 * 32; the padding columns are written as zeros).  Descriptors as dm_f32_clip_preprocess, crop = the whole image, left = top = 0. */
int dm_f32_clip_tower_preprocess(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev, int n,
                                 int layout, void* out_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_clipt.ready) DM_FAIL(e, "dm_f32_clip_tower_preprocess: CLIP tower weights not loaded (the config names the image and patch size)");
    if (!images_u8_dev || !descs_dev || !tables_dev || !out_dev || n <= 0 || (layout != 0 && layout != 1)) DM_FAIL(e, "dm_f32_clip_tower_preprocess: bad argument");
    DM_HIP(e, hipSetDevice(e->device));
    const ClipTower32& c = e->clipt;
    const size_t per = layout == 0 ? (size_t)3 * c.cfg.image_size * c.cfg.image_size : (size_t)c.G * c.G * c.KPAD;
    for (int n0 = 0; n0 < n; n0 += 65535) {
        const int m = (n - n0 < 65535) ? n - n0 : 65535;
        DM_HIP(e, launch_clip_tower_preprocess((const uint8_t*)images_u8_dev, descs_dev + n0, tables_dev, m, c.cfg.image_size, c.cfg.patch_size, c.KPAD,
                                              layout, (float*)out_dev + (size_t)n0 * per, (hipStream_t)stream));
    }
    return 0;
}

/* pixel_values_dev [n][3][S][S] -> out_tokens_dev [n][G^2][projection_dim] = visual_projection(post_layernorm(last_hidden_state[:, 1:, :])) and /
 * or out_hidden_dev [n][G^2+1][hidden] = last_hidden_state (either may be NULL, not both) */
int dm_f32_clip_tower_tokens(dm_f32_net* e, const void* pixel_values_dev, int n, void* out_tokens_dev, void* out_hidden_dev, void* stream) {
    if (!e) return 1;
    if (!pixel_values_dev || (!out_tokens_dev && !out_hidden_dev)) DM_FAIL(e, "dm_f32_clip_tower_tokens: bad argument");
    ImageArgs32 A;
    A.pix = (const float*)pixel_values_dev; A.n = n; A.out = (float*)out_tokens_dev; A.hidden = (float*)out_hidden_dev;
    return run_images_chunked32(e, true, A, stream, "dm_f32_clip_tower_tokens");
}

/* dm_f32_clip_tower_preprocess + dm_f32_clip_tower_tokens in one call: the preprocessing writes the patch rows; bit-equal to the two calls */
int dm_f32_clip_tower_image_tokens(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev, int n,
                                   void* out_tokens_dev, void* stream) {
    if (!e) return 1;
    if (!images_u8_dev || !descs_dev || !tables_dev || !out_tokens_dev) DM_FAIL(e, "dm_f32_clip_tower_image_tokens: bad argument");
    ImageArgs32 A;
    A.images = (const uint8_t*)images_u8_dev; A.desc = descs_dev; A.tables = tables_dev; A.n = n; A.out = (float*)out_tokens_dev;
    return run_images_chunked32(e, true, A, stream, "dm_f32_clip_tower_image_tokens");
}

}  // extern "C"
