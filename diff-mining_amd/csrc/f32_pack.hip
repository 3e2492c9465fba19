// f32_pack.hip — the fp32 net's six state dicts (U-Net, VAE encoder, VAE decoder, CLIP text tower, CLIP ViT-B/32 and the configurable image
// tower) -> their weight slabs: the name filters of the dm_f32_load_*_weight entries, the packers, and the dm_f32_finalize_* entries
// that lay a slab out in the order its schedule reads it.
#include "f32_impl.h"

#include <cmath>

using namespace sd15;
using namespace dm::f32;

int dm::f32::pack_vec(Packer32& P, const std::string& name, int c, size_t* off) {
    HostT* t = P.get(name, {c});
    if (!t) return 1;
    *off = P.put(t->data.data(), (size_t)c);
    return 0;
}
int dm::f32::pack_conv3(Packer32& P, const std::string& name, int cout, int cin, Conv* o) {      // [cout][cin][3][3] -> [cout][(tap, cin)]
    HostT* w = P.get(name + ".weight", {cout, cin, 3, 3});
    if (!w) return 1;
    std::vector<float> pk((size_t)cout * 9 * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) pk[((size_t)co * 9 + tap) * cin + ci] = w->data[((size_t)co * cin + ci) * 9 + tap];
    o->w = P.put(pk.data(), pk.size());
    o->cin = cin; o->cout = cout; o->k = 3;
    return pack_vec(P, name + ".bias", cout, &o->b);
}
// Upsample2D.conv folded onto the source grid (f32_gemm.hip mode 5): [4 = py*2+px][cout][(a*2+b)*cin + ci], an entry = the sum (in double,
// rounded to fp32 once: <= 2^-24 relative, a thirtieth of the fp32 summation-order noise of the layer) of the 3x3 taps that read source
// pixel (y - 1 + py + a, x - 1 + px + b) for output pixel (2y + py, 2x + px); shares the bias of the packed 3x3 layer
int dm::f32::pack_upconv4(Packer32& P, const std::string& name, int cout, int cin, const Conv& full, Conv* o) {
    HostT* w = P.get(name + ".weight", {cout, cin, 3, 3});
    if (!w) return 1;
    static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};
    std::vector<float> pk((size_t)16 * cout * cin);
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int co = 0; co < cout; ++co)
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b)
                        for (int ci = 0; ci < cin; ++ci) {
                            const float* k9 = w->data.data() + ((size_t)co * cin + ci) * 9;
                            double acc = 0.0;
                            for (int dy = lo[py][a]; dy <= hi[py][a]; ++dy)
                                for (int dx = lo[px][b]; dx <= hi[px][b]; ++dx) acc += (double)k9[dy * 3 + dx];
                            pk[(((size_t)(py * 2 + px) * cout + co) * 4 + (a * 2 + b)) * cin + ci] = (float)acc;
                        }
    o->w = P.put(pk.data(), pk.size());
    o->cin = cin; o->cout = cout; o->k = 2; o->b = full.b;
    return 0;
}
int dm::f32::pack_dense(Packer32& P, const std::string& name, int cout, int cin, bool conv1x1, bool bias, Conv* o) {
    HostT* w = conv1x1 ? P.get(name + ".weight", {cout, cin, 1, 1}) : P.get(name + ".weight", {cout, cin});
    if (!w) return 1;
    o->w = P.put(w->data.data(), (size_t)cout * cin);
    o->cin = cin; o->cout = cout; o->k = 1; o->b = NONE;
    return bias ? pack_vec(P, name + ".bias", cout, &o->b) : 0;
}
int dm::f32::pack_norm(Packer32& P, const std::string& name, int c, Norm* o) {
    o->c = c;
    DM_TRY(pack_vec(P, name + ".weight", c, &o->g));
    return pack_vec(P, name + ".bias", c, &o->b);
}
int dm::f32::pack_stack(Packer32& P, const std::vector<std::string>& names, int rows_each, int cin, Conv* o) {
    std::vector<float> pk((size_t)names.size() * rows_each * cin);
    for (size_t i = 0; i < names.size(); ++i) {
        HostT* w = P.get(names[i] + ".weight", {rows_each, cin});
        if (!w) return 1;
        memcpy(pk.data() + i * (size_t)rows_each * cin, w->data.data(), (size_t)rows_each * cin * sizeof(float));
    }
    o->w = P.put(pk.data(), pk.size());
    o->cin = cin; o->cout = (int)names.size() * rows_each; o->k = 1; o->b = NONE;
    return 0;
}
// q | k | v projections stacked [3C][C] with their biases [3C]
int dm::f32::pack_qkv(Packer32& P, const std::vector<std::string>& names, int c, Conv* o) {
    DM_TRY(pack_stack(P, names, c, c, o));
    std::vector<float> qb;
    for (const std::string& n : names) {
        HostT* b = P.get(n + ".bias", {c});
        if (!b) return 1;
        qb.insert(qb.end(), b->data.begin(), b->data.end());
    }
    o->b = P.put(qb.data(), qb.size());
    return 0;
}
// GEGLU projection [2F][C] (F = 4C): rows packed in quads (h 2q, h 2q+1, g 2q, g 2q+1) so that a lane of gemm32's epilogue holds a
// value pair and its gate pair (GemmParams::epi = 1)
int dm::f32::pack_geglu(Packer32& P, const std::string& name, int c, Conv* o) {
    const int F = 4 * c;
    HostT* w = P.get(name + ".weight", {2 * F, c});
    HostT* b = P.get(name + ".bias", {2 * F});
    if (!w || !b) return 1;
    std::vector<float> pk((size_t)2 * F * c), pb((size_t)2 * F);
    for (int rho = 0; rho < 2 * F; ++rho) {
        const int q = rho >> 2, r = rho & 3;
        const int src = (r < 2) ? (2 * q + r) : (F + 2 * q + (r - 2));
        memcpy(pk.data() + (size_t)rho * c, w->data.data() + (size_t)src * c, (size_t)c * sizeof(float));
        pb[rho] = b->data[src];
    }
    o->w = P.put(pk.data(), pk.size());
    o->b = P.put(pb.data(), pb.size());
    o->cin = c; o->cout = 2 * F; o->k = 1;
    return 0;
}
int dm::f32::pack_vae_res(Packer32& P, const std::string& name, int cin, int cout, Res* r) {
    DM_TRY(pack_norm(P, name + ".norm1", cin, &r->n1));
    DM_TRY(pack_conv3(P, name + ".conv1", cout, cin, &r->c1));
    DM_TRY(pack_norm(P, name + ".norm2", cout, &r->n2));
    DM_TRY(pack_conv3(P, name + ".conv2", cout, cout, &r->c2));
    r->has_sc = cin != cout;
    if (r->has_sc) DM_TRY(pack_dense(P, name + ".conv_shortcut", cout, cin, true, true, &r->sc));
    return 0;
}
// the U-Net's ResnetBlock2D = the VAE's + a time-embedding projection, whose rows go to P.tw / P.tb and not to the blob
int dm::f32::pack_res(Packer32& P, const std::string& name, int cin, int cout, Res* r) {
    HostT* w = P.get(name + ".time_emb_proj.weight", {cout, TEMB});
    HostT* b = P.get(name + ".time_emb_proj.bias", {cout});
    if (!w || !b) return 1;
    r->temb_off = (int)P.tb.size();
    P.tw.insert(P.tw.end(), w->data.begin(), w->data.end());
    P.tb.insert(P.tb.end(), b->data.begin(), b->data.end());
    return pack_vae_res(P, name, cin, cout, r);
}
int dm::f32::pack_clip_layer(Packer32& P, const std::string& b, ClipLayer32* L, int H, int F) {       // CLIPEncoderLayer, text and image towers alike
    DM_TRY(pack_norm(P, b + ".layer_norm1", H, &L->ln1));
    DM_TRY(pack_qkv(P, {b + ".self_attn.q_proj", b + ".self_attn.k_proj", b + ".self_attn.v_proj"}, H, &L->qkv));
    DM_TRY(pack_dense(P, b + ".self_attn.out_proj", H, H, false, true, &L->o));
    DM_TRY(pack_norm(P, b + ".layer_norm2", H, &L->ln2));
    DM_TRY(pack_dense(P, b + ".mlp.fc1", F, H, false, true, &L->fc1));
    return pack_dense(P, b + ".mlp.fc2", H, F, false, true, &L->fc2);
}
int dm::f32::pack_tfm(Packer32& P, const std::string& name, int c, Tfm* t) {
    dm_f32_net* e = P.e;
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
    return 0;
}

namespace {

// conv_in runs as a direct kernel on the NCHW input: weights [cout][cin][3][3] transposed to [(ci, dy, dx)][cout]
int pack_conv_in(Packer32& P, const std::string& name, int cin, int cout, Conv* o) {
    HostT* w = P.get(name + ".weight", {cout, cin, 3, 3});
    if (!w) return 1;
    const int K = 9 * cin;
    std::vector<float> wt((size_t)K * cout);
    for (int co = 0; co < cout; ++co)
        for (int k = 0; k < K; ++k) wt[(size_t)k * cout + co] = w->data[(size_t)co * K + k];
    o->w = P.put(wt.data(), wt.size());
    o->cin = cin; o->cout = cout; o->k = 3;
    return pack_vec(P, name + ".bias", cout, &o->b);
}
int pack_vae_attn(Packer32& P, const std::string& a, int C, VaeAttn32* o) {
    DM_TRY(pack_norm(P, a + ".group_norm", C, &o->gn));
    DM_TRY(pack_qkv(P, {a + ".to_q", a + ".to_k", a + ".to_v"}, C, &o->qkv));
    return pack_dense(P, a + ".to_out.0", C, C, false, true, &o->o);
}
// A tensor of an `AutoencoderKL.state_dict()` for the half whose loader calls: `vae.` stripped, the other half's prefixes (`skip`) dropped,
// the mid-block attention under its present names (pre-0.15 diffusers: query / key / value / proj_attn, stored as 1x1 convolutions)
int stage_vae(dm_f32_net* e, dm::WeightSet<float>& set, const char* name, std::initializer_list<const char*> skip, const void* host_ptr, int dtype,
              const int64_t* shape, int ndim) {
    std::string nm(name);
    if (nm.rfind("vae.", 0) == 0) nm = nm.substr(4);
    for (const char* pre : skip) if (nm.rfind(pre, 0) == 0) return 0;
    static const char* legacy[4][2] = {{".query.", ".to_q."}, {".key.", ".to_k."}, {".value.", ".to_v."}, {".proj_attn.", ".to_out.0."}};
    for (auto& l : legacy) { const size_t at = nm.find(l[0]); if (at != std::string::npos) nm.replace(at, strlen(l[0]), l[1]); }
    if (nm.find(".attentions.0.to_") != std::string::npos && ndim == 4 && shape[2] == 1 && shape[3] == 1) ndim = 2;      // [C, C, 1, 1] -> [C, C]
    return dm::stage_tensor(set.host, nm, host_ptr, dtype, shape, ndim, e->err);
}
// A tensor of an image tower out of `CLIPVisionModelWithProjection.state_dict()` or a full `CLIPModel.state_dict()`: the text half and
// the logit scale are not on this path; position_ids is an index buffer
int stage_image_tower(dm_f32_net* e, dm::WeightSet<float>& set, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    std::string nm(name);
    if (nm.rfind("text_model.", 0) == 0 || nm == "text_projection.weight" || nm == "logit_scale") return 0;
    if (nm.size() >= 12 && nm.compare(nm.size() - 12, 12, "position_ids") == 0) return 0;
    if (nm.rfind("vision_model.", 0) == 0) nm = nm.substr(strlen("vision_model."));
    return dm::stage_tensor(set.host, nm, host_ptr, dtype, shape, ndim, e->err);
}
// The slab of an image tower with config c0 (8 + 16 layers tensors); *out is written only when everything succeeded
int pack_image_tower(dm_f32_net* e, dm::WeightSet<float>& set, const dm_clip_tower_config& c0, const char* what, ClipTower32* out) {
    DM_HIP(e, hipSetDevice(e->device));
    Packer32 P{e, set};
    ClipTower32 c;
    c.cfg = c0;
    c.G = c0.image_size / c0.patch_size; c.T = c.G * c.G + 1;
    c.KP = 3 * c0.patch_size * c0.patch_size; c.KPAD = (c.KP + 31) / 32 * 32;
    const int H = c0.hidden;
    HostT* cls = P.get("embeddings.class_embedding", {H});
    HostT* pos = P.get("embeddings.position_embedding.weight", {c.T, H});
    HostT* pw = P.get("embeddings.patch_embedding.weight", {H, 3, c0.patch_size, c0.patch_size});      // [H][(c, ky, kx)]: the patch rows' k order
    if (!cls || !pos || !pw) return 1;
    c.cls = P.put(cls->data.data(), cls->data.size());
    c.pos = P.put(pos->data.data(), pos->data.size());
    std::vector<float> pk((size_t)H * c.KPAD, 0.f);           // zero columns KP .. KPAD - 1 against the zero columns of the rows
    for (int o = 0; o < H; ++o) memcpy(pk.data() + (size_t)o * c.KPAD, pw->data.data() + (size_t)o * c.KP, (size_t)c.KP * sizeof(float));
    c.patch.w = P.put(pk.data(), pk.size());
    c.patch.cin = c.KPAD; c.patch.cout = H; c.patch.k = 1; c.patch.b = NONE;
    DM_TRY(pack_norm(P, "pre_layrnorm", H, &c.pre_ln));
    c.layer.resize(c0.layers);
    for (int l = 0; l < c0.layers; ++l) DM_TRY(pack_clip_layer(P, "encoder.layers." + std::to_string(l), &c.layer[l], H, c0.intermediate));
    DM_TRY(pack_norm(P, "post_layernorm", H, &c.post_ln));
    DM_TRY(pack_dense(P, "visual_projection", c0.projection_dim, H, false, false, &c.proj));
    DM_TRY(P.finish(what, (size_t)8 + 16 * (size_t)c0.layers));
    *out = std::move(c);
    return 0;
}
}  // namespace

extern "C" {

int dm_f32_load_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->finalized) DM_FAIL(e, "load_weight after finalize");
    return dm::stage_tensor(e->w_unet.host, name, host_ptr, dtype, shape, ndim, e->err);
}

int dm_f32_finalize(dm_f32_net* e) {
    if (!e) return 1;
    if (e->finalized) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer32 P{e, e->w_unet};
    e->n_tf = 0; e->tfs.clear();
    DM_TRY(pack_conv_in(P, "conv_in", 4, BOC[0], &e->conv_in));
    DM_TRY(pack_dense(P, "time_embedding.linear_1", TEMB, BOC[0], false, true, &e->time1));
    DM_TRY(pack_dense(P, "time_embedding.linear_2", TEMB, TEMB, false, true, &e->time2));
    int cin = BOC[0];
    for (int i = 0; i < NB; ++i) {
        DownB& d = e->down[i];
        d.attn = DOWN_ATTN[i];
        for (int j = 0; j < LAYERS; ++j) {
            const std::string b = "down_blocks." + std::to_string(i);
            DM_TRY(pack_res(P, b + ".resnets." + std::to_string(j), cin, BOC[i], &d.res[j]));
            if (d.attn) DM_TRY(pack_tfm(P, b + ".attentions." + std::to_string(j), BOC[i], &d.tf[j]));
            cin = BOC[i];
        }
        d.has_down = i != NB - 1;
        if (d.has_down) DM_TRY(pack_conv3(P, "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", BOC[i], BOC[i], &d.down));
    }
    DM_TRY(pack_res(P, "mid_block.resnets.0", BOC[NB - 1], BOC[NB - 1], &e->mid_res[0]));
    DM_TRY(pack_tfm(P, "mid_block.attentions.0", BOC[NB - 1], &e->mid_tf));
    DM_TRY(pack_res(P, "mid_block.resnets.1", BOC[NB - 1], BOC[NB - 1], &e->mid_res[1]));
    // up blocks: reversed channel list; resnet j of block i takes cat([hidden, skip]) (UNet2DConditionModel.__init__)
    int prev = BOC[NB - 1];
    for (int i = 0; i < NB; ++i) {
        UpB& u = e->up[i];
        u.attn = UP_ATTN[i];
        const int out_c = BOC[NB - 1 - i];
        const int in_c = BOC[(NB - 2 - i) < 0 ? 0 : (NB - 2 - i)];
        for (int j = 0; j < LAYERS + 1; ++j) {
            const int skip_c = (j == LAYERS) ? in_c : out_c;
            const int res_in = (j == 0) ? prev : out_c;
            const std::string b = "up_blocks." + std::to_string(i);
            DM_TRY(pack_res(P, b + ".resnets." + std::to_string(j), res_in + skip_c, out_c, &u.res[j]));
            if (u.attn) DM_TRY(pack_tfm(P, b + ".attentions." + std::to_string(j), out_c, &u.tf[j]));
        }
        u.has_up = i != NB - 1;
        if (u.has_up) {
            DM_TRY(pack_conv3(P, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_c, out_c, &u.up));
            DM_TRY(pack_upconv4(P, "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_c, out_c, u.up, &u.up4));
            u.has_up4 = true;
        }
        prev = out_c;
    }
    DM_TRY(pack_norm(P, "conv_norm_out", BOC[0], &e->norm_out));
    DM_TRY(pack_conv3(P, "conv_out", 4, BOC[0], &e->conv_out));
    e->tproj_total = (int)P.tb.size();
    e->tproj_all.w = P.put(P.tw.data(), P.tw.size());
    e->tproj_all.b = P.put(P.tb.data(), P.tb.size());
    e->tproj_all.cin = TEMB; e->tproj_all.cout = e->tproj_total; e->tproj_all.k = 1;
    DM_TRY(P.finish("U-Net", 0));
    {   // scheduler coefficients as the reference forms them (acp.to(fp32)[t] ** 0.5, (1 - acp[t]) ** 0.5)
        std::vector<float> acp(1000), tab(2000);
        if (dm_scheduler_alphas_cumprod(1000, 0.00085f, 0.012f, acp.data())) DM_FAIL(e, "scheduler table");
        for (int i = 0; i < 1000; ++i) { tab[i] = sqrtf(acp[i]); tab[1000 + i] = sqrtf(1.0f - acp[i]); }
        DM_HIP(e, hipMalloc((void**)&e->sched_tab, tab.size() * sizeof(float)));
        DM_HIP(e, hipMemcpy(e->sched_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    e->finalized = true;
    return 0;
}

int dm_f32_load_vae_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_vae.ready) DM_FAIL(e, "load_vae_weight after finalize_vae");
    return stage_vae(e, e->w_vae, name, {"decoder.", "post_quant_conv."}, host_ptr, dtype, shape, ndim);      // the decoder's half: not on the path
}

int dm_f32_finalize_vae(dm_f32_net* e) {
    if (!e) return 1;
    if (e->w_vae.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer32 P{e, e->w_vae};
    Vae32& v = e->vae;
    DM_TRY(pack_conv_in(P, "encoder.conv_in", 3, VBOC[0], &v.conv_in));
    int cin = VBOC[0];
    for (int i = 0; i < VNB; ++i) {
        const int cout = VBOC[i];
        const std::string bn = "encoder.down_blocks." + std::to_string(i);
        for (int j = 0; j < 2; ++j) DM_TRY(pack_vae_res(P, bn + ".resnets." + std::to_string(j), j == 0 ? cin : cout, cout, &v.down[i][j]));
        if (i != VNB - 1) DM_TRY(pack_conv3(P, bn + ".downsamplers.0.conv", cout, cout, &v.ds[i]));
        cin = cout;
    }
    const int C = VBOC[VNB - 1];
    DM_TRY(pack_vae_res(P, "encoder.mid_block.resnets.0", C, C, &v.mid[0]));
    DM_TRY(pack_vae_attn(P, "encoder.mid_block.attentions.0", C, &v.attn));
    DM_TRY(pack_vae_res(P, "encoder.mid_block.resnets.1", C, C, &v.mid[1]));
    DM_TRY(pack_norm(P, "encoder.conv_norm_out", C, &v.norm_out));
    DM_TRY(pack_conv3(P, "encoder.conv_out", 8, C, &v.conv_out));
    {
        HostT* qw = P.get("quant_conv.weight", {8, 8, 1, 1});
        HostT* qb = P.get("quant_conv.bias", {8});
        if (!qw || !qb) return 1;
        v.qw = P.put(qw->data.data(), 64);
        v.qb = P.put(qb->data.data(), 8);
    }
    return P.finish("VAE", 108);
}

int dm_f32_load_clip_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_clip.ready) DM_FAIL(e, "load_clip_weight after finalize_clip");
    std::string nm(name);
    for (const char* pre : {"text_encoder.", "text_model."}) if (nm.rfind(pre, 0) == 0) nm = nm.substr(strlen(pre));
    if (nm.size() >= 12 && nm.compare(nm.size() - 12, 12, "position_ids") == 0) return 0;          // index buffer
    return dm::stage_tensor(e->w_clip.host, nm, host_ptr, dtype, shape, ndim, e->err);
}

int dm_f32_finalize_clip(dm_f32_net* e) {
    if (!e) return 1;
    if (e->w_clip.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer32 P{e, e->w_clip};
    Clip32& c = e->clip;
    {
        HostT* tok = P.get("embeddings.token_embedding.weight", {CL_VOCAB, CL_H});
        HostT* pos = P.get("embeddings.position_embedding.weight", {CL_T, CL_H});
        if (!tok || !pos) return 1;
        c.tok = P.put(tok->data.data(), tok->data.size());
        c.pos = P.put(pos->data.data(), pos->data.size());
    }
    for (int l = 0; l < CL_LAYERS; ++l) DM_TRY(pack_clip_layer(P, "encoder.layers." + std::to_string(l), &c.layer[l]));
    DM_TRY(pack_norm(P, "final_layer_norm", CL_H, &c.final_ln));
    // optional 197th tensor: `CLIPTextModelWithProjection.text_projection` (no bias), for dm_f32_clip_text_embeds
    const bool proj = e->w_clip.host.count("text_projection.weight") != 0;
    if (proj) DM_TRY(pack_dense(P, "text_projection", CL_H, CL_H, false, false, &c.tproj));
    DM_TRY(P.finish("CLIP text", proj ? 197 : 196));
    c.has_tproj = proj;
    return 0;
}

int dm_f32_load_clip_vision_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_clipv.ready) DM_FAIL(e, "load_clip_vision_weight after finalize_clip_vision");
    return stage_image_tower(e, e->w_clipv, name, host_ptr, dtype, shape, ndim);
}

int dm_f32_finalize_clip_vision(dm_f32_net* e) {
    if (!e) return 1;
    if (e->w_clipv.ready) return 0;
    static_assert(CV_TENSORS == 8 + 16 * CL_LAYERS && CV_T == CV_NPATCH + 1 && CV_KP % 32 == 0, "ViT-B/32 is the tower at CV_CONFIG");
    return pack_image_tower(e, e->w_clipv, CV_CONFIG, "CLIP vision", &e->clipv);
}

int dm_f32_load_clip_tower_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_clipt.ready) DM_FAIL(e, "load_clip_tower_weight after finalize_clip_tower");
    return stage_image_tower(e, e->w_clipt, name, host_ptr, dtype, shape, ndim);
}

int dm_f32_finalize_clip_tower(dm_f32_net* e, const dm_clip_tower_config* cfg) {
    if (!e) return 1;
    if (!cfg) DM_FAIL(e, "dm_f32_finalize_clip_tower: no config");
    const dm_clip_tower_config c0 = *cfg;
    if (e->w_clipt.ready) {
        if (memcmp(&e->clipt.cfg, &c0, sizeof(c0)) != 0) DM_FAIL(e, "dm_f32_finalize_clip_tower: a tower with another config is already loaded");
        return 0;
    }
    if (c0.hidden < 64 || c0.heads < 1 || c0.hidden != c0.heads * 64) DM_FAIL(e, "CLIP tower config: hidden %d != heads %d * 64", c0.hidden, c0.heads);
    if (c0.hidden % 32 != 0 || c0.intermediate < 32 || c0.intermediate % 32 != 0)
        DM_FAIL(e, "CLIP tower config: hidden %d and intermediate %d must be multiples of 32", c0.hidden, c0.intermediate);
    if (c0.projection_dim < 4 || c0.projection_dim % 4 != 0) DM_FAIL(e, "CLIP tower config: projection_dim %d must be a multiple of 4", c0.projection_dim);
    if (c0.layers < 1 || c0.layers > 64 || c0.hidden > 8192 || c0.intermediate > 32768 || c0.projection_dim > 8192)
        DM_FAIL(e, "CLIP tower config: layers %d / widths out of range", c0.layers);
    if (c0.patch_size < 1 || c0.patch_size > 64 || c0.image_size < c0.patch_size || c0.image_size > 2048 || c0.image_size % c0.patch_size != 0)
        DM_FAIL(e, "CLIP tower config: image_size %d is not a multiple of patch_size %d (or out of range)", c0.image_size, c0.patch_size);
    return pack_image_tower(e, e->w_clipt, c0, "CLIP tower", &e->clipt);
}

int dm_f32_load_vae_decoder_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !host_ptr || !shape) return 1;
    if (e->w_vaed.ready) DM_FAIL(e, "load_vae_decoder_weight after finalize_vae_decoder");
    return stage_vae(e, e->w_vaed, name, {"encoder.", "quant_conv."}, host_ptr, dtype, shape, ndim);          // the encoder's half: not on the path
}

int dm_f32_finalize_vae_decoder(dm_f32_net* e) {
    if (!e) return 1;
    if (e->w_vaed.ready) return 0;
    DM_HIP(e, hipSetDevice(e->device));
    Packer32 P{e, e->w_vaed};
    VaeDec32& v = e->vaed;
    const int C = VBOC[VNB - 1];
    {
        HostT* qw = P.get("post_quant_conv.weight", {4, 4, 1, 1});
        HostT* qb = P.get("post_quant_conv.bias", {4});
        HostT* w = P.get("decoder.conv_in.weight", {C, 4, 3, 3});            // asked for here too: nothing is put before all three are there
        if (!qw || !qb || !w) return 1;
        v.pqw = P.put(qw->data.data(), 16);
        v.pqb = P.put(qb->data.data(), 4);
        DM_TRY(pack_conv_in(P, "decoder.conv_in", 4, C, &v.conv_in));
    }
    DM_TRY(pack_vae_res(P, "decoder.mid_block.resnets.0", C, C, &v.mid[0]));
    DM_TRY(pack_vae_attn(P, "decoder.mid_block.attentions.0", C, &v.attn));
    DM_TRY(pack_vae_res(P, "decoder.mid_block.resnets.1", C, C, &v.mid[1]));
    int cin = C;
    for (int i = 0; i < VNB; ++i) {
        const int cout = VBOC[VNB - 1 - i];
        const std::string bn = "decoder.up_blocks." + std::to_string(i);
        for (int j = 0; j < 3; ++j) DM_TRY(pack_vae_res(P, bn + ".resnets." + std::to_string(j), j == 0 ? cin : cout, cout, &v.up[i][j]));
        if (i != VNB - 1) {
            DM_TRY(pack_conv3(P, bn + ".upsamplers.0.conv", cout, cout, &v.us[i]));
            DM_TRY(pack_upconv4(P, bn + ".upsamplers.0.conv", cout, cout, v.us[i], &v.us4[i]));
        }
        cin = cout;
    }
    DM_TRY(pack_norm(P, "decoder.conv_norm_out", VBOC[0], &v.norm_out));
    DM_TRY(pack_conv3(P, "decoder.conv_out", 3, VBOC[0], &v.conv_out));
    return P.finish("VAE decoder", 140);
}

}  // extern "C"
