// engine.hip — native runtime behind include/dm_engine.h: the engine handle, its stream-ordered workspace arena, the hipGraph
// cache, the per-prompt cross-attention K/V cache, chunking, and the product's entry points.  Weight intake: engine_pack.hip;
// the schedules: engine_forward.hip; the switches: options.hip; the parity tests' operator entry points: engine_ops.hip.
#include "engine_impl.h"

#include <cstdlib>

using namespace dm;
using namespace dm::eng;
using namespace sd15;

namespace {

thread_local std::string g_create_error;

void drop_graphs(dm_engine* e) {
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
}

// Workspace for one schedule run.  The exact peak comes from a dry run of the schedule against an unbounded virtual
// arena; it depends only on `key` (which schedule, batch, shape, options), so it is computed once per key and cached:
// the steady-state path does no host walk of the schedule and — once the largest shape has been seen or reserved
// (dm_engine_reserve) — no allocation either.
template <class RunFn>
int ensure_arena_for(dm_engine* e, hipStream_t s, const std::vector<long long>& key, RunFn run_dry) {
    size_t need;
    // a switch changed since the cached peaks / captured graphs were made: not every switch is part of every key (tap_reuse and gn_epi
    // choose allocation paths too), so both caches start over — correct for any switch, and set_option is not a steady-state call
    if (e->opt_epoch != options_epoch()) {
        if (!e->graphs.empty()) { DM_HIP(e, hipStreamSynchronize(s)); drop_graphs(e); }
        e->arena_need.clear(); e->graph_seen.clear();
        e->opt_epoch = options_epoch();
    }
    auto it = e->arena_need.find(key);
    if (it != e->arena_need.end()) need = it->second;
    else {
        e->arena.reset((size_t)1 << 60, true);
        char* keep = e->arena_base;
        e->arena_base = nullptr;
        int rc = run_dry();
        e->arena_base = keep;
        if (rc) return rc;
        need = e->arena.peak;
        e->arena_need[key] = need;
        ++e->n_dry_runs;
    }
    if (need > e->arena_cap) {
        DM_HIP(e, hipStreamSynchronize(s));
        drop_graphs(e);
        if (e->arena_base) DM_HIP(e, hipFree(e->arena_base));
        e->arena_base = nullptr; e->arena_cap = 0;
        const size_t cap = need + (need >> 4);
        DM_MALLOC(e, &e->arena_base, cap);
        e->arena_cap = cap;
    }
    e->arena.reset(e->arena_cap, false);
    return 0;
}

std::vector<long long> fwd_key(const FwdArgs& A) {
    return {0, A.B, A.H, A.W, A.n_cond, A.up_ft_index, A.add_noise ? 1 : 0, A.loss ? 1 : 0, A.pred ? 1 : 0, A.feat ? 1 : 0,
            A.feat_mean ? 1 : 0, option(OPT_LN_FOLD), option(OPT_IGEMM_SPLITK), option(OPT_LN_INKERNEL), option(OPT_GN_FOLD), option(OPT_SC_FOLD), option(OPT_FF_FOLD), option(OPT_UP_FOLD), option(OPT_Q_ONCE), option(OPT_GN_EPI), option(OPT_CONV_OUT_ROWS), option(OPT_GN_SKIP)};
}

int ensure_arena(dm_engine* e, const FwdArgs& A, hipStream_t s) {
    return ensure_arena_for(e, s, fwd_key(A), [&]() { return run_forward(e, A, s, true); });
}

// K/V cache capacity: at least 16 prompts (3.8 MB per prompt over the 16 transformer blocks), doubling when it has to grow,
// so that a stream of calls with varying prompt counts stops allocating after the first few; dm_engine_reserve pre-sizes it.
int reserve_prompts(dm_engine* e, int n_prompts, hipStream_t s) {
    if (n_prompts <= e->kv_capacity) return 0;
    int cap = e->kv_capacity > 0 ? 2 * e->kv_capacity : 16;
    if (cap < n_prompts) cap = n_prompts;
    DM_HIP(e, hipStreamSynchronize(s));
    drop_graphs(e);
    for (int l = 0; l < e->n_tf; ++l) {
        if (e->kv_cache[l]) DM_HIP(e, hipFree(e->kv_cache[l]));
        e->kv_cache[l] = nullptr;
        DM_MALLOC(e, &e->kv_cache[l], (size_t)cap * CTX_LEN * 2 * e->tfs[l]->c * sizeof(f16));
    }
    e->kv_capacity = cap;
    e->n_prompts = 0;                      // the old rows are gone
    return 0;
}

// One U-Net run on the stream: straight launches, or — option "graph", no per-launch profiling — the replay of a captured
// hipGraph.  A graph bakes in every pointer, so the key is the schedule key plus all pointer arguments; the
// host-side arena allocator is deterministic, so a replay uses the same workspace addresses as the capture did.
int run_forward_graphed(dm_engine* e, const FwdArgs& A, hipStream_t s) {
    // (the legacy default stream cannot be captured: callers that want graphs run on a stream of their own)
    if (!option(OPT_GRAPH) || e->prof || s == nullptr) return run_forward(e, A, s, false);
    std::vector<long long> key = fwd_key(A);
    for (const void* q : {A.x, (const void*)A.x_index, A.eps, (const void*)A.t, (const void*)A.slots, (const void*)A.loss,
                          (const void*)A.pred, (const void*)A.feat, (const void*)A.feat_mean, (const void*)s})
        key.push_back((long long)(size_t)q);
    for (long long v : {(long long)A.latent_f32, (long long)A.out_stride, (long long)A.out_off, (long long)A.ensemble, (long long)e->n_prompts})
        key.push_back(v);
    for (int o = 0; o < OPT_COUNT; ++o) key.push_back(option((Option)o));      // a graph bakes in the kernel choice of every switch
    for (auto& g : e->graphs)
        if (g.key == key) {
            g.stamp = ++e->graph_stamp;
            ++e->n_graph_launches;
            DM_HIP(e, hipGraphLaunch(g.exec, s));
            return 0;
        }
    if (e->graph_seen.size() > 256) e->graph_seen.clear();                   // callers that never repeat a key (fresh tensors every call) must not grow this
    if (e->graph_seen[key]++ == 0) return run_forward(e, A, s, false);      // first sight: plain run (function attributes, warm caches)
    hipGraph_t graph = nullptr;
    DM_HIP(e, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = run_forward(e, A, s, false);
    const hipError_t ec = hipStreamEndCapture(s, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ec != hipSuccess || !graph) DM_FAIL(e, "hipStreamEndCapture failed: %s", hipGetErrorString(ec));
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) DM_FAIL(e, "hipGraphInstantiate failed: %s", hipGetErrorString(ei));
    if (e->graphs.size() >= 8) {                                           // keep the eight most recently used
        size_t old = 0;
        for (size_t i = 1; i < e->graphs.size(); ++i) if (e->graphs[i].stamp < e->graphs[old].stamp) old = i;
        (void)hipGraphExecDestroy(e->graphs[old].exec);
        e->graphs.erase(e->graphs.begin() + old);
    }
    e->graphs.push_back({key, exec, ++e->graph_stamp});
    ++e->n_graph_captures; ++e->n_graph_launches;
    DM_HIP(e, hipGraphLaunch(exec, s));
    return 0;
}

int max_chunk(int h, int w) {
    const long long px = (long long)h * w;
    static long long budget = -1;           // samples of 64x64 per U-Net batch (DM_CHUNK overrides)
    if (budget < 0) { const char* e = getenv("DM_CHUNK"); budget = e ? atoll(e) : 160; if (budget < 1) budget = 1; }
    long long b = (budget * 4096) / px;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* dm_version(void) { return "dm_engine 0.2 (gfx950; igemm 128x320 / persistent 256x320 x64 mfma_f32_16x16x32_f16, LDS-DMA)"; }

const char* dm_last_error(dm_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int dm_engine_create(int device, dm_engine** out) {
    if (!out) return 1;
    int n = 0;
    hipError_t r = hipGetDeviceCount(&n);
    if (r != hipSuccess || n <= 0) { g_create_error = "no HIP device available (the engine has no CPU fallback)"; return 1; }
    if (device < 0 || device >= n) { g_create_error = "bad device index"; return 1; }
    r = hipSetDevice(device);
    if (r != hipSuccess) { g_create_error = hipGetErrorString(r); return 1; }
    dm_engine* e = new dm_engine();
    e->device = device;
    *out = e;
    return 0;
}

void dm_engine_destroy(dm_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (f16* slab : {e->w_unet.slab, e->w_vae.slab, e->w_vaed.slab, e->w_clip.slab}) if (slab) (void)hipFree(slab);
    if (e->arena_base) (void)hipFree(e->arena_base);
    if (e->loop_buf) (void)hipFree(e->loop_buf);
    if (e->tile_ctr) (void)hipFree(e->tile_ctr);
    if (e->slot_scratch) (void)hipFree(e->slot_scratch);
    if (e->sin_table) (void)hipFree(e->sin_table);
    if (e->sa_tab) (void)hipFree(e->sa_tab);
    if (e->sb_tab) (void)hipFree(e->sb_tab);
    if (e->sa32_tab) (void)hipFree(e->sa32_tab);
    if (e->sb32_tab) (void)hipFree(e->sb32_tab);
    for (auto p : e->kv_cache) if (p) (void)hipFree(p);
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
    for (auto& ev : e->prof_ev) for (hipEvent_t h : ev.pairs) (void)hipEventDestroy(h);
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    delete e;
}

int dm_vae_encode(dm_engine* e, const void* image_dev, const void* noise_dev, int batch, int draws_per_image, int H, int W,
                  float scaling_factor, void* latent_f16_dev, void* latent_f32_dev, void* moments_f32_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_vae.ready) DM_FAIL(e, "dm_vae_encode: VAE weights not loaded (dm_engine_finalize_vae)");
    if (!image_dev || (!latent_f16_dev && !latent_f32_dev && !moments_f32_dev)) DM_FAIL(e, "dm_vae_encode: null argument");
    // any size >= 8: like diffusers' three Downsample2D(padding=0) stages (pad right/bottom by one, 3x3 stride 2), each stage
    // floors odd sizes, so the latent is floor(H / 8) x floor(W / 8) (cars rescaled to 256 x 341 px -> 32 x 42)
    if (batch <= 0 || H < 8 || W < 8) DM_FAIL(e, "dm_vae_encode: H and W must be >= 8");
    if (draws_per_image < 1 || (draws_per_image > 1 && !noise_dev)) DM_FAIL(e, "dm_vae_encode: draws_per_image > 1 needs the noise draws");
    const int D = draws_per_image;
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t ipx = (size_t)H * W, lpx = (size_t)(H / 8) * (W / 8);
    long long chunk = (8LL * 512 * 512) / (long long)ipx;         // workspace ~ 2.7 GB per 8 images of 512^2
    if (chunk < 1) chunk = 1;
    for (int b0 = 0; b0 < batch; b0 += (int)chunk) {
        VaeArgs A{};
        A.B = (batch - b0 < chunk) ? (batch - b0) : (int)chunk;
        A.H = H; A.W = W; A.scaling = scaling_factor; A.draws = D;
        A.image = (const f16*)image_dev + (size_t)b0 * 3 * ipx;
        A.noise = noise_dev ? (const f16*)noise_dev + (size_t)b0 * D * 4 * lpx : nullptr;
        A.latent16 = latent_f16_dev ? (f16*)latent_f16_dev + (size_t)b0 * D * 4 * lpx : nullptr;
        A.latent32 = latent_f32_dev ? (float*)latent_f32_dev + (size_t)b0 * D * 4 * lpx : nullptr;
        A.moments = moments_f32_dev ? (float*)moments_f32_dev + (size_t)b0 * 8 * lpx : nullptr;
        DM_TRY(ensure_arena_for(e, s, {1, A.B, A.H, A.W, A.draws}, [&]() { return run_vae(e, A, s, true); }));
        DM_TRY(run_vae(e, A, s, false));
    }
    return 0;
}

/* `vae.decode(latents / scaling_factor).sample` under autocast and `VaeImageProcessor.postprocess` (finetuning/cars.py:235-255 through
 * StableDiffusionPipeline.__call__): the batch in chunks by image area, nothing leaves the device in between */
int dm_vae_decode(dm_engine* e, const void* latent_f32_dev, int batch, int h, int w, float scaling_factor, void* raw_f16_out_dev,
                  void* image_u8_out_dev, void* stream) {
    if (!e) return 1;
    if (!e->w_vaed.ready) DM_FAIL(e, "dm_vae_decode: no VAE decoder weights (dm_engine_load_vae_decoder_weight / dm_engine_finalize_vae_decoder)");
    if (!latent_f32_dev || (!raw_f16_out_dev && !image_u8_out_dev)) DM_FAIL(e, "dm_vae_decode: null argument (a latent and at least one output)");
    if (batch <= 0 || h < 1 || w < 1 || h > 8192 || w > 8192) DM_FAIL(e, "dm_vae_decode: bad batch / latent size");
    if (!(scaling_factor > 0.f)) DM_FAIL(e, "dm_vae_decode: scaling_factor must be positive");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const long long area = 64LL * h * w;
    long long chunk = 4LL * 512 * 512 / area;                 // ~0.6 GB of fp16 activations per 512 x 512 image (a resnet at 512 x 512 x 256)
    chunk = chunk < 1 ? 1 : chunk;
    for (int b0 = 0; b0 < batch; b0 += (int)chunk) {
        VaeDecArgs A{};
        A.B = batch - b0 < chunk ? batch - b0 : (int)chunk; A.h = h; A.w = w; A.scaling = scaling_factor;
        A.latent = (const float*)latent_f32_dev + (size_t)b0 * 4 * h * w;
        A.raw = raw_f16_out_dev ? (f16*)raw_f16_out_dev + (size_t)b0 * 3 * area : nullptr;
        A.image = image_u8_out_dev ? (uint8_t*)image_u8_out_dev + (size_t)b0 * 3 * area : nullptr;
        DM_TRY(ensure_arena_for(e, s, {3, A.B, A.h, A.w}, [&]() { return run_vae_dec(e, A, s, true); }));
        DM_TRY(run_vae_dec(e, A, s, false));
    }
    return 0;
}

/* n_steps guided DDIM updates on the device queue (StableDiffusionPipeline.__call__'s denoising loop with a DDIMScheduler, eta = 0):
 * eps = UNet(cat([x, x]) rounded to fp16, t_i, prompt[slot]) at batch 2B — conv_in's fp32-latent path reads x through a row index, so
 * the stacked copy is never made —, then x = cfg_ddim_step(x, eps, coef_i, g) in place.  Tables uploaded and the arena sized before the
 * loop; no host synchronisation inside it. */
int dm_sample_run(dm_engine* e, void* x_f32_dev, const int64_t* t_host, const float* coef_host, const int32_t* slot_dev, int B, int h, int w,
                  int n_steps, float guidance_scale, void* stream) {
    if (!e) return 1;
    if (n_steps <= 0) DM_FAIL(e, "dm_sample_run: n_steps %d", n_steps);
    if (!x_f32_dev || !t_host || !coef_host || !slot_dev) DM_FAIL(e, "dm_sample_run: null argument");
    if (!e->finalized) DM_FAIL(e, "engine not finalized");
    if (e->n_prompts <= 0) DM_FAIL(e, "dm_engine_set_prompts must be called first");
    if (B <= 0 || h < 1 || w < 1) DM_FAIL(e, "dm_sample_run: bad batch / latent size");
    if (2LL * B > max_chunk(h, w))
        DM_FAIL(e, "dm_sample_run: 2 x %d samples over the %d of one U-Net run at %d x %d: a step's two halves share a run", B, max_chunk(h, w), h, w);
    if ((long long)n_steps * 2 * B > (1LL << 24)) DM_FAIL(e, "dm_sample_run: n_steps %d", n_steps);
    for (int i = 0; i < n_steps; ++i) if (t_host[i] < 0 || t_host[i] > 999) DM_FAIL(e, "dm_sample_run: timestep %lld out of range", (long long)t_host[i]);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const int N = 2 * B;
    const size_t n = (size_t)B * 4 * h * w;
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t off_t = up256(2 * n * sizeof(f16)), off_c = off_t + up256((size_t)n_steps * N * sizeof(int64_t)),
                 off_i = off_c + up256((size_t)n_steps * 4 * sizeof(float)), need = off_i + up256((size_t)N * sizeof(int32_t));
    // the loop buffer is shared by every loop of this engine: an earlier loop queued on `s` may still read its tables, and the blocking
    // copies run on the null stream, which a non-blocking `s` is not ordered with — so the queue drains first (once, before the loop)
    DM_HIP(e, hipStreamSynchronize(s));
    if (need > e->loop_cap) {
        drop_graphs(e);
        if (e->loop_buf) DM_HIP(e, hipFree(e->loop_buf));
        e->loop_buf = nullptr; e->loop_cap = 0;
        DM_MALLOC(e, &e->loop_buf, need);
        e->loop_cap = need;
    }
    f16* eps = (f16*)e->loop_buf;
    int64_t* t_dev = (int64_t*)(e->loop_buf + off_t);
    float* coef = (float*)(e->loop_buf + off_c);
    int32_t* xi = (int32_t*)(e->loop_buf + off_i);
    {
        std::vector<int64_t> tt((size_t)n_steps * N);
        for (int i = 0; i < n_steps; ++i) for (int b = 0; b < N; ++b) tt[(size_t)i * N + b] = t_host[i];
        std::vector<int32_t> idx((size_t)N);
        for (int b = 0; b < N; ++b) idx[(size_t)b] = b % B;           // latent_model_input = cat([latents] * 2)
        DM_HIP(e, hipMemcpy(t_dev, tt.data(), tt.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        DM_HIP(e, hipMemcpy(coef, coef_host, (size_t)n_steps * 4 * sizeof(float), hipMemcpyHostToDevice));
        DM_HIP(e, hipMemcpy(xi, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    FwdArgs A{};
    A.x = x_f32_dev; A.x_index = xi; A.t = t_dev; A.slots = slot_dev; A.latent_f32 = 1;
    A.B = N; A.H = h; A.W = w; A.add_noise = false; A.up_ft_index = -1; A.pred = eps;
    DM_TRY(ensure_arena(e, A, s));
    for (int i = 0; i < n_steps; ++i) {
        A.t = t_dev + (size_t)i * N;
        DM_TRY(ensure_arena(e, A, s));              // a map lookup: the dry run and the allocation happened before the loop
        DM_TRY(run_forward(e, A, s, false));
        DM_HIP(e, launch_cfg_ddim_step((const float*)x_f32_dev, eps, guidance_scale, coef + 4 * i, (long long)n, (float*)x_f32_dev, s));
    }
    return 0;
}

int dm_clip_encode(dm_engine* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, void* out_f16_dev, void* out_f32_dev,
                   void* stream) {
    if (!e) return 1;
    if (!e->w_clip.ready) DM_FAIL(e, "dm_clip_encode: CLIP text weights not loaded (dm_engine_finalize_clip)");
    if (!input_ids_dev || (!out_f16_dev && !out_f32_dev) || n_prompts <= 0) DM_FAIL(e, "dm_clip_encode: bad argument");
    if (seq_len != CL_T) DM_FAIL(e, "dm_clip_encode: seq_len must be %d (padding=\"max_length\")", CL_T);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const int chunk = 256;                                   // prompts per pass (workspace ~ 0.5 GB)
    for (int n0 = 0; n0 < n_prompts; n0 += chunk) {
        const int n = (n_prompts - n0 < chunk) ? (n_prompts - n0) : chunk;
        const int32_t* ids = input_ids_dev + (size_t)n0 * CL_T;
        f16* o16 = out_f16_dev ? (f16*)out_f16_dev + (size_t)n0 * CL_T * CL_H : nullptr;
        float* o32 = out_f32_dev ? (float*)out_f32_dev + (size_t)n0 * CL_T * CL_H : nullptr;
        DM_TRY(ensure_arena_for(e, s, {2, n}, [&]() { return run_clip(e, ids, n, o16, o32, s, true); }));
        DM_TRY(run_clip(e, ids, n, o16, o32, s, false));
    }
    return 0;
}

int dm_patch_embed(dm_engine* e, const void* feat_f32_dev, int C, int h, int w, const int32_t* boxes_dev, int n_patches,
                   void* out_f32_dev, void* stream) {
    if (!e) return 1;
    if (!feat_f32_dev || !boxes_dev || !out_f32_dev) DM_FAIL(e, "dm_patch_embed: null argument");
    DM_HIP(e, hipSetDevice(e->device));
    DM_HIP(e, launch_patch_embed((const float*)feat_f32_dev, C, h, w, boxes_dev, n_patches, (float*)out_f32_dev, (hipStream_t)stream));
    return 0;
}

int dm_engine_set_prompts(dm_engine* e, const void* ctx_dev, int n_prompts, void* stream) {
    if (!e || !ctx_dev || n_prompts <= 0) return 1;
    if (!e->finalized) DM_FAIL(e, "set_prompts before finalize");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    DM_TRY(reserve_prompts(e, n_prompts, s));
    e->n_prompts = n_prompts;
    const int M = n_prompts * CTX_LEN;
    for (int l = 0; l < e->n_tf; ++l) {
        const ConvW& kv = e->tfs[l]->kv2;
        IGemmParams p;
        p.X = (const f16*)ctx_dev; p.X2 = nullptr; p.Wp = kv.w; p.bias = nullptr; p.temb = nullptr; p.res = nullptr;
        p.Y = e->kv_cache[l]; p.M = M; p.Cout = kv.cout; p.Cin = CTX_DIM; p.C1 = CTX_DIM;
        p.H = 1; p.W = M; p.OH = 1; p.OW = M; p.mode = IG_DENSE; p.epi = EPI_PLAIN; p.ldy = kv.cout; p.ldres = 0; p.temb_ld = 0;
        p.tile_ctr = e->tile_ctr;
        DM_HIP(e, launch_igemm(p, s));
    }
    return 0;
}

static int run_chunked(dm_engine* e, FwdArgs A, int n_x, void* stream) {
    if (!e->finalized) DM_FAIL(e, "engine not finalized");
    if (e->n_prompts <= 0) DM_FAIL(e, "dm_engine_set_prompts must be called first");
    if (A.B <= 0 || A.H <= 0 || A.W <= 0) DM_FAIL(e, "bad shape");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int chunk = max_chunk(A.H, A.W);
    if (A.feat_mean && A.ensemble > 0) { chunk = (chunk / A.ensemble) * A.ensemble; if (chunk < A.ensemble) chunk = A.ensemble; }
    const int total = A.B;
    const size_t hw = (size_t)A.H * A.W;
    int fc = 0, fh = 0, fw = 0;
    if (A.up_ft_index >= 0) dm_dift_shape(A.H, A.W, A.up_ft_index, &fc, &fh, &fw);
    for (int b0 = 0; b0 < total; b0 += chunk) {
        FwdArgs C = A;
        C.B = (total - b0 < chunk) ? (total - b0) : chunk;
        const size_t esz = A.latent_f32 ? 4 : 2;
        if (A.x_index) C.x_index = A.x_index + b0; else C.x = (const char*)A.x + (size_t)b0 * 4 * hw * esz;
        if (A.eps) C.eps = (const char*)A.eps + (size_t)b0 * 4 * hw * esz;
        C.t = A.t + b0; C.slots = A.slots + b0;
        if (A.loss) C.loss = A.loss + (size_t)b0 * 4 * hw;
        if (A.pred) C.pred = A.pred + (size_t)b0 * 4 * hw;
        if (A.feat) C.feat = A.feat + (size_t)b0 * fc * fh * fw;
        if (A.feat_mean) C.feat_mean = A.feat_mean + (size_t)(b0 / A.ensemble) * fc * fh * fw;
        DM_TRY(ensure_arena(e, C, s));
        DM_TRY(run_forward_graphed(e, C, s));
    }
    (void)n_x;
    return 0;
}

int dm_score(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev, const int64_t* t_dev,
             const int32_t* slot_dev, int batch, int n_x, int h, int w, int latent_dtype, void* loss_out_dev, void* stream) {
    if (!e) return 1;
    if (!x_dev || !eps_dev || !t_dev || !slot_dev || !loss_out_dev) DM_FAIL(e, "dm_score: null argument");
    if (latent_dtype != DM_F16 && latent_dtype != DM_F32) DM_FAIL(e, "dm_score: latent_dtype must be DM_F16 or DM_F32");
    if (!x_index_dev && n_x != batch) DM_FAIL(e, "dm_score: x_index is NULL but n_x (%d) != batch (%d)", n_x, batch);
    FwdArgs A{};
    A.x = x_dev; A.x_index = x_index_dev; A.eps = eps_dev; A.t = t_dev; A.slots = slot_dev;
    A.latent_f32 = latent_dtype == DM_F32;
    A.B = batch; A.H = h; A.W = w; A.add_noise = true; A.up_ft_index = -1; A.loss = (float*)loss_out_dev;
    return run_chunked(e, A, n_x, stream);
}

int dm_score_conds_slots(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev, const int64_t* t_dev,
                         const int32_t* slot_table_dev, int n_cond, int n_draws, int n_x, int h, int w, int latent_dtype,
                         void* loss_out_dev, void* stream) {
    if (!e) return 1;
    if (!x_dev || !eps_dev || !t_dev || !loss_out_dev) DM_FAIL(e, "dm_score_conds: null argument");
    if (latent_dtype != DM_F16 && latent_dtype != DM_F32) DM_FAIL(e, "dm_score_conds: latent_dtype must be DM_F16 or DM_F32");
    const size_t esz = latent_dtype == DM_F32 ? 4 : 2;
    if (n_cond < 1 || n_draws < 1) DM_FAIL(e, "dm_score_conds: bad n_cond / n_draws");
    if (n_cond == 1) DM_FAIL(e, "dm_score_conds: use dm_score for n_cond == 1");
    if (!slot_table_dev && n_cond > e->n_prompts) DM_FAIL(e, "dm_score_conds: n_cond %d exceeds the %d registered prompts", n_cond, e->n_prompts);
    if (slot_table_dev && e->n_prompts < 1) DM_FAIL(e, "dm_score_conds_slots: no prompts registered");
    if (!x_index_dev && n_x != n_draws) DM_FAIL(e, "dm_score_conds: x_index is NULL but n_x (%d) != n_draws (%d)", n_x, n_draws);
    if (!e->finalized) DM_FAIL(e, "engine not finalized");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)h * w;
    int uc = max_chunk(h, w) / n_cond;
    if (uc < 1) uc = 1;
    const bool one_chunk = n_draws <= uc;
    if (slot_table_dev && !one_chunk) {       // chunk-local [n_cond][nu] tables are gathered into an engine-owned buffer
        const size_t need = (size_t)n_cond * uc * sizeof(int32_t);
        if (need > e->slot_scratch_cap) {
            DM_HIP(e, hipStreamSynchronize(s));
            drop_graphs(e);
            if (e->slot_scratch) DM_HIP(e, hipFree(e->slot_scratch));
            e->slot_scratch = nullptr; e->slot_scratch_cap = 0;
            DM_MALLOC(e, &e->slot_scratch, need);
            e->slot_scratch_cap = need;
        }
    }
    for (int u0 = 0; u0 < n_draws; u0 += uc) {
        const int nu = (n_draws - u0 < uc) ? (n_draws - u0) : uc;
        FwdArgs A{};
        A.x = x_dev; A.x_index = x_index_dev ? x_index_dev + u0 : nullptr;
        A.latent_f32 = latent_dtype == DM_F32;
        if (!x_index_dev) A.x = (const char*)x_dev + (size_t)u0 * 4 * hw * esz;
        A.eps = (const char*)eps_dev + (size_t)u0 * 4 * hw * esz; A.t = t_dev + u0; A.slots = nullptr;
        if (slot_table_dev) {
            if (one_chunk) A.slots = slot_table_dev;
            else {
                DM_HIP(e, hipMemcpy2DAsync(e->slot_scratch, (size_t)nu * sizeof(int32_t), slot_table_dev + u0, (size_t)n_draws * sizeof(int32_t),
                                           (size_t)nu * sizeof(int32_t), n_cond, hipMemcpyDeviceToDevice, s));
                A.slots = (const int32_t*)e->slot_scratch;
            }
        }
        A.B = nu * n_cond; A.H = h; A.W = w; A.n_cond = n_cond; A.out_stride = n_draws; A.out_off = u0;
        A.add_noise = true; A.up_ft_index = -1; A.loss = (float*)loss_out_dev;
        DM_TRY(ensure_arena(e, A, s));
        DM_TRY(run_forward_graphed(e, A, s));
    }
    return 0;
}

int dm_score_conds(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev, const int64_t* t_dev,
                   int n_cond, int n_draws, int n_x, int h, int w, int latent_dtype, void* loss_out_dev, void* stream) {
    return dm_score_conds_slots(e, x_dev, x_index_dev, eps_dev, t_dev, nullptr, n_cond, n_draws, n_x, h, w, latent_dtype, loss_out_dev, stream);
}

int dm_unet_forward(dm_engine* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch,
                    int h, int w, void* out_dev, void* stream) {
    if (!e) return 1;
    if (!sample_dev || !t_dev || !slot_dev || !out_dev) DM_FAIL(e, "dm_unet_forward: null argument");
    FwdArgs A{};
    A.x = sample_dev; A.t = t_dev; A.slots = slot_dev; A.B = batch; A.H = h; A.W = w;
    A.add_noise = false; A.up_ft_index = -1; A.pred = (f16*)out_dev;
    return run_chunked(e, A, batch, stream);
}

int dm_dift_shape(int h, int w, int up_ft_index, int* c_out, int* h_out, int* w_out) {
    if (up_ft_index < 0 || up_ft_index >= NB) return 1;
    // spatial sizes of the down path: s[0]=h, s[k+1]=ceil(s[k]/2)
    int sh[NB], sw[NB];
    sh[0] = h; sw[0] = w;
    for (int k = 1; k < NB; ++k) { sh[k] = (sh[k - 1] + 1) / 2; sw[k] = (sw[k - 1] + 1) / 2; }
    // up block i works at level NB-1-i and (except the last) ends with an upsampler to level NB-2-i
    const int lvl = (up_ft_index == NB - 1) ? 0 : NB - 2 - up_ft_index;
    if (c_out) *c_out = BOC[NB - 1 - up_ft_index];
    if (h_out) *h_out = sh[lvl];
    if (w_out) *w_out = sw[lvl];
    return 0;
}

int dm_dift(dm_engine* e, const void* noisy_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
            int up_ft_index, void* feat_out_dev, void* mean_out_dev, int ensemble, void* stream) {
    if (!e) return 1;
    if (!noisy_dev || !t_dev || !slot_dev) DM_FAIL(e, "dm_dift: null argument");
    if (up_ft_index < 0 || up_ft_index >= NB) DM_FAIL(e, "dm_dift: bad up_ft_index %d", up_ft_index);
    if (mean_out_dev && (ensemble <= 0 || batch % ensemble)) DM_FAIL(e, "dm_dift: batch %d not a multiple of ensemble %d", batch, ensemble);
    FwdArgs A{};
    A.x = noisy_dev; A.t = t_dev; A.slots = slot_dev; A.B = batch; A.H = h; A.W = w;
    A.add_noise = false; A.up_ft_index = up_ft_index; A.feat = (f16*)feat_out_dev; A.feat_mean = (float*)mean_out_dev;
    A.ensemble = mean_out_dev ? ensemble : 1;
    return run_chunked(e, A, batch, stream);
}

int dm_reduce_typicality(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_draws, int n_cond, int h, int w,
                         void* map_out_dev, void* scalar_out_dev, void* stream) {
    if (!e || !loss_dev) return 1;
    if (!map_out_dev) DM_FAIL(e, "dm_reduce_typicality: map_out_dev is required (scalar is derived from it)");
    DM_HIP(e, hipSetDevice(e->device));
    DM_HIP(e, launch_typicality(loss_dev, loss_is_f16, 1, n_draws, n_cond, h * w, 0, (float*)map_out_dev, (float*)scalar_out_dev, (hipStream_t)stream));
    return 0;
}

int dm_reduce_typicality_batched(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_images, int n_draws, int n_cond,
                                 int h, int w, int cond_major, void* maps_out_dev, void* scalars_out_dev, void* stream) {
    if (!e || !loss_dev) return 1;
    if (!maps_out_dev) DM_FAIL(e, "dm_reduce_typicality_batched: maps_out_dev is required (the scalars are derived from it)");
    if (n_images < 1 || n_draws < 1 || n_cond < 1 || h < 1 || w < 1) DM_FAIL(e, "dm_reduce_typicality_batched: bad shape");
    DM_HIP(e, hipSetDevice(e->device));
    DM_HIP(e, launch_typicality(loss_dev, loss_is_f16, n_images, n_draws, n_cond, h * w, cond_major ? 1 : 0, (float*)maps_out_dev,
                                (float*)scalars_out_dev, (hipStream_t)stream));
    return 0;
}

int dm_typicality_image(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_draws, int n_cond, int h, int w,
                        int img_h, int img_w, int kx, int ky, void* work_dev, void* out_dev, void* stream) {
    if (!e) return 1;
    if (!loss_dev || !work_dev || !out_dev) DM_FAIL(e, "dm_typicality_image: null argument");
    if (kx < 1 || ky < 1 || kx > img_h || ky > img_w) DM_FAIL(e, "dm_typicality_image: bad window %dx%d for %dx%d", kx, ky, img_h, img_w);
    DM_HIP(e, hipSetDevice(e->device));
    float* map = (float*)work_dev;
    float* tmp = map + (size_t)h * w;
    DM_HIP(e, launch_typicality(loss_dev, loss_is_f16, 1, n_draws, n_cond, h * w, 0, map, nullptr, (hipStream_t)stream));
    DM_HIP(e, launch_typicality_image(map, h, w, img_h, img_w, kx, ky, tmp, (float*)out_dev, (hipStream_t)stream));
    return 0;
}

// the descriptor table of a mining call, read back once: the entry points check it and size their launches from it
static int read_mine_desc(dm_engine* e, const char* who, const dm_mine_desc* desc_dev, int n_images, int kx, int ky, int need_grid,
                          std::vector<dm_mine_desc>& host, hipStream_t s) {
    host.resize((size_t)n_images);
    DM_HIP(e, hipMemcpyAsync(host.data(), desc_dev, (size_t)n_images * sizeof(dm_mine_desc), hipMemcpyDeviceToHost, s));
    DM_HIP(e, hipStreamSynchronize(s));
    for (int b = 0; b < n_images; ++b) {
        const dm_mine_desc& d = host[(size_t)b];
        if (d.H < 1 || d.W < 1 || d.map_offset < 0) DM_FAIL(e, "%s: bad descriptor %d", who, b);
        if (kx > d.H || ky > d.W) DM_FAIL(e, "%s: bad window %dx%d for %dx%d (image %d)", who, kx, ky, d.H, d.W, b);
        if ((long long)d.H * d.W > 0x7fffffffLL) DM_FAIL(e, "%s: image %d too large", who, b);
        if (need_grid && (d.n_draws < 1 || d.n_cond < 1 || d.h < 1 || d.w < 1 || d.grid_offset < 0 || d.work_offset < 0))
            DM_FAIL(e, "%s: bad descriptor %d", who, b);
    }
    return 0;
}

int dm_typicality_image_batched(dm_engine* e, const void* loss_dev, int loss_is_f16, const dm_mine_desc* desc_dev, int n_images,
                                int kx, int ky, void* work_dev, void* maps_out_dev, void* stream) {
    if (!e) return 1;
    if (!loss_dev || !desc_dev || !work_dev || !maps_out_dev) DM_FAIL(e, "dm_typicality_image_batched: null argument");
    if (n_images < 1) DM_FAIL(e, "dm_typicality_image_batched: n_images %d", n_images);
    if (kx < 1 || ky < 1) DM_FAIL(e, "dm_typicality_image_batched: bad window %dx%d", kx, ky);
    DM_HIP(e, hipSetDevice(e->device));
    std::vector<dm_mine_desc> host;
    DM_TRY(read_mine_desc(e, "dm_typicality_image_batched", desc_dev, n_images, kx, ky, 1, host, (hipStream_t)stream));
    int max_hw = 0, max_rowsum = 0, max_out = 0;
    for (const dm_mine_desc& d : host) {
        max_hw = std::max(max_hw, d.h * d.w);
        max_rowsum = std::max(max_rowsum, d.H * (d.W - ky + 1));
        max_out = std::max(max_out, (d.H - kx + 1) * (d.W - ky + 1));
    }
    DM_HIP(e, launch_typicality_image_batched(loss_dev, loss_is_f16, desc_dev, n_images, kx, ky, max_hw, max_rowsum, max_out,
                                              (float*)work_dev, (float*)maps_out_dev, (hipStream_t)stream));
    return 0;
}

int dm_mine_patches(dm_engine* e, const void* maps_dev, const void* priority_dev, const dm_mine_desc* desc_dev, int n_images, int kx,
                    int ky, int k_per_image, int ascending, int32_t* boxes_out_dev, float* d_out_dev, int32_t* count_out_dev,
                    void* stream) {
    if (!e) return 1;
    if (!maps_dev || !desc_dev || !boxes_out_dev || !d_out_dev || !count_out_dev) DM_FAIL(e, "dm_mine_patches: null argument");
    if (n_images < 1) DM_FAIL(e, "dm_mine_patches: n_images %d", n_images);
    if (kx < 1 || ky < 1) DM_FAIL(e, "dm_mine_patches: bad window %dx%d", kx, ky);
    if (k_per_image < 1 || k_per_image > DM_MINE_MAX_K) DM_FAIL(e, "dm_mine_patches: k_per_image %d outside [1, %d]", k_per_image, DM_MINE_MAX_K);
    DM_HIP(e, hipSetDevice(e->device));
    std::vector<dm_mine_desc> host;
    DM_TRY(read_mine_desc(e, "dm_mine_patches", desc_dev, n_images, kx, ky, 0, host, (hipStream_t)stream));
    DM_HIP(e, launch_mine_select((const float*)maps_dev, (const float*)priority_dev, desc_dev, n_images, kx, ky, k_per_image, ascending,
                                 boxes_out_dev, d_out_dev, count_out_dev, (hipStream_t)stream));
    return 0;
}

int dm_mine_parallel(dm_engine* e, const void* maps_dev, const dm_mine_desc* desc_dev, int n_groups, int n_sets,
                     const dm_mine_desc* group_desc_dev, int kx, int ky, int k_per_image, int ascending, const void* priority_dev,
                     void* median_out_dev, int32_t* boxes_out_dev, float* d_out_dev, float* set_d_out_dev, int32_t* count_out_dev,
                     void* stream) {
    if (!e) return 1;
    if (!maps_dev || !desc_dev || !group_desc_dev || !median_out_dev || !boxes_out_dev || !d_out_dev || !set_d_out_dev || !count_out_dev)
        DM_FAIL(e, "dm_mine_parallel: null argument");
    if (n_groups < 1) DM_FAIL(e, "dm_mine_parallel: n_groups %d", n_groups);
    if (n_sets < 1 || n_sets > DM_MINE_MAX_SETS) DM_FAIL(e, "dm_mine_parallel: n_sets %d outside [1, %d]", n_sets, DM_MINE_MAX_SETS);
    if ((long long)n_groups * n_sets > 0x7fffffffLL) DM_FAIL(e, "dm_mine_parallel: n_groups %d", n_groups);
    if (kx < 1 || ky < 1) DM_FAIL(e, "dm_mine_parallel: bad window %dx%d", kx, ky);
    if (k_per_image < 1 || k_per_image > DM_MINE_MAX_K) DM_FAIL(e, "dm_mine_parallel: k_per_image %d outside [1, %d]", k_per_image, DM_MINE_MAX_K);
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<dm_mine_desc> sets, groups;
    DM_TRY(read_mine_desc(e, "dm_mine_parallel", group_desc_dev, n_groups, kx, ky, 0, groups, s));
    DM_TRY(read_mine_desc(e, "dm_mine_parallel", desc_dev, n_groups * n_sets, kx, ky, 0, sets, s));
    int max_n = 0;
    for (int g = 0; g < n_groups; ++g) {
        const dm_mine_desc& gd = groups[(size_t)g];
        for (int c = 0; c < n_sets; ++c) {
            const dm_mine_desc& d = sets[(size_t)g * n_sets + c];
            if (d.H != gd.H || d.W != gd.W)
                DM_FAIL(e, "dm_mine_parallel: set %d of group %d is %dx%d, the group %dx%d", c, g, d.H, d.W, gd.H, gd.W);
        }
        max_n = std::max(max_n, (gd.H - kx + 1) * (gd.W - ky + 1));
    }
    DM_HIP(e, launch_median_maps((const float*)maps_dev, desc_dev, group_desc_dev, n_groups, n_sets, kx, ky, max_n, (float*)median_out_dev, s));
    DM_HIP(e, launch_mine_select((const float*)median_out_dev, (const float*)priority_dev, group_desc_dev, n_groups, kx, ky, k_per_image,
                                 ascending, boxes_out_dev, d_out_dev, count_out_dev, s));
    DM_HIP(e, launch_gather_sets((const float*)maps_dev, desc_dev, n_groups, n_sets, ky, k_per_image, boxes_out_dev, count_out_dev,
                                 set_d_out_dev, s));
    return 0;
}

int dm_normalize_map(dm_engine* e, const void* map_dev, int64_t n, int mode, void* work_dev, void* out_dev, void* out_neg_dev,
                     void* stream) {
    if (!e) return 1;
    if (!map_dev || !work_dev || !out_dev) DM_FAIL(e, "dm_normalize_map: null argument");
    if (n < 1) DM_FAIL(e, "dm_normalize_map: empty map");
    if (mode < DM_NORM_SIGNED || mode > DM_NORM_SPLIT) DM_FAIL(e, "dm_normalize_map: unknown mode %d", mode);
    if (mode == DM_NORM_SPLIT && !out_neg_dev) DM_FAIL(e, "dm_normalize_map: DM_NORM_SPLIT needs out_neg_dev");
    DM_HIP(e, hipSetDevice(e->device));
    DM_HIP(e, launch_map_normalize((const float*)map_dev, (long long)n, mode, (float*)work_dev, (float*)out_dev, (float*)out_neg_dev,
                                   (hipStream_t)stream));
    return 0;
}

int dm_prof_read_folded(dm_engine* e, double* igemm_flops_folded) {
    if (!e || !igemm_flops_folded) return 1;
    *igemm_flops_folded = e->prof_folded_last;
    return 0;
}

int dm_prof_enable(dm_engine* e, int on) {
    if (!e) return 1;
    e->prof = on != 0;
    return 0;
}

int dm_prof_read(dm_engine* e, double* igemm_ms, double* igemm_flops, int64_t* igemm_launches, double* attn_ms,
                 double* attn_flops, int64_t* attn_launches) {
    if (!e) return 1;
    DM_HIP(e, hipSetDevice(e->device));
    DM_HIP(e, hipDeviceSynchronize());
    // DM_PROF_DUMP=<file>: append one line per timed launch (kind M N K mode flops ms) for tools/prof_shapes.py
    FILE* dump = nullptr;
    if (const char* dp = getenv("DM_PROF_DUMP")) dump = fopen(dp, "a");
    for (auto& ev : e->prof_ev) {
        float ms = 0.f;
        for (size_t i = 0; i + 1 < ev.pairs.size(); i += 2) {          // a launch = the sum of its dispatches' kernel times
            float d = 0.f;
            DM_HIP(e, hipEventElapsedTime(&d, ev.pairs[i], ev.pairs[i + 1]));
            ms += d;
        }
        if (dump) fprintf(dump, "%d %d %d %d %d %.0f %.6f\n", ev.kind, ev.M, ev.N, ev.K, ev.mode, ev.flops, ms);
        e->prof_ms[ev.kind] += ms; e->prof_flops[ev.kind] += ev.flops; e->prof_n[ev.kind] += 1; e->prof_folded += ev.folded;
        for (hipEvent_t h : ev.pairs) e->ev_pool.push_back(h);
    }
    if (dump) fclose(dump);
    e->prof_ev.clear();
    if (igemm_ms) *igemm_ms = e->prof_ms[0];
    if (igemm_flops) *igemm_flops = e->prof_flops[0];
    if (igemm_launches) *igemm_launches = e->prof_n[0];
    if (attn_ms) *attn_ms = e->prof_ms[1];
    if (attn_flops) *attn_flops = e->prof_flops[1];
    if (attn_launches) *attn_launches = e->prof_n[1];
    e->prof_ms[0] = e->prof_ms[1] = 0; e->prof_flops[0] = e->prof_flops[1] = 0; e->prof_n[0] = e->prof_n[1] = 0;
    e->prof_folded_last = e->prof_folded; e->prof_folded = 0;
    return 0;
}

int dm_engine_stats(dm_engine* e, int64_t* device_allocs, int64_t* schedule_dry_runs, int64_t* graph_launches) {
    if (!e) return 1;
    if (device_allocs) *device_allocs = e->n_device_allocs;
    if (schedule_dry_runs) *schedule_dry_runs = e->n_dry_runs;
    if (graph_launches) *graph_launches = e->n_graph_launches;
    return 0;
}

int dm_engine_reserve(dm_engine* e, int max_batch, int max_h, int max_w, int n_cond, int max_prompts, void* stream) {
    if (!e) return 1;
    if (!e->finalized) DM_FAIL(e, "dm_engine_reserve before finalize");
    if (max_batch < 0 || max_h < 0 || max_w < 0 || max_prompts < 0) DM_FAIL(e, "dm_engine_reserve: negative argument");
    DM_HIP(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (max_prompts > 0) {
        const int keep = e->n_prompts;
        if (max_prompts > e->kv_capacity && keep > 0) DM_FAIL(e, "dm_engine_reserve: grow the prompt cache before dm_engine_set_prompts (its rows would be lost)");
        DM_TRY(reserve_prompts(e, max_prompts, s));
        e->n_prompts = keep;
    }
    if (max_batch > 0 && max_h > 0 && max_w > 0) {
        // the largest U-Net batch a call of that size is cut into (DM_CHUNK), full forward with the loss epilogue
        int chunk = max_chunk(max_h, max_w);
        FwdArgs A{};
        A.H = max_h; A.W = max_w; A.add_noise = true; A.up_ft_index = -1; A.loss = reinterpret_cast<float*>(1);
        if (n_cond > 1) { int uc = chunk / n_cond; if (uc < 1) uc = 1; const int nu = max_batch / n_cond < uc ? max_batch / n_cond : uc; A.n_cond = n_cond; A.B = (nu < 1 ? 1 : nu) * n_cond; }
        else A.B = max_batch < chunk ? max_batch : chunk;
        DM_TRY(ensure_arena(e, A, s));
    }
    return 0;
}

int dm_engine_memory(dm_engine* e, size_t* weights_bytes, size_t* arena_bytes) {
    if (!e) return 1;
    if (weights_bytes) *weights_bytes = e->w_unet.bytes + e->w_vae.bytes + e->w_vaed.bytes + e->w_clip.bytes;     // U-Net + optional VAE / CLIP slabs
    if (arena_bytes) *arena_bytes = e->arena_cap;
    return 0;
}

}  // extern "C"
