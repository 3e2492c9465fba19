/*
 * dm_engine.h — C ABI of the MI355X typicality-scoring engine (libdm_engine.so).
 *
 * This is the drop-in boundary for diff-mining's hot path.  The reference has no FFI of its own:
 * its seam is the Python attribute `self.model.unet` / `self.pipe.unet` (a diffusers
 * `UNet2DConditionModel`), driven from
 *     diffmining/typicality/compute.py:95-102   SD.compute_loss   (add_noise -> unet -> mse_loss)
 *     diffmining/typicality/compute.py:134-160  D.compute_losses  ([N,2,4,h,w] fp16 grid)
 *     diffmining/typicality/dift.py:24-169      MyUNet2DConditionModel.forward (up_ft tap)
 *     diffmining/typicality/dift.py:214-232     SDFeaturizer.forward (ensemble mean)
 * Each entry point below names the reference call it replaces.  Signatures use plain pointers and
 * sizes only (no torch types); the Python shim in diff-mining_amd/engine.py binds them with ctypes
 * and INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, nonzero on failure; dm_last_error() gives the message.
 *   - *_dev pointers are device (HBM) addresses owned by the caller; `stream` is a hipStream_t
 *     (NULL = default stream).  Calls are asynchronous on that stream.
 *   - tensors at the boundary are NCHW like the reference; the engine is NHWC fp16 inside.
 *   - one engine per device, not re-entrant (the reference is single-stream, compute.py:215).
 */
#ifndef DM_ENGINE_H
#define DM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dm_engine dm_engine;

enum { DM_F16 = 0, DM_F32 = 1 };

/* Library version / build info string (host only; usable without a GPU). */
const char* dm_version(void);

/* Host-only helpers, callable without a GPU (used by the CPU test tier).
 * dm_scheduler_alphas_cumprod: the `scaled_linear` ᾱ table of the SDv1.5 scheduler whose
 *   `add_noise` the reference calls at compute.py:99 / dift.py:190.  out[n] fp32.
 * dm_timestep_sinusoid: diffusers `Timesteps(320, flip_sin_to_cos=True, shift=0)` row for
 *   integer t (dift.py:84), out[dim] fp32 = [cos | sin]. */
int dm_scheduler_alphas_cumprod(int num_train_timesteps, float beta_start, float beta_end, float* out);
int dm_timestep_sinusoid(int t, int dim, float* out);

/* Create an engine for the SDv1.5 U-Net architecture on HIP device `device`.
 * Replaces: StableDiffusionPipeline.from_pretrained(...).unet (compute.py:65-73). */
int dm_engine_create(int device, dm_engine** out);
void dm_engine_destroy(dm_engine* e);
const char* dm_last_error(dm_engine* e);   /* e may be NULL: last create() error */

/* Hand one diffusers-named tensor (e.g. "down_blocks.0.resnets.0.conv1.weight") to the engine.
 * `host_ptr` is host memory in the PyTorch layout ([Cout,Cin,kh,kw] / [out,in] / [C]);
 * dtype is DM_F16 or DM_F32 (values are rounded to fp16: the reference loads the pipeline with
 * torch_dtype=float16, compute.py:69).  Replaces: from_pretrained's state-dict load. */
int dm_engine_load_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype,
                          const int64_t* shape, int ndim);

/* Check that all 686 tensors arrived, pack them into the MFMA-friendly HBM layout, upload. */
int dm_engine_finalize(dm_engine* e);

/* Register the distinct prompt embeddings of the next calls and precompute the cross-attention
 * K/V of all 16 transformer blocks for them (K/V depend only on the prompt, not on (t, eps)).
 * ctx_dev: [n_prompts, 77, 768] fp16.  Replaces: the `c` argument of compute_loss
 * (compute.py:96,100) / `encoder_hidden_states` (dift.py:191), which the reference re-projects
 * for every sample. */
int dm_engine_set_prompts(dm_engine* e, const void* ctx_dev, int n_prompts, void* stream);

/* SD.compute_loss (compute.py:95-102), fused: noisy = add_noise(x[x_index[b]], eps[b], t[b]);
 * eps_hat = UNet(noisy, t, prompt[slot[b]]); loss = (float(eps_hat) - float(eps))^2.
 *   latent_dtype DM_F32 or DM_F16: the element type of x_dev / eps_dev AND the arithmetic of add_noise.
 *     DM_F32 is what the reference's run does: `encode_vae` returns an fp32 latent under autocast (the
 *     posterior's exp() is promoted, compute.py:91-93), so `randn_like(x)` (:116), the scheduler's
 *     sqrt(acp[t]) / sqrt(1-acp[t]) coefficients and the sum (:99) are fp32, autocast rounds the noisy latent
 *     to fp16 once at conv_in, and mse_loss (:101) sees the fp32 eps.
 *     DM_F16 is the flow of an fp16 latent: table cast to fp16 first, fp16 products and sum, fp16 eps in the loss.
 *   x_dev        [n_x,4,h,w] (n_x images; the reference broadcasts one x over 2B rows)
 *   x_index_dev  [batch] int32 row of x for sample b, or NULL for identity (n_x == batch)
 *   eps_dev      [batch,4,h,w]
 *   t_dev        [batch] int64 in [0,1000)
 *   slot_dev     [batch] int32 prompt slot in [0, n_prompts) (see dm_engine_set_prompts)
 *   loss_out_dev [batch,4,h,w] fp32 (NCHW, as F.mse_loss(reduction='none') returns)
 */
int dm_score(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev,
             const int64_t* t_dev, const int32_t* slot_dev, int batch, int n_x, int h, int w, int latent_dtype,
             void* loss_out_dev, void* stream);

/* The same, for the way D.compute_losses actually calls it (compute.py:145-155): every one of
 * n_draws (x, eps, t) draws is scored under the n_cond prompts registered in slots 0..n_cond-1.
 * The part of the U-Net that cannot see the prompt (conv_in, down_blocks.0.resnets.0 and its
 * transformer up to the self-attention residual) is evaluated once per draw instead of once per
 * (draw, prompt) pair; results are bit-identical to dm_score on the tiled batch.
 *   x_index_dev [n_draws] or NULL; eps_dev [n_draws,4,h,w]; t_dev [n_draws]
 *   loss_out_dev [n_cond * n_draws, 4, h, w] fp32, cond-major: row k*n_draws + i = draw i, prompt k
 *   (exactly the layout `torch.split(loss, [B]*n_cond)` expects at compute.py:155). */
int dm_score_conds(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev,
                   const int64_t* t_dev, int n_cond, int n_draws, int n_x, int h, int w, int latent_dtype,
                   void* loss_out_dev, void* stream);

/* dm_score_conds with a prompt-slot TABLE: slot_table_dev [n_cond][n_draws] int32, entry (k, i) = the registered prompt that
 * draw i is scored under in its k-th condition.  This is the batched form of the reference's work list (compute.py:284-290: one
 * `path,category` line per image, D.compute(country, path) scores each image under ITS OWN category and the shared null prompt,
 * :182-192): the draws of several images ride in one call, image j's draws carry (slot of category_j, slot of "") — the
 * prompt-independent prefix still runs once per draw, and every draw's bits equal those of a per-image dm_score_conds call.
 * slot_table_dev == NULL is dm_score_conds (prompt k for every draw).  Entries are clamped to the registered prompts on the device. */
int dm_score_conds_slots(dm_engine* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev,
                         const int64_t* t_dev, const int32_t* slot_table_dev, int n_cond, int n_draws, int n_x, int h, int w,
                         int latent_dtype, void* loss_out_dev, void* stream);

/* `unet(sample, t, encoder_hidden_states).sample` (compute.py:100) without the fused
 * add_noise / loss: sample_dev [batch,4,h,w] fp16 -> out_dev [batch,4,h,w] fp16 (NCHW). */
int dm_unet_forward(dm_engine* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev,
                    int batch, int h, int w, void* out_dev, void* stream);

/* MyUNet2DConditionModel.forward(latents_noisy, t, [up_ft_index], prompt_embeds) (dift.py:24-169):
 * early exit after up_blocks[up_ft_index]; feat_out_dev [batch, C_i, h_i, w_i] fp16 NCHW where
 * (C_i,h_i,w_i) = dm_dift_shape().  If mean_out_dev != NULL also writes the ensemble mean over
 * every consecutive group of `ensemble` samples (SDFeaturizer.forward, dift.py:231) as
 * [batch/ensemble, C_i, h_i, w_i] fp32. */
int dm_dift(dm_engine* e, const void* noisy_dev, const int64_t* t_dev, const int32_t* slot_dev,
            int batch, int h, int w, int up_ft_index, void* feat_out_dev,
            void* mean_out_dev, int ensemble, void* stream);
int dm_dift_shape(int h, int w, int up_ft_index, int* c_out, int* h_out, int* w_out);

/* Consumers' reductions of the loss grid (cluster.py:125-137, xray/compute.py:210-218) on device:
 * loss_dev [n_draws, n_cond, 4, h, w] fp32 (or fp16 when loss_is_f16) ->
 *   map_out_dev [h,w] fp32 = mean_N( mean_C(L[:,n_cond-1]) - mean_C(L[:,0]) ), and
 *   scalar_out_dev [1] fp32 = mean over pixels of the map (T(x|c)).  Either may be NULL. */
int dm_reduce_typicality(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_draws, int n_cond,
                         int h, int w, void* map_out_dev, void* scalar_out_dev, void* stream);

/* The same for the grids of n_images images in one launch: maps_out_dev [n_images,h,w] fp32 (required),
 * scalars_out_dev [n_images] fp32 (optional).  cond_major = 0: loss_dev is [n_images, n_draws, n_cond, 4, h, w]
 * (the reference's grids back to back); cond_major = 1: [n_cond, n_images, n_draws, 4, h, w], i.e. the rows
 * dm_score_conds writes when its n_draws argument is n_images * n_draws (image-major draws) - no transpose needed. */
int dm_reduce_typicality_batched(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_images, int n_draws,
                                 int n_cond, int h, int w, int cond_major, void* maps_out_dev, void* scalars_out_dev,
                                 void* stream);

/* Image-space form of the same reduction, as `Cluster.load_typicality` (cluster.py:125-137) and
 * `Typicallity.compute` (xray/compute.py:210-218) produce it: the latent map is resized with
 * bilinear interpolation (align_corners=False) to the image size (img_h, img_w) and averaged over
 * every kx x ky window (AvgPool2d((kx, ky), stride 1); kx = ky = 1 gives the per-pixel X-ray map).
 * out_dev [img_h-kx+1, img_w-ky+1] fp32; work_dev: scratch of (h*w + img_h*img_w) fp32. */
int dm_typicality_image(dm_engine* e, const void* loss_dev, int loss_is_f16, int n_draws, int n_cond,
                        int h, int w, int img_h, int img_w, int kx, int ky, void* work_dev, void* out_dev,
                        void* stream);

/* The consumers' normalisations of an image-space map (fp32 [n] on the device, e.g. dm_typicality_image's output with
 * kx = ky = 1), in numpy's fp32 arithmetic:
 *   DM_NORM_SIGNED    `normalize(dm)` of diffmining/typicality/cluster.py:32-47 as `Cluster.load_typicality_norm`
 *                     (cluster.py:112-123) calls it: negatives / |min|, positives / max, (dm + 1) / 2
 *   DM_NORM_MAXABS    `dm / np.max(np.abs(dm))`: `d_compute` (diffmining/typicality/utils.py:122-134) and utils.py:14-20
 *   DM_NORM_POSITIVE  positive_only=True (cluster.py:39-42, utils.py:16-19): max(dm, 0) / max(max(dm, 0))
 *   DM_NORM_SPLIT     positive_only='split' (cluster.py:34-36): d = dm / |max(dm)|; out = clip(d, 0, 1), out_neg = -clip(d, -1, 0)
 * out_dev (and out_neg_dev for DM_NORM_SPLIT) fp32 [n]; out_dev may alias map_dev.  work_dev: 2 floats of scratch. */
enum { DM_NORM_SIGNED = 1, DM_NORM_MAXABS = 2, DM_NORM_POSITIVE = 3, DM_NORM_SPLIT = 4 };
int dm_normalize_map(dm_engine* e, const void* map_dev, int64_t n, int mode, void* work_dev, void* out_dev,
                     void* out_neg_dev, void* stream);

/* ---- Image rescale + normalisation (D.rescale + D.load_image, compute.py:126-132,165-180) --------------
 * dm_resize_lanczos: `PIL.Image.resize((out_w, out_h), LANCZOS)` of `batch` uint8 RGB images followed by `to_tensor(x) * 2 - 1`,
 *   bit-equal to PIL + TypicalityScorer.load_image.  src_dev: the images' uint8 HWC pixels (image b at desc[b].src_offset, any
 *   source size per image); out_dev: fp32 [batch][3][out_h][out_w] in [-1,1].  tables_dev: int32, per image a horizontal and a
 *   vertical table, each = bounds [out][2] (window start, window length) at *b_off and fixed-point weights [out][k] (22 fraction
 *   bits, PIL's 8-bit precision) at *k_off, built on the host in float64 by PIL's precompute_coeffs + normalize_coeffs_8bpc
 *   (typicality.lanczos_axis).  The vertical table's window starts are relative to ybox_first: the horizontal pass resamples
 *   only source rows [ybox_first, ybox_first + tmp_rows) into tmp_dev, uint8 [batch][3][tmp_rows_max][out_w]
 *   (tmp_rows <= tmp_rows_max).  tables_dev = NULL: no resampling, only the normalisation (every src size must equal
 *   out_w x out_h; tmp_dev unused).  No engine handle: returns 0, 1 on a bad argument, 2 on a HIP launch error. */
typedef struct dm_resize_desc {
    int64_t src_offset;                 /* bytes from src_dev to the image's first pixel */
    int32_t src_w, src_h;
    int32_t ybox_first, tmp_rows;       /* source rows the vertical pass reads */
    int32_t kx, ky;                     /* table row strides (max taps) of the horizontal / vertical weights */
    int32_t xb_off, xk_off;             /* int32 offsets into tables_dev: horizontal bounds, weights */
    int32_t yb_off, yk_off;             /* vertical bounds, weights */
} dm_resize_desc;
int dm_resize_lanczos(const void* src_dev, const dm_resize_desc* desc_dev, const int32_t* tables_dev, int batch, int out_w,
                      int out_h, int tmp_rows_max, void* tmp_dev, float* out_dev, void* stream);

/* ---- Patch mining: grids -> pooled maps -> top non-overlapping boxes (Cluster.df_D, cluster.py:184-215) -----------------
 * dm_typicality_image_batched: dm_typicality_image for n_images images of any sizes in three launches.  Image b reads its grid
 *   [n_draws][n_cond][4][h][w] at loss_dev + desc[b].grid_offset elements (fp16 when loss_is_f16, else fp32 — one type per call),
 *   uses work_dev + desc[b].work_offset as scratch (h*w + H*(W-ky+1) floats) and writes its map [H-kx+1][W-ky+1] fp32 at
 *   maps_out_dev + desc[b].map_offset; every map is bit-equal to dm_typicality_image on that image.
 * dm_mine_patches: per image, the reference's candidate frame (one row per window position (i, j) of the pooled map: box
 *   (x_start, y_start, x_end, y_end) = (i, j, i+kx, j+ky), x = rows, D = map[i][j]), `sort` by D (utils.py:82-83; ascending != 0
 *   is compute_least's order, cluster.py:393) and `get_non_overlapping` (utils.py:94-102): take the best candidate, drop every
 *   candidate whose box touches it (inclusive comparisons: |i-i*| <= kx and |j-j*| <= ky), up to k_per_image times
 *   (1 <= k_per_image <= DM_MINE_MAX_K).  Reads maps_dev + desc[b].map_offset and desc[b].H / W only.  Among equal keys the
 *   lowest row-major index wins (pandas leaves ties undefined); NaN keys are never selected.  priority_dev (optional, laid out
 *   like maps_dev) supplies the sort key instead of the map — a permutation's ranks give the reference's shuffled arm — while D
 *   is still read from the map.  boxes_out_dev int32 [n_images][k_per_image][4], d_out_dev fp32 [n_images][k_per_image],
 *   count_out_dev int32 [n_images] = boxes found (fewer when the map runs out); unused slots hold -1 / NaN.
 * Both calls read the descriptor table back once to check it (windows larger than an image are refused) and to size the
 * launches, so they synchronise `stream` before they launch. */
#define DM_MINE_MAX_K 64
typedef struct dm_mine_desc {
    int64_t grid_offset;                /* elements from loss_dev to the image's grid */
    int64_t work_offset;                /* floats from work_dev to the image's scratch */
    int64_t map_offset;                 /* floats from maps(_out)_dev / priority_dev to the image's map */
    int32_t n_draws, n_cond;
    int32_t h, w;                       /* latent size */
    int32_t H, W;                       /* image size */
} dm_mine_desc;
int dm_typicality_image_batched(dm_engine* e, const void* loss_dev, int loss_is_f16, const dm_mine_desc* desc_dev, int n_images,
                                int kx, int ky, void* work_dev, void* maps_out_dev, void* stream);
int dm_mine_patches(dm_engine* e, const void* maps_dev, const void* priority_dev, const dm_mine_desc* desc_dev, int n_images, int kx,
                    int ky, int k_per_image, int ascending, int32_t* boxes_out_dev, float* d_out_dev, int32_t* count_out_dev,
                    void* stream);

/* ---- Parallel-dataset mining: the median map across sets (Cluster.df_PD, parallel-dataset/cluster.py:224-251) -------------
 * A parallel group is n_sets pooled maps of one size (an image and its translations; one map per set, `load_typicallity`
 * under the set's own category = dm_typicality_image_batched's output).  dm_mine_parallel, per group g:
 *   1. median_out[g] = np.median(np.stack(maps of g), axis=0) per candidate: the middle of the n_sets sorted values, for an
 *      even n_sets (s[n/2-1] + s[n/2]) * 0.5f; NaN when any of the n_sets values is NaN (numpy's rule).  Equal to np.median
 *      under ==; bit-equal except the sign of a zero when +0 and -0 tie for the middle.
 *   2. dm_mine_patches' selection on the median map (same kernel, same rules: inclusive zone, lowest row-major index among
 *      equal keys, NaN never selected; priority_dev, laid out like median_out_dev, supplies the key of the shuffled arm).
 *   3. set_d_out[g][r][c] = set c's own map at winner r (df_PD's per-country columns).
 * maps_dev + desc[g*n_sets + c].map_offset is set c's map of group g (desc: n_groups*n_sets rows, group-major, the table
 * dm_typicality_image_batched was called with; only map_offset, H, W are read); group_desc[g] places group g's median map
 * [H-kx+1][W-ky+1] at median_out_dev + group_desc[g].map_offset (map_offset, H, W read).  Outputs: boxes_out_dev int32
 * [n_groups][k_per_image][4], d_out_dev fp32 [n_groups][k_per_image] (the median at the winner), set_d_out_dev fp32
 * [n_groups][k_per_image][n_sets], count_out_dev int32 [n_groups]; unused slots hold -1 / NaN.
 * Refused (non-zero, dm_last_error): n_sets outside [1, DM_MINE_MAX_SETS], a set whose H / W differ from its group's, a
 * window larger than an image, k_per_image outside [1, DM_MINE_MAX_K].  Reads both tables back once, like its siblings. */
#define DM_MINE_MAX_SETS 16
int dm_mine_parallel(dm_engine* e, const void* maps_dev, const dm_mine_desc* desc_dev, int n_groups, int n_sets,
                     const dm_mine_desc* group_desc_dev, int kx, int ky, int k_per_image, int ascending, const void* priority_dev,
                     void* median_out_dev, int32_t* boxes_out_dev, float* d_out_dev, float* set_d_out_dev, int32_t* count_out_dev,
                     void* stream);

/* ---- CLIP baseline mining: token grid -> pooled score map -> eligible non-overlapping boxes -> box features (DESIGN.md 4u;
 * csrc/clipmine.hip; clipmining/ranking.py:72-108 `dot_text_image`, clipmining/utils.py:75-94) ---------------------------------
 * A stream-plus-workspace function (no engine handle).  Image b: projected patch tokens fp32 [P = gh*pw][E] at tokens +
 * desc[b].token_offset floats (token p*pw + q, not normalised), image size (H, W); text: fp32 [2][E], used as given.
 *   1. s[c][p][q] = sum_e text[c][e] tokens[pq][e] / |tokens[pq]|_2
 *   2. m_c = avgpool_{kx x ky, stride 1}(bilinear_{align_corners=False}(s[c], (H, W))), computed as A s[c] B^T with the tables
 *      A [OH = H-kx+1][gh] at tables_dev + a_offset and B [OW = W-ky+1][pw] at tables_dev + b_offset (fp32; A[i][p] = the mean over
 *      image rows i ... i+kx-1 of the bilinear row weights onto token row p; built by the caller, clipmine.axis_weights), p then q
 *      ascending.  D = m_0 - m_1 (DM_CLIPMINE_DIFF) or m_0 (DM_CLIPMINE_SIM).  Candidate (i, j) is the box (i, j, i+kx, j+ky),
 *      x = rows.  maps_out_or_null: when given, D [OH][OW] is also written at maps_out + desc[b].map_offset floats.
 *   3. Only the n = min(100 k_per_image, OH OW) candidates of largest D are candidates at all (the reference's topk before
 *      get_non_overlapping).  Among equal values the lowest row-major index ranks first (torch.topk leaves ties undefined); a NaN
 *      is never a candidate (torch.topk would rank it highest: non-finite tokens are outside the contract).
 *   4. Up to k_per_image times: take the best eligible candidate still alive, drop every candidate with |i-i*| <= kx and
 *      |j-j*| <= ky (inclusive, as dm_mine_patches); stop when no eligible candidate is alive.  boxes int32 [n_images][k][4],
 *      d fp32 [n_images][k], count int32 [n_images]; unused slots hold -1 / NaN.
 *   5. feats fp32 [n_images][k][E]: f[e] = sum_p sum_q A[i][p] B[j][q] tokens[pq][e] (the mean over the box of the bilinearly
 *      upsampled raw tokens), then f / |f|_2; unused rows NaN.
 * work: desc[b].work_offset floats into it image b owns 2 P + OH OW floats (contents do not matter; regions must not overlap);
 * dm_clipmine_workspace_bytes(n_images, sum P, sum OH OW) leaves room to start every region on a multiple of 64 floats (0 = bad
 * arguments).  fp32, fixed summation orders, no floating-point atomics: image b's results do not depend on the batch around it.
 * Reads the descriptor table back once, so it synchronises `stream` before it launches.  Refused without a launch
 * (DM_CLIPMINE_E_*): a window larger than an image or with exactly one side 1 (`pool` skips it) or OH OW >= 2^30, P != gh*pw or a
 * grid side outside [1, DM_CLIPMINE_MAX_GRID], k_per_image outside [1, DM_MINE_MAX_K], E < 1, n_images outside [1, 65535], a
 * negative offset, a region that
 * does not fit in work_bytes, an unknown mode. */
#define DM_CLIPMINE_MAX_GRID 1024
#define DM_CLIPMINE_DIFF 0
#define DM_CLIPMINE_SIM 1
#define DM_CLIPMINE_E_NULL 1
#define DM_CLIPMINE_E_IMAGES 2
#define DM_CLIPMINE_E_E 3
#define DM_CLIPMINE_E_K 4
#define DM_CLIPMINE_E_MODE 5
#define DM_CLIPMINE_E_WINDOW 6
#define DM_CLIPMINE_E_GRID 7
#define DM_CLIPMINE_E_OFFSET 8
#define DM_CLIPMINE_E_WORK 9
#define DM_CLIPMINE_E_HIP 10
typedef struct dm_clipmine_desc {
    int64_t token_offset;               /* floats from tokens to the image's [P][E] */
    int64_t a_offset, b_offset;         /* floats from tables_dev to A [OH][gh] and B [OW][pw] */
    int64_t work_offset;                /* floats from work to the image's scratch (2 P + OH OW floats) */
    int64_t map_offset;                 /* floats from maps_out to the image's map (read only when maps_out is given) */
    int32_t H, W;                       /* image size */
    int32_t gh, pw, P;                  /* token grid, P = gh * pw */
    int32_t reserved;
} dm_clipmine_desc;
size_t dm_clipmine_workspace_bytes(int n_images, int64_t total_tokens, int64_t total_candidates);
int dm_clipmine_rank(void* stream, const void* tokens, const void* text, int E, const dm_clipmine_desc* desc_dev, int n_images,
                     const void* tables_dev, int kx, int ky, int k_per_image, int mode, void* work, size_t work_bytes,
                     void* maps_out_or_null, int32_t* boxes, float* d, int32_t* count, float* feats);

/* ---- Clustering: scikit-learn's KMeans fit and the reference's ranked clusters (csrc/kmeans.hip) ------------------
 * Stream-plus-workspace functions (no engine handle): every launch goes to `stream`; `work` is device memory of at least
 * dm_kmeans_workspace_bytes(n, d, k) bytes whose contents do not matter.  They return 0 or one of the DM_KMEANS_E_* codes.
 *
 * dm_kmeans_fit = KMeans(n_clusters=k, random_state=seed).fit(X) as scikit-learn 1.4 ... 1.7 runs it (one k-means++ seeding in
 * fp64, Lloyd in fp32 on mean-centred rows).  X: fp32 [n][d] row-major on the device.  uniforms_f64: the device array of the
 * 1 + (k - 1) t draws k-means++ consumes, t = 2 + int(ln k) (clustering.kmeans_uniforms); NULL with n_uniforms = 0 means
 * seed_index_i32 is an INPUT: the k rows to start from (KMeans(init=X[seed_index], n_init=1)).  tol_rel: scikit-learn's tol
 * (1e-4); the loop stops strictly when the labels repeat, else when sum_j |c_new - c_old|^2 <= tol_rel * mean_j var_j(X), else at
 * max_iter; after a non-strict stop the labels are assigned once more.  Ties: the lowest centre index; the first candidate of
 * lowest potential; empty clusters, ascending, take the rows farthest from their own centre, descending, the lowest row among
 * equals.  The stop is decided on the device; the host reads the flag once per group of iterations, so the call returns with the
 * stream synchronised.  Outputs (device): labels_i32 [n], centers_f32 [k][d] (mean added back), seed_index_i32 [k], inertia_f32
 * [1], n_iter_i32 [1].  No floating-point atomics: the same input gives the same bits on every run.
 *
 * dm_cluster_rank = the tail of the reference's cluster().  key_i = |x_rank_i - ref_label_i| (fp64 accumulation).
 *   DM_RANK_CENTROID: ref_c = centers[c], x_rank = X, X_rank_or_null must be NULL (typicality/cluster.py:325, ranking.py:147);
 *   DM_RANK_FARTHEST: ref_c = x_rank[argmax_i |X_i - centers[c]|] over ALL rows, the first among equals; x_rank = X_rank_or_null
 *   [n][d_rank], or X when NULL (parallel-dataset/cluster.py:277-286).
 * Members of a cluster are ordered by ascending key, stably by row.  The aggregate of D_f32 [n] over a cluster: DM_AGG_MEDIAN =
 * np.median (mean of the two middle values for an even count, NaN if any member is NaN); DM_AGG_MEAN = the fp32 left-to-right
 * sum in member order / count.  Clusters are ordered by descending aggregate, a NaN aggregate after every number, stably in the
 * order of the label's first appearance by row.  Empty clusters do not appear.  labels must lie in [0, k) (a row whose label
 * does not is left out).  Outputs (device): order [n] row ids, cluster-major; cluster_of_rank [k]; offsets [k + 1] into order;
 * aggregate_out [k]; n_nonempty [1]; slots past n_nonempty hold -1 / n / NaN.  The place of a row costs O(members of its
 * cluster): meant for the stage's thousands of rows.
 * Refused: n < k, k outside [1, DM_KMEANS_MAX_K], d < 1, n >= 2^24, max_iter < 1, a wrong n_uniforms, a small workspace. */
#define DM_KMEANS_MAX_K 256
#define DM_KMEANS_E_NULL 1
#define DM_KMEANS_E_N_LT_K 2
#define DM_KMEANS_E_K 3
#define DM_KMEANS_E_D 4
#define DM_KMEANS_E_N_LARGE 5
#define DM_KMEANS_E_MAX_ITER 6
#define DM_KMEANS_E_UNIFORMS 7
#define DM_KMEANS_E_WORK 8
#define DM_KMEANS_E_MODE 9
#define DM_KMEANS_E_HIP 10
#define DM_RANK_CENTROID 0
#define DM_RANK_FARTHEST 1
#define DM_AGG_MEDIAN 0
#define DM_AGG_MEAN 1
int dm_kmeans_workspace_bytes(int n, int d, int k, size_t* bytes_out);
int dm_kmeans_fit(void* stream, const void* X, int n, int d, int k, const double* uniforms_f64, int n_uniforms, int max_iter,
                  float tol_rel, void* work, size_t work_bytes, int32_t* labels_i32, float* centers_f32, int32_t* seed_index_i32,
                  float* inertia_f32, int32_t* n_iter_i32);
int dm_cluster_rank(void* stream, const void* X, const void* X_rank_or_null, int n, int d, int d_rank, const int32_t* labels,
                    const float* centers, int k, const float* D_f32, int mode, int aggregate, void* work, size_t work_bytes,
                    int32_t* order, int32_t* cluster_of_rank, int32_t* offsets, float* aggregate_out, int32_t* n_nonempty);

/* ---- UMAP projection for the clustering stage: exact kNN, fuzzy graph, synchronous layout (csrc/umap.hip) ----------
 * Stream-plus-workspace functions (no engine handle), as the clustering ones.  The rules are stated in numpy in umapfit.py (a
 * restatement of umap-learn 0.5.6 at the reference's settings; PARITY UNPINNED: not yet checked against umap-learn itself).
 * `work`: device memory of at least dm_umap_workspace_bytes(n, d, n_neighbors, n_components) bytes; its contents do not matter,
 * except that dm_umap_layout keeps the edge schedule there between a call with first_epoch = 0 and later calls that go on.
 *
 * dm_umap_knn: X fp32 [n][d] -> idx_out int32 [n][n_neighbors], dist_out fp32 [n][n_neighbors]: the n_neighbors nearest rows of every
 * row, self included, ascending distance, ties to the lower index.  Squared distances are fp64 sums over ascending feature index
 * with separate multiply and add; the distance is the fp64 sqrt rounded to fp32: bit-equal to the numpy restatement.
 *
 * dm_umap_graph: rho_out, sigma_out fp32 [n] (smooth_knn_dist: 64-step bisection in fp64, local_connectivity 1); dense_P_out fp32
 * [n][n] = (A + A^T) - A o A^T of the memberships with entries below max(P) / n_epochs set to 0; the edge list = its non-zeros in
 * row-major order: row_ptr_out int32 [n + 1], col_out int32 and weight_out fp32 with room for 2 n n_neighbors entries,
 * n_edges_out int32 [1] (device).
 *
 * dm_umap_layout: epochs [first_epoch, last_epoch) of the synchronous layout on Y_inout fp32 [n][n_components], one launch per epoch,
 * back to back on `stream`, no host synchronisation.  a, b: the curve parameters; seed: of the counter-based draw of the repulsive
 * samples.  first_epoch = 0 starts the schedule (eps = max w / w, 5 negative samples per positive one); a later first_epoch goes on
 * from the schedule the same `work` holds.  No atomics: bit-reproducible.
 * Refused without a launch: a NULL pointer, n >= DM_UMAP_MAX_N, n_neighbors >= n, n_neighbors outside [2, DM_UMAP_MAX_NEIGHBORS],
 * n_components outside [1, DM_UMAP_MAX_COMPONENTS], d < 1, n_epochs < 1 or an epoch range outside 0 <= first <= last <= n_epochs,
 * a small workspace, n_edges outside [0, 2 n DM_UMAP_MAX_NEIGHBORS]. */
#define DM_UMAP_MAX_N 4096
#define DM_UMAP_MAX_NEIGHBORS 64
#define DM_UMAP_MAX_COMPONENTS 64
#define DM_UMAP_E_NULL 1
#define DM_UMAP_E_N_LARGE 2
#define DM_UMAP_E_NEIGHBORS_GE_N 3
#define DM_UMAP_E_NEIGHBORS 4
#define DM_UMAP_E_COMPONENTS 5
#define DM_UMAP_E_D 6
#define DM_UMAP_E_EPOCHS 7
#define DM_UMAP_E_WORK 8
#define DM_UMAP_E_EDGES 9
#define DM_UMAP_E_HIP 10
int dm_umap_workspace_bytes(int n, int d, int n_neighbors, int n_components, size_t* bytes_out);
int dm_umap_knn(void* stream, const void* X, int n, int d, int n_neighbors, void* work, size_t work_bytes, int32_t* idx_out,
                float* dist_out);
int dm_umap_graph(void* stream, const int32_t* idx, const float* dist, int n, int n_neighbors, int n_epochs, void* work,
                  size_t work_bytes, float* rho_out, float* sigma_out, float* dense_P_out, int32_t* row_ptr_out, int32_t* col_out,
                  float* weight_out, int32_t* n_edges_out);
int dm_umap_layout(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_edges, int n_components,
                   float a, float b, int n_epochs, int seed, int first_epoch, int last_epoch, float* Y_inout, void* work,
                   size_t work_bytes);

/* dm_umap_spectral: UMAP's spectral initialisation from the edge list of dm_umap_graph, without a host round trip (csrc/umap_spectral.hip;
 * the rules: `spectral_init_iter_host` in umapfit.py).  The n_components + 1 top eigenvectors of D^-1/2 P D^-1/2 by Chebyshev-filtered
 * subspace iteration in fp64 on a block of min(n, m + max(8, m / 2)) columns, m = n_components + 1; every outer iteration of the cap
 * (40) is enqueued on `stream`, and a device-side flag turns the ones after convergence into empty launches.  No floating-point
 * atomics: bit-reproducible.
 *   noise, fallback   fp32 [n][n_components], device: the seeded N(0, 1e-4) noise and the rescaled uniform(-10, 10) initialisation,
 *                     both drawn by the host (they do not depend on the graph)
 *   work              at least dm_umap_spectral_workspace_bytes(n, n_components) bytes; its contents do not matter
 *   Y0_out            fp32 [n][n_components]: eigenvectors 1 .. n_components, sign by the largest-magnitude entry, 10 / max|.|, + noise,
 *                     each coordinate rescaled to [0, 10]; `fallback` if the graph has more than one component or n_components + 1 >= n
 *   eigvals_out       fp64 [n_components + 1], descending (1 - these are the Laplacian's); eigvecs_out fp64 [n][n_components + 1] or NULL
 *   status_out        fp64 [8]: 0 spectral / 1 random, component count, outer iterations, converged (0 / 1), the largest residual
 *                     ||M v - theta v||_2 of the last iteration, the last filter's cut and degree, the block's columns.  A spectral
 *                     status that is not converged (40 iterations without every residual <= 1e-11) means Y0_out is not to be used.
 * Refused without a launch: a NULL pointer (eigvecs_out excepted), n >= DM_UMAP_MAX_N, n < 1 (DM_UMAP_E_NEIGHBORS_GE_N),
 * n_components outside [1, DM_UMAP_MAX_COMPONENTS], a small workspace. */
int dm_umap_spectral_workspace_bytes(int n, int n_components, size_t* bytes_out);
int dm_umap_spectral(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_components, int seed,
                     const float* noise, const float* fallback, void* work, size_t work_bytes, float* Y0_out, double* eigvals_out,
                     double* eigvecs_out, double* status_out);

/* ---- UMAP above DM_UMAP_MAX_N - 1 rows: the route without the n x n graph (csrc/umap_sparse.hip) --------------------
 * The same rules and error codes as dm_umap_*, for n < DM_UMAP_SPARSE_MAX_N; it takes smaller n too, and there every output is
 * bit-equal to the dm_umap_* function of the same name.  (Above 4095 rows umap-learn itself turns to approximate, unseeded
 * neighbours; these stay exact.)  `work`: at least dm_umap_sparse_workspace_bytes(n, d, n_neighbors, n_components) bytes, no n x n term.
 *
 * dm_umap_sparse_knn: a workgroup owns 32 rows and streams column tiles, merging each tile into a running top-k per row.
 * dm_umap_sparse_graph: memberships per list slot; row i's edges are its out- and in-neighbours (found by a scan of idx, no atomics);
 * there is no dense output; col_out / weight_out have room for 2 n n_neighbors entries.  A row may hold up to n - 1 edges.
 * dm_umap_sparse_layout: dm_umap_layout's kernels; `work` needs the layout's part only.
 * dm_umap_sparse_spectral: dm_umap_spectral's solver with the component labels in `work`
 * (dm_umap_sparse_spectral_workspace_bytes(n, n_components) bytes).
 * Refused without a launch: as dm_umap_*, with n >= DM_UMAP_SPARSE_MAX_N for DM_UMAP_E_N_LARGE. */
#define DM_UMAP_SPARSE_MAX_N 65536
int dm_umap_sparse_workspace_bytes(int n, int d, int n_neighbors, int n_components, size_t* bytes_out);
int dm_umap_sparse_knn(void* stream, const void* X, int n, int d, int n_neighbors, void* work, size_t work_bytes, int32_t* idx_out,
                       float* dist_out);
int dm_umap_sparse_graph(void* stream, const int32_t* idx, const float* dist, int n, int n_neighbors, int n_epochs, void* work,
                         size_t work_bytes, float* rho_out, float* sigma_out, int32_t* row_ptr_out, int32_t* col_out, float* weight_out,
                         int32_t* n_edges_out);
int dm_umap_sparse_layout(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_edges,
                          int n_components, float a, float b, int n_epochs, int seed, int first_epoch, int last_epoch, float* Y_inout,
                          void* work, size_t work_bytes);
int dm_umap_sparse_spectral_workspace_bytes(int n, int n_components, size_t* bytes_out);
int dm_umap_sparse_spectral(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_components, int seed,
                            const float* noise, const float* fallback, void* work, size_t work_bytes, float* Y0_out, double* eigvals_out,
                            double* eigvecs_out, double* status_out);

/* ---- UMAP on a disconnected graph: per-component spectral initialisation (csrc/umap_multi.hip) ----------------------
 * Opt-in (umapfit's disconnected='components'); the rules: `multi_component_init_host` in umapfit.py, a restatement of umap-learn's
 * multi_component_layout, PARITY UNPINNED.  One set of entries for both routes: n < DM_UMAP_SPARSE_MAX_N, no n x n buffer.  No
 * floating-point atomics, fixed summation orders: bit-reproducible.
 *
 * dm_umap_components: the connected components of the edge list (row_ptr int32 [n + 1], col, weight: `edge_capacity` slots each).
 *   X                  fp32 [n][d] or NULL (then d is ignored and centroids_out may be NULL)
 *   comp_out           int32 [n]: the component of every vertex; ids ascend with each component's smallest vertex
 *   count_out          int32 [1]: c
 *   offsets_out        int32 [n + 1]: component l owns grouped positions [offsets[l], offsets[l + 1]); entries past c hold n
 *   perm_out           int32 [n]: the vertex at each grouped position (grouped by component, ascending vertex inside: stable)
 *   edge_offsets_out   int32 [n + 1]: component l's edges are slots [edge_offsets[l], edge_offsets[l + 1]) of sub_col_out /
 *                      sub_weight_out (edge_capacity slots each); entries past c hold the total
 *   sub_row_ptr_out    int32 [2 n + 1]: component l's own CSR row pointer, offsets[l + 1] - offsets[l] + 1 entries from index
 *                      offsets[l] + l, starting at 0; entries from n + c hold 0
 *   sub_col_out        a vertex's position inside its component (grouped position - offsets[l]); rows and each row's edges keep
 *                      their order.  An edge into another component (an asymmetric list) is dropped.
 *   centroids_out      fp64 [min(n, DM_UMAP_MULTI_MAX_COMP)][d]: the mean of each component's rows, added in ascending row index in
 *                      fp64; rows past c hold 0
 * dm_umap_multi_init: Y0 from the sub-graph.  offsets_host / edge_offsets_host (int32 [c + 1]) and plan_host (int32 [c]: 1 = solve,
 * 0 = uniform) are HOST arrays, read before the call returns; the others are device memory.  Every component with plan 1 (it must
 * have more than n_components + 1 rows) runs dm_umap_sparse_spectral's launches on its slice; then new kernels take each
 * component's signs and max|E|, place R = E (range / max|E|) + meta (or meta + range unit for plan 0) through perm, take max|R|,
 * and finish as dm_umap_spectral does (10 / max|R|, the fp32 cast, + noise, each coordinate rescaled to [0, 10]).
 *   meta               fp64 [c][n_components]; range fp64 [c]; unit fp64 [n][n_components]; noise fp32 [n][n_components]
 *   Y0_out             fp32 [n][n_components];  R_out fp64 [n][n_components]
 *   eigvals_out        fp64 [c][n_components + 1];  eigvecs_out fp64 [n][n_components + 1], rows in grouped order
 *   status_out         fp64 [c][8]: dm_umap_spectral's record per component; a uniform one reads 2, 1, 0, 0, NaN, 0, 0, 0
 * Refused without a launch: a NULL pointer, n >= DM_UMAP_SPARSE_MAX_N, n < 1, d < 1 (with X), n_components outside
 * [1, DM_UMAP_MAX_COMPONENTS], edge_capacity outside [0, 2 n DM_UMAP_MAX_NEIGHBORS], a small workspace, c outside
 * [1, min(n, DM_UMAP_MULTI_MAX_COMP)] (DM_UMAP_E_COUNT), offsets that do not ascend from 0 to n or edge offsets that do not ascend
 * within edge_capacity (DM_UMAP_E_EDGES), a plan of 1 for a component of n_components + 1 rows or fewer (DM_UMAP_E_NEIGHBORS_GE_N). */
#define DM_UMAP_MULTI_MAX_COMP 1024
#define DM_UMAP_E_COUNT 11
int dm_umap_components_workspace_bytes(int n, size_t* bytes_out);
int dm_umap_components(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, const float* X, int n, int d,
                       int edge_capacity, void* work, size_t work_bytes, int32_t* comp_out, int32_t* count_out, int32_t* offsets_out,
                       int32_t* perm_out, int32_t* edge_offsets_out, int32_t* sub_row_ptr_out, int32_t* sub_col_out,
                       float* sub_weight_out, double* centroids_out);
int dm_umap_multi_workspace_bytes(int n, int n_components, size_t* bytes_out);
int dm_umap_multi_init(void* stream, const int32_t* sub_row_ptr, const int32_t* sub_col, const float* sub_weight, const int32_t* perm,
                       const int32_t* comp, const int32_t* offsets, const int32_t* plan, const int32_t* offsets_host,
                       const int32_t* edge_offsets_host, const int32_t* plan_host, int n, int n_comp, int edge_capacity, int n_components,
                       int seed, const double* meta, const double* range, const double* unit, const float* noise, void* work,
                       size_t work_bytes, float* Y0_out, double* R_out, double* eigvals_out, double* eigvecs_out, double* status_out);

/* ---- X-ray evaluation: threshold counts of a heat-map against a ground-truth box (csrc/xray_eval.hip) -------------
 * The device half of `aucpr` and `mean_typicallity` (applications/xray/compute.py:263-284).  A stream-plus-workspace function
 * (no engine handle).  Row r of the descriptor table names a map [H][W] fp32 at maps_dev + map_offset (floats, any value; two
 * rows may name one map) and a box (x1, y1, x2, y2) = dm[y1:y2, x1:x2]: x = COLUMNS, clipped to the map as numpy clips a slice,
 * possibly empty.  thresholds_dev: n_thresholds fp64 values, strictly decreasing.  Per row, for k in [0, T):
 *   tp[k] = pixels inside the box with (double)v > thresholds[k];  fp[k] = the same outside;  (fp32 value against fp64
 *   threshold, in fp64, strictly: a NaN pixel exceeds nothing);  n_in = the clipped box's area;  box_sum = the fp64 sum of
 *   the pixels inside (NaN if one is NaN; 0 for an empty box).
 * Counts are integers (LDS integer atomics, per-workgroup partials added in a fixed order): exact.  box_sum has no floating-point
 * atomic and a pixel-to-thread map that depends on the pixel's index alone: the same map and box give the same bits at any
 * position of any batch.  work_dev: at least dm_xray_eval_workspace_bytes(n_rows, n_thresholds, max_r H_r W_r) bytes (0 = bad
 * arguments) whose contents do not matter.  Reads the two tables back once, so it synchronises `stream` before it launches.
 * Refused without a launch (DM_XRAY_E_*): n_thresholds outside [1, DM_XRAY_MAX_THRESHOLDS]; thresholds not strictly decreasing
 * or NaN; H or W < 1; H W >= 2^24 (the reference's x.sum() is an fp32 sum of ones); a negative box coordinate (numpy would
 * count it from the end). */
#define DM_XRAY_MAX_THRESHOLDS 4096
#define DM_XRAY_E_NULL 1
#define DM_XRAY_E_ROWS 2
#define DM_XRAY_E_NTHR 3
#define DM_XRAY_E_THR_ORDER 4
#define DM_XRAY_E_SIZE 5
#define DM_XRAY_E_PIXELS 6
#define DM_XRAY_E_BOX 7
#define DM_XRAY_E_HIP 8
typedef struct dm_xray_desc { int64_t map_offset; int32_t H, W; int32_t x1, y1, x2, y2; } dm_xray_desc;
size_t dm_xray_eval_workspace_bytes(int n_rows, int n_thresholds, int64_t max_pixels);
int dm_xray_eval(const void* maps_dev, const dm_xray_desc* desc_dev, int n_rows, const double* thresholds_dev, int n_thresholds,
                 void* work_dev, int32_t* tp_out_dev /*[n_rows][T]*/, int32_t* fp_out_dev /*[n_rows][T]*/,
                 int32_t* n_in_out_dev /*[n_rows]*/, double* box_sum_out_dev /*[n_rows]*/, void* stream);

/* ---- Typicality overlays: Gaussian-filtered alpha blend per patch (csrc/overlay.hip) -------------------------------
 * The device half of `Cluster.load_and_apply_alpha_bbox` (typicality/cluster.py:93-110), `utils.apply_alpha` (typicality/utils.py:
 * 165-214), `Cluster.apply_alpha_` (applications/parallel-dataset/cluster.py:132-141) and `filter_patch` (utils.py:104-109).
 * Stream-plus-workspace functions (no engine handle).  Both read their descriptor table back once, so they synchronise `stream`
 * before they launch; both return 0, 1 (a bad argument: nothing was launched) or 2 (a HIP error).  No floating-point atomic.
 *
 * dm_gaussian_filter_maps: scipy.ndimage.gaussian_filter(a, sigma) (truncate 4, mode 'reflect') of n_maps fp32 maps of mixed sizes.
 * Map b is [H][W] at maps_dev + map_offset (floats); its result goes to out_dev + out_offset, its fp32 intermediate to the workspace
 * at work_offset (floats, into the intermediate region; regions of different maps must not overlap).  weights_dev: the 2 radius + 1
 * fp64 weights exp(-0.5/sigma^2 x^2) / sum, built by the caller with numpy so that the bits are numpy's; radius = (int)(4 sigma +
 * 0.5).  Axis 0, then axis 1; each pass stages a DM_GAUSS_TILE^2 output tile with its halo in LDS, resolving `reflect` (a mirror of
 * period 2n, as often as the halo wraps) at load time, starts from the centre tap a[i] w[0], adds the pairs (a[i-j] + a[i+j]) w[j] in
 * fp64 from j = radius inward to j = 1 (no fused multiply-add) and rounds to fp32 once: bit-equal to scipy.  post_op: DM_GAUSS_POST_
 * NONE; _CLAMP = T * (T > 0) in fp32 (a negative value becomes -0, NaN stays); _UNIT = T / max(T) in fp32, then the clamp, where
 * max is numpy's (NaN if any element is NaN) from per-tile partials reduced in a fixed order, written to max_out_dev[b] when that is
 * not NULL; a maximum of 0 or NaN makes the map all +0 (the `degenerate` rule of dm_overlay_blend).
 * work_dev: work_bytes >= dm_overlay_workspace_bytes(n_maps, sum_b H_b W_b, max_b H_b, max_b W_b) bytes (0 = bad arguments) whose
 * contents do not matter.  Bad arguments: a null pointer (max_out_dev may be NULL), n_maps < 1, sigma <= 0 or NaN, a radius that is
 * not sigma's or exceeds DM_GAUSS_MAX_RADIUS, n_maps > 65535, an unknown post_op, H or W outside [1, 2^24], H W >= 2^31, a negative offset, an
 * intermediate that leaves the workspace.
 *
 * dm_overlay_blend: one workgroup per row of the table.  A row names an image [img_h][img_w][3] uint8 at images_dev + image_offset
 * (bytes), a map [map_h][map_w] fp32 at maps_dev + map_offset (floats) - ALREADY filtered and clamped - placed with its first element
 * at image pixel (map_x0, map_y0) (T = 0 outside it: "a map smaller than its image" and "a map that is already the crop" are both
 * placements; map_h = 0 or map_w = 0 is "no map"), a box (x_start, y_start, x_end, y_end) with x = ROWS, and the dtype flow:
 *   DM_OVERLAY_IMAGE / DM_OVERLAY_STORED   t = (double)T;  R = 0.05 I + 0.95 (t I + (1.0 - t))          (all float64)
 *   DM_OVERLAY_CROP                         R = 0.05 I + 0.95 ((double)T I + (double)(1.0f - T))          (`1 - T` is fp32)
 * with I = (double)u8 / 255.0, no fused multiply-add; the byte is R * 255.0 truncated toward zero to int32 (saturating), modulo 256.
 * Per row: blended_out_dev + out_offset and plain_out_dev + out_offset (bytes) get the blended and the untouched crop [bh][bw][3];
 * alpha_out_dev (or NULL) + alpha_offset (floats) gets T [bh][bw]; lum_out_dev[r] = the sum over the plain crop of PIL's 'L' value
 * (19595 R + 38470 G + 7471 B + 0x8000) >> 16; verdict_out_dev[r] = 30 < sum / count < 225 in float64 (0 for an empty crop);
 * degenerate_out_dev[r] = 1 when the row is DM_OVERLAY_CROP, map_index >= 0 and map_max_dev[map_index] is 0 or NaN (its T is then
 * taken as 0).  A zero-area box writes no pixel.  Bad arguments: a null pointer (alpha_out_dev may be NULL, map_max_dev too when no
 * row has map_index >= 0), n_rows < 1, an unknown variant, an image of no pixels or one that leaves images_dev, a box outside its
 * image, a map that leaves maps_dev or overhangs its image, map_index outside [-1, n_map_max), a crop that leaves out_bytes /
 * alpha_elements. */
#define DM_GAUSS_TILE 32
#define DM_GAUSS_MAX_RADIUS 200
#define DM_GAUSS_POST_NONE 0
#define DM_GAUSS_POST_CLAMP 1
#define DM_GAUSS_POST_UNIT 2
#define DM_OVERLAY_IMAGE 0
#define DM_OVERLAY_CROP 1
#define DM_OVERLAY_STORED 2
typedef struct dm_gauss_desc { int64_t map_offset, out_offset, work_offset; int32_t H, W; } dm_gauss_desc;
typedef struct dm_overlay_row {
    int64_t image_offset, map_offset, out_offset, alpha_offset;
    int32_t img_h, img_w, map_h, map_w, map_x0, map_y0;
    int32_t x_start, y_start, x_end, y_end;
    int32_t variant, map_index;
} dm_overlay_row;
size_t dm_overlay_workspace_bytes(int n_maps, int64_t total_elements, int max_h, int max_w);
int dm_gaussian_filter_maps(const void* maps_dev, const dm_gauss_desc* desc_dev, int n_maps, double sigma, const double* weights_dev,
                            int radius, int post_op, void* work_dev, size_t work_bytes, void* out_dev, float* max_out_dev /*[n_maps]*/,
                            void* stream);
int dm_overlay_blend(const void* images_dev, int64_t image_bytes, const void* maps_dev, int64_t map_elements, const float* map_max_dev,
                     int n_map_max, const dm_overlay_row* rows_dev, int n_rows, void* blended_out_dev, void* plain_out_dev,
                     int64_t out_bytes, float* alpha_out_dev, int64_t alpha_elements, int64_t* lum_out_dev /*[n_rows]*/,
                     int32_t* verdict_out_dev /*[n_rows]*/, int32_t* degenerate_out_dev /*[n_rows]*/, void* stream);

/* ---- Doersch baseline: dense detector search, winners and top-k (csrc/dense_search.hip) --------------------------
 * The device half of `dense_search_cuda` (doersch/hog.py:124-185): every detector against every cell of every image, of which only
 * the best cell per (detector, image) and then the best images per detector are kept.  Stream-plus-workspace functions (no engine
 * handle); nothing synchronises the stream.
 *
 * dm_dense_search_winners, once per chunk of B images.  data_f16 [B][cells][C] fp16 row-major (the reference's [B, W, H, C] with
 * cells = W H, cell i = a H + b); w_f16 [K][C] fp16; mask_u8_or_null [B][cells] uint8 or NULL.  Both fp16 pointers 16-byte aligned.
 *   s(k, b, i) = the fp32 sum of the exact products data[b][i][c] w[k][c] (v_mfma_f32_16x16x32_f16, fp32 accumulation from +0) in
 *     an order that depends on C alone: not on B, K, the chunk, the position in it or the other detectors of the call;
 *   a cell whose mask byte is 0 scores +0 exactly (the reference multiplies by the mask: a masked cell beats every negative score),
 *     unless its score is NaN, which stays NaN (NaN * 0);
 *   the winner of (k, b) is the largest s, the lowest cell among equal values (-0 = +0); a NaN score never wins; an image without
 *     a non-NaN cell gives (-inf, -1).
 * score_f32 / cell_i32 are tables [K][ld] that live across chunks: this call writes column image_offset + b of every row k < K and
 * nothing else.  work: dm_dense_search_workspace_bytes(B, cells, K) bytes (0 = bad arguments), 8-byte aligned, contents free: one
 * packed (ordered score bits, inverted cell) key per detector and 64-cell tile, merged by an integer max.  The [cells][K] scores
 * never reach memory; a feature row is read once.  No floating-point atomics: the same input gives the same bits on every run.
 *
 * dm_dense_search_topk, once after the last chunk.  Per detector k over columns [0, n_images) of the two tables: the top_k entries
 * by descending score, ascending image among equal scores (the reference's stable `sorted(..., reverse=True)` over entries in
 * image order).  Never admitted: -inf or NaN scores; with only_pos != 0, scores that are not > 0 (hog.py:177).  top_score_f32,
 * top_image_i32, top_cell_i32 [K][top_k], count_i32 [K]; slots from count on hold NaN / -1 / -1.
 *
 * dm_dense_search_gather: pairs_i32 [n][2] = (image in the chunk, cell) on the device -> out_f16 [n][C], bit copies of
 * data[image][cell] (the reference's `ret_ws`); a pair outside [0, B) x [0, cells) reads nothing and gives a zero row.
 *
 * Refused without a launch (DM_DENSE_E_*): a null pointer; B, n_images, n, cells, K or top_k < 1; K > DM_DENSE_MAX_DETECTORS;
 * top_k > DM_DENSE_MAX_TOPK; C < 8 or C % 8 != 0 (rows are then 16-byte aligned); cells >= 2^24; image_offset < 0 or
 * ld < image_offset + B (top-k: ld < n_images); a workspace that is too small; a misaligned pointer. */
#define DM_DENSE_MAX_DETECTORS 128
#define DM_DENSE_MAX_TOPK 128
#define DM_DENSE_E_NULL 1
#define DM_DENSE_E_IMAGES 2
#define DM_DENSE_E_CELLS 3
#define DM_DENSE_E_CELLS_LARGE 4
#define DM_DENSE_E_K 5
#define DM_DENSE_E_TOPK 6
#define DM_DENSE_E_C 7
#define DM_DENSE_E_LD 8
#define DM_DENSE_E_WORK 9
#define DM_DENSE_E_ALIGN 10
#define DM_DENSE_E_HIP 11
size_t dm_dense_search_workspace_bytes(int B, int cells, int K);
int dm_dense_search_winners(void* stream, const void* data_f16, const void* w_f16, const void* mask_u8_or_null, int B, int cells, int C,
                            int K, int image_offset, int ld, void* work, size_t work_bytes, float* score_f32, int32_t* cell_i32);
int dm_dense_search_topk(void* stream, const float* score_f32, const int32_t* cell_i32, int K, int n_images, int ld, int top_k,
                         int only_pos, float* top_score_f32, int32_t* top_image_i32, int32_t* top_cell_i32, int32_t* count_i32);
int dm_dense_search_gather(void* stream, const void* data_f16, int B, int cells, int C, const int32_t* pairs_i32, int n, void* out_f16);

/* ---- Doersch baseline: detector initialisation, wide search and greedy ranking (csrc/dense_search_wide.hip) ------------
 * `init_detectors` and `rank_init_detectors` of doersch/doersch.py:317-385: every one of thousands of candidate detectors against
 * every cell of every image, then the greedy choice of the candidates whose neighbour lists do not overlap an accepted one's.
 *
 * dm_dense_wide_winners: the contract of dm_dense_search_winners — the same operands, tables [K][ld], mask / NaN / -0 / lowest-cell
 * rules and refusals — for 1 <= K <= DM_DENSE_WIDE_MAX_DETECTORS.  For every (k, image) the result is BIT-EQUAL to what
 * dm_dense_search_winners writes when the same detectors are given to it in blocks of DM_DENSE_MAX_DETECTORS: a score's chain of
 * MFMAs is the same (ascending blocks of 64 channels, two v_mfma_f32_16x16x32_f16 per block, the same channels in the same lane
 * groups, zero chunks past C).  A workgroup stages 256 cells x 256 detectors through LDS per 64-channel step.  work:
 * dm_dense_wide_workspace_bytes(B, cells, K) bytes (0 = bad arguments), 8-byte aligned, contents free: a [B][K] table of packed
 * (ordered score bits, inverted cell) keys that the call zeroes and merges into by a 64-bit unsigned integer atomic max (a vector
 * memory atomic; the order of arrival cannot matter).  No floating-point atomics: the same input gives the same bits on every run.
 *
 * dm_dense_wide_topk: dm_dense_search_topk's admission and order for K up to the wide limit.  Per listed entry it gives the
 * reference's box corner top_x = (cell / H) 8, top_y = (cell % H) 8 with H = image_h_i32[image] (images of one search may differ in
 * size) instead of the cell.  d20_i32_or_null [K]: the number of positive_u8_or_null[image] != 0 among the first min(20, count[k])
 * entries (`search_batch`, doersch.py:95); it needs positive_u8_or_null [n_images].  Slots from count on hold NaN / -1 / -1 / -1.
 *
 * dm_detector_rank: key_i32 [N] (the d20 count; any int32), the candidates' lists nb_image_i32 / nb_x_i32 / nb_y_i32 [N][L] of which
 * the first min(max(nb_count_i32[k], 0), L) entries count (an entry with a negative image is none).  Candidates are visited by
 * descending key, ascending index among equal keys.  Candidate k is rejected when for SOME accepted detector d the number of pairs
 * (entry of k, entry of d) with the same image and 13 inter > 6 box^2 (= IoU > 0.3 of the boxes (x, y, x + box, y + box), exactly)
 * exceeds max_pairs; the count starts from zero for every d.  Otherwise k is accepted.  The visit stops at num_detectors accepted
 * or after the last candidate: accepted_i32 [num_detectors] = candidate indices in acceptance order, -1 from n on;
 * n_accepted_i32 [1] = n.  Contract: within one candidate's list an image occurs at most once (what a top-k over per-image winners
 * yields).  work: dm_detector_rank_workspace_bytes(N, L, num_detectors) bytes (0 = bad arguments), 4-byte aligned, contents free
 * (the visiting order and the accepted detectors' lists).  Integer arithmetic throughout; one persistent workgroup.
 * Refused without a launch (DM_RANK_E_*): a null pointer; N, L, num_detectors or box outside [1, DM_DETECTOR_RANK_MAX_*];
 * max_pairs < 0; a workspace that is too small; a misaligned workspace. */
#define DM_DENSE_WIDE_MAX_DETECTORS 32768
#define DM_DETECTOR_RANK_MAX_N 32768
#define DM_DETECTOR_RANK_MAX_L 128
#define DM_DETECTOR_RANK_MAX_DETECTORS 4096
#define DM_DETECTOR_RANK_MAX_BOX 2048
#define DM_RANK_E_NULL 1
#define DM_RANK_E_N 2
#define DM_RANK_E_L 3
#define DM_RANK_E_DETECTORS 4
#define DM_RANK_E_BOX 5
#define DM_RANK_E_PAIRS 6
#define DM_RANK_E_WORK 7
#define DM_RANK_E_ALIGN 8
#define DM_RANK_E_HIP 9
size_t dm_dense_wide_workspace_bytes(int B, int cells, int K);
int dm_dense_wide_winners(void* stream, const void* data_f16, const void* w_f16, const void* mask_u8_or_null, int B, int cells, int C,
                          int K, int image_offset, int ld, void* work, size_t work_bytes, float* score_f32, int32_t* cell_i32);
int dm_dense_wide_topk(void* stream, const float* score_f32, const int32_t* cell_i32, int K, int n_images, int ld, int top_k, int only_pos,
                       const void* positive_u8_or_null, const int32_t* image_h_i32, float* top_score_f32, int32_t* top_image_i32,
                       int32_t* top_x_i32, int32_t* top_y_i32, int32_t* count_i32, int32_t* d20_i32_or_null);
size_t dm_detector_rank_workspace_bytes(int N, int L, int num_detectors);
int dm_detector_rank(void* stream, const int32_t* key_i32, const int32_t* nb_image_i32, const int32_t* nb_x_i32, const int32_t* nb_y_i32,
                     const int32_t* nb_count_i32, int N, int L, int box, int max_pairs, int num_detectors, void* work, size_t work_bytes,
                     int32_t* accepted_i32, int32_t* n_accepted_i32);

/* ---- Doersch baseline: HOG-LAB features from pixels (csrc/hoglab.hip) ------------------------------------------------
 * `get_hoglab_single` + `normalize` of doersch/hog.py:24-87 on the device: B RGB uint8 images [B][H][W][3] of one size -> per image
 * the [bc][br][2112] tensor the dense search reads (nr = H / 8, nc = W / 8 cells of 8 x 8 pixels, br = nr - 7, bc = nc - 7 blocks of
 * 8 x 8 cells; block COLUMN first, cell = q br + p).  A feature is 1984 HOG values (skimage.feature.hog: 31 orientations, unsigned
 * gradients, no interpolation, L2-Hys) followed by 128 Lab values ((a, b) of rgb2lab at the centres of the block's 64 cells).
 * Stream-plus-workspace functions (no engine handle); nothing synchronises the stream; no atomics: every float sum runs in a fixed
 * order, so an image gives the same bits on every run, alone or at any position of any batch, whichever outputs are asked for.
 *
 * dm_hoglab_bin_table (host only, needs no GPU): fills uint8 [511][511], entry (g_row + 255) 511 + (g_col + 255) = the orientation
 * bin of the integer gradient (g_row, g_col): o = fmod(atan2(g_row, g_col) 180 / pi, 180) made non-negative, in fp64; bin i holds o iff
 * (180.0 / 31) i <= o < (180.0 / 31) (i + 1).  The kernels take the bin from this table on the device (`bins`): fp32 atan2 places
 * integer gradients that lie 3e-6 degrees from a bin edge on the wrong side.
 * dm_hoglab_cells: the first kernel alone.  hog_cells fp32 [B][nr][nc][31]: per cell and bin the sum of the gradient magnitudes of
 * the cell's pixels in that bin / 64 (per pixel the channel of the largest g_row^2 + g_col^2, the lowest among equals; the sum in
 * ascending pixel order in fp64, rounded once).  lab_cells fp32 [B][2][nr][nc]: (a, b) averaged over pixels (8R+3..4, 8C+3..4).
 * dm_hoglab_features: both kernels.  work: dm_hoglab_workspace_bytes(B, H, W) bytes (0 = bad arguments), contents free (the two cell
 * maps).  out_f16 [B][bc][br][2112] fp16: feature / its L2 norm over the 2112 values; raw_f32, same shape, fp32: the feature before
 * that division; either may be NULL, not both.
 *
 * Refused without a launch (DM_HOGLAB_E_*): a null required pointer; B < 1, or a batch whose one-dimensional grid would reach 2^23
 * workgroups (grid x block stays below 2^32 threads: 33.5 million cells, 8192 images of 512 x 512); H or W below 64 or
 * above DM_HOGLAB_MAX_SIDE (every pixel, cell and block coordinate then fits 16 bits; offsets are 64-bit throughout); more than
 * 2^24 - 1 blocks per image (the search's limit); a workspace that is too small; images / bins are read by bytes and need no
 * alignment, out_f16 / raw_f32 / work must be 16-byte aligned, hog_cells / lab_cells 4-byte aligned. */
#define DM_HOGLAB_MAX_SIDE 65535
#define DM_HOGLAB_BINS 31
#define DM_HOGLAB_FEATURE 2112
#define DM_HOGLAB_E_NULL 1
#define DM_HOGLAB_E_BATCH 2
#define DM_HOGLAB_E_SIDE 3
#define DM_HOGLAB_E_BLOCKS 4
#define DM_HOGLAB_E_WORK 5
#define DM_HOGLAB_E_ALIGN 6
#define DM_HOGLAB_E_HIP 7
int dm_hoglab_bin_table(void* host_u8_511x511);
size_t dm_hoglab_workspace_bytes(int B, int H, int W);
int dm_hoglab_cells(void* stream, const void* images_u8, int B, int H, int W, const void* bins_u8, float* hog_cells_f32,
                    float* lab_cells_f32);
int dm_hoglab_features(void* stream, const void* images_u8, int B, int H, int W, const void* bins_u8, void* out_f16_or_null,
                       float* raw_f32_or_null, void* work, size_t work_bytes);

/* ---- Doersch baseline: the detectors' linear SVMs, batched SMO (csrc/svm.hip) ---------------------------------------
 * `train_svm` (doersch/doersch.py:66-79) for K detectors at once: scikit-learn's SVC(C=cost, kernel='linear', shrinking=False).fit
 * as libsvm's Solver::Solve iterates it, step for step, then the hard negatives by decision_function > 0.  Stream-plus-workspace
 * functions (no engine handle).  rows_f16 [R][C] fp16 row-major is a pool of feature rows; detector k's samples are the pool rows
 * sample_i32[k][0 .. n_i32[k]), the first n_pos_i32[k] of them labelled +1, the rest -1.  Detectors may share pool rows, list them
 * in any order and repeat one; nothing is copied into per-detector matrices.  sample_i32, alpha_f64, score_f64 and hard_i32 are
 * tables [K][ld]; n_i32, n_pos_i32, first_i32 and max_samples_i32 are device arrays [K].
 *
 * dm_svm_fit.  The solver works in libsvm's internal order (the negatives, in their own order, as y = +1, then the positives as
 * y = -1) and breaks ties by it: i = the LAST index of the largest violation, j = the LAST index of the lowest second-order gain.
 * alpha and G are fp64; QD_t = x_t . x_t in fp64; Q_i[t] = (float)(y_i y_t (x_i . x_t)) (libsvm's Qfloat); a dot is the sum of the
 * exact products of the fp16 values in fp64, in an order that depends on C alone; G_t += Q_i[t] d_alpha_i + Q_j[t] d_alpha_j in
 * fp64 without fused multiply-add.  Stop: Gmax + Gmax2 < eps, no j, or max_iter iterations (max_iter <= 0: libsvm's
 * max(10 000 000, 100 n)).  Outputs (device): w_f64 [K][C] = -sum_t alpha_t y_t x_t over the support vectors in ascending
 * internal index; b_f64 [K] = rho (the mean of y_t G_t over the free variables, else the midpoint of libsvm's ub / lb);
 * n_iter_i32 [K]; status_i32 [K] = DM_SVM_CONVERGED, DM_SVM_MAX_ITER, DM_SVM_NAN (a row with a NaN or an infinity; w and b are
 * NaN) or DM_SVM_BAD_LIST (n_pos < 1, n - n_pos < 1 or n > ld: nothing of the pool is read; or a sample outside [0, R): that row is
 * never dereferenced, the detector's other rows are read once and it stops before the first iteration; w and b are NaN); alpha_f64_or_null [K][ld], entry p = the alpha of sample p (slots from n on hold 0).  Every decision is made on the
 * device; the host enqueues a group of iterations and reads the K stop flags once per group, so the call synchronises `stream`
 * and returns with it synchronised.  work: dm_svm_workspace_bytes(K, ld) bytes (0 = bad arguments), 16-byte aligned, contents free.
 *
 * dm_svm_hard_negatives (doersch.py:75-78).  Per detector over the samples p in [first_i32[k], n_i32[k]): s_p = x_p . w_k + b_k in
 * fp64 (fp16 row value times fp64 weight, summed in an order that depends on C alone).  Admitted: s_p > 0.  hard_i32[k] = the
 * admitted p by descending s, ascending p among equals, at most max_samples_i32[k] of them; count_i32[k] = how many; slots from
 * count on hold -1.  score_f64[k][p] = s_p, NaN for p outside [first, n) and for a sample outside [0, R).  It does not synchronise.
 *
 * No floating-point atomics and no wait on another workgroup; every output of detector k depends on detector k's inputs alone:
 * not on K, on its place in the call or on the other detectors.
 * Refused without a launch (DM_SVM_E_*): a null required pointer; K outside [1, DM_SVM_MAX_DETECTORS]; C < 8, C % 8 != 0 or
 * C > DM_SVM_MAX_FEATURES (the hard negatives' score pass stages w in LDS as fp64: 8 C bytes, 64 KB at the limit; the fit stages
 * x_i as fp32, 4 C bytes); R < 1; ld < 2 or ld >= 2^24; cost or eps not > 0; a small workspace; rows_f16
 * or work not 16-byte aligned. */
#define DM_SVM_MAX_DETECTORS 128
#define DM_SVM_MAX_FEATURES 8192
#define DM_SVM_CONVERGED 0
#define DM_SVM_MAX_ITER 1
#define DM_SVM_NAN 2
#define DM_SVM_BAD_LIST 3
#define DM_SVM_E_NULL 1
#define DM_SVM_E_K 2
#define DM_SVM_E_C 3
#define DM_SVM_E_ROWS 4
#define DM_SVM_E_LD 5
#define DM_SVM_E_N_LARGE 6
#define DM_SVM_E_COST 7
#define DM_SVM_E_WORK 8
#define DM_SVM_E_ALIGN 9
#define DM_SVM_E_HIP 10
size_t dm_svm_workspace_bytes(int K, int n_max);
int dm_svm_fit(void* stream, const void* rows_f16, int R, int C, const int32_t* sample_i32, int ld, const int32_t* n_i32,
               const int32_t* n_pos_i32, int K, double cost, double eps, int max_iter, void* work, size_t work_bytes, double* w_f64,
               double* b_f64, int32_t* n_iter_i32, int32_t* status_i32, double* alpha_f64_or_null);
int dm_svm_hard_negatives(void* stream, const void* rows_f16, int R, int C, const int32_t* sample_i32, int ld, const int32_t* n_i32,
                          const int32_t* first_i32, const int32_t* max_samples_i32, int K, const double* w_f64, const double* b_f64,
                          void* work, size_t work_bytes, double* score_f64, int32_t* hard_i32, int32_t* count_i32);

/* Profiling support for bench.py: when enabled, every launch of the dominant (implicit-GEMM)
 * kernel is bracketed by hipEvents on the launch stream.  dm_prof_read synchronises and returns
 * the accumulated kernel milliseconds, launch count and algorithmic FLOPs since the last reset. */
int dm_prof_enable(dm_engine* e, int on);
/* Measurement only (bench.py's roofline; no product path calls it): the rate the matrix cores of this device sustain on
 * v_mfma_f32_16x16x32_f16 alone — the igemm tile's MFMA stream (8 waves per CU, 80 MFMAs per wave and step, 160 accumulator registers)
 * with nothing else in the loop, `steps` steps per CU, on random fp16 operands (zero_operands = 0) or zeros (1).  At the package power
 * cap the clock this returns is well below the nominal 2.4 GHz and depends on the operand statistics: it is the ceiling a
 * GEMM-shaped kernel can reach on real data (csrc/probe_peak.hip).  sclk_ghz (optional) = s_memtime ticks of one block per ns of wall time:
 * a diagnostic only — on the boxes of r06 it read ~0.5 x the clock amdsmi reports, so bench.py does not print it. */
int dm_measure_mfma_rate(void* stream, int steps, int zero_operands, double* tflops, double* sclk_ghz);
int dm_prof_read(dm_engine* e, double* igemm_ms, double* igemm_flops, int64_t* igemm_launches,
                 double* attn_ms, double* attn_flops, int64_t* attn_launches);
/* igemm_flops above counts the multiply-adds the launches EXECUTE.  With "up_fold" an Upsample2D + conv launch executes 4 / 9 of the
 * layer's definition (interpolate, then 9 taps: the count SURVEY 8d's 803.27 GFLOP per forward uses); this returns the difference
 * (definition minus executed) accumulated over the interval the last dm_prof_read closed, so a caller can quote either figure. */
int dm_prof_read_folded(dm_engine* e, double* igemm_flops_folded);

/* ---- VAE encoder -------------------------------------------------------------
 * Replaces `self.vae.encode(x).latent_dist.sample() * self.vae.config.scaling_factor`
 * (diffmining/typicality/compute.py:91-93, called at :137; dift.py:187) so the engine can start from
 * pixels.  Optional: an engine without VAE weights still scores latents.
 *
 * dm_engine_load_vae_weight: one tensor of `AutoencoderKL.state_dict()` by its diffusers name
 *   (`encoder.*`, `quant_conv.*`; an optional `vae.` prefix is stripped; `decoder.*` and
 *   `post_quant_conv.*` are accepted and ignored; the pre-0.15 attention names query/key/value/proj_attn
 *   and their [C,C,1,1] shapes are mapped to to_q/to_k/to_v/to_out.0).  Host memory, DM_F16 or DM_F32.
 * dm_engine_finalize_vae: checks the 108 encoder tensors (34,163,664 parameters), packs, uploads.
 * dm_vae_encode: image [batch,3,H,W] fp16 NCHW in [-1,1] (H, W >= 8; sizes that are not multiples of 8 floor at each of
 *   the three stride-2 stages like diffusers' Downsample2D(padding=0): the latent is floor(H/8) x floor(W/8)); `draws_per_image` D
 *   posterior samples per image from noise [batch*D,4,H/8,W/8] fp16 = the injected N(0,1) draws of
 *   `latent_dist.sample()` (NULL with D = 1 -> posterior mode, mean only).  D = 8 is the DIFT ensemble
 *   (dift.py:187,220 encode the same image 8 times; here the encoder runs once per image).
 *   Outputs (each optional, at least one): latents fp16 / fp32 [batch*D,4,H/8,W/8] (sample b*D+d belongs to
 *   image b) = (mean + exp(0.5 clamp(logvar,-30,20)) * noise) * scaling_factor, and the fp32 moments
 *   [batch,8,H/8,W/8] (mean | logvar) of `quant_conv(encoder(image))`.                               */
int dm_engine_load_vae_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype,
                              const int64_t* shape, int ndim);
int dm_engine_finalize_vae(dm_engine* e);
int dm_vae_encode(dm_engine* e, const void* image_dev, const void* noise_dev, int batch, int draws_per_image,
                  int H, int W, float scaling_factor, void* latent_f16_dev, void* latent_f32_dev,
                  void* moments_f32_dev, void* stream);

/* ---- Text-to-image sampling: guided DDIM loop and VAE decoder (csrc/sample.hip) ------------------------------------
 * Replaces `Trainer.sample` (finetuning/cars.py:235-255; the same call in ftt/geo/places and xray/finetune.py:228):
 * `StableDiffusionPipeline(prompt, negative_prompt, latents, num_inference_steps=50, eta=0.0, guidance_scale=7.5)` on a DDIMScheduler
 * under `torch.autocast('cuda')` with fp32 latents (`--mixed_precision no`), from the initial latents to uint8 images with nothing
 * leaving the device in between.  Optional: an engine without decoder weights still scores, and the loop needs only the U-Net.
 * Not covered: the `ddim=False` arm (the trainer's DDPM scheduler), fp16 latents (`--mixed_precision fp16`), the fp32 net.
 *
 * dm_engine_load_vae_decoder_weight: one tensor of `AutoencoderKL.state_dict()` by its diffusers name (`post_quant_conv.*`,
 *   `decoder.*`; the name rules of dm_engine_load_vae_weight: `vae.` prefix, pre-0.15 attention names and shapes; `encoder.*` and
 *   `quant_conv.*` are accepted and ignored).  A weight set of its own beside the encoder's.  Host memory, DM_F16 or DM_F32.
 * dm_engine_finalize_vae_decoder: checks the 140 decoder tensors (49,490,199 parameters), packs, uploads; an incomplete set is refused.
 * dm_vae_decode: latent [batch,4,h,w] fp32 NCHW -> `vae.decode(latent / scaling_factor).sample` in the arithmetic of dm_vae_encode
 *   (fp16 tensors, fp32 GroupNorm statistics): z = the correctly rounded fp32 quotient, rounded to fp16; post_quant_conv, conv_in, the mid
 *   block, four up blocks of three resnets (512, 512, 256, 128 channels, nearest-2x up-samplers between them); conv_norm_out + SiLU +
 *   conv_out + post-processing in one kernel that never writes the normalised [batch,8h,8w,128] tensor.  Outputs (each optional, at
 *   least one): raw [batch,3,8h,8w] fp16 NCHW = the sample; image [batch,8h,8w,3] uint8 = `VaeImageProcessor.postprocess`:
 *   (raw / 2 + 0.5).clamp(0, 1) in fp16, each operation rounded, widened to fp32, * 255, rounded half to even (NaN -> 0).  The batch is
 *   cut into chunks by image area (4 images of 512 x 512); a sample's bits do not depend on the batch.
 * dm_sample_run: n_steps guided DDIM updates of x [B,4,h,w] fp32 IN PLACE on the device queue.  t_host [n_steps] int64 (0..999) and
 *   coef_host [n_steps][4] fp32 = (sqrt(a_prev), sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev)) per step are HOST tables (the scheduler's
 *   0-dim fp32 tensors; the device computes no square root), uploaded once before the loop; slot_dev [2B] int32 on the device = the
 *   registered prompts of the B unconditional rows, then of the B conditional rows (`torch.cat([negative, prompt])`).  Per step:
 *   eps = UNet(cat([x, x]) rounded to fp16, t_i, slots) at batch 2B, then dm_op_cfg_ddim_step.  No host synchronisation inside the loop;
 *   the call waits for work queued on `stream` before its blocking uploads, and an engine runs its loops on one stream at a time (they
 *   share one table buffer).  Refused without a launch: n_steps <= 0, a timestep outside 0..999, 2B beyond one U-Net run (DM_CHUNK
 *   samples of 64 x 64, scaled by area), no prompts registered.  A sample's bits do not depend on B.                                    */
int dm_engine_load_vae_decoder_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_engine_finalize_vae_decoder(dm_engine* e);
int dm_vae_decode(dm_engine* e, const void* latent_f32_dev, int batch, int h, int w, float scaling_factor, void* raw_f16_out_dev,
                  void* image_u8_out_dev, void* stream);
int dm_sample_run(dm_engine* e, void* x_f32_dev, const int64_t* t_host, const float* coef_host, const int32_t* slot_dev, int B, int h, int w,
                  int n_steps, float guidance_scale, void* stream);

/* ---- CLIP text tower ----------------------------------------------------------
 * Replaces `self.clip(tokens.to(self.device))[0]` of `CategoryFeatures.embed`
 * (diffmining/typicality/compute.py:51; the pipeline's `text_encoder`, compute.py:68): CLIP ViT-L/14 text
 * model, token ids -> last_hidden_state.  Optional.  Tokenisation (BPE vocabulary) stays on the host.
 *
 * dm_engine_load_clip_weight: one tensor of `CLIPTextModel.state_dict()` (optional `text_encoder.` /
 *   `text_model.` prefixes are stripped; `position_ids` buffers are ignored).  Host memory, DM_F16 / DM_F32.
 * dm_engine_finalize_clip: checks the 196 tensors (123,060,480 parameters), packs, uploads.
 * dm_clip_encode: input_ids [n_prompts][seq_len = 77] int32 on the device (tokenizer output with
 *   padding="max_length") -> last_hidden_state [n_prompts][77][768] as fp16 and/or fp32 (the reference
 *   takes `.float()`).  The fp16 output is directly the `ctx` of dm_engine_set_prompts.               */
int dm_engine_load_clip_weight(dm_engine* e, const char* name, const void* host_ptr, int dtype,
                               const int64_t* shape, int ndim);
int dm_engine_finalize_clip(dm_engine* e);
int dm_clip_encode(dm_engine* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, void* out_f16_dev,
                   void* out_f32_dev, void* stream);

/* ---- DIFT patch descriptors ---------------------------------------------------
 * Replaces the per-patch tail of `Cluster.compute_embeddings` (diffmining/typicality/cluster.py:291-299):
 *   emb = emb[:, int(x0*H):int(x1*H), int(y0*W):int(y1*W)].mean(axis=(1,2)); emb / np.linalg.norm(emb)
 * for all patches of an image in one launch, from the ensemble-mean feature map dm_dift wrote
 * (feat [C,h,w] fp32).  boxes [n_patches][4] int32 = (r0, r1, c0, c1) in feature cells (numpy slice
 * semantics: clamped to the map; an empty window yields NaN).  out [n_patches][C] fp32.                 */
int dm_patch_embed(dm_engine* e, const void* feat_f32_dev, int C, int h, int w, const int32_t* boxes_dev,
                   int n_patches, void* out_f32_dev, void* stream);

/* Bytes of device memory currently held by the engine: packed weights (U-Net + optional VAE / CLIP slabs) and
 * the workspace arena (the per-prompt K/V cache, a few MB, is not included). */
int dm_engine_memory(dm_engine* e, size_t* weights_bytes, size_t* arena_bytes);

/* Steady-state contract ("no allocation on the steady-state path").  The engine allocates device memory in
 * three places only: weights at finalize, the per-prompt K/V cache when more prompts are registered than it holds
 * (capacity >= 16, doubling), and the workspace arena when a call needs more than it holds (exact peak from a dry run of
 * the schedule, done once per (batch, shape) and cached).  dm_engine_reserve pre-sizes the latter two for the largest
 * call the caller will make — a U-Net batch of up to `max_batch` samples (cut into DM_CHUNK-sized runs like the calls
 * themselves) of h x w latents scored under n_cond prompts per draw (n_cond <= 1: dm_score / dm_unet_forward / dm_dift),
 * and `max_prompts` registered prompts (call it before dm_engine_set_prompts: growing the cache drops its rows) — after
 * which no call within those bounds allocates.  dm_engine_stats reports how many device allocations and schedule dry runs
 * the engine has done so far, so a caller (tests/test_gpu_e2e.py::test_no_allocation_in_steady_state) can assert it, and how many
 * U-Net runs were replays of a captured hipGraph (option "graph" = 1: a run whose schedule key and pointer arguments repeat is
 * captured on its second occurrence and replayed from then on; needs a caller stream other than the legacy default stream and is
 * bypassed while dm_prof_enable is on, because a replay carries no per-launch events). */
int dm_engine_reserve(dm_engine* e, int max_batch, int max_h, int max_w, int n_cond, int max_prompts, void* stream);
int dm_engine_stats(dm_engine* e, int64_t* device_allocs, int64_t* schedule_dry_runs, int64_t* graph_launches);

/* ---- operator-level entry points ------------------------------------------------------------------
 * The individual gfx950 kernels behind the U-Net, exposed so that every op can be parity-tested
 * against the matching torch.nn.functional op.  All buffers are device
 * pointers; activations are NHWC fp16; weights are in the engine's packed layout:
 *   igemm : Y[m][co] = sum_k X~[m][k] Wp[co][k], k = (tap, cin); Wp [Cout][taps*Cin] fp16.
 *           mode 0 dense (1x1 conv / Linear), 1 conv3x3 s1 p1, 2 conv3x3 s2 p1,
 *           3 conv3x3 on the nearest-upsampled (OH x OW) image, 4 conv3x3 s2 on F.pad(x,(0,1,0,1))
 *           (VAE Downsample2D(padding=0)).  Cout must be a multiple of 160 (80-channel waves) or of
 *           128 (64-channel waves; VAE).  X2 = optional second source
 *           (channel concat cat([X, X2]), as the up blocks do).  epi 1 = GEGLU on quad-interleaved rows.
 *   attention : softmax(Q K^T * scale) V per head, head_dim D in {40, 80, 160}; strides in elements.
 *   groupnorm : (optionally concat) GroupNorm(G) (+SiLU), fp32 statistics; gamma/beta fp32.
 *   layernorm : per-row LayerNorm over C; gamma/beta fp32.                                        */
int dm_op_igemm(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb,
                const void* res, void* Y, int N, int H, int W, int C1, int C2, int Cout, int OH, int OW,
                int mode, int epi, int temb_ld);
/* Runtime switches for A/B measurements (process-wide; each defaults to the measured best and is initialised from the
 * environment variable DM_<NAME>).  Returns 1 for an unknown name and 2 for a value outside the switch's set (nothing changes then:
 * 0 / 1 / 2 for every switch, -1 too for "igemm_big", the list below for "attn_pipe"); an environment value outside the set is
 * reported on stderr and the default is kept.
 *   bit-neutral (the same arithmetic in the same order, asserted by tests/test_gpu_ops.py): "igemm_big" (-1 per shape /
 *     0 / 1: which tile geometry), "igemm_tail" (head / tail row split), "igemm_splitk" 0 vs 1 only for layers that
 *     do not split (a split layer sums its k parts in fp32 in a different order than the unsplit k loop);
 *   numerically equivalent but NOT bit-identical: "igemm_splitk" = 2 (four k parts instead of three tap-aligned ones),
 *     "ln_fold" (LayerNorm folded into the next GEMM: the rounding moves from the LN output to the folded weights),
 *     "attn_pipe" / "attn_cross" (pipelined / one-pass-softmax kernels vs the generic online-softmax kernel: different
 *     rescaling points), "ln_stats_g" (different lane order of the row reductions), "ln_inkernel" (0 / 1 / 2: LayerNorm
 *     statistics from a statistics kernel (two-pass) or inside the folded GEMM (one-pass fp32 sums; 1 = where cheaper));
 *   "gn_fold" (1 / 0): Transformer2D.norm folded into proj_in where the per-sample weights are <= 1/8 of a sample's activations (Cout * 8 <= H * W:
 *     the 320-channel level of latents >= 64x64, the 640-channel level of latents >= 144x144; per-sample weights; the rounding
 *     moves from the normalised activations to the scaled weights) — numerically equivalent, not bit-identical to 0;
 *   "sc_fold" (1 / 0): the ResNet blocks' conv_shortcut folded into conv2 as extra k steps wherever conv2 runs unsplit (one
 *     rounding of the sum instead of three) — numerically equivalent, not bit-identical to 0;
 *   "ff_fold" (1 / 0): ff.net.2 + residual + proj_out of a transformer block as one GEMM with the pre-multiplied weights Wp W2
 *     (the [tokens x C] intermediate and its fp16 rounding disappear) — numerically equivalent, not bit-identical to 0;
 *   "tap_reuse" (1 / 0 / 2): the 3x3 stride-1 convolutions of 64-pixel-wide images and the time-embedding ones (ResnetBlock2D.conv1)
 *     of 32-pixel-wide images (2: every eligible layer down to 16 pixels) run their k steps in the order
 *     (dy, 64-channel slab, dx) and fetch ONE activation stage per three horizontal taps (igemm_pers_tr.hip; the 128-row tile
 *     follows the same order, so the two tile kernels stay bit-identical) — numerically equivalent, not bit-identical to 0;
 *   "up_fold" (1 / 0): Upsample2D (nearest, exact 2x) + its 3x3 convolution as four 2x2 convolutions on the low-resolution source, one per
 *     output parity class, with the 3x3 taps that read the same source pixel pre-summed in fp32 and rounded to fp16 once (4 / 9 of the
 *     layer's MACs; the up-sampled tensor is never formed) — numerically equivalent, not bit-identical to 0; other sizes
 *     (F.interpolate(size=...) of odd latents) always run the unfolded layer;
 *   "q_once" (1 / 0 / 2): dm_score_conds — attn2.to_q of the first transformer block runs once per draw (its input is the same under every
 *     prompt) and the cross-attention reads the queries modulo the draw count; 2 also runs the two GEMMs that read the prefix's
 *     outputs as a residual once per prompt block against the per-draw rows, so two of the three stacking copies of the shared
 *     prefix disappear (measured +-0, hence not the default) — all bit-identical to 0;
 *   "attn_pipe" (1; 0 / 2 / 3 / 5 / 9 / 10 / 12 — any other value is refused): the head_dim-40 / 80 self-attention kernels: 1 = head_dim 40
 *     on attention_qk32.hip (r06: scores on 32x32x16 MFMAs, P moved to the PV layout by v_permlane16_swap), head_dim 80 on the
 *     software-pipelined kernel, and from 8192 keys the three-wave-set anti-phase kernel (attention_pp.hip, r05); 5 = attention_qk32.hip
 *     wherever it applies; 9 = the r04 pipelined kernels everywhere; 0 = the generic kernel; 2 = pipelined head_dim 40 only; 3 = head_dim 80
 *     with constant-chunk rows (A/B); 12 / 10 = the anti-phase kernel everywhere (three sets with / without static priorities).  9, 2, 10 and
 *     12 are bit-identical to each other for head_dim 40; 1 / 5 differ from them by the summation order of a score (k = 48 in one fp32
 *     chain instead of 64), at the same distance from fp32 SDPA.  (The two-set kernel and the timing-only ablation instantiations of
 *     r05 exist only in a -DDM_ATTN_PP_ABLATE debug build.)
 *   "gn_epi" (1 / 0): 1 = norm2's GroupNorm statistics as per-(64-row block, channel pair) sums written by conv1's epilogue where the
 *     persistent kernels run it and computed from conv1's output where they do not (bit-identical between the two, so independent of
 *     the batch); 0 = the statistics pass.  Numerically equivalent, not bit-identical to 0 (another summation order); -0.3 ms per step
 *     (DESIGN.md 4g);
 *   "conv_out_rows" (1 / 0): conv_out + eps-MSE with the input rows staged once in LDS and walked by all nine taps on the matrix cores
 *     (conv_out.hip) instead of the per-pixel gather (misc.hip) — equal to fp32 rounding, not bit-identical;
 *   "gn_skip" (1 / 0): 1 = the up path's norm1 over cat([x, skip]) sums x only and merges the skip's GroupNorm partial sums kept from the
 *     down path's norm1 of the same tensor (one read of the skip less, where the group widths nest) — numerically equivalent, not
 *     bit-identical to 0; a property of the network's channel counts, never of the batch;
 *   "graph" (0 / 1): replay whole U-Net runs as captured hipGraphs (bit-identical: the same kernels with the same arguments);
 *   "igemm_exp": experimental kernel paths of the current round (0 = shipped). */
int dm_set_option(const char* name, int value);
/* current value of a switch (bench.py prints the arithmetic rewrites a line was measured with); nonzero for an unknown name */
int dm_get_option(const char* name, int* value);

/* which tile geometry dm_op_igemm runs a shape on: 0 = 128-row tile (128x320 / 128x160), 1 = persistent 256x320 tile */
int dm_op_igemm_tile(int M, int Cin, int Cout, int mode);
/* rows [0, r) of such a launch run on the persistent 256x320 tile (whole rounds over the CUs), rows [r, M) on the
 * 128-row tile ("igemm_tail"; r = 0 / M: one kernel for all rows).  `spatial` = OH*OW of one sample (ignored for mode 0). */
int dm_op_igemm_head_rows(int M, int spatial, int Cin, int Cout, int mode);
/* channels of the longest row of ONE k-loop source (C1, C2, C3 or C4) the persistent 256x320 tile takes: its zero page, which halo
 * lanes walk at the pace of the tensor's lanes, is twice as many bytes; longer rows run on the 128-row tile */
int dm_op_igemm_pers_max_source_channels(void);
/* flash attention, head_dim 40 / 80 / 160: O[b] = softmax(scale Q[b] K[s]^T) V[s] per head, s = kv_slot[b] if kv_slot, else b */
int dm_op_attention(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv,
                    int ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot,
                    int B, int heads, int Tq, int Tk, int D, float scale);
/* the same with the engine's index rules: s = kv_slot[b] if kv_slot, else b / slot_div if slot_div > 0, else b; s clamped to
 * [0, n_slots) if n_slots > 0; sample b reads the queries of sample b % q_mod if q_mod > 0 (the shared-draw layout) */
int dm_op_attention_slots(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv,
                          int ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot, int slot_div, int n_slots,
                          int q_mod, int B, int heads, int Tq, int Tk, int D, float scale);
/* which kernel dm_op_attention runs a shape on under the current options (dm_set_option "attn_pipe" / "attn_cross"):
 * 0 = refused, 1 / 2 / 3 = generic head_dim 40 / 80 / 160, 4 = qk32, 5 = qk64, 6 = pipe (head_dim 40), 7 = pipe80,
 * 8 / 9 = anti-phase variants 10 / 12, 10 = d160, 11 = d160_cross, 12 = cross (77-key, head_dim 40 / 80) */
int dm_op_attention_route(int B, int heads, int Tq, int Tk, int D, int q_mod);
/* LayerNorm folded into a Linear (the transformer blocks' LN -> to_q/k/v, LN -> to_q, LN -> GEGLU projection):
 * dm_op_ln_stats writes (mean, rstd) per row of X [rows][C]; dm_op_igemm_ln computes
 *   Y[m][c] = rstd_m * (sum_k X[m][k] Wp[c][k] - mean_m * ln_s[c]) + ln_t[c]     (then GEGLU when epi = 1)
 * with Wp = fp16(W * gamma), ln_s[c] = sum_k Wp[c][k], ln_t[c] = sum_k W[c][k] beta[k] + bias[c]  (fp32).   */
int dm_op_ln_stats(void* stream, const void* X, int rows, int C, float eps, void* stats_f32);
int dm_op_igemm_ln(void* stream, const void* X, const void* Wp_folded, const void* ln_s, const void* ln_t,
                   const void* stats, void* Y, int M, int Cin, int Cout, int epi);
/* igemm with the k range cut into `ksplit` parts (>= 2, dividing the k steps) through an fp32 workspace of
 * ksplit * M * Cout floats, followed by the reduction + epilogue; the engine uses it for the 8x8 layers.   */
int dm_op_igemm_splitk(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb,
                       const void* res, void* Y, int N, int H, int W, int C1, int C2, int Cout, int OH, int OW,
                       int mode, int temb_ld, int ksplit, void* workspace_f32);
/* single-head attention with head_dim 512 (VAE mid block): Q/K/V [B][T][ld], O [B][T][ldo] */
int dm_op_attention512(void* stream, const void* Q, const void* K, const void* V, void* O, int B, int T, int ld,
                       int ldo, float scale);
int dm_op_groupnorm(void* stream, const void* X, const void* X2, int N, int HW, int C, int C1, int G, float eps,
                    const float* gamma, const float* beta, int silu, void* Y);
int dm_op_layernorm(void* stream, const void* X, int rows, int C, const float* gamma, const float* beta, float eps,
                    void* Y);
/* GroupNorm statistics as per-(64-row block, channel pair) fp32 sums (r05): blocks [rows / 64][C], entry (b, 2 k + {0, 1}) = (sum, sum of
 * squares) of channels 2 k, 2 k + 1 over rows 64 b .. 64 b + 63.  dm_op_gn_blocks computes the blocks of rows [row0, rows) from X [rows][C];
 * dm_op_conv_temb_gn_blocks is ResnetBlock2D.conv1 (3x3, + bias, + time-embedding row temb [N][temb_ld]) whose persistent kernels write the
 * blocks of the first *rows_done rows of Y from their epilogue (bit-identical to dm_op_gn_blocks on Y; 0 rows when another tile kernel takes
 * the launch); dm_op_groupnorm_blocks = the fixed-order fp64 combine + the apply (+ SiLU) — the path norm2 takes in the engine
 * (option "gn_epi").  rows % 64 == 0, HW % 64 == 0, C % 16 == 0, C / G even. */
/* conv_out (3x3, C0 -> 4, + bias, rounded to fp16 = `unet(...).sample`) on Xn [B,H,W,C0] fp16 NHWC with w [4][9*C0] (k = (tap, cin)): pred
 * [B,4,H,W] fp16 (optional) and, with eps [B,4,H,W] fp32, loss [B,4,H,W] fp32 = (pred - eps)^2 — the last two steps of SD.compute_loss
 * (compute.py:100-101).  Option "conv_out_rows" selects the kernel (1: input rows staged in LDS, conv_out.hip; 0: per-pixel gather). */
int dm_op_conv_out(void* stream, const void* Xn, const void* w, const void* bias, const float* eps, int B, int H, int W, int C0, float* loss,
                   void* pred);
int dm_op_conv_temb_gn_blocks(void* stream, const void* X, const void* Wp, const void* bias, const void* temb, void* Y, int N, int H, int W,
                              int Cin, int Cout, int temb_ld, float* blocks, int* rows_done);
int dm_op_gn_blocks(void* stream, const void* X, int rows, int C, int row0, float* blocks);
int dm_op_groupnorm_blocks(void* stream, const void* X, const float* blocks, int N, int HW, int C, int G, float eps, const float* gamma,
                           const float* beta, int silu, void* Y);
/* A GEMM with a second GEMM on another tensor folded into its k loop: after its own taps on X [N,H,W,Cin] (mode 1: 3x3 stride 1;
 * mode 0: dense) the loop runs a 1x1 convolution on cat([X3 (C3 channels), X4 (C4 channels)]) (same N, H, W).  Wp [Cout][taps*Cin + C3 + C4]:
 * the first GEMM's row (k = (tap, cin)) followed by the second's; bias = the sum of both; res = optional residual [M][Cout].
 * Used for ResnetBlock2D (out = conv_shortcut(x) + conv2(h)) and for ff.net.2 + residual + proj_out as one GEMM
 * ((Wp W2) f + Wp t2 + x).  Cout % 160 == 0; Cin, C3, C4 multiples of 64. */
int dm_op_igemm_shortcut(void* stream, const void* X, const void* X3, const void* X4, const void* Wp, const void* bias, const void* res,
                         void* Y, int N, int H, int W, int Cin, int C3, int C4, int Cout, int mode);
/* Upsample2D + conv (diffusers Upsample2D.forward: F.interpolate(scale_factor=2, mode="nearest") then Conv2d(3x3, padding 1)) folded onto
 * the source grid.  dm_op_fold_upconv_weights (host): w [Cout][Cin][3][3] fp16 -> W4 [4 = py*2+px][Cout][(a*2+b)*Cin + ci] fp16, entry =
 * fp16(fp32 sum of the 3x3 taps that read source pixel (y-1+py+a, x-1+px+b) for output pixel (2y+py, 2x+px)).
 * dm_op_upconv_folded (device): X [N][H][W][Cin], W4, bias [Cout] -> Y [N][2H][2W][Cout].  Cout % 320 == 0, Cin % 64 == 0. */
int dm_op_fold_upconv_weights(const void* w_oihw_f16_host, int Cout, int Cin, void* out_f16_host);
int dm_op_upconv_folded(void* stream, const void* X, const void* W4, const void* bias, void* Y, int N, int H, int W, int Cin, int Cout);
/* GroupNorm(G, eps) (no activation) folded into the following 1x1 convolution W [Cout][C] + bias (Transformer2DModel.norm ->
 * proj_in): statistics of X [N][HW][C], per-sample weights fp16(W diag(a_n)) and fp32 bias rows W b_n + bias, then the GEMM on
 * the raw X — Y [N][HW][Cout] fp16.  HW must be a multiple of 128, C of 64, Cout of 160. */
int dm_op_groupnorm_conv1x1(void* stream, const void* X, int N, int HW, int C, int G, float eps, const float* gamma,
                            const float* beta, const void* W, const void* bias, int Cout, void* Y);
/* The glue kernels around the matrix kernels, one launch each (fp16 tensors unless a float pointer says otherwise).  Every entry returns 1
 * WITHOUT launching for a null required pointer, a non-positive extent or the precondition named with it.
 *   time_gather    out [B][dim] = table [1000][dim] rows clamp(t[b], 0, 999), t int64
 *   silu           out[i] = x / (1 + exp(-x)), n elements
 *   im2col_in      scheduler.add_noise fused into conv_in's im2col: out [B*H*W][64], column c*9 + ky*3 + kx (< 36) = the zero-padded 3x3
 *                  patch of noisy = sa[t[b]] * x[x_index ? x_index[b] : b] + sb[t[b]] * eps[b] (x, eps NCHW [.,4,H,W], t clamped to
 *                  [0, 999]), columns 36..63 zero.  latent_f32 = 1: x / eps / sa / sb fp32, three fp32 roundings, then fp16 once; 0: all fp16,
 *                  every operation rounded to fp16.  sa = sb = NULL: the plain sample (eps, t unused).  Refused: exactly one of sa / sb
 *                  NULL; tables without eps or t
 *   nhwc_to_nchw   X [N][HW][C] -> Y [N][C][HW]; N <= 65535
 *   ensemble_mean  X [groups*ens][HW][C] fp16 -> Y [groups][C][HW] fp32, the mean over `ens` consecutive samples; ens >= 1, groups <= 65535
 *   im2col_rgb     x NCHW [B,3,H,W] -> out [B*H*W][64], column c*9 + ky*3 + kx (< 27), columns 27..63 zero
 *   posterior      quant_conv (qw [8][8], qb [8]) on the first 8 of the ldh channels of Hm [B*HW][ldh], rounded to fp16 = moments [B,8,HW]
 *                  (fp32 values, optional); latent32 / latent16 [B*draws,4,HW] = (mean + exp(0.5 clamp(logvar, -30, 20)) * noise) * scaling
 *                  with sample b*draws + d on image b's moments (noise NULL: the mode); ldh % 8 == 0, ldh >= 8, draws >= 1, an output
 *   clip_embed     out [rows][C] = tok [vocab][C] row clamp(ids[r], 0, vocab - 1) + pos [T][C] row r % T (one fp16 add); C % 8 == 0
 *   clip_attention causal self-attention on qkv [n*T][3*heads*64] (q pre-scaled) -> out [n*T][heads*64]; 1 <= T <= 80, heads >= 1
 *   quick_gelu     x * sigmoid(1.702 x) in place; n % 8 == 0
 *   f16_to_f32     y[i] = (float)x[i] */
int dm_op_time_gather(void* stream, const void* table, const int64_t* t, int B, int dim, void* out);
int dm_op_silu(void* stream, const void* in, void* out, int64_t n);
int dm_op_im2col_in(void* stream, const void* x, const int32_t* x_index, const void* eps, const int64_t* t, const void* sa, const void* sb,
                    int latent_f32, int B, int H, int W, void* out);
int dm_op_nhwc_to_nchw(void* stream, const void* X, int N, int HW, int C, void* Y);
int dm_op_ensemble_mean(void* stream, const void* X, int groups, int ens, int HW, int C, float* Y);
int dm_op_im2col_rgb(void* stream, const void* x, int B, int H, int W, void* out);
int dm_op_posterior(void* stream, const void* Hm, int ldh, const void* qw, const void* qb, const void* noise, int B, int draws, int HW,
                    float scaling, void* latent16, float* latent32, float* moments);
int dm_op_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, int rows, int T, int C, int vocab, void* out);
int dm_op_clip_attention(void* stream, const void* qkv, int n, int T, int heads, void* out);
int dm_op_quick_gelu(void* stream, void* x, int64_t n);
int dm_op_f16_to_f32(void* stream, const void* x, float* y, int64_t n);

/* The kernels of text-to-image sampling (csrc/sample.hip), one by one.  Each returns 1 WITHOUT launching for a null required pointer, a
 * non-positive extent or the precondition named with it.
 *   cfg_ddim_step    out [n] fp32 = one guided DDIM step of x [n] fp32 with eps [2n] fp16 (the n unconditional values first) and the row
 *                    coef4_dev = (c0, c1, c2, c3) on the device, in torch's type promotion of StableDiffusionPipeline.__call__ +
 *                    DDIMScheduler.step: e = rn16(u + rn16(g * rn16(c - u))); x0 = (x - rn16(c1 * e)) / c2; out = c0 * x0 + rn16(c3 * e) —
 *                    every fp16-tensor op an fp32 operation rounded to fp16, the scalars at fp32 precision, no FMA.  out may be x
 *   latent_prologue  latent NCHW fp32 [B,4,HW] -> out NHWC fp16 [B*HW][ldc]: channels 0..3 = post_quant_conv (w [4][4], b [4] fp16) of
 *                    rn16(latent / scaling_factor), the four products added in fp32 in input-channel order, then the bias, one rounding;
 *                    channels 4..ldc-1 zero.  ldc % 8 == 0, ldc >= 8, scaling_factor > 0
 *   decoder_tail     X [B,H,W,128] fp16 NHWC -> conv_out (Wp [3][9*128] fp16, k = (tap, channel); bias [3] fp16) of
 *                    silu(GroupNorm_32(X; gamma, beta fp32, eps)) with the normalised tensor never written: raw [B,3,H,W] fp16 NCHW and / or
 *                    image [B,H,W,3] uint8 as dm_vae_decode writes them (at least one).  work: dm_op_decoder_tail_workspace_bytes(B, H, W)
 *                    bytes on the device, 8-byte aligned (the statistics).  B <= 65535 */
int dm_op_cfg_ddim_step(void* stream, const float* x_f32, const void* eps_f16, const float* coef4_dev, float g, int64_t n, float* out_f32);
int dm_op_latent_prologue(void* stream, const float* latent_f32, const void* w_f16, const void* b_f16, int B, int HW, float scaling_factor,
                          void* out_f16, int ldc);
size_t dm_op_decoder_tail_workspace_bytes(int B, int H, int W);
int dm_op_decoder_tail(void* stream, const void* X, const float* gamma, const float* beta, const void* Wp, const void* bias, int B, int H, int W,
                       float eps, void* work, size_t work_bytes, void* raw_f16_out, void* image_u8_out);

/* ---- fp32 U-Net: the arithmetic of the reference's DIFT featuriser ------------------------------------------------------
 * `SDFeaturizer.__init__` (diffmining/typicality/dift.py:197-199) loads the pipeline WITHOUT torch_dtype and `forward`
 * (dift.py:214-232 -> OneStepSDPipeline.__call__, :173-193 -> MyUNet2DConditionModel.forward, :24-169) runs WITHOUT autocast:
 * every tensor and product of the DIFT path is fp32, unlike the typicality path (compute.py:98, fp16 autocast) that dm_engine
 * serves.  dm_f32_net is that second arithmetic: fp32 weights (values given as fp16 are widened exactly), fp32 NHWC
 * activations, fp32 matrix-core GEMMs (v_mfma_f32_16x16x4_f32, exact fp32 products) and attention.  Same U-Net, same
 * diffusers-named state dict, same prompt-slot mechanism as dm_engine; all *_dev tensors at this boundary are fp32.
 *   dm_f32_load_weight / dm_f32_finalize   replace from_pretrained's state-dict load (dift.py:197-199)
 *   dm_f32_set_prompts   ctx_dev [n_prompts,77,768] fp32 = `prompt_embeds` (dift.py:222-227); K/V of the 16 blocks per prompt
 *   dm_f32_dift          MyUNet2DConditionModel.forward(latents_noisy, t, [up_ft_index], prompt_embeds) (dift.py:24-169,191):
 *                        feat_out_dev [batch,C_i,h_i,w_i] fp32 NCHW and / or the mean over consecutive groups of `ensemble`
 *                        samples [batch/ensemble,C_i,h_i,w_i] (dift.py:231); shapes from dm_dift_shape()
 *   dm_f32_unet_forward  `unet(sample, t, encoder_hidden_states).sample` in fp32: out_dev [batch,4,h,w] — the full-size fp32
 *                        ground truth on the GPU for the fp16 engine's deviation measurements
 *   dm_f32_prof_*        as dm_prof_*: HIP events around every GEMM / attention launch, for bench.py's roofline leg */
typedef struct dm_f32_net dm_f32_net;
int dm_f32_create(int device, dm_f32_net** out);
void dm_f32_destroy(dm_f32_net* e);
const char* dm_f32_last_error(dm_f32_net* e);   /* e may be NULL: last create() error */
int dm_f32_load_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize(dm_f32_net* e);
int dm_f32_set_prompts(dm_f32_net* e, const void* ctx_dev, int n_prompts, void* stream);
int dm_f32_unet_forward(dm_f32_net* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch,
                        int h, int w, void* out_dev, void* stream);
int dm_f32_dift(dm_f32_net* e, const void* noisy_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
                int up_ft_index, void* feat_out_dev, void* mean_out_dev, int ensemble, void* stream);
/* SD.compute_loss (compute.py:95-102) with NO autocast: fp32 add_noise (x_dev [n_x,4,h,w], x_index_dev [batch] or NULL for identity,
 * eps_dev [batch,4,h,w], t_dev [batch]), fp32 U-Net, fp32 squared error -> loss_out_dev [batch,4,h,w] fp32: the exact-arithmetic
 * yardstick of dm_score (bench.py's `score_deviation`, tools/t_deviation_gpu.py). */
int dm_f32_score(dm_f32_net* e, const void* x_dev, const int32_t* x_index_dev, const void* eps_dev, const int64_t* t_dev,
                 const int32_t* slot_dev, int batch, int n_x, int h, int w, void* loss_out_dev, void* stream);
/* optional AutoencoderKL encoder in fp32: `pipe.vae.encode(img_tensor).latent_dist.sample() * scaling_factor` of the featuriser
 * (dift.py:187) — image_dev [batch,3,H,W] fp32 in [-1,1]; noise_dev [batch*draws_per_image,4,H/8,W/8] fp32 N(0,1) draws or NULL
 * (posterior mode); latent_dev [batch*draws_per_image,4,H/8,W/8] fp32 and / or moments_dev [batch,8,H/8,W/8] fp32 (either may be
 * NULL).  State-dict names as dm_engine_load_vae_weight (decoder tensors ignored, legacy attention names accepted). */
int dm_f32_load_vae_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize_vae(dm_f32_net* e);
int dm_f32_vae_encode(dm_f32_net* e, const void* image_dev, const void* noise_dev, int batch, int draws_per_image, int H, int W,
                      float scaling_factor, void* latent_dev, void* moments_dev, void* stream);
/* optional AutoencoderKL decoder in fp32, a weight set of its own: `vae.decode(1 / 0.18215 * latents).sample` of the parallel-dataset generator
 * (applications/parallel-dataset/pnp.py:137-142, :531-536; its pipelines have no torch_dtype and no autocast).  State-dict names:
 * `post_quant_conv.*` and `decoder.*` of a full AutoencoderKL state dict (140 tensors), optional `vae.` prefix, encoder tensors ignored, legacy
 * attention names accepted.  latent_dev [batch,4,h,w] fp32; z = latent * latent_scale (pass (float)(1 / 0.18215)); out_f32_dev [batch,3,8h,8w]
 * fp32 = the sample if raw, else `(sample / 2 + 0.5).clamp(0, 1)`; out_u8_dev [batch,8h,8w,3] uint8 = that image * 255, truncated as the
 * reference's `.astype(np.uint8)` (pnp.py:590-591).  Either output may be NULL, not both. */
int dm_f32_load_vae_decoder_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize_vae_decoder(dm_f32_net* e);
int dm_f32_vae_decode(dm_f32_net* e, const void* latent_dev, int batch, int h, int w, float latent_scale, int raw, void* out_f32_dev,
                      void* out_u8_dev, void* stream);
/* The generator's loops on the device queue (pnp.py:156-203, :538-577): no host synchronisation inside, tables uploaded and the arena sized
 * before the first step.  coef_host [n_steps][4] = (c0, c1, c2, c3) of x' = c0 * ((x - c1 * eps) / c2) + c3 * eps, built by the host as the
 * reference builds its scalars (fp32 torch, diff_mining_amd.pnp.ddim_coefficients); t_host [n_steps] = the timestep of every sample of step i.
 * dm_f32_unet_forward_inject: one forward with Plug-and-Play's injection, sample 0 = the source; mask bit 3 * res + block = up_blocks[res]
 * resnet (conv_mask) or attn1 (attn_mask) `block`, bits 12.. = the mid block's; at a masked resnet every sample's output is
 * shortcut(x_n) + the source's conv2 output, at a masked attn1 every sample attends with the source's queries and keys and its own values;
 * masks of 0 = dm_f32_unet_forward.  With a mask set the whole batch must fit one run.
 * dm_f32_ddim_run: x_dev [B,4,h,w] in / out; per step eps = UNet(x, t_i, prompt[slot_dev[b]]), the update, and, if save_row_host[i] >= 0, a copy
 * of the new x to row save_row_host[i] of traj_dev [rows][B,4,h,w] (both may be NULL).
 * dm_f32_pnp_run: B targets of one source.  src_dev [n_steps][4][h][w] = the source's latent at t_i; per step the batch [source, x, x] of
 * 1 + 2 B samples with slot_dev [1 + 2 B] = (source, B unconditional, B conditional prompts), the injected forward (conv_on_host[i] /
 * attn_on_host[i] switch the masks per step), eps = eps_u + g * (eps_c - eps_u), the update of x_dev [B,4,h,w].
 * Prompt slots live on the device, as for dm_f32_unet_forward: these entries cannot range-check them without a synchronisation and do not;
 * the attention kernels clamp a slot to the registered prompts (memory-safe), and the Python binding range-checks host-side slots before
 * the call (EngineError).  The loops of one net share its loop buffer and arena: a call waits for the work already queued on `stream` before
 * it uploads its tables (once, before its first step); use one stream at a time per net. */
int dm_f32_unet_forward_inject(dm_f32_net* e, const void* sample_dev, const int64_t* t_dev, const int32_t* slot_dev, int batch, int h, int w,
                               int conv_mask, int attn_mask, void* out_dev, void* stream);
int dm_f32_ddim_run(dm_f32_net* e, void* x_dev, const int64_t* t_host, const float* coef_host, const int32_t* slot_dev,
                    const int32_t* save_row_host, void* traj_dev, int B, int h, int w, int n_steps, void* stream);
int dm_f32_pnp_run(dm_f32_net* e, void* x_dev, const void* src_dev, const int64_t* t_host, const float* coef_host, const uint8_t* conv_on_host,
                   const uint8_t* attn_on_host, int conv_mask, int attn_mask, const int32_t* slot_dev, int B, int h, int w, int n_steps,
                   float guidance_scale, void* stream);
/* optional CLIP ViT-L/14 text tower in fp32: `pipe.encode_prompt(prompt, ...)[0]` of the featuriser (dift.py:222-226) — its pipeline is built
 * with no torch_dtype (dift.py:197-199), so `text_encoder(input_ids)[0]` is fp32 there; replaces transformers' CLIPTextModel.forward for that
 * call (12 layers, causal attention over 77 tokens, quick-GELU, final LayerNorm; fp32 GEMMs on the fp32 matrix cores).  State-dict names as
 * dm_engine_load_clip_weight (196 tensors; `text_model.` / `text_encoder.` prefixes and `position_ids` accepted).  input_ids_dev
 * [n_prompts, 77] int32 (tokenizer output, padding="max_length"); out_f32_dev [n_prompts, 77, 768] fp32 last_hidden_state. */
int dm_f32_load_clip_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize_clip(dm_f32_net* e);
int dm_f32_clip_encode(dm_f32_net* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, void* out_f32_dev, void* stream);
/* optional CLIP ViT-B/32 image tower in fp32: `CLIPModel("openai/clip-vit-base-patch32").get_image_features` of the clustering stage
 * (`Cluster.embed`, cluster.py:224-231; the reference loads it without a dtype and runs it without autocast) — CLIPVisionModelWithProjection:
 * stride-32 patch embedding (no bias), class token + position embedding, pre_layrnorm, 12 layers (LN1 -> q|k|v -> bidirectional attention
 * over 50 tokens x 12 heads of 64 -> out_proj + residual -> LN2 -> fc1 -> quick_gelu -> fc2 + residual), post_layernorm of the CLS token,
 * visual_projection 768 -> 512 (no bias); fp32 GEMMs on the fp32 matrix cores, calls split into runs of at most 512 images.
 * Weights: `CLIPVisionModelWithProjection` or full `CLIPModel` state-dict names (`vision_model.*`, `visual_projection.weight`;
 * `text_model.*`, `text_projection.weight`, `logit_scale` and `position_ids` are ignored); finalize checks all 200 tensors and shapes. */
int dm_f32_load_clip_vision_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize_clip_vision(dm_f32_net* e);
/* `CLIPImageProcessor` (PIL backend) of `batch` crops on the device, bit-equal to it: BICUBIC shortest-edge resize to 224 (PIL's 8-bit
 * two passes, a pass skipped when its axis keeps its size), center crop 224 x 224, `(u8.astype(float64) * (1/255)).astype(float32)`,
 * `(x - OPENAI_CLIP_MEAN) / OPENAI_CLIP_STD` in fp32.  images_u8_dev: uint8 HWC RGB images (any sizes) at desc.src_offset; desc.crop_*:
 * the crop in source pixels (col = PIL x); tables_dev: int32 BICUBIC tables (bounds [224][2] = window start relative to the crop, length;
 * weights [224][k] with 22 fraction bits) of the 224 output columns (xb_off, xk_off, stride kx) and rows (yb_off, yk_off, stride ky) the
 * crop keeps, built on the host (resample.bicubic_axis); flags: DM_CLIP_NEED_H / DM_CLIP_NEED_V, the passes PIL runs (a skipped pass
 * reads the crop from column `left` / row `top` on).  out_pixel_values_dev: fp32 [n_patches, 3, 224, 224]. */
#define DM_CLIP_NEED_H 1
#define DM_CLIP_NEED_V 2
typedef struct dm_clip_pre_desc {
    int64_t src_offset;                 /* bytes from images_u8_dev to the image's first pixel */
    int32_t src_w, src_h;
    int32_t crop_col0, crop_row0, crop_w, crop_h;
    int32_t left, top;                  /* center-crop offsets in the resized crop */
    int32_t kx, ky;                     /* weight row strides (max taps) */
    int32_t xb_off, xk_off, yb_off, yk_off;
    int32_t flags, pad;
} dm_clip_pre_desc;
int dm_f32_clip_preprocess(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                           int n_patches, void* out_pixel_values_dev, void* stream);
/* `get_image_features(pixel_values)` (normalize = 0) or that divided by its L2 norm (normalize = 1, `embed`'s
 * `features / features.norm(dim=-1, keepdim=True)`): pixel_values_dev fp32 [n, 3, 224, 224] -> out_f32_dev fp32 [n, 512] */
int dm_f32_clip_image_features(dm_f32_net* e, const void* pixel_values_dev, int n, int normalize, void* out_f32_dev, void* stream);
/* the vision transformer's last_hidden_state (before post_layernorm): pixel_values_dev [n, 3, 224, 224] -> out_f32_dev [n, 50, 768] */
int dm_f32_clip_vision_hidden(dm_f32_net* e, const void* pixel_values_dev, int n, void* out_f32_dev, void* stream);
/* dm_f32_clip_preprocess + dm_f32_clip_image_features in one call: the preprocessing writes the patch rows of the embedding GEMM
 * directly; bit-equal to the two calls */
int dm_f32_clip_patch_features(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                               int n_patches, int normalize, void* out_f32_dev, void* stream);
/* `CLIPTextModelWithProjection(input_ids).text_embeds` of the CLIP baseline (clipmining/ranking.py:58-64) on the fp32 text tower:
 * dm_f32_load_clip_weight accepts an optional 197th tensor `text_projection.weight` [768, 768] (without it everything behaves as before and this
 * entry fails).  The final-LayerNorm row at the first position of the largest id (`argmax(input_ids)`: the EOS token, so both of transformers'
 * pooling rules agree with it) times text_projection^T, divided by its L2 norm when normalize != 0.  input_ids_dev [n_prompts, 77] int32: the
 * reference pads with padding=True, the engine takes 77 ids — the tower is causal, so the EOS row does not see the padding.
 * out_f32_dev [n_prompts, 768]. */
int dm_f32_clip_text_embeds(dm_f32_net* e, const int32_t* input_ids_dev, int n_prompts, int seq_len, int normalize, void* out_f32_dev,
                            void* stream);
/* optional configurable CLIP image tower in fp32, beside the ViT-B/32 one (own weight set; nothing on that path changes): the patch tokens of
 * the CLIP baseline, `visual_projection(post_layernorm(vision_model(pixel_values).last_hidden_state[:, 1:, :]))` (ranking.py:66-70, StreetCLIP =
 * ViT-L/14-336: (1024, 4096, 24, 16, 336, 14, 768), 392 tensors).  The config is accepted only when hidden == heads * 64, hidden % 32 == 0,
 * intermediate % 32 == 0, projection_dim % 4 == 0 and image_size % patch_size == 0; finalize checks every tensor's shape against it (8 + 16 layers
 * tensors; names as dm_f32_load_clip_vision_weight).  G = image_size / patch_size, T = G^2 + 1 tokens; the patch rows of the embedding GEMM
 * are 3 patch_size^2 values padded with zeros to a multiple of 32 (588 -> 608); attention: heads of 64 on the fp32 MFMA flash kernel; calls
 * split into runs of 64 images, bit-equal whatever the split. */
typedef struct dm_clip_tower_config {
    int32_t hidden, intermediate, layers, heads, image_size, patch_size, projection_dim;
} dm_clip_tower_config;
int dm_f32_load_clip_tower_weight(dm_f32_net* e, const char* name, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int dm_f32_finalize_clip_tower(dm_f32_net* e, const dm_clip_tower_config* cfg);
/* The tower's processor, `CLIPImageProcessor(size={"shortest_edge": S}, do_center_crop=False)` (PIL backend), on SQUARE uint8 images, bit-equal
 * to it: descriptors and tables as dm_f32_clip_preprocess with crop = the whole image, left = top = 0 and tables of all S columns / rows
 * (resample.clip_tower_plan).  layout 0: out_dev = pixel_values [n, 3, S, S]; layout 1: the patch rows [n * G^2][KPAD], row = patch
 * (py * G + px), k = (c, ky, kx), columns 3 patch_size^2 .. KPAD - 1 written as zeros.  Needs the finalized tower (its config names S). */
int dm_f32_clip_tower_preprocess(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                                 int n, int layout, void* out_dev, void* stream);
/* pixel_values_dev [n, 3, S, S] -> out_tokens_dev [n, G^2, projection_dim] and / or out_hidden_dev [n, G^2 + 1, hidden] = last_hidden_state
 * (either may be NULL, not both) */
int dm_f32_clip_tower_tokens(dm_f32_net* e, const void* pixel_values_dev, int n, void* out_tokens_dev, void* out_hidden_dev, void* stream);
/* dm_f32_clip_tower_preprocess + dm_f32_clip_tower_tokens in one call (the preprocessing writes the patch rows); bit-equal to the two calls */
int dm_f32_clip_tower_image_tokens(dm_f32_net* e, const void* images_u8_dev, const dm_clip_pre_desc* descs_dev, const int32_t* tables_dev,
                                   int n, void* out_tokens_dev, void* stream);
int dm_f32_prof_enable(dm_f32_net* e, int on);
int dm_f32_prof_read(dm_f32_net* e, double* gemm_ms, double* gemm_flops, int64_t* gemm_launches, double* attn_ms,
                     double* attn_flops, int64_t* attn_launches);
int dm_f32_memory(dm_f32_net* e, size_t* weights_bytes, size_t* arena_bytes);
/* operator-level entry points of the fp32 kernels (parity tests): NHWC fp32 tensors; modes as dm_op_igemm (0 dense, 1 conv3x3,
 * 2 stride 2, 3 nearest-upsample to (OH, OW) + conv3x3, 4 stride 2 pad (0,1,0,1)); Wp [Cout][taps*Cin] k = (tap, cin); res [M][Cout] */
int dm_f32_op_gemm(void* stream, const void* X, const void* X2, const void* Wp, const void* bias, const void* temb, const void* res,
                   void* Y, int N, int H, int W, int OH, int OW, int Cin, int C1, int Cout, int mode, int temb_ld);
int dm_f32_op_attention(void* stream, const void* Q, const void* K, const void* V, void* O, int ldq, int ldk, int ldv, int ldo,
                        int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, const int32_t* kv_slot, int n_slots, int B, int heads,
                        int Tq, int Tk, int D, float scale);     /* D in {40, 64, 80, 160, 512} */
int dm_f32_op_groupnorm(void* stream, const void* X, const void* X2, int N, int HW, int C, int C1, int G, float eps,
                        const float* gamma, const float* beta, int silu, void* stats_work, void* Y);
int dm_f32_op_layernorm(void* stream, const void* X, int rows, int C, const float* gamma, const float* beta, float eps, void* Y);
/* the tower's patch-token head, first half: LayerNorm of rows 1 .. T-1 of every image (the CLS row skipped), X [n][T][C] -> Y [n*(T-1)][C] */
int dm_f32_op_clip_patch_ln(void* stream, const void* X, int n, int T, int C, const float* gamma, const float* beta, float eps, void* Y);
/* the generator's kernels one by one: the DDIM update out = c0 * ((x - c1 * eps) / c2) + c3 * eps on n elements, coef4 on the device, every
 * operation rounded on its own (out may be x); its guided form with eps = eps_u + g * (eps_c - eps_u); Y[b] = R[b] + Hs for B samples of `per`
 * elements; the decoder's tail (X NHWC [B,H,W,128], stats [B*32][2] from dm_f32_op_groupnorm's stats_work, Wp [3][9*128]) */
int dm_f32_op_ddim_step(void* stream, const void* x, const void* eps, const float* coef4, int64_t n, void* out);
int dm_f32_op_ddim_step_cfg(void* stream, const void* x, const void* eps_u, const void* eps_c, float g, const float* coef4, int64_t n, void* out);
int dm_f32_op_bcast_add(void* stream, const void* R, const void* Hs, int B, int64_t per, void* Y);
int dm_f32_op_decoder_tail(void* stream, const void* X, const void* stats, const float* gamma, const float* beta, const void* Wp, const float* bias,
                           int B, int H, int W, int C, int raw, void* out_f32, void* out_u8);
/* the two-kernel tail's convolution: X NHWC [B,H,W,C] (already normalised), Wp [Cout <= 8][9 C], Y NCHW [B,Cout,H,W] */
int dm_f32_op_conv_out(void* stream, const void* X, const void* Wp, const float* bias, int B, int H, int W, int C, int Cout, void* Y);
/* The fp32 net's glue kernels, one launch each, all tensors fp32; refusals as for the dm_op_* glue entries above.
 *   clip_embed / quick_gelu (in place) / silu / nhwc_to_nchw / ensemble_mean: as their fp16 namesakes (no C % 8 or n % 8 condition)
 *   clip_attention  heads of 64 on qkv [n*T][3*heads*64], q scaled by 1/8 inside: (T, causal) = (77, 1) or (50, 0), nothing else
 *   timestep_embed  out [B][dim] = [cos(t f_j) | sin(t f_j)], f_j = exp(-ln(10000) j / (dim/2)); dim even
 *   conv_in         x NCHW [B,Cin,H,W] (x) 3x3 pad 1 -> y NHWC [B,H,W,Cout]; w [(ci*3+dy)*3+dx][Cout], bias [Cout]
 *   add_noise       out[b] = sa[t[b]] * x[x_index ? x_index[b] : b] + sb[t[b]] * eps[b], `per` elements per sample, t clamped to [0, 999]
 *   sqerr           out = (pred - eps)^2
 *   posterior       Hm [B*HW][8]: moments [B,8,HW] and / or latent [B*draws,4,HW], as dm_op_posterior without the fp16 rounding */
int dm_f32_op_clip_embed(void* stream, const int32_t* ids, const void* tok, const void* pos, int rows, int T, int C, int vocab, void* out);
int dm_f32_op_clip_attention(void* stream, const void* qkv, int n, int T, int heads, int causal, void* out);
int dm_f32_op_quick_gelu(void* stream, void* x, int64_t n);
int dm_f32_op_silu(void* stream, const void* in, void* out, int64_t n);
int dm_f32_op_timestep_embed(void* stream, const int64_t* t, int B, int dim, void* out);
int dm_f32_op_conv_in(void* stream, const void* x, const void* w, const float* bias, int B, int Cin, int H, int W, int Cout, void* y);
int dm_f32_op_add_noise(void* stream, const void* x, const int32_t* x_index, const void* eps, const int64_t* t, const float* sa, const float* sb,
                        int B, int64_t per, void* out);
int dm_f32_op_sqerr(void* stream, const void* pred, const void* eps, int64_t n, void* out);
int dm_f32_op_nhwc_to_nchw(void* stream, const void* X, int N, int HW, int C, void* Y);
int dm_f32_op_ensemble_mean(void* stream, const void* X, int groups, int ens, int HW, int C, void* Y);
int dm_f32_op_posterior(void* stream, const void* Hm, const void* qw, const void* qb, const void* noise, int B, int draws, int HW, float scaling,
                        void* latent, void* moments);
/* Gradient operators of the fp32 net's convolutional blocks (ResnetBlock2D, Downsample2D, Upsample2D), all tensors fp32 NHWC, no
 * floating-point atomics: the same call gives the same bits.  The DATA gradient of a convolution is dm_f32_op_gemm itself on repacked
 * weights (train.py dgrad_weights); these are the rest.  Every entry returns 1 without launching on: a null required pointer, a
 * non-positive extent, a mode outside 0 .. 3, a channel count its kernel cannot take (named per entry), a workspace that is too small.
 *   gemm_wgrad   dWp [Cout][taps*Cin], k = (tap, cin) (the layout dm_f32_op_gemm reads) = sum over output pixels of dY [N,OH,OW,Cout] (x)
 *                im2col(X [N,H,W,C1] | X2 [N,H,W,Cin-C1]); modes 0 .. 3 and the (N, H, W, OH, OW) convention of dm_f32_op_gemm (mode 0:
 *                N*H*W rows, OH / OW ignored; mode 1 needs OH = H, OW = W; mode 2 OH = (H+1)/2, OW = (W+1)/2).  Cin % 32, C1 % 32, Cout % 4,
 *                X2 required when C1 < Cin.  The pixels are cut into slabs (a function of the pixel count alone); work receives one partial
 *                dWp per slab, work_bytes >= dm_f32_op_gemm_wgrad_workspace(...) (0 for arguments the kernel refuses); the partials are
 *                added in ascending slab order.  accumulate = 1: dWp += the finished gradient, one fp32 addition per element.
 *   colsum       out [N][C] = the sum of each sample's HW rows of dY [N*HW][C] (N = 1, HW = rows: dbias; per sample: the gradient into
 *                time_emb_proj), fp64 accumulators in a fixed order; C % 4; accumulate as above
 *   groupnorm_bwd  GroupNorm (+ SiLU when silu) backward over cat([X (C1), X2 (C - C1)]); stats [N*G][2] = the (mean, rstd) of
 *                dm_f32_op_groupnorm's stats_work; dY [N*HW][C]; writes dX [N*HW][C1], dX2 [N*HW][C-C1] (required when C1 < C),
 *                dgamma [C], dbeta [C]; work: 16 (N C + N G) bytes, 8-byte aligned; C % G == 0, C / G <= 256
 *   silu_bwd     dx = dy * silu'(x) on n elements
 *   zero_insert2 Z [N,H,W,C]: Z[2 oy][2 ox] = dY[oy][ox] of dY [N,(H+1)/2,(W+1)/2,C], zero elsewhere; C % 4
 *   nearest_bwd  dS [N,H,W,C]: every source pixel sums the pixels of dU [N,OH,OW,C] that mode 3's nearest rule maps to it
 *                (src = min(floor(dst * (float)H / (float)OH), H - 1)), in ascending destination order; C % 4 */
size_t dm_f32_op_gemm_wgrad_workspace(int N, int H, int W, int OH, int OW, int Cin, int Cout, int mode);
int dm_f32_op_gemm_wgrad(void* stream, const void* X, const void* X2, const void* dY, void* dWp, void* work, size_t work_bytes,
                         int N, int H, int W, int OH, int OW, int Cin, int C1, int Cout, int mode, int accumulate);
int dm_f32_op_colsum(void* stream, const void* dY, int N, int HW, int C, int accumulate, void* out);
int dm_f32_op_groupnorm_bwd(void* stream, const void* X, const void* X2, const void* dY, int N, int HW, int C, int C1, int G,
                            const float* gamma, const float* beta, const void* stats, int silu, void* work, size_t work_bytes,
                            void* dX, void* dX2, void* dgamma, void* dbeta);
int dm_f32_op_silu_bwd(void* stream, const void* x, const void* dy, void* dx, int64_t n);
int dm_f32_op_zero_insert2(void* stream, const void* dY, int N, int H, int W, int C, void* Z);
int dm_f32_op_nearest_bwd(void* stream, const void* dU, int N, int H, int W, int OH, int OW, int C, void* dS);
/* Gradient operators of the fp32 net's transformer blocks (LayerNorm, attention, GEGLU); the linear layers use dm_f32_op_gemm,
 * dm_f32_op_gemm_wgrad (mode 0) and dm_f32_op_colsum.  No floating-point atomics; every entry returns 1 without launching on arguments it
 * refuses.
 *   attention_bwd  dQ, dK, dV of O = softmax(Q K^T scale) V from Q, K, V, O, dO; row strides ld* and batch strides bs* in elements as
 *                dm_f32_op_attention, one per tensor in the HOST arrays ld8 / bs8 of eight entries each, in the order Q K V O dO dQ dK dV,
 *                so stacked q|k|v rows [tokens][3C] and k|v rows [B*Tk][2C] are read and written in place.  D in {40, 80, 160}.  Refused: any other
 *                D (64 and 512 included), a non-null kv_slot, a batch stride of 0, ld % 4 != 0 or bs % 4 != 0, ld < heads * D, a null or
 *                not 16-byte aligned pointer, heads > 65535 / B, work_bytes < dm_f32_op_attention_bwd_workspace(...) (which returns 0 for
 *                refused extents).  work starts with the statistics [B][heads][Tq][2] = (L, Delta), L = log2 sum_k 2^(s scale log2(e)),
 *                Delta = dO . O; behind them (rounded up to 16 bytes) lie the dK | dV partials [slabs][B][heads][Tk][2 D] of
 *                dm_f32_op_attention_bwd_slabs(Tq, Tk) query slabs (a function of Tq and Tk alone), added in ascending slab order.
 *                Every byte that is read is written first: the result does not depend on what work held.
 *   layernorm_bwd  dX [rows][C], dgamma [C], dbeta [C] of dm_f32_op_layernorm from X and dY; mean and rstd are recomputed per row with the
 *                forward kernel's expressions.  work: dm_f32_op_layernorm_bwd_workspace(rows, C) bytes, 8-byte aligned (fp64 partial
 *                sums per row slab, added in ascending order, then (mean, rstd) per row)
 *   geglu        Y [M][F] = h * gelu(g) of P [M][2F] = (h | g), gelu(g) = 0.5f g (1 + erff(g * 0.70710678f)) as dm_f32's fused GEMM
 *                epilogue computes it; F % 4 == 0
 *   geglu_bwd    dP [M][2F] = (dY gelu(g) | dY h (Phi(g) + g phi(g))) */
size_t dm_f32_op_attention_bwd_workspace(int B, int heads, int Tq, int Tk, int D);
int dm_f32_op_attention_bwd_slabs(int Tq, int Tk);
int dm_f32_op_attention_bwd(void* stream, const void* Q, const void* K, const void* V, const void* O, const void* dO, void* dQ, void* dK,
                            void* dV, const int32_t* ld8, const int64_t* bs8, const int32_t* kv_slot, int B, int heads, int Tq, int Tk,
                            int D, float scale, void* work, size_t work_bytes);
/* measurement only (tools/train_tfm_rate.py): the same call restricted to the kernels named by `phases` (bit 0 statistics, 1 dQ, 2 dK / dV
 * partials, 3 their sum; 1 .. 15), on a workspace that one full call has filled */
int dm_f32_op_attention_bwd_phases(void* stream, const void* Q, const void* K, const void* V, const void* O, const void* dO, void* dQ,
                                   void* dK, void* dV, const int32_t* ld8, const int64_t* bs8, const int32_t* kv_slot, int B, int heads,
                                   int Tq, int Tk, int D, float scale, void* work, size_t work_bytes, int phases);
size_t dm_f32_op_layernorm_bwd_workspace(int rows, int C);
int dm_f32_op_layernorm_bwd(void* stream, const void* X, const void* dY, int rows, int C, const float* gamma, float eps, void* work,
                            size_t work_bytes, void* dX, void* dgamma, void* dbeta);
int dm_f32_op_geglu(void* stream, const void* P, int M, int F, void* Y);
int dm_f32_op_geglu_bwd(void* stream, const void* P, const void* dY, int M, int F, void* dP);

#ifdef __cplusplus
}
#endif
#endif /* DM_ENGINE_H */
