// hoglab.hip — the Doersch-2012 baseline's HOG-LAB features from pixels (doersch/hog.py:24-87, `get_hoglab_single` +
// `normalize`): skimage.feature.hog(orientations=31, pixels_per_cell=(8, 8), cells_per_block=(8, 8), channel_axis=-1), the (a, b)
// planes of rgb2lab shrunk 8 : 1, the two concatenated per block of 8 x 8 cells, divided by their L2 norm and cast to fp16 — the
// [bc][br][2112] tensor dense_search.hip reads.
//
//   - hoglab_cell_kernel: one WAVE per 8 x 8 cell, one lane per pixel.  Central differences on the three channels in integers (0 on
//     the image's own first / last row and column; pixels past the 8-grid still feed their neighbours), the channel of the largest
//     g_row^2 + g_col^2 (the lowest among equals: strict >), the orientation bin from the host-built table `bins`
//     [(g_row + 255) 511 + g_col + 255] (fp32 atan2 misplaces integer gradients next to a bin edge), magnitude = sqrtf of the exact
//     integer.  The (bin, magnitude) pairs go to LDS; lane l sums bin l & 31 over pixels 32 (l >> 5) ... + 31 in ascending order in
//     fp64, the two halves are added (low + high) and rounded to fp32 once: the sum does not depend on anything but the cell's pixels.
//     The four lanes of pixels (3..4, 3..4) convert to Lab (sRGB -> linear by a 256-entry table rounded from fp64); lanes 0 / 1 store
//     ((p33 + p34) + (p43 + p44)) / 4 of a / b: the bilinear 64 -> 8 shrink with align_corners=False samples exactly there.
//   - hoglab_block_kernel: one workgroup per (image, block row p, tile of 16 block columns) stages cell rows p ... p + 7, columns
//     q0 ... q0 + 22 of both maps in LDS (at most 24.3 KB); its 8 waves take the blocks q in turn.  Lane l owns HOG values l + 64 t (t < 31;
//     consecutive lanes read consecutive LDS words) and Lab values l and l + 64.  Per block: sum of squares (31 fmaf per lane in
//     ascending t, then a fixed xor-shuffle tree 32, 16, ... 1, which leaves the same value in every lane), scale, clip at 0.2, second
//     sum, scale; Lab (m + 128) / 255; the overall sum of squares; the fp16 row goes through a per-wave LDS row so that every lane
//     stores 16 bytes (264 chunks of 8 values: 4 full rounds and 8 lanes of a fifth); raw fp32 values are stored 4 bytes per lane,
//     256 contiguous bytes per wave instruction.  The order of every sum depends on the lane and t alone.
// Nothing is atomic, nothing synchronises the stream, and no kernel reads an output.
#include "../../include/dm_engine.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dm {

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int kWave = 64;
constexpr int kBins = DM_HOGLAB_BINS;                  // 31
constexpr int kHog = 64 * kBins;                       // 1984 HOG values of a block
constexpr int kLab = 128;
constexpr int kFeat = DM_HOGLAB_FEATURE;               // 2112
constexpr int kChunks = kFeat / 8;                     // 264 stores of 16 bytes per fp16 row
constexpr int kCellWaves = 4;
constexpr int kBlockWaves = 8;
constexpr int kTileQ = 16;                             // block columns per workgroup
constexpr int kTileCols = kTileQ + 7;                  // cell columns staged
constexpr int64_t kMaxGroups = ((int64_t)1 << 32) / (kWave * kBlockWaves) - 1;   // workgroups of a launch: grid x block stays below 2^32 threads
constexpr int kRowHog = 8 * kBins;                     // 248: the HOG values one cell row gives a block
static_assert(kCellWaves <= kBlockWaves, "kMaxGroups is sized by the larger workgroup");
static_assert(kHog + kLab == kFeat && kHog == kWave * kBins && kFeat % 8 == 0, "feature layout");
static_assert(sizeof(float) * (8 * kTileCols * kBins + 2 * 8 * kTileCols) + sizeof(half8) * kBlockWaves * kChunks <= 64 * 1024,
              "static LDS of the block kernel");

// sRGB -> linear light of x / 255: ((x + 0.055) / 1.055)^2.4 above 0.04045, x / 12.92 below, in fp64, rounded to fp32
__device__ const float kSrgbLinear[256] = {
    0.f, 0.000303526991f, 0.000607053982f, 0.000910580973f, 0.00121410796f, 0.00151763496f, 0.00182116195f, 0.00212468882f,
    0.00242821593f, 0.0027317428f, 0.00303526991f, 0.00334653584f, 0.00367650739f, 0.00402471703f, 0.00439144205f, 0.00477695325f,
    0.00518151652f, 0.00560539169f, 0.00604883302f, 0.00651209056f, 0.00699541019f, 0.00749903219f, 0.00802319311f, 0.00856812578f,
    0.00913405884f, 0.00972121768f, 0.010329823f, 0.0109600937f, 0.0116122449f, 0.012286488f, 0.0129830325f, 0.0137020834f,
    0.0144438436f, 0.0152085144f, 0.0159962941f, 0.0168073755f, 0.0176419541f, 0.01850022f, 0.0193823613f, 0.0202885624f,
    0.0212190095f, 0.0221738853f, 0.0231533665f, 0.0241576321f, 0.0251868591f, 0.0262412224f, 0.0273208916f, 0.02842604f,
    0.0295568351f, 0.0307134446f, 0.0318960324f, 0.0331047662f, 0.0343398079f, 0.0356013142f, 0.0368894488f, 0.0382043719f,
    0.0395462364f, 0.0409151986f, 0.0423114114f, 0.043735031f, 0.045186203f, 0.0466650873f, 0.0481718257f, 0.0497065671f,
    0.0512694567f, 0.0528606474f, 0.054480277f, 0.0561284907f, 0.0578054301f, 0.0595112368f, 0.0612460524f, 0.0630100146f,
    0.064803265f, 0.0666259378f, 0.0684781671f, 0.0703600943f, 0.0722718537f, 0.0742135718f, 0.0761853829f, 0.078187421f,
    0.0802198201f, 0.0822827071f, 0.0843762085f, 0.0865004584f, 0.0886555836f, 0.0908417106f, 0.0930589661f, 0.0953074694f,
    0.097587347f, 0.0998987257f, 0.102241732f, 0.104616486f, 0.107023105f, 0.10946171f, 0.111932427f, 0.114435375f,
    0.116970666f, 0.119538426f, 0.122138776f, 0.124771819f, 0.127437681f, 0.130136475f, 0.13286832f, 0.135633335f,
    0.138431609f, 0.141263291f, 0.144128472f, 0.147027269f, 0.149959788f, 0.152926147f, 0.155926466f, 0.158960834f,
    0.162029371f, 0.165132195f, 0.168269396f, 0.171441108f, 0.174647406f, 0.177888423f, 0.18116425f, 0.18447499f,
    0.187820777f, 0.191201687f, 0.194617838f, 0.198069319f, 0.20155625f, 0.205078736f, 0.208636865f, 0.212230757f,
    0.215860501f, 0.219526201f, 0.223227963f, 0.226965874f, 0.230740055f, 0.23455058f, 0.238397568f, 0.242281124f,
    0.246201321f, 0.25015828f, 0.254152089f, 0.258182853f, 0.262250662f, 0.266355604f, 0.270497799f, 0.274677306f,
    0.278894275f, 0.283148736f, 0.287440836f, 0.291770637f, 0.296138257f, 0.300543785f, 0.304987311f, 0.309468925f,
    0.313988715f, 0.318546772f, 0.323143214f, 0.327778101f, 0.332451522f, 0.337163627f, 0.341914415f, 0.346704066f,
    0.351532608f, 0.356400132f, 0.361306787f, 0.366252601f, 0.371237695f, 0.376262128f, 0.38132602f, 0.386429429f,
    0.391572475f, 0.396755219f, 0.401977777f, 0.407240212f, 0.412542611f, 0.417885065f, 0.423267663f, 0.428690493f,
    0.434153646f, 0.439657182f, 0.445201188f, 0.450785786f, 0.456411034f, 0.462076992f, 0.467783809f, 0.473531485f,
    0.479320168f, 0.48514995f, 0.491020858f, 0.496932983f, 0.502886474f, 0.50888133f, 0.514917672f, 0.520995557f,
    0.527115107f, 0.533276379f, 0.539479494f, 0.545724452f, 0.55201143f, 0.558340371f, 0.564711511f, 0.571124852f,
    0.577580452f, 0.584078431f, 0.590618849f, 0.597201765f, 0.603827357f, 0.610495567f, 0.617206573f, 0.623960376f,
    0.630757153f, 0.637596846f, 0.644479692f, 0.651405632f, 0.658374846f, 0.665387273f, 0.672443151f, 0.679542482f,
    0.686685324f, 0.693871737f, 0.701101899f, 0.708375752f, 0.715693474f, 0.723055124f, 0.730460763f, 0.73791039f,
    0.745404184f, 0.752942204f, 0.760524511f, 0.768151164f, 0.775822222f, 0.783537805f, 0.791297913f, 0.799102724f,
    0.806952238f, 0.814846575f, 0.822785735f, 0.830769897f, 0.838799f, 0.846873224f, 0.854992628f, 0.863157213f,
    0.871367097f, 0.8796224f, 0.887923121f, 0.896269381f, 0.904661179f, 0.913098633f, 0.921581864f, 0.930110872f,
    0.938685715f, 0.947306514f, 0.955973327f, 0.964686275f, 0.973445296f, 0.982250571f, 0.991102099f, 1.f,
};

__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + (float)(16.0 / 116.0); }

__device__ __forceinline__ void wave_sync() {          // LDS written by this wave is read by other lanes of this wave only
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_sum(float v) {   // the same tree, and so the same bits, in every lane
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(kWave * kCellWaves)
void hoglab_cell_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ bins, int H, int W, int nr, int nc,
                        int64_t n_cells_all, float* __restrict__ hog_cells, float* __restrict__ lab_cells) {
    __shared__ float s_mag[kCellWaves][kWave];
    __shared__ int s_bin[kCellWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t gid = (int64_t)blockIdx.x * kCellWaves + wave;
    if (gid >= n_cells_all) return;                    // no workgroup barrier anywhere: a wave may leave alone
    const int per = nr * nc;
    const int64_t b = gid / per;
    const int rem = (int)(gid - b * per), R = rem / nc, Cc = rem - R * nc;
    const int r = lane >> 3, c = lane & 7;
    const int y = 8 * R + r, x = 8 * Cc + c;           // y < 8 nr <= H, x < 8 nc <= W
    const uint8_t* im = images + b * ((int64_t)H * W * 3);
    const uint8_t* at = im + ((int64_t)y * W + x) * 3;
    const bool row_in = y > 0 && y < H - 1, col_in = x > 0 && x < W - 1;
    const int64_t row_step = (int64_t)W * 3;

    int best = -1, g_row = 0, g_col = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int gr = row_in ? (int)at[row_step + ch] - (int)at[ch - row_step] : 0;
        const int gc = col_in ? (int)at[3 + ch] - (int)at[ch - 3] : 0;
        const int m2 = gr * gr + gc * gc;
        if (m2 > best) { best = m2; g_row = gr; g_col = gc; }
    }
    s_mag[wave][lane] = sqrtf((float)best);            // an exact integer <= 130050: correctly rounded
    s_bin[wave][lane] = bins[(g_row + 255) * 511 + (g_col + 255)];
    wave_sync();

    const int bin = lane & 31, first = (lane >> 5) * 32;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) acc += s_bin[wave][first + k] == bin ? (double)s_mag[wave][first + k] : 0.0;
    const double high = __shfl_down(acc, 32);
    if (lane < kBins) hog_cells[gid * kBins + lane] = (float)(acc + high) * (1.0f / 64.0f);

    float la = 0.f, lb = 0.f;
    if ((r == 3 || r == 4) && (c == 3 || c == 4)) {
        const float rl = kSrgbLinear[at[0]], gl = kSrgbLinear[at[1]], bl = kSrgbLinear[at[2]];
        const float X = (0.412453f * rl + 0.357580f * gl + 0.180423f * bl) / 0.95047f;
        const float Y = 0.212671f * rl + 0.715160f * gl + 0.072169f * bl;
        const float Z = (0.019334f * rl + 0.119193f * gl + 0.950227f * bl) / 1.08883f;
        const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
        la = 500.0f * (fx - fy);
        lb = 200.0f * (fy - fz);
    }
    // lanes 27, 28, 35, 36 hold pixels (3, 3), (3, 4), (4, 3), (4, 4)
    const float a00 = __shfl(la, 27), a01 = __shfl(la, 28), a10 = __shfl(la, 35), a11 = __shfl(la, 36);
    const float b00 = __shfl(lb, 27), b01 = __shfl(lb, 28), b10 = __shfl(lb, 35), b11 = __shfl(lb, 36);
    if (lane < 2) {
        const float m = lane == 0 ? ((a00 + a01) + (a10 + a11)) * 0.25f : ((b00 + b01) + (b10 + b11)) * 0.25f;
        lab_cells[((b * 2 + lane) * nr + R) * nc + Cc] = m;
    }
}

__global__ __launch_bounds__(kWave * kBlockWaves)
void hoglab_block_kernel(const float* __restrict__ hog_cells, const float* __restrict__ lab_cells, int nr, int nc, int br, int bc,
                         int q_tiles, _Float16* __restrict__ out, float* __restrict__ raw) {
    __shared__ float s_hog[8 * kTileCols * kBins];     // [cell row i][cell column][bin]
    __shared__ float s_lab[2 * 8 * kTileCols];         // [channel][cell row i][cell column]
    __shared__ half8 s_row[kBlockWaves][kChunks];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    int64_t g = blockIdx.x;
    const int qt = (int)(g % q_tiles);
    g /= q_tiles;
    const int p = (int)(g % br);
    const int64_t b = g / br;
    const int q0 = qt * kTileQ, nq = min(kTileQ, bc - q0), cols = nq + 7;      // q0 + cols <= bc + 7 = nc
    const int row_len = cols * kBins;

#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float* src = hog_cells + ((b * nr + p + i) * nc + q0) * kBins;
        for (int k = tid; k < row_len; k += kWave * kBlockWaves) s_hog[i * row_len + k] = src[k];
    }
    for (int k = tid; k < 16 * cols; k += kWave * kBlockWaves) {
        const int ci = k / cols, col = k - ci * cols;  // ci = channel * 8 + cell row
        s_lab[k] = lab_cells[((b * 2 + (ci >> 3)) * nr + p + (ci & 7)) * nc + q0 + col];
    }
    __syncthreads();

    int off[kBins];                                    // value l + 64 t of a block: cell row i = v / 248, the rest runs along the row
#pragma unroll
    for (int t = 0; t < kBins; ++t) {
        const int v = lane + kWave * t, i = v / kRowHog;
        off[t] = i * row_len + (v - i * kRowHog);
    }
    const int lab_off = (lane >> 3) * cols + (lane & 7);
    _Float16* stage = (_Float16*)&s_row[wave][0];

    for (int ql = wave; ql < nq; ql += kBlockWaves) {
        const float* cell = s_hog + ql * kBins;
        float h[kBins];
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < kBins; ++t) {
            h[t] = cell[off[t]];
            s = fmaf(h[t], h[t], s);
        }
        const float inv1 = 1.0f / sqrtf(wave_sum(s) + 1e-10f);
        s = 0.f;
#pragma unroll
        for (int t = 0; t < kBins; ++t) {
            h[t] = fminf(h[t] * inv1, 0.2f);
            s = fmaf(h[t], h[t], s);
        }
        const float inv2 = 1.0f / sqrtf(wave_sum(s) + 1e-10f);
        s = 0.f;
#pragma unroll
        for (int t = 0; t < kBins; ++t) {
            h[t] *= inv2;
            s = fmaf(h[t], h[t], s);
        }
        const float l0 = (s_lab[lab_off + ql] + 128.0f) / 255.0f;
        const float l1 = (s_lab[8 * cols + lab_off + ql] + 128.0f) / 255.0f;
        s = fmaf(l0, l0, s);
        s = fmaf(l1, l1, s);

        const int64_t row = (b * bc + q0 + ql) * br + p;
        if (raw) {
            float* o = raw + row * kFeat;
#pragma unroll
            for (int t = 0; t < kBins; ++t) o[lane + kWave * t] = h[t];
            o[kHog + lane] = l0;
            o[kHog + kWave + lane] = l1;
        }
        if (out) {
            const float inv3 = 1.0f / sqrtf(wave_sum(s));      // the Lab part is positive: never zero
#pragma unroll
            for (int t = 0; t < kBins; ++t) stage[lane + kWave * t] = (_Float16)(h[t] * inv3);
            stage[kHog + lane] = (_Float16)(l0 * inv3);
            stage[kHog + kWave + lane] = (_Float16)(l1 * inv3);
            wave_sync();
            half8* o = (half8*)(out + row * kFeat);
#pragma unroll
            for (int k = 0; k < kChunks / kWave; ++k) o[lane + kWave * k] = s_row[wave][lane + kWave * k];
            if (lane < kChunks % kWave) o[lane + kWave * (kChunks / kWave)] = s_row[wave][lane + kWave * (kChunks / kWave)];
            wave_sync();                               // the next block of this wave rewrites the row
        }
    }
}

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }
inline size_t hog_cells_bytes(int B, int nr, int nc) { return (size_t)B * nr * nc * kBins * sizeof(float); }
inline size_t lab_cells_bytes(int B, int nr, int nc) { return (size_t)B * 2 * nr * nc * sizeof(float); }

int check_shape(int B, int H, int W) {
    if (B < 1) return DM_HOGLAB_E_BATCH;
    if (H < 64 || W < 64 || H > DM_HOGLAB_MAX_SIDE || W > DM_HOGLAB_MAX_SIDE) return DM_HOGLAB_E_SIDE;
    const int64_t blocks = (int64_t)(H / 8 - 7) * (W / 8 - 7);
    if (blocks > (1 << 24) - 1) return DM_HOGLAB_E_BLOCKS;
    return 0;
}

int launch_cells(hipStream_t s, const void* images, int B, int H, int W, const void* bins, float* hog_cells, float* lab_cells) {
    const int nr = H / 8, nc = W / 8;
    const int64_t n_cells_all = (int64_t)B * nr * nc;
    const int64_t blocks = (n_cells_all + kCellWaves - 1) / kCellWaves;
    if (blocks > kMaxGroups) return DM_HOGLAB_E_BATCH;
    hipLaunchKernelGGL(hoglab_cell_kernel, dim3((unsigned)blocks), dim3(kWave * kCellWaves), 0, s, (const uint8_t*)images,
                       (const uint8_t*)bins, H, W, nr, nc, n_cells_all, hog_cells, lab_cells);
    return hipGetLastError() != hipSuccess ? DM_HOGLAB_E_HIP : 0;
}

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

int dm_hoglab_bin_table(void* host_u8_511x511) {
    if (!host_u8_511x511) return DM_HOGLAB_E_NULL;
    uint8_t* t = (uint8_t*)host_u8_511x511;
    const double per = 180.0 / 31;
    for (int gr = -255; gr <= 255; ++gr)
        for (int gc = -255; gc <= 255; ++gc) {
            double o = fmod(atan2((double)gr, (double)gc) * (180.0 / M_PI), 180.0);
            if (o < 0.0) o += 180.0;                   // numpy's %: the sign of the divisor
            int bin = 255;                             // no bin holds o: cannot happen for integer gradients (o <= 180 - 0.22)
            for (int i = 0; i < kBins; ++i)
                if (per * i <= o && o < per * (i + 1)) { bin = i; break; }
            t[(gr + 255) * 511 + (gc + 255)] = (uint8_t)bin;
        }
    return 0;
}

size_t dm_hoglab_workspace_bytes(int B, int H, int W) {
    if (check_shape(B, H, W)) return 0;
    return round256(hog_cells_bytes(B, H / 8, W / 8)) + round256(lab_cells_bytes(B, H / 8, W / 8));
}

int dm_hoglab_cells(void* stream, const void* images_u8, int B, int H, int W, const void* bins_u8, float* hog_cells_f32,
                    float* lab_cells_f32) {
    if (!images_u8 || !bins_u8 || !hog_cells_f32 || !lab_cells_f32) return DM_HOGLAB_E_NULL;
    if (const int rc = check_shape(B, H, W)) return rc;
    if (((uintptr_t)hog_cells_f32 | (uintptr_t)lab_cells_f32) & 3) return DM_HOGLAB_E_ALIGN;
    return launch_cells((hipStream_t)stream, images_u8, B, H, W, bins_u8, hog_cells_f32, lab_cells_f32);
}

int dm_hoglab_features(void* stream, const void* images_u8, int B, int H, int W, const void* bins_u8, void* out_f16_or_null,
                       float* raw_f32_or_null, void* work, size_t work_bytes) {
    if (!images_u8 || !bins_u8 || !work || (!out_f16_or_null && !raw_f32_or_null)) return DM_HOGLAB_E_NULL;
    if (const int rc = check_shape(B, H, W)) return rc;
    const int nr = H / 8, nc = W / 8, br = nr - 7, bc = nc - 7;
    const int q_tiles = (bc + kTileQ - 1) / kTileQ;
    const int64_t groups = (int64_t)B * br * q_tiles;
    if (groups > kMaxGroups || ((int64_t)B * nr * nc + kCellWaves - 1) / kCellWaves > kMaxGroups) return DM_HOGLAB_E_BATCH;
    if (work_bytes < round256(hog_cells_bytes(B, nr, nc)) + round256(lab_cells_bytes(B, nr, nc))) return DM_HOGLAB_E_WORK;
    if (((uintptr_t)out_f16_or_null | (uintptr_t)raw_f32_or_null | (uintptr_t)work) & 15) return DM_HOGLAB_E_ALIGN;
    float* hog_cells = (float*)work;
    float* lab_cells = (float*)((char*)work + round256(hog_cells_bytes(B, nr, nc)));
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = launch_cells(s, images_u8, B, H, W, bins_u8, hog_cells, lab_cells)) return rc;
    hipLaunchKernelGGL(hoglab_block_kernel, dim3((unsigned)groups), dim3(kWave * kBlockWaves), 0, s, (const float*)hog_cells,
                       (const float*)lab_cells, nr, nc, br, bc, q_tiles, (_Float16*)out_f16_or_null, raw_f32_or_null);
    return hipGetLastError() != hipSuccess ? DM_HOGLAB_E_HIP : 0;
}

}  // extern "C"
