// clipmine.hip — the CLIP baseline's patch mining (clipmining/ranking.py:72-108, `CLIPRankCluster.dot_text_image`) from the token grid
// (DESIGN.md 4u).  The reference upsamples the 2-channel score grid and all E feature channels bilinearly to the image size, pools the
// scores with a kx x ky window, takes topk(100 k_per_image), runs `get_non_overlapping` and averages the upsampled features over every
// winner's box.  Upsampling, pooling and the box mean are linear and separable, so with the per-image tables
//   A [OH][gh]: A[i][p] = mean over image rows i ... i+kx-1 of the bilinear row weights onto token row p     (B [OW][pw] for columns)
// both the pooled map and a box's feature are A X B^T on the gh x pw grid; the upsampled tensors are never formed.  Four kernels:
//   score    s[c][p][q] = text[c] . tokens[pq] / |tokens[pq]|                          one wave per token
//   map      D[i][j] = sum_q (sum_p A[i][p] s[p][q]) B[j][q]  (diff: channel 0 - channel 1)  one workgroup per map row
//   select   mine_select_kernel's rounds plus the eligibility rule: only the n = min(100 k_per_image, OH OW) best are candidates
//   feature  f[e] = sum_p sum_q A[i][p] B[j][q] tokens[pq][e], then f / |f|             one workgroup per (image, slot)
// All fp32, every sum in a fixed order (p, q ascending; lane-strided partials + an xor-shuffle tree; waves folded in index order), no
// floating-point atomics; what image b gets depends on image b alone.
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

#include <vector>

namespace dm {

namespace {

constexpr int kScoreWaves = 4;                 // tokens per 256-thread block of the score kernel
constexpr int kMapThreads = 256;
constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kFeatThreads = 256;
constexpr int kFeatWaves = kFeatThreads / 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// s[c][t] = (text[c] . v) / |v| for token t of image blockIdx.y: lane-strided partial sums over e, then the xor tree.
__global__ __launch_bounds__(kScoreWaves * 64)
void clipmine_score_kernel(const float* __restrict__ tokens, const float* __restrict__ text, int E,
                           const dm_clipmine_desc* __restrict__ desc, float* __restrict__ work) {
    const dm_clipmine_desc d = desc[blockIdx.y];
    const int lane = threadIdx.x & 63, t = blockIdx.x * kScoreWaves + (threadIdx.x >> 6);
    if (t >= d.P) return;
    const float* __restrict__ v = tokens + d.token_offset + (size_t)t * E;
    float ss = 0.f, d0 = 0.f, d1 = 0.f;
    for (int e = lane; e < E; e += 64) {
        const float x = v[e];
        ss += x * x;
        d0 += x * text[e];
        d1 += x * text[E + e];
    }
    ss = wave_sum(ss); d0 = wave_sum(d0); d1 = wave_sum(d1);
    if (lane == 0) {
        const float nrm = sqrtf(ss);
        float* __restrict__ s = work + d.work_offset;
        s[t] = d0 / nrm;
        s[d.P + t] = d1 / nrm;
    }
}

// Row i of image blockIdx.y's map: T[c][q] = sum_p A[i][p] s[c][p][q] into LDS, then D[i][j] = sum_q T[c][q] B[j][q].
__global__ __launch_bounds__(kMapThreads)
void clipmine_map_kernel(const dm_clipmine_desc* __restrict__ desc, const float* __restrict__ tables, int kx, int ky, int diff,
                         float* __restrict__ work, float* __restrict__ maps_out) {
    __shared__ float T[2][DM_CLIPMINE_MAX_GRID];
    const dm_clipmine_desc d = desc[blockIdx.y];
    const int OH = d.H - kx + 1, OW = d.W - ky + 1, gh = d.gh, pw = d.pw, i = blockIdx.x;
    if (i >= OH) return;
    const float* __restrict__ s = work + d.work_offset;
    const float* __restrict__ A = tables + d.a_offset + (size_t)i * gh;
    const float* __restrict__ B = tables + d.b_offset;
    for (int q = threadIdx.x; q < pw; q += kMapThreads) {
        float t0 = 0.f, t1 = 0.f;
        for (int p = 0; p < gh; ++p) {
            const float a = A[p];
            t0 += a * s[p * pw + q];
            if (diff) t1 += a * s[d.P + p * pw + q];
        }
        T[0][q] = t0; T[1][q] = t1;
    }
    __syncthreads();
    float* __restrict__ row = work + d.work_offset + 2 * (size_t)d.P + (size_t)i * OW;
    float* __restrict__ row_out = maps_out ? maps_out + d.map_offset + (size_t)i * OW : nullptr;
    for (int j = threadIdx.x; j < OW; j += kMapThreads) {
        const float* __restrict__ Bj = B + (size_t)j * pw;
        float m0 = 0.f, m1 = 0.f;
        for (int q = 0; q < pw; ++q) {
            const float b = Bj[q];
            m0 += T[0][q] * b;
            if (diff) m1 += T[1][q] * b;
        }
        const float v = diff ? m0 - m1 : m0;
        row[j] = v;
        if (row_out) row_out[j] = v;
    }
}

// Order-preserving image of a non-NaN fp32 in uint32 (-0 folded onto +0); no non-NaN value maps to 0.
__device__ __forceinline__ unsigned clipmine_key_bits(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ unsigned long long clipmine_key(float v, int idx) {
    return ((unsigned long long)clipmine_key_bits(v) << 32) | (unsigned)~(unsigned)idx;
}

// One workgroup per image; mine_select_kernel's rounds (64-bit key = value image | ~index: the best value, the lowest row-major index
// among equals; 0 = no candidate; NaN never selected) with the reference's eligibility rule on top: the candidates are the n_elig keys
// of highest rank only.  Keys are unique, so a round's winner w is eligible iff fewer than n_elig keys are greater than key_w — one
// integer counting pass per round.  The best alive candidate being ineligible means every alive one is: the image ran out.
__global__ __launch_bounds__(kSelThreads)
void clipmine_select_kernel(const dm_clipmine_desc* __restrict__ desc, const float* __restrict__ work, int kx, int ky, int k_per_image,
                            int32_t* __restrict__ boxes, float* __restrict__ d_out, int32_t* __restrict__ count) {
    __shared__ unsigned long long wave_best[kSelWaves];
    __shared__ int wave_cnt[kSelWaves];
    __shared__ int win_i[DM_MINE_MAX_K], win_j[DM_MINE_MAX_K];
    const dm_clipmine_desc d = desc[blockIdx.x];
    const int OH = d.H - kx + 1, OW = d.W - ky + 1, n = OH * OW;
    const int n_elig = 100 * k_per_image < n ? 100 * k_per_image : n;
    const float* __restrict__ dm = work + d.work_offset + 2 * (size_t)d.P;
    boxes += (size_t)blockIdx.x * k_per_image * 4;
    d_out += (size_t)blockIdx.x * k_per_image;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int taken = 0;
    for (int r = 0; r < k_per_image; ++r) {
        unsigned long long best = 0ull;
        for (int idx = tid; idx < n; idx += kSelThreads) {
            const float v = dm[idx];
            if (v != v) continue;
            const unsigned long long key = clipmine_key(v, idx);
            if (key <= best) continue;                     // the zone test only for a candidate that would lead
            const int i = idx / OW, j = idx - i * OW;
            bool is_free = true;
            for (int t = 0; t < r; ++t) {
                const int di = i - win_i[t], dj = j - win_j[t];
                if (di <= kx && di >= -kx && dj <= ky && dj >= -ky) { is_free = false; break; }
            }
            if (is_free) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned hi = __shfl_xor((unsigned)(best >> 32), o), lo = __shfl_xor((unsigned)best, o);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other > best ? other : best;
        }
        if (lane == 0) wave_best[wv] = best;
        __syncthreads();
        unsigned long long b = wave_best[0];
#pragma unroll
        for (int t = 1; t < kSelWaves; ++t) b = wave_best[t] > b ? wave_best[t] : b;
        if (b == 0ull) break;                              // nothing alive (uniform over the workgroup)
        int above = 0;                                     // keys that outrank the winner, alive or not
        for (int idx = tid; idx < n; idx += kSelThreads) {
            const float v = dm[idx];
            if (v == v && clipmine_key(v, idx) > b) ++above;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
        if (lane == 0) wave_cnt[wv] = above;
        __syncthreads();
        above = 0;
#pragma unroll
        for (int t = 0; t < kSelWaves; ++t) above += wave_cnt[t];
        if (above >= n_elig) break;                        // the winner is outside the top n: no eligible candidate is alive
        const int idx = (int)~(unsigned)b;
        const int i = idx / OW, j = idx - i * OW;
        if (tid == 0) {
            win_i[r] = i; win_j[r] = j;
            boxes[r * 4 + 0] = i; boxes[r * 4 + 1] = j; boxes[r * 4 + 2] = i + kx; boxes[r * 4 + 3] = j + ky;
            d_out[r] = dm[idx];
        }
        taken = r + 1;
        __syncthreads();                                   // winners visible, wave_best / wave_cnt free for the next round
    }
    for (int t = taken + tid; t < k_per_image; t += kSelThreads) {
        boxes[t * 4 + 0] = -1; boxes[t * 4 + 1] = -1; boxes[t * 4 + 2] = -1; boxes[t * 4 + 3] = -1;
        d_out[t] = __uint_as_float(0x7FC00000u);
    }
    if (tid == 0) count[blockIdx.x] = taken;
}

// Slot blockIdx.x of image blockIdx.y: threads along e (coalesced token reads), the grid in p, q ascending order, zero weights
// skipped (the same for every thread), the weight A[i][p] B[j][q] rounded once.  Then |f| by a fixed tree and f / |f|.
__global__ __launch_bounds__(kFeatThreads)
void clipmine_feature_kernel(const float* __restrict__ tokens, int E, const dm_clipmine_desc* __restrict__ desc,
                             const float* __restrict__ tables, int k_per_image, const int32_t* __restrict__ boxes,
                             const int32_t* __restrict__ count, float* __restrict__ feats) {
    __shared__ float wave_ss[kFeatWaves];
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    float* __restrict__ out = feats + ((size_t)b * k_per_image + r) * E;
    if (r >= count[b]) {
        for (int e = tid; e < E; e += kFeatThreads) out[e] = __uint_as_float(0x7FC00000u);
        return;
    }
    const dm_clipmine_desc d = desc[b];
    const int gh = d.gh, pw = d.pw;
    const int32_t* box = boxes + ((size_t)b * k_per_image + r) * 4;
    const float* __restrict__ A = tables + d.a_offset + (size_t)box[0] * gh;
    const float* __restrict__ B = tables + d.b_offset + (size_t)box[1] * pw;
    const float* __restrict__ tok = tokens + d.token_offset;
    float ss = 0.f;
    for (int e = tid; e < E; e += kFeatThreads) {
        float acc = 0.f;
        for (int p = 0; p < gh; ++p) {
            const float a = A[p];
            if (a == 0.f) continue;
            for (int q = 0; q < pw; ++q) {
                const float bq = B[q];
                if (bq == 0.f) continue;
                acc += (a * bq) * tok[(size_t)(p * pw + q) * E + e];
            }
        }
        out[e] = acc;
        ss += acc * acc;
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) wave_ss[tid >> 6] = ss;
    __syncthreads();
    float total = wave_ss[0];
#pragma unroll
    for (int t = 1; t < kFeatWaves; ++t) total += wave_ss[t];
    const float nrm = sqrtf(total);
    for (int e = tid; e < E; e += kFeatThreads) out[e] = out[e] / nrm;      // each thread rescales what it wrote itself
}

inline size_t image_floats(int64_t P, int64_t cands) { return (size_t)(2 * P + cands); }

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

size_t dm_clipmine_workspace_bytes(int n_images, int64_t total_tokens, int64_t total_candidates) {
    if (n_images < 1 || total_tokens < n_images || total_candidates < n_images) return 0;
    return (image_floats(total_tokens, total_candidates) + 64 * (size_t)n_images) * sizeof(float);
}

int dm_clipmine_rank(void* stream, const void* tokens, const void* text, int E, const dm_clipmine_desc* desc_dev, int n_images,
                     const void* tables_dev, int kx, int ky, int k_per_image, int mode, void* work, size_t work_bytes,
                     void* maps_out_or_null, int32_t* boxes, float* d, int32_t* count, float* feats) {
    if (!tokens || !text || !desc_dev || !tables_dev || !work || !boxes || !d || !count || !feats) return DM_CLIPMINE_E_NULL;
    if (n_images < 1 || n_images > 65535) return DM_CLIPMINE_E_IMAGES;                  // images ride on gridDim.y
    if (E < 1) return DM_CLIPMINE_E_E;
    if (k_per_image < 1 || k_per_image > DM_MINE_MAX_K) return DM_CLIPMINE_E_K;
    if (mode != DM_CLIPMINE_DIFF && mode != DM_CLIPMINE_SIM) return DM_CLIPMINE_E_MODE;
    if (kx < 1 || ky < 1 || ((kx == 1) != (ky == 1))) return DM_CLIPMINE_E_WINDOW;      // `pool` skips a window with one side 1
    hipStream_t s = (hipStream_t)stream;
    std::vector<dm_clipmine_desc> desc((size_t)n_images);
    if (hipMemcpyAsync(desc.data(), desc_dev, desc.size() * sizeof(dm_clipmine_desc), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return DM_CLIPMINE_E_HIP;
    int max_P = 0, max_OH = 0;
    for (const dm_clipmine_desc& im : desc) {
        if (im.H < 1 || im.W < 1 || kx > im.H || ky > im.W) return DM_CLIPMINE_E_WINDOW;
        if (im.gh < 1 || im.pw < 1 || im.gh > DM_CLIPMINE_MAX_GRID || im.pw > DM_CLIPMINE_MAX_GRID ||
            (int64_t)im.gh * im.pw != (int64_t)im.P)
            return DM_CLIPMINE_E_GRID;
        const int64_t OH = im.H - kx + 1, OW = im.W - ky + 1;
        if (OH * OW >= ((int64_t)1 << 30)) return DM_CLIPMINE_E_WINDOW;      // candidate indices are ints, stepped by the block size
        if (im.token_offset < 0 || im.a_offset < 0 || im.b_offset < 0 || im.work_offset < 0 || (maps_out_or_null && im.map_offset < 0))
            return DM_CLIPMINE_E_OFFSET;
        if (((size_t)im.work_offset + image_floats(im.P, OH * OW)) * sizeof(float) > work_bytes) return DM_CLIPMINE_E_WORK;
        if (im.P > max_P) max_P = im.P;
        if (OH > max_OH) max_OH = (int)OH;
    }
    hipLaunchKernelGGL(clipmine_score_kernel, dim3((max_P + kScoreWaves - 1) / kScoreWaves, n_images), dim3(kScoreWaves * 64), 0, s,
                       (const float*)tokens, (const float*)text, E, desc_dev, (float*)work);
    if (hipGetLastError() != hipSuccess) return DM_CLIPMINE_E_HIP;
    hipLaunchKernelGGL(clipmine_map_kernel, dim3(max_OH, n_images), dim3(kMapThreads), 0, s, desc_dev, (const float*)tables_dev, kx, ky,
                       mode == DM_CLIPMINE_DIFF ? 1 : 0, (float*)work, (float*)maps_out_or_null);
    if (hipGetLastError() != hipSuccess) return DM_CLIPMINE_E_HIP;
    hipLaunchKernelGGL(clipmine_select_kernel, dim3(n_images), dim3(kSelThreads), 0, s, desc_dev, (const float*)work, kx, ky,
                       k_per_image, boxes, d, count);
    if (hipGetLastError() != hipSuccess) return DM_CLIPMINE_E_HIP;
    hipLaunchKernelGGL(clipmine_feature_kernel, dim3(k_per_image, n_images), dim3(kFeatThreads), 0, s, (const float*)tokens, E, desc_dev,
                       (const float*)tables_dev, k_per_image, (const int32_t*)boxes, (const int32_t*)count, feats);
    if (hipGetLastError() != hipSuccess) return DM_CLIPMINE_E_HIP;
    return 0;
}

}  // extern "C"
