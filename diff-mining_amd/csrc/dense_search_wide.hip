// dense_search_wide.hip — the Doersch-2012 baseline's detector initialisation (doersch/doersch.py:317-385): the dense
// search for thousands of candidate detectors per call, and the greedy ranking of the candidates by their neighbour lists.
//
//   - dense_wide_kernel: the [cells x C] . [C x K] fp16 GEMM of dense_search.hip for K up to 32768, of which again only the
//     per-(detector, image) maximum leaves the chip.  A workgroup of 8 waves owns 256 cells of ONE image x 256 detectors; per step of
//     64 channels both operand tiles (256 rows of 128 bytes each) are staged through LDS, so a feature row and a detector row are
//     read from memory once per WORKGROUP instead of once per wave: the wave that needed 24 KB from L2 per step in the narrow kernel
//     takes them from LDS here, and memory sees 64 KB per 2 x 256 x 256 x 64 flop.  Staging goes through registers (4 + 4 loads of
//     16 bytes per thread, issued before the step's MFMAs, written to the OTHER buffer after them: one barrier per step); the
//     16-byte chunk c of row r sits at r 128 + ((c ^ ((r >> 1) & 7)) << 4), which puts the 16 rows a ds_read_b128 lane group
//     reads on 16 different slots of the 256-byte bank row.  Block ids run over the detector tiles first, so the workgroups that
//     run at the same time share their cell tile in L2.
//   - the chain of a score is the narrow kernel's, bit for bit: C in ascending blocks of 64 channels, two v_mfma_f32_16x16x32_f16
//     per block, lane group g carrying channels c0 + 16 g + 0 ... 7 into the first and c0 + 16 g + 8 ... 15 into the second, whole
//     8-channel chunks at or past C zero on both sides, fp32 accumulation from +0.  Wave w of the workgroup computes cells
//     64 (w & 3) ... + 63 x detectors 128 (w >> 2) ... + 127 of the tile with the narrow kernel's 4 x 8 accumulators and its epilogue
//     (NaN skipped, mask byte 0 -> +0, -0 -> +0, key = (ordered fp32 bits << 32) | (0xFFFFFFFF - cell)).
//   - merge: a 64-bit unsigned integer atomic max (a vector memory atomic) of the wave's 64-cell keys into a zeroed [B][K] key table —
//     an integer max does not depend on the order of arrival, so the same input gives the same bits on every run.  No floating-point
//     atomics.  dense_wide_finish_kernel decodes the table into column image_offset + b of the score / cell tables as the narrow
//     finish kernel does (key 0 = no non-NaN cell = (-inf, -1)).
//   - dense_wide_topk_kernel: dense_topk_kernel for any K, which also gives each entry's box corner ((cell / H) 8, (cell % H) 8) with
//     the H of the entry's own image, and the count of positive images among the first 20 entries.
//   - detector_order_kernel + detector_rank_kernel: `rank_init_detectors`.  The order (key descending, index ascending) is a rank by
//     counting over the packed (key, inverted index) words, which are distinct.  The greedy loop is ONE persistent workgroup: per
//     candidate its <= 128 entries go to LDS with a 256-slot hash keyed by image, every thread walks the lists of its accepted
//     detectors (table [3][L][num_detectors] in the workspace, detector fastest) and counts the entries whose image the candidate
//     holds too with 13 inter > 6 box^2; a count above max_pairs for some accepted detector rejects the candidate.
#include "../../include/dm_engine.h"
#include "dm_kernels.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dm {

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kTile = 256;                             // cells and detectors of a workgroup's tile
constexpr int kWaves = 8;
constexpr int kThreads = kWave * kWaves;               // 512
constexpr int kMT = 4;                                 // row tiles of 16 cells per wave
constexpr int kNT = 8;                                 // column tiles of 16 detectors per wave
constexpr int kBlockC = 64;                            // channels per step (two MFMAs of k = 32)
constexpr int kRowBytes = kBlockC * 2;                 // 128
constexpr int kOpBytes = kTile * kRowBytes;            // 32 KB: one operand tile of one step
constexpr int kLdsBytes = 4 * kOpBytes;                // two buffers of (cells, detectors)
constexpr int kStage = kTile * 8 / kThreads;           // 16-byte chunks per thread, operand and step: 4
constexpr int kTopkThreads = 256;
constexpr int kRankThreads = 1024;
constexpr int kRankHash = 256;
static_assert(kMT * 16 * 4 == kTile && kNT * 16 * 2 == kTile && kStage * kThreads == kTile * 8, "8 waves of 64 x 128 cover the tile");
static_assert(DM_DETECTOR_RANK_MAX_L * 2 <= kRankHash, "the hash is at most half full");

inline int tiles_of(int n) { return (n + kTile - 1) / kTile; }
inline size_t wide_bytes_of(int B, int K) { return (size_t)B * K * sizeof(uint64_t); }

__device__ __forceinline__ uint32_t ordered_bits(float s) {          // monotone map of the non-NaN floats onto uint32
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_ordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ int lds_offset(int row, int chunk) { return row * kRowBytes + ((chunk ^ ((row >> 1) & 7)) << 4); }

__global__ __launch_bounds__(kThreads)
void dense_wide_kernel(const _Float16* __restrict__ data, const _Float16* __restrict__ w, const uint8_t* __restrict__ mask, int cells,
                       int C, int K, int tiles_m, int tiles_n, unsigned long long* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int tn = (int)(blockIdx.x % (unsigned)tiles_n);
    const int tmb = (int)(blockIdx.x / (unsigned)tiles_n);
    const int b = tmb / tiles_m, tm = tmb - b * tiles_m;
    const int cell0 = tm * kTile, k0 = tn * kTile;
    const int r = lane & 15, g = lane >> 4;
    const int wm = wave & 3, wn = wave >> 2;

    // staging: chunk id q 512 + tid of the tile's 2048 = row id >> 3, 16-byte chunk id & 7 (8 threads cover a row's 128 bytes)
    const int sch = tid & 7;
    const _Float16* asrc[kStage];
    const _Float16* bsrc[kStage];
#pragma unroll
    for (int q = 0; q < kStage; ++q) {
        const int row = 64 * q + (tid >> 3);
        asrc[q] = data + ((int64_t)b * cells + min(cell0 + row, cells - 1)) * C + 8 * sch;      // rows past the image: the last row, dropped below
        bsrc[q] = w + (int64_t)min(k0 + row, K - 1) * C + 8 * sch;
    }
    const int sdst = lds_offset(tid >> 3, sch);        // row 64 q + (tid >> 3) swizzles like row tid >> 3: + 64 q rows of 128 bytes
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 sa[kStage], sb[kStage];
    auto stage_load = [&](int c0) {
        const bool in = c0 + 8 * sch < C;              // C % 8 == 0: a chunk of 8 lies wholly inside or wholly outside
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
            sa[q] = in ? *(const half8*)(asrc[q] + c0) : zero8;
            sb[q] = in ? *(const half8*)(bsrc[q] + c0) : zero8;
        }
    };
    auto stage_store = [&](int buf) {
        unsigned char* base = lds + buf * 2 * kOpBytes;
#pragma unroll
        for (int q = 0; q < kStage; ++q) {
            *(half8*)(base + sdst + 64 * kRowBytes * q) = sa[q];
            *(half8*)(base + kOpBytes + sdst + 64 * kRowBytes * q) = sb[q];
        }
    };

    // a wave whose 64 cells or 128 detectors all lie past the end computes nothing (it still stages and meets every barrier)
    const bool active = cell0 + 64 * wm < cells && k0 + 128 * wn < K;
    // lane l reads row l & 15 of every 16-row tile, chunks 2 g and 2 g + 1 of the step; rows 16 apart swizzle alike
    int aoff[2], boff[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        aoff[h] = lds_offset(64 * wm + r, 2 * g + h);
        boff[h] = kOpBytes + lds_offset(128 * wn + r, 2 * g + h);
    }

    floatx4 acc[kMT][kNT];
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < kNT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    stage_load(0);
    stage_store(0);
    __syncthreads();
    int buf = 0;
    for (int c0 = 0; c0 < C; c0 += kBlockC) {
        const bool more = c0 + kBlockC < C;            // uniform over the workgroup
        if (more) stage_load(c0 + kBlockC);
        if (active) {
            const unsigned char* base = lds + buf * 2 * kOpBytes;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                half8 a[kMT], bb[kNT];
#pragma unroll
                for (int i = 0; i < kMT; ++i) a[i] = *(const half8*)(base + aoff[h] + 16 * kRowBytes * i);
#pragma unroll
                for (int j = 0; j < kNT; ++j) bb[j] = *(const half8*)(base + boff[h] + 16 * kRowBytes * j);
#pragma unroll
                for (int i = 0; i < kMT; ++i)
#pragma unroll
                    for (int j = 0; j < kNT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], bb[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) stage_store(buf ^ 1);                // the buffer every wave left before the last barrier
        __syncthreads();
        buf ^= 1;
    }
    if (!active) return;

    // accumulator element e of lane l: cell 16 i + 4 (l >> 4) + e of the wave's 64, detector 16 j + (l & 15) of its 128
    const int wcell0 = cell0 + 64 * wm;
    uint8_t live[kMT][4];                               // 0 = past the image, 1 = masked, 2 = scored
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cell = wcell0 + 16 * i + 4 * g + e;
            live[i][e] = cell >= cells ? 0 : (mask && mask[(int64_t)b * cells + cell] == 0) ? 1 : 2;
        }
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
        uint64_t best = 0;
#pragma unroll
        for (int i = 0; i < kMT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = acc[i][j][e];
                if (live[i][e] == 0 || s != s) continue;    // NaN stays NaN under the mask too (NaN * 0), and never wins
                if (live[i][e] == 1) s = 0.f;
                s = s + 0.f;                            // -0 and +0 are one value: -0 + 0 = +0, every other s unchanged
                const uint32_t cell = (uint32_t)(wcell0 + 16 * i + 4 * g + e);
                const uint64_t key = ((uint64_t)ordered_bits(s) << 32) | (0xFFFFFFFFu - cell);
                best = key > best ? key : best;
            }
        uint64_t o = shfl_xor_u64(best, 16);
        best = o > best ? o : best;
        o = shfl_xor_u64(best, 32);
        best = o > best ? o : best;
        const int k = k0 + 128 * wn + 16 * j + lane;
        if (lane < 16 && k < K && best != 0) atomicMax(keys + (int64_t)b * K + k, (unsigned long long)best);
    }
}

__global__ void dense_wide_finish_kernel(const unsigned long long* __restrict__ keys, int B, int K, int image_offset, int ld,
                                         float* __restrict__ score, int32_t* __restrict__ cell) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * K) return;
    const int b = (int)(t / K), k = (int)(t - (int64_t)b * K);
    const uint64_t best = keys[t];
    const int64_t o = (int64_t)k * ld + image_offset + b;
    if (best == 0) {
        score[o] = -INFINITY;
        cell[o] = -1;
    } else {
        score[o] = from_ordered((uint32_t)(best >> 32));
        cell[o] = (int32_t)(0xFFFFFFFFu - (uint32_t)best);
    }
}

__global__ __launch_bounds__(kTopkThreads)
void dense_wide_topk_kernel(const float* __restrict__ score, const int32_t* __restrict__ cell, int n_images, int ld, int top_k, int only_pos,
                            const uint8_t* __restrict__ positive, const int32_t* __restrict__ image_h, float* __restrict__ top_score,
                            int32_t* __restrict__ top_image, int32_t* __restrict__ top_x, int32_t* __restrict__ top_y,
                            int32_t* __restrict__ count, int32_t* __restrict__ d20) {
    __shared__ uint64_t wbest[kTopkThreads / kWave];
    __shared__ uint64_t taken;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float* s = score + (int64_t)k * ld;
    uint64_t last = ~(uint64_t)0;                       // no key reaches it
    int n = 0, pos20 = 0;
    for (; n < top_k; ++n) {
        uint64_t best = 0;
        for (int i = tid; i < n_images; i += kTopkThreads) {
            const float v = s[i];
            if (v != v || v == -INFINITY || (only_pos && !(v > 0.f))) continue;
            const uint64_t key = ((uint64_t)ordered_bits(v == 0.f ? 0.f : v) << 32) | (0xFFFFFFFFu - (uint32_t)i);
            if (key < last && key > best) best = key;
        }
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            const uint64_t o = shfl_xor_u64(best, m);
            best = o > best ? o : best;
        }
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
        if (tid == 0) {
            uint64_t v = wbest[0];
            for (int q = 1; q < kTopkThreads / kWave; ++q) v = wbest[q] > v ? wbest[q] : v;
            taken = v;
        }
        __syncthreads();
        last = taken;
        __syncthreads();                                // `taken` and `wbest` are rewritten in the next round
        if (last == 0) break;                           // nothing admissible is left
        if (tid == 0) {
            const int img = (int)(0xFFFFFFFFu - (uint32_t)last);
            const int64_t o = (int64_t)k * top_k + n;
            const int c = cell[(int64_t)k * ld + img], H = max(image_h[img], 1);
            top_score[o] = s[img];
            top_image[o] = img;
            top_x[o] = (c / H) * 8;
            top_y[o] = (c % H) * 8;
            if (positive && n < 20 && positive[img] != 0) ++pos20;
        }
    }
    for (int i = n + tid; i < top_k; i += kTopkThreads) {
        const int64_t o = (int64_t)k * top_k + i;
        top_score[o] = __uint_as_float(0x7FC00000u);
        top_image[o] = -1;
        top_x[o] = -1;
        top_y[o] = -1;
    }
    if (tid == 0) {
        count[k] = n;
        if (d20) d20[k] = pos20;
    }
}

// ---- the greedy ranking ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t rank_word(int32_t key, int i) {          // key descending, index ascending = the word descending
    return ((uint64_t)((uint32_t)key ^ 0x80000000u) << 32) | (0xFFFFFFFFu - (uint32_t)i);
}

__global__ __launch_bounds__(256)
void detector_order_kernel(const int32_t* __restrict__ key, int N, int32_t* __restrict__ order) {
    __shared__ uint64_t words[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t mine = i < N ? rank_word(key[i], i) : 0;
    int rank = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + threadIdx.x;
        words[threadIdx.x] = j < N ? rank_word(key[j], j) : 0;      // 0 is below every word of a real index
        __syncthreads();
        for (int t = 0; t < 256; ++t) rank += words[t] > mine ? 1 : 0;
        __syncthreads();
    }
    if (i < N) order[rank] = i;                        // the words are distinct: the ranks are a permutation of 0 ... N - 1
}

__global__ __launch_bounds__(kRankThreads)
void detector_rank_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ nb_image, const int32_t* __restrict__ nb_x,
                          const int32_t* __restrict__ nb_y, const int32_t* __restrict__ nb_count, int N, int L, int box, int max_pairs,
                          int ND, int32_t* __restrict__ tab, int32_t* __restrict__ accepted, int32_t* __restrict__ n_accepted) {
    __shared__ int32_t hkey[kRankHash], hval[kRankHash];
    __shared__ int32_t cx[DM_DETECTOR_RANK_MAX_L], cy[DM_DETECTOR_RANK_MAX_L], cimg[DM_DETECTOR_RANK_MAX_L];
    __shared__ int32_t tcount[DM_DETECTOR_RANK_MAX_DETECTORS];
    const int tid = threadIdx.x;
    int32_t* tab_img = tab;                             // [L][ND] each: entry j of accepted detector d at j ND + d
    int32_t* tab_x = tab + (int64_t)L * ND;
    int32_t* tab_y = tab + 2 * (int64_t)L * ND;
    const int bound = 6 * box * box;                    // box <= 2048: 13 inter <= 13 * 2^22 fits an int
    int n_acc = 0;
    for (int pos = 0; pos < N && n_acc < ND; ++pos) {
        const int k = order[pos];
        const int cnt = min(max(nb_count[k], 0), L);
        if (tid < kRankHash) hkey[tid] = -1;
        __syncthreads();
        if (tid < cnt) {
            const int img = nb_image[(int64_t)k * L + tid];
            cimg[tid] = img;
            cx[tid] = nb_x[(int64_t)k * L + tid];
            cy[tid] = nb_y[(int64_t)k * L + tid];
            if (img >= 0) {                             // a negative image is no entry
                unsigned h = ((unsigned)img * 2654435761u) >> 24;
                for (;;) {
                    const int old = atomicCAS(&hkey[h], -1, img);
                    if (old == -1) { hval[h] = tid; break; }
                    if (old == img) break;              // outside the contract (an image twice in one list): the first to arrive stays
                    h = (h + 1) & (kRankHash - 1);
                }
            }
        }
        __syncthreads();
        int reject = 0;
        for (int d = tid; d < n_acc; d += kRankThreads) {
            const int dn = tcount[d];
            int pairs = 0;
            for (int j = 0; j < dn && pairs <= max_pairs; ++j) {
                const int img = tab_img[(int64_t)j * ND + d];
                if (img < 0) continue;
                unsigned h = ((unsigned)img * 2654435761u) >> 24;
                int at = -1;
                for (;;) {
                    const int q = hkey[h];
                    if (q == -1) break;
                    if (q == img) { at = hval[h]; break; }
                    h = (h + 1) & (kRankHash - 1);
                }
                if (at < 0) continue;
                int64_t ax = (int64_t)cx[at] - tab_x[(int64_t)j * ND + d], ay = (int64_t)cy[at] - tab_y[(int64_t)j * ND + d];
                ax = ax < 0 ? -ax : ax;
                ay = ay < 0 ? -ay : ay;
                if (ax >= box || ay >= box) continue;
                const int inter = (box - (int)ax) * (box - (int)ay);
                pairs += 13 * inter > bound ? 1 : 0;
            }
            if (pairs > max_pairs) reject = 1;
        }
        const int any = __syncthreads_or(reject);
        if (!any) {
            if (tid < cnt) {
                tab_img[(int64_t)tid * ND + n_acc] = cimg[tid];
                tab_x[(int64_t)tid * ND + n_acc] = cx[tid];
                tab_y[(int64_t)tid * ND + n_acc] = cy[tid];
            }
            if (tid == 0) {
                tcount[n_acc] = cnt;
                accepted[n_acc] = k;
            }
            ++n_acc;
        }
        __syncthreads();                                // the table, tcount and the hash are read and rewritten in the next step
    }
    for (int i = n_acc + tid; i < ND; i += kRankThreads) accepted[i] = -1;
    if (tid == 0) *n_accepted = n_acc;
}

inline size_t rank_bytes_of(int N, int L, int ND) { return ((size_t)N + 3 * (size_t)L * ND) * sizeof(int32_t); }

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

size_t dm_dense_wide_workspace_bytes(int B, int cells, int K) {
    if (B < 1 || cells < 1 || cells >= (1 << 24) || K < 1 || K > DM_DENSE_WIDE_MAX_DETECTORS) return 0;
    return wide_bytes_of(B, K);
}

int dm_dense_wide_winners(void* stream, const void* data_f16, const void* w_f16, const void* mask_u8_or_null, int B, int cells, int C,
                          int K, int image_offset, int ld, void* work, size_t work_bytes, float* score_f32, int32_t* cell_i32) {
    if (!data_f16 || !w_f16 || !work || !score_f32 || !cell_i32) return DM_DENSE_E_NULL;
    if (B < 1) return DM_DENSE_E_IMAGES;
    if (cells < 1) return DM_DENSE_E_CELLS;
    if (cells >= (1 << 24)) return DM_DENSE_E_CELLS_LARGE;
    if (K < 1 || K > DM_DENSE_WIDE_MAX_DETECTORS) return DM_DENSE_E_K;
    if (C < 8 || C % 8 != 0) return DM_DENSE_E_C;
    if (image_offset < 0 || (int64_t)ld < (int64_t)image_offset + B) return DM_DENSE_E_LD;
    if (work_bytes < wide_bytes_of(B, K)) return DM_DENSE_E_WORK;
    if (((uintptr_t)data_f16 | (uintptr_t)w_f16) & 15 || (uintptr_t)work & 7) return DM_DENSE_E_ALIGN;
    const int tiles_m = tiles_of(cells), tiles_n = tiles_of(K);
    const int64_t blocks = (int64_t)B * tiles_m * tiles_n;
    if (blocks > 0x7FFFFFFF) return DM_DENSE_E_IMAGES;
    hipStream_t s = (hipStream_t)stream;
    static std::atomic<uint64_t> attr_seen{0};         // hipFuncSetAttribute is per DEVICE, not per process
    if (first_use_on_device(attr_seen))
        (void)hipFuncSetAttribute((const void*)dense_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (hipMemsetAsync(work, 0, wide_bytes_of(B, K), s) != hipSuccess) return DM_DENSE_E_HIP;
    hipLaunchKernelGGL(dense_wide_kernel, dim3((unsigned)blocks), dim3(kThreads), kLdsBytes, s, (const _Float16*)data_f16,
                       (const _Float16*)w_f16, (const uint8_t*)mask_u8_or_null, cells, C, K, tiles_m, tiles_n, (unsigned long long*)work);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    const int64_t threads = (int64_t)B * K;
    hipLaunchKernelGGL(dense_wide_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)work,
                       B, K, image_offset, ld, score_f32, cell_i32);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    return 0;
}

int dm_dense_wide_topk(void* stream, const float* score_f32, const int32_t* cell_i32, int K, int n_images, int ld, int top_k, int only_pos,
                       const void* positive_u8_or_null, const int32_t* image_h_i32, float* top_score_f32, int32_t* top_image_i32,
                       int32_t* top_x_i32, int32_t* top_y_i32, int32_t* count_i32, int32_t* d20_i32_or_null) {
    if (!score_f32 || !cell_i32 || !image_h_i32 || !top_score_f32 || !top_image_i32 || !top_x_i32 || !top_y_i32 || !count_i32)
        return DM_DENSE_E_NULL;
    if (d20_i32_or_null && !positive_u8_or_null) return DM_DENSE_E_NULL;
    if (n_images < 1) return DM_DENSE_E_IMAGES;
    if (K < 1 || K > DM_DENSE_WIDE_MAX_DETECTORS) return DM_DENSE_E_K;
    if (top_k < 1 || top_k > DM_DENSE_MAX_TOPK) return DM_DENSE_E_TOPK;
    if (ld < n_images) return DM_DENSE_E_LD;
    hipLaunchKernelGGL(dense_wide_topk_kernel, dim3(K), dim3(kTopkThreads), 0, (hipStream_t)stream, score_f32, cell_i32, n_images, ld, top_k,
                       only_pos ? 1 : 0, (const uint8_t*)positive_u8_or_null, image_h_i32, top_score_f32, top_image_i32, top_x_i32,
                       top_y_i32, count_i32, d20_i32_or_null);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    return 0;
}

size_t dm_detector_rank_workspace_bytes(int N, int L, int num_detectors) {
    if (N < 1 || N > DM_DETECTOR_RANK_MAX_N || L < 1 || L > DM_DETECTOR_RANK_MAX_L || num_detectors < 1 ||
        num_detectors > DM_DETECTOR_RANK_MAX_DETECTORS)
        return 0;
    return rank_bytes_of(N, L, num_detectors);
}

int dm_detector_rank(void* stream, const int32_t* key_i32, const int32_t* nb_image_i32, const int32_t* nb_x_i32, const int32_t* nb_y_i32,
                     const int32_t* nb_count_i32, int N, int L, int box, int max_pairs, int num_detectors, void* work, size_t work_bytes,
                     int32_t* accepted_i32, int32_t* n_accepted_i32) {
    if (!key_i32 || !nb_image_i32 || !nb_x_i32 || !nb_y_i32 || !nb_count_i32 || !work || !accepted_i32 || !n_accepted_i32)
        return DM_RANK_E_NULL;
    if (N < 1 || N > DM_DETECTOR_RANK_MAX_N) return DM_RANK_E_N;
    if (L < 1 || L > DM_DETECTOR_RANK_MAX_L) return DM_RANK_E_L;
    if (num_detectors < 1 || num_detectors > DM_DETECTOR_RANK_MAX_DETECTORS) return DM_RANK_E_DETECTORS;
    if (box < 1 || box > DM_DETECTOR_RANK_MAX_BOX) return DM_RANK_E_BOX;
    if (max_pairs < 0) return DM_RANK_E_PAIRS;
    if (work_bytes < rank_bytes_of(N, L, num_detectors)) return DM_RANK_E_WORK;
    if ((uintptr_t)work & 3) return DM_RANK_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    int32_t* order = (int32_t*)work;
    hipLaunchKernelGGL(detector_order_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, key_i32, N, order);
    if (hipGetLastError() != hipSuccess) return DM_RANK_E_HIP;
    hipLaunchKernelGGL(detector_rank_kernel, dim3(1), dim3(kRankThreads), 0, s, (const int32_t*)order, nb_image_i32, nb_x_i32, nb_y_i32,
                       nb_count_i32, N, L, box, max_pairs, num_detectors, order + N, accepted_i32, n_accepted_i32);
    if (hipGetLastError() != hipSuccess) return DM_RANK_E_HIP;
    return 0;
}

}  // extern "C"
