// dense_search.hip — the Doersch-2012 baseline's dense detector search (doersch/hog.py:124-185):
//   scores = (data.reshape(B*W*H, C).unsqueeze(1) * w.unsqueeze(0)).sum(-1)        (:144; a [B W H, K, C] fp16 broadcast)
//   scores = scores * mask; torch.topk(scores.reshape(K*B, W*H), 1)                (:153-156)
//   sorted(buffer[k] + chunk[k], key=score, reverse=True)[:top_k]                  (:118)
// as a [cells x C] . [C x K] fp16 GEMM on the matrix cores whose [cells x K] output is never formed: only its per-(detector, image)
// maximum leaves the registers.
//
//   - dense_winners_kernel: one WAVE owns 64 consecutive cells of one image (4 row tiles of 16) and ALL detectors of the call
//     (NT = ceil(K / 16) column tiles, NT <= 8): 4 NT accumulators of v_mfma_f32_16x16x32_f16 stay resident while the loop walks C in
//     blocks of 64 channels, so a feature row is read from memory exactly once.  There is no LDS and no barrier: both operands are
//     row-major with C contiguous, which IS the MFMA operand layout (lane l: row l & 15, 8 consecutive channels).  Inside a block lane
//     group g = l >> 4 takes channels 16 g ... 16 g + 15 (two 16-byte loads: four lanes cover one 128-byte line of a row) and feeds
//     the first eight to the block's first MFMA, the other eight to its second.  The detectors come from L2 (K C 2 bytes, 270 KB at
//     the real size, shared by every wave of the chip); the next block's operands are fetched before the current block's MFMAs.
//     A chunk of 8 channels at or past C is zeros on both sides (C % 8 == 0, so chunks are whole): the chain of every score is
//     [C / 64 rounded up] x 2 MFMAs in ascending block order whatever B, K, the chunk or the position — it depends on C alone.
//   - epilogue: NaN is skipped; mask byte 0 -> the score is +0 exactly; key = (ordered fp32 bits << 32) | (0xFFFFFFFF - cell), so an
//     unsigned max picks the largest score and, among equal scores, the lowest cell.  16 cells per lane, then xor-shuffles across the
//     four lane groups; lanes 0 ... 15 store one key per detector and 64-cell tile into the workspace (plain stores, nothing zeroed).
//   - dense_finish_kernel: one thread per (image, detector) takes the max of its tiles' keys in ascending tile order (an integer max:
//     the order cannot matter) and writes score / cell at column image_offset + b; key 0 = no non-NaN cell = (-inf, -1).
//   - dense_topk_kernel: one workgroup per detector; top_k rounds of "the largest key below the last one taken" over the columns,
//     key = (ordered score << 32) | (0xFFFFFFFF - image): score descending, image ascending.
//   - dense_gather_kernel: 16-byte copies of n rows.
// Rows past the last cell and detectors past K are read from the last valid row (in bounds) and dropped in the epilogue.
#include "../../include/dm_engine.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dm {

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kMT = 4;                                 // row tiles of 16 cells per wave
constexpr int kTileCells = 16 * kMT;                   // 64
constexpr int kBlockC = 64;                            // channels per loop step (two MFMAs of k = 32)
constexpr int kMaxNT = DM_DENSE_MAX_DETECTORS / 16;
constexpr int kTopkThreads = 256;
static_assert(DM_DENSE_MAX_DETECTORS % 16 == 0 && kMaxNT == 8, "the kernel is instantiated for 1 ... 8 column tiles");

inline int tiles_of(int cells) { return (cells + kTileCells - 1) / kTileCells; }
inline int nt_of(int K) { return (K + 15) / 16; }
inline size_t work_bytes_of(int B, int cells, int K) { return (size_t)B * tiles_of(cells) * nt_of(K) * 16 * sizeof(uint64_t); }

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

template <int NT>
__global__ __launch_bounds__(kWave * kWavesPerBlock)
void dense_winners_kernel(const _Float16* __restrict__ data, const _Float16* __restrict__ w, const uint8_t* __restrict__ mask,
                          int cells, int C, int K, int tiles, int64_t n_tiles_all, uint64_t* __restrict__ partial) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t gid = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (gid >= n_tiles_all) return;                    // no barrier anywhere: a wave may leave alone
    const int b = (int)(gid / tiles), tile = (int)(gid - (int64_t)b * tiles);
    const int r = lane & 15, g = lane >> 4;
    const int cell0 = tile * kTileCells;

    const _Float16* arow[kMT];
#pragma unroll
    for (int i = 0; i < kMT; ++i) {
        const int cell = min(cell0 + 16 * i + r, cells - 1);
        arow[i] = data + ((int64_t)b * cells + cell) * C + 16 * g;
    }
    const _Float16* brow[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) brow[j] = w + (int64_t)min(16 * j + r, K - 1) * C + 16 * g;

    floatx4 acc[kMT][NT];
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 a[kMT][2], bb[NT][2], an[kMT][2], bn[NT][2];
    auto fetch = [&](int c0, half8 (&fa)[kMT][2], half8 (&fb)[NT][2]) {       // channels c0 + 16 g + {0 ... 7, 8 ... 15} of every row
        const int c = c0 + 16 * g;
        const bool in0 = c < C, in1 = c + 8 < C;        // C % 8 == 0: a chunk of 8 lies wholly inside or wholly outside
#pragma unroll
        for (int i = 0; i < kMT; ++i) {
            fa[i][0] = in0 ? *(const half8*)(arow[i] + c0) : zero8;
            fa[i][1] = in1 ? *(const half8*)(arow[i] + c0 + 8) : zero8;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            fb[j][0] = in0 ? *(const half8*)(brow[j] + c0) : zero8;
            fb[j][1] = in1 ? *(const half8*)(brow[j] + c0 + 8) : zero8;
        }
    };

    fetch(0, a, bb);
    for (int c0 = 0; c0 < C; c0 += kBlockC) {
        const bool more = c0 + kBlockC < C;             // wave-uniform
        if (more) fetch(c0 + kBlockC, an, bn);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < kMT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i][h], bb[j][h], acc[i][j], 0, 0, 0);
        if (more) {
#pragma unroll
            for (int i = 0; i < kMT; ++i) { a[i][0] = an[i][0]; a[i][1] = an[i][1]; }
#pragma unroll
            for (int j = 0; j < NT; ++j) { bb[j][0] = bn[j][0]; bb[j][1] = bn[j][1]; }
        }
    }

    // accumulator element e of lane l: cell 16 i + 4 (l >> 4) + e of the tile, detector 16 j + (l & 15)
    uint8_t live[kMT][4];                               // 0 = past the image, 1 = masked, 2 = scored
#pragma unroll
    for (int i = 0; i < kMT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cell = cell0 + 16 * i + 4 * g + e;
            live[i][e] = cell >= cells ? 0 : (mask && mask[(int64_t)b * cells + cell] == 0) ? 1 : 2;
        }
    uint64_t* out = partial + ((int64_t)b * tiles + tile) * (NT * 16);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        uint64_t best = 0;
#pragma unroll
        for (int i = 0; i < kMT; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = acc[i][j][e];
                if (live[i][e] == 0 || s != s) continue;    // NaN stays NaN under the mask too (NaN * 0), and never wins
                if (live[i][e] == 1) s = 0.f;
                s = s + 0.f;                            // -0 and +0 are one value: -0 + 0 = +0, every other s unchanged
                const uint32_t cell = (uint32_t)(cell0 + 16 * i + 4 * g + e);
                const uint64_t key = ((uint64_t)ordered_bits(s) << 32) | (0xFFFFFFFFu - cell);
                best = key > best ? key : best;
            }
        uint64_t o = shfl_xor_u64(best, 16);
        best = o > best ? o : best;
        o = shfl_xor_u64(best, 32);
        best = o > best ? o : best;
        if (lane < 16) out[16 * j + lane] = best;
    }
}

__global__ void dense_finish_kernel(const uint64_t* __restrict__ partial, int B, int K, int tiles, int ntk, int image_offset, int ld,
                                    float* __restrict__ score, int32_t* __restrict__ cell) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * K) return;
    const int b = (int)(t / K), k = (int)(t - (int64_t)b * K);
    const uint64_t* p = partial + (int64_t)b * tiles * ntk + k;
    uint64_t best = 0;
    for (int tile = 0; tile < tiles; ++tile) {
        const uint64_t v = p[(int64_t)tile * ntk];
        best = v > best ? v : best;
    }
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
void dense_topk_kernel(const float* __restrict__ score, const int32_t* __restrict__ cell, int n_images, int ld, int top_k, int only_pos,
                       float* __restrict__ top_score, int32_t* __restrict__ top_image, int32_t* __restrict__ top_cell,
                       int32_t* __restrict__ count) {
    __shared__ uint64_t wbest[kTopkThreads / kWave];
    __shared__ uint64_t taken;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const float* s = score + (int64_t)k * ld;
    uint64_t last = ~(uint64_t)0;                       // no key reaches it: the low word of a key is at most 0xFFFFFFFF - 0 with a high word < 2^32 - 1
    int n = 0;
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
            top_score[o] = s[img];
            top_image[o] = img;
            top_cell[o] = cell[(int64_t)k * ld + img];
        }
    }
    for (int i = n + tid; i < top_k; i += kTopkThreads) {
        const int64_t o = (int64_t)k * top_k + i;
        top_score[o] = __uint_as_float(0x7FC00000u);
        top_image[o] = -1;
        top_cell[o] = -1;
    }
    if (tid == 0) count[k] = n;
}

__global__ void dense_gather_kernel(const _Float16* __restrict__ data, int B, int cells, int C, const int32_t* __restrict__ pairs, int n,
                                    _Float16* __restrict__ out) {
    const int chunks = C / 8;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * chunks) return;
    const int row = (int)(t / chunks), c = (int)(t - (int64_t)row * chunks) * 8;
    const int img = pairs[2 * row], cell = pairs[2 * row + 1];
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};                 // a pair outside the chunk reads nothing and gives a zero row
    if (img >= 0 && img < B && cell >= 0 && cell < cells) v = *(const half8*)(data + ((int64_t)img * cells + cell) * C + c);
    *(half8*)(out + (int64_t)row * C + c) = v;
}

template <int NT>
void launch_winners(hipStream_t s, unsigned blocks, const void* data, const void* w, const void* mask, int cells, int C, int K, int tiles,
                    int64_t n_tiles_all, uint64_t* partial) {
    hipLaunchKernelGGL(dense_winners_kernel<NT>, dim3(blocks), dim3(kWave * kWavesPerBlock), 0, s, (const _Float16*)data,
                       (const _Float16*)w, (const uint8_t*)mask, cells, C, K, tiles, n_tiles_all, partial);
}

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

size_t dm_dense_search_workspace_bytes(int B, int cells, int K) {
    if (B < 1 || cells < 1 || cells >= (1 << 24) || K < 1 || K > DM_DENSE_MAX_DETECTORS) return 0;
    return work_bytes_of(B, cells, K);
}

int dm_dense_search_winners(void* stream, const void* data_f16, const void* w_f16, const void* mask_u8_or_null, int B, int cells, int C,
                            int K, int image_offset, int ld, void* work, size_t work_bytes, float* score_f32, int32_t* cell_i32) {
    if (!data_f16 || !w_f16 || !work || !score_f32 || !cell_i32) return DM_DENSE_E_NULL;
    if (B < 1) return DM_DENSE_E_IMAGES;
    if (cells < 1) return DM_DENSE_E_CELLS;
    if (cells >= (1 << 24)) return DM_DENSE_E_CELLS_LARGE;
    if (K < 1 || K > DM_DENSE_MAX_DETECTORS) return DM_DENSE_E_K;
    if (C < 8 || C % 8 != 0) return DM_DENSE_E_C;
    if (image_offset < 0 || (int64_t)ld < (int64_t)image_offset + B) return DM_DENSE_E_LD;
    if (work_bytes < work_bytes_of(B, cells, K)) return DM_DENSE_E_WORK;
    if (((uintptr_t)data_f16 | (uintptr_t)w_f16) & 15 || (uintptr_t)work & 7) return DM_DENSE_E_ALIGN;
    const int tiles = tiles_of(cells), nt = nt_of(K);
    const int64_t n_tiles_all = (int64_t)B * tiles;
    const int64_t blocks = (n_tiles_all + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > 0x7FFFFFFF) return DM_DENSE_E_IMAGES;
    hipStream_t s = (hipStream_t)stream;
    uint64_t* partial = (uint64_t*)work;
    switch (nt) {
#define DM_DENSE_CASE(NT) \
    case NT: launch_winners<NT>(s, (unsigned)blocks, data_f16, w_f16, mask_u8_or_null, cells, C, K, tiles, n_tiles_all, partial); break;
        DM_DENSE_CASE(1) DM_DENSE_CASE(2) DM_DENSE_CASE(3) DM_DENSE_CASE(4) DM_DENSE_CASE(5) DM_DENSE_CASE(6) DM_DENSE_CASE(7)
        DM_DENSE_CASE(8)
#undef DM_DENSE_CASE
        default: return DM_DENSE_E_K;
    }
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    const int64_t threads = (int64_t)B * K;
    hipLaunchKernelGGL(dense_finish_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const uint64_t*)partial, B, K, tiles,
                       nt * 16, image_offset, ld, score_f32, cell_i32);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    return 0;
}

int dm_dense_search_topk(void* stream, const float* score_f32, const int32_t* cell_i32, int K, int n_images, int ld, int top_k, int only_pos,
                         float* top_score_f32, int32_t* top_image_i32, int32_t* top_cell_i32, int32_t* count_i32) {
    if (!score_f32 || !cell_i32 || !top_score_f32 || !top_image_i32 || !top_cell_i32 || !count_i32) return DM_DENSE_E_NULL;
    if (n_images < 1) return DM_DENSE_E_IMAGES;
    if (K < 1 || K > DM_DENSE_MAX_DETECTORS) return DM_DENSE_E_K;
    if (top_k < 1 || top_k > DM_DENSE_MAX_TOPK) return DM_DENSE_E_TOPK;
    if (ld < n_images) return DM_DENSE_E_LD;
    hipLaunchKernelGGL(dense_topk_kernel, dim3(K), dim3(kTopkThreads), 0, (hipStream_t)stream, score_f32, cell_i32, n_images, ld, top_k,
                       only_pos ? 1 : 0, top_score_f32, top_image_i32, top_cell_i32, count_i32);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    return 0;
}

int dm_dense_search_gather(void* stream, const void* data_f16, int B, int cells, int C, const int32_t* pairs_i32, int n, void* out_f16) {
    if (!data_f16 || !pairs_i32 || !out_f16) return DM_DENSE_E_NULL;
    if (B < 1 || n < 1) return DM_DENSE_E_IMAGES;
    if (cells < 1) return DM_DENSE_E_CELLS;
    if (cells >= (1 << 24)) return DM_DENSE_E_CELLS_LARGE;
    if (C < 8 || C % 8 != 0) return DM_DENSE_E_C;
    if (((uintptr_t)data_f16 | (uintptr_t)out_f16) & 15) return DM_DENSE_E_ALIGN;
    const int64_t threads = (int64_t)n * (C / 8);
    if ((threads + 255) / 256 > 0x7FFFFFFF) return DM_DENSE_E_IMAGES;
    hipLaunchKernelGGL(dense_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)data_f16, B, cells, C, pairs_i32, n, (_Float16*)out_f16);
    if (hipGetLastError() != hipSuccess) return DM_DENSE_E_HIP;
    return 0;
}

}  // extern "C"
