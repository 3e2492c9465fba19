// umap_device.h — the device code of the clustering stage's UMAP projection: exact kNN, the fuzzy simplicial set and
// the synchronous 500-epoch layout, by the rules umapfit.py states in numpy (its module header is the specification; the restatement
// of umap-learn 0.5.6 it gives is PARITY UNPINNED).  Included by umap.hip (the route below DM_UMAP_MAX_N rows, with the dense n x n
// graph) and by umap_sparse.hip (the route without it): what both routes must compute alike is written once, here.
//
// Like kmeans.hip the work is small and launch-bound, so structure is what matters:
//   - every sum has a fixed order and there is no floating-point atomic: the same input gives the same bits on every run;
//   - the kNN distances are fp64 sums in ascending feature order with separate multiply and add, so they equal numpy's bit for bit;
//   - the edge list is compacted by a row-wise prefix sum (row-major order, ascending column), not by an atomic counter;
//   - an epoch is one launch that reads one coordinate buffer and writes the other; the wave that owns a vertex is the only writer of
//     that vertex's coordinates and of its edges' schedule entries.  The epochs are enqueued back to back, no host read between them;
//   - no kernel reads workspace it (or an earlier kernel of the same call, or of the layout call that started the schedule) has not
//     written.
#pragma once
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

#include <math.h>

namespace dm {

namespace {

constexpr int kWave = 64;
constexpr int kRowWaves = 4;                 // the wave-per-row kernels: 4 rows per 256-thread block
constexpr int kKnnThreads = 256;             // umap_knn_kernel: one column of the tile per thread
constexpr int kKnnRows = 2;                  // rows a workgroup owns: 2 x 4095 fp32 distances + the tile stay under 64 KiB of LDS
constexpr int kKnnChunk = 16;                // features per staged tile
constexpr int kScanThreads = 1024;
constexpr int kScanPer = DM_UMAP_MAX_N / kScanThreads;      // rows per thread of the single-block prefix sum

struct UmWork {                              // the workspace, carved by um_layout
    float *Y2, *eps, *epn, *next, *next_neg, *wmax;          // the layout's: second buffer, schedule [n_edges], max weight
    float *A, *rowmax;                                       // the graph's: dense memberships [n][n], row maxima of P
    int32_t* rowcount;
    size_t layout_bytes, bytes;
};

// `edges`: the capacity of the schedule arrays.  The layout's part comes first and depends on (n, dim, edges) alone, so a layout call
// carves it with its own n_edges.
UmWork um_layout(void* base, int n, int dim, size_t edges) {
    UmWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t N = (size_t)n;
    w.wmax = (float*)take(4);
    w.Y2 = (float*)take(N * (size_t)dim * 4);
    w.eps = (float*)take(edges * 4);
    w.epn = (float*)take(edges * 4);
    w.next = (float*)take(edges * 4);
    w.next_neg = (float*)take(edges * 4);
    w.layout_bytes = off;
    w.A = (float*)take(N * N * 4);
    w.rowmax = (float*)take(N * 4);
    w.rowcount = (int32_t*)take(N * 4);
    w.bytes = off;
    return w;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {            // xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// The kNN rule's arithmetic, shared by both routes' kernels: one feature's term of the fp64 squared distance (multiply and add
// separate), and the distance, the fp64 root rounded to fp32.
__device__ __forceinline__ double knn_add(double acc, double xi, double xj) {
#pragma clang fp contract(off)
    const double diff = xi - xj;
    const double sq = diff * diff;
    return acc + sq;
}

__device__ __forceinline__ float knn_root(double acc) { return (float)sqrt(acc); }

// ---- exact kNN ------------------------------------------------------------------------------------------------------------------
// A workgroup owns kKnnRows rows.  Thread t of column tile c holds the fp64 sums of rows i0, i0 + 1 against row j = 256 c + t; the
// features come through LDS in chunks of kKnnChunk (tile[e][t], read without bank conflicts; the owned rows' values are broadcasts).
// The fp32 distances of the whole row stay in LDS (dynamic, kKnnRows x n floats); then wave r selects row r's k smallest by k rounds
// of a wave-wide minimum over the key (distance bits << 32 | index): non-negative floats order as their bits, the index breaks ties
// towards the lower one, and a taken entry becomes all ones.  k < n, so every round finds an entry that is still there.
__global__ __launch_bounds__(kKnnThreads)
void umap_knn_kernel(const float* __restrict__ X, int n, int d, int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float knn_dist[];                  // [kKnnRows][n]
    __shared__ float tile[kKnnChunk][kKnnThreads + 1];
    __shared__ float own[kKnnRows][kKnnChunk];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * kKnnRows;
    for (int j0 = 0; j0 < n; j0 += kKnnThreads) {
        double acc[kKnnRows];
#pragma unroll
        for (int r = 0; r < kKnnRows; ++r) acc[r] = 0.0;
        for (int e0 = 0; e0 < d; e0 += kKnnChunk) {
            const int ne = min(kKnnChunk, d - e0);
            __syncthreads();                                            // the previous chunk has been read
            for (int q = t; q < kKnnThreads * kKnnChunk; q += kKnnThreads) {
                const int row = q / kKnnChunk, e = q % kKnnChunk;
                tile[e][row] = (j0 + row < n && e < ne) ? X[(size_t)(j0 + row) * d + e0 + e] : 0.f;
            }
            if (t < kKnnRows * kKnnChunk) {
                const int r = t / kKnnChunk, e = t % kKnnChunk;
                own[r][e] = (i0 + r < n && e < ne) ? X[(size_t)(i0 + r) * d + e0 + e] : 0.f;
            }
            __syncthreads();
            for (int e = 0; e < ne; ++e) {
                const double xj = (double)tile[e][t];
#pragma unroll
                for (int r = 0; r < kKnnRows; ++r) {
                    acc[r] = knn_add(acc[r], (double)own[r][e], xj);
                }
            }
        }
        if (j0 + t < n) {
#pragma unroll
            for (int r = 0; r < kKnnRows; ++r) knn_dist[(size_t)r * n + j0 + t] = knn_root(acc[r]);
        }
    }
    __syncthreads();
    const int wave = t / kWave, lane = t % kWave;
    if (wave >= kKnnRows || i0 + wave >= n) return;
    uint32_t* row = (uint32_t*)(knn_dist + (size_t)wave * n);            // read as bit patterns from here on
    const int i = i0 + wave;
    for (int s = 0; s < k; ++s) {
        unsigned long long best = ~0ull;
        for (int j = lane; j < n; j += kWave) {
            const unsigned long long key = ((unsigned long long)row[j] << 32) | (unsigned)j;
            const bool taken = row[j] == 0xFFFFFFFFu;
            best = (!taken && key < best) ? key : best;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, kWave);
            best = other < best ? other : best;
        }
        const int j = (int)(best & 0xFFFFFFFFull);
        if (best == ~0ull || j >= n) return;                            // cannot happen for k < n; never index with it
        if (lane == 0) {
            idx_out[(size_t)i * k + s] = j;
            dist_out[(size_t)i * k + s] = __uint_as_float((uint32_t)(best >> 32));
        }
        if (lane == j % kWave) row[j] = 0xFFFFFFFFu;                    // the lane that scans j marks it: no other lane reads row[j]
    }
}

// ---- smooth_knn_dist and the memberships ------------------------------------------------------------------------------------------
// One wave per row, lane j holds d_ij.  The bisection runs in fp64 with the terms added in ascending j (a broadcast per term: every
// lane carries the same sum), as the numpy restatement adds them.  The global mean distance is summed by every wave in the same
// lane-strided order, so all rows use the same bits.  kDense: memberships go to the dense A [n][n] (zeroed before the launch);
// otherwise to memb [n][k], slot by slot as idx lists them (0 for an index that is no row).
template <bool kDense>
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_smooth_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dist, int n, int k, float* __restrict__ rho_out,
                        float* __restrict__ sigma_out, float* __restrict__ A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const bool has = lane < k;
    const float dj = has ? dist[(size_t)i * k + lane] : 0.f;
    // rho: the smallest non-zero distance of the row
    float m = (has && dj > 0.f) ? dj : INFINITY;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, kWave));
    const float rho = m < INFINITY ? m : 0.f;
    const double x = (double)dj - (double)rho;
    const double target = log2((double)k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {
        const double term = x > 0.0 ? exp(-(x / mid)) : 1.0;
        double psum = 0.0;
        for (int j = 1; j < k; ++j) psum = psum + __shfl(term, j, kWave);
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    // the floor: 1e-3 x the row's mean distance, or x the global mean where rho is 0
    double row_sum = 0.0;
    for (int j = 0; j < k; ++j) row_sum = row_sum + (double)__shfl(dj, j, kWave);
    double floor_at;
    if (rho > 0.f) {
        floor_at = 1e-3 * (row_sum / (double)k);
    } else {
        double part = 0.0;
        const size_t total = (size_t)n * k;
        for (size_t q = lane; q < total; q += kWave) part = part + (double)dist[q];
        floor_at = 1e-3 * (wave_sum(part) / (double)total);
    }
    const float sigma = (float)(mid < floor_at ? floor_at : mid);
    if (lane == 0) {
        rho_out[i] = rho;
        sigma_out[i] = sigma;
    }
    if (has) {
        const int j = idx[(size_t)i * k + lane];
        if (j >= 0 && j < n) {
            const double xs = (double)dj - (double)rho;
            const float v = j == i ? 0.f : (xs <= 0.0 || sigma == 0.f) ? 1.f : (float)exp(-(xs / (double)sigma));
            A[kDense ? (size_t)i * n + j : (size_t)i * k + lane] = v;
        } else if (!kDense) {
            A[(size_t)i * k + lane] = 0.f;
        }
    }
}

// The fuzzy union of both routes: P_ij from a = a_ij and at = a_ji in fp32, the product rounded on its own.
__device__ __forceinline__ float umap_union_p(float a, float at) {
#pragma clang fp contract(off)
    const float prod = a * at;
    return (a + at) - prod;
}

// ---- union, pruning, compaction ---------------------------------------------------------------------------------------------------
// One 256-thread block per row: P_ij = (A_ij + A_ji) - A_ij A_ji in fp32 and the row's maximum.
__global__ __launch_bounds__(256)
void umap_union_kernel(const float* __restrict__ A, int n, float* __restrict__ P, float* __restrict__ rowmax) {
#pragma clang fp contract(off)
    __shared__ float part[256 / kWave];
    const int i = blockIdx.x;
    float m = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) {
        const float p = umap_union_p(A[(size_t)i * n + j], A[(size_t)j * n + i]);
        P[(size_t)i * n + j] = p;
        m = fmaxf(m, p);
    }
    m = wave_max(m);
    if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) rowmax[i] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// One block per row: entries below max(P) / n_epochs become 0; the row's count of non-zeros.  (A maximum has no order to fix.)
__global__ __launch_bounds__(256)
void umap_prune_kernel(float* __restrict__ P, const float* __restrict__ rowmax, int n, int n_epochs, int32_t* __restrict__ rowcount) {
    __shared__ float part[256 / kWave];
    __shared__ int cnt[256 / kWave];
    const int i = blockIdx.x;
    float m = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) m = fmaxf(m, rowmax[j]);
    m = wave_max(m);
    if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = m;
    __syncthreads();
    const float thr = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])) / (float)n_epochs;
    int c = 0;
    for (int j = threadIdx.x; j < n; j += 256) {
        float p = P[(size_t)i * n + j];
        if (p < thr) {
            p = 0.f;
            P[(size_t)i * n + j] = p;
        }
        c += p != 0.f;
    }
    c = wave_sum(c);
    if (threadIdx.x % kWave == 0) cnt[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) rowcount[i] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// One block: row_ptr = the exclusive prefix sum of rowcount (thread t owns kScanPer consecutive rows; Hillis-Steele over the threads'
// totals), n_edges = its last entry.
__global__ __launch_bounds__(kScanThreads)
void umap_scan_kernel(const int32_t* __restrict__ rowcount, int n, int32_t* __restrict__ row_ptr, int32_t* __restrict__ n_edges) {
    __shared__ int s[2][kScanThreads];
    const int t = threadIdx.x;
    int mine = 0;
    for (int r = 0; r < kScanPer; ++r) {
        const int i = t * kScanPer + r;
        mine += i < n ? rowcount[i] : 0;
    }
    int cur = 0;
    s[0][t] = mine;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {
        s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int at = s[cur][t] - mine;                                          // exclusive
    for (int r = 0; r < kScanPer; ++r) {
        const int i = t * kScanPer + r;
        if (i < n) {
            row_ptr[i] = at;
            at += rowcount[i];
        }
    }
    if (t == kScanThreads - 1) {
        row_ptr[n] = s[cur][t];
        *n_edges = s[cur][t];
    }
}

// One wave per row: the row's non-zeros in ascending column order to col / weight at row_ptr[i] (ballot + popcount of the lower lanes).
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_compact_kernel(const float* __restrict__ P, const int32_t* __restrict__ row_ptr, int n, size_t capacity,
                         int32_t* __restrict__ col, float* __restrict__ weight) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    size_t at = (size_t)row_ptr[i];
    for (int j0 = 0; j0 < n; j0 += kWave) {
        const int j = j0 + lane;
        const float p = j < n ? P[(size_t)i * n + j] : 0.f;
        const unsigned long long mask = __ballot(p != 0.f);
        const size_t slot = at + __popcll(mask & ((1ull << lane) - 1ull));
        if (p != 0.f && slot < capacity) {
            col[slot] = j;
            weight[slot] = p;
        }
        at += __popcll(mask);
    }
}

// ---- the layout ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t umap_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

// the counter-based draw of a repulsive move's other end (hash_host in umapfit.py)
__device__ __forceinline__ uint32_t umap_hash(uint32_t seed, uint32_t ep, uint32_t e, uint32_t p) {
    uint32_t h = umap_mix(seed ^ (ep * 0x9E3779B9u));
    h = umap_mix(h ^ (e * 0x85EBCA6Bu));
    return umap_mix(h ^ (p * 0xC2B2AE35u));
}

// One block: the maximum weight (a maximum has no order to fix).
__global__ __launch_bounds__(kScanThreads)
void umap_wmax_kernel(const float* __restrict__ weight, int n_edges, float* __restrict__ wmax) {
    __shared__ float part[kScanThreads / kWave];
    float m = 0.f;
    for (int e = threadIdx.x; e < n_edges; e += kScanThreads) m = fmaxf(m, weight[e]);
    m = wave_max(m);
    if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kScanThreads / kWave; ++w) m = fmaxf(m, part[w]);
        *wmax = m;
    }
}

__global__ __launch_bounds__(256)
void umap_schedule_kernel(const float* __restrict__ weight, int n_edges, const float* __restrict__ wmax, float* __restrict__ eps,
                          float* __restrict__ epn, float* __restrict__ next, float* __restrict__ next_neg) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const float s = *wmax / weight[e];
    const float q = s / 5.f;
    eps[e] = s;
    epn[e] = q;
    next[e] = s;
    next_neg[e] = q;
}

// One wave per vertex, lane c holds coordinate c (lanes past dim hold 0 and add 0 to every d^2).  Reads Yin, writes Yout.
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_epoch_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int n_edges, int dim, float a,
                       float b, int n_epochs, uint32_t seed, int ep, const float* __restrict__ eps, const float* __restrict__ epn,
                       float* __restrict__ next, float* __restrict__ next_neg, const float* __restrict__ Yin, float* __restrict__ Yout) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const bool has = lane < dim;
    const float alpha = 1.f - (float)ep / (float)n_epochs;
    const float fep = (float)ep;
    const float c_att = (-2.f * a) * b, c_rep = 2.f * b, bm1 = b - 1.f;
    const float yi = has ? Yin[(size_t)i * dim + lane] : 0.f;
    float acc = 0.f;
    const int e_lo = max(0, min(row_ptr[i], n_edges)), e_hi = max(e_lo, min(row_ptr[i + 1], n_edges));
    for (int e = e_lo; e < e_hi; ++e) {
        const float nx = next[e];
        if (!(nx <= fep)) continue;
        const int j = col[e];
        if (j >= 0 && j < n) {
            const float diff = yi - (has ? Yin[(size_t)j * dim + lane] : 0.f);
            const float d2 = wave_sum(diff * diff);
            float g = 0.f;
            if (d2 > 0.f) g = c_att * powf(d2, bm1) / (a * powf(d2, b) + 1.f);
            const float t = fminf(fmaxf(g * diff, -4.f), 4.f);
            acc = acc + (2.f * t) * alpha;
        }
        const float q = epn[e], ng = next_neg[e];
        const int n_neg = (int)((fep - ng) / q);
        for (int p = 0; p < n_neg; ++p) {
            const uint32_t k = umap_hash(seed, (uint32_t)ep, (uint32_t)e, (uint32_t)p) % (uint32_t)n;
            const float diff = yi - (has ? Yin[(size_t)k * dim + lane] : 0.f);
            const float d2 = wave_sum(diff * diff);
            if (d2 > 0.f) {
                const float g = c_rep / ((0.001f + d2) * (a * powf(d2, b) + 1.f));
                const float t = fminf(fmaxf(g * diff, -4.f), 4.f);
                acc = acc + t * alpha;
            }
        }
        if (lane == 0) {
            next[e] = nx + eps[e];
            next_neg[e] = ng + (float)n_neg * q;
        }
    }
    if (has) Yout[(size_t)i * dim + lane] = yi + acc;
}


int um_check(int n, int n_neighbors, int max_n = DM_UMAP_MAX_N) {
    if (n >= max_n) return DM_UMAP_E_N_LARGE;
    if (n_neighbors < 2 || n_neighbors > DM_UMAP_MAX_NEIGHBORS) return DM_UMAP_E_NEIGHBORS;
    if (n_neighbors >= n) return DM_UMAP_E_NEIGHBORS_GE_N;
    return 0;
}

inline int row_blocks(int rows) { return (rows + kRowWaves - 1) / kRowWaves; }

#define UM_LAUNCH(kernel, grid, block, lds, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__); \
    if (hipGetLastError() != hipSuccess) return DM_UMAP_E_HIP; } while (0)

// dm_umap_layout and dm_umap_sparse_layout: the same checks, carve and launches; only the row bound differs.
int um_run_layout(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_edges, int n_components,
                  float a, float b, int n_epochs, int seed, int first_epoch, int last_epoch, float* Y_inout, void* work, size_t work_bytes,
                  int max_n) {
    if (!row_ptr || !col || !weight || !Y_inout || !work) return DM_UMAP_E_NULL;
    if (n >= max_n) return DM_UMAP_E_N_LARGE;
    if (n < 1) return DM_UMAP_E_NEIGHBORS_GE_N;
    if (n_components < 1 || n_components > DM_UMAP_MAX_COMPONENTS) return DM_UMAP_E_COMPONENTS;
    if (n_edges < 0 || (size_t)n_edges > (size_t)2 * n * DM_UMAP_MAX_NEIGHBORS) return DM_UMAP_E_EDGES;
    if (n_epochs < 1 || first_epoch < 0 || first_epoch > last_epoch || last_epoch > n_epochs) return DM_UMAP_E_EPOCHS;
    const UmWork w = um_layout(work, n, n_components, (size_t)n_edges);
    if (work_bytes < w.layout_bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    if (first_epoch == 0 && n_edges > 0) {
        UM_LAUNCH(umap_wmax_kernel, dim3(1), dim3(kScanThreads), 0, weight, n_edges, w.wmax);
        UM_LAUNCH(umap_schedule_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, weight, n_edges, w.wmax, w.eps, w.epn, w.next, w.next_neg);
    }
    float* buf[2] = {Y_inout, w.Y2};
    int at = 0;
    for (int ep = first_epoch; ep < last_epoch; ++ep, at ^= 1)
        UM_LAUNCH(umap_epoch_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), 0, row_ptr, col, n, n_edges, n_components, a, b, n_epochs,
                  (uint32_t)seed, ep, w.eps, w.epn, w.next, w.next_neg, buf[at], buf[at ^ 1]);
    if (at == 1 && hipMemcpyAsync(Y_inout, w.Y2, (size_t)n * n_components * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return DM_UMAP_E_HIP;
    return 0;
}

}  // namespace

}  // namespace dm
