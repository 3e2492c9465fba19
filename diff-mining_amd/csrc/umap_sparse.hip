// umap_sparse.hip — the UMAP projection without the n x n graph, for n < DM_UMAP_SPARSE_MAX_N rows: dm_umap_sparse_knn,
// dm_umap_sparse_graph, dm_umap_sparse_layout, dm_umap_sparse_spectral.  The rules are umap.hip's (umapfit.py states them), and on any
// input both routes take, the results are the same bits: the arithmetic both must share (the kNN term, smooth_knn_dist, the union, the
// layout's kernels, the whole spectral solver) comes from umap_device.h and umap_spectral_device.h.  What is new here is the blocking:
//   - kNN: a workgroup owns kSkRows rows and streams column tiles of kSkCols rows, so X is read n / kSkRows times; a thread keeps one
//     fp64 sum per owned row in registers; after a tile, one wave per owned row merges the tile's distances into the row's k best keys
//     (distance bits << 32 | index).  Keys are totally ordered, so the k smallest do not depend on the tile order.  No LDS grows with n;
//   - graph: memberships stay in memb [n][k].  Row i's edges are its out-neighbours and its in-neighbours (the rows whose list holds
//     i); the in-lists are found by a scan of idx per row, in row-major order, so they come out ascending and no atomic is needed;
//     a wave then merges the two lists into the row's candidates, ascending column, and the dense route's steps follow on those:
//     global maximum, threshold, row counts, prefix sum (one block, looped with a carry), compaction;
//   - no kernel reads workspace that it, or an earlier kernel of the same call, has not written.
#include "umap_spectral_device.h"

namespace dm {

namespace {

constexpr int kSkRows = 32;                  // rows a workgroup of the kNN kernel owns: 32 fp64 sums = 64 VGPRs per thread
constexpr int kSkCols = 256;                 // columns per tile = threads
constexpr int kSkChunk = 16;                 // features per staged chunk
constexpr int kSkPitch = kSkCols + 2;        // tile[e][col]: the staging writes of a 32-lane half (16 features x 2 columns) hit 32 banks
constexpr int kSkWaves = kSkCols / kWave;
constexpr int kSrcBits = 6;                  // in_src = row << 6 | slot: slot < DM_UMAP_MAX_NEIGHBORS = 64, row < 65536
static_assert(DM_UMAP_MAX_NEIGHBORS <= (1 << kSrcBits) && DM_UMAP_MAX_NEIGHBORS <= kWave, "a row's list is one wave wide");
static_assert(kSkChunk * kSkPitch <= kSkRows * kSkCols, "the staged chunk shares the distance tile's LDS");

struct SkWork {                              // the workspace: the layout's part first (um_layout's), then the graph's
    UmWork lay;
    float *memb, *cand_p, *rowmax, *thr;     // memberships [n][k]; candidates' P [2 n k]; row maxima [n]; the threshold [1]
    int32_t *indeg, *in_ptr, *in_src, *cand_col, *candcount, *rowcount;
    size_t bytes;
};

SkWork sk_layout(void* base, int n, int k, int dim, size_t edges) {
    SkWork w;
    w.lay = um_layout(base, n, dim, edges);
    size_t off = w.lay.layout_bytes;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t N = (size_t)n, NK = N * (size_t)k;
    w.memb = (float*)take(NK * 4);
    w.indeg = (int32_t*)take(N * 4);
    w.in_ptr = (int32_t*)take((N + 1) * 4);
    w.in_src = (int32_t*)take(NK * 4);
    w.cand_col = (int32_t*)take(2 * NK * 4);
    w.cand_p = (float*)take(2 * NK * 4);
    w.candcount = (int32_t*)take(N * 4);
    w.rowmax = (float*)take(N * 4);
    w.rowcount = (int32_t*)take(N * 4);
    w.thr = (float*)take(4);
    w.bytes = off;
    return w;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(v, o, kWave);
        v = other < v ? other : v;
    }
    return v;
}

// ---- tiled exact kNN with a running top-k ------------------------------------------------------------------------------------------
// Thread t of column tile j0 holds the sums of rows i0 .. i0 + 31 against row j0 + t.  buf is the staged chunk (tile[e][col]) while the
// sums run and the tile's distance bits ([row][col]) while the waves merge.  best[r] is row r's current k smallest keys, ascending,
// one per lane, all ones where there is none yet.  A merge takes the tile's smallest remaining key while it is below the row's k-th:
// at most k times, since after k of them nothing left in the tile can be among the k smallest.
__global__ __launch_bounds__(kSkCols)
void umap_sparse_knn_kernel(const float* __restrict__ X, int n, int d, int k, int32_t* __restrict__ idx_out, float* __restrict__ dist_out) {
#pragma clang fp contract(off)
    __shared__ __align__(16) float buf[kSkRows * kSkCols];
    __shared__ __align__(16) double own[kSkChunk][kSkRows];
    __shared__ unsigned long long best[kSkRows][kWave];
    const int t = threadIdx.x, wave = t / kWave, lane = t % kWave;
    const int i0 = blockIdx.x * kSkRows;
    uint32_t* bits = (uint32_t*)buf;
    for (int q = t; q < kSkRows * kWave; q += kSkCols) best[q / kWave][q % kWave] = ~0ull;
    for (int j0 = 0; j0 < n; j0 += kSkCols) {
        double acc[kSkRows];
#pragma unroll
        for (int r = 0; r < kSkRows; ++r) acc[r] = 0.0;
        for (int e0 = 0; e0 < d; e0 += kSkChunk) {
            const int ne = min(kSkChunk, d - e0);
            __syncthreads();                                            // the previous chunk, or the previous tile's merge, has read buf
            for (int q = t; q < kSkCols * kSkChunk; q += kSkCols) {
                const int c = q / kSkChunk, e = q % kSkChunk;
                buf[e * kSkPitch + c] = (j0 + c < n && e < ne) ? X[(size_t)(j0 + c) * d + e0 + e] : 0.f;
            }
            for (int q = t; q < kSkRows * kSkChunk; q += kSkCols) {
                const int r = q / kSkChunk, e = q % kSkChunk;
                own[e][r] = (i0 + r < n && e < ne) ? (double)X[(size_t)(i0 + r) * d + e0 + e] : 0.0;
            }
            __syncthreads();
            for (int e = 0; e < ne; ++e) {
                const double xj = (double)buf[e * kSkPitch + t];
#pragma unroll
                for (int r = 0; r < kSkRows; ++r) acc[r] = knn_add(acc[r], own[e][r], xj);
            }
        }
        __syncthreads();                                                // every thread has read the last chunk
        const bool col_ok = j0 + t < n;
#pragma unroll
        for (int r = 0; r < kSkRows; ++r) bits[r * kSkCols + t] = col_ok ? __float_as_uint(knn_root(acc[r])) : 0xFFFFFFFFu;
        __syncthreads();
        for (int r = wave; r < kSkRows; r += kSkWaves) {
            if (i0 + r >= n) break;
            unsigned long long cand[kSkCols / kWave];
#pragma unroll
            for (int q = 0; q < kSkCols / kWave; ++q) {
                const int c = q * kWave + lane;
                cand[q] = j0 + c < n ? ((unsigned long long)bits[r * kSkCols + c] << 32) | (unsigned)(j0 + c) : ~0ull;
            }
            unsigned long long cur = best[r][lane];
            unsigned long long worst = __shfl(cur, k - 1, kWave);
            for (int round = 0; round < k; ++round) {
                unsigned long long m = cand[0];
#pragma unroll
                for (int q = 1; q < kSkCols / kWave; ++q) m = cand[q] < m ? cand[q] : m;
                m = wave_min_u64(m);
                if (m >= worst) break;                                  // the same in every lane
                const int pos = __popcll(__ballot(cur < m));            // cur is ascending: the lanes below pos keep theirs
                const unsigned long long up = __shfl_up(cur, 1, kWave);
                cur = lane < pos ? cur : lane == pos ? m : up;
#pragma unroll
                for (int q = 0; q < kSkCols / kWave; ++q) cand[q] = cand[q] == m ? ~0ull : cand[q];
                worst = __shfl(cur, k - 1, kWave);
            }
            best[r][lane] = cur;
        }
    }
    for (int r = wave; r < kSkRows; r += kSkWaves) {                    // the wave that merged row r wrote best[r]
        const int i = i0 + r;
        if (i >= n) break;
        const unsigned long long key = best[r][lane];
        const int j = (int)(key & 0xFFFFFFFFull);
        if (lane < k && key != ~0ull && j < n) {                        // k < n: every lane below k has a key
            idx_out[(size_t)i * k + lane] = j;
            dist_out[(size_t)i * k + lane] = __uint_as_float((uint32_t)(key >> 32));
        }
    }
}

// ---- the transpose of the lists --------------------------------------------------------------------------------------------------------
// One wave per row i scans idx in row-major order, 64 entries at a time: the entries equal to i, in rows other than i, are i's
// in-neighbours.  kFill = false counts them; kFill = true writes (row << 6 | slot) at in_ptr[i], ascending, by ballot and popcount.
template <bool kFill>
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_sparse_inlist_kernel(const int32_t* __restrict__ idx, int n, int k, int32_t* __restrict__ indeg, const int32_t* __restrict__ in_ptr,
                               int32_t* __restrict__ in_src) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const int total = n * k;                                            // < 65536 x 64
    const int own_lo = i * k, own_hi = own_lo + k;
    int at = kFill ? in_ptr[i] : 0;
    const int end = kFill ? in_ptr[i + 1] : 0;
    for (int q0 = 0; q0 < total; q0 += kWave) {
        const int q = q0 + lane;
        const bool match = q < total && idx[q] == i && (q < own_lo || q >= own_hi);
        const unsigned long long mask = __ballot(match);
        if (kFill && match) {
            const int slot = at + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < end) in_src[slot] = ((q / k) << kSrcBits) | (q % k);
        }
        at += __popcll(mask);
    }
    if (!kFill && lane == 0) indeg[i] = at;
}

// One block: ptr = the exclusive prefix sum of count [n], ptr[n] = the total (also to total_out if given).  1024 rows per pass, the
// passes chained by a carry: any n.
__global__ __launch_bounds__(kScanThreads)
void umap_sparse_scan_kernel(const int32_t* __restrict__ count, int n, int32_t* __restrict__ ptr, int32_t* __restrict__ total_out) {
    __shared__ int s[2][kScanThreads];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n; base += kScanThreads) {
        const int i = base + t;
        const int mine = i < n ? count[i] : 0;
        int cur = 0;
        s[0][t] = mine;
        __syncthreads();
        for (int o = 1; o < kScanThreads; o <<= 1) {
            s[cur ^ 1][t] = s[cur][t] + (t >= o ? s[cur][t - o] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (i < n) ptr[i] = carry + s[cur][t] - mine;
        carry += s[cur][kScanThreads - 1];
        __syncthreads();                                                // s is rewritten by the next pass
    }
    if (t == 0) {
        ptr[n] = carry;
        if (total_out) *total_out = carry;
    }
}

// ---- the union on the lists ---------------------------------------------------------------------------------------------------------------
// One wave per row i.  Lane s holds out-neighbour s (column idx[i][s], membership a_i,col); the in-list is ascending by row.  The row's
// candidates are the in-list's rows plus the out-neighbours that are not in it, merged in ascending column: an in-entry's place is its
// place in the in-list plus the out-only columns below it, an out-only entry's place is the in-entries below its column plus the
// out-only columns below it.  P = umap_union_p(a_ij, a_ji), an absent side 0.  Candidates go to cand_col / cand_p at in_ptr[i] + i k
// (at most k + in-degree of them), their number to candcount, the row's maximum to rowmax.
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_sparse_union_kernel(const int32_t* __restrict__ idx, const float* __restrict__ memb, const int32_t* __restrict__ in_ptr,
                              const int32_t* __restrict__ in_src, int n, int k, int32_t* __restrict__ cand_col, float* __restrict__ cand_p,
                              int32_t* __restrict__ candcount, float* __restrict__ rowmax) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const bool has = lane < k;
    const int oc = has ? idx[(size_t)i * k + lane] : -1;
    const float oa = has ? memb[(size_t)i * k + lane] : 0.f;
    const bool ov = has && oc >= 0 && oc < n && oc != i;
    const int lo = max(0, min(in_ptr[i], n * k)), hi = max(lo, min(in_ptr[i + 1], n * k));
    const int L = hi - lo;
    int lb = 0;                                                         // in-entries with a row below oc
    if (ov) {
        int a = 0, b = L;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if ((in_src[lo + mid] >> kSrcBits) < oc) a = mid + 1; else b = mid;
        }
        lb = a;
    }
    const bool mutual = ov && lb < L && (in_src[lo + lb] >> kSrcBits) == oc;
    const bool oonly = ov && !mutual;
    int orank = 0;                                                      // out-only columns below mine (a repeated column: the lower lane first)
    for (int s = 0; s < k; ++s) {
        const int c = __shfl(oc, s, kWave);
        const int f = __shfl((int)oonly, s, kWave);
        orank += (f && (c < oc || (c == oc && s < lane))) ? 1 : 0;
    }
    const size_t base = (size_t)lo + (size_t)i * k;
    float m = 0.f;
    if (oonly) {
        const float p = umap_union_p(oa, 0.f);
        cand_col[base + lb + orank] = oc;
        cand_p[base + lb + orank] = p;
        m = fmaxf(m, p);
    }
    for (int r0 = 0; r0 < L; r0 += kWave) {
        const int r = r0 + lane;
        const bool valid = r < L;
        const int src = valid ? in_src[lo + r] : 0;
        const int j = src >> kSrcBits, sl = src & ((1 << kSrcBits) - 1);
        const bool src_ok = valid && j < n && sl < k;                   // umap_sparse_inlist_kernel wrote it so
        const float at = src_ok ? memb[(size_t)j * k + sl] : 0.f;
        float a = 0.f;
        int below = 0;
        for (int s = 0; s < k; ++s) {
            const int c = __shfl(oc, s, kWave);
            const int v = __shfl((int)ov, s, kWave);
            const int f = __shfl((int)oonly, s, kWave);
            const float av = __shfl(oa, s, kWave);
            a = (v && c == j) ? av : a;
            below += (f && c < j) ? 1 : 0;
        }
        if (valid) {
            const float p = umap_union_p(a, at);
            cand_col[base + r + below] = j;
            cand_p[base + r + below] = p;
            m = fmaxf(m, p);
        }
    }
    m = wave_max(m);
    const int n_only = __popcll(__ballot(oonly));
    if (lane == 0) {
        rowmax[i] = m;
        candcount[i] = L + n_only;
    }
}

// One block: the threshold max(P) / n_epochs (umap_prune_kernel's, once).
__global__ __launch_bounds__(kScanThreads)
void umap_sparse_threshold_kernel(const float* __restrict__ rowmax, int n, int n_epochs, float* __restrict__ thr) {
    __shared__ float part[kScanThreads / kWave];
    float m = 0.f;
    for (int j = threadIdx.x; j < n; j += kScanThreads) m = fmaxf(m, rowmax[j]);
    m = wave_max(m);
    if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kScanThreads / kWave; ++w) m = fmaxf(m, part[w]);
        *thr = m / (float)n_epochs;
    }
}

// a candidate survives the pruning as an entry of the dense P does: not below the threshold, and not 0
__device__ __forceinline__ bool sk_kept(float p, float thr) { return !(p < thr) && p != 0.f; }

// One wave per row.  kWrite = false: the row's count of surviving candidates.  kWrite = true: they go to col / weight at row_ptr[i],
// in the candidates' order (ascending column).
template <bool kWrite>
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_sparse_compact_kernel(const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ cand_col, const float* __restrict__ cand_p,
                                const int32_t* __restrict__ candcount, const float* __restrict__ thr_p, int n, int k,
                                int32_t* __restrict__ rowcount, const int32_t* __restrict__ row_ptr, size_t capacity,
                                int32_t* __restrict__ col, float* __restrict__ weight) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const float thr = *thr_p;
    const size_t base = (size_t)max(0, min(in_ptr[i], n * k)) + (size_t)i * k;
    const int cnt = max(0, min(candcount[i], (int)(2 * (size_t)n * k - base)));        // base < 2 n k
    size_t at = kWrite ? (size_t)max(0, row_ptr[i]) : 0;
    for (int r0 = 0; r0 < cnt; r0 += kWave) {
        const int r = r0 + lane;
        const float p = r < cnt ? cand_p[base + r] : 0.f;
        const bool keep = r < cnt && sk_kept(p, thr);
        const unsigned long long mask = __ballot(keep);
        if (kWrite && keep) {
            const size_t slot = at + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < capacity) {
                col[slot] = cand_col[base + r];
                weight[slot] = p;
            }
        }
        at += __popcll(mask);
    }
    if (!kWrite && lane == 0) rowcount[i] = (int)at;
}

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

int dm_umap_sparse_workspace_bytes(int n, int d, int n_neighbors, int n_components, size_t* bytes_out) {
    if (!bytes_out) return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors, DM_UMAP_SPARSE_MAX_N)) return rc;
    if (n_components < 1 || n_components > DM_UMAP_MAX_COMPONENTS) return DM_UMAP_E_COMPONENTS;
    if (d < 1) return DM_UMAP_E_D;
    *bytes_out = sk_layout(nullptr, n, n_neighbors, n_components, (size_t)2 * n * n_neighbors).bytes;
    return 0;
}

int dm_umap_sparse_knn(void* stream, const void* X, int n, int d, int n_neighbors, void* work, size_t work_bytes, int32_t* idx_out,
                       float* dist_out) {
    if (!X || !work || !idx_out || !dist_out) return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors, DM_UMAP_SPARSE_MAX_N)) return rc;
    if (d < 1) return DM_UMAP_E_D;
    if (work_bytes < sk_layout(nullptr, n, n_neighbors, 1, (size_t)2 * n * n_neighbors).bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    UM_LAUNCH(umap_sparse_knn_kernel, dim3((n + kSkRows - 1) / kSkRows), dim3(kSkCols), 0, (const float*)X, n, d, n_neighbors, idx_out,
              dist_out);
    return 0;
}

int dm_umap_sparse_graph(void* stream, const int32_t* idx, const float* dist, int n, int n_neighbors, int n_epochs, void* work,
                         size_t work_bytes, float* rho_out, float* sigma_out, int32_t* row_ptr_out, int32_t* col_out, float* weight_out,
                         int32_t* n_edges_out) {
    if (!idx || !dist || !work || !rho_out || !sigma_out || !row_ptr_out || !col_out || !weight_out || !n_edges_out) return DM_UMAP_E_NULL;
    if (int rc = um_check(n, n_neighbors, DM_UMAP_SPARSE_MAX_N)) return rc;
    if (n_epochs < 1) return DM_UMAP_E_EPOCHS;
    const int k = n_neighbors;
    const size_t capacity = (size_t)2 * n * k;
    const SkWork w = sk_layout(work, n, k, 1, capacity);
    if (work_bytes < w.bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 rows(row_blocks(n)), row_threads(kRowWaves * kWave), one(1), scan_threads(kScanThreads);
    UM_LAUNCH(umap_smooth_kernel<false>, rows, row_threads, 0, idx, dist, n, k, rho_out, sigma_out, w.memb);
    UM_LAUNCH(umap_sparse_inlist_kernel<false>, rows, row_threads, 0, idx, n, k, w.indeg, (const int32_t*)nullptr, (int32_t*)nullptr);
    UM_LAUNCH(umap_sparse_scan_kernel, one, scan_threads, 0, w.indeg, n, w.in_ptr, (int32_t*)nullptr);
    UM_LAUNCH(umap_sparse_inlist_kernel<true>, rows, row_threads, 0, idx, n, k, (int32_t*)nullptr, w.in_ptr, w.in_src);
    UM_LAUNCH(umap_sparse_union_kernel, rows, row_threads, 0, idx, w.memb, w.in_ptr, w.in_src, n, k, w.cand_col, w.cand_p, w.candcount,
              w.rowmax);
    UM_LAUNCH(umap_sparse_threshold_kernel, one, scan_threads, 0, w.rowmax, n, n_epochs, w.thr);
    UM_LAUNCH(umap_sparse_compact_kernel<false>, rows, row_threads, 0, w.in_ptr, w.cand_col, w.cand_p, w.candcount, w.thr, n, k, w.rowcount,
              (const int32_t*)nullptr, capacity, (int32_t*)nullptr, (float*)nullptr);
    UM_LAUNCH(umap_sparse_scan_kernel, one, scan_threads, 0, w.rowcount, n, row_ptr_out, n_edges_out);
    UM_LAUNCH(umap_sparse_compact_kernel<true>, rows, row_threads, 0, w.in_ptr, w.cand_col, w.cand_p, w.candcount, w.thr, n, k,
              (int32_t*)nullptr, row_ptr_out, capacity, col_out, weight_out);
    return 0;
}

int dm_umap_sparse_layout(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_edges,
                          int n_components, float a, float b, int n_epochs, int seed, int first_epoch, int last_epoch, float* Y_inout,
                          void* work, size_t work_bytes) {
    return um_run_layout(stream, row_ptr, col, weight, n, n_edges, n_components, a, b, n_epochs, seed, first_epoch, last_epoch, Y_inout,
                         work, work_bytes, DM_UMAP_SPARSE_MAX_N);
}

int dm_umap_sparse_spectral_workspace_bytes(int n, int n_components, size_t* bytes_out) {
    return sp_workspace_bytes(n, n_components, bytes_out, DM_UMAP_SPARSE_MAX_N);
}

int dm_umap_sparse_spectral(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_components, int seed,
                            const float* noise, const float* fallback, void* work, size_t work_bytes, float* Y0_out, double* eigvals_out,
                            double* eigvecs_out, double* status_out) {
    return sp_run(stream, row_ptr, col, weight, n, n_components, seed, noise, fallback, work, work_bytes, Y0_out, eigvals_out, eigvecs_out,
                  status_out, DM_UMAP_SPARSE_MAX_N);
}

}  // extern "C"
