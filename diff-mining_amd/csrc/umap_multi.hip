// umap_multi.hip — UMAP's spectral initialisation on a disconnected graph: every connected component gets its own
// spectral embedding, placed around a meta-embedding of the components.  The rules are stated in numpy in umapfit.py
// (`component_groups_host`, `meta_embedding_host`, `multi_component_init_host`: a restatement of umap-learn's multi_component_layout,
// PARITY UNPINNED); this file follows them step by step.  One set of entries for both routes (n < DM_UMAP_SPARSE_MAX_N, no n x n
// buffer).
//
// Structure, as in umap_sparse.hip:
//   - no floating-point atomic and no integer one either: components are counted and grouped by ballot + popcount, a wave per
//     component, so the grouping permutation is the stable one by construction; every prefix sum is the one-workgroup scan with a
//     looped carry per thread; the centroid of a component is one thread per feature adding the rows in ascending index;
//   - dm_umap_components never waits for the device; the host reads c, the offsets and the edge offsets once, decides the plan, and
//     dm_umap_multi_init enqueues the existing solver (sp_run: its launches and its status record) per solvable component on that
//     component's own CSR slice, then three small kernels; nothing in it waits either;
//   - no kernel reads workspace that it, or an earlier kernel of the same call, has not written.
#include "umap_spectral_device.h"

namespace dm {

namespace {

constexpr int kCentThreads = 128;            // umap_multi_centroid_kernel: features per pass
constexpr int kPlaceThreads = 256;           // umap_multi_place_kernel: entries of R per block

struct McWork {                              // dm_umap_components' workspace
    SpState* st;
    int32_t *label, *flag, *rootrank, *size, *inv, *subcount, *gp;
    size_t bytes;
};

McWork mc_layout(void* base, int n) {
    McWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t N = (size_t)n;
    w.st = (SpState*)take(sizeof(SpState));
    w.label = (int32_t*)take(N * 4);
    w.flag = (int32_t*)take(N * 4);
    w.rootrank = (int32_t*)take((N + 1) * 4);
    w.size = (int32_t*)take(N * 4);
    w.inv = (int32_t*)take(N * 4);
    w.subcount = (int32_t*)take(N * 4);
    w.gp = (int32_t*)take((N + 1) * 4);
    w.bytes = off;
    return w;
}

struct MiWork {                              // dm_umap_multi_init's workspace
    void* sp;                                // the solver's, sized for a component of n rows (the largest any can be)
    size_t sp_bytes;
    float* Y0;                               // the solver's own Y0 goes here and is not used
    double *sign, *emax, *part;
    size_t bytes;
};

inline int place_blocks(int n, int dim) { return (int)(((size_t)n * dim + kPlaceThreads - 1) / kPlaceThreads); }

MiWork mi_layout(void* base, int n, int dim) {
    MiWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    w.sp_bytes = sp_layout(nullptr, n, sp_block(n, dim), true).bytes;
    w.sp = take(w.sp_bytes);
    w.Y0 = (float*)take((size_t)n * dim * 4);
    w.sign = (double*)take((size_t)DM_UMAP_MULTI_MAX_COMP * dim * 8);
    w.emax = (double*)take((size_t)DM_UMAP_MULTI_MAX_COMP * 8);
    w.part = (double*)take((size_t)place_blocks(n, dim) * 8);
    w.bytes = off;
    return w;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return max(lo, min(v, hi)); }

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double other = __shfl_xor(v, o, kWave);
        v = other > v ? other : v;
    }
    return v;
}

// ---- labels --------------------------------------------------------------------------------------------------------------------------
// One workgroup: the min-label propagation of the spectral solver (components_body), then flag[i] = 1 where vertex i is its
// component's smallest vertex.
__global__ __launch_bounds__(kOneThreads)
void umap_multi_label_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int* glabel,
                             int32_t* __restrict__ flag, SpState* __restrict__ st) {
    components_body(row_ptr, col, n, 0, (volatile int*)glabel, st);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kOneThreads) flag[i] = ((volatile int*)glabel)[i] == i ? 1 : 0;
}

// One workgroup: out[0 .. count] = the exclusive prefix sum of in[0 .. count) (thread t owns `per` consecutive entries and carries
// its sum through them; Hillis-Steele over the threads' totals, as umap_scan_kernel), out[count + 1 .. fill_to] = the total.
// count = *count_ptr (clamped to count_max) or count_max.
__global__ __launch_bounds__(kScanThreads)
void umap_multi_scan_kernel(const int32_t* __restrict__ in, const int32_t* __restrict__ count_ptr, int count_max, int32_t* __restrict__ out,
                            int fill_to, int32_t* __restrict__ total_out) {
    __shared__ int s[2][kScanThreads];
    const int t = threadIdx.x;
    const int count = count_ptr ? clampi(*count_ptr, 0, count_max) : count_max;
    const int per = (count + kScanThreads - 1) / kScanThreads;
    int mine = 0;
    for (int r = 0; r < per; ++r) {
        const int i = t * per + r;
        mine += i < count ? in[i] : 0;
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
    for (int r = 0; r < per; ++r) {
        const int i = t * per + r;
        if (i < count) {
            out[i] = at;
            at += in[i];
        }
    }
    const int total = s[cur][kScanThreads - 1];
    for (int j = count + t; j <= fill_to; j += kScanThreads) out[j] = total;
    if (t == 0 && total_out) *total_out = total;
}

// comp_i = the rank of vertex i's label among the roots: ids ascend with each component's smallest vertex
__global__ __launch_bounds__(256)
void umap_multi_comp_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ rootrank, int n, int32_t* __restrict__ comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    comp[i] = rootrank[clampi(label[i], 0, n - 1)];
}

// One wave per component l < c.  kPlace = false: size[l] = its vertex count.  kPlace = true: its vertices in ascending index to
// perm[offsets[l] ...] (ballot + popcount of the lower lanes) and inv = perm's inverse.
template <bool kPlace>
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_multi_group_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ count, int n, const int32_t* __restrict__ offsets,
                             int32_t* __restrict__ size, int32_t* __restrict__ perm, int32_t* __restrict__ inv) {
    const int lane = threadIdx.x % kWave;
    const int l = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (l >= n || l >= *count) return;
    int at = kPlace ? offsets[l] : 0;
    for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        const bool mine = i < n && comp[i] == l;
        const unsigned long long mask = __ballot(mine);
        if (kPlace && mine) {
            const int slot = at + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < n) {
                perm[slot] = i;
                inv[i] = slot;
            }
        }
        at += __popcll(mask);
    }
    if (!kPlace && lane == 0) size[l] = at;
}

// One wave per grouped row g (vertex i = perm[g]).  kWrite = false: subcount[g] = the row's edges that stay inside its component.
// kWrite = true: those edges, in edge order, to sub_col / sub_weight at gp[g], the column as the position inside the component; the
// component's own row pointer (gp relative to the component's first edge) at sub_row_ptr[g + l].
template <bool kWrite>
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_multi_sub_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const float* __restrict__ weight, int n,
                           int edge_capacity, const int32_t* __restrict__ comp, const int32_t* __restrict__ perm,
                           const int32_t* __restrict__ inv, const int32_t* __restrict__ offsets, const int32_t* __restrict__ gp,
                           int32_t* __restrict__ subcount, int32_t* __restrict__ sub_row_ptr, int32_t* __restrict__ sub_col,
                           float* __restrict__ sub_weight) {
    const int lane = threadIdx.x % kWave;
    const int g = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (g >= n) return;
    const int i = clampi(perm[g], 0, n - 1);
    const int l = comp[i];
    const int lo = clampi(row_ptr[i], 0, edge_capacity), hi = clampi(row_ptr[i + 1], lo, edge_capacity);
    int off = 0, at = 0;
    if (kWrite) {
        off = clampi(offsets[clampi(l, 0, n - 1)], 0, n - 1);
        const int first = gp[off];
        at = gp[g];
        if (lane == 0) {
            sub_row_ptr[g + l] = at - first;
            if (g + 1 == offsets[clampi(l, 0, n - 1) + 1]) sub_row_ptr[g + 1 + l] = gp[g + 1] - first;
        }
    }
    int kept = 0;
    for (int e0 = lo; e0 < hi; e0 += kWave) {
        const int e = e0 + lane;
        const int j = e < hi ? col[e] : -1;
        const bool keep = j >= 0 && j < n && comp[j] == l;
        const unsigned long long mask = __ballot(keep);
        if (kWrite && keep) {
            const int slot = at + kept + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < edge_capacity) {
                sub_col[slot] = inv[j] - off;
                sub_weight[slot] = weight[e];
            }
        }
        kept += __popcll(mask);
    }
    if (!kWrite && lane == 0) subcount[g] = kept;
}

// edge_offsets[l] = the first edge slot of component l (the total past c); the unused end of sub_row_ptr is zeroed
__global__ __launch_bounds__(256)
void umap_multi_finish_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ offsets, const int32_t* __restrict__ gp, int n,
                              int32_t* __restrict__ edge_offsets, int32_t* __restrict__ sub_row_ptr) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    const int c = clampi(*count, 0, n);
    edge_offsets[j] = j < c ? gp[clampi(offsets[j], 0, n)] : gp[n];
    const int q = n + c + j;
    if (q <= 2 * n) sub_row_ptr[q] = 0;
}

// Block l < min(n, DM_UMAP_MULTI_MAX_COMP), thread = feature: the component's rows added in ascending vertex index in fp64 (grouped
// order is that order), divided by the size.  Four loads are issued ahead of their adds; the adds stay in order.
__global__ __launch_bounds__(kCentThreads)
void umap_multi_centroid_kernel(const float* __restrict__ X, int n, int d, const int32_t* __restrict__ count,
                                const int32_t* __restrict__ offsets, const int32_t* __restrict__ perm, double* __restrict__ cent) {
#pragma clang fp contract(off)
    const int l = blockIdx.x;
    const bool live = l < *count;
    const int lo = live ? clampi(offsets[l], 0, n) : 0, hi = live ? clampi(offsets[l + 1], lo, n) : 0;
    for (int e = threadIdx.x; e < d; e += kCentThreads) {
        double s = 0.0;
        int g = lo;
        for (; g + 4 <= hi; g += 4) {
            const double x0 = (double)X[(size_t)clampi(perm[g], 0, n - 1) * d + e];
            const double x1 = (double)X[(size_t)clampi(perm[g + 1], 0, n - 1) * d + e];
            const double x2 = (double)X[(size_t)clampi(perm[g + 2], 0, n - 1) * d + e];
            const double x3 = (double)X[(size_t)clampi(perm[g + 3], 0, n - 1) * d + e];
            s = s + x0;
            s = s + x1;
            s = s + x2;
            s = s + x3;
        }
        for (; g < hi; ++g) s = s + (double)X[(size_t)clampi(perm[g], 0, n - 1) * d + e];
        cent[(size_t)l * d + e] = live ? s / (double)(hi - lo) : 0.0;
    }
}

// ---- after the solves ----------------------------------------------------------------------------------------------------------------
// Block l < c, wave per column (striding).  A solved component: the sign of each of eigenvectors 1 .. dim's largest-magnitude entry
// (the first one on a tie, numpy's argmax) and max|E| over all of them.  A uniform one: its status record, and zeros where the solver
// would have written.
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_multi_sign_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ plan, int n, int dim,
                            double* __restrict__ eigvecs, double* __restrict__ eigvals, double* __restrict__ status, double* __restrict__ sign,
                            double* __restrict__ emax) {
    __shared__ double colmax[DM_UMAP_MAX_COMPONENTS];
    const int l = blockIdx.x, t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    const int m = dim + 1;
    const int off = clampi(offsets[l], 0, n), rows = clampi(offsets[l + 1] - off, 0, n - off);
    if (!plan[l]) {
        for (int q = t; q < rows * m; q += kRowWaves * kWave) eigvecs[(size_t)off * m + q] = 0.0;
        for (int q = t; q < m; q += kRowWaves * kWave) eigvals[(size_t)l * m + q] = 0.0;
        for (int q = t; q < dim; q += kRowWaves * kWave) sign[(size_t)l * dim + q] = 0.0;
        if (t < 8) status[(size_t)l * 8 + t] = t == 0 ? 2.0 : t == 1 ? 1.0 : t == 4 ? __longlong_as_double(0x7FF8000000000000ll) : 0.0;
        if (t == 0) emax[l] = 1.0;
        return;
    }
    for (int j = wave; j < dim; j += kRowWaves) {
        double ba = -1.0, bv = 0.0;
        int br = 0;
        for (int r = lane; r < rows; r += kWave) {
            const double v = eigvecs[(size_t)(off + r) * m + 1 + j];
            if (fabs(v) > ba) {
                ba = fabs(v);
                bv = v;
                br = r;
            }
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const double oa = __shfl_xor(ba, o, kWave), ov = __shfl_xor(bv, o, kWave);
            const int orow = __shfl_xor(br, o, kWave);
            if (oa > ba || (oa == ba && orow < br)) {
                ba = oa;
                bv = ov;
                br = orow;
            }
        }
        if (lane == 0) {
            sign[(size_t)l * dim + j] = bv > 0.0 ? 1.0 : bv < 0.0 ? -1.0 : bv;      // numpy.sign
            colmax[j] = ba;
        }
    }
    __syncthreads();
    if (t == 0) {
        double g = colmax[0];
        for (int j = 1; j < dim; ++j) g = colmax[j] > g ? colmax[j] : g;
        emax[l] = g;
    }
}

// Thread per entry (g, j) of the grouped order: R[perm[g]][j] = E (range / max|E|) + meta for a solved component, meta + range unit
// for a uniform one; each block's max|R| to part[block] (a maximum has no order to fix).
__global__ __launch_bounds__(kPlaceThreads)
void umap_multi_place_kernel(const int32_t* __restrict__ perm, const int32_t* __restrict__ comp, const int32_t* __restrict__ plan, int n,
                             int n_comp, int dim, const double* __restrict__ eigvecs, const double* __restrict__ sign,
                             const double* __restrict__ emax, const double* __restrict__ meta, const double* __restrict__ range,
                             const double* __restrict__ unit, double* __restrict__ R, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double wmax[kPlaceThreads / kWave];
    const size_t q = (size_t)blockIdx.x * kPlaceThreads + threadIdx.x;
    double a = 0.0;
    if (q < (size_t)n * dim) {
        const int g = (int)(q / dim), j = (int)(q % dim);
        const int i = clampi(perm[g], 0, n - 1);
        const int l = clampi(comp[i], 0, n_comp - 1);
        const double mt = meta[(size_t)l * dim + j], rg = range[l];
        double r;
        if (plan[l]) {
            const double v = eigvecs[(size_t)g * (dim + 1) + 1 + j] * sign[(size_t)l * dim + j];
            r = v * (rg / emax[l]) + mt;
        } else {
            r = mt + rg * unit[(size_t)i * dim + j];
        }
        R[(size_t)i * dim + j] = r;
        a = fabs(r);
    }
    a = wave_max_f64(a);
    if (threadIdx.x % kWave == 0) wmax[threadIdx.x / kWave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kPlaceThreads / kWave; ++w) a = wmax[w] > a ? wmax[w] : a;
        part[blockIdx.x] = a;
    }
}

// One workgroup; lane = coordinate, the 16 waves stripe the rows: the end of umap_tail_kernel on R.  10 / max|R| in fp64, the fp32
// cast, the noise added in fp32, then per coordinate 10 (y - lo) / (hi - lo), every fp32 operation rounded on its own.
__global__ __launch_bounds__(kOneThreads)
void umap_multi_tail_kernel(const double* __restrict__ R, const double* __restrict__ part, int n_part, int n, int dim,
                            const float* __restrict__ noise, float* __restrict__ Y0) {
#pragma clang fp contract(off)
    constexpr int kWaves = kOneThreads / kWave;
    __shared__ double gmax_s[kWaves];
    __shared__ float lo_s[kWaves][kWave], hi_s[kWaves][kWave];
    __shared__ float lo_c[kWave], hi_c[kWave];
    __shared__ double scale_s;
    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    double g = 0.0;
    for (int q = t; q < n_part; q += kOneThreads) g = part[q] > g ? part[q] : g;
    g = wave_max_f64(g);
    if (lane == 0) gmax_s[wave] = g;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) g = gmax_s[w] > g ? gmax_s[w] : g;
        scale_s = 10.0 / g;
    }
    __syncthreads();
    const bool has = lane < dim;
    {
        float lo = INFINITY, hi = -INFINITY;
        if (has) {
            const double sc = scale_s;
            for (int i = wave; i < n; i += kWaves) {
                const float y = (float)(R[(size_t)i * dim + lane] * sc) + noise[(size_t)i * dim + lane];
                Y0[(size_t)i * dim + lane] = y;
                lo = fminf(lo, y);
                hi = fmaxf(hi, y);
            }
        }
        lo_s[wave][lane] = lo;
        hi_s[wave][lane] = hi;
    }
    __syncthreads();
    if (wave == 0) {
        float lo = lo_s[0][lane], hi = hi_s[0][lane];
        for (int w = 1; w < kWaves; ++w) {
            lo = fminf(lo, lo_s[w][lane]);
            hi = fmaxf(hi, hi_s[w][lane]);
        }
        lo_c[lane] = lo;
        hi_c[lane] = hi;
    }
    __syncthreads();
    if (has) {
        const float lo = lo_c[lane];
        const float den = hi_c[lane] - lo;
        for (int i = wave; i < n; i += kWaves) {                       // the thread that wrote the entry reads it back
            const float d = Y0[(size_t)i * dim + lane] - lo;
            const float s10 = 10.0f * d;
            Y0[(size_t)i * dim + lane] = (float)((double)s10 / (double)den);
        }
    }
}

int mc_check(int n) {
    if (n >= DM_UMAP_SPARSE_MAX_N) return DM_UMAP_E_N_LARGE;
    if (n < 1) return DM_UMAP_E_NEIGHBORS_GE_N;
    return 0;
}

}  // namespace

}  // namespace dm

using namespace dm;

extern "C" {

int dm_umap_components_workspace_bytes(int n, size_t* bytes_out) {
    if (!bytes_out) return DM_UMAP_E_NULL;
    if (int rc = mc_check(n)) return rc;
    *bytes_out = mc_layout(nullptr, n).bytes;
    return 0;
}

int dm_umap_components(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, const float* X, int n, int d,
                       int edge_capacity, void* work, size_t work_bytes, int32_t* comp_out, int32_t* count_out, int32_t* offsets_out,
                       int32_t* perm_out, int32_t* edge_offsets_out, int32_t* sub_row_ptr_out, int32_t* sub_col_out,
                       float* sub_weight_out, double* centroids_out) {
    if (!row_ptr || !col || !weight || !work || !comp_out || !count_out || !offsets_out || !perm_out || !edge_offsets_out ||
        !sub_row_ptr_out || !sub_col_out || !sub_weight_out || (X && !centroids_out))
        return DM_UMAP_E_NULL;
    if (int rc = mc_check(n)) return rc;
    if (X && d < 1) return DM_UMAP_E_D;
    if (edge_capacity < 0 || (size_t)edge_capacity > (size_t)2 * n * DM_UMAP_MAX_NEIGHBORS) return DM_UMAP_E_EDGES;
    const McWork w = mc_layout(work, n);
    if (work_bytes < w.bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 one(1), one_threads(kOneThreads), scan_threads(kScanThreads), rows(row_blocks(n)), row_threads(kRowWaves * kWave);
    const dim3 flat((n + 1 + 255) / 256), flat_threads(256);
    const int32_t* none = nullptr;
    SP_LAUNCH(umap_multi_label_kernel, one, one_threads, 0, row_ptr, col, n, (int*)w.label, w.flag, w.st);
    SP_LAUNCH(umap_multi_scan_kernel, one, scan_threads, 0, w.flag, none, n, w.rootrank, n, count_out);
    SP_LAUNCH(umap_multi_comp_kernel, flat, flat_threads, 0, w.label, w.rootrank, n, comp_out);
    SP_LAUNCH(umap_multi_group_kernel<false>, rows, row_threads, 0, comp_out, count_out, n, none, w.size, (int32_t*)nullptr, (int32_t*)nullptr);
    SP_LAUNCH(umap_multi_scan_kernel, one, scan_threads, 0, w.size, count_out, n, offsets_out, n, (int32_t*)nullptr);
    SP_LAUNCH(umap_multi_group_kernel<true>, rows, row_threads, 0, comp_out, count_out, n, offsets_out, (int32_t*)nullptr, perm_out, w.inv);
    SP_LAUNCH(umap_multi_sub_kernel<false>, rows, row_threads, 0, row_ptr, col, weight, n, edge_capacity, comp_out, perm_out, w.inv,
              offsets_out, none, w.subcount, (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr);
    SP_LAUNCH(umap_multi_scan_kernel, one, scan_threads, 0, w.subcount, none, n, w.gp, n, (int32_t*)nullptr);
    SP_LAUNCH(umap_multi_sub_kernel<true>, rows, row_threads, 0, row_ptr, col, weight, n, edge_capacity, comp_out, perm_out, w.inv,
              offsets_out, w.gp, (int32_t*)nullptr, sub_row_ptr_out, sub_col_out, sub_weight_out);
    SP_LAUNCH(umap_multi_finish_kernel, flat, flat_threads, 0, count_out, offsets_out, w.gp, n, edge_offsets_out, sub_row_ptr_out);
    if (X) {
        const int blocks = n < DM_UMAP_MULTI_MAX_COMP ? n : DM_UMAP_MULTI_MAX_COMP;
        SP_LAUNCH(umap_multi_centroid_kernel, dim3(blocks), dim3(kCentThreads), 0, X, n, d, count_out, offsets_out, perm_out, centroids_out);
    }
    return 0;
}

int dm_umap_multi_workspace_bytes(int n, int n_components, size_t* bytes_out) {
    if (!bytes_out) return DM_UMAP_E_NULL;
    if (int rc = sp_check(n, n_components, DM_UMAP_SPARSE_MAX_N)) return rc;
    *bytes_out = mi_layout(nullptr, n, n_components).bytes;
    return 0;
}

int dm_umap_multi_init(void* stream, const int32_t* sub_row_ptr, const int32_t* sub_col, const float* sub_weight, const int32_t* perm,
                       const int32_t* comp, const int32_t* offsets, const int32_t* plan, const int32_t* offsets_host,
                       const int32_t* edge_offsets_host, const int32_t* plan_host, int n, int n_comp, int edge_capacity, int n_components,
                       int seed, const double* meta, const double* range, const double* unit, const float* noise, void* work,
                       size_t work_bytes, float* Y0_out, double* R_out, double* eigvals_out, double* eigvecs_out, double* status_out) {
    if (!sub_row_ptr || !sub_col || !sub_weight || !perm || !comp || !offsets || !plan || !offsets_host || !edge_offsets_host ||
        !plan_host || !meta || !range || !unit || !noise || !work || !Y0_out || !R_out || !eigvals_out || !eigvecs_out || !status_out)
        return DM_UMAP_E_NULL;
    if (int rc = sp_check(n, n_components, DM_UMAP_SPARSE_MAX_N)) return rc;
    if (n_comp < 1 || n_comp > DM_UMAP_MULTI_MAX_COMP || n_comp > n) return DM_UMAP_E_COUNT;
    if (edge_capacity < 0 || (size_t)edge_capacity > (size_t)2 * n * DM_UMAP_MAX_NEIGHBORS) return DM_UMAP_E_EDGES;
    if (offsets_host[0] != 0 || offsets_host[n_comp] != n || edge_offsets_host[0] < 0 || edge_offsets_host[n_comp] > edge_capacity)
        return DM_UMAP_E_EDGES;
    for (int l = 0; l < n_comp; ++l) {
        if (offsets_host[l + 1] <= offsets_host[l] || edge_offsets_host[l + 1] < edge_offsets_host[l]) return DM_UMAP_E_EDGES;
        if (plan_host[l] && offsets_host[l + 1] - offsets_host[l] <= n_components + 1) return DM_UMAP_E_NEIGHBORS_GE_N;
    }
    const MiWork w = mi_layout(work, n, n_components);
    if (work_bytes < w.bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    const int m = n_components + 1;
    for (int l = 0; l < n_comp; ++l) {
        if (!plan_host[l]) continue;
        const int off = offsets_host[l], rows = offsets_host[l + 1] - off, eoff = edge_offsets_host[l];
        const float* some = noise + (size_t)off * n_components;          // the solver's noise and fallback: its own Y0 is not used
        if (int rc = sp_run(stream, sub_row_ptr + off + l, sub_col + eoff, sub_weight + eoff, rows, n_components, seed, some, some, w.sp,
                            w.sp_bytes, w.Y0, eigvals_out + (size_t)l * m, eigvecs_out + (size_t)off * m, status_out + (size_t)l * 8,
                            DM_UMAP_SPARSE_MAX_N))
            return rc;
    }
    const int blocks = place_blocks(n, n_components);
    SP_LAUNCH(umap_multi_sign_kernel, dim3(n_comp), dim3(kRowWaves * kWave), 0, offsets, plan, n, n_components, eigvecs_out, eigvals_out,
              status_out, w.sign, w.emax);
    SP_LAUNCH(umap_multi_place_kernel, dim3(blocks), dim3(kPlaceThreads), 0, perm, comp, plan, n, n_comp, n_components, eigvecs_out, w.sign,
              w.emax, meta, range, unit, R_out, w.part);
    SP_LAUNCH(umap_multi_tail_kernel, dim3(1), dim3(kOneThreads), 0, R_out, w.part, blocks, n, n_components, noise, Y0_out);
    return 0;
}

}  // extern "C"
