// umap_spectral_device.h — the device code of UMAP's spectral initialisation: the dim + 1 top eigenvectors of
// M = D^-1/2 P D^-1/2 from the edge list dm_umap_graph wrote, by Chebyshev-filtered subspace iteration in fp64.  The rules are stated
// in numpy in umapfit.py (`spectral_init_iter_host` and the comment above it); this file follows them step by step.  Included by
// umap_spectral.hip (below DM_UMAP_MAX_N rows) and by umap_sparse.hip (below DM_UMAP_SPARSE_MAX_N): one solver, two row bounds.
//
// Structure, as in umap.hip:
//   - every sum has a fixed order and there is no floating-point atomic: the same input gives the same bits on every run;
//   - the host enqueues the full cap of outer iterations and never waits: the residual test sets `done` in the state record and
//     every later kernel returns at once; the filter's degree and cut live in the same record, so a skipped filter step is a copy;
//   - the tall-skinny products (X^T X, Q^T (M Q)) are split over fixed slabs of kSlab rows and the slabs are summed in index order by
//     the one-workgroup kernel that consumes them (Cholesky, Jacobi).  They use plain fp64 FMAs-as-multiply-add, not
//     v_mfma_f64_16x16x4_f64: at b <= 97 and n < 4096 the products are a few MFLOP and the iteration is bound by its launches;
//   - no kernel reads workspace that it, or an earlier kernel of the same call, has not written.
//
// Buffers: four [n][b] blocks.  An outer iteration starts with the block in B0; filter step k writes B[k % 3], so the filtered block is
// in B1; Cholesky-QR: B1 -> B2 -> B3 (= Q); B1 = M Q; B0 = Q W, B2 = (M Q) W; the residual reads B0, B2.
#pragma once
#include "umap_device.h"

namespace dm {

namespace {

constexpr int kMaxB = 97;                    // block columns at DM_UMAP_MAX_COMPONENTS: 65 + 32
constexpr int kMaxM = DM_UMAP_MAX_COMPONENTS + 1;
constexpr int kSlab = 64;                    // rows per slab of the tall-skinny products
constexpr int kChunk = 32;                   // rows staged in LDS at a time
constexpr int kOneThreads = 1024;            // the one-workgroup kernels
constexpr int kDegree = 16;
constexpr int kMaxOuter = 40;
constexpr int kSweeps = 30;
constexpr double kGrowth = 1e6;
constexpr double kTol = 1e-11;
constexpr double kMinCut = -0.99;
constexpr uint32_t kHashEp = 0x5EED;
constexpr int kRotRows = 4;                  // rows a wave of umap_rotate_kernel owns

struct SpState {                             // device-side control record, written first by umap_components_kernel
    int done, iters, deg, ncomp, converged, pad;
    double cut, maxres;
};

struct SpWork {
    SpState* st;
    double *isd, *theta, *Rinv, *W, *B[4], *slabs, *res;
    int* label;                              // the component labels of the route past DM_UMAP_MAX_N rows (the other keeps them in LDS)
    size_t bytes;
};

inline int sp_block(int n, int dim) {
    const int m = dim + 1;
    const int b = m + (m / 2 > 8 ? m / 2 : 8);
    return b < n ? b : n;
}

inline int sp_slabs(int n) { return (n + kSlab - 1) / kSlab; }

SpWork sp_layout(void* base, int n, int b, bool global_labels) {
    SpWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t N = (size_t)n, Bc = (size_t)b, S = (size_t)sp_slabs(n);
    w.st = (SpState*)take(sizeof(SpState));
    w.isd = (double*)take(N * 8);
    w.theta = (double*)take(Bc * 8);
    w.Rinv = (double*)take(Bc * Bc * 8);
    w.W = (double*)take(Bc * Bc * 8);
    for (int i = 0; i < 4; ++i) w.B[i] = (double*)take(N * Bc * 8);
    w.slabs = (double*)take(S * Bc * Bc * 8);
    w.res = (double*)take(S * Bc * 8);
    w.label = global_labels ? (int*)take(N * 4) : nullptr;
    w.bytes = off;
    return w;
}

// hash_host in umapfit.py: the layout's umap_hash
__device__ __forceinline__ uint32_t sp_hash(uint32_t seed, uint32_t ep, uint32_t e, uint32_t p) { return umap_hash(seed, ep, e, p); }

// the filter's degree for a cut: the largest d <= kDegree with T_d((1 - c) / e) <= kGrowth (_cheb_degree in umapfit.py)
__device__ __forceinline__ int cheb_degree(double cut) {
    const double c = (cut - 1.0) / 2.0, e = (cut + 1.0) / 2.0;
    const double x = (1.0 - c) / e;
    double t0 = 1.0, t1 = x;
    int deg = 1;
    while (deg < kDegree) {
        const double t2 = 2.0 * x * t1 - t0;
        if (!(t2 <= kGrowth)) break;
        t0 = t1;
        t1 = t2;
        ++deg;
    }
    return deg;
}

// the edge range of row i, clamped to what an edge list of n rows can hold (n < 65536: the product fits an int)
__device__ __forceinline__ void edge_range(const int32_t* __restrict__ row_ptr, int i, int n, int& lo, int& hi) {
    const int cap = 2 * n * DM_UMAP_MAX_NEIGHBORS;
    lo = max(0, min(row_ptr[i], cap));
    hi = max(lo, min(row_ptr[i + 1], cap));
}

// ---- components ---------------------------------------------------------------------------------------------------------------------
// One workgroup: every row takes the smallest label among itself and its neighbours until a sweep changes nothing (a row's label is
// written by its own thread only and only falls, so reading a neighbour's label early or late changes the number of sweeps, not the
// fixed point).  The labels live in LDS (n < DM_UMAP_MAX_N), or in `glabel` [n] of the workspace, which the kernel writes
// before it reads (one workgroup: the barrier between sweeps orders its own global writes and reads).  Writes the state record: done
// at once if the graph is not one component or the caller forces the random initialisation.
template <typename Label>
__device__ __forceinline__ void components_body(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int force_random,
                                                Label label, SpState* __restrict__ st) {
    __shared__ int flag[2];
    __shared__ int part[kOneThreads / kWave];
    const int t = threadIdx.x;
    for (int i = t; i < n; i += kOneThreads) label[i] = i;
    if (t == 0) flag[0] = 0;
    __syncthreads();
    for (int sweep = 0; sweep < n; ++sweep) {
        if (t == 0) flag[(sweep + 1) & 1] = 0;
        for (int i = t; i < n; i += kOneThreads) {
            int lo, hi;
            edge_range(row_ptr, i, n, lo, hi);
            int best = label[i];
            for (int e = lo; e < hi; ++e) {
                const int j = col[e];
                if (j >= 0 && j < n) best = min(best, label[j]);
            }
            if (best < label[i]) {
                label[i] = best;
                flag[sweep & 1] = 1;
            }
        }
        __syncthreads();
        const int changed = flag[sweep & 1];
        __syncthreads();
        if (!changed) break;
    }
    int roots = 0;
    for (int i = t; i < n; i += kOneThreads) roots += label[i] == i;
    roots = wave_sum(roots);
    if (t % kWave == 0) part[t / kWave] = roots;
    __syncthreads();
    if (t == 0) {
        int ncomp = 0;
        for (int w = 0; w < kOneThreads / kWave; ++w) ncomp += part[w];
        st->ncomp = ncomp;
        st->done = (ncomp != 1 || force_random) ? 1 : 0;
        st->iters = 0;
        st->converged = 0;
        st->pad = 0;
        st->cut = 0.0;
        st->deg = cheb_degree(0.0);
        st->maxres = __longlong_as_double(0x7FF8000000000000ll);
    }
}

__global__ __launch_bounds__(kOneThreads)
void umap_components_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int force_random,
                            SpState* __restrict__ st) {
    __shared__ int label[DM_UMAP_MAX_N];
    components_body(row_ptr, col, n, force_random, (int*)label, st);
}

__global__ __launch_bounds__(kOneThreads)
void umap_components_global_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int force_random,
                                   int* glabel, SpState* __restrict__ st) {
    components_body(row_ptr, col, n, force_random, (volatile int*)glabel, st);
}

// ---- degrees, isd and the start block -------------------------------------------------------------------------------------------------
// One wave per row.  deg_i = the row's weights added in edge order (64 at a time through the lanes, then one broadcast per term).
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_degree_kernel(const int32_t* __restrict__ row_ptr, const float* __restrict__ weight, int n, int b, uint32_t seed,
                        double* __restrict__ isd, double* __restrict__ X) {
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    int lo, hi;
    edge_range(row_ptr, i, n, lo, hi);
    double deg = 0.0;
    for (int e0 = lo; e0 < hi; e0 += kWave) {
        const int cnt = min(kWave, hi - e0);
        const double w = lane < cnt ? (double)weight[e0 + lane] : 0.0;
        for (int t = 0; t < cnt; ++t) deg = deg + __shfl(w, t, kWave);
    }
    const double root = sqrt(deg);
    if (lane == 0) isd[i] = 1.0 / root;
    for (int c = lane; c < b; c += kWave)
        X[(size_t)i * b + c] = c == 0 ? root : (double)sp_hash(seed, kHashEp, (uint32_t)i, (uint32_t)c) / 4294967296.0 - 0.5;
}

// ---- the block product, with the Chebyshev recurrence fused ---------------------------------------------------------------------------
// One wave per row, lanes over block columns (a loop over column tiles when b > 64): (M X)_i = isd_i sum_e (w_e isd_col_e) X_col_e in
// edge order.  step = 0: out = M cur.  step = 1 .. kDegree: filter step; the last `deg` of the kDegree launches are the polynomial's
// steps (the first of them has no `prev`), the ones before copy cur to out.
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_spmm_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const float* __restrict__ weight,
                      const double* __restrict__ isd, int n, int b, const double* __restrict__ prev, const double* __restrict__ cur,
                      double* __restrict__ out, int step, const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st->done) return;
    const int lane = threadIdx.x % kWave;
    const int i = blockIdx.x * kRowWaves + threadIdx.x / kWave;
    if (i >= n) return;
    const int r = step ? step - (kDegree - st->deg) : 0;            // the polynomial's step number
    if (step && r <= 0) {
        for (int j = lane; j < b; j += kWave) out[(size_t)i * b + j] = cur[(size_t)i * b + j];
        return;
    }
    const double cut = st->cut;
    const double c = (cut - 1.0) / 2.0, e = (cut + 1.0) / 2.0;
    int lo, hi;
    edge_range(row_ptr, i, n, lo, hi);
    const double isd_i = isd[i];
    for (int j0 = 0; j0 < b; j0 += kWave) {
        const int j = j0 + lane;
        const bool has = j < b;
        double acc = 0.0;
        for (int e0 = lo; e0 < hi; e0 += kWave) {
            const int cnt = min(kWave, hi - e0);
            int jn = lane < cnt ? col[e0 + lane] : 0;
            const bool ok = lane < cnt && jn >= 0 && jn < n;
            jn = ok ? jn : 0;
            const double coef = ok ? (double)weight[e0 + lane] * isd[jn] : 0.0;
            for (int t = 0; t < cnt; ++t) {
                const int k = __shfl(jn, t, kWave);
                const double cf = __shfl(coef, t, kWave);
                const double x = has ? cur[(size_t)k * b + j] : 0.0;
                acc = acc + cf * x;
            }
        }
        if (!has) continue;
        const double my = isd_i * acc;
        double y = my;
        if (step) {
            const double yc = cur[(size_t)i * b + j];
            const double t = my - c * yc;
            y = r == 1 ? t / e : (2.0 * t) / e - prev[(size_t)i * b + j];
        }
        out[(size_t)i * b + j] = y;
    }
}

// ---- tall-skinny products -----------------------------------------------------------------------------------------------------------------
// Block s: slabs[s] = A[rows of slab s]^T B[the same rows], [b][b], rows added in ascending order.  A thread owns one 4 x 4 tile of the
// result; the slab's rows come through LDS kChunk at a time.
__global__ __launch_bounds__(kOneThreads)
void umap_gram_kernel(const double* __restrict__ A, const double* __restrict__ B, int n, int b, double* __restrict__ slabs,
                      const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    __shared__ double sa[kChunk * kMaxB];
    __shared__ double sb[kChunk * kMaxB];
    if (st->done) return;
    const int t = threadIdx.x;
    const int nt = (b + 3) / 4;
    const bool active = t < nt * nt;
    const int p0 = (t / nt) * 4, q0 = (t % nt) * 4;
    const int row_lo = blockIdx.x * kSlab, row_hi = min(n, row_lo + kSlab);
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int r0 = row_lo; r0 < row_hi; r0 += kChunk) {
        const int rows = min(kChunk, row_hi - r0);
        __syncthreads();                                             // the previous chunk has been read
        for (int q = t; q < rows * b; q += kOneThreads) {
            sa[q] = A[(size_t)r0 * b + q];
            sb[q] = B[(size_t)r0 * b + q];
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < rows; ++r) {
                double a[4], bb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = p0 + u < b ? sa[r * b + p0 + u] : 0.0;
                    bb[u] = q0 + u < b ? sb[r * b + q0 + u] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = acc[u][v] + a[u] * bb[v];
            }
        }
    }
    if (!active) return;
    double* out = slabs + (size_t)blockIdx.x * b * b;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (p0 + u < b && q0 + v < b) out[(size_t)(p0 + u) * b + q0 + v] = acc[u][v];
}

// ---- Cholesky and the triangular inverse ----------------------------------------------------------------------------------------------------
// One workgroup.  G = the slabs summed in index order (dynamic LDS, [b][pitch]); right-looking Cholesky G = L L^T in place; then wave
// per column c: column c of L^-1 by forward substitution (the column lives in the lanes' registers, lane k % 64 holds entry k; each
// entry is one lane-strided dot product summed by the xor tree).  Rinv = (L^T)^-1 = (L^-1)^T, written whole, zeros below the diagonal.
// A pivot that is not positive turns the block into NaN; the residual test then never passes and the status says so.
__global__ __launch_bounds__(kOneThreads)
void umap_chol_kernel(const double* __restrict__ slabs, int n_slabs, int b, double* __restrict__ Rinv, const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) double sp_lds[];
    if (st->done) return;
    const int t = threadIdx.x;
    const int pitch = b | 1;
    double* G = sp_lds;
    for (int q = t; q < b * b; q += kOneThreads) {
        double s = 0.0;
        for (int k = 0; k < n_slabs; ++k) s = s + slabs[(size_t)k * b * b + q];
        G[(q / b) * pitch + q % b] = s;
    }
    for (int j = 0; j < b; ++j) {
        __syncthreads();
        const double ljj = sqrt(G[j * pitch + j]);
        __syncthreads();                                             // every thread has read the pivot
        for (int i = j + t; i < b; i += kOneThreads) G[i * pitch + j] = i == j ? ljj : G[i * pitch + j] / ljj;
        __syncthreads();
        const int r = b - j - 1;
        for (int q = t; q < r * r; q += kOneThreads) {
            const int i = j + 1 + q / r, k = j + 1 + q % r;
            if (k <= i) G[i * pitch + k] = G[i * pitch + k] - G[i * pitch + j] * G[k * pitch + j];
        }
    }
    __syncthreads();
    const int lane = t % kWave;
    for (int c = t / kWave; c < b; c += kOneThreads / kWave) {
        double v0 = 0.0, v1 = 0.0;                                   // entries lane and lane + 64 of column c of L^-1
        for (int i = c; i < b; ++i) {
            double dot = 0.0;
            if (lane >= c && lane < i) dot = G[i * pitch + lane] * v0;
            if (lane + kWave >= c && lane + kWave < i) dot = dot + G[i * pitch + lane + kWave] * v1;
            dot = wave_sum(dot);
            const double x = ((i == c ? 1.0 : 0.0) - dot) / G[i * pitch + i];
            if (lane == i % kWave) {
                if (i < kWave) v0 = x; else v1 = x;
            }
        }
        for (int i = lane; i < b; i += kWave) Rinv[(size_t)c * b + i] = i < c ? 0.0 : (i < kWave ? v0 : v1);
    }
}

// ---- Rayleigh-Ritz: cyclic Jacobi -------------------------------------------------------------------------------------------------------------
// One workgroup.  H = the slabs summed in index order and symmetrised, W = I (both in dynamic LDS).  A sweep is the round-robin
// tournament of `_jacobi_rounds` in umapfit.py: P - 1 rounds of disjoint pairs; a round computes every pair's rotation from the matrix
// as the round finds it, rotates the columns of H and W, then the rows of H.  Sweeps end when one rotates nothing (at most kSweeps).
// theta = the diagonal in descending order (ties: the lower column first), W's columns in that order.
__global__ __launch_bounds__(kOneThreads)
void umap_jacobi_kernel(const double* __restrict__ slabs, int n_slabs, int b, double* __restrict__ W_out, double* __restrict__ theta_out,
                        const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) double sp_lds[];
    __shared__ int pp[(kMaxB + 1) / 2], qq[(kMaxB + 1) / 2];
    __shared__ double cc[(kMaxB + 1) / 2], ss[(kMaxB + 1) / 2];
    __shared__ int rotated[kSweeps];
    if (st->done) return;
    const int t = threadIdx.x;
    const int pitch = b | 1;
    double* H = sp_lds;
    double* W = sp_lds + (size_t)b * pitch;
    for (int q = t; q < b * b; q += kOneThreads) {
        const int i = q / b, j = q % b;
        double s = 0.0, st2 = 0.0;
        for (int k = 0; k < n_slabs; ++k) {
            s = s + slabs[(size_t)k * b * b + (size_t)i * b + j];
            st2 = st2 + slabs[(size_t)k * b * b + (size_t)j * b + i];
        }
        H[i * pitch + j] = 0.5 * (s + st2);
        W[i * pitch + j] = i == j ? 1.0 : 0.0;
    }
    if (t < kSweeps) rotated[t] = 0;
    __syncthreads();
    const int P = b + (b & 1), half = P / 2;
    for (int sweep = 0; sweep < kSweeps && b > 1; ++sweep) {
        for (int s = 0; s < P - 1; ++s) {
            if (t < half) {
                const int x = t == 0 ? P - 1 : (s + t) % (P - 1);
                const int y = t == 0 ? s : (s - t + P - 1) % (P - 1);
                const int p = min(x, y), q = max(x, y);
                double c = 1.0, sn = 0.0;
                if (q < b) {
                    const double hpp = H[p * pitch + p], hqq = H[q * pitch + q], hpq = H[p * pitch + q];
                    if (fabs(hpq) > 1e-20 * (fabs(hpp) + fabs(hqq))) {
                        const double tau = (hqq - hpp) / (2.0 * hpq);
                        const double tn = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + tn * tn);
                        sn = tn * c;
                        rotated[sweep] = 1;
                    }
                }
                pp[t] = q < b ? p : -1;
                qq[t] = q;
                cc[t] = c;
                ss[t] = sn;
            }
            __syncthreads();
            for (int w = t; w < b * half; w += kOneThreads) {           // columns: H <- H J, W <- W J
                const int k = w % half, r = w / half;
                const int p = pp[k], q = qq[k];
                if (p < 0) continue;
                const double c = cc[k], sn = ss[k];
                const double hp = H[r * pitch + p], hq = H[r * pitch + q];
                H[r * pitch + p] = c * hp - sn * hq;
                H[r * pitch + q] = sn * hp + c * hq;
                const double wp = W[r * pitch + p], wq = W[r * pitch + q];
                W[r * pitch + p] = c * wp - sn * wq;
                W[r * pitch + q] = sn * wp + c * wq;
            }
            __syncthreads();
            for (int w = t; w < b * half; w += kOneThreads) {           // rows: H <- J^T H
                const int k = w / b, j = w % b;
                const int p = pp[k], q = qq[k];
                if (p < 0) continue;
                const double c = cc[k], sn = ss[k];
                const double hp = H[p * pitch + j], hq = H[q * pitch + j];
                H[p * pitch + j] = c * hp - sn * hq;
                H[q * pitch + j] = sn * hp + c * hq;
            }
            __syncthreads();
        }
        if (!rotated[sweep]) break;
    }
    for (int j = t; j < b; j += kOneThreads) {
        const double th = H[j * pitch + j];
        int rank = 0;
        for (int i = 0; i < b; ++i) {
            const double o = H[i * pitch + i];
            rank += (o > th || (o == th && i < j)) ? 1 : 0;
        }
        theta_out[rank] = th;
        for (int r = 0; r < b; ++r) W_out[(size_t)r * b + rank] = W[r * pitch + j];
    }
}

// ---- [n][b] x [b][b] ----------------------------------------------------------------------------------------------------------------------------
// A wave owns kRotRows rows, lanes over the result's columns: out_ij = sum_k in_ik Bm_kj, k ascending.
__global__ __launch_bounds__(kRowWaves * kWave)
void umap_rotate_kernel(const double* __restrict__ in, const double* __restrict__ Bm, int n, int b, double* __restrict__ out,
                        const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st->done) return;
    const int lane = threadIdx.x % kWave;
    const int i0 = (blockIdx.x * kRowWaves + threadIdx.x / kWave) * kRotRows;
    if (i0 >= n) return;
    const double* row[kRotRows];
#pragma unroll
    for (int r = 0; r < kRotRows; ++r) row[r] = in + (size_t)min(i0 + r, n - 1) * b;
    for (int j0 = 0; j0 < b; j0 += kWave) {
        const int j = j0 + lane;
        if (j >= b) continue;
        double acc[kRotRows];
#pragma unroll
        for (int r = 0; r < kRotRows; ++r) acc[r] = 0.0;
        for (int k = 0; k < b; ++k) {
            const double bv = Bm[(size_t)k * b + j];
#pragma unroll
            for (int r = 0; r < kRotRows; ++r) acc[r] = acc[r] + row[r][k] * bv;
        }
#pragma unroll
        for (int r = 0; r < kRotRows; ++r)
            if (i0 + r < n) out[(size_t)(i0 + r) * b + j] = acc[r];
    }
}

// ---- the residual test -----------------------------------------------------------------------------------------------------------------------------
// Block s, thread j < m: res[s][j] = sum over the slab's rows, ascending, of (MX_ij - theta_j X_ij)^2.
__global__ __launch_bounds__(128)
void umap_residual_kernel(const double* __restrict__ X, const double* __restrict__ MX, const double* __restrict__ theta, int n, int b, int m,
                          double* __restrict__ res, const SpState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st->done) return;
    const int j = threadIdx.x;
    if (j >= m) return;
    const int row_lo = blockIdx.x * kSlab, row_hi = min(n, row_lo + kSlab);
    const double th = theta[j];
    double s = 0.0;
    for (int i = row_lo; i < row_hi; ++i) {
        const double d = MX[(size_t)i * b + j] - th * X[(size_t)i * b + j];
        s = s + d * d;
    }
    res[(size_t)blockIdx.x * b + j] = s;
}

// One workgroup: the slabs in index order, the norms, the verdict.  Sets done / converged, counts the iteration, and otherwise sets the
// next filter's cut (the smallest Ritz value, not below kMinCut) and degree.
__global__ __launch_bounds__(128)
void umap_verdict_kernel(const double* __restrict__ res, const double* __restrict__ theta, int n_slabs, int b, int m, SpState* __restrict__ st) {
#pragma clang fp contract(off)
    __shared__ double norm[kMaxM];
    if (st->done) return;
    const int j = threadIdx.x;
    if (j < m) {
        double s = 0.0;
        for (int k = 0; k < n_slabs; ++k) s = s + res[(size_t)k * b + j];
        norm[j] = sqrt(s);
    }
    __syncthreads();
    if (j != 0) return;
    bool ok = true, nan = false;
    double mx = 0.0;
    for (int q = 0; q < m; ++q) {
        const double r = norm[q];
        ok = ok && r <= kTol;
        nan = nan || r != r;
        mx = r > mx ? r : mx;
    }
    st->iters = st->iters + 1;
    st->maxres = nan ? __longlong_as_double(0x7FF8000000000000ll) : mx;
    if (ok) {
        st->converged = 1;
        st->done = 1;
        return;
    }
    const double last = theta[b - 1];
    const double cut = last > kMinCut ? last : kMinCut;              // a NaN gives kMinCut
    st->cut = cut;
    st->deg = cheb_degree(cut);
}

// ---- the tail ---------------------------------------------------------------------------------------------------------------------------------------
// One workgroup; lane = coordinate, the 16 waves stripe the rows.  `_spectral_tail` in umapfit.py line by line: the sign of each column's
// largest-magnitude entry (the first one on a tie), 10 / max|.| in fp64, the fp32 cast, the noise added in fp32, then per coordinate
// 10 (y - lo) / (hi - lo) with every fp32 operation rounded on its own (the quotient through fp64, which rounds as fp32 division does).
// With more than one component, or forced, Y0 is the uploaded random fallback.  Writes eigvals, eigvecs (if asked) and the status record.
__global__ __launch_bounds__(kOneThreads)
void umap_tail_kernel(const double* __restrict__ X, const double* __restrict__ theta, int n, int b, int dim, int force_random,
                      const float* __restrict__ noise, const float* __restrict__ fallback, const SpState* __restrict__ st,
                      float* __restrict__ Y0, double* __restrict__ eigvals, double* __restrict__ eigvecs, double* __restrict__ status) {
#pragma clang fp contract(off)
    constexpr int kWaves = kOneThreads / kWave;
    __shared__ double best_abs[kWaves][kWave], best_val[kWaves][kWave];
    __shared__ int best_row[kWaves][kWave];
    __shared__ float lo_s[kWaves][kWave], hi_s[kWaves][kWave];
    __shared__ double sign_s[kWave], scale_s;
    __shared__ float lo_c[kWave], hi_c[kWave];
    const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
    const int m = dim + 1;
    const bool spectral = st->ncomp == 1 && !force_random;
    if (t == 0) {
        status[0] = spectral ? 0.0 : 1.0;
        status[1] = (double)st->ncomp;
        status[2] = (double)st->iters;
        status[3] = (double)st->converged;
        status[4] = st->maxres;
        status[5] = st->cut;
        status[6] = (double)st->deg;
        status[7] = (double)b;
    }
    if (!spectral) {
        for (int q = t; q < n * dim; q += kOneThreads) Y0[q] = fallback[q];
        for (int q = t; q < m; q += kOneThreads) eigvals[q] = 0.0;
        if (eigvecs)
            for (int q = t; q < n * m; q += kOneThreads) eigvecs[q] = 0.0;
        return;
    }
    for (int q = t; q < m; q += kOneThreads) eigvals[q] = theta[q];
    if (eigvecs)
        for (int q = t; q < n * m; q += kOneThreads) eigvecs[q] = X[(size_t)(q / m) * b + q % m];
    const bool has = lane < dim;
    {   // the largest-magnitude entry of every column
        double ba = -1.0, bv = 0.0;
        int br = 0;
        if (has)
            for (int i = wave; i < n; i += kWaves) {
                const double v = X[(size_t)i * b + 1 + lane];
                if (fabs(v) > ba) {
                    ba = fabs(v);
                    bv = v;
                    br = i;
                }
            }
        best_abs[wave][lane] = ba;
        best_val[wave][lane] = bv;
        best_row[wave][lane] = br;
    }
    __syncthreads();
    if (wave == 0 && has) {
        double ba = best_abs[0][lane], bv = best_val[0][lane];
        int br = best_row[0][lane];
        for (int w = 1; w < kWaves; ++w) {
            const double a = best_abs[w][lane];
            if (a > ba || (a == ba && best_row[w][lane] < br)) {
                ba = a;
                bv = best_val[w][lane];
                br = best_row[w][lane];
            }
        }
        sign_s[lane] = bv > 0.0 ? 1.0 : bv < 0.0 ? -1.0 : bv;        // numpy.sign: 0 stays 0, NaN stays NaN
        best_abs[0][lane] = ba;
    }
    __syncthreads();
    if (t == 0) {
        double g = best_abs[0][0];
        for (int c = 1; c < dim; ++c) g = best_abs[0][c] > g ? best_abs[0][c] : g;
        scale_s = 10.0 / g;
    }
    __syncthreads();
    {   // the fp32 coordinates with their noise, and every coordinate's range
        float lo = INFINITY, hi = -INFINITY;
        if (has) {
            const double sg = sign_s[lane], sc = scale_s;
            for (int i = wave; i < n; i += kWaves) {
                const double v = X[(size_t)i * b + 1 + lane] * sg;
                const float y = (float)(v * sc) + noise[(size_t)i * dim + lane];
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


int sp_check(int n, int n_components, int max_n) {
    if (n >= max_n) return DM_UMAP_E_N_LARGE;
    if (n < 1) return DM_UMAP_E_NEIGHBORS_GE_N;
    if (n_components < 1 || n_components > DM_UMAP_MAX_COMPONENTS) return DM_UMAP_E_COMPONENTS;
    return 0;
}

#define SP_LAUNCH(kernel, grid, block, lds, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__); \
    if (hipGetLastError() != hipSuccess) return DM_UMAP_E_HIP; } while (0)

int sp_workspace_bytes(int n, int n_components, size_t* bytes_out, int max_n) {
    if (!bytes_out) return DM_UMAP_E_NULL;
    if (int rc = sp_check(n, n_components, max_n)) return rc;
    *bytes_out = sp_layout(nullptr, n, sp_block(n, n_components), max_n > DM_UMAP_MAX_N).bytes;
    return 0;
}

// dm_umap_spectral and dm_umap_sparse_spectral: the same checks and launches; the row bound decides where the component labels live.
int sp_run(void* stream, const int32_t* row_ptr, const int32_t* col, const float* weight, int n, int n_components, int seed,
           const float* noise, const float* fallback, void* work, size_t work_bytes, float* Y0_out, double* eigvals_out,
           double* eigvecs_out, double* status_out, int max_n) {
    if (!row_ptr || !col || !weight || !noise || !fallback || !work || !Y0_out || !eigvals_out || !status_out) return DM_UMAP_E_NULL;
    if (int rc = sp_check(n, n_components, max_n)) return rc;
    const int m = n_components + 1, b = sp_block(n, n_components);
    const bool global_labels = max_n > DM_UMAP_MAX_N;
    const SpWork w = sp_layout(work, n, b, global_labels);
    if (work_bytes < w.bytes) return DM_UMAP_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    const int force_random = m >= n ? 1 : 0;
    const int slabs = sp_slabs(n);
    const size_t lds_chol = (size_t)b * (b | 1) * sizeof(double), lds_jacobi = 2 * lds_chol;
    static std::atomic<uint64_t> attr_seen{0};
    if (first_use_on_device(attr_seen)) {
        const int most = kMaxB * (kMaxB | 1) * (int)sizeof(double);
        (void)hipFuncSetAttribute((const void*)umap_chol_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        (void)hipFuncSetAttribute((const void*)umap_jacobi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * most);
    }
    const dim3 rows(row_blocks(n)), row_threads(kRowWaves * kWave), one(1), one_threads(kOneThreads);
    const dim3 rot((n + kRowWaves * kRotRows - 1) / (kRowWaves * kRotRows));
    if (global_labels)
        SP_LAUNCH(umap_components_global_kernel, one, one_threads, 0, row_ptr, col, n, force_random, w.label, w.st);
    else
        SP_LAUNCH(umap_components_kernel, one, one_threads, 0, row_ptr, col, n, force_random, w.st);
    if (!force_random) {
        SP_LAUNCH(umap_degree_kernel, rows, row_threads, 0, row_ptr, weight, n, b, (uint32_t)seed & 0x7FFFFFFFu, w.isd, w.B[0]);
        for (int it = 0; it < kMaxOuter; ++it) {
            for (int k = 1; k <= kDegree; ++k)
                SP_LAUNCH(umap_spmm_kernel, rows, row_threads, 0, row_ptr, col, weight, w.isd, n, b, w.B[(k + 1) % 3], w.B[(k + 2) % 3],
                          w.B[k % 3], k, w.st);
            for (int pass = 0; pass < 2; ++pass) {                      // Cholesky-QR twice: B1 -> B2 -> B3
                SP_LAUNCH(umap_gram_kernel, dim3(slabs), one_threads, 0, w.B[1 + pass], w.B[1 + pass], n, b, w.slabs, w.st);
                SP_LAUNCH(umap_chol_kernel, one, one_threads, lds_chol, w.slabs, slabs, b, w.Rinv, w.st);
                SP_LAUNCH(umap_rotate_kernel, rot, row_threads, 0, w.B[1 + pass], w.Rinv, n, b, w.B[2 + pass], w.st);
            }
            SP_LAUNCH(umap_spmm_kernel, rows, row_threads, 0, row_ptr, col, weight, w.isd, n, b, (const double*)nullptr, w.B[3], w.B[1], 0, w.st);
            SP_LAUNCH(umap_gram_kernel, dim3(slabs), one_threads, 0, w.B[3], w.B[1], n, b, w.slabs, w.st);
            SP_LAUNCH(umap_jacobi_kernel, one, one_threads, lds_jacobi, w.slabs, slabs, b, w.W, w.theta, w.st);
            SP_LAUNCH(umap_rotate_kernel, rot, row_threads, 0, w.B[3], w.W, n, b, w.B[0], w.st);
            SP_LAUNCH(umap_rotate_kernel, rot, row_threads, 0, w.B[1], w.W, n, b, w.B[2], w.st);
            SP_LAUNCH(umap_residual_kernel, dim3(slabs), dim3(128), 0, w.B[0], w.B[2], w.theta, n, b, m, w.res, w.st);
            SP_LAUNCH(umap_verdict_kernel, one, dim3(128), 0, w.res, w.theta, slabs, b, m, w.st);
        }
    }
    SP_LAUNCH(umap_tail_kernel, one, one_threads, 0, w.B[0], w.theta, n, b, n_components, force_random, noise, fallback, w.st, Y0_out,
              eigvals_out, eigvecs_out, status_out);
    return 0;
}

}  // namespace

}  // namespace dm
