// kmeans.hip — the clustering stage's last step on the device: scikit-learn's KMeans(n_clusters=k, random_state=10)
// .fit(X) as it runs for this call (one k-means++ seeding in fp64, Lloyd in fp32 on mean-centred rows, max_iter 300, tol 1e-4),
// and the tail of the reference's cluster() (typicality/cluster.py:319-328, parallel-dataset/cluster.py:274-289,
// clipmining/ranking.py:135-149): members ordered by distance to their cluster's reference point, clusters ranked by the median /
// mean D of their members.
//
// The work is launch-bound (about 33 MFLOP per Lloyd iteration at 1000 x 512, k = 32), so the kernels are plain fp32 / fp64 FMAs and
// the structure is what matters:
//   - every sum has a fixed order (lane-strided partials + an xor-shuffle tree per wave; chunked partials + an LDS tree per block, the
//     block size a compile-time constant), and there is no floating-point atomic: the same input gives the same bits on every run;
//   - every decision is made on the device.  KmState in the workspace holds the stop flag and the iteration counter; once the flag is
//     set the iteration kernels return at once.  The host enqueues kIterGroup iterations, reads the flag once, and goes on;
//   - iterations are separate launches; nothing waits on another workgroup inside a kernel;
//   - no kernel reads workspace it (or an earlier kernel of the same call) has not written.
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

#include <math.h>

namespace dm {

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // the single-block kernels: 16 waves
constexpr int kRowWaves = 4;                 // the wave-per-row kernels: 4 rows per 256-thread block
constexpr int kMaxTrials = 8;                // 2 + int(ln 256) = 7
constexpr int kIterGroup = 8;                // Lloyd iterations enqueued between two reads of the stop flag

enum { KM_RUN = 0, KM_STRICT = 1, KM_TOL = 2, KM_MAXITER = 3 };

struct KmState {
    int done;                                // KM_*
    int n_iter;
    int ncand;
    int cand[kMaxTrials];
    float tol_abs;
    double pot;                              // current k-means++ potential
};

struct KmWork {                              // the workspace, carved by km_layout
    KmState* state;
    float *mean, *colvar, *Xc, *closest, *dcand, *C, *Cnew, *cnorm, *rowdist, *agg, *mid;
    double *xx, *prefix, *key;
    int32_t *prev, *counts, *starts, *sorted, *within, *far;
    size_t bytes;
};

KmWork km_layout(void* base, int n, int d, int k) {
    KmWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t N = (size_t)n, D = (size_t)d, K = (size_t)k;
    w.state = (KmState*)take(sizeof(KmState));
    w.xx = (double*)take(N * 8);
    w.prefix = (double*)take(N * 8);
    w.key = (double*)take(N * 8);
    w.mean = (float*)take(D * 4);
    w.colvar = (float*)take(D * 4);
    w.Xc = (float*)take(N * D * 4);
    w.closest = (float*)take(N * 4);
    w.dcand = (float*)take(N * kMaxTrials * 4);
    w.C = (float*)take(K * D * 4);
    w.Cnew = (float*)take(K * D * 4);
    w.cnorm = (float*)take(K * 4);
    w.rowdist = (float*)take(N * 4);
    w.agg = (float*)take(K * 4);
    w.mid = (float*)take(K * 2 * 4);
    w.prev = (int32_t*)take(N * 4);
    w.counts = (int32_t*)take(K * 4);
    w.starts = (int32_t*)take((K + 1) * 4);
    w.sorted = (int32_t*)take(N * 4);
    w.within = (int32_t*)take(N * 4);
    w.far = (int32_t*)take(K * 4);
    w.bytes = off;
    return w;
}

// ---- fixed-order reductions ---------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {            // xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// sum of one value per thread over a kBlock-thread block, in a fixed tree; every thread gets the result.  s: kBlock doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (t < o) s[t] += s[t + o];
        __syncthreads();
    }
    return s[0];
}

// thread t of a kBlock block owns rows [t * chunk, min(n, (t + 1) * chunk))
__device__ __forceinline__ void chunk_of(int n, int& lo, int& hi) {
    const int chunk = (n + kBlock - 1) / kBlock;
    lo = min(n, (int)threadIdx.x * chunk);
    hi = min(n, lo + chunk);
}

// ---- centring -------------------------------------------------------------------------------------------------------------------
// One thread per column: mean_e = (x_0e + x_1e + ...) / n in row order (numpy's add.reduce over axis 0), the variance the same way
// from (x - mean)^2 (np.var), Xc = X - mean on the way.
__global__ __launch_bounds__(256)
void km_center_kernel(const float* __restrict__ X, int n, int d, float* __restrict__ mean, float* __restrict__ colvar,
                      float* __restrict__ Xc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d) return;
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += X[(size_t)i * d + e];
    const float m = s / (float)n;
    float v = 0.f;
    for (int i = 0; i < n; ++i) {
        const float c = X[(size_t)i * d + e] - m;
        Xc[(size_t)i * d + e] = c;
        v += c * c;
    }
    mean[e] = m;
    colvar[e] = v / (float)n;
}

// One wave per row: xx_i = |xc_i|^2 in fp64 (the k-means++ distances are taken on the upcast rows).
__global__ __launch_bounds__(kRowWaves * kWave)
void km_rownorm_kernel(const float* __restrict__ Xc, int n, int d, double* __restrict__ xx) {
    const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* x = Xc + (size_t)i * d;
    double a = 0.0;
    for (int e = lane; e < d; e += kWave) a += (double)x[e] * (double)x[e];
    a = wave_sum(a);
    if (lane == 0) xx[i] = a;
}

// Single block: the state, tol_abs = tol_rel * mean_e var_e, prev labels = -1 (scikit-learn's labels_old).
__global__ __launch_bounds__(kBlock)
void km_begin_kernel(KmState* st, const float* __restrict__ colvar, int n, int d, float tol_rel, int32_t* __restrict__ prev) {
    __shared__ double s[kBlock];
    double a = 0.0;
    for (int e = threadIdx.x; e < d; e += kBlock) a += (double)colvar[e];
    a = block_sum(a, s);
    for (int i = threadIdx.x; i < n; i += kBlock) prev[i] = -1;
    if (threadIdx.x == 0) {
        st->done = KM_RUN;
        st->n_iter = 0;
        st->ncand = 0;
        st->pot = 0.0;
        st->tol_abs = (float)(a / (double)d * (double)tol_rel);
    }
}

// ---- k-means++ ------------------------------------------------------------------------------------------------------------------
// One wave per row: the row's squared distance to every current candidate, fp64, rounded to fp32 and clamped at 0 (scikit-learn's
// _euclidean_distances on float32 input: upcast chunks, the result stored as float32).
__global__ __launch_bounds__(kRowWaves * kWave)
void km_seed_dist_kernel(const KmState* __restrict__ st, const float* __restrict__ Xc, const double* __restrict__ xx, int n, int d,
                         float* __restrict__ dcand) {
    const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* x = Xc + (size_t)i * d;
    const int nc = st->ncand;
    for (int c = 0; c < nc; ++c) {
        const int ci = st->cand[c];
        const float* y = Xc + (size_t)ci * d;
        double a = 0.0;
        for (int e = lane; e < d; e += kWave) a += (double)x[e] * (double)y[e];
        a = wave_sum(a);
        if (lane == 0) dcand[(size_t)c * n + i] = fmaxf((float)(xx[i] + xx[ci] - 2.0 * a), 0.f);
    }
}

// Single block, step = 0 .. k.  Step >= 1 settles centre step - 1 among the candidates of the previous step (lowest potential, first
// among equals; `closest` is +inf before the first centre); step < k draws the candidates of centre `step`: the first by
// floor(u0 n), the later ones by searchsorted (side left) of u * potential in the inclusive prefix sum of `closest`, clipped to n - 1.
__global__ __launch_bounds__(kBlock)
void km_seed_pick_kernel(KmState* st, int step, int k, int n, int trials, const double* __restrict__ uniforms,
                         const float* __restrict__ dcand, float* __restrict__ closest, double* __restrict__ prefix,
                         int32_t* __restrict__ seed_index) {
    __shared__ double s[kBlock];
    __shared__ double pots[kMaxTrials];
    int lo, hi;
    chunk_of(n, lo, hi);
    if (step >= 1) {
        const int nc = st->ncand;
        for (int c = 0; c < nc; ++c) {
            double a = 0.0;
            for (int i = lo; i < hi; ++i) {
                const float v = dcand[(size_t)c * n + i];
                a += (double)(step == 1 ? v : fminf(closest[i], v));
            }
            a = block_sum(a, s);
            if (threadIdx.x == 0) pots[c] = a;
        }
        __syncthreads();
        int best = 0;
        for (int c = 1; c < nc; ++c) if (pots[c] < pots[best]) best = c;
        for (int i = lo; i < hi; ++i) {
            const float v = dcand[(size_t)best * n + i];
            closest[i] = step == 1 ? v : fminf(closest[i], v);
        }
        if (threadIdx.x == 0) {
            seed_index[step - 1] = st->cand[best];
            st->pot = pots[best];
        }
        __syncthreads();
    }
    if (step >= k) return;
    if (step == 0) {
        if (threadIdx.x == 0) {
            st->cand[0] = max(0, min(n - 1, (int)floor(uniforms[0] * (double)n)));
            st->ncand = 1;
        }
        return;
    }
    // inclusive prefix sum of closest, row order: chunk totals, a Hillis-Steele scan of the kBlock totals, then the chunk again
    double a = 0.0;
    for (int i = lo; i < hi; ++i) a += (double)closest[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        double v = s[threadIdx.x];
        if ((int)threadIdx.x >= o) v += s[threadIdx.x - o];
        __syncthreads();
        s[threadIdx.x] = v;
        __syncthreads();
    }
    double run = threadIdx.x == 0 ? 0.0 : s[threadIdx.x - 1];
    for (int i = lo; i < hi; ++i) {
        run += (double)closest[i];
        prefix[i] = run;
    }
    __threadfence_block();
    __syncthreads();
    if ((int)threadIdx.x < trials) {
        const double r = uniforms[1 + (size_t)(step - 1) * trials + threadIdx.x] * st->pot;
        int a0 = 0, b0 = n;                              // first index with prefix[i] >= r
        while (a0 < b0) {
            const int m = a0 + (b0 - a0) / 2;
            if (prefix[m] < r) a0 = m + 1; else b0 = m;
        }
        st->cand[threadIdx.x] = min(a0, n - 1);
    }
    if (threadIdx.x == 0) st->ncand = trials;
}

// ---- Lloyd ----------------------------------------------------------------------------------------------------------------------
// One block per centre: C_j = Xc[seed_index_j].
__global__ void km_gather_kernel(const float* __restrict__ Xc, const int32_t* __restrict__ seed_index, int n, int d, float* __restrict__ Cn) {
    const int j = blockIdx.x;
    const int r = min(max(seed_index[j], 0), n - 1);
    for (int e = threadIdx.x; e < d; e += blockDim.x) Cn[(size_t)j * d + e] = Xc[(size_t)r * d + e];
}

// `final` kernels run after the loop, when the stop was not strict (the labels then belong to the centres before the last update).
__device__ __forceinline__ bool km_skip(const KmState* st, int final) {
    const int done = st->done;
    return final ? done == KM_STRICT : done != KM_RUN;
}

// One wave per centre: |c_j|^2, fp32.
__global__ __launch_bounds__(kRowWaves * kWave)
void km_cnorm_kernel(const KmState* __restrict__ st, int final, const float* __restrict__ Cn, int k, int d, float* __restrict__ cnorm) {
    if (km_skip(st, final)) return;
    const int j = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= k) return;
    float a = 0.f;
    for (int e = lane; e < d; e += kWave) a += Cn[(size_t)j * d + e] * Cn[(size_t)j * d + e];
    a = wave_sum(a);
    if (lane == 0) cnorm[j] = a;
}

// One wave per row: label_i = argmin_j |c_j|^2 - 2 xc_i . c_j, the lowest j among equals.
__global__ __launch_bounds__(kRowWaves * kWave)
void km_assign_kernel(const KmState* __restrict__ st, int final, const float* __restrict__ Xc, const float* __restrict__ Cn,
                      const float* __restrict__ cnorm, int n, int d, int k, int32_t* __restrict__ labels) {
    if (km_skip(st, final)) return;
    const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* x = Xc + (size_t)i * d;
    float best = 0.f;
    int arg = 0;
    for (int j = 0; j < k; ++j) {
        const float* c = Cn + (size_t)j * d;
        float a = 0.f;
        for (int e = lane; e < d; e += kWave) a += x[e] * c[e];
        a = wave_sum(a);
        const float sc = cnorm[j] - 2.f * a;
        if (j == 0 || sc < best) { best = sc; arg = j; }
    }
    if (lane == 0) labels[i] = arg;
}

// One wave per cluster: a stable counting sort of the rows by label.  Pass 1 counts the rows of lower labels and of this one, pass
// 2 writes this cluster's rows, ascending, at sorted[starts_j ..].  st may be null (the ranking's use).
__global__ __launch_bounds__(kWave)
void km_bucket_kernel(const KmState* __restrict__ st, const int32_t* __restrict__ labels, int n, int k, int32_t* __restrict__ counts,
                      int32_t* __restrict__ starts, int32_t* __restrict__ sorted) {
    if (st && st->done != KM_RUN) return;
    const int j = blockIdx.x, lane = threadIdx.x;
    int lt = 0, eq = 0;
    for (int i = lane; i < n; i += kWave) {
        const int l = labels[i];
        lt += l < j;
        eq += l == j;
    }
    lt = wave_sum(lt);
    eq = wave_sum(eq);
    if (lane == 0) {
        counts[j] = eq;
        starts[j] = lt;
        if (j == k - 1) starts[k] = lt + eq;
    }
    int at = lt;
    for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        const bool mine = i < n && labels[i] == j;
        const unsigned long long m = __ballot(mine);
        if (mine) sorted[at + __popcll(m & ((1ull << lane) - 1ull))] = i;
        at += __popcll(m);
    }
}

// One thread per (cluster, column): the member sum in ascending row order, fp32.
__global__ __launch_bounds__(256)
void km_sum_kernel(const KmState* __restrict__ st, const float* __restrict__ Xc, const int32_t* __restrict__ counts,
                   const int32_t* __restrict__ starts, const int32_t* __restrict__ sorted, int d, float* __restrict__ Cnew) {
    if (st->done != KM_RUN) return;
    const int j = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d) return;
    const int32_t* rows = sorted + starts[j];
    const int cnt = counts[j];
    float a = 0.f;
    for (int m = 0; m < cnt; ++m) a += Xc[(size_t)rows[m] * d + e];
    Cnew[(size_t)j * d + e] = a;
}

// Single block: the rest of one Lloyd iteration.  Relocates empty clusters (_relocate_empty_clusters_dense), averages, measures the
// shift, compares the labels with the previous iteration's, decides, and makes the new centres current.
__global__ __launch_bounds__(kBlock)
void km_finish_kernel(KmState* st, const float* __restrict__ Xc, int n, int d, int k, int max_iter, const int32_t* __restrict__ labels,
                      int32_t* __restrict__ prev, int32_t* __restrict__ counts, float* __restrict__ Cn, float* __restrict__ Cnew,
                      float* __restrict__ rowdist) {
    if (st->done != KM_RUN) return;
    __shared__ double s[kBlock];
    __shared__ float sv[kBlock];
    __shared__ int si[kBlock];
    __shared__ float shift_j[DM_KMEANS_MAX_K];
    __shared__ int empty[DM_KMEANS_MAX_K];
    __shared__ int n_empty;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t == 0) {
        int ne = 0;
        for (int j = 0; j < k; ++j) if (counts[j] == 0) empty[ne++] = j;
        n_empty = ne;
    }
    __syncthreads();
    if (n_empty > 0) {
        for (int i = wave; i < n; i += kBlock / kWave) {            // squared distance of every row to its own (old) centre
            const float* x = Xc + (size_t)i * d;
            const float* c = Cn + (size_t)labels[i] * d;
            float a = 0.f;
            for (int e = lane; e < d; e += kWave) { const float v = x[e] - c[e]; a += v * v; }
            a = wave_sum(a);
            if (lane == 0) rowdist[i] = a;
        }
        __threadfence_block();
        __syncthreads();
        for (int q = 0; q < n_empty; ++q) {
            float bv = -1.f;                                          // the farthest row not yet taken, the lowest row among equals
            int bi = n;
            for (int i = t; i < n; i += kBlock) {
                const float v = rowdist[i];
                if (v > bv) { bv = v; bi = i; }
            }
            sv[t] = bv; si[t] = bi;
            __syncthreads();
            for (int o = kBlock / 2; o > 0; o >>= 1) {
                if (t < o && (sv[t + o] > sv[t] || (sv[t + o] == sv[t] && si[t + o] < si[t]))) { sv[t] = sv[t + o]; si[t] = si[t + o]; }
                __syncthreads();
            }
            const int far = si[0];
            __syncthreads();
            if (far >= n) break;                                      // (n >= k: cannot happen with finite data)
            const int from = labels[far], to = empty[q];
            for (int e = t; e < d; e += kBlock) {
                const float v = Xc[(size_t)far * d + e];
                Cnew[(size_t)from * d + e] -= v;
                Cnew[(size_t)to * d + e] = v;
            }
            if (t == 0) {
                rowdist[far] = -1.f;
                counts[to] = 1;
                counts[from] -= 1;
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    // average (times 1 / count, scikit-learn's _average_centers) and the shift |c_new - c_old|^2 per centre, one wave per centre
    for (int j = wave; j < k; j += kBlock / kWave) {
        const int cnt = counts[j];
        const float alpha = cnt > 0 ? 1.0f / (float)cnt : 1.0f;
        float a = 0.f;
        for (int e = lane; e < d; e += kWave) {
            const float c = Cnew[(size_t)j * d + e] * alpha;
            const float v = c - Cn[(size_t)j * d + e];
            Cnew[(size_t)j * d + e] = c;
            a += v * v;
        }
        a = wave_sum(a);
        const float r = sqrtf(a);
        if (lane == 0) shift_j[j] = r * r;
    }
    // labels against the previous iteration's
    double changed = 0.0;
    for (int i = t; i < n; i += kBlock) {
        const int l = labels[i];
        changed += l != prev[i];
        prev[i] = l;
    }
    changed = block_sum(changed, s);
    for (int x = t; x < k * d; x += kBlock) Cn[x] = Cnew[x];
    if (t == 0) {
        float shift = 0.f;
        for (int j = 0; j < k; ++j) shift += shift_j[j];
        const int it = st->n_iter + 1;
        st->n_iter = it;
        st->done = changed == 0.0 ? KM_STRICT : shift <= st->tol_abs ? KM_TOL : it >= max_iter ? KM_MAXITER : KM_RUN;
    }
}

// One wave per row: |xc_i - c_label_i|^2, fp32.
__global__ __launch_bounds__(kRowWaves * kWave)
void km_rowdist_kernel(const float* __restrict__ Xc, const float* __restrict__ Cn, const int32_t* __restrict__ labels, int n, int d,
                       float* __restrict__ rowdist) {
    const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* x = Xc + (size_t)i * d;
    const float* c = Cn + (size_t)labels[i] * d;
    float a = 0.f;
    for (int e = lane; e < d; e += kWave) { const float v = x[e] - c[e]; a += v * v; }
    a = wave_sum(a);
    if (lane == 0) rowdist[i] = a;
}

// Single block: inertia, n_iter, centres + mean.
__global__ __launch_bounds__(kBlock)
void km_end_kernel(const KmState* __restrict__ st, const float* __restrict__ rowdist, const float* __restrict__ Cn,
                   const float* __restrict__ mean, int n, int d, int k, float* __restrict__ centers, float* __restrict__ inertia,
                   int32_t* __restrict__ n_iter) {
    __shared__ double s[kBlock];
    int lo, hi;
    chunk_of(n, lo, hi);
    double a = 0.0;
    for (int i = lo; i < hi; ++i) a += (double)rowdist[i];
    a = block_sum(a, s);
    for (int x = threadIdx.x; x < k * d; x += kBlock) centers[x] = Cn[x] + mean[x % d];
    if (threadIdx.x == 0) {
        *inertia = (float)a;
        *n_iter = st->n_iter;
    }
}

// ---- ranking --------------------------------------------------------------------------------------------------------------------
// One block per centre: far_j = argmax_i |x_i - centre_j| over ALL rows, the first among equals (np.argmax), squared distances in fp64.
__global__ __launch_bounds__(kRowWaves * kWave)
void rk_far_kernel(const float* __restrict__ X, const float* __restrict__ centers, int n, int d, int32_t* __restrict__ far) {
    __shared__ double sv[kRowWaves];
    __shared__ int si[kRowWaves];
    const int j = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* c = centers + (size_t)j * d;
    double bv = -1.0;
    int bi = n;
    for (int i = wave; i < n; i += kRowWaves) {
        const float* x = X + (size_t)i * d;
        double a = 0.0;
        for (int e = lane; e < d; e += kWave) { const double v = (double)x[e] - (double)c[e]; a += v * v; }
        a = wave_sum(a);
        if (a > bv) { bv = a; bi = i; }
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRowWaves; ++w) if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
        far[j] = min(bi, n - 1);
    }
}

// One wave per row: key_i = |xr_i - ref_label_i| (np.linalg.norm), accumulated in fp64.  ref = the centre, or row far_label of Xr.
__global__ __launch_bounds__(kRowWaves * kWave)
void rk_key_kernel(const float* __restrict__ Xr, const float* __restrict__ centers, const int32_t* __restrict__ far,
                   const int32_t* __restrict__ labels, int n, int k, int dr, double* __restrict__ key) {
    const int i = blockIdx.x * kRowWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int j = labels[i];
    if (j < 0 || j >= k) return;                                   // a label outside [0, k) belongs to no cluster
    const float* x = Xr + (size_t)i * dr;
    const float* r = far ? Xr + (size_t)far[j] * dr : centers + (size_t)j * dr;
    double a = 0.0;
    for (int e = lane; e < dr; e += kWave) { const double v = (double)x[e] - (double)r[e]; a += v * v; }
    a = wave_sum(a);
    if (lane == 0) key[i] = sqrt(a);
}

// (value, row) order with NaN after every number
__device__ __forceinline__ bool rk_before(double a, int ia, double b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na == nb ? ia < ib : nb;
    return a < b || (a == b && ia < ib);
}

// One thread per row: its place among its cluster's members by (key, row) -> within[starts_j + place] = row; and its place by (D,
// row): the two middle values of the cluster's sorted D go to mid[2 j], mid[2 j + 1].  O(members) per row.
__global__ __launch_bounds__(256)
void rk_place_kernel(const double* __restrict__ key, const float* __restrict__ D, const int32_t* __restrict__ labels,
                     const int32_t* __restrict__ counts, const int32_t* __restrict__ starts, const int32_t* __restrict__ sorted, int n,
                     int k, int32_t* __restrict__ within, float* __restrict__ mid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = labels[i];
    if (j < 0 || j >= k) return;
    const int cnt = counts[j];
    const int32_t* rows = sorted + starts[j];
    const double ki = key[i], di = (double)D[i];
    int pk = 0, pd = 0;
    for (int m = 0; m < cnt; ++m) {
        const int r = rows[m];
        pk += rk_before(key[r], r, ki, i);
        pd += rk_before((double)D[r], r, di, i);
    }
    within[starts[j] + pk] = i;
    if (pd == cnt / 2) mid[2 * j + 1] = D[i];
    if (pd == cnt / 2 - 1) mid[2 * j] = D[i];
}

// Single block of DM_KMEANS_MAX_K threads, one per cluster: the aggregate, the rank (descending aggregate, NaN last, stably in order
// of the label's first appearance by row), then the outputs.
__global__ __launch_bounds__(DM_KMEANS_MAX_K)
void rk_rank_kernel(const float* __restrict__ D, const int32_t* __restrict__ counts, const int32_t* __restrict__ starts,
                    const int32_t* __restrict__ sorted, const int32_t* __restrict__ within, const float* __restrict__ mid, int n, int k,
                    int aggregate, int32_t* __restrict__ order, int32_t* __restrict__ cluster_of_rank, int32_t* __restrict__ offsets,
                    float* __restrict__ aggregate_out, int32_t* __restrict__ n_nonempty) {
    __shared__ float agg[DM_KMEANS_MAX_K];
    __shared__ int first[DM_KMEANS_MAX_K], cnt_s[DM_KMEANS_MAX_K], by_rank[DM_KMEANS_MAX_K], off_s[DM_KMEANS_MAX_K + 1];
    __shared__ int n_ne;
    const int j = threadIdx.x;
    const float nan = __uint_as_float(0x7FC00000u);
    int cnt = 0;
    if (j < k) {
        cnt = counts[j];
        float a = nan;
        if (cnt > 0) {
            const int32_t* rows = within + starts[j];
            if (aggregate == 0) {                                  // np.median: NaN if any member is NaN
                bool has_nan = false;
                for (int m = 0; m < cnt; ++m) { const float v = D[rows[m]]; has_nan |= v != v; }
                a = has_nan ? nan : (cnt & 1) ? mid[2 * j + 1] : (mid[2 * j] + mid[2 * j + 1]) * 0.5f;
            } else {                                               // the reference's mean(): left to right in member order, / count
                float sum = 0.f;
                for (int m = 0; m < cnt; ++m) sum += D[rows[m]];
                a = sum / (float)cnt;
            }
        }
        agg[j] = a;
        cnt_s[j] = cnt;
        first[j] = cnt > 0 ? sorted[starts[j]] : n;
    }
    if (j == 0) n_ne = 0;
    __syncthreads();
    if (j < k && cnt > 0) {
        int r = 0;
        const float a = agg[j];
        for (int c = 0; c < k; ++c) {
            if (c == j || cnt_s[c] == 0) continue;
            const float b = agg[c];
            const bool na = a != a, nb = b != b;
            const bool tie = (na && nb) || (!na && !nb && a == b);
            r += tie ? first[c] < first[j] : (na ? !nb : (!nb && b > a));
        }
        by_rank[r] = j;
        atomicAdd(&n_ne, 1);
    }
    __syncthreads();
    if (j == 0) {
        int at = 0;
        for (int r = 0; r < n_ne; ++r) { off_s[r] = at; at += cnt_s[by_rank[r]]; }
        for (int r = n_ne; r <= k; ++r) off_s[r] = n;
        *n_nonempty = n_ne;
    }
    __syncthreads();
    for (int r = j; r <= k; r += DM_KMEANS_MAX_K) offsets[r] = off_s[r];
    if (j < k) {
        cluster_of_rank[j] = j < n_ne ? by_rank[j] : -1;
        aggregate_out[j] = j < n_ne ? agg[by_rank[j]] : nan;
    }
    for (int r = 0; r < n_ne; ++r) {
        const int c = by_rank[r];
        for (int m = j; m < cnt_s[c]; m += DM_KMEANS_MAX_K) order[off_s[r] + m] = within[starts[c] + m];
    }
}

int km_check(int n, int d, int k) {
    if (k < 1 || k > DM_KMEANS_MAX_K) return DM_KMEANS_E_K;
    if (n < k) return DM_KMEANS_E_N_LT_K;
    if (d < 1) return DM_KMEANS_E_D;
    if (n >= (1 << 24)) return DM_KMEANS_E_N_LARGE;
    return 0;
}

int km_trials(int k) { return 2 + (int)log((double)k); }

inline int row_blocks(int rows) { return (rows + kRowWaves - 1) / kRowWaves; }

}  // namespace

}  // namespace dm

using namespace dm;

#define KM_LAUNCH(kernel, grid, block, ...) do { hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__); \
    if (hipGetLastError() != hipSuccess) return DM_KMEANS_E_HIP; } while (0)

extern "C" {

int dm_kmeans_workspace_bytes(int n, int d, int k, size_t* bytes_out) {
    if (!bytes_out) return DM_KMEANS_E_NULL;
    if (int rc = km_check(n, d, k)) return rc;
    *bytes_out = km_layout(nullptr, n, d, k).bytes;
    return 0;
}

int dm_kmeans_fit(void* stream, const void* X, int n, int d, int k, const double* uniforms_f64, int n_uniforms, int max_iter,
                  float tol_rel, void* work, size_t work_bytes, int32_t* labels_i32, float* centers_f32, int32_t* seed_index_i32,
                  float* inertia_f32, int32_t* n_iter_i32) {
    if (int rc = km_check(n, d, k)) return rc;
    if (max_iter < 1) return DM_KMEANS_E_MAX_ITER;
    if (!X || !work || !labels_i32 || !centers_f32 || !seed_index_i32 || !inertia_f32 || !n_iter_i32) return DM_KMEANS_E_NULL;
    const int trials = km_trials(k);
    if (uniforms_f64 ? n_uniforms != 1 + (k - 1) * trials : n_uniforms != 0) return DM_KMEANS_E_UNIFORMS;
    const KmWork w = km_layout(work, n, d, k);
    if (work_bytes < w.bytes) return DM_KMEANS_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    const float* Xf = (const float*)X;

    KM_LAUNCH(km_center_kernel, dim3((d + 255) / 256), dim3(256), Xf, n, d, w.mean, w.colvar, w.Xc);
    KM_LAUNCH(km_rownorm_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), w.Xc, n, d, w.xx);
    KM_LAUNCH(km_begin_kernel, dim3(1), dim3(kBlock), w.state, w.colvar, n, d, tol_rel, w.prev);
    if (uniforms_f64) {                                              // k-means++; otherwise seed_index_i32 is the caller's start
        for (int step = 0; step <= k; ++step) {
            if (step > 0)
                KM_LAUNCH(km_seed_dist_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), w.state, w.Xc, w.xx, n, d, w.dcand);
            KM_LAUNCH(km_seed_pick_kernel, dim3(1), dim3(kBlock), w.state, step, k, n, trials, uniforms_f64, w.dcand, w.closest,
                      w.prefix, seed_index_i32);
        }
    }
    KM_LAUNCH(km_gather_kernel, dim3(k), dim3(256), w.Xc, seed_index_i32, n, d, w.C);
    int done = KM_RUN;
    for (int it = 0; it < max_iter && done == KM_RUN; it += kIterGroup) {
        for (int g = 0; g < kIterGroup && it + g < max_iter; ++g) {
            KM_LAUNCH(km_cnorm_kernel, dim3(row_blocks(k)), dim3(kRowWaves * kWave), w.state, 0, w.C, k, d, w.cnorm);
            KM_LAUNCH(km_assign_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), w.state, 0, w.Xc, w.C, w.cnorm, n, d, k, labels_i32);
            KM_LAUNCH(km_bucket_kernel, dim3(k), dim3(kWave), w.state, labels_i32, n, k, w.counts, w.starts, w.sorted);
            KM_LAUNCH(km_sum_kernel, dim3((d + 255) / 256, k), dim3(256), w.state, w.Xc, w.counts, w.starts, w.sorted, d, w.Cnew);
            KM_LAUNCH(km_finish_kernel, dim3(1), dim3(kBlock), w.state, w.Xc, n, d, k, max_iter, labels_i32, w.prev, w.counts, w.C,
                      w.Cnew, w.rowdist);
        }
        if (hipMemcpyAsync(&done, &w.state->done, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess) return DM_KMEANS_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess) return DM_KMEANS_E_HIP;
    }
    KM_LAUNCH(km_cnorm_kernel, dim3(row_blocks(k)), dim3(kRowWaves * kWave), w.state, 1, w.C, k, d, w.cnorm);
    KM_LAUNCH(km_assign_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), w.state, 1, w.Xc, w.C, w.cnorm, n, d, k, labels_i32);
    KM_LAUNCH(km_rowdist_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), w.Xc, w.C, labels_i32, n, d, w.rowdist);
    KM_LAUNCH(km_end_kernel, dim3(1), dim3(kBlock), w.state, w.rowdist, w.C, w.mean, n, d, k, centers_f32, inertia_f32, n_iter_i32);
    return 0;
}

int dm_cluster_rank(void* stream, const void* X, const void* X_rank_or_null, int n, int d, int d_rank, const int32_t* labels,
                    const float* centers, int k, const float* D_f32, int mode, int aggregate, void* work, size_t work_bytes,
                    int32_t* order, int32_t* cluster_of_rank, int32_t* offsets, float* aggregate_out, int32_t* n_nonempty) {
    if (int rc = km_check(n, d, k)) return rc;
    if (!X || !labels || !centers || !D_f32 || !work || !order || !cluster_of_rank || !offsets || !aggregate_out || !n_nonempty)
        return DM_KMEANS_E_NULL;
    if ((mode != DM_RANK_CENTROID && mode != DM_RANK_FARTHEST) || (aggregate != DM_AGG_MEDIAN && aggregate != DM_AGG_MEAN))
        return DM_KMEANS_E_MODE;
    if (mode == DM_RANK_CENTROID && X_rank_or_null) return DM_KMEANS_E_MODE;       // a centre lives in the clustered space
    const float* Xr = X_rank_or_null ? (const float*)X_rank_or_null : (const float*)X;
    const int dr = X_rank_or_null ? d_rank : d;
    if (dr < 1) return DM_KMEANS_E_D;
    const KmWork w = km_layout(work, n, d > dr ? d : dr, k);
    if (work_bytes < w.bytes) return DM_KMEANS_E_WORK;
    hipStream_t s = (hipStream_t)stream;
    if (mode == DM_RANK_FARTHEST)
        KM_LAUNCH(rk_far_kernel, dim3(k), dim3(kRowWaves * kWave), (const float*)X, centers, n, d, w.far);
    KM_LAUNCH(km_bucket_kernel, dim3(k), dim3(kWave), (const KmState*)nullptr, labels, n, k, w.counts, w.starts, w.sorted);
    KM_LAUNCH(rk_key_kernel, dim3(row_blocks(n)), dim3(kRowWaves * kWave), Xr, centers, mode == DM_RANK_FARTHEST ? w.far : (const int32_t*)nullptr,
              labels, n, k, dr, w.key);
    KM_LAUNCH(rk_place_kernel, dim3((n + 255) / 256), dim3(256), w.key, D_f32, labels, w.counts, w.starts, w.sorted, n, k, w.within, w.mid);
    KM_LAUNCH(rk_rank_kernel, dim3(1), dim3(DM_KMEANS_MAX_K), D_f32, w.counts, w.starts, w.sorted, w.within, w.mid, n, k, aggregate, order,
              cluster_of_rank, offsets, aggregate_out, n_nonempty);
    return 0;
}

}  // extern "C"
