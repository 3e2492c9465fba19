// svm.hip — the Doersch baseline's detector SVMs on the device: scikit-learn's SVC(C=cost, kernel='linear',
// shrinking=False).fit as libsvm's Solver::Solve iterates it (doersch/doersch.py:66-79), for K detectors at once, and the hard
// negatives by decision_function > 0.  The rules are at the top of diff-mining_amd/doersch.py (`svm_fit_host` restates them in numpy).
//
// A detector's samples are rows of one shared fp16 pool, named by a row of an index table; nothing is copied.  The fit is two
// streaming passes over the detector's rows per iteration (Q_i, then Q_j with the update of G), and the structure follows kmeans.hip:
//   - SvmState in the workspace holds the stop flag, n_iter and what one launch hands to the next; iterations are separate launches
//     over a (row block, detector) grid; the host enqueues kIterGroup iterations and reads the K states once per group; the blocks of
//     a finished detector return at once;
//   - every block reduces the per-block candidates of the previous launch to the same i (step A) or the same j and the same stop
//     decision (step B), in a fixed tree; nothing waits on another workgroup;
//   - no value is read in the launch that writes it: step A reads `done`, G, alpha and the i-candidates and writes Q_i, the
//     j-candidates and its own fields of the state; step B reads those and writes G, alpha, the i-candidates and `done`.  What step B
//     needs of rows i and j (G, alpha, QD, Q_i[j]) travels in the state and in the winning j-candidate, because their owners update
//     them in that same launch;
//   - every sum has a fixed order (lane-strided partials over 16-byte chunks + an xor-shuffle tree) that depends on C alone, and
//     there is no floating-point atomic: the same input gives the same bits on every run, in any batch.
// fp64 arithmetic of the trajectory runs without fused multiply-add, as libsvm's build does.
#include "dm_kernels.h"
#include "../../include/dm_engine.h"

#include <math.h>

#pragma clang fp contract(off)

namespace dm {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;                // the row kernels: 4 waves
constexpr int kWaves = kThreads / kWave;
constexpr int kRows = 128;                   // rows per block, 32 consecutive ones per wave
constexpr int kRowsPerWave = kRows / kWaves;
constexpr int kSortBlock = 1024;
constexpr int kIterGroup = 8;                // iterations enqueued between two reads of the states
constexpr double kTau = 1e-12;               // libsvm's TAU

enum { SVM_RUN = 0, SVM_DONE_CONVERGED = 1, SVM_DONE_MAX_ITER = 2, SVM_DONE_NAN = 3, SVM_DONE_BAD = 4 };   // DM_SVM_* status + 1

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct SvmState {
    int done;                                // step B (and the init kernel): SVM_RUN, SVM_DONE_CONVERGED, SVM_DONE_MAX_ITER
    int n_iter;                              // step B, with done
    int stop_a;                              // step A: SVM_RUN, a copy of done, SVM_DONE_NAN or SVM_DONE_BAD
    int i;                                   // step A: the selected i (-1: none)
    double gmax, G_i, alpha_i, QD_i;         // step A
};

struct SvmCandI { double v; int idx; int flag; };                           // flag: 0, SVM_DONE_NAN, SVM_DONE_BAD
struct SvmCandJ { double obj, gmax2, G, alpha, QD; float Qij; int idx; };

struct SvmWork {                             // the workspace, carved by svm_layout
    SvmState* state;
    SvmCandI* ci;
    SvmCandJ* cj;
    double *G, *alpha, *QD;
    float* Qi;
    int32_t *sv, *nsv;
    unsigned long long* key;                 // the hard negatives' entry: it shares the bytes of the fit's arrays
    int32_t *pos, *counter;
    int nb;
    size_t P;
    size_t bytes;
};

inline size_t pow2_ceil(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }

SvmWork svm_layout(void* base, int K, int ld) {
    SvmWork w;
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = base ? (char*)base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    const size_t Kk = (size_t)K, N = (size_t)ld;
    w.nb = (ld + kRows - 1) / kRows;
    w.state = (SvmState*)take(Kk * sizeof(SvmState));
    w.ci = (SvmCandI*)take(Kk * w.nb * sizeof(SvmCandI));
    w.cj = (SvmCandJ*)take(Kk * w.nb * sizeof(SvmCandJ));
    w.G = (double*)take(Kk * N * 8);
    w.alpha = (double*)take(Kk * N * 8);
    w.QD = (double*)take(Kk * N * 8);
    w.Qi = (float*)take(Kk * N * 4);
    w.sv = (int32_t*)take(Kk * N * 4);
    w.nsv = (int32_t*)take(Kk * 4);
    const size_t fit_bytes = off;
    off = 0;
    w.P = pow2_ceil(N);
    w.key = (unsigned long long*)take(Kk * w.P * 8);
    w.pos = (int32_t*)take(Kk * w.P * 4);
    w.counter = (int32_t*)take(Kk * 4);
    w.bytes = off > fit_bytes ? off : fit_bytes;
    return w;
}

// ---- the rules' small pieces ----------------------------------------------------------------------------------------------------
// internal index t -> its place in the detector's sample list, and its libsvm label: the negatives first, as +1
__device__ __forceinline__ int svm_place(int t, int n_pos, int n_neg) { return t < n_neg ? n_pos + t : t - n_neg; }
__device__ __forceinline__ int svm_y(int t, int n_neg) { return t < n_neg ? 1 : -1; }

// a detector whose list cannot be used occupies block 0 alone; it flags itself there
__device__ __forceinline__ bool svm_bad_list(int n, int n_pos, int ld) { return n_pos < 1 || n - n_pos < 1 || n > ld; }
__device__ __forceinline__ int svm_blocks(int n, int n_pos, int ld) { return svm_bad_list(n, n_pos, ld) ? 1 : (n + kRows - 1) / kRows; }

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {            // xor tree: every lane ends with the same bits
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// x . lds over C = 8 C8 features: per lane the chunks lane, lane + 64, ... in ascending order, the eight exact fp32 products of a
// chunk added one by one in fp64; then the xor tree.  Every lane returns the same bits.
__device__ __forceinline__ double wave_dot(const half8* __restrict__ x, const float* xs, int C8, int lane) {
    double a = 0.0;
    for (int c = lane; c < C8; c += kWave) {
        const half8 v = x[c];
        const float4 s0 = *(const float4*)(xs + 8 * c), s1 = *(const float4*)(xs + 8 * c + 4);
        a += (double)((float)v[0] * s0.x);
        a += (double)((float)v[1] * s0.y);
        a += (double)((float)v[2] * s0.z);
        a += (double)((float)v[3] * s0.w);
        a += (double)((float)v[4] * s1.x);
        a += (double)((float)v[5] * s1.y);
        a += (double)((float)v[6] * s1.z);
        a += (double)((float)v[7] * s1.w);
    }
    return wave_sum(a);
}

__device__ __forceinline__ void stage_row(const half8* __restrict__ x, float* xs, int C8) {     // fp16 row -> fp32 in LDS, exact
    for (int c = threadIdx.x; c < C8; c += kThreads) {
        const half8 v = x[c];
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[8 * c + e] = (float)v[e];
    }
}

// the candidate of row t for i: -G over y = +1 rows below the upper bound, G over y = -1 rows above the lower bound
__device__ __forceinline__ bool cand_i(int y, double G, double alpha, double cost, double& v) {
    if (y > 0) { if (alpha >= cost) return false; v = -G; return true; }
    if (alpha <= 0.0) return false;
    v = G;
    return true;
}

// (value, index): libsvm's `>=` keeps the LAST index among equals
__device__ __forceinline__ bool better_i(double v, int idx, double bv, int bidx) {
    if (idx < 0) return false;
    if (bidx < 0) return true;
    return v > bv || (v == bv && idx > bidx);
}
__device__ __forceinline__ bool better_j(double obj, int idx, double bobj, int bidx) {          // libsvm's `<=`
    if (idx < 0) return false;
    if (bidx < 0) return true;
    return obj < bobj || (obj == bobj && idx > bidx);
}

// libsvm's two-variable update (Solver::Solve), both classes at one cost
__device__ __forceinline__ void svm_pair(int yi, int yj, double Gi, double Gj, double ai, double aj, float Qij, double QDi, double QDj,
                                         double cost, double& nai, double& naj) {
    if (yi != yj) {
        double quad = QDi + QDj + 2.0 * (double)Qij;
        if (quad <= 0) quad = kTau;
        const double delta = (-Gi - Gj) / quad;
        const double diff = ai - aj;
        ai += delta;
        aj += delta;
        if (diff > 0) { if (aj < 0) { aj = 0; ai = diff; } }
        else { if (ai < 0) { ai = 0; aj = -diff; } }
        if (diff > 0) { if (ai > cost) { ai = cost; aj = cost - diff; } }                        // C_i - C_j = 0
        else { if (aj > cost) { aj = cost; ai = cost + diff; } }
    } else {
        double quad = QDi + QDj - 2.0 * (double)Qij;
        if (quad <= 0) quad = kTau;
        const double delta = (Gi - Gj) / quad;
        const double sum = ai + aj;
        ai -= delta;
        aj += delta;
        if (sum > cost) { if (ai > cost) { ai = cost; aj = sum - cost; } }
        else { if (aj < 0) { aj = 0; ai = sum; } }
        if (sum > cost) { if (aj > cost) { aj = cost; ai = sum - cost; } }
        else { if (ai < 0) { ai = 0; aj = sum; } }
    }
    nai = ai;
    naj = aj;
}

// ---- the fit --------------------------------------------------------------------------------------------------------------------
// Per row: QD, G = -1, alpha = 0; per block the first i-candidate and the flag of a row that cannot be used.
__global__ __launch_bounds__(kThreads)
void svm_init_kernel(const half8* __restrict__ rows, int R, int C8, const int32_t* __restrict__ sample, int ld,
                     const int32_t* __restrict__ n_arr, const int32_t* __restrict__ n_pos_arr, double cost, SvmWork w) {
    __shared__ SvmCandI part[kWaves];
    const int k = blockIdx.y, b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = n_arr[k], n_pos = n_pos_arr[k];
    if (b >= svm_blocks(n, n_pos, ld)) return;
    const int n_neg = n - n_pos;
    SvmCandI best = {0.0, -1, 0};
    if (svm_bad_list(n, n_pos, ld)) {
        best.flag = SVM_DONE_BAD;
    } else {
        const size_t base = (size_t)k * ld;
        for (int r = 0; r < kRowsPerWave; ++r) {
            const int t = b * kRows + wave * kRowsPerWave + r;
            if (t >= n) break;
            const int s = sample[base + svm_place(t, n_pos, n_neg)];
            if (s < 0 || s >= R) { best.flag = SVM_DONE_BAD; continue; }
            const half8* x = rows + (size_t)s * C8;
            double a = 0.0;
            for (int c = lane; c < C8; c += kWave) {
                const half8 v = x[c];
#pragma unroll
                for (int e = 0; e < 8; ++e) a += (double)((float)v[e] * (float)v[e]);
            }
            a = wave_sum(a);
            if (lane == 0) {
                w.G[base + t] = -1.0;
                w.alpha[base + t] = 0.0;
                w.QD[base + t] = a;
            }
            if (!(fabs(a) <= 1.79769313486231570815e308) && best.flag == 0) best.flag = SVM_DONE_NAN;      // inf or NaN
            double v;
            if (cand_i(svm_y(t, n_neg), -1.0, 0.0, cost, v) && better_i(v, t, best.v, best.idx)) { best.v = v; best.idx = t; }
        }
    }
    if (lane == 0) part[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < kWaves; ++q) {
            if (better_i(part[q].v, part[q].idx, best.v, best.idx)) { best.v = part[q].v; best.idx = part[q].idx; }
            best.flag = max(best.flag, part[q].flag);
        }
        w.ci[(size_t)k * w.nb + b] = best;
        if (b == 0) {
            w.state[k].done = SVM_RUN;
            w.state[k].n_iter = 0;
        }
    }
}

// Step A: every block reduces the i-candidates to the same i, then Q_i over its rows and its j-candidate.
__global__ __launch_bounds__(kThreads)
void svm_step_a_kernel(const half8* __restrict__ rows, int C8, const int32_t* __restrict__ sample, int ld,
                       const int32_t* __restrict__ n_arr, const int32_t* __restrict__ n_pos_arr, double cost, SvmWork w) {
    extern __shared__ __align__(16) float xs[];
    __shared__ SvmCandI ri[kThreads];
    __shared__ SvmCandJ part[kWaves];
    const int k = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = n_arr[k], n_pos = n_pos_arr[k];
    const int nbk = svm_blocks(n, n_pos, ld);
    if (b >= nbk) return;
    SvmState* st = w.state + k;
    const int done = st->done;
    if (done != SVM_RUN) {
        if (b == 0 && tid == 0) st->stop_a = done;
        return;
    }
    SvmCandI best = {0.0, -1, 0};
    for (int q = tid; q < nbk; q += kThreads) {
        const SvmCandI c = w.ci[(size_t)k * w.nb + q];
        if (better_i(c.v, c.idx, best.v, best.idx)) { best.v = c.v; best.idx = c.idx; }
        best.flag = max(best.flag, c.flag);
    }
    ri[tid] = best;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const SvmCandI c = ri[tid + o];
            SvmCandI m = ri[tid];
            if (better_i(c.v, c.idx, m.v, m.idx)) { m.v = c.v; m.idx = c.idx; }
            m.flag = max(m.flag, c.flag);
            ri[tid] = m;
        }
        __syncthreads();
    }
    best = ri[0];
    if (best.flag) {
        if (b == 0 && tid == 0) st->stop_a = best.flag;
        return;
    }
    const int n_neg = n - n_pos;
    const size_t base = (size_t)k * ld;
    const int i = best.idx;
    const double gmax = best.v;
    if (b == 0 && tid == 0) {
        st->stop_a = SVM_RUN;
        st->i = i;
        st->gmax = gmax;
        if (i >= 0) {
            st->G_i = w.G[base + i];
            st->alpha_i = w.alpha[base + i];
            st->QD_i = w.QD[base + i];
        }
    }
    SvmCandJ bj = {0.0, -INFINITY, 0.0, 0.0, 0.0, 0.f, -1};
    if (i < 0) {                                             // nothing can move up: step B stops
        if (tid == 0) w.cj[(size_t)k * w.nb + b] = bj;
        return;
    }
    stage_row(rows + (size_t)sample[base + svm_place(i, n_pos, n_neg)] * C8, xs, C8);
    __syncthreads();
    const int yi = svm_y(i, n_neg);
    const double QDi = w.QD[base + i];
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int t = b * kRows + wave * kRowsPerWave + r;
        if (t >= n) break;
        const int yt = svm_y(t, n_neg);
        const double dot = wave_dot(rows + (size_t)sample[base + svm_place(t, n_pos, n_neg)] * C8, xs, C8, lane);
        const float q = (float)((double)(yi * yt) * dot);
        if (lane == 0) w.Qi[base + t] = q;
        const double Gt = w.G[base + t], at = w.alpha[base + t];
        if (yt > 0 ? at <= 0.0 : at >= cost) continue;       // not a candidate for j
        const double grad = yt > 0 ? gmax + Gt : gmax - Gt;
        const double g2 = yt > 0 ? Gt : -Gt;
        if (g2 >= bj.gmax2) bj.gmax2 = g2;
        if (grad > 0) {
            const double QDt = w.QD[base + t];
            double quad = (QDi + QDt) - 2.0 * (double)((float)(yi * yt) * q);
            if (!(quad > 0)) quad = kTau;
            const double obj = -(grad * grad) / quad;
            if (better_j(obj, t, bj.obj, bj.idx)) { bj.obj = obj; bj.idx = t; bj.G = Gt; bj.alpha = at; bj.QD = QDt; bj.Qij = q; }
        }
    }
    if (lane == 0) part[wave] = bj;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < kWaves; ++q) {
            const SvmCandJ c = part[q];
            const double g2 = c.gmax2 > bj.gmax2 ? c.gmax2 : bj.gmax2;
            if (better_j(c.obj, c.idx, bj.obj, bj.idx)) bj = c;
            bj.gmax2 = g2;
        }
        w.cj[(size_t)k * w.nb + b] = bj;
    }
}

// Step B: every block reduces the j-candidates to the same j and the same stop decision, recomputes the two new alphas, then Q_j
// over its rows, the update of G, the two alphas where it owns them, and its i-candidate of the next iteration.
__global__ __launch_bounds__(kThreads)
void svm_step_b_kernel(const half8* __restrict__ rows, int C8, const int32_t* __restrict__ sample, int ld,
                       const int32_t* __restrict__ n_arr, const int32_t* __restrict__ n_pos_arr, double cost, double eps, int max_iter,
                       int it, SvmWork w) {
    extern __shared__ __align__(16) float xs[];
    __shared__ SvmCandJ rj[kThreads];
    __shared__ SvmCandI part[kWaves];
    const int k = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = n_arr[k], n_pos = n_pos_arr[k];
    const int nbk = svm_blocks(n, n_pos, ld);
    if (b >= nbk) return;
    SvmState* st = w.state + k;
    if (st->stop_a != SVM_RUN) return;
    SvmCandJ bj = {0.0, -INFINITY, 0.0, 0.0, 0.0, 0.f, -1};
    for (int q = tid; q < nbk; q += kThreads) {
        const SvmCandJ c = w.cj[(size_t)k * w.nb + q];
        const double g2 = c.gmax2 > bj.gmax2 ? c.gmax2 : bj.gmax2;
        if (better_j(c.obj, c.idx, bj.obj, bj.idx)) bj = c;
        bj.gmax2 = g2;
    }
    rj[tid] = bj;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const SvmCandJ c = rj[tid + o];
            SvmCandJ m = rj[tid];
            const double g2 = c.gmax2 > m.gmax2 ? c.gmax2 : m.gmax2;
            if (better_j(c.obj, c.idx, m.obj, m.idx)) m = c;
            m.gmax2 = g2;
            rj[tid] = m;
        }
        __syncthreads();
    }
    bj = rj[0];
    const int i = st->i, j = bj.idx;
    if (i < 0 || j < 0 || st->gmax + bj.gmax2 < eps) {
        if (b == 0 && tid == 0) {
            st->done = SVM_DONE_CONVERGED;
            st->n_iter = it;
        }
        return;
    }
    const int n_neg = n - n_pos;
    const size_t base = (size_t)k * ld;
    const int yi = svm_y(i, n_neg), yj = svm_y(j, n_neg);
    const double ai = st->alpha_i, aj = bj.alpha;
    double nai, naj;
    svm_pair(yi, yj, st->G_i, bj.G, ai, aj, bj.Qij, st->QD_i, bj.QD, cost, nai, naj);
    const double dai = nai - ai, daj = naj - aj;
    stage_row(rows + (size_t)sample[base + svm_place(j, n_pos, n_neg)] * C8, xs, C8);
    __syncthreads();
    SvmCandI best = {0.0, -1, 0};
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int t = b * kRows + wave * kRowsPerWave + r;
        if (t >= n) break;
        const int yt = svm_y(t, n_neg);
        const double dot = wave_dot(rows + (size_t)sample[base + svm_place(t, n_pos, n_neg)] * C8, xs, C8, lane);
        const float qj = (float)((double)(yj * yt) * dot);
        const double Gt = w.G[base + t] + ((double)w.Qi[base + t] * dai + (double)qj * daj);
        double at = w.alpha[base + t];
        if (t == i) at = nai;
        if (t == j) at = naj;
        if (lane == 0) {
            w.G[base + t] = Gt;
            if (t == i || t == j) w.alpha[base + t] = at;
        }
        double v;
        if (cand_i(yt, Gt, at, cost, v) && better_i(v, t, best.v, best.idx)) { best.v = v; best.idx = t; }
    }
    if (lane == 0) part[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < kWaves; ++q)
            if (better_i(part[q].v, part[q].idx, best.v, best.idx)) { best.v = part[q].v; best.idx = part[q].idx; }
        w.ci[(size_t)k * w.nb + b] = best;
        if (b == 0) {
            const int limit = max_iter > 0 ? max_iter : max(10000000, 100 * n);
            if (it + 1 >= limit) {
                st->done = SVM_DONE_MAX_ITER;
                st->n_iter = it + 1;
            }
        }
    }
}

// One wave per detector: status, n_iter, rho, the alphas in sample order, and the support vectors in ascending internal index.
__global__ __launch_bounds__(kWave)
void svm_finish_kernel(int ld, const int32_t* __restrict__ n_arr, const int32_t* __restrict__ n_pos_arr, double cost, SvmWork w,
                       double* __restrict__ b_out, int32_t* __restrict__ n_iter_out, int32_t* __restrict__ status_out,
                       double* __restrict__ alpha_out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const SvmState* st = w.state + k;
    const int code = st->stop_a >= SVM_DONE_NAN ? st->stop_a : st->done;
    const size_t base = (size_t)k * ld;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    if (code >= SVM_DONE_NAN || code == SVM_RUN) {
        if (alpha_out) for (int p = lane; p < ld; p += kWave) alpha_out[base + p] = 0.0;
        if (lane == 0) {
            b_out[k] = nan;
            n_iter_out[k] = 0;
            status_out[k] = (code == SVM_RUN ? SVM_DONE_BAD : code) - 1;
            w.nsv[k] = 0;
        }
        return;
    }
    const int n = n_arr[k], n_pos = n_pos_arr[k], n_neg = n - n_pos;
    double sum_free = 0.0, ub = INFINITY, lb = -INFINITY;
    int nr_free = 0, nsv = 0;
    for (int t0 = 0; t0 < n; t0 += kWave) {
        const int t = t0 + lane;
        const bool in = t < n;
        const double a = in ? w.alpha[base + t] : 0.0;
        const int y = svm_y(t, n_neg);
        const double yG = in ? (double)y * w.G[base + t] : 0.0;
        const bool upper = a >= cost, lower = a <= 0.0;
        if (in) {
            if (upper) { if (y < 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
            else if (lower) { if (y > 0) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
        }
        unsigned long long free_m = __ballot(in && !upper && !lower);
        nr_free += __popcll(free_m);
        while (free_m) {                                     // libsvm's sum, in index order
            const int l = __ffsll((long long)free_m) - 1;
            sum_free += __shfl(yG, l, kWave);
            free_m &= free_m - 1;
        }
        const bool is_sv = in && a > 0.0;
        const unsigned long long sv_m = __ballot(is_sv);
        if (is_sv) w.sv[base + nsv + __popcll(sv_m & ((1ull << lane) - 1ull))] = t;
        nsv += __popcll(sv_m);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        ub = fmin(ub, __shfl_xor(ub, o, kWave));
        lb = fmax(lb, __shfl_xor(lb, o, kWave));
    }
    if (alpha_out)
        for (int p = lane; p < ld; p += kWave)
            alpha_out[base + p] = p < n ? w.alpha[base + (p < n_pos ? n_neg + p : p - n_pos)] : 0.0;
    if (lane == 0) {
        b_out[k] = nr_free > 0 ? sum_free / (double)nr_free : (ub + lb) / 2;
        n_iter_out[k] = st->n_iter;
        status_out[k] = code - 1;
        w.nsv[k] = nsv;
    }
}

// One thread per (detector, feature): w = -sum alpha_t y_t x_t over the support vectors in ascending internal index.
__global__ __launch_bounds__(kThreads)
void svm_w_kernel(const _Float16* __restrict__ rows, int C, const int32_t* __restrict__ sample, int ld,
                  const int32_t* __restrict__ n_arr, const int32_t* __restrict__ n_pos_arr, const int32_t* __restrict__ status, SvmWork w,
                  double* __restrict__ w_out) {
    const int k = blockIdx.y, c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    if (status[k] >= DM_SVM_NAN) {
        w_out[(size_t)k * C + c] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const int n = n_arr[k], n_pos = n_pos_arr[k], n_neg = n - n_pos;
    const size_t base = (size_t)k * ld;
    const int nsv = w.nsv[k];
    double a = 0.0;
    for (int m = 0; m < nsv; ++m) {
        const int t = w.sv[base + m];
        const double coef = w.alpha[base + t] * (double)svm_y(t, n_neg);
        a = a - coef * (double)rows[(size_t)sample[base + svm_place(t, n_pos, n_neg)] * C + c];
    }
    w_out[(size_t)k * C + c] = a;
}

// ---- hard negatives -------------------------------------------------------------------------------------------------------------
// One wave per sample p: s = x_p . w + b in fp64; the admitted ones (s > 0) go, in any order, into the detector's key list — the sort
// orders them by (score, p), and no two keys are equal.
__global__ __launch_bounds__(kThreads)
void svm_score_kernel(const half8* __restrict__ rows, int R, int C8, const int32_t* __restrict__ sample, int ld,
                      const int32_t* __restrict__ n_arr, const int32_t* __restrict__ first_arr, const double* __restrict__ w_in,
                      const double* __restrict__ b_in, SvmWork w, double* __restrict__ score) {
    extern __shared__ __align__(16) double ws[];
    const int k = blockIdx.y, b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = min(n_arr[k], ld), first = max(first_arr[k], 0);
    const size_t base = (size_t)k * ld;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const int p0 = b * kRows;
    if (p0 + kRows <= first || p0 >= n) {                    // no sample of this block is searched
        for (int p = p0 + threadIdx.x; p < min(p0 + kRows, ld); p += kThreads) score[base + p] = nan;
        return;
    }
    for (int c = threadIdx.x; c < 8 * C8; c += kThreads) ws[c] = w_in[(size_t)k * 8 * C8 + c];
    __syncthreads();
    const double bias = b_in[k];
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int p = p0 + wave * kRowsPerWave + r;
        if (p >= ld) break;
        double s = nan;
        if (p >= first && p < n) {
            const int si = sample[base + p];
            if (si >= 0 && si < R) {
                const half8* x = rows + (size_t)si * C8;
                double a = 0.0;
                for (int c = lane; c < C8; c += kWave) {
                    const half8 v = x[c];
#pragma unroll
                    for (int e = 0; e < 8; ++e) a += (double)(float)v[e] * ws[8 * c + e];
                }
                s = wave_sum(a) + bias;
            }
        }
        if (lane == 0) {
            score[base + p] = s;
            if (s > 0) {
                const int slot = atomicAdd(w.counter + k, 1);
                w.key[(size_t)k * w.P + slot] = ~(unsigned long long)__double_as_longlong(s);     // descending score
                w.pos[(size_t)k * w.P + slot] = p;
            }
        }
    }
}

// One block per detector: a bitonic sort of its (key, p) pairs in global memory, ascending, then the list.
__global__ __launch_bounds__(kSortBlock)
void svm_sort_kernel(int ld, const int32_t* __restrict__ max_samples_arr, SvmWork w, int32_t* __restrict__ hard,
                     int32_t* __restrict__ count) {
    const int k = blockIdx.x, tid = threadIdx.x;
    const int m = min(w.counter[k], ld);
    unsigned long long* key = w.key + (size_t)k * w.P;
    int32_t* pos = w.pos + (size_t)k * w.P;
    int P = 1;
    while (P < m) P <<= 1;
    for (int q = m + tid; q < P; q += kSortBlock) { key[q] = ~0ull; pos[q] = 0x7FFFFFFF; }
    __threadfence_block();
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = tid; q < P / 2; q += kSortBlock) {
                const int lo = 2 * q - (q & (stride - 1)), hi = lo + stride;
                const unsigned long long ka = key[lo], kb = key[hi];
                const int pa = pos[lo], pb = pos[hi];
                const bool a_after_b = ka > kb || (ka == kb && pa > pb);
                if (a_after_b == ((lo & size) == 0)) { key[lo] = kb; key[hi] = ka; pos[lo] = pb; pos[hi] = pa; }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    const int cnt = min(m, max(max_samples_arr[k], 0));
    for (int q = tid; q < ld; q += kSortBlock) hard[(size_t)k * ld + q] = q < cnt ? pos[q] : -1;
    if (tid == 0) count[k] = cnt;
}

int svm_check(int R, int C, int ld, int K) {
    if (K < 1 || K > DM_SVM_MAX_DETECTORS) return DM_SVM_E_K;
    if (C < 8 || C % 8 || C > DM_SVM_MAX_FEATURES) return DM_SVM_E_C;
    if (R < 1) return DM_SVM_E_ROWS;
    if (ld < 2) return DM_SVM_E_LD;
    if (ld >= (1 << 24)) return DM_SVM_E_N_LARGE;
    return 0;
}

}  // namespace

}  // namespace dm

using namespace dm;

#define SVM_LAUNCH(kernel, grid, block, lds, ...) do { hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__); \
    if (hipGetLastError() != hipSuccess) return DM_SVM_E_HIP; } while (0)

extern "C" {

size_t dm_svm_workspace_bytes(int K, int n_max) {
    if (K < 1 || K > DM_SVM_MAX_DETECTORS || n_max < 2 || n_max >= (1 << 24)) return 0;
    return svm_layout(nullptr, K, n_max).bytes;
}

int dm_svm_fit(void* stream, const void* rows_f16, int R, int C, const int32_t* sample_i32, int ld, const int32_t* n_i32,
               const int32_t* n_pos_i32, int K, double cost, double eps, int max_iter, void* work, size_t work_bytes, double* w_f64,
               double* b_f64, int32_t* n_iter_i32, int32_t* status_i32, double* alpha_f64_or_null) {
    if (!rows_f16 || !sample_i32 || !n_i32 || !n_pos_i32 || !work || !w_f64 || !b_f64 || !n_iter_i32 || !status_i32) return DM_SVM_E_NULL;
    if (int rc = svm_check(R, C, ld, K)) return rc;
    if (!(cost > 0) || !(eps > 0)) return DM_SVM_E_COST;
    const SvmWork w = svm_layout(work, K, ld);
    if (work_bytes < w.bytes) return DM_SVM_E_WORK;
    if (((uintptr_t)rows_f16 | (uintptr_t)work) & 15) return DM_SVM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const half8* rows = (const half8*)rows_f16;
    const int C8 = C / 8;
    const dim3 grid(w.nb, K), block(kThreads);
    const size_t lds = (size_t)C * sizeof(float);
    SVM_LAUNCH(svm_init_kernel, grid, block, 0, rows, R, C8, sample_i32, ld, n_i32, n_pos_i32, cost, w);
    const long long limit = max_iter > 0 ? max_iter : (100ll * ld > 10000000ll ? 100ll * ld : 10000000ll);
    std::vector<SvmState> states((size_t)K);
    bool running = true;
    for (long long it = 0; running && it < limit; it += kIterGroup) {
        for (int g = 0; g < kIterGroup && it + g < limit; ++g) {
            SVM_LAUNCH(svm_step_a_kernel, grid, block, lds, rows, C8, sample_i32, ld, n_i32, n_pos_i32, cost, w);
            SVM_LAUNCH(svm_step_b_kernel, grid, block, lds, rows, C8, sample_i32, ld, n_i32, n_pos_i32, cost, eps, max_iter,
                       (int)(it + g), w);
        }
        if (hipMemcpyAsync(states.data(), w.state, (size_t)K * sizeof(SvmState), hipMemcpyDeviceToHost, s) != hipSuccess)
            return DM_SVM_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess) return DM_SVM_E_HIP;
        running = false;
        for (int k = 0; k < K; ++k) running |= states[k].done == SVM_RUN && states[k].stop_a == SVM_RUN;
    }
    SVM_LAUNCH(svm_finish_kernel, dim3(K), dim3(kWave), 0, ld, n_i32, n_pos_i32, cost, w, b_f64, n_iter_i32, status_i32,
               alpha_f64_or_null);
    SVM_LAUNCH(svm_w_kernel, dim3((C + kThreads - 1) / kThreads, K), block, 0, (const _Float16*)rows_f16, C, sample_i32, ld, n_i32,
               n_pos_i32, status_i32, w, w_f64);
    if (hipStreamSynchronize(s) != hipSuccess) return DM_SVM_E_HIP;
    return 0;
}

int dm_svm_hard_negatives(void* stream, const void* rows_f16, int R, int C, const int32_t* sample_i32, int ld, const int32_t* n_i32,
                          const int32_t* first_i32, const int32_t* max_samples_i32, int K, const double* w_f64, const double* b_f64,
                          void* work, size_t work_bytes, double* score_f64, int32_t* hard_i32, int32_t* count_i32) {
    if (!rows_f16 || !sample_i32 || !n_i32 || !first_i32 || !max_samples_i32 || !w_f64 || !b_f64 || !work || !score_f64 || !hard_i32 ||
        !count_i32)
        return DM_SVM_E_NULL;
    if (int rc = svm_check(R, C, ld, K)) return rc;
    const SvmWork w = svm_layout(work, K, ld);
    if (work_bytes < w.bytes) return DM_SVM_E_WORK;
    if (((uintptr_t)rows_f16 | (uintptr_t)work) & 15) return DM_SVM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w.counter, 0, (size_t)K * 4, s) != hipSuccess) return DM_SVM_E_HIP;
    SVM_LAUNCH(svm_score_kernel, dim3(w.nb, K), dim3(kThreads), (size_t)C * sizeof(double), (const half8*)rows_f16, R, C / 8,
               sample_i32, ld, n_i32, first_i32, w_f64, b_f64, w, score_f64);
    SVM_LAUNCH(svm_sort_kernel, dim3(K), dim3(kSortBlock), 0, ld, max_samples_i32, w, hard_i32, count_i32);
    return 0;
}

}  // extern "C"
