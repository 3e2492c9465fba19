// f32_train_attn.hip — attention backward of the fp32 net's transformer blocks, gfx950: dQ, dK, dV of O = softmax(Q K^T scale) V from
// Q, K, V, O, dO.  fp32 operands on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), no floating-point atomics: every sum
// has one fixed order, the same bits from run to run.  That costs matrix products: 1 (statistics) + 3 (dQ) + 4 (dK, dV) = 7 + 1 against
// the forward pass's 2, because the query-owned and the key-owned sweep each recompute S and dP instead of sharing them through atomics.
//
// The MFMA roles are those of attn32_kernel (f32_ops.hip): lane (c = lane & 15, g = lane >> 4) feeds A[row c][k g] and B[k g][column c] and
// holds D[row 4 g + r][column c] in register r.  A D tile therefore lies in its lanes exactly as the B operand of a following product whose
// k index is that tile's row: P and dS never leave their lanes.
//
//   attn32_stats   blocks own 64 queries and sweep the keys: S^T = K Q^T with the forward kernel's online maximum and sum ->
//                  L[q] = m + log2(l) in the exp2 domain (scores pre-scaled by scale log2 e), and Delta[q] = sum_d dO[q][d] O[q][d];
//                  (L, Delta) per (b, head, q) go to the head of the workspace.  It lives here, not in attn32_kernel, so that the forward
//                  kernel's machine code stays what it was.
//   attn32_dq      blocks own 64 queries (a wave: 16) and sweep the keys: S^T = K Q^T and dP^T = V dO^T (A = rows of K / V from LDS,
//                  B = Q^T / dO^T in registers), P = 2^(s' - L), dS^T = P (dP^T - Delta) scale stays in its lanes (key 4 g + r, query c) as
//                  the B operand of dQ^T += K^T dS^T (A = K^T: d = 16 dt + c, key 4 g + r).
//   attn32_dkv     blocks own 64 keys (a wave: 16) and sweep the queries of one slab: S = Q K^T and dP = dO V^T (A = rows of Q scale log2 e /
//                  dO from LDS, B = K^T / V^T in registers); the accumulators (query 4 g + r, key c) are the B operands of
//                  dV^T += dO^T P and dK^T += Q'^T dS (dS = P (dP - Delta) ln 2, because Q' carries scale log2 e).  L and Delta are read per
//                  query row; a padded query gets L = +inf, so its P is exactly 0.
//   attn32_dkv_reduce  cross-attention has two key tiles per (b, head) — too few blocks —, so the queries are cut into attn_bwd_slabs(Tq, Tk)
//                  slabs; every slab writes its partial dK | dV rows to the workspace and this kernel adds them in ascending slab order
//                  into dK and dV (one slab too: one code path).
//
// LDS strides, as derived above attn32_kernel: a fragment read "row c, column 4 s + g" (the A operand of S, dP) is conflict-free on a row
// stride D + 2 (half of it odd: 42 / 82 / 162), a read "row 4 g + r, column 16 dt + c" (the A operand of dQ^T, dK^T, dV^T) on D + 4
// (4 x odd: rows 4 apart lie 16 banks apart).  No stride serves both, so an operand that is read both ways (K in attn32_dq; Q and dO in
// attn32_dkv) is staged twice, once per layout.  A tile is staged, a barrier, consumed, a barrier: one stage, no register prefetch.
#include "f32_kernels.h"
#include <math.h>

namespace dm32 {
namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;
constexpr int AB_QB = 64;          // queries per block of the statistics and dQ kernels, keys per block of the dK / dV kernel

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }      // one v_exp_f32; -inf -> 0

// rows r0 .. r0 + T - 1 of `src` (row stride ld, D floats each; rows >= rend are zeros) times `mul` -> LDS layout A (row stride D + 2; rows
// are 8-byte aligned only) and / or layout B (row stride D + 4)
template <int D, int T, bool WA, bool WB>
__device__ __forceinline__ void stage_rows(const float* src, int ld, int r0, int rend, float mul, float* A, float* Bm, int tid) {
    constexpr int Q4 = D / 4;
    for (int i = tid; i < T * Q4; i += 256) {
        const int r = i / Q4, c4 = i - r * Q4, row = r0 + r;
        v4f v = {0.f, 0.f, 0.f, 0.f};
        if (row < rend) v = *reinterpret_cast<const v4f*>(src + (long long)row * ld + 4 * c4) * mul;
        if (WA) {
            float* a = A + r * (D + 2) + 4 * c4;
            *reinterpret_cast<v2f*>(a) = v2f{v[0], v[1]};
            *reinterpret_cast<v2f*>(a + 2) = v2f{v[2], v[3]};
        }
        if (WB) *reinterpret_cast<v4f*>(Bm + r * (D + 4) + 4 * c4) = v;
    }
}

template <int D, int KT>
__global__ __launch_bounds__(256) void attn32_stats_kernel(AttnBwdParams p, float* stats) {
    constexpr int LDK = D + 2, KS = D / 4, NKT = KT / 16;
    __shared__ __attribute__((aligned(16))) float Ks[KT * LDK];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.heads, h = bh - b * p.heads;
    const int q = blockIdx.x * AB_QB + wid * 16 + c, qi = q < p.Tq ? q : p.Tq - 1;
    const float* Qr = p.Q + (long long)b * p.bsq + (long long)qi * p.ldq + h * D;
    const float* Kb = p.K + (long long)b * p.bsk + h * D;
    const float qscale = p.scale * LOG2E;
    float qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = Qr[4 * s + g] * qscale;
    float mrun = -INFINITY, lrun = 0.f;
    for (int k0 = 0; k0 < p.Tk; k0 += KT) {
        __syncthreads();
        stage_rows<D, KT, true, false>(Kb, p.ldk, k0, p.Tk, 1.0f, Ks, nullptr, tid);
        __syncthreads();
        v4f sacc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) sacc[kt] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) sacc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(kt * 16 + c) * LDK + 4 * s + g], qf[s], sacc[kt], 0, 0, 0);
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = k0 + kt * 16 + 4 * g + r < p.Tk ? sacc[kt][r] : -INFINITY;
                sacc[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mnew = fmaxf(mrun, mx);              // finite: every key tile holds at least one real key
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += fast_exp2(sacc[kt][r] - mnew);
        lrun = lrun * fast_exp2(mrun - mnew) + sum;
        mrun = mnew;
    }
    float l = lrun;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    // Delta: lane g sums the g-th quarter of the row in ascending order, the quarters are added pairwise
    const float* Or = p.O + (long long)b * p.bso + (long long)qi * p.ldo + h * D + g * KS;
    const float* dOr = p.dO + (long long)b * p.bsdo + (long long)qi * p.lddo + h * D + g * KS;
    float dl = 0.f;
#pragma unroll
    for (int i = 0; i < KS; ++i) dl += dOr[i] * Or[i];
    dl += __shfl_xor(dl, 16);
    dl += __shfl_xor(dl, 32);
    if (g == 0 && q < p.Tq) {
        float* o = stats + 2 * ((long long)bh * p.Tq + q);
        o[0] = mrun + log2f(l);
        o[1] = dl;
    }
}

template <int D, int KT>
__global__ __launch_bounds__(256) void attn32_dq_kernel(AttnBwdParams p, const float* stats) {
    constexpr int LDK = D + 2, LD = D + 4, KS = D / 4, DT = (D + 15) / 16, NKT = KT / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* K1 = smem;                       // [KT][LDK]: rows of K for S^T
    float* V1 = K1 + KT * LDK;              // [KT][LDK]: rows of V for dP^T
    float* K2 = V1 + KT * LDK;              // [KT][LD] (+ 16 of slack: the last d tile of D = 40 reads columns 40 .. 47): K^T for dQ^T
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.heads, h = bh - b * p.heads;
    const int q = blockIdx.x * AB_QB + wid * 16 + c, qi = q < p.Tq ? q : p.Tq - 1;
    const float* Qr = p.Q + (long long)b * p.bsq + (long long)qi * p.ldq + h * D;
    const float* dOr = p.dO + (long long)b * p.bsdo + (long long)qi * p.lddo + h * D;
    const float* Kb = p.K + (long long)b * p.bsk + h * D;
    const float* Vb = p.V + (long long)b * p.bsv + h * D;
    const float qscale = p.scale * LOG2E;
    float qf[KS], dof[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) { qf[s] = Qr[4 * s + g] * qscale; dof[s] = dOr[4 * s + g]; }
    const float Lq = stats[2 * ((long long)bh * p.Tq + qi)], Dq = stats[2 * ((long long)bh * p.Tq + qi) + 1];
    v4f acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = v4f{0.f, 0.f, 0.f, 0.f};
    if (tid < 16) K2[KT * LD + tid] = 0.f;
    for (int k0 = 0; k0 < p.Tk; k0 += KT) {
        __syncthreads();
        stage_rows<D, KT, true, true>(Kb, p.ldk, k0, p.Tk, 1.0f, K1, K2, tid);
        stage_rows<D, KT, true, false>(Vb, p.ldv, k0, p.Tk, 1.0f, V1, nullptr, tid);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            v4f s4 = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(K1[(kt * 16 + c) * LDK + 4 * s + g], qf[s], s4, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(V1[(kt * 16 + c) * LDK + 4 * s + g], dof[s], dp, 0, 0, 0);
            }
            v4f ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = k0 + kt * 16 + 4 * g + r < p.Tk ? fast_exp2(s4[r] - Lq) : 0.f;
                ds[r] = pv * (dp[r] - Dq) * p.scale;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(K2[(kt * 16 + 4 * g + r) * LD + dt * 16 + c], ds[r], acc[dt], 0, 0, 0);
        }
    }
    if (q < p.Tq) {
        float* o = p.dQ + (long long)b * p.bsdq + (long long)q * p.lddq + h * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = dt * 16 + 4 * g;
            if (d < D) *reinterpret_cast<v4f*>(o + d) = acc[dt];
        }
    }
}

template <int D, int QT>
__global__ __launch_bounds__(256) void attn32_dkv_kernel(AttnBwdParams p, const float* stats, float* part, int slab_len) {
    constexpr int LDK = D + 2, LD = D + 4, KS = D / 4, DT = (D + 15) / 16, NQT = QT / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Q1 = smem;                       // [QT][LDK]: rows of Q scale log2 e for S
    float* O1 = Q1 + QT * LDK;              // [QT][LDK]: rows of dO for dP
    float* Q2 = O1 + QT * LDK;              // [QT][LD] + 16: Q'^T for dK^T
    float* O2 = Q2 + QT * LD + 16;          // [QT][LD] + 16: dO^T for dV^T
    float* Ls = O2 + QT * LD + 16;          // [QT]
    float* Ds = Ls + QT;                    // [QT]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.heads, h = bh - b * p.heads;
    const int key = blockIdx.x * AB_QB + wid * 16 + c, ki = key < p.Tk ? key : p.Tk - 1;
    const float* Kr = p.K + (long long)b * p.bsk + (long long)ki * p.ldk + h * D;
    const float* Vr = p.V + (long long)b * p.bsv + (long long)ki * p.ldv + h * D;
    const float* Qb = p.Q + (long long)b * p.bsq + h * D;
    const float* dOb = p.dO + (long long)b * p.bsdo + h * D;
    const float* st = stats + 2 * (long long)bh * p.Tq;
    const float qscale = p.scale * LOG2E;
    float kf[KS], vf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) { kf[s] = Kr[4 * s + g]; vf[s] = Vr[4 * s + g]; }
    v4f dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = v4f{0.f, 0.f, 0.f, 0.f}; dv[dt] = v4f{0.f, 0.f, 0.f, 0.f}; }
    if (tid < 16) { Q2[QT * LD + tid] = 0.f; O2[QT * LD + tid] = 0.f; }
    const int q_begin = blockIdx.z * slab_len;
    const int q_end = p.Tq < q_begin + slab_len ? p.Tq : q_begin + slab_len;
    for (int q0 = q_begin; q0 < q_end; q0 += QT) {
        __syncthreads();
        stage_rows<D, QT, true, true>(Qb, p.ldq, q0, q_end, qscale, Q1, Q2, tid);
        stage_rows<D, QT, true, true>(dOb, p.lddo, q0, q_end, 1.0f, O1, O2, tid);
        if (tid < QT) {
            const int q = q0 + tid;
            Ls[tid] = q < q_end ? st[2 * q] : INFINITY;          // a padded query: P = 2^(-inf) = 0
            Ds[tid] = q < q_end ? st[2 * q + 1] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            v4f s4 = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(Q1[(qt * 16 + c) * LDK + 4 * s + g], kf[s], s4, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(O1[(qt * 16 + c) * LDK + 4 * s + g], vf[s], dp, 0, 0, 0);
            }
            v4f pr, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = qt * 16 + 4 * g + r;
                pr[r] = fast_exp2(s4[r] - Ls[ql]);
                ds[r] = pr[r] * (dp[r] - Ds[ql]) * LN2;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const int at = (qt * 16 + 4 * g + r) * LD + dt * 16 + c;
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(O2[at], pr[r], dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Q2[at], ds[r], dk[dt], 0, 0, 0);
                }
        }
    }
    if (key < p.Tk) {
        float* o = part + (((long long)blockIdx.z * gridDim.y + bh) * p.Tk + key) * (2 * D);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = dt * 16 + 4 * g;
            if (d < D) { *reinterpret_cast<v4f*>(o + d) = dk[dt]; *reinterpret_cast<v4f*>(o + D + d) = dv[dt]; }
        }
    }
}

// part [slabs][B heads][Tk][dK row | dV row] -> dK, dV, the slabs in ascending order
__global__ void attn32_dkv_reduce_kernel(const float* part, int slabs, long long per_slab, long long n4, int heads, int Tk, int D, float* dK, int lddk,
                                         long long bsdk, float* dV, int lddv, long long bsdv) {
    const int w4 = 2 * D / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        v4f s = *reinterpret_cast<const v4f*>(part + 4 * i);
        for (int k = 1; k < slabs; ++k) s += *reinterpret_cast<const v4f*>(part + (long long)k * per_slab + 4 * i);
        const long long row = i / w4;
        const int d = 4 * (int)(i - row * w4), bh = (int)(row / Tk), key = (int)(row - (long long)bh * Tk), b = bh / heads, h = bh - b * heads;
        if (d < D) *reinterpret_cast<v4f*>(dK + (long long)b * bsdk + (long long)key * lddk + h * D + d) = s;
        else *reinterpret_cast<v4f*>(dV + (long long)b * bsdv + (long long)key * lddv + h * D + (d - D)) = s;
    }
}

inline unsigned grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 * 16 ? 65536 * 16 : g));
}

inline size_t stats_floats(int B, int heads, int Tq) { return ((size_t)2 * B * heads * Tq + 3) / 4 * 4; }

template <int D>
hipError_t launch_attn_bwd_t(const AttnBwdParams& p, hipStream_t s) {
    constexpr int T = D == 160 ? 32 : 64;          // keys per tile of the dQ sweep, queries per tile of the dK / dV sweep
    const size_t lds_dq = (size_t)(2 * T * (D + 2) + T * (D + 4) + 16) * sizeof(float);
    const size_t lds_dkv = (size_t)(2 * T * (D + 2) + 2 * (T * (D + 4) + 16) + 2 * T) * sizeof(float);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn32_dq_kernel<D, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dq);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn32_dkv_kernel<D, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dkv);
    if (e != hipSuccess) return e;
    const int BH = p.B * p.heads;
    float* stats = (float*)p.work;
    float* part = stats + stats_floats(p.B, p.heads, p.Tq);
    int slab_len = 0;
    const int slabs = attn_bwd_slabs(p.Tq, p.Tk, &slab_len);
    const unsigned qblocks = (unsigned)((p.Tq + AB_QB - 1) / AB_QB), kblocks = (unsigned)((p.Tk + AB_QB - 1) / AB_QB);
    if (p.phases & 1) hipLaunchKernelGGL((attn32_stats_kernel<D, 64>), dim3(qblocks, (unsigned)BH), dim3(256), 0, s, p, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.phases & 2) hipLaunchKernelGGL((attn32_dq_kernel<D, T>), dim3(qblocks, (unsigned)BH), dim3(256), lds_dq, s, p, (const float*)stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.phases & 4)
        hipLaunchKernelGGL((attn32_dkv_kernel<D, T>), dim3(kblocks, (unsigned)BH, (unsigned)slabs), dim3(256), lds_dkv, s, p, (const float*)stats, part, slab_len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const long long per_slab = (long long)BH * p.Tk * 2 * D, n4 = per_slab / 4;
    if (p.phases & 8)
        hipLaunchKernelGGL(attn32_dkv_reduce_kernel, dim3(grid_for(n4)), dim3(256), 0, s, (const float*)part, slabs, per_slab, n4, p.heads, p.Tk, D, p.dK, p.lddk,
                           p.bsdk, p.dV, p.lddv, p.bsdv);
    return hipGetLastError();
}

}  // namespace

// The query slabs of the dK / dV sweep: a function of (Tq, Tk) alone.  More than two key tiles (Tk > 128: self-attention) give enough
// blocks: one slab.  Otherwise (cross-attention's 77 keys) one slab per 512 queries, at most 16; the slab length is a multiple of 64.
// When the cap binds, trailing slabs may be empty; they write zero partials.
int attn_bwd_slabs(int Tq, int Tk, int* slab_len) {
    int s = Tk > 2 * AB_QB ? 1 : (Tq + 511) / 512;
    s = s < 1 ? 1 : (s > 16 ? 16 : s);
    if (slab_len) *slab_len = ((Tq + s - 1) / s + 63) / 64 * 64;
    return s;
}

size_t attn_bwd_workspace_bytes(int B, int heads, int Tq, int Tk, int D) {
    if (B <= 0 || heads <= 0 || Tq <= 0 || Tk <= 0 || (D != 40 && D != 80 && D != 160) || (long long)B * heads > 65535 || Tq > (1 << 24) || Tk > (1 << 24))
        return 0;
    return (stats_floats(B, heads, Tq) + (size_t)attn_bwd_slabs(Tq, Tk, nullptr) * B * heads * Tk * 2 * D) * sizeof(float);
}

hipError_t launch_attention_bwd(const AttnBwdParams& p, hipStream_t s) {
    const size_t need = attn_bwd_workspace_bytes(p.B, p.heads, p.Tq, p.Tk, p.D);
    if (need == 0 || !p.work || p.work_bytes < need || p.phases < 1 || p.phases > 15) return hipErrorInvalidValue;
    const void* ptrs[9] = {p.Q, p.K, p.V, p.O, p.dO, p.dQ, p.dK, p.dV, p.work};
    for (const void* q : ptrs) if (!q || ((uintptr_t)q & 15) != 0) return hipErrorInvalidValue;
    const int lds[8] = {p.ldq, p.ldk, p.ldv, p.ldo, p.lddo, p.lddq, p.lddk, p.lddv};
    const long long bss[8] = {p.bsq, p.bsk, p.bsv, p.bso, p.bsdo, p.bsdq, p.bsdk, p.bsdv};
    for (int i = 0; i < 8; ++i)
        if (lds[i] < p.heads * p.D || lds[i] % 4 != 0 || bss[i] <= 0 || bss[i] % 4 != 0) return hipErrorInvalidValue;
    switch (p.D) {
        case 40: return launch_attn_bwd_t<40>(p, s);
        case 80: return launch_attn_bwd_t<80>(p, s);
        case 160: return launch_attn_bwd_t<160>(p, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dm32
