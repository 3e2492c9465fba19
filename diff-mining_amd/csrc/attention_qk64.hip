// attention_qk64.hip — head_dim-40 self-attention, two 32-query sets per wave sharing each tile's K / V^T fragments.
// Reached from `unet(...)` like attention_qk32.hip (BasicTransformerBlock.attn1 at the 64x64 level), selected by attn_pipe = 6.
//
// attention_qk32.hip issues, per 32 queries and 64-key tile, six ds_read_b128 K fragment reads, twelve ds_read_b64_tr_b16 V^T
// reads and (per 128-query block) twelve LDS-DMA pieces.  None of them depends on the query: the K and V^T fragments are the A
// operands of the score / PV MFMAs, the query side is their B operand (qf, P in pk).  Here a wave holds two 32-query sets
// (queries q0 + 32 j + (lane & 31), j = 0, 1) and issues those reads once for both, and a 4-wave block of 256 queries issues the
// same twelve pieces per tile for twice the scores.  Everything per query is qk32's, per set: qf, the score tile, pk, O^T, m_run
// and the lazy-rescale ballot (one per set, so every rescale decision is the one a qk32 wave makes for the same 32 queries).
// The score chain (3 k steps, -m columns folded in), every exp2 input and the PV accumulation order are unchanged, so the
// output is bit-identical to attn_qk32_kernel.
//
// The LDS layout, the LDS-DMA pieces and the three-stage ring are qk32's (see the header of attention_qk32.hip).  The scores are
// not ping-ponged (two sets x two tiles would not fit 256 registers): the other set's tile is the independent work.  One tile t:
//   P1  exp / pack / swaps of set 0's S(t)                    || K(t+1) and V(t)^T fragment reads
//   P2  S(t+1) MFMAs of set 0                                 || exp / pack of set 1's S(t), key block 0 and part of 1
//   P3  PV(t) MFMAs of set 0                                  || the rest of set 1's exps, its swaps, set 0's lane-partial max
//   P4  S(t+1) MFMAs of set 1                                 || the wave's LDS-DMA pieces, set 0's ballot / rescale
//   P5  PV(t) MFMAs of set 1                                  || set 1's lane-partial max
// The lane-partial max runs as four independent v_max3 chains (key block x half), two steps per asm statement: fmax is exact and
// order-free, and the chains no longer stall the issue on s_nops.
#include "attention_common.h"

namespace dm {

namespace {

constexpr int D = 40;
constexpr int NT = 256;               // threads per block
constexpr int QS = 32;                // queries per set
constexpr int NS = 2;                 // sets per wave
constexpr int QW = NS * QS;           // queries per wave
constexpr int RS = Geo40::RS, TILE = Geo40::TILE, KOFF = Geo40::KOFF, VOFF = Geo40::VOFF, STAGE = Geo40::STAGE;   // 96, 6144, 0, 6176, 12352
constexpr int EF = Geo40::EF;         // 16-row blocks of O^T (40 rows + the ones row)
static_assert(NSTG * STAGE == 3 * Geo40::STAGE, "the launcher asks for attn_pipe_kernel's LDS size: its stage, its ring depth");

// two independent chain steps in one asm statement: the hazard recognizer cannot see into an asm block and pads every boundary
// between two of them with an s_nop, which independent v_max ops do not need
__device__ __forceinline__ void vmax2x2(float& x, float& y, float a0, float a1, float b0, float b1) {
    asm("v_max_f32 %0, %2, %3\n\tv_max_f32 %1, %4, %5" : "=&v"(x), "=&v"(y) : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
}
__device__ __forceinline__ void vmax3x2(float& x, float& y, float a0, float a1, float b0, float b1) {
    asm("v_max3_f32 %0, %0, %2, %3\n\tv_max3_f32 %1, %1, %4, %5" : "+v"(x), "+v"(y) : "v"(a0), "v"(a1), "v"(b0), "v"(b1));
}

__global__ __launch_bounds__(NT, 2)
void attn_qk64_kernel(AttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15;
    const int lg = lane >> 4;
    const int l31 = lane & 31;
    const int hh5 = lane >> 5;
    const int nqb = (p.Tq + 4 * QW - 1) / (4 * QW);
    const int v = xcd_block_order();
    const int qblk = v % nqb;
    const int bh = v / nqb;
    const int h = bh % p.heads;
    const int b = bh / p.heads;
    const int q0 = qblk * (4 * QW) + wid * QW;       // set j: queries q0 + 32 j + l31
    const int kvb = kv_batch(p, b);

    const f16* Qb = p.Q + (size_t)b * p.bsq + h * D;
    const f16* Kb = p.K + (size_t)kvb * p.bsk + h * D;
    const f16* Vb = p.V + (size_t)kvb * p.bsv + h * D;
    f16* Ob = p.O + (size_t)b * p.bso + h * D;

    // ---- Q' = fp16(sc * q) per set, qk32's B operand layout (head_dim 40 / 41 of k step 2 carry -m_hi / -m_lo) ----
    const float sc = p.scale * 1.44269504088896340736f;
    half8 qf[NS][3];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        int q = q0 + QS * j + l31;
        q = q < p.Tq ? q : p.Tq - 1;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int d = 16 * s + 8 * hh5;
            if (d < D) qf[j][s] = *reinterpret_cast<const half8*>(Qb + (size_t)q * p.ldq + d);
            else qf[j][s] = half8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 8; ++k) qf[j][s][k] = (f16)((float)qf[j][s][k] * sc);
        }
    }

    // ---- LDS-DMA: qk32's pieces (6 K + 6 V of 1 KiB per tile, 3 per wave; K chunk pairs swapped on key bit 3, V rows with key
    //      bits 2 and 4 exchanged, logical chunk 5 from a global constant) ----
    const f16* gsrc[3];
    int ginc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = wid + 4 * i;
        const bool isv = j >= 6;
        const int jj = isv ? j - 6 : j;
        const int idx = jj * 64 + lane;
        const int row = idx / 6, pch = idx - row * 6;
        const int key = isv ? ((row & ~20) | ((row & 4) << 2) | ((row & 16) >> 2)) : row;
        const int ch = isv ? pch : (pch ^ ((row >> 3) & 1));
        const int ld = isv ? p.ldv : p.ldk;
        if (ch < 5) { gsrc[i] = (isv ? Vb : Kb) + (size_t)key * ld + ch * 8; ginc[i] = KT * ld; }
        else { gsrc[i] = reinterpret_cast<const f16*>(isv ? g_vconst : g_kconst); ginc[i] = 0; }
    }
    auto piece_is_v = [&](int i) __attribute__((always_inline)) { return wid + 4 * i >= 6; };
    auto piece = [&](int i, int kst, int vst) __attribute__((always_inline)) {
        const int j = wid + 4 * i;
        char* dst = smem + ((j >= 6) ? vst * STAGE + VOFF + (j - 6) * 1024 : kst * STAGE + KOFF + j * 1024);
        __builtin_amdgcn_global_load_lds((gptr_t)gsrc[i], (lptr_t)dst, 16, 0, 0);
        gsrc[i] += ginc[i];
    };

    const char* kbase = smem + l31 * RS + 16 * (hh5 ^ ((lane >> 3) & 1));
    const unsigned vbase = (unsigned)(size_t)(smem + (4 * (lg & 1) + 16 * (lg >> 1) + (l15 >> 2)) * RS + 8 * (l15 & 3));

    floatx4 oacc[NS][EF][2];
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int e = 0; e < EF; ++e)
#pragma unroll
            for (int jq = 0; jq < 2; ++jq) oacc[j][e][jq] = floatx4{0, 0, 0, 0};
    float m_run[NS] = {0.f, 0.f};      // running max (log2 units) of query l31 of each set

    floatx16 S[NS][2];                 // raw score tile sc*(q.k) - m_run of key blocks mb = 0 / 1, per set
    unsigned pk[NS][2][8];             // P as packed fp16 pairs; after the swaps pk[j][mb][4 jq .. 4 jq + 3] = PV B operand

    // qk32's rescale, for set j: rescale O, refresh the -m columns of Q', fix the already computed score tile up in place
    auto rescale = [&](const int j, const float mxl, bool first) __attribute__((always_inline)) {
        float mown = mxl;
        PIN(mown);
        const float mx = __builtin_fmaxf(mown, __shfl_xor(mown, 32));
        const float delta = first ? mx : __builtin_fmaxf(mx, 0.f);
        const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-delta);
        m_run[j] += delta;
        const float alpha_x = __shfl_xor(alpha, 16);
        const float a0 = (lg & 1) ? alpha_x : alpha, a1 = (lg & 1) ? alpha : alpha_x;
#pragma unroll
        for (int e = 0; e < EF; ++e) { oacc[j][e][0] *= a0; oacc[j][e][1] *= a1; }
        if (hh5 == 1) {
            const f16 mh = (f16)m_run[j];
            const f16 ml = (f16)(m_run[j] - (float)mh);
            qf[j][2][0] = -mh; qf[j][2][1] = -ml;
        }
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) S[j][mb][r] -= delta;
    };
    // exp slice i (0..15) of set j: scores 2 p, 2 p + 1 of key block mb = i / 8 (p = i % 8) -> one packed fp16 pair
    auto exp_slice = [&](const int j, int i) __attribute__((always_inline)) {
        const int mb = i >> 3, pp = i & 7;
        const half2v hv = half2v{(f16)__builtin_amdgcn_exp2f(S[j][mb][2 * pp]), (f16)__builtin_amdgcn_exp2f(S[j][mb][2 * pp + 1])};
        unsigned u;
        __builtin_memcpy(&u, &hv, 4);
        PIN(u);
        pk[j][mb][pp] = u;
    };
    // score MFMA m (0..5) of set j: k step m / 2, key block m % 2 (qk32's order)
    auto score_mfma = [&](const int j, const half8 (&kf)[3][2], int m) __attribute__((always_inline)) {
        const int s = m >> 1, mb = m & 1;
        S[j][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s][mb], qf[j][s], S[j][mb], 0, 0, 0);
        PIN(S[j][mb]);
    };
    // PV MFMA m (0..11) of set j: qk32's snake over (e, jq), k step m / 6
    auto pv_mfma = [&](const int j, const u32x2 (&vraw)[2][EF][2], int m) __attribute__((always_inline)) {
        const int ss = m / 6, e = (m % 6) >> 1, jq = (m & 1) ^ (DM_MFMA_SNAKE ? (e & 1) : 0);
        half8 va, pbv;
        __builtin_memcpy(&va, &vraw[ss][e][0], 8);
        __builtin_memcpy(reinterpret_cast<char*>(&va) + 8, &vraw[ss][e][1], 8);
        __builtin_memcpy(&pbv, &pk[j][ss][4 * jq], 16);
        oacc[j][e][jq] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pbv, oacc[j][e][jq], 0, 0, 0);
        PIN(oacc[j][e][jq]);
    };
    // lane-partial max step o (0..7) of set j: four independent chains (key block mb, half c of its 16 scores), each 8 long
    auto max_step = [&](const int j, float (&mx)[4], int o) __attribute__((always_inline)) {
        const int c = o & 1, r = 8 * c + 2 * (o >> 1);
        if (o < 2) vmax2x2(mx[c], mx[2 + c], S[j][0][r], S[j][0][r + 1], S[j][1][r], S[j][1][r + 1]);
        else vmax3x2(mx[c], mx[2 + c], S[j][0][r], S[j][0][r + 1], S[j][1][r], S[j][1][r + 1]);
    };

    const int ntiles = p.Tk / KT;       // even, >= 4 (dispatch condition)

    // ---- prologue: K(0) -> S(0) of both sets, first running max ----
#pragma unroll
    for (int i = 0; i < 3; ++i) if (!piece_is_v(i)) piece(i, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) piece(i, 1, 0);              // K(1) -> stage 1, V(0) -> stage 0
#pragma unroll
    for (int i = 0; i < 3; ++i) piece(i, 2, 1);              // K(2) -> stage 2, V(1) -> stage 1
    {
        half8 kf[3][2];
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) kf[s][mb] = *reinterpret_cast<const half8*>(kbase + KOFF + 32 * s + mb * 32 * RS);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[j][mb][r] = 0.f;
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) S[j][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[s][mb], qf[j][s], S[j][mb], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            float m = S[j][0][0];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) m = __builtin_fmaxf(m, S[j][mb][r]);
            rescale(j, m, true);
        }
    }

    // One iteration t: S[j] holds tile t of set j on entry, tile t+1 on exit.  Ring as in qk32, s0 = t % 3:
    //   K(t+1) sits in stage (t+1)%3, V(t) in stage s0; DMA: K(t+3) -> stage s0, V(t+2) -> stage (t+2)%3.
    int s0 = 0;
    auto iteration = [&](const bool next, const bool dma_k, const bool dma_v, const bool wait3) __attribute__((always_inline)) {
        constexpr int KB = KOFF, VB = VOFF;
        const int s1 = (s0 == NSTG - 1) ? 0 : s0 + 1;
        const int s2 = (s1 == NSTG - 1) ? 0 : s1 + 1;
        const char* kcur = kbase + s1 * STAGE;                // K(t+1)
        const unsigned vcur = vbase + (unsigned)(s0 * STAGE); // V(t)
        if (wait3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");               // raw: __syncthreads() would drain the counted wait (vmcnt(0) fence)
        // ---------------- P1: exp / pack / swaps of set 0 || K(t+1), V(t)^T fragment reads ----------------
        half8 kf[3][2];
        u32x2 vraw[2][EF][2];
        if (next) {
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) kf[s][mb] = *reinterpret_cast<const half8*>(kcur + KB + 32 * s + mb * 32 * RS);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            exp_slice(0, i);
            // V(t)^T fragments: offset = 32 e + (32 ss + 8 hh) RS
            if (i == 2) { tr_read<VB + 0 + 0 * 8 * RS>(vraw[0][0][0], vcur); tr_read<VB + 0 + 1 * 8 * RS>(vraw[0][0][1], vcur); }
            if (i == 4) { tr_read<VB + 32 + 0 * 8 * RS>(vraw[0][1][0], vcur); tr_read<VB + 32 + 1 * 8 * RS>(vraw[0][1][1], vcur); }
            if (i == 6) { tr_read<VB + 64 + 0 * 8 * RS>(vraw[0][2][0], vcur); tr_read<VB + 64 + 1 * 8 * RS>(vraw[0][2][1], vcur); }
            if (i == 8) { tr_read<VB + 0 + 4 * 8 * RS>(vraw[1][0][0], vcur); tr_read<VB + 0 + 5 * 8 * RS>(vraw[1][0][1], vcur); }
            if (i == 10) { tr_read<VB + 32 + 4 * 8 * RS>(vraw[1][1][0], vcur); tr_read<VB + 32 + 5 * 8 * RS>(vraw[1][1][1], vcur); }
            if (i == 12) { tr_read<VB + 64 + 4 * 8 * RS>(vraw[1][2][0], vcur); tr_read<VB + 64 + 5 * 8 * RS>(vraw[1][2][1], vcur); }
            if (i == 9) { swap16(pk[0][0][0], pk[0][0][4]); swap16(pk[0][0][1], pk[0][0][5]); }
            if (i == 11) { swap16(pk[0][0][2], pk[0][0][6]); swap16(pk[0][0][3], pk[0][0][7]); }
            if (i & 1) __builtin_amdgcn_sched_barrier(0);      // regions of two slices: a pack need not follow its exps directly
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) swap16(pk[0][1][i], pk[0][1][4 + i]);
        __builtin_amdgcn_sched_barrier(0);
        // ---------------- P2: S(t+1) MFMAs of set 0 || exps of set 1, slices 0..11 ----------------
        if (next) asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");    // the six K fragments (the twelve V^T reads may fly on)
        __builtin_amdgcn_sched_barrier(0);
        if (next) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[0][mb][r] = 0.f;
        }
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            if (next) score_mfma(0, kf, m);
            exp_slice(1, 2 * m);
            exp_slice(1, 2 * m + 1);
            if (m == 4) { swap16(pk[1][0][0], pk[1][0][4]); swap16(pk[1][0][1], pk[1][0][5]); }
            if (m == 5) { swap16(pk[1][0][2], pk[1][0][6]); swap16(pk[1][0][3], pk[1][0][7]); }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---------------- P3: PV(t) of set 0 || exps 12..15 and swaps of set 1, lane-partial max of set 0's S(t+1) ----------------
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        float mx0[4], mx1[4];
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            pv_mfma(0, vraw, m);
            if (m < 2) { exp_slice(1, 12 + 2 * m); exp_slice(1, 13 + 2 * m); }
            if (m >= 2 && m < 6) swap16(pk[1][1][m - 2], pk[1][1][m + 2]);
            if (next && m >= 4) max_step(0, mx0, m - 4);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---------------- P4: S(t+1) MFMAs of set 1 || LDS-DMA issue, set 0's ballot ----------------
        if (next) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[1][mb][r] = 0.f;
        }
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            if (next) score_mfma(1, kf, m);
            if (m == 0 || m == 2 || m == 4) {
                const int i = m >> 1;
                if (piece_is_v(i) ? dma_v : dma_k) piece(i, s0, s2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (next) {
            const float mx = vmax2(vmax3(mx0[0], mx0[1], mx0[2]), mx0[3]);
            if (__builtin_amdgcn_ballot_w64(mx > RESCALE_THR) != 0ull) rescale(0, mx, false);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---------------- P5: PV(t) of set 1 || lane-partial max of set 1's S(t+1) ----------------
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            pv_mfma(1, vraw, m);
            if (next && m >= 4) max_step(1, mx1, m - 4);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (next) {
            const float mx = vmax2(vmax3(mx1[0], mx1[1], mx1[2]), mx1[3]);
            if (__builtin_amdgcn_ballot_w64(mx > RESCALE_THR) != 0ull) rescale(1, mx, false);
        }
        s0 = s1;
    };

    // iterations 0 .. nt-4 issue a full set of pieces; nt-3 only V(nt-1); nt-2, nt-1 nothing
    for (int t = 0; t < ntiles - 3; ++t) iteration(true, true, true, true);
    iteration(true, false, true, true);        // t = nt-3
    iteration(true, false, false, false);      // t = nt-2
    iteration(false, false, false, false);     // t = nt-1

#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int jq = 0; jq < 2; ++jq) {
            // row d = 40 of O^T (the ones row of V^T) is the softmax denominator: fragment 2, lane group 2, register 0
            const float l = __shfl(oacc[j][2][jq][0], (2 << 4) | l15);
            const float inv = 1.0f / l;
            const int q = q0 + QS * j + 16 * jq + l15;
            if (q >= p.Tq) continue;
#pragma unroll
            for (int e = 0; e < EF; ++e) {
                const int d = 16 * e + 4 * lg;
                if (d < D) {
                    const half4 o = half4{(f16)(oacc[j][e][jq][0] * inv), (f16)(oacc[j][e][jq][1] * inv),
                                          (f16)(oacc[j][e][jq][2] * inv), (f16)(oacc[j][e][jq][3] * inv)};
                    *reinterpret_cast<half4*>(Ob + (size_t)q * p.ldo + d) = o;
                }
            }
        }
}

}  // namespace

bool attention_qk64_supports(const AttnParams& p) {
    return p.D == 40 && p.Tk >= 256 && (p.Tk % 128) == 0 && p.q_mod == 0;
}

hipError_t launch_attention_qk64(const AttnParams& p, hipStream_t s) {
    if (!attention_qk64_supports(p)) return hipErrorInvalidValue;
    constexpr int QBLK = 4 * QW;
    dim3 grid(((p.Tq + QBLK - 1) / QBLK) * p.heads * p.B), block(NT);
    const size_t lds = NSTG * (size_t)STAGE;
    launch_timed(attn_qk64_kernel, grid, block, lds, s, p);
    return hipGetLastError();
}

}  // namespace dm
