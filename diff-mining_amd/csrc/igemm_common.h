// igemm_common.h — what the 128-row tile (igemm_tile.h) and the persistent 256-row tiles (igemm_pers_tile.h) both use, defined
// once: vector types, the k step, erf-GELU, the XCD block ranges, the in-kernel LayerNorm statistics and the nearest-upsample
// source index.  The two tile geometries give bit-identical results because these are the same code, not copies of it.
#pragma once
#include "dm_kernels.h"

namespace dm {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2_ __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 ln_half2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BK = 64;           // k per step (one tap, 64 input channels)

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// erf-GELU  x * Phi(x) = max(x, 0) - |x| * T(|x|),  T(a) = 0.5 * (1 - erf(a / sqrt 2)) by Abramowitz-Stegun 7.1.26
// (|erf error| < 1.5e-7; measured over all 63 488 finite fp16 inputs: max |error| 3.3e-7, i.e. far below the fp16
// rounding of the result): 1 rcp + 1 exp2 + 12 plain VALU instead of libm erff (~40 instructions), which dominated the
// GEGLU epilogue (40 calls per lane per 256 x 320 tile).  The tail T is formed directly (no 1 - 1 cancellation for
// negative x), the 0.5 lives in the coefficients and 1 / sqrt 2 in the constants, and the max / |x| form needs no
// compare-and-select (r02: -2..3 % on the GEGLU launches against the x * (x < 0 ? T : 1 - T) form; a fused-multiply-add
// form and an inline-asm max measured the same).
__device__ __forceinline__ float gelu_erf(float x) {
    const float ax = __builtin_fabsf(x);
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f * 0.70710678118654752440f, ax, 1.0f));
    float poly = __builtin_fmaf(t, 0.5f * 1.061405429f, 0.5f * -1.453152027f);
    poly = __builtin_fmaf(t, poly, 0.5f * 1.421413741f);
    poly = __builtin_fmaf(t, poly, 0.5f * -0.284496736f);
    poly = __builtin_fmaf(t, poly, 0.5f * 0.254829592f);
    poly *= t;
    const float e = __builtin_amdgcn_exp2f((x * x) * -0.72134752044448170368f);        // exp(-x^2 / 2)
    return __builtin_fmaxf(x, 0.f) - ax * (poly * e);
}

// Blocks are dealt to the 8 XCDs round robin (XCD = block % 8), and an XCD's blocks share an L2: XCD x owns a contiguous range
// of the n items (tiles), n / 8 of them and one more on the first n % 8 XCDs.  First item of the range of `block`'s XCD.
__device__ __forceinline__ int xcd_range_start(int block, int n) {
    const int q = n >> 3, r = n & 7, xcd = block & 7;
    return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}

// Folded LayerNorm without a statistics kernel (IGemmParams::ln_stats == nullptr): lane pair (2r, 2r + 1) owns row r of the tile
// and lane-half hf adds logical chunks 4 hf .. 4 hf + 3 of every 64-channel k slab, ascending, to (sum, sum of squares) in fp32.
// The order depends on the row only, never on the tile geometry or the batch.  One step: the eight channels of one chunk.
__device__ __forceinline__ void ln_stats_acc(half8 xv, float& s1, float& s2) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {          // v_dot2_f32_f16: two exact fp16 products + the fp32 accumulator per instruction
        const ln_half2 v2 = ln_half2{xv[k], xv[k + 1]};
        s1 = __builtin_amdgcn_fdot2(v2, ln_half2{(_Float16)1.0f, (_Float16)1.0f}, s1, false);
        s2 = __builtin_amdgcn_fdot2(v2, v2, s2, false);
    }
}
// After the k loop: the pair's sums -> (mean, rstd) of row m (clamped to M - 1); `on` = this lane owns a row of the tile at all.
__device__ __forceinline__ float2 ln_stats_finish(const IGemmParams& p, float s1, float s2, int m, int hf, bool on) {
    const float t1 = s1 + __shfl_xor(s1, 1), t2 = s2 + __shfl_xor(s2, 1);
    const float mean = t1 / (float)p.Cin;
    float var = t2 / (float)p.Cin - mean * mean;
    var = var > 0.f ? var : 0.f;
    if (on && mean * mean > LN_REDO_RATIO2 * var) {      // cancellation: exact second pass over this row (dm_kernels.h)
        m = m < p.M ? m : p.M - 1;
        const int half_c = p.Cin >> 1;
        const f16* xr = p.X + (size_t)m * p.Cin + hf * half_c;
        float q = 0.f;
        for (int c = 0; c < half_c; c += 8) {
            const half8 v = *reinterpret_cast<const half8*>(xr + c);
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = (float)v[k] - mean; q = __builtin_fmaf(d, d, q); }
        }
        var = (q + __shfl_xor(q, 1)) / (float)p.Cin;
    }
    return float2{mean, rsqrtf(var + p.ln_eps)};
}

// F.interpolate(mode="nearest") to an arbitrary size: source index of up-sampled coordinate u (scale = in / out, n = in)
__device__ __forceinline__ int nearest_src(int u, float scale, int n) {
    const int i = (int)floorf((float)u * scale);
    return i < n - 1 ? i : n - 1;
}

}  // namespace
}  // namespace dm
