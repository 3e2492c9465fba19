// attention_common.h — what the attention translation units (attention*.hip) share: vector and LDS-DMA pointer types,
// the small device helpers, the prompt-slot rule, the XCD-aware block order, the constant LDS chunks, the LDS geometry of the
// pipelined kernels and the launchers' prototypes.  Everything here is inlined or internal to the including TU (there is no
// -fgpu-rdc), so sharing the text must not change a kernel's machine code: tools/kernel_isa.py compares the instruction
// streams of two trees.
#pragma once
#include "dm_kernels.h"

#include <type_traits>
#include <utility>

namespace dm {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;     // operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int KT = 64;                // keys per tile
constexpr float RESCALE_THR = 8.0f;   // log2 units
constexpr int NSTG = 3;               // K/V ring depth of the pipelined kernels: K is fetched three, V two tiles ahead of their use

// the constant 16-byte chunk behind an LDS row of the layouts with CC = 1: {1,1,0..} for K (the k columns that take
// -m_hi / -m_lo from Q'), {1,0..} for V (the ones row of V^T); the LDS-DMA fetches them like any other chunk
static __device__ __attribute__((aligned(16))) const unsigned short g_kconst[8] = {0x3C00, 0x3C00, 0, 0, 0, 0, 0, 0};
static __device__ __attribute__((aligned(16))) const unsigned short g_vconst[8] = {0x3C00, 0, 0, 0, 0, 0, 0, 0};

#define PIN(x) asm volatile("" : "+v"(x))

// max through inline asm: __builtin_fmaxf (llvm.maxnum) first canonicalises operands that come out of MFMAs
// or asm (v_max x, x), 2-3 extra VALU per row block and tile; scores are never NaN here
__device__ __forceinline__ float vmax2(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ void swap16(unsigned& a, unsigned& b) {      // a.row1 <-> b.row0, a.row3 <-> b.row2 (rows of 16 lanes)
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
}

// LDS transpose read with an immediate offset: lane i of a 16-lane group receives 4 consecutive keys of column i
template <int OFF>
__device__ __forceinline__ void tr_read(u32x2& out, unsigned base) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(out) : "v"(base), "n"(OFF) : "memory");
}

// compile-time loop: f(std::integral_constant<int, i>) for i in [0, N)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// the K/V batch entry (prompt slot) that sample b attends to
__device__ __forceinline__ int kv_batch(const AttnParams& p, int b) {
    int kvb = p.kv_slot ? p.kv_slot[b] : (p.slot_div > 0 ? b / p.slot_div : b);
    if (p.n_slots > 0) kvb = kvb < 0 ? 0 : (kvb < p.n_slots ? kvb : p.n_slots - 1);      // memory safety: never beyond the registered prompts
    return kvb;
}

// XCD-aware block order: one XCD walks consecutive (sample, head) pairs, so all query blocks of a
// pair (which stream the same K/V) share that XCD's L2.  Returns this block's position in that walk.  It reads
// gridDim.x / blockIdx.x itself: taken as parameters, the compiler orders one s_mul_i32 / s_add_i32 pair differently.
__device__ __forceinline__ int xcd_block_order() {
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, loc = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// LDS geometry of the pipelined self-attention kernels at head_dim D.
// CC = 1: rows carry a constant 16-byte chunk behind the data ({1,1,0..} for K: the k columns that take -m_hi / -m_lo from
// Q'; {1,0..} for V: the ones row of V^T), as attention_pipe.hip does.  CC = 0: bare rows; the running max enters as the
// initial value of the score accumulators and the ones row block of V^T is a register constant (D % 16 == 0).
template <int D, int CC>
struct Geo {
    static constexpr int CH = D / 8;                       // real 16-byte chunks per row
    static constexpr int RS = (CH + CC) * 16;              // LDS row stride (bytes)
    static constexpr int KS = (D + 8 * CC + 31) / 32;      // k steps of S^T = K Q^T
    static constexpr int EF = (D + 1 + 15) / 16;           // 16-row blocks of O^T
    static constexpr int EFV = CC ? EF : D / 16;           // ... of which read from LDS
    static constexpr int S_M = D / 32, LG_M = (D % 32) / 8;   // where k = D, D + 1 live in the Q' fragments
    static constexpr int E_L = D / 16, LG_L = (D % 16) / 4;   // where row D of O^T lives in the accumulators
    static constexpr int TILE = KT * RS;
    static constexpr int PAD = 32;                         // zero bytes behind each tile (fragment reads overrun a row)
    static constexpr int KOFF = 0, VOFF = TILE + PAD;
    static constexpr int STAGE = 2 * (TILE + PAD);
    static constexpr int NP = KT * (CH + CC) / 64;         // 1 KiB LDS-DMA pieces per operand tile
    static constexpr int NPW = (2 * NP + 3) / 4;           // piece slots per wave
    static constexpr int SCRATCH = NSTG * STAGE;           // 1 KiB target of the dummy slots
    static constexpr int LDS = NSTG * STAGE + 1024;
    static_assert(D % 8 == 0 && (KT * (CH + CC)) % 64 == 0 && (CC || D % 16 == 0), "tile must be whole pieces");
    static_assert(16 * 3 + 64 * (KS - 1) + 16 <= RS + PAD && 32 * (EFV - 1) + 8 * 3 + 8 <= RS + PAD, "fragment overrun must stay inside the pad");
};
// head_dim 40 (attention_pipe / _pp / _qk32 / _qk64.hip): 96-byte rows of 5 real chunks + 1 constant chunk, 6144-byte tiles,
// 12352-byte stages, 2 k steps of the 16x16x32 score MFMA, 3 row blocks of O^T
using Geo40 = Geo<40, 1>;

// ---- the launchers behind launch_attention (attention.hip routes; each lives in the file named) ----
hipError_t launch_attention_pipe(const AttnParams& p, hipStream_t s);    // attention_pipe.hip
bool attention_pipe_supports(const AttnParams& p);
hipError_t launch_attention_pipe80(const AttnParams& p, hipStream_t s);  // attention_pipe80.hip
bool attention_pipe80_supports(const AttnParams& p);
hipError_t launch_attention_cross(const AttnParams& p, hipStream_t s);   // attention_cross.hip
bool attention_cross_supports(const AttnParams& p);
hipError_t launch_attention_d160(const AttnParams& p, hipStream_t s);    // attention_d160.hip (r06: head_dim 160, eight waves per block)
bool attention_d160_supports(const AttnParams& p);
hipError_t launch_attention_d160_cross(const AttnParams& p, hipStream_t s);   // the 77-key cross-attention at head_dim 160 (one pass)
bool attention_d160_cross_supports(const AttnParams& p);
hipError_t launch_attention_qk32(const AttnParams& p, hipStream_t s);    // attention_qk32.hip (r06: scores on 32x32x16 MFMAs)
bool attention_qk32_supports(const AttnParams& p);
hipError_t launch_attention_qk64(const AttnParams& p, hipStream_t s);    // attention_qk64.hip (two 32-query sets per wave, bit-identical to qk32)
bool attention_qk64_supports(const AttnParams& p);
hipError_t launch_attention_pp(const AttnParams& p, int variant, hipStream_t s);   // attention_pp.hip
bool attention_pp_supports(const AttnParams& p);

}  // namespace dm
