// igemm_pers_ws.hip — the persistent 256 x 320 tile with per-sample weights and bias row (igemm_pers_tile.h, template
// parameter WS): `Transformer2DModel.norm` (GroupNorm, no activation) folded into `proj_in` (1x1 convolution) — the GEMM runs
// on the raw residual stream, the normalised tensor is never written or read.  Own translation unit.
#include "igemm_pers_tile.h"

namespace dm {

hipError_t launch_igemm_pers_ws(const IGemmParams& p, hipStream_t s) {
    if (p.mode != IG_DENSE || p.epi != EPI_PLAIN || !p.ln_t || p.w_sample_stride <= 0 || p.rows_per_sample <= 0 ||
        p.rows_per_sample % PERS_TP != 0 || p.M % p.rows_per_sample != 0 || p.Cout % PERS_TC != 0 || p.res || p.temb) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_seen{0};
    set_lds_once(attr_seen, PERS_LDS, {igemm_pers_kernel<EPI_PLAIN, true, PX_NONE, true>});
    return launch_pers(igemm_pers_kernel<EPI_PLAIN, true, PX_NONE, true>, PERS_LDS, pers_tiles(p), p, s);
}

}  // namespace dm
