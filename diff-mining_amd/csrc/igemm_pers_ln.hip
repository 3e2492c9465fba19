// igemm_pers_ln.hip — LayerNorm-folded instantiations of the persistent 256 x 320 tile (igemm_pers_tile.h).
#include "igemm_pers_tile.h"

namespace dm {

// (the folded-LayerNorm layers never carry a time embedding or a residual: igemm_pers_ok)
hipError_t launch_igemm_pers_ln(const IGemmParams& p, hipStream_t s) {
    static std::atomic<uint64_t> attr_seen{0};
    set_lds_once(attr_seen, PERS_LDS, {igemm_pers_kernel<EPI_PLAIN, true, PX_NONE>, igemm_pers_kernel<EPI_GEGLU, true, PX_NONE>});
    return launch_pers(p.epi == EPI_GEGLU ? igemm_pers_kernel<EPI_GEGLU, true, PX_NONE> : igemm_pers_kernel<EPI_PLAIN, true, PX_NONE>,
                       PERS_LDS, pers_tiles(p), p, s);
}

#ifdef DM_IGEMM_TIMING
extern "C" int dm_debug_pers_ln_timing(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pers_dbg), sizeof(long long) * 8) == hipSuccess ? 0 : 1;
}
#endif

}  // namespace dm
