// igemm_pers.hip — plain instantiations of the persistent 256 px x 320 ch implicit-GEMM tile (igemm_pers_tile.h).
// Own translation unit like the other tile kernels (co-compiling large kernels perturbs their register allocation).
#include "igemm_pers_tile.h"

namespace dm {

hipError_t launch_igemm_pers(const IGemmParams& p, hipStream_t s) {
    static std::atomic<uint64_t> attr_seen{0};
    set_lds_once(attr_seen, PERS_LDS, {igemm_pers_kernel<EPI_PLAIN, false, PX_NONE>, igemm_pers_kernel<EPI_GEGLU, false, PX_NONE>,
                                       igemm_pers_kernel<EPI_PLAIN, false, PX_TEMB>, igemm_pers_kernel<EPI_PLAIN, false, PX_RES>});
    pers_kernel_t k = igemm_pers_kernel<EPI_PLAIN, false, PX_NONE>;
    if (p.epi == EPI_GEGLU) k = igemm_pers_kernel<EPI_GEGLU, false, PX_NONE>;
    else if (p.temb) k = igemm_pers_kernel<EPI_PLAIN, false, PX_TEMB>;
    else if (p.res) k = igemm_pers_kernel<EPI_PLAIN, false, PX_RES>;
    return launch_pers(k, PERS_LDS, pers_tiles(p), p, s);
}

#ifdef DM_IGEMM_TIMING
extern "C" int dm_debug_pers_timing(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pers_dbg), sizeof(long long) * 8) == hipSuccess ? 0 : 1;
}
#endif

}  // namespace dm
