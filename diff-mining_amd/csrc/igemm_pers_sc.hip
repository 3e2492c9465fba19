// igemm_pers_sc.hip — the persistent 256 x 320 tile with a ResNet block's `conv_shortcut` (1x1 on the block's, possibly
// concatenated, input) folded into its conv2 as extra k steps (igemm_pers_tile.h, template parameter SC).  Own translation unit.
#include "igemm_pers_tile.h"

namespace dm {

hipError_t launch_igemm_pers_sc(const IGemmParams& p, hipStream_t s) {
    if ((p.mode != IG_CONV3 && p.mode != IG_DENSE) || p.epi != EPI_PLAIN || p.ln_s || p.temb || p.X2 || !p.X3 || p.Csc <= 0 || p.Csc % BK ||
        p.C3 % BK || (p.C3 < p.Csc && !p.X4) || p.Cout % PERS_TC != 0 || p.ksplit > 1) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_seen{0};
    set_lds_once(attr_seen, PERS_LDS, {igemm_pers_kernel<EPI_PLAIN, false, PX_NONE, false, true>, igemm_pers_kernel<EPI_PLAIN, false, PX_RES, false, true>});
    return launch_pers(p.res ? igemm_pers_kernel<EPI_PLAIN, false, PX_RES, false, true> : igemm_pers_kernel<EPI_PLAIN, false, PX_NONE, false, true>,
                       PERS_LDS, pers_tiles(p), p, s);
}

}  // namespace dm
