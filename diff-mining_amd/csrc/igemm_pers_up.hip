// igemm_pers_up.hip — `Upsample2D` (F.interpolate nearest, exact 2x) + its 3x3 convolution as FOUR 2x2 convolutions on the
// low-resolution source, one per output parity class, on the persistent 256 x 320 tile (igemm_pers_tile.h, template parameter UP4):
// 4 k taps instead of 9 (the taps of the 3x3 kernel that read the same source pixel are pre-summed), the up-sampled tensor never
// exists.  The layer behind it: diffusers `Upsample2D.forward` inside `UNet2DConditionModel.up_blocks[0..2]`, reached from
// diffmining/typicality/compute.py:100 and dift.py:191.  Own translation unit (the other instantiations do not change by a byte).
#include "igemm_pers_tile.h"

namespace dm {

// Always this kernel, for every batch size (no 128-row partner, no head / tail cut): a sample's bits cannot depend on its batch.
hipError_t launch_igemm_pers_up4(const IGemmParams& p, hipStream_t s) {
    if (p.mode != IG_CONV2_UP4 || p.epi != EPI_PLAIN || p.ln_s || p.temb || p.res || p.X2 || p.X3 || p.ksplit > 1 || p.w_sample_stride ||
        p.Cout % PERS_TC != 0 || p.Cin % BK != 0 || p.C1 != p.Cin || p.OH != p.H || p.OW != p.W || p.H < 1 || p.W < 1 || p.H > 511 || p.W > 511 ||
        p.M < 2 || p.M != (p.M / (p.H * p.W)) * p.H * p.W || p.M / (p.H * p.W) > 8191) return hipErrorInvalidValue;
    // 32-bit element offsets: activations (row * channels + chunk), the four weight matrices, and 4 x tiles in an int
    if ((long long)p.M * p.Cin >= (1LL << 31) || 16LL * p.Cout * p.Cin >= (1LL << 32)) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_seen{0};
    set_lds_once(attr_seen, PERS_LDS, {igemm_pers_kernel<EPI_PLAIN, false, PX_NONE, false, false, true>});
    return launch_pers(igemm_pers_kernel<EPI_PLAIN, false, PX_NONE, false, false, true>, PERS_LDS, 4 * pers_tiles(p), p, s);      // 4 parity classes
}

}  // namespace dm
