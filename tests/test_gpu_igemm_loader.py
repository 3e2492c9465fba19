"""The LDS-DMA source addresses of the persistent 256 x 320 implicit-GEMM tile (igemm_pers_tile.h: load_piece / set_src).

Its k step forms a weight piece's address from a wave-uniform base and a constant lane offset, and an activation piece's from a
64-bit lane address that is set at a tap / source change and advanced by one add per step — for halo lanes and rows beyond M too,
which walk the zero page at the pace of the lanes that read the tensor.  What can go wrong is an address: a lane that advanced off
its row, a source switch that kept the old base, a zero page shorter than a row.  So every case runs through the operator entry
inside NaN-filled guard bands (tests/test_gpu_guards.py: run3 — untouched guards, equal bits under both fills) on the smallest
shape that takes the path, and its output is compared `torch.equal` with the 128-row tile (igemm_tile.h, whose loader is the
untouched one) where that partner exists, else with fp32 F.conv2d at the tolerance tests/test_gpu_ops.py uses for the layer.
`igemm_big` = 1 puts every shape the persistent tile accepts on it, 0 none."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import gpu_util as U  # noqa: E402
from tests.test_gpu_guards import F16, F32, _lib, _options, igemm_case, run3  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _both_tiles(what, N, H, W, C1, C2, Cout, mode, OH=None, OW=None, variants=("plain", "res"), opts=None):
    """the case on the persistent tile between guards and against fp32 (igemm_case), then the same device operands on the 128-row tile"""
    opts = dict(opts or {})
    got = igemm_case(what, N, H, W, C1, C2, Cout, mode=mode, OH=OH, OW=OW, variants=variants, tile=1, opts=dict(opts, igemm_big=1))
    for var, (dv, y) in got.items():
        with _options(**dict(opts, igemm_big=0)):
            y128 = U.op_igemm(dv["x"], dv["w"], dv["bias"], X2=dv.get("x2"), temb=dv.get("temb"), res=dv.get("res"), mode=mode, OH=OH, OW=OW)
        assert torch.equal(y, y128), f"{what} [{var}]: {(y != y128).sum().item()} elements differ from the 128-row tile"
    return got


@pytest.mark.parametrize("N,H,W", [(2, 16, 16), (3, 12, 10)])
def test_conv3x3_two_sources(N, H, W):
    """64 + 64 channels: the source switches in the middle of every tap.  2 x 16 x 16: a tile is a whole image, all four borders are
    halo.  3 x 12 x 10: M = 360, a tile straddles samples and the last one is ragged — rows beyond M ride the zero page for all 18 steps."""
    _both_tiles(f"conv3x3 64+64 {N}x{H}x{W}", N, H, W, 64, 64, 320, 1)


def test_conv3x3_stride2():
    _both_tiles("conv3x3 stride 2", 5, 16, 16, 128, 0, 320, 2, OH=8, OW=8)            # M = 320: ragged


@pytest.mark.parametrize("H,OH", [(5, 10), (7, 13)])
def test_conv3x3_nearest_upsampled(H, OH):
    """exact 2x, and F.interpolate(size=...) onto an odd size; one 64-channel slab: a new lane address at every k step"""
    _both_tiles(f"conv3x3 up {H}->{OH}", 3, H, H, 64, 0, 320, 3, OH=OH, OW=OH, variants=("plain",))


def test_dense_two_channel_tiles_ragged_rows():
    _both_tiles("dense 300 x 320 -> 640", 1, 1, 300, 320, 0, 640, 0)


def test_dense_longest_source_row():
    """K = the longest single-source row the persistent tile takes (launch_pers checks the launch against the zero page's size with the
    same constant): the 56 rows beyond M = 200 walk the zero page to its last byte.  One more 64-channel slab no longer fits: 128-row tile."""
    lib = _lib()
    K = lib.dm_op_igemm_pers_max_source_channels()
    assert K % 64 == 0 and K >= 5120                # ff.net.2 at 1280 channels reads 5120
    with _options(igemm_big=1):
        assert lib.dm_op_igemm_tile(200, K, 320, 0) == 1 and lib.dm_op_igemm_tile(200, K + 64, 320, 0) == 0
    _both_tiles(f"dense 200 x {K} -> 320", 1, 1, 200, K, 0, 320, 0, variants=("plain",))


def test_folded_upsampler():
    """UP4 at 8 x 8 -> 16 x 16: four 2x2 convolutions on the source grid, M = 192 rows per parity class (ragged).  No bit-identical
    partner (the summed taps are rounded once more): reference and tolerances of test_upconv_folded."""
    lib = _lib()
    N, H, W, Cin, Cout = 3, 8, 8, 128, 320
    x = U.f16_randn(N, H, W, Cin, seed=71)
    w, b = U.f16_randn(Cout, Cin, 3, 3, seed=72, scale=(9 * Cin) ** -0.5), U.f16_randn(Cout, seed=73, scale=0.1)
    w4 = U.fold_upconv_torch(w)

    def launch(v):
        assert lib.dm_op_upconv_folded(U.stream(), U.ptr(v["x"]), U.ptr(v["w4"]), U.ptr(v["bias"]), U.ptr(v["y"]), N, H, W, Cin, Cout) == 0
    y = run3("folded up-sampler 8x8", {"x": x, "w4": w4, "bias": b}, {"y": ((N, 2 * H, 2 * W, Cout), F16)}, launch)["y"]
    xs = U.to_nchw(x.float())
    ref = F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), w.float(), b.float(), padding=1)
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "folded up-sampler vs interpolate + conv2d")
    own = torch.empty_like(ref)
    for py in (0, 1):
        for px in (0, 1):
            k = w4[py * 2 + px].float().view(Cout, 2, 2, Cin).permute(0, 3, 1, 2)
            own[:, :, py::2, px::2] = F.conv2d(F.pad(xs, (1 - px, px, 1 - py, py)), k, b.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), own, "folded up-sampler vs its own arithmetic in fp32", **U.TOL_UPFOLD_OWN)


def test_folded_shortcut_third_and_fourth_source():
    """SC: after the nine taps on X (64 channels) the k loop runs 3 steps of the 1x1 shortcut on cat([X3 (64), X4 (128)])"""
    lib = _lib()
    N, H, W, Cin, C3, C4, Cout = 2, 16, 16, 64, 64, 128, 320
    h, x3, x4 = U.f16_randn(N, H, W, Cin, seed=1), U.f16_randn(N, H, W, C3, seed=2), U.f16_randn(N, H, W, C4, seed=3, scale=0.5)
    w2 = U.f16_randn(Cout, Cin, 3, 3, seed=6, scale=(9 * Cin) ** -0.5)
    ws = U.f16_randn(Cout, C3 + C4, seed=7, scale=(C3 + C4) ** -0.5)
    b2, bs = U.f16_randn(Cout, seed=8, scale=0.1), U.f16_randn(Cout, seed=9, scale=0.1)
    inputs = {"h": h, "x3": x3, "x4": x4, "w": torch.cat([U.pack_conv3(w2), ws], dim=1).contiguous(), "bias": (b2.float() + bs.float()).half()}

    def launch(v):
        assert lib.dm_op_igemm_shortcut(U.stream(), U.ptr(v["h"]), U.ptr(v["x3"]), U.ptr(v["x4"]), U.ptr(v["w"]), U.ptr(v["bias"]), None, U.ptr(v["y"]),
                                        N, H, W, Cin, C3, C4, Cout, 1) == 0
    with _options(igemm_big=1):
        assert lib.dm_op_igemm_tile(N * H * W, Cin, Cout, 1) == 1
        y = run3("conv2 + folded shortcut, persistent", inputs, {"y": ((N, H, W, Cout), F16)}, launch)["y"]
    with _options(igemm_big=0):
        dv = {k: t.to(U.dev()) for k, t in inputs.items()}
        dv["y"] = torch.full_like(y, float("nan"))
        launch(dv)
        torch.cuda.synchronize()
    assert torch.equal(y, dv["y"]), "differs from the 128-row tile"
    ref = F.conv2d(U.to_nchw(h.float()), w2.float(), b2.float(), padding=1) + \
        F.conv2d(U.to_nchw(torch.cat([x3, x4], 3).float()), ws.float()[:, :, None, None], bs.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "conv2 + folded shortcut")


def test_per_sample_weights():
    """WS: GroupNorm folded into a 1x1 convolution, 2 samples of 256 rows: the weight base moves by a sample's stride between the tiles"""
    lib = _lib()
    N, H, W, C, Cout, G = 2, 16, 16, 320, 320, 32
    g = torch.Generator().manual_seed(C + N)
    x = (torch.randn(N, C, H, W, generator=g) * (1.0 + torch.rand(N, C, 1, 1, generator=g)) + torch.randn(N, C, 1, 1, generator=g)).half()
    w, b = U.f16_randn(Cout, C, seed=2, scale=C ** -0.5), U.f16_randn(Cout, seed=3, scale=0.1)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).float(), (0.1 * torch.randn(C, generator=g)).float()
    inputs = {"x": U.to_nhwc(x), "gamma": gamma, "beta": beta, "w": w, "bias": b}

    def launch(v):
        assert lib.dm_op_groupnorm_conv1x1(U.stream(), U.ptr(v["x"]), N, H * W, C, G, 1e-6, U.ptr(v["gamma"]), U.ptr(v["beta"]), U.ptr(v["w"]), U.ptr(v["bias"]),
                                           Cout, U.ptr(v["y"])) == 0
    with _options(igemm_big=1):
        y = run3("GroupNorm folded into conv1x1, persistent", inputs, {"y": ((N, H, W, Cout), F16)}, launch)["y"]
    with _options(igemm_big=0):
        dv = {k: t.to(U.dev()) for k, t in inputs.items()}
        dv["y"] = torch.full_like(y, float("nan"))
        launch(dv)
        torch.cuda.synchronize()
    assert torch.equal(y, dv["y"]), "differs from the 128-row tile"
    ref = F.conv2d(F.group_norm(x.float(), G, gamma, beta, 1e-6), w.float()[:, :, None, None], b.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "GroupNorm folded into conv1x1", **U.TOL_FP16_CHAIN)


def test_splitk_three_tap_aligned_parts():
    """PART: 8 x 8, Cin = 128, on the persistent split-K kernel, which walks whole taps: three parts of three.  172 samples reach it on a
    256-CU device (splitk_on_pers, restated as in test_igemm_splitk of tests/test_gpu_guards.py); the result must have the 128-row split-K
    kernel's bits on the same three parts and match the unsplit kernel.  (FOUR parts of this layer exist on neither kernel: its 18 k steps
    are no multiple of four, and the entry says so before it launches anything — asserted first.)"""
    lib = _lib()
    N, ks = 172, 3
    H = W = 8
    Cin, Cout, M = 128, 320, N * 64
    inputs = {"x": U.f16_randn(N, H, W, Cin, seed=1), "w": U.f16_randn(Cout, 9 * Cin, seed=3, scale=(9 * Cin) ** -0.5),
              "bias": U.f16_randn(Cout, seed=4, scale=0.1), "temb": U.f16_randn(N, Cout, seed=5), "res": U.f16_randn(N, H, W, Cout, seed=6)}

    def launch(v, parts=ks, expect=0):
        rc = lib.dm_op_igemm_splitk(U.stream(), U.ptr(v["x"]), None, U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(v["temb"]), U.ptr(v["res"]), U.ptr(v["y"]),
                                    N, H, W, Cin, 0, Cout, H, W, 1, Cout, parts, U.ptr(v["ws"]))
        assert (rc == 0) == (expect == 0), f"dm_op_igemm_splitk with {parts} parts returned {rc}"
    d = U.dev()
    dv = {k: t.to(d) for k, t in inputs.items()}
    dv["y"], dv["ws"] = torch.empty(N, H, W, Cout, dtype=F16, device=d), torch.empty(4 * M * Cout, dtype=F32, device=d)
    with _options(igemm_splitk=1):
        launch(dv, parts=4, expect=1)
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        up, us = -(-M // 256) * (Cout // 320) * ks, -(-M // 128) * (Cout // 320) * ks
        assert -(-up // n_cu) < 0.73 * -(-us // n_cu), "the launch does not reach the persistent split-K kernel on this device"
        ref = U.op_igemm(dv["x"], dv["w"], dv["bias"], temb=dv["temb"], res=dv["res"], mode=1)
        y = run3(f"split-K parts={ks}", inputs, {"y": ((N, H, W, Cout), F16), "ws": ((ks, M, Cout), F32)}, launch, work=("ws",))["y"]
    U.assert_splitk_matches_unsplit(y, ref)
    dv["y"].fill_(float("nan"))
    with _options(igemm_splitk=2):
        launch(dv)
        torch.cuda.synchronize()
    assert torch.equal(dv["y"], y), "differs from the 128-row split-K kernel"


@pytest.mark.parametrize("var", ["temb", "res"])
@pytest.mark.parametrize("W", [64, 32, 16])
def test_tap_reuse_widths_one_slab_per_source(W, var):
    """One image of W x W with one 64-channel slab per source.  igemm_pers_tr_ok wants Cin >= 320, so under `tap_reuse` = 2 this shape
    runs the (dy, slab, dx) k order on the 128-row tile whichever `igemm_big` says: the case pins that route's bits and its guards."""
    _both_tiles(f"tap-reuse order W={W} 64+64", 1, W, W, 64, 64, 320, 1, variants=(var,), opts={"tap_reuse": 2})


@pytest.mark.parametrize("W,var", [(64, "temb"), (32, "res"), (16, "temb")])
def test_tap_reuse_kernels(W, var):
    """the tap-reuse kernels proper (igemm_pers_tr.hip) at their smallest channel count, one image: equal to the 128-row tile's KO variant"""
    _both_tiles(f"tap reuse W={W} C=320", 1, W, W, 320, 0, 320, 1, variants=(var,), opts={"tap_reuse": 2})
