"""Guard bands around every operand of the gradient entries (tests/test_gpu_guards.py run3: a plain run, then all device operands —
workspaces included — inside one allocation between guards filled with 0xFF, then 0x00): the guards and the inputs come back untouched,
and the three results are equal bit for bit, so no load outside a tensor (or of workspace the call did not write) reaches a result.
Shapes: the ragged cases of tests/test_gpu_train_ops.py, and the 16-slab weight gradient of tests/train_net_cases.py (the cap of the slab rule:
sixteen partials in the workspace, the last slab ragged); the plain result is checked against float64 there."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_cases as TC  # noqa: E402
from tests import train_net_cases as TN  # noqa: E402
from tests.test_gpu_guards import run3  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


@pytest.mark.parametrize("c", [TC.CONV_CASES[0], TC.CONV_CASES[1], TC.CONV_CASES[4], TC.CONV_CASES[6], TC.CONV_CASES[8], TN.CONV_16_SLABS], ids=TC.case_id)
def test_wgrad32(c):
    lib = E.load_library()
    mode, N, H, W, C1, C2, Cout, out_hw = c
    k = TC.conv_case(*c)
    xn, dy = TC.nhwc(k["x"]), TC.nhwc(k["dy"])
    OH, OW = dy.shape[1], dy.shape[2]
    inputs = {"x": xn[..., :C1].contiguous(), "dy": dy}
    if C2:
        inputs["x2"] = xn[..., C1:].contiguous()
    nbytes = lib.dm_f32_op_gemm_wgrad_workspace(N, H, W, OH, OW, C1 + C2, Cout, mode)
    assert nbytes > 0
    if c == TN.CONV_16_SLABS:
        assert nbytes == 16 * 4 * Cout * (C1 + C2) and TN.wgrad_slab_rule(N * OH * OW)[::2] == (16, [2080] * 15 + [1605])

    def launch(v):
        assert lib.dm_f32_op_gemm_wgrad(U.stream(), U.ptr(v["x"]), U.ptr(v.get("x2")), U.ptr(v["dy"]), U.ptr(v["dw"]), U.ptr(v["work"]), nbytes, N, H, W, OH, OW,
                                        C1 + C2, C1, Cout, mode, 0) == 0
    dw = run3(f"wgrad32 {TC.case_id(c)}", inputs, {"dw": ((Cout, T.taps_of(mode) * (C1 + C2)), F32), "work": ((nbytes // 4,), F32)}, launch, work=("work",))["dw"]
    TC.check(f"guarded wgrad32 {TC.case_id(c)}", dw.cpu(), T.pack_conv(k["g64"][1]), T.pack_conv(k["g32"][1]))


@pytest.mark.parametrize("c", [TC.CONV_CASES[0], TC.CONV_CASES[6], TC.CONV_CASES[8]], ids=TC.case_id)
def test_data_gradient_chain(c):
    """the data gradient's own kernels (zero_insert2, nearest_bwd) and the gemm32 launches between them, every intermediate guarded"""
    lib = E.load_library()
    mode, N, H, W, C1, C2, Cout, out_hw = c
    k = TC.conv_case(*c)
    dy = TC.nhwc(k["dy"])
    OH, OW = dy.shape[1], dy.shape[2]
    wd = T.dgrad_weights(T.pack_conv(k["w"]), mode, pad_to=32)
    coutp = wd.shape[1] // 9
    dyp = torch.nn.functional.pad(dy, (0, coutp - Cout))
    GH, GW = (H, W) if mode == 2 else (OH, OW)           # the grid the mode-1 convolution runs on
    outputs = {"dx": ((N, H, W, C1), F32)}
    if C2:
        outputs["dx2"] = ((N, H, W, C2), F32)
    if mode == 2:
        outputs["z"] = ((N, H, W, coutp), F32)
    if mode == 3:
        outputs["du"] = ((N, OH, OW, C1), F32)

    def launch(v):
        g = v["dy"]
        if mode == 2:
            assert lib.dm_f32_op_zero_insert2(U.stream(), U.ptr(g), N, H, W, coutp, U.ptr(v["z"])) == 0
            g = v["z"]
        for name, lo, hi in (("dx", 0, C1), ("dx2", C1, C1 + C2)):
            if hi == lo:
                continue
            tgt = v["du"] if mode == 3 else v[name]
            assert lib.dm_f32_op_gemm(U.stream(), U.ptr(g), None, U.ptr(v["wd"][lo:hi]), None, None, None, U.ptr(tgt), N, GH, GW, GH, GW, coutp, coutp, hi - lo, 1, 0) == 0
            if mode == 3:
                assert lib.dm_f32_op_nearest_bwd(U.stream(), U.ptr(tgt), N, H, W, OH, OW, hi - lo, U.ptr(v[name])) == 0
    out = run3(f"dgrad {TC.case_id(c)}", {"dy": dyp, "wd": wd}, outputs, launch)
    got = out["dx"] if not C2 else torch.cat([out["dx"], out["dx2"]], dim=-1)
    TC.check(f"guarded dgrad {TC.case_id(c)}", got.cpu(), TC.nhwc(k["g64"][0]), TC.nhwc(k["g32"][0]))


@pytest.mark.parametrize("N,HW,Cc", [(3, 63, 196), (1, 231, 36)])
def test_colsum(N, HW, Cc):
    lib = E.load_library()
    dy = TC.randn(N, HW, Cc, seed=31)

    def launch(v):
        assert lib.dm_f32_op_colsum(U.stream(), U.ptr(v["dy"]), N, HW, Cc, 0, U.ptr(v["per"])) == 0
        assert lib.dm_f32_op_colsum(U.stream(), U.ptr(v["dy"]), 1, N * HW, Cc, 0, U.ptr(v["all"])) == 0
    out = run3(f"colsum {N}x{HW}x{Cc}", {"dy": dy}, {"per": ((N, Cc), F32), "all": ((Cc,), F32)}, launch)
    TC.check("guarded colsum per sample", out["per"].cpu(), dy.double().sum(1), dy.sum(1))
    TC.check("guarded colsum all rows", out["all"].cpu(), dy.double().sum((0, 1)), dy.sum((0, 1)))


@pytest.mark.parametrize("N,H,W,C1,C2,G", [(2, 9, 7, 64, 32, 32), (2, 3, 5, 32, 32, 1), (2, 1, 1, 64, 32, 32)])
def test_groupnorm_backward(N, H, W, C1, C2, G):
    lib = E.load_library()
    Cc, HW = C1 + C2, H * W
    k = TC.gn_case(N, H, W, Cc, G, True, False)
    x, dy, gamma, beta = TC.nhwc(k["x"]).reshape(N, HW, Cc), TC.nhwc(k["dy"]).reshape(N, HW, Cc), k["gamma"], k["beta"]
    nwork = 2 * (N * Cc + N * G)

    def launch(v):
        assert lib.dm_f32_op_groupnorm(U.stream(), U.ptr(v["x1"]), U.ptr(v["x2"]), N, HW, Cc, C1, G, 1e-5, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1, U.ptr(v["stats"]),
                                       U.ptr(v["y"])) == 0
        assert lib.dm_f32_op_groupnorm_bwd(U.stream(), U.ptr(v["x1"]), U.ptr(v["x2"]), U.ptr(v["dy"]), N, HW, Cc, C1, G, U.ptr(v["gamma"]), U.ptr(v["beta"]),
                                           U.ptr(v["stats"]), 1, U.ptr(v["work"]), nwork * 8, U.ptr(v["dx1"]), U.ptr(v["dx2"]), U.ptr(v["dgamma"]), U.ptr(v["dbeta"])) == 0
    out = run3(f"gn_bwd {N}x{HW} {C1}+{C2} G={G}", {"x1": x[..., :C1].contiguous(), "x2": x[..., C1:].contiguous(), "dy": dy, "gamma": gamma, "beta": beta},
               {"stats": ((N * G, 2), F32), "y": ((N, HW, Cc), F32), "work": ((nwork,), F64), "dx1": ((N, HW, C1), F32), "dx2": ((N, HW, C2), F32),
                "dgamma": ((Cc,), F32), "dbeta": ((Cc,), F32)}, launch)          # the workspace is written in full: compared too
    r64, r32 = k["r64"], k["r32"]
    TC.check("guarded gn_bwd dx", TC.nchw(torch.cat([out["dx1"], out["dx2"]], dim=-1).reshape(N, H, W, Cc)).cpu(), r64[1], r32[1])
    TC.check("guarded gn_bwd dgamma", out["dgamma"].cpu(), r64[2], r32[2])
    TC.check("guarded gn_bwd dbeta", out["dbeta"].cpu(), r64[3], r32[3])


def test_small_kernels():
    lib = E.load_library()
    x, dy = TC.randn(5, 129, seed=51) * 3, TC.randn(5, 129, seed=52)
    out = run3("silu_bwd", {"x": x, "dy": dy}, {"dx": ((5, 129), F32)},
               lambda v: _ok(lib.dm_f32_op_silu_bwd(U.stream(), U.ptr(v["x"]), U.ptr(v["dy"]), U.ptr(v["dx"]), x.numel())))["dx"]
    ref = []
    for dt in (F64, F32):
        xs = x.to(dt, copy=True).requires_grad_()
        ref.append(torch.autograd.grad(torch.nn.functional.silu(xs), xs, dy.to(dt))[0])
    TC.check("guarded silu_bwd", out.cpu(), ref[0], ref[1])
    N, H, W, Cc = 1, 9, 7, 36
    g = TC.randn(N, 5, 4, Cc, seed=61)
    z = run3("zero_insert2", {"dy": g}, {"z": ((N, H, W, Cc), F32)}, lambda v: _ok(lib.dm_f32_op_zero_insert2(U.stream(), U.ptr(v["dy"]), N, H, W, Cc, U.ptr(v["z"]))))["z"]
    assert torch.equal(z.cpu(), T.zero_insert2_host(g, H, W))
    for (h, w, oh, ow) in ((5, 4, 9, 7), (5, 4, 11, 3)):
        du = TC.randn(2, oh, ow, 36, seed=71)
        ds = run3(f"nearest_bwd {h}x{w}<-{oh}x{ow}", {"du": du}, {"ds": ((2, h, w, 36), F32)},
                  lambda v: _ok(lib.dm_f32_op_nearest_bwd(U.stream(), U.ptr(v["du"]), 2, h, w, oh, ow, 36, U.ptr(v["ds"]))))["ds"]
        TC.check("guarded nearest_bwd", ds.cpu(), T.nearest_bwd_host(du.double(), h, w), T.nearest_bwd_host(du, h, w))


def _ok(rc):
    assert rc == 0
