"""The gradient operators of the fp32 net's convolutional blocks (dm_f32_op_gemm_wgrad, _colsum, _groupnorm_bwd, _silu_bwd, _zero_insert2,
_nearest_bwd, and the data gradient = dm_f32_op_gemm on dgrad_weights) against torch.autograd on the CPU in float64.

Tolerance (tests/train_cases.py): device within max(2e-6, 4 x rel-L2(CPU fp32 autograd, float64)) of float64; every case prints its three
figures (lines starting TRAIN_OPS; profiles/train_ops.txt is that table).  Shapes: the smallest that reach each hazard, see CONV_CASES, and
the shapes of tests/train_net_cases.py at which a real training step takes the slab branches (M >= 8192, the cap of 16) and the up
blocks' GroupNorm geometry.
Also: determinism (two runs, and a workspace pre-filled with 0xFF bytes, give the same bits), accumulate = 1 is one fp32 addition onto what
the output holds, and every refusal of include/dm_engine.h returns 1 and leaves the output untouched."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_cases as TC  # noqa: E402
from tests import train_net_cases as TN  # noqa: E402

CONV_CASES = TC.CONV_CASES + TN.NET_CONV_CASES


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _dev_case(c):
    mode, N, H, W, C1, C2, Cout, out_hw = c
    k = TC.conv_case(*c)
    xn = TC.nhwc(k["x"]).cuda()
    xa, xb = (xn[..., :C1].contiguous(), xn[..., C1:].contiguous()) if C2 else (xn, None)
    return k, xa, xb, T.pack_conv(k["w"]).cuda(), TC.nhwc(k["dy"]).cuda()


@pytest.mark.parametrize("c", CONV_CASES, ids=TC.case_id)
def test_wgrad32(c):
    k, xa, xb, _, dy = _dev_case(c)
    got = T.wgrad32(xa, xb, dy, c[0], c[7])
    torch.cuda.synchronize()
    TC.check(f"wgrad32 {TC.case_id(c)}", got.cpu(), T.pack_conv(k["g64"][1]), T.pack_conv(k["g32"][1]))
    # and the float64 restatement in plain indexing says the same as autograd
    assert TC.rel_l2(T.wgrad_host(xa.cpu(), None if xb is None else xb.cpu(), dy.cpu(), c[0], c[7]), T.pack_conv(k["g64"][1])) < 1e-12


@pytest.mark.parametrize("c", CONV_CASES, ids=TC.case_id)
def test_data_gradient(c):
    mode, N, H, W, C1, C2, Cout, out_hw = c
    k, xa, xb, wp, dy = _dev_case(c)
    dx, dx2 = T.dgrad32(dy, wp, mode, xa.shape, C1)
    torch.cuda.synchronize()
    assert (dx2 is None) == (C2 == 0) and dx.shape == xa.shape
    got = dx if dx2 is None else torch.cat([dx, dx2], dim=-1)
    TC.check(f"dgrad {TC.case_id(c)}", got.cpu(), TC.nhwc(k["g64"][0]), TC.nhwc(k["g32"][0]))


@pytest.mark.parametrize("N,HW,Cc", [(3, 63, 196), (2, 1024, 320), (1, 1, 32), (5, 1, 1280)])
def test_colsum(N, HW, Cc):
    dy = TC.randn(N, HW, Cc, seed=31)
    d = dy.cuda()
    per = T.colsum32(d, per_sample=True)
    allrows = T.colsum32(d, per_sample=False)
    torch.cuda.synchronize()
    assert per.shape == (N, Cc) and allrows.shape == (Cc,)
    TC.check(f"colsum dtemb {N}x{HW}x{Cc}", per.cpu(), dy.double().sum(1), dy.sum(1))
    TC.check(f"colsum dbias {N}x{HW}x{Cc}", allrows.cpu(), dy.double().sum((0, 1)), dy.sum((0, 1)))
    # accumulate: one fp32 addition onto what the output holds
    base = TC.randn(N, Cc, seed=32).cuda()
    acc = base.clone()
    assert E.load_library().dm_f32_op_colsum(U.stream(), U.ptr(d), N, HW, Cc, 1, U.ptr(acc)) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc, base + per)


GN_CASES = [(2, 9, 7, 64, 32, 32, True, False),       # HW = 63, three channels per group
            (2, 9, 7, 32, 32, 4, True, False),        # 16 channels per group: a group straddles nothing, group 1 ends at the source boundary
            (2, 9, 7, 32, 64, 3, True, False),        # 32 channels per group over C1 = 32 | C2 = 64
            (2, 3, 5, 32, 32, 1, True, False),        # one group of 64 channels straddles the source boundary
            (2, 1, 1, 64, 32, 32, True, False),       # HW = 1
            (2, 9, 7, 64, 32, 32, False, False),      # without SiLU
            (2, 4, 4, 32, 32, 4, True, True)]         # a constant-input group: var = 0
GN_CASES += TN.NET_GN_CASES                           # 60, 30, 80 and 20 channels per group; a group across C1 | C2 at 60 and 30


@pytest.mark.parametrize("N,H,W,C1,C2,G,silu,const", GN_CASES)
def test_groupnorm_backward(N, H, W, C1, C2, G, silu, const):
    Cc = C1 + C2
    k = TC.gn_case(N, H, W, Cc, G, silu, const)
    x, gamma, beta, dy = k["x"], k["gamma"], k["beta"], k["dy"]
    xn = TC.nhwc(x).cuda()
    xa, xb = xn[..., :C1].contiguous().requires_grad_(), xn[..., C1:].contiguous().requires_grad_()
    ga, be = gamma.cuda().requires_grad_(), beta.cuda().requires_grad_()
    y = T.groupnorm_silu32(xa, xb, ga, be, G, 1e-5, silu)
    y.backward(TC.nhwc(dy).cuda())
    torch.cuda.synchronize()
    what = f"gn_bwd {N}x{H}x{W} {C1}+{C2} G={G} silu={int(silu)}{' var0' if const else ''}"
    r64, r32 = k["r64"], k["r32"]
    TC.check(what + " y", TC.nchw(y.detach()).cpu(), r64[0], r32[0])
    TC.check(what + " dx", TC.nchw(torch.cat([xa.grad, xb.grad], dim=-1)).cpu(), r64[1], r32[1])
    TC.check(what + " dgamma", ga.grad.cpu(), r64[2], r32[2])
    TC.check(what + " dbeta", be.grad.cpu(), r64[3], r32[3])


def test_silu_backward():
    x, dy = TC.randn(5, 1280, seed=51) * 3, TC.randn(5, 1280, seed=52)
    ref = {}
    for dt in (torch.float64, torch.float32):
        xs = x.to(dt, copy=True).requires_grad_()
        ref[dt] = torch.autograd.grad(F.silu(xs), xs, dy.to(dt))[0]
    xd = x.cuda().requires_grad_()
    T.silu32(xd).backward(dy.cuda())
    TC.check("silu_bwd 5x1280", xd.grad.cpu(), ref[torch.float64], ref[torch.float32])


@pytest.mark.parametrize("N,H,W,Cc", [(2, 16, 16, 96), (1, 9, 7, 36), (1, 1, 1, 4), (2, 2, 5, 8)])
def test_zero_insert2(N, H, W, Cc):
    dy = TC.randn(N, (H + 1) // 2, (W + 1) // 2, Cc, seed=61)
    z = T.zero_insert2(dy.cuda(), H, W)
    assert torch.equal(z.cpu(), T.zero_insert2_host(dy, H, W))


@pytest.mark.parametrize("N,H,W,OH,OW,Cc", [(2, 4, 4, 8, 8, 64), (1, 5, 4, 9, 7, 32), (1, 5, 4, 11, 3, 8), (1, 3, 3, 10, 7, 4), (1, 32, 43, 64, 85, 4)])
def test_nearest_backward(N, H, W, OH, OW, Cc):
    du = TC.randn(N, OH, OW, Cc, seed=71)
    ds = T.nearest_bwd(du.cuda(), H, W)
    # the same index rule as F.interpolate, checked through autograd
    xs = torch.zeros(N, Cc, H, W, dtype=torch.float64, requires_grad=True)
    ref = TC.nhwc(torch.autograd.grad(F.interpolate(xs, size=(OH, OW), mode="nearest"), xs, TC.nchw(du).double())[0])
    TC.check(f"nearest_bwd {H}x{W}<-{OH}x{OW}", ds.cpu(), ref, T.nearest_bwd_host(du, H, W))


# ---------------------------------------------------------------------------------------------------------------------------------------
# determinism, accumulation, refusals (through the C ABI, with the caller's own workspace)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _wgrad_raw(c, xa, xb, dy, wk, out, accumulate=0, **over):
    mode, N, H, W, C1, C2, Cout, out_hw = c
    OH, OW = (H, W) if mode in (0, 1) else (dy.shape[1], dy.shape[2])
    a = dict(X=U.ptr(xa), X2=U.ptr(xb), dY=U.ptr(dy), dWp=U.ptr(out), work=U.ptr(wk), work_bytes=wk.numel() * wk.element_size(),
             N=N, H=H, W=W, OH=OH, OW=OW, Cin=C1 + C2, C1=C1, Cout=Cout, mode=mode, accumulate=accumulate)
    a.update(over)
    rc = E.load_library().dm_f32_op_gemm_wgrad(U.stream(), a["X"], a["X2"], a["dY"], a["dWp"], a["work"], a["work_bytes"], a["N"], a["H"], a["W"],
                                               a["OH"], a["OW"], a["Cin"], a["C1"], a["Cout"], a["mode"], a["accumulate"])
    torch.cuda.synchronize()
    return rc


def _work_for(c, dy, fill):
    mode, N, H, W, C1, C2, Cout, out_hw = c
    OH, OW = (H, W) if mode in (0, 1) else (dy.shape[1], dy.shape[2])
    nbytes = E.load_library().dm_f32_op_gemm_wgrad_workspace(N, H, W, OH, OW, C1 + C2, Cout, mode)
    assert nbytes > 0 and nbytes % (4 * Cout * T.taps_of(mode) * (C1 + C2)) == 0      # one partial dWp per slab
    slabs = nbytes // (4 * Cout * T.taps_of(mode) * (C1 + C2))
    assert slabs == TN.wgrad_slab_rule(N * OH * OW)[0]                                # the rule of DESIGN 4ab, restated on the host
    return torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda"), slabs


@pytest.mark.parametrize("c", [TC.CONV_CASES[0], TC.CONV_CASES[2], TC.CONV_CASES[4], TC.CONV_CASES[6], TC.CONV_CASES[8]] + TN.NET_CONV_CASES, ids=TC.case_id)
def test_wgrad32_is_deterministic_and_accumulates(c):
    _, xa, xb, _, dy = _dev_case(c)
    if c in TN.NET_CONV_PARTITIONS:
        assert _work_for(c, dy, 0)[1] == TN.NET_CONV_PARTITIONS[c][0]
    ref = T.wgrad32(xa, xb, dy, c[0], c[7])
    again = T.wgrad32(xa, xb, dy, c[0], c[7])
    torch.cuda.synchronize()
    assert torch.equal(ref, again)
    for fill in (0xFF, 0x00):           # nothing reads workspace the call did not write
        work, slabs = _work_for(c, dy, fill)
        out = torch.full_like(ref, float("nan"))
        assert _wgrad_raw(c, xa, xb, dy, work, out) == 0
        assert torch.equal(out, ref), (fill, slabs)
    base = TC.randn(*ref.shape, seed=81).cuda()
    acc = base.clone()
    assert _wgrad_raw(c, xa, xb, dy, work, acc, accumulate=1) == 0
    assert torch.equal(acc, base + ref)
    assert torch.equal(T.wgrad32(xa, xb, dy, c[0], c[7], out=base.clone(), accumulate=True), base + ref)


def test_slab_count_follows_the_pixel_count_alone():
    ws = E.load_library().dm_f32_op_gemm_wgrad_workspace
    per = lambda N, H, W, Cin, Cout, mode: ws(N, H, W, H, W, Cin, Cout, mode) // (4 * Cout * T.taps_of(mode) * Cin)      # noqa: E731
    assert per(1, 1, 1, 32, 32, 1) == 1 and per(2, 16, 16, 320, 320, 1) == 4 and per(2, 16, 16, 32, 4, 1) == 4
    assert per(1, 1, 231, 768, 64, 0) == 2 and per(4, 64, 64, 320, 320, 1) == 8 and per(4, 64, 64, 960, 320, 1) == 8
    for c, (slabs, _, _) in TN.NET_CONV_PARTITIONS.items():          # M = 8191 | 8197 ... 32 805: both sides of the branch at 8192, and the cap
        mode, N, H, W, C1, C2, Cout, out_hw = c
        OH, OW = (H, W) if mode in (0, 1) else ((H + 1) // 2, (W + 1) // 2) if mode == 2 else out_hw
        assert ws(N, H, W, OH, OW, C1 + C2, Cout, mode) == slabs * 4 * Cout * T.taps_of(mode) * (C1 + C2), c
    assert ws(2, 16, 16, 16, 16, 320, 320, 4) == 0 and ws(2, 16, 16, 16, 16, 320, 320, -1) == 0 and ws(0, 16, 16, 16, 16, 320, 320, 1) == 0


def test_refusals_leave_the_output_untouched():
    lib = E.load_library()
    c = TC.CONV_CASES[0]
    mode, N, H, W, C1, C2, Cout, _ = c
    _, xa, xb, _, dy = _dev_case(c)
    work, _ = _work_for(c, dy, 0x5A)
    sentinel = TC.randn(Cout, 9 * (C1 + C2), seed=91).cuda()
    out = sentinel.clone()
    bad = [dict(X=None), dict(dY=None), dict(work=None), dict(X2=None), dict(Cin=C1 + C2 + 16), dict(Cin=C1 + C2 - 16, C1=C1 - 16), dict(C1=48),
           dict(Cout=Cout + 2), dict(mode=4), dict(mode=-1), dict(mode=5), dict(work_bytes=work.numel() - 1), dict(work_bytes=0), dict(N=0), dict(OH=H + 1),
           dict(mode=2), dict(C1=0), dict(C1=C1 + C2 + 32)]
    for over in bad:
        assert _wgrad_raw(c, xa, xb, dy, work, out, **over) == 1, over
        assert torch.equal(out, sentinel), over
    assert _wgrad_raw(c, xa, xb, dy, work, None) == 1
    assert not (work != 0x5A).any().item()                   # nothing was launched at all
    assert _wgrad_raw(c, xa, xb, dy, work, out) == 0 and not torch.equal(out, sentinel)

    # column sums
    d = TC.randn(3, 63, 196, seed=92).cuda()
    o = torch.full((3, 196), 7.0, device="cuda")
    for args in ((None, 3, 63, 196, 0, U.ptr(o)), (U.ptr(d), 0, 63, 196, 0, U.ptr(o)), (U.ptr(d), 3, 0, 196, 0, U.ptr(o)), (U.ptr(d), 3, 63, 194, 0, U.ptr(o)),
                 (U.ptr(d), 3, 63, 0, 0, U.ptr(o))):
        assert lib.dm_f32_op_colsum(U.stream(), *args) == 1, args
    assert lib.dm_f32_op_colsum(U.stream(), U.ptr(d), 3, 63, 196, 0, None) == 1
    torch.cuda.synchronize()
    assert (o == 7.0).all().item()

    # GroupNorm backward: N, HW, C, C1, G = 2, 63, 96, 64, 32
    x1, x2, g, b = TC.randn(2, 63, 64, seed=93).cuda(), TC.randn(2, 63, 32, seed=94).cuda(), torch.ones(96, device="cuda"), torch.zeros(96, device="cuda")
    st = torch.ones(64, 2, device="cuda")
    wk = torch.zeros(2 * (2 * 96 + 2 * 32) + 1, dtype=torch.float64, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in ((2, 63, 64), (2, 63, 32), (96,), (96,))]
    dyg = TC.randn(2, 63, 96, seed=95).cuda()

    def gn(X=x1, X2=x2, dY=dyg, N=2, HW=63, Cc=96, C1=64, G=32, gamma=g, beta=b, stats=st, work=U.ptr(wk), nbytes=(wk.numel() - 1) * 8, dX=outs[0], dX2=outs[1],
           dg=outs[2], db=outs[3]):
        return lib.dm_f32_op_groupnorm_bwd(U.stream(), U.ptr(X), U.ptr(X2), U.ptr(dY), N, HW, Cc, C1, G, U.ptr(gamma), U.ptr(beta), U.ptr(stats), 1, work, nbytes,
                                           U.ptr(dX), U.ptr(dX2), U.ptr(dg), U.ptr(db))
    for kw in (dict(X=None), dict(X2=None), dict(dY=None), dict(gamma=None), dict(beta=None), dict(stats=None), dict(work=None), dict(dX=None), dict(dX2=None),
               dict(dg=None), dict(db=None), dict(G=5), dict(G=0), dict(N=0), dict(HW=0), dict(C1=0), dict(C1=128), dict(nbytes=(wk.numel() - 1) * 8 - 1),
               dict(work=C.c_void_p(wk.data_ptr() + 4))):
        assert gn(**kw) == 1, kw
    torch.cuda.synchronize()
    assert all((t == 7.0).all().item() for t in outs) and not wk.any().item()
    assert gn() == 0

    # the small kernels
    v = torch.full((64,), 7.0, device="cuda")
    src = TC.randn(64, seed=96).cuda()
    assert lib.dm_f32_op_silu_bwd(U.stream(), None, U.ptr(src), U.ptr(v), 64) == 1 and lib.dm_f32_op_silu_bwd(U.stream(), U.ptr(src), None, U.ptr(v), 64) == 1
    assert lib.dm_f32_op_silu_bwd(U.stream(), U.ptr(src), U.ptr(src), None, 64) == 1 and lib.dm_f32_op_silu_bwd(U.stream(), U.ptr(src), U.ptr(src), U.ptr(v), 0) == 1
    assert lib.dm_f32_op_zero_insert2(U.stream(), None, 1, 4, 4, 4, U.ptr(v)) == 1 and lib.dm_f32_op_zero_insert2(U.stream(), U.ptr(src), 1, 4, 4, 4, None) == 1
    assert lib.dm_f32_op_zero_insert2(U.stream(), U.ptr(src), 1, 4, 4, 2, U.ptr(v)) == 1 and lib.dm_f32_op_zero_insert2(U.stream(), U.ptr(src), 0, 4, 4, 4, U.ptr(v)) == 1
    assert lib.dm_f32_op_nearest_bwd(U.stream(), None, 1, 2, 2, 4, 4, 4, U.ptr(v)) == 1 and lib.dm_f32_op_nearest_bwd(U.stream(), U.ptr(src), 1, 2, 2, 4, 4, 4, None) == 1
    assert lib.dm_f32_op_nearest_bwd(U.stream(), U.ptr(src), 1, 2, 2, 4, 4, 2, U.ptr(v)) == 1 and lib.dm_f32_op_nearest_bwd(U.stream(), U.ptr(src), 1, 2, 2, 0, 4, 4, U.ptr(v)) == 1
    torch.cuda.synchronize()
    assert (v == 7.0).all().item()
