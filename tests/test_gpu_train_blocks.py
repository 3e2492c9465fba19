"""ResnetBlock32 / Downsample32 / Upsample32 (diff-mining_amd/train.py) against float64 autograd of the same block written with F.* ops.

For a seeded upstream gradient: dX, dX_skip, dtemb and every parameter gradient within max(2e-5, 4 x rel-L2(CPU fp32 autograd, float64)) of
float64 (tests/train_cases.py; 2e-5 = TOL_E2E, these are chains of operators).  Also: the block's forward pass is the composed inference
operator entries bit for bit; a second backward() accumulates into .grad as torch does; three SGD steps lower the loss."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_cases as TC  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _block(case):
    cin, cskip, cout, N, H, W, tch, groups = case
    k = TC.resnet_case(*case)
    blk = T.ResnetBlock32(cin, cout, tch, skip_channels=cskip, groups=groups)
    blk.load_state_dict(k["sd"])
    blk = blk.cuda()
    x = TC.nhwc(k["x"]).cuda().requires_grad_()
    temb = k["temb"].cuda().requires_grad_()
    skip = TC.nhwc(k["skip"]).cuda().requires_grad_() if cskip else None
    return k, blk, x, temb, skip


@pytest.mark.parametrize("case", TC.RESNET_CASES, ids=lambda c: f"{c[0]}+{c[1]}-{c[2]}")
def test_resnet_block_gradients(case):
    k, blk, x, temb, skip = _block(case)
    what = f"resnet {case[0]}+{case[1]}->{case[2]} {case[3]}x{case[4]}x{case[5]}"
    y = blk(x, temb, skip)
    y.backward(TC.nhwc(k["dy"]).cuda())
    torch.cuda.synchronize()
    g64, g32 = k["g64"], k["g32"]
    TC.check(what + " y", TC.nchw(y.detach()).cpu(), k["y64"], k["y32"], TC.TOL_E2E)
    TC.check(what + " dX", TC.nchw(x.grad).cpu(), g64["x"], g32["x"], TC.TOL_E2E)
    if skip is not None:
        TC.check(what + " dX_skip", TC.nchw(skip.grad).cpu(), g64["skip"], g32["skip"], TC.TOL_E2E)
    TC.check(what + " dtemb", temb.grad.cpu(), g64["temb"], g32["temb"], TC.TOL_E2E)
    grads = blk.grad_dict()
    assert list(grads) == list(k["sd"]) and len(grads) == (12 if blk.has_shortcut else 10)
    for name, g in grads.items():
        assert g is not None and g.shape == k["sd"][name].shape, name
        TC.check(f"{what} d{name}", g.cpu(), g64[name], g32[name], TC.TOL_E2E)


def test_resnet_forward_is_the_composed_inference_operators():
    """norm1 + SiLU -> conv1 (+ bias, + time_emb_proj(SiLU(temb))) -> norm2 + SiLU -> conv2 (+ bias, + conv_shortcut(x | skip)) through the
    C ABI one entry at a time, on cat-free two-source operands: the block's output, bit for bit"""
    lib = E.load_library()
    case = TC.RESNET_CASES[2]
    cin, cskip, cout, N, H, W, tch, G = case
    k, blk, x, temb, skip = _block(case)
    with torch.no_grad():
        y = blk(x, temb, skip)
    d, S, P = x.device, U.stream, U.ptr
    sd = {n: v.cuda() for n, v in k["sd"].items()}
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=d)          # noqa: E731
    Cc = cin + cskip
    xa, xb = x.detach(), skip.detach()

    def gemm(X, X2, Wp, bias, tb, res, Cin, C1, mode):
        out = new(N, H, W, cout) if X.dim() == 4 else new(X.shape[0], cout)
        n, h, w = (N, H, W) if X.dim() == 4 else (1, 1, X.shape[0])
        assert lib.dm_f32_op_gemm(S(), P(X), P(X2), P(Wp), P(bias), P(tb), P(res), P(out), n, h, w, h, w, Cin, C1, cout, mode, cout if tb is not None else 0) == 0
        return out
    h1, st = new(N, H, W, Cc), new(N * G, 2)
    assert lib.dm_f32_op_groupnorm(S(), P(xa), P(xb), N, H * W, Cc, cin, G, 1e-5, P(sd["norm1.weight"]), P(sd["norm1.bias"]), 1, P(st), P(h1)) == 0
    ts = new(N, tch)
    assert lib.dm_f32_op_silu(S(), P(temb.detach()), P(ts), ts.numel()) == 0
    tp = gemm(ts, None, sd["time_emb_proj.weight"], sd["time_emb_proj.bias"], None, None, tch, tch, 0)
    c1 = gemm(h1, None, U.pack_conv3(sd["conv1.weight"]), sd["conv1.bias"], tp, None, Cc, Cc, 1)
    h2 = new(N, H, W, cout)
    assert lib.dm_f32_op_groupnorm(S(), P(c1), None, N, H * W, cout, cout, G, 1e-5, P(sd["norm2.weight"]), P(sd["norm2.bias"]), 1, P(st), P(h2)) == 0
    sc = gemm(xa, xb, sd["conv_shortcut.weight"].reshape(cout, Cc).contiguous(), sd["conv_shortcut.bias"], None, None, Cc, cin, 0)
    out = gemm(h2, None, U.pack_conv3(sd["conv2.weight"]), sd["conv2.bias"], None, sc, cout, cout, 1)
    torch.cuda.synchronize()
    assert torch.equal(out, y)


def test_second_backward_accumulates_like_torch():
    case = TC.RESNET_CASES[1]
    k, blk, x, temb, _ = _block(case)
    dy = TC.nhwc(k["dy"]).cuda()
    blk(x, temb).backward(dy)
    first = {n: p.grad.clone() for n, p in blk.named_parameters()}
    gx = x.grad.clone()
    blk(x, temb).backward(dy)
    torch.cuda.synchronize()
    assert len(first) == 12
    for n, p in blk.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n
    assert torch.equal(x.grad, gx + gx)


def test_three_sgd_steps_lower_the_loss():
    """sign and wiring, not a rate: plain SGD on one block, a fixed batch and target; the learning rate is one at which the float64
    yardstick itself descends monotonically (asserted)"""
    case = TC.RESNET_CASES[1]
    cin, _, cout, N, H, W, tch, G = case
    k, blk, x, temb, _ = _block(case)
    target = TC.randn(N, cout, H, W, seed=77)
    lr = 0.05
    ref = {n: v.double().requires_grad_() for n, v in k["sd"].items()}
    ref_losses = []
    for _ in range(4):
        loss = F.mse_loss(TC.resnet_ref(ref, k["x"].double(), k["temb"].double(), None, G), target.double())
        ref_losses.append(loss.item())
        grads = torch.autograd.grad(loss, list(ref.values()))
        ref = {n: (v - lr * g).detach().requires_grad_() for (n, v), g in zip(ref.items(), grads)}
    assert all(b < a for a, b in zip(ref_losses, ref_losses[1:])), ref_losses
    x, temb, tgt = x.detach(), temb.detach(), TC.nhwc(target).cuda()
    losses = []
    for _ in range(4):
        blk.zero_grad(set_to_none=True)
        loss = ((blk(x, temb) - tgt) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        with torch.no_grad():
            for p in blk.parameters():
                p -= lr * p.grad
    print("TRAIN_OPS sgd losses device", [f"{v:.6f}" for v in losses], "float64", [f"{v:.6f}" for v in ref_losses])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


@pytest.mark.parametrize("kind,N,H,W,Cc,out_hw", [("down", 2, 9, 7, 32, None), ("down", 1, 16, 16, 64, None), ("up", 2, 4, 4, 64, None), ("up", 1, 5, 4, 32, (9, 7)),
                                                  ("up", 1, 5, 4, 32, (11, 3))])
def test_sampler_gradients(kind, N, H, W, Cc, out_hw):
    x, w, b = TC.randn(N, Cc, H, W, seed=1), TC.randn(Cc, Cc, 3, 3, seed=2, scale=(9 * Cc) ** -0.5), TC.randn(Cc, seed=3)
    mode = 2 if kind == "down" else 3
    size = out_hw if out_hw is not None else (2 * H, 2 * W)
    ref, dy = {}, None
    for dt in (torch.float64, torch.float32):
        xs, ws, bs = (t.to(dt, copy=True).requires_grad_() for t in (x, w, b))
        y = TC.conv_ref(xs, ws, bs, mode, size)
        dy = TC.randn(*y.shape, seed=4) if dy is None else dy
        ref[dt] = (y.detach(),) + torch.autograd.grad(y, (xs, ws, bs), dy.to(dt))
    m = (T.Downsample32 if kind == "down" else T.Upsample32)(Cc)
    m.load_state_dict({"conv.weight": w, "conv.bias": b})
    m = m.cuda()
    xd = TC.nhwc(x).cuda().requires_grad_()
    y = m(xd) if kind == "down" else m(xd, out_hw)
    y.backward(TC.nhwc(dy).cuda())
    torch.cuda.synchronize()
    what = f"{kind}sample {N}x{H}x{W}x{Cc}" + (f" to {out_hw}" if out_hw else "")
    r64, r32 = ref[torch.float64], ref[torch.float32]
    g = m.grad_dict()
    TC.check(what + " y", TC.nchw(y.detach()).cpu(), r64[0], r32[0], TC.TOL_E2E)
    TC.check(what + " dX", TC.nchw(xd.grad).cpu(), r64[1], r32[1], TC.TOL_E2E)
    TC.check(what + " dW", g["conv.weight"].cpu(), r64[2], r32[2], TC.TOL_E2E)
    TC.check(what + " db", g["conv.bias"].cpu(), r64[3], r32[3], TC.TOL_E2E)
