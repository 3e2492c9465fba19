"""Transformer2D32 / BasicTransformerBlock32 (diff-mining_amd/train.py) against float64 autograd of the same block written with F.* ops
and torch.softmax.

For a seeded upstream gradient: dX, dcontext and every parameter gradient (under the diffusers names: the stacked q|k|v and k|v
parameters come back split) within max(2e-5, 4 x rel-L2(CPU fp32 autograd, float64)) of float64 (tests/train_tfm_cases.py).  Also: the
forward pass is the composed inference operator entries bit for bit (ff.net.0 composes as dm_f32_op_gemm, then dm_f32_op_geglu); a context
that does not require a gradient gets none; a second backward() accumulates into .grad as torch does; three SGD steps lower the loss."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_cases as TC  # noqa: E402
from tests import train_tfm_cases as TT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _model(case, ctx_grad=True):
    Cc, heads, N, H, W, ctx_dim, groups = case
    k = TT.tfm_case(*case)
    m = T.Transformer2D32(Cc, heads, ctx_dim, groups)
    m.load_state_dict(k["sd"])
    m = m.cuda()
    x = TC.nhwc(k["x"]).cuda().requires_grad_()
    ctx = k["ctx"].cuda().requires_grad_(ctx_grad)
    return k, m, x, ctx


@pytest.mark.parametrize("case", TT.TFM_CASES, ids=lambda c: f"{c[0]}c-{c[1]}h-{c[2]}x{c[3]}x{c[4]}")
def test_transformer_gradients(case):
    k, m, x, ctx = _model(case)
    what = f"transformer {case[0]}c {case[1]}h {case[2]}x{case[3]}x{case[4]}"
    y = m(x, ctx)
    y.backward(TC.nhwc(k["dy"]).cuda())
    torch.cuda.synchronize()
    g64, g32 = k["g64"], k["g32"]
    TT.check(what + " y", TC.nchw(y.detach()).cpu(), k["y64"], k["y32"], TT.TOL_E2E)
    TT.check(what + " dX", TC.nchw(x.grad).cpu(), g64["x"], g32["x"], TT.TOL_E2E)
    TT.check(what + " dcontext", ctx.grad.cpu(), g64["ctx"], g32["ctx"], TT.TOL_E2E)
    grads = m.grad_dict()
    assert list(grads) == TT.TFM_KEYS and len(grads) == 26
    for name, g in grads.items():
        assert g is not None and g.shape == k["sd"][name].shape, name
        TT.check(f"{what} d{name}", g.cpu(), g64[name], g32[name], TT.TOL_E2E)


def test_forward_is_the_composed_inference_operators():
    """GroupNorm -> proj_in -> [LayerNorm -> q|k|v GEMM -> attention -> to_out + x] -> [LayerNorm -> to_q, k|v GEMM on the context ->
    attention -> to_out + x] -> [LayerNorm -> ff.net.0 GEMM -> geglu -> ff.net.2 + x] -> proj_out + input, through the C ABI one entry at a
    time: the module's output, bit for bit"""
    lib = E.load_library()
    case = TT.TFM_CASES[0]
    Cc, heads, N, H, W, ctx_dim, G = case
    k, m, x, ctx = _model(case)
    with torch.no_grad():
        y = m(x, ctx)
    S, P = U.stream, U.ptr
    sd = {n: v.cuda() for n, v in k["sd"].items()}
    b = "transformer_blocks.0."
    M, Tq, Tk, D = N * H * W, H * W, TT.TFM_TK, Cc // heads
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=x.device)          # noqa: E731

    def gemm(X, Wp, bias, res):
        rows, cin = X.shape
        out = new(rows, Wp.shape[0])
        assert lib.dm_f32_op_gemm(S(), P(X), None, P(Wp), P(bias), None, P(res), P(out), 1, 1, rows, 1, rows, cin, cin, Wp.shape[0], 0, 0) == 0
        return out

    def ln(X, name):
        out = new(*X.shape)
        assert lib.dm_f32_op_layernorm(S(), P(X), X.shape[0], Cc, P(sd[b + name + ".weight"]), P(sd[b + name + ".bias"]), 1e-5, P(out)) == 0
        return out

    def attn(q, kk, v, ldq, ldkv, tk):
        out = new(M, Cc)
        assert lib.dm_f32_op_attention(S(), P(q), P(kk), P(v), P(out), ldq, ldkv, ldkv, Cc, Tq * ldq, tk * ldkv, tk * ldkv, Tq * Cc, None, 0, N, heads, Tq, tk, D,
                                       D ** -0.5) == 0
        return out
    xa = x.detach()
    h, st = new(N, H, W, Cc), new(N * G, 2)
    assert lib.dm_f32_op_groupnorm(S(), P(xa), None, N, H * W, Cc, Cc, G, 1e-6, P(sd["norm.weight"]), P(sd["norm.bias"]), 0, P(st), P(h)) == 0
    t = gemm(h.reshape(M, Cc), sd["proj_in.weight"].reshape(Cc, Cc).contiguous(), sd["proj_in.bias"], None)
    qkv = gemm(ln(t, "norm1"), torch.cat([sd[b + f"attn1.to_{n}.weight"] for n in "qkv"]).contiguous(), None, None)
    t = gemm(attn(qkv, qkv[:, Cc:], qkv[:, 2 * Cc:], 3 * Cc, 3 * Cc, Tq), sd[b + "attn1.to_out.0.weight"], sd[b + "attn1.to_out.0.bias"], t)
    q = gemm(ln(t, "norm2"), sd[b + "attn2.to_q.weight"], None, None)
    kv = gemm(ctx.detach().reshape(N * Tk, ctx_dim), torch.cat([sd[b + f"attn2.to_{n}.weight"] for n in "kv"]).contiguous(), None, None)
    t = gemm(attn(q, kv, kv[:, Cc:], Cc, 2 * Cc, Tk), sd[b + "attn2.to_out.0.weight"], sd[b + "attn2.to_out.0.bias"], t)
    p = gemm(ln(t, "norm3"), sd[b + "ff.net.0.proj.weight"], sd[b + "ff.net.0.proj.bias"], None)
    gg = new(M, 4 * Cc)
    assert lib.dm_f32_op_geglu(S(), P(p), M, 4 * Cc, P(gg)) == 0
    t = gemm(gg, sd[b + "ff.net.2.weight"], sd[b + "ff.net.2.bias"], t)
    out = gemm(t, sd["proj_out.weight"].reshape(Cc, Cc).contiguous(), sd["proj_out.bias"], xa.reshape(M, Cc))
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(N, H, W, Cc), y)


def test_context_without_requires_grad_gets_no_gradient():
    case = TT.TFM_CASES[2]
    k, m, x, ctx = _model(case, ctx_grad=False)
    m(x, ctx).backward(TC.nhwc(k["dy"]).cuda())
    k2, m2, x2, ctx2 = _model(case)
    m2(x2, ctx2).backward(TC.nhwc(k["dy"]).cuda())
    torch.cuda.synchronize()
    assert ctx.grad is None and ctx2.grad is not None
    assert torch.equal(x.grad, x2.grad)
    for (n, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.grad, p2.grad), n


def test_second_backward_accumulates_like_torch():
    case = TT.TFM_CASES[1]
    k, m, x, ctx = _model(case)
    dy = TC.nhwc(k["dy"]).cuda()
    m(x, ctx).backward(dy)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    gx, gc = x.grad.clone(), ctx.grad.clone()
    m(x, ctx).backward(dy)
    torch.cuda.synchronize()
    assert len(first) == 23
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n
    assert torch.equal(x.grad, gx + gx) and torch.equal(ctx.grad, gc + gc)


def test_three_sgd_steps_lower_the_loss():
    """sign and wiring, not a rate: plain SGD on one block, a fixed batch and target; the learning rate is one at which the float64
    yardstick itself descends monotonically (asserted)"""
    case = TT.TFM_CASES[2]
    Cc, heads, N, H, W, ctx_dim, G = case
    k, m, x, ctx = _model(case)
    target = TC.randn(N, Cc, H, W, seed=77)
    lr = 0.02
    ref = {n: v.double().requires_grad_() for n, v in k["sd"].items()}
    ref_losses = []
    for _ in range(4):
        loss = F.mse_loss(TT.tfm_ref(ref, k["x"].double(), k["ctx"].double(), heads, G), target.double())
        ref_losses.append(loss.item())
        grads = torch.autograd.grad(loss, list(ref.values()))
        ref = {n: (v - lr * g).detach().requires_grad_() for (n, v), g in zip(ref.items(), grads)}
    assert all(b < a for a, b in zip(ref_losses, ref_losses[1:])), ref_losses
    x, ctx, tgt = x.detach(), ctx.detach(), TC.nhwc(target).cuda()
    losses = []
    for _ in range(4):
        m.zero_grad(set_to_none=True)
        loss = ((m(x, ctx) - tgt) ** 2).mean()
        losses.append(loss.item())
        loss.backward()
        with torch.no_grad():
            for p in m.parameters():
                p -= lr * p.grad
    print("TRAIN_OPS tfm sgd losses device", [f"{v:.6f}" for v in losses], "float64", [f"{v:.6f}" for v in ref_losses])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
