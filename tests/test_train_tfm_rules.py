"""CPU tier of the transformer half of the training operators (diff-mining_amd/train.py), pinned to torch.autograd in float64 on a machine
without a GPU:

  * attention_bwd_host (the device kernels' rule: P recomputed as 2^(s' - L), dS = P (dP - Delta)) equals autograd's dq, dk, dv, and its
    (L, Delta) are the log2-domain log-sum-exp and the row dots dO . O
  * layernorm_bwd_host and geglu_bwd_host equal autograd (a constant row included: rstd = eps^-1/2, xhat = 0)
  * BasicTransformerBlock32 / Transformer2D32 hold to_q | to_k | to_v (and attn2's to_k | to_v) as one stacked parameter each, and their
    state dicts speak the diffusers names and shapes and round-trip exactly

Everything is float64, so the bound is round-off of sums of a few thousand terms: 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

from diff_mining_amd import train as T
from tests import train_tfm_cases as TT

TOL64 = 1e-12


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("c", [(2, 2, 50, 50, 40, 1), (2, 2, 33, 77, 40, 1), (1, 1, 17, 9, 160, 1), (1, 1, 1, 5, 80, 1), (1, 2, 40, 40, 40, 8)], ids=TT.attn_id)
def test_attention_backward_rule(c):
    B, heads, Tq, Tk, D, qs = c
    Cc = heads * D
    q, k, v, do = (TT.randn(B, t, Cc, seed=s).double() for t, s in ((Tq, 1), (Tk, 2), (Tk, 3), (Tq, 4)))
    q = (q * qs).requires_grad_()
    k, v = k.requires_grad_(), v.requires_grad_()
    o = TT.attn_ref(q, k, v, heads)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), do)
    with torch.no_grad():
        assert _rel(T.attention_host(q, k, v, heads), o) < TOL64
        dq, dk, dv, L, delta = T.attention_bwd_host(q, k, v, do, heads)
        assert _rel(dq, gq) < TOL64 and _rel(dk, gk) < TOL64 and _rel(dv, gv) < TOL64
        qh, kh = (t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (q, k))
        s2 = qh @ kh.transpose(-1, -2) * (D ** -0.5 * TT.LOG2E)
        assert _rel(L, torch.log2(torch.exp2(s2 - s2.amax(-1, keepdim=True)).sum(-1)) + s2.amax(-1)) < TOL64
        assert _rel(delta, (do * o).reshape(B, Tq, heads, D).sum(-1).transpose(1, 2)) < TOL64


@pytest.mark.parametrize("rows,Cc,const", [(5, 320, False), (33, 64, False), (4, 320, True)])
def test_layernorm_backward_rule(rows, Cc, const):
    x = (TT.randn(rows, Cc, seed=5) * 2 + 0.5).double()
    if const:
        x[0] = 1.25
    x.requires_grad_()
    gamma, beta = (1 + 0.3 * TT.randn(Cc, seed=6)).double().requires_grad_(), TT.randn(Cc, seed=7).double().requires_grad_()
    dy = TT.randn(rows, Cc, seed=8).double()
    gx, gg, gb = torch.autograd.grad(F.layer_norm(x, (Cc,), gamma, beta, 1e-5), (x, gamma, beta), dy)
    with torch.no_grad():
        dx, dg, db = T.layernorm_bwd_host(x, dy, gamma, 1e-5)
    assert torch.isfinite(dx).all()
    assert _rel(dx, gx) < TOL64 and _rel(dg, gg) < TOL64 and _rel(db, gb) < TOL64
    if const:
        dg0 = dy[0] * gamma.detach()          # a constant row: xhat = 0, rstd = eps^-1/2, so dx = eps^-1/2 (dy gamma - mean(dy gamma))
        assert _rel(dx[0], 1e-5 ** -0.5 * (dg0 - dg0.mean())) < TOL64


def test_geglu_rule():
    p = TT.geglu_case(5, 1280)["p"].double().requires_grad_()
    dy = TT.geglu_case(5, 1280)["dy"].double()
    h, g = p.chunk(2, dim=-1)
    y = h * F.gelu(g)
    (gp,) = torch.autograd.grad(y, p, dy)
    with torch.no_grad():
        assert g.abs().max().item() == 6.0
        assert _rel(T.geglu_host(p), y) < TOL64
        assert _rel(T.geglu_bwd_host(p, dy), gp) < TOL64


def test_block_state_dict_round_trip():
    Cc, heads, ctx_dim = 160, 4, 96
    sd = TT.block_sd(Cc, ctx_dim, seed=3)
    blk = T.BasicTransformerBlock32(Cc, heads, ctx_dim)
    assert {n: tuple(p.shape) for n, p in blk.named_parameters() if "to_qkv" in n or "to_kv" in n} == {
        "attn1_to_qkv_weight": (3 * Cc, Cc), "attn2_to_kv_weight": (2 * Cc, ctx_dim)}
    blk.load_state_dict(sd)
    assert torch.equal(blk.attn1_to_qkv_weight.detach(), torch.cat([sd[f"attn1.to_{n}.weight"] for n in "qkv"]))
    assert torch.equal(blk.attn2_to_kv_weight.detach(), torch.cat([sd[f"attn2.to_{n}.weight"] for n in "kv"]))
    back = blk.state_dict()
    assert list(back) == TT.BLOCK_KEYS
    for k, v in sd.items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    assert list(blk.grad_dict()) == TT.BLOCK_KEYS and all(g is None for g in blk.grad_dict().values())
    with pytest.raises(RuntimeError):
        blk.load_state_dict({k: v for k, v in sd.items() if k != "norm2.bias"})
    with pytest.raises(RuntimeError):
        blk.load_state_dict({**sd, "attn2.to_k.weight": sd["attn2.to_k.weight"][:, :8]})
    with pytest.raises(T.EngineError):
        T.BasicTransformerBlock32(128, 2, ctx_dim)          # head_dim 64: no backward kernel


def test_transformer2d_state_dict_round_trip():
    Cc, heads, ctx_dim = 160, 2, 96
    sd = TT.tfm_sd(Cc, ctx_dim, seed=4)
    m = T.Transformer2D32(Cc, heads, ctx_dim)
    m.load_state_dict(sd)
    back = m.state_dict()
    assert list(back) == TT.TFM_KEYS and list(sd) == TT.TFM_KEYS
    assert back["proj_in.weight"].shape == (Cc, Cc, 1, 1) and back["proj_out.weight"].shape == (Cc, Cc, 1, 1)
    for k, v in sd.items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    assert len(list(m.parameters())) == 4 + 17 + 2          # the stacked projections count once


def test_block_reference_equals_the_host_rules():
    """the F.* reference of the block, rebuilt from the host restatements (stacked projections, GEGLU on P = h | g): the same numbers"""
    Cc, heads, ctx_dim, B, Tq = 160, 4, 96, 2, 11
    sd = {k: v.double() for k, v in TT.block_sd(Cc, ctx_dim, seed=5).items()}
    x, ctx = TT.randn(B, Tq, Cc, seed=1).double(), TT.randn(B, 7, ctx_dim, seed=2).double()
    ref = TT.block_ref(sd, x, ctx, heads)
    ln = lambda t, n: F.layer_norm(t, (Cc,), sd[n + ".weight"], sd[n + ".bias"], 1e-5)          # noqa: E731
    qkv = F.linear(ln(x, "norm1"), torch.cat([sd[f"attn1.to_{n}.weight"] for n in "qkv"]))
    y = x + F.linear(T.attention_host(*qkv.chunk(3, dim=-1), heads), sd["attn1.to_out.0.weight"], sd["attn1.to_out.0.bias"])
    kv = F.linear(ctx, torch.cat([sd[f"attn2.to_{n}.weight"] for n in "kv"]))
    y = y + F.linear(T.attention_host(F.linear(ln(y, "norm2"), sd["attn2.to_q.weight"]), *kv.chunk(2, dim=-1), heads), sd["attn2.to_out.0.weight"],
                     sd["attn2.to_out.0.bias"])
    y = y + F.linear(T.geglu_host(F.linear(ln(y, "norm3"), sd["ff.net.0.proj.weight"], sd["ff.net.0.proj.bias"])), sd["ff.net.2.weight"], sd["ff.net.2.bias"])
    assert _rel(y, ref) < TOL64
