"""Shared by the tests of the transformer half of the training operators (test_train_tfm_rules, test_gpu_train_tfm_ops / _blocks /
_guards): the cases and the float64 yardsticks.  The tolerance rule is tests/train_cases.py's: torch.autograd on the CPU in float64 over
plain F.* ops and torch.softmax is the yardstick, the same autograd in CPU fp32 gives the scale, and the device must lie within
max(floor, 4 x rel-L2(CPU fp32, float64)).  Floors: TOL_OP for LayerNorm backward, GEGLU and the attention statistics (L, Delta); TOL_E2E
for the attention gradients (three chained products through a recomputed softmax and the cancellation in dP - Delta) and for the blocks.
Every reference is computed once (lru_cache) and never written to."""
import functools

import torch
import torch.nn.functional as F

from tests.train_cases import MARGIN, TOL_E2E, TOL_OP, check, randn, rel_l2  # noqa: F401

LOG2E = 1.4426950408889634

# (B, heads, Tq, Tk, D, q-scale)
ATTN_CASES = [
    (2, 2, 200, 200, 40, 1),       # stacked [.][3C] strides, ragged in both directions, four key tiles
    (2, 2, 130, 77, 40, 1),        # cross-attention, k|v stacked
    (1, 1, 65, 65, 80, 1),         # one row past a tile
    (1, 1, 64, 64, 160, 1),        # the mid-block's real shape
    (1, 1, 17, 77, 160, 1),
    (1, 1, 1, 5, 40, 1),
    (1, 1, 1030, 77, 40, 1),       # >= 2 query slabs, the last one ragged
    (1, 2, 100, 100, 40, 8),       # peaked softmax
]


def attn_id(c):
    return "-".join(str(v) for v in c)


def attn_ref(q, k, v, heads):
    """softmax(q k^T / sqrt(D)) v per head, [B,T,C] operands, plain torch ops"""
    B, Tq, Cc = q.shape
    D = Cc // heads
    qh, kh, vh = (t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, Cc)


@functools.lru_cache(maxsize=None)
def attn_case(B, heads, Tq, Tk, D, qscale):
    """q (times qscale), k, v, dO [B,T,heads D] and r64 / r32 = (o, dq, dk, dv, L [B,heads,Tq], delta [B,heads,Tq]) in float64 / fp32:
    L = log2 sum_k 2^(s scale log2 e), delta = sum_d dO O"""
    Cc = heads * D
    q, k, v, do = randn(B, Tq, Cc, seed=81) * qscale, randn(B, Tk, Cc, seed=82), randn(B, Tk, Cc, seed=83), randn(B, Tq, Cc, seed=84)
    out = {"q": q, "k": k, "v": v, "do": do}
    for name, dt in (("r64", torch.float64), ("r32", torch.float32)):
        qs, ks, vs = (t.to(dt, copy=True).requires_grad_() for t in (q, k, v))
        o = attn_ref(qs, ks, vs, heads)
        grads = torch.autograd.grad(o, (qs, ks, vs), do.to(dt))
        with torch.no_grad():
            qh, kh = (t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (qs, ks))
            L = torch.logsumexp(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1) * LOG2E
            delta = (do.to(dt) * o).reshape(B, Tq, heads, D).sum(-1).transpose(1, 2)
        out[name] = (o.detach(),) + grads + (L, delta)
    return out


# (rows, C, constant row): (600, 320) takes three row slabs of the parameter sums
LN_CASES = [(5, 320, False), (231, 640, False), (1, 1280, False), (600, 320, False), (7, 320, True)]


@functools.lru_cache(maxsize=None)
def ln_case(rows, Cc, const):
    """x (`const`: row 0 holds one value, var = 0), gamma, beta, dy and r64 / r32 = (y, dx, dgamma, dbeta) of F.layer_norm"""
    x = randn(rows, Cc, seed=91) * 2 + 0.5
    if const:
        x[0] = 1.25
    gamma, beta, dy = 1 + 0.3 * randn(Cc, seed=92), 0.3 * randn(Cc, seed=93), randn(rows, Cc, seed=94)
    out = {"x": x, "gamma": gamma, "beta": beta, "dy": dy}
    for name, dt in (("r64", torch.float64), ("r32", torch.float32)):
        xs, gs, bs = (t.to(dt, copy=True).requires_grad_() for t in (x, gamma, beta))
        y = F.layer_norm(xs, (Cc,), gs, bs, 1e-5)
        out[name] = (y.detach(),) + torch.autograd.grad(y, (xs, gs, bs), dy.to(dt))
    return out


GEGLU_CASES = [(5, 1280), (63, 2560)]


@functools.lru_cache(maxsize=None)
def geglu_case(M, Fh):
    """P [M][2F] = (h | g) with |g| up to 6, dy, and r64 / r32 = (y, dP) of h * F.gelu(g)"""
    p = randn(M, 2 * Fh, seed=95)
    p[:, Fh:] = (p[:, Fh:] * 2.5).clamp(-6, 6)
    p[0, Fh], p[0, Fh + 1] = 6.0, -6.0
    dy = randn(M, Fh, seed=96)
    out = {"p": p, "dy": dy}
    for name, dt in (("r64", torch.float64), ("r32", torch.float32)):
        ps = p.to(dt, copy=True).requires_grad_()
        h, g = ps.chunk(2, dim=-1)
        y = h * F.gelu(g)
        out[name] = (y.detach(),) + torch.autograd.grad(y, ps, dy.to(dt))
    return out


# ---- the blocks -------------------------------------------------------------------------------------------------------------------------
def block_ref(sd, x, ctx, heads, prefix=""):
    """diffusers BasicTransformerBlock (SD 1.5 settings) in plain F.* ops: x [B,T,C], ctx [B,Tk,ctx_dim]; sd in the diffusers names"""
    w = lambda n: sd[prefix + n]          # noqa: E731
    Cc = x.shape[-1]
    h = F.layer_norm(x, (Cc,), w("norm1.weight"), w("norm1.bias"), 1e-5)
    a = attn_ref(F.linear(h, w("attn1.to_q.weight")), F.linear(h, w("attn1.to_k.weight")), F.linear(h, w("attn1.to_v.weight")), heads)
    x = x + F.linear(a, w("attn1.to_out.0.weight"), w("attn1.to_out.0.bias"))
    h = F.layer_norm(x, (Cc,), w("norm2.weight"), w("norm2.bias"), 1e-5)
    a = attn_ref(F.linear(h, w("attn2.to_q.weight")), F.linear(ctx, w("attn2.to_k.weight")), F.linear(ctx, w("attn2.to_v.weight")), heads)
    x = x + F.linear(a, w("attn2.to_out.0.weight"), w("attn2.to_out.0.bias"))
    h = F.layer_norm(x, (Cc,), w("norm3.weight"), w("norm3.bias"), 1e-5)
    hh, g = F.linear(h, w("ff.net.0.proj.weight"), w("ff.net.0.proj.bias")).chunk(2, dim=-1)
    return x + F.linear(hh * F.gelu(g), w("ff.net.2.weight"), w("ff.net.2.bias"))


def tfm_ref(sd, x, ctx, heads, groups):
    """diffusers Transformer2DModel as SD 1.5 uses it, NCHW x [N,C,H,W]"""
    N, Cc, H, W = x.shape
    h = F.group_norm(x, groups, sd["norm.weight"], sd["norm.bias"], 1e-6)
    h = F.conv2d(h, sd["proj_in.weight"], sd["proj_in.bias"])
    t = block_ref(sd, h.permute(0, 2, 3, 1).reshape(N, H * W, Cc), ctx, heads, "transformer_blocks.0.")
    return F.conv2d(t.reshape(N, H, W, Cc).permute(0, 3, 1, 2), sd["proj_out.weight"], sd["proj_out.bias"]) + x


BLOCK_KEYS = ["norm1.weight", "norm1.bias", "attn1.to_q.weight", "attn1.to_k.weight", "attn1.to_v.weight", "attn1.to_out.0.weight", "attn1.to_out.0.bias",
              "norm2.weight", "norm2.bias", "attn2.to_q.weight", "attn2.to_k.weight", "attn2.to_v.weight", "attn2.to_out.0.weight", "attn2.to_out.0.bias",
              "norm3.weight", "norm3.bias", "ff.net.0.proj.weight", "ff.net.0.proj.bias", "ff.net.2.weight", "ff.net.2.bias"]
TFM_KEYS = ["norm.weight", "norm.bias", "proj_in.weight", "proj_in.bias"] + ["transformer_blocks.0." + k for k in BLOCK_KEYS] + ["proj_out.weight", "proj_out.bias"]


def block_sd(Cc, ctx_dim, seed=0, prefix=""):
    """seeded fp32 parameters of one BasicTransformerBlock under the diffusers names (norm weights around 1)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    sd = {}
    for k in BLOCK_KEYS:
        if k.startswith("norm"):
            sd[k] = 1 + 0.2 * r(Cc) if k.endswith("weight") else 0.2 * r(Cc)
        elif k.endswith("bias"):
            sd[k] = 0.1 * r(8 * Cc if "net.0" in k else Cc)
        else:
            cout = 8 * Cc if "net.0" in k else Cc
            cin = 4 * Cc if "net.2" in k else ctx_dim if k in ("attn2.to_k.weight", "attn2.to_v.weight") else Cc
            sd[k] = r(cout, cin, scale=cin ** -0.5)
    return {prefix + k: v for k, v in sd.items()}


def tfm_sd(Cc, ctx_dim, seed=0):
    g = torch.Generator().manual_seed(seed + 1000)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    sd = {"norm.weight": 1 + 0.2 * r(Cc), "norm.bias": 0.2 * r(Cc), "proj_in.weight": r(Cc, Cc, 1, 1, scale=Cc ** -0.5), "proj_in.bias": 0.1 * r(Cc)}
    sd.update(block_sd(Cc, ctx_dim, seed, "transformer_blocks.0."))
    sd.update({"proj_out.weight": r(Cc, Cc, 1, 1, scale=Cc ** -0.5), "proj_out.bias": 0.1 * r(Cc)})
    return sd


# (C, heads, N, H, W, ctx_dim, groups): head_dim 40, 80, 160 and the real 320-channel level at 8 x 8; 77 context tokens throughout.
# C = 160 is the smallest width that is both a multiple of 32 and heads * D.
TFM_CASES = [(160, 4, 2, 9, 7, 96, 32), (160, 2, 2, 9, 7, 96, 32), (160, 1, 1, 5, 4, 96, 32), (320, 8, 1, 8, 8, 768, 32)]
TFM_TK = 77


@functools.lru_cache(maxsize=None)
def tfm_case(Cc, heads, N, H, W, ctx_dim, groups):
    """inputs, parameters, a seeded upstream gradient and autograd's gradients of everything in float64 and fp32:
    g64 / g32 = {"x", "ctx", <parameter names>}; y64 / y32 = the output (NCHW)"""
    sd = tfm_sd(Cc, ctx_dim, seed=31)
    x, ctx, dy = randn(N, Cc, H, W, seed=32), randn(N, TFM_TK, ctx_dim, seed=33), randn(N, Cc, H, W, seed=34)
    out = {"sd": sd, "x": x, "ctx": ctx, "dy": dy}
    for name, dt in (("g64", torch.float64), ("g32", torch.float32)):
        leaves = {k: v.to(dt, copy=True).requires_grad_() for k, v in {"x": x, "ctx": ctx, **sd}.items()}
        y = tfm_ref({k: leaves[k] for k in sd}, leaves["x"], leaves["ctx"], heads, groups)
        out[name] = dict(zip(leaves, torch.autograd.grad(y, list(leaves.values()), dy.to(dt))))
        out["y" + name[1:]] = y.detach()
    return out
