"""The gradient operators of the transformer blocks (attention, LayerNorm, GEGLU; diff-mining_amd/train.py over f32_train_attn.hip and
f32_train.hip) against torch.autograd in float64 on the CPU.

Rule (tests/train_tfm_cases.py): within max(floor, 4 x rel-L2(CPU fp32 autograd, float64)) of float64; floor 2e-6 for LayerNorm backward,
GEGLU and the attention statistics (L, Delta), 2e-5 for the attention gradients.  Every check prints its three figures (lines starting
TRAIN_OPS; profiles/train_tfm_ops.txt is that table).  Also: the slab rule, determinism (two runs, and a workspace pre-filled with 0xFF
bytes, give the same bits) and every refusal of include/dm_engine.h (1, nothing launched).  The shapes of tests/train_net_cases.py add the
partitions a real step takes: the cap of 16 query slabs with an empty trailing slab (it must write zeros), a slab of one query,
B * heads = 32, and LayerNorm's cap of 64 row slabs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_net_cases as TN  # noqa: E402
from tests import train_tfm_cases as TT  # noqa: E402

ATTN_CASES = TT.ATTN_CASES + TN.NET_ATTN_CASES
LN_CASES = TT.LN_CASES + TN.NET_LN_CASES


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _operands(c):
    """device operands in the layout the blocks use: self-attention (Tq == Tk) on stacked q|k|v rows, cross-attention on q and stacked k|v"""
    B, heads, Tq, Tk, D, _ = c
    k = TT.attn_case(*c)
    Cc = heads * D
    if Tq == Tk:
        a = torch.cat([k["q"], k["k"], k["v"]], dim=-1).cuda()
        return k, (a, None, None), (a[..., :Cc], a[..., Cc:2 * Cc], a[..., 2 * Cc:]), 1
    q, kv = k["q"].cuda(), torch.cat([k["k"], k["v"]], dim=-1).cuda()
    return k, (q, kv, None), (q, kv[..., :Cc], kv[..., Cc:]), 2


@pytest.mark.parametrize("c", ATTN_CASES, ids=TT.attn_id)
def test_attention_gradients(c):
    B, heads, Tq, Tk, D, _ = c
    k, leaves, (q, kk, v), layout = _operands(c)
    Cc = heads * D
    what = f"attention {TT.attn_id(c)}"
    leaves = tuple(t.requires_grad_() if t is not None else None for t in leaves)
    o = T._Attention32.apply(*leaves, heads, layout)
    o.backward(k["do"].cuda())
    torch.cuda.synchronize()
    if layout == 1:
        g = leaves[0].grad
        dq, dk, dv = g[..., :Cc], g[..., Cc:2 * Cc], g[..., 2 * Cc:]
    else:
        dq, dk, dv = leaves[0].grad, leaves[1].grad[..., :Cc], leaves[1].grad[..., Cc:]
    r64, r32 = k["r64"], k["r32"]
    TT.check(what + " o", o.detach().cpu(), r64[0], r32[0], TT.TOL_E2E)
    TT.check(what + " dq", dq.cpu(), r64[1], r32[1], TT.TOL_E2E)
    TT.check(what + " dk", dk.cpu(), r64[2], r32[2], TT.TOL_E2E)
    TT.check(what + " dv", dv.cpu(), r64[3], r32[3], TT.TOL_E2E)
    # the statistics at the head of the workspace, through the operator with a caller's workspace
    do = k["do"].cuda()
    outs = [torch.empty(B, t, Cc, device="cuda") for t in (Tq, Tk, Tk)]
    work = T.attention_bwd32(q.detach(), kk.detach(), v.detach(), o.detach(), do, *outs, heads)
    torch.cuda.synchronize()
    st = work[: 2 * B * heads * Tq].reshape(B, heads, Tq, 2).cpu()
    TT.check(what + " L", st[..., 0], r64[4], r32[4], TT.TOL_OP)
    TT.check(what + " delta", st[..., 1], r64[5], r32[5], TT.TOL_OP)
    assert torch.equal(outs[0], dq) and torch.equal(outs[1], dk) and torch.equal(outs[2], dv)          # contiguous outputs: the same bits


def test_separate_operands():
    """attention32 on three separate tensors equals the stacked call bit for bit"""
    c = TT.ATTN_CASES[1]
    k = TT.attn_case(*c)
    q, kk, v = (k[n].cuda().requires_grad_() for n in "qkv")
    T.attention32(q, kk, v, c[1]).backward(k["do"].cuda())
    _, leaves, _, layout = _operands(c)
    leaves = tuple(t.requires_grad_() if t is not None else None for t in leaves)
    T._Attention32.apply(*leaves, c[1], layout).backward(k["do"].cuda())
    torch.cuda.synchronize()
    Cc = c[1] * c[4]
    assert torch.equal(q.grad, leaves[0].grad) and torch.equal(kk.grad, leaves[1].grad[..., :Cc]) and torch.equal(v.grad, leaves[1].grad[..., Cc:])


def test_slab_rule():
    lib = E.load_library()
    slabs, ws = lib.dm_f32_op_attention_bwd_slabs, lib.dm_f32_op_attention_bwd_workspace
    assert slabs(1030, 77) == 3 and slabs(200, 200) == 1 and slabs(4096, 4096) == 1 and slabs(4096, 77) == 8 and slabs(1024, 77) == 2
    assert slabs(64, 77) == 1 and slabs(100000, 77) == 16 and slabs(512, 128) == 1 and slabs(513, 128) == 2 and slabs(513, 129) == 1
    # the workspace: (L, Delta) per (b, head, q), rounded up to 16 bytes, then slabs x [B heads][Tk][2 D] partials
    assert ws(1, 1, 1030, 77, 40) == 4 * (2 * 1030 + 3 * 77 * 80) and ws(1, 1, 1, 5, 40) == 4 * (4 + 5 * 80)
    assert ws(4, 8, 4096, 4096, 40) == 4 * (2 * 32 * 4096 + 32 * 4096 * 80) and ws(4, 8, 4096, 77, 40) == 4 * (2 * 32 * 4096 + 8 * 32 * 77 * 80)
    for c, (n, _, _) in TN.NET_ATTN_PARTITIONS.items():          # and the host's restatement of the rule says the same
        assert slabs(c[2], c[3]) == n == TN.attn_slab_rule(c[2], c[3])[0], c
    for tq, tk in ((1030, 77), (200, 200), (4096, 77), (513, 128), (513, 129), (100000, 77), (8200, 77), (4097, 77), (1, 5)):
        assert slabs(tq, tk) == TN.attn_slab_rule(tq, tk)[0], (tq, tk)
    for bad in ((1, 1, 64, 64, 64), (1, 1, 64, 64, 512), (0, 1, 64, 64, 40), (1, 0, 64, 64, 40), (1, 1, 0, 64, 40), (1, 1, 64, 0, 40), (1, 1, 64, 64, 0),
                (256, 256, 64, 64, 40)):
        assert ws(*bad) == 0, bad


def _raw(c, **over):
    """dm_f32_op_attention_bwd through the C ABI on separate contiguous tensors; `over` replaces arguments"""
    lib = E.load_library()
    B, heads, Tq, Tk, D, _ = c
    k = TT.attn_case(*c)
    Cc = heads * D
    t = {n: k[n].cuda() for n in ("q", "k", "v", "do")}
    t["o"] = T.attention_fwd32(t["q"], t["k"], t["v"], heads)
    for n, rows in (("dq", Tq), ("dk", Tk), ("dv", Tk)):
        t[n] = torch.full((B, rows, Cc), 7.0, device="cuda")
    nbytes = lib.dm_f32_op_attention_bwd_workspace(B, heads, Tq, Tk, D)
    t["work"] = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    a = dict(ptr={n: U.ptr(t[n]) for n in t}, ld=[Cc] * 8, bs=[Tq * Cc, Tk * Cc, Tk * Cc, Tq * Cc, Tq * Cc, Tq * Cc, Tk * Cc, Tk * Cc], slot=None, B=B, heads=heads, Tq=Tq,
             Tk=Tk, D=D, nbytes=nbytes)
    for key, val in over.items():
        if key in a["ptr"]:
            a["ptr"][key] = val
        elif key.startswith("ld") or key.startswith("bs"):
            a[key[:2]][int(key[2:])] = val
        else:
            a[key] = val
    p = a["ptr"]
    rc = lib.dm_f32_op_attention_bwd(U.stream(), p["q"], p["k"], p["v"], p["o"], p["do"], p["dq"], p["dk"], p["dv"], (C.c_int32 * 8)(*a["ld"]),
                                     (C.c_int64 * 8)(*a["bs"]), a["slot"], a["B"], a["heads"], a["Tq"], a["Tk"], a["D"], a["D"] ** -0.5 if a["D"] > 0 else 1.0,
                                     p["work"], a["nbytes"])
    torch.cuda.synchronize()
    return rc, t


@pytest.mark.parametrize("c", [TT.ATTN_CASES[1], TT.ATTN_CASES[6], TT.ATTN_CASES[0]] + TN.NET_ATTN_CASES, ids=TT.attn_id)
def test_attention_backward_is_deterministic(c):
    """two runs, and a workspace pre-filled with 0xFF bytes: the same bits; a query slab that holds no query leaves zero partials"""
    lib = E.load_library()
    B, heads, Tq, Tk, D, _ = c
    if c == TT.ATTN_CASES[6]:
        assert lib.dm_f32_op_attention_bwd_slabs(Tq, Tk) >= 2 and Tq % 64 != 0          # several query slabs, the last one ragged
    rc, a = _raw(c)
    rc2, b = _raw(c)
    assert rc == 0 and rc2 == 0 and not (a["dq"] == 7.0).all().item()
    k = TT.attn_case(*c)
    t = {n: k[n].cuda() for n in ("q", "k", "v", "do")}
    o = T.attention_fwd32(t["q"], t["k"], t["v"], heads)
    outs = [torch.empty_like(a[n]) for n in ("dq", "dk", "dv")]
    work = torch.full((a["work"].numel() // 4,), float("nan"), device="cuda")
    work.view(torch.int32).fill_(-1)
    T.attention_bwd32(t["q"], t["k"], t["v"], o, t["do"], *outs, heads, work=work)
    torch.cuda.synchronize()
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(a[n], b[n]), n
        assert torch.equal(a[n], outs[i]), n
    # the workspace: the statistics, up to 3 floats of padding to 16 bytes that nothing writes or reads (they keep their fill), the partials
    n_st = 2 * B * heads * Tq
    wa, wb, wc = (w.view(torch.int32) for w in (a["work"], b["work"], work))
    for sl in (slice(0, n_st), slice((n_st + 3) // 4 * 4, None)):
        assert torch.equal(wa[sl], wb[sl]) and torch.equal(wa[sl], wc[sl])
    assert (a["work"][4 * n_st:4 * ((n_st + 3) // 4 * 4)] == 0x5A).all().item() and (wc[n_st:(n_st + 3) // 4 * 4] == -1).all().item()
    # the partials behind the statistics, [slabs][B heads][Tk][2 D]: an empty slab wrote zeros over the 0xFF bytes, a populated one did not
    slabs, _, pop = TN.attn_slab_rule(Tq, Tk)
    assert slabs == lib.dm_f32_op_attention_bwd_slabs(Tq, Tk)
    part = work[(2 * B * heads * Tq + 3) // 4 * 4:].reshape(slabs, -1)
    for s in range(slabs):
        assert torch.isfinite(part[s]).all().item() and (not part[s].any().item()) == (pop[s] == 0), (s, pop[s])
    if c == TN.ATTN_EMPTY_SLAB:
        assert pop[15] == 0 and pop[14] == 136


def test_phases_one_by_one_equal_the_full_call():
    """dm_f32_op_attention_bwd_phases (the rate tool's entry): the four kernels launched one call each give the full call's bits; a mask
    outside 1 .. 15 is refused"""
    lib = E.load_library()
    c = TT.ATTN_CASES[6]
    B, heads, Tq, Tk, D, _ = c
    Cc = heads * D
    rc, t = _raw(c)
    assert rc == 0
    outs = [torch.full_like(t[n], 7.0) for n in ("dq", "dk", "dv")]
    work = torch.full_like(t["work"], 0x5A)
    ld, bs = (C.c_int32 * 8)(*[Cc] * 8), (C.c_int64 * 8)(*[Tq * Cc, Tk * Cc, Tk * Cc, Tq * Cc, Tq * Cc, Tq * Cc, Tk * Cc, Tk * Cc])

    def run(phases):
        return lib.dm_f32_op_attention_bwd_phases(U.stream(), *(U.ptr(t[n]) for n in ("q", "k", "v", "o", "do")), *(U.ptr(o) for o in outs), ld, bs, None, B, heads, Tq, Tk, D,
                                                  D ** -0.5, U.ptr(work), work.numel(), phases)
    assert run(0) == 1 and run(16) == 1 and run(-1) == 1
    torch.cuda.synchronize()
    assert all((o == 7.0).all().item() for o in outs) and (work == 0x5A).all().item()
    for ph in (1, 2, 4, 8):
        assert run(ph) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(o, t[n]) for o, n in zip(outs, ("dq", "dk", "dv"))) and torch.equal(work, t["work"])


def test_peaked_softmax_is_finite():
    c = TT.ATTN_CASES[7]
    rc, t = _raw(c)
    assert rc == 0 and all(torch.isfinite(t[n]).all().item() for n in ("dq", "dk", "dv"))
    assert torch.isfinite(t["work"].view(torch.float32)).all().item()


def test_attention_refusals_launch_nothing():
    c = TT.ATTN_CASES[1]
    B, heads, Tq, Tk, D, _ = c
    Cc = heads * D
    rc, t = _raw(c)
    assert rc == 0
    slot = torch.zeros(B, dtype=torch.int32, device="cuda")
    bad = [dict(D=64), dict(D=512), dict(D=0), dict(slot=U.ptr(slot)), dict(B=0), dict(heads=0), dict(Tq=0), dict(Tk=0), dict(nbytes=0)]
    bad += [{f"bs{i}": 0} for i in range(8)] + [{f"ld{i}": Cc + 2} for i in range(8)] + [{f"ld{i}": Cc - 4} for i in range(8)] + [dict(bs1=Tk * Cc + 2)]
    bad += [{n: None} for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv", "work")]
    for over in bad:
        rc, t = _raw(c, **over)
        assert rc == 1, over
        assert all((t[n] == 7.0).all().item() for n in ("dq", "dk", "dv")) and (t["work"] == 0x5A).all().item(), over
    rc, t = _raw(c)
    for over in (dict(nbytes=t["work"].numel() - 1), dict(work=C.c_void_p(t["work"].data_ptr() + 4), nbytes=t["work"].numel()), dict(q=C.c_void_p(t["q"].data_ptr() + 4)),
                 dict(dv=C.c_void_p(t["dv"].data_ptr() + 8))):
        rc, t2 = _raw(c, **over)
        assert rc == 1, over
        assert all((t2[n] == 7.0).all().item() for n in ("dq", "dk", "dv")) and (t2["work"] == 0x5A).all().item(), over
    with pytest.raises(E.EngineError):          # head_dim 64 has a forward kernel but no backward: refused, not approximated
        T.attention_bwd32(*(torch.zeros(1, 16, 64, device="cuda") for _ in range(8)), 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm, GEGLU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Cc,const", LN_CASES, ids=lambda v: str(v))
def test_layernorm_gradients(rows, Cc, const):
    lib = E.load_library()
    k = TT.ln_case(rows, Cc, const)
    what = f"layernorm {rows}x{Cc}" + (" const" if const else "")
    slabs = TN.ln_slab_rule(rows)[0]                                                                # min(64, ceil(rows / 256)), restated on the host
    assert lib.dm_f32_op_layernorm_bwd_workspace(rows, Cc) == slabs * 2 * Cc * 8 + rows * 8
    assert slabs == {600: 3, 16391: 64}.get(rows, 1)                                                # three row slabs at 600, the cap at 16 391
    x, gamma, beta = (k[n].cuda().requires_grad_() for n in ("x", "gamma", "beta"))
    y = T.layernorm32(x, gamma, beta, 1e-5)
    y.backward(k["dy"].cuda())
    torch.cuda.synchronize()
    r64, r32 = k["r64"], k["r32"]
    TT.check(what + " y", y.detach().cpu(), r64[0], r32[0])
    TT.check(what + " dx", x.grad.cpu(), r64[1], r32[1])
    TT.check(what + " dgamma", gamma.grad.cpu(), r64[2], r32[2])
    TT.check(what + " dbeta", beta.grad.cpu(), r64[3], r32[3])


@pytest.mark.parametrize("M,Fh", TT.GEGLU_CASES)
def test_geglu_gradients(M, Fh):
    k = TT.geglu_case(M, Fh)
    p = k["p"].cuda().requires_grad_()
    y = T.geglu32(p)
    y.backward(k["dy"].cuda())
    torch.cuda.synchronize()
    TT.check(f"geglu {M}x{Fh} y", y.detach().cpu(), k["r64"][0], k["r32"][0])
    TT.check(f"geglu {M}x{Fh} dP", p.grad.cpu(), k["r64"][1], k["r32"][1])


def test_layernorm_and_geglu_refusals():
    lib = E.load_library()
    rows, Cc = 5, 320
    k = TT.ln_case(rows, Cc, False)
    x, dy, gamma = (k[n].cuda() for n in ("x", "dy", "gamma"))
    nbytes = lib.dm_f32_op_layernorm_bwd_workspace(rows, Cc)
    assert nbytes == 2 * Cc * 8 + rows * 8 and lib.dm_f32_op_layernorm_bwd_workspace(0, Cc) == 0 and lib.dm_f32_op_layernorm_bwd_workspace(rows, 0) == 0
    wk = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in ((rows, Cc), (Cc,), (Cc,))]

    def ln(**kw):
        a = dict(x=U.ptr(x), dy=U.ptr(dy), rows=rows, C=Cc, gamma=U.ptr(gamma), work=U.ptr(wk), nbytes=nbytes, dx=U.ptr(outs[0]), dg=U.ptr(outs[1]), db=U.ptr(outs[2]))
        a.update(kw)
        return lib.dm_f32_op_layernorm_bwd(U.stream(), a["x"], a["dy"], a["rows"], a["C"], a["gamma"], 1e-5, a["work"], a["nbytes"], a["dx"], a["dg"], a["db"])
    for kw in (dict(x=None), dict(dy=None), dict(gamma=None), dict(work=None), dict(dx=None), dict(dg=None), dict(db=None), dict(rows=0), dict(C=0),
               dict(nbytes=nbytes - 1), dict(work=C.c_void_p(wk.data_ptr() + 4))):
        assert ln(**kw) == 1, kw
    torch.cuda.synchronize()
    assert all((t == 7.0).all().item() for t in outs) and not wk.any().item()
    assert ln() == 0
    p, d = TT.randn(4, 16, seed=97).cuda(), TT.randn(4, 8, seed=98).cuda()
    v, v2 = torch.full((4, 8), 7.0, device="cuda"), torch.full((4, 16), 7.0, device="cuda")
    assert lib.dm_f32_op_geglu(U.stream(), None, 4, 8, U.ptr(v)) == 1 and lib.dm_f32_op_geglu(U.stream(), U.ptr(p), 4, 8, None) == 1
    assert lib.dm_f32_op_geglu(U.stream(), U.ptr(p), 0, 8, U.ptr(v)) == 1 and lib.dm_f32_op_geglu(U.stream(), U.ptr(p), 4, 0, U.ptr(v)) == 1
    assert lib.dm_f32_op_geglu(U.stream(), U.ptr(p), 8, 6, U.ptr(v)) == 1          # F % 4
    assert lib.dm_f32_op_geglu_bwd(U.stream(), None, U.ptr(d), 4, 8, U.ptr(v2)) == 1 and lib.dm_f32_op_geglu_bwd(U.stream(), U.ptr(p), None, 4, 8, U.ptr(v2)) == 1
    assert lib.dm_f32_op_geglu_bwd(U.stream(), U.ptr(p), U.ptr(d), 4, 8, None) == 1 and lib.dm_f32_op_geglu_bwd(U.stream(), U.ptr(p), U.ptr(d), 4, 6, U.ptr(v2)) == 1
    assert lib.dm_f32_op_geglu_bwd(U.stream(), U.ptr(p), U.ptr(d), 0, 8, U.ptr(v2)) == 1
    torch.cuda.synchronize()
    assert (v == 7.0).all().item() and (v2 == 7.0).all().item()
