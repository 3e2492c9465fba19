"""Guard bands around every operand of the transformer half's gradient entries (tests/test_gpu_guards.py run3: a plain run, then all
device operands — workspaces included — inside one allocation between guards filled with 0xFF, then 0x00): the guards and the inputs come
back untouched, and the three results are equal bit for bit, so no load outside a tensor (or of workspace the call did not write) reaches a
result.  Shapes: the ragged cases of tests/test_gpu_train_tfm_ops.py, and the Tq = 8200 cross-attention of tests/train_net_cases.py (sixteen
query slabs, the fifteenth ragged, the sixteenth empty: its zero partials are part of the compared workspace); the plain result is checked
against float64 here too."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import train_net_cases as TN  # noqa: E402
from tests import train_tfm_cases as TT  # noqa: E402
from tests.test_gpu_guards import run3  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


@pytest.mark.parametrize("c", [TT.ATTN_CASES[0], TT.ATTN_CASES[1], TT.ATTN_CASES[2], TT.ATTN_CASES[4], TT.ATTN_CASES[5], TT.ATTN_CASES[6],
                               TN.ATTN_EMPTY_SLAB], ids=TT.attn_id)
def test_attention_forward_and_backward(c):
    """self-attention on stacked q|k|v rows with a stacked gradient, cross-attention on q and stacked k|v: the strided views end exactly at
    the tensors' ends, so a read or write past a row's head slice lands in a guard"""
    lib = E.load_library()
    B, heads, Tq, Tk, D, _ = c
    k = TT.attn_case(*c)
    Cc = heads * D
    self_attn = Tq == Tk
    nbytes = lib.dm_f32_op_attention_bwd_workspace(B, heads, Tq, Tk, D)
    assert nbytes > 0 and nbytes % 4 == 0
    if c == TN.ATTN_EMPTY_SLAB:
        assert nbytes == 4 * (2 * Tq + 16 * Tk * 2 * D) and TN.attn_slab_rule(Tq, Tk)[2][14:] == [136, 0]
    if self_attn:
        inputs = {"qkv": torch.cat([k["q"], k["k"], k["v"]], dim=-1), "do": k["do"]}
        outputs = {"o": ((B, Tq, Cc), F32), "dqkv": ((B, Tq, 3 * Cc), F32), "work": ((nbytes // 4,), F32)}
    else:
        inputs = {"q": k["q"], "kv": torch.cat([k["k"], k["v"]], dim=-1), "do": k["do"]}
        outputs = {"o": ((B, Tq, Cc), F32), "dq": ((B, Tq, Cc), F32), "dkv": ((B, Tk, 2 * Cc), F32), "work": ((nbytes // 4,), F32)}

    def at(t, off):
        return C.c_void_p(t.data_ptr() + 4 * off)

    def launch(v):
        if self_attn:
            q, kk, vv, dq, dk, dv = at(v["qkv"], 0), at(v["qkv"], Cc), at(v["qkv"], 2 * Cc), at(v["dqkv"], 0), at(v["dqkv"], Cc), at(v["dqkv"], 2 * Cc)
            lq = lkv = ldq = ldkv = 3 * Cc
        else:
            q, kk, vv, dq, dk, dv = at(v["q"], 0), at(v["kv"], 0), at(v["kv"], Cc), at(v["dq"], 0), at(v["dkv"], 0), at(v["dkv"], Cc)
            lq, lkv, ldq, ldkv = Cc, 2 * Cc, Cc, 2 * Cc
        assert lib.dm_f32_op_attention(U.stream(), q, kk, vv, U.ptr(v["o"]), lq, lkv, lkv, Cc, Tq * lq, Tk * lkv, Tk * lkv, Tq * Cc, None, 0, B, heads, Tq, Tk, D,
                                       D ** -0.5) == 0
        ld = [lq, lkv, lkv, Cc, Cc, ldq, ldkv, ldkv]
        bs = [Tq * lq, Tk * lkv, Tk * lkv, Tq * Cc, Tq * Cc, Tq * ldq, Tk * ldkv, Tk * ldkv]
        assert lib.dm_f32_op_attention_bwd(U.stream(), q, kk, vv, U.ptr(v["o"]), U.ptr(v["do"]), dq, dk, dv, (C.c_int32 * 8)(*ld), (C.c_int64 * 8)(*bs), None, B, heads,
                                           Tq, Tk, D, D ** -0.5, U.ptr(v["work"]), nbytes) == 0
    whole = 2 * B * heads * Tq % 4 == 0          # otherwise 8 bytes of padding behind the statistics stay unwritten: the workspace is not compared
    out = run3(f"attention_bwd {TT.attn_id(c)}", inputs, outputs, launch, work=() if whole else ("work",))
    r64, r32 = k["r64"], k["r32"]
    if self_attn:
        dq, dk, dv = out["dqkv"][..., :Cc], out["dqkv"][..., Cc:2 * Cc], out["dqkv"][..., 2 * Cc:]
    else:
        dq, dk, dv = out["dq"], out["dkv"][..., :Cc], out["dkv"][..., Cc:]
    what = f"guarded attention {TT.attn_id(c)}"
    TT.check(what + " dq", dq.cpu(), r64[1], r32[1], TT.TOL_E2E)
    TT.check(what + " dk", dk.cpu(), r64[2], r32[2], TT.TOL_E2E)
    TT.check(what + " dv", dv.cpu(), r64[3], r32[3], TT.TOL_E2E)


@pytest.mark.parametrize("rows,Cc,const", [TT.LN_CASES[0], TT.LN_CASES[1], TT.LN_CASES[3], TT.LN_CASES[4]], ids=lambda v: str(v))
def test_layernorm_backward(rows, Cc, const):
    lib = E.load_library()
    k = TT.ln_case(rows, Cc, const)
    nbytes = lib.dm_f32_op_layernorm_bwd_workspace(rows, Cc)
    assert nbytes > 0 and nbytes % 8 == 0

    def launch(v):
        assert lib.dm_f32_op_layernorm(U.stream(), U.ptr(v["x"]), rows, Cc, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1e-5, U.ptr(v["y"])) == 0
        assert lib.dm_f32_op_layernorm_bwd(U.stream(), U.ptr(v["x"]), U.ptr(v["dy"]), rows, Cc, U.ptr(v["gamma"]), 1e-5, U.ptr(v["work"]), nbytes, U.ptr(v["dx"]),
                                           U.ptr(v["dgamma"]), U.ptr(v["dbeta"])) == 0
    out = run3(f"layernorm_bwd {rows}x{Cc}", {n: k[n] for n in ("x", "dy", "gamma", "beta")},
               {"y": ((rows, Cc), F32), "work": ((nbytes // 8,), F64), "dx": ((rows, Cc), F32), "dgamma": ((Cc,), F32), "dbeta": ((Cc,), F32)},
               launch)          # the workspace is written in full: compared too
    r64, r32 = k["r64"], k["r32"]
    TT.check("guarded layernorm_bwd dx", out["dx"].cpu(), r64[1], r32[1])
    TT.check("guarded layernorm_bwd dgamma", out["dgamma"].cpu(), r64[2], r32[2])
    TT.check("guarded layernorm_bwd dbeta", out["dbeta"].cpu(), r64[3], r32[3])


@pytest.mark.parametrize("M,Fh", TT.GEGLU_CASES)
def test_geglu(M, Fh):
    lib = E.load_library()
    k = TT.geglu_case(M, Fh)

    def launch(v):
        assert lib.dm_f32_op_geglu(U.stream(), U.ptr(v["p"]), M, Fh, U.ptr(v["y"])) == 0
        assert lib.dm_f32_op_geglu_bwd(U.stream(), U.ptr(v["p"]), U.ptr(v["dy"]), M, Fh, U.ptr(v["dp"])) == 0
    out = run3(f"geglu {M}x{Fh}", {"p": k["p"], "dy": k["dy"]}, {"y": ((M, Fh), F32), "dp": ((M, 2 * Fh), F32)}, launch)
    TT.check("guarded geglu y", out["y"].cpu(), k["r64"][0], k["r32"][0])
    TT.check("guarded geglu dP", out["dp"].cpu(), k["r64"][1], k["r32"][1])
