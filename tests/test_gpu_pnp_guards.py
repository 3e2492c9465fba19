"""Guard-band runs of the kernels the parallel-dataset generator adds (tests/gpu_util.Guarded): the two DDIM update kernels at an element
count that is no multiple of the block, the decoder's tail at a full tile and at ragged tiles, the broadcast add of the feature injection,
and the attention with zero Q / K batch strides (the self-attention injection).  Every operand lies in one allocation between guard tiles; a
guarded run must leave guards and inputs untouched and give the same bytes under the 0xFF and the 0x00 fill."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from tests.gpu_util import Guarded, dev, pack_conv3, to_nhwc  # noqa: E402

FILLS = (0xFF, 0x00)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def _at(g, name, byte_offset=0):
    return C.c_void_p(g.offset(name) + byte_offset)


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _both_fills(inputs, outputs, call, keep):
    got = {}
    for fill in FILLS:
        g = Guarded(inputs, outputs, fill=fill, device=dev())
        with torch.cuda.device(dev()):
            assert call(g) == 0
            torch.cuda.synchronize()
        g.check()
        got[fill] = {k: g.view(k).cpu() for k in keep}
    for k in keep:
        assert torch.equal(got[0xFF][k].view(torch.uint8), got[0x00][k].view(torch.uint8)), k
    return got[0xFF]


def test_update_kernels_at_a_ragged_element_count():
    lib = E.load_library()
    n = 4 * 256 + 37
    x, eu, ec = _randn(n, seed=1), _randn(n, seed=2), _randn(n, seed=3)
    coef = torch.tensor([0.9, 0.3, 0.95, 0.2])
    ins = {"x": x, "eu": eu, "ec": ec, "coef": coef}
    got = _both_fills(ins, {"out": ((n,), torch.float32)},
                      lambda g: lib.dm_f32_op_ddim_step(_stream(), _at(g, "x"), _at(g, "eu"), _at(g, "coef"), n, _at(g, "out")), ["out"])
    c0, c1, c2, c3 = coef.unbind()
    assert torch.equal(got["out"], c0 * ((x - c1 * eu) / c2) + c3 * eu)
    got = _both_fills(ins, {"out": ((n,), torch.float32)},
                      lambda g: lib.dm_f32_op_ddim_step_cfg(_stream(), _at(g, "x"), _at(g, "eu"), _at(g, "ec"), 7.5, _at(g, "coef"), n, _at(g, "out")),
                      ["out"])
    eps = eu + 7.5 * (ec - eu)
    assert torch.equal(got["out"], c0 * ((x - c1 * eps) / c2) + c3 * eps)


def test_broadcast_add():
    lib = E.load_library()
    B, per = 5, 4 * 333
    r, h = _randn(B, per, seed=4), _randn(per, seed=5)
    got = _both_fills({"r": r, "h": h}, {"y": ((B, per), torch.float32)},
                      lambda g: lib.dm_f32_op_bcast_add(_stream(), _at(g, "r"), _at(g, "h"), B, per, _at(g, "y")), ["y"])
    assert torch.equal(got["y"], r + h[None])


@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (1, 5, 7), (1, 17, 9)])
def test_decoder_tail(B, H, W):
    """a full 8 x 8 tile, one ragged tile, and ragged last tiles in both directions behind full ones; against torch in float64 at the
    operator tolerance of tests/test_gpu_f32.py (2e-6: fp32 on both sides, summation order)"""
    lib = E.load_library()
    Cc, G = 128, 32
    x = _randn(B, Cc, H, W, seed=H * 10 + W) * 1.3 + 0.2
    gamma, beta = 1 + 0.1 * _randn(Cc, seed=6), 0.05 * _randn(Cc, seed=7)
    w, b = _randn(3, Cc, 3, 3, seed=8) * (9 * Cc) ** -0.5, 0.3 * _randn(3, seed=9)
    ins = {"x": to_nhwc(x), "gamma": gamma, "beta": beta, "w": pack_conv3(w), "b": b}
    outs = {"stats": ((B * G, 2), torch.float32), "norm": ((B, H, W, Cc), torch.float32), "raw": ((B, 3, H, W), torch.float32),
            "img": ((B, 3, H, W), torch.float32), "u8": ((B, H, W, 3), torch.uint8)}

    def call(g):
        if lib.dm_f32_op_groupnorm(_stream(), _at(g, "x"), None, B, H * W, Cc, Cc, G, 1e-6, _at(g, "gamma"), _at(g, "beta"), 1, _at(g, "stats"),
                                   _at(g, "norm")):
            return 1
        if lib.dm_f32_op_decoder_tail(_stream(), _at(g, "x"), _at(g, "stats"), _at(g, "gamma"), _at(g, "beta"), _at(g, "w"), _at(g, "b"), B, H, W, Cc, 1,
                                      _at(g, "raw"), None):
            return 1
        return lib.dm_f32_op_decoder_tail(_stream(), _at(g, "x"), _at(g, "stats"), _at(g, "gamma"), _at(g, "beta"), _at(g, "w"), _at(g, "b"), B, H, W, Cc,
                                          0, _at(g, "img"), _at(g, "u8"))
    got = _both_fills(ins, outs, call, ["raw", "img", "u8", "norm"])
    assert torch.isfinite(got["raw"]).all()
    ref = F.conv2d(F.silu(F.group_norm(x.double(), G, gamma.double(), beta.double(), 1e-6)), w.double(), b.double(), padding=1)
    r = ((got["raw"].double() - ref).norm() / ref.norm()).item()
    print(f"decoder tail {B}x{H}x{W}: rel-L2 {r:.2e}")
    assert r < 2e-6
    want = (got["raw"] / 2 + 0.5).clamp(0, 1)
    assert torch.equal(got["img"], want)
    assert torch.equal(got["u8"], (want.permute(0, 2, 3, 1) * 255).to(torch.uint8))
    # the fused load is the two-kernel path's GroupNorm + SiLU: a convolution of that tensor by torch agrees as closely
    two = F.conv2d(got["norm"].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)
    assert ((got["raw"].double() - two).norm() / two.norm()).item() < 2e-6
    assert lib.dm_f32_op_decoder_tail(_stream(), None, None, None, None, None, None, B, H, W, 64, 1, None, None) != 0      # refused, not launched


@pytest.mark.parametrize("T", [4, 64])
def test_attention_with_the_sources_queries_and_keys(T):
    """batch strides of 0 for Q and K, the samples' own V: what a masked attn1 runs.  Equal to the ordinary call on a batch whose Q and K
    rows were copied from sample 0, bit for bit."""
    lib = E.load_library()
    B, heads, D = 3, 8, 40
    Cc = heads * D
    qkv = _randn(B, T, 3 * Cc, seed=T)

    def call_with(bsq, bsk):
        return lambda g: lib.dm_f32_op_attention(_stream(), _at(g, "qkv"), _at(g, "qkv", 4 * Cc), _at(g, "qkv", 8 * Cc), _at(g, "o"), 3 * Cc, 3 * Cc,
                                                 3 * Cc, Cc, bsq, bsk, T * 3 * Cc, T * Cc, None, 0, B, heads, T, T, D, float(D) ** -0.5)
    got = _both_fills({"qkv": qkv}, {"o": ((B, T, Cc), torch.float32)}, call_with(0, 0), ["o"])
    copied = qkv.clone()
    copied[:, :, :2 * Cc] = qkv[:1, :, :2 * Cc]
    ref = _both_fills({"qkv": copied}, {"o": ((B, T, Cc), torch.float32)}, call_with(T * 3 * Cc, T * 3 * Cc), ["o"])
    assert torch.isfinite(got["o"]).all() and torch.equal(got["o"], ref["o"])
    q, k, v = (copied[..., i * Cc:(i + 1) * Cc].reshape(B, T, heads, D).transpose(1, 2).double() for i in range(3))
    want = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, dim=-1) @ v).transpose(1, 2).reshape(B, T, Cc)
    assert ((got["o"].double() - want).norm() / want.norm()).item() < 2e-6
