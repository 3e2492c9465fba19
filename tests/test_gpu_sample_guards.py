"""Guard-band runs of the kernels text-to-image sampling adds (tests/gpu_util.Guarded): the latent prologue, the decoder's tail at a ragged
size and the guided step at an element count that is no multiple of the block.  Every operand lies in one allocation between guard tiles; a
guarded run must leave guards and inputs untouched and give the same bytes under the 0xFF and the 0x00 fill and as the plain run."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import sample as S  # noqa: E402
from tests import sample_ref as SR  # noqa: E402
from tests.gpu_util import Guarded, dev, pack_conv3, to_nhwc  # noqa: E402

FILLS = (0xFF, 0x00)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def _at(g, name, byte_offset=0):
    return C.c_void_p(g.offset(name) + byte_offset)


def _p(t):
    return C.c_void_p(t.data_ptr())


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


def test_guided_step_at_a_ragged_element_count():
    lib = E.load_library()
    n = 4 * 256 + 37
    x, eps = _randn(n, seed=1) * 1.7, (_randn(2 * n, seed=2) * 1.2).half()
    row = S.sample_coefficients(S.sample_timesteps(50))[25]
    ins = {"x": x, "eps": eps, "coef": torch.from_numpy(row.copy())}
    got = _both_fills(ins, {"out": ((n,), torch.float32)},
                      lambda g: lib.dm_op_cfg_ddim_step(_stream(), _at(g, "x"), _at(g, "eps"), _at(g, "coef"), 7.5, n, _at(g, "out")), ["out"])
    assert torch.equal(got["out"], SR.table_update(x, eps, row, 7.5))
    xd, ed, cd = x.to(dev()), eps.to(dev()), torch.from_numpy(row.copy()).to(dev())
    plain = torch.empty_like(xd)
    assert lib.dm_op_cfg_ddim_step(_stream(), _p(xd), _p(ed), _p(cd), 7.5, n, _p(plain)) == 0
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu(), got["out"])


@pytest.mark.parametrize("B,h,w,ldc", [(2, 5, 7, 64), (1, 17, 16, 8)])
def test_latent_prologue(B, h, w, ldc):
    """35 and 272 pixels per sample (one ragged block, one block and a ragged one); 64-channel rows as the decoder uses them and the
    narrowest row.  Against torch op by op: the fp32 quotient, its fp16 rounding, the four exact products added in order, the bias."""
    lib = E.load_library()
    HW = h * w
    lat = _randn(B, 4, h, w, seed=h) * 1.1
    wq, bq = (_randn(4, 4, seed=3) * 0.5).half(), (_randn(4, seed=4) * 0.1).half()
    sf = np.float32(0.18215)
    ins = {"lat": lat, "w": wq, "b": bq}
    call = lambda g: lib.dm_op_latent_prologue(_stream(), _at(g, "lat"), _at(g, "w"), _at(g, "b"), B, HW, float(sf), _at(g, "out"), ldc)      # noqa: E731
    got = _both_fills(ins, {"out": ((B * HW, ldc), torch.float16)}, call, ["out"])["out"]
    z = (lat / torch.tensor(sf)).half().float()                               # [B,4,h,w]
    acc = torch.zeros(B, 4, h, w)
    for i in range(4):
        acc = acc + wq.float()[:, i].view(1, 4, 1, 1) * z[:, i:i + 1]
    want = (acc + bq.float().view(1, 4, 1, 1)).half().permute(0, 2, 3, 1).reshape(B * HW, 4)
    assert torch.equal(got[:, :4], want)
    assert (got[:, 4:] == 0).all()
    ld, wd, bd = lat.to(dev()), wq.to(dev()), bq.to(dev())
    plain = torch.full((B * HW, ldc), 3.0, dtype=torch.float16, device=dev())
    assert lib.dm_op_latent_prologue(_stream(), _p(ld), _p(wd), _p(bd), B, HW, float(sf), _p(plain), ldc) == 0
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu(), got)
    # refused, not launched: a row pitch that is no multiple of 8, a non-positive scaling factor, a null pointer
    for bad in (lambda: lib.dm_op_latent_prologue(_stream(), _p(ld), _p(wd), _p(bd), B, HW, float(sf), _p(plain), 4),
                lambda: lib.dm_op_latent_prologue(_stream(), _p(ld), _p(wd), _p(bd), B, HW, 0.0, _p(plain), ldc),
                lambda: lib.dm_op_latent_prologue(_stream(), None, _p(wd), _p(bd), B, HW, float(sf), _p(plain), ldc)):
        assert bad() != 0
    torch.cuda.synchronize()
    assert torch.equal(plain.cpu(), got)


@pytest.mark.parametrize("B,H,W", [(1, 17, 9), (2, 8, 16)])
def test_decoder_tail(B, H, W):
    """ragged last tiles in both directions behind full ones, and exactly one tile per sample"""
    lib = E.load_library()
    Cc = 128
    x = (_randn(B, Cc, H, W, seed=H * 10 + W) * 1.3 + 0.2).half()
    gamma, beta = 1 + 0.1 * _randn(Cc, seed=6), 0.05 * _randn(Cc, seed=7)
    w, b = (_randn(3, Cc, 3, 3, seed=8) * (9 * Cc) ** -0.5).half(), (0.3 * _randn(3, seed=9)).half()
    nbytes = lib.dm_op_decoder_tail_workspace_bytes(B, H, W)
    ins = {"x": to_nhwc(x), "gamma": gamma, "beta": beta, "w": pack_conv3(w), "b": b}
    outs = {"work": ((nbytes,), torch.uint8), "raw": ((B, 3, H, W), torch.float16), "u8": ((B, H, W, 3), torch.uint8),
            "raw_only": ((B, 3, H, W), torch.float16), "u8_only": ((B, H, W, 3), torch.uint8)}

    def call(g):
        args = (_stream(), _at(g, "x"), _at(g, "gamma"), _at(g, "beta"), _at(g, "w"), _at(g, "b"), B, H, W, 1e-6, _at(g, "work"), nbytes)
        if lib.dm_op_decoder_tail(*args, _at(g, "raw"), _at(g, "u8")):
            return 1
        if lib.dm_op_decoder_tail(*args, _at(g, "raw_only"), None):
            return 1
        return lib.dm_op_decoder_tail(*args, None, _at(g, "u8_only"))
    got = _both_fills(ins, outs, call, ["raw", "u8", "raw_only", "u8_only"])
    assert torch.isfinite(got["raw"]).all()
    assert torch.equal(got["raw"], got["raw_only"]) and torch.equal(got["u8"], got["u8_only"])
    assert np.array_equal(got["u8"].numpy(), SR.postprocess_pil(got["raw"]))
    d = {k: v.to(dev()) for k, v in ins.items()}
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    raw = torch.empty(B, 3, H, W, dtype=torch.float16, device=dev())
    assert lib.dm_op_decoder_tail(_stream(), _p(d["x"]), _p(d["gamma"]), _p(d["beta"]), _p(d["w"]), _p(d["b"]), B, H, W, 1e-6, _p(work), nbytes,
                                  _p(raw), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.cpu(), got["raw"])
