"""Guard-band runs of the kernels the configurable CLIP image tower adds (tests/gpu_util.Guarded): the head_dim-64 flash attention at
the tower's 577 tokens, the preprocessing that writes the 608-wide patch rows, and the patch-token head's LayerNorm.  Every operand
lies in one allocation between guard tiles; a guarded run must leave guards and inputs untouched, give the same bytes under the
0xFF and the 0x00 fill, and the bytes of the plain run."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import clip_spec as S  # noqa: E402
from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import resample as RS  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402

TEST_CFG = S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=336, patch_size=14,
                              projection_dim=64)
FILLS = (0xFF, 0x00)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def _at(g, name, byte_offset=0):
    return C.c_void_p(g.offset(name) + byte_offset)


def test_attention_head_dim_64_at_577_tokens():
    lib = E.load_library()
    B, heads, D, T = 2, 2, 64, 577
    Cc = heads * D
    qkv = torch.randn(B, T, 3 * Cc, generator=torch.Generator().manual_seed(577))
    got = {}
    for fill in FILLS:
        g = Guarded({"qkv": qkv}, {"o": ((B, T, Cc), torch.float32)}, fill=fill, device=dev())
        with torch.cuda.device(dev()):
            rc = lib.dm_f32_op_attention(_stream(), _at(g, "qkv"), _at(g, "qkv", 4 * Cc), _at(g, "qkv", 8 * Cc), _at(g, "o"), 3 * Cc, 3 * Cc,
                                         3 * Cc, Cc, T * 3 * Cc, T * 3 * Cc, T * 3 * Cc, T * Cc, None, 0, B, heads, T, T, D, 0.125)
            assert rc == 0
            torch.cuda.synchronize()
        g.check()
        got[fill] = g.view("o").cpu()
        assert torch.isfinite(got[fill]).all()
    assert torch.equal(got[0xFF], got[0x00])
    X = qkv.to(dev())
    O = torch.empty(B, T, Cc, device=dev())
    p = X.data_ptr()
    with torch.cuda.device(dev()):
        assert lib.dm_f32_op_attention(_stream(), C.c_void_p(p), C.c_void_p(p + 4 * Cc), C.c_void_p(p + 8 * Cc), C.c_void_p(O.data_ptr()), 3 * Cc,
                                       3 * Cc, 3 * Cc, Cc, T * 3 * Cc, T * 3 * Cc, T * 3 * Cc, T * Cc, None, 0, B, heads, T, T, D, 0.125) == 0
        torch.cuda.synchronize()
    assert torch.equal(O.cpu(), got[0xFF])


def _host_patch_rows(img, size=336, patch=14, kpad=608):
    """The patch rows the preprocessing must write: row = patch (py * G + px), k = (c, ky, kx), zeros from 3 * patch^2 on."""
    pv = RS.clip_tower_preprocess_numpy(img, size)                                       # [3, S, S]
    G = size // patch
    rows = pv.reshape(3, G, patch, G, patch).transpose(1, 3, 0, 2, 4).reshape(G * G, 3 * patch * patch)
    out = np.zeros((G * G, kpad), np.float32)
    out[:, :rows.shape[1]] = rows
    return out


def test_preprocess_writes_the_608_wide_patch_rows():
    e = E.UNetEngineF32(0)
    try:
        e.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, TEST_CFG), TEST_CFG)
        rng = np.random.default_rng(14)
        imgs = [rng.integers(0, 256, (s, s, 3), dtype=np.uint8) for s in (350, 336, 120)]          # a downscale, no pass at all, an upscale
        desc, tables = RS.clip_tower_plan(imgs, 336)
        ins = {"images": torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])), "desc": torch.from_numpy(desc.view(np.uint8).copy()),
               "tables": torch.from_numpy(tables.copy())}
        n, rows_per, kpad = len(imgs), 576, 608
        got = {}
        for fill in FILLS:
            g = Guarded(ins, {"rows": ((n * rows_per, kpad), torch.float32)}, fill=fill, device=dev())
            with torch.cuda.device(dev()):
                rc = e.lib.dm_f32_clip_tower_preprocess(e._h, _at(g, "images"), _at(g, "desc"), _at(g, "tables"), n, 1, _at(g, "rows"), _stream())
                assert rc == 0, e.lib.dm_f32_last_error(e._h)
                torch.cuda.synchronize()
            g.check()
            got[fill] = g.view("rows").cpu().numpy()
        # the zero columns 588..607 are the kernel's own stores: under the 0xFF fill they would read NaN otherwise
        assert (got[0xFF][:, 588:] == 0).all() and np.array_equal(got[0xFF].view(np.uint32), got[0x00].view(np.uint32))
        ref = np.concatenate([_host_patch_rows(a) for a in imgs])
        assert np.array_equal(got[0xFF].view(np.uint32), ref.view(np.uint32))
        # the plain run (ordinary allocations), and the pixel_values layout of the same images
        d = {k: v.to(dev()) for k, v in ins.items()}
        out = torch.empty(n * rows_per, kpad, device=dev())
        with torch.cuda.device(dev()):
            assert e.lib.dm_f32_clip_tower_preprocess(e._h, C.c_void_p(d["images"].data_ptr()), C.c_void_p(d["desc"].data_ptr()),
                                                      C.c_void_p(d["tables"].data_ptr()), n, 1, C.c_void_p(out.data_ptr()), _stream()) == 0
            torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), got[0xFF].view(np.uint32))
        pv = e.clip_tower_preprocess(imgs).cpu().numpy()
        for i, a in enumerate(imgs):
            assert np.array_equal(pv[i], RS.clip_tower_preprocess_numpy(a, 336))
    finally:
        e.close()


def test_patch_token_head_layernorm():
    lib = E.load_library()
    n, T, Cc = 2, 577, 128
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, T, Cc, generator=gen) * 1.5 - 0.2
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=gen), 0.05 * torch.randn(Cc, generator=gen)
    got = {}
    for fill in FILLS:
        g = Guarded({"x": x, "gamma": gamma, "beta": beta}, {"y": ((n * (T - 1), Cc), torch.float32)}, fill=fill, device=dev())
        with torch.cuda.device(dev()):
            assert lib.dm_f32_op_clip_patch_ln(_stream(), _at(g, "x"), n, T, Cc, _at(g, "gamma"), _at(g, "beta"), 1e-5, _at(g, "y")) == 0
            torch.cuda.synchronize()
        g.check()
        got[fill] = g.view("y").cpu()
        assert torch.isfinite(got[fill]).all()
    assert torch.equal(got[0xFF], got[0x00])
    X, G, Bt = x.to(dev()), gamma.to(dev()), beta.to(dev())
    Y = torch.empty(n * (T - 1), Cc, device=dev())
    with torch.cuda.device(dev()):
        assert lib.dm_f32_op_clip_patch_ln(_stream(), C.c_void_p(X.data_ptr()), n, T, Cc, C.c_void_p(G.data_ptr()), C.c_void_p(Bt.data_ptr()), 1e-5,
                                           C.c_void_p(Y.data_ptr())) == 0
        torch.cuda.synchronize()
    assert torch.equal(Y.cpu(), got[0xFF])
    ref = torch.nn.functional.layer_norm(x[:, 1:, :].double().reshape(-1, Cc), (Cc,), gamma.double(), beta.double(), 1e-5)
    assert ((got[0xFF].double() - ref).norm() / ref.norm()).item() < 2e-6
