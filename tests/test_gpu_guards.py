"""Guard bands around every operand of the operator entries: accesses OUTSIDE a tensor.

The parity tests give every operand its own allocation, 512-byte aligned inside the caching allocator's segments: a ragged last tile
that stores past row M, a 3x3 tap that reads pixel (-1, .) of sample 0, a split-K part that spills over its workspace all land in
slack nobody looks at.  Here every entry runs three times — plain (separate allocations, as its parity test calls it), and twice
with ALL device operands inside one allocation (tests/gpu_util.py: Guarded), every tensor between guards of at least one 256-row
tile (>= 64 KiB), payloads at odd multiples of 256 bytes, guards and outputs pre-filled with 0xFF (NaN / -1), then with 0x00:

  1. the guards and the inputs come back untouched (Guarded.check);
  2. the three results are equal bit for bit: a load outside a tensor that reaches a result makes it depend on the fill;
  3. the plain result meets the entry's reference at the tolerance of its parity test;
  4. the kernel the case names is the one that ran (route queries, asserted before the launches).

Shapes: the smallest of the parity tests with a ragged last row tile.  Out of reach: an overrun longer than the guard, and a stray
load whose value is discarded."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from diff_mining_amd import clustering as CL  # noqa: E402
from diff_mining_amd import engine as E  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import kmeans_cases as KC  # noqa: E402

F16, F32, I32, U8 = torch.float16, torch.float32, torch.int32, torch.uint8
FILLS = (0xFF, 0x00)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def run3(what, inputs, outputs, launch, work=()):
    """launch(v) with v = {name: device tensor}: plain, then guarded under both fills.  Names in `work` are workspaces: guarded and
    pre-filled like outputs, but not compared (a workspace may keep unwritten bytes).  Returns the plain run's outputs."""
    d = U.dev()
    plain = {k: t.contiguous().to(d) for k, t in inputs.items()}
    plain.update({k: torch.empty(tuple(s), dtype=dt, device=d) for k, (s, dt) in outputs.items()})
    launch(plain)
    torch.cuda.synchronize()
    compared = [k for k in outputs if k not in work]
    for fill in FILLS:
        g = U.Guarded(inputs, outputs, fill=fill, device=d)
        if fill == FILLS[0]:
            print(f"{what}: " + ", ".join(f"{k}{list(L[4])} guard {g.guard_bytes[k][0]}+{g.guard_bytes[k][1]} B" for k, L in g.layout.items()))
        assert all(g.offset(k) % 512 == 256 for k in g.layout)
        launch(g.views())
        torch.cuda.synchronize()
        g.check()
        for k in compared:
            a, b = _bits(plain[k]), _bits(g.view(k))
            assert torch.equal(a, b), f"{what}: output {k} under guard fill {fill:#04x} differs from the plain run in {(a != b).sum().item()} elements"
    return {k: plain[k] for k in outputs}


def _lib():
    return E.load_library()


class _options:
    """dm_set_option inside try / finally: set on entry, the defaults back on exit"""
    DEFAULTS = {"igemm_big": -1, "igemm_tail": 1, "igemm_splitk": 1, "tap_reuse": 1, "attn_pipe": 1, "attn_cross": 1, "conv_out_rows": 1}

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        try:
            for k, v in self.kw.items():
                assert _lib().dm_set_option(k.encode(), v) == 0, k
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            _lib().dm_set_option(k.encode(), self.DEFAULTS[k])
        return False


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp16 igemm family
# ---------------------------------------------------------------------------------------------------------------------------------------
def _conv_ref(xs, w, b, mode, OH, OW):
    """xs [n,Cin,H,W] fp32, w [Cout,Cin,3,3] or [Cout,Cin] -> [n,Cout,OH,OW] fp32: the layer's definition, as the parity tests state it"""
    if mode == 0:
        return F.conv2d(xs, w.float()[:, :, None, None], b)
    if mode == 1:
        return F.conv2d(xs, w.float(), b, padding=1)
    if mode == 2:
        return F.conv2d(xs, w.float(), b, stride=2, padding=1)
    if mode == 3:
        return F.conv2d(F.interpolate(xs, size=(OH, OW), mode="nearest"), w.float(), b, padding=1)
    return F.conv2d(F.pad(xs, (0, 1, 0, 1)), w.float(), b, stride=2, padding=0)


def igemm_case(what, N, H, W, C1, C2, Cout, mode=0, OH=None, OW=None, variants=("plain",), geglu=False, tile=None, head=None,
               samples=None, opts=None):
    """dm_op_igemm on [N,H,W,C1 (+C2)] -> [N,OH,OW,Cout]; one launch per variant ("plain", "res", "temb", "temb_strided": the table
    [:, 160:] of a wider one) against F.conv2d / F.linear in fp32 (test_igemm_dense_bias_residual, test_igemm_conv3x3,
    test_igemm_geglu).  tile: the dm_op_igemm_tile the case is about; head: a predicate on dm_op_igemm_head_rows."""
    lib = _lib()
    Cin = C1 + C2
    OH, OW = (H, W) if OH is None else (OH, OW)
    M = N * (H * W if mode == 0 else OH * OW)
    x = U.f16_randn(N, H, W, Cin, seed=5)
    x1, x2 = x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None)
    if mode == 0:
        w = U.f16_randn(8 * Cin if geglu else Cout, Cin, seed=6, scale=Cin ** -0.5)
    else:
        w = U.f16_randn(Cout, Cin, 3, 3, seed=6, scale=(9 * Cin) ** -0.5)
    b = U.f16_randn(w.shape[0], seed=7, scale=0.1)
    wp, bp = (U.pack_geglu(w, b) if geglu else ((w if mode == 0 else U.pack_conv3(w)), b))
    cy = w.shape[0] // 2 if geglu else Cout
    sh_out = (N, H, W, cy) if mode == 0 else (N, OH, OW, cy)
    temb = U.f16_randn(N, Cout + 160, seed=8)
    res = U.f16_randn(*sh_out, seed=9)
    sel = list(range(N)) if samples is None else sorted(set(samples))
    ref = _conv_ref(U.to_nchw(x[sel].float()), w, b.float(), mode, OH, OW)          # [n, Cout(x2), OH, OW]
    got = {}                                     # variant -> (its inputs on the device, the plain run's output)
    with _options(**(opts or {})):
        if tile is not None:
            assert lib.dm_op_igemm_tile(M, Cin, w.shape[0], mode) == tile, f"{what}: not on the {'256 x 320' if tile else '128-row'} tile"
        if head is not None:
            hr = lib.dm_op_igemm_head_rows(M, (OH * OW) if mode else M, Cin, w.shape[0], mode)
            assert head(hr, M), f"{what}: head rows {hr} of {M}"
        for var in variants:
            inputs = {"x": x1, "w": wp, "bias": bp}
            if x2 is not None:
                inputs["x2"] = x2
            if var.startswith("temb"):
                assert mode != 0
                inputs["temb"] = temb if var == "temb_strided" else temb[:, 160:].contiguous()
            if var == "res":
                inputs["res"] = res

            def launch(v, var=var):
                tb = v.get("temb")
                if var == "temb_strided":
                    tb = tb[:, 160:]                 # non-contiguous view: ld = Cout + 160
                assert lib.dm_op_igemm(U.stream(), U.ptr(v["x"]), U.ptr(v.get("x2")), U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(tb), U.ptr(v.get("res")),
                                       U.ptr(v["y"]), N, H, W, C1, C2, w.shape[0], OH, OW, mode, 1 if geglu else 0,
                                       tb.stride(0) if tb is not None else 0) == 0, "dm_op_igemm failed"
            y = run3(f"{what} [{var}]", inputs, {"y": (sh_out, F16)}, launch)["y"]
            got[var] = ({k: t.to(U.dev()) for k, t in inputs.items()}, y)
            if geglu:
                proj = ref.permute(0, 2, 3, 1).reshape(-1, w.shape[0]).half().float()
                a, g = proj.chunk(2, dim=-1)
                U.assert_close_fp16(y.view(-1, cy), a * F.gelu(g).half().float(), what, **U.TOL_GEGLU)
                continue
            want = ref
            if var.startswith("temb"):
                want = ref.half().float() + temb[sel, 160:].float()[:, :, None, None]
            if var == "res":
                want = ref.half().float() + U.to_nchw(res[sel].float())
            U.assert_close_fp16(U.to_nchw(y.cpu()[sel]), want, f"{what} [{var}]")
    return got


@pytest.mark.parametrize("M,K,Cout,tile_cols", [(300, 320, 320, 320), (1000, 64, 160, 160), (20, 1280, 1280, 320)])
def test_igemm_dense_tiles(M, K, Cout, tile_cols):
    assert (Cout % 320 == 0) == (tile_cols == 320)           # launch_small: the 128 x 320 tile when Cout % 320 == 0, else 128 x 160
    igemm_case(f"dense 128x{tile_cols} M={M}", 1, 1, M, K, 0, Cout, variants=("res", "plain"), tile=0)


@pytest.mark.parametrize("sub", ["s1", "s2", "up2x", "up_to_size"])
def test_igemm_conv3x3_modes(sub):
    N, H, W, Cin, Cout = 2, 9, 7, 64, 160
    mode, OH, OW, variants = {"s1": (1, H, W, ("temb_strided", "res", "plain")), "s2": (2, (H + 1) // 2, (W + 1) // 2, ("plain",)),
                              "up2x": (3, 2 * H, 2 * W, ("plain",)), "up_to_size": (3, 2 * H - 1, 2 * W - 1, ("plain",))}[sub]
    igemm_case(f"conv3x3 {sub}", N, H, W, Cin, 0, Cout, mode=mode, OH=OH, OW=OW, variants=variants, tile=0)


def test_igemm_conv3x3_concat_sources():
    igemm_case("conv3x3 concat", 2, 8, 8, 128, 64, 320, mode=1, tile=0)


def test_igemm_geglu():
    igemm_case("geglu", 1, 1, 200, 320, 0, 2560, geglu=True, tile=0)


def _smallest_ragged_rows(Cin, Cout, mode, unit=1, start=257):
    """the smallest row count (a multiple of `unit`) above one 256-row tile that the persistent tile takes with a ragged last tile"""
    lib = _lib()
    for M in range((start + unit - 1) // unit * unit, 4096, unit):
        if M % 256 and lib.dm_op_igemm_tile(M, Cin, Cout, mode) == 1:
            return M
    raise AssertionError("the persistent tile takes no ragged row count below 4096")


@pytest.mark.parametrize("kind", ["dense_res", "conv_temb", "conv_concat"])
def test_igemm_persistent_tile(kind):
    """The persistent 256 x 320 tile (`igemm_big` = 1: every shape it accepts).  A time embedding needs samples of whole 256-row tiles
    (igemm_pers_ok), so that kind cannot have a ragged last tile: three whole tiles, one per 32 x 8 sample."""
    with _options(igemm_big=1):
        if kind == "dense_res":
            M = _smallest_ragged_rows(320, 320, 0)
            case = (1, 1, M, 320, 0, 320, 0, None, None, ("res",))
        elif kind == "conv_temb":
            assert _lib().dm_op_igemm_tile(3 * 256, 320, 320, 1) == 1
            case = (3, 32, 8, 320, 0, 320, 1, 32, 8, ("temb",))               # 256 pixels, 8 wide: row ends and image ends inside every tile
        else:
            M = _smallest_ragged_rows(192, 320, 1, unit=63)
            case = (M // 63, 9, 7, 128, 64, 320, 1, 9, 7, ("plain",))
        N, H, W, C1, C2, Cout, mode, OH, OW, variants = case
        igemm_case(f"persistent {kind}", N, H, W, C1, C2, Cout, mode=mode, OH=OH, OW=OW, variants=variants, tile=1, head=lambda h, M: h == M)


def test_igemm_head_rows_between_zero_and_all():
    """Default options: full rounds of 256 x 320 tiles on the persistent kernel, the rest of the rows on the 128-row tile.  8 x 8 samples,
    640 -> 1280 channels with a residual: the smallest sample count, preferring a ragged last tile, whose cut is inside the launch."""
    lib = _lib()
    found = None
    for N in range(8, 2048):
        M = N * 64
        if 0 < lib.dm_op_igemm_head_rows(M, 64, 640, 1280, 1) < M:
            if found is None:
                found = N
            if M % 256:
                found = N
                break
            if N > found + 8:
                break
    assert found is not None, "no batch size below 2048 samples gives a head / tail cut"
    N = found
    igemm_case(f"head / tail cut N={N}", N, 8, 8, 640, 0, 1280, mode=1, variants=("res",), tile=1, head=lambda h, M: 0 < h < M and h % 256 == 0,
               samples=(0, N // 2, N - 1))


@pytest.mark.parametrize("W,C,N,var", [(64, 320, 6, "temb"), (32, 640, 10, "res")])
def test_igemm_tap_reuse_tile(W, C, N, var):
    """igemm_pers_tr.hip (`tap_reuse` = 2: every eligible width; `igemm_big` = 1: all rows on the persistent tile), as test_igemm_tap_reuse_tile
    of tests/test_gpu_ops.py selects it.  (dm_op_igemm_head_rows takes the sample's pixel count as one image row and so cannot describe a
    1024- or 4096-pixel sample: the tile query alone names the route here.)"""
    assert (N * W * W) % 256 == 0 and C >= 320 and C % 320 == 0          # igemm_pers_tr_ok: else the launch falls back to the 128-row tile
    got = igemm_case(f"tap reuse W={W}", N, W, W, C, 0, C, mode=1, variants=(var,), tile=1, samples=(0, N // 2, N - 1),
                     opts={"tap_reuse": 2, "igemm_big": 1})
    # which kernel ran: the (dy, slab, dx) k order gives the bits of the 128-row tile's KO variant (test_igemm_tap_reuse_tile of test_gpu_ops.py)
    # and not those of the plain persistent tile, whose k order is (tap, slab)
    d = U.dev()
    dv, y = got[var]
    args = dict(temb=dv.get("temb"), res=dv.get("res"), mode=1)
    with _options(tap_reuse=2, igemm_big=0):
        y_ko = U.op_igemm(dv["x"], dv["w"], dv["bias"], **args)
    with _options(tap_reuse=0, igemm_big=1):
        y_plain = U.op_igemm(dv["x"], dv["w"], dv["bias"], **args)
    assert torch.equal(y, y_ko), "not the bits of the KO tile: the tap-reuse kernel did not run"
    assert not torch.equal(y, y_plain), "the bits of the plain persistent tile: the launch fell back from igemm_pers_tr.hip"


@pytest.mark.parametrize("N,Cin,Cout,ks,pers", [(40, 1280, 1280, 4, False), (157, 640, 1280, 3, True)])
def test_igemm_splitk(N, Cin, Cout, ks, pers):
    """dm_op_igemm_splitk with its fp32 workspace [parts][M][Cout] between guards, against the unsplit kernel as
    test_igemm_splitk_matches_unsplit does.  pers: three tap-aligned parts on the persistent 256 x 320 tile (splitk_on_pers in igemm.hip:
    fewer weighted rounds over the CUs than on the 128-row tile), else the 128-row split-K kernel (`igemm_splitk` = 2, four parts).  The library
    has no route query for split-K launches: `on_pers` below RESTATES splitk_on_pers (its 0.73 and its rounding) and must follow it if that rule
    changes; what the library itself supplies is the bit-equality with the 128-row kernel on the same three parts, asserted at the end."""
    lib = _lib()
    H = W = 8
    M = N * H * W
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    up, us = -(-M // 256) * (Cout // 320) * ks, -(-M // 128) * (Cout // 320) * ks
    on_pers = ks == 3 and -(-up // n_cu) < 0.73 * -(-us // n_cu)
    inputs = {"x": U.f16_randn(N, H, W, Cin, seed=1), "w": U.f16_randn(Cout, 9 * Cin, seed=3, scale=(9 * Cin) ** -0.5),
              "bias": U.f16_randn(Cout, seed=4, scale=0.1), "temb": U.f16_randn(N, Cout, seed=5), "res": U.f16_randn(N, H, W, Cout, seed=6)}

    def launch(v):
        assert lib.dm_op_igemm_splitk(U.stream(), U.ptr(v["x"]), None, U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(v["temb"]), U.ptr(v["res"]), U.ptr(v["y"]),
                                      N, H, W, Cin, 0, Cout, H, W, 1, Cout, ks, U.ptr(v["ws"])) == 0
    with _options(igemm_splitk=1 if pers else 2):
        if pers:
            assert on_pers, "the launch does not reach the persistent split-K kernel on this device"
        d = U.dev()
        ref = U.op_igemm(inputs["x"].to(d), inputs["w"].to(d), inputs["bias"].to(d), temb=inputs["temb"].to(d), res=inputs["res"].to(d), mode=1)
        y = run3(f"split-K parts={ks}", inputs, {"y": ((N, H, W, Cout), F16), "ws": ((ks, M, Cout), F32)}, launch, work=("ws",))["y"]
    U.assert_splitk_matches_unsplit(y, ref)
    if pers:
        # the 128-row split-K kernel with the same three parts gives the same bits (test_persistent_splitk_is_bit_identical)
        d = U.dev()
        dv = {k_: t.to(d) for k_, t in inputs.items()}
        dv["y"], dv["ws"] = torch.full_like(y, float("nan")), torch.empty(ks * M * Cout, dtype=F32, device=d)
        with _options(igemm_splitk=2):
            launch(dv)
            torch.cuda.synchronize()
        assert torch.equal(dv["y"], y)


@pytest.mark.parametrize("M,C,Cout,epi", [(300, 320, 960, 0), (8192, 1280, 10240, 1)])
def test_ln_stats_and_folded_linear(M, C, Cout, epi):
    """dm_op_ln_stats -> dm_op_igemm_ln, the statistics [M][2] as a guarded tensor between the two launches; reference and tolerances of
    test_layernorm_folded_into_linear."""
    lib = _lib()
    x = (U.f16_randn(M, C, seed=1).float() * 1.5 + 0.7 * U.f16_randn(M, 1, seed=2).float()).half()
    w = U.f16_randn(Cout, C, seed=3, scale=C ** -0.5)
    b = U.f16_randn(Cout, seed=4, scale=0.1)
    gamma = (1 + 0.1 * U.f16_randn(C, seed=5).float()).half()
    beta = (0.05 * U.f16_randn(C, seed=6).float()).half()
    wq, bq = U.pack_geglu(w, b) if epi == 1 else (w, b)
    wf = (wq.float() * gamma.float()[None]).half()
    inputs = {"x": x, "w": wf, "ln_s": wf.float().sum(1), "ln_t": (wq.float() @ beta.float()) + bq.float()}
    cy = Cout // 2 if epi else Cout

    def launch(v):
        assert lib.dm_op_ln_stats(U.stream(), U.ptr(v["x"]), M, C, 1e-5, U.ptr(v["stats"])) == 0
        assert lib.dm_op_igemm_ln(U.stream(), U.ptr(v["x"]), U.ptr(v["w"]), U.ptr(v["ln_s"]), U.ptr(v["ln_t"]), U.ptr(v["stats"]), U.ptr(v["y"]),
                                  M, C, Cout, epi) == 0
    out = run3(f"LN-folded linear M={M} epi={epi}", inputs, {"stats": ((M, 2), F32), "y": ((M, cy), F16)}, launch)
    rows = torch.arange(M) if M <= 1024 else torch.cat([torch.arange(0, 512), torch.arange(M - 512, M)])
    xr = x[rows].float()
    st = out["stats"].cpu()[rows]
    assert torch.allclose(st[:, 0], xr.mean(1), atol=1e-5) and torch.allclose(st[:, 1], (xr.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=1e-4)
    h = F.linear(F.layer_norm(xr, (C,), gamma.float(), beta.float(), 1e-5), w.float(), b.float())
    if epi == 1:
        hh = h.half().float()
        h = hh[:, :Cout // 2] * F.gelu(hh[:, Cout // 2:]).half().float()
    U.assert_close_fp16(out["y"].cpu()[rows], h, f"LN-folded linear epi={epi}", **U.TOL_FP16_CHAIN)


def test_igemm_shortcut():
    """dm_op_igemm_shortcut, 2 x 9 x 7, conv2 320 -> 320 with the 1x1 shortcut on 128 + 64 channels in its k loop (test_conv_shortcut_folded_into_conv2)"""
    lib = _lib()
    N, H, W, C3, C4, Cout = 2, 9, 7, 128, 64, 320
    h, x3, x4 = U.f16_randn(N, H, W, Cout, seed=1), U.f16_randn(N, H, W, C3, seed=2), U.f16_randn(N, H, W, C4, seed=3, scale=0.5)
    w2 = U.f16_randn(Cout, Cout, 3, 3, seed=6, scale=(9 * Cout) ** -0.5)
    ws = U.f16_randn(Cout, C3 + C4, seed=7, scale=(C3 + C4) ** -0.5)
    b2, bs = U.f16_randn(Cout, seed=8, scale=0.1), U.f16_randn(Cout, seed=9, scale=0.1)
    inputs = {"h": h, "x3": x3, "x4": x4, "w": torch.cat([U.pack_conv3(w2), ws], dim=1).contiguous(), "bias": (b2.float() + bs.float()).half()}

    def launch(v):
        assert lib.dm_op_igemm_shortcut(U.stream(), U.ptr(v["h"]), U.ptr(v["x3"]), U.ptr(v["x4"]), U.ptr(v["w"]), U.ptr(v["bias"]), None, U.ptr(v["y"]),
                                        N, H, W, Cout, C3, C4, Cout, 1) == 0
    assert lib.dm_op_igemm_tile(N * H * W, Cout, Cout, 1) == 0
    y = run3("conv2 + folded shortcut", inputs, {"y": ((N, H, W, Cout), F16)}, launch)["y"]
    ref = F.conv2d(U.to_nchw(h.float()), w2.float(), b2.float(), padding=1) + \
        F.conv2d(U.to_nchw(torch.cat([x3, x4], 3).float()), ws.float()[:, :, None, None], bs.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "conv2 + folded shortcut")


def test_groupnorm_conv1x1():
    """dm_op_groupnorm_conv1x1 at 5 x 16 x 8, 64 -> 160 (test_groupnorm_folded_into_conv1x1)"""
    lib = _lib()
    N, H, W, C, Cout, G = 5, 16, 8, 64, 160, 32
    g = torch.Generator().manual_seed(C + N)
    x = (torch.randn(N, C, H, W, generator=g) * (1.0 + torch.rand(N, C, 1, 1, generator=g)) + torch.randn(N, C, 1, 1, generator=g)).half()
    w, b = U.f16_randn(Cout, C, seed=2, scale=C ** -0.5), U.f16_randn(Cout, seed=3, scale=0.1)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).float(), (0.1 * torch.randn(C, generator=g)).float()
    inputs = {"x": U.to_nhwc(x), "gamma": gamma, "beta": beta, "w": w, "bias": b}

    def launch(v):
        assert lib.dm_op_groupnorm_conv1x1(U.stream(), U.ptr(v["x"]), N, H * W, C, G, 1e-6, U.ptr(v["gamma"]), U.ptr(v["beta"]), U.ptr(v["w"]), U.ptr(v["bias"]),
                                           Cout, U.ptr(v["y"])) == 0
    y = run3("GroupNorm folded into conv1x1", inputs, {"y": ((N, H, W, Cout), F16)}, launch)["y"]
    ref = F.conv2d(F.group_norm(x.float(), G, gamma, beta, 1e-6), w.float()[:, :, None, None], b.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "GroupNorm folded into conv1x1", **U.TOL_FP16_CHAIN)


def test_upconv_folded():
    """dm_op_upconv_folded at 3 x 5 x 7, 128 -> 320 (test_upconv_folded: against the definition, and against its own arithmetic in fp32)"""
    lib = _lib()
    N, H, W, Cin, Cout = 3, 5, 7, 128, 320
    x = U.f16_randn(N, H, W, Cin, seed=71)
    w, b = U.f16_randn(Cout, Cin, 3, 3, seed=72, scale=(9 * Cin) ** -0.5), U.f16_randn(Cout, seed=73, scale=0.1)
    w4 = U.fold_upconv_torch(w)

    def launch(v):
        assert lib.dm_op_upconv_folded(U.stream(), U.ptr(v["x"]), U.ptr(v["w4"]), U.ptr(v["bias"]), U.ptr(v["y"]), N, H, W, Cin, Cout) == 0
    y = run3("folded up-sampler", {"x": x, "w4": w4, "bias": b}, {"y": ((N, 2 * H, 2 * W, Cout), F16)}, launch)["y"]
    xs = U.to_nchw(x.float())
    ref = F.conv2d(F.interpolate(xs, scale_factor=2, mode="nearest"), w.float(), b.float(), padding=1)
    U.assert_close_fp16(U.to_nchw(y.cpu()), ref, "folded upsample conv vs interpolate + conv2d")
    own = torch.empty_like(ref)
    for py in (0, 1):
        for px in (0, 1):
            k = w4[py * 2 + px].float().view(Cout, 2, 2, Cin).permute(0, 3, 1, 2)
            own[:, :, py::2, px::2] = F.conv2d(F.pad(xs, (1 - px, px, 1 - py, py)), k, b.float())
    U.assert_close_fp16(U.to_nchw(y.cpu()), own, "folded upsample conv vs its own arithmetic in fp32", **U.TOL_UPFOLD_OWN)


def test_groupnorm_block_sums():
    """dm_op_conv_temb_gn_blocks -> dm_op_gn_blocks (the rows the epilogue did not cover) -> dm_op_groupnorm_blocks at the smallest "head" row of
    test_groupnorm_block_sums_from_the_conv1_epilogue (160 x 16 x 16, 1280 -> 1280: full rounds from the persistent kernel's epilogue, the tail
    from the tensor); the block sums [M / 64][Cout] fp32 and both fp16 tensors between guards."""
    from tests.test_gpu_ops import _block_sums_torch
    lib = _lib()
    N, H, W, Cin, Cout, n_chk = 160, 16, 16, 1280, 1280, 4
    M = N * H * W
    inputs = {"x": U.f16_randn(N, H, W, Cin, seed=41, scale=0.7), "w": U.f16_randn(Cout, 9 * Cin, seed=42, scale=(9 * Cin) ** -0.5),
              "bias": U.f16_randn(Cout, seed=43, scale=0.2), "temb": U.f16_randn(N, Cout, seed=44, scale=0.5),
              "gamma": torch.randn(Cout, generator=torch.Generator().manual_seed(45)) * 0.1 + 1,
              "beta": torch.randn(Cout, generator=torch.Generator().manual_seed(46)) * 0.1}
    done = []

    def launch(v):
        rows = ctypes.c_int(-1)
        assert lib.dm_op_conv_temb_gn_blocks(U.stream(), U.ptr(v["x"]), U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(v["temb"]), U.ptr(v["y"]), N, H, W, Cin, Cout,
                                             Cout, U.ptr(v["blocks"]), ctypes.byref(rows)) == 0
        done.append(rows.value)
        assert lib.dm_op_gn_blocks(U.stream(), U.ptr(v["y"]), M, Cout, rows.value, U.ptr(v["blocks"])) == 0
        assert lib.dm_op_groupnorm_blocks(U.stream(), U.ptr(v["y"]), U.ptr(v["blocks"]), n_chk, H * W, Cout, 32, 1e-5, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1,
                                          U.ptr(v["out"])) == 0
    assert 0 < lib.dm_op_igemm_head_rows(M, H * W, Cin, Cout, 1) < M and lib.dm_op_igemm_tile(M, Cin, Cout, 1) == 1
    out = run3("GroupNorm block sums", inputs, {"y": ((N, H, W, Cout), F16), "blocks": ((M // 64, Cout), F32), "out": ((n_chk, H, W, Cout), F16)}, launch)
    assert len(set(done)) == 1 and 0 < done[0] < M and done[0] % 256 == 0, done      # the epilogue wrote the head, dm_op_gn_blocks the tail
    d = U.dev()
    y_ref = U.op_igemm(inputs["x"].to(d), inputs["w"].to(d), bias=inputs["bias"].to(d), temb=inputs["temb"].to(d), mode=1)
    assert torch.equal(out["y"], y_ref)
    ref, scale = _block_sums_torch(out["y"].view(M, Cout)), _block_sums_torch(out["y"].view(M, Cout).abs())
    U.assert_block_sums(out["blocks"], ref, scale)
    refn = F.silu(F.group_norm(U.to_nchw(out["y"][:n_chk]).float().cpu(), 32, inputs["gamma"], inputs["beta"], 1e-5))
    U.assert_close_fp16(U.to_nchw(out["out"].cpu()), refn, "groupnorm from block sums")


@pytest.mark.parametrize("kind", ["dense", "conv3x3", "down_pad0"])
def test_igemm64_vae_family(kind):
    """The 64-channel-wave instantiation the VAE's channel counts take (Cout % 160 != 0, or mode 4), as tests/test_gpu_vae.py calls it"""
    N, H, W, Cin, Cout, mode, OH, OW, variants = {"dense": (1, 1, 257, 512, 256, 0, None, None, ("res", "plain")),
                                                  "conv3x3": (2, 9, 7, 128, 128, 1, 9, 7, ("res", "plain")),
                                                  "down_pad0": (3, 4, 4, 512, 512, 4, 2, 2, ("plain",))}[kind]
    assert Cout % 160 != 0 or mode == 4
    igemm_case(f"igemm64 {kind}", N, H, W, Cin, 0, Cout, mode=mode, OH=OH, OW=OW, variants=variants, tile=0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp16 attention
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sdpa(q, k, v, heads):
    B, Tq, Cc = q.shape
    D = Cc // heads

    def split(t):
        return t.float().view(B, -1, heads, D).transpose(1, 2)
    return F.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(1, 2).reshape(B, Tq, Cc)


def _launch_attention(v, Q, K, V, heads, B, slots=None, slot_div=0, n_slots=0, q_mod=0):
    Tq, Cc = Q.shape[1], Q.shape[2]
    Tk, D = K.shape[1], Cc // heads
    assert _lib().dm_op_attention_slots(U.stream(), U.ptr(Q), U.ptr(K), U.ptr(V), U.ptr(v["o"]), Q.stride(1), K.stride(1), V.stride(1), Cc,
                                        Q.stride(0), K.stride(0), V.stride(0), Tq * Cc, U.ptr(slots), slot_div, n_slots, q_mod,
                                        B, heads, Tq, Tk, D, float(D) ** -0.5) == 0, "dm_op_attention failed"


SELF_ROUTES = [("generic40", 40, 200, 200, 1), ("generic80", 80, 336, 336, 1), ("generic160", 160, 40, 192, 9), ("qk32", 40, 300, 384, 5),
               ("qk64", 40, 300, 384, 1), ("pipe", 40, 300, 384, 9), ("pipe80", 80, 130, 512, 1), ("pp10", 40, 300, 384, 10),
               ("pp12", 40, 300, 384, 12), ("d160", 160, 40, 192, 1)]


@pytest.mark.parametrize("route,D,Tq,Tk,attn_pipe", SELF_ROUTES, ids=[r[0] for r in SELF_ROUTES])
def test_attention_self_routes(route, D, Tq, Tk, attn_pipe):
    """Q / K / V as strided column slices of one fused buffer (Tq == Tk), else Q alone and K / V as slices of a fused K/V buffer;
    against fp32 SDPA at the tolerance of test_attention_self."""
    heads, B = 8, 2
    Cc = heads * D
    if Tq == Tk:
        qkv = U.f16_randn(B, Tq, 3 * Cc, seed=17)
        q, k, v_ = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
        inputs = {"qkv": qkv}
    else:
        q, kv = U.f16_randn(B, Tq, Cc, seed=23), U.f16_randn(B, Tk, 2 * Cc, seed=24)
        k, v_ = kv[..., :Cc], kv[..., Cc:]
        inputs = {"q": q, "kv": kv}

    def launch(v):
        if Tq == Tk:
            g = v["qkv"]
            _launch_attention(v, g[..., :Cc], g[..., Cc:2 * Cc], g[..., 2 * Cc:], heads, B)
        else:
            _launch_attention(v, v["q"], v["kv"][..., :Cc], v["kv"][..., Cc:], heads, B)
    with _options(attn_pipe=attn_pipe):
        assert U.attention_route(B, heads, Tq, Tk, D) == route
        o = run3(f"attention {route}", inputs, {"o": ((B, Tq, Cc), F16)}, launch)["o"]
    U.assert_close_fp16(o, _sdpa(q, k, v_, heads), f"attention {route} D={D} Tq={Tq} Tk={Tk}", **U.TOL_FP16_CHAIN)


CROSS_ROUTES = [("d160_cross", 160, 24, 77, 5, 0), ("cross", 40, 300, 65, 3, 0), ("cross", 80, 300, 80, 3, 0), ("cross", 40, 300, 77, 12, 4)]


@pytest.mark.parametrize("route,D,Tq,Tk,B,q_mod", CROSS_ROUTES, ids=[f"{r[0]}-{r[1]}-{r[2]}-{r[3]}" + ("-qmod" if r[5] else "") for r in CROSS_ROUTES])
def test_attention_cross_routes(route, D, Tq, Tk, B, q_mod):
    """The resident-K/V cross-attention kernels through a slot table, K / V as column slices of one [prompts][Tk][2 C] buffer; q_mod: sample b
    reads the queries of draw b % q_mod and the keys of prompt b // q_mod (test_attention_cross_shared_draw_layout_and_slot_rules)."""
    heads, P = 8, 3
    Cc = heads * D
    kv = U.f16_randn(P, Tk, 2 * Cc, seed=29)
    b = torch.arange(B)
    if q_mod:
        q = U.f16_randn(q_mod, Tq, Cc, seed=61)
        kvb, q_of = b // q_mod, b % q_mod
        inputs = {"q": q, "kv": kv}
    else:
        q = U.f16_randn(B, Tq, Cc, seed=28)
        slots = torch.tensor([2, 1, 0, 1, 2][:B], dtype=torch.int32)
        kvb, q_of = slots.long(), b
        inputs = {"q": q, "kv": kv, "slots": slots}

    def launch(v):
        K, V = v["kv"][..., :Cc], v["kv"][..., Cc:]
        if q_mod:
            _launch_attention(v, v["q"], K, V, heads, B, slot_div=q_mod, n_slots=P, q_mod=q_mod)
        else:
            _launch_attention(v, v["q"], K, V, heads, B, slots=v["slots"])
    assert U.attention_route(B, heads, Tq, Tk, D, q_mod=q_mod) == route
    o = run3(f"attention {route} D={D}", inputs, {"o": ((B, Tq, Cc), F16)}, launch)["o"]
    ref = _sdpa(q[q_of], kv[..., :Cc][kvb], kv[..., Cc:][kvb], heads)
    U.assert_close_fp16(o, ref, f"attention {route} D={D} Tq={Tq} Tk={Tk}", **U.TOL_FP16_CHAIN)


@pytest.mark.parametrize("B,T", [(3, 80), (1, 33)])
def test_attention512(B, T):
    """the VAE's single head of 512 (test_attention512): one [B][T][1536] row per token"""
    q, k, v_ = U.f16_randn(B, T, 512, seed=21, scale=1.5), U.f16_randn(B, T, 512, seed=22, scale=1.5), U.f16_randn(B, T, 512, seed=23)

    def launch(v):
        p = v["qkv"].data_ptr()
        assert _lib().dm_op_attention512(U.stream(), ctypes.c_void_p(p), ctypes.c_void_p(p + 1024), ctypes.c_void_p(p + 2048), U.ptr(v["o"]), B, T, 1536, 512,
                                         512.0 ** -0.5) == 0
    o = run3("attention512", {"qkv": torch.cat([q, k, v_], dim=2).contiguous()}, {"o": ((B, T, 512), F16)}, launch)["o"]
    ref = torch.softmax(torch.matmul(q.float(), k.float().transpose(1, 2)) * 512 ** -0.5, dim=-1) @ v_.float()
    U.assert_close_fp16(o, ref, f"attention512 T={T}", **U.TOL_ATTN512)


# ---------------------------------------------------------------------------------------------------------------------------------------
# norms and the loss layer
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_groupnorm():
    N, H, W, C1, C2 = 2, 9, 7, 1280, 640
    x1 = U.f16_randn(N, C1, H, W, seed=23) * 2 + 0.5
    x2 = U.f16_randn(N, C2, H, W, seed=24) * 0.5 - 1.0
    Ct = C1 + C2
    g = torch.randn(Ct, generator=torch.Generator().manual_seed(25)) * 0.1 + 1
    b = torch.randn(Ct, generator=torch.Generator().manual_seed(26)) * 0.1

    def launch(v):
        assert _lib().dm_op_groupnorm(U.stream(), U.ptr(v["x"]), U.ptr(v["x2"]), N, H * W, Ct, C1, 32, 1e-5, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1, U.ptr(v["y"])) == 0
    y = run3("groupnorm", {"x": U.to_nhwc(x1), "x2": U.to_nhwc(x2), "gamma": g, "beta": b}, {"y": ((N, H, W, Ct), F16)}, launch)["y"]
    U.assert_close_fp16(U.to_nchw(y.cpu()), F.silu(F.group_norm(torch.cat([x1, x2], 1).float(), 32, g, b, 1e-5)), f"groupnorm C={Ct}")


@pytest.mark.parametrize("rows,Cc", [(257, 1280), (77, 768)])
def test_layernorm(rows, Cc):
    x = U.f16_randn(rows, Cc, seed=27) * 3 + 1
    g = torch.randn(Cc, generator=torch.Generator().manual_seed(28)) * 0.1 + 1
    b = torch.randn(Cc, generator=torch.Generator().manual_seed(29)) * 0.1

    def launch(v):
        assert _lib().dm_op_layernorm(U.stream(), U.ptr(v["x"]), rows, Cc, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1e-5, U.ptr(v["y"])) == 0
    y = run3("layernorm", {"x": x, "gamma": g, "beta": b}, {"y": ((rows, Cc), F16)}, launch)["y"]
    U.assert_close_fp16(y, F.layer_norm(x.float(), (Cc,), g, b, 1e-5), f"layernorm C={Cc}")


@pytest.mark.parametrize("conv_out_rows", [1, 0])
@pytest.mark.parametrize("B,H,W", [(2, 5, 3), (1, 4, 170), (2, 12, 10)])
def test_conv_out(B, H, W, conv_out_rows):
    """dm_op_conv_out, loss and prediction both guarded (test_conv_out_with_rows_staged_in_lds: pred within half an fp16 ulp of F.conv2d in
    fp64, loss = (float(pred) - eps)^2 bit for bit)"""
    C0 = 320
    x = U.f16_randn(B, H, W, C0, seed=51, scale=1.0)
    w4 = U.f16_randn(4, C0, 3, 3, seed=52, scale=(9 * C0) ** -0.5)
    bias = U.f16_randn(4, seed=53, scale=0.1)
    eps = torch.randn(B, 4, H, W, generator=torch.Generator().manual_seed(54))
    ref = F.conv2d(U.to_nchw(x).double(), w4.double(), bias.double(), padding=1)

    def launch(v):
        assert _lib().dm_op_conv_out(U.stream(), U.ptr(v["x"]), U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(v["eps"]), B, H, W, C0, U.ptr(v["loss"]), U.ptr(v["pred"])) == 0
    with _options(conv_out_rows=conv_out_rows):
        out = run3(f"conv_out rows={conv_out_rows}", {"x": x, "w": U.pack_conv3(w4), "bias": bias, "eps": eps},
                   {"loss": ((B, 4, H, W), F32), "pred": ((B, 4, H, W), F16)}, launch)
    U.assert_conv_out_pred(out["pred"], ref, conv_out_rows)
    assert torch.equal(out["loss"], (out["pred"].float() - eps.to(U.dev())) ** 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp32 net operators
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gemm32(v, N, H, W, OH, OW, Cin, C1, Cout, mode, temb=None):
    assert _lib().dm_f32_op_gemm(U.stream(), U.ptr(v["x"]), U.ptr(v.get("x2")), U.ptr(v["w"]), U.ptr(v["bias"]), U.ptr(temb), U.ptr(v.get("res")), U.ptr(v["y"]),
                                 N, H, W, OH, OW, Cin, C1, Cout, mode, temb.stride(0) if temb is not None else 0) == 0, "dm_f32_op_gemm failed"


@pytest.mark.parametrize("mode,N,H,W,C1,C2,Cout,OH,OW", [(1, 3, 9, 7, 640, 320, 640, 9, 7), (2, 1, 9, 7, 320, 0, 320, 5, 4), (3, 1, 5, 4, 320, 0, 320, 9, 7),
                                                         (4, 1, 16, 16, 128, 0, 128, 8, 8)])
def test_gemm32_conv_modes(mode, N, H, W, C1, C2, Cout, OH, OW):
    from tests.test_gpu_f32 import TOL_OP
    Cin = C1 + C2
    x = _randn(N, Cin, H, W, seed=1)
    w = _randn(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    b = _randn(Cout, seed=3)
    temb = _randn(N, Cout + 64, seed=4) if mode == 1 else None
    res = _randn(N, Cout, OH, OW, seed=5)
    ref = _conv_ref(x, w, b, mode, OH, OW)
    if mode == 1:
        ref = ref + temb[:, 32:32 + Cout, None, None]
    ref = ref + res
    xn = U.to_nhwc(x)
    inputs = {"x": xn[..., :C1].contiguous(), "w": U.pack_conv3(w), "bias": b, "res": U.to_nhwc(res)}
    if C2:
        inputs["x2"] = xn[..., C1:].contiguous()
    if temb is not None:
        inputs["temb"] = temb

    def launch(v):
        _gemm32(v, N, H, W, OH, OW, Cin, C1, Cout, mode, v["temb"][:, 32:] if "temb" in v else None)
    y = run3(f"gemm32 mode {mode}", inputs, {"y": ((N, OH, OW, Cout), F32)}, launch)["y"]
    assert U.rel_l2(U.to_nchw(y).cpu(), ref) < TOL_OP


def test_gemm32_dense():
    from tests.test_gpu_f32 import TOL_OP
    M, K, Nn = 5, 320, 1280
    x, w, b = _randn(M, K, seed=1), _randn(Nn, K, seed=2, scale=K ** -0.5), _randn(Nn, seed=3)
    y = run3("gemm32 dense", {"x": x.view(1, 1, M, K), "w": w, "bias": b}, {"y": ((1, 1, M, Nn), F32)},
             lambda v: _gemm32(v, 1, 1, M, 1, M, K, K, Nn, 0))["y"]
    assert U.rel_l2(y.view(M, Nn).cpu(), F.linear(x, w, b)) < TOL_OP


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(3, 5, 7, 64, 320), (1, 1, 2, 32, 128)])
def test_gemm32_upconv_folded(N, H, W, Cin, Cout):
    from tests.test_gpu_f32 import TOL_OP
    x = _randn(N, Cin, H, W, seed=1)
    w = _randn(Cout, Cin, 3, 3, seed=2, scale=(9 * Cin) ** -0.5)
    b = _randn(Cout, seed=3)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    sel = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    wd = w.double()
    w4 = torch.stack([torch.cat([wd[:, :, sel[py][a], :][:, :, :, sel[px][bb]].sum(dim=(2, 3)) for a in (0, 1) for bb in (0, 1)], dim=1)
                      for py in (0, 1) for px in (0, 1)], 0).float().contiguous()
    y = run3("gemm32 mode 5", {"x": U.to_nhwc(x), "w": w4, "bias": b}, {"y": ((N, 2 * H, 2 * W, Cout), F32)},
             lambda v: _gemm32(v, N, H, W, H, W, Cin, Cin, Cout, 5))["y"]
    assert U.rel_l2(U.to_nchw(y).cpu(), ref) < TOL_OP


@pytest.mark.parametrize("B,heads,Tq,Tk,D,cross", [(1, 8, 90, 90, 40, False), (3, 8, 100, 77, 160, True)])
def test_attention32(B, heads, Tq, Tk, D, cross):
    from tests.test_gpu_f32 import TOL_OP, _attention64
    Cc = heads * D
    nk = 2 if cross else B
    q, k, v_ = _randn(B, Tq, Cc, seed=1), _randn(nk, Tk, Cc, seed=2), _randn(nk, Tk, Cc, seed=3)
    inputs = {"q": q, "k": k, "v": v_}
    if cross:
        inputs["slots"] = torch.tensor([1, 0, 1][:B], dtype=torch.int32)

    def launch(v):
        assert _lib().dm_f32_op_attention(U.stream(), U.ptr(v["q"]), U.ptr(v["k"]), U.ptr(v["v"]), U.ptr(v["o"]), Cc, Cc, Cc, Cc, Tq * Cc, Tk * Cc, Tk * Cc, Tq * Cc,
                                          U.ptr(v.get("slots")), nk, B, heads, Tq, Tk, D, float(D) ** -0.5) == 0
    o = run3("attention32", inputs, {"o": ((B, Tq, Cc), F32)}, launch)["o"]
    sl = inputs["slots"].long() if cross else torch.arange(B)
    assert U.rel_l2(o.cpu(), _attention64(q, k[sl], v_[sl], heads)) < TOL_OP


def test_norms32():
    from tests.test_gpu_f32 import TOL_OP
    lib = _lib()
    N, H, W, C1, C2, G = 2, 9, 7, 1280, 640, 32
    C = C1 + C2
    x = _randn(N, C, H, W, seed=1) * 3 + 5.0
    g, b = _randn(C, seed=2), _randn(C, seed=3)
    xn = U.to_nhwc(x)

    def launch(v):
        assert lib.dm_f32_op_groupnorm(U.stream(), U.ptr(v["xa"]), U.ptr(v["xb"]), N, H * W, C, C1, G, 1e-5, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1, U.ptr(v["work"]),
                                       U.ptr(v["y"])) == 0
    y = run3("groupnorm32", {"xa": xn[..., :C1].contiguous(), "xb": xn[..., C1:].contiguous(), "gamma": g, "beta": b},
             {"work": ((N * G * 2,), F32), "y": ((N, H, W, C), F32)}, launch, work=("work",))["y"]
    assert U.rel_l2(U.to_nchw(y).cpu(), F.silu(F.group_norm(x, G, g, b, 1e-5))) < TOL_OP
    rows, Cl = 333, 640
    t = _randn(rows, Cl, seed=4) * 2 + 1.0
    gl, bl = _randn(Cl, seed=5), _randn(Cl, seed=6)

    def launch_ln(v):
        assert lib.dm_f32_op_layernorm(U.stream(), U.ptr(v["x"]), rows, Cl, U.ptr(v["gamma"]), U.ptr(v["beta"]), 1e-5, U.ptr(v["y"])) == 0
    yl = run3("layernorm32", {"x": t, "gamma": gl, "beta": bl}, {"y": ((rows, Cl), F32)}, launch_ln)["y"]
    assert U.rel_l2(yl.cpu(), F.layer_norm(t, (Cl,), gl, bl, 1e-5)) < TOL_OP


# ---------------------------------------------------------------------------------------------------------------------------------------
# entries that walk descriptor tables (called through ctypes as diff-mining_amd/engine.py calls them)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    e = E.UNetEngine(0)                      # the map, resize and mining entry points need no weights (tests/test_gpu_mining.py)
    yield e
    e.close()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def test_resize_lanczos(engine):
    """dm_resize_lanczos on the smallest group of tests/test_gpu_worklist.py::GROUPS (three sources of different sizes -> 7 x 5 in one
    launch): descriptors, coefficient tables, the uint8 scratch and the output between guards; equal to PIL bit for bit."""
    from diff_mining_amd import resample as RS
    from tests.test_gpu_worklist import GROUPS, _pil_unit, _rand_image
    (out_w, out_h), srcs = min(GROUPS, key=lambda g: g[0][0] * g[0][1] * len(g[1]))
    assert len({s for s in srcs}) >= 2
    imgs = [_rand_image(w, h, seed=i * 131 + w + h) for i, (w, h) in enumerate(srcs)]
    n = len(imgs)
    desc, tables, tmp_rows = RS.resize_plan([(a.shape[1], a.shape[0]) for a in imgs], out_w, out_h)
    inputs = {"src": torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])), "desc": _u8(desc), "tables": torch.from_numpy(tables)}

    def launch(v):
        assert engine.lib.dm_resize_lanczos(_vp(v["src"]), _vp(v["desc"]), _vp(v["tables"]), n, out_w, out_h, tmp_rows, _vp(v["tmp"]), _vp(v["out"]),
                                            engine._stream()) == 0
    out = run3("resize_lanczos", inputs, {"tmp": ((n * 3 * tmp_rows * out_w,), U8), "out": ((n, 3, out_h, out_w), F32)}, launch, work=("tmp",))["out"].cpu()
    for b, a in enumerate(imgs):
        assert torch.equal(out[b:b + 1], _pil_unit(a, out_w, out_h)), f"image {b}"


def test_typicality_image_batched(engine):
    """dm_typicality_image_batched: two images of different (h, w, H, W), a 3 x 3 window; every map equal to its own dm_typicality_image
    call bit for bit (test_batched_maps_bit_equal_to_the_single_image_entry)"""
    rng = np.random.default_rng(7)
    spec = [(3, 2, 8, 8, 64, 64), (2, 2, 12, 10, 45, 37)]
    k = 3
    grids = [torch.from_numpy((1.0 + 0.3 * rng.standard_normal((N, nc, 4, h, w))).astype(np.float32)) for (N, nc, h, w, _, _) in spec]
    desc = np.zeros(len(spec), dtype=E.MINE_DESC_DTYPE)
    g_at = w_at = m_at = 0
    for b, (N, nc, h, w, H, W) in enumerate(spec):
        desc[b] = (g_at, w_at, m_at, N, nc, h, w, H, W)
        g_at += grids[b].numel()
        w_at += h * w + H * (W - k + 1)
        m_at += (H - k + 1) * (W - k + 1)

    def launch(v):
        engine._check(engine.lib.dm_typicality_image_batched(engine._h, _vp(v["loss"]), 0, _vp(v["desc"]), len(spec), k, k, _vp(v["work"]), _vp(v["maps"]),
                                                             engine._stream()), "dm_typicality_image_batched")
    maps = run3("typicality_image_batched", {"loss": torch.cat([g.reshape(-1) for g in grids]), "desc": _u8(desc)},
                {"work": ((w_at,), F32), "maps": ((m_at,), F32)}, launch, work=("work",))["maps"]
    for b, (N, nc, h, w, H, W) in enumerate(spec):
        at, n_el = int(desc[b]["map_offset"]), (H - k + 1) * (W - k + 1)
        assert torch.equal(maps[at:at + n_el].view(H - k + 1, W - k + 1), engine.typicality_image(grids[b], (H, W), k, k)), b


@pytest.mark.parametrize("cond_major", [0, 1])
def test_reduce_typicality_batched(engine, cond_major):
    """dm_reduce_typicality_batched in both layouts: maps equal to the per-image dm_reduce_typicality bit for bit, scalars at
    U.TOL_TYPICALITY_SCALAR of the float64 mean (tests/test_gpu_e2e.py)"""
    n_img, N, nc, h, w = 3, 2, 2, 9, 7
    grids = (1.0 + 0.3 * _randn(n_img, N, nc, 4, h, w, seed=3)).half()
    loss = grids.permute(2, 0, 1, 3, 4, 5).contiguous() if cond_major else grids

    def launch(v):
        engine._check(engine.lib.dm_reduce_typicality_batched(engine._h, _vp(v["loss"]), 1, n_img, N, nc, h, w, cond_major, _vp(v["maps"]), _vp(v["T"]),
                                                              engine._stream()), "dm_reduce_typicality_batched")
    out = run3(f"reduce_typicality_batched cond_major={cond_major}", {"loss": loss}, {"maps": ((n_img, h, w), F32), "T": ((n_img,), F32)}, launch)
    for i in range(n_img):
        assert torch.equal(engine.reduce_typicality(grids[i])[0], out["maps"][i])
        want = (grids[i, :, nc - 1].double() - grids[i, :, 0].double()).mean().item()
        assert abs(out["T"][i].item() - want) <= U.TOL_TYPICALITY_SCALAR * max(1.0, abs(want))


@pytest.mark.parametrize("mode", ["signed", "maxabs", "positive", "split"])
def test_normalize_map(engine, mode):
    """dm_normalize_map on the reference's own 45 x 37 map (1665 elements: no multiple of 256), its two floats of scratch guarded; bit-exact
    against the reference's normalisations in tests/golden/consumers_ref.npz (test_consumers_vs_the_reference_fixture)"""
    import os
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumers_ref.npz"))
    dm = torch.from_numpy(f["a_load_typicality_k1"])
    n = dm.numel()
    assert n % 256 != 0
    outputs = {"work": ((2,), F32), "out": (tuple(dm.shape), F32)}
    if mode == "split":
        outputs["neg"] = (tuple(dm.shape), F32)

    def launch(v):
        engine._check(engine.lib.dm_normalize_map(engine._h, _vp(v["dm"]), n, engine.NORM_MODES[mode], _vp(v["work"]), _vp(v["out"]), _vp(v.get("neg")),
                                                  engine._stream()), "dm_normalize_map")
    out = run3(f"normalize_map {mode}", {"dm": dm}, outputs, launch, work=("work",))
    want = {"signed": "a_load_typicality_norm", "maxabs": "a_unorm", "positive": "a_cnorm_positive", "split": "a_cnorm_split_pos"}[mode]
    assert np.array_equal(out["out"].cpu().numpy(), f[want])
    if mode == "split":
        assert np.array_equal(out["neg"].cpu().numpy(), f["a_cnorm_split_neg"])


def test_patch_embed(engine):
    """dm_patch_embed with windows that touch the map's edges and windows that reach past them (clamped like a numpy slice), against the
    window mean + L2 normalisation in float64 at the bound of test_dift_patch_embeddings"""
    Cc, h, w = 96, 6, 5
    feat = _randn(Cc, h, w, seed=3)
    boxes = torch.tensor([[0, 6, 0, 5], [0, 1, 0, 1], [5, 6, 4, 5], [4, 9, 3, 8], [2, 7, 0, 5], [1, 3, 1, 4], [0, 100, 2, 100]], dtype=torch.int32)
    P = boxes.shape[0]

    def launch(v):
        engine._check(engine.lib.dm_patch_embed(engine._h, _vp(v["feat"]), Cc, h, w, _vp(v["boxes"]), P, _vp(v["out"]), engine._stream()), "dm_patch_embed")
    out = run3("patch_embed", {"feat": feat, "boxes": boxes}, {"out": ((P, Cc), F32)}, launch)["out"].cpu().numpy()
    fd = feat.numpy().astype(np.float64)
    for i, (r0, r1, c0, c1) in enumerate(boxes.tolist()):
        m = fd[:, r0:r1, c0:c1].mean((1, 2))
        ref = m / np.linalg.norm(m)
        assert np.abs(out[i] - ref).max() < U.TOL_PATCH_EMBED, (i, np.abs(out[i] - ref).max())


def test_mine_patches(engine):
    """dm_mine_patches on three maps in one launch (the smaller call of test_all_fixture_maps_in_one_call), against the numpy restatement of
    the reference's selection, bit for bit"""
    import os
    from tests.test_gpu_mining import _check_against
    from tests.test_mining import greedy_numpy
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mining_ref.npz"))
    kx, ky, k, _ = (int(v) for v in fx["short_desc_args"])
    maps = [fx["short_desc_map"], fx["short_desc_map"][:, ::-1].copy(), fx["short_desc_map"][1:, :-1].copy()]
    n = len(maps)
    desc = np.zeros(n, dtype=E.MINE_DESC_DTYPE)
    at = 0
    for b, m in enumerate(maps):
        desc[b]["map_offset"], desc[b]["H"], desc[b]["W"] = at, m.shape[0] + kx - 1, m.shape[1] + ky - 1
        at += m.size
    inputs = {"maps": torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps]).astype(np.float32)), "desc": _u8(desc)}

    def launch(v):
        engine._check(engine.lib.dm_mine_patches(engine._h, _vp(v["maps"]), None, _vp(v["desc"]), n, kx, ky, k, 0, _vp(v["boxes"]), _vp(v["D"]), _vp(v["count"]),
                                                 engine._stream()), "dm_mine_patches")
    out = run3("mine_patches", inputs, {"boxes": ((n, k, 4), I32), "D": ((n, k), F32), "count": ((n,), I32)}, launch)
    for b, m in enumerate(maps):
        rb, rd = greedy_numpy(m, kx, ky, k)
        _check_against(out["boxes"], out["D"], out["count"], b, rb, rd, k)


def test_mine_parallel(engine):
    """dm_mine_parallel on two groups of three sets of 37 x 53 maps (test_every_set_count_against_np_median at n_sets = 3): both descriptor
    tables, the median maps and every result between guards; against np.median and the numpy restatement, bit for bit"""
    from tests.test_gpu_parallel_mining import _check_group
    from tests.test_parallel_mining import parallel_numpy
    noise16 = np.random.default_rng(1961).standard_normal((16, 37, 53)).astype(np.float32)
    n_sets, kx, ky, k = 3, 5, 5, 3
    stacks = [noise16[:n_sets], noise16[16 - n_sets:][::-1]]
    G = len(stacks)
    desc = np.zeros(G * n_sets, dtype=E.MINE_DESC_DTYPE)
    gdesc = np.zeros(G, dtype=E.MINE_DESC_DTYPE)
    at = m_at = 0
    for g, s in enumerate(stacks):
        for c in range(n_sets):
            desc[g * n_sets + c]["map_offset"], desc[g * n_sets + c]["H"], desc[g * n_sets + c]["W"] = at, s.shape[1] + kx - 1, s.shape[2] + ky - 1
            at += s[c].size
        gdesc[g]["map_offset"], gdesc[g]["H"], gdesc[g]["W"] = m_at, s.shape[1] + kx - 1, s.shape[2] + ky - 1
        m_at += s[0].size
    inputs = {"maps": torch.from_numpy(np.concatenate([np.ascontiguousarray(s).reshape(-1) for s in stacks])), "desc": _u8(desc), "gdesc": _u8(gdesc)}
    outputs = {"med": ((m_at,), F32), "boxes": ((G, k, 4), I32), "D": ((G, k), F32), "set_D": ((G, k, n_sets), F32), "count": ((G,), I32)}

    def launch(v):
        engine._check(engine.lib.dm_mine_parallel(engine._h, _vp(v["maps"]), _vp(v["desc"]), G, n_sets, _vp(v["gdesc"]), kx, ky, k, 0, None, _vp(v["med"]),
                                                  _vp(v["boxes"]), _vp(v["D"]), _vp(v["set_D"]), _vp(v["count"]), engine._stream()), "dm_mine_parallel")
    out = run3("mine_parallel", inputs, outputs, launch)
    medians = [out["med"][int(d["map_offset"]):int(d["map_offset"]) + 37 * 53].view(37, 53) for d in gdesc]
    res = (out["boxes"], out["D"], out["set_D"], out["count"], medians)
    for g, s in enumerate(stacks):
        rb, rd, rs, _ = parallel_numpy(s, kx, ky, k)
        _check_group(res, g, s, rb, rd, rs, np.median(s, axis=0), k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# entries with caller workspaces: k-means and the cluster ranking
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nk5", "k1", "long257"])
def test_kmeans_fit_and_cluster_rank(tag):
    """dm_kmeans_fit and dm_cluster_rank through ctypes as diff-mining_amd/clustering.py calls them, the workspace exactly
    dm_kmeans_workspace_bytes long between guards; against scikit-learn's fit in tests/golden/kmeans_ref.npz at the bounds of
    tests/test_gpu_kmeans.py::test_fit_equals_sklearn, and the ranking against the numpy restatement, exactly."""
    import os
    from tests.test_kmeans import case_input
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_ref.npz"))
    X, k = case_input(gold, tag)
    n, d = X.shape
    lib = CL._lib()
    need = CL.workspace_bytes(n, d, k)
    u = CL.kmeans_uniforms(k, 10)
    D = KC.typicality(n, 5)
    inputs = {"X": torch.from_numpy(X), "u": torch.from_numpy(u), "D": torch.from_numpy(D)}
    outputs = {"work": ((need,), U8), "labels": ((n,), I32), "centers": ((k, d), F32), "seeds": ((k,), I32), "inertia": ((), F32), "n_iter": ((), I32),
               "order": ((n,), I32), "cluster_of_rank": ((k,), I32), "offsets": ((k + 1,), I32), "agg": ((k,), F32), "n_nonempty": ((), I32)}

    def launch(v):
        p = CL._p
        rc = lib.dm_kmeans_fit(U.stream(), p(v["X"]), n, d, k, p(v["u"]), len(u), 300, 1e-4, p(v["work"]), need, p(v["labels"]), p(v["centers"]), p(v["seeds"]),
                               p(v["inertia"]), p(v["n_iter"]))
        assert rc == 0, CL.ERRORS.get(rc, rc)
        rc = lib.dm_cluster_rank(U.stream(), p(v["X"]), None, n, d, d, p(v["labels"]), p(v["centers"]), k, p(v["D"]), CL.RANK_CENTROID, CL.AGG_MEDIAN,
                                 p(v["work"]), need, p(v["order"]), p(v["cluster_of_rank"]), p(v["offsets"]), p(v["agg"]), p(v["n_nonempty"]))
        assert rc == 0, CL.ERRORS.get(rc, rc)
    out = {a: t.cpu().numpy() for a, t in run3(f"kmeans {tag}", inputs, outputs, launch, work=("work",)).items()}
    assert np.array_equal(out["seeds"], gold[f"{tag}_seed_index"]) and int(out["n_iter"]) == int(gold[f"{tag}_n_iter"])
    assert np.array_equal(out["labels"], gold[f"{tag}_labels"])
    assert np.abs(out["centers"] - gold[f"{tag}_centers"]).max() <= 16 * float(gold["restatement_center_err"])
    assert abs(float(out["inertia"]) - float(gold[f"{tag}_inertia"])) <= 1e-5 * float(gold[f"{tag}_inertia"])
    want = CL.rank_clusters_host(X, out["labels"], out["centers"], D)
    for name, w_ in zip(("order", "cluster_of_rank", "offsets", "agg", "n_nonempty"), want):
        np.testing.assert_array_equal(out[name], np.asarray(w_), err_msg=name)
