"""The engines' glue kernels one by one (dm_op_* of engine_ops.hip, dm_f32_op_* of f32_net.hip) against the references of
tests/glue_cases.py, which tests/test_glue_refs.py proves on the CPU.

Every operand of every call lives in a tests/gpu_util.py Guarded buffer: check() after the call catches a store outside a tensor and a
written input; every case runs under two fill bytes (0xFF, 0x00) and must give the same bits, which catches a load outside a tensor
that reaches a result.  No engine, no full-size weights.  Bounded tests print the worst measured ratio to their bound
(profiles/glue_ops.txt keeps one run's figures)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from tests import glue_cases as G  # noqa: E402
from tests import gpu_util as U  # noqa: E402

F64 = np.float64
F16, F32 = torch.float16, torch.float32
FILLS = (0xFF, 0x00)
TOL_OP = G.TOL_OP
TDT = {np.dtype(np.float16): F16, np.dtype(np.float32): F32}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tests.test_gpu_f32 import TOL_OP as tol
    assert tol == TOL_OP


def _lib():
    return E.load_library()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run2(what, inputs, outputs, launch, init=None):
    """launch(v), v = {name: device tensor}, with every operand between guards, under both fills: guards and inputs untouched, outputs
    equal bit for bit.  inputs {name: numpy array or None (left out)}; outputs {name: (shape, torch dtype)}; init {name: numpy array}:
    outputs that are written before the call (an operand updated in place).  Returns the outputs as numpy arrays."""
    res = None
    inputs = {k: _t(a) for k, a in inputs.items() if a is not None}
    for fill in FILLS:
        g = U.Guarded(inputs, outputs, fill=fill, device=U.dev())
        v = g.views()
        for k, a in (init or {}).items():
            v[k].copy_(_t(a))
        launch(v)
        torch.cuda.synchronize()
        g.check()
        out = {k: g.view(k).cpu().numpy().copy() for k in outputs}
        if res is None:
            res = out
        else:
            for k in outputs:
                ne = int((_bits(res[k]) != _bits(out[k])).sum())
                assert ne == 0, f"{what}: output {k} depends on the guard fill in {ne} elements"
    return res


def refused(what, inputs, outputs, call):
    """call(v) must return 1 and leave every output byte and every guard as it was"""
    g = U.Guarded({k: _t(a) for k, a in inputs.items()}, outputs, fill=0xA5, device=U.dev())
    rc = call(g.views())
    torch.cuda.synchronize()
    assert rc == 1, f"{what}: rc = {rc}, expected the refusal 1"
    g.check()
    for k in outputs:
        assert bool((g.view(k).view(torch.uint8) == 0xA5).all()), f"{what}: output {k} was written by a refused call"


def _ratio(what, err, bound):
    r = float((err / bound).max())
    print(f"{what}: worst |err| / bound = {r:.3f}")
    return r


S, P = U.stream, U.ptr


# ---------------------------------------------------------------------------------------------------------------------------------------
# bit-exact expectations
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_time_gather():
    table = G.rng(1).standard_normal((1000, 320)).astype(np.float16)
    t = np.array([-5, 0, 1, 500, 999, 1000, 2 ** 40], dtype=np.int64)
    out = run2("time_gather", {"table": table, "t": t}, {"out": ((7, 320), F16)},
               lambda v: _assert0(_lib().dm_op_time_gather(S(), P(v["table"]), P(v["t"]), 7, 320, P(v["out"]))))["out"]
    assert np.array_equal(_bits(out), _bits(G.time_gather(table, t)))


def _assert0(rc):
    assert rc == 0, "the entry refused the call"


@pytest.mark.parametrize("B,H,W", G.IMAGE_SIZES)
@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "x_index"])
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("flow", ["f32", "f16"])
def test_im2col_in(flow, noise, indexed, B, H, W):
    c = G.im2col_in_case(B, H, W, np.float32 if flow == "f32" else np.float16, noise, indexed)
    if indexed:
        assert c["x"].shape[0] == 2
    inputs = {"x": c["x"], "x_index": c["x_index"], "eps": c["eps"] if noise else None, "t": c["t"] if noise else None, "sa": c["sa"], "sb": c["sb"]}

    def launch(v):
        _assert0(_lib().dm_op_im2col_in(S(), P(v["x"]), P(v.get("x_index")), P(v.get("eps")), P(v.get("t")), P(v.get("sa")), P(v.get("sb")),
                                        1 if flow == "f32" else 0, B, H, W, P(v["out"])))
    out = run2("im2col_in", inputs, {"out": ((B * H * W, 64), F16)}, launch)["out"]
    ref = G.im2col_in_ref(c)
    bad = _bits(out) != _bits(ref)
    assert not bad[:, 36:].any(), "columns 36..63 are not +0"
    assert not bad.any(), f"{int(bad.sum())} elements differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("H,W", [s[1:] for s in G.IMAGE_SIZES])
def test_im2col_rgb(H, W):
    B = 2
    x = G.rng(H * 31 + W).standard_normal((B, 3, H, W)).astype(np.float16)
    out = run2("im2col_rgb", {"x": x}, {"out": ((B * H * W, 64), F16)},
               lambda v: _assert0(_lib().dm_op_im2col_rgb(S(), P(v["x"]), B, H, W, P(v["out"]))))["out"]
    bad = _bits(out) != _bits(G.im2col(x))
    assert not bad[:, 27:].any(), "columns 27..63 are not +0"
    assert not bad.any(), f"{int(bad.sum())} elements differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("N,HW,C", [(2, 15, 320), (1, 120, 40), (3, 33, 1280), (1, 1, 8)])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_nhwc_to_nchw(dtype, N, HW, C):
    x = G.rng(HW).standard_normal((N, HW, C)).astype(dtype)
    fn = _lib().dm_op_nhwc_to_nchw if dtype == np.float16 else _lib().dm_f32_op_nhwc_to_nchw
    out = run2("nhwc_to_nchw", {"x": x}, {"y": ((N, C, HW), TDT[np.dtype(dtype)])}, lambda v: _assert0(fn(S(), P(v["x"]), N, HW, C, P(v["y"]))))["y"]
    assert np.array_equal(_bits(out), _bits(G.nhwc_to_nchw(x)))


@pytest.mark.parametrize("rows", [154, 100], ids=["2x77", "rows_not_a_multiple_of_T"])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_clip_embed(dtype, rows):
    vocab, T, C = 101, 77, 768
    tok, pos = G.rng(1).standard_normal((vocab, C)).astype(dtype), G.rng(2).standard_normal((T, C)).astype(dtype)
    ids = G.clip_ids(rows, vocab, 3)
    assert {-3, 0, 100, 101, 49407} <= set(ids.tolist())
    fn = _lib().dm_op_clip_embed if dtype == np.float16 else _lib().dm_f32_op_clip_embed
    out = run2("clip_embed", {"ids": ids, "tok": tok, "pos": pos}, {"out": ((rows, C), TDT[np.dtype(dtype)])},
               lambda v: _assert0(fn(S(), P(v["ids"]), P(v["tok"]), P(v["pos"]), rows, T, C, vocab, P(v["out"]))))["out"]
    ref = G.clip_embed(ids, tok, pos, T)
    bad = _bits(out) != _bits(ref)
    assert not bad.any(), f"{int(bad.sum())} elements differ, first at (row, column) {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("n", [65536, 65536 - 3])
def test_f16_to_f32_over_every_bit_pattern(n):
    x = np.arange(65536, dtype=np.uint16).view(np.float16)[:n]
    out = run2("f16_to_f32", {"x": x}, {"y": ((n,), F32)}, lambda v: _assert0(_lib().dm_op_f16_to_f32(S(), P(v["x"]), P(v["y"]), n)))["y"]
    ref = x.astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan) and np.array_equal(_bits(out[~nan]), _bits(ref[~nan]))


def test_sqerr32():
    n = 1027
    pred, eps = G.rng(1).standard_normal(n).astype(np.float32), G.rng(2).standard_normal(n).astype(np.float32)
    out = run2("sqerr32", {"pred": pred, "eps": eps}, {"out": ((n,), F32)},
               lambda v: _assert0(_lib().dm_f32_op_sqerr(S(), P(v["pred"]), P(v["eps"]), n, P(v["out"]))))["out"]
    assert np.array_equal(_bits(out), _bits(G.sqerr32(pred, eps)))


@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "x_index"])
def test_add_noise32(indexed):
    """three separately rounded fp32 operations (sa x, sb eps, their sum): a fused multiply-add shows as a differing bit"""
    B, per = 3, 4 * 5 * 3 + 1
    r = G.rng(4)
    x, eps = r.standard_normal((2 if indexed else B, per)).astype(np.float32), r.standard_normal((B, per)).astype(np.float32)
    t = np.array([-1, 999, 1200], dtype=np.int64)
    xi = np.array([1, 0, 1], dtype=np.int32) if indexed else None
    sa, sb = G.noise_tables(np.float32)
    out = run2("add_noise32", {"x": x, "x_index": xi, "eps": eps, "t": t, "sa": sa, "sb": sb}, {"out": ((B, per), F32)},
               lambda v: _assert0(_lib().dm_f32_op_add_noise(S(), P(v["x"]), P(v.get("x_index")), P(v["eps"]), P(v["t"]), P(v["sa"]), P(v["sb"]), B, per,
                                                             P(v["out"]))))["out"]
    assert np.array_equal(_bits(out), _bits(G.add_noise(x, xi, eps, t, sa, sb)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# bounded expectations
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_silu_over_every_finite_fp16():
    """x / (1 + exp(-x)) on all 63 488 finite fp16 values: within one fp16 ulp of the correctly rounded float64 value everywhere, and
    that value itself except at most 2 * 4 + 16 = 24 times (4 = what the same formula in IEEE fp32 misses, measured on the CPU by
    tests/test_glue_refs.py; the margin is the kernel's fast exponential).  Measured: 3 (profiles/glue_ops.txt)."""
    x = G.finite_fp16()
    n = x.size
    out = run2("silu", {"x": x}, {"y": ((n,), F16)}, lambda v: _assert0(_lib().dm_op_silu(S(), P(v["x"]), P(v["y"]), n)))["y"]
    G.assert_one_ulp16(out, G.silu64(x), 2 * G.SILU_F32_MISROUNDED + 16, "silu fp16")


def test_quick_gelu_over_every_finite_fp16():
    """x sigmoid(1.702 x), in place, on all 63 488 finite fp16 values: within one fp16 ulp of the correctly rounded float64 value, and
    that value itself except at most 2 * 3 + 16 = 22 times (3 = the same formula in IEEE fp32 on the CPU).  Measured: 2."""
    x = G.finite_fp16()
    n = x.size
    assert n % 8 == 0
    out = run2("quick_gelu", {}, {"x": ((n,), F16)}, lambda v: _assert0(_lib().dm_op_quick_gelu(S(), P(v["x"]), n)), init={"x": x})["x"]
    G.assert_one_ulp16(out, G.quick_gelu64(x), 2 * G.QGELU_F32_MISROUNDED + 16, "quick_gelu fp16")


@pytest.mark.parametrize("shape", [(8,), (5, 3072)], ids=["n8", "5x3072"])
def test_quick_gelu_sizes(shape):
    """one vector of eight, and more than one block.  The cap: an fp32 result within 8 * 2^-24 of the exact one lies across an fp16
    rounding boundary (spacing >= 2^-11 relative) with probability <= 2 * 2^-21 / 2^-11 = 2^-9 per element; twice that expectation, + 1."""
    x = (G.rng(shape[0]).standard_normal(shape) * 3).astype(np.float16)
    n = x.size
    out = run2("quick_gelu", {}, {"x": (shape, F16)}, lambda v: _assert0(_lib().dm_op_quick_gelu(S(), P(v["x"]), n)), init={"x": x})["x"]
    G.assert_one_ulp16(out, G.quick_gelu64(x), n // 256 + 1, f"quick_gelu fp16 {shape}")


@pytest.mark.parametrize("op", ["silu", "quick_gelu"])
def test_activations32(op):
    """4099 values across +-90 (more than sixteen 256-thread blocks, a ragged last one): |y - ref64| <= 8 * 2^-24 |ref| + 2^-149 — four
    roundings and a 2-ulp expf relative, one denormal step absolute.  The regression test of two findings (figures in
    profiles/glue_ops.txt): silu32 returned -0 below x = -88.73, where exp(-x) overflows and x e^x is still a normal number (30 values),
    and quick_gelu32 did so below x = -52.14 and carried the rounding of 1.702f * x through exp() as a relative error of up to ~50
    roundings (989 values over the bound).  Both kernels now meet it (worst ratios 0.33 and 0.87)."""
    n = 4099
    x = np.linspace(-90.0, 90.0, n).astype(np.float32)
    if op == "silu":
        out = run2("silu32", {"x": x}, {"y": ((n,), F32)}, lambda v: _assert0(_lib().dm_f32_op_silu(S(), P(v["x"]), P(v["y"]), n)))["y"]
        ref = G.silu64(x)
    else:
        out = run2("quick_gelu32", {}, {"x": ((n,), F32)}, lambda v: _assert0(_lib().dm_f32_op_quick_gelu(S(), P(v["x"]), n)), init={"x": x})["x"]
        ref = G.quick_gelu64(x)
    err, bound = np.abs(out.astype(F64) - ref), 8 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
    r = _ratio(f"{op}32", err, bound)
    if r > 1:
        i = np.argsort(err / bound)[::-1][:5]
        print(f"{op}32: {int((err > bound).sum())} of {n} over the bound; worst at x = {x[i].tolist()}, got {out[i].tolist()}, ref {ref[i].tolist()}")
    assert not np.isnan(out).any() and r <= 1


@pytest.mark.parametrize("groups,ens,HW,C", [(2, 1, 15, 320), (1, 3, 120, 40), (2, 8, 33, 1280)])
@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_ensemble_mean(dtype, groups, ens, HW, C):
    """fp32 sum of `ens` values, one division: |err| <= ens * 2^-24 * mean |x| against the float64 mean"""
    x = (G.rng(HW).standard_normal((groups * ens, HW, C)) * 2).astype(dtype)
    fn = _lib().dm_op_ensemble_mean if dtype == np.float16 else _lib().dm_f32_op_ensemble_mean
    out = run2("ensemble_mean", {"x": x}, {"y": ((groups, C, HW), F32)}, lambda v: _assert0(fn(S(), P(v["x"]), groups, ens, HW, C, P(v["y"]))))["y"]
    ref, mag = G.ensemble_mean64(x, groups, ens)
    assert _ratio(f"ensemble_mean {np.dtype(dtype).name} ens={ens}", np.abs(out - ref), ens * 2.0 ** -24 * mag + 1e-300) <= 1
    if ens == 1:
        assert np.array_equal(out, ref.astype(np.float32))


def _posterior16(c, B, draws, HW, ldh, noise=True, moments=True, lat16=True, lat32=True):
    outs = {}
    if lat16:
        outs["l16"] = ((B * draws, 4, HW), F16)
    if lat32:
        outs["l32"] = ((B * draws, 4, HW), F32)
    if moments:
        outs["m"] = ((B, 8, HW), F32)

    def launch(v):
        _assert0(_lib().dm_op_posterior(S(), P(v["h"]), ldh, P(v["qw"]), P(v["qb"]), P(v.get("noise")), B, draws, HW, c["scaling"], P(v.get("l16")),
                                        P(v.get("l32")), P(v.get("m"))))
    return run2("posterior", {"h": c["h"], "qw": c["qw"], "qb": c["qb"], "noise": c["noise"] if noise else None}, outs, launch)


def _check_latents(what, lat, m_gpu, c, draws, noise):
    ref, mag = G.posterior_latent64(m_gpu, c["noise"] if noise else None, draws, c["scaling"])
    assert not np.isnan(lat).any()
    return _ratio(what, np.abs(lat.astype(F64) - ref), 8 * 2.0 ** -24 * c["scaling"] * mag + 1e-300)


@pytest.mark.parametrize("kind", ["sample", "mode", "clamp"])
@pytest.mark.parametrize("ldh", [8, 64])
@pytest.mark.parametrize("B,draws,HW", G.POSTERIOR_SIZES)
def test_posterior16(B, draws, HW, ldh, kind):
    """quant_conv + sampling of the fp16 VAE.  Moments: fp16(fp32 sum) within half an fp16 ulp + 2^-20 sum |w h| of float64.  Latents
    against float64 FROM the moments the GPU returned (so the check is on the sampling): |err| <= 8 * 2^-24 * scaling * (|mean| + std |noise|).
    Image b's activations are 30^b times image 0's: a draw on another image's moments cannot pass.  latent16 == fp16(latent32); the same
    latents with `moments` NULL."""
    c = G.posterior_case(B, draws, HW, ldh, np.float16, clamp=(kind == "clamp"))
    noise = kind != "mode"
    out = _posterior16(c, B, draws, HW, ldh, noise=noise)
    m64, mag = G.posterior_moments64(c)
    bound = 0.5 * G.ulp16(m64) + 2.0 ** -20 * mag
    assert _ratio(f"posterior16 moments ({B},{draws},{HW}) ldh={ldh} {kind}", np.abs(out["m"].astype(F64) - m64), bound) <= 1
    assert np.array_equal(out["m"], out["m"].astype(np.float16).astype(np.float32)), "the moments are not fp16 values"
    if kind == "clamp":
        assert (out["m"][:, 4:6] == 25).all() and (out["m"][:, 6:] == -40).all()
    assert _check_latents(f"posterior16 latents ({B},{draws},{HW}) ldh={ldh} {kind}", out["l32"], out["m"], c, draws, noise) <= 1
    assert np.array_equal(_bits(out["l16"]), _bits(_t(out["l32"]).half().numpy())), "latent16 != fp16(latent32)"
    if ldh == 8:
        alone = _posterior16(c, B, draws, HW, ldh, noise=noise, moments=False, lat16=False)
        assert np.array_equal(_bits(alone["l32"]), _bits(out["l32"])), "the latents depend on whether the moments are asked for"
        only16 = _posterior16(c, B, draws, HW, ldh, noise=noise, moments=False, lat32=False)
        assert np.array_equal(_bits(only16["l16"]), _bits(out["l16"]))


@pytest.mark.parametrize("kind", ["sample", "mode", "clamp"])
@pytest.mark.parametrize("B,draws,HW", G.POSTERIOR_SIZES)
def test_posterior32(B, draws, HW, kind):
    """the fp32 net's posterior (pitch 8): moments rel-L2 < TOL_OP against float64, latents as test_posterior16"""
    c = G.posterior_case(B, draws, HW, 8, np.float32, clamp=(kind == "clamp"))
    noise = kind != "mode"
    inputs = {"h": c["h"], "qw": c["qw"], "qb": c["qb"], "noise": c["noise"] if noise else None}

    def launch(v):
        _assert0(_lib().dm_f32_op_posterior(S(), P(v["h"]), P(v["qw"]), P(v["qb"]), P(v.get("noise")), B, draws, HW, c["scaling"], P(v.get("lat")), P(v.get("m"))))
    out = run2("posterior32", inputs, {"lat": ((B * draws, 4, HW), F32), "m": ((B, 8, HW), F32)}, launch)
    m64, _ = G.posterior_moments64(c)
    r = G.rel_l2(out["m"], m64)
    print(f"posterior32 moments ({B},{draws},{HW}) {kind}: rel-L2 {r:.2e} / {TOL_OP:.0e} = {r / TOL_OP:.3f}")
    assert r < TOL_OP
    for b in range(B):
        assert G.rel_l2(out["m"][b], m64[b]) < TOL_OP
    if kind == "clamp":
        assert (out["m"][:, 4:6] == 25).all() and (out["m"][:, 6:] == -40).all()
    assert _check_latents(f"posterior32 latents ({B},{draws},{HW}) {kind}", out["lat"], out["m"], c, draws, noise) <= 1
    alone = run2("posterior32", inputs, {"lat": ((B * draws, 4, HW), F32)}, launch)
    assert np.array_equal(_bits(alone["lat"]), _bits(out["lat"]))
    only_m = run2("posterior32", inputs, {"m": ((B, 8, HW), F32)}, launch)
    assert np.array_equal(_bits(only_m["m"]), _bits(out["m"]))


def test_timestep_embed32():
    """[cos | sin] of t * exp(-ln(10000) j / 160): |err| <= 2^-21 |t f| + 2^-22 against float64 (the fp32 frequency's relative error
    carried through the argument, and the rounding of a value <= 1)"""
    t = np.array([0, 1, 500, 999], dtype=np.int64)
    out = run2("timestep_embed32", {"t": t}, {"out": ((4, 320), F32)}, lambda v: _assert0(_lib().dm_f32_op_timestep_embed(S(), P(v["t"]), 4, 320, P(v["out"]))))["out"]
    ref, arg = G.sinusoid64(t, 320)
    bound = 2.0 ** -21 * np.abs(np.concatenate([arg, arg], 1)) + 2.0 ** -22
    half = 160
    tt = torch.from_numpy(t)
    emb = tt[:, None].float() * torch.exp(-np.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)[None]
    own = torch.cat([torch.cos(emb), torch.sin(emb)], -1).double().numpy()
    _ratio("timestep_embed32: torch's own fp32 evaluation", np.abs(own - ref), bound)
    err = np.abs(out.astype(F64) - ref)
    r = _ratio("timestep_embed32", err, bound)
    if r > 1:
        b, j = np.unravel_index(np.argmax(err / bound), err.shape)
        print(f"timestep_embed32: {int((err > bound).sum())} over the bound; worst at t = {t[b]}, column {j}: err {err[b, j]:.3e}, bound {bound[b, j]:.3e}")
    assert r <= 1


@pytest.mark.parametrize("B,Cin,H,W,Cout", G.CONV_IN_SIZES)
def test_conv_in32(B, Cin, H, W, Cout):
    x, w, b = G.conv_in_case(B, Cin, H, W, Cout)
    out = run2("conv_in32", {"x": x, "w": G.conv_in_pack(w), "bias": b}, {"y": ((B, H, W, Cout), F32)},
               lambda v: _assert0(_lib().dm_f32_op_conv_in(S(), P(v["x"]), P(v["w"]), P(v["bias"]), B, Cin, H, W, Cout, P(v["y"]))))["y"]
    got, ref = _t(np.transpose(out, (0, 3, 1, 2))), _t(G.conv_in64(x, w, b))
    r = U.rel_l2(got, ref)
    rows, cols = U.line_rel_l2(got, ref)
    worst = max(r, rows.max().item(), cols.max().item())
    print(f"conv_in32 ({B},{Cin},{H},{W},{Cout}): rel-L2 {r:.2e}, worst row {rows.max().item():.2e}, worst column {cols.max().item():.2e}; / {TOL_OP:.0e} = {worst / TOL_OP:.3f}")
    assert worst < TOL_OP


def _attn32(qkv, n, T, heads, causal):
    return run2("clip_attention32", {"qkv": qkv}, {"o": ((n * T, heads * 64), F32)},
                lambda v: _assert0(_lib().dm_f32_op_clip_attention(S(), P(v["qkv"]), n, T, heads, int(causal), P(v["o"]))))["o"]


def _attn16(qkv, n, T, heads):
    return run2("clip_attention", {"qkv": qkv}, {"o": ((n * T, heads * 64), F16)},
                lambda v: _assert0(_lib().dm_op_clip_attention(S(), P(v["qkv"]), n, T, heads, P(v["o"]))))["o"]


@pytest.mark.parametrize("T,causal", [(77, True), (50, False)])
def test_clip_attention32(T, causal):
    """q four times a unit draw: after the kernel's 1/8 a score deviates by ~4, so a row's softmax is carried by a few keys"""
    n, heads = 2, 12
    qkv = G.attention_case(n, T, heads, np.float32, 4.0)
    ref, _, _ = G.attention64(qkv, n, T, heads, causal, q_factor=0.125)
    r = G.rel_l2(_attn32(qkv, n, T, heads, causal), ref)
    print(f"clip_attention32 T={T} causal={causal}: rel-L2 {r:.2e} / {TOL_OP:.0e} = {r / TOL_OP:.3f}")
    assert r < TOL_OP


@pytest.mark.parametrize("T", [77, 5, 1])
def test_clip_attention16(T):
    """Per element against the float64 reference whose probabilities are rounded to fp16 once, as the kernel's are:
    |err| <= ulp16(ref) / 2 + sum_k ulp16(p_k) |v_k| + 2^-20 sum_k p_k |v_k| — the output's rounding, every probability one fp16 step away,
    fp32 accumulation.  q arrives pre-scaled: a unit draw / 2 gives scores that deviate by ~4."""
    n, heads = 3, 12
    qkv = G.attention_case(n, T, heads, np.float16, 0.5)
    out = _attn16(qkv, n, T, heads)
    ref, pu, pv = G.attention64(qkv, n, T, heads, True, p16=True)
    exact, _, _ = G.attention64(qkv, n, T, heads, True)
    print(f"clip_attention fp16 T={T}: rel-L2 to the modelled reference {G.rel_l2(out, ref):.2e}, to the unmodelled one {G.rel_l2(out, exact):.2e}")
    assert not np.isnan(out).any()
    assert _ratio(f"clip_attention fp16 T={T}", np.abs(out.astype(F64) - ref), 0.5 * G.ulp16(ref) + pu + 2.0 ** -20 * pv) <= 1
    if T == 1:
        assert np.array_equal(_bits(out), _bits(qkv[:, 2 * heads * 64:])), "one key: the output is v_0"


# ---------------------------------------------------------------------------------------------------------------------------------------
# properties of the two attentions, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _runner(kind):
    if kind == "f16":
        return np.float16, 0.2, (lambda q, n, T, heads: _attn16(q, n, T, heads))
    return np.float32, 1.6, (lambda q, n, T, heads: _attn32(q, n, T, heads, True))


@pytest.mark.parametrize("kind", ["f16", "f32"])
def test_causal_attention_properties(kind):
    """Tokens after t0 (their q, k and v rows) do not reach outputs 0..t0; key 0 reaches every output row; a sequence's result does not
    depend on its neighbours.  (Milder scores than the parity tests, deviation ~1.6, so key 0 keeps a weight fp16 can hold.)"""
    dtype, q_scale, run = _runner(kind)
    n, T, heads, t0 = 2, 77, 12, 37
    C = heads * 64
    qkv = G.attention_case(n, T, heads, dtype, q_scale)
    base = run(qkv, n, T, heads).reshape(n, T, C)
    later = qkv.copy().reshape(n, T, 3 * C)
    later[:, t0 + 1:] = G.rng(99).standard_normal((n, T - t0 - 1, 3 * C)).astype(dtype) * 3
    got = run(later.reshape(n * T, 3 * C), n, T, heads).reshape(n, T, C)
    assert np.array_equal(_bits(got[:, :t0 + 1]), _bits(base[:, :t0 + 1])), "a later token reached an earlier output"
    assert (_bits(got[:, t0 + 1:]) != _bits(base[:, t0 + 1:])).reshape(n, T - t0 - 1, heads, 64).any(-1).all()
    key0 = qkv.copy().reshape(n, T, 3 * C)
    key0[:, 0, C:2 * C] = 0                      # score 0 under every query
    key0[:, 0, 2 * C:] = 2048                    # and a value that moves the output by p_0 * 2048
    got = run(key0.reshape(n * T, 3 * C), n, T, heads).reshape(n, T, heads, 64)
    changed = (_bits(got) != _bits(base.reshape(n, T, heads, 64))).any(-1)
    assert changed.all(), f"key 0 does not reach {int((~changed).sum())} (sequence, query, head) outputs"
    alone = run(qkv[T:], 1, T, heads)
    assert np.array_equal(_bits(alone), _bits(base[1])), "sequence 1 alone differs from sequence 1 of the batch"


def test_full_attention32_properties():
    """the non-causal T = 50 kernel: permuting the keys together with their values moves the result by no more than TOL_OP (the order of
    an fp32 sum); sequences are independent"""
    n, T, heads = 2, 50, 12
    C = heads * 64
    qkv = G.attention_case(n, T, heads, np.float32, 4.0)
    base = _attn32(qkv, n, T, heads, False)
    perm = G.rng(5).permutation(T)
    p = qkv.copy().reshape(n, T, 3 * C)
    p[:, :, C:] = p[:, perm, C:]
    got = _attn32(p.reshape(n * T, 3 * C), n, T, heads, False)
    r = G.rel_l2(got, base)
    print(f"clip_attention32 T=50: keys and values permuted, rel-L2 {r:.2e} / {TOL_OP:.0e} = {r / TOL_OP:.3f}")
    assert r < TOL_OP
    key0 = qkv.copy().reshape(n, T, 3 * C)
    key0[:, 0, C:2 * C] = 0
    key0[:, 0, 2 * C:] = 2048
    got = _attn32(key0.reshape(n * T, 3 * C), n, T, heads, False).reshape(n, T, heads, 64)
    assert (_bits(got) != _bits(base.reshape(n, T, heads, 64))).any(-1).all(), "key 0 does not reach every output"
    assert np.array_equal(_bits(_attn32(qkv[T:], 1, T, heads, False)), _bits(base[T:]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals: rc = 1, nothing launched, every output byte as it was
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _lib()
    h16 = lambda *s: np.ones(s, dtype=np.float16)          # noqa: E731
    f32 = lambda *s: np.ones(s, dtype=np.float32)          # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)           # noqa: E731
    i32 = lambda *v: np.array(v, dtype=np.int32)           # noqa: E731
    cases = []

    def case(what, inputs, outputs, call):
        cases.append(what)
        refused(what, inputs, outputs, call)

    # ---- fp16 engine ----
    tg = ({"table": h16(1000, 8), "t": i64(1, 2)}, {"out": ((2, 8), F16)})
    case("time_gather dim = 0", *tg, lambda v: lib.dm_op_time_gather(S(), P(v["table"]), P(v["t"]), 2, 0, P(v["out"])))
    case("time_gather B = 0", *tg, lambda v: lib.dm_op_time_gather(S(), P(v["table"]), P(v["t"]), 0, 8, P(v["out"])))
    case("time_gather B * dim overflows", *tg, lambda v: lib.dm_op_time_gather(S(), P(v["table"]), P(v["t"]), 1 << 20, 1 << 12, P(v["out"])))
    case("time_gather null table", *tg, lambda v: lib.dm_op_time_gather(S(), None, P(v["t"]), 2, 8, P(v["out"])))
    case("time_gather null t", *tg, lambda v: lib.dm_op_time_gather(S(), P(v["table"]), None, 2, 8, P(v["out"])))
    sl = ({"x": h16(16)}, {"y": ((16,), F16)})
    case("silu n = 0", *sl, lambda v: lib.dm_op_silu(S(), P(v["x"]), P(v["y"]), 0))
    case("silu n < 0", *sl, lambda v: lib.dm_op_silu(S(), P(v["x"]), P(v["y"]), -16))
    case("silu null in", *sl, lambda v: lib.dm_op_silu(S(), None, P(v["y"]), 16))
    for flow, mk in ((1, f32), (0, h16)):
        ii = ({"x": mk(2, 4, 3, 3), "eps": mk(2, 4, 3, 3), "t": i64(1, 2), "sa": mk(1000), "sb": mk(1000)}, {"out": ((18, 64), F16)})
        call = lambda v, **kw: lib.dm_op_im2col_in(S(), P(kw.get("x", v["x"])), None, P(kw.get("eps", v["eps"])), P(kw.get("t", v["t"])),      # noqa: E731
                                                   P(kw.get("sa", v["sa"])), P(kw.get("sb", v["sb"])), flow, kw.get("B", 2), kw.get("H", 3), kw.get("W", 3), P(v["out"]))
        case(f"im2col_in flow {flow}: sa without sb", *ii, lambda v: call(v, sb=None))
        case(f"im2col_in flow {flow}: sb without sa", *ii, lambda v: call(v, sa=None))
        case(f"im2col_in flow {flow}: noise without eps", *ii, lambda v: call(v, eps=None))
        case(f"im2col_in flow {flow}: noise without t", *ii, lambda v: call(v, t=None))
        case(f"im2col_in flow {flow}: null x", *ii, lambda v: call(v, x=None))
        case(f"im2col_in flow {flow}: B = 0", *ii, lambda v: call(v, B=0))
        case(f"im2col_in flow {flow}: H = 0", *ii, lambda v: call(v, H=0))
        case(f"im2col_in flow {flow}: W = -3", *ii, lambda v: call(v, W=-3))
    tr = ({"x": h16(2, 4, 8)}, {"y": ((2, 8, 4), F16)})
    case("nhwc_to_nchw N > 65535", *tr, lambda v: lib.dm_op_nhwc_to_nchw(S(), P(v["x"]), 65536, 4, 8, P(v["y"])))
    case("nhwc_to_nchw HW = 0", *tr, lambda v: lib.dm_op_nhwc_to_nchw(S(), P(v["x"]), 2, 0, 8, P(v["y"])))
    case("nhwc_to_nchw C = 0", *tr, lambda v: lib.dm_op_nhwc_to_nchw(S(), P(v["x"]), 2, 4, 0, P(v["y"])))
    case("nhwc_to_nchw null X", *tr, lambda v: lib.dm_op_nhwc_to_nchw(S(), None, 2, 4, 8, P(v["y"])))
    em = ({"x": h16(2, 4, 8)}, {"y": ((1, 8, 4), F32)})
    case("ensemble_mean ens = 0", *em, lambda v: lib.dm_op_ensemble_mean(S(), P(v["x"]), 1, 0, 4, 8, P(v["y"])))
    case("ensemble_mean groups > 65535", *em, lambda v: lib.dm_op_ensemble_mean(S(), P(v["x"]), 65536, 2, 4, 8, P(v["y"])))
    case("ensemble_mean groups = 0", *em, lambda v: lib.dm_op_ensemble_mean(S(), P(v["x"]), 0, 2, 4, 8, P(v["y"])))
    case("ensemble_mean null X", *em, lambda v: lib.dm_op_ensemble_mean(S(), None, 1, 2, 4, 8, P(v["y"])))
    rg = ({"x": h16(1, 3, 3, 3)}, {"out": ((9, 64), F16)})
    case("im2col_rgb B = 0", *rg, lambda v: lib.dm_op_im2col_rgb(S(), P(v["x"]), 0, 3, 3, P(v["out"])))
    case("im2col_rgb W = 0", *rg, lambda v: lib.dm_op_im2col_rgb(S(), P(v["x"]), 1, 3, 0, P(v["out"])))
    case("im2col_rgb null x", *rg, lambda v: lib.dm_op_im2col_rgb(S(), None, 1, 3, 3, P(v["out"])))
    po = ({"h": h16(4, 16), "qw": h16(8, 8), "qb": h16(8), "noise": h16(1, 4, 4)}, {"l16": ((1, 4, 4), F16), "l32": ((1, 4, 4), F32), "m": ((1, 8, 4), F32)})
    pcall = lambda v, ldh=16, B=1, draws=1, HW=4, outs=True, **kw: lib.dm_op_posterior(                                                       # noqa: E731
        S(), P(kw.get("h", v["h"])), ldh, P(kw.get("qw", v["qw"])), P(kw.get("qb", v["qb"])), P(v["noise"]), B, draws, HW, 0.18215,
        P(v["l16"]) if outs else None, P(v["l32"]) if outs else None, P(v["m"]) if outs else None)
    case("posterior ldh % 8", *po, lambda v: pcall(v, ldh=12))
    case("posterior ldh < 8", *po, lambda v: pcall(v, ldh=0))
    case("posterior ldh = 4", *po, lambda v: pcall(v, ldh=4))
    case("posterior draws = 0", *po, lambda v: pcall(v, draws=0))
    case("posterior no output", *po, lambda v: pcall(v, outs=False))
    case("posterior B = 0", *po, lambda v: pcall(v, B=0))
    case("posterior HW = 0", *po, lambda v: pcall(v, HW=0))
    case("posterior null Hm", *po, lambda v: pcall(v, h=None))
    case("posterior null qw", *po, lambda v: pcall(v, qw=None))
    ce = ({"ids": i32(1, 2), "tok": h16(4, 16), "pos": h16(2, 16)}, {"out": ((2, 16), F16)})
    ecall = lambda v, rows=2, T=2, C=16, vocab=4, **kw: lib.dm_op_clip_embed(S(), P(kw.get("ids", v["ids"])), P(v["tok"]), P(kw.get("pos", v["pos"])), rows, T, C,      # noqa: E731
                                                                             vocab, P(v["out"]))
    case("clip_embed C % 8", *ce, lambda v: ecall(v, C=12))
    case("clip_embed T = 0", *ce, lambda v: ecall(v, T=0))
    case("clip_embed vocab = 0", *ce, lambda v: ecall(v, vocab=0))
    case("clip_embed rows = 0", *ce, lambda v: ecall(v, rows=0))
    case("clip_embed null ids", *ce, lambda v: ecall(v, ids=None))
    case("clip_embed null pos", *ce, lambda v: ecall(v, pos=None))
    ca = ({"qkv": h16(4, 192)}, {"o": ((4, 64), F16)})
    case("clip_attention T > 80", *ca, lambda v: lib.dm_op_clip_attention(S(), P(v["qkv"]), 1, 81, 1, P(v["o"])))
    case("clip_attention heads = 0", *ca, lambda v: lib.dm_op_clip_attention(S(), P(v["qkv"]), 1, 4, 0, P(v["o"])))
    case("clip_attention T = 0", *ca, lambda v: lib.dm_op_clip_attention(S(), P(v["qkv"]), 1, 0, 1, P(v["o"])))
    case("clip_attention n = 0", *ca, lambda v: lib.dm_op_clip_attention(S(), P(v["qkv"]), 0, 4, 1, P(v["o"])))
    case("clip_attention null qkv", *ca, lambda v: lib.dm_op_clip_attention(S(), None, 1, 4, 1, P(v["o"])))
    case("quick_gelu n % 8", {}, {"x": ((16,), F16)}, lambda v: lib.dm_op_quick_gelu(S(), P(v["x"]), 12))
    case("quick_gelu n = 0", {}, {"x": ((16,), F16)}, lambda v: lib.dm_op_quick_gelu(S(), P(v["x"]), 0))
    cv = ({"x": h16(16)}, {"y": ((16,), F32)})
    case("f16_to_f32 n = 0", *cv, lambda v: lib.dm_op_f16_to_f32(S(), P(v["x"]), P(v["y"]), 0))
    case("f16_to_f32 null x", *cv, lambda v: lib.dm_op_f16_to_f32(S(), None, P(v["y"]), 16))

    # ---- fp32 net ----
    c32 = ({"ids": i32(1, 2), "tok": f32(4, 16), "pos": f32(2, 16)}, {"out": ((2, 16), F32)})
    e32 = lambda v, rows=2, T=2, C=16, vocab=4, **kw: lib.dm_f32_op_clip_embed(S(), P(kw.get("ids", v["ids"])), P(v["tok"]), P(v["pos"]), rows, T, C, vocab, P(v["out"]))   # noqa: E731
    case("clip_embed32 T = 0", *c32, lambda v: e32(v, T=0))
    case("clip_embed32 vocab = 0", *c32, lambda v: e32(v, vocab=0))
    case("clip_embed32 rows = 0", *c32, lambda v: e32(v, rows=0))
    case("clip_embed32 C = 0", *c32, lambda v: e32(v, C=0))
    case("clip_embed32 null ids", *c32, lambda v: e32(v, ids=None))
    a32 = ({"qkv": f32(77, 192)}, {"o": ((77, 64), F32)})
    for T, causal in ((77, 0), (50, 1), (64, 0), (64, 1), (0, 1)):
        case(f"clip_attention32 T = {T} causal = {causal}", *a32, lambda v, T=T, causal=causal: lib.dm_f32_op_clip_attention(S(), P(v["qkv"]), 1, T, 1, causal, P(v["o"])))
    case("clip_attention32 heads = 0", *a32, lambda v: lib.dm_f32_op_clip_attention(S(), P(v["qkv"]), 1, 77, 0, 1, P(v["o"])))
    case("clip_attention32 n = 0", *a32, lambda v: lib.dm_f32_op_clip_attention(S(), P(v["qkv"]), 0, 77, 1, 1, P(v["o"])))
    case("clip_attention32 null qkv", *a32, lambda v: lib.dm_f32_op_clip_attention(S(), None, 1, 77, 1, 1, P(v["o"])))
    case("quick_gelu32 n = 0", {}, {"x": ((16,), F32)}, lambda v: lib.dm_f32_op_quick_gelu(S(), P(v["x"]), 0))
    case("quick_gelu32 n < 0", {}, {"x": ((16,), F32)}, lambda v: lib.dm_f32_op_quick_gelu(S(), P(v["x"]), -1))
    s32 = ({"x": f32(16)}, {"y": ((16,), F32)})
    case("silu32 n = 0", *s32, lambda v: lib.dm_f32_op_silu(S(), P(v["x"]), P(v["y"]), 0))
    case("silu32 null in", *s32, lambda v: lib.dm_f32_op_silu(S(), None, P(v["y"]), 16))
    te = ({"t": i64(1, 2)}, {"out": ((2, 8), F32)})
    case("timestep_embed32 dim = 0", *te, lambda v: lib.dm_f32_op_timestep_embed(S(), P(v["t"]), 2, 0, P(v["out"])))
    case("timestep_embed32 odd dim", *te, lambda v: lib.dm_f32_op_timestep_embed(S(), P(v["t"]), 2, 7, P(v["out"])))
    case("timestep_embed32 B = 0", *te, lambda v: lib.dm_f32_op_timestep_embed(S(), P(v["t"]), 0, 8, P(v["out"])))
    case("timestep_embed32 null t", *te, lambda v: lib.dm_f32_op_timestep_embed(S(), None, 2, 8, P(v["out"])))
    ci = ({"x": f32(1, 4, 3, 3), "w": f32(36, 8), "bias": f32(8)}, {"y": ((1, 3, 3, 8), F32)})
    icall = lambda v, B=1, Cin=4, H=3, W=3, Cout=8, **kw: lib.dm_f32_op_conv_in(S(), P(v["x"]), P(kw.get("w", v["w"])), P(kw.get("bias", v["bias"])), B, Cin, H, W, Cout,   # noqa: E731
                                                                              P(v["y"]))
    case("conv_in32 B = 0", *ci, lambda v: icall(v, B=0))
    case("conv_in32 Cin = 0", *ci, lambda v: icall(v, Cin=0))
    case("conv_in32 H = 0", *ci, lambda v: icall(v, H=0))
    case("conv_in32 Cout = 0", *ci, lambda v: icall(v, Cout=0))
    case("conv_in32 null w", *ci, lambda v: icall(v, w=None))
    case("conv_in32 null bias", *ci, lambda v: icall(v, bias=None))
    an = ({"x": f32(2, 8), "eps": f32(2, 8), "t": i64(1, 2), "sa": f32(1000), "sb": f32(1000)}, {"out": ((2, 8), F32)})
    ncall = lambda v, B=2, per=8, **kw: lib.dm_f32_op_add_noise(S(), P(v["x"]), None, P(kw.get("eps", v["eps"])), P(kw.get("t", v["t"])), P(kw.get("sa", v["sa"])),        # noqa: E731
                                                                P(kw.get("sb", v["sb"])), B, per, P(v["out"]))
    case("add_noise32 B = 0", *an, lambda v: ncall(v, B=0))
    case("add_noise32 per = 0", *an, lambda v: ncall(v, per=0))
    case("add_noise32 null eps", *an, lambda v: ncall(v, eps=None))
    case("add_noise32 null t", *an, lambda v: ncall(v, t=None))
    case("add_noise32 null sa", *an, lambda v: ncall(v, sa=None))
    case("add_noise32 null sb", *an, lambda v: ncall(v, sb=None))
    sq = ({"p": f32(16), "e": f32(16)}, {"out": ((16,), F32)})
    case("sqerr32 n = 0", *sq, lambda v: lib.dm_f32_op_sqerr(S(), P(v["p"]), P(v["e"]), 0, P(v["out"])))
    case("sqerr32 null eps", *sq, lambda v: lib.dm_f32_op_sqerr(S(), P(v["p"]), None, 16, P(v["out"])))
    t32 = ({"x": f32(2, 4, 8)}, {"y": ((2, 8, 4), F32)})
    case("nhwc_to_nchw32 N = 0", *t32, lambda v: lib.dm_f32_op_nhwc_to_nchw(S(), P(v["x"]), 0, 4, 8, P(v["y"])))
    case("nhwc_to_nchw32 C = -8", *t32, lambda v: lib.dm_f32_op_nhwc_to_nchw(S(), P(v["x"]), 2, 4, -8, P(v["y"])))
    case("nhwc_to_nchw32 null X", *t32, lambda v: lib.dm_f32_op_nhwc_to_nchw(S(), None, 2, 4, 8, P(v["y"])))
    m32 = ({"x": f32(2, 4, 8)}, {"y": ((1, 8, 4), F32)})
    case("ensemble_mean32 ens = 0", *m32, lambda v: lib.dm_f32_op_ensemble_mean(S(), P(v["x"]), 1, 0, 4, 8, P(v["y"])))
    case("ensemble_mean32 groups = 0", *m32, lambda v: lib.dm_f32_op_ensemble_mean(S(), P(v["x"]), 0, 2, 4, 8, P(v["y"])))
    case("ensemble_mean32 null X", *m32, lambda v: lib.dm_f32_op_ensemble_mean(S(), None, 1, 2, 4, 8, P(v["y"])))
    p32 = ({"h": f32(4, 8), "qw": f32(8, 8), "qb": f32(8), "noise": f32(1, 4, 4)}, {"lat": ((1, 4, 4), F32), "m": ((1, 8, 4), F32)})
    qcall = lambda v, B=1, draws=1, HW=4, outs=True, **kw: lib.dm_f32_op_posterior(S(), P(kw.get("h", v["h"])), P(v["qw"]), P(kw.get("qb", v["qb"])), P(v["noise"]), B,     # noqa: E731
                                                                               draws, HW, 0.18215, P(v["lat"]) if outs else None, P(v["m"]) if outs else None)
    case("posterior32 draws = 0", *p32, lambda v: qcall(v, draws=0))
    case("posterior32 no output", *p32, lambda v: qcall(v, outs=False))
    case("posterior32 B = 0", *p32, lambda v: qcall(v, B=0))
    case("posterior32 HW = 0", *p32, lambda v: qcall(v, HW=0))
    case("posterior32 null Hm", *p32, lambda v: qcall(v, h=None))
    case("posterior32 null qb", *p32, lambda v: qcall(v, qb=None))
    print(f"{len(cases)} refusals, each rc = 1 with every output byte untouched")
    assert len(set(cases)) == len(cases)
