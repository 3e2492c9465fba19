"""CPU tier: every reference of tests/glue_cases.py against an independent formulation, so that a failure of tests/test_gpu_glue.py on
the GPU is the kernel's and not the reference's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as R
from oracle import vae_ref as VR
from tests import glue_cases as G

F64 = np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_round16_rounds_once_where_torch_rounds_twice():
    """1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10: fp16 must give 1 + 2^-10.  Through fp32 the 2^-30 is lost first, the
    tie goes to even and the result is 1."""
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30])
    assert float(G.round16(x)[0]) == 1.0 + 2.0 ** -10
    assert float(x.astype(np.float32).astype(np.float16)[0]) == 1.0
    assert np.array_equal(G.ulp16(np.array([1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0])),
                          np.array([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]))
    x = G.finite_fp16()
    assert x.size == 63488
    up = np.nextafter(x[(x > 0) & (x < 60000)], np.float16(np.inf)).astype(F64)
    assert np.array_equal(up - x[(x > 0) & (x < 60000)].astype(F64), G.ulp16(x[(x > 0) & (x < 60000)].astype(F64)))


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("B,H,W", G.IMAGE_SIZES)
def test_im2col_against_unfold(B, H, W, C):
    x = G.rng(B + H).standard_normal((B, C, H, W)).astype(np.float16)
    got = G.im2col(x)
    want = F.unfold(_t(x).double(), 3, padding=1).transpose(1, 2).reshape(B * H * W, 9 * C).numpy()      # k = c*9 + dy*3 + dx
    assert np.array_equal(got[:, :9 * C].astype(F64), want)
    assert not got[:, 9 * C:].any() and got.shape == (B * H * W, 64)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("indexed", [False, True])
def test_im2col_in_reference_is_unfold_of_the_noised_tensor(dtype, indexed):
    B, H, W = 3, 5, 3
    c = G.im2col_in_case(B, H, W, dtype, True, indexed)
    assert c["x"].shape[0] == (2 if indexed else 3) and set(c["t"].tolist()) == {-1, 999, 1200}
    got = G.im2col_in_ref(c)
    xs = _t(c["x"])[_t(c["x_index"]).long()] if indexed else _t(c["x"])
    acp = R.alphas_cumprod()
    tt = _t(G.clamp_t(c["t"]))
    if dtype == np.float32:
        noisy = R.add_noise(xs, _t(c["eps"]), tt, acp)
        # the tables (inputs of the case, built in float64): the oracle takes the roots of its fp32 cumprod, a few fp32 ulps away
        assert np.abs(c["sa"].astype(F64) - (acp.double() ** 0.5).numpy()).max() < 1e-6
        sa, sb = _t(c["sa"])[tt][:, None, None, None], _t(c["sb"])[tt][:, None, None, None]
        noisy_tab = sa * xs + sb * _t(c["eps"])                              # three fp32 operations on the kernel's own tables
        assert np.array_equal(G.add_noise(c["x"], c["x_index"], c["eps"], c["t"], c["sa"], c["sb"]), noisy_tab.numpy())
        assert (noisy - noisy_tab).abs().max() < 5e-6
        noisy = noisy_tab.half()
    else:
        noisy = R.add_noise(xs, _t(c["eps"]), tt, acp)                      # fp16 CPU arithmetic: each operation rounded to fp16
        assert noisy.dtype == torch.float16
        mine = G.add_noise(c["x"], c["x_index"], c["eps"], c["t"], c["sa"], c["sb"])
        # torch's CPU half arithmetic may go through fp32 (a sum rounded twice): equal up to one fp16 step, and mostly equal
        d = np.abs(mine.astype(F64) - noisy.numpy().astype(F64))
        assert (d <= G.ulp16(mine.astype(F64))).all() and (d != 0).mean() < 0.01
        noisy = _t(mine)
    want = F.unfold(noisy.double(), 3, padding=1).transpose(1, 2).reshape(B * H * W, 36).numpy()
    assert np.array_equal(got[:, :36].astype(F64), want) and not got[:, 36:].any()
    plain = G.im2col_in_ref(G.im2col_in_case(B, H, W, dtype, False, indexed))
    wantp = F.unfold(xs.double(), 3, padding=1).transpose(1, 2).reshape(B * H * W, 36).numpy()
    assert np.array_equal(plain[:, :36].astype(F64), _t(wantp).to(torch.float16 if dtype == np.float32 else torch.float64).double().numpy())


def test_fp16_sum_is_exact_in_float64_but_not_in_fp32():
    """the reason the fp16 flow's p1 + p2 is formed in float64: 2048 + 2^-14 + ... a pair whose fp32 sum is already rounded"""
    a, b = np.float16(1024.0), np.float16(2.0 ** -14 * 1.5)
    s64 = F64(a) + F64(b)
    assert s64 != F64(np.float32(a) + np.float32(b)) and s64 == 1024.0 + 1.5 * 2.0 ** -14


@pytest.mark.parametrize("T,causal", [(77, True), (50, False), (5, True), (1, True)])
def test_attention_references_against_sdpa(T, causal):
    n, heads = 2, 12
    qkv = G.attention_case(n, T, heads, np.float32, 0.5)
    got, _, pv = G.attention64(qkv, n, T, heads, causal, q_factor=0.125)
    x = _t(qkv).double().view(n, T, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(n * T, heads * 64).numpy()     # scale = 64^-0.5
    assert G.rel_l2(got, want) < 1e-14
    assert (np.abs(got) <= pv + 1e-15).all()
    # the modelled reference: P rounded to fp16 moves the result by at most sum_k ulp16(p_k) |v_k| / 2
    q16 = G.attention_case(n, T, heads, np.float16, 0.5)
    exact, pu, _ = G.attention64(q16, n, T, heads, causal)
    model, _, _ = G.attention64(q16, n, T, heads, causal, p16=True)
    assert (np.abs(model - exact) <= 0.5 * pu + 1e-15).all()
    if T > 1:
        assert G.rel_l2(model, exact) > 1e-6
    else:
        assert np.array_equal(model, q16.astype(F64)[:, 2 * heads * 64:])


@pytest.mark.parametrize("B,draws,HW", G.POSTERIOR_SIZES)
@pytest.mark.parametrize("clamp", [False, True])
def test_posterior_reference_against_the_oracle(B, draws, HW, clamp):
    c = G.posterior_case(B, draws, HW, 8, np.float32, clamp=clamp)
    m, mag = G.posterior_moments64(c)
    want_m = F.conv2d(_t(c["h"]).double().view(B, HW, 1, 8).permute(0, 3, 1, 2), _t(c["qw"]).double()[:, :, None, None], _t(c["qb"]).double())
    assert np.abs(m - want_m.reshape(B, 8, HW).numpy()).max() <= 1e-12 * max(1.0, np.abs(m).max())
    assert (np.abs(m) <= mag + np.abs(c["qb"].astype(F64))[None, :, None] + 1e-12).all()
    if clamp:
        assert (m[:, 4:6] == 25.0).all() and (m[:, 6:] == -40.0).all()
    else:
        assert m[:, 4:].min() > -30 and m[:, 4:].max() < 20
        assert np.abs(m[-1]).mean() > 10 * np.abs(m[0]).mean() or B == 1
    lat, mag_l = G.posterior_latent64(m, c["noise"], draws, c["scaling"])
    assert lat.shape == (B * draws, 4, HW)
    for b in range(B):                # the oracle samples one draw per moments row: image b's moments with each of its draws
        for d in range(draws):
            o = b * draws + d
            want = VR.posterior_sample(_t(m[b:b + 1]).view(1, 8, HW, 1).float(), _t(c["noise"][o:o + 1]).view(1, 4, HW, 1), c["scaling"])
            ref = want.view(4, HW).double().numpy()
            assert (np.abs(lat[o] - ref) <= 1e-5 * c["scaling"] * mag_l[o] + 1e-30).all()
    mode, _ = G.posterior_latent64(m, None, draws, c["scaling"])
    assert np.array_equal(mode, np.repeat(m[:, :4], draws, axis=0) * c["scaling"])
    if clamp:
        std = (lat / c["scaling"] - np.repeat(m[:, :4], draws, axis=0)) / c["noise"].astype(F64)
        assert np.allclose(std[:, :2], np.exp(10.0)) and np.allclose(std[:, 2:], np.exp(-15.0), rtol=1e-6, atol=0)


def test_add_noise32_and_sqerr32_are_the_torch_fp32_operations():
    r = G.rng(1)
    x, eps = r.standard_normal((2, 1027)).astype(np.float32), r.standard_normal((3, 1027)).astype(np.float32)
    t, xi = np.array([-5, 500, 2 ** 40], dtype=np.int64), np.array([1, 0, 1], dtype=np.int32)
    sa, sb = G.noise_tables(np.float32)
    got = G.add_noise(x, xi, eps, t, sa, sb)
    tt = _t(G.clamp_t(t))
    want = _t(sa)[tt][:, None] * _t(x)[_t(xi).long()] + _t(sb)[tt][:, None] * _t(eps)
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    assert (R.add_noise(_t(x)[_t(xi).long()], _t(eps), tt) - want).abs().max() < 5e-6       # the oracle's own tables: a few fp32 ulps from these
    assert np.array_equal(G.sqerr32(x[0], eps[0]), F.mse_loss(_t(x[0]), _t(eps[0]), reduction="none").numpy())


def test_sinusoid_against_the_oracle():
    t = np.array([0, 1, 500, 999], dtype=np.int64)
    got, arg = G.sinusoid64(t, 320)
    want = R.timestep_sinusoid(_t(t), 320).double().numpy()          # fp32: [cos | sin]
    assert got.shape == (4, 320) and arg.shape == (4, 160)
    bound = np.concatenate([arg, arg], 1) * 2.0 ** -21 + 2.0 ** -22
    print(f"sinusoid: torch fp32 vs float64, worst |err| / bound = {(np.abs(want - got) / bound).max():.3f}")
    assert np.abs(want - got).max() < 1e-4                            # the oracle's fp32 argument rounding at t f ~ 1e3
    assert np.array_equal(got[0], np.concatenate([np.ones(160), np.zeros(160)]))


def test_activations_against_torch_float64():
    x = np.concatenate([G.finite_fp16().astype(F64), np.linspace(-90, 90, 4099)])
    xt = _t(x)
    assert np.allclose(G.silu64(x), F.silu(xt).numpy(), rtol=1e-14, atol=1e-300)
    assert np.allclose(G.quick_gelu64(x), (xt * torch.sigmoid(1.702 * xt)).numpy(), rtol=1e-13, atol=1e-300)
    assert not np.isnan(G.silu64(x)).any() and not np.isnan(G.quick_gelu64(x)).any()


def test_fp32_formula_counts_behind_the_caps():
    """The caps of the fp16 SiLU / quick-GELU tests are 2 * these + 16: how often the kernels' own formula, evaluated in IEEE fp32 by
    numpy and cast to fp16, misses the correctly rounded float64 value over all finite fp16 inputs.  (A libm with another exp may move a
    count by a few.)"""
    silu, qgelu = G.f32_formula_misrounded(1.0), G.f32_formula_misrounded(1.702)
    print(f"fp32-formula results that are not correctly rounded: SiLU {silu}, quick-GELU {qgelu} of 63488")
    assert abs(silu - G.SILU_F32_MISROUNDED) <= 4 and abs(qgelu - G.QGELU_F32_MISROUNDED) <= 4


def test_small_references():
    tab = G.rng(2).standard_normal((1000, 320)).astype(np.float16)
    t = np.array([-5, 0, 1, 500, 999, 1000, 2 ** 40], dtype=np.int64)
    assert np.array_equal(G.time_gather(tab, t), tab[[0, 0, 1, 500, 999, 999, 999]])
    x = G.rng(3).standard_normal((2, 15, 40)).astype(np.float32)
    assert np.array_equal(G.nhwc_to_nchw(x), _t(x).view(2, 5, 3, 40).permute(0, 3, 1, 2).reshape(2, 40, 15).numpy())
    m, a = G.ensemble_mean64(x, 1, 2)
    assert np.allclose(m[0], (x[0].astype(F64) + x[1]).T / 2) and (a >= np.abs(m)).all()
    tok, pos = G.rng(4).standard_normal((101, 16)).astype(np.float16), G.rng(5).standard_normal((7, 16)).astype(np.float16)
    ids = G.clip_ids(20, 101, 6)
    assert set([-3, 0, 100, 101, 49407]) <= set(ids.tolist())
    e = G.clip_embed(ids, tok, pos, 7)
    assert np.array_equal(e[0], tok[0] + pos[0]) and np.array_equal(e[3], tok[100] + pos[3]) and np.array_equal(e[8], tok[ids[8]] + pos[1])
    e32 = G.clip_embed(ids, tok.astype(np.float32), pos.astype(np.float32), 7)
    assert e32.dtype == np.float32 and np.array_equal(e32[4], tok[100].astype(np.float32) + pos[4].astype(np.float32))
    for sz in G.CONV_IN_SIZES:
        xw = G.conv_in_case(*sz)
        wk = G.conv_in_pack(xw[1])
        assert wk.shape == (sz[1] * 9, sz[4]) and wk[(1 * 3 + 2) * 3 + 0, 5] == xw[1][5, 1, 2, 0]
