"""The parallel-dataset generator on the GPU (dm_f32_vae_decode, dm_f32_op_ddim_step[_cfg], dm_f32_ddim_run, dm_f32_pnp_run,
dm_f32_unet_forward_inject) against tests/pnp_ref.py, the torch-fp32 CPU restatement of the reference's pnp.py (parity unpinned: see its
header), and against its own pieces composed in Python.

Tolerances: both sides compute in fp32 and differ in summation order only, so the end-to-end bound of tests/test_gpu_f32.py holds
(TOL_E2E = 2e-5, derived in that file's header).  Everything that is elementwise, or the same kernels in another composition, is compared
bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import pnp as P  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from oracle import unet_ref as R  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import pnp_ref as PR  # noqa: E402

TOL_E2E = 2e-5          # tests/test_gpu_f32.py
N_PROMPTS = 4


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def dec_sd():
    return {k: torch.from_numpy(v) for k, v in synth.synth_vae_decoder_state_dict().items()}        # fp16-valued, widened


@pytest.fixture(scope="module")
def ctx():
    return _randn(N_PROMPTS, 77, 768, seed=77)


@pytest.fixture(scope="module")
def net32(sd15_weights_f16, dec_sd, ctx):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = E.UNetEngineF32(0)
    e.load_state_dict(sd15_weights_f16)
    e.load_vae_decoder_state_dict(dec_sd)
    e.load_vae_state_dict(synth.synth_vae_state_dict())        # the encoder, for extract_latents
    e.set_prompts(ctx)
    yield e
    e.close()


@pytest.fixture
def up_fold_restored():
    before = E.get_options(("up_fold",))["up_fold"]
    yield
    assert E.load_library().dm_set_option(b"up_fold", before) == 0


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
_DEC_CASES = {"8x8": (2, 8, 8, 21), "5x7": (1, 5, 7, 22)}
_dec_ref = {}


def _decoder_case(dec_sd, key):
    """latent and the reference's raw sample, computed once.  The latents are N(0, 1): on the CPU 86 % / 92 % of the reference's raw values
    lie strictly inside (-1, 1), so the clamp does not hide the convolution."""
    if key not in _dec_ref:
        B, h, w, seed = _DEC_CASES[key]
        lat = _randn(B, 4, h, w, seed=seed)
        raw = PR.vae_decode_raw(dec_sd, lat)
        assert (raw.abs() < 1).float().mean().item() >= 0.5
        _dec_ref[key] = (lat, raw)
    return _dec_ref[key]


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("key", list(_DEC_CASES))
def test_decoder_raw_against_the_reference(net32, dec_sd, up_fold_restored, key, fold):
    lat, ref = _decoder_case(dec_sd, key)
    assert net32.lib.dm_set_option(b"up_fold", fold) == 0
    got = net32.vae_decode(lat, raw=True).cpu()
    r = U.rel_l2(got, ref)
    print(f"decoder raw {key} up_fold {fold}: rel-L2 {r:.2e}")
    assert got.shape == ref.shape and r < TOL_E2E


@pytest.mark.parametrize("key", list(_DEC_CASES))
def test_decoder_postprocessing_is_torchs_bit_for_bit(net32, dec_sd, key):
    lat, _ = _decoder_case(dec_sd, key)
    raw = net32.vae_decode(lat, raw=True).cpu()
    img, u8 = net32.vae_decode(lat, want="both")
    want = PR.postprocess(raw)
    assert torch.equal(img.cpu(), want)
    assert np.array_equal(u8.cpu().numpy(), PR.pilify(want))
    assert np.array_equal(net32.vae_decode(lat, want="u8").cpu().numpy(), PR.pilify(want))
    assert 0.02 < (want == 0).float().mean() + (want == 1).float().mean() < 0.5          # the clamp is exercised, and is not everything


# ---- the update kernels -----------------------------------------------------------------------------------------------------------------
def _op_step(x, eps, row, eps_c=None, g=0.0):
    lib = E.load_library()
    coef = torch.from_numpy(np.asarray(row, dtype=np.float32)).cuda()
    out = torch.empty_like(x)
    if eps_c is None:
        rc = lib.dm_f32_op_ddim_step(U.stream(), U.ptr(x), U.ptr(eps), U.ptr(coef), x.numel(), U.ptr(out))
    else:
        rc = lib.dm_f32_op_ddim_step_cfg(U.stream(), U.ptr(x), U.ptr(eps), U.ptr(eps_c), float(g), U.ptr(coef), x.numel(), U.ptr(out))
    assert rc == 0
    torch.cuda.synchronize()
    return out


def _near_one_row():
    """a row of the 999-step inversion table with c0 / c2 within 1e-3 of 1"""
    tab = P.ddim_coefficients(P.ddim_timesteps(999)[::-1].copy(), "invert")
    i = int(np.argmin(np.abs(tab[:, 0] / tab[:, 2] - 1)))
    assert abs(tab[i, 0] / tab[i, 2] - 1) < 1e-3
    return tab[i]


def test_update_kernels_bit_equal_to_torch():
    rows = [_near_one_row(), P.ddim_coefficients(P.ddim_timesteps(50), "step")[0], P.ddim_coefficients(P.ddim_timesteps(50), "sample")[-1]]
    x, eu, ec = _randn(3, 4, 9, 7, seed=1), _randn(3, 4, 9, 7, seed=2), _randn(3, 4, 9, 7, seed=3)
    for row in rows:
        c0, c1, c2, c3 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
        want = c0 * ((x - c1 * eu) / c2) + c3 * eu
        assert torch.equal(_op_step(x.cuda(), eu.cuda(), row).cpu(), want)
        eps = eu + 7.5 * (ec - eu)
        want = c0 * ((x - c1 * eps) / c2) + c3 * eps
        assert torch.equal(_op_step(x.cuda(), eu.cuda(), row, ec.cuda(), 7.5).cpu(), want)


# ---- the loops --------------------------------------------------------------------------------------------------------------------------
def test_ddim_run_equals_its_steps_composed(net32):
    ts = np.array([1, 251, 501, 751], dtype=np.int64)
    coef = P.ddim_coefficients(ts, "invert")
    x0 = _randn(2, 4, 8, 8, seed=5).cuda()
    slots = [1, 2]
    save = [0, -1, 2, 1]                                   # a skipped step, rows out of order
    got, traj = net32.ddim_run(x0, ts, coef, slots, save_rows=save, n_rows=3)
    x, rows = x0, {}
    for i, t in enumerate(ts):
        x = _op_step(x, net32.unet(x, int(t), slots), coef[i])
        rows[save[i]] = x
    assert torch.equal(got, x)
    for r in (0, 1, 2):
        assert torch.equal(traj[r], rows[r])
    # a batch of two images = two single-image runs
    for b in (0, 1):
        one, _ = net32.ddim_run(x0[b:b + 1], ts, coef, slots[b:b + 1])
        assert torch.equal(one[0], got[b])


def test_loops_queued_back_to_back_on_a_side_stream(net32):
    """Two loops queued one behind the other on a non-blocking side stream (which the null stream does not wait for): the second call
    uploads its own timestep and coefficient tables into the net's loop buffer, and must do so behind the first loop's pending steps."""
    ts = P.ddim_timesteps(4)
    inv_ts = ts[::-1].copy()
    ci, cs = P.ddim_coefficients(inv_ts, "invert"), P.ddim_coefficients(ts, "sample")
    x0 = _randn(2, 4, 8, 8, seed=8).cuda()
    want_inv, _ = net32.ddim_run(x0, inv_ts, ci, [1, 2])
    want_rec, _ = net32.ddim_run(want_inv, ts, cs, [1, 2])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inv, _ = net32.ddim_run(x0, inv_ts, ci, [1, 2])
        rec, _ = net32.ddim_run(inv, ts, cs, [1, 2])
        src = torch.stack([inv[0], rec[0], inv[1], rec[1]])
        pnp = net32.pnp_run(rec, src, ts, P.ddim_coefficients(ts, "step"), [1, 1, 0, 0], [1, 0, 0, 0], 16, 16, [0, 0, 3, 1, 2])
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(inv, want_inv) and torch.equal(rec, want_rec)
    assert torch.equal(pnp, net32.pnp_run(want_rec, src, ts, P.ddim_coefficients(ts, "step"), [1, 1, 0, 0], [1, 0, 0, 0], 16, 16, [0, 0, 3, 1, 2]))


def test_pnp_run_equals_its_steps_composed(net32):
    B, n = 2, 3
    ts = P.ddim_timesteps(n)
    coef = P.ddim_coefficients(ts, "step")
    conv_mask, attn_mask = P.layer_mask(P.DEFAULT_CONV_LAYERS), P.layer_mask(P.DEFAULT_ATTN_LAYERS)
    conv_on, attn_on = [1, 1, 0], [1, 0, 0]
    src = _randn(n, 4, 8, 8, seed=6).cuda()
    x0 = _randn(B, 4, 8, 8, seed=7).cuda()
    slots = [0, 0, 3, 1, 2]
    got = net32.pnp_run(x0, src, ts, coef, conv_on, attn_on, conv_mask, attn_mask, slots, guidance_scale=7.5)
    x = x0
    for i, t in enumerate(ts):
        eps = net32.unet_inject(torch.cat([src[i:i + 1], x, x]), int(t), slots, conv_mask if conv_on[i] else 0, attn_mask if attn_on[i] else 0)
        x = _op_step(x, eps[1:1 + B].contiguous(), coef[i], eps[1 + B:].contiguous(), 7.5)
    assert torch.equal(got, x)
    for b in (0, 1):
        one = net32.pnp_run(x0[b:b + 1], src, ts, coef, conv_on, attn_on, conv_mask, attn_mask, [slots[0], slots[1 + b], slots[1 + B + b]], 7.5)
        assert torch.equal(one[0], got[b])


# ---- the injected forward ------------------------------------------------------------------------------------------------------------------
_INJ_FLAGS = {"conv": (True, False), "attn": (False, True), "both": (True, True)}
_inj_inputs = {}


def _inject_inputs(hw):
    if hw not in _inj_inputs:
        B = 2
        _inj_inputs[hw] = (_randn(1 + 2 * B, 4, *hw, seed=hw[0] * 100 + hw[1]), [0, 3, 0, 1, 2], 581)
    return _inj_inputs[hw]


@pytest.mark.parametrize("flags", list(_INJ_FLAGS))
@pytest.mark.parametrize("hw", [(8, 8), (16, 12)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_injected_forward_against_the_monkeypatched_reference(net32, sd15_weights_torch, ctx, monkeypatch, hw, flags):
    B = 2
    sample, slots, t = _inject_inputs(hw)
    conv, attn = _INJ_FLAGS[flags]
    conv_mask = P.layer_mask(P.DEFAULT_CONV_LAYERS) if conv else 0
    attn_mask = P.layer_mask(P.DEFAULT_ATTN_LAYERS) if attn else 0
    got = net32.unet_inject(sample, t, slots, conv_mask, attn_mask).cpu()
    plain = net32.unet(sample, t, slots).cpu()
    PR.install_injection(monkeypatch, P.DEFAULT_CONV_LAYERS if conv else (), P.DEFAULT_ATTN_LAYERS if attn else ())
    ref3 = R.unet_forward(sd15_weights_torch, PR.to_reference_rows(sample, B), torch.tensor(t), PR.to_reference_rows(ctx[slots], B))
    ref = torch.cat([ref3[:1], ref3[B:]])                  # reference row B + i <-> row 1 + i here; its B source rows are identical
    assert torch.equal(ref3[0], ref3[B - 1])
    r = U.rel_l2(got, ref)
    moved = U.rel_l2(got[1:], plain[1:])
    print(f"injected forward {hw} {flags}: rel-L2 {r:.2e}; injected vs plain target rows {moved:.2e}")
    assert r < TOL_E2E
    assert max(U.rel_l2(got[i], ref[i]) for i in range(1 + 2 * B)) < TOL_E2E
    assert moved > 100 * TOL_E2E                           # the test cannot pass with the injection silently off
    assert torch.equal(got[0], plain[0])                   # the source row is the source's own forward ...
    assert torch.equal(got[:1], net32.unet(sample[:1], t, slots[:1]).cpu())      # ... run alone
    assert torch.equal(net32.unet_inject(sample, t, slots, 0, 0).cpu(), plain)    # masks of 0: the bits of the plain forward


# ---- one free-running pass -------------------------------------------------------------------------------------------------------------------
def test_free_running_inversion_reconstruction_decode(net32, sd15_weights_torch, dec_sd, ctx):
    """2 inversion steps + 2 reconstruction steps + decode at 8 x 8 against tests/pnp_ref.py.  A conforming implementation may differ from
    the reference's eps by TOL_E2E at every step, so the bound is measured: the CPU restatement runs a second time with each eps perturbed
    by a random field of relative L2 norm TOL_E2E, and the device must stay within twice that run's distance from the unperturbed one (one
    random draw is not the worst case) on the inverted latent, the reconstructed latent and the decoded sample alike.  Measured: device
    2.4e-6, 4.6e-6, 5.2e-6; perturbed reference 1.4e-5, 2.8e-5, 2.7e-5."""
    acp = R.alphas_cumprod()
    ts = P.ddim_timesteps(2)
    x0 = _randn(1, 4, 8, 8, seed=31)
    slot = 2

    def eps_fn(x, t):
        return R.unet_forward(sd15_weights_torch, x, torch.tensor(t), ctx[slot:slot + 1])

    gen = torch.Generator().manual_seed(32)

    def eps_perturbed(x, t):
        e = eps_fn(x, t)
        n = torch.randn(e.shape, generator=gen)
        return e + n * (TOL_E2E * e.norm() / n.norm())

    def run(fn):
        inv, _ = PR.ddim_inversion(fn, x0, ts, acp)
        rec = PR.ddim_sample(fn, inv, ts, acp)
        return inv, rec, PR.vae_decode_raw(dec_sd, rec)

    ref, pert = run(eps_fn), run(eps_perturbed)
    inv_ts = ts[::-1].copy()
    inv, _ = net32.ddim_run(x0, inv_ts, P.ddim_coefficients(inv_ts, "invert"), [slot])
    rec, _ = net32.ddim_run(inv, ts, P.ddim_coefficients(ts, "sample"), [slot])
    img = net32.vae_decode(rec, raw=True)
    d_dev = [U.rel_l2(a, b) for a, b in zip((inv, rec, img), ref)]
    d_pert = [U.rel_l2(a, b) for a, b in zip(pert, ref)]
    print("free-running rel-L2 (inverted, reconstructed, decoded): device " + " ".join(f"{v:.2e}" for v in d_dev)
          + " | perturbed reference " + " ".join(f"{v:.2e}" for v in d_pert))
    assert all(d <= 2 * p for d, p in zip(d_dev, d_pert)), (d_dev, d_pert)


def test_extract_latents_is_its_stages(net32):
    """`pnp.extract_latents` = posterior-mode encode, inversion, reconstruction, decode, with the kept trajectory rows"""
    img = torch.from_numpy(synth.synth_image(1, 64, 64)).float()
    ts = P.ddim_timesteps(2)
    inv_ts = ts[::-1].copy()
    u8, inverted, (traj, kept) = P.extract_latents(net32, img, [1], steps=2, keep=[int(ts[0])])
    lat = net32.vae_encode(img, noise=None)
    inv, _ = net32.ddim_run(lat, inv_ts, P.ddim_coefficients(inv_ts, "invert"), [1])
    rec, _ = net32.ddim_run(inv, ts, P.ddim_coefficients(ts, "sample"), [1])
    assert kept == [int(ts[0])] and torch.equal(inverted, inv) and torch.equal(traj[0], inv)
    assert u8.shape == (1, 64, 64, 3) and u8.dtype == torch.uint8 and torch.equal(u8, net32.vae_decode(rec, want="u8"))


def test_generator_is_pnp_run_and_decode(net32):
    """`Generator.generate` on a seed of `extract_latents`: the slots of `PNP.load` (the empty-prompt branch included), the trajectory rows in
    schedule order, the default injection plan, then the decode"""
    img = torch.from_numpy(synth.synth_image(1, 64, 64)).float()
    seed = P.extract_latents(net32, img, [1], steps=2)
    gen = P.Generator(net32, seed, uncond_slot=1, base_slot=0, n_timesteps=2)
    got = gen.generate([2, 3], empty=[False, True])
    assert gen.pnp.slots == [1, 1, 0, 2, 3]
    ts = P.ddim_timesteps(2)
    _, inverted, (rows, kept) = seed
    assert kept == [1, 501]
    src = torch.stack([rows[kept.index(int(t)), 0] for t in ts])
    conv_on, attn_on, conv_mask, attn_mask = P.injection_plan(2)
    x = net32.pnp_run(inverted.expand(2, -1, -1, -1), src, ts, P.ddim_coefficients(ts, "step"), conv_on, attn_on, conv_mask, attn_mask,
                      [1, 1, 0, 2, 3], 7.5)
    assert got.shape == (2, 64, 64, 3) and torch.equal(got, net32.vae_decode(x, want="u8"))


# ---- error behaviour: non-zero with a message, nothing launched ----------------------------------------------------------------------------
def test_errors(net32, sd15_weights_f16):
    bare = E.UNetEngineF32(0)
    try:
        with pytest.raises(E.EngineError, match="decoder weights"):
            bare.vae_decode(torch.zeros(1, 4, 8, 8))
        with pytest.raises(E.EngineError, match="missing tensor"):
            bare.load_vae_decoder_state_dict({"post_quant_conv.bias": np.zeros(4, np.float32)})
    finally:
        bare.close()
    ts = P.ddim_timesteps(2)
    coef = P.ddim_coefficients(ts, "step")
    x = torch.zeros(8, 4, 128, 128)                        # 1 + 2 * 8 = 17 samples over the 16 of one run at 128 x 128
    with pytest.raises(E.EngineError, match="share a run"):
        net32.pnp_run(x, torch.zeros(2, 4, 128, 128), ts, coef, [1, 1], [1, 1], 16, 16, [0] * 17)
    with pytest.raises(E.EngineError, match="prompt slot"):
        net32.ddim_run(torch.zeros(1, 4, 8, 8), ts, coef, [N_PROMPTS])
    with pytest.raises(E.EngineError, match="n_steps"):
        net32.ddim_run(torch.zeros(1, 4, 8, 8), [], np.zeros((0, 4), np.float32), [0])
    with pytest.raises(E.EngineError, match="n_steps"):
        net32.pnp_run(torch.zeros(1, 4, 8, 8), torch.zeros(0, 4, 8, 8), [], np.zeros((0, 4), np.float32), [], [], 16, 16, [0, 0, 0])
    with pytest.raises(E.EngineError, match="layer mask"):
        net32.unet_inject(torch.zeros(3, 4, 8, 8), 1, [0, 0, 0], 1 << 20, 0)
