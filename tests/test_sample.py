"""CPU tier of text-to-image sampling (diff_mining_amd/sample.py): the coefficient table and the restated guided step against
tests/sample_ref.py bit for bit, the type promotion the step pins, and the decoder's weight inventory.  No GPU."""
import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd import pnp as P
from diff_mining_amd import sample as S
from diff_mining_amd import synth, vae_spec
from tests import sample_ref as SR


def _randn(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _stub_eps(x2, t):
    """a stand-in for the autocast U-Net: any deterministic fp16 function of (latent_model_input, t) with distinct halves"""
    B = x2.shape[0] // 2
    s = torch.cat([torch.full((B, 1, 1, 1), 0.9), torch.full((B, 1, 1, 1), -1.1)])
    return (torch.sin(x2 * s + 0.013 * t) * 1.3).half()


def test_timesteps_and_table_shape():
    ts = S.sample_timesteps(50)
    assert ts[0] == 981 and ts[-1] == 1 and len(ts) == 50 and np.all(np.diff(ts) == -20)
    tab = S.sample_coefficients(ts)
    assert tab.shape == (50, 4) and tab.dtype == np.float32
    acp = P.alphas_cumprod()
    # first row: t = 981, prev = 961; last row: prev < 0 -> final_alpha_cumprod = acp[0] (set_alpha_to_one = False)
    assert tab[0].tolist() == [float(acp[961] ** 0.5), float((1 - acp[981]) ** 0.5), float(acp[981] ** 0.5), float((1 - acp[961]) ** 0.5)]
    assert tab[-1].tolist() == [float(acp[0] ** 0.5), float((1 - acp[1]) ** 0.5), float(acp[1] ** 0.5), float((1 - acp[0]) ** 0.5)]
    assert np.array_equal(tab, P.ddim_coefficients(ts, "step"))          # eta = 0: the scheduler's own detour through std_dev_t changes nothing
    with pytest.raises(ValueError):
        S.sample_coefficients([])
    with pytest.raises(ValueError):
        S.sample_coefficients([1000])


@pytest.mark.parametrize("n", [50, 3])
def test_table_plus_restated_update_is_the_reference_loop(n):
    """`row of the table + the restated update`, step by step, equals sample_ref.sample_loop bit for bit with a stub eps — the first row
    (t = 981 at n = 50) and the last (a_prev = acp[0]) included."""
    ts = S.sample_timesteps(n)
    tab = S.sample_coefficients(ts)
    acp = P.alphas_cumprod()
    x0 = _randn(2, 4, 5, 7, seed=n)
    want = SR.sample_loop(_stub_eps, x0, ts, acp, 7.5)
    x = x0.clone()
    for i, t in enumerate(ts):
        x_next = SR.table_update(x, _stub_eps(torch.cat([x] * 2), int(t)), tab[i], 7.5)
        if i in (0, len(ts) - 1):                                           # the first and the last row on their own
            step = SR.scheduler_step_autocast(SR.guided_noise(_stub_eps(torch.cat([x] * 2), int(t)), 7.5), int(t), x, n, acp)
            assert torch.equal(step, x_next), i
        x = x_next
    assert x.dtype == torch.float32 and torch.equal(x, want)
    assert torch.isfinite(x).all()


def test_the_step_is_not_an_fp32_evaluation():
    """The promotion is what is pinned: the restated step differs from the same formula evaluated with everything widened to fp32, on the
    same inputs — for the guidance combination and for the scheduler's two fp16 products alike."""
    ts = S.sample_timesteps(50)
    acp = P.alphas_cumprod()
    x = _randn(2, 4, 8, 8, seed=5)
    eps16 = _stub_eps(torch.cat([x] * 2), 981)
    for i in (0, 25, 49):
        t = int(ts[i])
        e16 = SR.guided_noise(eps16, 7.5)
        a = SR.scheduler_step_autocast(e16, t, x, 50, acp)
        b = SR.scheduler_step_fp32(e16, t, x, 50, acp)
        assert a.dtype == b.dtype == torch.float32
        assert not torch.equal(a, b), i
        # ... by the two fp16 roundings, nothing more: each product is off by <= 2^-11 |e|, the first enters scaled by c0 / c2
        c0, _, c2, _ = S.sample_coefficients(ts)[i]
        assert (a - b).abs().max() <= 2.0 ** -11 * float(e16.float().abs().max()) * (c0 / c2 + 1) * 1.01
    u, c = eps16.float().chunk(2)
    assert not torch.equal(SR.guided_noise(eps16, 7.5).float(), u + 7.5 * (c - u))


def test_promotion_rules_are_torchs():
    """what sample_ref writes out by hand is what torch's promotion decides: a 0-dim fp32 tensor or a Python scalar times an fp16 tensor is
    fp16; fp32 minus / plus fp16 is fp32; `tensor * scalar` on the CPU is the fp32 op-math product sample_ref._mul16 spells out."""
    e = _randn(4, 4, 8, 8, seed=9).half()
    s = torch.tensor(0.7123456, dtype=torch.float32)
    x = _randn(4, 4, 8, 8, seed=10)
    assert (s * e).dtype == torch.float16 and (7.5 * e).dtype == torch.float16 and (e * s).dtype == torch.float16
    assert (x - e).dtype == torch.float32 and (x + e).dtype == torch.float32
    assert torch.equal(x - e, x - e.float())
    assert torch.equal(e * s, SR._mul16(s, e)) and torch.equal(7.5 * e, SR._mul16(7.5, e))


def test_postprocess_rounds_where_pilify_truncates():
    raw = torch.tensor([[-1.5, -1.0, -0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.7, float("nan")]] * 3, dtype=torch.float16).reshape(1, 3, 1, 10)
    u8 = SR.postprocess_pil(raw)
    assert u8.shape == (1, 1, 10, 3) and u8.dtype == np.uint8
    assert u8[0, 0, :, 0].tolist() == [0, 0, 64, 128, 159, 191, 223, 255, 255, 0]          # 63.75 -> 64, 127.5 -> 128 (half to even)
    trunc = ((raw / 2 + 0.5).clamp(0, 1).float().permute(0, 2, 3, 1).numpy() * 255)
    assert np.nan_to_num(trunc).astype(np.uint8)[0, 0, 2, 0] == 63


def test_decoder_inventory():
    spec = vae_spec.vae_decoder_tensor_spec()
    assert len(spec) == 140 and vae_spec.vae_decoder_param_count() == 49_490_199
    sd = synth.synth_vae_decoder_state_dict()
    assert set(sd) == {n for n, _ in spec} and sum(int(v.size) for v in sd.values()) == 49_490_199
    assert all(tuple(sd[n].shape) == tuple(shp) for n, shp in spec)


def test_loader_refuses_an_incomplete_decoder_set():
    """the Python binding's own check, before anything is staged: it needs neither the library nor a GPU"""
    spec = vae_spec.vae_decoder_tensor_spec()
    eng = object.__new__(E.UNetEngine)               # no handle: the refusal must come before the first C call
    full = {n: np.zeros(shp, dtype=np.float16) for n, shp in spec}
    for drop in ("post_quant_conv.bias", "decoder.up_blocks.3.resnets.0.conv_shortcut.weight", "decoder.conv_out.weight"):
        sd = {("vae." + k): v for k, v in full.items() if k != drop}
        with pytest.raises(E.EngineError, match="1 of the 140 decoder tensors are missing"):
            E.UNetEngine.load_vae_decoder_state_dict(eng, sd)
    with pytest.raises(E.EngineError, match="140 of the 140"):
        E.UNetEngine.load_vae_decoder_state_dict(eng, {"encoder.conv_in.weight": np.zeros((128, 3, 3, 3), np.float16)})
    # the pre-0.15 attention names count as the tensors they are
    legacy = {k.replace(".to_q.", ".query.").replace(".to_k.", ".key.").replace(".to_v.", ".value.").replace(".to_out.0.", ".proj_attn."): v
              for k, v in full.items() if k != "decoder.conv_out.bias"}
    with pytest.raises(E.EngineError, match="first: decoder.conv_out.bias"):
        E.UNetEngine.load_vae_decoder_state_dict(eng, legacy)


def test_slots_are_checked_on_the_host():
    class _Eng:
        n_prompts = 3
    with pytest.raises(E.EngineError, match="slot 3"):
        S.sample_latents(_Eng(), torch.zeros(2, 4, 8, 8), [0, 3], [1, 1], steps=3)
    with pytest.raises(E.EngineError, match="slot -1"):
        S.sample_latents(_Eng(), torch.zeros(2, 4, 8, 8), [0, 1], [-1, 1], steps=3)
    with pytest.raises(E.EngineError, match="steps 0"):
        S.sample_latents(_Eng(), torch.zeros(2, 4, 8, 8), [0, 1], [1, 1], steps=0)
    with pytest.raises(ValueError):
        S.sample_latents(_Eng(), torch.zeros(2, 4, 8, 8), [0], [1, 1], steps=3)
