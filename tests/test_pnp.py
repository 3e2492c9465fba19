"""CPU tier of the parallel-dataset generator (diff_mining_amd.pnp): the DDIM schedules and coefficient tables against the reference's loops
restated in tests/pnp_ref.py (bit for bit), the injection plan, the decoder's tensor inventory, and the monkeypatched injected reference
that the GPU tier compares against."""
import numpy as np
import pytest
import torch

from diff_mining_amd import pnp as P
from diff_mining_amd import vae_spec as VS
from oracle import unet_ref as R
from tests import pnp_ref as PR


def test_ddim_timesteps():
    t50 = P.ddim_timesteps(50)
    assert t50.dtype == np.int64 and t50.tolist() == list(range(981, 0, -20))
    assert P.ddim_timesteps(999).tolist() == list(range(999, 0, -1))
    with pytest.raises(ValueError):
        P.ddim_timesteps(0)


def test_alphas_cumprod_is_the_scheduler_table():
    assert torch.equal(P.alphas_cumprod(), R.alphas_cumprod())


@pytest.mark.parametrize("n", [50, 999])
def test_coefficient_tables_equal_the_reference_expressions(n):
    acp = R.alphas_cumprod()
    ts = P.ddim_timesteps(n)
    inv = ts[::-1].copy()
    ci, cs, cp = P.ddim_coefficients(inv, "invert"), P.ddim_coefficients(ts, "sample"), P.ddim_coefficients(ts, "step")
    assert ci.shape == cs.shape == cp.shape == (n, 4) and ci.dtype == np.float32
    for i in (0, 1, n // 2, n - 1):
        t = int(inv[i])
        a, ap = acp[t], (acp[int(inv[i - 1])] if i > 0 else acp[0])
        want = torch.stack([a ** 0.5, (1 - ap) ** 0.5, ap ** 0.5, (1 - a) ** 0.5]).numpy()
        assert np.array_equal(ci[i].view(np.uint32), want.view(np.uint32)), ("invert", i)
        t = int(ts[i])
        a, ap = acp[t], (acp[int(ts[i + 1])] if i < n - 1 else acp[0])
        want = torch.stack([ap ** 0.5, (1 - a) ** 0.5, a ** 0.5, (1 - ap) ** 0.5]).numpy()
        assert np.array_equal(cs[i].view(np.uint32), want.view(np.uint32)), ("sample", i)
        prev = t - 1000 // n
        ap = acp[prev] if prev >= 0 else acp[0]
        want = torch.stack([ap ** 0.5, (1 - a) ** 0.5, a ** 0.5, (1 - ap) ** 0.5]).numpy()
        assert np.array_equal(cp[i].view(np.uint32), want.view(np.uint32)), ("step", i)
    with pytest.raises(ValueError):
        P.ddim_coefficients(ts, "nope")


def _stub_eps(x, t):
    """any fixed elementwise function of x and t"""
    return torch.sin(x * 1.7 + 0.013 * t) * 0.9 + 0.05 * x


def test_loops_and_table_updates_give_identical_bits():
    """pnp.py's three loops (tests/pnp_ref.py) against "table row + four-scalar update": pins the rows, their order and the
    final_alpha_cumprod ends."""
    acp = R.alphas_cumprod()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 4, 5, 7, generator=g)
    for n in (7, 50):
        ts = P.ddim_timesteps(n)
        inv = ts[::-1].copy()
        want, want_traj = PR.ddim_inversion(_stub_eps, x0, ts, acp)
        x, ci = x0, P.ddim_coefficients(inv, "invert")
        for i, t in enumerate(inv):
            x = PR.table_update(x, _stub_eps(x, int(t)), ci[i])
            assert torch.equal(x, want_traj[int(t)]), ("invert", n, i)
        assert torch.equal(x, want)
        want = PR.ddim_sample(_stub_eps, x, ts, acp)
        y, cs = x, P.ddim_coefficients(ts, "sample")
        for i, t in enumerate(ts):
            y = PR.table_update(y, _stub_eps(y, int(t)), cs[i])
        assert torch.equal(y, want), ("sample", n)
        # the PnP loop: stub eps on the reference's 3B rows, guidance, DDIMScheduler.step
        lat = {int(t): torch.randn(1, 4, 5, 7, generator=g) for t in ts}
        gs = 7.5

        def eps3(xx, t):                                                     # the conditional third answers differently
            e = _stub_eps(xx, t)
            return torch.cat([e[:4], e[4:] * 1.25 + 0.01])
        want = PR.pnp_sample_loop(eps3, x0, lat, ts, acp, gs)
        z, cp = x0, P.ddim_coefficients(ts, "step")
        for i, t in enumerate(ts):
            eu = _stub_eps(z, int(t))
            ec = _stub_eps(z, int(t)) * 1.25 + 0.01
            z = PR.table_update(z, eu + gs * (ec - eu), cp[i])
        assert torch.equal(z, want), ("step", n)


def test_injection_plan_defaults():
    conv_on, attn_on, conv_mask, attn_mask = P.injection_plan(50)
    assert conv_on.dtype == np.uint8 and conv_on.sum() == 40 and conv_on[:40].all() and not conv_on[40:].any()
    assert attn_on.sum() == 25 and attn_on[:25].all() and not attn_on[25:].any()
    assert conv_mask == 1 << 4                                               # plotum: rbf = {1: [1]}
    assert attn_mask == sum(1 << (3 * r + b) for r, bs in {1: [1, 2], 2: [0, 1, 2], 3: [0, 1, 2]}.items() for b in bs)
    assert P.layer_mask([(-1, 0), (-1, 1)]) == (1 << 12) | (1 << 13)
    with pytest.raises(ValueError):
        P.layer_mask([(4, 0)])
    assert P.injection_plan(999)[0].sum() == 799 and P.injection_plan(999)[1].sum() == 499


def test_decoder_inventory():
    spec = VS.vae_decoder_tensor_spec()
    dec = [(n, s) for n, s in spec if n.startswith("decoder.")]
    assert len(dec) == 138 and sum(int(np.prod(s)) for _, s in dec) == 49_490_179
    assert len(spec) == 140 and VS.vae_decoder_param_count() == 49_490_199
    assert len({n for n, _ in spec}) == 140
    d = dict(spec)
    assert d["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert d["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in d and d["decoder.conv_out.weight"] == (3, 128, 3, 3)


def test_canonical_decoder_names():
    f = VS.canonical_vae_decoder_name
    assert f("vae.decoder.conv_in.weight") == "decoder.conv_in.weight"
    assert f("decoder.mid_block.attentions.0.query.weight") == "decoder.mid_block.attentions.0.to_q.weight"
    assert f("vae.decoder.mid_block.attentions.0.proj_attn.bias") == "decoder.mid_block.attentions.0.to_out.0.bias"
    assert f("post_quant_conv.bias") == "post_quant_conv.bias"
    assert f("encoder.conv_in.weight") is None and f("vae.quant_conv.weight") is None
    assert VS.canonical_vae_name("decoder.conv_in.weight") is None           # the encoder's set keeps ignoring the decoder


def test_injected_reference(sd15_weights_torch, monkeypatch):
    """The monkeypatched oracle: with no layer selected it is plain unet_forward to the bit; with the default layers it moves the target
    rows and leaves the source rows alone."""
    B, h, w = 1, 8, 8
    g = torch.Generator().manual_seed(11)
    sample = torch.randn(3 * B, 4, h, w, generator=g)
    ctx = torch.randn(3 * B, 77, 768, generator=g)
    t = torch.tensor(581)
    plain = R.unet_forward(sd15_weights_torch, sample, t, ctx)
    PR.install_injection(monkeypatch)
    assert torch.equal(R.unet_forward(sd15_weights_torch, sample, t, ctx), plain)
    PR.install_injection(monkeypatch, P.DEFAULT_CONV_LAYERS, P.DEFAULT_ATTN_LAYERS)
    inj = R.unet_forward(sd15_weights_torch, sample, t, ctx)
    assert torch.equal(inj[:B], plain[:B])
    rel = ((inj[B:] - plain[B:]).norm() / plain[B:].norm()).item()
    print(f"injected vs plain target rows: rel-L2 {rel:.3e}")
    assert rel > 1e-3
