"""The stage of the reference that WRITES a parallel dataset (`diffmining/applications/parallel-dataset/pnp.py`) on the fp32 net:
DDIM inversion and reconstruction of an image, Plug-and-Play sampling of its translations, the VAE decoder.

The reference builds its pipelines with no `torch_dtype` and runs them with no autocast (`pnp.py:121-125`, `:491-495`): plain fp32, the
arithmetic of `UNetEngineF32`.  The names mirror the reference's: `extract_latents` replaces `Preprocess.extract_latents`, `PNP` replaces
`PNP`, `Generator` replaces `Generator`.  Prompts are prompt slots of the net (`set_prompts`), not strings: tokenising is the caller's.

Scheduler arithmetic: the inversion (`:169-177`), the reconstruction (`:193-201`) and `DDIMScheduler.step` with eta = 0 and
clip_sample = False (what `:557` calls) are one expression with four scalars,

    x' = c0 * ((x - c1 * eps) / c2) + c3 * eps

and the scalars are formed here as the reference forms them — on 0-dim fp32 CPU tensors (`acp[t] ** 0.5`, `(1 - acp[t]) ** 0.5`) — so
the device computes no square root and the table is what torch computes, bit for bit.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

NUM_TRAIN_TIMESTEPS = 1000
DEFAULT_CONV_LAYERS = ((1, 1),)                                                            # plotum's rbf (pnp.py:612)
DEFAULT_ATTN_LAYERS = ((1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2))      # plotum's rbg (pnp.py:613)
MID_BIT = 12                                                                               # mask bits from here on name the mid block


def alphas_cumprod():
    """`DDIMScheduler.alphas_cumprod` of the SDv1.5 scheduler config (scaled_linear, 0.00085 .. 0.012, 1000 steps): fp32 torch, on the CPU."""
    import torch
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, NUM_TRAIN_TIMESTEPS, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def ddim_timesteps(n: int, steps_offset: int = 1) -> np.ndarray:
    """`DDIMScheduler.set_timesteps(n).timesteps` (leading spacing, steps_offset 1): 999 -> 999 .. 1; 50 -> 981, 961 .. 1."""
    if not 0 < n <= NUM_TRAIN_TIMESTEPS:
        raise ValueError(f"{n} inference steps")
    ratio = NUM_TRAIN_TIMESTEPS // n
    return (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64) + steps_offset


def ddim_coefficients(timesteps: Sequence[int], kind: str) -> np.ndarray:
    """The [n][4] fp32 table (c0, c1, c2, c3) for the steps in the order the loop takes them.

    "invert" (pnp.py:160-177; timesteps ascending = `reversed(scheduler.timesteps)`): a_prev = the previous step's alpha, `final_alpha_cumprod`
             = acp[0] at the first; (mu, sigma_prev, mu_prev, sigma).
    "sample" (pnp.py:184-201; descending): a_prev = the next step's alpha, acp[0] after the last; (mu_prev, sigma, mu, sigma_prev).
    "step"   (`DDIMScheduler.step`, eta = 0): prev_timestep = t - 1000 // n, acp[0] below 0; the same four as "sample"."""
    import torch
    acp = alphas_cumprod()
    final = acp[0]
    ts = [int(t) for t in timesteps]
    n = len(ts)
    rows = []
    for i, t in enumerate(ts):
        a_t = acp[t]
        if kind == "invert":
            a_prev = acp[ts[i - 1]] if i > 0 else final
        elif kind == "sample":
            a_prev = acp[ts[i + 1]] if i < n - 1 else final
        elif kind == "step":
            prev = t - NUM_TRAIN_TIMESTEPS // n
            a_prev = acp[prev] if prev >= 0 else final
        else:
            raise ValueError(f"kind {kind!r}")
        mu, sigma = a_t ** 0.5, (1 - a_t) ** 0.5
        mu_prev, sigma_prev = a_prev ** 0.5, (1 - a_prev) ** 0.5
        rows.append(torch.stack([mu, sigma_prev, mu_prev, sigma] if kind == "invert" else [mu_prev, sigma, mu, sigma_prev]))
    return torch.stack(rows).to(torch.float32).numpy()


def layer_mask(layers) -> int:
    """(res, block) pairs -> the mask of the net's injected forward: bit 3 * res + block for up_blocks[res]; res = -1 names the mid block
    (bits MID_BIT + block)."""
    m = 0
    for res, block in layers:
        if res == -1:
            m |= 1 << (MID_BIT + block)
        elif 0 <= res <= 3 and 0 <= block <= 2:
            m |= 1 << (3 * res + block)
        else:
            raise ValueError(f"no layer ({res}, {block})")
    return m


def injection_plan(n: int, pnp_f_t: float = 0.8, pnp_attn_t: float = 0.5, conv_layers=DEFAULT_CONV_LAYERS, attn_layers=DEFAULT_ATTN_LAYERS):
    """`run_pnp` / `init_pnp` / `plotum` (pnp.py:560-569, :612-615): features are injected at the first int(n * pnp_f_t) steps of the schedule,
    self-attention at the first int(n * pnp_attn_t).  Returns (conv_on [n] uint8, attn_on [n] uint8, conv_mask, attn_mask).
    The `or self.t == 1000` clause of pnp.py:345 / :424 never fires: these schedules end at 981 or 999."""
    conv_on = (np.arange(n) < int(n * pnp_f_t)).astype(np.uint8)
    attn_on = (np.arange(n) < int(n * pnp_attn_t)).astype(np.uint8)
    return conv_on, attn_on, layer_mask(conv_layers), layer_mask(attn_layers)


def extract_latents(net, images, prompt_slots, steps: int = 999, keep: Optional[Sequence[int]] = None):
    """`Preprocess.extract_latents` (pnp.py:205-216) for a batch: posterior-mode encode (`:150-154`), DDIM inversion, DDIM reconstruction,
    decode.  images [B,3,H,W] in [-1,1] (`process_image`, :248); prompt_slots [B]: the inversion prompt of each image.  keep: the timesteps
    whose inverted latent is kept (None: all, as the reference's `latents_`).  Returns (reconstruction uint8 [B,H,W,3], inverted
    [B,4,h,w], (rows [len(keep),B,4,h,w], kept timesteps)).  The reference inverts one image at a time; a batch is where the throughput is."""
    ts = ddim_timesteps(steps)
    inv = ts[::-1].copy()
    kept = [int(t) for t in (inv if keep is None else keep)]
    row = {t: i for i, t in enumerate(kept)}
    save = np.array([row.get(int(t), -1) for t in inv], dtype=np.int32)
    latent = net.vae_encode(images, noise=None, scaling_factor=0.18215)
    inverted, traj = net.ddim_run(latent, inv, ddim_coefficients(inv, "invert"), prompt_slots, save_rows=save, n_rows=len(kept))
    recon, _ = net.ddim_run(inverted, ts, ddim_coefficients(ts, "sample"), prompt_slots)
    return net.vae_decode(recon, want="u8"), inverted, (traj, kept)


class PNP:
    """The reference's `PNP` (pnp.py:476-577) for one source image: its inverted latent, the trajectory rows of the sampling schedule and
    the prompt slots.  uncond_slot: the reference's `uncond` (the source's prompt, or '' with uncond_ignore); base_slot: `base_prompt`."""

    def __init__(self, net, inverted, trajectory, uncond_slot: int, base_slot: int, n_timesteps: int = 50, guidance_scale: float = 7.5,
                 pnp_attn_t: float = 0.5, pnp_f_t: float = 0.8, conv_layers=DEFAULT_CONV_LAYERS, attn_layers=DEFAULT_ATTN_LAYERS):
        import torch
        self.net = net
        self.timesteps = ddim_timesteps(n_timesteps)
        rows, kept = trajectory
        at = {int(t): i for i, t in enumerate(kept)}
        missing = [int(t) for t in self.timesteps if int(t) not in at]
        if missing:
            raise ValueError(f"the trajectory lacks timesteps {missing[:4]}...")
        assert inverted.shape[0] == 1 and rows.shape[1] == 1, "one source image per PNP"
        self.eps = inverted
        self.lat = torch.stack([rows[at[int(t)], 0] for t in self.timesteps])         # `self.lat[t.item()]` (pnp.py:541) in schedule order
        self.coef = ddim_coefficients(self.timesteps, "step")
        self.plan = injection_plan(n_timesteps, pnp_f_t, pnp_attn_t, conv_layers, attn_layers)
        self.guidance_scale = float(guidance_scale)
        self.uncond_slot, self.base_slot = int(uncond_slot), int(base_slot)
        self.slots: List[int] = []

    def load(self, target_slots: Sequence[int], empty: Optional[Sequence[bool]] = None):
        """pnp.py:516-529.  target_slots: the prompt of each target; empty[i]: that target's prompt is the empty string — then its
        unconditional row gets the base prompt instead of `uncond` (the reference's first branch).  The source row carries `uncond`."""
        empty = [False] * len(target_slots) if empty is None else list(empty)
        assert len(empty) == len(target_slots)
        neg = [self.base_slot if e else self.uncond_slot for e in empty]
        self.slots = [self.uncond_slot] + neg + [int(s) for s in target_slots]

    def run_pnp(self):
        """`run_pnp` + `sample_loop` (pnp.py:566-577) without the decode: the latents of the targets [B,4,h,w]."""
        B = (len(self.slots) - 1) // 2
        assert B >= 1, "PNP.load first"
        conv_on, attn_on, conv_mask, attn_mask = self.plan
        x = self.eps.expand(B, -1, -1, -1)
        return self.net.pnp_run(x, self.lat, self.timesteps, self.coef, conv_on, attn_on, conv_mask, attn_mask, self.slots, self.guidance_scale)


class Generator:
    """The reference's `Generator` (pnp.py:580-608) on a seed from `extract_latents` (one image): `generate` returns the translations as
    uint8 [B,H,W,3] (`export` + `pilify`: `(x * 255).astype(np.uint8)`)."""

    def __init__(self, net, seed: Tuple, uncond_slot: int, base_slot: int, pnp_attn_t: float = 0.5, pnp_f_t: float = 0.8, **kw):
        _, inverted, trajectory = seed
        self.net = net
        self.pnp = PNP(net, inverted, trajectory, uncond_slot, base_slot, pnp_attn_t=pnp_attn_t, pnp_f_t=pnp_f_t, **kw)

    def generate(self, target_slots: Sequence[int], empty: Optional[Sequence[bool]] = None):
        self.pnp.load(target_slots, empty)
        return self.net.vae_decode(self.pnp.run_pnp(), want="u8")
