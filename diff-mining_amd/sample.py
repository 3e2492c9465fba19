"""Text-to-image sampling on the fp16 engine: what `Trainer.sample` of the reference does at every logging step and at both ends of a run
(`diffmining/finetuning/cars.py:235-255`, the same call in `ftt`, `geo`, `places` and `xray/finetune.py:228`),

    StableDiffusionPipeline(prompt, negative_prompt, latents, num_inference_steps=50, eta=0.0, guidance_scale=7.5)

on a `DDIMScheduler` under `torch.autocast('cuda')`, with fp32 latents (`--mixed_precision no`, the reference's default): token ids ->
`clip_encode` -> `set_prompts` -> the guided loop on the device queue (`dm_sample_run`) -> `vae_decode` -> uint8 images, with nothing leaving
the GPU in between.  Prompt templates and tokenisation stay with the caller, as in `clipmine.rank_images`.

Scheduler arithmetic.  `DDIMScheduler.step` (eta = 0, clip_sample = False, epsilon prediction) with an fp16 `noise_pred` and fp32 latents is

    e  = u + g * (c - u)                                   fp16 tensors: every op rounded to fp16 (g enters at fp32 precision)
    x' = c0 * ((x - c1 * e) / c2) + c3 * e                 c1 * e and c3 * e are fp16 (a 0-dim fp32 tensor does not promote a
                                                           dimensioned fp16 tensor); the subtraction, division, product and sum are fp32

with (c0, c1, c2, c3) = (sqrt(a_prev), sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev)).  The four scalars are formed here as the scheduler forms
them, on 0-dim fp32 CPU tensors, so the device computes no square root and the table is torch's, bit for bit.

Not covered: the `ddim=False` arm of `Trainer.sample` (the trainer's DDPM scheduler), fp16 latents (`--mixed_precision fp16`), the fp32 net
(its loops are `pnp.py`'s arithmetic: `diff_mining_amd.pnp`).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import pnp
from .engine import EngineError

NUM_TRAIN_TIMESTEPS = pnp.NUM_TRAIN_TIMESTEPS


def sample_timesteps(n: int = 50) -> np.ndarray:
    """`DDIMScheduler.set_timesteps(n).timesteps` of the SDv1.5 scheduler config (leading spacing, steps_offset 1): 50 -> 981, 961 .. 1."""
    return pnp.ddim_timesteps(n, steps_offset=1)


def sample_coefficients(timesteps: Sequence[int]) -> np.ndarray:
    """The [n][4] fp32 table (sqrt(a_prev), sqrt(1 - a_t), sqrt(a_t), sqrt(1 - a_prev)) of `DDIMScheduler.step` for the steps in loop order,
    built as the scheduler builds its scalars: prev_timestep = t - 1000 // n, `final_alpha_cumprod` = acp[0] below 0 (set_alpha_to_one =
    False), eta = 0 (std_dev_t = 0 * variance ** 0.5 is subtracted as its square, which changes nothing)."""
    import torch
    acp = pnp.alphas_cumprod()
    final = acp[0]
    ts = [int(t) for t in timesteps]
    n = len(ts)
    if n < 1:
        raise ValueError("no timesteps")
    rows = []
    for t in ts:
        if not 0 <= t < NUM_TRAIN_TIMESTEPS:
            raise ValueError(f"timestep {t}")
        prev = t - NUM_TRAIN_TIMESTEPS // n
        alpha_prod_t = acp[t]
        alpha_prod_t_prev = acp[prev] if prev >= 0 else final
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
        std_dev_t = 0.0 * variance ** 0.5
        rows.append(torch.stack([alpha_prod_t_prev ** 0.5, beta_prod_t ** 0.5, alpha_prod_t ** 0.5,
                                 (1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5]))
    return torch.stack(rows).to(torch.float32).numpy()


def _check_slots(engine, slots, n: int, what: str):
    s = np.asarray([int(v) for v in slots], dtype=np.int64).reshape(-1)
    if s.shape[0] != n:
        raise ValueError(f"{what}: {s.shape[0]} slots for {n} samples")
    if s.size and (int(s.min()) < 0 or int(s.max()) >= engine.n_prompts):
        bad = int(s.min()) if int(s.min()) < 0 else int(s.max())
        raise EngineError(f"{what}: prompt slot {bad} outside the {engine.n_prompts} prompts registered by set_prompts")
    return s


def sample_latents(engine, latents, cond_slots, uncond_slots, steps: int = 50, guidance_scale: float = 7.5):
    """The denoising loop of `StableDiffusionPipeline.__call__` on a DDIMScheduler: latents [B,4,h,w] (taken as fp32; `init_noise_sigma` is
    1) -> the final latents, fp32, on the device.  cond_slots / uncond_slots [B]: the registered prompt (`set_prompts`) of each sample and
    of its negative prompt; range-checked here, on the host."""
    B = int(latents.shape[0])
    if steps < 1:
        raise EngineError(f"sample_latents: steps {steps}")
    cond = _check_slots(engine, cond_slots, B, "sample_latents")
    uncond = _check_slots(engine, uncond_slots, B, "sample_latents")
    ts = sample_timesteps(steps)
    slots = np.concatenate([uncond, cond]).astype(np.int32)          # the pipeline's torch.cat([negative_prompt_embeds, prompt_embeds])
    return engine.sample_run(latents, ts, sample_coefficients(ts), slots.tolist(), guidance_scale)


def sample(engine, prompt_ids, negative_ids, latents=None, seed: Optional[int] = None, size: int = 512, steps: int = 50,
           guidance_scale: float = 7.5, want: str = "u8"):
    """`Trainer.sample` (cars.py:235-255) for B prompts: prompt_ids / negative_ids [B,77] (or [1,77], broadcast) token ids (tokenizer output,
    padding="max_length") -> uint8 images [B,size,size,3] on the device (want "f16": the decoder's raw sample [B,3,size,size]).

    latents [B,4,size/8,size/8]: the initial noise.  None draws it with torch's generator on the engine's device (`seed`, or the global
    generator) — NOT the stream of the reference's `randn_tensor` (a CPU generator per call there): pass `latents` for reproducibility
    against it.  Needs the CLIP text tower and the VAE decoder (`load_pipeline_dir(..., vae_decoder=True)`)."""
    torch = engine._torch
    if size < 8 or size % 8:
        raise EngineError(f"sample: size {size} must be a positive multiple of 8")
    ids = torch.as_tensor(prompt_ids).reshape(-1, 77)
    neg = torch.as_tensor(negative_ids).reshape(-1, 77)
    B = max(int(ids.shape[0]), int(neg.shape[0])) if latents is None else int(latents.shape[0])
    for name, t in (("prompt_ids", ids), ("negative_ids", neg)):
        if t.shape[0] not in (1, B):
            raise ValueError(f"sample: {name} has {t.shape[0]} rows for {B} samples")
    h = size // 8
    if latents is None:
        gen = None
        if seed is not None:
            gen = torch.Generator(device=engine.device)
            gen.manual_seed(int(seed))
        latents = torch.randn(B, 4, h, h, dtype=torch.float32, device=engine.device, generator=gen)
    elif tuple(latents.shape) != (B, 4, h, h):
        raise ValueError(f"sample: latents {tuple(latents.shape)} for size {size} (expected {(B, 4, h, h)})")
    # the distinct prompts once each: negative rows first, as the pipeline stacks them
    ctx = engine.clip_encode(torch.cat([neg, ids]), out_dtype=torch.float16)
    engine.set_prompts(ctx)
    n_neg = int(neg.shape[0])
    uncond = [i if n_neg == B else 0 for i in range(B)]
    cond = [n_neg + (i if ids.shape[0] == B else 0) for i in range(B)]
    x = sample_latents(engine, latents, cond, uncond, steps, guidance_scale)
    return engine.vae_decode(x, want=want)
