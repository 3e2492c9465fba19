"""REFERENCE FOR THE TESTS of text-to-image sampling on the fp16 engine — test infrastructure only.  PARITY UNPINNED.

A torch CPU restatement of what `Trainer.sample` runs (`diffmining/finetuning/cars.py:235-255`; the same call in ftt / geo / places and
`xray/finetune.py:228`): `StableDiffusionPipeline(prompt, negative_prompt, latents, num_inference_steps=50, eta=0.0, guidance_scale=7.5)` on
a `DDIMScheduler` under `torch.autocast('cuda')`, with fp32 latents (`--mixed_precision no`, so `weight_dtype` is fp32) and an fp16
`noise_pred` out of the autocast U-Net.

diffusers is not available to the tests, so the pipeline itself cannot be executed: like `tests/pnp_ref.py` this restates diffusers 0.24
from its public semantics (`StableDiffusionPipeline.__call__`, `DDIMScheduler.step`, `AutoencoderKL.decode`, `VaeImageProcessor.postprocess`)
and is pinned structurally only.  The decoder is `pnp_ref.vae_decode_raw`'s sequence on `oracle/vae_ref.py`'s `_conv / _gn / _resnet /
_attention`, with the latent DIVIDED by the scaling factor (the pipeline divides; pnp.py multiplies by the reciprocal).

Type promotion.  The scheduler's `alphas_cumprod` stays on the CPU, so `alpha_prod_t` and its kin are 0-dim fp32 CPU tensors, and the products
`beta_prod_t ** 0.5 * model_output` meet an fp16 CUDA tensor: the result is fp16 (a 0-dim tensor does not promote a dimensioned one of the
same category), and the GPU kernel takes the 0-dim operand as an fp32 op-math scalar — fp32 product, one rounding to fp16.  torch's CPU
kernels do the same for `tensor * scalar` but round a LEADING 0-dim operand to fp16 first (`scalar * tensor`); since the reference runs on
the GPU, `_mul16` below writes the GPU's arithmetic out: widen, multiply in fp32, round.  A Python scalar (`guidance_scale`) enters the same way.

A second open point, for whoever pins this against real diffusers: the two divisions by a scalar — `latents / scaling_factor` and
`(sample - ...) / alpha_prod_t ** 0.5` — are kept here as true fp32 divisions, correctly rounded, and the kernels use `__fdiv_rn` to match.
torch's GPU true-divide by a CPU scalar (a Python number or a 0-dim CPU tensor) may instead multiply by the reciprocal formed in op-math
(`a * (1 / b)`), which can differ from the quotient by one fp32 ulp.  Not decided here: diffusers cannot be run by the tests.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_ref as R
from oracle import vae_ref as V

SCALING_FACTOR = 0.18215


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
def vae_decode_raw(sd, latent, autocast=True, scaling_factor=SCALING_FACTOR):
    """`vae.decode(latents / vae.config.scaling_factor).sample` (StableDiffusionPipeline.__call__): diffusers 0.24 `Decoder` of the SDv1.5
    vae/config.json.  autocast=True: conv / linear / attention take and emit fp16, GroupNorm, SiLU and softmax run in fp32."""
    p = R._SD(sd)
    ac = autocast
    z = latent.float() / scaling_factor
    h = V._conv(p, "post_quant_conv", z, ac, padding=0)
    h = V._conv(p, "decoder.conv_in", h, ac)
    h = V._resnet(p, "decoder.mid_block.resnets.0", h, ac)
    h = V._attention(p, "decoder.mid_block.attentions.0", h, ac)
    h = V._resnet(p, "decoder.mid_block.resnets.1", h, ac)
    for i in range(4):                                                       # UpDecoderBlock2D: three resnets, Upsample2D on all but the last
        for j in range(3):
            h = V._resnet(p, f"decoder.up_blocks.{i}.resnets.{j}", h, ac)
        if i != 3:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = V._conv(p, f"decoder.up_blocks.{i}.upsamplers.0.conv", h, ac)
    return V._conv(p, "decoder.conv_out", F.silu(V._gn(p, "decoder.conv_norm_out", h)), ac)


def postprocess_pil(raw16):
    """`VaeImageProcessor.postprocess(image, output_type="pil")` up to the PIL object: raw [B,3,H,W] fp16 -> uint8 [B,H,W,3].
    denormalize `(images / 2 + 0.5).clamp(0, 1)` in the sample's dtype (fp16: every op rounded), pt_to_numpy `.cpu().permute(0, 2, 3,
    1).float().numpy()`, numpy_to_pil `(images * 255).round().astype("uint8")` — ROUNDS (half to even); pnp.py's `pilify` truncates."""
    assert raw16.dtype == torch.float16
    img = (raw16 / 2 + 0.5).clamp(0, 1)
    x = img.cpu().permute(0, 2, 3, 1).float().numpy()
    return np.nan_to_num((x * 255).round(), nan=0.0).astype("uint8")


# ---- the scheduler ----------------------------------------------------------------------------------------------------------------------
def _mul16(scalar, t16):
    """scalar (a Python number or a 0-dim fp32 tensor) * fp16 tensor on the GPU: fp32 op-math, rounded to fp16 once"""
    assert t16.dtype == torch.float16
    s = torch.as_tensor(scalar, dtype=torch.float32)
    return (s * t16.float()).half()


def guided_noise(noise_pred16, guidance_scale):
    """`noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)` on the fp16 output of the autocast U-Net [2B,...]"""
    assert noise_pred16.dtype == torch.float16
    u, c = noise_pred16.chunk(2)
    return u + _mul16(guidance_scale, c - u)


def scheduler_step_autocast(model_output16, timestep, sample32, num_inference_steps, acp, eta=0.0):
    """`DDIMScheduler.step(noise_pred, t, latents).prev_sample` (diffusers 0.24; epsilon prediction, clip_sample = False, thresholding off)
    with an fp16 model_output and an fp32 sample, every tensor in the dtype torch's promotion gives it."""
    assert model_output16.dtype == torch.float16 and sample32.dtype == torch.float32 and eta == 0.0
    prev_timestep = timestep - 1000 // num_inference_steps
    alpha_prod_t = acp[timestep]
    alpha_prod_t_prev = acp[prev_timestep] if prev_timestep >= 0 else acp[0]          # final_alpha_cumprod: set_alpha_to_one = False
    beta_prod_t = 1 - alpha_prod_t
    pred_original_sample = (sample32 - _mul16(beta_prod_t ** 0.5, model_output16)) / alpha_prod_t ** 0.5          # fp32 - fp16 -> fp32
    pred_epsilon = model_output16
    beta_prod_t_prev = 1 - alpha_prod_t_prev
    variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
    std_dev_t = eta * variance ** 0.5
    pred_sample_direction = _mul16((1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5, pred_epsilon)                  # fp16
    prev_sample = alpha_prod_t_prev ** 0.5 * pred_original_sample + pred_sample_direction                        # fp32 + fp16 -> fp32
    assert pred_original_sample.dtype == torch.float32 and prev_sample.dtype == torch.float32
    return prev_sample


def scheduler_step_fp32(model_output, timestep, sample32, num_inference_steps, acp):
    """the same formula with everything widened to fp32 first: what the step is NOT"""
    return _step_fp32(model_output.float(), timestep, sample32, num_inference_steps, acp)


def _step_fp32(eps, timestep, x, n, acp):
    prev_timestep = timestep - 1000 // n
    a_t = acp[timestep]
    a_prev = acp[prev_timestep] if prev_timestep >= 0 else acp[0]
    x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    return a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * eps


def sample_loop(eps_fn, x, timesteps, acp, g):
    """The denoising loop of `StableDiffusionPipeline.__call__` (do_classifier_free_guidance): eps_fn(latent_model_input [2B] fp32, t) ->
    noise_pred [2B] fp16 (rows 0..B-1 under the negative prompt).  `scale_model_input` is the identity for DDIM and init_noise_sigma is 1."""
    timesteps = [int(t) for t in timesteps]
    x = x.float()
    for t in timesteps:
        latent_model_input = torch.cat([x] * 2)
        noise_pred = eps_fn(latent_model_input, t)
        assert noise_pred.dtype == torch.float16
        x = scheduler_step_autocast(guided_noise(noise_pred, g), t, x, len(timesteps), acp)
    return x


# ---- the host form of "row of the table + the restated update" -------------------------------------------------------------------------------
def table_update(x32, noise_pred16, row, g):
    """one guided step from a row (c0, c1, c2, c3) of `sample.sample_coefficients`, op by op as dm_op_cfg_ddim_step takes them"""
    c0, c1, c2, c3 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    e = guided_noise(noise_pred16, g)
    x0 = (x32 - _mul16(c1, e)) / c2
    return c0 * x0 + _mul16(c3, e)
