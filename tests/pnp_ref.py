"""REFERENCE FOR THE TESTS of the parallel-dataset generator — test infrastructure only.  PARITY UNPINNED.

A torch-fp32 CPU restatement of `diffmining/applications/parallel-dataset/pnp.py`: the VAE decoder and the post-processing
(`:137-142`, `:531-536`, `:590-591`), the DDIM inversion (`:156-180`) and reconstruction (`:182-203`), the Plug-and-Play step
(`:538-558`, with `DDIMScheduler.step` at eta = 0, clip_sample = False) and the two injected forwards (`:345-350`, `:424-432`).

diffusers and xformers are not available to the tests, so `pnp.py` itself cannot be executed: like `oracle/unet_ref.py` (see its header) this
restates the public SDv1.5 configs and diffusers-0.24 semantics and is pinned structurally only.  The decoder is built from
`oracle/vae_ref.py`'s `_conv / _gn / _resnet / _attention`.  The injected forward is `oracle/unet_ref.unet_forward` itself: it looks `_resnet`
and `_attention` up in its module at call time, so `install_injection` swaps restated versions of the two in with pytest's `monkeypatch` and
the reference's own `3B` batch layout (source repeated B times, then B unconditional and B conditional rows) is run unchanged.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_ref as R
from oracle import vae_ref as V


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------
def vae_decode_raw(sd, latent):
    """`vae.decode(1 / 0.18215 * latents).sample` (pnp.py:139-140): diffusers 0.24 `Decoder` of the SDv1.5 vae/config.json."""
    p = R._SD(sd)
    ac = False
    z = 1 / 0.18215 * latent.float()
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


def postprocess(raw):
    """pnp.py:141 / :535"""
    return (raw / 2 + 0.5).clamp(0, 1)


def pilify(img):
    """`export` + `pilify` (pnp.py:590-591, :601): [B,3,H,W] in [0,1] -> uint8 [B,H,W,3], truncating"""
    x = img.permute(0, 2, 3, 1).cpu().numpy()
    return (x * 255).astype(np.uint8)


# ---- the three loops; eps_fn(x, t) stands for `self.unet(x, t, encoder_hidden_states=cond).sample` ---------------------------------------------
def ddim_inversion(eps_fn, latent, scheduler_timesteps, acp):
    """pnp.py:156-180.  scheduler_timesteps: descending, as `scheduler.timesteps`.  Returns (latent, {t: latent after the step at t})."""
    timesteps = list(reversed([int(t) for t in scheduler_timesteps]))
    final_alpha_cumprod = acp[0]                                             # set_alpha_to_one = False in the SDv1.5 scheduler config
    latents_ = {}
    for i, t in enumerate(timesteps):
        alpha_prod_t = acp[t]
        alpha_prod_t_prev = acp[timesteps[i - 1]] if i > 0 else final_alpha_cumprod
        mu = alpha_prod_t ** 0.5
        mu_prev = alpha_prod_t_prev ** 0.5
        sigma = (1 - alpha_prod_t) ** 0.5
        sigma_prev = (1 - alpha_prod_t_prev) ** 0.5
        eps = eps_fn(latent, t)
        pred_x0 = (latent - sigma_prev * eps) / mu_prev
        latent = mu * pred_x0 + sigma * eps
        latents_[t] = latent.clone()
    return latent, latents_


def ddim_sample(eps_fn, x, scheduler_timesteps, acp):
    """pnp.py:182-203"""
    timesteps = [int(t) for t in scheduler_timesteps]
    for i, t in enumerate(timesteps):
        alpha_prod_t = acp[t]
        alpha_prod_t_prev = acp[timesteps[i + 1]] if i < len(timesteps) - 1 else acp[0]
        mu = alpha_prod_t ** 0.5
        sigma = (1 - alpha_prod_t) ** 0.5
        mu_prev = alpha_prod_t_prev ** 0.5
        sigma_prev = (1 - alpha_prod_t_prev) ** 0.5
        eps = eps_fn(x, t)
        pred_x0 = (x - sigma * eps) / mu
        x = mu_prev * pred_x0 + sigma_prev * eps
    return x


def scheduler_step(model_output, timestep, sample, num_inference_steps, acp, eta=0.0):
    """`DDIMScheduler.step(...).prev_sample` (diffusers 0.24; epsilon prediction, clip_sample = False, thresholding off)."""
    prev_timestep = timestep - 1000 // num_inference_steps
    alpha_prod_t = acp[timestep]
    alpha_prod_t_prev = acp[prev_timestep] if prev_timestep >= 0 else acp[0]
    beta_prod_t = 1 - alpha_prod_t
    pred_original_sample = (sample - beta_prod_t ** 0.5 * model_output) / alpha_prod_t ** 0.5
    pred_epsilon = model_output
    beta_prod_t_prev = 1 - alpha_prod_t_prev
    variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
    std_dev_t = eta * variance ** 0.5
    pred_sample_direction = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5 * pred_epsilon
    return alpha_prod_t_prev ** 0.5 * pred_original_sample + pred_sample_direction


def pnp_sample_loop(eps3_fn, x, lat, scheduler_timesteps, acp, guidance_scale):
    """pnp.py:538-577 without the decode.  eps3_fn(latent_model_input [3B], t) -> noise_pred [3B]; lat: {t: source latent [1,4,h,w]}."""
    timesteps = [int(t) for t in scheduler_timesteps]
    B = x.shape[0]
    for t in timesteps:
        latent_model_input = torch.cat([lat[t]] * B + [x] * 2)
        noise_pred = eps3_fn(latent_model_input, t)
        _, noise_pred_uncond, noise_pred_cond = noise_pred.chunk(3)
        noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_cond - noise_pred_uncond)
        x = scheduler_step(noise_pred, t, x, len(timesteps), acp)
    return x


# ---- the injected forward -----------------------------------------------------------------------------------------------------------------
def _layer_names(layers, leaf_up, leaf_mid):
    return {(leaf_mid if res == -1 else leaf_up).format(res=res, block=block) for res, block in layers}


def install_injection(monkeypatch, conv_layers=(), attn_layers=()):
    """Swap `_resnet` / `_attention` of oracle/unet_ref for versions that inject at the named (res, block) layers (res -1 = the mid block), as
    `register_conv_control_efficient` / `register_attention_control_efficient` do for a timestep inside the injection schedule.  The batch is
    the reference's: [source] * B + [uncond] * B + [cond] * B."""
    conv_names = _layer_names(conv_layers, "up_blocks.{res}.resnets.{block}", "mid_block.resnets.{block}")
    attn_names = _layer_names(attn_layers, "up_blocks.{res}.attentions.{block}.transformer_blocks.0.attn1",
                              "mid_block.attentions.{block}.transformer_blocks.0.attn1")
    _conv, _linear, _gn, _r = R._conv, R._linear, R._gn, R._r

    def resnet(p, name, x, temb_act, cfg, ac):
        h = F.silu(_gn(p, name + ".norm1", x, cfg.norm_num_groups, cfg.norm_eps))
        h = _conv(p, name + ".conv1", h, ac)
        t = _linear(p, name + ".time_emb_proj", temb_act, ac)
        h = _r(h + t[:, :, None, None], ac, "temb")
        h = F.silu(_gn(p, name + ".norm2", h, cfg.norm_num_groups, cfg.norm_eps))
        h = _conv(p, name + ".conv2", h, ac)
        if name in conv_names:                                               # pnp.py:345-350
            sb = int(h.shape[0] // 3)
            h = h.clone()
            h[sb:2 * sb] = h[:sb]
            h[2 * sb:] = h[:sb]
        if p.has(name + ".conv_shortcut.weight"):
            x = _conv(p, name + ".conv_shortcut", x, ac, padding=0)
        return _r(x + h, ac, "res")                                          # pnp.py:357, output_scale_factor 1

    def attention(p, name, x, ctx, heads, ac):
        B, T, C = x.shape
        kv = x if ctx is None else ctx
        q = _linear(p, name + ".to_q", x, ac, bias=False)
        k = _linear(p, name + ".to_k", kv, ac, bias=False)
        if ctx is None and name in attn_names:                               # pnp.py:424-432
            sb = int(q.shape[0] // 3)
            q, k = q.clone(), k.clone()
            q[sb:2 * sb] = q[:sb]
            k[sb:2 * sb] = k[:sb]
            q[2 * sb:] = q[:sb]
            k[2 * sb:] = k[:sb]
        v = _linear(p, name + ".to_v", kv, ac, bias=False)
        d = C // heads
        q = q.view(B, T, heads, d).transpose(1, 2)
        k = k.view(B, kv.shape[1], heads, d).transpose(1, 2)
        v = v.view(B, kv.shape[1], heads, d).transpose(1, 2)
        s = torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5)
        o = _r(torch.matmul(_r(torch.softmax(s, dim=-1), ac, "p"), v), ac, "o")
        o = o.transpose(1, 2).reshape(B, T, C)
        return _linear(p, name + ".to_out.0", o, ac)

    monkeypatch.setattr(R, "_resnet", resnet)
    monkeypatch.setattr(R, "_attention", attention)


def to_reference_rows(sample, B):
    """this project's batch [source, B uncond, B cond] -> the reference's [source] * B + [uncond] * B + [cond] * B (row B + i <-> row 1 + i)"""
    return torch.cat([sample[:1]] * B + [sample[1:]])


# ---- the host form of "table + four-scalar update" ----------------------------------------------------------------------------------------------
def table_update(x, eps, row):
    """x' = c0 * ((x - c1 * eps) / c2) + c3 * eps with a row of `pnp.ddim_coefficients`, op by op in fp32"""
    c0, c1, c2, c3 = (torch.tensor(float(v), dtype=torch.float32) for v in row)
    return c0 * ((x - c1 * eps) / c2) + c3 * eps
