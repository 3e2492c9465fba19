#!/usr/bin/env python3
"""One `name sha256` line per result of every entry point of the fp32 net (UNetEngineF32), on synthetic weights and inputs with fixed
seeds.  Run it on two trees on the same GPU and `diff` the outputs: a change of the net's host runtime that must not change a bit of
any result shows equal lines.

    python tools/f32_digest.py [--no-seam] > digest.txt

The shapes are the smallest that cross every branch of the host runtime: two latent sizes (one that is no multiple of 8), both DIFT
taps, the injected forward and both sampling loops, both VAE halves, the text tower's two outputs, ViT-B/32 from pixels and from crops,
and the configurable image tower at a config whose patch rows are padded (588 -> 608), also with one image more than a run holds.
--no-seam leaves out the one large case: DIFT with one sample more than a run holds at 8 x 8 (4097).  The last line is dm_f32_memory.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diff_mining_amd import clip_spec as S  # noqa: E402
from diff_mining_amd import pnp as P  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.engine import CLIP_TOWER_CHUNK, UNetEngineF32  # noqa: E402

# the smallest tower the config check admits: a 2 x 2 grid, one head of 64, patch rows of 3 * 14 * 14 = 588 values padded to 608
TOWER = S.CLIPVisionConfig(hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, image_size=28, patch_size=14,
                           projection_dim=8)


def emit(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy()
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    print(name, h.hexdigest(), flush=True)


def unet(e, seam):
    e.load_state_dict(synth.synth_state_dict(seed=0, dtype=np.float32))
    for h, w in ((8, 8), (12, 10)):
        x, eps, t, c = (torch.from_numpy(a) for a in synth.synth_inputs(3, 3, h, w, n_prompts=3, latent_dtype=np.float32))
        e.set_prompts(c.float())
        slots = [0, 1, 2]
        emit(f"unet_forward {h}x{w}", e.unet(x, t, slots))
        emit(f"score {h}x{w}", e.score(x, eps, t, slots))
        emit(f"score_x_index {h}x{w}", e.score(x[:2], eps, t, slots, x_index=[1, 0, 1]))
        for k in (1, 3):
            emit(f"dift up{k} {h}x{w}", *e.dift(x, t, slots, up_ft_index=k, ensemble=3))
    x, eps, t, c = (torch.from_numpy(a) for a in synth.synth_inputs(3, 3, 8, 8, n_prompts=3, latent_dtype=np.float32))
    e.set_prompts(c.float())
    emit("forward_inject 8x8", e.unet_inject(x, t, [0, 1, 2], conv_mask=1 << 4, attn_mask=1 << 5))
    ts = P.ddim_timesteps(2)
    inv_ts = ts[::-1].copy()
    inv, traj = e.ddim_run(x[:2], inv_ts, P.ddim_coefficients(inv_ts, "invert"), [1, 2], save_rows=[0, 1], n_rows=2)
    emit("ddim_run 8x8", inv, traj)
    emit("pnp_run 8x8", e.pnp_run(x[1:3], traj[:, 0], ts, P.ddim_coefficients(ts, "step"), [1, 0], [1, 1], 1 << 4, 1 << 5, [0, 0, 0, 1, 2]))
    if seam:
        n = 64 * 4096 // 64 + 1                   # one sample more than a run holds at 8 x 8
        xs, _, tt, _ = (torch.from_numpy(a) for a in synth.synth_inputs(n, n, 8, 8, n_prompts=3, latent_dtype=np.float32))
        feat, _ = e.dift(xs, tt, torch.arange(n) % 3, up_ft_index=1)
        emit(f"dift up1 8x8 batch {n}", feat)


def vae(e):
    e.load_vae_state_dict(synth.synth_vae_state_dict(seed=0))
    e.load_vae_decoder_state_dict(synth.synth_vae_decoder_state_dict(seed=0))
    img = torch.from_numpy(synth.synth_image(1, 32, 24)).float()
    noise = torch.from_numpy(synth.hash_normal("input.vae_noise", 2 * 4 * 4 * 3, 11).reshape(2, 4, 4, 3).astype(np.float32))
    emit("vae_encode draws", *e.vae_encode(img, noise, return_moments=True, draws_per_image=2))
    emit("vae_encode mode", e.vae_encode(img, None))
    lat = torch.from_numpy(synth.hash_normal("input.vae_latent", 4 * 4 * 3, 12).reshape(1, 4, 4, 3).astype(np.float32))
    emit("vae_decode raw", e.vae_decode(lat, raw=True, want="f32"))
    emit("vae_decode u8", *e.vae_decode(lat, want="both"))


def clip(e):
    sd = {"text_model." + k: v for k, v in synth.synth_clip_state_dict(seed=0).items()}
    sd["text_projection.weight"] = synth.synth_clip_text_projection(0)
    e.load_clip_state_dict(sd)
    ids = synth.synth_token_ids(2)
    emit("clip_encode", e.clip_encode(ids))
    for norm in (False, True):
        emit(f"clip_text_embeds normalize={int(norm)}", e.clip_text_embeds(ids, normalize=norm))

    e.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
    pv = torch.from_numpy(synth.synth_clip_pixel_values(3))
    for norm in (False, True):
        emit(f"clip_image_features normalize={int(norm)}", e.clip_image_features(pv, normalize=norm))
    emit("clip_vision_hidden", e.clip_vision_hidden(pv))
    rng = np.random.default_rng(21)
    crops = [rng.integers(0, 256, (70, 90, 3), dtype=np.uint8), rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)]
    boxes = [[(3, 5, 43, 61), None], [(0, 0, 33, 32)]]
    emit("clip_preprocess", e.clip_preprocess(crops, boxes))
    emit("clip_patch_features", e.clip_patch_features(crops, boxes, normalize=True))

    e.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, TOWER), TOWER)
    for n in (3, CLIP_TOWER_CHUNK + 1):
        pt = torch.from_numpy(synth.synth_clip_pixel_values(n, seed=1, size=TOWER.image_size))
        emit(f"clip_patch_tokens n={n}", *e.clip_patch_tokens(pt, return_hidden=True))
        squares = [rng.integers(0, 256, (40 + i % 5, 40 + i % 5, 3), dtype=np.uint8) for i in range(n)]
        emit(f"clip_tower_preprocess n={n}", e.clip_tower_preprocess(squares))
        emit(f"clip_image_tokens n={n}", e.clip_image_tokens(squares))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--no-seam", action="store_true", help="skip the 4097-sample DIFT call")
    a = ap.parse_args()
    e = UNetEngineF32(0)
    unet(e, not a.no_seam)
    vae(e)
    clip(e)
    torch.cuda.synchronize()
    m = e.memory()
    print("memory", m["weights_bytes"], m["arena_bytes"], flush=True)
    e.close()


if __name__ == "__main__":
    main()
