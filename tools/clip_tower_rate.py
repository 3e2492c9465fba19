#!/usr/bin/env python
"""Images/s of the CLIP baseline from pixels on the fp32 net: the ViT-L/14-336 image tower (UNetEngineF32.clip_image_tokens) alone and
with the mining behind it (clipmine.rank_images), at the reference's shapes — 512 x 512 center crops, 577 tokens, k_per_image = 5
boxes of 64 x 64 (clipmining/ranking.py:58-125).

    python tools/clip_tower_rate.py [--images 64] [--repeat 3] [--size 512] [--out profiles/clip_tower_rate.txt]

Synthetic weights (304 M parameters, about 12 s to generate) and images.  `tower` = host plan + upload of the uint8 images + fused
preprocess + tower; `device only` = clip_patch_tokens on preprocessed pixel values; `tower + mining` = rank_images (text embeddings
once, tower, dm_clipmine_rank, the rows back on the host).  One more device-only pass runs with the net's event profile on and
prints gemm32's and the attention's time, FLOP and share of the 157 TFLOP/s fp32 MFMA peak — the only related figure measured before
is the DIFT-fp32 path's 0.83 of peak on gemm32, printed beside it.  Prints a table and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import clipmine, synth  # noqa: E402
from diff_mining_amd.clip_spec import CLIP_L14_336_VISION as CFG  # noqa: E402
from diff_mining_amd.engine import UNetEngineF32  # noqa: E402

PEAK_F32_MFMA = 157.0e12           # MI355X fp32 matrix peak, FLOP/s
DIFT_F32_GEMM_FRACTION = 0.83      # gemm32's share of that peak on the DIFT-fp32 path, for comparison

G2 = (CFG.image_size // CFG.patch_size) ** 2
T = G2 + 1
H, F, L = CFG.hidden_size, CFG.intermediate_size, CFG.num_hidden_layers
# per image (2 FLOP per multiply-add): layers x (q|k|v + out_proj + fc1 + fc2) over T tokens, the patch embedding over the real 588
# columns, visual_projection over the patch tokens, attention (QK^T + PV) per head
FLOP_LAYERS = L * 2.0 * T * H * (3 * H + H + F + F)
FLOP_PATCH = 2.0 * G2 * 3 * CFG.patch_size ** 2 * H
FLOP_PROJ = 2.0 * G2 * H * CFG.projection_dim
FLOP_ATTN = L * CFG.num_attention_heads * 2 * 2.0 * T * T * 64
FLOP_PER_IMAGE = FLOP_LAYERS + FLOP_PATCH + FLOP_PROJ + FLOP_ATTN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    net = UNetEngineF32(0)
    t0 = time.perf_counter()
    net.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, CFG), CFG)
    sd = {"text_model." + k: v for k, v in synth.synth_clip_state_dict(seed=0).items()}
    sd["text_projection.weight"] = synth.synth_clip_text_projection(0)
    net.load_clip_state_dict(sd)
    del sd
    t_load = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    S = a.size
    imgs = []
    for i in range(a.images):
        small = rng.integers(0, 256, (S // 32, S // 32, 3), dtype=np.uint8)
        big = np.repeat(np.repeat(small, 32, 0), 32, 1).astype(np.int16) + rng.integers(-12, 13, (S, S, 3), dtype=np.int16)
        imgs.append(big.clip(0, 255).astype(np.uint8))
    ids = synth.synth_token_ids(2)

    def timed(fn):
        fn()                                             # warm-up: arena sizing, table caches
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.repeat):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.repeat, out

    t_tower, tok = timed(lambda: net.clip_image_tokens(imgs))
    assert tok.shape == (a.images, G2, CFG.projection_dim) and torch.isfinite(tok).all()
    pv = net.clip_tower_preprocess(imgs)
    t_dev, tok2 = timed(lambda: net.clip_patch_tokens(pv))
    assert torch.equal(tok, tok2)
    t_rank, (rows, feats) = timed(lambda: clipmine.rank_images(net, imgs, ids, k_per_image=5, kx=64, ky=64))
    t_text, _ = timed(lambda: net.clip_text_embeds(ids))

    net.prof_enable(True)
    net.clip_patch_tokens(pv)
    torch.cuda.synchronize()
    prof = net.prof_read()
    net.prof_enable(False)
    gemm_tf = prof["igemm_flops"] / (prof["igemm_ms"] * 1e-3) / 1e12
    attn_tf = prof["attn_flops"] / (prof["attn_ms"] * 1e-3) / 1e12
    mem = net.memory()

    n = a.images
    res = {
        "images": n, "image_size": S, "gflop_per_image": round(FLOP_PER_IMAGE / 1e9, 2), "load_s": round(t_load, 1),
        "tower_images_per_s": round(n / t_tower, 2), "tower_tflops": round(n / t_tower * FLOP_PER_IMAGE / 1e12, 2),
        "device_only_images_per_s": round(n / t_dev, 2), "device_only_tflops": round(n / t_dev * FLOP_PER_IMAGE / 1e12, 2),
        "tower_plus_mining_images_per_s": round(n / t_rank, 2), "text_embeds_ms": round(t_text * 1e3, 2), "rows_mined": int(len(rows["D"])),
        "gemm32_ms": round(prof["igemm_ms"], 2), "gemm32_tflops": round(gemm_tf, 2), "gemm32_fraction_of_peak": round(gemm_tf * 1e12 / PEAK_F32_MFMA, 3),
        "gemm32_launches": prof["igemm_launches"], "attention_ms": round(prof["attn_ms"], 2), "attention_tflops": round(attn_tf, 2),
        "attention_time_share": round(prof["attn_ms"] / (prof["attn_ms"] + prof["igemm_ms"]), 3),
        "attention_flop_share": round(FLOP_ATTN / FLOP_PER_IMAGE, 3), "dift_f32_gemm32_fraction_of_peak": DIFT_F32_GEMM_FRACTION,
        "arena_mb": round(mem["arena_bytes"] / 2 ** 20, 1), "weights_mb": round(mem["weights_bytes"] / 2 ** 20, 1),
        "device": torch.cuda.get_device_name(0),
    }
    lines = [
        f"CLIP ViT-L/14-336 image tower, fp32 ({res['device']}), {n} images of {S}x{S}, {FLOP_PER_IMAGE / 1e9:.1f} GFLOP per image, "
        f"synthetic weights ({res['weights_mb']} MB with the text tower), arena {res['arena_mb']} MB",
        f"  tower (plan + upload + preprocess + tower): {n / t_tower:8.2f} images/s  {res['tower_tflops']:7.2f} TFLOP/s  ({t_tower * 1e3:.1f} ms per call)",
        f"  device only (pixel_values -> tokens):       {n / t_dev:8.2f} images/s  {res['device_only_tflops']:7.2f} TFLOP/s",
        f"  tower + mining (rank_images, 5 x 64x64):    {n / t_rank:8.2f} images/s  ({res['rows_mined']} rows; text embeddings {res['text_embeds_ms']} ms per call)",
        f"  gemm32:    {res['gemm32_ms']:8.2f} ms in {res['gemm32_launches']} launches, {gemm_tf:6.2f} TFLOP/s = {res['gemm32_fraction_of_peak']:.3f} of the "
        f"157 TFLOP/s fp32 MFMA peak (DIFT-fp32 path: {DIFT_F32_GEMM_FRACTION})",
        f"  attention: {res['attention_ms']:8.2f} ms, {attn_tf:6.2f} TFLOP/s; {res['attention_time_share']:.3f} of the timed GEMM + attention time "
        f"for {res['attention_flop_share']:.3f} of the FLOP",
        json.dumps(res),
    ]
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    net.close()


if __name__ == "__main__":
    main()
