#!/usr/bin/env python
"""Patches/s and TFLOP/s of the fp32 CLIP ViT-B/32 image tower (UNetEngineF32.clip_patch_features) at the clustering stage's
defaults: k_per_image = 5 boxes of 64 x 64 on each of k = 1000 images per category (P = 5000), in calls of 500 patches
(100 images), against the reference's schedule of one patch per call (`Cluster.embed`, cluster.py:224-231) on the same engine.

    python tools/clip_image_rate.py [--images 1000] [--per-image 5] [--call 500] [--single 200] [--size 512] [--out FILE]

Synthetic weights and images (uint8, `--size` square, 100 distinct images cycled).  Each call includes the host plan, the upload
of its uint8 images, the fused preprocess and the tower; `device only` times clip_image_features on preprocessed pixel values.
Prints a table and one JSON line."""
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
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.engine import UNetEngineF32  # noqa: E402

# per patch: 12 layers x (q|k|v 2304 + out_proj 768 + fc1 3072 + fc2 3072 x 768) x 50 tokens, patch embedding 49 x 3072 x 768,
# attention 12 x 12 heads x (QK^T + PV) over 50 x 50 x 64, visual_projection 768 x 512 (2 FLOP per multiply-add)
FLOP_LAYERS = 12 * 2.0 * 50 * 768 * (2304 + 768 + 3072 + 3072)
FLOP_PATCH = 2.0 * 49 * 3072 * 768
FLOP_ATTN = 12 * 12 * 2 * 2.0 * 50 * 50 * 64
FLOP_PROJ = 2.0 * 768 * 512
FLOP_PER_PATCH = FLOP_LAYERS + FLOP_PATCH + FLOP_ATTN + FLOP_PROJ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--per-image", type=int, default=5)
    ap.add_argument("--call", type=int, default=500, help="patches per call")
    ap.add_argument("--single", type=int, default=200, help="patches timed one per call")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.call % a.per_image == 0
    torch.cuda.init()
    net = UNetEngineF32(0)
    net.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
    rng = np.random.default_rng(0)
    S = a.size
    pool = []
    for i in range(100):
        small = rng.integers(0, 256, (S // 32, S // 32, 3), dtype=np.uint8)
        big = np.repeat(np.repeat(small, 32, 0), 32, 1).astype(np.int16) + rng.integers(-12, 13, (S, S, 3), dtype=np.int16)
        pool.append(big.clip(0, 255).astype(np.uint8))
    imgs = [pool[i % 100] for i in range(a.images)]
    boxes = [[tuple(int(v) for v in (r, c, r + 64, c + 64)) for r, c in rng.integers(0, S - 64, (a.per_image, 2))] for _ in range(a.images)]
    P = a.images * a.per_image
    ipc = a.call // a.per_image

    def run_all():
        outs = []
        for i0 in range(0, a.images, ipc):
            outs.append(net.clip_patch_features(imgs[i0:i0 + ipc], boxes[i0:i0 + ipc]))
        return outs
    run_all()                                            # warm-up: arena sizing, tables cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = run_all()
    torch.cuda.synchronize()
    t_batched = time.perf_counter() - t0
    feats = torch.cat(outs)
    assert feats.shape == (P, 512) and torch.isfinite(feats).all()

    # device only: the tower on preprocessed pixel values, calls of `call`
    pv = net.clip_preprocess(imgs[:ipc], boxes[:ipc])
    net.clip_image_features(pv)
    torch.cuda.synchronize()
    n_dev = max(1, P // a.call)
    t0 = time.perf_counter()
    for _ in range(n_dev):
        net.clip_image_features(pv)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / (n_dev * pv.shape[0])

    # the reference's schedule: one patch per call
    singles = [(imgs[i // a.per_image], boxes[i // a.per_image][i % a.per_image]) for i in range(a.single)]
    for im, b in singles[:5]:
        net.clip_patch_features([im], [[b]])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for im, b in singles:
        net.clip_patch_features([im], [[b]])
    torch.cuda.synchronize()
    t_single = (time.perf_counter() - t0) / a.single

    rate_b, rate_s, rate_d = P / t_batched, 1.0 / t_single, 1.0 / t_dev
    res = {
        "patches": P, "patches_per_call": a.call, "image_size": S,
        "batched_patches_per_s": round(rate_b, 1), "batched_tflops": round(rate_b * FLOP_PER_PATCH / 1e12, 2),
        "device_only_patches_per_s": round(rate_d, 1), "device_only_tflops": round(rate_d * FLOP_PER_PATCH / 1e12, 2),
        "one_per_call_patches_per_s": round(rate_s, 1), "one_per_call_tflops": round(rate_s * FLOP_PER_PATCH / 1e12, 3),
        "speedup_vs_one_per_call": round(rate_b / rate_s, 1), "gflop_per_patch": round(FLOP_PER_PATCH / 1e9, 4),
        "device": torch.cuda.get_device_name(0),
    }
    lines = [
        f"CLIP ViT-B/32 image tower, fp32 ({res['device']}), {P} patches of 64x64 from {a.images} images of {S}x{S}, "
        f"{FLOP_PER_PATCH / 1e9:.3f} GFLOP per patch",
        f"  calls of {a.call} (plan + upload + preprocess + tower): {rate_b:9.1f} patches/s  {res['batched_tflops']:7.2f} TFLOP/s"
        f"  ({t_batched:.3f} s total)",
        f"  device only, calls of {pv.shape[0]} pixel_values:       {rate_d:9.1f} patches/s  {res['device_only_tflops']:7.2f} TFLOP/s",
        f"  one patch per call ({a.single} calls):                {rate_s:9.1f} patches/s  {res['one_per_call_tflops']:7.3f} TFLOP/s",
        f"  batched / one-per-call: {res['speedup_vs_one_per_call']}x",
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
