#!/usr/bin/env python
"""Images/s of `compute_submission` vs `compute_worklist` on a synthetic CarDB-like work list, and the host cost per image of
decode and rescale (PIL's LANCZOS on the host vs the device resize's host share: tables + packing).

    python tools/worklist_rate.py [--images 64] [--N 10] [--images-per-call 8] [--seed 0]

The mixed list: `--images` landscape JPEGs with short side 256-480 whose cars-rule latents cover 32 x {40 ... 56}, categories
written round-robin and then shuffled (the reference's lists, compute.py:300-341).  The control list has as many images of one
size with the same total pixel count.  Synthetic weights, 4 categories + the null prompt.  Each list is
scored twice per entry; the second pass is reported (the first one meets every latent shape for the first time)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import PIL.Image  # noqa: E402
import torch  # noqa: E402

import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import resample as RS  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.typicality import TypicalityScorer  # noqa: E402

CATS = ["1950", "1970", "1990", "2010"]


def _photo(w, h, rng):
    """A smooth random image (JPEG-compressible like a photo, unlike uniform noise)."""
    small = rng.integers(0, 256, (max(2, h // 32), max(2, w // 32), 3), dtype=np.uint8)
    im = PIL.Image.fromarray(small).resize((w, h), PIL.Image.BILINEAR)
    a = np.asarray(im).astype(np.int16) + rng.integers(-12, 13, (h, w, 3), dtype=np.int16)
    return PIL.Image.fromarray(a.clip(0, 255).astype(np.uint8))


def make_lists(d, n, seed):
    rng = np.random.default_rng(seed)
    mixed = []
    for i in range(n):
        wl = 40 + i % 17                                             # latent width 40 ... 56 under the cars rule
        s = int(rng.integers(256, 481))
        long_ = int(np.ceil((wl * 8 + 4) * s / 256))
        w, h = long_, s
        tw, th = TypicalityScorer.rescale_size("cars", w, h)
        assert (th // 8, tw // 8) == (32, wl), (w, h, tw, th, wl)
        mixed.append((w, h))
    cats = [CATS[i % len(CATS)] for i in range(n)]
    order = rng.permutation(n)
    px = sum(w * h for w, h in mixed) / n
    s = 368
    cw = int(round(px / s))
    lines = {"mixed": [], "control": []}
    for k, i in enumerate(order):
        w, h = mixed[i]
        p = os.path.join(d, f"{cats[k]}__mixed_{k:03d}.jpg")
        _photo(w, h, rng).save(p, quality=90)
        lines["mixed"].append(f"{p},{cats[k]}")
        p = os.path.join(d, f"{cats[k]}__control_{k:03d}.jpg")
        _photo(cw, s, rng).save(p, quality=90)
        lines["control"].append(f"{p},{cats[k]}")
    return lines, (cw, s), px


def host_costs(lines):
    """ms per image: decode (PIL open + load), PIL LANCZOS to the cars size, and the device path's host share with a cold and a
    warm table cache (resize_plan + packing the pixels into one upload buffer)."""
    dec, pil, plan_cold, plan_warm = [], [], [], []
    RS.lanczos_axis.cache_clear()
    for line in lines:
        path = line.split(",")[0]
        t0 = time.perf_counter()
        with PIL.Image.open(path) as im:
            im.load()
            a = np.asarray(im)
            t1 = time.perf_counter()
            tw, th = TypicalityScorer.rescale_size("cars", im.width, im.height)
            im.resize((tw, th), PIL.Image.LANCZOS)
            t2 = time.perf_counter()
        RS.resize_plan([(a.shape[1], a.shape[0])], tw, th)
        np.concatenate([a.reshape(-1)])
        t3 = time.perf_counter()
        RS.resize_plan([(a.shape[1], a.shape[0])], tw, th)
        np.concatenate([a.reshape(-1)])
        t4 = time.perf_counter()
        dec.append(t1 - t0)
        pil.append(t2 - t1)
        plan_cold.append(t3 - t2)
        plan_warm.append(t4 - t3)
    ms = lambda v: round(1e3 * float(np.mean(v)), 2)     # noqa: E731
    return {"decode_ms": ms(dec), "pil_lanczos_ms": ms(pil), "device_resize_host_ms_cold_tables": ms(plan_cold),
            "device_resize_host_ms_warm_tables": ms(plan_warm)}


def rate(scorer, fn, lines, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(lines, **kw)
    torch.cuda.synchronize()
    return len(lines) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--images-per-call", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from diff_mining_amd.engine import UNetEngine
    eng = UNetEngine(0)
    eng.load_state_dict(synth.synth_state_dict(seed=0, dtype=np.float16))
    eng.load_vae_state_dict(synth.synth_vae_state_dict(seed=0, dtype=np.float16))
    g = torch.Generator().manual_seed(a.seed)
    embeds = {c: torch.randn(77, 768, generator=g).half() for c in CATS + [""]}
    res = {"images": a.images, "N": a.N, "images_per_call": a.images_per_call, "decode_threads": TypicalityScorer.decode_threads()}
    with tempfile.TemporaryDirectory() as d:
        lines, csize, px = make_lists(d, a.images, a.seed)
        res["control_size"], res["mean_pixels"] = list(csize), round(px)
        sc = TypicalityScorer(eng, seed=42, N=a.N, t_min=0.1, t_max=0.7, typicality_path=os.path.join(d, "out"), which="cars",
                              country_embeds=embeds)
        for lst in ("mixed", "control"):
            for entry in ("compute_submission", "compute_worklist"):
                fn = getattr(sc, entry)
                rate(sc, fn, lines[lst], images_per_call=a.images_per_call)               # warm-up: every shape once
                res[f"{entry}_{lst}_images_per_s"] = round(rate(sc, fn, lines[lst], images_per_call=a.images_per_call), 2)
            sc.compute_worklist(lines[lst], images_per_call=a.images_per_call)
            sizes = [len(c) for c in sc.last_worklist_calls]
            res[f"worklist_{lst}_calls"] = len(sizes)
            res[f"worklist_{lst}_mean_images_per_call"] = round(float(np.mean(sizes)), 2)
        res["worklist_mixed_vs_control"] = round(res["compute_worklist_mixed_images_per_s"] / res["compute_worklist_control_images_per_s"], 3)
        res.update({f"mixed_{k}": v for k, v in host_costs(lines["mixed"]).items()})
    for k, v in res.items():
        print(f"{k:48s} {v}")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
