#!/usr/bin/env python
"""Rate of the HOG-LAB features on one MI355X at the reference's batch: 64 images of 512 x 512 pixels already on the device ->
fp16 [64, 57, 57, 2112] (doersch/hog.py:24-87).

  features  `doersch.hoglab_features` (dm_hoglab_features: the cell kernel and the block kernel), normalised fp16 output only, one call
  cells     `doersch.hoglab_cells` (dm_hoglab_cells: the cell kernel alone)
  copy      a device-to-device `copy_` of the same fp16 output: the store stream the block kernel is judged against

Timed with device events around single calls, after a warm-up, in alternating order (features, copy, copy, features, ...); medians
of --reps.  The output (878 MB) exceeds every cache.  Reported: ms per batch, microseconds per image, output bytes per second, and
the block kernel's share (features - cells) as a store stream against the copy's write rate.  Prints a table and one JSON line;
--out writes both to a file.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import doersch as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    n, side = a.images, a.side
    g = torch.Generator(device="cuda").manual_seed(7)
    images = torch.randint(0, 256, (n, side, side, 3), generator=g, device="cuda", dtype=torch.uint8)
    work = torch.empty(D.hoglab_workspace_bytes(n, side, side), dtype=torch.uint8, device="cuda")
    kept = {}

    def features():
        kept["out"] = D.hoglab_features(images, normalized=True, raw=False, work=work)[0]

    def cells():
        kept["cells"] = D.hoglab_cells(images)

    for _ in range(3):
        features()
        cells()
    torch.cuda.synchronize()
    src = kept["out"].clone()
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    def timed(fn):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        fn()
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1])

    for _ in range(3):
        copy()
    torch.cuda.synchronize()
    ms = {"features": [], "cells": [], "copy": []}
    for rep in range(a.reps):
        for name in (("features", "copy") if rep % 2 == 0 else ("copy", "features")):
            ms[name].append(timed(features if name == "features" else copy))
        ms["cells"].append(timed(cells))
    med = statistics.median
    out_bytes = src.numel() * 2
    res = {"workload": f"{n} images of {side}x{side} -> fp16 {list(src.shape)}", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "output_bytes": out_bytes, "input_bytes": images.numel()}
    for name in ("features", "cells", "copy"):
        m = med(ms[name])
        res[name] = {"ms_median": round(m, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "us_per_image": round(m / n * 1e3, 2)}
    for name in ("features", "copy"):
        res[name]["output_tb_per_s"] = round(out_bytes / (res[name]["ms_median"] * 1e-3) / 1e12, 3)
    block_ms = res["features"]["ms_median"] - res["cells"]["ms_median"]
    res["block_kernel_ms"] = round(block_ms, 4)
    res["block_kernel_output_tb_per_s"] = round(out_bytes / (block_ms * 1e-3) / 1e12, 3)
    res["block_over_copy_write_rate"] = round(res["block_kernel_output_tb_per_s"] / res["copy"]["output_tb_per_s"], 3)
    lines = [f"hoglab rate: {res['workload']}; device: {res['device']}; medians of {a.reps}, alternating order"]
    for name in ("features", "cells", "copy"):
        r = res[name]
        tail = f", output at {r['output_tb_per_s']:.2f} TB/s" if "output_tb_per_s" in r else ""
        lines.append(f"  {name:8s}: {r['ms_median']:.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}) = {r['us_per_image']:.2f} us per image{tail}")
    lines.append(f"  block kernel = features - cells: {block_ms:.3f} ms, its stores at {res['block_kernel_output_tb_per_s']:.2f} TB/s = "
                 f"{res['block_over_copy_write_rate']:.2f} x the copy's write rate (the copy also reads as much as it writes)")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
