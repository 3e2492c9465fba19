#!/usr/bin/env python
"""Rate of the patch-mining stage, grids -> boxes: 64 images of 512 x 683 (64 x 85 latents, N draws x 2 prompts, fp16 grids on the
device), 64 x 64 windows, k_per_image 5.

  batched   UNetEngine.typicality_image_batched + mine_patches, one call for all images; device events around the pair,
            warm-up, median of --reps repetitions (>= 20)
  (b)       what a user had before: the per-image `typicality_image` loop, every pooled map copied to the host, a numpy greedy
            selection there (host clock around work that ends with the last copy)
  (a)       the reference's own pandas path (`df_D.compute`'s frame + `sort` + `get_non_overlapping`, single process) on this
            machine's CPU, from the same pooled maps — only with --reference DIR (a checkout of the reference; its three
            functions are compiled from its text with `ast`, nothing is copied), else reported as not measured.  A machine
            that has the checkout but no GPU can time it on the maps a GPU run stored: --save-maps FILE there, then
            --reference DIR --reference-maps FILE here (appends its line to --out)

    python tools/mining_rate.py [--images 64] [--reps 20] [--draws 10] [--reference DIR] [--out profiles/mining_rate.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def greedy_host(dm, kx, ky, k_per_image):
    """numpy greedy a user would write on the host: argmax, suppress the inclusive zone, repeat"""
    dm = dm.copy()
    out = []
    for _ in range(k_per_image):
        idx = int(np.nanargmax(dm))
        i, j = divmod(idx, dm.shape[1])
        if not np.isfinite(dm[i, j]):
            break
        out.append((i, j, i + kx, j + ky))
        dm[max(0, i - kx):i + kx + 1, max(0, j - ky):j + ky + 1] = -np.inf
    return np.array(out, dtype=np.int32)


def pandas_reference(ref_dir, maps, kx, ky, k_per_image):
    """seconds per image of the reference's frame + sort + get_non_overlapping, and its boxes"""
    import ast

    import pandas as pd
    path = os.path.join(ref_dir, "diffmining", "typicality", "utils.py")
    tree = ast.parse(open(path).read())
    ns = {"np": np, "pd": pd}
    for name in ("sort", "get_non_overlapping"):
        node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
        exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    times, boxes = [], []
    for dm in maps:
        t0 = time.perf_counter()
        df = [("x.jpg", i, j, i + kx, j + ky, dm[i, j], "real") for i in range(dm.shape[0]) for j in range(dm.shape[1])]
        df = pd.DataFrame(df, columns=["seed", "x_start", "y_start", "x_end", "y_end", "D", "origin"])
        got = ns["get_non_overlapping"](ns["sort"](df, "D", ascending=False), k_per_image=k_per_image)
        times.append(time.perf_counter() - t0)
        boxes.append(got[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32))
    return times, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--reference-images", type=int, default=3)
    ap.add_argument("--save-maps", default=None)
    ap.add_argument("--reference-maps", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mining_rate.txt"))
    a = ap.parse_args()
    if a.reference_maps:
        assert a.reference, "--reference-maps needs --reference"
        f = np.load(a.reference_maps)
        n = len(f["boxes"])
        tp, pb = pandas_reference(a.reference, [f[f"map{b}"] for b in range(n)], 64, 64, 5)
        same_p = all(np.array_equal(f["boxes"][b], pb[b]) for b in range(n))
        line = (f"(a) the reference's pandas path, single process, on the CPU of the build machine ({os.cpu_count()} cores; NOT the GPU box), "
                f"{n} pooled maps stored by the run above: median {statistics.median(tp):.2f} s per image = "
                f"{1.0 / statistics.median(tp):.2f} images/s; same boxes as the batched call: {same_p}\n")
        print(line, end="")
        with open(a.out, "a") as fo:
            fo.write(line)
        return
    import torch
    from diff_mining_amd.engine import UNetEngine
    if not torch.cuda.is_available():
        sys.exit("mining_rate needs the GPU: a rate is measured there or not at all")
    assert a.reps >= 20, "median of at least 20 repetitions"
    eng = UNetEngine(0)
    H, W, h, w, kx, ky, k = 512, 683, 64, 85, 64, 64, 5
    g = torch.Generator().manual_seed(20261017)
    grids = [(1.0 + 0.3 * torch.randn(a.draws, 2, 4, h, w, generator=g) + 0.05 * torch.randn(1, 2, 1, h, w, generator=g)).half().cuda()
             for _ in range(a.images)]
    sizes = [(H, W)] * a.images

    def batched():
        maps = eng.typicality_image_batched(grids, sizes, kx, ky)
        return maps, eng.mine_patches(maps, kx, ky, k)

    def loop():
        out = []
        for gr in grids:
            out.append(greedy_host(eng.typicality_image(gr, (H, W), kx, ky).cpu().numpy(), kx, ky, k))
        return out
    for _ in range(3):
        maps, (boxes, D, count) = batched()
    torch.cuda.synchronize()
    ts, ts_maps = [], []
    for _ in range(a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        maps = eng.typicality_image_batched(grids, sizes, kx, ky)
        e1.record()
        eng.mine_patches(maps, kx, ky, k)
        e2.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e2))
        ts_maps.append(e0.elapsed_time(e1))
    # the host clock around the same call including the copy of the winners: what the caller waits for
    tw = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, (bx, dv, cn) = batched()
        bx.cpu(), dv.cpu(), cn.cpu()
        tw.append((time.perf_counter() - t0) * 1e3)
    loop()
    tl = []
    for _ in range(a.loop_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_boxes = loop()
        tl.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(boxes[b, :int(count[b])].cpu().numpy(), host_boxes[b]) for b in range(a.images))
    med, med_maps, med_w, med_l = (statistics.median(v) for v in (ts, ts_maps, tw, tl))
    lines = [
        f"mining rate: {a.images} images of {H}x{W} (latents {h}x{w}, {a.draws} draws x 2 prompts, fp16 grids on the device), "
        f"{kx}x{ky} windows, k_per_image {k}: grids -> boxes",
        f"device: {torch.cuda.get_device_name(0)}",
        f"batched (typicality_image_batched + mine_patches, one call): device events, median of {a.reps}: {med:.3f} ms "
        f"(min {min(ts):.3f}, max {max(ts):.3f}; maps {med_maps:.3f} ms, packing + selection {med - med_maps:.3f} ms) = "
        f"{a.images / med * 1e3:.0f} images/s",
        f"batched, host clock incl. the copy of the winners to the host, median of {a.reps}: {med_w:.3f} ms = {a.images / med_w * 1e3:.0f} images/s",
        f"(b) per-image typicality_image loop + map to the host + numpy greedy, host clock, median of {a.loop_reps}: {med_l:.1f} ms "
        f"(min {min(tl):.1f}, max {max(tl):.1f}) = {a.images / med_l * 1e3:.0f} images/s",
        f"batched vs (b): {med_l / med_w:.1f}x (host clock both); same boxes: {same}",
    ]
    if a.reference:
        n = min(a.reference_images, a.images)
        host_maps = [eng.typicality_image(gr, (H, W), kx, ky).cpu().numpy() for gr in grids[:n]]
        tp, pb = pandas_reference(a.reference, host_maps, kx, ky, k)
        same_p = all(np.array_equal(boxes[b, :int(count[b])].cpu().numpy(), pb[b]) for b in range(n))
        lines.append(f"(a) the reference's pandas path on this CPU, single process, {n} images: median {statistics.median(tp):.2f} s per image "
                     f"= {1.0 / statistics.median(tp):.2f} images/s; same boxes: {same_p}")
    else:
        lines.append("(a) the reference's pandas path: not measured in this run (no --reference checkout on this machine)")
    if a.save_maps:
        n = min(a.reference_images, a.images)
        os.makedirs(os.path.dirname(os.path.abspath(a.save_maps)), exist_ok=True)
        np.savez_compressed(a.save_maps, boxes=boxes[:n].cpu().numpy(), **{f"map{b}": maps[b].cpu().numpy() for b in range(n)})
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
