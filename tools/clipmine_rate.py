#!/usr/bin/env python
"""Rate of the CLIP baseline's mining stage, tokens -> boxes + features: 64 images of 512 x 512, 24 x 24 x 768 projected patch tokens
(fp32, on the device), 64 x 64 windows, k_per_image 5, mode diff.

  device      clipmine.rank_device, one dm_clipmine_rank call for all images: device events around the call (table upload, the four
              kernels), warm-up, median of --reps repetitions (>= 20); and the host clock around `rank_patches` including the copy of
              the rows to the host
  reference   the reference's own `dot_text_image` (clipmining/ranking.py:72-108: upsample 2 + 768 channels to 512 x 512, pool,
              topk, pandas frame, get_non_overlapping, crop means) on ONE image on this machine's CPU — only with --reference DIR (a
              checkout of the reference; its functions are compiled from its text with `ast`, nothing is copied).  Needs no GPU:
              a machine that has the checkout but no GPU appends its line to --out.

Both rows check their boxes against the float64 restatement (`rank_patches_host`) on the same seeded tokens.

    python tools/clipmine_rate.py [--images 64] [--reps 20] [--out profiles/clipmine_rate.txt]
    python tools/clipmine_rate.py --reference DIR [--reference-reps 3]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 512
GH = PW = 24
E = 768
KX = KY = 64
K = 5


def inputs(b, seed=20261019):
    """tokens [576, 768] fp32 of image b and the text [2, 768] (the same on every machine)"""
    rng = np.random.default_rng(seed)
    t0 = rng.standard_normal(E)
    t1 = t0 + 0.7 * rng.standard_normal(E)
    text = np.stack([t0 / np.linalg.norm(t0), t1 / np.linalg.norm(t1)]).astype(np.float32)
    rng = np.random.default_rng((seed, b))
    tokens = (rng.standard_normal((GH * PW, E)) + 0.5 * rng.standard_normal(E)) * rng.uniform(0.5, 2.0, size=(GH * PW, 1))
    return tokens.astype(np.float32), text


def host_boxes(b):
    from diff_mining_amd import clipmine as CM
    tokens, text = inputs(b)
    rows, _ = CM.rank_patches_host([tokens], text, [(H, W)], PW, K, KX, KY, "diff")
    return np.stack([rows[n] for n in ("x_start", "y_start", "x_end", "y_end")], axis=1)


def reference_row(ref_dir, reps):
    import ast
    import types

    import pandas as pd
    import torch
    from torch.nn.functional import interpolate
    ns = {"torch": torch, "pd": pd, "np": np, "interpolate": interpolate}

    def compile_from(rel, path):
        node = ast.parse(open(os.path.join(ref_dir, rel)).read())
        for name in path:
            node = next(ch for ch in ast.iter_child_nodes(node) if isinstance(ch, (ast.FunctionDef, ast.ClassDef)) and ch.name == name)
        exec(compile(ast.Module(body=[node], type_ignores=[]), os.path.join(ref_dir, rel), "exec"), ns)
        return ns[path[-1]]

    compile_from("clipmining/utils.py", ("pool",))
    compile_from("clipmining/utils.py", ("get_non_overlapping",))
    fn = compile_from("clipmining/ranking.py", ("CLIPRankCluster", "dot_text_image"))
    tokens, text = inputs(0)
    me = types.SimpleNamespace(mode="diff")
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        with torch.no_grad():
            df, emb = fn(me, "x.jpg", torch.from_numpy(text), torch.from_numpy(tokens)[None], (H, W), PW, K, KX, KY)
        ts.append(time.perf_counter() - t0)
    boxes = df[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32).reshape(-1, 4)
    same = np.array_equal(boxes, host_boxes(0))
    med = statistics.median(ts)
    return (f"reference: dot_text_image on ONE image, torch {torch.__version__} on the CPU of the build machine ({os.cpu_count()} cores, "
            f"{torch.get_num_threads()} torch threads; NOT the GPU box), median of {reps}: {med:.2f} s per image (min {min(ts):.2f}, max {max(ts):.2f}) "
            f"= {1.0 / med:.2f} images/s; {len(boxes)} boxes, same as the float64 restatement: {same}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--reference-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clipmine_rate.txt"))
    a = ap.parse_args()
    if a.reference:
        line = reference_row(a.reference, a.reference_reps)
        print(line, end="")
        with open(a.out, "a") as f:
            f.write(line)
        return
    import torch
    from diff_mining_amd import clipmine as CM
    if not torch.cuda.is_available():
        sys.exit("clipmine_rate needs the GPU: a rate is measured there or not at all")
    assert a.reps >= 20, "median of at least 20 repetitions"
    text = torch.from_numpy(inputs(0)[1]).cuda()
    tokens = [torch.from_numpy(inputs(b)[0]).cuda() for b in range(a.images)]
    packed = torch.stack(tokens)                              # [n, P, E]: rank_device packs a list into one buffer per call
    sizes = [(H, W)] * a.images
    kw = dict(pw=PW, k_per_image=K, kx=KX, ky=KY, mode="diff")
    for _ in range(3):
        boxes, D, count, feats = CM.rank_device(list(packed), text, sizes, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        CM.rank_device(list(packed), text, sizes, **kw)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    tw = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, f = CM.rank_patches(list(packed), text, sizes, images_per_call=a.images, **kw)
        torch.cuda.synchronize()
        tw.append((time.perf_counter() - t0) * 1e3)
    n_check = min(3, a.images)
    same = all(np.array_equal(boxes[b, :int(count[b])].cpu().numpy(), host_boxes(b)) for b in range(n_check))
    med, med_w = statistics.median(ts), statistics.median(tw)
    lines = [
        f"clip mining rate: {a.images} images of {H}x{W}, {GH}x{PW}x{E} projected patch tokens (fp32, on the device), {KX}x{KY} windows, "
        f"k_per_image {K}, diff: tokens -> boxes + features",
        f"device: {torch.cuda.get_device_name(0)}",
        f"rank_device (one dm_clipmine_rank call incl. packing the tokens and the table upload): device events, median of {a.reps}: {med:.3f} ms "
        f"(min {min(ts):.3f}, max {max(ts):.3f}) = {a.images / med * 1e3:.0f} images/s",
        f"rank_patches, host clock incl. the copy of the rows to the host, median of {a.reps}: {med_w:.3f} ms = {a.images / med_w * 1e3:.0f} images/s",
        f"rows found: {int(count.sum())} of {a.images * K} slots (the eligibility rule: 500 candidates per image, crowded around the peak); "
        f"same boxes as the float64 restatement on the first {n_check} images: {same}",
    ]
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
