#!/usr/bin/env python
"""Rate of the parallel-dataset mining stage, grids -> rows: 8 groups x 10 sets of 512 x 683 images (64 x 85 latents, N draws x 2
prompts, fp16 grids on the device), 64 x 64 windows, k_per_image 5.

  batched   UNetEngine.typicality_image_batched (all 80 images) + mine_parallel (all 8 groups), device events around each,
            warm-up, median of --reps repetitions (>= 20).  The split of mine_parallel: the selection alone is timed as
            dm_mine_patches on the same median maps in place; median + gather is the rest, by difference.
  host      what a user had before: per group the batched maps, the ten maps copied to the host, np.median and a numpy greedy
            selection there (host clock around work that ends with the last selection)

    python tools/parallel_mining_rate.py [--groups 8] [--sets 10] [--reps 20] [--draws 10] [--out profiles/parallel_mining_rate.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.mining_rate import greedy_host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--sets", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--draws", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parallel_mining_rate.txt"))
    a = ap.parse_args()
    import torch
    from diff_mining_amd import engine as E
    if not torch.cuda.is_available():
        sys.exit("parallel_mining_rate needs the GPU: a rate is measured there or not at all")
    assert a.reps >= 20, "median of at least 20 repetitions"
    eng = E.UNetEngine(0)
    H, W, h, w, kx, ky, k = 512, 683, 64, 85, 64, 64, 5
    G, S = a.groups, a.sets
    g = torch.Generator().manual_seed(20261018)
    grids = [(1.0 + 0.3 * torch.randn(a.draws, 2, 4, h, w, generator=g) + 0.05 * torch.randn(1, 2, 1, h, w, generator=g)).half().cuda()
             for _ in range(G * S)]
    sizes = [(H, W)] * (G * S)

    def by_group(maps):
        return [maps[i * S:(i + 1) * S] for i in range(G)]

    def batched():
        maps = eng.typicality_image_batched(grids, sizes, kx, ky)
        return eng.mine_parallel(by_group(maps), kx, ky, k)

    def host():
        out = []
        for i in range(G):
            maps = eng.typicality_image_batched(grids[i * S:(i + 1) * S], sizes[:S], kx, ky)
            dm = np.median(np.stack([m.cpu().numpy() for m in maps], axis=0), axis=0)
            out.append(greedy_host(dm, kx, ky, k))
        return out
    for _ in range(3):
        boxes, D, set_D, count, medians = batched()
    torch.cuda.synchronize()
    # the selection alone: dm_mine_patches on the median maps where they lie
    base, off, copied = E.UNetEngine._place_maps(torch, medians, eng.device)
    assert not copied
    gdesc = np.zeros(G, dtype=E.MINE_DESC_DTYPE)
    gdesc["map_offset"], gdesc["H"], gdesc["W"] = off, H, W
    gdesc_d = torch.from_numpy(gdesc.view(np.uint8)).cuda()
    b2, d2, c2 = torch.empty_like(boxes), torch.empty_like(D), torch.empty_like(count)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def select_only():
        assert eng.lib.dm_mine_patches(eng._h, p(base), None, p(gdesc_d), G, kx, ky, k, 0, p(b2), p(d2), p(c2), eng._stream()) == 0
    select_only()
    torch.cuda.synchronize()
    assert torch.equal(b2, boxes) and torch.equal(c2, count)
    ts, ts_maps, ts_sel = [], [], []
    for _ in range(a.reps):
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record()
        maps = eng.typicality_image_batched(grids, sizes, kx, ky)
        e1.record()
        eng.mine_parallel(by_group(maps), kx, ky, k)
        e2.record()
        select_only()
        e3.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e2))
        ts_maps.append(e0.elapsed_time(e1))
        ts_sel.append(e2.elapsed_time(e3))
    tw = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bx, dv, sd, cn, _ = batched()
        bx.cpu(), dv.cpu(), sd.cpu(), cn.cpu()
        tw.append((time.perf_counter() - t0) * 1e3)
    host()
    th = []
    for _ in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_boxes = host()
        th.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(boxes[i, :int(count[i])].cpu().numpy(), host_boxes[i]) for i in range(G))
    med, med_maps, med_sel, med_w, med_h = (statistics.median(v) for v in (ts, ts_maps, ts_sel, tw, th))
    mine = med - med_maps
    n_cand = (H - kx + 1) * (W - ky + 1)
    lines = [
        f"parallel mining rate: {G} groups x {S} sets of {H}x{W} (latents {h}x{w}, {a.draws} draws x 2 prompts, fp16 grids on the device), "
        f"{kx}x{ky} windows, k_per_image {k}: grids -> rows",
        f"device: {torch.cuda.get_device_name(0)}",
        f"batched (typicality_image_batched + mine_parallel, one call each): device events, median of {a.reps}: {med:.3f} ms "
        f"(min {min(ts):.3f}, max {max(ts):.3f}) = {G / med * 1e3:.0f} groups/s",
        f"  split: maps {med_maps:.3f} ms; mine_parallel {mine:.3f} ms = selection alone {med_sel:.3f} ms (dm_mine_patches on the same "
        f"median maps, its own table read-back included) + median, gather, tables and upload {mine - med_sel:.3f} ms (by difference); "
        f"the median kernel moves {G * n_cand * (S + 1) * 4 / 1e6:.1f} MB",
        f"batched, host clock incl. the copy of the winners to the host, median of {a.reps}: {med_w:.3f} ms = {G / med_w * 1e3:.0f} groups/s",
        f"host path (per group: batched maps, {S} maps to the host, np.median + numpy greedy), host clock, median of {a.host_reps}: "
        f"{med_h:.1f} ms (min {min(th):.1f}, max {max(th):.1f}) = {G / med_h * 1e3:.1f} groups/s",
        f"batched vs host path: {med_h / med_w:.1f}x (host clock both); same boxes: {same}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()
