#!/usr/bin/env python
"""Rate of the X-ray evaluation on one MI355X: `xray.xray_eval` on 8 heat-maps of 1024 x 1024 that are already on the device
(smoothed noise on the fixture's magnitude scale, boxes of about 300 x 400, the reference's 1000 thresholds).

  device      device events around one `xray_eval` call, warm-up, median of --reps (>= 20); the bytes the kernel must read (each map
              once) over that time, next to the chip's HBM figure (6.3 TB/s measured, 8 TB/s nominal)
  host clock  the same call plus the copy of the counts and `xray_scores_from_counts`
  host path   the maps copied to the host, then `xray_counts_host` + `xray_scores_from_counts`
  reference   the reference's expression (a thresholds x pixels comparison, compute.py:268-284) on ONE map, restated here

Writes the table to stdout and, with --out, to a file (profiles/xray_eval_rate.txt).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import xray as X  # noqa: E402

HBM_MEASURED_TBS, HBM_NOMINAL_TBS = 6.3, 8.0


def smoothed_noise(n, size, seed):
    """[n, size, size] fp32 on the device: white noise box-filtered to about 32 px and scaled to a standard deviation of 5e-3 (the
    threshold table spans 2e-7 ... 2e-2)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 1, size, size, generator=g, device="cuda")
    x = torch.nn.functional.avg_pool2d(x, 33, stride=1, padding=16)
    return (x / x.std() * 5e-3).squeeze(1).contiguous()


def reference_aucpr(bbox, dm):
    thresholds = 2 * 10 ** (-np.linspace(2, 7, 1000))
    x = np.zeros_like(dm)
    x[bbox[1]:bbox[3], bbox[0]:bbox[2]] = 1
    dm_flattened, x_flattened = dm.flatten(), x.flatten()
    tp = np.sum(dm_flattened[x_flattened == 1] > thresholds[:, np.newaxis], axis=1)
    fp = np.sum(dm_flattened[x_flattened == 0] > thresholds[:, np.newaxis], axis=1)
    denominator = tp + fp
    with np.errstate(all="ignore"):
        precision = np.where(denominator > 0, tp / denominator, 0)
        recall = tp / x.sum()
    return (np.trapz if hasattr(np, "trapz") else np.trapezoid)(precision, recall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, S = a.maps, a.size
    maps_d = smoothed_noise(n, S, 7)
    maps = [maps_d[b] for b in range(n)]
    rs = np.random.RandomState(3)
    boxes = []
    for _ in range(n):
        x1, y1 = int(rs.randint(0, S - 300)), int(rs.randint(0, S - 400))
        boxes.append((x1, y1, x1 + 300, y1 + 400))
    thr = X.xray_thresholds()
    work = torch.empty(X.workspace_bytes(n, len(thr), S * S), dtype=torch.uint8, device="cuda")
    dev_ms, wall_ms = [], []
    for rep in range(a.reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        got = X.xray_eval(maps, boxes, thr, work)
        e[1].record()
        mean, auc = X.xray_scores_from_counts(*got)
        t1 = time.perf_counter()
        if rep >= 3:
            dev_ms.append(e[0].elapsed_time(e[1]))
            wall_ms.append((t1 - t0) * 1e3)
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        hm = [m.cpu().numpy() for m in maps]
        h_mean, h_auc = X.xray_scores_from_counts(*X.xray_counts_host(hm, boxes, thr))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    ref_auc = reference_aucpr(boxes[0], hm[0])
    ref_ms = (time.perf_counter() - t0) * 1e3
    med = statistics.median
    bytes_read = n * S * S * 4
    lines = [f"xray eval rate: {n} maps of {S} x {S}, boxes 300 x 400, T = {len(thr)}; device: {torch.cuda.get_device_name(0)}",
             f"  device events, one xray_eval call, median of {a.reps}: {med(dev_ms):.3f} ms (min {min(dev_ms):.3f}, max {max(dev_ms):.3f}) "
             f"= {med(dev_ms) / n * 1e3:.1f} us per map (the call reads its two tables back before it launches)",
             f"  maps read once: {bytes_read / 1e6:.1f} MB -> {bytes_read / (med(dev_ms) * 1e-3) / 1e12:.3f} TB/s over the median, "
             f"{bytes_read / (min(dev_ms) * 1e-3) / 1e12:.3f} TB/s over the minimum (HBM: {HBM_MEASURED_TBS} TB/s measured, {HBM_NOMINAL_TBS} nominal)",
             f"  host clock incl. the copy of the counts and xray_scores_from_counts, median of {a.reps}: {med(wall_ms):.3f} ms",
             f"  host path (maps to the host, xray_counts_host, scores), median of {a.host_reps}: {med(host_ms):.1f} ms; "
             f"same auc bits: {h_auc.tobytes() == auc.tobytes()}, same mean bits: {h_mean.tobytes() == mean.tobytes()}",
             f"  the reference's expression on ONE map ({os.cpu_count()} CPUs visible): {ref_ms:.1f} ms; same auc bits: {ref_auc == auc[0]}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
