#!/usr/bin/env python
"""Rate of the clustering stage's last step on one MI355X: `clustering.kmeans_fit` + `clustering.rank_clusters` at the reference's
size (1000 patches, k = 32) for CLIP (512) and CLIP+DIFT (1792) features.

  device   device events around the fit and around the rank, warm-up, median of --reps (>= 20)
  host clock  fit + rank + the copy of the labels and the ranking to the host
  numpy    clustering.kmeans_fit_host + rank_clusters_host on the host
  sklearn  KMeans(n_clusters=32, random_state=10).fit where scikit-learn is importable (the fit only)

Writes the table to stdout and, with --out, to a file (profiles/cluster_rate.txt).
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
from diff_mining_amd import clustering as CL  # noqa: E402


def blobs(n, d, seed):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((40, d))[rs.randint(0, 40, size=n)] + 0.08 * rs.standard_normal((n, d))
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"cluster rate: n = 1000, k = 32, KMeans(random_state=10) + ranked clusters (centroid order, median); device: {torch.cuda.get_device_name(0)}"]
    for d in (512, 1792):
        X = blobs(1000, d, 27)
        D = np.random.RandomState(1).standard_normal(1000).astype(np.float32)
        Xd, Dd = torch.from_numpy(X).cuda(), torch.from_numpy(D).cuda()
        work = torch.empty(CL.workspace_bytes(1000, d, 32), dtype=torch.uint8, device="cuda")
        fit_ms, rank_ms, wall_ms = [], [], []
        for rep in range(a.reps + 3):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e[0].record()
            labels, centers, seeds, inertia, n_iter = CL.kmeans_fit(Xd, 32, work=work)
            e[1].record()
            rank = CL.rank_clusters(Xd, labels, centers, Dd, work=work)
            e[2].record()
            got = [labels.cpu().numpy()] + [r.cpu().numpy() for r in rank]
            t1 = time.perf_counter()
            if rep >= 3:
                fit_ms.append(e[0].elapsed_time(e[1]))
                rank_ms.append(e[1].elapsed_time(e[2]))
                wall_ms.append((t1 - t0) * 1e3)
        host_ms = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            hl, hc, hs, hi, hn = CL.kmeans_fit_host(X, 32)
            hr = CL.rank_clusters_host(X, hl, hc, D)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        same = np.array_equal(hl, got[0]) and np.array_equal(hr[0], got[1]) and hn == int(n_iter)
        med = statistics.median
        lines.append(f"1000 x {d}: {int(n_iter)} Lloyd iterations")
        lines.append(f"  device events, median of {a.reps}: fit {med(fit_ms):.3f} ms (min {min(fit_ms):.3f}, max {max(fit_ms):.3f}), "
                     f"rank {med(rank_ms):.3f} ms (min {min(rank_ms):.3f}, max {max(rank_ms):.3f})")
        lines.append(f"  host clock incl. the copy of the labels and the ranking, median of {a.reps}: {med(wall_ms):.3f} ms")
        lines.append(f"  numpy restatement (kmeans_fit_host + rank_clusters_host), median of {a.host_reps}: {med(host_ms):.1f} ms; "
                     f"same labels, n_iter and order: {same}")
        try:
            from sklearn.cluster import KMeans
            sk = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                km = KMeans(n_clusters=32, random_state=10).fit(X)
                sk.append((time.perf_counter() - t0) * 1e3)
            lines.append(f"  scikit-learn KMeans.fit alone, median of {a.host_reps}: {med(sk):.1f} ms ({os.cpu_count()} CPUs visible); "
                         f"same labels: {np.array_equal(km.labels_, got[0])}")
        except ImportError:
            lines.append("  scikit-learn: not importable here")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
