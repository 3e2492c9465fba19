#!/usr/bin/env python
"""Rate of the batched SVM fit on one MI355X at the reference's batch: K = 64 detectors, each 5 positives + 25 000 negatives of 2112
features (doersch/doersch.py:462-471), rows already on the device in one shared pool.

  fit      `doersch.svm_fit` (dm_svm_fit: two streaming passes over a detector's rows per SMO iteration), whole calls
  hard     `doersch.svm_hard_negatives` (one more pass, compaction and sort)
  sklearn  the same 64 fits by `SVC(C=0.1, kernel='linear')` on 8 joblib workers, as the reference runs them, when scikit-learn and
           joblib are importable (the rows are copied to the host first; that copy is not timed)

The device calls are timed with device events around whole calls after a warm-up call; medians of --reps.  Reported: milliseconds per
batch, microseconds per (iteration, detector) — the batch's time over the sum of the detectors' n_iter: detectors that stop early
still ride along until the slowest one stops, which this figure charges —, and the achieved share of the HBM rate: two passes of
n C 2 bytes per iteration and running detector against the chip's HBM figure (6.3 TB/s measured, 8 TB/s nominal).  By default no two
detectors share a row (a pool of 6.8 GB, far more than every cache), so row bytes are HBM bytes; with --pool N the detectors draw from N
shared rows and part of the traffic is served by the caches.  Prints a table and one JSON line; --out writes both to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import doersch as D  # noqa: E402

HBM_MEASURED_TBS, HBM_NOMINAL_TBS = 6.3, 8.0


def features(n, channels, seed):
    """fp16 [n, channels] on the device: sparse non-negative rows of unit norm, as normalised HOG-LAB cells are"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, channels, dtype=torch.float16, device="cuda")
    for at in range(0, n, 65536):
        m = min(65536, n - at)
        f = torch.rand(m, channels, generator=g, device="cuda") ** 2 * (torch.rand(m, channels, generator=g, device="cuda") < 0.1)
        f[:, 0] += 1e-3
        out[at:at + m] = (f / f.norm(dim=1, keepdim=True)).half()
    return out


def sklearn_fit(X, n_pos):
    from sklearn.svm import SVC
    svm = SVC(C=0.1, kernel="linear").fit(X, [1] * n_pos + [-1] * (len(X) - n_pos))
    return int(svm.n_iter_[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detectors", type=int, default=64)
    ap.add_argument("--positives", type=int, default=5)
    ap.add_argument("--negatives", type=int, default=25000)
    ap.add_argument("--channels", type=int, default=2112)
    ap.add_argument("--pool", type=int, default=0, help="negative rows in the shared pool, from which every detector draws its own; "
                    "0: detectors x negatives rows, dealt out so that no two detectors share one (6.8 GB at the default size)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    K, n_pos, n_neg, Cc = a.detectors, a.positives, a.negatives, a.channels
    n = n_pos + n_neg
    # per detector: its own positives (a seed row and noisy copies), and its own draw of negatives from the shared pool
    disjoint = a.pool <= 0
    if disjoint:
        a.pool = K * n_neg
    negatives = features(a.pool, Cc, 5)
    seeds = features(K, Cc, 6)
    g = torch.Generator(device="cuda").manual_seed(7)
    pos = seeds[:, None, :].float() + 0.02 * torch.rand(K, n_pos, Cc, generator=g, device="cuda")
    pos = (pos / pos.norm(dim=2, keepdim=True)).half().view(K * n_pos, Cc)
    pool = torch.cat([pos, negatives])
    table = torch.empty(K, n, dtype=torch.int32, device="cuda")
    gen = torch.Generator().manual_seed(8)
    deal = torch.randperm(a.pool, generator=gen) if disjoint else None
    for k in range(K):
        table[k, :n_pos] = torch.arange(k * n_pos, (k + 1) * n_pos)
        draw = deal[k * n_neg:(k + 1) * n_neg] if disjoint else torch.randperm(a.pool, generator=gen)[:n_neg]
        table[k, n_pos:] = (K * n_pos + draw).int()
    work = torch.empty(D.svm_workspace_bytes(K, n), dtype=torch.uint8, device="cuda")

    def timed(fn):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        out = fn()
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]), out

    fit = lambda: D.svm_fit(pool, table, n, n_pos, 0.1, 1e-3, -1, work)                                  # noqa: E731
    _, (w, b, n_iter, status, _) = timed(fit)
    hard = lambda: D.svm_hard_negatives(pool, table, n, n_pos, n_neg, w, b, work)                         # noqa: E731
    timed(hard)
    ms_fit = [timed(fit)[0] for _ in range(a.reps)]
    ms_hard = [timed(hard)[0] for _ in range(a.reps)]
    _, _, count = hard()
    iters = n_iter.cpu().numpy().astype(np.int64)
    med = statistics.median
    m = med(ms_fit)
    bytes_moved = 2.0 * n * Cc * 2 * float(iters.sum())
    res = {"workload": f"K = {K} detectors of {n_pos} + {n_neg} samples x {Cc} features, pool of {len(pool)} rows "
                       f"({'no row shared between detectors' if disjoint else 'detectors draw from one pool and share rows'})",
           "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "n_iter": {"min": int(iters.min()), "median": float(np.median(iters)), "max": int(iters.max()), "sum": int(iters.sum())},
           "status": sorted(set(status.cpu().tolist())), "hard_negatives": int(count.sum()),
           "fit": {"ms_median": round(m, 3), "ms_min": round(min(ms_fit), 3), "ms_max": round(max(ms_fit), 3),
                   "us_per_iteration_and_detector": round(m * 1e3 / float(iters.sum()), 3),
                   "ms_per_lockstep_iteration": round(m / float(iters.max()), 4),
                   "row_tb_per_s": round(bytes_moved / (m * 1e-3) / 1e12, 3),
                   "share_of_measured_hbm": round(bytes_moved / (m * 1e-3) / 1e12 / HBM_MEASURED_TBS, 3)},
           "hard": {"ms_median": round(med(ms_hard), 3), "ms_min": round(min(ms_hard), 3), "ms_max": round(max(ms_hard), 3),
                    "row_tb_per_s": round(K * n * Cc * 2.0 / (med(ms_hard) * 1e-3) / 1e12, 3)},
           "hbm_tb_per_s_measured": HBM_MEASURED_TBS, "hbm_tb_per_s_nominal": HBM_NOMINAL_TBS}
    lines = [f"svm rate: {res['workload']}; device: {res['device']}; medians of {a.reps}",
             f"  n_iter per detector: min {res['n_iter']['min']}, median {res['n_iter']['median']:.0f}, max {res['n_iter']['max']}; "
             f"statuses {res['status']}; {res['hard_negatives']} hard negatives",
             f"  fit : {m:.2f} ms per batch (min {min(ms_fit):.2f}, max {max(ms_fit):.2f}) = "
             f"{res['fit']['us_per_iteration_and_detector']:.2f} us per iteration and detector, {res['fit']['ms_per_lockstep_iteration']:.3f} ms "
             f"per lock-step iteration; rows at {res['fit']['row_tb_per_s']:.2f} TB/s = {res['fit']['share_of_measured_hbm']:.2f} of the "
             f"measured HBM rate ({HBM_MEASURED_TBS} TB/s; {HBM_NOMINAL_TBS} nominal)",
             f"  hard: {res['hard']['ms_median']:.2f} ms per batch (min {res['hard']['ms_min']:.2f}, max {res['hard']['ms_max']:.2f}), rows at "
             f"{res['hard']['row_tb_per_s']:.2f} TB/s"]
    if not a.no_sklearn:
        try:
            import joblib
            import sklearn  # noqa: F401
        except ImportError:
            lines.append("  sklearn: scikit-learn or joblib not importable, not timed")
        else:
            pool_h, table_h = pool.cpu().numpy(), table.cpu().numpy()
            t0 = time.perf_counter()                       # rows travel to the workers as they are dispatched, not through a memmap
            its = joblib.Parallel(n_jobs=a.workers, max_nbytes=None)(joblib.delayed(sklearn_fit)(pool_h[table_h[k]], n_pos) for k in range(K))
            dt = time.perf_counter() - t0
            res["sklearn"] = {"s_per_batch": round(dt, 3), "workers": a.workers, "n_iter_equal": bool((np.array(its) == iters).all()),
                              "over_fit": round(dt * 1e3 / m, 1)}
            lines.append(f"  sklearn: {dt:.2f} s per batch on {a.workers} joblib workers = {dt * 1e3 / m:.1f} x the device fit; n_iter "
                         f"{'equal' if res['sklearn']['n_iter_equal'] else 'NOT equal'} to the device's for every detector")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
