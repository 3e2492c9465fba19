#!/usr/bin/env python
"""Rate of the UMAP projection on one MI355X at the two product shapes, synthetic features (unit-normalised Gaussian blobs):

  main stage        umapfit.umap_fit(1000 x 1280 -> 5)                          (typicality/cluster.py: project=True)
  parallel dataset  umapfit.compress(1000 x (10 x 1280), 10 groups -> 10 x 32)   (parallel-dataset/cluster.py: compress)

  device   ms per fit split into kNN, graph (incl. the read of n_edges), init and layout (500 epochs); host clock with a device
           synchronisation at each boundary, warm-up, median of --reps.  init, per --init-solver (default: both, in this process, one
           after the other): 'host' = the copy of the dense graph, numpy eigh, the copy back; 'device' = dm_umap_spectral from the
           upload of its two random arrays to the read of its status record
  numpy    the restatement (umapfit.umap_fit_host) on the same machine, once; for the parallel shape --host-groups of the ten
           groups are run and the time is scaled to ten
  quality  trustworthiness (k = 15) of both embeddings, and for the test suite's blob cases the device figure beside the
           restatement's and its spread over five seeds (tests/umap_cases.py, measured on the CPU)

Writes the table to stdout and, with --out, to a file (profiles/umap_rate.txt; --append adds to it).
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
from diff_mining_amd import umapfit as UM  # noqa: E402
from tests import umap_cases as UC  # noqa: E402

STEPS = ("knn", "graph", "init", "layout")
NOISE = 3.5            # blobs wide enough for a connected graph: the spectral initialisation (numpy eigh of 1000 x 1000) is what runs


def device_fit_ms(X, dim, reps, solver="host"):
    """median ms per step over `reps` fits (after one warm-up), and the last fit"""
    rows = []
    for rep in range(reps + 1):
        times = {}
        fit = UM.umap_fit(X, dim, 15, UC.SEED, times=times, init_solver=solver)
        if rep:
            rows.append([times[s] * 1e3 for s in STEPS])
    return [statistics.median(c) for c in zip(*rows)], fit


def fmt(ms):
    return ", ".join(f"{s} {v:.2f}" for s, v in zip(STEPS, ms)) + f"; total {sum(ms):.2f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-groups", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--init-solver", choices=("host", "device", "both"), default="both")
    a = ap.parse_args()
    solvers = UM.INIT_SOLVERS if a.init_solver == "both" else (a.init_solver,)
    lines = []
    kept = open(a.out).read() if a.out and a.append and os.path.exists(a.out) else ""

    def say(line):                   # every line goes to stdout (and to --out) as soon as it is measured
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(kept + "\n".join(lines) + "\n")

    say(f"umap rate: n = 1000, n_neighbors 15, 500 epochs, seed {UC.SEED}; device: {torch.cuda.get_device_name(0)}; "
        f"{os.cpu_count()} CPUs visible.  Parity with umap-learn: unpinned (umapfit.py).")
    X5, _ = UC.blobs(1000, 1280, 20, 11, NOISE)
    Xg = np.hstack([UC.blobs(1000, 1280, 20, 20 + g, NOISE)[0] for g in range(10)])
    # main stage
    for solver in solvers:
        ms, fit = device_fit_ms(torch.from_numpy(X5).cuda(), 5, a.reps, solver)
        say(f"1000 x 1280 -> 5, init solver {fit['init_solver']}: init {fit['init_used']} ({fit['init_iters']} outer iterations), {fit['n_edges']} edges")
        say(f"  device, median of {a.reps}: {fmt(ms)}")
        say(f"  trustworthiness of the device embedding: {UC.trust(X5, fit['embedding'].cpu().numpy()):.4f}")
    if not a.no_host:
        times = {}
        t0 = time.perf_counter()
        h = UM.umap_fit_host(X5, 5, 15, UC.SEED, times=times)
        say(f"  numpy restatement, once: {fmt([times[s] * 1e3 for s in STEPS])} (wall {(time.perf_counter() - t0) * 1e3:.0f} ms); "
                     f"trustworthiness {UC.trust(X5, h['embedding']):.4f}")
    # parallel dataset: ten fits, one per group
    Xd = torch.from_numpy(Xg).cuda()
    for solver in solvers:
        total, inits, iters = np.zeros(4), [], []
        for g in range(10):
            ms, fit = device_fit_ms(Xd[:, g * 1280:(g + 1) * 1280], 32, a.reps, solver)
            total += ms
            inits.append(fit["init_used"])
            iters.append(fit["init_iters"])
        t0 = time.perf_counter()
        emb = UM.compress(Xd, 10, 32, 15, seed=UC.SEED, init_solver=solver)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        say(f"1000 x (10 x 1280) -> 10 x 32 (compress), init solver {solver}: embedding {tuple(emb.shape)}, init {inits.count('spectral')} spectral / "
            f"{inits.count('random')} random, outer iterations {min(iters)}..{max(iters)}")
        say(f"  device, ten fits, each step the sum of the per-group medians of {a.reps}: {fmt(list(total))}")
        say(f"  device, one compress() call, host clock: {wall:.2f} ms")
    if not a.no_host:
        rows = []
        for g in range(a.host_groups):
            times = {}
            UM.umap_fit_host(Xg[:, g * 1280:(g + 1) * 1280], 32, 15, UC.SEED, times=times)
            rows.append([times[s] * 1e3 for s in STEPS])
        scaled = [10.0 * float(np.mean(c)) for c in zip(*rows)]
        say(f"  numpy restatement, {a.host_groups} of the 10 groups run, scaled to 10: {fmt(scaled)}")
    # the suite's blob cases
    for tag in UC.BLOBS:
        X, k, dim, _ = UC.case(tag)
        fit = UM.umap_fit(torch.from_numpy(X).cuda(), dim, k, UC.SEED)
        say(f"{tag} ({X.shape[0]} x {X.shape[1]} -> {dim}): trustworthiness device {UC.trust(X, fit['embedding'].cpu().numpy()):.4f}; "
                     f"numpy restatement {UC.HOST_TRUST[tag]:.4f}, max - min over seeds {UC.SPREAD_SEEDS}: {UC.HOST_TRUST_SPREAD[tag]:.4f} (CPU)")


if __name__ == "__main__":
    main()
