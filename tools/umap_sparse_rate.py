#!/usr/bin/env python
"""Rate of the UMAP route without the n x n graph (umapfit route='sparse'; csrc/umap_sparse.hip) on one MI355X, by the method of
tools/umap_rate.py: host clock with a device synchronisation at each step boundary, one warm-up, median of --reps.

  4000 x 1280 -> 32      both routes, one after the other in this process: what the new blocking costs or gains against the dense
                         route's kernels at a size both take (init solver 'device' on both, so the routes differ in nothing else)
  10 000 x 1280 -> 32    the sparse route at the parallel dataset's default size (cluster.py:391), both init solvers
  compress               10 000 x (10 x 1280) -> 10 x 32, ten fits, both init solvers

Inputs are Gaussian clouds (tests/umap_cases.cloud), which come out connected at these sizes; unit-normalised blobs do not (32
components at 10 000 x 128 on the CPU).  Every line says which initialisation ran.  No time is required of this tool, and above 4095
rows there is no earlier figure to compare with.  Writes the table to stdout and, with --out, to a file (profiles/umap_sparse_rate.txt).
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


def device_fit_ms(X, dim, reps, solver, route, warm=1):
    """median ms per step over `reps` fits (after `warm` warm-ups), and the last fit"""
    rows = []
    for rep in range(reps + warm):
        times = {}
        fit = UM.umap_fit(X, dim, 15, UC.SEED, times=times, init_solver=solver, route=route)
        if rep >= warm:
            rows.append([times[s] * 1e3 for s in STEPS])
    return [statistics.median(c) for c in zip(*rows)], fit


def fmt(ms):
    return ", ".join(f"{s} {v:.2f}" for s, v in zip(STEPS, ms)) + f"; total {sum(ms):.2f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-compress", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(line):                   # every line goes to stdout (and to --out) as soon as it is measured
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def describe(fit):
        return (f"route {fit['route']}, init solver {fit['init_solver']}: init {fit['init_used']} ({fit['init_iters']} outer iterations), "
                f"{fit['n_edges']} edges")

    say(f"umap sparse rate: n_neighbors 15, seed {UC.SEED}, Gaussian clouds; device: {torch.cuda.get_device_name(0)}; {os.cpu_count()} CPUs "
        f"visible.  Parity with umap-learn: unpinned (umapfit.py); above 4095 rows umap-learn is approximate and unseeded, this is exact.")
    X4 = torch.from_numpy(UC.cloud(4000, 1280, 4)).cuda()
    fits = {}
    for route in ("dense", "sparse"):
        ms, fits[route] = device_fit_ms(X4, 32, a.reps, "device", route)
        say(f"4000 x 1280 -> 32, 500 epochs, {describe(fits[route])}")
        say(f"  device, median of {a.reps}: {fmt(ms)}")
    same = torch.equal(fits["dense"]["embedding"].view(torch.int32), fits["sparse"]["embedding"].view(torch.int32))
    say(f"  the two routes' embeddings are {'bit-equal' if same else 'NOT bit-equal'}")
    del X4
    X10 = torch.from_numpy(UC.cloud(10000, 1280, 10)).cuda()
    for solver in UM.INIT_SOLVERS:
        ms, fit = device_fit_ms(X10, 32, a.reps, solver, "auto")
        say(f"10000 x 1280 -> 32, {UM.default_epochs(10000)} epochs, {describe(fit)}")
        say(f"  device, median of {a.reps}: {fmt(ms)}")
    del X10
    if a.no_compress:
        return
    Xg = torch.from_numpy(np.hstack([UC.cloud(10000, 1280, 20 + g) for g in range(10)])).cuda()
    for solver in UM.INIT_SOLVERS:
        total, inits, iters, solvers = np.zeros(4), [], [], set()
        for g in range(10):
            ms, fit = device_fit_ms(Xg[:, g * 1280:(g + 1) * 1280], 32, a.reps, solver, "auto", warm=1 if g == 0 else 0)
            total += ms
            inits.append(fit["init_used"])
            iters.append(fit["init_iters"])
            solvers.add(fit["init_solver"])
        t0 = time.perf_counter()
        emb = UM.compress(Xg, 10, 32, 15, seed=UC.SEED, init_solver=solver)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        say(f"10000 x (10 x 1280) -> 10 x 32 (compress), init solver {' / '.join(sorted(solvers))}: embedding {tuple(emb.shape)}, init "
            f"{inits.count('spectral')} spectral / {inits.count('random')} random, outer iterations {min(iters)}..{max(iters)}")
        say(f"  device, ten fits, each step the sum of the per-group medians of {a.reps}: {fmt(list(total))}")
        say(f"  device, one compress() call, host clock: {wall:.2f} ms")


if __name__ == "__main__":
    main()
