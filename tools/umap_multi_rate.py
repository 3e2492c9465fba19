#!/usr/bin/env python
"""What UMAP's per-component initialisation (umapfit disconnected='components'; csrc/umap_multi.hip) costs and gives on one MI355X, by
the method of tools/umap_sparse_rate.py: host clock with a device synchronisation at each step boundary, one warm-up, median of --reps.

  10 000 x 128 -> 32     unit-normalised blobs (tests/umap_cases.blobs, 32 centres, noise 0.25), the parallel dataset's default size
  1000 x 1280 -> 5       unit-normalised blobs (12 centres, noise 0.25), the main stage's width

Per input: the component count, the components step (dm_umap_components alone), then per arm of `disconnected` and per init solver the
steps of the whole fit, and per arm the trustworthiness (k = 15) of the final embedding and Spearman's rank correlation of pairwise
distances, input against embedding (all pairs up to 2000 rows, a fixed sample of --pairs pairs above).  The 'random' arm is the fit
as it was before the option existed, measured in the same run: that is the yardstick, no threshold is set.  Writes the table to
stdout and, with --out, to a file (profiles/umap_multi_rate.txt)."""
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
from tests import umap_multi_cases as MC  # noqa: E402

STEPS = ("knn", "graph", "init", "layout")


def device_fit_ms(X, dim, reps, solver, arm, warm=1):
    rows = []
    for rep in range(reps + warm):
        times = {}
        fit = UM.umap_fit(X, dim, 15, UC.SEED, times=times, init_solver=solver, disconnected=arm)
        if rep >= warm:
            rows.append([times[s] * 1e3 for s in STEPS])
    return [statistics.median(c) for c in zip(*rows)], fit


def components_ms(X, reps, warm=1):
    idx, dist = UM.knn(X, 15)
    G = UM.fuzzy_graph(idx, dist, UM.default_epochs(len(X)))
    ms = []
    for rep in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = UM.components(G, X)
        torch.cuda.synchronize()
        if rep >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    sizes = np.diff(UM.components_to_host(out)["offsets"])
    return statistics.median(ms), sizes


def fmt(ms):
    return ", ".join(f"{s} {v:.2f}" for s, v in zip(STEPS, ms)) + f"; total {sum(ms):.2f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(line):                   # every line goes to stdout (and to --out) as soon as it is measured
        lines.append(line)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"umap multi-component rate: n_neighbors 15, seed {UC.SEED}, unit-normalised blobs; device: {torch.cuda.get_device_name(0)}.  Parity with "
        f"umap-learn: unpinned (umapfit.py).  'random' is the fit as it was before the option; 'components' is the option.")
    for n, d, centres, dim in ((10000, 128, 32, 32), (1000, 1280, 12, 5)):
        Xh = UC.blobs(n, d, centres, 0, 0.25)[0]
        X = torch.from_numpy(Xh).cuda()
        pairs = None if n <= 2000 else np.random.RandomState(0).randint(0, n, size=(a.pairs, 2))
        ms, sizes = components_ms(X, a.reps)
        say(f"{n} x {d} -> {dim}, {UM.default_epochs(n)} epochs: {len(sizes)} components, sizes {int(sizes.min())}..{int(sizes.max())}; "
            f"{int(UM.multi_component_plan(sizes, dim).sum())} solved, meta {'table' if len(sizes) <= 2 * dim else 'affinity'}")
        say(f"  components step (dm_umap_components with centroids), median of {a.reps}: {ms:.2f} ms")
        for arm in UM.DISCONNECTED:
            for solver in UM.INIT_SOLVERS:
                ms, fit = device_fit_ms(X, dim, a.reps, solver, arm)
                say(f"  {arm:10s} init solver {fit['init_solver']}: init {fit['init_used']} ({fit['init_iters']} outer iterations at the most"
                    f"{', reason ' + str(fit['init_reason']) if fit.get('init_reason') else ''}); median of {a.reps}: {fmt(ms)}")
            Y = fit["embedding"].cpu().numpy()
            say(f"  {arm:10s} quality (device solver): trustworthiness {MC.trust(Xh, Y):.4f}, Spearman of pairwise distances "
                f"{MC.spearman(Xh, Y, pairs):.4f} ({'all pairs' if pairs is None else str(len(pairs)) + ' sampled pairs'})")
        del X


if __name__ == "__main__":
    main()
