#!/usr/bin/env python
"""Rate of the detector initialisation on one MI355X (doersch/doersch.py:317-385), features already on the device.

  search   one chunk of 16 images of 57 x 57 cells x 2112 channels against K = 4096 random detectors,
             wide   `doersch.wide_winners` (dm_dense_wide_winners), one call
             loop   the parent commit's only route: `doersch.winners` (dm_dense_search_winners) over 32 blocks of 128 detectors
           timed with device events around whole routes, after a warm-up, in alternating order (wide, loop, loop, wide, ...);
           medians of --reps.  The two tables must be equal bit for bit, or the tool fails.  Reported: milliseconds, the fp16 MFMA
           TFLOP/s of both routes (2 cells C K per image; what the matrix cores sustain alone on this box next to it) and loop / wide.
  ranking  `doersch.detector_rank` (dm_detector_rank) at N = 25 000 candidates of L = 50 neighbours, num_detectors = 1000, on
           synthetic near-duplicate lists (groups of candidates that share most of their images at nearby corners): milliseconds,
           how many candidates the visit took and how many it accepted.

Prints a table and one JSON line; --out writes both to a file (profiles/detector_init_rate.txt).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import doersch as D  # noqa: E402
from diff_mining_amd.engine import load_library  # noqa: E402


def features(n, cells, channels, seed):
    """fp16 [n, cells, channels] on the device: sparse non-negative rows of unit norm, as normalised HOG-LAB cells are"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(n, cells, channels, dtype=torch.float16, device="cuda")
    for b in range(n):
        f = torch.rand(cells, channels, generator=g, device="cuda") ** 2 * (torch.rand(cells, channels, generator=g, device="cuda") < 0.1)
        f[:, 0] += 1e-3
        out[b] = (f / f.norm(dim=1, keepdim=True)).half()
    return out


def near_duplicate_lists(N, L, n_images, group, seed):
    """key int32 [N], nb_image / nb_x / nb_y int32 [N, L], nb_count int32 [N]: groups of `group` candidates around a base list of L
    distinct images; a member replaces one entry in four by another image and moves every corner by 8 * (-2 ... 2)"""
    rng = np.random.default_rng(seed)
    img, x, y = (np.empty((N, L), dtype=np.int32) for _ in range(3))
    for k0 in range(0, N, group):
        m = min(group, N - k0)
        base = rng.choice(n_images, size=L, replace=False)
        rows = np.tile(base, (m, 1))
        swap = rng.random((m, L)) < 0.25
        rows[swap] = n_images + rng.integers(0, 1 << 20, size=int(swap.sum()))       # images nobody else holds (distinct with near certainty per row)
        for r in range(m):                                                           # the contract: an image at most once per list
            while len(np.unique(rows[r])) < L:
                rows[r, swap[r]] = n_images + rng.integers(0, 1 << 20, size=int(swap[r].sum()))
        img[k0:k0 + m] = rows
        x[k0:k0 + m] = 8 * rng.integers(4, 40, size=L)[None, :] + 8 * rng.integers(-2, 3, size=(m, L))
        y[k0:k0 + m] = 8 * rng.integers(4, 40, size=L)[None, :] + 8 * rng.integers(-2, 3, size=(m, L))
    return rng.integers(0, 21, size=N).astype(np.int32), img, x, y, np.full(N, L, dtype=np.int32)


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--side", type=int, default=57)
    ap.add_argument("--channels", type=int, default=2112)
    ap.add_argument("--detectors", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=25000)
    ap.add_argument("--neighbours", type=int, default=50)
    ap.add_argument("--num-detectors", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    n, cells, Cc, K = a.images, a.side * a.side, a.channels, a.detectors
    data = features(n, cells, Cc, 5)
    w = torch.randn(K, Cc, generator=torch.Generator().manual_seed(6)).half().cuda()
    tables = {name: (torch.empty(K, n, dtype=torch.float32, device="cuda"), torch.empty(K, n, dtype=torch.int32, device="cuda"))
              for name in ("wide", "loop")}
    wide_work = torch.empty(D.wide_workspace_bytes(n, cells, K), dtype=torch.uint8, device="cuda")
    loop_work = torch.empty(D.workspace_bytes(n, cells, D.DENSE_MAX_DETECTORS), dtype=torch.uint8, device="cuda")
    blocks = [(k0, min(K, k0 + D.DENSE_MAX_DETECTORS)) for k0 in range(0, K, D.DENSE_MAX_DETECTORS)]

    def wide():
        D.wide_winners(data, w, tables["wide"][0], tables["wide"][1], 0, None, wide_work)

    def loop():
        for k0, k1 in blocks:
            D.winners(data, w[k0:k1], tables["loop"][0][k0:k1], tables["loop"][1][k0:k1], 0, None, loop_work)

    routes = {"wide": wide, "loop": loop}
    for _ in range(2):
        wide()
        loop()
    torch.cuda.synchronize()
    assert torch.equal(tables["wide"][0].view(torch.int32), tables["loop"][0].view(torch.int32)), "wide and narrow scores differ"
    assert torch.equal(tables["wide"][1], tables["loop"][1]), "wide and narrow cells differ"
    ms = {"wide": [], "loop": []}
    for rep in range(a.reps):
        for name in (("wide", "loop") if rep % 2 == 0 else ("loop", "wide")):
            ms[name].append(timed(routes[name]))
    tf, ghz = C.c_double(), C.c_double()
    rc = load_library().dm_measure_mfma_rate(C.c_void_p(torch.cuda.current_stream().cuda_stream), 80000, 0, C.byref(tf), C.byref(ghz))
    assert rc == 0
    flop = 2.0 * n * cells * Cc * K
    res = {"workload": f"{n} images of {a.side}x{a.side}x{Cc}, K = {K}", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "tables_bit_equal": True}
    for name in ("wide", "loop"):
        m = statistics.median(ms[name])
        res[name] = {"ms_median": round(m, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "tflops": round(flop / (m * 1e-3) / 1e12, 1)}
    ratio = res["loop"]["ms_median"] / res["wide"]["ms_median"]
    res.update({"mfma_only_tflops_measured": round(tf.value, 1), "loop_over_wide": round(ratio, 3),
                "verdict": "the wide route is not slower than the loop" if ratio >= 1.0 else "THE WIDE ROUTE IS SLOWER THAN THE LOOP"})

    N, L, nd = a.candidates, a.neighbours, a.num_detectors
    lists = [torch.from_numpy(t).cuda() for t in near_duplicate_lists(N, L, 20000, 8, 7)]
    out = {}

    def rank():
        out["accepted"], out["n"] = D.detector_rank(*lists, nd)
    rank()
    torch.cuda.synchronize()
    rank_ms = [timed(rank) for _ in range(3)]
    accepted, n_acc = out["accepted"].cpu().numpy(), int(out["n"].cpu()[0])
    key = lists[0].cpu().numpy()
    order = np.argsort(-key.astype(np.int64), kind="stable")
    visited = int(np.flatnonzero(order == accepted[n_acc - 1])[0]) + 1 if n_acc == nd else N
    res["ranking"] = {"N": N, "L": L, "num_detectors": nd, "ms_median": round(statistics.median(rank_ms), 3), "ms_min": round(min(rank_ms), 3),
                      "ms_max": round(max(rank_ms), 3), "accepted": n_acc, "visited": visited}
    lines = [f"detector init rate: {res['workload']}; device: {res['device']}; medians of {a.reps}, alternating order; tables bit-equal"]
    for name, what in (("wide", "one dm_dense_wide_winners call"), ("loop", f"{len(blocks)} dm_dense_search_winners calls of 128 detectors")):
        r = res[name]
        lines.append(f"  {name:4s}: {r['ms_median']:.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}), {r['tflops']:.1f} fp16 MFMA TFLOP/s  ({what})")
    lines.append(f"  matrix cores alone on this box: {res['mfma_only_tflops_measured']} TFLOP/s; loop / wide = {ratio:.3f}: {res['verdict']}")
    r = res["ranking"]
    lines.append(f"  ranking: N = {N}, L = {L}, num_detectors = {nd}: {r['ms_median']:.3f} ms (min {r['ms_min']:.3f}, max {r['ms_max']:.3f}); "
                 f"{r['visited']} candidates visited, {r['accepted']} accepted")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
