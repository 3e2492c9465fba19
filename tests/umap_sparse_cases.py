"""The inputs of the sparse-route UMAP tests (tests/test_umap_sparse.py, tests/test_gpu_umap_sparse.py,
tests/test_gpu_umap_sparse_guards.py) and the bounds measured for the ones above the dense route's limit.

Small cases, where the sparse route must give the dense route's bits: the cases of tests/umap_cases.py, and
  tall     cloud(1100, 5), k 15, dim 2: past 1024 rows (two passes of the prefix sum), 35 row blocks and 5 column tiles of the kNN
           kernel, the last of both ragged;
  k64      cloud(130, 7), k 64, dim 2: the top-k at its cap, one key per lane;
  hub      300 equal rows, k 5, dim 2: every list is rows 0..4, so five rows have 299 edges (in-degree far past k and past a wave).
Cases past 4095 rows, against the numpy restatement's sparse route:
  big3     cloud(4200, 3), k 15, dim 2;
  big16    cloud(4200, 16), k 15, dim 32: block of 49 columns, rows of more than 64 edges;
  hub4096  4096 equal rows, k 5, dim 2: five rows of 4095 edges, every eigenvalue gap 0.

`python -m tests.umap_sparse_cases` measures and prints, per big case, what umap_cases.measure does (fp32 against float64 of the
restatement: sigma, weights, coordinates after one and three moving epochs; the distance of the nearest weight to the pruning
threshold), the edge count, the largest row, the restatement solver's iterations and the smallest eigenvalue gap of the dense `eigh`.
The figures below are that output; the GPU tests bound the kernels by 4 x them, the rule of umap_cases.BOUNDS."""
import functools

import numpy as np

from diff_mining_amd import umapfit as UM
from tests import umap_cases as UC

SEED_X = 7
# tag: (n, d, n_neighbors, n_components)
SMALL = {"tall": (1100, 5, 15, 2), "k64": (130, 7, 64, 2), "hub": (300, 1, 5, 2)}
BIG = {"big3": (4200, 3, 15, 2), "big16": (4200, 16, 15, 32), "hub4096": (4096, 1, 5, 2)}
EQUAL = list(UC.SHAPES) + list(SMALL)            # the cases on which both routes run
SOLVED = ("big3", "big16")                       # the big cases with a spectrum to compare
TOL = 1e-11                                      # the solver's stopping residual
MIN_GAP = 1e-5
MARGIN = 4.0


def case(tag):
    """(X, n_neighbors, n_components)"""
    if tag in UC.SHAPES:
        X, k, dim, _ = UC.case(tag)
        return X, k, dim
    n, d, k, dim = (SMALL.get(tag) or BIG[tag])
    X = np.zeros((n, d), np.float32) if tag.startswith("hub") else UC.cloud(n, d, SEED_X)
    return X, k, dim


@functools.lru_cache(maxsize=None)
def host(tag):
    """the restatement's sparse route on the case: kNN, the float64 graph; computed once, left unchanged"""
    X, k, dim = case(tag)
    idx, dist = UM.knn_host(X, k, route="sparse")
    return {"X": X, "k": k, "dim": dim, "n": len(X), "idx": idx, "dist": dist,
            "G": UM.fuzzy_graph_host(idx, dist, 500, np.float64, route="sparse")}


@functools.lru_cache(maxsize=None)
def solve(tag):
    """`spectral_init_iter_host` on the case's float64 graph: (Y0, used, info)"""
    h = host(tag)
    G = h["G"]
    return UM.spectral_init_iter_host(G["row_ptr"], G["col"], G["weight"], h["n"], h["dim"], UC.SEED)


@functools.lru_cache(maxsize=None)
def eigh(tag):
    """numpy's eigh of the dense M = D^-1/2 P D^-1/2 of the case's float64 graph: (val descending, vec, gap per eigenvalue)"""
    h = host(tag)
    G, n = h["G"], h["n"]
    P = np.zeros((n, n))
    P[np.repeat(np.arange(n), np.diff(G["row_ptr"])), G["col"]] = G["weight"]
    isd = 1.0 / np.sqrt(P.sum(axis=1))
    M = isd[:, None] * P * isd[None, :]
    val, vec = np.linalg.eigh((M + M.T) * 0.5)
    val, vec = val[::-1].copy(), vec[:, ::-1].copy()
    gap = np.minimum(np.abs(np.diff(val, prepend=np.inf)), np.abs(np.diff(val, append=-np.inf)))
    return val, vec, gap


def compare(tag, eigvals, eigvecs):
    """(largest |theta - lambda|, largest ||v - v_eigh||_2 / (2 TOL / gap), smallest gap) over the wanted pairs (Weyl, Davis-Kahan: see
    tests/umap_spectral_cases.py); v's sign is taken from eigh's"""
    val, vec, gap = eigh(tag)
    m = eigvecs.shape[1]
    sign = np.where((eigvecs * vec[:, :m]).sum(axis=0) < 0, -1.0, 1.0)
    dist = np.linalg.norm(eigvecs * sign[None, :] - vec[:, :m], axis=0)
    return float(np.abs(eigvals - val[:m]).max()), float((dist / (2.0 * TOL / gap[:m])).max()), float(gap[:m].min())


def tail(tag, eigvecs, seed=UC.SEED):
    h = host(tag)
    noise, _ = UM.spectral_host_arrays(h["n"], h["dim"], seed)
    return UM._spectral_tail(eigvecs[:, 1:], noise)


def threshold_gap(h):
    """min |P_ij - threshold| over the non-zero entries of the unpruned union, from the lists (umap_cases.threshold_gap without n x n)"""
    idx, dist, G, n = h["idx"], h["dist"], h["G"], h["n"]
    x = dist.astype(np.float64) - G["rho"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        val = np.where((x <= 0) | (G["sigma"][:, None] == 0), 1.0, np.exp(-(x / G["sigma"].astype(np.float64)[:, None]))).astype(np.float32)
    rows = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    cols = idx.astype(np.int64).ravel()
    ok = cols != rows
    rows, cols, a = rows[ok], cols[ok], val.ravel()[ok]
    keys = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))
    a_ij, a_ji = np.zeros(len(keys), np.float32), np.zeros(len(keys), np.float32)
    a_ij[np.searchsorted(keys, rows * n + cols)] = a
    a_ji[np.searchsorted(keys, cols * n + rows)] = a
    p = (a_ij + a_ji) - a_ij * a_ji
    return float(np.abs(p[p > 0].astype(np.float64) - float(G["threshold"])).min())


def measure(tag, a, b):
    h = host(tag)
    G64 = h["G"]
    G32 = UM.fuzzy_graph_host(h["idx"], h["dist"], 500, np.float32, route="sparse")
    same = np.array_equal(G64["row_ptr"], G32["row_ptr"]) and np.array_equal(G64["col"], G32["col"])
    out = {"sigma": float(np.abs(G64["sigma"].astype(np.float64) - G32["sigma"]).max()),
           "weight": float(np.abs(G64["weight"].astype(np.float64) - G32["weight"]).max()) if same else float("nan"),
           "gap": threshold_gap(h), "edges": len(G64["col"]), "row": int(np.diff(G64["row_ptr"]).max()),
           "n_comp": UM.components_host(G64["row_ptr"], G64["col"], h["n"])}
    if tag in SOLVED:
        Y0, used, info = solve(tag)
        out.update(iters=info["iters"], eig_gap=float(eigh(tag)[2][:h["dim"] + 1].min()))
        for count in (1, 3):
            last = UC.moving_epochs(count)
            y64, _ = UM.layout_host(G64["row_ptr"], G64["col"], G64["weight"], Y0, a, b, 500, UC.SEED, 0, last, np.float64)
            y32, _ = UM.layout_host(G64["row_ptr"], G64["col"], G64["weight"], Y0, a, b, 500, UC.SEED, 0, last, np.float32)
            out[f"layout{count}"] = float(np.abs(y64 - y32).max())
    return out


# ---- measured (python -m tests.umap_sparse_cases) -------------------------------------------------------------------------------------
BOUNDS = {
    "big3": {"sigma": 9.537e-07, "weight": 2.086e-06, "gap": 2.478e-04, "edges": 70934, "row": 27, "n_comp": 1, "iters": 9, "eig_gap": 1.125e-04, "layout1": 1.329e-06, "layout3": 1.173e-03},
    "big16": {"sigma": 1.907e-06, "weight": 2.921e-06, "gap": 2.210e-05, "edges": 93150, "row": 110, "n_comp": 1, "iters": 12, "eig_gap": 1.241e-04, "layout1": 5.862e-07, "layout3": 1.356e-04},
    "hub4096": {"sigma": 0.000e+00, "weight": 0.000e+00, "gap": 9.980e-01, "edges": 40930, "row": 4095, "n_comp": 1},
}


if __name__ == "__main__":
    a, b = UM.find_ab_params()
    print("BOUNDS = {")
    for tag in BIG:
        m = measure(tag, a, b)
        print(f'    "{tag}": {{' + ", ".join(f'"{k}": {v:.3e}' if isinstance(v, float) else f'"{k}": {v}' for k, v in m.items()) + "},")
    print("}")
