"""The inputs and the `eigh` yardstick of the spectral-initialisation tests (tests/test_umap_spectral.py on the CPU,
tests/test_gpu_umap_spectral.py and tests/test_gpu_umap_spectral_guards.py on the GPU).

Cases: the cases of tests/umap_cases.py; `cloud1000`, a Gaussian cloud 1000 x 16 -> 32 (block of 49 columns, 16 slabs of rows);
`cloud9`, 9 rows at dim 2 (the block is the whole space, b = n); `wide150`, 150 x 8 -> 64 (the widest block, 97 columns: two
column tiles of the wave-per-row kernels, the largest one-workgroup problems).

The yardstick is numpy's `eigh` of the dense M = D^-1/2 P D^-1/2.  A solver that stops at residual ||M v - theta v|| <= TOL has
|theta - lambda| <= TOL (Weyl) and sin(angle(v, v_eigh)) <= TOL / gap (Davis-Kahan; gap = the eigenvalue's distance to its
neighbours); the bound on the 2-norm distance is 2 TOL / gap: chord against sine, and eigh's own rounding (~1e-15 / gap).  The
comparison means something only if no gap is tiny and the sign rule of the tail cannot flip; `preconditions` asserts both."""
import functools

import numpy as np

from diff_mining_amd import umapfit as UM
from tests import umap_cases as UC

TOL = 1e-11                   # the solver's stopping residual: SPECTRAL_TOL
MIN_GAP = 1e-5
MIN_LEAD = 1e-6
MAX_ITERS = 20
EXTRA = {"cloud1000": (1000, 16, 15, 32), "cloud9": (9, 3, 4, 2), "wide150": (150, 8, 10, 64)}     # n, d, n_neighbors, n_components
CONNECTED = [t for t in UC.SHAPES if t != "split"] + ["cloud1000"]


@functools.lru_cache(maxsize=None)
def case(tag):
    """{'n', 'dim', 'G': the float64 restatement's graph, 'val', 'vec': eigh of M, descending, 'gap': per eigenvalue}; left unchanged"""
    if tag in EXTRA:
        n, d, k, dim = EXTRA[tag]
        X = UC.cloud(n, d, n)
    else:
        X, k, dim, _ = UC.case(tag)
    n = len(X)
    idx, dist = UM.knn_host(X, k)
    G = UM.fuzzy_graph_host(idx, dist, 500, np.float64)
    out = {"X": X, "k": k, "n": n, "dim": dim, "G": G}
    P = G["P"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        isd = 1.0 / np.sqrt(P.sum(axis=1))
    if np.isfinite(isd).all():
        M = isd[:, None] * P * isd[None, :]
        val, vec = np.linalg.eigh((M + M.T) * 0.5)
        val, vec = val[::-1].copy(), vec[:, ::-1].copy()
        gap = np.minimum(np.abs(np.diff(val, prepend=np.inf)), np.abs(np.diff(val, append=-np.inf)))
        out.update(val=val, vec=vec, gap=gap)
    return out


def preconditions(tag):
    """what makes the comparison with eigh meaningful: (smallest gap among the wanted eigenvalues, smallest relative lead of an
    eigenvector's largest |entry| over the runner-up of the OTHER sign).  Only a runner-up of the other sign can flip the sign rule:
    the duplicated rows of `dup` have equal entries, so the largest one ties with its copies there, all of one sign."""
    c = case(tag)
    m = c["dim"] + 1
    v = c["vec"][:, 1:m]
    pos, neg = np.where(v > 0, v, 0.0).max(axis=0), np.where(v < 0, -v, 0.0).max(axis=0)
    lead = float((np.abs(pos - neg) / np.maximum(pos, neg)).min())
    return float(c["gap"][:m].min()), lead


def compare(tag, eigvals, eigvecs):
    """(largest |theta - lambda|, largest ||v - v_eigh||_2 / (2 TOL / gap)) over the wanted pairs; v's sign is taken from eigh's"""
    c = case(tag)
    m = c["dim"] + 1
    vec = c["vec"][:, :m]
    sign = np.where((eigvecs * vec).sum(axis=0) < 0, -1.0, 1.0)
    dist = np.linalg.norm(eigvecs * sign[None, :] - vec, axis=0)
    return float(np.abs(eigvals - c["val"][:m]).max()), float((dist / (2.0 * TOL / c["gap"][:m])).max())


def tail(tag, eigvecs, seed=UC.SEED):
    """the shared tail on a solver's own eigenvectors"""
    c = case(tag)
    noise, _ = UM.spectral_host_arrays(c["n"], c["dim"], seed)
    return UM._spectral_tail(eigvecs[:, 1:], noise)
