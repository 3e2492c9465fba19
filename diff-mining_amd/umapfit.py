"""UMAP projection for the clustering stage: `umap.UMAP(n_components=c, n_neighbors=k).fit_transform(X)` as the reference calls it
(typicality/cluster.py:312-317 with c = 5; applications/parallel-dataset/cluster.py:253-270 with c = 32, k = 15, once per country's
block of the features).  Kernels: csrc/umap.hip, csrc/umap_spectral.hip, csrc/umap_sparse.hip; C ABI: dm_umap_workspace_bytes /
dm_umap_knn / dm_umap_graph / dm_umap_layout, dm_umap_spectral_workspace_bytes / dm_umap_spectral, and the same names after
dm_umap_sparse_; csrc/umap_multi.hip: dm_umap_components, dm_umap_multi_init and their workspace functions.

Two routes, one set of rules.  `route='dense'` goes through the n x n graph and takes n < 4096 (UMAP_MAX_N).  `route='sparse'` works
from the neighbour lists alone, takes n < 65536 (UMAP_SPARSE_MAX_N) and gives the same bits wherever both run; 'auto' (the device
functions' default) is dense below 4096 rows and sparse from there.  The parallel dataset's default is 10 000 patches per fit
(cluster.py:391), which is why the sparse route exists.  Above 4095 rows umap-learn itself switches to approximate NN-descent
neighbours, unseeded; this module stays exact there, so nothing of umap-learn's is bit-comparable above the limit, and parity
stays unpinned on both routes.  Not measured: real DIFT features at 10 000 rows, whether real graphs of that size are connected (a
disconnected one takes the random initialisation, as below, unless disconnected='components' is asked for), and quality against
umap-learn.

PARITY UNPINNED.  The rules below restate umap-learn 0.5.6 (the reference's environment.yaml) at the two call sites' settings from
the paper and from memory: umap-learn was not at hand to record its outputs.  tests/make_golden_umap.py records them wherever it is
installed; until tests/golden/umap_ref.npz is committed, nothing here is checked against umap-learn itself.  The layout departs from
umap-learn on purpose (below), so the embedding is never bit-comparable; kNN, rho, sigma, the graph, a and b are meant to be.

Settings: euclidean, min_dist 0.1, spread 1, n_epochs None -> 500 (n <= 10 000), learning_rate 1, init 'spectral',
negative_sample_rate 5, set_op_mix_ratio 1, local_connectivity 1, repulsion_strength 1.  Each rule is written once in numpy here
(`*_host`) and once in the kernels:

  a, b      scipy curve_fit of 1 / (1 + a x^(2b)) to y = 1 (x < min_dist), exp(-(x - min_dist) / spread) on linspace(0, 3 spread,
            300): 1.5769, 0.8951 at the defaults.  Host only.
  kNN       exact (umap-learn's own path below 4096 rows; the sparse route stays exact above).  Squared distance = the sum over ascending
            feature index of (double(x_i) - double(x_k))^2 in fp64, multiply and add separate; distance = fp64 sqrt rounded to
            fp32; the n_neighbors smallest per row, self included, ties to the lower index.  Host and device agree bit for bit.
  smooth    rho_i = the smallest non-zero neighbour distance (0 if none).  sigma_i: 64 bisection steps at most (lo 0, hi inf, mid
            1, doubling while hi is inf) on sum_{j >= 1} (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / sigma) : 1) = log2(n_neighbors),
            stopping at |diff| < 1e-5; then the floor 1e-3 x the row's mean distance (rho_i > 0) or 1e-3 x the global mean.  The
            sum runs over j in ascending order in fp64 (umap-learn's numba loop is fp64 too); rho, sigma are stored as fp32.
  graph     membership 0 for self (by index), 1 where d - rho <= 0 or sigma = 0, else exp(-(d - rho) / sigma) rounded to fp32;
            P = (A + A^T) - A o A^T in fp32; entries below max(P) / n_epochs become 0.  Edges = the non-zeros of P in row-major
            order, ascending column; that order is the edge id.
  schedule  fp32: eps_e = max(P) / P_e, epn_e = eps_e / 5, next_e = eps_e, next_neg_e = epn_e.
  init      (host; runs once, the graph is dense below 4096 rows) eigenvectors 1..dim of I - D^-1/2 P D^-1/2 (numpy eigh), sign
            fixed so the largest-magnitude entry is positive, scaled to 10 / max|.|, plus seeded N(0, 1e-4) noise.  A disconnected
            graph or dim + 1 >= n: umap-learn's init='random', seeded uniform(-10, 10).  Either way each coordinate is then rescaled
            to [0, 10], as umap-learn does for every init.  Opt-in, disconnected='components': umap-learn's multi-component
            spectral layout instead of the random fallback -- one spectral embedding per connected component around a
            meta-embedding of the components; the rules are above `multi_component_init_host`, the device runs them in
            csrc/umap_multi.hip.  The default, 'random', is the behaviour and the bits as before.
            init_solver='device' finds the same eigenvectors from the edge list on the device instead (dm_umap_spectral; the rules
            are above `spectral_init_iter_host`); the default is the host.
  layout    SYNCHRONOUS within an epoch -- the departure.  umap-learn's numba loop updates coordinates in place from parallel
            threads, which is not reproducible even on the CPU.  Here, in epoch ep (alpha = 1 - ep / n_epochs, fp32): every read
            is of the epoch's input coordinates; vertex i walks its edges (i, j) in edge order, and for each with next_e <= ep
              1. adds 2 clip(g (y_i - y_j), +-4) alpha, g = -2ab d^(2(b-1)) / (a d^(2b) + 1), g = 0 at d^2 = 0.  The 2 is exact:
                 the graph is symmetric, (j, i) has the same weight and schedule, and umap-learn's move_other update of (j, i)
                 moves i by the same amount;
              2. n_neg = int((ep - next_neg_e) / epn_e) repulsive moves clip(g (y_i - y_k), +-4) alpha, g = 2b / ((0.001 + d^2)
                 (a d^(2b) + 1)), k = hash(seed, ep, e, p) mod n, nothing at d^2 = 0;
              3. next_e += eps_e, next_neg_e += n_neg epn_e;
            all into one accumulator per coordinate in that order, then y_new = y + acc into the second buffer.  No atomics: the
            result is bit-reproducible.  d^2 is summed by the 64-lane halving tree the kernel's wave reduction uses.  The schedule
            and alpha are fp32 everywhere; `layout_host(dtype=)` sets the precision of coordinates, gradients and accumulator.

A GPU tensor takes the device path and a numpy array the restatement; there is no quiet fall-back between them.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from .engine import EngineError, _p, load_library as _lib

UMAP_MAX_N = 4096            # DM_UMAP_MAX_N: the dense route refuses n >= this (umap-learn switches to approximate neighbours there)
UMAP_SPARSE_MAX_N = 65536    # DM_UMAP_SPARSE_MAX_N: the sparse route refuses n >= this
ROUTES = ("auto", "dense", "sparse")
UMAP_MAX_NEIGHBORS = 64      # DM_UMAP_MAX_NEIGHBORS
UMAP_MAX_COMPONENTS = 64     # DM_UMAP_MAX_COMPONENTS
NEG_RATE = 5
SMOOTH_STEPS = 64
SMOOTH_TOL = 1e-5
MIN_K_DIST_SCALE = 1e-3
# dm_umap_* return codes (include/dm_engine.h)
ERRORS = {1: "null argument", 2: f"n >= {UMAP_MAX_N} (dense route) or {UMAP_SPARSE_MAX_N} (sparse route)", 3: "n_neighbors >= n", 4: f"n_neighbors outside [2, {UMAP_MAX_NEIGHBORS}]",
          5: f"n_components outside [1, {UMAP_MAX_COMPONENTS}]", 6: "d < 1", 7: "bad epoch range", 8: "workspace too small",
          9: "bad edge count", 10: "HIP error", 11: "component count outside [1, min(n, 1024)]"}


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def pick_route(route: str, n: int) -> str:
    """'dense' or 'sparse': 'auto' is dense below UMAP_MAX_N rows (the behaviour before the sparse route existed) and sparse from there"""
    if route not in ROUTES:
        raise ValueError(f"umap: route {route!r} is not one of {ROUTES}")
    return ("dense" if n < UMAP_MAX_N else "sparse") if route == "auto" else route


def _check(n, d, k, dim=1, route="dense"):
    if route not in ("dense", "sparse"):
        raise ValueError(f"umap: route {route!r} is not 'dense' or 'sparse'")
    if route == "dense" and n >= UMAP_MAX_N:
        raise ValueError(f"umap: n {n} >= {UMAP_MAX_N} (exact neighbours only)")
    if n >= UMAP_SPARSE_MAX_N:
        raise ValueError(f"umap: n {n} >= {UMAP_SPARSE_MAX_N}")
    if k < 2 or k > UMAP_MAX_NEIGHBORS:
        raise ValueError(f"umap: n_neighbors {k} outside [2, {UMAP_MAX_NEIGHBORS}]")
    if k >= n:
        raise ValueError(f"umap: n_neighbors {k} >= n {n}")
    if dim < 1 or dim > UMAP_MAX_COMPONENTS:
        raise ValueError(f"umap: n_components {dim} outside [1, {UMAP_MAX_COMPONENTS}]")
    if d < 1:
        raise ValueError("umap: d < 1")


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement: the CPU-tier yardstick, and what runs on a numpy array
# ------------------------------------------------------------------------------------------------------------------------------
def find_ab_params(spread: float = 1.0, min_dist: float = 0.1):
    from scipy.optimize import curve_fit

    def curve(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    xv = np.linspace(0, spread * 3, 300)
    yv = np.zeros(xv.shape)
    yv[xv < min_dist] = 1.0
    yv[xv >= min_dist] = np.exp(-(xv[xv >= min_dist] - min_dist) / spread)
    params, _ = curve_fit(curve, xv, yv)
    return float(params[0]), float(params[1])


KNN_HOST_BLOCK = 256         # rows per block of the sparse route's restatement


def knn_host(X, n_neighbors: int = 15, route: str = "dense"):
    """(idx int32 [n, k], dist fp32 [n, k]) by the kNN rule at the top of this module.  route 'sparse': the same per-feature fp64
    passes on blocks of KNN_HOST_BLOCK rows, so n x n is never formed; the same bits."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    _check(n, d, n_neighbors, route=route)
    Xd = X.astype(np.float64)
    if route == "sparse":
        idx = np.empty((n, n_neighbors), np.int32)
        dist = np.empty((n, n_neighbors), np.float32)
        for i0 in range(0, n, KNN_HOST_BLOCK):
            rows = slice(i0, min(n, i0 + KNN_HOST_BLOCK))
            sq = np.zeros((rows.stop - i0, n), dtype=np.float64)
            t = np.empty_like(sq)
            for e in range(d):
                np.subtract(Xd[rows, e][:, None], Xd[None, :, e], out=t)
                np.multiply(t, t, out=t)
                sq += t
            db = np.sqrt(sq).astype(np.float32)
            ib = np.argsort(db, axis=1, kind="stable")[:, :n_neighbors]
            idx[rows] = ib
            dist[rows] = np.take_along_axis(db, ib, axis=1)
        return idx, dist
    sq = np.zeros((n, n), dtype=np.float64)
    t = np.empty((n, n), dtype=np.float64)
    for e in range(d):                                   # ascending feature index, multiply and add separate
        col = Xd[:, e]
        np.subtract(col[:, None], col[None, :], out=t)
        np.multiply(t, t, out=t)
        sq += t
    dist = np.sqrt(sq).astype(np.float32)
    idx = np.argsort(dist, axis=1, kind="stable")[:, :n_neighbors].astype(np.int32)
    return idx, np.take_along_axis(dist, idx, axis=1)


def _smooth_host(dist, dtype):
    """rho, sigma (fp32 [n]) and the flag of rows where the floor or the step cap decided sigma."""
    n, k = dist.shape
    f = np.dtype(dtype).type
    target = f(np.log2(k))
    big = np.where(dist > 0, dist, np.float32(np.inf)).min(axis=1)
    rho = np.where(np.isfinite(big), big, np.float32(0)).astype(np.float32)
    x = dist.astype(dtype) - rho.astype(dtype)[:, None]
    lo = np.zeros(n, dtype)
    hi = np.full(n, np.inf, dtype)
    mid = np.ones(n, dtype)
    live = np.ones(n, bool)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for _ in range(SMOOTH_STEPS):
            psum = np.zeros(n, dtype)
            for j in range(1, k):
                psum = psum + np.where(x[:, j] > 0, np.exp(-(x[:, j] / mid)), f(1))
            live &= ~(np.abs(psum - target) < f(SMOOTH_TOL))
            if not live.any():
                break
            over = psum > target
            new_hi = np.where(over, mid, hi)
            new_lo = np.where(over, lo, mid)
            new_mid = np.where(over, (lo + mid) / f(2), np.where(np.isinf(hi), mid * f(2), (mid + hi) / f(2)))
            hi, lo, mid = np.where(live, new_hi, hi), np.where(live, new_lo, lo), np.where(live, new_mid, mid)
    d64 = dist.astype(np.float64)
    row_sum = np.zeros(n, np.float64)
    for j in range(k):
        row_sum = row_sum + d64[:, j]
    floor = np.where(rho > 0, MIN_K_DIST_SCALE * (row_sum / k), MIN_K_DIST_SCALE * (row_sum.sum() / (n * k)))
    floored = mid.astype(np.float64) < floor
    sigma = np.where(floored, floor, mid.astype(np.float64)).astype(np.float32)
    return rho, sigma, floored | live


def fuzzy_graph_host(idx, dist, n_epochs: int = 500, dtype=np.float64, route: str = "dense"):
    """The fuzzy simplicial set from the kNN arrays.  dtype: the precision of the bisection and of exp (float64 is the rule; float32
    is there to measure what fp32 costs).  Returns a dict: rho, sigma (fp32 [n]), exempt (bool [n]: floor or step cap decided sigma),
    P (fp32 [n, n], pruned; route 'dense' only), threshold, row_ptr (int32 [n + 1]), col (int32 [E]), weight (fp32 [E]).  route
    'sparse' takes the union on the lists (an edge's two memberships are looked up by the key row n + column) and has no P; the
    rest is the same bits."""
    if route not in ("dense", "sparse"):
        raise ValueError(f"umap: route {route!r} is not 'dense' or 'sparse'")
    idx = np.asarray(idx)
    dist = np.asarray(dist, dtype=np.float32)
    n, k = dist.shape
    rho, sigma, exempt = _smooth_host(dist, dtype)
    x = dist.astype(dtype) - rho.astype(dtype)[:, None]
    s = sigma.astype(dtype)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        val = np.where((x <= 0) | (s == 0), np.dtype(dtype).type(1), np.exp(-(x / s))).astype(np.float32)
    val[idx == np.arange(n)[:, None]] = 0
    if route == "sparse":
        rows = np.repeat(np.arange(n, dtype=np.int64), k)
        cols = idx.astype(np.int64).ravel()
        ok = (cols >= 0) & (cols < n) & (cols != rows)
        rows, cols, a = rows[ok], cols[ok], val.ravel()[ok]
        out_key, in_key = rows * n + cols, cols * n + rows
        keys = np.unique(np.concatenate([out_key, in_key]))            # ascending: row-major, ascending column
        a_ij = np.zeros(len(keys), np.float32)
        a_ji = np.zeros(len(keys), np.float32)
        a_ij[np.searchsorted(keys, out_key)] = a
        a_ji[np.searchsorted(keys, in_key)] = a
        p = (a_ij + a_ji) - a_ij * a_ji
        thr = np.float32(p.max(initial=np.float32(0)) / np.float32(n_epochs))
        keep = ~(p < thr) & (p != 0)
        keys, p = keys[keep], p[keep]
        row_ptr = np.zeros(n + 1, np.int32)
        row_ptr[1:] = np.cumsum(np.bincount(keys // n, minlength=n))
        return {"rho": rho, "sigma": sigma, "exempt": exempt, "threshold": thr, "row_ptr": row_ptr, "col": (keys % n).astype(np.int32),
                "weight": p}
    A = np.zeros((n, n), np.float32)
    np.put_along_axis(A, idx.astype(np.int64), val, axis=1)
    P = (A + A.T) - A * A.T
    thr = np.float32(P.max() / np.float32(n_epochs))
    P[P < thr] = 0
    rows, cols = np.nonzero(P)                                 # row-major, ascending column
    row_ptr = np.zeros(n + 1, np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return {"rho": rho, "sigma": sigma, "exempt": exempt, "P": P, "threshold": thr, "row_ptr": row_ptr, "col": cols.astype(np.int32),
            "weight": P[rows, cols]}


def schedule_host(weight):
    """(eps, epn, next, next_neg), fp32 [E]"""
    weight = np.asarray(weight, np.float32)
    eps = (weight.max() if len(weight) else np.float32(1)) / weight
    epn = eps / np.float32(NEG_RATE)
    return eps, epn, eps.copy(), epn.copy()


def _rescale(Y):
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    return (10.0 * (Y - lo) / (hi - lo)).astype(np.float32)


def spectral_init_host(P, dim: int, seed: int = 42):
    """(Y0 fp32 [n, dim], 'spectral' | 'random') from the dense graph, by the init rule at the top of this module."""
    from scipy.sparse.csgraph import connected_components
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[0]
    rs = np.random.RandomState(seed)
    n_comp = connected_components(P > 0, directed=False)[0] if n else 0
    if n_comp != 1 or dim + 1 >= n:
        return _rescale(rs.uniform(low=-10.0, high=10.0, size=(n, dim))), "random"
    _, vec = _laplacian_eigh(P)
    return _spectral_tail(vec[:, 1:dim + 1], rs.normal(scale=0.0001, size=(n, dim)).astype(np.float32)), "spectral"


def _laplacian_eigh(P):
    """numpy's eigh of I - D^-1/2 P D^-1/2, P dense float64: (eigenvalues ascending, eigenvectors)"""
    n = P.shape[0]
    isd = 1.0 / np.sqrt(P.sum(axis=1))
    L = np.eye(n) - isd[:, None] * P * isd[None, :]
    L = (L + L.T) * 0.5
    return np.linalg.eigh(L)


def spectral_init_sparse_host(row_ptr, col, weight, n: int, dim: int, seed: int = 42, dense_below: int = UMAP_MAX_N):
    """(Y0 fp32 [n, dim], 'spectral' | 'random', info) from the edge list, by the init rule at the top of this module.  Below
    `dense_below` rows the rule's own solver still fits -- numpy's eigh of the dense Laplacian, `spectral_init_host`'s, the same bits --
    and from there the dense matrix is never formed: scipy's `eigsh` (ARPACK, largest algebraic, started from the all-ones vector so
    that it is reproducible) on the sparse M = D^-1/2 P D^-1/2, whose top eigenvectors are the Laplacian's bottom ones.  Then
    `_spectral_tail`.  dense_below = 0 takes eigsh at any size.  info: 'n_comp', 'solver' ('eigh' | 'eigsh'), and after a solve
    'eigvals' (float64 [dim + 1], of M, descending) and 'eigvecs' (float64 [n, dim + 1])."""
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)[:row_ptr[-1]]
    w = np.asarray(weight, np.float32)[:row_ptr[-1]].astype(np.float64)
    rs = np.random.RandomState(seed)
    P = sparse.csr_matrix((w, col, row_ptr), shape=(n, n))
    n_comp = connected_components(P, directed=False)[0] if n else 0
    info = {"n_comp": int(n_comp), "solver": None}
    if n_comp != 1 or dim + 1 >= n:
        return _rescale(rs.uniform(low=-10.0, high=10.0, size=(n, dim))), "random", info
    m = dim + 1
    if n < dense_below or m + 1 >= n:                       # ARPACK takes fewer than n - 1 pairs
        val, vec = _laplacian_eigh(P.toarray())
        info.update(solver="eigh", eigvals=1.0 - val[:m], eigvecs=vec[:, :m].copy())
    else:
        from scipy.sparse.linalg import eigsh
        isd = 1.0 / np.sqrt(np.asarray(P.sum(axis=1)).ravel())
        M = sparse.diags(isd) @ P @ sparse.diags(isd)
        val, vec = eigsh(((M + M.T) * 0.5).tocsr(), k=m, which="LA", v0=np.ones(n), tol=0, ncv=min(n, max(2 * m + 1, 40)))
        order = np.argsort(-val, kind="stable")
        info.update(solver="eigsh", eigvals=val[order].copy(), eigvecs=vec[:, order].copy())
    return _spectral_tail(info["eigvecs"][:, 1:], rs.normal(scale=0.0001, size=(n, dim)).astype(np.float32)), "spectral", info


def _spectral_tail(vec, noise):
    """The end of the spectral initialisation, shared by both solvers: eigenvectors 1..dim (float64 [n, dim]) -> Y0 fp32 [n, dim].
    Sign by the largest-magnitude entry, 10 / max|.|, the fp32 cast, the noise (fp32 [n, dim]), the rescale to [0, 10]."""
    return _init_tail(_fix_signs(vec), noise)


def _fix_signs(vec):
    """float64 copy of `vec` with every column's largest-magnitude entry (the first on a tie) made positive"""
    Y = np.array(vec, dtype=np.float64)
    top = np.abs(Y).argmax(axis=0)
    Y *= np.sign(Y[top, np.arange(Y.shape[1])])[None, :]
    return Y


def _init_tail(R, noise):
    """The last steps of every non-random initialisation: float64 [n, dim] -> 10 / max|.|, the fp32 cast, the noise, the rescale."""
    return _rescale((R * (10.0 / np.abs(R).max())).astype(np.float32) + noise)


# ---- the iterative solver of the spectral initialisation: what csrc/umap_spectral.hip runs, stated in numpy --------------------------
# The dim + 1 top eigenvectors of M = D^-1/2 P D^-1/2 (the bottom ones of the Laplacian above) from the edge list alone, by
# Chebyshev-filtered subspace iteration on a block of b = min(n, m + max(8, m // 2)) columns, m = dim + 1:
#   matrix   deg_i = the sum of row i's weights in edge order (fp64), isd = 1 / sqrt(deg); (M X)_i = isd_i sum_e (w_e isd_col_e) X_col_e,
#            edges in edge order.
#   start    column 0 = sqrt(deg) (the top eigenvector, eigenvalue 1), column c > 0 of row i = hash(seed, SPECTRAL_HASH_EP, i, c) / 2^32 - 1/2.
#   filter   the Chebyshev polynomial that damps [-1, cut]: cut = 0 at first, then the smallest Ritz value of the iteration before
#            (not below -0.99).  Degree 16, lowered until T_deg at eigenvalue 1 is <= SPECTRAL_GROWTH: the filtered block's condition number
#            is about that value, and Cholesky-QR applied twice orthonormalises a block only while it stays well below u^-1/2 = 6.7e7
#            (at degree 16 and cut = 0 it is T_16(3) = 9e11 on a graph whose spectrum is spread: the first Cholesky factorisation then
#            fails on tests/umap_cases.py's n130, for one).
#   ortho    Cholesky-QR twice: G = X^T X, R = chol(G)^T, X <- X R^-1.
#   Ritz     H = Q^T (M Q), symmetrised; cyclic Jacobi in the round-robin order of `_jacobi_rounds` until a sweep rotates nothing;
#            Ritz values in descending order (ties: the lower column first); Q and M Q are rotated.
#   stop     every wanted pair has ||M v - theta v||_2 <= SPECTRAL_TOL; at most SPECTRAL_MAX_OUTER iterations.
SPECTRAL_DEGREE = 16
SPECTRAL_GROWTH = 1e6
SPECTRAL_TOL = 1e-11
SPECTRAL_MAX_OUTER = 40
SPECTRAL_SWEEPS = 30
SPECTRAL_MIN_CUT = -0.99
SPECTRAL_HASH_EP = 0x5EED


def spectral_block(n: int, dim: int) -> int:
    m = dim + 1
    return min(n, m + max(8, m // 2))


def components_host(row_ptr, col, n: int) -> int:
    """The number of connected components, by min-label propagation over the edge list."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    head = np.repeat(np.arange(n), np.diff(row_ptr))
    label = np.arange(n)
    while True:
        new = label.copy()
        np.minimum.at(new, head, label[col])
        if np.array_equal(new, label):
            return int(np.sum(label == np.arange(n)))
        label = new


def _csr_apply(row_ptr, coef, col, X):
    """out_i = sum over row i's edges e, in edge order, of coef_e X[col_e] (float64)"""
    n = len(row_ptr) - 1
    cnt = np.diff(row_ptr)
    out = np.zeros((n, X.shape[1]), np.float64)
    for r in range(int(cnt.max()) if n else 0):
        rows = np.flatnonzero(cnt > r)
        e = row_ptr[rows] + r
        out[rows] = out[rows] + coef[e, None] * X[col[e]]
    return out


def _cheb_degree(cut: float) -> int:
    c, e = (cut - 1.0) / 2.0, (cut + 1.0) / 2.0
    x = (1.0 - c) / e
    t0, t1, deg = 1.0, x, 1
    while deg < SPECTRAL_DEGREE:
        t2 = 2.0 * x * t1 - t0
        if not t2 <= SPECTRAL_GROWTH:
            break
        t0, t1, deg = t1, t2, deg + 1
    return deg


def _jacobi_rounds(b: int):
    """The fixed sweep order: the round-robin tournament of b players (one dummy if b is odd), P - 1 rounds of disjoint pairs (p < q)."""
    P = b + (b & 1)
    rounds = []
    for s in range(P - 1):
        k = np.arange(1, P // 2)
        x = np.concatenate([[P - 1], (s + k) % (P - 1)])
        y = np.concatenate([[s], (s - k) % (P - 1)])
        p, q = np.minimum(x, y), np.maximum(x, y)
        keep = q < b
        rounds.append((p[keep], q[keep]))
    return rounds


def _jacobi_host(H):
    """(theta descending, W, sweeps): H W = W diag(theta) by cyclic Jacobi in the order of `_jacobi_rounds`."""
    H = np.array(H, dtype=np.float64)
    b = len(H)
    W = np.eye(b)
    rounds = _jacobi_rounds(b)
    sweeps = 0
    for sweeps in range(1, SPECTRAL_SWEEPS + 1):
        rotated = False
        for p, q in rounds:
            hpp, hqq, hpq = H[p, p], H[q, q], H[p, q]
            act = np.abs(hpq) > 1e-20 * (np.abs(hpp) + np.abs(hqq))
            if not act.any():
                continue
            rotated = True
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                tau = (hqq - hpp) / (2.0 * hpq)
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
            c, s = np.where(act, c, 1.0), np.where(act, s, 0.0)
            for A in (H, W):                                   # columns: A <- A J
                ap, aq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * ap - s * aq, s * ap + c * aq
            hp, hq = H[p, :].copy(), H[q, :].copy()            # rows: H <- J^T H
            H[p, :], H[q, :] = c[:, None] * hp - s[:, None] * hq, s[:, None] * hp + c[:, None] * hq
        if not rotated:
            break
    theta = np.diag(H).copy()
    order = np.argsort(-theta, kind="stable")
    return theta[order], W[:, order], sweeps


def spectral_init_iter_host(row_ptr, col, weight, n: int, dim: int, seed: int = 42):
    """(Y0 fp32 [n, dim], 'spectral' | 'random', info) from the edge list, by the rules above.  info: 'status' ('converged',
    'not_converged' -- the caller takes `spectral_init_host` -- or 'random'), 'n_comp', 'iters', 'max_residual', 'degrees' (the
    filter's, per iteration), and after a solve 'eigvals' (float64 [dim + 1], of M, descending) and 'eigvecs' (float64 [n, dim + 1])."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)[:row_ptr[-1]]
    w = np.asarray(weight, np.float32)[:row_ptr[-1]].astype(np.float64)
    rs = np.random.RandomState(seed)
    n_comp = components_host(row_ptr, col, n) if n else 0
    info = {"status": "random", "n_comp": n_comp, "iters": 0, "max_residual": float("nan"), "degrees": []}
    if n_comp != 1 or dim + 1 >= n:
        return _rescale(rs.uniform(low=-10.0, high=10.0, size=(n, dim))), "random", info
    m, b = dim + 1, spectral_block(n, dim)
    deg = _csr_apply(row_ptr, w, col, np.ones((n, 1)))[:, 0]
    isd = 1.0 / np.sqrt(deg)
    coef = w * isd[col]

    def mul(X):
        return isd[:, None] * _csr_apply(row_ptr, coef, col, X)

    X = hash_host(seed, SPECTRAL_HASH_EP, np.arange(n)[:, None], np.arange(b, dtype=np.uint64)[None, :]).astype(np.float64) / 2.0 ** 32 - 0.5
    X[:, 0] = np.sqrt(deg)
    cut = 0.0
    info["status"] = "not_converged"
    with np.errstate(all="ignore"):
        for it in range(1, SPECTRAL_MAX_OUTER + 1):
            d = _cheb_degree(cut)
            info["degrees"].append(d)
            c, e = (cut - 1.0) / 2.0, (cut + 1.0) / 2.0
            Y0, Y1 = X, (mul(X) - c * X) / e
            for _ in range(2, d + 1):
                Y0, Y1 = Y1, 2.0 * (mul(Y1) - c * Y1) / e - Y0
            Q = Y1
            try:
                for _ in range(2):                              # Cholesky-QR, twice
                    R = np.linalg.cholesky(Q.T @ Q).T
                    Q = Q @ np.linalg.inv(R)
            except np.linalg.LinAlgError:
                break
            MQ = mul(Q)
            H = Q.T @ MQ
            theta, W, _ = _jacobi_host(0.5 * (H + H.T))
            X, MX = Q @ W, MQ @ W
            res = np.sqrt(((MX[:, :m] - theta[None, :m] * X[:, :m]) ** 2).sum(axis=0))
            info.update(iters=it, max_residual=float(res.max()), eigvals=theta[:m].copy(), eigvecs=X[:, :m].copy())
            if res.max() <= SPECTRAL_TOL:
                info["status"] = "converged"
                break
            cut = max(float(theta[-1]), SPECTRAL_MIN_CUT)
    noise = rs.normal(scale=0.0001, size=(n, dim)).astype(np.float32)
    if "eigvecs" not in info:
        info.update(eigvals=np.full(m, np.nan), eigvecs=np.full((n, m), np.nan))
    return _spectral_tail(info["eigvecs"][:, 1:], noise), "spectral", info


# ---- a disconnected graph: one spectral embedding per component (opt-in: disconnected='components') -----------------------------------
# PARITY UNPINNED, like the rest of this module: umap-learn 0.5.6's `multi_component_layout` / `component_layout`, restated from
# memory.  Deliberate departures are marked (+).  What csrc/umap_multi.hip runs, stated in numpy:
#   components  labels by min-label propagation; ids 0 .. c - 1 ascend with each component's smallest vertex (scipy's
#               connected_components order).  c = 1: the spectral initialisation as before; dim + 1 >= n: the random one as before;
#               c > MULTI_MAX_COMP: the random one (+: a cap on the host eigh of the meta-embedding; a k-NN component holds at least k
#               rows, so 10 000 rows at k = 15 cannot reach it).
#   grouping    vertices grouped by component, ascending index inside (the stable permutation); each component's sub-graph keeps that
#               order, so the column renumbering is monotone and every row's edge order survives.
#   centroids   only when c > 2 dim: the fp64 sum of double(X[i]) over the component's rows in ascending row index, separate adds,
#               divided by the size.
#   meta        `meta_embedding_host`.  c <= 2 dim: the table vstack([I_k | 0], -[I_k | 0])[:c], k = ceil(c / 2).  Otherwise the
#               spectral embedding of A = exp(-|cent_l - cent_m|^2) (zero diagonal): eigenvectors 1 .. dim of I - D^-1/2 A D^-1/2,
#               rows divided by sqrt(deg) (scikit-learn SpectralEmbedding's recovery), sign by each column's largest-magnitude entry
#               (+: scikit-learn's flip rule differs), the whole divided by its largest entry.  Degenerate -- a zero row sum of A, a
#               disconnected A > 0, or two coinciding meta rows -- means the random initialisation with the reason 'meta degenerate'
#               (+: umap-learn has no defined behaviour once exp(-d^2) underflows).
#   range       range_l = half the smallest positive distance from meta[l] to another meta row.
#   component   size < 2 dim or size <= dim + 1: R[i] = meta[l] + range_l unit[i], unit = RandomState(seed).uniform(-1, 1, (n, dim))
#               drawn up front and indexed by the vertex's own row (+: umap-learn draws per component in sequence; here the draw does
#               not depend on the graph, so the device takes it as an upload).  Otherwise E = eigenvectors 1 .. dim of the component's
#               own normalised Laplacian, signs as `_spectral_tail`, R[i] = E[i] (range_l / max|E|) + meta[l].
#   tail        `_init_tail`: Y0 = _rescale(fp32(R (10 / max|R|)) + noise), the noise of the spectral initialisation.
MULTI_MAX_COMP = 1024        # DM_UMAP_MULTI_MAX_COMP
DISCONNECTED = ("random", "components")
MULTI_SOLVERS = ("host", "iter")


def component_labels_host(row_ptr, col, n: int):
    """int64 [n]: every vertex's smallest reachable vertex, by the min-label propagation of `components_host`"""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)[:row_ptr[-1]]
    head = np.repeat(np.arange(n), np.diff(row_ptr))
    label = np.arange(n)
    while True:
        new = label.copy()
        np.minimum.at(new, head, label[col])
        if np.array_equal(new, label):
            return label
        label = new


def component_groups_host(row_ptr, col, weight, n: int, X=None):
    """The components step of the rule above, as dm_umap_components lays it out.  A dict: 'comp' int32 [n], 'n_comp', 'offsets' int32
    [c + 1], 'perm' int32 [n] (the vertex at each grouped position), 'edge_offsets' int32 [c + 1], 'sub_row_ptr' int32 [n + c]
    (component l's own row pointer, size_l + 1 entries from index offsets[l] + l, starting at 0), 'sub_col' (positions inside the
    component), 'sub_weight', and with X 'centroids' float64 [c, d]."""
    row_ptr = np.asarray(row_ptr, np.int64)
    E = int(row_ptr[-1])
    col = np.asarray(col, np.int64)[:E]
    weight = np.asarray(weight, np.float32)[:E]
    label = component_labels_host(row_ptr, col, n)
    roots = np.flatnonzero(label == np.arange(n))                     # ascending: the order of the ids
    c = len(roots)
    rank = np.zeros(n, np.int64)
    rank[roots] = np.arange(c)
    comp = rank[label]
    perm = np.argsort(comp, kind="stable")
    offsets = np.zeros(c + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(comp, minlength=c))
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    head = np.repeat(np.arange(n), np.diff(row_ptr))
    keep = comp[col] == comp[head]                                    # all of them on a symmetric list
    e_order = np.argsort(inv[head], kind="stable")                    # edges by grouped row, each row's order kept
    e_order = e_order[keep[e_order]]
    g_head = inv[head[e_order]]
    sub_col = inv[col[e_order]] - offsets[comp[col[e_order]]]
    gp = np.zeros(n + 1, np.int64)
    gp[1:] = np.cumsum(np.bincount(g_head, minlength=n))
    edge_offsets = gp[offsets]
    sub_row_ptr = np.zeros(n + c, np.int64)
    for l in range(c):
        lo, hi = offsets[l], offsets[l + 1]
        sub_row_ptr[lo + l:hi + l + 1] = gp[lo:hi + 1] - gp[lo]
    out = {"comp": comp.astype(np.int32), "n_comp": c, "offsets": offsets.astype(np.int32), "perm": perm.astype(np.int32),
           "edge_offsets": edge_offsets.astype(np.int32), "sub_row_ptr": sub_row_ptr.astype(np.int32), "sub_col": sub_col.astype(np.int32),
           "sub_weight": weight[e_order].copy()}
    if X is not None:
        Xd = np.ascontiguousarray(X, dtype=np.float32).astype(np.float64)
        cent = np.zeros((c, Xd.shape[1]), np.float64)
        for l in range(c):
            s = np.zeros(Xd.shape[1], np.float64)
            for i in perm[offsets[l]:offsets[l + 1]]:                 # ascending row index, one add per row
                s = s + Xd[i]
            cent[l] = s / float(offsets[l + 1] - offsets[l])
        out["centroids"] = cent
    return out


def sub_graph(groups, l: int):
    """(row_ptr, col, weight, size) of component l from `component_groups_host`'s (or, brought to the host, `components`') dict"""
    off, end = int(groups["offsets"][l]), int(groups["offsets"][l + 1])
    e0, e1 = int(groups["edge_offsets"][l]), int(groups["edge_offsets"][l + 1])
    return groups["sub_row_ptr"][off + l:end + l + 1], groups["sub_col"][e0:e1], groups["sub_weight"][e0:e1], end - off


def meta_embedding_host(cent, c: int, dim: int):
    """Where the components go, by the rule above: a dict with 'meta' float64 [c, dim], 'range' float64 [c], 'kind' ('table' |
    'affinity') and 'reason' (None, or 'meta degenerate' with 'detail': 'zero row sum' | 'disconnected' | 'coincident rows'; then
    there is no 'meta').  cent: float64 [c, d], read only when c > 2 dim."""
    out = {"kind": "table" if c <= 2 * dim else "affinity", "reason": None, "detail": None}

    def degenerate(detail):
        out.update(reason="meta degenerate", detail=detail)
        return out

    if c <= 2 * dim:
        k = (c + 1) // 2
        base = np.hstack([np.eye(k), np.zeros((k, dim - k))])
        meta = np.vstack([base, -base])[:c]
    else:
        from scipy.sparse.csgraph import connected_components
        cent = np.asarray(cent, np.float64)[:c]
        diff = cent[:, None, :] - cent[None, :, :]
        A = np.exp(-(diff * diff).sum(axis=2))
        np.fill_diagonal(A, 0.0)
        deg = A.sum(axis=1)
        if not np.all(deg > 0):
            return degenerate("zero row sum")
        if connected_components(A > 0, directed=False)[0] != 1:
            return degenerate("disconnected")
        isd = 1.0 / np.sqrt(deg)
        L = np.eye(c) - isd[:, None] * A * isd[None, :]
        _, vec = np.linalg.eigh((L + L.T) * 0.5)
        meta = _fix_signs(vec[:, 1:dim + 1] * isd[:, None])
        meta = meta / meta.max()
        if not np.all(np.isfinite(meta)):
            return degenerate("coincident rows")
    rng = meta_range_host(meta)
    if rng is None:
        return degenerate("coincident rows")
    out.update(meta=meta, range=rng)
    return out


def meta_range_host(meta):
    """float64 [c]: half the smallest positive Euclidean distance from each meta row to another; None if two rows coincide"""
    meta = np.asarray(meta, np.float64)
    c = len(meta)
    dist = np.sqrt(((meta[:, None, :] - meta[None, :, :]) ** 2).sum(axis=2))
    dist[np.arange(c), np.arange(c)] = np.inf
    if not np.all(dist > 0):
        return None
    return dist.min(axis=1) / 2.0


def multi_component_plan(sizes, dim: int):
    """int32 [c]: 1 where a component gets its own spectral embedding, 0 where it is placed uniformly around its meta row"""
    sizes = np.asarray(sizes)
    return (~((sizes < 2 * dim) | (sizes <= dim + 1))).astype(np.int32)


def multi_host_arrays(n: int, dim: int, seed: int = 42):
    """unit float64 [n, dim]: the uniform(-1, 1) draw of the uniformly placed components, by the vertex's own row"""
    return np.random.RandomState(seed).uniform(low=-1.0, high=1.0, size=(n, dim))


def place_components_host(groups, meta, plan, eigvecs, dim: int, seed: int = 42):
    """Steps 5 and 6 of the rule above from given eigenvectors (float64 [n, dim + 1], rows in grouped order; read where plan is 1):
    (Y0 fp32 [n, dim], R float64 [n, dim]).  The device's eigenvectors go through this in the GPU tests."""
    offsets, perm = np.asarray(groups["offsets"], np.int64), np.asarray(groups["perm"], np.int64)
    n = len(perm)
    unit = multi_host_arrays(n, dim, seed)
    R = np.zeros((n, dim), np.float64)
    for l in range(len(offsets) - 1):
        rows = perm[offsets[l]:offsets[l + 1]]
        if plan[l]:
            E = _fix_signs(np.asarray(eigvecs, np.float64)[offsets[l]:offsets[l + 1], 1:dim + 1])
            R[rows] = E * (meta["range"][l] / np.abs(E).max()) + meta["meta"][l]
        else:
            R[rows] = meta["meta"][l] + meta["range"][l] * unit[rows]
    noise = np.random.RandomState(seed).normal(scale=0.0001, size=(n, dim)).astype(np.float32)
    return _init_tail(R, noise), R


def multi_component_init_host(row_ptr, col, weight, X, dim: int, seed: int = 42, solver: str = "host", dense_below: int = UMAP_MAX_N):
    """(Y0 fp32 [n, dim], 'components' | 'spectral' | 'random', info) from the edge list and X fp32 [n, d], by the rule above.
    PARITY UNPINNED (a restatement of umap-learn's multi_component_layout from memory; the departures are marked there).
    solver 'host': per component the eigh / eigsh choice `spectral_init_sparse_host` makes at that component's size; 'iter':
    `spectral_init_iter_host` per component, which is what the device runs.  One component, or dim + 1 >= n, is today's function of
    that solver, bit for bit; so is every fallback ('reason' says why: 'more than 1024 components' | 'meta degenerate').  info:
    'n_comp', 'sizes', 'plan' (1 solved / 0 uniform), 'meta_kind', 'reason', 'iters' and 'status' per component, 'groups', 'meta',
    'R', 'eigvecs' (float64 [n, dim + 1], grouped order) and 'eigvals' (float64 [c, dim + 1])."""
    if solver not in MULTI_SOLVERS:
        raise ValueError(f"multi_component_init_host: solver {solver!r} is not one of {MULTI_SOLVERS}")
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    row_ptr = np.asarray(row_ptr, np.int64)
    E = int(row_ptr[-1])
    col, weight = np.asarray(col)[:E], np.asarray(weight, np.float32)[:E]

    def single(rp, cl, w, rows):
        if solver == "iter":
            return spectral_init_iter_host(rp, cl, w, rows, dim, seed)
        return spectral_init_sparse_host(rp, cl, w, rows, dim, seed, dense_below)

    n_comp = components_host(row_ptr, col, n) if n else 0
    info = {"n_comp": int(n_comp), "sizes": None, "plan": None, "meta_kind": None, "reason": None, "iters": [], "status": []}
    if n_comp == 1 or dim + 1 >= n or n_comp > MULTI_MAX_COMP:
        Y0, used, inner = single(row_ptr, col, weight, n)
        info.update(inner=inner, reason=None if n_comp == 1 else "n_components + 1 >= n" if dim + 1 >= n else f"more than {MULTI_MAX_COMP} components")
        return Y0, used, info
    groups = component_groups_host(row_ptr, col, weight, n, X if n_comp > 2 * dim else None)
    sizes = np.diff(groups["offsets"])
    meta = meta_embedding_host(groups.get("centroids"), n_comp, dim)
    info.update(sizes=sizes, meta_kind=meta["kind"], groups=groups, meta=meta)
    if meta["reason"]:
        info.update(reason=meta["reason"], detail=meta["detail"])
        return _rescale(np.random.RandomState(seed).uniform(low=-10.0, high=10.0, size=(n, dim))), "random", info
    plan = multi_component_plan(sizes, dim)
    vecs, vals = np.zeros((n, dim + 1), np.float64), np.zeros((n_comp, dim + 1), np.float64)
    for l in range(n_comp):
        if not plan[l]:
            info["iters"].append(0)
            info["status"].append("uniform")
            continue
        rp, cl, w, rows = sub_graph(groups, l)
        _, _, inner = single(rp, cl, w, rows)
        vecs[groups["offsets"][l]:groups["offsets"][l + 1]] = inner["eigvecs"]
        vals[l] = inner["eigvals"]
        info["iters"].append(int(inner.get("iters", 0)))
        info["status"].append(inner.get("status", "converged"))
    Y0, R = place_components_host(groups, meta, plan, vecs, dim, seed)
    info.update(plan=plan, R=R, eigvecs=vecs, eigvals=vals)
    return Y0, "components", info


_M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & _M32
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & _M32
    return h ^ (h >> np.uint64(16))


def hash_host(seed, ep, e, p):
    """The layout's counter-based 32-bit mix (umap_hash in csrc/umap.hip): uint64 arrays holding 32-bit values."""
    e = np.asarray(e).astype(np.uint64)
    h = _mix32(np.uint64(int(seed) & 0x7FFFFFFF) ^ ((np.uint64(ep) * np.uint64(0x9E3779B9)) & _M32))
    h = _mix32(h ^ ((e * np.uint64(0x85EBCA6B)) & _M32))
    return _mix32(h ^ ((np.uint64(p) * np.uint64(0xC2B2AE35)) & _M32))


def _d2_tree(diff):
    """sum of squares over the coordinates by the kernel's tree: 64 lanes, halved six times"""
    m, dim = diff.shape
    v = np.zeros((m, 64), diff.dtype)
    v[:, :dim] = diff * diff
    w = 32
    while w:
        v = v[:, :w] + v[:, w:2 * w]
        w >>= 1
    return v[:, 0]


def layout_host(row_ptr, col, weight, Y0, a, b, n_epochs: int = 500, seed: int = 42, first_epoch: int = 0, last_epoch=None,
                dtype=np.float32, schedule=None, counts=None):
    """The synchronous layout.  Returns (Y, schedule): schedule = (eps, epn, next, next_neg) to pass back in when a later call goes
    on from `last_epoch`.  counts: an int array [E] that receives each edge's number of activations."""
    f = np.dtype(dtype).type
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(row_ptr) - 1
    Y = np.asarray(Y0).astype(dtype).copy()
    dim = Y.shape[1]
    last_epoch = n_epochs if last_epoch is None else last_epoch
    eps, epn, nxt, nneg = schedule if schedule is not None else schedule_host(weight)
    nxt, nneg = nxt.copy(), nneg.copy()
    a32, b32 = np.float32(a), np.float32(b)
    fa, fb = f(a32), f(b32)
    c_att = f(np.float32(np.float32(-2) * a32) * b32)
    c_rep = f(np.float32(2) * b32)
    bm1 = f(b32 - np.float32(1))
    head = np.repeat(np.arange(n), np.diff(row_ptr))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for ep in range(first_epoch, last_epoch):
            alpha = f(np.float32(1) - np.float32(ep) / np.float32(n_epochs))
            fep = np.float32(ep)
            es = np.flatnonzero(nxt <= fep)                        # ascending edge id: grouped by head, in each vertex's order
            if not len(es):
                continue
            n_neg = ((fep - nneg[es]) / epn[es]).astype(np.int32)
            # every move of the epoch at once (all read the epoch's input), then added per vertex in order
            per = 1 + np.maximum(n_neg, 0)
            me = np.repeat(es, per)                                # the move's edge
            mp = np.arange(len(me)) - np.repeat(np.cumsum(per) - per, per)       # 0 = attractive, p + 1 = the p-th repulsive
            att = mp == 0
            i = head[me]
            other = np.where(att, col[me], (hash_host(seed, ep, me, np.maximum(mp - 1, 0).astype(np.uint64)) % np.uint64(n)).astype(np.int64))
            diff = Y[i] - Y[other]
            d2 = _d2_tree(diff)
            den = fa * np.power(d2, fb) + f(1)
            g = np.where(att, c_att * np.power(d2, bm1) / den, c_rep / ((f(0.001) + d2) * den))
            g = np.where(d2 > 0, g, f(0))
            t = np.clip(g[:, None] * diff, f(-4), f(4))
            move = np.where(att[:, None], f(2) * t, t) * alpha
            rank = np.arange(len(me)) - np.searchsorted(i, i, side="left")          # i is sorted: place within the vertex
            order = np.argsort(rank, kind="stable")
            cuts = np.searchsorted(rank[order], np.arange(int(rank.max()) + 2))
            acc = np.zeros((n, dim), dtype)
            for r in range(len(cuts) - 1):
                sel = order[cuts[r]:cuts[r + 1]]                   # distinct vertices
                acc[i[sel]] += move[sel]
            nxt[es] = nxt[es] + eps[es]
            nneg[es] = nneg[es] + n_neg.astype(np.float32) * epn[es]
            if counts is not None:
                counts[es] += 1
            Y = Y + acc
    return Y, (eps, epn, nxt, nneg)


def _check_disconnected(disconnected):
    if disconnected not in DISCONNECTED:
        raise ValueError(f"umap: disconnected {disconnected!r} is not one of {DISCONNECTED}")


def umap_fit_host(X, n_components: int, n_neighbors: int = 15, seed: int = 42, n_epochs=None, dtype=np.float32, times=None,
                  route: str = "dense", disconnected: str = "random"):
    """The whole restatement on a numpy array: {'embedding' fp32 [n, c], 'init_used', 'a', 'b', 'n_edges', 'route'}.  times: a dict
    that receives seconds per step.  route: 'dense' (the default: n < 4096) or 'sparse' (n < 65536, no n x n array; the initialisation
    is `spectral_init_sparse_host`) -- the restatement does not choose by itself.  disconnected: 'random' (the default: a graph of
    several components takes the random initialisation) or 'components' (`multi_component_init_host`; 'init_used' may then be
    'components' and 'init_info' holds its info)."""
    _check_disconnected(disconnected)
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    _check(n, d, n_neighbors, n_components, route)
    n_epochs = default_epochs(n) if n_epochs is None else int(n_epochs)
    t = [time.perf_counter()]
    a, b = find_ab_params()
    idx, dist = knn_host(X, n_neighbors, route)
    t.append(time.perf_counter())
    G = fuzzy_graph_host(idx, dist, n_epochs, route=route)
    t.append(time.perf_counter())
    init_info = None
    if disconnected == "components":
        Y0, used, init_info = multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, n_components, seed)
    elif route == "sparse":
        Y0, used, _ = spectral_init_sparse_host(G["row_ptr"], G["col"], G["weight"], n, n_components, seed)
    else:
        Y0, used = spectral_init_host(G["P"], n_components, seed)
    t.append(time.perf_counter())
    Y, _ = layout_host(G["row_ptr"], G["col"], G["weight"], Y0, a, b, n_epochs, seed, dtype=dtype)
    t.append(time.perf_counter())
    if times is not None:
        times.update(zip(("knn", "graph", "init", "layout"), np.diff(t)))
    out = {"embedding": Y.astype(np.float32), "init_used": used, "a": a, "b": b, "n_edges": int(len(G["col"])), "init": Y0, "route": route}
    if init_info is not None:
        out["init_info"] = init_info
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------------------------------------
def _fail(what, rc):
    raise EngineError(f"{what}: {ERRORS.get(rc, 'error')} (code {rc})")


def _entry(name: str, route: str) -> str:
    """the C function of a step on a route: dm_umap_<name> or dm_umap_sparse_<name>"""
    return ("dm_umap_sparse_" if route == "sparse" else "dm_umap_") + name


def workspace_bytes(n: int, d: int, n_neighbors: int, n_components: int, route: str = "dense") -> int:
    out = C.c_size_t(0)
    name = _entry("workspace_bytes", pick_route(route, n))
    rc = getattr(_lib(), name)(int(n), int(d), int(n_neighbors), int(n_components), C.byref(out))
    if rc:
        _fail(name, rc)
    return out.value


def _gpu_f32(X, what):
    import torch
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise EngineError(f"{what}: a torch tensor on the GPU is required (the *_host functions are the numpy restatement)")
    return X.to(torch.float32).contiguous()


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _work(work, need, dev):
    import torch
    return torch.empty(need, dtype=torch.uint8, device=dev) if work is None else work


def knn(X, n_neighbors: int = 15, work=None, route: str = "auto"):
    """dm_umap_knn / dm_umap_sparse_knn: (idx int32 [n, k], dist fp32 [n, k]) device tensors, bit-equal to `knn_host` on either route."""
    import torch
    X = _gpu_f32(X, "umapfit.knn")
    n, d = X.shape
    dev = X.device
    route = pick_route(route, n)
    name = _entry("knn", route)
    idx = torch.empty((n, n_neighbors), dtype=torch.int32, device=dev)
    dist = torch.empty((n, n_neighbors), dtype=torch.float32, device=dev)
    work = _work(work, workspace_bytes(n, d, n_neighbors, 1, route), dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib(), name)(_stream(dev), _p(X), n, d, int(n_neighbors), _p(work), work.numel(), _p(idx), _p(dist))
    if rc:
        _fail(name, rc)
    return idx, dist


def fuzzy_graph(idx, dist, n_epochs: int = 500, work=None, route: str = "auto"):
    """dm_umap_graph / dm_umap_sparse_graph: a dict of device tensors: rho, sigma [n], P [n, n] (the dense route only), row_ptr [n + 1],
    col, weight (2 n k slots; the first n_edges hold the edges), n_edges (int32 [])."""
    import torch
    dist = _gpu_f32(dist, "umapfit.fuzzy_graph")
    dev = dist.device
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    n, k = dist.shape
    if idx.shape != dist.shape:
        raise EngineError("umapfit.fuzzy_graph: idx and dist must both be [n, k]")
    route = pick_route(route, n)
    out = {"rho": torch.empty(n, dtype=torch.float32, device=dev), "sigma": torch.empty(n, dtype=torch.float32, device=dev),
           "row_ptr": torch.empty(n + 1, dtype=torch.int32, device=dev),
           "col": torch.empty(2 * n * k, dtype=torch.int32, device=dev), "weight": torch.empty(2 * n * k, dtype=torch.float32, device=dev),
           "n_edges": torch.empty((), dtype=torch.int32, device=dev)}
    if route == "dense":
        if n >= UMAP_MAX_N:                                # before the n x n allocation
            _fail("dm_umap_graph", 2)
        out["P"] = torch.empty((n, n), dtype=torch.float32, device=dev)
    work = _work(work, workspace_bytes(n, 1, k, 1, route), dev)
    dense = (_p(out["P"]),) if route == "dense" else ()
    name = _entry("graph", route)
    with torch.cuda.device(dev):
        rc = getattr(_lib(), name)(_stream(dev), _p(idx), _p(dist), n, k, int(n_epochs), _p(work), work.numel(), _p(out["rho"]),
                                   _p(out["sigma"]), *dense, _p(out["row_ptr"]), _p(out["col"]), _p(out["weight"]), _p(out["n_edges"]))
    if rc:
        _fail(name, rc)
    return out


def layout(row_ptr, col, weight, n_edges: int, Y0, a: float, b: float, n_epochs: int = 500, seed: int = 42, first_epoch: int = 0,
           last_epoch=None, work=None, n_neighbors: int = UMAP_MAX_NEIGHBORS, route: str = "auto"):
    """dm_umap_layout / dm_umap_sparse_layout: epochs [first_epoch, last_epoch) enqueued back to back on the current stream; returns the new coordinates
    (Y0 is left alone).  The schedule lives in `work`: first_epoch = 0 starts it, a later first_epoch goes on from the same `work`."""
    import torch
    Y = _gpu_f32(Y0, "umapfit.layout").clone()
    dev = Y.device
    n, dim = Y.shape
    last_epoch = n_epochs if last_epoch is None else last_epoch
    route = pick_route(route, n)
    name = _entry("layout", route)
    work = _work(work, workspace_bytes(n, 1, min(n_neighbors, max(n - 1, 2)), dim, route), dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib(), name)(_stream(dev), _p(row_ptr), _p(col), _p(weight), n, int(n_edges), dim, float(a), float(b),
                                   int(n_epochs), int(seed) & 0x7FFFFFFF, int(first_epoch), int(last_epoch), _p(Y), _p(work), work.numel())
    if rc:
        _fail(name, rc)
    return Y


def spectral_workspace_bytes(n: int, n_components: int, route: str = "dense") -> int:
    out = C.c_size_t(0)
    name = _entry("spectral_workspace_bytes", pick_route(route, n))
    rc = getattr(_lib(), name)(int(n), int(n_components), C.byref(out))
    if rc:
        _fail(name, rc)
    return out.value


def spectral_host_arrays(n: int, dim: int, seed: int = 42):
    """(noise, fallback) fp32 [n, dim]: what dm_umap_spectral takes from the host, drawn as `spectral_init_host` draws them (each from
    a fresh RandomState(seed): a fit uses one or the other)."""
    noise = np.random.RandomState(seed).normal(scale=0.0001, size=(n, dim)).astype(np.float32)
    return noise, _rescale(np.random.RandomState(seed).uniform(low=-10.0, high=10.0, size=(n, dim)))


def spectral_status(status):
    """The status record of dm_umap_spectral (8 float64 values, on the host) as `spectral_init_iter_host` reports it."""
    s = [float(v) for v in status]
    used = "random" if s[0] else "spectral"
    return {"init_used": used, "status": "random" if s[0] else "converged" if s[3] else "not_converged", "n_comp": int(s[1]), "iters": int(s[2]),
            "max_residual": s[4], "cut": s[5], "degree": int(s[6]), "block": int(s[7])}


def spectral_init(G, dim: int, seed: int = 42, work=None, return_vectors: bool = False, route: str = "auto"):
    """dm_umap_spectral / dm_umap_sparse_spectral on the edge list of `fuzzy_graph` (G: 'row_ptr', 'col', 'weight' on the device): a dict of device tensors,
    'Y0' fp32 [n, dim], 'eigvals' float64 [dim + 1], 'eigvecs' float64 [n, dim + 1] (return_vectors) and 'status' float64 [8], read
    with `spectral_status`.  Nothing here waits for the device."""
    import torch
    row_ptr = G["row_ptr"]
    if not (isinstance(row_ptr, torch.Tensor) and row_ptr.is_cuda):
        raise EngineError("umapfit.spectral_init: the graph must be on the GPU (spectral_init_iter_host is the numpy restatement)")
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    if dim < 1 or dim > UMAP_MAX_COMPONENTS:
        raise EngineError(f"umapfit.spectral_init: n_components {dim} outside [1, {UMAP_MAX_COMPONENTS}]")
    noise, fallback = (torch.from_numpy(a).to(dev) for a in spectral_host_arrays(n, dim, seed))
    out = {"Y0": torch.empty((n, dim), dtype=torch.float32, device=dev), "eigvals": torch.empty(dim + 1, dtype=torch.float64, device=dev),
           "eigvecs": torch.empty((n, dim + 1), dtype=torch.float64, device=dev) if return_vectors else None,
           "status": torch.empty(8, dtype=torch.float64, device=dev)}
    route = pick_route(route, n)
    name = _entry("spectral", route)
    work = _work(work, spectral_workspace_bytes(n, dim, route), dev)
    with torch.cuda.device(dev):
        rc = getattr(_lib(), name)(_stream(dev), _p(row_ptr), _p(G["col"]), _p(G["weight"]), n, int(dim), int(seed) & 0x7FFFFFFF, _p(noise),
                                   _p(fallback), _p(work), work.numel(), _p(out["Y0"]), _p(out["eigvals"]),
                                   _p(out["eigvecs"]) if return_vectors else None, _p(out["status"]))
    if rc:
        _fail(name, rc)
    return out


def components(G, X=None, work=None):
    """dm_umap_components on the edge list of `fuzzy_graph` (G: 'row_ptr', 'col', 'weight' on the device; either route's): a dict of
    device tensors laid out as `component_groups_host` lays them out, sized for any component count -- 'comp' int32 [n], 'count' int32
    [1], 'offsets' and 'edge_offsets' int32 [n + 1] (c + 1 entries count), 'perm' int32 [n], 'sub_row_ptr' int32 [2 n + 1] (n + c
    count), 'sub_col' / 'sub_weight' (as many slots as G's; edge_offsets[c] count), and with X (fp32 [n, d] on the device)
    'centroids' float64 [min(n, 1024), d].  Nothing here waits for the device."""
    import torch
    row_ptr = G["row_ptr"]
    if not (isinstance(row_ptr, torch.Tensor) and row_ptr.is_cuda):
        raise EngineError("umapfit.components: the graph must be on the GPU (component_groups_host is the numpy restatement)")
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    cap = int(min(G["col"].numel(), G["weight"].numel()))
    d = 1
    if X is not None:
        X = _gpu_f32(X, "umapfit.components")
        if X.dim() != 2 or X.shape[0] != n:
            raise EngineError(f"umapfit.components: X must be [{n}, d], got {tuple(X.shape)}")
        d = X.shape[1]
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"comp": torch.empty(max(n, 0), **i32), "count": torch.empty(1, **i32), "offsets": torch.empty(max(n, 0) + 1, **i32),
           "perm": torch.empty(max(n, 0), **i32), "edge_offsets": torch.empty(max(n, 0) + 1, **i32),
           "sub_row_ptr": torch.empty(2 * max(n, 0) + 1, **i32), "sub_col": torch.empty(cap, **i32),
           "sub_weight": torch.empty(cap, dtype=torch.float32, device=dev),
           "centroids": torch.empty((min(max(n, 0), MULTI_MAX_COMP), d), dtype=torch.float64, device=dev) if X is not None else None}
    need = C.c_size_t(0)
    rc = _lib().dm_umap_components_workspace_bytes(n, C.byref(need))
    if rc:
        _fail("dm_umap_components_workspace_bytes", rc)
    work = _work(work, need.value, dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_umap_components(_stream(dev), _p(row_ptr), _p(G["col"]), _p(G["weight"]), _p(X) if X is not None else None, n, d, cap,
                                       _p(work), work.numel(), _p(out["comp"]), _p(out["count"]), _p(out["offsets"]), _p(out["perm"]),
                                       _p(out["edge_offsets"]), _p(out["sub_row_ptr"]), _p(out["sub_col"]), _p(out["sub_weight"]),
                                       _p(out["centroids"]) if X is not None else None)
    if rc:
        _fail("dm_umap_components", rc)
    return out


def components_to_host(comps, centroids: bool = False):
    """`components`' dict on the host in `component_groups_host`'s form, trimmed to the component count.  Two reads at most: the
    integers first (c decides how much of the rest counts), the centroids if asked."""
    import torch
    n = comps["comp"].numel()
    ints = torch.cat([comps["count"], comps["offsets"], comps["edge_offsets"], comps["comp"], comps["perm"], comps["sub_row_ptr"]]).cpu().numpy()
    c = int(ints[0])
    cut = np.cumsum([1, n + 1, n + 1, n, n, 2 * n + 1])
    offsets, edge_offsets, comp, perm, srp = (ints[a:b] for a, b in zip(cut[:-1], cut[1:]))
    total = int(edge_offsets[c])
    out = {"comp": comp.copy(), "n_comp": c, "offsets": offsets[:c + 1].copy(), "perm": perm.copy(), "edge_offsets": edge_offsets[:c + 1].copy(),
           "sub_row_ptr": srp[:n + c].copy(), "sub_col": comps["sub_col"][:total].cpu().numpy(), "sub_weight": comps["sub_weight"][:total].cpu().numpy()}
    if centroids and comps["centroids"] is not None:
        out["centroids"] = comps["centroids"][:min(c, MULTI_MAX_COMP)].cpu().numpy()
    return out


def multi_workspace_bytes(n: int, n_components: int) -> int:
    out = C.c_size_t(0)
    rc = _lib().dm_umap_multi_workspace_bytes(int(n), int(n_components), C.byref(out))
    if rc:
        _fail("dm_umap_multi_workspace_bytes", rc)
    return out.value


def multi_status(status):
    """The status records of dm_umap_multi_init (float64 [c, 8], on the host), one dict per component as `spectral_status` reads
    them; 'status' is 'uniform' for a component that was placed, not solved."""
    out = []
    for rec in np.asarray(status, np.float64).reshape(-1, 8):
        st = spectral_status(rec)
        if rec[0] == 2.0:
            st.update(init_used="uniform", status="uniform")
        out.append(st)
    return out


def multi_component_init(G, X, dim: int, seed: int = 42, work=None, route: str = "auto", comps=None):
    """The device's initialisation with disconnected='components' (dm_umap_components, dm_umap_multi_init; `multi_component_init_host`
    with solver='iter' is the restatement).  G: `fuzzy_graph`'s dict, X: fp32 [n, d], both on the device.  The component count, the
    offsets and the edge offsets are read once (a second read takes the centroids when there are more than 2 dim components); the host
    makes the meta-embedding (`meta_embedding_host`) and the plan, uploads them, and everything else is enqueued without waiting.
    One component takes `spectral_init` (dm_umap_spectral on `route`) and every fallback its random Y0, bit for bit as before.
    Returns a dict: 'Y0' (device fp32 [n, dim]), 'status' (device float64 [c, 8]; read with `multi_status`, or `spectral_status` when
    'mode' is 'single'), 'mode' ('multi' | 'single' | 'random'), 'info' ('n_comp', 'sizes', 'plan', 'meta_kind', 'reason', 'meta') and
    for 'multi' also 'R', 'eigvals', 'eigvecs' (grouped order) and 'comps'."""
    import torch
    row_ptr = G["row_ptr"]
    if not (isinstance(row_ptr, torch.Tensor) and row_ptr.is_cuda):
        raise EngineError("umapfit.multi_component_init: the graph must be on the GPU (multi_component_init_host is the numpy restatement)")
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    if dim < 1 or dim > UMAP_MAX_COMPONENTS:
        raise EngineError(f"umapfit.multi_component_init: n_components {dim} outside [1, {UMAP_MAX_COMPONENTS}]")
    X = _gpu_f32(X, "umapfit.multi_component_init")
    # The centroids are computed whether or not c > 2 dim will need them: c is not known before the read below, the pass over X is
    # inside the 1.2 ms the whole step takes at 10 000 x 128, and a second call after the read would cost a launch round more.
    comps = components(G, X) if comps is None else comps
    head = torch.cat([comps["count"], comps["offsets"], comps["edge_offsets"]]).cpu().numpy()          # the added host read
    c = int(head[0])
    offsets, edge_offsets = np.ascontiguousarray(head[1:c + 2]), np.ascontiguousarray(head[n + 2:n + c + 3])
    sizes = np.diff(offsets)
    info = {"n_comp": c, "sizes": sizes, "plan": None, "meta_kind": None, "reason": None, "meta": None}
    if c == 1 or dim + 1 >= n or c > MULTI_MAX_COMP:
        S = spectral_init(G, dim, seed, route=route)
        info["reason"] = None if c == 1 else "n_components + 1 >= n" if dim + 1 >= n else f"more than {MULTI_MAX_COMP} components"
        return {"Y0": S["Y0"], "status": S["status"], "mode": "single", "info": info}
    if c > 2 * dim and comps.get("centroids") is None:
        raise EngineError(f"umapfit.multi_component_init: {c} components > 2 x {dim} need the centroids: call components(G, X) with X")
    cent = comps["centroids"][:c].cpu().numpy() if c > 2 * dim else None
    meta = meta_embedding_host(cent, c, dim)
    info.update(meta_kind=meta["kind"], meta=meta)
    noise, fallback = spectral_host_arrays(n, dim, seed)
    if meta["reason"]:
        info.update(reason=meta["reason"], detail=meta["detail"])
        return {"Y0": torch.from_numpy(fallback).to(dev), "status": None, "mode": "random", "info": info}
    plan = multi_component_plan(sizes, dim)
    info["plan"] = plan
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    d_plan, d_meta, d_range, d_unit, d_noise = up(plan), up(meta["meta"]), up(meta["range"]), up(multi_host_arrays(n, dim, seed)), up(noise)
    m = dim + 1
    out = {"Y0": torch.empty((n, dim), dtype=torch.float32, device=dev), "R": torch.empty((n, dim), dtype=torch.float64, device=dev),
           "eigvals": torch.empty((c, m), dtype=torch.float64, device=dev), "eigvecs": torch.empty((n, m), dtype=torch.float64, device=dev),
           "status": torch.empty((c, 8), dtype=torch.float64, device=dev), "mode": "multi", "info": info, "comps": comps}
    work = _work(work, multi_workspace_bytes(n, dim), dev)
    h_off, h_eoff, h_plan = (np.ascontiguousarray(a, dtype=np.int32) for a in (offsets, edge_offsets, plan))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731
    with torch.cuda.device(dev):
        rc = _lib().dm_umap_multi_init(_stream(dev), _p(comps["sub_row_ptr"]), _p(comps["sub_col"]), _p(comps["sub_weight"]), _p(comps["perm"]),
                                       _p(comps["comp"]), _p(comps["offsets"]), _p(d_plan), hp(h_off), hp(h_eoff), hp(h_plan), n, c,
                                       comps["sub_col"].numel(), int(dim), int(seed) & 0x7FFFFFFF, _p(d_meta), _p(d_range), _p(d_unit),
                                       _p(d_noise), _p(work), work.numel(), _p(out["Y0"]), _p(out["R"]), _p(out["eigvals"]),
                                       _p(out["eigvecs"]), _p(out["status"]))
    if rc:
        _fail("dm_umap_multi_init", rc)
    return out


INIT_SOLVERS = ("host", "device")


def umap_fit(X, n_components: int, n_neighbors: int = 15, seed: int = 42, n_epochs=None, work=None, times=None, init_solver: str = "host",
             route: str = "auto", disconnected: str = "random"):
    """`umap.UMAP(n_components, n_neighbors).fit_transform(X)` by the rules of this module, on the device X lives on: {'embedding'
    (device fp32 [n, c]), 'init_used', 'a', 'b', 'n_edges', 'init_solver', 'init_iters', 'route'}.  route: 'auto' (dense below 4096 rows,
    sparse from there), 'dense' or 'sparse'; the same bits wherever both run with init_solver 'device'.  init_solver 'host': the graph
    comes to the host once for the spectral initialisation (`spectral_init_host` of the dense P; on the sparse route
    `spectral_init_sparse_host` of the edge list: the same eigh below 4096 rows, scipy's eigsh from there).  'device': dm_umap_spectral; the only host read is its status
    record, together with n_edges; a status of not converged takes the host's initialisation instead, and 'init_solver' says
    'host (device not converged)'.  The epochs run without a host round trip.  Bit-reproducible.  times: a dict that receives
    seconds per step (it synchronises).  disconnected: 'random' (the default: a graph of several components takes the random
    initialisation, as above) or 'components': every component gets its own spectral embedding around a meta-embedding of the
    components (`multi_component_init_host` states the rule).  With init_solver 'host' the graph comes to the host as before and the
    restatement runs; with 'device', `multi_component_init` (one more host read: the component count and offsets); 'init_used' is
    then 'components', or 'spectral' / 'random' where the rule falls back to them, and 'init_reason' says why."""
    import torch
    if init_solver not in INIT_SOLVERS:
        raise ValueError(f"umap_fit: init_solver {init_solver!r} is not one of {INIT_SOLVERS}")
    _check_disconnected(disconnected)
    X = _gpu_f32(X, "umapfit.umap_fit")
    if X.dim() != 2:
        raise EngineError(f"umapfit.umap_fit: X must be [n, d], got {tuple(X.shape)}")
    n, d = X.shape
    dev = X.device
    n_epochs = default_epochs(n) if n_epochs is None else int(n_epochs)
    route = pick_route(route, n)
    work = _work(work, workspace_bytes(n, d, n_neighbors, n_components, route), dev)

    def mark():
        if times is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    a, b = find_ab_params()
    t = [mark()]
    idx, dist = knn(X, n_neighbors, work, route)
    t.append(mark())
    G = fuzzy_graph(idx, dist, n_epochs, work, route)
    solver, iters, reason = "host", 0, None
    multi = disconnected == "components"
    if init_solver == "device" and multi:
        if times is not None:
            n_edges = int(G["n_edges"])
        t.append(mark())
        M = multi_component_init(G, X, n_components, seed, route=route)
        reason = M["info"]["reason"]
        if M["status"] is None:                            # a fallback the host decided: nothing of the device's to read
            if times is None:
                n_edges = int(G["n_edges"])
            Y0, used, solver = M["Y0"], "random", "device"
        else:
            if times is not None:
                flat = M["status"].reshape(-1).cpu().numpy()
            else:
                both = torch.cat([G["n_edges"].to(torch.float64).reshape(1), M["status"].reshape(-1)]).cpu().numpy()   # the fit's last read
                n_edges, flat = int(both[0]), both[1:]
            if M["mode"] == "single":
                st = spectral_status(flat)
                used, iters, bad = st["init_used"], st["iters"], st["status"] == "not_converged"
            else:
                sts = multi_status(flat)
                used, iters = "components", max(s["iters"] for s in sts)
                bad = any(s["status"] not in ("converged", "uniform") for s in sts)
            Y0, solver = M["Y0"], "host (device not converged)" if bad else "device"
    elif init_solver == "device":
        if times is not None:                              # timed: the graph's step ends before the solve is enqueued
            n_edges = int(G["n_edges"])
        t.append(mark())
        S = spectral_init(G, n_components, seed, route=route)       # its own workspace; enqueued before anything is read
        if times is not None:
            st = spectral_status(S["status"].cpu().numpy())
        else:
            both = torch.cat([G["n_edges"].to(torch.float64).reshape(1), S["status"]]).cpu().numpy()       # the fit's one host read
            n_edges, st = int(both[0]), spectral_status(both[1:])
        Y0, used, solver, iters = S["Y0"], st["init_used"], "device", st["iters"]
        if st["status"] == "not_converged":
            solver = "host (device not converged)"
    else:
        n_edges = int(G["n_edges"])
        t.append(mark())
    if solver != "device" and multi:
        Y0, used, hinfo = multi_component_init_host(G["row_ptr"].cpu().numpy(), G["col"][:n_edges].cpu().numpy(),
                                                    G["weight"][:n_edges].cpu().numpy(), X.cpu().numpy(), n_components, seed)
        reason = hinfo["reason"]
        Y0 = torch.from_numpy(Y0).to(dev)
    elif solver != "device":
        if route == "sparse":
            Y0, used, _ = spectral_init_sparse_host(G["row_ptr"].cpu().numpy(), G["col"][:n_edges].cpu().numpy(),
                                                    G["weight"][:n_edges].cpu().numpy(), n, n_components, seed)
        else:
            Y0, used = spectral_init_host(G["P"].cpu().numpy(), n_components, seed)
        Y0 = torch.from_numpy(Y0).to(dev)
    t.append(mark())
    Y = layout(G["row_ptr"], G["col"], G["weight"], n_edges, Y0, a, b, n_epochs, seed, work=work, n_neighbors=n_neighbors, route=route)
    t.append(mark())
    if times is not None:
        times.update(zip(("knn", "graph", "init", "layout"), np.diff(t)))
    out = {"embedding": Y, "init_used": used, "a": a, "b": b, "n_edges": n_edges, "init_solver": solver, "init_iters": iters,
           "route": route}
    if multi:
        out["init_reason"] = reason
    return out


def compress(X, n_groups: int, num_components: int = 32, n_neighbors: int = 15, seed: int = 42, n_epochs=None, init_solver: str = "host",
             disconnected: str = "random"):
    """`compress` of the parallel dataset (cluster.py:253-266): one fit per group of d // n_groups consecutive features (a country's
    block), the embeddings side by side.  A GPU tensor stays on the device (init_solver: `umap_fit`'s); a numpy array takes the
    restatement.  From 4096 rows both take the sparse route by themselves (the reference's default is 10 000 rows).  disconnected:
    `umap_fit`'s ('random', the default, or 'components')."""
    import torch
    _check_disconnected(disconnected)
    on_gpu = isinstance(X, torch.Tensor) and X.is_cuda
    if isinstance(X, torch.Tensor) and not on_gpu:
        X = X.numpy()
    d = X.shape[1]
    group = d // int(n_groups)
    if group < 1:
        raise ValueError(f"compress: {n_groups} groups of {d} features")
    parts = []
    for i in range(0, d, group):
        if on_gpu:
            parts.append(umap_fit(X[:, i:i + group], num_components, n_neighbors, seed, n_epochs, init_solver=init_solver,
                                  disconnected=disconnected)["embedding"])
        else:
            parts.append(umap_fit_host(X[:, i:i + group], num_components, n_neighbors, seed, n_epochs,
                                       route=pick_route("auto", X.shape[0]), disconnected=disconnected)["embedding"])
    return torch.cat(parts, dim=1) if on_gpu else np.hstack(parts)
