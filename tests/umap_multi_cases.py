"""The inputs of the disconnected-graph UMAP tests (tests/test_umap_multi.py, tests/test_gpu_umap_multi.py,
tests/test_gpu_umap_multi_guards.py) and what was measured for them on the CPU.

`python -m tests.umap_multi_cases` prints, per case, the components the restatement finds and the smallest eigen-gap among eigenvalues
0 .. dim + 1 of any solved component, and for `blob1200` the trustworthiness and the Spearman figure (all pairwise distances, input
against final embedding) of the restatement's fit over five seeds, disconnected='random' against 'components'.  The figures below
are that output; the CPU tier checks that they still describe the cases."""
import functools

import numpy as np

from tests import umap_cases as UC

SEED = UC.SEED
SPREAD_SEEDS = UC.SPREAD_SEEDS


def clouds(sizes, d, centres, sigma, seed):
    """Gaussian clouds, one per component, in order; then the rows permuted, so that grouping by component is never the identity."""
    rs = np.random.RandomState(seed)
    parts = [np.asarray(c, np.float64) + sigma * rs.normal(size=(s, d)) for s, c in zip(sizes, centres)]
    X = np.concatenate(parts)
    return X[rs.permutation(len(X))].astype(np.float32)


def _e(d, i, scale):
    v = np.zeros(d)
    v[i] = scale
    return v


_META6 = np.random.RandomState(7).normal(size=(6, 3))
# tag: (sizes, d, centres, sigma, seed, n_neighbors, n_components)
CLOUDS = {
    "two": ([40, 20], 3, [(0, 0, 0), (100, 0, 0)], 1.0, 1, 5, 2),                                   # the table, both solved
    "tiny": ([50, 30, 7], 8, [np.zeros(8), _e(8, 0, 50.0), _e(8, 1, 50.0)], 1.0, 2, 5, 5),        # 7 < 2 dim: a uniform component
    "edge": ([5, 6, 40], 4, [np.zeros(4), _e(4, 0, 60.0), _e(4, 1, 60.0)], 1.0, 1, 5, 3),         # 5 = 2 dim - 1 uniform, 6 = 2 dim solved, block = size
    "dim1": ([12, 9], 3, [(0, 0, 0), (80, 0, 0)], 1.0, 5, 5, 1),                                    # one eigenvector (seed: see STALL)
    "dim1s4": ([12, 9], 3, [(0, 0, 0), (80, 0, 0)], 1.0, 4, 5, 1),                                  # the same at seed 4: STALL
    "meta6": ([20, 12, 16, 14, 18, 13], 3, _META6, 0.02, 3, 5, 2),                                  # 6 > 2 dim: the affinity meta-embedding
    "far6": ([20, 12, 16, 14, 18, 13], 3, _META6 * 200.0, 0.02, 3, 5, 2),                           # every affinity 0: degenerate
    "wide": ([100, 100, 100], 33, [np.zeros(33), _e(33, 0, 30.0), _e(33, 1, 30.0)], 1.0, 5, 15, 32),  # block 49 < 100 rows, dim 32
}
MULTI = ("two", "tiny", "edge", "dim1", "meta6", "wide", "blob1200")        # take the 'components' initialisation
# `dim1` was first drawn at seed 4 (kept as `dim1s4`: components 12 + 9, gap 0.22).  There the 9-row component's block is the whole
# space (b = min(9, 2 + 8) = n), so the Chebyshev filter cannot damp anything out of the block: the filtered block's condition number
# is T_8(3) / min_j |T_8(x_j)| = 6.7e5 / 0.017 (the eigenvalue -0.2231 of M lies next to a root of the degree-8 polynomial), its Gram
# matrix's is the square, 1.5e15, and the restatement's first Cholesky factorisation fails: 'not_converged' after 0 iterations.  That
# is the single-component solver's own limit (tests/umap_spectral_cases.py's cloud9 has b = n too and converges), not this rule's,
# and the rule's answer to it is the host's initialisation; so the case moved to seed 5 and seed 4 stays as the input of that answer.
STALL = "dim1s4"
CONNECTED = ("n65", "blob300")                                  # tests/umap_cases.py's: one component
ALL = MULTI + ("far6",) + CONNECTED
# what the CPU tier asserts: the component sizes (sorted), the meta kind, how many components are solved
EXPECT = {"two": ([20, 40], "table", 2), "tiny": ([7, 30, 50], "table", 2), "edge": ([5, 6, 40], "table", 2), "dim1": ([9, 12], "table", 2),
          "dim1s4": ([9, 12], "table", 2),
          "meta6": ([12, 13, 14, 16, 18, 20], "affinity", 6), "far6": ([12, 13, 14, 16, 18, 20], "affinity", 0),
          "wide": ([100, 100, 100], "table", 3), "blob1200": ([100] * 12, "affinity", 12)}
MIN_GAP = 1e-5                                                  # every solved component's gaps are above this


@functools.lru_cache(maxsize=None)
def case(tag):
    """(X fp32 [n, d], n_neighbors, n_components)"""
    if tag in CLOUDS:
        sizes, d, centres, sigma, seed, k, dim = CLOUDS[tag]
        return clouds(sizes, d, centres, sigma, seed), k, dim
    if tag == "blob1200":
        return UC.blobs(1200, 64, 12, 0, 0.25)[0], 15, 5
    X, k, dim, _ = UC.case(tag)
    return X, k, dim


@functools.lru_cache(maxsize=None)
def graph(tag):
    """The restatement's fuzzy graph of the case (computed once, shared, not to be changed)"""
    from diff_mining_amd import umapfit as U
    X, k, _ = case(tag)
    idx, dist = U.knn_host(X, k)
    G = U.fuzzy_graph_host(idx, dist, U.default_epochs(len(X)))
    G.pop("P", None)
    return G


@functools.lru_cache(maxsize=None)
def host_init(tag, solver="iter"):
    """(Y0, init_used, info) of `multi_component_init_host` on the case (computed once, shared, not to be changed)"""
    from diff_mining_amd import umapfit as U
    X, _, dim = case(tag)
    G = graph(tag)
    return U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, SEED, solver)


TOL = 1e-11                                                     # the solver's stopping residual: SPECTRAL_TOL
MAX_ITERS = 20                                                  # as tests/umap_spectral_cases.py


def component_eigh(groups, l):
    """(val, vec, gap) of component l as tests/umap_spectral_cases.py takes them: numpy's eigh of the dense M = D^-1/2 P D^-1/2,
    eigenvalues descending, and every eigenvalue's distance to its nearest neighbour"""
    from diff_mining_amd import umapfit as U
    rp, cl, w, rows = U.sub_graph(groups, l)
    P = np.zeros((rows, rows))
    P[np.repeat(np.arange(rows), np.diff(rp)), cl] = w.astype(np.float64)
    isd = 1.0 / np.sqrt(P.sum(axis=1))
    M = isd[:, None] * P * isd[None, :]
    val, vec = np.linalg.eigh((M + M.T) * 0.5)
    val, vec = val[::-1].copy(), vec[:, ::-1].copy()
    gap = np.minimum(np.abs(np.diff(val, prepend=np.inf)), np.abs(np.diff(val, append=-np.inf)))
    return val, vec, gap


def compare(groups, l, dim, eigvals, eigvecs):
    """(largest |theta - lambda|, largest ||v - v_eigh||_2 / (2 TOL / gap)) over component l's wanted pairs (the Davis-Kahan bound of
    tests/test_umap_spectral.py); eigvals [c, dim + 1], eigvecs [n, dim + 1] in grouped order; v's sign is taken from eigh's"""
    m = dim + 1
    val, vec, gap = component_eigh(groups, l)
    got = eigvecs[groups["offsets"][l]:groups["offsets"][l + 1], :m]
    sign = np.where((got * vec[:, :m]).sum(axis=0) < 0, -1.0, 1.0)
    dist = np.linalg.norm(got * sign[None, :] - vec[:, :m], axis=0)
    return float(np.abs(eigvals[l] - val[:m]).max()), float((dist / (2.0 * TOL / gap[:m])).max())


def min_gap(tag):
    """the smallest gap of eigenvalues 0 .. dim of any solved component to a neighbour (eigenvalue dim + 1 included)"""
    _, _, info = host_init(tag)
    dim = case(tag)[2]
    return min(float(component_eigh(info["groups"], l)[2][:dim + 1].min()) for l in np.flatnonzero(info["plan"]))


def trust(X, Y, k=15):
    return UC.trust(X, Y, k)


def spearman(X, Y, pairs=None):
    """Spearman's rank correlation of the pairwise Euclidean distances of X against those of Y: all pairs, or the given [p, 2] ones"""
    from scipy.spatial.distance import pdist
    from scipy.stats import spearmanr
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if pairs is None:
        return float(spearmanr(pdist(X), pdist(Y))[0])
    i, j = pairs[:, 0], pairs[:, 1]
    return float(spearmanr(np.linalg.norm(X[i] - X[j], axis=1), np.linalg.norm(Y[i] - Y[j], axis=1))[0])


# ---- measured (python -m tests.umap_multi_cases) -----------------------------------------------------------------------------------
GAPS = {"two": 3.659e-02, "tiny": 2.404e-02, "edge": 1.153e-02, "dim1": 2.535e-01, "meta6": 6.506e-02, "wide": 9.303e-04,
        "blob1200": 3.085e-03}
# the restatement's fit (umap_fit_host) per arm of `disconnected`: the figure at SEED and its spread (max - min) over SPREAD_SEEDS.
# blob1200 has 12 components (the affinity meta-embedding), wide 3 (the table).  Seeds 42 .. 46:
#   blob1200 random      trust 0.9800 0.9803 0.9803 0.9805 0.9798   Spearman 0.2211 0.2234 0.2608 0.1882 0.4003   (initialisation's trust 0.5014)
#   blob1200 components  trust 0.9806 0.9801 0.9804 0.9799 0.9797   Spearman 0.7833 0.7851 0.7727 0.7624 0.7742   (0.9788)
#   wide random          trust 0.9428 0.9414 0.9429 0.9424 0.9406   Spearman 0.5448 0.5333 0.5594 0.6167 0.6994   (0.5141)
#   wide components      trust 0.9435 0.9424 0.9429 0.9428 0.9404   Spearman 0.8348 0.8109 0.8570 0.8784 0.8777   (0.7475)
HOST_TRUST = {"blob1200": {"random": 0.9800, "components": 0.9806}, "wide": {"random": 0.9428, "components": 0.9435}}
HOST_TRUST_SPREAD = {"blob1200": {"random": 0.0007, "components": 0.0009}, "wide": {"random": 0.0024, "components": 0.0032}}
HOST_SPEARMAN = {"blob1200": {"random": 0.2211, "components": 0.7833}, "wide": {"random": 0.5448, "components": 0.8348}}
HOST_SPEARMAN_SPREAD = {"blob1200": {"random": 0.2121, "components": 0.0227}, "wide": {"random": 0.1661, "components": 0.0676}}


if __name__ == "__main__":
    from diff_mining_amd import umapfit as U
    print("GAPS = {" + ", ".join(f'"{t}": {min_gap(t):.3e}' for t in MULTI) + "}")
    for tag in ("blob1200", "wide"):
        X, k, dim = case(tag)
        for arm in U.DISCONNECTED:
            fits = [U.umap_fit_host(X, dim, k, seed, disconnected=arm) for seed in SPREAD_SEEDS]
            ts = [trust(X, f["embedding"]) for f in fits]
            ss = [spearman(X, f["embedding"]) for f in fits]
            print(tag, arm, fits[0]["init_used"], fits[0].get("init_info", {}).get("n_comp"), "trust", [round(v, 4) for v in ts],
                  f"spread {max(ts) - min(ts):.4f}", "spearman", [round(v, 4) for v in ss], f"spread {max(ss) - min(ss):.4f}",
                  "init trust", round(trust(X, fits[0]["init"]), 4))
