"""The inputs of the UMAP tests (tests/test_umap.py, tests/test_gpu_umap.py) and the bounds measured for them on the CPU.

`python -m tests.umap_cases` measures and prints, per case, what the numpy restatement in fp32 differs from itself in float64 by
(sigma, edge weights, coordinates after one and three moving epochs), how far the nearest weight lies from the pruning threshold,
and, for the two blob cases, the trustworthiness of the restatement's embedding over five seeds.  The figures below are that
output; the GPU tests bound the kernels by 4 x them (another exp / pow implementation) and the CPU tier checks that they still
describe the cases."""
import numpy as np


def blobs(n, d, c, seed, noise):
    """unit-normalised Gaussian blobs: (X fp32 [n, d], blob of each row)"""
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(c, d))
    label = np.arange(n) % c
    X = centres[label] + noise * rs.normal(size=(n, d))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X.astype(np.float32), label


def cloud(n, d, seed):
    return np.random.RandomState(seed).normal(size=(n, d)).astype(np.float32)


def duplicates(seed=3):
    """40 rows in 3 dimensions: rows 0..6 are one point (more copies than n_neighbors = 5: rho = 0 there, the global floor decides
    sigma), rows 7, 8 and 9, 10 are pairs (rho skips the zero)."""
    X = cloud(40, 3, seed)
    X[1:7] = X[0]
    X[8] = X[7]
    X[10] = X[9]
    return X


def split(seed=4):
    """two clouds of 30 rows far apart: with n_neighbors = 5 the graph is disconnected"""
    X = cloud(60, 3, seed)
    X[30:] += 100.0
    return X


# tag: (n, d, n_neighbors, n_components).  n = 17: one above n_neighbors + 1; 65: one past a wave, an odd count for the kNN kernel's row
# pairs; 130: a ragged block of the wave-per-row kernels (4 rows each); 300, 400: several blocks of every kernel, two column tiles of
# the kNN kernel.  d = 3, 33: below and past one staged chunk of 16 features, neither a multiple of it; 64, 128: whole chunks.
SHAPES = {"n17": (17, 3, 15, 2), "n65": (65, 33, 5, 5), "n130": (130, 128, 15, 32), "n300": (300, 33, 15, 5),
          "dup": (40, 3, 5, 2), "split": (60, 3, 5, 2), "blob300": (300, 64, 15, 5), "blob400": (400, 128, 15, 32)}
BLOBS = {"blob300": (6, 0, 1.3), "blob400": (8, 0, 1.5)}          # blobs, seed, noise
SEED = 42
SPREAD_SEEDS = (42, 43, 44, 45, 46)


def case(tag):
    """(X, n_neighbors, n_components, true blob per row or None)"""
    n, d, k, dim = SHAPES[tag]
    if tag in BLOBS:
        c, seed, noise = BLOBS[tag]
        X, label = blobs(n, d, c, seed, noise)
        return X, k, dim, label
    X = duplicates() if tag == "dup" else split() if tag == "split" else cloud(n, d, len(tag) + n)
    assert X.shape == (n, d)
    return X, k, dim, None


def moving_epochs(count):
    """Epoch 0 moves nothing (every next_e starts at eps_e >= 1): `count` moving epochs are epochs [0, count + 1)."""
    return count + 1


def measure(tag, a, b):
    """What fp32 costs the numpy restatement on this case: max |fp32 - float64| of sigma, of the weights, of the coordinates after one
    and three moving epochs from the same initialisation; and the least distance of a weight (pruned or kept) from the threshold."""
    from diff_mining_amd import umapfit as U
    X, k, dim, _ = case(tag)
    idx, dist = U.knn_host(X, k)
    G64, G32 = U.fuzzy_graph_host(idx, dist, 500, np.float64), U.fuzzy_graph_host(idx, dist, 500, np.float32)
    out = {"sigma": float(np.abs(G64["sigma"].astype(np.float64) - G32["sigma"]).max())}
    same = np.array_equal(G64["row_ptr"], G32["row_ptr"]) and np.array_equal(G64["col"], G32["col"])
    out["weight"] = float(np.abs(G64["weight"].astype(np.float64) - G32["weight"]).max()) if same else float("nan")
    out["gap"] = threshold_gap(idx, dist, G64)
    Y0, _ = U.spectral_init_host(G64["P"], dim, SEED)
    for count in (1, 3):
        last = moving_epochs(count)
        y64, _ = U.layout_host(G64["row_ptr"], G64["col"], G64["weight"], Y0, a, b, 500, SEED, 0, last, np.float64)
        y32, _ = U.layout_host(G64["row_ptr"], G64["col"], G64["weight"], Y0, a, b, 500, SEED, 0, last, np.float32)
        out[f"layout{count}"] = float(np.abs(y64 - y32).max())
    return out


def threshold_gap(idx, dist, G):
    """min |P_ij - threshold| over the entries of the unpruned union that are not 0 already"""
    n = len(idx)
    x = dist.astype(np.float64) - G["rho"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        val = np.where((x <= 0) | (G["sigma"][:, None] == 0), 1.0, np.exp(-(x / G["sigma"].astype(np.float64)[:, None]))).astype(np.float32)
    val[idx == np.arange(n)[:, None]] = 0
    A = np.zeros((n, n), np.float32)
    np.put_along_axis(A, idx.astype(np.int64), val, axis=1)
    P = (A + A.T) - A * A.T
    return float(np.abs(P[P > 0].astype(np.float64) - float(G["threshold"])).min())


def trust(X, Y, k=15):
    from sklearn.manifold import trustworthiness
    return float(trustworthiness(X, Y, n_neighbors=k))


# ---- measured (python -m tests.umap_cases) -----------------------------------------------------------------------------------------
BOUNDS = {
    "n17": {"sigma": 1.907e-06, "weight": 1.013e-06, "gap": 1.577e-03, "layout1": 4.932e-07, "layout3": 5.698e-06},
    "n65": {"sigma": 0.000e+00, "weight": 5.960e-08, "gap": 1.356e-03, "layout1": 5.440e-07, "layout3": 2.574e-06},
    "n130": {"sigma": 3.815e-06, "weight": 1.803e-06, "gap": 5.323e-04, "layout1": 5.056e-07, "layout3": 3.273e-06},
    "n300": {"sigma": 1.907e-06, "weight": 1.371e-06, "gap": 1.164e-03, "layout1": 5.668e-07, "layout3": 1.376e-05},
    "dup": {"sigma": 0.000e+00, "weight": 1.192e-07, "gap": 4.082e-04, "layout1": 1.117e-06, "layout3": 6.951e-05},
    "split": {"sigma": 7.629e-06, "weight": 7.004e-06, "gap": 5.298e-02, "layout1": 7.724e-07, "layout3": 2.344e-05},
    "blob300": {"sigma": 2.384e-07, "weight": 2.056e-06, "gap": 6.806e-04, "layout1": 1.063e-06, "layout3": 1.066e-04},
    "blob400": {"sigma": 2.384e-07, "weight": 1.609e-06, "gap": 3.821e-03, "layout1": 6.117e-07, "layout3": 1.420e-05},
}
# trustworthiness (k = 15) of the numpy restatement's embedding: at SEED, and its spread (max - min) over SPREAD_SEEDS
HOST_TRUST = {"blob300": 0.9695, "blob400": 0.9789}                # seeds 42..46: 0.9695 0.9684 0.9717 0.9692 0.9714 / 0.9789 0.9781 0.9778 0.9783 0.9786
HOST_TRUST_SPREAD = {"blob300": 0.0033, "blob400": 0.0011}


if __name__ == "__main__":
    from diff_mining_amd import umapfit as U
    a, b = U.find_ab_params()
    print("BOUNDS = {")
    for tag in SHAPES:
        m = measure(tag, a, b)
        print(f'    "{tag}": {{' + ", ".join(f'"{k}": {v:.3e}' for k, v in m.items()) + "},")
    print("}")
    for tag in BLOBS:
        X, k, dim, _ = case(tag)
        ts = [trust(X, U.umap_fit_host(X, dim, k, seed)["embedding"]) for seed in SPREAD_SEEDS]
        print(f'HOST_TRUST["{tag}"] = {ts[0]:.4f}; HOST_TRUST_SPREAD["{tag}"] = {max(ts) - min(ts):.4f}    # {[round(t, 4) for t in ts]}')
