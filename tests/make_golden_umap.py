#!/usr/bin/env python
"""Golden vectors that pin the numpy restatement of diff-mining_amd/umapfit.py to umap-learn (needs umap-learn 0.5.x with numba and
pynndescent; no test needs them).  Until tests/golden/umap_ref.npz is committed, tests/test_umap.py::test_matches_umap_learn skips
and the projection's parity with umap-learn is unpinned.

Recorded per case of GOLDEN_CASES (inputs from tests/umap_cases.py), all from umap-learn's own functions at the reference's
settings (euclidean, n_neighbors of the case, local_connectivity 1, set_op_mix_ratio 1):

    <case>_X          float32 [n, d]     the input (the test checks it against its own generator)
    <case>_knn_idx    int32   [n, k]     umap.umap_.nearest_neighbors (exact below 4096 rows)
    <case>_knn_dist   float32 [n, k]
    <case>_sigma      float32 [n]        umap.umap_.smooth_knn_dist
    <case>_rho        float32 [n]
    <case>_graph      float32 [n, n]     umap.umap_.fuzzy_simplicial_set, densified, entries below max / 500 set to 0
    a, b              float64            umap.umap_.find_ab_params(1.0, 0.1)
    tags, umap        the case names and the version string

umap-learn's embedding is not recorded: its layout is unseeded at both call sites of the reference and racy, and the layout here
departs from it on purpose.

    python tests/make_golden_umap.py            # writes the file
    python tests/make_golden_umap.py --check    # validates keys / shapes / dtypes of an existing file; needs no umap-learn
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests import umap_cases as UC  # noqa: E402

NPZ = os.path.join(HERE, "golden", "umap_ref.npz")
GOLDEN_CASES = ("n65", "n130", "dup", "blob300")          # under 1 MiB together: the dense graphs are 300 x 300 at the most


def expected_layout():
    """key -> (shape, dtype)"""
    out = {"a": ((), np.float64), "b": ((), np.float64)}
    for tag in GOLDEN_CASES:
        n, d, k, _ = UC.SHAPES[tag]
        out.update({f"{tag}_X": ((n, d), np.float32), f"{tag}_knn_idx": ((n, k), np.int32), f"{tag}_knn_dist": ((n, k), np.float32),
                    f"{tag}_sigma": ((n,), np.float32), f"{tag}_rho": ((n,), np.float32), f"{tag}_graph": ((n, n), np.float32)})
    return out


def check(path=NPZ):
    """-> list of complaints about the file (empty = fine)"""
    if not os.path.exists(path):
        return [f"{path} is absent"]
    bad = []
    with np.load(path) as z:
        for key, (shape, dtype) in expected_layout().items():
            if key not in z.files:
                bad.append(f"{key}: missing")
            elif z[key].shape != shape or z[key].dtype != dtype:
                bad.append(f"{key}: {z[key].dtype} {z[key].shape}, expected {np.dtype(dtype)} {shape}")
            elif key.endswith("_X") and not np.array_equal(z[key], UC.case(key[:-2])[0]):
                bad.append(f"{key}: not the input tests/umap_cases.py generates")
            elif not np.isfinite(z[key]).all():
                bad.append(f"{key}: not finite")
        for key in ("tags", "umap"):
            if key not in z.files:
                bad.append(f"{key}: missing")
    if os.path.getsize(path) > (1 << 20):
        bad.append(f"{path}: larger than 1 MiB")
    return bad


def main():
    if "--check" in sys.argv:
        bad = check()
        print("\n".join(bad) if bad else f"{NPZ}: fine")
        return 1 if bad else 0
    import umap
    from umap.umap_ import find_ab_params, fuzzy_simplicial_set, nearest_neighbors, smooth_knn_dist
    out = {"tags": np.array(GOLDEN_CASES), "umap": np.array(umap.__version__)}
    a, b = find_ab_params(1.0, 0.1)
    out["a"], out["b"] = np.float64(a), np.float64(b)
    for tag in GOLDEN_CASES:
        X, k, _, _ = UC.case(tag)
        rs = np.random.RandomState(UC.SEED)
        idx, dist, _ = nearest_neighbors(X, k, "euclidean", {}, False, rs)
        sigma, rho = smooth_knn_dist(dist.astype(np.float32), float(k), local_connectivity=1.0)
        graph = fuzzy_simplicial_set(X, k, rs, "euclidean", knn_indices=idx, knn_dists=dist)[0].toarray().astype(np.float32)
        graph[graph < graph.max() / np.float32(500)] = 0
        out.update({f"{tag}_X": X, f"{tag}_knn_idx": idx.astype(np.int32), f"{tag}_knn_dist": dist.astype(np.float32),
                    f"{tag}_sigma": sigma.astype(np.float32), f"{tag}_rho": rho.astype(np.float32), f"{tag}_graph": graph})
    os.makedirs(os.path.dirname(NPZ), exist_ok=True)
    np.savez_compressed(NPZ, **out)
    bad = check()
    print("\n".join(bad) if bad else f"wrote {NPZ} ({os.path.getsize(NPZ)} bytes) from umap-learn {umap.__version__}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
