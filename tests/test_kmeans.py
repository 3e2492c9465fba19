"""CPU tier of the clustering stage's last step: the numpy restatement (clustering.kmeans_fit_host, rank_clusters_host) against
scikit-learn's own fit and the reference's own cluster() tail, both recorded in tests/golden/kmeans_ref.npz by
tests/make_golden_kmeans.py; the draws; the C entry points' refusals (they are checked before any device call)."""
import os
import re

import numpy as np
import pytest

from diff_mining_amd import clustering as CL
from diff_mining_amd import engine as E
from tests import kmeans_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_ARMS = [(t, m, a, nan) for t in ("long257", "k32") for m in ("centroid", "farthest") for a in ("median", "mean")
             for nan in (False, True)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_ref.npz"))


def case_input(gold, tag):
    n, d, k, nb, _ = KC.EMPTY_CASE if tag == "empty" else KC.CASES[tag]
    X = KC.blobs(n, d, nb, float(gold[f"{tag}_noise"]), int(gold[f"{tag}_data_seed"]))
    assert KC.digest(X) == str(gold[f"{tag}_sha256"]), "the regenerated input differs from the one the fixture was made from"
    return X, k


@pytest.mark.parametrize("tag", list(KC.CASES) + ["empty"])
def test_host_fit_equals_sklearn(gold, tag):
    X, k = case_input(gold, tag)
    init = gold["empty_seed_index"] if tag == "empty" else None
    labels, centers, seeds, inertia, n_iter = CL.kmeans_fit_host(X, k, init_index=init)
    assert np.array_equal(seeds, gold[f"{tag}_seed_index"])
    assert np.array_equal(labels, gold[f"{tag}_labels"])
    assert n_iter == int(gold[f"{tag}_n_iter"])
    assert np.abs(centers - gold[f"{tag}_centers"]).max() <= float(gold["restatement_center_err"])
    assert abs(inertia - float(gold[f"{tag}_inertia"])) <= 1e-5 * float(gold[f"{tag}_inertia"])
    if tag == "empty":      # the duplicated start left centre 1 empty in the first iteration; relocation filled it
        assert init[0] == init[1] and np.bincount(labels, minlength=k).min() > 0
    if tag.startswith("long"):
        assert n_iter >= 5


@pytest.mark.parametrize("tag,mode,agg,nan", RANK_ARMS)
def test_host_ranking_equals_reference(gold, tag, mode, agg, nan):
    X, k = case_input(gold, tag)
    labels, centers = gold[f"{tag}_labels"], gold[f"{tag}_centers"]
    D, Xr = KC.rank_inputs(labels, int(gold[f"{tag}_rank{'_nan' if nan else ''}_d_seed"]), nan)
    got = CL.rank_clusters_host(X, labels, centers, D, agg, mode, Xr if mode == "farthest" else None)
    pre = f"{tag}_rank_{mode}_{agg}{'_nan' if nan else ''}_"
    for name, g in zip(("order", "cluster_of_rank", "offsets", "aggregate", "n_nonempty"), got):
        np.testing.assert_array_equal(np.asarray(g), gold[pre + name], err_msg=name)
    if nan and agg == "median":
        assert np.isnan(got[3][got[4] - 1]) and not np.isnan(got[3][:got[4] - 1]).any()
    counts = np.bincount(labels, minlength=k)
    assert (counts[counts > 0] % 2 == 0).any()      # an even member count is among them


def test_uniforms_are_randomstates_draws():
    for k in (1, 2, 7, 8, 32, 256):
        rs = np.random.RandomState(10)
        t = 2 + int(np.log(k))
        want = [rs.random_sample()] + [v for _ in range(1, k) for v in rs.uniform(size=t)]
        got = CL.kmeans_uniforms(k)
        assert got.dtype == np.float64 and np.array_equal(got, np.array(want))
    assert not np.array_equal(CL.kmeans_uniforms(8, seed=11), CL.kmeans_uniforms(8))


def test_host_refusals():
    X = np.zeros((4, 3), np.float32)
    for k, kw in ((5, {}), (0, {}), (257, {}), (2, {"max_iter": 0})):
        with pytest.raises(ValueError):
            CL.kmeans_fit_host(X, k, **kw)
    with pytest.raises(ValueError):
        CL.kmeans_fit_host(np.zeros((4, 0), np.float32), 2)


def test_abi_declares_and_refuses():
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    for s in ("dm_kmeans_workspace_bytes", "dm_kmeans_fit", "dm_cluster_rank"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr) and s in E.SYMBOLS
    assert int(re.search(r"#define DM_KMEANS_MAX_K (\d+)", hdr).group(1)) == CL.KMEANS_MAX_K
    try:
        lib = CL._lib()
    except (E.EngineError, OSError) as e:
        pytest.skip(f"library does not load here: {e}")
    size = E.C.c_size_t(0)
    wb = lambda n, d, k: lib.dm_kmeans_workspace_bytes(n, d, k, E.C.byref(size))      # noqa: E731
    assert wb(1000, 512, 32) == 0 and size.value > 1000 * 512 * 4
    assert (wb(3, 4, 5), wb(10, 4, 0), wb(300, 4, 257), wb(10, 0, 2), wb(1 << 24, 1, 2)) == (2, 3, 3, 4, 5)
    assert lib.dm_kmeans_workspace_bytes(10, 4, 2, None) == 1
    fit = lambda n, d, k, it=300: lib.dm_kmeans_fit(None, None, n, d, k, None, 0, it, 1e-4, None, 0, None, None, None, None, None)     # noqa: E731
    assert (fit(3, 4, 5), fit(10, 4, 0), fit(300, 4, 257), fit(10, 0, 2), fit(1 << 24, 1, 2), fit(10, 4, 2, 0), fit(10, 4, 2)) == \
        (2, 3, 3, 4, 5, 6, 1)
    assert lib.dm_cluster_rank(None, None, None, 3, 4, 4, None, None, 5, None, 0, 0, None, 0, None, None, None, None, None) == 2
    assert lib.dm_cluster_rank(None, None, None, 10, 4, 4, None, None, 2, None, 0, 0, None, 0, None, None, None, None, None) == 1
    assert set(range(1, 11)) == set(CL.ERRORS)


def test_device_entry_points_have_no_host_path():
    import torch
    for f in (CL.kmeans_fit, lambda x: CL.rank_clusters(x, None, None, None)):
        with pytest.raises(E.EngineError):
            f(torch.zeros(8, 4))
    from diff_mining_amd.typicality import TypicalityScorer
    assert callable(TypicalityScorer.cluster_patches) and callable(E.UNetEngine.kmeans_fit) and callable(E.UNetEngineF32.kmeans_fit)


def test_cluster_patches_on_host_arrays(gold):
    X, k = case_input(gold, "k32")
    labels = gold["k32_labels"]
    D, _ = KC.rank_inputs(labels, int(gold["k32_rank_d_seed"]))
    res = CL.cluster_patches(X, D, num_clusters=k)
    pre = "k32_rank_centroid_median_"
    assert np.array_equal(res["labels"], labels) and res["n_iter"] == int(gold["k32_n_iter"])
    assert len(res["clusters"]) == int(gold[pre + "n_nonempty"])
    off = gold[pre + "offsets"]
    for r, c in enumerate(res["clusters"]):
        assert c["cluster"] == gold[pre + "cluster_of_rank"][r] and c["aggregate"] == gold[pre + "aggregate"][r]
        assert np.array_equal(c["rows"], gold[pre + "order"][off[r]:off[r + 1]])
