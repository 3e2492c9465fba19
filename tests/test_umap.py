"""CPU tier of the UMAP projection: the numpy restatement of diff-mining_amd/umapfit.py against its own rules, on the cases of
tests/umap_cases.py.  The restatement's parity with umap-learn is unpinned: test_matches_umap_learn reads tests/golden/umap_ref.npz
(tests/make_golden_umap.py) and skips until that file is committed."""
import os

import numpy as np
import pytest

from diff_mining_amd import clustering as CL
from diff_mining_amd import umapfit as UM
from tests import kmeans_cases as KC
from tests import umap_cases as UC
from tests.test_kmeans import case_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "umap_ref.npz")
GRAPH_TAGS = list(UC.SHAPES)


@pytest.fixture(scope="module")
def graphs():
    """per case: kNN and the float64 graph, computed once and left unchanged"""
    out = {}
    for tag in GRAPH_TAGS:
        X, k, dim, _ = UC.case(tag)
        idx, dist = UM.knn_host(X, k)
        out[tag] = (X, k, dim, idx, dist, UM.fuzzy_graph_host(idx, dist, 500))
    return out


@pytest.fixture(scope="module")
def blob_fits():
    out = {}
    for tag in UC.BLOBS:
        X, k, dim, label = UC.case(tag)
        out[tag] = (X, label, UM.umap_fit_host(X, dim, k, UC.SEED))
    return out


def test_curve_parameters():
    a, b = UM.find_ab_params()
    assert abs(a - 1.5769) < 1e-3 and abs(b - 0.8951) < 1e-3


def test_knn_rule_on_a_small_case():
    """against the definition, pair by pair: the fp64 sum in ascending feature order, sqrt, fp32; stable order"""
    X, k, _, _ = UC.case("dup")
    idx, dist = UM.knn_host(X, k)
    n, d = X.shape
    full = np.zeros((n, n), np.float32)
    for i in range(n):
        for j in range(n):
            s = 0.0
            for e in range(d):
                diff = float(X[i, e]) - float(X[j, e])
                s = s + diff * diff
            full[i, j] = np.float32(np.sqrt(s))
    for i in range(n):
        order = sorted(range(n), key=lambda j: (full[i, j], j))[:k]
        assert idx[i].tolist() == order and np.array_equal(dist[i], full[i, order])
    assert idx[7].tolist()[:2] == [7, 8] and idx[8].tolist()[:2] == [7, 8]        # ties to the lower index: self is not always first


@pytest.mark.parametrize("tag", GRAPH_TAGS)
def test_sigma_satisfies_its_equation(graphs, tag):
    """sum_{j >= 1} (x_ij > 0 ? exp(-x_ij / sigma_i) : 1) = log2(k) to 1e-5 at the bisection's float64 sigma.  The stored sigma is
    that value rounded to fp32: |d sigma| <= 2^-24 sigma.  With t = x / sigma a term's derivative in sigma is t exp(-t) / sigma <=
    1 / (e sigma), so the k - 1 terms move the sum by at most (k - 1) / e x 2^-24 (x (1 + 2^-23) for the second order)."""
    _, k, _, _, dist, G = graphs[tag]
    rho, sigma = G["rho"].astype(np.float64), G["sigma"].astype(np.float64)
    x = dist[:, 1:].astype(np.float64) - rho[:, None]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        psum = np.where(x > 0, np.exp(-(x / sigma[:, None])), 1.0).sum(axis=1)
    storage = (k - 1) / np.e * 2.0 ** -24 * (1 + 2.0 ** -23)
    err = np.abs(psum - np.log2(k))[~G["exempt"]]
    print(f"{tag}: {int(G['exempt'].sum())} exempt rows, worst {err.max() if len(err) else 0:.3e}, bound {1e-5 + storage:.3e}")
    # exempt (the floor or the step cap decided): only in "dup", the seven copies and the row whose four neighbours are copies at one distance
    assert int(G["exempt"].sum()) == (8 if tag == "dup" else 0)
    assert (err < 1e-5 + storage).all()


def test_duplicate_rows(graphs):
    X, k, _, idx, dist, G = graphs["dup"]
    rho, sigma, P = G["rho"], G["sigma"], G["P"]
    assert (rho[:7] == 0).all() and G["exempt"][:7].all()             # seven copies, k = 5: every neighbour at distance 0
    assert np.allclose(sigma[:7], 1e-3 * dist.astype(np.float64).mean(), rtol=1e-6)       # the global floor
    for i, j in ((7, 8), (9, 10)):
        assert dist[i, 1] == 0 and rho[i] > 0 and rho[i] == dist[i][dist[i] > 0].min()    # rho skips the zero
        assert P[i, j] == 1 and P[j, i] == 1
    for i in range(7):
        members = [j for j in idx[i] if j != i]
        assert all(j < 7 for j in members) and all(P[i, j] == 1 for j in members)
    assert (np.diag(P) == 0).all()


@pytest.mark.parametrize("tag", GRAPH_TAGS)
def test_graph_and_edge_list(graphs, tag):
    _, _, _, _, _, G = graphs[tag]
    P, row_ptr, col, w = G["P"], G["row_ptr"], G["col"], G["weight"]
    assert np.array_equal(P, P.T) and P.min() >= 0 and P.max() <= 1
    rows = np.repeat(np.arange(len(P)), np.diff(row_ptr))
    flat = rows.astype(np.int64) * len(P) + col
    assert (np.diff(flat) > 0).all()                                    # row-major, ascending column, no repeats
    assert len(col) == np.count_nonzero(P) and np.array_equal(P[rows, col], w)
    assert w.min() >= G["threshold"] and G["threshold"] == np.float32(P.max() / np.float32(500))


@pytest.mark.parametrize("tag", GRAPH_TAGS)
def test_recorded_bounds_describe_the_case(graphs, tag):
    """What the GPU tier relies on: fp32 and float64 give the same edge structure, and no weight of the unpruned union lies within
    4 x the recorded fp32 weight error of the pruning threshold.  (The fp32 errors themselves are printed, not asserted: numpy's fp32
    exp is not the same code on every CPU.)"""
    _, _, _, idx, dist, G = graphs[tag]
    G32 = UM.fuzzy_graph_host(idx, dist, 500, np.float32)
    bound = UC.BOUNDS[tag]
    assert np.array_equal(G32["row_ptr"], G["row_ptr"]) and np.array_equal(G32["col"], G["col"])
    sig = float(np.abs(G["sigma"].astype(np.float64) - G32["sigma"]).max())
    wgt = float(np.abs(G["weight"].astype(np.float64) - G32["weight"]).max())
    gap = UC.threshold_gap(idx, dist, G)
    print(f"{tag}: sigma {sig:.3e} weight {wgt:.3e} gap {gap:.3e}")
    assert gap > 4 * bound["weight"] and gap >= bound["gap"] * 0.999


@pytest.mark.parametrize("tag", ["n65", "blob300"])
def test_schedule_activation_counts(graphs, tag):
    _, _, dim, _, _, G = graphs[tag]
    w = G["weight"]
    counts = np.zeros(len(w), np.int64)
    Y0 = np.random.RandomState(0).uniform(0, 10, size=(len(G["P"]), dim)).astype(np.float32)
    UM.layout_host(G["row_ptr"], G["col"], w, Y0, 1.5769, 0.8951, 500, UC.SEED, counts=counts)
    want = np.floor(500.0 * w.astype(np.float64) / float(w.max()))
    assert np.abs(counts - want).max() <= 1
    assert counts.max() == 499                                         # epoch 0 moves nothing: next_e starts at eps_e >= 1


def test_layout_is_deterministic_and_finite(graphs):
    _, _, dim, _, _, G = graphs["n130"]
    Y0, used = UM.spectral_init_host(G["P"], dim, UC.SEED)
    runs = [UM.layout_host(G["row_ptr"], G["col"], G["weight"], Y0, 1.5769, 0.8951, 500, UC.SEED, 0, 40)[0] for _ in range(2)]
    assert used == "spectral" and np.isfinite(runs[0]).all() and np.array_equal(runs[0], runs[1])
    # epoch by epoch with the schedule handed on: the same bits
    Y, sched = Y0, None
    for ep in range(6):
        Y, sched = UM.layout_host(G["row_ptr"], G["col"], G["weight"], Y, 1.5769, 0.8951, 500, UC.SEED, ep, ep + 1, schedule=sched)
    assert np.array_equal(Y, UM.layout_host(G["row_ptr"], G["col"], G["weight"], Y0, 1.5769, 0.8951, 500, UC.SEED, 0, 6)[0])
    other = UM.layout_host(G["row_ptr"], G["col"], G["weight"], Y0, 1.5769, 0.8951, 500, UC.SEED + 1, 0, 6)[0]
    assert not np.array_equal(Y, other)                                # the seed reaches the repulsive draws


def test_hash_is_the_documented_mix():
    def mix(h):
        h ^= h >> 16
        h = (h * 0x7FEB352D) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x846CA68B) & 0xFFFFFFFF
        return h ^ (h >> 16)
    for seed, ep, e, p in ((42, 0, 0, 0), (42, 499, 123456, 4), (7, 3, 2 ** 20 + 5, 2499)):
        h = mix(seed ^ ((ep * 0x9E3779B9) & 0xFFFFFFFF))
        h = mix(h ^ ((e * 0x85EBCA6B) & 0xFFFFFFFF))
        h = mix(h ^ ((p * 0xC2B2AE35) & 0xFFFFFFFF))
        assert int(UM.hash_host(seed, ep, np.array([e]), p)[0]) == h
    draws = UM.hash_host(42, 5, np.arange(20000), 1) % np.uint64(10)
    assert np.bincount(draws.astype(np.int64), minlength=10).min() > 1800


def test_disconnected_input_reports_the_random_initialisation(graphs):
    X, k, dim, _, _, G = graphs["split"]
    assert (G["P"][:30, 30:] == 0).all()
    Y0, used = UM.spectral_init_host(G["P"], dim, UC.SEED)
    assert used == "random" and Y0.min() == 0 and Y0.max() == 10
    fit = UM.umap_fit_host(X, dim, k, UC.SEED, n_epochs=20)
    assert fit["init_used"] == "random" and np.isfinite(fit["embedding"]).all()
    assert UM.spectral_init_host(graphs["n17"][5]["P"], 16, UC.SEED)[1] == "random"        # dim + 1 >= n


@pytest.mark.parametrize("tag", list(UC.BLOBS))
def test_blobs_optimise(blob_fits, tag):
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score
    X, label, fit = blob_fits[tag]
    t0, t1 = UC.trust(X, fit["init"]), UC.trust(X, fit["embedding"])
    ari = adjusted_rand_score(label, KMeans(int(label.max()) + 1, random_state=10).fit_predict(fit["embedding"]))
    print(f"{tag}: trustworthiness {t0:.4f} -> {t1:.4f}, ARI {ari}, {fit['n_edges']} edges")
    assert fit["init_used"] == "spectral" and t1 >= t0 and ari == 1.0
    assert abs(t1 - UC.HOST_TRUST[tag]) <= UC.HOST_TRUST_SPREAD[tag]                  # the figure the GPU tier compares with


def test_compress_is_the_per_group_loop():
    X, _, _, _ = UC.case("n65")
    X = np.hstack([X, X[::-1] * 2])[:, :65]                              # 65 features in 2 groups of 32: a one-feature tail block
    got = UM.compress(X, 2, 3, 5, seed=UC.SEED, n_epochs=30)
    parts = [UM.umap_fit_host(X[:, i:i + 32], 3, 5, UC.SEED, 30)["embedding"] for i in (0, 32, 64)]
    assert got.shape == (65, 9) and np.array_equal(got, np.hstack(parts))


@pytest.mark.parametrize("tag", ["long257", "long300"])
def test_cluster_patches_without_project_is_unchanged(tag):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "kmeans_ref.npz"))
    X, k = case_input(gold, tag)
    D = KC.typicality(len(X), 5)
    plain, none = CL.cluster_patches(X, D, num_clusters=k), CL.cluster_patches(X, D, num_clusters=k, project=None, project_seed=1)
    assert set(plain) == set(none) == {"clusters", "labels", "centers", "seed_index", "inertia", "n_iter"}
    assert np.array_equal(none["labels"], gold[f"{tag}_labels"])
    labels, centers, seeds, inertia, n_iter = CL.kmeans_fit_host(X, k)
    order, cor, off, agg, nn = CL.rank_clusters_host(X, labels, centers, D)
    for res in (plain, none):
        assert np.array_equal(res["labels"], labels) and np.array_equal(res["centers"].view(np.int32), centers.view(np.int32))
        assert np.array_equal(res["seed_index"], seeds) and res["inertia"] == inertia and res["n_iter"] == n_iter
        assert len(res["clusters"]) == nn
        for r, c in enumerate(res["clusters"]):
            assert c["cluster"] == cor[r] and c["aggregate"] == float(agg[r]) and np.array_equal(c["rows"], order[off[r]:off[r + 1]])


def test_cluster_patches_projects_on_the_host():
    from sklearn.metrics import adjusted_rand_score
    X, k, dim, label = UC.case("blob300")
    D = KC.typicality(len(X), 5)
    res = CL.cluster_patches(X, D, num_clusters=6, project=5, project_seed=UC.SEED)
    assert res["embedding"].shape == (300, 5) and adjusted_rand_score(label, res["labels"]) == 1.0
    with pytest.raises(ValueError):
        CL.cluster_patches(X, D, num_clusters=6, project=("blocks", 2, 5))


def test_refusals_on_the_host():
    X = np.zeros((20, 3), np.float32)
    for args in ((np.zeros((4096, 1), np.float32), 2, 5), (X, 2, 20), (X, 2, 65), (X, 2, 1), (X, 65, 5), (X, 0, 5)):
        with pytest.raises(ValueError):
            UM.umap_fit_host(*args)


def test_matches_umap_learn(graphs):
    """umap-learn's own kNN, rho, sigma, graph, a and b on the cases the fixture holds (tests/make_golden_umap.py)."""
    if not os.path.exists(GOLD):
        pytest.skip("tests/golden/umap_ref.npz is not committed yet: UMAP parity with umap-learn unpinned (README)")
    z = np.load(GOLD)
    a, b = UM.find_ab_params()
    assert abs(a - float(z["a"])) < 1e-6 and abs(b - float(z["b"])) < 1e-6
    for tag in [str(t) for t in z["tags"]]:
        X, k, _, idx, dist, G = graphs[tag]
        assert np.array_equal(X, z[f"{tag}_X"])
        assert np.array_equal(np.sort(dist, axis=1), np.sort(z[f"{tag}_knn_dist"], axis=1).astype(np.float32))
        np.testing.assert_allclose(G["rho"], z[f"{tag}_rho"], rtol=1e-6)
        np.testing.assert_allclose(G["sigma"], z[f"{tag}_sigma"], rtol=1e-5)
        np.testing.assert_allclose(G["P"], z[f"{tag}_graph"], atol=1e-5)
