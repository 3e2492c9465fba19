"""CPU tier of UMAP's initialisation on a disconnected graph (umapfit's disconnected='components'): the numpy restatement against scipy
and against itself.  Cases and measured figures: tests/umap_multi_cases.py.

  components  ids equal scipy's connected_components labels; the grouping permutation is the stable one; each component's sub-graph
              equals scipy's P[m][:, m] in CSR order; centroids equal the explicit ascending-order fp64 sum; count and sizes as listed.
  meta        the table for c = 2, 3, 2 dim; the affinity embedding finite with largest entry 1; every degenerate reason.
  rule        |R_i - meta[comp_i]|_inf <= range[comp_i], reached in each solved component; Y0 in [0, 10], finite, deterministic;
              connected graphs and `far6` give today's functions bit for bit.
  solver      with solver='iter' every component converges within the cap, Ritz values within 1e-11 of that component's eigh and
              eigenvectors within 2e-11 / gap (the bounds tests/test_umap_spectral.py derives).
  surface     umap_fit_host / compress / cluster_patches take the option; the default and project=None are unchanged."""
import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.csgraph import connected_components

from diff_mining_amd import clustering as CL
from diff_mining_amd import umapfit as U
from tests import umap_multi_cases as MC

CLOUDS = tuple(t for t in MC.MULTI if t in MC.CLOUDS) + ("far6", MC.STALL)     # the small cases: whole fits at few epochs


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _csr(tag):
    G = MC.graph(tag)
    n = len(MC.case(tag)[0])
    return sparse.csr_matrix((G["weight"], G["col"], G["row_ptr"]), shape=(n, n))


@pytest.mark.parametrize("tag", CLOUDS + ("blob1200",))
def test_components_against_scipy(tag):
    X, _, dim = MC.case(tag)
    G = MC.graph(tag)
    n = len(X)
    P = _csr(tag)
    c, label = connected_components(P, directed=False)
    g = U.component_groups_host(G["row_ptr"], G["col"], G["weight"], n, X)
    sizes = np.diff(g["offsets"])
    print(f"{tag}: {c} components, sizes {sorted(sizes.tolist())}")
    assert g["n_comp"] == c == U.components_host(G["row_ptr"], G["col"], n) and np.array_equal(g["comp"], label)
    assert sorted(sizes.tolist()) == MC.EXPECT[tag][0]
    assert np.array_equal(g["perm"], np.argsort(label, kind="stable")) and not np.array_equal(g["perm"], np.arange(n))
    for l in range(c):
        rows = g["perm"][g["offsets"][l]:g["offsets"][l + 1]]
        assert np.all(np.diff(rows) > 0) and np.all(label[rows] == l)
        want = P[label == l][:, label == l].tocsr()
        want.sort_indices()
        rp, cl, w, size = U.sub_graph(g, l)
        assert size == len(rows) and np.array_equal(rp, want.indptr) and np.array_equal(cl, want.indices)
        assert np.array_equal(_bits(w), _bits(want.data.astype(np.float32)))
        s = np.zeros(X.shape[1])
        for i in np.flatnonzero(label == l):
            s = s + X[i].astype(np.float64)
        assert np.array_equal(_bits(g["centroids"][l]), _bits(s / len(rows)))
    assert len(g["sub_row_ptr"]) == n + c and g["edge_offsets"][-1] == len(g["sub_col"]) == len(G["col"])


def test_meta_table():
    for c, dim in ((2, 2), (3, 2), (3, 5), (4, 2), (10, 5), (2, 1)):
        m = U.meta_embedding_host(None, c, dim)
        k = (c + 1) // 2
        base = np.hstack([np.eye(k), np.zeros((k, dim - k))])
        assert m["kind"] == "table" and m["reason"] is None and np.array_equal(m["meta"], np.vstack([base, -base])[:c])
        want = np.full(c, np.sqrt(2.0) / 2.0) if c > 2 else np.full(c, 1.0)
        if c == 3 and k == 2:                                         # e0, e1, -e0: every row's nearest is sqrt(2) away
            want = np.full(3, np.sqrt(2.0) / 2.0)
        assert np.allclose(m["range"], want, rtol=0, atol=1e-15)


def test_meta_affinity_and_degenerate_reasons():
    cent = np.random.RandomState(7).normal(size=(6, 3))
    m = U.meta_embedding_host(cent, 6, 2)
    assert m["kind"] == "affinity" and m["reason"] is None and m["meta"].shape == (6, 2)
    assert np.isfinite(m["meta"]).all() and m["meta"].max() == 1.0 and np.all(m["range"] > 0) and np.isfinite(m["range"]).all()
    again = U.meta_embedding_host(cent.copy(), 6, 2)
    assert np.array_equal(_bits(again["meta"]), _bits(m["meta"])) and np.array_equal(_bits(again["range"]), _bits(m["range"]))
    d = np.sqrt(((m["meta"][:, None] - m["meta"][None]) ** 2).sum(axis=2))
    assert np.allclose(m["range"], np.where(d > 0, d, np.inf).min(axis=1) / 2.0, rtol=0, atol=0)
    far = U.meta_embedding_host(cent * 200.0, 6, 2)                   # exp(-d^2) is exactly 0 everywhere
    assert (far["reason"], far["detail"]) == ("meta degenerate", "zero row sum") and "meta" not in far
    two = np.vstack([cent[:3], cent[3:] + 100.0])                     # two groups of centroids out of each other's reach
    assert U.meta_embedding_host(two, 6, 2)["detail"] == "disconnected"
    assert U.meta_range_host(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])) is None        # two coinciding rows
    assert U.meta_range_host(np.array([[1.0, 0.0], [-1.0, 0.0]])).tolist() == [1.0, 1.0]


def test_meta_coincident_rows(monkeypatch):
    """Two identical centroids have equal rows in every eigenvector below the top one, but LAPACK returns them equal to 1e-16 .. 1e-14,
    not to the bit (measured: six random sets of 3 and 5 centroids), and the rule asks for no positive distance.  So the helper is
    driven there with an eigen-decomposition that is symmetric to the bit: the true one with rows 0 and 1 averaged."""
    cent = np.random.RandomState(7).normal(size=(6, 3))
    cent[1] = cent[0]
    real = np.linalg.eigh
    near = U.meta_embedding_host(cent, 6, 2)
    assert near["reason"] is None and np.abs(near["meta"][0] - near["meta"][1]).max() < 1e-13 and near["range"][0] < 1e-13

    def symmetric(L):
        val, vec = real(L)
        vec[0] = vec[1] = 0.5 * (vec[0] + vec[1])
        return val, vec

    monkeypatch.setattr(np.linalg, "eigh", symmetric)
    m = U.meta_embedding_host(cent, 6, 2)
    assert (m["reason"], m["detail"]) == ("meta degenerate", "coincident rows") and "meta" not in m


@pytest.mark.parametrize("tag", MC.MULTI)
def test_rule(tag):
    X, _, dim = MC.case(tag)
    G = MC.graph(tag)
    Y0, used, info = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, MC.SEED, "host")
    sizes, kind, solved = MC.EXPECT[tag]
    assert used == "components" and info["meta_kind"] == kind and int(info["plan"].sum()) == solved and info["reason"] is None
    assert np.array_equal(info["plan"], U.multi_component_plan(info["sizes"], dim))
    assert [s == "uniform" for s in info["status"]] == [not p for p in info["plan"]]
    meta, comp = info["meta"], info["groups"]["comp"]
    dev = np.abs(info["R"] - meta["meta"][comp]).max(axis=1)
    # |meta| <= 1 and range <= 1: the product, the sum and this difference round once each, 2^-53 of a value below 2 at the most
    slack = 3 * 2.0 ** -52
    assert np.all(dev <= meta["range"][comp] + slack)
    for l in np.flatnonzero(info["plan"]):
        assert abs(dev[comp == l].max() - meta["range"][l]) <= slack
    assert Y0.dtype == np.float32 and np.isfinite(Y0).all() and Y0.min() == 0.0
    # `_rescale` forms 10 (y - lo) / (hi - lo) in fp32: at y = hi the product's rounding can leave the quotient one ulp past 10, as it
    # does for the spectral and random initialisations too
    assert 10.0 <= Y0.max() <= np.nextafter(np.float32(10), np.float32(11))
    again = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, MC.SEED, "host")[0]
    assert np.array_equal(_bits(again), _bits(Y0))


@pytest.mark.parametrize("tag", MC.CONNECTED + ("far6",))
def test_one_component_and_degenerate_are_todays_functions(tag):
    X, k, dim = MC.case(tag)
    n = len(X)
    idx, dist = U.knn_host(X, k)
    G = U.fuzzy_graph_host(idx, dist, 500)
    want_dense, used_dense = U.spectral_init_host(G["P"], dim, MC.SEED)
    want_iter, used_iter, _ = U.spectral_init_iter_host(G["row_ptr"], G["col"], G["weight"], n, dim, MC.SEED)
    got, used, info = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, MC.SEED, "host")
    assert used == used_dense and np.array_equal(_bits(got), _bits(want_dense))
    got, used, info = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, MC.SEED, "iter")
    assert used == used_iter and np.array_equal(_bits(got), _bits(want_iter))
    if tag == "far6":
        assert used == "random" and (info["reason"], info["detail"], info["n_comp"]) == ("meta degenerate", "zero row sum", 6)
    else:
        assert used == "spectral" and info["n_comp"] == 1 and info["reason"] is None
    for route in ("dense", "sparse") if tag != "blob300" else ():     # the whole fit, at the small cases (n_epochs prunes the graph: all 500)
        a = U.umap_fit_host(X, dim, k, MC.SEED, route=route)
        b = U.umap_fit_host(X, dim, k, MC.SEED, route=route, disconnected="components")
        assert a["init_used"] == b["init_used"] and np.array_equal(_bits(a["embedding"]), _bits(b["embedding"]))


def test_more_components_than_the_cap_is_random(monkeypatch):
    X, k, dim = MC.case("two")
    G = MC.graph("two")
    monkeypatch.setattr(U, "MULTI_MAX_COMP", 1)
    got, used, info = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, dim, MC.SEED)
    want = U.spectral_init_sparse_host(G["row_ptr"], G["col"], G["weight"], len(X), dim, MC.SEED)[0]
    assert used == "random" and "more than" in info["reason"] and np.array_equal(_bits(got), _bits(want))
    got, used, info = U.multi_component_init_host(G["row_ptr"], G["col"], G["weight"], X, len(X) - 1, MC.SEED)       # dim + 1 >= n
    assert used == "random" and info["reason"] == "n_components + 1 >= n"


@pytest.mark.parametrize("tag", MC.MULTI)
def test_iter_solver_per_component(tag):
    _, _, dim = MC.case(tag)
    _, used, info = MC.host_init(tag)
    gap = MC.min_gap(tag)
    print(f"{tag}: smallest gap {gap:.3e}; iterations {info['iters']}")
    assert used == "components" and gap >= MC.MIN_GAP, "the case does not make the comparison meaningful: change its seed"
    _, _, href = MC.host_init(tag, "host")
    assert np.array_equal(href["plan"], info["plan"])
    for l in np.flatnonzero(info["plan"]):
        assert info["status"][l] == "converged" and 1 <= info["iters"][l] <= MC.MAX_ITERS
        val_err, vec_ratio = MC.compare(info["groups"], l, dim, info["eigvals"], info["eigvecs"])
        print(f"  component {l} ({info['sizes'][l]} rows): |theta - eigh| {val_err:.2e}, eigenvector distance / bound {vec_ratio:.3f}")
        assert val_err <= MC.TOL and vec_ratio <= 1.0


def test_a_component_the_iterative_solver_gives_up_on():
    """tests/umap_multi_cases.py's STALL: the restatement reports it per component, and the 'host' solver is not affected"""
    _, used, info = MC.host_init(MC.STALL)
    assert used == "components" and sorted(info["status"]) == ["converged", "not_converged"]
    assert info["iters"][info["status"].index("not_converged")] == 0 and info["sizes"][info["status"].index("not_converged")] == 9
    Y0, used, href = MC.host_init(MC.STALL, "host")
    assert used == "components" and href["status"] == ["converged", "converged"] and np.isfinite(Y0).all()


@pytest.mark.parametrize("tag", CLOUDS)
def test_fit_host_is_finite(tag):
    X, k, dim = MC.case(tag)
    epochs = 20 if tag == "wide" else 60
    fit = U.umap_fit_host(X, dim, k, MC.SEED, n_epochs=epochs, disconnected="components")
    assert np.isfinite(fit["embedding"]).all() and fit["init_used"] == ("random" if tag == "far6" else "components")
    assert fit["init_info"]["n_comp"] == len(MC.EXPECT[tag][0])
    base = U.umap_fit_host(X, dim, k, MC.SEED, n_epochs=epochs)
    assert base["init_used"] == "random" and "init_info" not in base
    assert np.array_equal(_bits(base["embedding"]), _bits(U.umap_fit_host(X, dim, k, MC.SEED, n_epochs=epochs, disconnected="random")["embedding"]))
    if tag != "far6":
        assert not np.array_equal(_bits(base["init"]), _bits(fit["init"]))


def test_the_option_passes_through():
    X, k, dim = MC.case("two")
    X6 = np.hstack([X, X])
    want = np.hstack([U.umap_fit_host(X6[:, i:i + 3], dim, k, MC.SEED, 30, disconnected="components")["embedding"] for i in (0, 3)])
    got = U.compress(X6, 2, dim, k, MC.SEED, 30, disconnected="components")
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(U.compress(X6, 2, dim, k, MC.SEED, 30)))
    assert np.array_equal(_bits(U.compress(X6, 2, dim, k, MC.SEED, 30)), _bits(U.compress(X6, 2, dim, k, MC.SEED, 30, disconnected="random")))
    Xb = X                                                            # 40 + 20 rows: two components at the default k = 15 too
    D = np.random.RandomState(0).rand(len(Xb)).astype(np.float32)
    res = CL.cluster_patches(Xb, D, num_clusters=3, project=2, project_seed=MC.SEED, project_disconnected="components")
    assert np.isfinite(res["embedding"]).all() and len(res["clusters"]) == 3
    plain = CL.cluster_patches(Xb, D, num_clusters=3, project=None, project_disconnected="components")
    assert "embedding" not in plain and np.array_equal(plain["labels"], CL.cluster_patches(Xb, D, num_clusters=3)["labels"])
    from diff_mining_amd.typicality import TypicalityScorer
    Xg = X6
    on, off = U.compress(Xg, 2, 2, seed=MC.SEED, disconnected="components"), U.compress(Xg, 2, 2, seed=MC.SEED)
    assert not np.array_equal(_bits(on), _bits(off))
    via = TypicalityScorer.cluster_patches(Xb, D, num_clusters=3, project=2, project_seed=MC.SEED, project_disconnected="components")
    assert np.array_equal(_bits(via["embedding"]), _bits(res["embedding"]))
    for fn in (CL.cluster_patches, TypicalityScorer.cluster_patches):
        grouped = fn(Xg, D, num_clusters=3, project=("groups", 2, 2), project_seed=MC.SEED, project_disconnected="components")
        assert np.array_equal(_bits(grouped["embedding"]), _bits(on))
    for bad in ("component", None, "spectral"):
        with pytest.raises(ValueError):
            U.umap_fit_host(X, dim, k, disconnected=bad)
        with pytest.raises(ValueError):
            U.compress(X6, 2, dim, k, disconnected=bad)
    with pytest.raises(ValueError):
        U.multi_component_init_host(*[MC.graph("two")[q] for q in ("row_ptr", "col", "weight")], X, dim, solver="device")


def test_recorded_figures_describe_the_cases():
    """GAPS and the blob1200 / wide quality figures of tests/umap_multi_cases.py (measured with its __main__) against a fresh run of
    the restatement at SEED"""
    for tag in MC.MULTI:
        assert np.isclose(MC.min_gap(tag), MC.GAPS[tag], rtol=0.05), tag
    X, k, dim = MC.case("blob1200")
    for arm in U.DISCONNECTED:
        fit = U.umap_fit_host(X, dim, k, MC.SEED, disconnected=arm)
        t, s = MC.trust(X, fit["embedding"]), MC.spearman(X, fit["embedding"])
        print(f"blob1200 {arm}: init {fit['init_used']}, trustworthiness {t:.4f} (recorded {MC.HOST_TRUST['blob1200'][arm]:.4f}), "
              f"Spearman {s:.4f} (recorded {MC.HOST_SPEARMAN['blob1200'][arm]:.4f})")
        assert fit["init_used"] == arm
        assert abs(t - MC.HOST_TRUST["blob1200"][arm]) <= 5e-4 + MC.HOST_TRUST_SPREAD["blob1200"][arm]
        assert abs(s - MC.HOST_SPEARMAN["blob1200"][arm]) <= 5e-3 + MC.HOST_SPEARMAN_SPREAD["blob1200"][arm]
    # what the option is for: where the components sit relative to each other
    assert MC.HOST_SPEARMAN["blob1200"]["components"] - MC.HOST_SPEARMAN_SPREAD["blob1200"]["components"] > \
        MC.HOST_SPEARMAN["blob1200"]["random"] + MC.HOST_SPEARMAN_SPREAD["blob1200"]["random"]
