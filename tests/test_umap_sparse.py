"""The numpy restatement's sparse route (diff-mining_amd/umapfit.py, route='sparse') on the CPU: on every case both routes take it
gives the dense route's bits; it runs past 4095 rows; `spectral_init_sparse_host` finds `spectral_init_host`'s eigenpairs; `compress`
picks it by itself; and the default call still refuses 4096 rows."""
import numpy as np
import pytest

from diff_mining_amd import umapfit as UM
from tests import umap_cases as UC
from tests import umap_sparse_cases as XC
from tests import umap_spectral_cases as SC

ALL = list(UC.SHAPES)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tag", ALL)
def test_sparse_route_equals_dense_route(tag):
    X, k, dim, _ = UC.case(tag)
    dense, sparse = UM.knn_host(X, k), UM.knn_host(X, k, route="sparse")
    assert _same(dense[0], sparse[0]) and _same(dense[1], sparse[1])
    for dtype in (np.float64, np.float32):
        Gd, Gs = UM.fuzzy_graph_host(*dense, 500, dtype), UM.fuzzy_graph_host(*sparse, 500, dtype, route="sparse")
        for name in ("rho", "sigma", "row_ptr", "col", "weight"):
            assert _same(Gd[name], Gs[name]), name
        assert _same(Gd["threshold"], Gs["threshold"]) and "P" not in Gs


@pytest.mark.parametrize("tag", ALL)
def test_sparse_fit_equals_dense_fit(tag):
    X, k, dim, _ = UC.case(tag)
    fd = UM.umap_fit_host(X, dim, k, UC.SEED, n_epochs=20)
    fs = UM.umap_fit_host(X, dim, k, UC.SEED, n_epochs=20, route="sparse")
    assert (fd["init_used"], fd["n_edges"]) == (fs["init_used"], fs["n_edges"]) and (fd["route"], fs["route"]) == ("dense", "sparse")
    assert _same(fd["init"], fs["init"]) and _same(fd["embedding"], fs["embedding"])


def test_runs_past_the_dense_limit():
    X = UC.cloud(4200, 3, 7)
    fit = UM.umap_fit_host(X, 2, 15, UC.SEED, n_epochs=20, route="sparse")
    assert fit["embedding"].shape == (4200, 2) and np.isfinite(fit["embedding"]).all() and fit["route"] == "sparse"
    assert fit["init_used"] == "spectral"
    assert _same(fit["embedding"], UM.umap_fit_host(X, 2, 15, UC.SEED, n_epochs=20, route="sparse")["embedding"])


@pytest.mark.parametrize("tag", ["n65", "n130", "n300", "dup", "blob400", "cloud1000"])
def test_sparse_host_solver_against_eigh(tag):
    """eigsh forced at small n (dense_below=0) against the dense eigh: Weyl and Davis-Kahan as tests/umap_spectral_cases.py states them"""
    c = SC.case(tag)
    G, n, dim = c["G"], c["n"], c["dim"]
    gap, lead = SC.preconditions(tag)
    assert gap >= SC.MIN_GAP and lead >= SC.MIN_LEAD
    Y0, used, info = UM.spectral_init_sparse_host(G["row_ptr"], G["col"], G["weight"], n, dim, UC.SEED, dense_below=0)
    want, want_used = UM.spectral_init_host(G["P"], dim, UC.SEED)
    val_err, vec_ratio = SC.compare(tag, info["eigvals"], info["eigvecs"])
    print(f"{tag}: {info['solver']}: |theta - eigh| {val_err:.2e}, eigenvector distance / bound {vec_ratio:.3f}, "
          f"max |Y0 - spectral_init_host's| {np.abs(Y0 - want).max():.2e}")
    assert used == want_used == "spectral" and info["n_comp"] == 1 and info["solver"] == "eigsh"
    assert val_err <= 1e-10
    assert vec_ratio <= 1.0
    assert _same(Y0, SC.tail(tag, info["eigvecs"]))
    # below the dense limit the default is the rule's own eigh: spectral_init_host's bits
    Y0d, _, infod = UM.spectral_init_sparse_host(G["row_ptr"], G["col"], G["weight"], n, dim, UC.SEED)
    assert infod["solver"] == "eigh" and _same(Y0d, want)


def test_random_fallback_and_small_n():
    c = SC.case("split")
    G = c["G"]
    Y0, used, info = UM.spectral_init_sparse_host(G["row_ptr"], G["col"], G["weight"], c["n"], c["dim"], UC.SEED)
    want, want_used = UM.spectral_init_host(G["P"], c["dim"], UC.SEED)
    assert used == want_used == "random" and info["n_comp"] == 2 and _same(Y0, want)


def test_compress_picks_the_route_and_the_default_still_refuses(monkeypatch):
    seen = []
    real = UM.umap_fit_host

    def spy(X, *args, **kw):
        seen.append((len(X), kw.get("route")))
        return {"embedding": np.zeros((len(X), args[0]), np.float32)} if len(X) >= UM.UMAP_MAX_N else real(X, *args, **kw)

    monkeypatch.setattr(UM, "umap_fit_host", spy)
    out = UM.compress(UC.cloud(4200, 6, 1), 2, 2, n_epochs=5)
    assert out.shape == (4200, 4) and seen == [(4200, "sparse"), (4200, "sparse")]
    del seen[:]
    UM.compress(UC.cloud(40, 6, 1), 2, 2, n_neighbors=5, n_epochs=5)
    assert seen == [(40, "dense"), (40, "dense")]
    monkeypatch.undo()
    X = UC.cloud(4096, 3, 1)
    with pytest.raises(ValueError):
        UM.umap_fit_host(X, 2)
    with pytest.raises(ValueError):
        UM.knn_host(X, 15)
    with pytest.raises(ValueError):
        UM.knn_host(np.zeros((65536, 1), np.float32), 15, route="sparse")
    with pytest.raises(ValueError):
        UM.pick_route("tiled", 10)
    assert (UM.pick_route("auto", 4095), UM.pick_route("auto", 4096), UM.pick_route("sparse", 10)) == ("dense", "sparse", "sparse")


def test_bounds_describe_the_big_cases():
    """the pasted figures are there for every big case, and no weight lies within the weight bound of the threshold where the GPU test
    asserts the edge structure"""
    for tag in XC.BIG:
        assert tag in XC.BOUNDS, "run python -m tests.umap_sparse_cases and paste its output"
    b = XC.BOUNDS
    assert (b["big3"]["edges"], b["big3"]["n_comp"], b["hub4096"]["edges"], b["hub4096"]["row"], b["hub4096"]["n_comp"]) == (70934, 1, 40930, 4095, 1)
    assert b["big3"]["gap"] > XC.MARGIN * b["big3"]["weight"] and b["hub4096"]["gap"] > XC.MARGIN * b["hub4096"]["weight"]
    assert b["big3"]["eig_gap"] >= XC.MIN_GAP and b["big16"]["eig_gap"] >= XC.MIN_GAP
