"""The UMAP route without the n x n graph (dm_umap_sparse_*; csrc/umap_sparse.hip) on the GPU.

  equal     on every case both routes take (tests/umap_sparse_cases.EQUAL), route='sparse' gives route='dense''s bits: kNN, graph, three
            moving epochs of the layout, the spectral initialisation, the whole fit with the device's solver.
  big       past 4095 rows, against the numpy restatement's sparse route (big3, big16, hub4096): kNN and rho bit-equal; sigma and the
            weights within 4 x the restatement's own fp32-to-float64 distance (umap_sparse_cases.BOUNDS, measured on the CPU); the
            edge structure bit-equal where the case's threshold gap exceeds 4 x its weight bound; one and three moving epochs within
            4 x the restatement's distance; the device's initialisation against the restatement's and a dense eigh.
  product   cluster_patches(project=('groups', 2, 2)) on 4200 rows: it raised before this route existed.
  refusals  every new entry returns its code without a launch.
Each case prints its figures before it asserts (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import clustering as CL
from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import umap_cases as UC
from tests import umap_sparse_cases as XC

pytestmark = pytest.mark.gpu
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
MARGIN = XC.MARGIN


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int64) if t.dtype == F64 else t


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def ab():
    return UM.find_ab_params()


# ---- 1. equal to the dense route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", XC.EQUAL)
def test_sparse_route_equals_dense_route(ab, tag):
    X, k, dim = XC.case(tag)
    a, b = ab
    Xd = _dev(X)
    n = len(X)
    kd, ks = UM.knn(Xd, k, route="dense"), UM.knn(Xd, k, route="sparse")
    assert _eq(kd[0], ks[0]) and _eq(kd[1], ks[1]), "kNN"
    Gd, Gs = UM.fuzzy_graph(*kd, 500, route="dense"), UM.fuzzy_graph(*kd, 500, route="sparse")
    ne = int(Gd["n_edges"])
    rows = int(torch.diff(Gs["row_ptr"]).max())
    print(f"{tag}: n {n}, k {k}: {ne} edges (sparse route {int(Gs['n_edges'])}), largest row {rows}")
    assert int(Gs["n_edges"]) == ne and "P" not in Gs
    for name in ("rho", "sigma", "row_ptr"):
        assert _eq(Gd[name], Gs[name]), name
    assert _eq(Gd["col"][:ne], Gs["col"][:ne]) and _eq(Gd["weight"][:ne], Gs["weight"][:ne])
    Y0 = _dev(np.random.RandomState(1).uniform(0, 10, size=(n, dim)).astype(np.float32))
    last = UC.moving_epochs(3)
    Ld = UM.layout(Gd["row_ptr"], Gd["col"], Gd["weight"], ne, Y0, a, b, 500, UC.SEED, 0, last, n_neighbors=k, route="dense")
    Ls = UM.layout(Gd["row_ptr"], Gd["col"], Gd["weight"], ne, Y0, a, b, 500, UC.SEED, 0, last, n_neighbors=k, route="sparse")
    assert _eq(Ld, Ls) and not _eq(Ld, Y0), "layout"
    Sd = UM.spectral_init(Gd, dim, UC.SEED, return_vectors=True, route="dense")
    Ss = UM.spectral_init(Gd, dim, UC.SEED, return_vectors=True, route="sparse")
    st = UM.spectral_status(Ss["status"].cpu().numpy())
    print(f"{tag}: initialisation {st['status']}, {st['n_comp']} component(s), {st['iters']} iterations")
    for name in ("status", "Y0", "eigvals", "eigvecs"):
        assert _eq(Sd[name], Ss[name]), f"spectral_init {name}"
    fd = UM.umap_fit(Xd, dim, k, UC.SEED, init_solver="device", route="dense")
    fs = UM.umap_fit(Xd, dim, k, UC.SEED, init_solver="device", route="sparse")
    assert (fd["route"], fs["route"]) == ("dense", "sparse") and UM.umap_fit(Xd, dim, k, UC.SEED)["route"] == "dense"
    assert (fd["init_used"], fd["n_edges"], fd["init_solver"], fd["init_iters"]) == (fs["init_used"], fs["n_edges"], fs["init_solver"], fs["init_iters"])
    assert _eq(fd["embedding"], fs["embedding"]), "fit"


# ---- 2. above the old limit -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """per big case: the device's kNN, and its graph of the restatement's kNN arrays; computed once"""
    out = {}
    for tag in XC.BIG:
        h = XC.host(tag)
        idx, dist = UM.knn(_dev(h["X"]), h["k"])                      # route='auto': sparse from 4096 rows
        out[tag] = {"idx": idx, "dist": dist, "G": UM.fuzzy_graph(_dev(h["idx"]), _dev(h["dist"]), 500)}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", list(XC.BIG))
def test_big_knn_and_graph_against_the_restatement(big, tag):
    h, d, bound = XC.host(tag), big[tag], XC.BOUNDS[tag]
    G, D = h["G"], d["G"]
    idx, dist = d["idx"].cpu().numpy(), d["dist"].cpu().numpy()
    print(f"{tag}: {np.sum(idx != h['idx'])} indices, {np.sum(dist.view(np.int32) != h['dist'].view(np.int32))} distances differ")
    assert np.array_equal(idx, h["idx"]) and np.array_equal(dist.view(np.int32), h["dist"].view(np.int32))
    ne = int(D["n_edges"])
    rho, sigma = D["rho"].cpu().numpy(), D["sigma"].cpu().numpy()
    row_ptr, col, weight = D["row_ptr"].cpu().numpy(), D["col"].cpu().numpy()[:ne], D["weight"].cpu().numpy()[:ne]
    sig_err = float(np.abs(sigma.astype(np.float64) - G["sigma"]).max())
    same = ne == len(G["col"]) and np.array_equal(row_ptr, G["row_ptr"]) and np.array_equal(col, G["col"])
    w_err = float(np.abs(weight.astype(np.float64) - G["weight"]).max()) if same else float("nan")
    promised = bound["gap"] > MARGIN * bound["weight"]
    print(f"{tag}: sigma err {sig_err:.3e} (bound {MARGIN * bound['sigma']:.3e}), weight err {w_err:.3e} (bound {MARGIN * bound['weight']:.3e}), "
          f"{ne} edges against {len(G['col'])}, largest row {int(np.diff(row_ptr).max())}; threshold gap {bound['gap']:.3e}: edge structure "
          f"{'asserted' if promised else 'not promised'}, {'equal' if same else 'differs'}")
    assert len(G["col"]) == bound["edges"] and int(np.diff(G["row_ptr"]).max()) == bound["row"]
    assert np.array_equal(rho.view(np.int32), G["rho"].view(np.int32))
    assert sig_err <= MARGIN * bound["sigma"]
    assert "P" not in D
    if promised:
        assert same, "edge structure"
    if same:
        assert w_err <= MARGIN * bound["weight"]
    if tag == "hub4096":                                               # all memberships are exactly 1: the whole list, bit for bit
        assert np.array_equal(weight.view(np.int32), G["weight"].view(np.int32))


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("tag", XC.SOLVED)
def test_big_layout_epochs_against_the_float64_restatement(ab, tag, count):
    h = XC.host(tag)
    G, last = h["G"], UC.moving_epochs(count)
    a, b = ab
    Y0 = XC.solve(tag)[0]
    want, _ = UM.layout_host(G["row_ptr"], G["col"], G["weight"], Y0, a, b, 500, UC.SEED, 0, last, np.float64)
    got = UM.layout(_dev(G["row_ptr"]), _dev(G["col"]), _dev(G["weight"]), len(G["col"]), _dev(Y0), a, b, 500, UC.SEED, 0, last, n_neighbors=h["k"])
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    moved = float(np.abs(want - Y0).max())
    print(f"{tag}: {count} moving epoch(s): err {err:.3e} (bound {MARGIN * XC.BOUNDS[tag][f'layout{count}']:.3e}), largest move {moved:.3e}")
    assert moved > 1e-3, "the epochs moved nothing"
    assert err <= MARGIN * XC.BOUNDS[tag][f"layout{count}"]


@pytest.mark.parametrize("tag", XC.SOLVED)
def test_big_initialisation_against_eigh_and_the_restatement(tag):
    h = XC.host(tag)
    G = h["G"]
    Y0h, used, info = XC.solve(tag)
    dev = {name: _dev(G[name]) for name in ("row_ptr", "col", "weight")}
    out = UM.spectral_init(dev, h["dim"], UC.SEED, return_vectors=True)
    d = {name: v.cpu().numpy() for name, v in out.items()}
    st = UM.spectral_status(d["status"])
    val_err, vec_ratio, gap = XC.compare(tag, d["eigvals"], d["eigvecs"])
    print(f"{tag}: block {st['block']}, {st['status']} after {st['iters']} iterations (restatement {info['iters']}), residual "
          f"{st['max_residual']:.2e}; smallest gap {gap:.2e}; |theta - eigh| {val_err:.2e}, eigenvector distance / bound {vec_ratio:.3f}")
    assert gap >= XC.MIN_GAP
    assert info["status"] == "converged" and info["iters"] == XC.BOUNDS[tag]["iters"]
    assert (st["status"], st["n_comp"], st["init_used"]) == (info["status"], info["n_comp"], used) == ("converged", 1, "spectral")
    assert abs(st["iters"] - info["iters"]) <= 1
    assert val_err <= XC.TOL
    assert vec_ratio <= 1.0
    assert np.array_equal(d["Y0"].view(np.int32), XC.tail(tag, d["eigvecs"]).view(np.int32)), "Y0 is not the numpy tail of the device's eigenvectors"


@pytest.mark.parametrize("tag", list(XC.BIG))
def test_big_fit_is_finite_and_reproducible(tag):
    h = XC.host(tag)
    Xd = _dev(h["X"])
    fit = UM.umap_fit(Xd, h["dim"], h["k"], UC.SEED, n_epochs=30, init_solver="device")
    again = UM.umap_fit(Xd, h["dim"], h["k"], UC.SEED, n_epochs=30, init_solver="device")
    print(f"{tag}: route {fit['route']}, {fit['n_edges']} edges, init {fit['init_used']} by {fit['init_solver']} in {fit['init_iters']} iterations")
    assert fit["route"] == "sparse" and bool(torch.isfinite(fit["embedding"]).all())
    assert _eq(fit["embedding"], again["embedding"]), "two runs differ"
    if tag == "hub4096":
        dev = UM.fuzzy_graph(*UM.knn(Xd, h["k"]), 500)
        st = UM.spectral_status(UM.spectral_init(dev, h["dim"], UC.SEED)["status"].cpu().numpy())
        assert st["n_comp"] == 1 == XC.BOUNDS[tag]["n_comp"]


# ---- 3. the product call ----------------------------------------------------------------------------------------------------------------------
def test_cluster_patches_above_the_dense_limit():
    from diff_mining_amd.typicality import TypicalityScorer
    X = _dev(UC.cloud(4200, 6, 7))
    D = _dev(np.random.RandomState(0).rand(4200).astype(np.float32))
    res = CL.cluster_patches(X, D, 6, project=("groups", 2, 2), project_seed=42)
    halves = [UM.umap_fit(X[:, i:i + 3], 2, 15, 42)["embedding"] for i in (0, 3)]
    assert _eq(res["embedding"], torch.cat(halves, dim=1))
    assert sorted(np.concatenate([c["rows"] for c in res["clusters"]]).tolist()) == list(range(4200))
    via = TypicalityScorer.cluster_patches(X, D, num_clusters=6, project=("groups", 2, 2), project_seed=42)
    assert _eq(via["embedding"], res["embedding"])


def test_engine_umap_fit_passes_the_route():
    """UNetEngine.umap_fit is a pass-through: its signature carries `route` to umapfit.umap_fit (an engine needs weights; the call is
    checked on a stand-in that has only what the method touches)"""
    class Stand:
        _torch = torch
        device = torch.device("cuda", torch.cuda.current_device())
    X = _dev(UC.cloud(4200, 3, 7))
    got = E.UNetEngine.umap_fit(Stand(), X, 2, 15, 42, 30)
    assert got["route"] == "sparse" and _eq(got["embedding"], UM.umap_fit(X, 2, 15, 42, 30)["embedding"])
    small = _dev(UC.cloud(300, 3, 7))
    assert E.UNetEngine.umap_fit(Stand(), small, 2, 15, 42, 30, route="sparse")["route"] == "sparse"
    with pytest.raises(E.EngineError):
        E.UNetEngine.umap_fit(Stand(), X, 2, 15, 42, 30, route="dense")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = E.load_library()
    n, d, k, dim = 20, 3, 5, 2
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = UM.workspace_bytes(n, d, k, dim, "sparse")
    sneed = UM.spectral_workspace_bytes(n, dim, "sparse")
    t = {"X": torch.zeros(n, d, device="cuda"), "idx": torch.full((n, k), -7, dtype=I32, device="cuda"),
         "dist": torch.full((n, k), -7.0, device="cuda"), "rho": torch.full((n,), -7.0, device="cuda"),
         "sigma": torch.full((n,), -7.0, device="cuda"), "row_ptr": torch.full((n + 1,), -7, dtype=I32, device="cuda"),
         "col": torch.full((2 * n * k,), -7, dtype=I32, device="cuda"), "weight": torch.full((2 * n * k,), -7.0, device="cuda"),
         "n_edges": torch.full((1,), -7, dtype=I32, device="cuda"), "Y": torch.full((n, dim), -7.0, device="cuda"),
         "work": torch.full((max(need, sneed),), 0xF9, dtype=U8, device="cuda"), "noise": torch.zeros(n, dim, device="cuda"),
         "fallback": torch.zeros(n, dim, device="cuda"), "Y0": torch.full((n, dim), -7.0, device="cuda"),
         "eigvals": torch.full((dim + 1,), -7.0, dtype=F64, device="cuda"), "eigvecs": torch.full((n, dim + 1), -7.0, dtype=F64, device="cuda"),
         "status": torch.full((8,), -7.0, dtype=F64, device="cuda")}
    before = {name: v.clone() for name, v in t.items()}
    p = lambda name: None if name is None else C.c_void_p(t[name].data_ptr())        # noqa: E731
    BIG_N = 65536

    def knn(X="X", n=n, d=d, k=k, work="work", wb=need, idx="idx", dist="dist"):
        return lib.dm_umap_sparse_knn(s, p(X), n, d, k, p(work), wb, p(idx), p(dist))

    def graph(idx="idx", dist="dist", n=n, k=k, ne=500, work="work", wb=need, rho="rho", n_edges="n_edges", col="col"):
        return lib.dm_umap_sparse_graph(s, p(idx), p(dist), n, k, ne, p(work), wb, p(rho), p("sigma"), p("row_ptr"), p(col), p("weight"), p(n_edges))

    def layout(row_ptr="row_ptr", n=n, ne=10, dim=dim, epochs=500, first=0, last=2, Y="Y", work="work", wb=need):
        return lib.dm_umap_sparse_layout(s, p(row_ptr), p("col"), p("weight"), n, ne, dim, 1.5, 0.9, epochs, 1, first, last, p(Y), p(work), wb)

    def solve(row_ptr="row_ptr", col="col", weight="weight", n=n, dim=dim, noise="noise", fallback="fallback", work="work", wb=sneed, Y0="Y0",
              eigvals="eigvals", status="status"):
        return lib.dm_umap_sparse_spectral(s, p(row_ptr), p(col), p(weight), n, dim, 1, p(noise), p(fallback), p(work), wb, p(Y0), p(eigvals),
                                           p("eigvecs"), p(status))

    out = C.c_size_t(123)
    assert lib.dm_umap_sparse_workspace_bytes(n, d, k, dim, None) == 1
    assert [lib.dm_umap_sparse_workspace_bytes(*a, C.byref(out)) for a in ((BIG_N, d, k, dim), (5, d, 5, dim), (100, d, 65, dim), (100, d, 1, dim),
                                                                           (n, d, k, 65), (n, d, k, 0), (n, 0, k, dim))] == [2, 3, 4, 4, 5, 5, 6]
    assert lib.dm_umap_sparse_spectral_workspace_bytes(n, dim, None) == 1
    assert [lib.dm_umap_sparse_spectral_workspace_bytes(*a, C.byref(out)) for a in ((BIG_N, dim), (0, dim), (n, 65), (n, 0))] == [2, 3, 5, 5]
    assert out.value == 123
    assert lib.dm_umap_sparse_workspace_bytes(4096, d, k, dim, C.byref(out)) == 0 and out.value > 0       # past the dense limit
    assert [knn(X=None), knn(idx=None), knn(dist=None), knn(work=None), knn(n=BIG_N), knn(n=5), knn(n=100, k=65), knn(n=100, k=1), knn(d=0),
            knn(wb=need // 2)] == [1, 1, 1, 1, 2, 3, 4, 4, 6, 8]
    assert [graph(idx=None), graph(dist=None), graph(work=None), graph(rho=None), graph(col=None), graph(n_edges=None), graph(n=BIG_N), graph(n=5),
            graph(n=100, k=65), graph(ne=0), graph(wb=64)] == [1, 1, 1, 1, 1, 1, 2, 3, 4, 7, 8]
    assert [layout(row_ptr=None), layout(Y=None), layout(work=None), layout(n=BIG_N), layout(n=0), layout(dim=65), layout(dim=0),
            layout(first=3, last=2), layout(last=501), layout(first=-1), layout(epochs=0), layout(ne=-1), layout(ne=2 * n * 64 + 1),
            layout(wb=16)] == [1, 1, 1, 2, 3, 5, 5, 7, 7, 7, 7, 9, 9, 8]
    assert [solve(row_ptr=None), solve(col=None), solve(weight=None), solve(noise=None), solve(fallback=None), solve(work=None), solve(Y0=None),
            solve(eigvals=None), solve(status=None)] == [1] * 9
    assert [solve(n=BIG_N), solve(n=0), solve(dim=65), solve(dim=0), solve(wb=sneed - 1), solve(wb=0)] == [2, 3, 5, 5, 8, 8]
    torch.cuda.synchronize()
    for name, v in t.items():
        assert torch.equal(v, before[name]), f"{name} was written by a refused call"
    X = _dev(UC.cloud(4200, 3, 7))
    for fn in (lambda: UM.knn(X, 15, route="dense"), lambda: UM.umap_fit(X, 2, 15, route="dense"),
               lambda: UM.fuzzy_graph(torch.zeros(4200, 15, dtype=I32, device="cuda"), torch.zeros(4200, 15, device="cuda"), route="dense"),
               lambda: UM.layout(t["row_ptr"], t["col"], t["weight"], 0, torch.zeros(4200, 2, device="cuda"), 1.5, 0.9, route="dense"),
               lambda: UM.knn(t["X"], 64, route="sparse"), lambda: UM.umap_fit(t["X"].cpu(), 2, 5, route="sparse")):
        with pytest.raises(E.EngineError):
            fn()
    with pytest.raises(ValueError):
        UM.knn(t["X"], 5, route="tiled")
