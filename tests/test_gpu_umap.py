"""The UMAP projection on the GPU (dm_umap_knn, dm_umap_graph, dm_umap_layout; csrc/umap.hip) against the numpy restatement of
diff-mining_amd/umapfit.py on the cases of tests/umap_cases.py.  The restatement's own parity with umap-learn is unpinned
(tests/make_golden_umap.py); these tests pin the kernels to the restatement.

  kNN      bit-equal, indices and distances.
  graph    rho bit-equal; sigma and the weights within 4 x what the restatement in fp32 differs from itself in float64 by on the
           same case (umap_cases.BOUNDS, measured on the CPU; 4 x for another exp); the edge structure bit-equal (no weight of any
           case lies within that bound of the pruning threshold: tests/test_umap.py asserts it).
  layout   one and three moving epochs from the restatement's initialisation and edge list, against the float64 restatement, within
           4 x the restatement's own fp32-to-float64 distance after the same epochs (4 x for another pow).  Nothing beyond three
           epochs is compared coordinate by coordinate: the iteration amplifies rounding.
  fit      the whole pipeline on the two blob cases: finite; bit-equal across runs and with every operand inside one guarded
           allocation under both fills; trustworthiness at least the restatement's minus its seed-to-seed spread; ARI 1.0.
Each case prints its figures before it asserts (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import clustering as CL
from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import gpu_util as GU
from tests import umap_cases as UC

pytestmark = pytest.mark.gpu
ALL = list(UC.SHAPES)
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
MARGIN = 4.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def ab():
    return UM.find_ab_params()


@pytest.fixture(scope="module")
def host():
    """per case: the restatement's kNN, float64 graph and initialisation; computed once, left unchanged"""
    out = {}
    for tag in ALL:
        X, k, dim, label = UC.case(tag)
        idx, dist = UM.knn_host(X, k)
        G = UM.fuzzy_graph_host(idx, dist, 500, np.float64)
        Y0, used = UM.spectral_init_host(G["P"], dim, UC.SEED)
        out[tag] = {"X": X, "k": k, "dim": dim, "label": label, "idx": idx, "dist": dist, "G": G, "Y0": Y0, "init_used": used}
    return out


@pytest.fixture(scope="module")
def device(host):
    """per case: the device kNN, and the device graph of the restatement's kNN arrays"""
    out = {}
    for tag in ALL:
        h = host[tag]
        idx, dist = UM.knn(_dev(h["X"]), h["k"])
        out[tag] = {"idx": idx, "dist": dist, "G": UM.fuzzy_graph(_dev(h["idx"]), _dev(h["dist"]), 500)}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", ALL)
def test_knn_is_bit_equal(host, device, tag):
    h, d = host[tag], device[tag]
    idx, dist = d["idx"].cpu().numpy(), d["dist"].cpu().numpy()
    print(f"{tag}: {np.sum(idx != h['idx'])} indices, {np.sum(dist.view(np.int32) != h['dist'].view(np.int32))} distances differ")
    assert np.array_equal(idx, h["idx"])
    assert np.array_equal(dist.view(np.int32), h["dist"].view(np.int32))


@pytest.mark.parametrize("tag", ALL)
def test_graph_against_the_float64_restatement(host, device, tag):
    G, D = host[tag]["G"], device[tag]["G"]
    bound = UC.BOUNDS[tag]
    n_edges = int(D["n_edges"])
    rho, sigma, P = D["rho"].cpu().numpy(), D["sigma"].cpu().numpy(), D["P"].cpu().numpy()
    row_ptr, col, weight = D["row_ptr"].cpu().numpy(), D["col"].cpu().numpy()[:n_edges], D["weight"].cpu().numpy()[:n_edges]
    sig_err = float(np.abs(sigma.astype(np.float64) - G["sigma"]).max())
    same = n_edges == len(G["col"]) and np.array_equal(row_ptr, G["row_ptr"]) and np.array_equal(col, G["col"])
    w_err = float(np.abs(weight.astype(np.float64) - G["weight"]).max()) if same else float("nan")
    p_err = float(np.abs(P.astype(np.float64) - G["P"]).max())
    print(f"{tag}: sigma err {sig_err:.3e} (bound {MARGIN * bound['sigma']:.3e}), weight err {w_err:.3e} / dense {p_err:.3e} "
          f"(bound {MARGIN * bound['weight']:.3e}), {n_edges} edges against {len(G['col'])}")
    assert np.array_equal(rho.view(np.int32), G["rho"].view(np.int32))
    assert sig_err <= MARGIN * bound["sigma"]
    assert same, "edge structure"
    assert w_err <= MARGIN * bound["weight"] and p_err <= MARGIN * bound["weight"]
    assert np.array_equal(P[np.repeat(np.arange(len(P)), np.diff(row_ptr)), col].view(np.int32), weight.view(np.int32))


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("tag", ALL)
def test_layout_epochs_against_the_float64_restatement(host, ab, tag, count):
    h = host[tag]
    G, last = h["G"], UC.moving_epochs(count)
    a, b = ab
    want, _ = UM.layout_host(G["row_ptr"], G["col"], G["weight"], h["Y0"], a, b, 500, UC.SEED, 0, last, np.float64)
    args = (_dev(G["row_ptr"]), _dev(G["col"]), _dev(G["weight"]), len(G["col"]), _dev(h["Y0"]), a, b, 500, UC.SEED)
    got = UM.layout(*args, 0, last, n_neighbors=h["k"])
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    moved = float(np.abs(want - h["Y0"]).max())
    print(f"{tag}: {count} moving epoch(s): err {err:.3e} (bound {MARGIN * UC.BOUNDS[tag][f'layout{count}']:.3e}), largest move {moved:.3e}")
    assert moved > 1e-3, "the epochs moved nothing"
    assert err <= MARGIN * UC.BOUNDS[tag][f"layout{count}"]
    # epoch by epoch on one workspace (first_epoch / last_epoch): the same bits as the run in one call
    n, dim = h["Y0"].shape
    work = torch.full((UM.workspace_bytes(n, 1, h["k"], dim),), 0xFF, dtype=U8, device="cuda")
    step = args[4]
    for ep in range(last):
        step = UM.layout(args[0], args[1], args[2], args[3], step, a, b, 500, UC.SEED, ep, ep + 1, work=work)
    assert torch.equal(_bits(step), _bits(got))


def _fit_raw(v, n, d, k, dim, a, b, seed, n_epochs=500):
    """The pipeline of `umap_fit` on caller-held tensors v[name] (so that they can live inside one guarded allocation)."""
    lib = E.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda name: C.c_void_p(v[name].data_ptr())        # noqa: E731
    wb = v["work"].numel()
    assert lib.dm_umap_knn(s, p("X"), n, d, k, p("work"), wb, p("idx"), p("dist")) == 0
    assert lib.dm_umap_graph(s, p("idx"), p("dist"), n, k, n_epochs, p("work"), wb, p("rho"), p("sigma"), p("P"), p("row_ptr"), p("col"),
                             p("weight"), p("n_edges")) == 0
    n_edges = int(v["n_edges"])
    Y0, used = UM.spectral_init_host(v["P"].cpu().numpy(), dim, seed)
    v["Y"].copy_(torch.from_numpy(Y0))
    assert lib.dm_umap_layout(s, p("row_ptr"), p("col"), p("weight"), n, n_edges, dim, a, b, n_epochs, seed, 0, n_epochs, p("Y"), p("work"),
                              wb) == 0
    torch.cuda.synchronize()
    return n_edges, used


@pytest.mark.parametrize("tag", list(UC.BLOBS))
def test_fit_on_blobs(host, ab, tag):
    from sklearn.metrics import adjusted_rand_score
    h = host[tag]
    X, k, dim, label = h["X"], h["k"], h["dim"], h["label"]
    n, d = X.shape
    Xd = _dev(X)
    fit = UM.umap_fit(Xd, dim, k, UC.SEED)
    Y = fit["embedding"]
    assert bool(torch.isfinite(Y).all()) and fit["init_used"] == h["init_used"] == "spectral"
    assert torch.equal(_bits(UM.umap_fit(Xd, dim, k, UC.SEED)["embedding"]), _bits(Y)), "two runs differ"
    # every operand inside one guarded allocation, NaN / -1 and zero fills
    outputs = {"idx": ((n, k), I32), "dist": ((n, k), F32), "rho": ((n,), F32), "sigma": ((n,), F32), "P": ((n, n), F32),
               "row_ptr": ((n + 1,), I32), "col": ((2 * n * k,), I32), "weight": ((2 * n * k,), F32), "n_edges": ((1,), I32),
               "Y": ((n, dim), F32), "work": ((UM.workspace_bytes(n, d, k, dim),), U8)}
    for fill in (0xFF, 0x00):
        g = GU.Guarded({"X": torch.from_numpy(X)}, outputs, fill=fill, device="cuda")
        n_edges, used = _fit_raw(g.views(), n, d, k, dim, fit["a"], fit["b"], UC.SEED)
        g.check()
        assert n_edges == fit["n_edges"] and used == "spectral"
        assert torch.equal(_bits(g.view("Y")), _bits(Y)), f"guard fill {fill:#04x}: the embedding differs from the plain run"
        assert bool((g.view("col")[n_edges:] == (-1 if fill else 0)).all()), "col written past n_edges"
    Yh = Y.cpu().numpy()
    t = UC.trust(X, Yh)
    floor = UC.HOST_TRUST[tag] - UC.HOST_TRUST_SPREAD[tag]
    labels = CL.kmeans_fit(Y, int(label.max()) + 1)[0].cpu().numpy()
    ari = adjusted_rand_score(label, labels)
    print(f"{tag}: trustworthiness {t:.4f} (restatement {UC.HOST_TRUST[tag]:.4f}, spread {UC.HOST_TRUST_SPREAD[tag]:.4f}), ARI {ari:.4f}, "
          f"{fit['n_edges']} edges")
    assert t >= floor
    assert ari == 1.0


def test_disconnected_and_duplicate_cases_fit(host):
    for tag, used in (("split", "random"), ("dup", None)):
        h = host[tag]
        fit = UM.umap_fit(_dev(h["X"]), h["dim"], h["k"], UC.SEED)
        assert bool(torch.isfinite(fit["embedding"]).all()) and fit["init_used"] == h["init_used"]
        assert used is None or fit["init_used"] == used


def test_refusals_launch_nothing():
    lib = E.load_library()
    n, d, k, dim = 20, 3, 5, 2
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = {"X": torch.zeros(n, d, device="cuda"), "idx": torch.full((n, k), -7, dtype=I32, device="cuda"),
         "dist": torch.full((n, k), -7.0, device="cuda"), "rho": torch.full((n,), -7.0, device="cuda"),
         "sigma": torch.full((n,), -7.0, device="cuda"), "P": torch.full((n, n), -7.0, device="cuda"),
         "row_ptr": torch.full((n + 1,), -7, dtype=I32, device="cuda"), "col": torch.full((2 * n * k,), -7, dtype=I32, device="cuda"),
         "weight": torch.full((2 * n * k,), -7.0, device="cuda"), "n_edges": torch.full((1,), -7, dtype=I32, device="cuda"),
         "Y": torch.full((n, dim), -7.0, device="cuda"), "work": torch.full((UM.workspace_bytes(n, d, k, dim),), 0xF9, dtype=U8, device="cuda")}
    before = {name: v.clone() for name, v in t.items()}
    p = lambda name: None if name is None else C.c_void_p(t[name].data_ptr())        # noqa: E731
    wb = t["work"].numel()

    def knn(X="X", n=n, d=d, k=k, work="work", wb=wb, idx="idx", dist="dist"):
        return lib.dm_umap_knn(s, p(X), n, d, k, p(work), wb, p(idx), p(dist))

    def graph(idx="idx", dist="dist", n=n, k=k, ne=500, work="work", wb=wb, rho="rho", n_edges="n_edges"):
        return lib.dm_umap_graph(s, p(idx), p(dist), n, k, ne, p(work), wb, p(rho), p("sigma"), p("P"), p("row_ptr"), p("col"), p("weight"),
                                 p(n_edges))

    def layout(row_ptr="row_ptr", n=n, ne=10, dim=dim, epochs=500, first=0, last=2, Y="Y", work="work", wb=wb):
        return lib.dm_umap_layout(s, p(row_ptr), p("col"), p("weight"), n, ne, dim, 1.5, 0.9, epochs, 1, first, last, p(Y), p(work), wb)

    out = C.c_size_t(123)
    assert lib.dm_umap_workspace_bytes(n, d, k, dim, None) == 1
    assert [lib.dm_umap_workspace_bytes(*a, C.byref(out)) for a in ((4096, d, k, dim), (5, d, 5, dim), (100, d, 65, dim), (100, d, 1, dim),
                                                                    (n, d, k, 65), (n, d, k, 0), (n, 0, k, dim))] == [2, 3, 4, 4, 5, 5, 6]
    assert out.value == 123
    assert [knn(X=None), knn(idx=None), knn(work=None), knn(n=4096), knn(n=5), knn(n=100, k=65), knn(d=0), knn(wb=wb // 2)] == \
        [1, 1, 1, 2, 3, 4, 6, 8]
    assert [graph(idx=None), graph(n_edges=None), graph(n=4096), graph(n=5), graph(n=100, k=65), graph(ne=0), graph(wb=64)] == \
        [1, 1, 2, 3, 4, 7, 8]
    assert [layout(row_ptr=None), layout(Y=None), layout(n=4096), layout(dim=65), layout(dim=0), layout(first=3, last=2), layout(last=501),
            layout(epochs=0), layout(ne=-1), layout(wb=16)] == [1, 1, 2, 5, 5, 7, 7, 7, 9, 8]
    torch.cuda.synchronize()
    for name, v in t.items():
        assert torch.equal(v, before[name]), f"{name} was written by a refused call"
    for fn, args in ((UM.knn, (t["X"], 64)), (UM.knn, (t["X"], 20)), (UM.umap_fit, (t["X"], 65, 5)), (UM.umap_fit, (t["X"].cpu(), 2, 5))):
        with pytest.raises(E.EngineError):
            fn(*args)


def test_cluster_patches_projects_on_the_device(host):
    """project=5 (the main stage's project=True): the clusters' label partition is the true blobs.  project=('groups', 2, 5): the
    embedding is the two halves' fits side by side, and the ranking runs on the original features."""
    from sklearn.metrics import adjusted_rand_score
    from diff_mining_amd.typicality import TypicalityScorer
    h = host["blob300"]
    X, label = _dev(h["X"]), h["label"]
    D = _dev(np.random.RandomState(0).rand(len(label)).astype(np.float32))
    res = TypicalityScorer.cluster_patches(X, D, num_clusters=6, project=5, project_seed=UC.SEED)
    assert adjusted_rand_score(label, res["labels"].cpu().numpy()) == 1.0
    assert tuple(res["embedding"].shape) == (300, 5) and sorted(np.concatenate([c["rows"] for c in res["clusters"]]).tolist()) == list(range(300))
    res = CL.cluster_patches(X, D, num_clusters=6, project=("groups", 2, 5), project_seed=UC.SEED)
    halves = [UM.umap_fit(X[:, i:i + 32], 5, 15, UC.SEED)["embedding"] for i in (0, 32)]
    assert torch.equal(_bits(res["embedding"]), _bits(torch.cat(halves, dim=1)))
    labels, centers = res["labels"], res["centers"]
    want = CL.rank_clusters(res["embedding"], labels, centers, D, "median", "farthest", X)
    order, off = want[0].cpu().numpy(), want[2].cpu().numpy()
    for r, c in enumerate(res["clusters"]):
        assert np.array_equal(c["rows"], order[off[r]:off[r + 1]])
