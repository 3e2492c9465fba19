"""UMAP's spectral initialisation on the GPU (dm_umap_spectral; csrc/umap_spectral.hip) against numpy's `eigh` and against the numpy
restatement (umapfit.spectral_init_iter_host) on the restatement's own edge lists.  Cases, bounds and what they rest on:
tests/umap_spectral_cases.py.

  solve   status, component count and init_used equal the restatement's; outer iterations within +-1 of it (another summation order in
          the Gram matrices); Ritz values within 1e-11 of eigh's and eigenvectors within 2e-11 / gap; Y0 bit-equal to the numpy tail on
          the device's own eigenvectors; two runs bit-equal.
  fit     umap_fit(init_solver='device'): finite, bit-reproducible, trustworthiness and ARI by the criteria of tests/test_gpu_umap.py;
          init_solver='host' is the pipeline as it was, bit for bit.
Each case prints its figures before it asserts (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import clustering as CL
from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import umap_cases as UC
from tests import umap_spectral_cases as SC

pytestmark = pytest.mark.gpu
SOLVED = ["n17", "cloud9", "n65", "n130", "n300", "dup", "blob400", "cloud1000", "wide150"]
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(tag):
    G = SC.case(tag)["G"]
    return {"row_ptr": _dev(G["row_ptr"]), "col": _dev(G["col"]), "weight": _dev(G["weight"])}


def _run(tag, dim=None):
    c = SC.case(tag)
    out = UM.spectral_init(_graph(tag), c["dim"] if dim is None else dim, UC.SEED, return_vectors=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def host():
    out = {}
    for tag in SOLVED + ["split"]:
        c = SC.case(tag)
        G = c["G"]
        out[tag] = UM.spectral_init_iter_host(G["row_ptr"], G["col"], G["weight"], c["n"], c["dim"], UC.SEED)
    return out


@pytest.fixture(scope="module")
def device():
    return {tag: _run(tag) for tag in SOLVED + ["split"]}


@pytest.mark.parametrize("tag", SOLVED)
def test_solve_against_eigh_and_the_restatement(host, device, tag):
    c = SC.case(tag)
    Y0h, used, info = host[tag]
    d = device[tag]
    st = UM.spectral_status(d["status"])
    gap, lead = SC.preconditions(tag)
    val_err, vec_ratio = SC.compare(tag, d["eigvals"], d["eigvecs"])
    print(f"{tag}: block {st['block']}, {st['status']} after {st['iters']} iterations (restatement {info['iters']}), residual "
          f"{st['max_residual']:.2e}, last degree {st['degree']}; smallest gap {gap:.2e}, sign lead {lead:.2e}; |theta - eigh| {val_err:.2e}, "
          f"eigenvector distance / bound {vec_ratio:.3f}; max |Y0 - restatement's| {np.abs(d['Y0'] - Y0h).max():.2e}")
    assert gap >= SC.MIN_GAP and lead >= SC.MIN_LEAD, "the case does not make the comparison meaningful: change its seed"
    assert info["status"] == "converged" and info["iters"] <= SC.MAX_ITERS
    assert (st["status"], st["n_comp"], st["init_used"]) == (info["status"], info["n_comp"], used) == ("converged", 1, "spectral")
    assert st["block"] == UM.spectral_block(c["n"], c["dim"])
    assert abs(st["iters"] - info["iters"]) <= 1
    assert st["max_residual"] <= SC.TOL
    assert val_err <= SC.TOL
    assert vec_ratio <= 1.0
    assert np.array_equal(d["Y0"].view(np.int32), SC.tail(tag, d["eigvecs"]).view(np.int32)), "Y0 is not the numpy tail of the device's eigenvectors"
    again = _run(tag)
    for name in ("Y0", "eigvals", "eigvecs", "status"):
        assert np.array_equal(again[name].view(np.int64 if again[name].dtype == np.float64 else np.int32),
                              d[name].view(np.int64 if d[name].dtype == np.float64 else np.int32)), f"two runs differ in {name}"


def test_random_fallbacks(host, device):
    """`split` (two components) and dim + 1 >= n: the uploaded random initialisation, the host's bit for bit"""
    Y0h, used, info = host["split"]
    st = UM.spectral_status(device["split"]["status"])
    assert (st["status"], st["init_used"], st["n_comp"], st["iters"]) == ("random", "random", info["n_comp"], 0) and info["n_comp"] == 2
    assert np.array_equal(device["split"]["Y0"].view(np.int32), Y0h.view(np.int32))
    assert not device["split"]["eigvals"].any() and not device["split"]["eigvecs"].any()
    for dim in (16, 20):
        G = SC.case("n17")["G"]
        want, _ = UM.spectral_init_host(G["P"], dim, UC.SEED)
        d = _run("n17", dim)
        st = UM.spectral_status(d["status"])
        assert (st["status"], st["n_comp"], st["iters"]) == ("random", 1, 0)
        assert np.array_equal(d["Y0"].view(np.int32), want.view(np.int32))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("tag", list(UC.BLOBS))
def test_fit_with_the_device_solver(tag):
    from sklearn.metrics import adjusted_rand_score
    X, k, dim, label = UC.case(tag)
    Xd = _dev(X)
    fit = UM.umap_fit(Xd, dim, k, UC.SEED, init_solver="device")
    Y = fit["embedding"]
    assert bool(torch.isfinite(Y).all()) and fit["init_used"] == "spectral" and fit["init_solver"] == "device"
    assert 1 <= fit["init_iters"] <= SC.MAX_ITERS + 1
    assert torch.equal(_bits(UM.umap_fit(Xd, dim, k, UC.SEED, init_solver="device")["embedding"]), _bits(Y)), "two runs differ"
    t = UC.trust(X, Y.cpu().numpy())
    ari = adjusted_rand_score(label, CL.kmeans_fit(Y, int(label.max()) + 1)[0].cpu().numpy())
    print(f"{tag}: device solver, {fit['init_iters']} iterations: trustworthiness {t:.4f} (restatement {UC.HOST_TRUST[tag]:.4f}, spread "
          f"{UC.HOST_TRUST_SPREAD[tag]:.4f}), ARI {ari:.4f}")
    assert t >= UC.HOST_TRUST[tag] - UC.HOST_TRUST_SPREAD[tag]
    assert ari == 1.0
    # init_solver='host' (the default): the pipeline as it was, step by step
    a, b = UM.find_ab_params()
    idx, dist = UM.knn(Xd, k)
    G = UM.fuzzy_graph(idx, dist, 500)
    Y0, used = UM.spectral_init_host(G["P"].cpu().numpy(), dim, UC.SEED)
    want = UM.layout(G["row_ptr"], G["col"], G["weight"], int(G["n_edges"]), _dev(Y0), a, b, 500, UC.SEED, n_neighbors=k)
    for got in (UM.umap_fit(Xd, dim, k, UC.SEED), UM.umap_fit(Xd, dim, k, UC.SEED, init_solver="host")):
        assert got["init_solver"] == "host" and got["init_used"] == used and torch.equal(_bits(got["embedding"]), _bits(want))


def test_the_choice_passes_through():
    X, k, dim, label = UC.case("blob300")
    Xd = _dev(X)
    D = _dev(np.random.RandomState(0).rand(len(label)).astype(np.float32))
    halves = [UM.umap_fit(Xd[:, i:i + 32], 5, 15, UC.SEED, init_solver="device")["embedding"] for i in (0, 32)]
    assert torch.equal(_bits(UM.compress(Xd, 2, 5, 15, UC.SEED, init_solver="device")), _bits(torch.cat(halves, dim=1)))
    res = CL.cluster_patches(Xd, D, num_clusters=6, project=5, project_seed=UC.SEED, project_solver="device")
    assert torch.equal(_bits(res["embedding"]), _bits(UM.umap_fit(Xd, 5, 15, UC.SEED, init_solver="device")["embedding"]))
    with pytest.raises(ValueError):
        UM.umap_fit(Xd, 5, 15, UC.SEED, init_solver="gpu")


def test_refusals_launch_nothing():
    lib = E.load_library()
    n, dim = 20, 2
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = UM.spectral_workspace_bytes(n, dim)
    t = {"row_ptr": torch.zeros(n + 1, dtype=I32, device="cuda"), "col": torch.zeros(8, dtype=I32, device="cuda"),
         "weight": torch.ones(8, device="cuda"), "noise": torch.zeros(n, dim, device="cuda"), "fallback": torch.zeros(n, dim, device="cuda"),
         "work": torch.full((need,), 0xF9, dtype=U8, device="cuda"), "Y0": torch.full((n, dim), -7.0, device="cuda"),
         "eigvals": torch.full((dim + 1,), -7.0, dtype=F64, device="cuda"), "eigvecs": torch.full((n, dim + 1), -7.0, dtype=F64, device="cuda"),
         "status": torch.full((8,), -7.0, dtype=F64, device="cuda")}
    before = {name: v.clone() for name, v in t.items()}
    p = lambda name: None if name is None else C.c_void_p(t[name].data_ptr())        # noqa: E731

    def solve(row_ptr="row_ptr", col="col", weight="weight", n=n, dim=dim, noise="noise", fallback="fallback", work="work", wb=need, Y0="Y0",
              eigvals="eigvals", status="status"):
        return lib.dm_umap_spectral(s, p(row_ptr), p(col), p(weight), n, dim, 1, p(noise), p(fallback), p(work), wb, p(Y0), p(eigvals),
                                    p("eigvecs"), p(status))

    out = C.c_size_t(123)
    assert lib.dm_umap_spectral_workspace_bytes(n, dim, None) == 1
    assert [lib.dm_umap_spectral_workspace_bytes(*a, C.byref(out)) for a in ((4096, dim), (0, dim), (n, 65), (n, 0))] == [2, 3, 5, 5]
    assert out.value == 123
    assert [solve(row_ptr=None), solve(col=None), solve(weight=None), solve(noise=None), solve(fallback=None), solve(work=None), solve(Y0=None),
            solve(eigvals=None), solve(status=None)] == [1] * 9
    assert [solve(n=4096), solve(n=0), solve(dim=65), solve(dim=0), solve(wb=need - 1), solve(wb=0)] == [2, 3, 5, 5, 8, 8]
    torch.cuda.synchronize()
    for name, v in t.items():
        assert torch.equal(v, before[name]), f"{name} was written by a refused call"
    with pytest.raises(E.EngineError):
        UM.spectral_init({"row_ptr": t["row_ptr"].cpu(), "col": t["col"], "weight": t["weight"]}, dim)
    with pytest.raises(E.EngineError):
        UM.spectral_init(t, 65)
