"""UMAP's initialisation on a disconnected graph on the GPU (dm_umap_components, dm_umap_multi_init; csrc/umap_multi.hip) against the
numpy restatement (umapfit.multi_component_init_host with solver='iter') on the restatement's own edge lists, and the fit with
disconnected='components'.  Cases and recorded figures: tests/umap_multi_cases.py.

  components  every integer output and the centroids bit-equal to `component_groups_host`; the unused ends hold what the header says.
  init        per-component status, solved / uniform split and init_used equal the restatement's; iterations within +-1; eigenvectors
              within the Davis-Kahan bound of each component's eigh; Y0 and R bit-equal to the numpy rule (steps 3-6) applied to the
              device's own eigenvectors; two runs and the two routes bit-equal.
  fallbacks   connected graphs and `far6`: dm_umap_spectral's Y0 of the same route, bit for bit.
  fit         umap_fit(disconnected='components') finite and bit-reproducible on both routes with both solvers; trustworthiness (and on
              blob1200 the Spearman figure) not below the restatement's recorded value minus its recorded spread.
  refusals    every bad argument of both entries returns its code and writes nothing.
Each case prints its figures before it asserts (-s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from diff_mining_amd import clustering as CL
from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import umap_multi_cases as MC

pytestmark = pytest.mark.gpu
ROUTES = ("dense", "sparse")
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64 if a.dtype == np.float64 else a.dtype)


def _graph(tag):
    G = MC.graph(tag)
    return {"row_ptr": _dev(G["row_ptr"]), "col": _dev(G["col"]), "weight": _dev(G["weight"])}


@functools.lru_cache(maxsize=None)
def _init(tag, route):
    """`multi_component_init` on the restatement's graph of the case, brought to the host (computed once per case and route)"""
    X, _, dim = MC.case(tag)
    out = UM.multi_component_init(_graph(tag), _dev(X), dim, MC.SEED, route=route)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor)}
    host.update(mode=out["mode"], info=out["info"])
    if "comps" in out:
        host["groups"] = UM.components_to_host(out["comps"], centroids=True)
    return host


@pytest.mark.parametrize("tag", MC.ALL + (MC.STALL,))
def test_components_entry(tag):
    X, _, _ = MC.case(tag)
    G = MC.graph(tag)
    n = len(X)
    want = UM.component_groups_host(G["row_ptr"], G["col"], G["weight"], n, X)
    c = want["n_comp"]
    out = UM.components(_graph(tag), _dev(X))
    torch.cuda.synchronize()
    got = UM.components_to_host(out, centroids=True)
    print(f"{tag}: {got['n_comp']} components (restatement {c}), {got['edge_offsets'][-1]} edges")
    assert got["n_comp"] == c
    for name in ("comp", "offsets", "perm", "edge_offsets", "sub_row_ptr", "sub_col"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), name
    assert np.array_equal(_bits(got["sub_weight"]), _bits(want["sub_weight"]))
    assert np.array_equal(_bits(got["centroids"]), _bits(want["centroids"][:UM.MULTI_MAX_COMP]))
    assert bool((out["offsets"][c:] == n).all()) and bool((out["edge_offsets"][c:] == len(G["col"])).all())
    assert not bool(out["sub_row_ptr"][n + c:].any()) and not bool(out["centroids"][c:].any())
    again = UM.components_to_host(UM.components(_graph(tag), _dev(X)), centroids=True)
    for name in got:
        if name != "n_comp":
            assert np.array_equal(_bits(again[name]), _bits(got[name])), f"two runs differ in {name}"
    plain = UM.components_to_host(UM.components(_graph(tag)))                # without X: no centroids, the rest the same
    assert "centroids" not in plain and all(np.array_equal(_bits(plain[k]), _bits(got[k])) for k in plain if k != "n_comp")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tag", MC.MULTI)
def test_init_against_the_restatement(tag, route):
    _, _, dim = MC.case(tag)
    Y0h, used, info = MC.host_init(tag)
    d = _init(tag, route)
    sts = UM.multi_status(d["status"])
    assert d["mode"] == "multi" and used == "components"
    assert np.array_equal(d["info"]["plan"], info["plan"]) and d["info"]["meta_kind"] == info["meta_kind"] == MC.EXPECT[tag][1]
    assert np.array_equal(_bits(d["info"]["meta"]["meta"]), _bits(info["meta"]["meta"]))
    assert np.array_equal(_bits(d["info"]["meta"]["range"]), _bits(info["meta"]["range"]))
    gap = MC.min_gap(tag)
    assert gap >= MC.MIN_GAP, "the case does not make the comparison meaningful: change its seed"
    for l, st in enumerate(sts):
        if not info["plan"][l]:
            assert (st["status"], st["init_used"], st["iters"]) == ("uniform", "uniform", 0) and info["status"][l] == "uniform"
            continue
        val_err, vec_ratio = MC.compare(d["groups"], l, dim, d["eigvals"], d["eigvecs"])
        print(f"{tag}/{route} component {l} ({info['sizes'][l]} rows): block {st['block']}, {st['status']} after {st['iters']} iterations "
              f"(restatement {info['iters'][l]}), residual {st['max_residual']:.2e}; |theta - eigh| {val_err:.2e}, eigenvector distance / bound "
              f"{vec_ratio:.3f}")
        assert (st["status"], st["n_comp"], st["init_used"]) == (info["status"][l], 1, "spectral") and st["status"] == "converged"
        assert st["block"] == UM.spectral_block(int(info["sizes"][l]), dim)
        assert abs(st["iters"] - info["iters"][l]) <= 1 and st["iters"] <= MC.MAX_ITERS + 1
        assert st["max_residual"] <= MC.TOL and val_err <= MC.TOL and vec_ratio <= 1.0
    want_Y0, want_R = UM.place_components_host(d["groups"], d["info"]["meta"], d["info"]["plan"], d["eigvecs"], dim, MC.SEED)
    print(f"{tag}/{route}: max |Y0 - restatement's| {np.abs(d['Y0'] - Y0h).max():.2e}")
    assert np.array_equal(_bits(d["R"]), _bits(want_R)), "R is not the numpy rule on the device's own eigenvectors"
    assert np.array_equal(_bits(d["Y0"]), _bits(want_Y0)), "Y0 is not the numpy rule on the device's own eigenvectors"
    X = MC.case(tag)[0]
    again = UM.multi_component_init(_graph(tag), _dev(X), dim, MC.SEED, route=route)
    torch.cuda.synchronize()
    other = _init(tag, ROUTES[1 - ROUTES.index(route)])
    for name in ("Y0", "R", "eigvals", "eigvecs", "status"):
        assert np.array_equal(_bits(again[name]), _bits(d[name])), f"two runs differ in {name}"
        assert np.array_equal(_bits(other[name]), _bits(d[name])), f"the routes differ in {name}"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tag", MC.CONNECTED + ("far6",))
def test_one_component_and_degenerate_are_dm_umap_spectral(tag, route):
    X, _, dim = MC.case(tag)
    want = UM.spectral_init(_graph(tag), dim, MC.SEED, route=route)
    d = _init(tag, route)
    assert np.array_equal(_bits(d["Y0"]), _bits(want["Y0"]))
    if tag == "far6":
        assert d["mode"] == "random" and (d["info"]["reason"], d["info"]["detail"], d["info"]["n_comp"]) == ("meta degenerate", "zero row sum", 6)
        assert UM.spectral_status(want["status"].cpu().numpy())["init_used"] == "random"
    else:
        assert d["mode"] == "single" and d["info"]["n_comp"] == 1 and np.array_equal(_bits(d["status"]), _bits(want["status"]))
        assert UM.spectral_status(d["status"])["init_used"] == "spectral"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("tag", MC.MULTI + ("far6", MC.STALL) + MC.CONNECTED)
def test_fit(tag, route):
    X, k, dim = MC.case(tag)
    Xd = _dev(X)
    fit = UM.umap_fit(Xd, dim, k, MC.SEED, init_solver="device", route=route, disconnected="components")
    Y = fit["embedding"]
    print(f"{tag}/{route}: init {fit['init_used']} by {fit['init_solver']}, {fit['init_iters']} iterations at the most, reason {fit['init_reason']}")
    assert bool(torch.isfinite(Y).all()) and fit["route"] == route
    assert fit["init_used"] == ("random" if tag == "far6" else "spectral" if tag in MC.CONNECTED else "components")
    if tag != MC.STALL:                                    # there the device may or may not get past the first factorisation
        assert fit["init_solver"] == "device"
    again = UM.umap_fit(Xd, dim, k, MC.SEED, init_solver="device", route=route, disconnected="components")
    assert np.array_equal(_bits(again["embedding"]), _bits(Y)) and again["init_solver"] == fit["init_solver"], "two runs differ"
    off = UM.umap_fit(Xd, dim, k, MC.SEED, init_solver="device", route=route)
    assert np.array_equal(_bits(UM.umap_fit(Xd, dim, k, MC.SEED, init_solver="device", route=route, disconnected="random")["embedding"]),
                          _bits(off["embedding"])) and "init_reason" not in off
    if tag in MC.CONNECTED or tag == "far6":
        assert np.array_equal(_bits(off["embedding"]), _bits(Y)) and off["init_used"] == fit["init_used"]
    host = UM.umap_fit(Xd, dim, k, MC.SEED, init_solver="host", route=route, disconnected="components")
    assert bool(torch.isfinite(host["embedding"]).all()) and host["init_used"] == fit["init_used"] and host["init_solver"] == "host"
    if tag in MC.HOST_TRUST:
        for name, f in (("device", fit), ("host", host)):
            Yh = f["embedding"].cpu().numpy()
            t = MC.trust(X, Yh)
            print(f"  {name} solver: trustworthiness {t:.4f} (restatement {MC.HOST_TRUST[tag]['components']:.4f}, spread "
                  f"{MC.HOST_TRUST_SPREAD[tag]['components']:.4f})")
            assert t >= MC.HOST_TRUST[tag]["components"] - MC.HOST_TRUST_SPREAD[tag]["components"]
            if tag == "blob1200":
                s = MC.spearman(X, Yh)
                print(f"  {name} solver: Spearman {s:.4f} (restatement {MC.HOST_SPEARMAN[tag]['components']:.4f}, spread "
                      f"{MC.HOST_SPEARMAN_SPREAD[tag]['components']:.4f}; 'random' {MC.spearman(X, off['embedding'].cpu().numpy()):.4f})")
                assert s >= MC.HOST_SPEARMAN[tag]["components"] - MC.HOST_SPEARMAN_SPREAD[tag]["components"]


def test_the_option_passes_through():
    X, k, dim = MC.case("two")
    Xd = _dev(np.hstack([X, X]))
    halves = [UM.umap_fit(Xd[:, i:i + 3], dim, k, MC.SEED, init_solver="device", disconnected="components")["embedding"] for i in (0, 3)]
    got = UM.compress(Xd, 2, dim, k, MC.SEED, init_solver="device", disconnected="components")
    assert np.array_equal(_bits(got), _bits(torch.cat(halves, dim=1)))
    Xb = _dev(MC.case("wide")[0][:, :8].copy())
    D = _dev(np.random.RandomState(0).rand(len(Xb)).astype(np.float32))
    res = CL.cluster_patches(Xb, D, num_clusters=3, project=2, project_seed=MC.SEED, project_solver="device", project_disconnected="components")
    want = UM.umap_fit(Xb, 2, 15, MC.SEED, init_solver="device", disconnected="components")
    assert np.array_equal(_bits(res["embedding"]), _bits(want["embedding"]))
    from diff_mining_amd.typicality import TypicalityScorer
    Xg = torch.cat([Xb[:, :4], Xb[:, :4]], dim=1).contiguous()
    for fn in (CL.cluster_patches, TypicalityScorer.cluster_patches):
        via = fn(Xb, D, num_clusters=3, project=2, project_seed=MC.SEED, project_solver="device", project_disconnected="components")
        assert np.array_equal(_bits(via["embedding"]), _bits(want["embedding"]))
        grouped = fn(Xg, D, num_clusters=3, project=("groups", 2, 2), project_seed=MC.SEED, project_solver="device",
                     project_disconnected="components")
        assert np.array_equal(_bits(grouped["embedding"]),
                              _bits(UM.compress(Xg, 2, 2, seed=MC.SEED, init_solver="device", disconnected="components")))
        assert not np.array_equal(_bits(grouped["embedding"]), _bits(UM.compress(Xg, 2, 2, seed=MC.SEED, init_solver="device")))
    for bad in ("component", None):
        with pytest.raises(ValueError):
            UM.umap_fit(Xd, dim, k, disconnected=bad)
    with pytest.raises(E.EngineError):
        UM.components({"row_ptr": torch.zeros(4, dtype=I32), "col": Xd, "weight": Xd})
    with pytest.raises(E.EngineError):
        UM.multi_component_init(_graph("two"), _dev(X), 65)
    X6, _, dim6 = MC.case("meta6")                                    # 6 components > 2 dim: the centroids are needed
    with pytest.raises(E.EngineError, match="centroids"):
        UM.multi_component_init(_graph("meta6"), _dev(X6), dim6, comps=UM.components(_graph("meta6")))


@pytest.mark.parametrize("route", ROUTES)
def test_more_components_than_the_cap(monkeypatch, route):
    """the device path past MULTI_MAX_COMP components (the cap lowered to 1): dm_umap_spectral's random Y0, with the reason"""
    X, k, dim = MC.case("two")
    monkeypatch.setattr(UM, "MULTI_MAX_COMP", 1)
    want = UM.spectral_init(_graph("two"), dim, MC.SEED, route=route)
    d = UM.multi_component_init(_graph("two"), _dev(X), dim, MC.SEED, route=route)
    assert d["mode"] == "single" and d["info"]["n_comp"] == 2 and "more than 1 components" in d["info"]["reason"]
    assert np.array_equal(_bits(d["Y0"]), _bits(want["Y0"])) and UM.spectral_status(d["status"].cpu().numpy())["init_used"] == "random"
    fit = UM.umap_fit(_dev(X), dim, k, MC.SEED, init_solver="device", route=route, disconnected="components")
    off = UM.umap_fit(_dev(X), dim, k, MC.SEED, init_solver="device", route=route)
    assert (fit["init_used"], fit["init_solver"], fit["init_reason"]) == ("random", "device", d["info"]["reason"])
    assert np.array_equal(_bits(fit["embedding"]), _bits(off["embedding"]))


def test_refusals_launch_nothing():
    lib = E.load_library()
    n, d, dim, c, cap = 20, 3, 2, 2, 8
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need_c, need_m = C.c_size_t(0), C.c_size_t(123)
    assert lib.dm_umap_components_workspace_bytes(n, None) == 1
    assert [lib.dm_umap_components_workspace_bytes(a, C.byref(need_m)) for a in (65536, 0)] == [2, 3] and need_m.value == 123
    assert lib.dm_umap_multi_workspace_bytes(n, dim, None) == 1
    assert [lib.dm_umap_multi_workspace_bytes(*a, C.byref(need_m)) for a in ((65536, dim), (0, dim), (n, 65), (n, 0))] == [2, 3, 5, 5]
    assert need_m.value == 123
    assert lib.dm_umap_components_workspace_bytes(n, C.byref(need_c)) == 0 and lib.dm_umap_multi_workspace_bytes(n, dim, C.byref(need_m)) == 0
    i32 = lambda *shape: torch.full(shape, -7, dtype=I32, device="cuda")             # noqa: E731
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=F64, device="cuda")           # noqa: E731
    t = {"row_ptr": torch.zeros(n + 1, dtype=I32, device="cuda"), "col": torch.zeros(cap, dtype=I32, device="cuda"),
         "weight": torch.ones(cap, device="cuda"), "X": torch.zeros(n, d, device="cuda"),
         "work_c": torch.full((need_c.value,), 0xF9, dtype=U8, device="cuda"), "comp": i32(n), "count": i32(1), "offsets": i32(n + 1),
         "perm": i32(n), "edge_offsets": i32(n + 1), "sub_row_ptr": i32(2 * n + 1), "sub_col": i32(cap), "sub_weight": torch.full((cap,), -7.0, device="cuda"),
         "centroids": f64(n, d), "plan": torch.ones(c, dtype=I32, device="cuda"), "meta": f64(c, dim), "range": f64(c), "unit": f64(n, dim),
         "noise": torch.zeros(n, dim, device="cuda"), "work_m": torch.full((need_m.value,), 0xF9, dtype=U8, device="cuda"),
         "Y0": torch.full((n, dim), -7.0, device="cuda"), "R": f64(n, dim), "eigvals": f64(c, dim + 1), "eigvecs": f64(n, dim + 1), "status": f64(c, 8)}
    before = {name: v.clone() for name, v in t.items()}
    p = lambda name: None if name is None else C.c_void_p(t[name].data_ptr())        # noqa: E731
    names_c = ["row_ptr", "col", "weight", "X", "work_c", "comp", "count", "offsets", "perm", "edge_offsets", "sub_row_ptr", "sub_col",
               "sub_weight", "centroids"]

    def comps(n=n, d=d, cap=cap, wb=need_c.value, **null):
        a = {k: (None if k in null else k) for k in names_c}
        return lib.dm_umap_components(s, p(a["row_ptr"]), p(a["col"]), p(a["weight"]), p(a["X"]), n, d, cap, p(a["work_c"]), wb, p(a["comp"]),
                                      p(a["count"]), p(a["offsets"]), p(a["perm"]), p(a["edge_offsets"]), p(a["sub_row_ptr"]), p(a["sub_col"]),
                                      p(a["sub_weight"]), p(a["centroids"]))

    assert [comps(**{k: 1}) for k in names_c if k != "X"] == [1] * (len(names_c) - 1)
    assert [comps(n=65536), comps(n=0), comps(d=0), comps(cap=-1), comps(cap=2 * n * 64 + 1), comps(wb=need_c.value - 1), comps(wb=0)] == \
        [2, 3, 6, 9, 9, 8, 8]
    h = {"offsets": np.array([0, 12, n], np.int32), "edge_offsets": np.array([0, 4, cap], np.int32), "plan": np.array([1, 1], np.int32)}
    names_m = ["sub_row_ptr", "sub_col", "sub_weight", "perm", "comp", "offsets", "plan", "meta", "range", "unit", "noise", "work_m", "Y0", "R",
               "eigvals", "eigvecs", "status"]

    def init(n=n, c=c, cap=cap, dim=dim, wb=need_m.value, h_off=h["offsets"], h_eoff=h["edge_offsets"], h_plan=h["plan"], **null):
        a = {k: (None if k in null else k) for k in names_m}
        hp = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)           # noqa: E731
        return lib.dm_umap_multi_init(s, p(a["sub_row_ptr"]), p(a["sub_col"]), p(a["sub_weight"]), p(a["perm"]), p(a["comp"]), p(a["offsets"]),
                                      p(a["plan"]), hp(h_off), hp(h_eoff), hp(h_plan), n, c, cap, dim, 1, p(a["meta"]), p(a["range"]),
                                      p(a["unit"]), p(a["noise"]), p(a["work_m"]), wb, p(a["Y0"]), p(a["R"]), p(a["eigvals"]), p(a["eigvecs"]),
                                      p(a["status"]))

    assert [init(**{k: 1}) for k in names_m] == [1] * len(names_m)
    assert [init(h_off=None), init(h_eoff=None), init(h_plan=None)] == [1, 1, 1]
    assert [init(n=65536), init(n=0), init(dim=65), init(dim=0), init(c=0), init(c=1025), init(c=n + 1), init(cap=-1), init(wb=need_m.value - 1), init(wb=0)] == \
        [2, 3, 5, 5, 11, 11, 11, 9, 8, 8]
    bad_off = [np.array(v, np.int32) for v in ([1, 12, n], [0, 12, n - 1], [0, 0, n], [0, n, n])]
    bad_eoff = [np.array(v, np.int32) for v in ([-1, 4, cap], [0, 4, cap + 1], [0, 5, 4])]
    assert [init(h_off=v) for v in bad_off] == [9] * 4 and [init(h_eoff=v) for v in bad_eoff] == [9] * 3
    assert init(h_off=np.array([0, 3, n], np.int32)) == 3                           # a plan of 1 for a component of dim + 1 rows
    torch.cuda.synchronize()
    for name, v in t.items():
        assert torch.equal(v, before[name]), f"{name} was written by a refused call"
