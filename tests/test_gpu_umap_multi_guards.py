"""dm_umap_components and dm_umap_multi_init with every device operand inside one guarded allocation (tests/gpu_util.Guarded) under both
fills: guards and inputs come back untouched, and the results are bit-equal to the plain run -- so no kernel of csrc/umap_multi.hip
(nor the solver it enqueues per component) reads or writes outside its operands, or reads workspace or output it has not written
(0xFF fills them with NaN / -1, 0x00 with zeros)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import gpu_util as GU
from tests import umap_multi_cases as MC

pytestmark = pytest.mark.gpu
F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8


def _same(a, b):
    return torch.equal(a.contiguous().view(U8), b.contiguous().view(U8))


@pytest.mark.parametrize("tag", ["edge", "meta6"])
def test_guarded_components_and_init(tag):
    X, _, dim = MC.case(tag)
    G = MC.graph(tag)
    n, d, E_n, m = len(X), X.shape[1], len(G["col"]), dim + 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(G[k])).cuda() for k in ("row_ptr", "col", "weight")}
    plain = UM.multi_component_init(dev, torch.from_numpy(X).cuda(), dim, MC.SEED)
    torch.cuda.synchronize()
    assert plain["mode"] == "multi" and all(s["status"] in ("converged", "uniform") for s in UM.multi_status(plain["status"].cpu().numpy()))
    comps, info = plain["comps"], plain["info"]
    c = info["n_comp"]
    total = int(comps["edge_offsets"][c])
    lib = E.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need_c, need_m = C.c_size_t(0), C.c_size_t(0)
    assert lib.dm_umap_components_workspace_bytes(n, C.byref(need_c)) == 0 and lib.dm_umap_multi_workspace_bytes(n, dim, C.byref(need_m)) == 0
    noise, _ = UM.spectral_host_arrays(n, dim, MC.SEED)
    h_off, h_eoff = comps["offsets"][:c + 1].cpu().numpy().copy(), comps["edge_offsets"][:c + 1].cpu().numpy().copy()
    h_plan = np.ascontiguousarray(info["plan"], dtype=np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    for fill in (0xFF, 0x00):
        inputs = {"row_ptr": torch.from_numpy(G["row_ptr"]), "col": torch.from_numpy(G["col"]), "weight": torch.from_numpy(G["weight"]),
                  "X": torch.from_numpy(X)}
        outputs = {"work": ((need_c.value,), U8), "comp": ((n,), I32), "count": ((1,), I32), "offsets": ((n + 1,), I32), "perm": ((n,), I32),
                   "edge_offsets": ((n + 1,), I32), "sub_row_ptr": ((2 * n + 1,), I32), "sub_col": ((E_n,), I32), "sub_weight": ((E_n,), F32),
                   "centroids": ((min(n, UM.MULTI_MAX_COMP), d), F64)}
        g = GU.Guarded(inputs, outputs, fill=fill, device="cuda")
        v = g.views()
        p = lambda name: C.c_void_p(v[name].data_ptr())               # noqa: E731
        assert lib.dm_umap_components(s, p("row_ptr"), p("col"), p("weight"), p("X"), n, d, E_n, p("work"), v["work"].numel(), p("comp"),
                                      p("count"), p("offsets"), p("perm"), p("edge_offsets"), p("sub_row_ptr"), p("sub_col"), p("sub_weight"),
                                      p("centroids")) == 0
        torch.cuda.synchronize()
        g.check()
        for name in ("comp", "count", "offsets", "perm", "edge_offsets", "sub_row_ptr", "centroids"):
            assert _same(g.view(name), comps[name]), f"fill {fill:#04x}: {name} differs from the plain run"
        for name in ("sub_col", "sub_weight"):
            assert _same(g.view(name)[:total], comps[name][:total]), f"fill {fill:#04x}: {name} differs from the plain run"
        # the second entry on the first one's outputs, now inputs
        first = {name: g.view(name).cpu() for name in ("sub_row_ptr", "sub_col", "sub_weight", "perm", "comp", "offsets")}
        inputs = dict(first, plan=torch.from_numpy(h_plan), meta=torch.from_numpy(info["meta"]["meta"]), range=torch.from_numpy(info["meta"]["range"]),
                      unit=torch.from_numpy(UM.multi_host_arrays(n, dim, MC.SEED)), noise=torch.from_numpy(noise))
        outputs = {"work": ((need_m.value,), U8), "Y0": ((n, dim), F32), "R": ((n, dim), F64), "eigvals": ((c, m), F64), "eigvecs": ((n, m), F64),
                   "status": ((c, 8), F64)}
        g = GU.Guarded(inputs, outputs, fill=fill, device="cuda")
        v = g.views()
        assert lib.dm_umap_multi_init(s, p("sub_row_ptr"), p("sub_col"), p("sub_weight"), p("perm"), p("comp"), p("offsets"), p("plan"),
                                      hp(h_off), hp(h_eoff), hp(h_plan), n, c, E_n, dim, MC.SEED, p("meta"), p("range"), p("unit"), p("noise"),
                                      p("work"), v["work"].numel(), p("Y0"), p("R"), p("eigvals"), p("eigvecs"), p("status")) == 0
        torch.cuda.synchronize()
        g.check()
        for name in ("Y0", "R", "eigvals", "eigvecs", "status"):
            assert _same(g.view(name), plain[name]), f"fill {fill:#04x}: {name} differs from the plain run"
