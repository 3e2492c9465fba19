"""dm_umap_sparse_knn / _graph / _layout / _spectral with every operand inside one guarded allocation (tests/gpu_util.Guarded) under both
fills: guards and inputs come back untouched, and the results are bit-equal to each other and to the plain run -- so no kernel of
csrc/umap_sparse.hip reads or writes outside its operands, or reads workspace it has not written (0xFF fills it with NaN / -1, 0x00
with zeros).  Cases: n65 (one ragged row block), tall (several row blocks and column tiles, two passes of the prefix sum), hub (rows of
299 edges)."""
import ctypes as C

import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import gpu_util as GU
from tests import umap_cases as UC
from tests import umap_sparse_cases as XC

pytestmark = pytest.mark.gpu
F64, F32, I32, U8 = torch.float64, torch.float32, torch.int32, torch.uint8
EPOCHS = 4


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int64) if t.dtype == F64 else t


@pytest.mark.parametrize("tag", ["n65", "tall", "hub"])
def test_guarded_sparse_route(tag):
    X, k, dim = XC.case(tag)
    n, d = X.shape
    m = dim + 1
    a, b = UM.find_ab_params()
    Xd = torch.from_numpy(X).cuda()
    idx, dist = UM.knn(Xd, k, route="sparse")
    G = UM.fuzzy_graph(idx, dist, 500, route="sparse")
    S = UM.spectral_init(G, dim, UC.SEED, return_vectors=True, route="sparse")
    ne = int(G["n_edges"])
    Y = UM.layout(G["row_ptr"], G["col"], G["weight"], ne, S["Y0"], a, b, 500, UC.SEED, 0, EPOCHS, n_neighbors=k, route="sparse")
    plain = {"idx": idx, "dist": dist, "rho": G["rho"], "sigma": G["sigma"], "row_ptr": G["row_ptr"], "col": G["col"][:ne],
             "weight": G["weight"][:ne], "Y0": S["Y0"], "eigvals": S["eigvals"], "eigvecs": S["eigvecs"], "status": S["status"], "Y": Y}
    noise, fallback = UM.spectral_host_arrays(n, dim, UC.SEED)
    inputs = {"X": torch.from_numpy(X), "noise": torch.from_numpy(noise), "fallback": torch.from_numpy(fallback)}
    outputs = {"idx": ((n, k), I32), "dist": ((n, k), F32), "rho": ((n,), F32), "sigma": ((n,), F32), "row_ptr": ((n + 1,), I32),
               "col": ((2 * n * k,), I32), "weight": ((2 * n * k,), F32), "n_edges": ((1,), I32), "Y": ((n, dim), F32),
               "work": ((UM.workspace_bytes(n, d, k, dim, "sparse"),), U8), "swork": ((UM.spectral_workspace_bytes(n, dim, "sparse"),), U8),
               "Y0": ((n, dim), F32), "eigvals": ((m,), F64), "eigvecs": ((n, m), F64), "status": ((8,), F64)}
    lib = E.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fill in (0xFF, 0x00):
        g = GU.Guarded(inputs, outputs, fill=fill, device="cuda")
        v = g.views()
        p = lambda name: C.c_void_p(v[name].data_ptr())        # noqa: E731
        wb = v["work"].numel()
        assert lib.dm_umap_sparse_knn(s, p("X"), n, d, k, p("work"), wb, p("idx"), p("dist")) == 0
        assert lib.dm_umap_sparse_graph(s, p("idx"), p("dist"), n, k, 500, p("work"), wb, p("rho"), p("sigma"), p("row_ptr"), p("col"),
                                        p("weight"), p("n_edges")) == 0
        assert lib.dm_umap_sparse_spectral(s, p("row_ptr"), p("col"), p("weight"), n, dim, UC.SEED, p("noise"), p("fallback"), p("swork"),
                                           v["swork"].numel(), p("Y0"), p("eigvals"), p("eigvecs"), p("status")) == 0
        assert int(v["n_edges"]) == ne
        v["Y"].copy_(v["Y0"])
        assert lib.dm_umap_sparse_layout(s, p("row_ptr"), p("col"), p("weight"), n, ne, dim, a, b, 500, UC.SEED, 0, EPOCHS, p("Y"), p("work"),
                                         wb) == 0
        torch.cuda.synchronize()
        g.check()
        for name, want in plain.items():
            got = g.view(name)[:ne] if name in ("col", "weight") else g.view(name)
            assert torch.equal(_bits(got), _bits(want)), f"fill {fill:#04x}: {name} differs from the plain run"
        assert bool((g.view("col")[ne:] == (-1 if fill else 0)).all()), "col written past n_edges"
