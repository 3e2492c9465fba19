"""dm_umap_spectral with every operand inside one guarded allocation (tests/gpu_util.Guarded) under both fills: guards and inputs come
back untouched, and the result is bit-equal to the plain run -- so no kernel of csrc/umap_spectral.hip reads or writes outside its
operands, or reads workspace it has not written (0xFF fills it with NaN, 0x00 with zeros)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd import umapfit as UM
from tests import gpu_util as GU
from tests import umap_cases as UC
from tests import umap_spectral_cases as SC

pytestmark = pytest.mark.gpu
F64, F32, U8 = torch.float64, torch.float32, torch.uint8


@pytest.mark.parametrize("tag", ["n65", "n130"])
def test_guarded_solve(tag):
    c = SC.case(tag)
    G, n, dim = c["G"], c["n"], c["dim"]
    m = dim + 1
    dev = {k: torch.from_numpy(np.ascontiguousarray(G[k])).cuda() for k in ("row_ptr", "col", "weight")}
    plain = UM.spectral_init(dev, dim, UC.SEED, return_vectors=True)
    torch.cuda.synchronize()
    assert UM.spectral_status(plain["status"].cpu().numpy())["status"] == "converged"
    noise, fallback = UM.spectral_host_arrays(n, dim, UC.SEED)
    inputs = {"row_ptr": torch.from_numpy(G["row_ptr"]), "col": torch.from_numpy(G["col"]), "weight": torch.from_numpy(G["weight"]),
              "noise": torch.from_numpy(noise), "fallback": torch.from_numpy(fallback)}
    outputs = {"work": ((UM.spectral_workspace_bytes(n, dim),), U8), "Y0": ((n, dim), F32), "eigvals": ((m,), F64), "eigvecs": ((n, m), F64),
               "status": ((8,), F64)}
    lib = E.load_library()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fill in (0xFF, 0x00):
        g = GU.Guarded(inputs, outputs, fill=fill, device="cuda")
        v = g.views()
        p = lambda name: C.c_void_p(v[name].data_ptr())        # noqa: E731
        assert lib.dm_umap_spectral(s, p("row_ptr"), p("col"), p("weight"), n, dim, UC.SEED, p("noise"), p("fallback"), p("work"),
                                    v["work"].numel(), p("Y0"), p("eigvals"), p("eigvecs"), p("status")) == 0
        torch.cuda.synchronize()
        g.check()
        assert torch.equal(g.view("Y0").view(torch.int32), plain["Y0"].view(torch.int32)), f"fill {fill:#04x}: Y0 differs from the plain run"
        for name in ("eigvals", "eigvecs", "status"):
            assert torch.equal(g.view(name).view(torch.int64), plain[name].view(torch.int64)), f"fill {fill:#04x}: {name} differs"
