"""Guard bands around the HOG-LAB kernels (tests/gpu_util.Guarded): cases A (one block) and C (ragged: the stencil reads pixels past
the 8-grid, and must stop at the image) with every device operand of the two launch entries in ONE allocation — images, bin table,
both cell maps, workspace, both outputs.  A store outside an operand changes a guard byte; a load outside one that reaches a result
makes the result depend on the fill byte.  Results are bit-equal to the plain run under both fills; guards and inputs stay untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import hoglab_cases as HC  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402
from tests.hoglab_gpu_run import run  # noqa: E402


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ff", "00"))
@pytest.mark.parametrize("tag", ("A", "C"))
def test_guarded_run_equals_the_plain_run(tag, fill):
    images = HC.images(tag)
    B, H, W, _ = images.shape
    nr, nc = H // 8, W // 8
    bc, br = D.hoglab_shape(H, W)
    need = D.hoglab_workspace_bytes(B, H, W)
    ins = {"images": torch.from_numpy(images.copy()), "bins": torch.from_numpy(D.hoglab_bin_table().copy())}
    outs = {"hog": ((B, nr, nc, 31), torch.float32), "lab": ((B, 2, nr, nc), torch.float32), "work": ((need,), torch.uint8),
            "out": ((B, bc, br, 2112), torch.float16), "raw": ((B, bc, br, 2112), torch.float32)}
    g = Guarded(ins, outs, fill=fill, device=dev())
    v = g.views()
    lib, stream, ptr = D._lib(), D._stream(torch, dev()), D._p
    assert lib.dm_hoglab_cells(stream, ptr(v["images"]), B, H, W, ptr(v["bins"]), ptr(v["hog"]), ptr(v["lab"])) == 0
    assert lib.dm_hoglab_features(stream, ptr(v["images"]), B, H, W, ptr(v["bins"]), ptr(v["out"]), ptr(v["raw"]), ptr(v["work"]),
                                  need) == 0
    torch.cuda.synchronize()
    g.check()
    plain = run(tag)
    for name in ("hog", "lab", "out", "raw"):
        assert v[name].cpu().numpy().tobytes() == plain[name].tobytes(), name
    # the workspace holds the two cell maps and nothing else: its padding keeps the fill
    work = v["work"].cpu().numpy()
    n_hog, n_lab = plain["hog"].nbytes, plain["lab"].nbytes
    lab_at = (n_hog + 255) // 256 * 256
    assert work[:n_hog].tobytes() == plain["hog"].tobytes() and work[lab_at:lab_at + n_lab].tobytes() == plain["lab"].tobytes()
    assert (work[n_hog:lab_at] == fill).all() and (work[lab_at + n_lab:] == fill).all()
