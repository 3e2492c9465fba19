"""Guard bands around the dense detector search (tests/gpu_util.Guarded): S1 and S2 with every device operand of the three entry
points in ONE allocation.  A store outside an operand changes a guard byte; a load outside one that reaches the result makes the
result depend on the fill byte.  Results are bit-equal to the plain run under both fills; guards and inputs stay untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import dense_search_cases as DC  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402
from tests.test_gpu_dense_search import inputs, search  # noqa: E402

PAD = 3          # table columns past the last image: no call may write them


def guarded_run(tag, fill):
    s = DC.SHAPES[tag]
    K, top_k, cells, C_ = s["K"], s["top_k"], s["W"] * s["H"], s["C"]
    w, chunks = inputs(tag)
    n = sum(len(c[0]) for c in chunks)
    plain = search(tag)
    _, top_image, top_cell, count = plain.topk()
    # the rows of chunk 0's entries in the final top-k, and one pair outside the chunk (a zero row, nothing read)
    B0 = len(chunks[0][0])
    pairs = [(int(top_image[k, j]), int(top_cell[k, j])) for k in range(K) for j in range(int(count[k])) if top_image[k, j] < B0]
    pairs = np.array(pairs + [(B0, 0)], dtype=np.int32)
    ins = {"w": torch.from_numpy(w), "pairs": torch.from_numpy(pairs)}
    for j, (_, data, mask) in enumerate(chunks):
        ins[f"data{j}"] = torch.from_numpy(data).view(len(data), cells, C_)
        if mask is not None:
            ins[f"mask{j}"] = torch.from_numpy(mask)
    need = max(D.workspace_bytes(len(c[0]), cells, K) for c in chunks)
    outs = {"work": ((need,), torch.uint8), "score": ((K, n + PAD), torch.float32), "cell": ((K, n + PAD), torch.int32),
            "top_score": ((K, top_k), torch.float32), "top_image": ((K, top_k), torch.int32), "top_cell": ((K, top_k), torch.int32),
            "count": ((K,), torch.int32), "rows": ((len(pairs), C_), torch.float16)}
    g = Guarded(ins, outs, fill=fill, device=dev())
    v = g.views()
    lib, stream = D._lib(), D._stream(torch, dev())
    ptr = D._p
    at = 0
    for j, (paths, _, mask) in enumerate(chunks):
        rc = lib.dm_dense_search_winners(stream, ptr(v[f"data{j}"]), ptr(v["w"]), ptr(v[f"mask{j}"]) if mask is not None else None,
                                         len(paths), cells, C_, K, at, n + PAD, ptr(v["work"]), need, ptr(v["score"]), ptr(v["cell"]))
        assert rc == 0
        at += len(paths)
    assert lib.dm_dense_search_topk(stream, ptr(v["score"]), ptr(v["cell"]), K, n, n + PAD, top_k, 0, ptr(v["top_score"]),
                                    ptr(v["top_image"]), ptr(v["top_cell"]), ptr(v["count"])) == 0
    assert lib.dm_dense_search_gather(stream, ptr(v["data0"]), B0, cells, C_, ptr(v["pairs"]), len(pairs), ptr(v["rows"])) == 0
    torch.cuda.synchronize()
    g.check()
    return g, v, pairs, n


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ff", "00"))
@pytest.mark.parametrize("tag", ("S1", "S2"))
def test_guarded_run_equals_the_plain_run(tag, fill):
    g, v, pairs, n = guarded_run(tag, fill)
    plain = search(tag)
    score, cell = plain.tables()
    assert v["score"][:, :n].cpu().numpy().tobytes() == score.tobytes()
    assert v["cell"][:, :n].cpu().numpy().tobytes() == cell.tobytes()
    for name in ("score", "cell"):                                                   # the columns past the last image keep the fill
        assert (v[name][:, n:].contiguous().view(torch.uint8) == fill).all(), name
    for got, want in zip((v["top_score"], v["top_image"], v["top_cell"], v["count"]), plain.topk()):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    data0 = inputs(tag)[1][0][1]
    data0 = data0.reshape(len(data0), -1, data0.shape[-1])
    rows = v["rows"].cpu().numpy()
    for r, (b, c) in enumerate(pairs[:-1]):
        assert rows[r].tobytes() == data0[b, c].tobytes()
    assert not rows[-1].view(np.uint16).any()                                        # the pair outside the chunk: zeros
