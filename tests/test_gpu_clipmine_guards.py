"""Guard bands around the CLIP-mining entry (tests/gpu_util.Guarded): every device operand of dm_clipmine_rank in ONE allocation.  A
store outside an operand changes a guard byte; a load outside one that reaches a result makes the result depend on the fill byte.
Results are bit-equal under both fills and equal to the plain run; guards and inputs stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import clipmine as CM  # noqa: E402
from tests import clipmine_cases as CC  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402

OUTPUTS = ("maps", "boxes", "d", "count", "feats")


def _call(v, E, n, c, need, stream=None):
    p = CM._p
    return CM._lib().dm_clipmine_rank(stream, p(v["tokens"]), p(v["text"]), E, p(v["desc"]), n, p(v["tables"]), c.kx, c.ky, c.k,
                                      CM.MODES[c.mode], p(v["work"]), need, p(v["maps"]), p(v["boxes"]), p(v["d"]), p(v["count"]),
                                      p(v["feats"]))


@functools.lru_cache(maxsize=None)
def guarded_run(tag, fill):
    c = CC.case(tag)
    E = c.tokens.shape[1]
    desc, tables, need, map_floats = CM.plan_call([(c.size[0], c.size[1], c.gh, c.pw)], E, c.kx, c.ky)
    ins = {"tokens": torch.from_numpy(c.tokens), "text": torch.from_numpy(c.text), "tables": torch.from_numpy(tables.copy()),
           "desc": torch.from_numpy(desc.view(np.uint8).copy())}
    outs = {"work": ((need,), torch.uint8), "maps": ((map_floats,), torch.float32), "boxes": ((1, c.k, 4), torch.int32),
            "d": ((1, c.k), torch.float32), "count": ((1,), torch.int32), "feats": ((1, c.k, E), torch.float32)}
    g = Guarded(ins, outs, fill=fill, device=dev())
    v = g.views()
    with torch.cuda.device(dev()):
        stream = C.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
        assert _call(v, E, 1, c, need, stream) == 0
        torch.cuda.synchronize()
        g.check()
        # what the entry refuses once it has read the table: nothing may be written then either
        assert _call(v, E, 1, c, need // 8, stream) == 9                                     # a workspace that is too small
        small = desc.copy()
        small["H"] = c.kx - 1
        bad_grid = desc.copy()
        bad_grid["P"] += 1
        for table, code in ((small, 6), (bad_grid, 7)):
            w = dict(v, desc=torch.from_numpy(table.view(np.uint8).copy()).to(dev()))
            assert _call(w, E, 1, c, need, stream) == code
        torch.cuda.synchronize()
    g.check()
    return {n: v[n].cpu().numpy().tobytes() for n in OUTPUTS}


@pytest.mark.parametrize("tag", ("g45_diff", "run_out"))
def test_guarded_run_equals_the_plain_run_under_both_fills(tag):
    c = CC.case(tag)
    ff, zero = guarded_run(tag, 0xFF), guarded_run(tag, 0x00)
    assert ff == zero
    boxes, d, count, feats, maps = CM.rank_device([torch.from_numpy(c.tokens).to(dev())], torch.from_numpy(c.text).to(dev()), [c.size],
                                                  return_maps=True, **CC.kwargs(c))
    torch.cuda.synchronize()
    plain = {"maps": maps[0], "boxes": boxes, "d": d, "count": count, "feats": feats}
    for n in OUTPUTS:
        assert plain[n].cpu().numpy().tobytes() == ff[n], n
    assert int(count[0]) == len(c.boxes) and np.array_equal(boxes[0, :len(c.boxes)].cpu().numpy(), c.boxes)
