"""Guard bands around the detectors' SVMs (tests/gpu_util.Guarded): `ties`, `hard264` and `wide` (the feature limit) with every device operand of both entry
points in ONE allocation.  A store outside an operand changes a guard byte; a load outside one that reaches the result — or a read
of workspace nothing has written — makes the result depend on the fill byte.  Results are bit-equal to the plain run under both
fills; guards and inputs stay untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import svm_cases as SC  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402

PAD = 5          # table columns past the last sample: never read, and written only with the documented fillers
CASES = {"ties": ("ties", 1.0, 0, 80), "hard264": ("hard264", 1.0, 20, 5), "wide": ("wide", 1.0, 0, 4)}      # tag -> data, cost, n_hn, max_samples
OUTPUTS = ("w", "b", "n_iter", "status", "alpha", "score", "hard", "count")


def operands(tag):
    data, cost, n_hn, max_samples = CASES[tag]
    X = SC.case_rows(data, SC.fixture())
    n, n_pos = len(X), SC.CASES[data]["n_pos"]
    table = np.full((1, n + PAD), 1 << 30, dtype=np.int32)
    table[0, :n] = np.arange(n)
    ins = {"pool": torch.from_numpy(X), "table": torch.from_numpy(table), "n": torch.tensor([n], dtype=torch.int32),
           "n_pos": torch.tensor([n_pos], dtype=torch.int32), "first": torch.tensor([n_pos + n_hn], dtype=torch.int32),
           "max_samples": torch.tensor([max_samples], dtype=torch.int32)}
    return ins, cost, n, X.shape[1]


def run(v, cost, n, C_, work_bytes):
    lib, stream, ptr = D._lib(), D._stream(torch, dev()), D._p
    ld = n + PAD
    assert lib.dm_svm_fit(stream, ptr(v["pool"]), n, C_, ptr(v["table"]), ld, ptr(v["n"]), ptr(v["n_pos"]), 1, cost, 1e-3, -1,
                          ptr(v["work"]), work_bytes, ptr(v["w"]), ptr(v["b"]), ptr(v["n_iter"]), ptr(v["status"]), ptr(v["alpha"])) == 0
    assert lib.dm_svm_hard_negatives(stream, ptr(v["pool"]), n, C_, ptr(v["table"]), ld, ptr(v["n"]), ptr(v["first"]),
                                     ptr(v["max_samples"]), 1, ptr(v["w"]), ptr(v["b"]), ptr(v["work"]), work_bytes, ptr(v["score"]),
                                     ptr(v["hard"]), ptr(v["count"])) == 0
    torch.cuda.synchronize()


def out_specs(n, C_, need):
    ld = n + PAD
    return {"work": ((need,), torch.uint8), "w": ((1, C_), torch.float64), "b": ((1,), torch.float64), "n_iter": ((1,), torch.int32),
            "status": ((1,), torch.int32), "alpha": ((1, ld), torch.float64), "score": ((1, ld), torch.float64),
            "hard": ((1, ld), torch.int32), "count": ((1,), torch.int32)}


_plain = {}


def plain(tag):
    if tag not in _plain:
        ins, cost, n, C_ = operands(tag)
        need = D.svm_workspace_bytes(1, n + PAD)
        v = {name: t.to(dev()) for name, t in ins.items()}
        v.update({name: torch.empty(shape, dtype=dt, device=dev()) for name, (shape, dt) in out_specs(n, C_, need).items()})
        run(v, cost, n, C_, need)
        _plain[tag] = {name: v[name].cpu().numpy() for name in OUTPUTS}
    return _plain[tag]


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ff", "00"))
@pytest.mark.parametrize("tag", tuple(CASES))
def test_guarded_run_equals_the_plain_run(tag, fill):
    ins, cost, n, C_ = operands(tag)
    need = D.svm_workspace_bytes(1, n + PAD)
    g = Guarded(ins, out_specs(n, C_, need), fill=fill, device=dev())
    v = g.views()
    run(v, cost, n, C_, need)
    g.check()
    want = plain(tag)
    for name in OUTPUTS:
        assert v[name].cpu().numpy().tobytes() == want[name].tobytes(), name
    data, _, n_hn, max_samples = CASES[tag]
    hard = SC.expected_hard(SC.fixture()[f"{data}_c1_hard" if tag == "ties" else f"{data}_hard"], SC.CASES[data]["n_pos"] + n_hn, max_samples)
    assert int(want["status"][0]) == D.SVM_CONVERGED and np.array_equal(want["hard"][0, :int(want["count"][0])], hard)
    assert (want["alpha"][0, n:] == 0).all() and (want["hard"][0, n:] == -1).all() and np.isnan(want["score"][0, n:]).all()
