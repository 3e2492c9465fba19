"""The guard-band helper of the GPU operator tests (tests/gpu_util.py: Guarded) on CPU tensors: a fake operator that behaves, and three
that do not — one row too many behind its output, one element in front of it, a store into an input.  check() must pass the first and
name the tensor, the side and the byte offsets of each of the others: the detector detects."""
import pytest
import torch

from tests import gpu_util as U

M, K, C = 5, 8, 6


def _operands(fill):
    x = torch.arange(M * K, dtype=torch.float32).view(M, K).half()
    w = (torch.arange(C * K, dtype=torch.float32).view(C, K) % 7 - 3).half()
    return U.Guarded({"x": x, "w": w}, {"y": ((M, C), torch.float16), "work": ((3,), torch.int32)}, fill=fill), x, w


def _rows(t, first, n):
    """rows [first, first + n) of the 2-D view `t`, whether or not they lie inside it (the storage is the whole guarded allocation)"""
    return torch.as_strided(t, (n, t.shape[1]), t.stride(), t.storage_offset() + first * t.stride(0))


def _fake_op(v, rows=M, first_row=0, touch_input=False, front_element=False):
    y = (v["x"].float() @ v["w"].float().T).half()
    out = _rows(v["y"], first_row, rows)
    out.copy_(torch.cat([y, y])[:rows])
    v["work"].fill_(7)
    if front_element:
        torch.as_strided(v["y"], (1,), (1,), v["y"].storage_offset() - 1).fill_(1.0)
    if touch_input:
        v["w"][2, 3] = 9.0


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_layout_and_clean_pass(fill):
    g, x, w = _operands(fill)
    for name, (front, start, end, back, shape, dt, is_input) in g.layout.items():
        es = torch.empty(0, dtype=dt).element_size()
        assert g.offset(name) % 512 == 256                                  # an odd multiple of 256
        need = max(256 * shape[-1] * es if len(shape) >= 2 else 0, 64 * 1024)
        assert start - front >= need and back - end >= need and (back - front) % 256 == 0
        assert (g.buf[front:start] == fill).all() and (g.buf[end:back] == fill).all()
        if not is_input:
            assert (g.buf[start:end] == fill).all()
    assert g.buf.data_ptr() + g.layout["x"][0] == g.buf.data_ptr()          # one allocation, the regions back to back
    assert [g.layout[a][3] for a in ("x", "w", "y")] == [g.layout[b][0] for b in ("w", "y", "work")]
    if fill == 0xFF:
        assert torch.isnan(g.view("y")).all() and (g.view("work") == -1).all()
    assert torch.equal(g.view("x"), x) and torch.equal(g.view("w"), w)
    assert torch.equal(g.view("x")[:, 2:5], x[:, 2:5]) and g.view("x")[:, 2:5].stride() == (K, 1)      # strided sub-views work on top
    g.check()
    _fake_op(g.views())
    g.check()                                                               # outputs and workspaces may change; nothing else did
    assert torch.equal(g.view("y"), (x.float() @ w.float().T).half()) and (g.view("work") == 7).all()


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_one_row_too_many_behind_the_output(fill):
    g, _, _ = _operands(fill)
    _fake_op(g.views(), rows=M + 1)
    with pytest.raises(U.GuardViolation) as e:
        g.check()
    v = e.value
    assert (v.name, v.side) == ("y", "back") and 0 <= v.first <= v.last <= C * 2 - 1 and 1 <= v.count <= C * 2      # (a byte that equals the fill does not count)
    assert "y" in str(v) and "back" in str(v)


def test_one_row_too_many_is_reported_to_the_byte():
    g, _, _ = _operands(0xFF)
    _fake_op(g.views())
    _rows(g.view("y"), M, 1).fill_(1.0)                      # 0x3C00 per element: both bytes differ from 0xFF
    with pytest.raises(U.GuardViolation) as e:
        g.check()
    v = e.value
    assert (v.name, v.side, v.first, v.last, v.count) == ("y", "back", 0, C * 2 - 1, C * 2)


def test_one_element_in_front_of_the_output():
    g, _, _ = _operands(0xFF)
    _fake_op(g.views(), front_element=True)
    with pytest.raises(U.GuardViolation) as e:
        g.check()
    v = e.value
    assert (v.name, v.side, v.first, v.last, v.count) == ("y", "front", -2, -1, 2)


def test_a_store_into_an_input():
    g, _, w = _operands(0x00)
    _fake_op(g.views(), touch_input=True)
    with pytest.raises(U.GuardViolation) as e:
        g.check()
    v = e.value
    first = (2 * K + 3) * 2
    assert w[2, 3].item() == 2.0                              # 0x4000 -> 0x4880: both bytes change
    assert (v.name, v.side, v.first, v.last, v.count) == ("w", "payload", first, first + 1, 2)


def test_an_output_that_starts_one_row_early_hits_the_front_guard():
    g, _, _ = _operands(0x00)
    _fake_op(g.views(), first_row=-1)
    with pytest.raises(U.GuardViolation) as e:
        g.check()
    v = e.value
    assert (v.name, v.side) == ("y", "front") and -C * 2 <= v.first <= v.last <= -1
