"""The X-ray evaluation on the GPU (dm_xray_eval: csrc/xray_eval.hip) against the reference's own `aucpr` / `mean_typicallity`
results in tests/golden/xray_ref.npz (tests/make_golden_xray.py) and against the numpy restatement that tests/test_xray_eval.py
pins to them.  Counts are integers: every comparison of counts is exact, and the AUC taken from them is bit-equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import xray as X  # noqa: E402
from tests import xray_cases as XC  # noqa: E402
from tests.gpu_util import Guarded  # noqa: E402
from tests.test_xray_eval import check_against_fixture, same  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xray_ref.npz")
MAP_TAGS = tuple(t for t in XC.ORDER if t != "a2")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def host_maps():
    return {t: XC.case_map(t) for t in MAP_TAGS}


def pack(host_maps, tags):
    """the rows' maps as views of ONE device buffer, back to back in first-appearance order (a map named twice lies there once)"""
    order = []
    for t in tags:
        t = "a" if t == "a2" else t
        if t not in order:
            order.append(t)
    buf = torch.from_numpy(np.concatenate([host_maps[t].ravel() for t in order])).cuda()
    at, views = 0, {}
    for t in order:
        H, W = host_maps[t].shape
        views[t] = buf[at:at + H * W].view(H, W)
        at += H * W
    return [views["a" if t == "a2" else t] for t in tags]


def run(host_maps, tags, thresholds=None, work=None):
    got = X.xray_eval(pack(host_maps, tags), [XC.case_box(t) for t in tags], thresholds, work)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


def bits_equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def batch(host_maps):
    """the nine rows in one call, computed once and left unchanged"""
    views = pack(host_maps, XC.ORDER)
    assert views[XC.ORDER.index("e")].storage_offset() % 2 == 1          # case e: an odd map_offset (the scalar-load path)
    assert views[XC.ORDER.index("a2")].data_ptr() == views[0].data_ptr()  # one map under two boxes
    return run(host_maps, XC.ORDER)


def test_batch_equals_the_reference(gold, host_maps, batch):
    tp, fp, n_in, box_sum = batch
    assert tp.dtype == fp.dtype == n_in.dtype == np.int32 and box_sum.dtype == np.float64 and tp.shape == (9, 1000)
    for b, tag in enumerate(XC.ORDER):
        check_against_fixture(gold, tag, tp[b], fp[b], n_in[b], box_sum[b])         # counts exact, auc bit for bit
        fs = float(gold[f"{tag}_fsum"])
        if np.isnan(fs):
            assert np.isnan(box_sum[b]), tag
        else:
            bound = int(n_in[b]) * 2.0 ** -53 * XC.box_fsum(host_maps["a" if tag == "a2" else tag], XC.case_box(tag))[1]
            print(f"{tag}: |box_sum - fsum| {abs(box_sum[b] - fs):.3e} (bound {bound:.3e})")
            assert abs(box_sum[b] - fs) <= bound, tag
    host = X.xray_counts_host([host_maps["a" if t == "a2" else t] for t in XC.ORDER], [XC.case_box(t) for t in XC.ORDER])
    assert all(same(g, h) for g, h in zip(batch[:3], host[:3]))


@pytest.mark.parametrize("tag", XC.SHORT_TABLES)
def test_short_threshold_tables(gold, host_maps, tag):
    tp, fp, n_in, box_sum = run(host_maps, ["a"], XC.short_table(tag))
    check_against_fixture(gold, tag, tp[0], fp[0], n_in[0], box_sum[0])


def test_longest_threshold_table(host_maps):
    """T = DM_XRAY_MAX_THRESHOLDS: the histograms and the table need more LDS than a kernel gets without asking."""
    table = 2 * 10 ** (-np.linspace(2, 7, X.XRAY_MAX_THRESHOLDS))
    got = run(host_maps, ["a", "e"], table)
    host = X.xray_counts_host([host_maps["a"], host_maps["e"]], [XC.case_box("a"), XC.case_box("e")], table)
    assert all(same(g, h) for g, h in zip(got[:3], host[:3]))


def test_rows_do_not_depend_on_their_place(host_maps, batch):
    rev = run(host_maps, XC.ORDER[::-1])                         # permuted: other offsets, other alignments, other blockIdx.y
    for b, tag in enumerate(XC.ORDER):
        alone = run(host_maps, [tag])                            # alone: the map at the start of its own allocation
        here = tuple(a[b:b + 1] for a in batch)
        there = tuple(a[len(XC.ORDER) - 1 - b:len(XC.ORDER) - b] for a in rev)
        assert bits_equal(alone, here) and bits_equal(alone, there), tag


def test_calls_repeat_and_ignore_the_workspace(host_maps, batch):
    assert bits_equal(run(host_maps, XC.ORDER), batch)
    need = X.workspace_bytes(len(XC.ORDER), 1000, max(m.size for m in host_maps.values()))
    work = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run(host_maps, XC.ORDER, work=work)
    assert bits_equal(got, batch)


def test_refusals_launch_nothing():
    lib = X._lib()
    maps = torch.zeros(16, dtype=torch.float32, device="cuda")
    out = torch.full((4096,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def call(desc_row, thr):
        desc = np.zeros(1, dtype=X.XRAY_DESC_DTYPE)
        desc[0] = desc_row
        d = torch.from_numpy(desc.view(np.uint8)).cuda()
        t = torch.from_numpy(np.asarray(thr, dtype=np.float64)).cuda()
        rc = lib.dm_xray_eval(p(maps), p(d), 1, p(t), len(thr), p(out), p(out), p(out), p(out), p(out), None)
        torch.cuda.synchronize()
        return rc
    ok = (0, 4, 4, 0, 0, 2, 2)
    assert call(ok, [0.2, 0.2]) == 4 and call(ok, [0.1, 0.2]) == 4 and call(ok, [0.2, float("nan")]) == 4
    assert call((0, 4096, 4096, 0, 0, 2, 2), [0.5]) == 6
    assert call((0, 0, 4, 0, 0, 2, 2), [0.5]) == 5
    assert call((0, 4, 4, 0, -1, 2, 2), [0.5]) == 7
    assert lib.dm_xray_eval(p(maps), p(out), 1, p(out), 0, p(out), p(out), p(out), p(out), p(out), None) == 3
    assert lib.dm_xray_eval(p(maps), p(out), 1, p(out), 4097, p(out), p(out), p(out), p(out), p(out), None) == 3
    assert lib.dm_xray_eval(p(maps), p(out), 0, p(out), 1, p(out), p(out), p(out), p(out), p(out), None) == 2
    assert lib.dm_xray_eval(None, p(out), 1, p(out), 1, p(out), p(out), p(out), p(out), p(out), None) == 1
    assert lib.dm_xray_eval_workspace_bytes(1, 1000, 1 << 24) == 0 and lib.dm_xray_eval_workspace_bytes(1, 4097, 16) == 0
    assert bool((out == -7).all())
    with pytest.raises(ValueError):
        X.xray_eval([maps.view(4, 4)], [(0, 0, -1, 2)])
    with pytest.raises(E.EngineError):
        X.xray_eval([maps.view(4, 4).cpu()], [(0, 0, 2, 2)])


def test_guard_bands(host_maps, batch):
    """Cases b and e with every device operand of the call inside one guarded allocation: no byte outside a payload changes, no
    input changes, and the results do not depend on what lies around them."""
    tags = ("b", "e")
    thr = X.xray_thresholds()
    desc = np.zeros(2, dtype=X.XRAY_DESC_DTYPE)
    at = 0
    for r, t in enumerate(tags):
        H, W = host_maps[t].shape
        desc[r] = (at, H, W) + tuple(XC.case_box(t))
        at += H * W
    assert desc[1]["map_offset"] % 2 == 1
    need = X.workspace_bytes(2, len(thr), int(max(host_maps[t].size for t in tags)))
    inputs = {"maps": torch.from_numpy(np.concatenate([host_maps[t].ravel() for t in tags])),
              "desc": torch.from_numpy(desc.view(np.uint8).copy()), "thr": torch.from_numpy(thr.copy())}
    outputs = {"work": ((need,), torch.uint8), "tp": ((2, len(thr)), torch.int32), "fp": ((2, len(thr)), torch.int32),
               "n_in": ((2,), torch.int32), "box_sum": ((2,), torch.float64)}
    rows = [XC.ORDER.index(t) for t in tags]
    plain = tuple(a[rows] for a in batch)
    for fill in (0xFF, 0x00):
        g = Guarded(inputs, outputs, fill=fill, device="cuda")
        v = g.views()
        p = lambda name: C.c_void_p(v[name].data_ptr())          # noqa: E731,B023
        rc = X._lib().dm_xray_eval(p("maps"), p("desc"), 2, p("thr"), len(thr), p("work"), p("tp"), p("fp"), p("n_in"), p("box_sum"),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        g.check()
        got = tuple(v[n].cpu().numpy() for n in ("tp", "fp", "n_in", "box_sum"))
        assert bits_equal(got, plain), hex(fill)


# ---- end to end: grids -> per-pixel maps -> counts, the maps never leaving the device ------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = E.UNetEngine(0)                      # the map and evaluation entry points need no weights
    yield e
    e.close()


def test_xray_evaluate_end_to_end(gold, engine):
    from diff_mining_amd.typicality import TypicalityScorer
    sc = TypicalityScorer(engine)
    grids = [XC.e2e_grid(j) for j in range(XC.E2E_N)]
    sizes, boxes = [XC.E2E_SIZE] * XC.E2E_N, list(XC.E2E_BOXES)
    for j, g in enumerate(grids):
        assert XC.digest(g.numpy()) == str(gold[f"e2e{j}_sha256"])
    got = sc.xray_evaluate(grids, sizes, boxes, images_per_call=2)
    assert got["mean_typicality"].dtype == np.float32 and got["auc"].dtype == np.float64 and got["auc"].shape == (XC.E2E_N,)
    # (i) the engine's own maps on the host: counts equal exactly, scores bit for bit
    maps = engine.typicality_image_batched(grids, sizes, 1, 1)
    tp, fp, n_in, box_sum = (a.cpu().numpy() for a in engine.xray_eval(maps, boxes))
    host = X.xray_counts_host([m.cpu().numpy() for m in maps], boxes)
    assert same(tp, host[0]) and same(fp, host[1]) and same(n_in, host[2])
    mean, auc = X.xray_scores_from_counts(tp, fp, n_in, box_sum)
    assert mean.tobytes() == got["mean_typicality"].tobytes() and auc.tobytes() == got["auc"].tobytes()
    # (ii) the reference's path (Typicallity.compute on the CPU, then its aucpr), recorded in the fixture.  The engine's map is held to
    # atol + rtol |v| of the reference's (tests/test_gpu_e2e.py, kx = ky = 1), so a count at thr[k] can differ by no more than the
    # reference pixels that lie within that distance of thr[k], on either side of the box
    assert tuple(gold["e2e_tol"]) == (2e-5, 1e-4)
    for j in range(XC.E2E_N):
        band_in, band_out = gold[f"e2e{j}_band_in"].astype(np.int64), gold[f"e2e{j}_band_out"].astype(np.int64)
        assert (band_in + band_out).max() < 0.01 * XC.E2E_SIZE[0] * XC.E2E_SIZE[1]          # the bound cannot swallow a wrong kernel
        d_tp = np.abs(tp[j].astype(np.int64) - gold[f"e2e{j}_tp"])
        d_fp = np.abs(fp[j].astype(np.int64) - gold[f"e2e{j}_fp"])
        print(f"e2e{j}: max |d tp| {d_tp.max()} (band up to {band_in.max()}), max |d fp| {d_fp.max()} (band up to {band_out.max()}); "
              f"auc {auc[j]!r} against {float(gold[f'e2e{j}_auc'])!r}; mean {mean[j]!r} against {float(gold[f'e2e{j}_mean'])!r}")
        assert int(n_in[j]) == int(gold[f"e2e{j}_n_in"])
        assert (d_tp <= band_in).all() and (d_fp <= band_out).all(), j
        # the mean of pixels that are each within atol + rtol |v| of the reference's, |v| <= 0.2 (the grids' range)
        assert abs(float(mean[j]) - float(gold[f"e2e{j}_mean"])) <= 2e-5 + 1e-4 * 0.2, j
