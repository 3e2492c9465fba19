"""The dense detector search on the GPU (csrc/dense_search.hip through diff-mining_amd/doersch.py) against the exact expectation of
tests/golden/dense_search_ref.npz: cells and image order equal, fp32 scores within the case's tol32 (8 x the deviation of a numpy
fp32 matmul from fp64; every gap the comparison relies on is at least 16 tol32, tests/make_golden_dense_search.py)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import dense_search_cases as DC  # noqa: E402
from tests.gpu_util import dev  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(DC.NPZ)


@pytest.fixture(scope="module")
def tol32():
    with open(DC.JSON) as f:
        return {k: v["tol32"] for k, v in json.load(f)["cases"].items()}


_inputs, _searches = {}, {}


def inputs(tag):
    """(w fp16 [K, C], [(paths, data, mask), ...]) of the case on the host: generated once"""
    if tag not in _inputs:
        seed = DC.seeds()[tag]
        _inputs[tag] = (DC.detectors(tag, seed), DC.chunks(tag, seed))
    return _inputs[tag]


def search(tag, only_pos=False, fresh=False, **kw):
    """the device search over the case's chunks; computed once per (case, only_pos) unless `fresh`"""
    key = (tag, only_pos)
    if fresh or key not in _searches:
        w, chunks = inputs(tag)
        ds = D.DenseSearch(w, top_k=DC.SHAPES[tag]["top_k"], only_pos=only_pos, keep_rows=True, scores="f32", **kw)
        for paths, data, mask in chunks:
            ds.add(paths, torch.from_numpy(data).to(dev()), None if mask is None else torch.from_numpy(mask).to(dev()))
        torch.cuda.synchronize()
        if fresh:
            return ds
        _searches[key] = ds
    return _searches[key]


def assert_close_to_fixture(gold, tol, tag, ds, sfx=""):
    score, cell = ds.tables()
    want = gold[f"{tag}_score"]
    assert score.dtype == np.float32 and cell.dtype == np.int32
    assert np.array_equal(cell, gold[f"{tag}_cell"]), tag
    inf = want == -np.inf
    assert np.array_equal(score == -np.inf, inf)
    err = np.abs(score[~inf].astype(np.float64) - want[~inf]).max()
    print(f"{tag}{sfx}: max |score - exact| = {err:.3g}, tol32 = {tol:.3g}")
    assert err <= tol, (tag, err, tol)
    assert np.array_equal(score == 0, want == 0)                                     # a masked zero is exactly zero
    top_score, top_image, top_cell, count = ds.topk()
    assert np.array_equal(count, gold[f"{tag}_count{sfx}"])
    assert np.array_equal(top_image, gold[f"{tag}_top_image{sfx}"]) and np.array_equal(top_cell, gold[f"{tag}_top_cell{sfx}"])
    want = gold[f"{tag}_top_score{sfx}"]
    assert np.array_equal(np.isnan(top_score), np.isnan(want))
    assert (np.abs(top_score.astype(np.float64) - want)[~np.isnan(want)] <= tol).all()
    for k in range(len(count)):                                                      # the top-k copies its scores from the table
        for j in range(int(count[k])):
            assert top_score[k, j] == score[k, top_image[k, j]]


@pytest.mark.parametrize("tag", DC.ORDER)
def test_case_equals_the_exact_expectation(gold, tol32, tag):
    ds = search(tag)
    assert_close_to_fixture(gold, tol32[tag], tag, ds)
    if tag == "S4":
        assert_close_to_fixture(gold, tol32[tag], tag, search(tag, only_pos=True), "_pos")
    # ret_ws: bit copies of data[image, cell]
    _, chunks = inputs(tag)
    data = np.concatenate([c[1] for c in chunks], axis=0)
    data = data.reshape(data.shape[0], -1, data.shape[-1])
    names = DC.paths(tag)
    H = DC.SHAPES[tag]["H"]
    lists = ds.result(ret_ws=True)
    assert sum(len(e) for e in lists) == int(gold[f"{tag}_count"].sum())
    for k, entries in enumerate(lists):
        for j, (score, bbox, path, row) in enumerate(entries):
            b, cell = names.index(path), (bbox[0] // 8) * H + bbox[1] // 8
            assert (b, cell) == (gold[f"{tag}_top_image"][k, j], gold[f"{tag}_top_cell"][k, j])
            assert row.dtype == np.float16 and row.tobytes() == data[b, cell].tobytes(), (tag, k, j)


@pytest.mark.parametrize("tag", ("S2", "S3"))
def test_two_runs_are_bit_equal(tag):
    a, b = search(tag), search(tag, fresh=True)
    for x, y in zip(a.tables() + a.topk(), b.tables() + b.topk()):
        assert x.tobytes() == y.tobytes()


def _tables(K, ld):
    return (torch.full((K, ld), 7.0, dtype=torch.float32, device=dev()), torch.full((K, ld), -7, dtype=torch.int32, device=dev()))


def test_a_column_does_not_depend_on_where_the_image_travels():
    """the last image of S2's second chunk: alone, as the last of its chunk of 4, and at image_offset 5 — the same bits; and a call
    writes its own columns only"""
    w, chunks = inputs("S2")
    _, data, mask = chunks[1]
    B, cells, C_ = data.shape[0], data.shape[1] * data.shape[2], data.shape[3]
    wd = torch.from_numpy(w).to(dev())
    dd, md = torch.from_numpy(data).to(dev()).view(B, cells, C_), torch.from_numpy(mask).to(dev())
    s4, c4 = _tables(70, 4)
    D.winners(dd, wd, s4, c4, 0, md)
    s1, c1 = _tables(70, 1)
    D.winners(dd[3:].contiguous(), wd, s1, c1, 0, md[3:].contiguous())
    s9, c9 = _tables(70, 9)
    D.winners(dd[3:].contiguous(), wd, s9, c9, 5, md[3:].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(s4[:, 3], s1[:, 0]) and torch.equal(c4[:, 3], c1[:, 0])
    assert torch.equal(s4[:, 3], s9[:, 5]) and torch.equal(c4[:, 3], c9[:, 5])
    keep = [j for j in range(9) if j != 5]
    assert (s9[:, keep] == 7.0).all() and (c9[:, keep] == -7).all()
    assert (c4 >= 0).all() and torch.isfinite(s4).all()


def test_detectors_do_not_depend_on_their_company():
    """detectors 0 ... 4 of S2 alone (one column tile) against the same five among the 70 (five column tiles)"""
    w, chunks = inputs("S2")
    few = D.DenseSearch(w[:5], top_k=5, scores="f32")
    for paths, data, mask in chunks:
        few.add(paths, torch.from_numpy(data).to(dev()), torch.from_numpy(mask).to(dev()))
    a, b = few.tables(), search("S2").tables()
    assert a[0].tobytes() == b[0][:5].tobytes() and a[1].tobytes() == b[1][:5].tobytes()
    for x, y in zip(few.topk(), search("S2").topk()):
        assert x.tobytes() == y[:5].tobytes()


def test_drop_in_on_shards(tmp_path, gold, tol32):
    from safetensors.torch import save_file
    w, chunks = inputs("S2")
    shards = []
    for j, (paths, data, _) in enumerate(chunks):
        shards.append(str(tmp_path / f"{j}.safetensors"))
        save_file({";;".join(paths): torch.from_numpy(data)}, shards[-1])
    plain = [(p, d, None) for p, d, _ in chunks]
    want = D.dense_search_host(w, plain, top_k=5, ret_ws=True, scores="f32")
    want16 = D.dense_search_host(w, plain, top_k=5)
    got = D.dense_search(w.astype(np.float32), shards, top_k=5, ret_ws=True, device_id="cuda", scores="f32")
    half = D.dense_search(w.astype(np.float32), shards, top_k=5, device_id="cuda")
    assert len(got) == len(half) == 70
    for a, b, h, h_host in zip(got, want, half, want16):
        assert len(a) == len(b) == len(h) == 5
        assert h == h_host                                                           # the shown fp16 scores: the same rows, the same host sum
        for x, y, z in zip(a, b, h):
            assert x[1:3] == y[1:3] == z[1:3] and x[3].tobytes() == y[3].tobytes()
            assert x[0].dtype == np.float32 and abs(float(x[0]) - float(y[0])) <= tol32["S2"]
            # the reference's arithmetic against the fp32 sum: each fp16 product is off by at most 2^-11 of itself and the products of
            # two unit vectors sum to at most 1 in magnitude; the last rounding adds half an fp16 unit below 1
            assert type(z[0]) is np.float16 and abs(float(z[0]) - float(x[0])) <= 2.0 ** -11 + 2.0 ** -12
    # fold: the mask is drawn on the device (torch-ROCm's bits); the same draw, taken to the host, gives the same lists
    got = D.dense_search(w.astype(np.float32), shards, top_k=5, fold=(1, 3), device_id="cuda", scores="f32")
    masked = [(p, d, D.fold_mask(j, len(p), 63, (1, 3), dev()).cpu().numpy()) for j, (p, d, _) in enumerate(chunks)]
    assert all(int(m.sum()) == 21 * len(p) for p, _, m in masked)
    want = D.dense_search_host(w, masked, top_k=5, scores="f32")
    for a, b in zip(got, want):
        assert [x[1:3] for x in a] == [y[1:3] for y in b]
