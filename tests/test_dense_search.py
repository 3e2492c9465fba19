"""CPU tier of the dense detector search (diff-mining_amd/doersch.py): the numpy restatement against the exact expectation and the
reference's own lists (tests/golden/dense_search_ref.npz / .json, written by tests/make_golden_dense_search.py), the rules, the
shard reader, and the refusals of the C entry points (they return before any HIP call)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from diff_mining_amd import doersch as D
from diff_mining_amd import engine as E
from tests import dense_search_cases as DC


@pytest.fixture(scope="module")
def gold():
    return np.load(DC.NPZ)


@pytest.fixture(scope="module")
def report():
    with open(DC.JSON) as f:
        return json.load(f)


_searches = {}


def host_search(tag, only_pos=False):
    """the host restatement over the case's chunks; computed once per (case, only_pos) and never changed"""
    if (tag, only_pos) not in _searches:
        seed = DC.seeds()[tag]
        ds = D.DenseSearch(DC.detectors(tag, seed), top_k=DC.SHAPES[tag]["top_k"], only_pos=only_pos, keep_rows=True, scores="f32")
        for paths, data, mask in DC.chunks(tag, seed):
            ds.add(paths, data, mask)
        _searches[(tag, only_pos)] = ds
    return _searches[(tag, only_pos)]


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def assert_equals_fixture(gold, tag, tables, top, sfx=""):
    score, cell = tables
    if not sfx:
        assert same(score, gold[f"{tag}_score"]) and same(cell, gold[f"{tag}_cell"]), tag
    for got, name in zip(top, ("top_score", "top_image", "top_cell", "count")):
        assert same(got, gold[f"{tag}_{name}{sfx}"]), (tag, name + sfx)


@pytest.mark.parametrize("tag", DC.ORDER + ("S4clean",))
def test_host_equals_the_exact_expectation(gold, tag):
    """cells, image order and fp32 scores, bit for bit: both sides are the fp64 sum rounded to fp32 once"""
    ds = host_search(tag)
    assert_equals_fixture(gold, tag, ds.tables(), ds.topk())
    if tag.startswith("S4"):
        pos = host_search(tag, only_pos=True)
        assert_equals_fixture(gold, tag, pos.tables(), pos.topk(), "_pos")


def test_the_gaps_the_tests_rely_on(report):
    """what the generator asserted, read back: every winner / rank / zero gap is at least 16 tol32, so no pair is left out"""
    assert report["gap_factor"] == 16 and "dense_search_cuda" in report["reference_route"]
    for tag in DC.ORDER:
        c = report["cases"][tag]
        assert c["tol32"] == 8 * c["fp32_matmul_dev"] and 0 < c["tol32"] < 1e-5
        assert min(c["winner_gap"], c["rank_gap"], c.get("zero_gap", np.inf)) >= 16 * c["tol32"], tag
    assert report["cases"]["S2"]["seed"] == report["cases"]["S4"]["seed"] == report["cases"]["S4clean"]["seed"]


@pytest.mark.parametrize("tag,mine", [("S1", "S1"), ("S2", "S2"), ("S4", "S4clean")])
def test_host_against_the_references_lists(gold, tag, mine):
    """Every (detector, rank): the same image and cell as the reference's list, or the reference's own fp16 score of this library's
    choice within 2 ref_err of the reference's score at that rank (a near-tie of its fp16 arithmetic); at most 2 % of the entries
    take the second branch."""
    s = DC.SHAPES[mine]
    seed = DC.seeds()[mine]
    lists = D.dense_search_host(DC.detectors(mine, seed), DC.chunks(mine, seed), top_k=s["top_k"])
    ref_score, ref_bbox, ref_image = gold[f"{tag}_ref_score"], gold[f"{tag}_ref_bbox"], gold[f"{tag}_ref_image"]
    ref_full, ref_err = gold[f"{tag}_ref_full"].astype(np.float64), float(gold[f"{tag}_ref_err"])
    names = DC.paths(mine)
    assert len(lists) == s["K"] and 0 < ref_err < 4e-3
    second = total = 0
    for k, entries in enumerate(lists):
        assert len(entries) == s["top_k"] == ref_score.shape[1]
        for j, (score, bbox, path) in enumerate(entries):
            assert type(score) is np.float16
            img, cell = names.index(path), (bbox[0] // 8) * s["H"] + bbox[1] // 8
            total += 1
            if img == ref_image[k, j] and tuple(bbox) == tuple(ref_bbox[k, j]):
                continue
            second += 1
            assert abs(ref_full[k, img, cell] - float(ref_score[k, j])) <= 2 * ref_err, (tag, k, j)
    assert second <= 0.02 * total, (tag, second, total)


@pytest.mark.parametrize("tag,mine", [("S1", "S1"), ("S2", "S2"), ("S4", "S4clean")])
def test_fp16_scores_equal_the_references_within_ref_err(gold, tag, mine):
    """The fp16 score of every (detector, rank) against the reference's score at that rank, within ref_err = max |reference fp16
    score - exact| of the case.  ref_err is about half an fp16 unit (2.55e-4 on S1, 3.64e-4 on S2, against a unit of 4.88e-4 in
    [0.5, 1)) and two fp16 numbers are equal or a whole unit apart, so in [0.5, 1) this asks for the reference's own value: the
    shown fp16 score is `reference_score_f16`, the reference's arithmetic (fp16 products, summed, rounded to fp16) on the winning
    row, not a rounding of the fp32 score (which misses the bound on 1 of 10 entries of S1 and 3 of 350 of S2, by one unit)."""
    s, seed = DC.SHAPES[mine], DC.seeds()[mine]
    lists = D.dense_search_host(DC.detectors(mine, seed), DC.chunks(mine, seed), top_k=s["top_k"])
    ref_score, ref_err = gold[f"{tag}_ref_score"], float(gold[f"{tag}_ref_err"])
    diff = np.array([[abs(float(e[0]) - float(ref_score[k, j])) for j, e in enumerate(entries)] for k, entries in enumerate(lists)])
    print(f"{tag}: ref_err {ref_err:.3g}; {int((diff > 0).sum())} of {diff.size} fp16 scores differ, {int((diff > ref_err).sum())} by more "
          f"than ref_err, the largest by {diff.max():.3g}")
    assert (diff <= ref_err).all(), (tag, int((diff > ref_err).sum()), float(diff.max()), ref_err)


def test_fp32_scores_lie_within_ref_err_of_the_references(gold):
    """what the fp16 comparison above cannot show: before the last rounding the scores are as close to the reference's as the
    reference is to the exact sum (one fp32 rounding allowed for)"""
    for tag, mine in (("S1", "S1"), ("S2", "S2"), ("S4", "S4clean")):
        s, seed = DC.SHAPES[mine], DC.seeds()[mine]
        lists = D.dense_search_host(DC.detectors(mine, seed), DC.chunks(mine, seed), top_k=s["top_k"], scores="f32")
        ref_score, ref_err = gold[f"{tag}_ref_score"], float(gold[f"{tag}_ref_err"])
        for k, entries in enumerate(lists):
            for j, e in enumerate(entries):
                assert abs(float(e[0]) - float(ref_score[k, j])) <= ref_err + 2.0 ** -24 * 3, (tag, k, j)


def test_rules_on_s4(gold):
    seed = DC.seeds()["S4"]
    ds, pos = host_search("S4"), host_search("S4", only_pos=True)
    score, cell = ds.tables()
    w64 = DC.detectors("S4", seed).astype(np.float64)
    f = DC.features("S4", seed).reshape(7, 63, -1)
    mask = np.concatenate(DC.masks("S4"), axis=0)
    with np.errstate(all="ignore"):
        raw = np.einsum("bic,kc->kbi", f.astype(np.float64), w64)                   # unmasked exact scores [K, n, cells]
    # a masked zero over negatives, and the lowest index among the equal zeros
    zero = np.argwhere((score == 0) & (cell >= 0))
    assert len(zero) >= 5
    for k, b in zero:
        live = raw[k, b][(mask[b] == 1) & ~np.isnan(raw[k, b])]
        assert (live < 0).all()
        masked = np.nonzero((mask[b] == 0) & ~np.isnan(raw[k, b]))[0]
        assert cell[k, b] == masked[0] and mask[b, cell[k, b]] == 0
    # the NaN row never wins although image 1 is searched; the all-NaN image is absent (-inf, -1; in no list)
    img, row = DC.S4_NAN_ROW
    assert np.isfinite(score[:, img]).all() and not (cell[:, img] == row).any()
    assert (score[:, DC.S4_NAN_IMAGE] == -np.inf).all() and (cell[:, DC.S4_NAN_IMAGE] == -1).all()
    top_score, top_image, top_cell, count = ds.topk()
    assert not (top_image == DC.S4_NAN_IMAGE).any() and (count == 5).all()
    # equal scores: ascending image
    tied = 0
    for k in range(70):
        for j in range(4):
            if top_score[k, j] == top_score[k, j + 1]:
                tied += 1
                assert top_image[k, j] < top_image[k, j + 1]
    assert tied >= 1
    # only_pos: score > 0 only, count below top_k, the unused slots
    p_score, p_image, p_cell, p_count = pos.topk()
    assert (p_count < 5).any() and (p_count == 5).any()
    for k in range(70):
        n = int(p_count[k])
        assert n == min(5, int((score[k] > 0).sum()))
        assert (p_score[k, :n] > 0).all() and np.isnan(p_score[k, n:]).all() and (p_image[k, n:] == -1).all() and (p_cell[k, n:] == -1).all()
    lists = pos.result(ret_ws=True)
    assert [len(e) for e in lists] == list(p_count)
    k = int(np.argmax(p_count > 0))
    s, bbox, path, row = lists[k][0]
    b = DC.paths("S4").index(path)
    assert s == p_score[k, 0] and s.dtype == np.float32                              # scores="f32"
    assert row.dtype == np.float16 and row.tobytes() == f[b, p_cell[k, 0]].tobytes()
    assert bbox == ((p_cell[k, 0] // 7) * 8, (p_cell[k, 0] % 7) * 8)


def test_fold_mask_is_the_references_draw(gold):
    for tag, fold in (("S2", (1, 3)), ("S4", (2, 3))):
        mine = np.concatenate(DC.masks(tag), axis=0)
        assert mine.dtype == np.uint8 and np.array_equal(mine, gold[f"{tag}_ref_mask"]), tag
        assert (mine.sum(axis=1) == fold[0] * 63 // fold[1]).all()
    m = D.fold_mask(3, 2, 10, (1, 2), "cpu")
    assert m.dtype == torch.uint8 and m.shape == (2, 10) and m.sum().item() == 10 and not torch.equal(m[0], m[1])


def test_shard_round_trip_on_the_cpu(tmp_path):
    """`dense_search(..., device_id="cpu")` reads the reference's shard format and takes the numpy path"""
    from safetensors.torch import save_file
    seed = DC.seeds()["S2"]
    w = DC.detectors("S2", seed)
    shards = []
    for j, (paths, data, _) in enumerate(DC.chunks("S2", seed)):
        shards.append(str(tmp_path / f"{j}.safetensors"))
        save_file({";;".join(paths): torch.from_numpy(data)}, shards[-1])
    for fold in (None, (1, 3)):
        chunks = [(p, d, m if fold else None) for p, d, m in DC.chunks("S2", seed)]
        for ret_ws in (False, True):
            got = D.dense_search(w.astype(np.float32), shards, top_k=5, ret_ws=ret_ws, fold=fold, device_id="cpu")
            want = D.dense_search_host(w, chunks, top_k=5, ret_ws=ret_ws)
            assert len(got) == len(want) == 70
            for a, b in zip(got, want):
                assert len(a) == len(b) == 5
                for x, y in zip(a, b):
                    assert x[:3] == y[:3] and type(x[0]) is np.float16
                    if ret_ws:
                        assert x[3].tobytes() == y[3].tobytes() and x[3].shape == (72,)


def test_discriminative_20():
    result = [[(np.float16(1 - j / 64), (0, 0), f"p{j}") for j in range(30)], [(np.float16(0.5), (8, 8), "p3")], []]
    assert D.discriminative_20(result, {"p0", "p3", "p19", "p20", "p29", "other"}) == [3, 1, 0]
    assert D.discriminative_20(result, []) == [0, 0, 0]


def test_host_argument_checks():
    w = np.zeros((2, 16), dtype=np.float16)
    with pytest.raises(ValueError):
        D.DenseSearch(np.zeros((2, 12), dtype=np.float16))                           # C % 8
    with pytest.raises(ValueError):
        D.DenseSearch(np.zeros((129, 16), dtype=np.float16))
    with pytest.raises(ValueError):
        D.DenseSearch(w, top_k=129)
    with pytest.raises(ValueError):
        D.DenseSearch(w, scores="f64")
    ds = D.DenseSearch(w, top_k=1)
    with pytest.raises(ValueError):
        ds.add(["a"], np.zeros((1, 2, 2, 8), dtype=np.float16))
    with pytest.raises(ValueError):
        ds.add(["a", "b"], np.zeros((1, 2, 2, 16), dtype=np.float16))
    with pytest.raises(ValueError):
        ds.result()
    ds.add(["a"], np.ones((1, 2, 2, 16), dtype=np.float16))
    assert len(ds.result(ret_ws=True)[0][0]) == 4                                    # scores="f16" keeps the rows it scores from
    ds32 = D.DenseSearch(w, top_k=1, scores="f32")
    ds32.add(["a"], np.ones((1, 2, 2, 16), dtype=np.float16))
    with pytest.raises(ValueError):
        ds32.result(ret_ws=True)                                                     # needs keep_rows
    with pytest.raises(E.EngineError):
        ds2 = D.DenseSearch(w)
        ds2.add(["a"], torch.zeros(1, 2, 2, 16, dtype=torch.float16))                # a CPU tensor is not a device chunk


def test_refusals_of_the_c_entries():
    """Each refusal by its code, through the library's own entries with pointers that are never followed: nothing is launched."""
    lib = E.load_library()
    p, n = C.c_void_p(0x1000), None
    ok = dict(B=2, cells=63, Cc=72, K=5, off=0, ld=2)
    need = lib.dm_dense_search_workspace_bytes(2, 63, 5)
    assert need == 2 * 1 * 16 * 8 and lib.dm_dense_search_workspace_bytes(1, 3249, 64) == 51 * 64 * 8
    for bad in ((0, 63, 5), (2, 0, 5), (2, 1 << 24, 5), (2, 63, 0), (2, 63, 129)):
        assert lib.dm_dense_search_workspace_bytes(*bad) == 0, bad
    assert lib.dm_dense_search_workspace_bytes(1, (1 << 24) - 1, 128) > 0

    def winners(data=p, w=p, mask=n, work=p, work_bytes=need, score=p, cell=p, **kw):
        a = dict(ok, **kw)
        return lib.dm_dense_search_winners(None, data, w, mask, a["B"], a["cells"], a["Cc"], a["K"], a["off"], a["ld"], work, work_bytes,
                                           score, cell)
    for name in ("data", "w", "work", "score", "cell"):
        assert winners(**{name: n}) == 1, name
    assert winners(B=0) == 2 and winners(cells=0) == 3 and winners(cells=1 << 24) == 4
    assert winners(K=0) == 5 and winners(K=129) == 5
    assert winners(Cc=0) == 7 and winners(Cc=4) == 7 and winners(Cc=76) == 7
    assert winners(ld=1) == 8 and winners(off=1) == 8 and winners(off=-1) == 8
    assert winners(work_bytes=need - 1) == 9 and winners(K=17) == 9                  # 17 detectors need two column tiles
    assert winners(data=C.c_void_p(0x1008)) == 10 and winners(work=C.c_void_p(0x1004)) == 10

    def topk(score=p, cell=p, ts=p, ti=p, tc=p, count=p, K=5, n_images=7, ld=7, top_k=5):
        return lib.dm_dense_search_topk(None, score, cell, K, n_images, ld, top_k, 0, ts, ti, tc, count)
    for name in ("score", "cell", "ts", "ti", "tc", "count"):
        assert topk(**{name: n}) == 1, name
    assert topk(n_images=0) == 2 and topk(K=0) == 5 and topk(K=129) == 5
    assert topk(top_k=0) == 6 and topk(top_k=129) == 6 and topk(ld=6) == 8

    def gather(data=p, pairs=p, out=p, B=2, cells=63, Cc=72, n_rows=3):
        return lib.dm_dense_search_gather(None, data, B, cells, Cc, pairs, n_rows, out)
    for name in ("data", "pairs", "out"):
        assert gather(**{name: n}) == 1, name
    assert gather(B=0) == 2 and gather(n_rows=0) == 2 and gather(cells=0) == 3 and gather(cells=1 << 24) == 4
    assert gather(Cc=12) == 7 and gather(out=C.c_void_p(0x1002)) == 10
    assert D.ERRORS.keys() == set(range(1, 12))
