"""The detector initialisation on the GPU (csrc/dense_search_wide.hip through diff-mining_amd/doersch.py).

  wide search   bit-equal to the narrow kernel (`doersch.winners`) over blocks of 128 detectors: the narrow kernel is the reference, so
                there is no tolerance.  Shapes: 63-cell images (a ragged 64-cell wave tile inside a 256-cell tile), 299 cells (two cell
                tiles), C = 72 (one block of 64 plus one 8-channel chunk), 136 and 2112, K = 1, 130, 200, 260, 300 (ragged over 16,
                128 and 256), masks, a NaN row and an all-NaN image.
  wide top-k    against `topk_host`, the box formula with mixed image heights, and the d20 count over the first min(20, count) entries.
  ranking       kernel == host restatement == the reference's run (tests/golden/detector_init_ref.json) on every case.
  guards        all three entries inside tests/gpu_util.Guarded under fills 0xFF and 0x00.
  refusals      every error code comes back with the outputs untouched.
  composition   image files -> features -> candidates' rows -> wide search -> ranking on the device against device_id="cpu"."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import detector_init_cases as IC  # noqa: E402
from tests.gpu_util import Guarded, dev  # noqa: E402

_wide, _rank = {}, {}


def wide_tables(tag, fresh=False):
    """(w, chunks, score [K, n] and cell [K, n] on the device) of the wide entry over the case's chunks; computed once per case"""
    if fresh or tag not in _wide:
        w, chunks = IC.wide_inputs(tag)
        K, n = len(w), sum(len(c[0]) for c in chunks)
        score = torch.full((K, n), 7.0, dtype=torch.float32, device=dev())
        cell = torch.full((K, n), -7, dtype=torch.int32, device=dev())
        wd, at = torch.from_numpy(w).to(dev()), 0
        for paths, data, mask in chunks:
            B = len(paths)
            dd = torch.from_numpy(data).to(dev()).view(B, -1, data.shape[-1])
            D.wide_winners(dd, wd, score, cell, at, None if mask is None else torch.from_numpy(mask).to(dev()))
            at += B
        torch.cuda.synchronize()
        if fresh:
            return w, chunks, score, cell
        _wide[tag] = (w, chunks, score, cell)
    return _wide[tag]


def narrow_tables(tag):
    w, chunks = IC.wide_inputs(tag)
    K, n = len(w), sum(len(c[0]) for c in chunks)
    score = torch.full((K, n), 7.0, dtype=torch.float32, device=dev())
    cell = torch.full((K, n), -7, dtype=torch.int32, device=dev())
    at = 0
    for paths, data, mask in chunks:
        B = len(paths)
        dd = torch.from_numpy(data).to(dev()).view(B, -1, data.shape[-1])
        md = None if mask is None else torch.from_numpy(mask).to(dev())
        for k0 in range(0, K, D.DENSE_MAX_DETECTORS):
            k1 = min(K, k0 + D.DENSE_MAX_DETECTORS)
            s, c = torch.empty((k1 - k0, B), dtype=torch.float32, device=dev()), torch.empty((k1 - k0, B), dtype=torch.int32, device=dev())
            D.winners(dd, torch.from_numpy(w[k0:k1]).to(dev()), s, c, 0, md)
            score[k0:k1, at:at + B], cell[k0:k1, at:at + B] = s, c
        at += B
    torch.cuda.synchronize()
    return score, cell


@pytest.mark.parametrize("tag", list(IC.WIDE))
def test_wide_equals_narrow_bit_for_bit(tag):
    _, _, score, cell = wide_tables(tag)
    want_score, want_cell = narrow_tables(tag)
    assert score.cpu().numpy().tobytes() == want_score.cpu().numpy().tobytes(), tag
    assert cell.cpu().numpy().tobytes() == want_cell.cpu().numpy().tobytes(), tag
    s = score.cpu().numpy()
    if IC.WIDE[tag]["nan"]:
        assert (s[:, IC.NAN_IMAGE] == -np.inf).all() and (cell.cpu().numpy()[:, IC.NAN_IMAGE] == -1).all()
        assert np.isfinite(np.delete(s, IC.NAN_IMAGE, axis=1)).all()
    else:
        assert np.isfinite(s).all() and (cell >= 0).all()
    if IC.WIDE[tag]["fold"] is not None:
        assert (s == 0).any() and (s > 0).any()                                      # masked zeros win somewhere, real scores elsewhere


def test_two_wide_runs_are_bit_equal():
    a, b = wide_tables("W1"), wide_tables("W1", fresh=True)
    assert a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes() and a[3].cpu().numpy().tobytes() == b[3].cpu().numpy().tobytes()


def test_wide_winners_writes_its_own_columns_only():
    w, chunks = IC.wide_inputs("W1")
    paths, data, mask = chunks[1]
    dd = torch.from_numpy(data).to(dev()).view(4, 63, 72)
    score = torch.full((300, 9), 7.0, dtype=torch.float32, device=dev())
    cell = torch.full((300, 9), -7, dtype=torch.int32, device=dev())
    D.wide_winners(dd, torch.from_numpy(w).to(dev()), score, cell, 3, torch.from_numpy(mask).to(dev()))
    torch.cuda.synchronize()
    _, _, all_score, all_cell = wide_tables("W1")
    assert torch.equal(score[:, 3:7], all_score[:, 3:7]) and torch.equal(cell[:, 3:7], all_cell[:, 3:7])
    keep = [0, 1, 2, 7, 8]
    assert (score[:, keep] == 7.0).all() and (cell[:, keep] == -7).all()


def expected_topk(score, cell, top_k, only_pos, image_h, positive):
    top_score, top_image, top_cell, count = D.topk_host(score, cell, top_k, only_pos)
    h = image_h[np.maximum(top_image, 0)]
    x = np.where(top_image >= 0, (top_cell // h) * 8, -1).astype(np.int32)
    y = np.where(top_image >= 0, (top_cell % h) * 8, -1).astype(np.int32)
    lists = [[(None, None, int(i)) for i in top_image[k, :count[k]]] for k in range(len(count))]
    d20 = np.array(D.discriminative_20(lists, set(np.flatnonzero(positive).tolist())), dtype=np.int32)
    return top_score, top_image, x, y, count, d20


def assert_topk(got, want):
    for name, g, w in zip(("score", "image", "x", "y", "count", "d20"), got, want):
        assert g.cpu().numpy().tobytes() == w.tobytes(), name


@pytest.mark.parametrize("top_k,only_pos", ((5, True), (5, False), (50, False)))
def test_wide_topk_boxes_and_d20(top_k, only_pos):
    _, _, score, cell = wide_tables("W1")
    n = score.shape[1]
    image_h = np.array([7, 9, 7, 5, 9, 7, 63], dtype=np.int32)                     # images of one search may differ in size
    positive = np.array([1, 0, 0, 1, 1, 0, 1], dtype=np.uint8)
    want = expected_topk(score.cpu().numpy(), cell.cpu().numpy(), top_k, only_pos, image_h, positive)
    if only_pos:
        assert (want[4] < top_k).any() and (want[4] == top_k).any()                  # top_k above some detectors' admissible images
    else:
        assert (want[4] == min(top_k, n)).all()
    got = D.wide_topk(score, cell, n, top_k, torch.from_numpy(image_h).to(dev()), torch.from_numpy(positive).to(dev()), only_pos)
    torch.cuda.synchronize()
    assert_topk(got, want)
    assert np.isnan(got[0].cpu().numpy()[:, min(top_k, n):]).all() and (got[1].cpu().numpy()[:, min(top_k, n):] == -1).all()
    assert (got[5].cpu().numpy() > 0).any()


def test_wide_topk_counts_positives_among_the_first_twenty_only():
    """a table of 300 detectors over 45 images with ties, -inf and NaN columns; top_k 30: d20 stops at entry 20"""
    rng = np.random.default_rng(31)
    K, n, ld = 300, 45, 48
    score = np.full((K, ld), 7.0, dtype=np.float32)
    score[:, :n] = (rng.integers(-3, 12, size=(K, n)) / 4).astype(np.float32)       # many equal scores: image order decides
    score[:, 5], score[rng.integers(0, K, 40), rng.integers(0, n, 40)] = -np.inf, np.nan
    score[7, :n] = -np.inf                                                           # a detector without an entry
    cell = rng.integers(0, 63, size=(K, ld)).astype(np.int32)
    image_h = rng.integers(1, 12, size=n).astype(np.int32)
    positive = (rng.random(n) < 0.5).astype(np.uint8)
    want = expected_topk(score[:, :n], cell[:, :n], 30, False, image_h, positive)
    later = [sum(int(positive[i]) for i in want[1][k, 20:want[4][k]]) for k in range(K)]
    assert max(later) > 0 and want[4][7] == 0 and want[5][7] == 0
    got = D.wide_topk(torch.from_numpy(score).to(dev()), torch.from_numpy(cell).to(dev()), n, 30, torch.from_numpy(image_h).to(dev()),
                      torch.from_numpy(positive).to(dev()))
    torch.cuda.synchronize()
    assert_topk(got, want)
    none = D.wide_topk(torch.from_numpy(score).to(dev()), torch.from_numpy(cell).to(dev()), n, 30, torch.from_numpy(image_h).to(dev()))
    assert none[5] is None and none[1].cpu().numpy().tobytes() == want[1].tobytes()


# ---- the ranking -------------------------------------------------------------------------------------------------------------
def device_rank(tag, max_pairs=IC.MAX_PAIRS, box=IC.BOX):
    arrays = IC.ranking(tag)
    nd = IC.RANKING[tag]["num_detectors"]
    accepted, n = D.detector_rank(arrays["key"], arrays["nb_image"], arrays["nb_x"], arrays["nb_y"], arrays["nb_count"], nd, box, max_pairs,
                                  device=dev())
    torch.cuda.synchronize()
    return arrays, accepted.cpu().numpy(), int(n.cpu()[0])


@pytest.mark.parametrize("tag", list(IC.RANKING))
def test_ranking_kernel_equals_host_equals_reference(tag):
    arrays, accepted, n = device_rank(tag)
    nd = IC.RANKING[tag]["num_detectors"]
    host = [k for k, _, _ in D.rank_init_detectors_host(nd, IC.stats_of(arrays), IC.patches_of(arrays))]
    want = IC.golden()["ranking"][tag]["accepted"]
    assert host == want
    assert accepted.dtype == np.int32 and accepted.shape == (nd,)
    assert accepted[:n].tolist() == want and n == len(want)
    assert (accepted[n:] == -1).all()
    if tag == "E3":                                                                  # all keys equal: index order
        assert want == sorted(want) and want[0] == 0


@pytest.mark.parametrize("tag,max_pairs,box", (("E1", 0, 64), ("R1", 0, 64), ("R3", 2, 64), ("R2", 5, 40), ("R1", 5, 2048)))
def test_ranking_kernel_equals_host_at_other_bounds(tag, max_pairs, box):
    """L = 1 rejects only with max_pairs 0; other bounds and boxes move the decisions"""
    arrays, accepted, n = device_rank(tag, max_pairs, box)
    nd = IC.RANKING[tag]["num_detectors"]
    host = [k for k, _, _ in D.rank_init_detectors_host(nd, IC.stats_of(arrays), IC.patches_of(arrays), box, max_pairs)]
    assert accepted[:n].tolist() == host and (accepted[n:] == -1).all()
    if (tag, max_pairs) == ("E1", 0):
        assert host != IC.golden()["ranking"]["E1"]["accepted"]                      # the bound of 0 does reject with one-entry lists


def test_rank_init_detectors_runs_on_device_arrays():
    arrays = IC.ranking("R1")
    stats = IC.stats_of(arrays)
    patches = IC.patches_of(arrays)
    stats["arrays"] = {k: torch.from_numpy(v).to(dev()) for k, v in arrays.items()}
    got = D.rank_init_detectors(12, stats, patches)
    assert got == D.rank_init_detectors_host(12, stats, patches)
    twice = dict(arrays)
    twice["nb_image"] = arrays["nb_image"].copy()
    twice["nb_image"][3, 1] = twice["nb_image"][3, 0]
    with pytest.raises(ValueError):                                                  # the contract, checked where the lists come from the host
        D.detector_rank(twice["key"], twice["nb_image"], twice["nb_x"], twice["nb_y"], twice["nb_count"], 12, device=dev())


# ---- guards ------------------------------------------------------------------------------------------------------------------
PAD = 3


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ff", "00"))
def test_guarded_search_equals_the_plain_run(fill):
    w, chunks, score, cell = wide_tables("W1")
    K, n, C_, cells, top_k = 300, 7, 72, 63, 5
    image_h = np.array([7, 9, 7, 5, 9, 7, 63], dtype=np.int32)
    positive = np.array([1, 0, 0, 1, 1, 0, 1], dtype=np.uint8)
    ins = {"w": torch.from_numpy(w), "image_h": torch.from_numpy(image_h), "positive": torch.from_numpy(positive)}
    for j, (_, data, mask) in enumerate(chunks):
        ins[f"data{j}"], ins[f"mask{j}"] = torch.from_numpy(data).view(len(data), cells, C_), torch.from_numpy(mask)
    need = max(D.wide_workspace_bytes(len(c[0]), cells, K) for c in chunks)
    outs = {"work": ((need,), torch.uint8), "score": ((K, n + PAD), torch.float32), "cell": ((K, n + PAD), torch.int32),
            "top_score": ((K, top_k), torch.float32), "top_image": ((K, top_k), torch.int32), "top_x": ((K, top_k), torch.int32),
            "top_y": ((K, top_k), torch.int32), "count": ((K,), torch.int32), "d20": ((K,), torch.int32)}
    g = Guarded(ins, outs, fill=fill, device=dev())
    v = g.views()
    lib, stream, ptr = D._lib(), D._stream(torch, dev()), D._p
    at = 0
    for j, (paths, _, _) in enumerate(chunks):
        assert lib.dm_dense_wide_winners(stream, ptr(v[f"data{j}"]), ptr(v["w"]), ptr(v[f"mask{j}"]), len(paths), cells, C_, K, at, n + PAD,
                                         ptr(v["work"]), need, ptr(v["score"]), ptr(v["cell"])) == 0
        at += len(paths)
    assert lib.dm_dense_wide_topk(stream, ptr(v["score"]), ptr(v["cell"]), K, n, n + PAD, top_k, 1, ptr(v["positive"]), ptr(v["image_h"]),
                                  ptr(v["top_score"]), ptr(v["top_image"]), ptr(v["top_x"]), ptr(v["top_y"]), ptr(v["count"]),
                                  ptr(v["d20"])) == 0
    torch.cuda.synchronize()
    g.check()
    assert v["score"][:, :n].cpu().numpy().tobytes() == score.cpu().numpy().tobytes()
    assert v["cell"][:, :n].cpu().numpy().tobytes() == cell.cpu().numpy().tobytes()
    for name in ("score", "cell"):                                                   # the columns past the last image keep the fill
        assert (v[name][:, n:].contiguous().view(torch.uint8) == fill).all(), name
    plain = D.wide_topk(score, cell, n, top_k, torch.from_numpy(image_h).to(dev()), torch.from_numpy(positive).to(dev()), True)
    for name, want in zip(("top_score", "top_image", "top_x", "top_y", "count", "d20"), plain):
        assert v[name].cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), name


@pytest.mark.parametrize("fill", (0xFF, 0x00), ids=("ff", "00"))
@pytest.mark.parametrize("tag", ("R2", "R3"))
def test_guarded_ranking_equals_the_plain_run(tag, fill):
    arrays, accepted, n = device_rank(tag)
    s = IC.RANKING[tag]
    need = D.detector_rank_workspace_bytes(s["N"], s["L"], s["num_detectors"])
    g = Guarded({k: torch.from_numpy(a) for k, a in arrays.items()},
                {"work": ((need,), torch.uint8), "accepted": ((s["num_detectors"],), torch.int32), "n": ((1,), torch.int32)},
                fill=fill, device=dev())
    v = g.views()
    ptr = D._p
    assert D._lib().dm_detector_rank(D._stream(torch, dev()), ptr(v["key"]), ptr(v["nb_image"]), ptr(v["nb_x"]), ptr(v["nb_y"]),
                                     ptr(v["nb_count"]), s["N"], s["L"], IC.BOX, IC.MAX_PAIRS, s["num_detectors"], ptr(v["work"]), need,
                                     ptr(v["accepted"]), ptr(v["n"])) == 0
    torch.cuda.synchronize()
    g.check()
    assert v["accepted"].cpu().numpy().tobytes() == accepted.tobytes() and int(v["n"].cpu()[0]) == n


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_codes_without_a_launch():
    lib, stream, ptr = D._lib(), D._stream(torch, dev()), D._p
    data = torch.zeros((1, 4, 8), dtype=torch.float16, device=dev())
    w = torch.zeros((2, 8), dtype=torch.float16, device=dev())
    score, cell = torch.full((2, 1), 7.0, dtype=torch.float32, device=dev()), torch.full((2, 1), -7, dtype=torch.int32, device=dev())
    need = D.wide_workspace_bytes(1, 4, 2)
    work = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=dev())

    def winners(data_p=ptr(data), w_p=ptr(w), B=1, cells=4, C_=8, K=2, off=0, ld=1, work_p=ptr(work), nbytes=need, score_p=ptr(score)):
        return lib.dm_dense_wide_winners(stream, data_p, w_p, None, B, cells, C_, K, off, ld, work_p, nbytes, score_p, ptr(cell))
    assert winners(K=32769) == 5 and winners(K=0) == 5                               # DM_DENSE_E_K
    assert winners(nbytes=need - 1) == 9                                             # DM_DENSE_E_WORK
    assert winners(data_p=C.c_void_p(data.data_ptr() + 2)) == 10                     # DM_DENSE_E_ALIGN
    assert winners(work_p=C.c_void_p(work.data_ptr() + 4)) == 10
    assert winners(data_p=None) == 1 and winners(score_p=None) == 1                  # DM_DENSE_E_NULL
    assert winners(B=0) == 2 and winners(cells=0) == 3 and winners(cells=1 << 24) == 4 and winners(C_=12) == 7 and winners(ld=0) == 8
    top = [torch.full((2, 3), -7, dtype=torch.int32, device=dev()) for _ in range(3)]
    top_score, count = torch.full((2, 3), 7.0, dtype=torch.float32, device=dev()), torch.full((2,), -7, dtype=torch.int32, device=dev())
    image_h = torch.ones(1, dtype=torch.int32, device=dev())

    def topk(K=2, n=1, ld=1, top_k=3, h_p=ptr(image_h), d20_p=None, pos_p=None):
        return lib.dm_dense_wide_topk(stream, ptr(score), ptr(cell), K, n, ld, top_k, 0, pos_p, h_p, ptr(top_score), ptr(top[0]), ptr(top[1]),
                                      ptr(top[2]), ptr(count), d20_p)
    assert topk(K=32769) == 5 and topk(top_k=129) == 6 and topk(n=0) == 2 and topk(ld=0) == 8 and topk(h_p=None) == 1
    assert topk(d20_p=ptr(count)) == 1                                               # d20 without the positive flags
    key = torch.zeros(4, dtype=torch.int32, device=dev())
    nb = torch.zeros((4, 2), dtype=torch.int32, device=dev())
    rneed = D.detector_rank_workspace_bytes(4, 2, 3)
    rwork = torch.full((rneed + 16,), 0x5A, dtype=torch.uint8, device=dev())
    accepted, n_acc = torch.full((3,), -7, dtype=torch.int32, device=dev()), torch.full((1,), -7, dtype=torch.int32, device=dev())

    def rank(key_p=ptr(key), N=4, L=2, box=64, max_pairs=5, nd=3, work_p=ptr(rwork), nbytes=rneed, acc_p=ptr(accepted)):
        return lib.dm_detector_rank(stream, key_p, ptr(nb), ptr(nb), ptr(nb), ptr(key), N, L, box, max_pairs, nd, work_p, nbytes, acc_p, ptr(n_acc))
    assert rank(N=0) == 2 and rank(N=32769) == 2 and rank(L=129) == 3 and rank(L=0) == 3 and rank(nd=0) == 4 and rank(nd=4097) == 4
    assert rank(box=0) == 5 and rank(box=2049) == 5 and rank(max_pairs=-1) == 6
    assert rank(nbytes=rneed - 1) == 7 and rank(work_p=C.c_void_p(rwork.data_ptr() + 1)) == 8
    assert rank(key_p=None) == 1 and rank(acc_p=None) == 1
    torch.cuda.synchronize()
    assert (score == 7.0).all() and (cell == -7).all() and (work == 0x5A).all() and (rwork == 0x5A).all()
    assert (top_score == 7.0).all() and all((t == -7).all() for t in top) and (count == -7).all()
    assert (accepted == -7).all() and (n_acc == -7).all()
    with pytest.raises(ValueError):
        D.wide_workspace_bytes(1, 4, 32769)
    with pytest.raises(ValueError):
        D.detector_rank_workspace_bytes(4, 129, 3)


# ---- composition -------------------------------------------------------------------------------------------------------------
def test_images_to_ranked_detectors_device_equals_host(tmp_path):
    """`init_detectors_images` + `rank_init_detectors` on the device against the same calls with device_id="cpu": indices, neighbours
    and d20.  The seed is the one at which every gap of the host run is at least 16 x the distance between features computed in fp32
    and in fp64 (tests/make_golden_detector_init.py).  max_pairs 1: with three neighbours per candidate the reference's bound of 5
    would reject nothing."""
    from PIL import Image
    seed = IC.golden()["compose"]["seed"]
    s = IC.COMPOSE
    names = []
    for j, im in enumerate(IC.compose_images(seed)):
        names.append(str(tmp_path / f"c{j}.png"))
        Image.fromarray(im).save(names[-1])
    patches = IC.compose_patches(seed, names)
    positives = [names[j] for j in s["positives"]]
    host = D.init_detectors_images(patches, names, positives, batch=s["batch"], top_k=s["top_k"], device_id="cpu")
    got = D.init_detectors_images(patches, names, positives, batch=s["batch"], top_k=s["top_k"], device_id="cuda")
    small = D.init_detectors_images(patches, names, positives, batch=s["batch"], top_k=s["top_k"], device_id="cuda", cache_bytes=0)
    assert isinstance(got["arrays"]["key"], torch.Tensor) and got["arrays"]["key"].is_cuda and isinstance(host["arrays"]["key"], np.ndarray)
    for other in (got, small):                                                       # kept features or a second pass: the same answer
        assert other["neighbors"] == host["neighbors"] and other["discriminative-20"] == host["discriminative-20"]
    for k, (bbox, path) in enumerate(patches):                                       # a candidate finds itself first
        assert host["neighbors"][k][0] == ((bbox[0], bbox[1]), path) and len(host["neighbors"][k]) == s["top_k"]
    assert len(set(host["discriminative-20"].values())) > 1
    want = D.rank_init_detectors(s["num_detectors"], host, patches, max_pairs=1)
    ranked = D.rank_init_detectors(s["num_detectors"], got, patches, max_pairs=1)
    assert [k for k, _, _ in ranked] == [k for k, _, _ in want] and [p for _, p, _ in ranked] == [p for _, p, _ in want]
    assert len(want) == s["num_detectors"] and [k for k, _, _ in want] != sorted(host["discriminative-20"], key=lambda k: -host["discriminative-20"][k])[:len(want)]
    for (_, _, a), (_, _, b) in zip(ranked, want):       # rows of unit norm from fp32 and from fp64 arithmetic: at most one fp16 unit below 1 apart
        assert a.dtype == b.dtype == np.float16 and np.abs(a.astype(np.float32) - b.astype(np.float32)).max() <= 2.0 ** -11
