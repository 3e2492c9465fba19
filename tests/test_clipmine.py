"""CPU tier of the CLIP baseline's mining (diff_mining_amd.clipmine): the float64 restatement against the reference's own
`dot_text_image` (tests/golden/clipmine_ref.npz, tests/make_golden_clipmine.py), the weight tables, the refusals, and
`rank_and_cluster` against the chain it wraps."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_mining_amd import clipmine as CM
from diff_mining_amd import clustering
from diff_mining_amd.typicality import TypicalityScorer
from tests import clipmine_cases as CC


@pytest.mark.parametrize("tag", CC.CASES)
def test_restatement_against_the_reference(tag):
    c = CC.case(tag)
    assert (c.leads >= 1e-5).all()                             # no tie decides a round (the generator's rule)
    rows, feats = CM.rank_patches_host([c.tokens], c.text, [c.size], **CC.kwargs(c))
    boxes = np.stack([rows[n] for n in ("x_start", "y_start", "x_end", "y_end")], axis=1)
    assert rows["D"].dtype == np.float32 and boxes.dtype == np.int32 and (rows["image"] == 0).all()
    CC.check_against_reference(c, boxes, rows["D"], feats, "host")


def test_fixture_has_the_run_out_and_all_eligible_cases():
    c = CC.case("run_out")
    assert len(c.boxes) < c.k
    c = CC.case("all_eligible")
    assert (c.size[0] - c.kx + 1) * (c.size[1] - c.ky + 1) == 81 < 100 * c.k
    c = CC.case("real")
    assert (c.gh, c.pw, c.size, c.kx, c.ky, c.k) == (24, 24, (512, 512), 64, 64, 5)


def test_rows_of_several_images_come_in_image_then_round_order():
    cs = [CC.case(t) for t in ("g33_small", "run_out", "all_eligible")]                  # one window, one k
    rows, feats, maps = CM.rank_patches_host([c.tokens for c in cs], cs[0].text, [c.size for c in cs], pw=3, k_per_image=2, kx=8,
                                             ky=8, return_maps=True)
    assert [m.shape for m in maps] == [(17, 17), (41, 41), (9, 9)] and feats.shape == (len(rows["D"]), 32)
    assert np.array_equal(np.stack([rows["x_start"], rows["y_start"]], 1)[:2], cs[0].boxes[:, :2])
    at = 0
    for b, c in enumerate(cs):                                 # image b's rows are what image b gives alone, in place
        one, f1 = CM.rank_patches_host([c.tokens], cs[0].text, [c.size], pw=3, k_per_image=2, kx=8, ky=8)
        m = len(one["D"])
        assert 1 <= m <= 2 and (rows["image"][at:at + m] == b).all() and np.array_equal(feats[at:at + m], f1)
        assert all(np.array_equal(rows[k][at:at + m], one[k]) for k in ("x_start", "y_start", "x_end", "y_end", "D"))
        at += m
    assert at == len(rows["D"])
    # numpy input through the public entry takes the restatement
    rows2, feats2 = CM.rank_patches([torch.from_numpy(c.tokens) for c in cs], torch.from_numpy(cs[0].text), [c.size for c in cs], pw=3,
                                    k_per_image=2, kx=8, ky=8)
    assert all(np.array_equal(rows[k], rows2[k]) for k in rows) and np.array_equal(feats, feats2)


@pytest.mark.parametrize("out,n_in,window", [(40, 4, 8), (52, 5, 8), (37, 5, 8), (45, 4, 6), (16, 3, 8), (512, 24, 64), (7, 9, 1), (5, 1, 5)])
def test_axis_weights_are_the_mean_of_bilinear_rows(out, n_in, window):
    A = CM.axis_weights(out, n_in, window)
    assert A.dtype == np.float64 and A.shape == (out - window + 1, n_in)
    assert np.abs(A.sum(axis=1) - 1.0).max() < 1e-14
    # brute force: torch's own align_corners=False interpolation of the unit vectors, in float64, then the window mean
    up = torch.nn.functional.interpolate(torch.eye(n_in, dtype=torch.float64)[None], size=out, mode="linear", align_corners=False)[0].numpy().T
    brute = np.stack([up[i:i + window].mean(axis=0) for i in range(out - window + 1)])
    assert np.abs(A - brute).max() < 1e-14
    if n_in >= 3 and out >= 4 * n_in:                          # a banded table: a window touches few tokens
        assert (np.count_nonzero(A, axis=1) < n_in).any()


def test_refusals_raise():
    c = CC.case("g45_diff")
    ok = dict(CC.kwargs(c))

    def call(tokens=c.tokens, text=c.text, size=c.size, **kw):
        return CM.rank_patches_host([tokens], text, [size], **dict(ok, **kw))

    call()
    with pytest.raises(ValueError):
        call(size=(7, 52))                                     # a window larger than the image
    with pytest.raises(ValueError):
        call(size=(40, 7))
    with pytest.raises(ValueError):
        call(pw=3)                                             # 20 tokens are not rows of 3
    for k in (0, CM.MINE_MAX_K + 1):
        with pytest.raises(ValueError):
            call(k_per_image=k)
    with pytest.raises(ValueError):
        call(tokens=c.tokens[:, :0], text=c.text[:, :0])       # E < 1
    with pytest.raises(ValueError):
        call(mode="max")
    with pytest.raises(ValueError):
        call(kx=1)                                             # `pool` skips a window with one side 1
    with pytest.raises(ValueError):
        call(text=c.text[:, :40])
    with pytest.raises(ValueError):
        CM.rank_patches_host([c.tokens, c.tokens], c.text, [c.size], **ok)
    with pytest.raises(ValueError):
        CM.axis_weights(8, 3, 9)


def test_the_c_entry_refuses_bad_arguments_before_any_launch():
    """The checks dm_clipmine_rank makes before it touches the device (the pointers are never followed)."""
    lib = CM._lib()
    p = C.c_void_p(256)

    def rc(E=8, n=1, kx=8, ky=8, k=2, mode=0, tokens=p):
        return lib.dm_clipmine_rank(None, tokens, p, E, p, n, p, kx, ky, k, mode, p, 1 << 20, None, p, p, p, p)

    assert rc(tokens=None) == 1 and rc(n=0) == 2 and rc(E=0) == 3
    assert rc(k=0) == 4 and rc(k=CM.MINE_MAX_K + 1) == 4 and rc(mode=2) == 5
    assert rc(kx=0) == 6 and rc(kx=1) == 6 and rc(ky=1) == 6
    assert set(CM.ERRORS) == set(range(1, 11))
    assert lib.dm_clipmine_workspace_bytes(0, 10, 10) == 0 and lib.dm_clipmine_workspace_bytes(2, 1, 10) == 0
    assert lib.dm_clipmine_workspace_bytes(2, 18, 100) == (2 * 18 + 100 + 128) * 4
    assert CM.CLIPMINE_DESC_DTYPE.itemsize == 64


def test_rank_and_cluster_is_top_k_then_cluster_patches():
    rng = np.random.default_rng(5)
    n, E = 60, 16
    centres = rng.standard_normal((4, E))
    feats = centres[rng.integers(0, 4, n)] + 0.1 * rng.standard_normal((n, E))
    feats = (feats / np.linalg.norm(feats, axis=1, keepdims=True)).astype(np.float32)
    rows = {"image": np.arange(n) // 3, "x_start": rng.integers(0, 9, n).astype(np.int32), "y_start": rng.integers(0, 9, n).astype(np.int32),
            "D": rng.standard_normal(n).astype(np.float32)}
    rows["x_end"], rows["y_end"] = rows["x_start"] + 8, rows["y_start"] + 8
    top, got = CM.rank_and_cluster(rows, feats, k=40, num_clusters=4)
    want_top = TypicalityScorer.top_k(dict(rows, index=np.arange(n)), 40)
    want = clustering.cluster_patches(feats[want_top["index"]], want_top["D"], 4, aggregate="median", order_by="centroid")
    assert len(top["D"]) == 40 and all(np.array_equal(top[k], want_top[k]) for k in want_top)
    assert (np.diff(top["D"].astype(np.float64)) <= 0).all()
    assert len(got["clusters"]) == len(want["clusters"]) == 4
    for a, b in zip(got["clusters"], want["clusters"]):
        assert a["cluster"] == b["cluster"] and np.array_equal(a["rows"], b["rows"]) and a["aggregate"] == b["aggregate"]
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["centers"], want["centers"])
    with pytest.raises(ValueError):
        CM.rank_and_cluster(rows, feats[:-1])
