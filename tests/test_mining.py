"""Patch mining (Cluster.df_D -> sort + get_non_overlapping -> get_top_k), CPU tier: the numpy restatement of the selection that
the GPU tests compare the kernel with is itself pinned to the reference's pandas code (tests/golden/mining_ref.npz, written by
tests/make_golden_mining.py), and the host side of the new entry points is checked without a device."""
import os
import re

import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd.typicality import TypicalityScorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SORTED_CASES = ("a_desc", "a_asc", "b_desc", "b_asc", "short_desc", "short_asc")
MIN_LEAD = 1e-5


def greedy_numpy(dm, kx, ky, k_per_image, ascending=False, priority=None):
    """The selection contract in numpy: k_per_image rounds of "first row-major index of the best key among the candidates alive;
    report dm there; kill every candidate with |i - i*| <= kx and |j - j*| <= ky".  NaN keys are never alive.  Comparisons are
    numpy's (so -0 == +0).  Returns (boxes [c, 4] int32, D [c] fp32)."""
    dm = np.asarray(dm, dtype=np.float32)
    key = np.asarray(dm if priority is None else priority, dtype=np.float32)
    assert key.shape == dm.shape
    OW = dm.shape[1]
    alive = ~np.isnan(key)
    key = np.where(alive, -key if ascending else key, 0.0)
    boxes, D = [], []
    for _ in range(k_per_image):
        if not alive.any():
            break
        best = key[alive].max()
        i, j = divmod(int(np.flatnonzero(((key == best) & alive).ravel())[0]), OW)
        boxes.append((i, j, i + kx, j + ky))
        D.append(dm[i, j])
        alive[max(0, i - kx):i + kx + 1, max(0, j - ky):j + ky + 1] = False
    return np.array(boxes, dtype=np.int32).reshape(-1, 4), np.array(D, dtype=np.float32)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "mining_ref.npz"))


@pytest.mark.parametrize("tag", SORTED_CASES)
def test_numpy_restatement_equals_the_reference_boxes(fx, tag):
    kx, ky, k, asc = (int(v) for v in fx[f"{tag}_args"])
    boxes, D = greedy_numpy(fx[f"{tag}_map"], kx, ky, k, bool(asc))
    assert np.array_equal(boxes, fx[f"{tag}_boxes"]) and boxes.dtype == fx[f"{tag}_boxes"].dtype
    assert np.array_equal(D.view(np.uint32), fx[f"{tag}_D"].view(np.uint32))
    if tag.startswith("short"):
        assert 2 <= len(boxes) <= 3 < k                     # the map ran out


def test_numpy_restatement_equals_the_reference_on_the_shuffled_frame(fx):
    kx, ky, k, _ = (int(v) for v in fx["perm_args"])
    dm, perm = fx["perm_map"], fx["perm_perm"]
    prio = TypicalityScorer.permutation_priority(perm).reshape(dm.shape)
    assert np.array_equal(np.argsort(-prio.ravel(), kind="stable"), perm)       # a descending pass visits the frame's rows in order
    boxes, D = greedy_numpy(dm, kx, ky, k, False, priority=prio)
    assert np.array_equal(boxes, fx["perm_boxes"])
    assert np.array_equal(D.view(np.uint32), fx["perm_D"].view(np.uint32))


def test_restatement_tie_and_nan_rules():
    dm = np.zeros((7, 9), dtype=np.float32)
    b, _ = greedy_numpy(dm, 2, 2, 4)
    assert b[:, :2].tolist() == [[0, 0], [0, 3], [0, 6], [3, 0]]                 # lowest row-major index first
    dm[:] = np.nan
    dm[5, 5] = -3.0
    b, d = greedy_numpy(dm, 2, 2, 4)
    assert b.tolist() == [[5, 5, 7, 7]] and d.tolist() == [-3.0]
    z = np.array([[0.0, -0.0, 0.0]], dtype=np.float32)
    assert greedy_numpy(z, 1, 1, 1, True)[0][0, 1] == 0                         # the two zeros tie


def test_top_k_equals_the_reference(fx):
    rows = {"D": fx["topk_in_D"], "x_start": fx["topk_in_boxes"][:, 0], "y_start": fx["topk_in_boxes"][:, 1],
            "x_end": fx["topk_in_boxes"][:, 2], "y_end": fx["topk_in_boxes"][:, 3]}
    top = TypicalityScorer.top_k(rows, int(fx["topk_k"]))
    assert np.array_equal(top["D"].view(np.uint32), fx["topk_out_D"].view(np.uint32))
    got = np.stack([top["x_start"], top["y_start"], top["x_end"], top["y_end"]], axis=1)
    assert np.array_equal(got, fx["topk_out_boxes"])
    assert len(TypicalityScorer.top_k(rows, 10 ** 6)["D"]) == len(rows["D"])   # k = min(len(df), k)
    # stable among equal D
    t = TypicalityScorer.top_k({"D": np.array([1.0, 2.0, 1.0, 2.0], np.float32), "n": np.arange(4)}, 3)
    assert t["n"].tolist() == [1, 3, 0]


def test_recorded_leads_exclude_ties(fx):
    for tag in SORTED_CASES:
        ld = fx[f"{tag}_leads"]
        assert len(ld) == len(fx[f"{tag}_boxes"]) and (ld >= MIN_LEAD).all(), (tag, ld)
    d = np.sort(fx["topk_in_D"].astype(np.float64))
    assert np.diff(d).min() / np.abs(d).max() >= MIN_LEAD


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    lib = E.load_library()
    for s in ("dm_typicality_image_batched", "dm_mine_patches"):
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert s in E.SYMBOLS and hasattr(lib, s)
    m = re.search(r"#define\s+DM_MINE_MAX_K\s+(\d+)", hdr)
    assert m and int(m.group(1)) == E.MINE_MAX_K == 64
    assert E.MINE_DESC_DTYPE.itemsize == 48                 # three int64 offsets + six int32 sizes, no padding
    assert re.search(r"typedef struct dm_mine_desc \{[^}]*grid_offset[^}]*work_offset[^}]*map_offset[^}]*n_draws, n_cond[^}]*h, w[^}]*H, W",
                     hdr, re.S)


def test_mining_fails_loudly_without_an_engine():
    """Like its neighbours the shim has no host path: no GPU, no engine, no `mine_patches`; the C entry points refuse a null
    handle instead of touching a device."""
    lib = E.load_library()
    assert lib.dm_mine_patches(None, None, None, None, 1, 4, 4, 5, 0, None, None, None, None) != 0
    assert lib.dm_typicality_image_batched(None, None, 1, None, 1, 4, 4, None, None, None) != 0
    if not torch.cuda.is_available():
        with pytest.raises(E.EngineError):
            E.UNetEngine(0).mine_patches([torch.zeros(4, 4)], 2, 2)
        with pytest.raises(E.EngineError):
            E.UNetEngine(0).typicality_image_batched([torch.zeros(1, 2, 4, 2, 2)], [(8, 8)], 2, 2)
    assert callable(E.UNetEngine.mine_patches) and callable(E.UNetEngine.typicality_image_batched)
    assert callable(TypicalityScorer.mine_patches)
