"""Parallel-dataset mining (Cluster.df_PD: median map across sets -> sort + get_non_overlapping -> per-set columns), CPU tier: the
numpy restatement that the GPU tests compare the kernels with is itself pinned to the reference's pandas code and to np.median
(tests/golden/parallel_ref.npz, written by tests/make_golden_parallel.py); `parallel_groups` is pinned to the reference's
`load_paths`; the host mirror's columns are checked on a stubbed engine."""
import os
import re

import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from diff_mining_amd import typicality as T
from diff_mining_amd.typicality import TypicalityScorer
from tests.test_mining import greedy_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SORTED_CASES = ("p10_desc", "p10_asc", "short_desc", "p3_desc", "p4_desc")
MIN_LEAD = 1e-5


def case_maps(fx, tag):
    """the cases on the 10-set maps share one stored copy"""
    t = tag if f"{tag}_maps" in fx.files else "p10_desc"
    return fx[f"{t}_maps"], fx[f"{t}_median"]


def median_by_sort(stack):
    """The kernel's rule in numpy: sort the C values of a candidate, take the middle one, or for an even C
    (s[C/2-1] + s[C/2]) * 0.5 in fp32; NaN where any of the C is NaN."""
    stack = np.asarray(stack, dtype=np.float32)
    C = stack.shape[0]
    nan = np.isnan(stack).any(axis=0)
    s = np.sort(np.where(nan[None], np.float32(0), stack), axis=0)
    m = s[C // 2] if C & 1 else (s[C // 2 - 1] + s[C // 2]) * np.float32(0.5)
    return np.where(nan, np.float32(np.nan), m).astype(np.float32)


def parallel_numpy(stack, kx, ky, k_per_image, ascending=False, priority=None):
    """df_PD.compute in numpy: median by sort, then tests.test_mining.greedy_numpy (greedy with the inclusive zone, lowest
    row-major index on ties, NaN never chosen), then every set's own value at the winners.
    Returns (boxes [c, 4] int32, D [c] fp32, set_D [c, C] fp32, median [OH, OW] fp32)."""
    stack = np.asarray(stack, dtype=np.float32)
    med = median_by_sort(stack)
    boxes, D = greedy_numpy(med, kx, ky, k_per_image, ascending, priority)
    set_D = np.array([stack[:, b[0], b[1]] for b in boxes], dtype=np.float32).reshape(-1, stack.shape[0])
    return boxes, D, set_D, med


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "parallel_ref.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("tag", SORTED_CASES + ("perm",))
def test_numpy_restatement_equals_the_reference(fx, tag):
    kx, ky, k, asc = (int(v) for v in fx[f"{tag}_args"])
    stack, ref_med = case_maps(fx, tag)
    prio = None
    if tag == "perm":
        prio = TypicalityScorer.permutation_priority(fx["perm_perm"]).reshape(stack.shape[1:])
    boxes, D, set_D, med = parallel_numpy(stack, kx, ky, k, bool(asc), prio)
    assert med.dtype == ref_med.dtype == np.float32 and np.array_equal(med, ref_med)          # the stored np.median
    assert np.array_equal(boxes, fx[f"{tag}_boxes"]) and boxes.dtype == fx[f"{tag}_boxes"].dtype
    assert np.array_equal(_bits(D), _bits(fx[f"{tag}_D"]))
    assert np.array_equal(_bits(set_D), _bits(fx[f"{tag}_set_D"]))
    if tag.startswith("short"):
        assert 2 <= len(boxes) <= 3 < k                     # the map ran out


def test_fixture_has_the_cases_and_no_ties(fx):
    assert fx["p10_desc_maps"].shape == (10, 29, 41) and fx["short_desc_maps"].shape == (10, 5, 12)
    assert fx["p3_desc_maps"].shape == (3, 23, 31) and fx["p4_desc_maps"].shape == (4, 23, 31)
    assert [int(v) for v in fx["p10_desc_args"]] == [8, 8, 5, 0] and [int(v) for v in fx["p10_asc_args"]] == [8, 8, 5, 1]
    assert [int(v) for v in fx["short_desc_args"]] == [4, 4, 5, 0] and [int(v) for v in fx["p4_desc_args"]] == [6, 6, 4, 0]
    assert sorted(fx["perm_perm"].tolist()) == list(range(29 * 41))
    for tag in SORTED_CASES:
        ld = fx[f"{tag}_leads"]
        assert len(ld) == len(fx[f"{tag}_boxes"]) and (ld >= MIN_LEAD).all(), (tag, ld)
    assert os.path.getsize(os.path.join(GOLDEN, "parallel_ref.npz")) < 200 * 1024


@pytest.mark.parametrize("C", [1, 2, 3, 4, 7, 10, 16])
def test_median_by_sort_is_np_median(C):
    rng = np.random.default_rng(C)
    stack = rng.standard_normal((C, 37, 53)).astype(np.float32)
    assert np.array_equal(_bits(median_by_sort(stack)), _bits(np.median(stack, axis=0)))
    ints = rng.integers(-2, 3, (C, 37, 53)).astype(np.float32)
    ints[rng.random(ints.shape) < 0.2] = -0.0
    got, ref = median_by_sort(ints), np.median(ints, axis=0)
    assert (got == ref).all() and not np.isnan(got).any()                 # equal; the sign of a tied zero is free
    stack[C // 2, 5, 6] = np.nan
    got, ref = median_by_sort(stack), np.median(stack, axis=0)
    assert np.isnan(got[5, 6]) and np.isnan(ref[5, 6]) and np.isnan(got).sum() == np.isnan(ref).sum() == 1


def test_parallel_groups_equal_the_reference(fx):
    by_dir = {}
    for d, n in zip(fx["files_dir"].tolist(), fx["files_name"].tolist()):
        by_dir.setdefault(d, []).append(n)
    got = T.parallel_groups(by_dir)
    want = {}
    for d, gi, p, c in zip(fx["groups_dir"].tolist(), fx["groups_index"].tolist(), fx["groups_path"].tolist(), fx["groups_country"].tolist()):
        groups = want.setdefault(d, [])
        if gi == len(groups):
            groups.append([])
        groups[gi].append((p, c))
    assert got == want
    assert sum(len(g) for g in want.values()) == 6 and ("United_Kingdom/Japan_x__7.jpg", "Japan") in got["United_Kingdom"][0]
    assert ("France/United_Kingdom__001.jpg", "United") in got["France"][0]          # the single-'_' split of compute.py:207
    assert T.parallel_groups({"A": reversed(["gt--A__1.jpg", "B__1.jpg"])}, "/data") == {"A": [[("/data/A/gt--A__1.jpg", "A"), ("/data/A/B__1.jpg", "B")]]}


class StubEngine:
    """maps = the grid's first plane as it is; mine_parallel = the numpy restatement"""
    device = torch.device("cpu")

    def __init__(self):
        self.map_calls, self.mine_calls = [], []

    def typicality_image_batched(self, grids, image_sizes, kx, ky):
        self.map_calls.append(len(grids))
        return [torch.as_tensor(g)[0, 0, 0, :H - kx + 1, :W - ky + 1].float() for g, (H, W) in zip(grids, image_sizes)]

    def mine_parallel(self, maps_by_group, kx, ky, k_per_image=5, ascending=False, priority=None):
        self.mine_calls.append(len(maps_by_group))
        G, C = len(maps_by_group), len(maps_by_group[0])
        boxes = np.full((G, k_per_image, 4), -1, np.int32)
        D = np.full((G, k_per_image), np.nan, np.float32)
        sD = np.full((G, k_per_image, C), np.nan, np.float32)
        cnt = np.zeros(G, np.int32)
        meds = []
        for g, ms in enumerate(maps_by_group):
            b, d, s, m = parallel_numpy(np.stack([x.numpy() for x in ms]), kx, ky, k_per_image, ascending,
                                        None if priority is None else priority[g].numpy())
            cnt[g] = len(b)
            boxes[g, :len(b)], D[g, :len(b)], sD[g, :len(b)] = b, d, s
            meds.append(torch.from_numpy(m))
        return torch.from_numpy(boxes), torch.from_numpy(D), torch.from_numpy(sD), torch.from_numpy(cnt), meds


def _stub_groups(fx):
    def grids(stack):
        return [torch.from_numpy(np.ascontiguousarray(m))[None, None, None].expand(1, 2, 4, *m.shape) for m in stack]
    a, s = fx["p3_desc_maps"], fx["short_desc_maps"][:3]
    return [grids(a), grids(s), grids(a[::-1])], [(23 + 5, 31 + 5), (5 + 5, 12 + 5), (23 + 5, 31 + 5)]


def test_host_mirror_columns_and_dtypes_on_a_stub(fx, tmp_path):
    names = ["France", "Japan", "Italy"]
    groups, sizes = _stub_groups(fx)
    eng = StubEngine()
    sc = TypicalityScorer(eng, typicality_path=str(tmp_path))
    path = "/data/Japan/Japan__001.jpg"
    sc.save_grid(os.path.join(str(tmp_path), "Japan"), path, groups[0][1])            # the set's own directory
    groups[0][1] = path
    rows = sc.mine_parallel_patches(groups, sizes, names, ["France", "Italy", "Japan"], k_per_image=4, kx=6, ky=6, groups_per_call=2)
    assert eng.map_calls == [6, 3] and eng.mine_calls == [2, 1]                       # groups_per_call x n_sets images per call
    assert list(rows) == ["x_start", "y_start", "x_end", "y_end", "origin", "D", "France", "Japan", "Italy",
                          "path_France", "path_Japan", "path_Italy", "group", "image"] == TypicalityScorer.parallel_columns(names)
    n = len(rows["D"])
    assert all(len(v) == n for v in rows.values())
    assert all(rows[c].dtype == np.int32 for c in ("x_start", "y_start", "x_end", "y_end"))
    assert all(rows[c].dtype == np.float32 for c in ("D", "France", "Japan", "Italy"))
    assert rows["group"].dtype == np.int64 and rows["origin"].dtype == object and rows["path_Japan"].dtype == object
    b0, d0, s0, _ = parallel_numpy(fx["p3_desc_maps"], 6, 6, 4)
    b1, d1, s1, _ = parallel_numpy(fx["short_desc_maps"][:3], 6, 6, 4)
    assert np.array_equal(b0, fx["p3_desc_boxes"]) and len(b1) < 4                    # group 0 is the fixture's case; group 1 runs out
    assert rows["group"].tolist() == [0] * 4 + [1] * len(b1) + [2] * 4
    assert rows["origin"].tolist() == ["France"] * 4 + ["Italy"] * len(b1) + ["Japan"] * 4
    per = TypicalityScorer.boxes_by_image(rows)                                       # as it is
    assert len(per) == 3 and np.array_equal(per[0], b0) and np.array_equal(per[1], b1) and np.array_equal(per[2], b0)
    assert np.array_equal(_bits(rows["D"][:4]), _bits(d0))
    for c, name in enumerate(names):
        assert np.array_equal(_bits(rows[name][:4]), _bits(s0[:, c]))
        assert np.array_equal(_bits(rows[name][-4:]), _bits(s0[:, 2 - c]))            # group 2 holds the sets in reverse
    assert rows["path_France"].tolist()[:4] == [0] * 4 and rows["path_Japan"].tolist()[:4] == [path] * 4
    assert rows["path_Italy"].tolist()[-4:] == [8] * 4                                # g * n_sets + c
    top = TypicalityScorer.top_k(rows, 3)                                             # as it is
    assert list(top) == list(rows) and len(top["D"]) == 3 and (np.diff(top["D"]) <= 0).all()
    assert top["D"][0] == rows["D"].max()
    # the random arm: a seeded permutation per group, D only reported
    rnd = sc.mine_parallel_patches(groups[2:], sizes[2:], names, ["Japan"], k_per_image=4, kx=6, ky=6, randomized=True, seed=7)
    perm = np.random.default_rng((7, 0)).permutation(23 * 31)
    rb, rd, _, _ = parallel_numpy(fx["p3_desc_maps"][::-1], 6, 6, 4, priority=TypicalityScorer.permutation_priority(perm).reshape(23, 31))
    assert np.array_equal(TypicalityScorer.boxes_by_image(rnd)[0], rb) and np.array_equal(_bits(rnd["D"]), _bits(rd))
    assert rb[0, 0] * 31 + rb[0, 1] == perm[0]


def test_host_refusals_that_need_no_gpu(fx):
    groups, sizes = _stub_groups(fx)
    sc = TypicalityScorer(StubEngine())
    with pytest.raises(ValueError, match="image sizes"):
        sc.mine_parallel_patches(groups, sizes[:2], ["a", "b", "c"], ["a"] * 3)
    with pytest.raises(ValueError, match="set name"):
        sc.mine_parallel_patches(groups, sizes, ["a", "b"], ["a"] * 3)
    with pytest.raises(ValueError, match="set name"):
        sc.mine_parallel_patches(groups, sizes, ["a", "b", "b"], ["a"] * 3)
    with pytest.raises(ValueError, match="one side 1"):
        sc.mine_parallel_patches(groups, sizes, ["a", "b", "c"], ["a"] * 3, kx=1, ky=4)


def test_place_maps_reads_views_of_one_buffer_in_place():
    buf = torch.arange(100, dtype=torch.float32)
    views = [buf[10:22].view(3, 4), buf[40:60].view(4, 5), buf[22:34].view(3, 4)]
    base, off, copied = E.UNetEngine._place_maps(torch, views, "cpu")
    assert not copied and off == [0, 30, 12] and base.data_ptr() == buf[10:].data_ptr() and base.numel() == 50
    assert all(torch.equal(base[o:o + v.numel()].view(v.shape), v) for o, v in zip(off, views))
    for other in ([buf[:12].view(3, 4), torch.zeros(3, 4)], [buf[:12].view(3, 4).double()], [buf[:24].view(4, 6)[:, :3]]):
        base, off, copied = E.UNetEngine._place_maps(torch, other, "cpu")
        assert copied and base.dtype == torch.float32 and off[0] == 0
        assert all(torch.equal(base[o:o + v.numel()].view(v.shape), v.float()) for o, v in zip(off, other))


def test_new_symbol_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    lib = E.load_library()
    assert re.search(r"\bint\s+dm_mine_parallel\s*\(", hdr)
    assert "dm_mine_parallel" in E.SYMBOLS and hasattr(lib, "dm_mine_parallel")
    m = re.search(r"#define\s+DM_MINE_MAX_SETS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == E.MINE_MAX_SETS == 16


def test_parallel_mining_fails_loudly_without_an_engine():
    lib = E.load_library()
    assert lib.dm_mine_parallel(None, None, None, 1, 3, None, 4, 4, 5, 0, None, None, None, None, None, None, None) != 0
    if not torch.cuda.is_available():
        with pytest.raises(E.EngineError):
            E.UNetEngine(0).mine_parallel([[torch.zeros(4, 4)] * 3], 2, 2)
    assert callable(E.UNetEngine.mine_parallel) and callable(TypicalityScorer.mine_parallel_patches)
    from diff_mining_amd import dift
    assert callable(dift.parallel_patch_features)
    with pytest.raises(ValueError, match="feature_which"):
        dift.parallel_patch_features("clip+clip", [], [])
