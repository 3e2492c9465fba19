"""Patch mining on the GPU: dm_typicality_image_batched + dm_mine_patches against the reference's own pandas selection
(tests/golden/mining_ref.npz, tests/make_golden_mining.py) and against the numpy restatement that tests/test_mining.py pins to it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd.typicality import TypicalityScorer  # noqa: E402
from tests.test_mining import SORTED_CASES, greedy_numpy  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = E.UNetEngine(0)                      # the map and mining entry points need no weights
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "mining_ref.npz"))


@pytest.fixture(scope="module")
def cons():
    return np.load(os.path.join(GOLDEN, "consumers_ref.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_against(boxes, D, count, b, ref_boxes, ref_D, k):
    """image b of a mine_patches result == (ref_boxes, ref_D) bit for bit, unused slots -1 / NaN"""
    boxes, D, c = boxes[b].cpu().numpy(), D[b].cpu().numpy(), int(count[b])
    assert boxes.shape == (k, 4) and boxes.dtype == np.int32 and D.shape == (k,) and D.dtype == np.float32
    assert c == len(ref_boxes), (c, len(ref_boxes))
    assert np.array_equal(boxes[:c], ref_boxes), (boxes[:c].tolist(), np.asarray(ref_boxes).tolist())
    assert np.array_equal(_bits(D[:c]), _bits(ref_D))
    assert (boxes[c:] == -1).all() and np.isnan(D[c:]).all()


@pytest.mark.parametrize("tag", SORTED_CASES + ("perm",))
def test_reference_pin_on_the_fixture_maps(engine, fx, tag):
    """The reference's `sort` + `get_non_overlapping` on its own frame, both orders, the map that runs out after 2 boxes and the
    shuffled frame: same boxes, same D bits."""
    kx, ky, k, asc = (int(v) for v in fx[f"{tag}_args"])
    dm = torch.from_numpy(fx[f"{tag}_map"])
    prio = None
    if tag == "perm":
        prio = [torch.from_numpy(TypicalityScorer.permutation_priority(fx["perm_perm"]).reshape(tuple(dm.shape)))]
    boxes, D, count = engine.mine_patches([dm], kx, ky, k, bool(asc), prio)
    assert boxes.is_cuda and D.is_cuda and count.is_cuda
    _check_against(boxes, D, count, 0, fx[f"{tag}_boxes"], fx[f"{tag}_D"], k)


def test_all_fixture_maps_in_one_call(engine, fx):
    """maps of different sizes ride in one launch (the fixture's `a`, `short` and `a` again share their window only pairwise, so
    each window gets its call): per image the same result as alone"""
    for tags in (("a_desc", "perm"), ("short_desc", "short_desc")):
        kx, ky, k, _ = (int(v) for v in fx[f"{tags[0]}_args"])
        maps = [torch.from_numpy(fx[f"{t}_map"]) for t in tags] + [torch.from_numpy(fx["short_desc_map"])]
        boxes, D, count = engine.mine_patches(maps, kx, ky, k)
        for b, m in enumerate(maps):
            rb, rd = greedy_numpy(m.numpy(), kx, ky, k)
            _check_against(boxes, D, count, b, rb, rd, k)
    _check_against(boxes, D, count, 0, fx["short_desc_boxes"], fx["short_desc_D"], k)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_end_to_end_from_the_fp16_grids(engine, fx, cons, tag):
    """grids -> typicality_image_batched -> mine_patches: the reference's boxes exactly (every round's lead is >= 1e-5 of max|dm|,
    the engine's map is within ~1e-6 of the reference's), D within 1e-6 relative (of max(max|dm|, 1), the form of
    test_consumers_vs_the_reference_fixture's bound on the maps)."""
    grid = torch.from_numpy(cons[f"{tag}_grid"])
    H, W, k = (int(v) for v in cons[f"{tag}_size"])
    assert grid.dtype == torch.float16
    maps = engine.typicality_image_batched([grid], [(H, W)], k, k)
    scale = max(float(np.abs(fx[f"{tag}_desc_map"]).max()), 1.0)
    print(f"[{tag}] map vs the reference's: max |d| {np.abs(maps[0].cpu().numpy() - fx[f'{tag}_desc_map']).max():.3e}, max|dm| {np.abs(fx[f'{tag}_desc_map']).max():.3e}")
    for order, asc in (("desc", False), ("asc", True)):
        boxes, D, count = engine.mine_patches(maps, k, k, 5, asc)
        ref_b, ref_D = fx[f"{tag}_{order}_boxes"], fx[f"{tag}_{order}_D"]
        got_b, got_D = boxes[0].cpu().numpy(), D[0].cpu().numpy()
        err = np.abs(got_D.astype(np.float64) - ref_D.astype(np.float64)).max() / scale
        print(f"[{tag} {order}] boxes {got_b.tolist()} max |dD| / scale {err:.3e} (min lead {fx[f'{tag}_{order}_leads'].min():.3e})")
        assert int(count[0]) == len(ref_b) == 5 and np.array_equal(got_b, ref_b)
        assert err <= 1e-6, err


def _grid(rng, N, nc, h, w, dtype):
    return torch.from_numpy((1.0 + 0.3 * rng.standard_normal((N, nc, 4, h, w))).astype(dtype))


def test_batched_maps_bit_equal_to_the_single_image_entry(engine):
    """7 images of mixed sizes, fp16 and fp32 grids, n_cond 1 and 2, draw counts 1..5: every map equals its own
    dm_typicality_image call bit for bit; likewise an all-fp16 batch (the packed buffer stays fp16 then)."""
    rng = np.random.default_rng(7)
    spec = [(3, 2, 8, 8, 64, 64, np.float16), (2, 2, 12, 10, 45, 37, np.float32), (5, 2, 16, 21, 128, 171, np.float16),
            (1, 1, 8, 10, 40, 50, np.float16), (4, 2, 21, 16, 171, 128, np.float32), (2, 1, 6, 6, 33, 47, np.float32),
            (3, 2, 32, 42, 256, 341, np.float16)]
    grids = [_grid(rng, N, nc, h, w, dt) for (N, nc, h, w, _, _, dt) in spec]
    sizes = [(H, W) for (_, _, _, _, H, W, _) in spec]
    for kx, ky in ((5, 5), (32, 20), (1, 1)):
        for sel in (range(7), [0, 2, 3, 6]):
            gs, ss = [grids[i] for i in sel], [sizes[i] for i in sel]
            maps = engine.typicality_image_batched(gs, ss, kx, ky)
            assert len(maps) == len(gs)
            for g, s, m in zip(gs, ss, maps):
                one = engine.typicality_image(g, s, kx, ky)
                assert m.shape == one.shape == (s[0] - kx + 1, s[1] - ky + 1) and m.dtype == torch.float32 and m.is_cuda
                assert torch.equal(m, one), (kx, ky, s, (m - one).abs().max().item())


def _real_size_maps(n):
    g = torch.Generator().manual_seed(449620)
    return [torch.randn((449, 620) if b % 2 == 0 else (193, 278), generator=g) for b in range(n)]


def test_selection_at_real_sizes_batched_and_one_by_one(engine):
    """449 x 620 (a 512 x 683 image) and 193 x 278 (256 x 341) candidate maps, 64 x 64 windows: 64 images in one call == the same
    images one by one == the numpy restatement, both orders; and on the engine's own pooled maps of such images."""
    maps = _real_size_maps(64)
    for asc in (False, True):
        boxes, D, count = engine.mine_patches(maps, 64, 64, 5, asc)
        for b, m in enumerate(maps):
            b1, d1, c1 = engine.mine_patches([m], 64, 64, 5, asc)
            assert torch.equal(b1[0], boxes[b]) and torch.equal(d1[0].view(torch.int32), D[b].view(torch.int32)) and torch.equal(c1[0], count[b])
            if b < 8:
                rb, rd = greedy_numpy(m.numpy(), 64, 64, 5, asc)
                _check_against(boxes, D, count, b, rb, rd, 5)
    rng = np.random.default_rng(11)
    grids = [_grid(rng, 2, 2, 64, 85, np.float16), _grid(rng, 2, 2, 32, 42, np.float16)]
    own = engine.typicality_image_batched(grids, [(512, 683), (256, 341)], 64, 64)
    assert tuple(own[0].shape) == (449, 620) and tuple(own[1].shape) == (193, 278)
    for asc in (False, True):
        boxes, D, count = engine.mine_patches(own, 64, 64, 5, asc)
        for b, m in enumerate(own):
            rb, rd = greedy_numpy(m.cpu().numpy(), 64, 64, 5, asc)
            _check_against(boxes, D, count, b, rb, rd, 5)


def test_ties_go_to_the_lowest_row_major_index(engine):
    const = torch.full((40, 50), 0.25)
    two = torch.zeros(40, 50)
    two[30, 7] = two[12, 44] = 3.0                       # two equal maxima, the later row first in value order
    zeros = torch.zeros(9, 9)
    zeros[4, 4] = -0.0                                   # -0 ties with +0
    for m, k in ((const, 6), (two, 3), (zeros, 2)):
        for asc in (False, True):
            boxes, D, count = engine.mine_patches([m], 8, 8, k, asc)
            rb, rd = greedy_numpy(m.numpy(), 8, 8, k, asc)
            _check_against(boxes, D, count, 0, rb, rd, k)
    boxes, _, _ = engine.mine_patches([two], 8, 8, 3)
    assert boxes[0, :2, :2].tolist() == [[12, 44], [30, 7]]
    boxes, _, _ = engine.mine_patches([const], 8, 8, 6)
    assert boxes[0, :, :2].tolist() == [[0, 0], [0, 9], [0, 18], [0, 27], [0, 36], [0, 45]]


def test_nan_entries_are_never_chosen(engine):
    g = torch.Generator().manual_seed(3)
    m = torch.randn(60, 70, generator=g)
    m[torch.rand(60, 70, generator=g) < 0.3] = float("nan")
    m[10, 10] = float("nan")
    for asc in (False, True):
        boxes, D, count = engine.mine_patches([m, torch.full((20, 20), float("nan"))], 6, 6, 8, asc)
        rb, rd = greedy_numpy(m.numpy(), 6, 6, 8, asc)
        _check_against(boxes, D, count, 0, rb, rd, 8)
        assert not torch.isnan(D[0, :int(count[0])]).any() and int(count[0]) == 8
        assert int(count[1]) == 0 and (boxes[1] == -1).all() and torch.isnan(D[1]).all()
    # a NaN priority hides a candidate, a NaN in the map under a finite priority is reported as it is
    pr = torch.arange(16, dtype=torch.float32).reshape(4, 4)
    pr[3, 3] = float("nan")
    dm = torch.ones(4, 4)
    dm[3, 2] = float("nan")
    boxes, D, count = engine.mine_patches([dm], 1, 1, 1, False, [pr])
    assert boxes[0, 0].tolist() == [3, 2, 4, 3] and torch.isnan(D[0, 0]) and int(count[0]) == 1


def test_k_per_image_one_and_the_cap(engine):
    g = torch.Generator().manual_seed(5)
    m = torch.randn(449, 620, generator=g)
    for k in (1, E.MINE_MAX_K):
        boxes, D, count = engine.mine_patches([m], 16, 16, k)
        rb, rd = greedy_numpy(m.numpy(), 16, 16, k)
        assert len(rb) == k                               # 16 x 16 windows: far more than 64 fit
        _check_against(boxes, D, count, 0, rb, rd, k)


def test_refusals_are_errors(engine):
    m = [torch.zeros(8, 8)]
    for k in (0, -1, E.MINE_MAX_K + 1):
        with pytest.raises(E.EngineError, match="k_per_image"):
            engine.mine_patches(m, 2, 2, k)
    with pytest.raises(E.EngineError, match="bad window"):
        engine.typicality_image_batched([torch.zeros(1, 2, 4, 4, 4, dtype=torch.float16)] * 2, [(32, 32), (8, 40)], 9, 9)
    # the C entry points themselves
    lib, h = engine.lib, engine._h
    desc = np.zeros(1, dtype=E.MINE_DESC_DTYPE)
    desc[0] = (0, 0, 0, 1, 2, 4, 4, 8, 40)
    dd = torch.from_numpy(desc.view(np.uint8)).cuda()
    buf = torch.zeros(4096, device="cuda")
    bx = torch.zeros(64 * 4 + 64, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    s = engine._stream()

    def err():
        return lib.dm_last_error(h).decode()
    assert lib.dm_mine_patches(h, p(buf), None, p(dd), 1, 9, 9, 5, 0, p(bx), p(buf), p(bx), s) != 0 and "bad window 9x9 for 8x40" in err()
    assert lib.dm_mine_patches(h, p(buf), None, p(dd), 1, 4, 4, 65, 0, p(bx), p(buf), p(bx), s) != 0 and "k_per_image 65" in err()
    assert lib.dm_mine_patches(h, p(buf), None, p(dd), 1, 4, 4, 0, 0, p(bx), p(buf), p(bx), s) != 0 and "k_per_image 0" in err()
    assert lib.dm_mine_patches(h, None, None, p(dd), 1, 4, 4, 5, 0, p(bx), p(buf), p(bx), s) != 0 and "null argument" in err()
    assert lib.dm_mine_patches(h, p(buf), None, None, 1, 4, 4, 5, 0, p(bx), p(buf), p(bx), s) != 0 and "null argument" in err()
    assert lib.dm_mine_patches(h, p(buf), None, p(dd), 1, 4, 4, 5, 0, None, p(buf), p(bx), s) != 0 and "null argument" in err()
    assert lib.dm_typicality_image_batched(h, p(buf), 0, p(dd), 1, 9, 9, p(buf), p(buf), s) != 0 and "bad window 9x9 for 8x40" in err()
    assert lib.dm_typicality_image_batched(h, None, 0, p(dd), 1, 4, 4, p(buf), p(buf), s) != 0 and "null argument" in err()
    assert lib.dm_typicality_image_batched(h, p(buf), 0, p(dd), 1, 4, 4, None, p(buf), s) != 0 and "null argument" in err()
    assert lib.dm_typicality_image_batched(h, p(buf), 0, p(dd), 0, 4, 4, p(buf), p(buf), s) != 0
    torch.cuda.synchronize()
    boxes, _, count = engine.mine_patches(m, 2, 2, 2)     # the engine is still usable
    assert int(count[0]) == 2 and boxes[0, 0].tolist() == [0, 0, 2, 2]


def test_selection_is_bit_identical_run_to_run(engine):
    maps = _real_size_maps(6)
    first = engine.mine_patches(maps, 64, 64, 5)
    for _ in range(3):
        again = engine.mine_patches(maps, 64, 64, 5)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))


def test_host_mirror_rows_and_the_random_arm(engine, fx, cons, tmp_path):
    """TypicalityScorer.mine_patches: the reference's columns in image order then round order, from grids and from stored
    .npy paths, in calls of a given size; the random arm is a seeded permutation's selection."""
    sc = TypicalityScorer(engine)
    sc.typicality_path = str(tmp_path)
    ga = cons["a_grid"]
    H, W, k = (int(v) for v in cons["a_size"])
    path = "/data/cars/1970__img_001.jpg"
    sc.save_grid(str(tmp_path), path, torch.from_numpy(ga))
    rows = sc.mine_patches([ga, path, torch.from_numpy(ga)], [(H, W)] * 3, k_per_image=5, kx=k, ky=k, images_per_call=2)
    assert set(rows) == set(TypicalityScorer.MINE_COLUMNS) | {"image"}
    assert rows["image"].tolist() == [0] * 5 + [1] * 5 + [2] * 5 and rows["seed"].tolist() == [0] * 5 + [path] * 5 + [2] * 5
    assert (rows["origin"] == "real").all() and rows["D"].dtype == np.float32
    per = TypicalityScorer.boxes_by_image(rows)
    assert len(per) == 3 and all(np.array_equal(b, fx["a_desc_boxes"]) for b in per)
    least = sc.mine_patches([ga], [(H, W)], k_per_image=5, kx=k, ky=k, ascending=True)
    assert np.array_equal(TypicalityScorer.boxes_by_image(least)[0], fx["a_asc_boxes"])
    top = TypicalityScorer.top_k(rows, 4)
    assert len(top["D"]) == 4 and (np.diff(top["D"]) <= 0).all()
    rnd = sc.mine_patches([ga, ga], [(H, W)] * 2, k_per_image=5, kx=k, ky=k, randomized=True, seed=42)
    dm = engine.typicality_image(torch.from_numpy(ga), (H, W), k, k).cpu().numpy()
    for i, b in enumerate(TypicalityScorer.boxes_by_image(rnd)):
        perm = np.random.default_rng((42, i)).permutation(dm.size)
        rb, rd = greedy_numpy(dm, k, k, 5, priority=TypicalityScorer.permutation_priority(perm).reshape(dm.shape))
        assert np.array_equal(b, rb) and np.array_equal(_bits(rnd["D"][rnd["image"] == i]), _bits(rd))
        assert rb[0, 0] * dm.shape[1] + rb[0, 1] == perm[0]                   # the shuffled frame's first row is taken first
    assert not np.array_equal(*TypicalityScorer.boxes_by_image(rnd))          # another permutation per image


def test_mined_boxes_feed_the_clip_patch_features(engine):
    """grids -> maps -> boxes -> features: the mined rows go into clip_patch_features as they are, and give the features of
    the same boxes written out as host tuples."""
    from diff_mining_amd import synth
    from tests.test_gpu_clip_vision import _img
    net = E.UNetEngineF32(0)
    try:
        net.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
        rng = np.random.default_rng(13)
        sizes = [(256, 341), (200, 256)]
        grids = [_grid(rng, 2, 2, 32, 42, np.float16), _grid(rng, 2, 2, 25, 32, np.float16)]
        rows = TypicalityScorer(engine).mine_patches(grids, sizes, k_per_image=3, kx=64, ky=64)
        per = TypicalityScorer.boxes_by_image(rows)
        assert [len(b) for b in per] == [3, 3]
        imgs = [_img(h, w, i) for i, (h, w) in enumerate(sizes)]
        feats = net.clip_patch_features(imgs, per)
        tuples = [[tuple(int(v) for v in b) for b in bl] for bl in per]
        assert feats.shape == (6, 512) and torch.equal(feats, net.clip_patch_features(imgs, tuples))
        assert torch.isfinite(feats).all()
    finally:
        net.close()
