"""Parallel-dataset mining on the GPU: dm_mine_parallel (median map across sets -> selection -> per-set gather) against the
reference's own pandas selection and np.median (tests/golden/parallel_ref.npz, tests/make_golden_parallel.py) and against the
numpy restatement that tests/test_parallel_mining.py pins to them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd.typicality import TypicalityScorer  # noqa: E402
from tests.test_parallel_mining import SORTED_CASES, case_maps, median_by_sort, parallel_numpy  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = E.UNetEngine(0)                      # the map and mining entry points need no weights
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "parallel_ref.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(stack):
    return [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in stack]


def _check_group(res, g, stack, ref_boxes, ref_D, ref_set_D, ref_median, k):
    """group g of a mine_parallel result == the reference bit for bit (the median under ==), unused slots -1 / NaN"""
    boxes, D, set_D, count, medians = res
    boxes, D, set_D, c = boxes[g].cpu().numpy(), D[g].cpu().numpy(), set_D[g].cpu().numpy(), int(count[g])
    n_sets = len(stack)
    assert boxes.shape == (k, 4) and boxes.dtype == np.int32 and D.shape == (k,) and D.dtype == np.float32
    assert set_D.shape == (k, n_sets) and set_D.dtype == np.float32
    assert c == len(ref_boxes), (c, len(ref_boxes))
    assert np.array_equal(boxes[:c], ref_boxes), (boxes[:c].tolist(), np.asarray(ref_boxes).tolist())
    assert np.array_equal(_bits(D[:c]), _bits(ref_D))
    assert np.array_equal(_bits(set_D[:c]), _bits(ref_set_D))
    for r in range(c):                                                        # the input maps at the winners, bit for bit
        assert np.array_equal(_bits(set_D[r]), _bits(np.asarray(stack)[:, boxes[r, 0], boxes[r, 1]]))
    assert (boxes[c:] == -1).all() and np.isnan(D[c:]).all() and np.isnan(set_D[c:]).all()
    med = medians[g].cpu().numpy()
    assert med.dtype == np.float32 and np.array_equal(med, ref_median)


def _prio(fx, shape):
    return torch.from_numpy(TypicalityScorer.permutation_priority(fx["perm_perm"]).reshape(shape))


@pytest.mark.parametrize("tag", SORTED_CASES + ("perm",))
def test_reference_pin_on_the_fixture_cases(engine, fx, tag):
    """df_PD.compute with the reference's `sort` + `get_non_overlapping` and np.median itself: 10 sets in both orders, the group
    that runs out after 3 boxes, 3 and 4 sets, the shuffled frame — same boxes, same D and per-set bits, the same median map."""
    kx, ky, k, asc = (int(v) for v in fx[f"{tag}_args"])
    stack, ref_med = case_maps(fx, tag)
    prio = [_prio(fx, stack.shape[1:])] if tag == "perm" else None
    res = engine.mine_parallel([_dev(stack)], kx, ky, k, bool(asc), prio)
    assert all(t.is_cuda for t in res[:4]) and res[4][0].is_cuda
    _check_group(res, 0, stack, fx[f"{tag}_boxes"], fx[f"{tag}_D"], fx[f"{tag}_set_D"], ref_med, k)


def test_groups_of_mixed_sizes_in_one_call(engine, fx):
    """groups of different sizes ride in one call.  The fixture's cases differ in window and set count, so each (window, set
    count) gets its call, padded with the other maps cut to that set count: per group the same result as alone."""
    big, short, p3, p4 = (fx[f"{t}_maps"] for t in ("p10_desc", "short_desc", "p3_desc", "p4_desc"))
    for tag, others in (("p10_desc", [short, big[:, 3:, 5:]]), ("short_desc", [big, short[::-1]]), ("p3_desc", [big[:3], short[:3]]),
                        ("p4_desc", [short[:4], big[:4]]), ("p10_asc", [short, big[::-1]])):
        kx, ky, k, asc = (int(v) for v in fx[f"{tag}_args"])
        stack, ref_med = case_maps(fx, tag)
        stacks = [others[0], stack, others[1]]
        res = engine.mine_parallel([_dev(s) for s in stacks], kx, ky, k, bool(asc))
        _check_group(res, 1, stack, fx[f"{tag}_boxes"], fx[f"{tag}_D"], fx[f"{tag}_set_D"], ref_med, k)
        for g in (0, 2):
            rb, rd, rs, rm = parallel_numpy(stacks[g], kx, ky, k, bool(asc))
            _check_group(res, g, stacks[g], rb, rd, rs, np.median(stacks[g], axis=0), k)
    # the shuffled arm next to other groups: priority is laid out like the medians
    stacks = [short, big, big[::-1]]
    shapes = [s.shape[1:] for s in stacks]
    prios = [torch.from_numpy(TypicalityScorer.permutation_priority(np.random.default_rng(1).permutation(5 * 12)).reshape(5, 12)),
             _prio(fx, shapes[1]), _prio(fx, shapes[2])]
    res = engine.mine_parallel([_dev(s) for s in stacks], 8, 8, 5, False, prios)
    _check_group(res, 1, big, fx["perm_boxes"], fx["perm_D"], fx["perm_set_D"], fx["p10_desc_median"], 5)
    for g in (0, 2):
        rb, rd, rs, rm = parallel_numpy(stacks[g], 8, 8, 5, False, prios[g].numpy())
        _check_group(res, g, stacks[g], rb, rd, rs, np.median(stacks[g], axis=0), 5)


@pytest.fixture(scope="module")
def noise16():
    return np.random.default_rng(1961).standard_normal((16, 37, 53)).astype(np.float32)


@pytest.mark.parametrize("n_sets", range(1, 17))
def test_every_set_count_against_np_median(engine, noise16, n_sets):
    """37 x 53 = 1961 candidates: no multiple of 64, 256 or 1024, several blocks; two groups, so blockIdx.y is used."""
    stacks = [noise16[:n_sets], noise16[16 - n_sets:][::-1]]
    res = engine.mine_parallel([_dev(s) for s in stacks], 5, 5, 3)
    for g, s in enumerate(stacks):
        ref = np.median(s, axis=0)
        assert ref.dtype == np.float32
        med = res[4][g].cpu().numpy()
        assert np.array_equal(med, ref) and np.array_equal(_bits(med), _bits(ref))          # no zeros here: bit-equal too
        rb, rd, rs, _ = parallel_numpy(s, 5, 5, 3)
        _check_group(res, g, s, rb, rd, rs, ref, 3)


def test_nan_and_signed_zeros(engine, noise16):
    """One NaN in one set makes that candidate's median NaN (numpy's rule) and the candidate is never chosen; integer-valued
    maps with +0 and -0 match np.median under == (the sign of a zero that ties for the middle is free)."""
    for n_sets in (1, 2, 3, 10, 16):
        s = noise16[:n_sets].copy()
        top = np.unravel_index(np.argmax(np.median(s, axis=0)), s.shape[1:])
        s[n_sets // 2][top] = np.nan                                   # the would-be first winner
        s[0, 36, 52] = np.nan                                          # the last candidate
        ref = np.median(s, axis=0)
        assert np.isnan(ref[top]) and np.isnan(ref[36, 52]) and np.isnan(ref).sum() == 2
        res = engine.mine_parallel([_dev(s)], 4, 4, 6)
        med = res[4][0].cpu().numpy()
        assert np.array_equal(np.isnan(med), np.isnan(ref)) and np.array_equal(med[~np.isnan(ref)], ref[~np.isnan(ref)])
        rb, rd, rs, _ = parallel_numpy(s, 4, 4, 6)
        assert int(res[3][0]) == 6 and not np.isnan(rd).any() and tuple(rb[0, :2]) != tuple(top)
        assert np.array_equal(res[0][0].cpu().numpy(), rb) and np.array_equal(_bits(res[1][0].cpu().numpy()), _bits(rd))
        assert np.array_equal(_bits(res[2][0].cpu().numpy()), _bits(rs))
    s = noise16[:3].copy()
    s[1] = np.nan                                                      # a whole set of NaN: nothing to choose
    res = engine.mine_parallel([_dev(s)], 4, 4, 2)
    assert int(res[3][0]) == 0 and (res[0][0] == -1).all() and torch.isnan(res[1][0]).all() and torch.isnan(res[2][0]).all()
    assert torch.isnan(res[4][0]).all()
    rng = np.random.default_rng(5)
    for n_sets in (2, 3, 4, 7, 10, 16):
        z = rng.integers(-2, 3, (n_sets, 37, 53)).astype(np.float32)
        z[rng.random(z.shape) < 0.25] = -0.0
        res = engine.mine_parallel([_dev(z)], 5, 5, 1)
        med, ref = res[4][0].cpu().numpy(), np.median(z, axis=0)
        assert (med == ref).all() and not np.isnan(med).any()
        assert np.array_equal(med, median_by_sort(z))


def _grid(rng, N, nc, h, w, dtype=np.float16):
    return torch.from_numpy((1.0 + 0.3 * rng.standard_normal((N, nc, 4, h, w))).astype(dtype))


@pytest.fixture(scope="module")
def e2e():
    rng = np.random.default_rng(23)
    sizes = [(64, 85), (45, 37), (64, 85)]
    lat = [(8, 11), (6, 5), (8, 11)]
    groups = [[_grid(rng, 2, 2, h, w) for _ in range(3)] for (h, w) in lat]
    return groups, sizes, ["France", "Japan", "Italy"], ["Japan", "France", "Italy"]


def _host_rows(engine, groups, sizes, kx, ky, k, ascending=False):
    """batched maps (pinned bit-exact elsewhere), downloaded, then the numpy restatement, as rows"""
    out = []
    for g, (gr, hw) in enumerate(zip(groups, sizes)):
        maps = engine.typicality_image_batched(gr, [hw] * len(gr), kx, ky)
        stack = np.stack([m.cpu().numpy() for m in maps])
        b, d, s, _ = parallel_numpy(stack, kx, ky, k, ascending)
        out.append((g, b, d, s))
    return out


def test_end_to_end_from_the_fp16_grids(engine, e2e):
    """groups of three fp16 grids at different image sizes: mine_parallel_patches == batched maps, downloaded, then the numpy
    restatement; groups_per_call 1 and 8 give identical rows; top_k and boxes_by_image take the rows as they are."""
    groups, sizes, names, origins = e2e
    sc = TypicalityScorer(engine)
    for asc in (False, True):
        rows = sc.mine_parallel_patches(groups, sizes, names, origins, k_per_image=3, kx=9, ky=9, ascending=asc)
        assert list(rows) == TypicalityScorer.parallel_columns(names)
        host = _host_rows(engine, groups, sizes, 9, 9, 3, asc)
        assert rows["group"].tolist() == [g for g, b, _, _ in host for _ in b] and len(rows["D"]) >= 6
        assert np.array_equal(np.stack([rows[c] for c in ("x_start", "y_start", "x_end", "y_end")], 1), np.concatenate([b for _, b, _, _ in host]))
        assert np.array_equal(_bits(rows["D"]), _bits(np.concatenate([d for _, _, d, _ in host])))
        for c, name in enumerate(names):
            assert np.array_equal(_bits(rows[name]), _bits(np.concatenate([s[:, c] for _, _, _, s in host])))
        assert rows["origin"].tolist() == [origins[g] for g in rows["group"]]
        one = sc.mine_parallel_patches(groups, sizes, names, origins, k_per_image=3, kx=9, ky=9, ascending=asc, groups_per_call=1)
        assert list(one) == list(rows)
        for c in rows:
            assert one[c].dtype == rows[c].dtype and (np.array_equal(_bits(one[c]), _bits(rows[c])) if rows[c].dtype == np.float32
                                                      else one[c].tolist() == rows[c].tolist()), c
    per = TypicalityScorer.boxes_by_image(rows)
    assert len(per) == 3 and all(np.array_equal(p, b) for p, (_, b, _, _) in zip(per, host))
    top = TypicalityScorer.top_k(rows, 4)
    assert list(top) == list(rows) and len(top["D"]) == 4 and (np.diff(top["D"]) <= 0).all() and top["D"][0] == rows["D"].max()
    order = np.argsort(-rows["D"].astype(np.float64), kind="stable")[:4]
    assert all(np.array_equal(top[n], rows[n][order]) for n in names) and top["group"].tolist() == rows["group"][order].tolist()


def test_random_arm_is_a_seeded_permutation_per_group(engine, e2e):
    groups, sizes, names, origins = e2e
    sc = TypicalityScorer(engine)
    rnd = sc.mine_parallel_patches(groups, sizes, names, origins, k_per_image=3, kx=9, ky=9, randomized=True, seed=42, groups_per_call=2)
    for g, (gr, hw) in enumerate(zip(groups, sizes)):
        stack = np.stack([m.cpu().numpy() for m in engine.typicality_image_batched(gr, [hw] * 3, 9, 9)])
        perm = np.random.default_rng((42, g)).permutation(stack[0].size)
        rb, rd, rs, _ = parallel_numpy(stack, 9, 9, 3, priority=TypicalityScorer.permutation_priority(perm).reshape(stack.shape[1:]))
        sel = rnd["group"] == g
        assert np.array_equal(TypicalityScorer.boxes_by_image(rnd)[g], rb) and np.array_equal(_bits(rnd["D"][sel]), _bits(rd))
        assert np.array_equal(_bits(rnd["Japan"][sel]), _bits(rs[:, 1]))
        assert rb[0, 0] * stack.shape[2] + rb[0, 1] == perm[0]                # the shuffled frame's first row is taken first


def test_views_of_the_packed_map_buffer_are_read_in_place(engine, e2e):
    groups, sizes, _, _ = e2e
    maps = engine.typicality_image_batched(groups[0] + groups[2], [sizes[0]] * 6, 9, 9)
    base, off, copied = E.UNetEngine._place_maps(torch, maps, engine.device)
    assert not copied and base.data_ptr() == maps[0].data_ptr() and off == [i * maps[0].numel() for i in range(6)]
    a = engine.mine_parallel([maps[:3], maps[3:]], 9, 9, 3)
    b = engine.mine_parallel([[m.clone() for m in maps[:3]], [m.clone() for m in maps[3:]]], 9, 9, 3)          # separate buffers: packed
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:4], b[:4]))
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def test_refusals_are_errors(engine):
    m = torch.zeros(8, 8)
    with pytest.raises(E.EngineError, match="n_sets 17"):
        engine.mine_parallel([[m] * 17], 2, 2)
    with pytest.raises(E.EngineError, match="set 1 of group 1"):
        engine.mine_parallel([[m, m], [m, torch.zeros(8, 9)]], 2, 2)
    for k in (0, 65):
        with pytest.raises(E.EngineError, match="k_per_image"):
            engine.mine_parallel([[m, m]], 2, 2, k)
    with pytest.raises(E.EngineError, match="bad window"):
        TypicalityScorer(engine).mine_parallel_patches([[torch.zeros(1, 2, 4, 4, 4, dtype=torch.float16)] * 2], [(8, 40)], ["a", "b"], ["a"], kx=9, ky=9)
    # the C entry point itself
    lib, h = engine.lib, engine._h
    n_sets = 2
    desc = np.zeros(2 * n_sets, dtype=E.MINE_DESC_DTYPE)
    gdesc = np.zeros(2, dtype=E.MINE_DESC_DTYPE)
    for g in range(2):
        gdesc[g]["map_offset"], gdesc[g]["H"], gdesc[g]["W"] = g * 500, 8, 40
        for c in range(n_sets):
            desc[g * n_sets + c]["map_offset"], desc[g * n_sets + c]["H"], desc[g * n_sets + c]["W"] = (g * n_sets + c) * 500, 8, 40
    odd = desc.copy()
    odd[3]["W"] = 39
    up = lambda a: torch.from_numpy(a.view(np.uint8)).cuda()          # noqa: E731
    dd, gd, od = up(desc), up(gdesc), up(odd)
    buf = torch.zeros(8192, device="cuda")
    bx = torch.zeros(2 * 64 * 4, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())               # noqa: E731
    s = engine._stream()

    def call(desc_d=dd, n_sets=2, kx=4, ky=4, k=5, maps=buf, med=buf):
        return lib.dm_mine_parallel(h, p(maps) if maps is not None else None, p(desc_d), 2, n_sets, p(gd), kx, ky, k, 0, None,
                                    p(med) if med is not None else None, p(bx), p(buf), p(buf), p(bx), s)

    def err():
        return lib.dm_last_error(h).decode()
    assert call(n_sets=17) != 0 and "n_sets 17 outside [1, 16]" in err()
    assert call(n_sets=0) != 0 and "n_sets 0" in err()
    assert call(desc_d=od) != 0 and "set 1 of group 1 is 8x39, the group 8x40" in err()
    assert call(kx=9, ky=9) != 0 and "bad window 9x9 for 8x40" in err()
    assert call(k=65) != 0 and "k_per_image 65" in err()
    assert call(k=0) != 0 and "k_per_image 0" in err()
    assert call(maps=None) != 0 and "null argument" in err()
    assert call(med=None) != 0 and "null argument" in err()
    torch.cuda.synchronize()
    res = engine.mine_parallel([[m, m]], 2, 2, 2)         # the engine is still usable
    assert int(res[3][0]) == 2 and res[0][0, 0].tolist() == [0, 0, 2, 2]


def test_bit_identical_run_to_run(engine, noise16):
    g = torch.Generator().manual_seed(449620)
    stacks = [[torch.randn(193, 278, generator=g).cuda() for _ in range(10)], _dev(noise16[:10])]
    first = engine.mine_parallel(stacks, 16, 16, 5)
    for _ in range(3):
        again = engine.mine_parallel(stacks, 16, 16, 5)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first[:4], again[:4]))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first[4], again[4]))
    rb, rd, rs, rm = parallel_numpy(np.stack([m.cpu().numpy() for m in stacks[0]]), 16, 16, 5)
    _check_group(first, 0, np.stack([m.cpu().numpy() for m in stacks[0]]), rb, rd, rs, rm, 5)


def test_parallel_patch_features_layout():
    """`embed_batch`'s layout: the sets' blocks one after another; for 'clip+dift-T' every CLIP block, then every DIFT block —
    each block torch.equal to the per-image `patch_features`."""
    from diff_mining_amd import dift, synth
    from tests.test_gpu_clip_vision import _img
    net = E.UNetEngineF32(0)
    aux = E.UNetEngine(0)                                 # the DIFT patch kernel only: no weights needed
    try:
        net.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
        fz = dift.SDFeaturizer(net, aux=aux)
        imgs = [_img(90, 70, s) for s in range(3)]
        boxes = [(0, 0, 64, 64), (26, 6, 90, 70)]
        rng = np.random.default_rng(0)
        feats = [torch.from_numpy(rng.normal(size=(1, 1280, 12, 9)).astype(np.float32)).to(net.device) for _ in range(3)]
        a = dift.parallel_patch_features("clip", imgs, boxes, clip_net=net)
        b = dift.parallel_patch_features("dift-261", imgs, boxes, featurizer=fz, feats=feats)
        ab = dift.parallel_patch_features("clip+dift-261", imgs, boxes, featurizer=fz, clip_net=net, feats=feats)
        assert a.shape == (2, 3 * 512) and b.shape == (2, 3 * 1280) and ab.shape == (2, 3 * 1792) and ab.dtype == torch.float32
        for c in range(3):
            one = dift.patch_features("clip+dift-261", imgs[c], boxes, featurizer=fz, clip_net=net, feat=feats[c])
            assert torch.equal(a[:, c * 512:(c + 1) * 512], one[:, :512])
            assert torch.equal(b[:, c * 1280:(c + 1) * 1280], one[:, 512:])
        assert torch.equal(ab, torch.cat([a, b], 1))                           # all CLIP blocks first, then all DIFT blocks
        assert not torch.equal(a[:, :512], a[:, 512:1024])
        with pytest.raises(ValueError):
            dift.parallel_patch_features("clip", imgs + [_img(64, 64, 0)], boxes, clip_net=net)
        with pytest.raises(ValueError):
            dift.parallel_patch_features("dift-261", imgs, boxes, featurizer=fz)
    finally:
        aux.close()
        net.close()
