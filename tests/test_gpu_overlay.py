"""Typicality overlays on the GPU: dm_gaussian_filter_maps and dm_overlay_blend against the numpy restatements that tests/test_overlay.py
pins to scipy, PIL and the reference's own functions (tests/golden/overlay_ref.npz) - bit for bit and byte for byte, no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import overlay as O  # noqa: E402
from diff_mining_amd.typicality import TypicalityScorer  # noqa: E402
from tests import gpu_util as U  # noqa: E402
from tests import make_golden_overlay as G  # noqa: E402

T = O.GAUSS_TILE
# 1 x 1; one row; 23 rows (narrower than the radius of 40: the index reflects repeatedly); two tiles by two; a map exactly one tile wide, one
# element wider, one narrower (40 rows: a second, partial tile row)
FILTER_SHAPES = [(1, 1), (1, 57), (23, 130), (64, 64), (40, T), (40, T + 1), (40, T - 1)]
SIGMAS = (0.4, 2, 10)


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = E.UNetEngine(0)                      # the map and overlay entry points need no weights
    yield e
    e.close()


@pytest.fixture(scope="module")
def fx():
    return np.load(G.PATH)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _filter_inputs():
    rng = np.random.default_rng(77)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in FILTER_SHAPES)


@functools.lru_cache(maxsize=None)
def _filtered(sigma):
    """the restatement of every test map at one sigma, computed once and shared by the three post-ops"""
    return tuple(O.gaussian_filter_host(a, sigma) for a in _filter_inputs())


@pytest.mark.parametrize("post_op", list(O.POST_OPS))
@pytest.mark.parametrize("sigma", SIGMAS)
def test_filter_is_the_restatement_bit_for_bit(engine, sigma, post_op):
    """all seven maps in ONE call per (sigma, post-op); -0.0 of the clamp included"""
    maps = [torch.from_numpy(a).to(engine.device) for a in _filter_inputs()]
    got, mx = engine.gaussian_filter(maps, sigma, post_op, return_max=True)
    assert len(got) == len(FILTER_SHAPES)
    for shape, g, F in zip(FILTER_SHAPES, got, _filtered(sigma)):
        want, m, degenerate = O.post_op_host(F, post_op)
        assert tuple(g.shape) == shape and not degenerate
        bad = int((_bits(_np(g)) != _bits(want)).sum())
        print(f"filter sigma {sigma} {post_op} {shape}: {bad} of {want.size} elements differ")
        assert bad == 0, (shape, sigma, post_op, bad)
    if post_op == "unit":
        assert np.array_equal(_bits(_np(mx)), _bits(np.array([F.max() for F in _filtered(sigma)], np.float32)))
    else:
        assert mx is None


def test_filter_reads_views_in_place_and_refuses(engine):
    """views of one packed buffer (what `typicality_image_batched` returns) are read where they lie; bad arguments are refused
    without a launch and the device stays usable"""
    a, b = _filter_inputs()[2], _filter_inputs()[5]
    buf = torch.cat([torch.from_numpy(a).reshape(-1), torch.from_numpy(b).reshape(-1)]).to(engine.device)
    views = [buf[:a.size].view(a.shape), buf[a.size:].view(b.shape)]
    got = engine.gaussian_filter(views, 2)
    assert np.array_equal(_bits(_np(got[0])), _bits(_filtered(2)[2])) and np.array_equal(_bits(_np(got[1])), _bits(_filtered(2)[5]))
    lib, s = engine.lib, engine._stream()
    w, r = O.gauss_weights(2)
    w_d = torch.from_numpy(w).to(engine.device)
    desc = np.zeros(1, O.GAUSS_DESC_DTYPE)
    desc["H"], desc["W"] = a.shape
    out = torch.empty(a.size, dtype=torch.float32, device=engine.device)
    need = O.workspace_bytes(1, a.size, *a.shape)
    work = torch.empty(need, dtype=torch.uint8, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def call(d, work_bytes=need, sigma=2.0, radius=r):
        d_d = torch.from_numpy(d.view(np.uint8)).to(engine.device)
        return lib.dm_gaussian_filter_maps(p(buf), p(d_d), 1, sigma, p(w_d), radius, 0, p(work), work_bytes, p(out), None, s)
    assert call(desc) == 0
    assert call(desc, work_bytes=need - 4) == 1                            # a workspace that is too small
    assert call(desc, sigma=0.0, radius=0) == 1 and call(desc, sigma=-1.0) == 1 and call(desc, radius=r + 1) == 1
    for field, v in (("H", 0), ("W", -3), ("map_offset", -1), ("work_offset", 1), ("out_offset", -8)):
        bad = desc.copy()
        bad[field] = v
        assert call(bad) == 1, field
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(out.view(a.shape))), _bits(_filtered(2)[2]))


def _rows(boxes, image=None):
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    return {"image": np.arange(len(b)) if image is None else np.asarray(image), "x_start": b[:, 0], "y_start": b[:, 1],
            "x_end": b[:, 2], "y_end": b[:, 3]}


def _dev(engine, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(engine.device) for a in arrays]


def _check_patch_stats(got, q, plain):
    s, verdict = O.filter_patch_host(plain)
    assert int(got["lum_sum"][q]) == s and bool(got["verdict"][q]) == verdict
    assert np.array_equal(_np(got["plain"][q]), plain)


def test_blend_image_variant_vs_the_reference(engine, fx):
    """`load_and_apply_alpha_bbox`: the four fixture cases (a map smaller than its image, the corner box, the whole-image box on a map
    narrower than the radius) in one call, plus a second box on the first image and a zero-area box"""
    cases = list(G.IMAGE_CASES)
    images = [fx[f"image_{k}_img"] for k in cases]
    maps = [fx[f"image_{k}_alpha"] for k in cases]
    boxes = [fx[f"image_{k}_box"] for k in cases] + [(0, 0, 17, 33), (5, 7, 5, 40)]
    rows = _rows(boxes, list(range(len(cases))) + [0, 1])
    got = engine.overlay_rows(_dev(engine, images), _dev(engine, maps), rows, "image", 10, want_alpha=True)
    for q, k in enumerate(cases):
        assert np.array_equal(_np(got["blended"][q]), fx[f"image_{k}_out"]), k
        assert np.array_equal(_bits(_np(got["alpha"][q]).astype(np.float64)), _bits(fx[f"image_{k}_alpha_crop"][..., 0])), k
        b = boxes[q]
        _check_patch_stats(got, q, images[q][b[0]:b[2], b[1]:b[3]])
    u8, alpha = O.alpha_bbox_host(maps[0], images[0], boxes[4])
    assert np.array_equal(_np(got["blended"][4]), u8) and np.array_equal(_np(got["alpha"][4]).astype(np.float64), alpha[..., 0])
    _check_patch_stats(got, 4, images[0][0:17, 0:33])
    assert tuple(got["blended"][5].shape) == (0, 33, 3) and int(got["lum_sum"][5]) == 0 and not bool(got["verdict"][5])
    assert not _np(got["degenerate"]).any()


def test_blend_crop_variant_vs_the_reference(engine, fx):
    """`apply_alpha`: sigma 10 and sigma 2, the all-negative crops, and a `degenerate` row (a zero map: the flag, and the pixels T = 0
    gives) beside a zero-area row"""
    for sigma in (10, 2):
        cases = [k for k, c in G.CROP_CASES.items() if c[1] == sigma]
        patches = [fx[f"crop_{k}_patch"] for k in cases]
        maps = [fx[f"crop_{k}_T"] for k in cases]
        boxes = [(0, 0) + m.shape for m in maps]
        image = list(range(len(cases)))
        if sigma == 10:
            patches.append(fx["patch_mid_rgb"])
            maps.append(np.zeros((64, 64), np.float32))
            boxes += [(3, 5, 40, 64), (9, 9, 20, 9)]
            image += [len(cases), len(cases)]
        got = engine.overlay_rows(_dev(engine, patches), _dev(engine, maps), _rows(boxes, image), "crop", sigma, want_alpha=True)
        for q, k in enumerate(cases):
            assert np.array_equal(_np(got["blended"][q]), fx[f"crop_{k}_out"]), k
            want = O.post_op_host(O.gaussian_filter_host(maps[q], sigma), "unit")[0]
            assert np.array_equal(_bits(_np(got["alpha"][q])), _bits(want)), k
            _check_patch_stats(got, q, patches[q])
        flags = _np(got["degenerate"])
        assert not flags[:len(cases)].any()
        if sigma == 10:
            q = len(cases)
            plain = patches[-1][3:40, 5:64]
            assert flags[q] and not flags[q + 1]
            assert np.array_equal(_np(got["blended"][q]), O.blend_host(np.zeros(plain.shape[:2], np.float32), plain))
            assert not _np(got["alpha"][q]).any()
            _check_patch_stats(got, q, plain)
            assert tuple(got["blended"][q + 1].shape) == (11, 0, 3) and int(got["lum_sum"][q + 1]) == 0 and not bool(got["verdict"][q + 1])


def test_blend_stored_variant_and_verdicts_vs_the_reference(engine, fx):
    """`apply_alpha_` from a stored T, and `filter_patch`'s sums and verdicts on the fixture's patches (a zero T leaves them plain
    enough: only the luminance is looked at)"""
    cases = list(G.STORED_CASES)
    patches = [fx[f"stored_{k}_patch"] for k in cases] + [fx[f"patch_{k}_rgb"] for k in G.PATCH_CASES]
    Ts = [fx[f"stored_{k}_T"][..., 0].astype(np.float32) for k in cases] + [np.zeros(fx[f"patch_{k}_rgb"].shape[:2], np.float32) for k in G.PATCH_CASES]
    got = engine.overlay_rows(_dev(engine, patches), _dev(engine, Ts), _rows([(0, 0) + t.shape for t in Ts]), "stored")
    for q, k in enumerate(cases):
        assert np.array_equal(_np(got["blended"][q]), fx[f"stored_{k}_out"]), k
    for q, k in enumerate(G.PATCH_CASES, start=len(cases)):
        assert int(got["lum_sum"][q]) == int(fx[f"patch_{k}_lum_sum"]) and bool(got["verdict"][q]) == bool(fx[f"patch_{k}_verdict"]), k
    assert got["alpha"] is None


def test_blend_refusals(engine, fx):
    """a box outside the image, a map that overhangs the image, a null pointer: 1 without a launch; the same table then runs"""
    img = torch.from_numpy(fx["image_inner_img"]).to(engine.device)
    H, W = img.shape[:2]
    m = torch.zeros(H, W, device=engine.device)
    tab = np.zeros(1, O.OVERLAY_ROW_DTYPE)
    tab["img_h"], tab["img_w"], tab["map_h"], tab["map_w"] = H, W, H, W
    tab["x_end"], tab["y_end"], tab["map_index"] = 8, 8, -1
    out = torch.empty(8 * 8 * 3, dtype=torch.uint8, device=engine.device)
    keep = torch.empty_like(out)
    lum = torch.empty(1, dtype=torch.int64, device=engine.device)
    flag = torch.empty(2, dtype=torch.int32, device=engine.device)
    p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def call(t, images=img, map_elements=m.numel()):
        t_d = torch.from_numpy(t.view(np.uint8)).to(engine.device)
        return engine.lib.dm_overlay_blend(None if images is None else p(images), img.numel(), p(m), map_elements, None, 0, p(t_d), 1, p(out),
                                           p(keep), out.numel(), None, 0, p(lum), p(flag[:1]), p(flag[1:]), engine._stream())
    for field, v in (("x_end", H + 1), ("y_end", W + 1), ("x_start", -1), ("y_start", 9), ("map_h", H + 1), ("map_x0", 1), ("map_y0", 2),
                     ("variant", 3), ("map_index", 0), ("img_h", H + 1), ("out_offset", 1), ("image_offset", -1), ("map_offset", 1)):
        bad = tab.copy()
        bad[field] = v
        assert call(bad) == 1, field
    assert call(tab, images=None) == 1 and call(tab, map_elements=m.numel() - 1) == 1
    assert call(tab) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(out.view(8, 8, 3)), O.blend_host(np.zeros((8, 8), np.float64), fx["image_inner_img"][:8, :8]))


@pytest.mark.parametrize("variant", ["image", "crop"])
def test_overlay_patches_end_to_end(engine, variant):
    """three synthetic grids of different latent sizes, five rows each (rows of one image share its map; two of them share a box
    corner): byte-equal to the restatement chain on the host fed with the device's own normalised maps, and to a second run"""
    rng = np.random.default_rng(31)
    latents, sizes = [(8, 8), (6, 9), (5, 7)], [(64, 64), (48, 72), (40, 56)]
    grids = [(1.0 + 0.3 * rng.standard_normal((2, 2, 4, h, w))).astype(np.float16) for h, w in latents]
    images = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    boxes, image = [], []
    for b, (H, W) in enumerate(sizes):
        for q in range(5):
            x0, y0 = int(rng.integers(0, H - 24)), int(rng.integers(0, W - 24))
            boxes.append((x0, y0, x0 + 24, y0 + 24) if q else (0, 0, 24, 24))
            image.append(b)
    rows = _rows(boxes, image)
    sc = TypicalityScorer(engine)
    got = sc.overlay_patches(grids, _dev(engine, images), sizes, rows, variant=variant, sigma=10, images_per_call=2, want_alpha=True)
    maps = [_np(m) for m in got["maps"]]
    assert [m.shape for m in maps] == sizes
    want = O.overlay_rows(images, maps, rows, variant, 10, want_alpha=True)
    again = sc.overlay_patches(grids, _dev(engine, images), sizes, rows, variant=variant, sigma=10, want_alpha=True)
    for q in range(len(boxes)):
        for key in ("blended", "plain"):
            assert np.array_equal(_np(got[key][q]), want[key][q]), (key, q)
            assert torch.equal(got[key][q], again[key][q]), (key, q)
        assert np.array_equal(_bits(_np(got["alpha"][q])), _bits(want["alpha"][q])), q
    for key in ("lum_sum", "verdict", "degenerate"):
        assert np.array_equal(_np(got[key]), want[key]) and torch.equal(got[key], again[key]), key
    host = sc.overlay_patches(grids, images, sizes, rows, variant=variant, sigma=10)          # numpy images: the restatements
    assert all(np.array_equal(a, b) for a, b in zip(host["blended"], want["blended"]))


# -- guard bands: every device operand of a call inside one allocation between guards (tests/gpu_util.Guarded, through run3 of
# -- tests/test_gpu_guards.py: guards and inputs untouched, results equal to the plain run under 0xFF and 0x00 fills)
U8, F32, F64, I32, I64 = torch.uint8, torch.float32, torch.float64, torch.int32, torch.int64


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("post_op", ["clamp", "unit"])
def test_filter_guarded(engine, post_op):
    """dm_gaussian_filter_maps at sigma 10 on the 23 x 130 map (the halo wraps), the one-tile-and-one map and the 1 x 57 map"""
    from tests.test_gpu_guards import run3
    picks = [_filter_inputs()[i] for i in (2, 5, 1)]
    sigma = 10
    w, r = O.gauss_weights(sigma)
    desc = np.zeros(len(picks), O.GAUSS_DESC_DTYPE)
    desc["H"], desc["W"] = [a.shape[0] for a in picks], [a.shape[1] for a in picks]
    sizes = np.array([a.size for a in picks])
    desc["map_offset"] = desc["out_offset"] = desc["work_offset"] = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    need = O.workspace_bytes(len(picks), total, int(desc["H"].max()), int(desc["W"].max()))
    inputs = {"maps": torch.from_numpy(np.concatenate([a.ravel() for a in picks])), "desc": torch.from_numpy(desc.view(np.uint8).copy()),
              "w": torch.from_numpy(w)}
    outputs = {"work": ((need,), U8), "out": ((total,), F32), "max": ((len(picks),), F32)}

    def launch(v):
        rc = engine.lib.dm_gaussian_filter_maps(_vp(v["maps"]), _vp(v["desc"]), len(picks), float(sigma), _vp(v["w"]), r, O.POST_OPS[post_op],
                                                _vp(v["work"]), need, _vp(v["out"]), _vp(v["max"]), engine._stream())
        assert rc == 0, rc
    work = ("work",) if post_op == "unit" else ("work", "max")             # the maxima are written by the 'unit' pass only
    out = run3(f"gaussian_filter {post_op}", inputs, outputs, launch, work=work)
    flat = _np(out["out"])
    for d, a in zip(desc, picks):
        want = O.post_op_host(O.gaussian_filter_host(a, sigma), post_op)[0]
        at = int(d["out_offset"])
        assert np.array_equal(_bits(flat[at:at + a.size]), _bits(want.ravel()))


def test_blend_guarded(engine, fx):
    """dm_overlay_blend with one row of every variant: the small map in its larger image with the box across the map's edge, an
    all-negative crop with its maximum, a stored T; the image rows end at the last byte of their images"""
    from tests.test_gpu_guards import run3
    k = "small_map"
    img0, box0 = fx[f"image_{k}_img"], tuple(int(v) for v in fx[f"image_{k}_box"])
    map0 = O.post_op_host(O.gaussian_filter_host(fx[f"image_{k}_alpha"], 10), "clamp")[0]
    img1 = fx["crop_negative_patch"]
    map1, max1, _ = O.post_op_host(O.gaussian_filter_host(fx["crop_negative_T"], 10), "unit")
    img2 = fx["stored_corner_patch"]
    map2 = fx["stored_corner_T"][..., 0].astype(np.float32)
    images, maps = [img0, img1, img2], [map0, map1, map2]
    boxes = [box0, (0, 0) + map1.shape, (0, 0) + map2.shape]
    tab = np.zeros(3, O.OVERLAY_ROW_DTYPE)
    tab["variant"], tab["map_index"] = [0, 1, 2], [-1, 0, -1]
    tab["image_offset"] = np.cumsum([0] + [i.size for i in images[:-1]])
    tab["map_offset"] = np.cumsum([0] + [m.size for m in maps[:-1]])
    tab["img_h"], tab["img_w"] = [i.shape[0] for i in images], [i.shape[1] for i in images]
    tab["map_h"], tab["map_w"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    for q, b in enumerate(boxes):
        tab[q]["x_start"], tab[q]["y_start"], tab[q]["x_end"], tab[q]["y_end"] = b
    px = np.array([(b[2] - b[0]) * (b[3] - b[1]) for b in boxes])
    tab["alpha_offset"] = np.cumsum(px) - px
    tab["out_offset"] = 3 * tab["alpha_offset"]
    n_px = int(px.sum())
    inputs = {"images": torch.from_numpy(np.concatenate([i.ravel() for i in images])), "maps": torch.from_numpy(np.concatenate([m.ravel() for m in maps])),
              "max": torch.from_numpy(np.array([max1], np.float32)), "rows": torch.from_numpy(tab.view(np.uint8).copy())}
    outputs = {"blended": ((3 * n_px,), U8), "plain": ((3 * n_px,), U8), "alpha": ((n_px,), F32), "lum": ((3,), I64), "verdict": ((3,), I32),
               "degenerate": ((3,), I32)}

    def launch(v):
        rc = engine.lib.dm_overlay_blend(_vp(v["images"]), v["images"].numel(), _vp(v["maps"]), v["maps"].numel(), _vp(v["max"]), 1, _vp(v["rows"]), 3,
                                         _vp(v["blended"]), _vp(v["plain"]), 3 * n_px, _vp(v["alpha"]), n_px, _vp(v["lum"]), _vp(v["verdict"]),
                                         _vp(v["degenerate"]), engine._stream())
        assert rc == 0, rc
    out = {k_: _np(t) for k_, t in run3("overlay_blend", inputs, outputs, launch).items()}
    want = [fx[f"image_{k}_out"], fx["crop_negative_out"], fx["stored_corner_out"]]
    for q, (b, w_) in enumerate(zip(boxes, want)):
        at = int(tab[q]["out_offset"])
        assert np.array_equal(out["blended"][at:at + w_.size], w_.ravel()), q
        plain = images[q][b[0]:b[2], b[1]:b[3]]
        assert np.array_equal(out["plain"][at:at + w_.size], plain.ravel())
        s, verdict = O.filter_patch_host(plain)
        assert int(out["lum"][q]) == s and bool(out["verdict"][q]) == verdict
    assert not out["degenerate"].any()
