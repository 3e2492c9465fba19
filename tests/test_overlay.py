"""Typicality overlays, CPU tier: the numpy restatements that the GPU tests compare the kernels with are pinned here, without a
tolerance, to scipy.ndimage.gaussian_filter, to PIL's 'L' conversion and to the reference's own three blend functions
(tests/golden/overlay_ref.npz, written by tests/make_golden_overlay.py); the refusals and the `degenerate` rule; the host side of
the new entry points without a device."""
import os

import numpy as np
import pytest

from diff_mining_amd import engine as E
from diff_mining_amd import overlay as O
from tests import make_golden_overlay as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(G.PATH)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("sigma", [0.4, 2, 10])
@pytest.mark.parametrize("shape", [(1, 1), (1, 57), (23, 130), (64, 64), (65, 63), (256, 341)], ids=lambda s: "x".join(map(str, s)))
def test_gaussian_filter_host_is_scipy_bit_for_bit(shape, sigma):
    """fp64 accumulation per 1-D pass, one rounding to fp32 per axis, `reflect` as often as the halo wraps (23 rows and 1 row are
    narrower than the radius of 40 at sigma 10); sigma 0.4 has radius 2"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    a = rng.standard_normal(shape).astype(np.float32)
    assert np.array_equal(_bits(O.gaussian_filter_host(a, sigma)), _bits(gaussian_filter(a, sigma=sigma)))


def test_gauss_weights_are_scipys():
    from scipy.ndimage import _filters
    for sigma in (0.4, 2, 10, 3.3):
        w, r = O.gauss_weights(sigma)
        assert r == int(4.0 * sigma + 0.5) and w.dtype == np.float64
        assert np.array_equal(_bits(w), _bits(_filters._gaussian_kernel1d(sigma, 0, r)))


def test_fixture_holds_what_its_script_says():
    assert G.check() == len(G.manifest()) == 63


def test_gaussian_filter_host_vs_fixture(fx):
    for k in G.GAUSS_CASES:
        got = O.gaussian_filter_host(fx[f"gauss_{k}_in"], float(fx[f"gauss_{k}_sigma"]))
        assert np.array_equal(_bits(got), _bits(fx[f"gauss_{k}_out"])), k


@pytest.mark.parametrize("case", list(G.IMAGE_CASES))
def test_alpha_bbox_host_vs_the_reference(fx, case):
    """`load_and_apply_alpha_bbox`: the uint8 crop byte for byte and the float64 alpha crop bit for bit (negative filtered values are
    -0.0 there, as `T*(T>0)` leaves them)"""
    u8, alpha = O.alpha_bbox_host(fx[f"image_{case}_alpha"], fx[f"image_{case}_img"], fx[f"image_{case}_box"])
    assert u8.dtype == np.uint8 and np.array_equal(u8, fx[f"image_{case}_out"])
    assert alpha.dtype == np.float64 and np.array_equal(_bits(alpha), _bits(fx[f"image_{case}_alpha_crop"]))


@pytest.mark.parametrize("case", list(G.CROP_CASES))
def test_apply_alpha_host_vs_the_reference(fx, case):
    """`apply_alpha`: `1 - T` in fp32; the all-negative crops divide by a negative maximum, so T >= 1 there"""
    u8, degenerate = O.apply_alpha_host(fx[f"crop_{case}_T"], fx[f"crop_{case}_patch"], float(fx[f"crop_{case}_sigma"]))
    assert not degenerate and np.array_equal(u8, fx[f"crop_{case}_out"])
    if case.startswith("negative"):
        assert O.gaussian_filter_host(fx[f"crop_{case}_T"], float(fx[f"crop_{case}_sigma"])).max() < 0


@pytest.mark.parametrize("case", list(G.STORED_CASES))
def test_blend_host_vs_the_reference(fx, case):
    T = fx[f"stored_{case}_T"]
    assert np.array_equal(O.blend_host(T, fx[f"stored_{case}_patch"]), fx[f"stored_{case}_out"])
    # the 2-D form the device takes: the fp32 value, widened again
    T32 = T[..., 0].astype(np.float32)
    assert np.array_equal(T32.astype(np.float64), T[..., 0]) and np.array_equal(T[..., 0], T[..., 2])
    assert np.array_equal(O.blend_host(T32.astype(np.float64), fx[f"stored_{case}_patch"]), fx[f"stored_{case}_out"])


def test_dtype_flows_differ():
    """the fixture can tell the variants apart: `1 - T` in fp32 and in float64 give different bytes somewhere"""
    rng = np.random.default_rng(5)
    T = rng.random((64, 64)).astype(np.float32)
    patch = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    assert not np.array_equal(O.blend_host(T, patch), O.blend_host(T.astype(np.float64), patch))


def test_filter_patch_host_vs_the_reference_and_pil(fx):
    from PIL import Image
    for k in G.PATCH_CASES:
        s, verdict = O.filter_patch_host(fx[f"patch_{k}_rgb"])
        assert s == int(fx[f"patch_{k}_lum_sum"]) and verdict == bool(fx[f"patch_{k}_verdict"]), k
    rng = np.random.default_rng(11)
    for shape in ((17, 23), (64, 64), (1, 1), (3, 200)):
        p = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
        for c in (3, 4):                                                  # RGB and RGBA
            L = np.array(Image.fromarray(np.ascontiguousarray(p[..., :c])).convert("L"))
            s, verdict = O.filter_patch_host(p[..., :c])
            assert s == int(L.astype(np.int64).sum())
            assert verdict == bool(30 < np.mean(L) < 225)
    assert O.filter_patch_host(np.zeros((0, 5, 3), np.uint8)) == (0, False)


def test_degenerate_rule():
    """a maximum of exactly 0 after filtering: the reference divides by it; here the flag, and the pixels T = 0 gives"""
    patch = np.random.default_rng(3).integers(0, 256, (9, 12, 3)).astype(np.uint8)
    u8, degenerate = O.apply_alpha_host(np.zeros((9, 12), np.float32), patch, 10)
    assert degenerate
    assert np.array_equal(u8, O.blend_host(np.zeros((9, 12), np.float32), patch))
    assert np.array_equal(u8, ((0.05 * (patch / 255.0) + 0.95 * 1.0) * 255).astype(np.uint8))
    F, m, deg = O.post_op_host(np.full((4, 4), np.nan, np.float32), "unit")
    assert deg and np.isnan(m) and not F.any()
    F, m, deg = O.post_op_host(np.array([[-2.0, -1.0]], np.float32), "unit")
    assert not deg and m == -1 and np.array_equal(F, [[2.0, 1.0]])
    F, _, _ = O.post_op_host(np.array([[-2.0, 3.0]], np.float32), "clamp")
    assert np.array_equal(_bits(F), _bits(np.array([[-0.0, 3.0]], np.float32)))


def test_refusals():
    img = np.zeros((20, 30, 3), np.uint8)
    m = np.zeros((20, 30), np.float32)
    for bad in ((0, 0, 21, 30), (0, 0, 20, 31), (-1, 0, 5, 5), (6, 0, 5, 5), (0, 9, 5, 8)):
        with pytest.raises(ValueError, match="outside"):
            O.alpha_bbox_host(m, img, bad)
    for shape in ((21, 30), (20, 31)):                                    # the reference raises on a map larger than the image
        with pytest.raises(ValueError, match="overhangs"):
            O.alpha_bbox_host(np.zeros(shape, np.float32), img, (0, 0, 5, 5))
    for sigma in (0, -1, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            O.gaussian_filter_host(m, sigma)
    with pytest.raises(ValueError, match="radius"):
        O.gaussian_filter_host(m, 60)
    with pytest.raises(ValueError):
        O.gaussian_filter_host(np.zeros((0, 4), np.float32), 2)
    with pytest.raises(ValueError):
        O.apply_alpha_host(np.zeros((5, 5), np.float32), np.zeros((5, 6, 3), np.uint8))
    with pytest.raises(ValueError):
        O.blend_host(np.zeros((5, 5)), np.zeros((5, 6, 3), np.uint8))
    with pytest.raises(ValueError):
        O.overlay_rows([img], [m], {"image": [1], "x_start": [0], "y_start": [0], "x_end": [1], "y_end": [1]})
    with pytest.raises(ValueError, match="variant"):
        O.overlay_rows([img], [m], {"image": [0], "x_start": [0], "y_start": [0], "x_end": [1], "y_end": [1]}, variant="x")


def test_overlay_rows_on_numpy_takes_the_restatements(fx):
    """numpy inputs: the three variants through the public entry, a zero-area box among the rows"""
    k = "small_map"
    img, alpha, box = fx[f"image_{k}_img"], fx[f"image_{k}_alpha"], fx[f"image_{k}_box"]
    rows = {"image": [0, 0], "x_start": [box[0], 3], "y_start": [box[1], 4], "x_end": [box[2], 3], "y_end": [box[3], 9]}
    got = O.overlay_rows([img], [alpha], rows, "image", want_alpha=True)
    assert np.array_equal(got["blended"][0], fx[f"image_{k}_out"])
    assert np.array_equal(got["alpha"][0].astype(np.float64), fx[f"image_{k}_alpha_crop"][..., 0])
    assert got["blended"][1].shape == (0, 5, 3) and got["lum_sum"][1] == 0 and not got["verdict"][1]
    assert np.array_equal(got["plain"][0], img[box[0]:box[2], box[1]:box[3]])
    assert (got["lum_sum"][0], got["verdict"][0]) == O.filter_patch_host(got["plain"][0])
    T, patch = fx["crop_negative_T"], fx["crop_negative_patch"]
    bh, bw = T.shape
    got = O.overlay_rows([patch], [T], {"image": [0], "x_start": [0], "y_start": [0], "x_end": [bh], "y_end": [bw]}, "crop", sigma=10)
    assert np.array_equal(got["blended"][0], fx["crop_negative_out"]) and not got["degenerate"][0]
    T = fx["stored_corner_T"][..., 0].astype(np.float32)
    patch = fx["stored_corner_patch"]
    got = O.overlay_rows([patch], [T], {"image": [0], "x_start": [0], "y_start": [0], "x_end": [T.shape[0]], "y_end": [T.shape[1]]}, "stored")
    assert np.array_equal(got["blended"][0], fx["stored_corner_out"])


def test_abi_and_refusals_without_a_device():
    """the three symbols are exported with the table's signatures; the helper sizes the workspace; a bad argument is refused before
    anything touches a device; without a GPU the device path raises instead of falling back"""
    import torch
    lib = E.load_library()
    for s in ("dm_overlay_workspace_bytes", "dm_gaussian_filter_maps", "dm_overlay_blend"):
        assert s in E.SIGNATURES and hasattr(lib, s)
    # 3 maps of at most 100 x 70: 4 x 3 tiles each -> 36 floats of tile maxima (rounded up to 256 bytes), then the intermediate
    assert O.workspace_bytes(3, 1000, 100, 70) == 256 + 4000
    assert lib.dm_overlay_workspace_bytes(0, 10, 4, 4) == 0 and lib.dm_overlay_workspace_bytes(1, 0, 4, 4) == 0
    assert lib.dm_overlay_workspace_bytes(1, 10, 0, 4) == 0 and lib.dm_overlay_workspace_bytes(1, 10, 4, (1 << 24) + 1) == 0
    one = E.C.c_void_p(256)                                                # never dereferenced: every call below is refused first
    assert lib.dm_gaussian_filter_maps(None, one, 1, 10.0, one, 40, 0, one, 4096, one, None, None) == 1
    assert lib.dm_gaussian_filter_maps(one, one, 1, 0.0, one, 0, 0, one, 4096, one, None, None) == 1          # sigma <= 0
    assert lib.dm_gaussian_filter_maps(one, one, 1, -2.0, one, 8, 0, one, 4096, one, None, None) == 1
    assert lib.dm_gaussian_filter_maps(one, one, 1, float("nan"), one, 8, 0, one, 4096, one, None, None) == 1
    assert lib.dm_gaussian_filter_maps(one, one, 1, 10.0, one, 39, 0, one, 4096, one, None, None) == 1         # not sigma's radius
    assert lib.dm_gaussian_filter_maps(one, one, 1, 60.0, one, 240, 0, one, 4096, one, None, None) == 1        # past the LDS tile
    assert lib.dm_gaussian_filter_maps(one, one, 1, 10.0, one, 40, 3, one, 4096, one, None, None) == 1         # unknown post-op
    assert lib.dm_gaussian_filter_maps(one, one, 0, 10.0, one, 40, 0, one, 4096, one, None, None) == 1
    assert lib.dm_overlay_blend(None, 1, one, 1, None, 0, one, 1, one, one, 1, None, 0, one, one, one, None) == 1
    assert lib.dm_overlay_blend(one, 1, one, 1, None, 0, one, 0, one, one, 1, None, 0, one, one, one, None) == 1
    assert lib.dm_overlay_blend(one, 1, one, 1, None, 0, one, 1, one, one, 1, None, 0, None, one, one, None) == 1
    assert O.GAUSS_DESC_DTYPE.itemsize == 32 and O.OVERLAY_ROW_DTYPE.itemsize == 80
    assert callable(E.UNetEngine.gaussian_filter) and callable(E.UNetEngine.overlay_rows)
    from diff_mining_amd.typicality import TypicalityScorer
    assert callable(TypicalityScorer.overlay_patches)
    with pytest.raises(E.EngineError):                                    # torch tensors that are not on a GPU: no quiet host path
        O.gaussian_filter([torch.zeros(4, 4)], 2)
    with pytest.raises(E.EngineError):
        O.overlay_rows([torch.zeros(4, 4, 3, dtype=torch.uint8)], [torch.zeros(4, 4)],
                       {"image": [0], "x_start": [0], "y_start": [0], "x_end": [2], "y_end": [2]})


def test_build_lists_the_new_translation_unit():
    import importlib
    b = importlib.import_module("diff_mining_amd.build")
    assert "overlay.hip" in b.SOURCES and os.path.exists(os.path.join(b.CSRC, "overlay.hip"))
    assert "-ffp-contract=off" in b.FLAGS
