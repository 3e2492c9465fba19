"""CPU tier of the HOG-LAB features (diff-mining_amd/doersch.py: `hoglab_host`, the numpy restatement of the reference's
`get_hoglab_single` + `normalize` that the kernels of csrc/hoglab.hip are pinned to): the orientation-bin table of the C ABI, images
whose features can be worked out by hand, the reference's own Lab route, and every refusal of the two launch entries."""
import ctypes as C
import os

import numpy as np
import pytest

from diff_mining_amd import doersch as D
from tests import hoglab_cases as HC
from tests.make_golden_hoglab import NPZ, check

HOG = 1984


@pytest.fixture(scope="module")
def lib():
    return D._lib()


def test_bin_table_of_the_library_equals_the_numpy_statement(lib):
    want = D.hoglab_bin_table()
    got = np.full((511, 511), 77, dtype=np.uint8)
    assert lib.dm_hoglab_bin_table(got.ctypes.data_as(C.c_void_p)) == 0
    assert want.shape == (511, 511) and want.dtype == np.uint8 and np.array_equal(got, want)      # all 261 121 entries
    assert want.max() <= 30 and want.min() == 0
    assert not want[255].any()                                                       # g_row = 0: 0 or 180 degrees, bin 0
    assert want[255 + 1, 255 + 1] == 7 and want[255 + 1, 255] == 15                  # 45 and 90 degrees: 45 / 5.806 = 7.75, 90 / 5.806 = 15.5
    assert want[255 + 1, 255 - 1] == 23 == want[255 - 1, 255 + 1]                    # 135 degrees, and -45 % 180
    assert lib.dm_hoglab_bin_table(None) == 1


def test_uniform_images_have_no_hog_and_a_constant_lab():
    for colour in ((255, 255, 255), (255, 0, 0), (13, 200, 77)):
        im = np.empty((72, 88, 3), dtype=np.uint8)
        im[...] = colour
        x = D.hoglab_host(im, normalized=False)
        assert x.shape == (4, 2, 2112) and not x[..., :HOG].any()                   # exactly zero: 0 / sqrt(0 + eps^2)
        lab = x[..., HOG:].reshape(4, 2, 2, 64)
        assert (lab == lab[0, 0, :, :1]).all()                                       # one value per channel
        n = D.hoglab_host(im)
        assert np.isfinite(n).all() and np.allclose(np.linalg.norm(n, axis=-1), 1.0, atol=1e-15)
    white = np.full((64, 64, 3), 255, dtype=np.uint8)
    assert np.abs(D.hoglab_host(white, normalized=False)[..., HOG:] - 128 / 255).max() <= 1e-4      # a = b = 0
    red = np.zeros((64, 64, 3), dtype=np.uint8)
    red[..., 0] = 255
    _, lab = D.hoglab_cells_host(red)
    assert np.abs(lab[0] - 80.1).max() <= 0.1 and np.abs(lab[1] - 67.2).max() <= 0.1               # the published Lab of sRGB red


def test_a_vertical_step_edge_lands_in_bin_zero_beside_the_edge():
    """columns 0 ... 23 hold 0, columns 24 ... hold 200 in every channel: g_row = 0 everywhere, g_col = 200 at columns 23 and 24 (the
    last column of cell column 2, the first of cell column 3), on all 8 rows of a cell: 8 * 200 / 64 = 25 in bin 0 (0 degrees)"""
    im = np.zeros((72, 88, 3), dtype=np.uint8)
    im[:, 24:] = 200
    hog, _ = D.hoglab_cells_host(im)
    want = np.zeros((9, 11, 31))
    want[:, 2:4, 0] = 25.0
    assert np.array_equal(hog, want)
    hog32, _ = D.hoglab_cells_host(im, np.float32)
    assert hog32.dtype == np.float32 and np.array_equal(hog32, want)


def test_a_grey_image_gives_the_hog_of_its_red_channel_alone():
    grey = np.repeat(HC.images("B")[0][..., :1], 3, axis=2)
    red = grey.copy()
    red[..., 1:] = 0
    a, b = D.hoglab_cells_host(grey), D.hoglab_cells_host(red)
    assert np.array_equal(a[0], b[0]) and a[0].any()                                # equal magnitudes: the lowest channel wins
    assert not np.array_equal(a[1], b[1])                                            # the colour is another


def test_shape_and_transposition():
    im = HC.images("B")[0]
    hog, lab = D.hoglab_cells_host(im)
    assert hog.shape == (9, 11, 31) and lab.shape == (2, 9, 11)
    x = D.hoglab_host(im, normalized=False)
    assert x.shape == (4, 2, 2112) and x.dtype == np.float64 and D.hoglab_shape(72, 88) == (4, 2)
    for q in range(4):                                                               # block column first
        for p in range(2):
            v = hog[p:p + 8, q:q + 8].reshape(-1)
            v = v / np.sqrt((v ** 2).sum() + 1e-10)
            v = np.minimum(v, 0.2)
            v = v / np.sqrt((v ** 2).sum() + 1e-10)
            assert np.abs(x[q, p, :HOG] - v).max() <= 1e-15
            assert np.array_equal(x[q, p, HOG:], ((lab[:, p:p + 8, q:q + 8] + 128) / 255).reshape(-1))
    n = D.hoglab_host(im)
    assert np.abs(n - x / np.linalg.norm(x, axis=-1, keepdims=True)).max() <= 1e-15
    assert D.hoglab(im[None]).dtype == np.float16 and D.hoglab(im[None], normalized=False).dtype == np.float32
    assert D.hoglab(im).shape == (1, 4, 2, 2112)


def test_a_ragged_image_equals_its_crop_except_at_the_crop_border():
    """67 x 93 against its 64 x 88 crop: the same 8 x 11 cells.  The crop makes row 63 and column 87 image borders, where g_row /
    g_col are 0; in the full image they take rows 62, 64 / columns 86, 88.  So only HOG cell row 7 and cell column 10 may differ."""
    full = HC.images("C")[1]                                                         # noise
    crop = np.ascontiguousarray(full[:64, :88])
    a, b = D.hoglab_cells_host(full), D.hoglab_cells_host(crop)
    assert a[0].shape == b[0].shape == (8, 11, 31)
    assert np.array_equal(a[1], b[1])                                                # Lab reads no neighbour
    assert np.array_equal(a[0][:7, :10], b[0][:7, :10])
    assert not np.array_equal(a[0][7, :10], b[0][7, :10]) and not np.array_equal(a[0][:7, 10], b[0][:7, 10])
    assert D.hoglab_host(full).shape == (4, 1, 2112)


def test_lab_cell_map_equals_the_reference_route_of_windows_and_two_tap_means():
    """step by step as the reference does it: every 64 x 64 window at stride 8 of the a / b planes, shrunk to 8 x 8 by bilinear
    interpolation with align_corners=False, which at scale 8 samples at 8 d + 3.5: weights 1/2, 1/2 on pixels 8 d + 3 and 8 d + 4"""
    im = HC.images("B")[0]
    planes = D._lab_ab(im, np.float64)                                               # (a, b) [72, 88]
    x = D.hoglab_host(im, normalized=False)
    worst = 0.0
    for p in range(2):
        for q in range(4):
            for ch in range(2):
                w = planes[ch][8 * p:8 * p + 64, 8 * q:8 * q + 64]
                rows = 0.5 * w[3::8] + 0.5 * w[4::8]                                 # [8, 64]
                small = 0.5 * rows[:, 3::8] + 0.5 * rows[:, 4::8]                    # [8, 8]
                got = x[q, p, HOG + 64 * ch:HOG + 64 * ch + 64].reshape(8, 8)
                worst = max(worst, float(np.abs(got - (small + 128.0) / 255.0).max()))
    assert worst <= 1e-15, worst


def test_refusals_come_back_without_a_launch(lib):
    """every DM_HOGLAB_E_* of the two launch entries (the pointers are never followed: each call is refused first)"""
    p, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 8)
    ok = lib.dm_hoglab_workspace_bytes(2, 64, 64)
    assert ok == 2 * (8 * 8 * 31 * 4 + 2 * 8 * 8 * 4) and lib.dm_hoglab_workspace_bytes(1, 512, 512) == 64 * 64 * 33 * 4
    for B, H, W in ((0, 64, 64), (1, 63, 64), (1, 64, 63), (1, D.HOGLAB_MAX_SIDE + 1, 64), (1, 32832, 32832)):
        assert lib.dm_hoglab_workspace_bytes(B, H, W) == 0
    assert lib.dm_hoglab_workspace_bytes(1, D.HOGLAB_MAX_SIDE, 64) > 0

    def cells(images=p, B=1, H=64, W=64, bins=p, hog=p, lab=p):
        return lib.dm_hoglab_cells(None, images, B, H, W, bins, hog, lab)

    def feats(images=p, B=1, H=64, W=64, bins=p, out=p, raw=p, work=p, nbytes=1 << 30):
        return lib.dm_hoglab_features(None, images, B, H, W, bins, out, raw, work, nbytes)

    for kw in ({"images": None}, {"bins": None}, {"hog": None}, {"lab": None}):
        assert cells(**kw) == 1, kw
    for kw in ({"images": None}, {"bins": None}, {"work": None}, {"out": None, "raw": None}):
        assert feats(**kw) == 1, kw
    for call in (cells, feats):
        assert call(B=0) == 2 and call(B=-3) == 2
        assert call(B=1 << 23, H=512, W=512) == 2                                    # 2^23 block rows x tiles, 2^33 cells: grid x block >= 2^32
        assert call(H=63) == 3 and call(W=56) == 3 and call(H=D.HOGLAB_MAX_SIDE + 1) == 3 and call(W=1 << 20) == 3
        assert call(H=32832, W=32832) == 4                                           # 4097^2 blocks > 2^24 - 1
        assert call(H=32824, W=32824) == 4                                           # 4096^2 = 2^24 blocks
    assert feats(H=32816, W=32816, nbytes=0) == 5                                    # 4095^2 blocks pass; no workspace does
    assert feats(nbytes=ok // 2 - 1) == 5 and feats(B=2, nbytes=ok - 1) == 5
    assert feats(out=odd) == 6 and feats(raw=odd) == 6 and feats(work=odd) == 6
    assert feats(out=odd, raw=None) == 6 and feats(out=None, raw=odd) == 6
    assert cells(hog=C.c_void_p((1 << 20) + 2)) == 6 and cells(lab=C.c_void_p((1 << 20) + 1)) == 6
    assert set(D.HOGLAB_ERRORS) == {1, 2, 3, 4, 5, 6, 7}


def test_python_entries_refuse_what_they_cannot_take():
    with pytest.raises(ValueError):
        D.hoglab_host(np.zeros((63, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        D.hoglab_host(np.zeros((64, 64, 4), dtype=np.uint8))                         # RGBA
    with pytest.raises(ValueError):
        D.hoglab_host(np.zeros((64, 64, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        D.hoglab_workspace_bytes(1, 32, 64)
    with pytest.raises(D.EngineError):
        D.hoglab_features([[1, 2, 3]])                                               # neither numpy nor a device tensor
    f = D.hoglab(HC.images("B")[:1])[0]
    assert D.detector_from_patch(f, (24, 8)).tobytes() == f[3, 1].tobytes()
    with pytest.raises(ValueError):
        D.detector_from_patch(f, (32, 0))


def test_search_from_image_files_on_the_host(tmp_path):
    """`dense_search_images(device_id="cpu")`: PNG files -> `read_images` -> `hoglab_host` -> the numpy search; a patch finds itself"""
    from PIL import Image
    imgs = HC.images("B")
    paths = []
    for j, im in enumerate(imgs):
        paths.append(str(tmp_path / f"{j}.png"))
        Image.fromarray(im).save(paths[-1])
    Image.fromarray(HC.images("A")[0]).save(str(tmp_path / "other.png"))
    groups = D.read_images(paths + [str(tmp_path / "other.png")])
    assert [g[0] for g in groups] == [[0, 1, 2], [3]] and np.array_equal(groups[0][1], imgs) and groups[1][1].shape == (1, 64, 64, 3)
    feats = D.hoglab(imgs)
    w = np.stack([D.detector_from_patch(feats[1], (16, 8)), D.detector_from_patch(feats[2], (0, 0))])
    got = D.dense_search_images(w, paths, top_k=2, batch=2, device_id="cpu", scores="f32")
    assert got[0][0][1:] == ((16, 8), paths[1]) and got[1][0][1:] == ((0, 0), paths[2])
    assert abs(float(got[0][0][0]) - 1.0) <= 2e-3 and len(got[0]) == 2              # fp16 unit vectors: |x|^2 = 1 within 2112 * 2^-11 * x^2
    want = D.dense_search_host(w, [(paths, feats)], top_k=2, scores="f32")
    assert [[e[1:] for e in k] for k in got] == [[e[1:] for e in k] for k in want]


def test_hoglab_host_matches_skimage_fixture():
    """`hoglab_host` against scikit-image's own numbers (tests/make_golden_hoglab.py), fp64 against fp64"""
    if not os.path.exists(NPZ):
        pytest.skip("tests/golden/hoglab_skimage.npz is not committed yet: HOG-LAB parity with skimage unpinned (README)")
    assert check() == []
    with np.load(NPZ) as z:
        for tag in HC.GOLDEN_CASES:
            im = z[f"{tag}_image"]
            for key, normalized in ((f"{tag}_raw", False), (f"{tag}_norm", True)):
                want, got = z[key], D.hoglab_host(im, normalized=normalized)
                assert got.shape == want.shape
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), key
