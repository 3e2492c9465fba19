#!/usr/bin/env python
"""Golden vectors for the typicality overlays, produced by the reference's own code run where the reference is at hand.

Like tests/make_golden_consumers.py this script parses the reference's modules with `ast`, compiles exactly the function definitions
it needs - the reference's text, unmodified, never written anywhere - and calls them with seeded synthetic inputs:

    Cluster.load_and_apply_alpha_bbox   diffmining/typicality/cluster.py:93-110
    apply_alpha                         diffmining/typicality/utils.py:165-214
    filter_patch                        diffmining/typicality/utils.py:104-109
    Cluster.apply_alpha_                diffmining/applications/parallel-dataset/cluster.py:132-141

and scipy.ndimage.gaussian_filter itself.  What the functions load from disk is given instead: `load_typicality_norm` returns the
case's map, `load_image` its image, `joblib.load` its stored T, `PIL.Image.open` its patch.  Only inputs and outputs are stored:
tests/golden/overlay_ref.npz.  The cases (CASES below): a map narrower than the filter's radius in one axis, a map smaller than its
image, a box that touches two image borders, a box that is the whole image, sigma 10 and sigma 2, and an `apply_alpha` crop whose
filtered values are all negative (the division by the maximum flips their sign).

    python tests/make_golden_overlay.py            # writes the fixture (needs the reference)
    python tests/make_golden_overlay.py --check    # the committed fixture has the keys, shapes and dtypes CASES implies
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "overlay_ref.npz")

# variant 'image': (image H, W), (map h, w), box (x_start, y_start, x_end, y_end) with x = rows; sigma is the reference's 10
IMAGE_CASES = {
    "inner": ((96, 130), (96, 130), (20, 31, 84, 95)),
    "small_map": ((70, 90), (64, 80), (30, 40, 70, 88)),              # the map is smaller than its image; the box straddles its edge
    "corner": ((96, 130), (96, 130), (56, 80, 96, 130)),              # the box touches two image borders
    "whole_narrow": ((23, 130), (23, 130), (0, 0, 23, 130)),          # the box is the whole image; 23 rows < the radius of 40
}
# variant 'crop': (bh, bw), sigma, the range the crop's values are drawn from
CROP_CASES = {
    "s10": ((64, 64), 10, (-1.0, 1.0)),
    "s2": ((37, 50), 2, (-1.0, 1.0)),
    "negative": ((23, 60), 10, (-0.9, -0.2)),                         # all negative after filtering; 23 rows < the radius
    "negative_s2": ((33, 31), 2, (-0.9, -0.2)),
}
# variant 'stored': the alpha crop of an 'image' case as `a[bbox]` stores it (float64 [bh, bw, 3]), with that case's plain crop
STORED_CASES = {"inner": "inner", "corner": "corner"}
# filter_patch: (h, w, channel range)
PATCH_CASES = {"mid": (64, 64, (0, 256)), "dark": (17, 23, (0, 40)), "bright": (31, 9, (215, 256)), "edge": (8, 8, (28, 33))}
# scipy's gaussian_filter alone: (H, W), sigma
GAUSS_CASES = {"narrow": ((23, 130), 10), "s2": ((50, 50), 2), "tiny": ((1, 57), 0.4)}


def manifest():
    """key -> (shape, dtype name) of everything the fixture holds"""
    m = {}
    for k, ((H, W), (h, w), b) in IMAGE_CASES.items():
        bh, bw = b[2] - b[0], b[3] - b[1]
        m.update({f"image_{k}_alpha": ((h, w), "float32"), f"image_{k}_img": ((H, W, 3), "uint8"), f"image_{k}_box": ((4,), "int64"),
                  f"image_{k}_out": ((bh, bw, 3), "uint8"), f"image_{k}_alpha_crop": ((bh, bw, 3), "float64")})
    for k, ((bh, bw), _, _) in CROP_CASES.items():
        m.update({f"crop_{k}_T": ((bh, bw), "float32"), f"crop_{k}_patch": ((bh, bw, 3), "uint8"), f"crop_{k}_sigma": ((), "float64"),
                  f"crop_{k}_out": ((bh, bw, 3), "uint8")})
    for k, src in STORED_CASES.items():
        b = IMAGE_CASES[src][2]
        bh, bw = b[2] - b[0], b[3] - b[1]
        m.update({f"stored_{k}_T": ((bh, bw, 3), "float64"), f"stored_{k}_patch": ((bh, bw, 3), "uint8"),
                  f"stored_{k}_out": ((bh, bw, 3), "uint8")})
    for k, (h, w, _) in PATCH_CASES.items():
        m.update({f"patch_{k}_rgb": ((h, w, 3), "uint8"), f"patch_{k}_lum_sum": ((), "int64"), f"patch_{k}_verdict": ((), "bool")})
    for k, ((H, W), _) in GAUSS_CASES.items():
        m.update({f"gauss_{k}_in": ((H, W), "float32"), f"gauss_{k}_sigma": ((), "float64"), f"gauss_{k}_out": ((H, W), "float32")})
    return m


def check():
    f = np.load(PATH)
    want = manifest()
    assert set(f.files) == set(want), sorted(set(f.files) ^ set(want))
    for k, (shape, dt) in want.items():
        assert f[k].shape == tuple(shape) and f[k].dtype == np.dtype(dt), (k, f[k].shape, f[k].dtype, shape, dt)
    return len(want)


def _image(rng, H, W):
    """a uint8 picture with structure: a smooth ramp plus noise, some pixels exactly 0 and 255"""
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(y / 9.0)[..., None] * np.cos(x / 13.0)[..., None] + rng.normal(0, 30, (H, W, 3))
    img = np.clip(base, 0, 255).astype(np.uint8)
    img[rng.random((H, W)) < 0.02] = 0
    img[rng.random((H, W)) < 0.02] = 255
    return img


def main():
    sys.path.insert(0, HERE)
    from make_golden_consumers import REF, ref_function
    if not os.path.isdir(REF):
        sys.exit("needs the reference")
    import PIL.Image
    from scipy.ndimage import gaussian_filter
    CL, UT = "diffmining/typicality/cluster.py", "diffmining/typicality/utils.py"
    PD = "diffmining/applications/parallel-dataset/cluster.py"
    rng = np.random.default_rng(20261021)
    out = {}

    # -- load_and_apply_alpha_bbox: `self` supplies what it loads
    bbox_fn = ref_function(CL, ("Cluster", "load_and_apply_alpha_bbox"), {"np": np, "PIL": PIL, "gaussian_filter": gaussian_filter})
    for k, ((H, W), (h, w), box) in IMAGE_CASES.items():
        alpha = rng.random((h, w)).astype(np.float32)                     # `normalize` leaves [0, 1]
        alpha[rng.random((h, w)) < 0.3] = 0.0
        img = _image(rng, H, W)
        me = types.SimpleNamespace(D={"c": None}, decompose_save_path=lambda idd, e, country: (box, country, "x.jpg"),
                                   load_typicality_norm=lambda d, path: alpha.copy(),
                                   load_image=lambda path, pil=True: np.array(PIL.Image.fromarray(img)) / 255.0)
        pil, alpha_crop = bbox_fn(me, "c", None, "id", None)
        out[f"image_{k}_alpha"], out[f"image_{k}_img"], out[f"image_{k}_box"] = alpha, img, np.array(box, dtype=np.int64)
        out[f"image_{k}_out"], out[f"image_{k}_alpha_crop"] = np.array(pil), np.array(alpha_crop)

    # -- apply_alpha / apply_alpha_: joblib and PIL.Image.open are given
    def loaders(T, patch):
        return {"np": np, "os": os, "join": os.path.join, "gaussian_filter": gaussian_filter,
                "joblib": types.SimpleNamespace(load=lambda p: T.copy()),
                "PIL": types.SimpleNamespace(Image=types.SimpleNamespace(open=lambda p: PIL.Image.fromarray(patch),
                                                                         fromarray=PIL.Image.fromarray))}
    for k, ((bh, bw), sigma, (lo, hi)) in CROP_CASES.items():
        T = rng.uniform(lo, hi, (bh, bw)).astype(np.float32)
        patch = _image(rng, bh, bw)
        fn = ref_function(UT, ("apply_alpha",), loaders(T, patch))
        with np.errstate(all="ignore"):
            pil = fn("cars/x_1-2-3-4.png", sigma=sigma)
        out[f"crop_{k}_T"], out[f"crop_{k}_patch"], out[f"crop_{k}_sigma"] = T, patch, np.float64(sigma)
        out[f"crop_{k}_out"] = np.array(pil)
    for k, src in STORED_CASES.items():
        b = IMAGE_CASES[src][2]
        T = out[f"image_{src}_alpha_crop"]
        patch = np.ascontiguousarray(out[f"image_{src}_img"][b[0]:b[2], b[1]:b[3]])
        fn = ref_function(PD, ("Cluster", "apply_alpha_"), loaders(T, patch))
        out[f"stored_{k}_T"], out[f"stored_{k}_patch"] = T, patch
        out[f"stored_{k}_out"] = np.array(fn(None, "x/y.png"))

    # -- filter_patch, and the 'L' values it averages
    filter_patch = ref_function(UT, ("filter_patch",), {"np": np})
    for k, (h, w, (lo, hi)) in PATCH_CASES.items():
        rgb = rng.integers(lo, hi, (h, w, 3)).astype(np.uint8)
        pil = PIL.Image.fromarray(rgb)
        out[f"patch_{k}_rgb"] = rgb
        out[f"patch_{k}_lum_sum"] = np.int64(np.array(pil.convert("L")).astype(np.int64).sum())
        out[f"patch_{k}_verdict"] = np.bool_(filter_patch(pil))

    for k, ((H, W), sigma) in GAUSS_CASES.items():
        a = rng.standard_normal((H, W)).astype(np.float32)
        out[f"gauss_{k}_in"], out[f"gauss_{k}_sigma"], out[f"gauss_{k}_out"] = a, np.float64(sigma), gaussian_filter(a, sigma=sigma)

    np.savez_compressed(PATH, **out)
    print("wrote", PATH, check(), "arrays,", os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    if "--check" in sys.argv:
        print("ok:", check(), "arrays")
    else:
        main()
