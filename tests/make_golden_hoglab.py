#!/usr/bin/env python
"""Golden vectors that pin `hoglab_host` to scikit-image (needs scikit-image and the reference checkout that
tests/make_golden_consumers.py reads; neither is needed by any test).

    get_hoglab_single, normalize      doersch/hog.py:24-45, :81-87

The reference's two functions, compiled from its text with `ast` (never written anywhere), run on PNG files this script writes to a
temporary directory from the first image of the cases tests/hoglab_cases.GOLDEN_CASES (72 x 88 and 67 x 93).  Only results are
stored, in tests/golden/hoglab_skimage.npz:

    <case>_image   uint8 [H, W, 3]          the pixels the PNG held (the test checks them against its own generator)
    <case>_raw     float64 [bc, br, 2112]   get_hoglab_single(path)
    <case>_norm    float64 [bc, br, 2112]   normalize(get_hoglab_single(path))
    skimage        the version string

    python tests/make_golden_hoglab.py            # writes the file
    python tests/make_golden_hoglab.py --check    # validates keys / shapes / dtypes of an existing file; needs no scikit-image
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests import hoglab_cases as HC  # noqa: E402

NPZ = os.path.join(HERE, "golden", "hoglab_skimage.npz")
HOG = "doersch/hog.py"


def expected_layout():
    """key -> (shape, dtype)"""
    out = {}
    for tag in HC.GOLDEN_CASES:
        H, W, _ = HC.SHAPES[tag]
        shape = (W // 8 - 7, H // 8 - 7, 2112)
        out[f"{tag}_image"] = ((H, W, 3), np.uint8)
        out[f"{tag}_raw"] = (shape, np.float64)
        out[f"{tag}_norm"] = (shape, np.float64)
    return out


def check(path=NPZ):
    """-> list of complaints about the file (empty = fine)"""
    if not os.path.exists(path):
        return [f"{path} is absent"]
    bad = []
    with np.load(path) as z:
        for key, (shape, dtype) in expected_layout().items():
            if key not in z.files:
                bad.append(f"{key}: missing")
            elif z[key].shape != shape or z[key].dtype != dtype:
                bad.append(f"{key}: {z[key].dtype} {z[key].shape}, expected {np.dtype(dtype)} {shape}")
            elif key.endswith("_image") and not np.array_equal(z[key], HC.images(key[0])[0]):
                bad.append(f"{key}: not the image tests/hoglab_cases.py generates")
            elif not key.endswith("_image") and not np.isfinite(z[key]).all():
                bad.append(f"{key}: not finite")
        if "skimage" not in z.files:
            bad.append("skimage: missing")
    return bad


def main():
    if "--check" in sys.argv:
        bad = check()
        print("\n".join(bad) if bad else f"{NPZ}: ok")
        sys.exit(1 if bad else 0)
    import skimage
    import torch
    import torch.nn.functional as F
    from PIL import Image
    from skimage.color import rgb2lab
    from skimage.feature import hog
    from skimage.io import imread
    from tests.make_golden_consumers import REF, ref_function
    if not os.path.isdir(REF):
        sys.exit(f"needs {REF}")
    ns = {"np": np, "torch": torch, "F": F, "rgb2lab": rgb2lab, "hog": hog, "imread": imread}
    get_hoglab_single = ref_function(HOG, ("get_hoglab_single",), ns)
    normalize = ref_function(HOG, ("normalize",), ns)
    arrays = {"skimage": np.array(skimage.__version__)}
    with tempfile.TemporaryDirectory() as td:
        for tag in HC.GOLDEN_CASES:
            image = HC.images(tag)[0]
            path = os.path.join(td, f"{tag}.png")
            Image.fromarray(image).save(path)
            assert np.array_equal(imread(path), image)
            raw = np.asarray(get_hoglab_single(path), dtype=np.float64)
            arrays[f"{tag}_image"], arrays[f"{tag}_raw"], arrays[f"{tag}_norm"] = image, raw, normalize(raw.copy())
            print(f"{tag}: {image.shape} -> {raw.shape}")
    np.savez_compressed(NPZ, **arrays)
    bad = check()
    assert not bad, bad
    print(f"wrote {NPZ} ({os.path.getsize(NPZ)} bytes, scikit-image {skimage.__version__})")


if __name__ == "__main__":
    main()
