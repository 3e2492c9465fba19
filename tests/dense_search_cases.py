"""The cases of the dense detector search (tests/test_dense_search.py, tests/test_gpu_dense_search*.py): generated from
`numpy.random.default_rng(seed)`, never stored.  The seed of each case is the one tests/make_golden_dense_search.py settled on (the
first at which every gap the tests rely on is wide enough) and is read from tests/golden/dense_search_ref.json.

    features   f = random**2 * (random < density), f[..., 0] += 1e-3 (no row is zero), L2-normalised per cell in fp64, fp32 -> fp16
    detectors  K distinct cells of the case + 0.05 |normal| on a `density` share of the channels, renormalised, cast the same way
    S4         S2's data and masks of fold (2, 3); detectors as after an SVM round: S2's * (+-1 per channel, -1 for three in five) * 3, not normalised;
               one feature row NaN, one image NaN entirely ("S4"); "S4clean" is the same without the NaN (what the reference ran on)
"""
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLDEN_DIR, "dense_search_ref.json")
NPZ = os.path.join(GOLDEN_DIR, "dense_search_ref.npz")

#            images per chunk, W, H, C, K, top_k, density, fold
SHAPES = {
    "S1": dict(chunks=(2, 1), W=9, H=7, C=2112, K=5, top_k=2, density=0.1, fold=None),
    "S2": dict(chunks=(3, 4), W=9, H=7, C=72, K=70, top_k=5, density=0.3, fold=(1, 3)),
    "S3": dict(chunks=(1, 1), W=57, H=57, C=2112, K=64, top_k=1, density=0.1, fold=None),
    "S4": dict(chunks=(3, 4), W=9, H=7, C=72, K=70, top_k=5, density=0.3, fold=(2, 3)),
}
SHAPES["S4clean"] = SHAPES["S4"]
ORDER = ("S1", "S2", "S3", "S4")
S4_NAN_ROW = (1, 17)             # (image, cell): one feature row of NaN
S4_NAN_IMAGE = 5                 # an image of NaN only
_BASE = {"S4": "S2", "S4clean": "S2"}


def seeds():
    with open(JSON) as f:
        return {k: v["seed"] for k, v in json.load(f)["cases"].items()}


def to_f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float16)


def _normalised(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def features(tag, seed):
    """fp16 [n_images, W, H, C]"""
    s = SHAPES[tag]
    rng = np.random.default_rng(seed)
    shape = (sum(s["chunks"]), s["W"], s["H"], s["C"])
    f = rng.random(shape) ** 2 * (rng.random(shape) < s["density"])
    f[..., 0] += 1e-3
    f = to_f16(_normalised(f))
    if tag == "S4":
        f[S4_NAN_ROW[0]].reshape(-1, s["C"])[S4_NAN_ROW[1]] = np.nan
        f[S4_NAN_IMAGE] = np.nan
    return f


def detectors(tag, seed):
    """fp16 [K, C]"""
    s = SHAPES[tag]
    if tag in _BASE:
        w = detectors(_BASE[tag], seed).astype(np.float64)
        sign = np.where(np.random.default_rng(seed + 2000).random(s["C"]) < 0.6, -1.0, 1.0)
        return to_f16(w * sign[None, :] * 3)
    f = features(tag, seed).reshape(-1, s["C"]).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    rows = rng.choice(len(f), size=s["K"], replace=False)
    w = f[rows] + 0.05 * np.abs(rng.normal(size=(s["K"], s["C"]))) * (rng.random((s["K"], s["C"])) < s["density"])
    return to_f16(_normalised(w))


def masks(tag):
    """per chunk uint8 [B, W H] (1 = the cell takes part) or None: `fold_mask(chunk index, ...)` drawn on the CPU — a chunk is one shard"""
    from diff_mining_amd.doersch import fold_mask
    s = SHAPES[tag]
    if s["fold"] is None:
        return [None] * len(s["chunks"])
    return [fold_mask(j, B, s["W"] * s["H"], s["fold"], "cpu").numpy() for j, B in enumerate(s["chunks"])]


def paths(tag):
    return [f"img{n:03d}.jpg" for n in range(sum(SHAPES[tag]["chunks"]))]


def chunks(tag, seed):
    """[(paths, data fp16 [B, W, H, C], mask or None), ...]"""
    s, f, p, m = SHAPES[tag], features(tag, seed), paths(tag), masks(tag)
    out, at = [], 0
    for j, B in enumerate(s["chunks"]):
        out.append((p[at:at + B], np.ascontiguousarray(f[at:at + B]), m[j]))
        at += B
    return out
