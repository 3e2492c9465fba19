"""The CLIP-mining cases of tests/golden/clipmine_ref.npz (tests/make_golden_clipmine.py), shared by the CPU and the GPU tests."""
import functools
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "clipmine_ref.npz")
# grid / E / size / window / k / mode
CASES = ("g45_diff",          # 4 x 5 / 48 / (40, 52) / 8 x 8 / 3 / diff: gh != pw, scale 10.4, an E tail
         "g45_sim",           # the same in sim
         "g54_rect",          # 5 x 4 / 40 / (37, 45) / 8 x 6 / 5: kx != ky
         "g33_small",         # 3 x 3 / 32 / (24, 24) / 8 x 8 / 2
         "all_eligible",      # 3 x 3 / 32 / (16, 16) / 8 x 8 / 2: n = OH OW = 81
         "run_out",           # 3 x 3 / 32 / (48, 48) / 8 x 8 / 2, one dominant token: the reference returns 1 box
         "real")              # 24 x 24 / 64 / (512, 512) / 64 x 64 / 5
MODE_NAMES = ("diff", "sim")
TOL_FACTOR = 4.0              # D and features: within 4 x the reference's own recorded distance from the float64 restatement


@functools.lru_cache(maxsize=None)
def _file():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def case(tag):
    f = _file()
    gh, pw, H, W, kx, ky, k, mode, _ = (int(v) for v in f[f"{tag}_args"])
    return SimpleNamespace(tag=tag, tokens=f[f"{tag}_tokens"], text=f[f"{tag}_text"], gh=gh, pw=pw, size=(H, W), kx=kx, ky=ky, k=k,
                           mode=MODE_NAMES[mode], boxes=f[f"{tag}_boxes"], D=f[f"{tag}_D"], feats=f[f"{tag}_feats"],
                           leads=f[f"{tag}_leads"], max_abs_D=float(f[f"{tag}_max_abs_D"]),
                           D_err=float(f[f"{tag}_restatement_D_err"]), feat_err=float(f[f"{tag}_restatement_feat_err"]))


def kwargs(c):
    return dict(pw=c.pw, k_per_image=c.k, kx=c.kx, ky=c.ky, mode=c.mode)


def check_against_reference(c, boxes, D, feats, what=""):
    """boxes [rows, 4], D [rows], feats [rows, E] of one image against the fixture: boxes, order and count equal; D within
    TOL_FACTOR x restatement_D_err of max|D|; every feature row within TOL_FACTOR x restatement_feat_err in rel-L2.  Prints the
    figures before it asserts."""
    boxes, D, feats = np.asarray(boxes), np.asarray(D, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    assert boxes.shape == c.boxes.shape and np.array_equal(boxes, c.boxes), (what, c.tag, boxes.tolist(), c.boxes.tolist())
    d_err = float(np.abs(D - c.D.astype(np.float64)).max() / c.max_abs_D)
    ref = c.feats.astype(np.float64)
    f_err = float((np.linalg.norm(feats - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())
    print(f"{what} {c.tag}: count {len(boxes)}/{c.k} D err {d_err:.3g} (bound {TOL_FACTOR * c.D_err:.3g}) "
          f"feature err {f_err:.3g} (bound {TOL_FACTOR * c.feat_err:.3g})")
    assert d_err <= TOL_FACTOR * c.D_err, (what, c.tag, d_err, c.D_err)
    assert f_err <= TOL_FACTOR * c.feat_err, (what, c.tag, f_err, c.feat_err)
    return d_err, f_err
