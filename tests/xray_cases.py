"""Inputs of the X-ray evaluation tests, regenerated from their seeds.  Shared by tests/make_golden_xray.py, which records each
map's sha256 and the reference's results in tests/golden/xray_ref.npz, and by the tests, which check the sha256.

`magnitudes` uses only operations whose result is fixed: the legacy `RandomState` stream (frozen by numpy) and `ldexp` of an
integer mantissa (exact).  The thresholds are numpy's own (`xray.xray_thresholds`); case `e` plants pixels at float32(thr[k])."""
import hashlib
import math

import numpy as np

# tag -> (H, W, box (x1, y1, x2, y2) with x = columns, seed)
CASES = {
    "a": (96, 80, (20, 30, 60, 70), 1),          # interior box, every bin in use
    "b": (33, 47, (30, 20, 60, 50), 2),          # odd sizes, less than one workgroup's chunk, box past the right and bottom edges
    "c": (64, 64, (0, 0, 64, 64), 3),            # the box is the whole map: fp == 0
    "d": (40, 40, (5, 5, 5, 9), 4),              # empty box: both results NaN
    "e": (257, 300, (50, 40, 250, 200), 5),      # several workgroups per row; specials and ties (below)
    "f": (64, 64, (10, 10, 30, 40), 6),          # constant above thr[0]: every pixel in bin 0
    "g": (64, 64, (10, 10, 30, 40), 7),          # all negative: every pixel in bin T
    "i": (1, 3, (1, 0, 3, 1), 8),                # shorter than one group of four pixels
}
A_SECOND_BOX = (0, 0, 33, 17)                    # map `a` under a second finding (tag "a2")
ORDER = ("a", "b", "c", "d", "e", "f", "g", "i", "a2")          # the batch of nine rows
SHORT_TABLES = ("h1", "h7")                      # map `a` under tables of T = 1 and T = 7 (`short_table`)
E_TIES = tuple(range(5, 1000, 25))               # forty k: pixels set to float32(thr[k])


def thresholds():
    return 2 * 10 ** (-np.linspace(2, 7, 1000))


def short_table(tag):
    return np.array([1e-4]) if tag == "h1" else 2 * 10 ** (-np.linspace(2, 7, 7))


def magnitudes(H, W, seed):
    """fp32 [H, W]: mantissa uniform in [2^23, 2^24), exponent uniform in [-27, -4] (7.5e-9 ... 0.125), random sign."""
    rs = np.random.RandomState(seed)
    m = rs.randint(1 << 23, 1 << 24, size=(H, W))
    e = rs.randint(-27, -3, size=(H, W))
    s = rs.randint(0, 2, size=(H, W)) * 2 - 1
    return np.ascontiguousarray(np.ldexp((m * s).astype(np.float64), e - 23).astype(np.float32))


def case_map(tag):
    tag = "a" if tag in ("a2", "h1", "h7") else tag
    H, W, box, seed = CASES[tag]
    dm = magnitudes(H, W, seed)
    if tag == "f":
        dm[:] = np.float32(0.05)
    elif tag == "g":
        dm = -np.abs(dm)
    elif tag == "e":
        x1, y1, x2, y2 = box
        special = [np.nan, np.inf, -np.inf, 0.0, -0.0]
        for j, v in enumerate(special):
            dm[y1 + 3, x1 + 7 * j + 1] = v       # inside the box
            dm[y2 + 11, 5 * j + 2] = v           # outside
        thr = thresholds()
        for j, k in enumerate(E_TIES):
            if j % 2 == 0:
                dm[y1 + 20 + j, x1 + 3 * j + 2] = np.float32(thr[k])          # inside
            else:
                dm[2 + j // 2, 290 - j] = np.float32(thr[k])                  # outside (rows above the box)
    return dm


def case_box(tag):
    return A_SECOND_BOX if tag == "a2" else CASES["a" if tag in ("h1", "h7") else tag][2]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def box_values(dm, box):
    x1, y1, x2, y2 = box
    return dm[y1:y2, x1:x2].astype(np.float64).ravel()


def box_fsum(dm, box):
    """(math.fsum of the box, or NaN when it holds a value that is not finite; math.fsum of |v| over the finite ones)."""
    v = box_values(dm, box)
    fin = np.isfinite(v)
    return (math.fsum(v.tolist()) if fin.all() else float("nan")), math.fsum(np.abs(v[fin]).tolist())


# the end-to-end case: three fp16 grids of 10 draws x 2 prompts at latent 16 x 16, scored at 128 x 128.  The scale puts the map's
# standard deviation near 0.01, inside the threshold table's range (2e-7 ... 2e-2).
E2E_N = 3
E2E_SIZE = (128, 128)
E2E_BOXES = ((30, 40, 90, 100), (0, 0, 50, 128), (64, 10, 200, 70))          # the last one runs past the right edge


def e2e_grid(j):
    import torch
    g = torch.Generator().manual_seed(9000 + j)
    return (torch.rand(10, 2, 4, 16, 16, generator=g) * 0.2).half()
