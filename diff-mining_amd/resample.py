"""Host half of the device LANCZOS rescale (dm_resize_lanczos, csrc/resize.hip): PIL's coefficient tables and the
per-image descriptors of one batched launch.

`PIL.Image.resize(size, LANCZOS)` on an 8-bit image (what `D.rescale`, compute.py:165-180, calls) is integer arithmetic
over per-output-pixel windows (Pillow's Resample.c):
  * precompute_coeffs: for output position xx, center = (xx + 0.5) * scale, the window [int(center - support + 0.5),
    int(center + support + 0.5)) clipped to the image, weights lanczos((x + xmin - center + 0.5) / filterscale) in
    double, divided by their sum;
  * normalize_coeffs_8bpc: each weight -> int(w * 2^22 +- 0.5) (PRECISION_BITS = 22);
  * a horizontal pass over only the source rows the vertical pass reads, then a vertical pass, each accumulating
    2^21 + sum(pixel * weight) in int32 and storing clip8 = clamp(acc >> 22, 0, 255) as uint8;
  * a pass whose axis keeps its size is skipped (and `resize` to the image's own size is a copy).
`lanczos_axis` restates the first two steps in float64 in PIL's operation order (math.sin is the C library's sin, as in
PIL), so the tables are the ones PIL uses and the device passes are bit-equal.  `resize_numpy` runs the two integer
passes on the host: the CPU tests drive the tables through it against PIL itself.
"""
from __future__ import annotations

import functools
import math
from typing import Sequence, Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2
SUPPORT = 3.0                          # lanczos_filter's support

# mirrors `dm_resize_desc` (include/dm_engine.h): 48 bytes, no padding
DESC_DTYPE = np.dtype([("src_offset", "<i8"), ("src_w", "<i4"), ("src_h", "<i4"), ("ybox_first", "<i4"), ("tmp_rows", "<i4"),
                       ("kx", "<i4"), ("ky", "<i4"), ("xb_off", "<i4"), ("xk_off", "<i4"), ("yb_off", "<i4"), ("yk_off", "<i4")])
assert DESC_DTYPE.itemsize == 48


def _sinc_v(x: np.ndarray) -> np.ndarray:
    """PIL's sinc_filter elementwise; the sine is the C library's (math.sin), not numpy's vectorised one, whose last
    bit may differ."""
    y = x * math.pi
    sy = np.fromiter(map(math.sin, y.tolist()), dtype=np.float64, count=y.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, sy / y)


@functools.lru_cache(maxsize=4096)
def lanczos_axis(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's table for one axis resized from in_size to out_size: bounds int32 [out_size, 2] (window start, length) and
    fixed-point weights int32 [out_size, ksize] (zero past each window's length).  An axis that keeps its size is a pass
    PIL skips: the identity table (one tap of weight 2^22) gives the same bytes.  Cached: work lists repeat axis sizes."""
    assert in_size >= 1 and out_size >= 1, (in_size, out_size)
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size, dtype=np.int32), np.ones(out_size, dtype=np.int32)], 1)
        kk = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        scale = float(in_size) / out_size          # (double)(in1 - in0) / outSize with the default box (0, in_size)
        filterscale = max(scale, 1.0)
        support = SUPPORT * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        # vectorised over (output position, tap); every step is one IEEE double operation in PIL's order
        center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)       # (int) truncates toward zero
        xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
        taps = np.arange(ksize)
        x = ((xmin[:, None] + taps[None, :]).astype(np.float64) - center[:, None] + 0.5) * ss
        live = (taps[None, :] < xmax[:, None]) & (x >= -3.0) & (x < 3.0)
        w = np.zeros_like(x)
        xs = x[live]
        w[live] = _sinc_v(xs) * _sinc_v(xs / 3)
        ww = np.zeros(out_size)
        for t in range(ksize):                     # PIL sums the weights left to right: no pairwise summation
            ww = ww + w[:, t]
        w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
        one = float(1 << PRECISION_BITS)
        kk = np.trunc(np.where(w < 0, -0.5 + w * one, 0.5 + w * one)).astype(np.int32)
        bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def resize_plan(src_sizes: Sequence[Tuple[int, int]], out_w: int, out_h: int):
    """Descriptors + tables of one dm_resize_lanczos launch over images of sizes src_sizes [(w, h)] packed back to back
    (uint8 HWC) in that order.  Returns (desc [n] DESC_DTYPE, tables int32 [T], tmp_rows_max)."""
    desc = np.zeros(len(src_sizes), dtype=DESC_DTYPE)
    parts, at, off = [], 0, 0
    axis_at = {}                                   # one copy of each distinct axis table per launch

    def put(key, arr):
        nonlocal at
        if key not in axis_at:
            axis_at[key] = at
            parts.append(arr.reshape(-1))
            at += arr.size
        return axis_at[key]
    for i, (w, h) in enumerate(src_sizes):
        xb, xk = lanczos_axis(w, out_w)
        yb, yk = lanczos_axis(h, out_h)
        ybox_first = int(yb[0, 0])
        ybox_last = int(yb[-1, 0] + yb[-1, 1])
        yb_rel = yb.copy()
        yb_rel[:, 0] -= ybox_first
        assert (xb[:, 0] + xb[:, 1] <= w).all() and (yb_rel[:, 0] >= 0).all() and (yb_rel[:, 0] + yb_rel[:, 1] <= ybox_last - ybox_first).all()
        d = desc[i]
        d["src_offset"], d["src_w"], d["src_h"] = off, w, h
        d["ybox_first"], d["tmp_rows"] = ybox_first, ybox_last - ybox_first
        d["kx"], d["ky"] = xk.shape[1], yk.shape[1]
        d["xb_off"], d["xk_off"] = put(("xb", w, out_w), xb), put(("xk", w, out_w), xk)
        d["yb_off"], d["yk_off"] = put(("yb", h, out_h), yb_rel), put(("yk", h, out_h), yk)
        off += w * h * 3
    tables = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    assert at < 2 ** 31
    return desc, tables, int(desc["tmp_rows"].max()) if len(desc) else 0


def _clip8(acc: np.ndarray) -> np.ndarray:
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_numpy(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """The two integer passes of PIL's 8-bit resampler on the host, driven by `lanczos_axis`'s tables (what the device
    kernels compute): uint8 [H, W, C] -> uint8 [out_h, out_w, C]."""
    h, w = img.shape[:2]
    xb, xk = lanczos_axis(w, out_w)
    yb, yk = lanczos_axis(h, out_h)
    y0, y1 = int(yb[0, 0]), int(yb[-1, 0] + yb[-1, 1])
    src = img[y0:y1].astype(np.int64)
    tmp = np.empty((y1 - y0, out_w) + img.shape[2:], dtype=np.uint8)
    for x in range(out_w):
        s, n = xb[x]
        acc = np.full(tmp[:, x].shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(n):
            acc += src[:, s + t] * int(xk[x, t])
        tmp[:, x] = _clip8(acc)
    tmp = tmp.astype(np.int64)
    out = np.empty((out_h, out_w) + img.shape[2:], dtype=np.uint8)
    for y in range(out_h):
        s, n = yb[y]
        s -= y0
        acc = np.full(out[y].shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(n):
            acc += tmp[s + t] * int(yk[y, t])
        out[y] = _clip8(acc)
    return out
