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


# ---- CLIP image preprocessing (`CLIPImageProcessor`, PIL backend): BICUBIC shortest-edge resize, center crop, rescale, normalise ----
# `Cluster.embed` (cluster.py:224-231) feeds `processor(images=[crop])` to CLIP ViT-B/32.  The processor resizes the uint8 crop with
# `PIL.Image.resize((new_w, new_h), BICUBIC)` (short side -> 224, long side -> int(224 * long / short)), center-crops 224 x 224 at
# ((h - 224) // 2, (w - 224) // 2), rescales `uint8.astype(float64) * (1 / 255)` -> float32 and normalises `(x - mean) / std` in
# float32.  BICUBIC is the same 8-bit two-pass resampler as LANCZOS with PIL's bicubic filter (a = -0.5, support 2): only the output
# columns / rows that survive the crop are computed, each from its own coefficient window, so the result is bit-equal.
CLIP_SIZE = 224
CLIP_PATCH = 32
CLIP_MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)     # OPENAI_CLIP_MEAN
CLIP_STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)      # OPENAI_CLIP_STD
BICUBIC_SUPPORT = 2.0
CLIP_NEED_H, CLIP_NEED_V = 1, 2

# mirrors `dm_clip_pre_desc` (include/dm_engine.h): 72 bytes, no padding
CLIP_DESC_DTYPE = np.dtype([("src_offset", "<i8"), ("src_w", "<i4"), ("src_h", "<i4"),
                            ("crop_col0", "<i4"), ("crop_row0", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"),
                            ("left", "<i4"), ("top", "<i4"), ("kx", "<i4"), ("ky", "<i4"),
                            ("xb_off", "<i4"), ("xk_off", "<i4"), ("yb_off", "<i4"), ("yk_off", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert CLIP_DESC_DTYPE.itemsize == 72


def _bicubic_v(x: np.ndarray) -> np.ndarray:
    """PIL's bicubic_filter (a = -0.5) elementwise, in its operation order."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=4096)
def bicubic_axis(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's BICUBIC table for one axis resized from in_size to out_size, in `lanczos_axis`'s format and by the same float64
    formula (precompute_coeffs + normalize_coeffs_8bpc): bounds int32 [out_size, 2], fixed-point weights int32 [out_size, ksize].
    An axis that keeps its size gets the identity table (PIL skips that pass)."""
    assert in_size >= 1 and out_size >= 1, (in_size, out_size)
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size, dtype=np.int32), np.ones(out_size, dtype=np.int32)], 1)
        kk = np.full((out_size, 1), 1 << PRECISION_BITS, dtype=np.int32)
    else:
        scale = float(in_size) / out_size
        filterscale = max(scale, 1.0)
        support = BICUBIC_SUPPORT * filterscale
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / filterscale
        center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5), 0).astype(np.int64)
        xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
        taps = np.arange(ksize)
        x = ((xmin[:, None] + taps[None, :]).astype(np.float64) - center[:, None] + 0.5) * ss
        live = taps[None, :] < xmax[:, None]
        w = np.where(live, _bicubic_v(x), 0.0)
        ww = np.zeros(out_size)
        for t in range(ksize):                     # left to right, as PIL
            ww = ww + w[:, t]
        w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
        one = float(1 << PRECISION_BITS)
        kk = np.trunc(np.where(w < 0, -0.5 + w * one, 0.5 + w * one)).astype(np.int32)
        bounds = np.stack([xmin, xmax], 1).astype(np.int32)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def clip_resize_size(w: int, h: int, size: int = CLIP_SIZE) -> Tuple[int, int]:
    """`get_resize_output_image_size(..., size=224, default_to_square=False)`: (new_w, new_h), short side -> size."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def _window(table: Tuple[np.ndarray, np.ndarray], start: int, n: int):
    b, k = table
    return b[start:start + n], k[start:start + n]


def clip_crop_box(img_hw: Tuple[int, int], box) -> Tuple[int, int, int, int]:
    """The reference's box (x_start, y_start, x_end, y_end; x = rows, cluster.py:258-262) or None (the whole image) ->
    (row0, col0, rows, cols), checked: an empty box or one reaching outside the image raises ValueError (PIL would zero-pad it)."""
    H, W = img_hw
    if box is None:
        return 0, 0, H, W
    x0, y0, x1, y1 = (int(v) for v in box)
    if not (0 <= x0 < x1 <= H and 0 <= y0 < y1 <= W):
        raise ValueError(f"box {tuple(box)} is empty or outside the {H}x{W} image (x = rows, y = columns)")
    return x0, y0, x1 - x0, y1 - y0


def check_clip_image(img) -> np.ndarray:
    """uint8 HWC RGB array (a PIL image is converted to RGB first), else TypeError / ValueError."""
    if hasattr(img, "convert") and hasattr(img, "size"):
        img = np.asarray(img.convert("RGB"))
    if not isinstance(img, np.ndarray):
        raise TypeError(f"expected a uint8 HWC numpy array or a PIL image, got {type(img).__name__}")
    if img.dtype != np.uint8:
        raise ValueError(f"expected uint8 pixels, got {img.dtype}")
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"expected an HWC RGB image with 3 channels, got shape {img.shape}")
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"empty image {img.shape}")
    return np.ascontiguousarray(img)


def clip_patch_tables(crop_w: int, crop_h: int):
    """The per-patch geometry of the processor: (need_h, need_v, left, top, x table window, y table window), the windows covering
    only the 224 output columns / rows the center crop keeps."""
    new_w, new_h = clip_resize_size(crop_w, crop_h)
    top, left = (new_h - CLIP_SIZE) // 2, (new_w - CLIP_SIZE) // 2
    need_h, need_v = new_w != crop_w, new_h != crop_h
    xt = _window(bicubic_axis(crop_w, new_w), left, CLIP_SIZE)
    yt = _window(bicubic_axis(crop_h, new_h), top, CLIP_SIZE)
    return need_h, need_v, left, top, xt, yt


def clip_plan(images: Sequence[np.ndarray], boxes: Sequence):
    """Descriptors + tables of one dm_f32_clip_preprocess launch.  images: checked uint8 HWC arrays packed back to back in that
    order; boxes: per image a list of boxes (or None = the whole image).  Returns (desc [P] CLIP_DESC_DTYPE, tables int32 [T],
    owner [P] image index).  Window starts in the tables are relative to the crop."""
    if len(images) != len(boxes):
        raise ValueError(f"{len(images)} images but {len(boxes)} box lists")
    rows, owner = [], []
    src_off = 0
    for i, (img, bl) in enumerate(zip(images, boxes)):
        H, W = img.shape[:2]
        for box in ([None] if bl is None else bl):
            rows.append((src_off, W, H) + clip_crop_box((H, W), box))
            owner.append(i)
        src_off += H * W * 3
    desc = np.zeros(len(rows), dtype=CLIP_DESC_DTYPE)
    parts, at = [], 0
    table_at = {}                                  # one copy of each distinct table window per launch

    def put(key, arr):
        nonlocal at
        if key not in table_at:
            table_at[key] = at
            parts.append(np.ascontiguousarray(arr).reshape(-1))
            at += arr.size
        return table_at[key]
    for p, (off, W, H, r0, c0, rh, cw) in enumerate(rows):
        need_h, need_v, left, top, (xb, xk), (yb, yk) = clip_patch_tables(cw, rh)
        assert (xb[:, 0] >= 0).all() and (xb[:, 0] + xb[:, 1] <= cw).all() and (yb[:, 0] >= 0).all() and (yb[:, 0] + yb[:, 1] <= rh).all()
        assert (need_h or left + CLIP_SIZE <= cw) and (need_v or top + CLIP_SIZE <= rh)
        d = desc[p]
        d["src_offset"], d["src_w"], d["src_h"] = off, W, H
        d["crop_col0"], d["crop_row0"], d["crop_w"], d["crop_h"] = c0, r0, cw, rh
        d["left"], d["top"], d["kx"], d["ky"] = left, top, xk.shape[1], yk.shape[1]
        d["xb_off"], d["xk_off"] = put(("xb", cw, rh), xb), put(("xk", cw, rh), xk)
        d["yb_off"], d["yk_off"] = put(("yb", cw, rh), yb), put(("yk", cw, rh), yk)
        d["flags"] = (CLIP_NEED_H if need_h else 0) | (CLIP_NEED_V if need_v else 0)
    tables = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    if at >= 2 ** 31:
        raise ValueError("too many distinct crop sizes in one call")
    return desc, tables, np.asarray(owner, dtype=np.int64)


def resize_numpy_tables(img: np.ndarray, xt, yt, need_h: bool, need_v: bool, x_first: int = 0, y_first: int = 0) -> np.ndarray:
    """PIL's two 8-bit passes over the windows (xt, yt) = (bounds, weights) of the output columns / rows wanted; a skipped pass
    (need_* False) copies the source columns / rows from x_first / y_first on, as PIL's resize returns a copy there."""
    xb, xk = xt
    yb, yk = yt
    nx, ny = xb.shape[0], yb.shape[0]
    if need_v:
        y0, y1 = int(yb[0, 0]), int(yb[-1, 0] + yb[-1, 1])
    else:
        y0, y1 = y_first, y_first + ny
    src = img[y0:y1].astype(np.int64)
    if need_h:
        tmp = np.empty((y1 - y0, nx) + img.shape[2:], dtype=np.uint8)
        for x in range(nx):
            s, n = xb[x]
            acc = np.full(tmp[:, x].shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
            for t in range(n):
                acc += src[:, s + t] * int(xk[x, t])
            tmp[:, x] = _clip8(acc)
    else:
        tmp = img[y0:y1, x_first:x_first + nx].copy()
    if not need_v:
        return tmp
    tmp = tmp.astype(np.int64)
    out = np.empty((ny, nx) + img.shape[2:], dtype=np.uint8)
    for y in range(ny):
        s, n = yb[y]
        s -= y0
        acc = np.full(out[y].shape, 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(n):
            acc += tmp[s + t] * int(yk[y, t])
        out[y] = _clip8(acc)
    return out


def clip_normalize_numpy(u8: np.ndarray) -> np.ndarray:
    """uint8 HWC -> float32 CHW: `(u8.astype(float64) * (1 / 255)).astype(float32)`, then `(x - mean) / std` in float32."""
    x = (u8.astype(np.float64) * (1 / 255)).astype(np.float32)
    x = (x - CLIP_MEAN) / CLIP_STD
    return np.ascontiguousarray(x.transpose(2, 0, 1))


def clip_preprocess_numpy(image_u8, box=None) -> np.ndarray:
    """`CLIPImageProcessor(images=[image.crop((y0, x0, y1, x1))])["pixel_values"][0]` restated on the host with `bicubic_axis`'s
    tables (what the device kernels compute): box in the reference's convention (x = rows) or None -> float32 [3, 224, 224]."""
    img = check_clip_image(image_u8)
    r0, c0, rh, cw = clip_crop_box(img.shape[:2], box)
    crop = img[r0:r0 + rh, c0:c0 + cw]
    need_h, need_v, left, top, xt, yt = clip_patch_tables(cw, rh)
    return clip_normalize_numpy(resize_numpy_tables(crop, xt, yt, need_h, need_v, left, top))


# ---- the configurable tower's processor (CLIP baseline, clipmining/ranking.py:60-66): `CLIPImageProcessor(size={"shortest_edge": S},
# do_center_crop=False)` on the 512 x 512 center crop.  Only square inputs: a non-square one would change the token grid, which the
# reference never does.  The whole s x s image maps onto S x S, so left = top = 0 and the tables cover every output column / row.
def check_clip_tower_image(img) -> np.ndarray:
    img = check_clip_image(img)
    if img.shape[0] != img.shape[1]:
        raise ValueError(f"the tower takes square images (the reference center-crops to 512 x 512 first), got {img.shape[0]}x{img.shape[1]}")
    return img


def clip_tower_plan(images: Sequence[np.ndarray], size: int = 336):
    """Descriptors + tables of one dm_f32_clip_tower_preprocess / dm_f32_clip_tower_image_tokens call: checked square uint8 HWC
    images packed back to back -> (desc [n] CLIP_DESC_DTYPE, tables int32 [T]).  One copy of the table of each distinct side."""
    desc = np.zeros(len(images), dtype=CLIP_DESC_DTYPE)
    parts, at, where = [], 0, {}
    src_off = 0
    for p, img in enumerate(images):
        s = check_clip_tower_image(img).shape[0]
        if s not in where:
            b, k = bicubic_axis(s, size)
            assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= s).all()
            where[s] = (at, at + b.size, k.shape[1])
            parts += [b.reshape(-1), k.reshape(-1)]
            at += b.size + k.size
        b_off, k_off, taps = where[s]
        d = desc[p]
        d["src_offset"], d["src_w"], d["src_h"] = src_off, s, s
        d["crop_col0"], d["crop_row0"], d["crop_w"], d["crop_h"] = 0, 0, s, s
        d["left"], d["top"], d["kx"], d["ky"] = 0, 0, taps, taps
        d["xb_off"], d["xk_off"], d["yb_off"], d["yk_off"] = b_off, k_off, b_off, k_off
        d["flags"] = (CLIP_NEED_H | CLIP_NEED_V) if s != size else 0
        src_off += s * s * 3
    if at >= 2 ** 31:
        raise ValueError("too many distinct image sizes in one call")
    tables = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)
    return desc, tables


def clip_tower_preprocess_numpy(image, size: int = 336) -> np.ndarray:
    """`CLIPImageProcessor(size={"shortest_edge": size}, do_center_crop=False)(images=image)["pixel_values"][0]` for a square image,
    restated on the host with `bicubic_axis`'s tables (what the device kernel computes) -> float32 [3, size, size]."""
    img = check_clip_tower_image(image)
    t = bicubic_axis(img.shape[0], size)
    need = img.shape[0] != size
    return clip_normalize_numpy(resize_numpy_tables(img, t, t, need, need))
