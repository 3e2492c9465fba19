"""Typicality overlays: the patches faded to white wherever they are not typical (what a person looks at), from maps and images that
stay on the GPU.  Kernels: csrc/overlay.hip; C ABI: dm_overlay_workspace_bytes / dm_gaussian_filter_maps / dm_overlay_blend.

The reference keeps this code in three places, and the three differ in their dtype flow:

  'image'   `Cluster.load_and_apply_alpha_bbox` (typicality/cluster.py:93-110): the whole-image map of `load_typicality_norm`,
            `gaussian_filter(sigma=10)`, `T*(T>0)`, written into a float64 `zeros_like(I)` (a map smaller than the image leaves zeros),
            the blend in float64, then the crop to the box.
  'crop'    `utils.apply_alpha` (typicality/utils.py:165-214): the `d_compute` crop, `gaussian_filter`, division by the maximum,
            `T*(T>0)` - all in fp32 - and the blend, where `1 - T` is still an fp32 operation and only then meets the float64 image.
  'stored'  `Cluster.apply_alpha_` (applications/parallel-dataset/cluster.py:132-141): the blend alone from a stored T (numpy's own
            promotion by T's dtype; on the device T is the fp32 value widened to float64, which is what 'image' stores).

The rules `*_host` (numpy, the CPU tier's yardstick and the path a numpy input takes) and the kernels share:

  filter    scipy.ndimage.gaussian_filter(a, sigma) on a 2-D fp32 map, truncate=4, mode='reflect': the weights are
            exp(-0.5/sigma^2 x^2) / sum on arange(-r, r+1), r = int(4 sigma + 0.5), taken with numpy so that the bits are numpy's;
            reflect is a mirror of period 2n (d c b a | a b c d | d c b a), repeated when the map is narrower than the radius; each
            1-D pass starts from the centre tap a[i] w[0] and adds the symmetric pairs (a[i-j] + a[i+j]) w[j] in fp64 from j = r
            inward to j = 1, then rounds to fp32 once; axis 0 first, then axis 1.  Bit-equal to scipy (tests/test_overlay.py).
  post-op   'none'; 'clamp' = T*(T>0) in fp32 (a negative value becomes -0.0, as numpy gives it); 'unit' = T / max(T) in fp32, then
            the clamp.  A maximum of exactly 0 (or NaN) after filtering is a DEPARTURE: the reference divides by it and casts NaN to
            uint8, which is undefined; here the map becomes all zeros and the row carries a `degenerate` flag.
  blend     per pixel and channel in float64, I = u8 / 255.0, R = 0.05*I + 0.95*(T*I + (1-T)) with the variant's dtype flow, then
            (R*255) truncated toward zero to an integer and reduced modulo 256 (what numpy's `.astype(np.uint8)` gives on x86-64
            for |R*255| < 2^31; inside [0, 255] no reduction happens).
  box       (x_start, y_start, x_end, y_end) with x = ROWS (the mining convention), inside the image; a map that overhangs the image
            is refused (the reference raises); a zero-area box writes nothing.
  luminance `filter_patch` (utils.py:104-109): PIL's 'L' value (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the PLAIN crop, summed
            as an integer; the verdict is 30 < sum / count < 225 in float64 (False for an empty crop: the mean of nothing is NaN).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import EngineError, UNetEngine, _p, load_library as _lib

GAUSS_TILE = 32                 # DM_GAUSS_TILE: the filter's output tile is 32 x 32
GAUSS_MAX_RADIUS = 200          # DM_GAUSS_MAX_RADIUS: (32 + 2 r) x 32 fp32 of LDS stay below 64 KiB
POST_OPS = {"none": 0, "clamp": 1, "unit": 2}
VARIANTS = {"image": 0, "crop": 1, "stored": 2}
# dm_gauss_desc (32 bytes) and dm_overlay_row (80 bytes) of include/dm_engine.h
GAUSS_DESC_DTYPE = np.dtype([("map_offset", "<i8"), ("out_offset", "<i8"), ("work_offset", "<i8"), ("H", "<i4"), ("W", "<i4")])
OVERLAY_ROW_DTYPE = np.dtype([("image_offset", "<i8"), ("map_offset", "<i8"), ("out_offset", "<i8"), ("alpha_offset", "<i8"),
                              ("img_h", "<i4"), ("img_w", "<i4"), ("map_h", "<i4"), ("map_w", "<i4"), ("map_x0", "<i4"), ("map_y0", "<i4"),
                              ("x_start", "<i4"), ("y_start", "<i4"), ("x_end", "<i4"), ("y_end", "<i4"), ("variant", "<i4"),
                              ("map_index", "<i4")])


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatements
# ------------------------------------------------------------------------------------------------------------------------------
def gauss_weights(sigma: float):
    """scipy's `_gaussian_kernel1d(sigma, 0, r)` -> (float64 [2 r + 1], r)."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError(f"overlay: sigma {sigma} must be > 0")
    r = int(4.0 * sigma + 0.5)
    if r > GAUSS_MAX_RADIUS:
        raise ValueError(f"overlay: sigma {sigma} gives radius {r}, more than {GAUSS_MAX_RADIUS}")
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum(), r


def _reflect_index(lo: int, hi: int, n: int) -> np.ndarray:
    m = np.mod(np.arange(lo, hi), 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def _filter_axis0(a, w, r):
    n = a.shape[0]
    ap = a.astype(np.float64)[_reflect_index(-r, n + r, n)]
    acc = ap[r:r + n] * w[r]
    for j in range(r, 0, -1):                         # far to near, as the kernel
        acc += (ap[r - j:r - j + n] + ap[r + j:r + j + n]) * w[r - j]
    return acc.astype(np.float32)


def _as_map(a, what="map"):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"overlay: {what} must be [H, W] with H, W >= 1, got {a.shape}")
    return a.astype(np.float32, copy=False)


def gaussian_filter_host(a, sigma):
    """`scipy.ndimage.gaussian_filter(a, sigma)` for a 2-D fp32 map, bit for bit (the rules at the top of this module)."""
    a = _as_map(a)
    w, r = gauss_weights(sigma)
    with np.errstate(all="ignore"):
        t = _filter_axis0(a, w, r)
        return np.ascontiguousarray(_filter_axis0(np.ascontiguousarray(t.T), w, r).T)


def post_op_host(F, post_op: str = "none"):
    """The filter's post-op on an fp32 map -> (map, max or None, degenerate)."""
    F = _as_map(F)
    if post_op not in POST_OPS:
        raise ValueError(f"overlay: unknown post-op {post_op!r}")
    with np.errstate(all="ignore"):
        if post_op == "none":
            return F, None, False
        if post_op == "clamp":
            return F * (F > 0), None, False
        m = np.max(F)
        if m == 0 or np.isnan(m):
            return np.zeros_like(F), m, True
        F = F / m
        return F * (F > 0), m, False


def _to_u8(R):
    with np.errstate(all="ignore"):
        return (R * 255).astype(np.int64).astype(np.uint8)


def _as_image(image_u8, what="image"):
    I = np.asarray(image_u8)
    if I.dtype != np.uint8 or I.ndim != 3 or I.shape[2] != 3:
        raise ValueError(f"overlay: {what} must be uint8 [H, W, 3], got {I.dtype} {I.shape}")
    return I


def _check_box(bbox, H, W):
    x0, y0, x1, y1 = (int(v) for v in bbox)
    if not (0 <= x0 <= x1 <= H and 0 <= y0 <= y1 <= W):
        raise ValueError(f"overlay: box {(x0, y0, x1, y1)} outside the {H}x{W} image (x = rows)")
    return x0, y0, x1, y1


def alpha_bbox_host(alpha, image_u8, bbox, sigma=10):
    """`load_and_apply_alpha_bbox` after `load_typicality_norm` -> (uint8 crop [bh, bw, 3], alpha crop float64 [bh, bw, 3])."""
    alpha, image_u8 = _as_map(alpha), _as_image(image_u8)
    H, W = image_u8.shape[:2]
    if alpha.shape[0] > H or alpha.shape[1] > W:
        raise ValueError(f"overlay: the {alpha.shape[0]}x{alpha.shape[1]} map overhangs the {H}x{W} image")
    bbox = _check_box(bbox, H, W)
    I = image_u8 / 255.0
    T = gaussian_filter_host(alpha, sigma)
    T = T * (T > 0)
    T = np.stack((T, T, T), axis=-1)
    a = np.zeros_like(I)
    a[:T.shape[0], :T.shape[1], :] = T
    T = a
    R = 0.05 * I + 0.95 * (T * I + (1 - T))
    R = R[bbox[0]:bbox[2], bbox[1]:bbox[3]]
    return _to_u8(R), a[bbox[0]:bbox[2], bbox[1]:bbox[3]]


def apply_alpha_host(T_crop, patch_u8, sigma=10):
    """`apply_alpha` from `gaussian_filter` on -> (uint8 [bh, bw, 3], degenerate)."""
    T_crop, patch_u8 = _as_map(T_crop, "crop"), _as_image(patch_u8, "patch")
    if T_crop.shape != patch_u8.shape[:2]:
        raise ValueError(f"overlay: the crop is {T_crop.shape}, the patch {patch_u8.shape[:2]}")
    I = patch_u8 / 255.0
    T, _, degenerate = post_op_host(gaussian_filter_host(T_crop, sigma), "unit")
    T = np.stack((T, T, T), axis=-1)
    with np.errstate(all="ignore"):
        R = 0.05 * I + 0.95 * (T * I + (1 - T))
    return _to_u8(R), degenerate


def blend_host(T, patch_u8):
    """`apply_alpha_` of the parallel dataset: the blend alone.  T: [bh, bw] or [bh, bw, 3], any float dtype (numpy promotes as the
    reference's line does)."""
    patch_u8 = _as_image(patch_u8, "patch")
    T = np.asarray(T)
    if T.ndim == 2:
        T = np.stack((T, T, T), axis=-1)
    if T.shape != patch_u8.shape:
        raise ValueError(f"overlay: T is {T.shape}, the patch {patch_u8.shape}")
    I = patch_u8 / 255.0
    with np.errstate(all="ignore"):
        R = 0.05 * I + 0.95 * (T * I + (1 - T))
    return _to_u8(R)


def filter_patch_host(patch_u8, black_threshold=30, white_threshold=225):
    """`filter_patch` -> (the integer sum of PIL's 'L' values of an RGB / RGBA uint8 patch, the reference's verdict)."""
    p = np.asarray(patch_u8)
    if p.dtype != np.uint8 or p.ndim != 3 or p.shape[2] not in (3, 4):
        raise ValueError(f"overlay: patch must be uint8 [h, w, 3 | 4], got {p.dtype} {p.shape}")
    p = p.astype(np.int64)
    lum = (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16
    s, count = int(lum.sum()), lum.size
    return s, bool(count and black_threshold < np.float64(s) / np.float64(count) < white_threshold)


# ------------------------------------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------------------------------------
def workspace_bytes(n_maps: int, total_elements: int, max_h: int, max_w: int) -> int:
    need = _lib().dm_overlay_workspace_bytes(int(n_maps), int(total_elements), int(max_h), int(max_w))
    if not need:
        raise ValueError(f"overlay: no workspace for {n_maps} maps of {total_elements} elements, at most {max_h}x{max_w}")
    return need


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def gaussian_filter(maps, sigma, post_op: str = "none", work=None, return_max: bool = False):
    """`gaussian_filter_host` (+ `post_op_host`) for a list of fp32 [H, W] maps of mixed sizes in ONE call (dm_gaussian_filter_maps) on
    the device the maps live on; contiguous views of one buffer are read where they lie.  Returns a list of fp32 maps (views of one
    packed buffer), each bit-equal to the restatement; with return_max also the fp32 [n] maxima of post_op='unit' (NaN bits aside).
    A list of numpy arrays takes the restatement; anything else that is not on a GPU raises."""
    import torch
    if post_op not in POST_OPS:
        raise ValueError(f"overlay: unknown post-op {post_op!r}")
    if len(maps) < 1:
        raise ValueError("overlay: no maps")
    if all(isinstance(m, np.ndarray) for m in maps):
        got = [post_op_host(gaussian_filter_host(m, sigma), post_op) for m in maps]
        out = [g[0] for g in got]
        return (out, np.array([np.nan if g[1] is None else g[1] for g in got], dtype=np.float32)) if return_max else out
    if not all(isinstance(m, torch.Tensor) and m.is_cuda for m in maps):
        raise EngineError("overlay.gaussian_filter: maps must be torch tensors on the GPU (gaussian_filter_host is the numpy restatement)")
    w, r = gauss_weights(sigma)
    for b, m in enumerate(maps):
        if m.dim() != 2 or m.numel() < 1:
            raise ValueError(f"overlay: map {b} must be [H, W] with H, W >= 1, got {tuple(m.shape)}")
    dev = maps[0].device
    n = len(maps)
    packed, offsets, _ = UNetEngine._place_maps(torch, list(maps), dev)
    desc = np.zeros(n, dtype=GAUSS_DESC_DTYPE)
    desc["H"], desc["W"] = [m.shape[0] for m in maps], [m.shape[1] for m in maps]
    sizes = desc["H"].astype(np.int64) * desc["W"]
    desc["map_offset"] = offsets
    desc["out_offset"] = desc["work_offset"] = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    need = workspace_bytes(n, total, int(desc["H"].max()), int(desc["W"].max()))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    elif work.numel() * work.element_size() < need:
        raise ValueError(f"overlay: workspace of {work.numel() * work.element_size()} bytes, {need} needed")
    up = torch.from_numpy(np.concatenate([w.view(np.uint8), desc.view(np.uint8)])).to(dev)          # both tables in one upload
    w_d, desc_d = up[:w.nbytes], up[w.nbytes:]
    out = torch.empty(total, dtype=torch.float32, device=dev)
    mx = torch.empty(n, dtype=torch.float32, device=dev) if POST_OPS[post_op] == 2 else None
    with torch.cuda.device(dev):
        rc = _lib().dm_gaussian_filter_maps(_p(packed), _p(desc_d), n, float(sigma), _p(w_d), r, POST_OPS[post_op], _p(work),
                                            work.numel() * work.element_size(), _p(out), _p(mx), _stream(torch, dev))
    if rc:
        raise EngineError(f"dm_gaussian_filter_maps: {'bad argument' if rc == 1 else 'HIP error'} (code {rc})")
    views = [out[int(d["out_offset"]):int(d["out_offset"]) + int(d["H"]) * int(d["W"])].view(int(d["H"]), int(d["W"])) for d in desc]
    return (views, mx) if return_max else views


def _row_columns(rows, n_images):
    cols = {k: np.asarray(rows[k]).astype(np.int64) for k in ("image", "x_start", "y_start", "x_end", "y_end")}
    n = len(cols["image"])
    if any(len(v) != n for v in cols.values()):
        raise ValueError("overlay: the row columns differ in length")
    if n and (cols["image"].min() < 0 or cols["image"].max() >= n_images):
        raise ValueError(f"overlay: a row names image {cols['image'].max()} of {n_images}")
    return cols, n


def _rows_host(images, maps, cols, n, variant, sigma, want_alpha):
    out = {"blended": [], "plain": [], "alpha": [] if want_alpha else None, "lum_sum": np.zeros(n, np.int64),
           "verdict": np.zeros(n, bool), "degenerate": np.zeros(n, bool)}
    for q in range(n):
        b = int(cols["image"][q])
        I = _as_image(images[b])
        box = _check_box([cols[k][q] for k in ("x_start", "y_start", "x_end", "y_end")], *I.shape[:2])
        plain = I[box[0]:box[2], box[1]:box[3]]
        if variant == "image":
            u8, alpha = alpha_bbox_host(maps[b], I, box, sigma)
            alpha = alpha[..., 0].astype(np.float32)
        elif variant == "crop":
            m = _as_map(maps[b])
            if m.shape[0] > I.shape[0] or m.shape[1] > I.shape[1] or box[2] > m.shape[0] or box[3] > m.shape[1]:
                raise ValueError(f"overlay: box {box} and the {m.shape} map of the {I.shape[:2]} image do not fit")
            if plain.size:
                crop = m[box[0]:box[2], box[1]:box[3]]
                u8, out["degenerate"][q] = apply_alpha_host(crop, plain, sigma)
                alpha = post_op_host(gaussian_filter_host(crop, sigma), "unit")[0]
            else:
                u8, alpha = plain.copy(), np.zeros(plain.shape[:2], np.float32)
        else:
            T = _as_map(maps[q]) if plain.size else np.zeros(plain.shape[:2], np.float32)
            u8, alpha = blend_host(T.astype(np.float64), plain), T
        out["blended"].append(u8)
        out["plain"].append(plain.copy())
        if want_alpha:
            out["alpha"].append(alpha)
        out["lum_sum"][q], out["verdict"][q] = filter_patch_host(plain)
    return out


def overlay_rows(images, maps, rows, variant: str = "image", sigma=10, want_alpha: bool = False):
    """The three blend variants for a table of rows in ONE filter call and ONE blend call (dm_gaussian_filter_maps, dm_overlay_blend).
    images: a list of uint8 [H, W, 3] tensors on the GPU.  rows: a dict with the columns `image` (index into `images`), `x_start`,
    `y_start`, `x_end`, `y_end` (x = rows; `TypicalityScorer.mine_patches`' result has them).  maps, by variant:
      'image'   one normalised whole-image map per image (`load_typicality_norm`; it may be smaller than its image), filtered once per
                image with the clamp;
      'crop'    one `maxabs` whole-image map per image (`d_compute` before its crop); every row's crop is filtered on its own,
                divided by its own maximum and clamped;
      'stored'  one stored fp32 T per ROW, of the box's size; no filter.
    Returns {'blended': list of uint8 [bh, bw, 3], 'plain': list of uint8 [bh, bw, 3], 'alpha': list of fp32 [bh, bw] (the T that was
    blended; None unless want_alpha), 'lum_sum': int64 [n], 'verdict': bool [n], 'degenerate': bool [n]} as device tensors, byte-equal
    to the restatements.  Numpy inputs take the restatements and return numpy arrays; anything else that is not on a GPU raises."""
    import torch
    if variant not in VARIANTS:
        raise ValueError(f"overlay: unknown variant {variant!r}")
    cols, n = _row_columns(rows, len(images))
    if n < 1:
        raise ValueError("overlay: no rows")
    if len(maps) != (n if variant == "stored" else len(images)):
        raise ValueError(f"overlay: {len(maps)} maps for {len(images)} images and {n} rows ({variant})")
    if all(isinstance(t, np.ndarray) for t in list(images) + list(maps)):
        return _rows_host(images, maps, cols, n, variant, sigma, want_alpha)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in list(images) + list(maps)):
        raise EngineError("overlay.overlay_rows: images and maps must be torch tensors on the GPU (the *_host functions are the restatement)")
    dev = images[0].device
    for b, I in enumerate(images):
        if I.dtype != torch.uint8 or I.dim() != 3 or I.shape[2] != 3:
            raise ValueError(f"overlay: image {b} must be uint8 [H, W, 3], got {I.dtype} {tuple(I.shape)}")
    for b, m in enumerate(maps):
        if m.dim() != 2:
            raise ValueError(f"overlay: map {b} must be [H, W], got {tuple(m.shape)}")
    boxes = [_check_box([cols[k][q] for k in ("x_start", "y_start", "x_end", "y_end")], *images[int(cols["image"][q])].shape[:2])
             for q in range(n)]
    tab = np.zeros(n, dtype=OVERLAY_ROW_DTYPE)
    tab["variant"] = VARIANTS[variant]
    tab["map_index"] = -1
    img_at = np.cumsum([0] + [I.numel() for I in images[:-1]])
    mx = None
    if variant == "image":
        for b, (I, m) in enumerate(zip(images, maps)):
            if m.shape[0] > I.shape[0] or m.shape[1] > I.shape[1]:
                raise ValueError(f"overlay: the {tuple(m.shape)} map overhangs the {tuple(I.shape[:2])} image {b}")
        used = sorted(set(int(b) for b in cols["image"]))
        filtered = dict(zip(used, gaussian_filter([maps[b] for b in used], sigma, "clamp")))
        row_maps = [filtered[int(b)] for b in cols["image"]]
    elif variant == "crop":
        live, crops = [], []
        for q, box in enumerate(boxes):
            m = maps[int(cols["image"][q])]
            if box[2] > m.shape[0] or box[3] > m.shape[1]:
                raise ValueError(f"overlay: box {box} of row {q} leaves its {tuple(m.shape)} map")
            if box[2] > box[0] and box[3] > box[1]:
                live.append(q)
                crops.append(m[box[0]:box[2], box[1]:box[3]].contiguous())
        row_maps = [None] * n
        if live:
            got, mx = gaussian_filter(crops, sigma, "unit", return_max=True)
            for j, q in enumerate(live):
                row_maps[q] = got[j]
                tab["map_index"][q] = j
    else:
        row_maps = [m.to(dev, torch.float32) for m in maps]
        for q, (m, box) in enumerate(zip(row_maps, boxes)):
            if tuple(m.shape) != (box[2] - box[0], box[3] - box[1]):
                raise ValueError(f"overlay: stored T {tuple(m.shape)} of row {q} is not its box {box}")
    present = [m for m in row_maps if m is not None and m.numel()]
    if present:
        map_buf, map_at, _ = UNetEngine._place_maps(torch, present, dev)
    else:
        map_buf, map_at = torch.zeros(1, dtype=torch.float32, device=dev), []
    at, px = 0, 0
    for q, (box, m) in enumerate(zip(boxes, row_maps)):
        I = images[int(cols["image"][q])]
        t = tab[q]
        t["image_offset"], t["img_h"], t["img_w"] = img_at[int(cols["image"][q])], I.shape[0], I.shape[1]
        t["x_start"], t["y_start"], t["x_end"], t["y_end"] = box
        if m is not None and m.numel():
            t["map_offset"], t["map_h"], t["map_w"] = map_at[at], m.shape[0], m.shape[1]
            at += 1
            if variant != "image":
                t["map_x0"], t["map_y0"] = box[0], box[1]
        t["out_offset"], t["alpha_offset"] = 3 * px, px
        px += (box[2] - box[0]) * (box[3] - box[1])
    img_buf = torch.cat([I.contiguous().reshape(-1) for I in images])
    tab_d = torch.from_numpy(tab.view(np.uint8)).to(dev)
    blended = torch.empty(max(3 * px, 1), dtype=torch.uint8, device=dev)
    plain = torch.empty(max(3 * px, 1), dtype=torch.uint8, device=dev)
    alpha = torch.empty(max(px, 1), dtype=torch.float32, device=dev) if want_alpha else None
    lum = torch.empty(n, dtype=torch.int64, device=dev)
    verdict = torch.empty(n, dtype=torch.int32, device=dev)
    degenerate = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_overlay_blend(_p(img_buf), img_buf.numel(), _p(map_buf), map_buf.numel(), _p(mx), 0 if mx is None else mx.numel(),
                                     _p(tab_d), n, _p(blended), _p(plain), blended.numel(), _p(alpha), 0 if alpha is None else alpha.numel(),
                                     _p(lum), _p(verdict), _p(degenerate), _stream(torch, dev))
    if rc:
        raise EngineError(f"dm_overlay_blend: {'bad argument' if rc == 1 else 'HIP error'} (code {rc})")
    out = {"blended": [], "plain": [], "alpha": [] if want_alpha else None, "lum_sum": lum, "verdict": verdict != 0,
           "degenerate": degenerate != 0}
    for t in tab:
        bh, bw, o = int(t["x_end"] - t["x_start"]), int(t["y_end"] - t["y_start"]), int(t["out_offset"])
        out["blended"].append(blended[o:o + 3 * bh * bw].view(bh, bw, 3))
        out["plain"].append(plain[o:o + 3 * bh * bw].view(bh, bw, 3))
        if want_alpha:
            out["alpha"].append(alpha[o // 3:o // 3 + bh * bw].view(bh, bw))
    return out
