"""The CLIP baseline's patch mining (clipmining/ranking.py:72-108 `CLIPRankCluster.dot_text_image`, clipmining/utils.py:75-94) from
the token grid, on the GPU.  Kernels: csrc/clipmine.hip; C ABI: dm_clipmine_workspace_bytes / dm_clipmine_rank; DESIGN.md 4u.

Per image the reference upsamples the 2-channel text-score grid and all E token channels bilinearly from gh x pw to H x W, pools the
scores with a kx x ky window, keeps `topk(100 k_per_image)` positions, runs `get_non_overlapping` on them and averages the upsampled
features over each winner's box.  Upsampling, pooling and the box mean are linear and separable: with

    A[i][p] = mean over image rows i ... i+kx-1 of the bilinear row weights onto token row p        (`axis_weights`; B for columns)

the pooled map of a channel X [gh][pw] is A X B^T, and so is a box's feature per channel.  The upsampled tensors never exist.

The five steps, which `rank_patches_host` (numpy, float64 inside) and the kernels share:

  1. scores       s[p][q][c] = sum_e text[c][e] tokens[pq][e] / |tokens[pq]|_2       (tokens as given, not normalised; text as given)
  2. map          m_c = A s[..c] B^T; D = m_0 - m_1 (mode 'diff') or m_0 ('sim'); candidate (i, j) = box (i, j, i+kx, j+ky), x = ROWS
  3. eligibility  only the n = min(100 k_per_image, OH OW) candidates of largest D are candidates at all.  Among equal values the
                  lowest row-major index ranks first (torch.topk leaves ties undefined).  A NaN is never a candidate — torch.topk
                  would rank it HIGHEST; non-finite tokens are outside the pinned contract.
  4. selection    up to k_per_image times: the best eligible candidate still alive wins and every candidate with |i-i*| <= kx and
                  |j-j*| <= ky dies (inclusive); stop when no eligible candidate is alive.  On a smooth map the eligible ones crowd
                  around the peak, so an image often yields fewer than k_per_image boxes — that is the reference's behaviour.
  5. features     f[e] = sum_p sum_q A[i][p] B[j][q] tokens[pq][e], then f / |f|_2

The tower that makes the tokens is on the fp32 net: `rank_images` runs the baseline from pixels — `center_crop`, the device
preprocessing and StreetCLIP's ViT-L/14-336 image tower (`UNetEngineF32.clip_image_tokens`: 577 tokens, hidden 1024, `post_layernorm` and
`visual_projection` on the patch tokens), `clip_text_embeds` for the two prompts, then `rank_device` on tensors that never leave the GPU.
Callers that already hold `tokens` and `text` (e.g. from `transformers`) use `rank_patches`.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from .engine import MINE_MAX_K, EngineError, _p, load_library as _lib

CLIPMINE_MAX_GRID = 1024         # DM_CLIPMINE_MAX_GRID
MODES = {"diff": 0, "sim": 1}    # DM_CLIPMINE_DIFF / DM_CLIPMINE_SIM
# dm_clipmine_desc of include/dm_engine.h (64 bytes)
CLIPMINE_DESC_DTYPE = np.dtype([("token_offset", "<i8"), ("a_offset", "<i8"), ("b_offset", "<i8"), ("work_offset", "<i8"),
                                ("map_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("gh", "<i4"), ("pw", "<i4"), ("P", "<i4"),
                                ("reserved", "<i4")])
# dm_clipmine_rank return codes (include/dm_engine.h)
ERRORS = {1: "null argument", 2: "n_images outside [1, 65535]", 3: "E < 1", 4: f"k_per_image outside [1, {MINE_MAX_K}]", 5: "unknown mode",
          6: "window larger than an image, with exactly one side 1, or too many candidates",
          7: f"P != gh * pw or a grid side outside [1, {CLIPMINE_MAX_GRID}]", 8: "negative offset", 9: "workspace too small",
          10: "HIP error"}
COLUMNS = ("image", "x_start", "y_start", "x_end", "y_end", "D")


# ------------------------------------------------------------------------------------------------------------------------------
# tables and argument checks (shared by the host restatement and the device entry)
# ------------------------------------------------------------------------------------------------------------------------------
def axis_weights(out: int, n_in: int, window: int) -> np.ndarray:
    """float64 [out - window + 1][n_in]: row i = the mean over output positions i ... i+window-1 of the weights with which
    `interpolate(mode='bilinear', align_corners=False)` reads the n_in inputs along one axis (source index
    max((d + 0.5) n_in / out - 0.5, 0), the upper neighbour clamped to n_in - 1).  Every row sums to 1."""
    out, n_in, window = int(out), int(n_in), int(window)
    if n_in < 1 or window < 1 or window > out:
        raise ValueError(f"axis_weights: out {out}, n_in {n_in}, window {window}")
    src = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (n_in / out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    w = np.zeros((out, n_in), dtype=np.float64)
    np.add.at(w, (np.arange(out), i0), 1.0 - l1)
    np.add.at(w, (np.arange(out), i1), l1)
    return np.lib.stride_tricks.sliding_window_view(w, window, axis=0).sum(axis=-1) / window


@functools.lru_cache(maxsize=64)
def _axis_weights_f32(out: int, n_in: int, window: int) -> np.ndarray:
    """`axis_weights` rounded to fp32 once per distinct (size, grid, window) — what the kernels read."""
    t = np.ascontiguousarray(axis_weights(out, n_in, window), dtype=np.float32).reshape(-1)
    t.setflags(write=False)
    return t


def _check_args(n_tokens, E, image_sizes, pw, k_per_image, kx, ky, mode):
    """Everything dm_clipmine_rank refuses, as ValueError.  Returns the per-image (H, W, gh, pw)."""
    n = len(n_tokens)
    if n < 1:
        raise ValueError("clipmine: no images")
    if len(image_sizes) != n:
        raise ValueError(f"clipmine: {n} token grids but {len(image_sizes)} image sizes")
    if mode not in MODES:
        raise ValueError(f"clipmine: mode {mode!r}, expected 'diff' or 'sim'")
    if int(E) < 1:
        raise ValueError("clipmine: E < 1")
    if not 1 <= int(k_per_image) <= MINE_MAX_K:
        raise ValueError(f"clipmine: k_per_image {k_per_image} outside [1, {MINE_MAX_K}]")
    kx, ky = int(kx), int(ky)
    if kx < 1 or ky < 1 or (kx == 1) != (ky == 1):          # `pool` (utils.py:75-81) skips a window with one side 1
        raise ValueError(f"clipmine: window {kx}x{ky}: sides must be >= 1, and one side 1 with the other not is not a frame the reference can mine")
    pws = [int(pw)] * n if np.isscalar(pw) else [int(v) for v in pw]
    if len(pws) != n:
        raise ValueError(f"clipmine: {n} token grids but {len(pws)} grid widths")
    geo = []
    for b, (P, (H, W), q) in enumerate(zip(n_tokens, image_sizes, pws)):
        H, W, P = int(H), int(W), int(P)
        if q < 1 or P < 1 or P % q != 0:
            raise ValueError(f"clipmine: image {b}: {P} tokens are not rows of {q}")
        if q > CLIPMINE_MAX_GRID or P // q > CLIPMINE_MAX_GRID:
            raise ValueError(f"clipmine: image {b}: grid {P // q}x{q} has a side above {CLIPMINE_MAX_GRID}")
        if kx > H or ky > W:
            raise ValueError(f"clipmine: image {b}: window {kx}x{ky} larger than the image {H}x{W}")
        if (H - kx + 1) * (W - ky + 1) >= 1 << 30:
            raise ValueError(f"clipmine: image {b}: {H}x{W} has 2^30 or more candidates")
        geo.append((H, W, P // q, q))
    return geo


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _select_host(D, kx, ky, k_per_image, n_elig=None, eligible=None):
    """Steps 3 and 4 on a float64 map.  `eligible` (a boolean map) replaces the rank rule — the fixture's boundary check."""
    OH, OW = D.shape
    flat = D.reshape(-1)
    order = np.argsort(-flat, kind="stable")                 # descending, the lowest index first among equals, NaN last
    order = order[~np.isnan(flat[order])]
    order = order[:n_elig] if eligible is None else order[eligible.reshape(-1)[order]]
    alive = np.ones(len(order), dtype=bool)
    oi, oj = order // OW, order % OW
    boxes = []
    while len(boxes) < k_per_image and alive.any():
        w = int(np.argmax(alive))
        i, j = int(oi[w]), int(oj[w])
        boxes.append((i, j, i + kx, j + ky))
        alive &= ~((np.abs(oi - i) <= kx) & (np.abs(oj - j) <= ky))
    return np.array(boxes, dtype=np.int32).reshape(-1, 4)


def _image_host(tokens, text, H, W, gh, pw, k_per_image, kx, ky, mode):
    t = np.asarray(tokens, dtype=np.float64)
    E = t.shape[1]
    s = (t / np.sqrt((t * t).sum(axis=1, keepdims=True))) @ np.asarray(text, dtype=np.float64).T          # 1. [P][2]
    A, B = axis_weights(H, gh, kx), axis_weights(W, pw, ky)
    m = [A @ s[:, c].reshape(gh, pw) @ B.T for c in range(2)]                                                # 2.
    D = m[0] - m[1] if mode == "diff" else m[0]
    boxes = _select_host(D, kx, ky, k_per_image, min(100 * k_per_image, D.size))                            # 3. 4.
    grid = t.reshape(gh, pw, E)
    feats = np.empty((len(boxes), E), dtype=np.float64)
    for r, (i, j, _, _) in enumerate(boxes):                                                                 # 5.
        f = np.einsum("p,q,pqe->e", A[i], B[j], grid)
        feats[r] = f / np.sqrt((f * f).sum())
    return boxes, D, feats


def _rows(image, boxes, D):
    rows = {"image": np.asarray(image, dtype=np.int64)}
    for c, name in enumerate(("x_start", "y_start", "x_end", "y_end")):
        rows[name] = np.ascontiguousarray(boxes[:, c], dtype=np.int32)
    rows["D"] = np.asarray(D, dtype=np.float32)
    return rows


def rank_patches_host(tokens, text, image_sizes, pw=24, k_per_image=5, kx=64, ky=64, mode="diff", return_maps=False):
    """The five steps of the module's docstring in numpy, float64 inside: the restatement that pins the rules.  tokens: per image
    [P, E]; text [2, E]; image_sizes: per image (H, W); pw: the grid width, one for all images or one per image.  Returns (rows,
    features): rows = the reference's columns as numpy arrays (image int64, x_start, y_start, x_end, y_end int32 with x = rows, D
    fp32), image order then round order; features float64 [rows, E].  return_maps adds the list of float64 maps [OH, OW]."""
    tokens = [np.asarray(t) for t in tokens]
    text = np.asarray(text)
    if any(t.ndim != 2 for t in tokens) or text.ndim != 2 or text.shape[0] != 2:
        raise ValueError("clipmine: tokens must be [P, E] per image and text [2, E]")
    E = text.shape[1]
    if any(t.shape[1] != E for t in tokens):
        raise ValueError(f"clipmine: tokens of width {[t.shape[1] for t in tokens]} against text of width {E}")
    geo = _check_args([t.shape[0] for t in tokens], E, image_sizes, pw, k_per_image, kx, ky, mode)
    image, boxes, Ds, feats, maps = [], [], [], [], []
    for b, (t, (H, W, gh, q)) in enumerate(zip(tokens, geo)):
        bx, D, f = _image_host(t, text, H, W, gh, q, int(k_per_image), int(kx), int(ky), mode)
        image += [b] * len(bx)
        boxes.append(bx)
        Ds.append(D[bx[:, 0], bx[:, 1]])
        feats.append(f)
        maps.append(D)
    out = (_rows(image, np.concatenate(boxes), np.concatenate(Ds)), np.concatenate(feats))
    return out + (maps,) if return_maps else out


# ------------------------------------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------------------------------------
def _round64(n):
    return (int(n) + 63) // 64 * 64


def plan_call(geo, E, kx, ky):
    """The host half of one dm_clipmine_rank call for images of geometry `geo` = [(H, W, gh, pw), ...] whose tokens are packed one
    after the other: (desc table, fp32 weight tables in one array, workspace bytes, map floats).  A distinct (size, grid, window)
    table appears once."""
    n = len(geo)
    desc = np.zeros(n, dtype=CLIPMINE_DESC_DTYPE)
    parts, where, at = [], {}, 0

    def table(key):
        nonlocal at
        if key not in where:
            t = _axis_weights_f32(*key)
            where[key] = at
            parts.append(t)
            at += t.size
        return where[key]

    tok = work = maps = 0
    for b, (H, W, gh, pw) in enumerate(geo):
        cands = (H - kx + 1) * (W - ky + 1)
        desc[b] = (tok, table((H, gh, kx)), table((W, pw, ky)), work, maps, H, W, gh, pw, gh * pw, 0)
        tok += gh * pw * E
        work += _round64(2 * gh * pw + cands)
        maps += cands
    need = _lib().dm_clipmine_workspace_bytes(n, int(desc["P"].astype(np.int64).sum()), maps)
    if not need or need < work * 4:
        raise EngineError(f"dm_clipmine_workspace_bytes: {need} bytes for {n} images")
    return desc, np.concatenate(parts), need, maps


def rank_device(tokens, text, image_sizes, pw=24, k_per_image=5, kx=64, ky=64, mode="diff", return_maps=False):
    """ONE dm_clipmine_rank call on the device the tokens live on.  Arguments as `rank_patches`.  Returns device tensors (boxes
    int32 [n, k, 4], D fp32 [n, k], count int32 [n], feats fp32 [n, k, E]); slots past count[b] hold -1 / NaN.  return_maps adds
    the list of maps [OH_b, OW_b] fp32 (views of one buffer)."""
    import torch
    tokens = list(tokens)
    if not tokens or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tokens) or not (isinstance(text, torch.Tensor) and text.is_cuda):
        raise EngineError("rank_device: tokens and text must be torch tensors on the GPU (rank_patches_host is the numpy restatement)")
    if any(t.dim() != 2 for t in tokens) or text.dim() != 2 or text.shape[0] != 2:
        raise ValueError("clipmine: tokens must be [P, E] per image and text [2, E]")
    E = int(text.shape[1])
    if any(t.shape[1] != E for t in tokens):
        raise ValueError(f"clipmine: tokens of width {[int(t.shape[1]) for t in tokens]} against text of width {E}")
    geo = _check_args([t.shape[0] for t in tokens], E, image_sizes, pw, k_per_image, kx, ky, mode)
    kx, ky, k, n = int(kx), int(ky), int(k_per_image), len(tokens)
    dev = tokens[0].device
    desc, tables, need, map_floats = plan_call(geo, E, kx, ky)
    packed = tokens[0].to(torch.float32).contiguous() if n == 1 else torch.cat([t.to(dev, torch.float32).reshape(-1) for t in tokens])
    text = text.to(dev, torch.float32).contiguous()
    up = torch.from_numpy(np.concatenate([tables.view(np.uint8), desc.view(np.uint8)])).to(dev)              # both tables in one upload
    tables_d, desc_d = up[:tables.nbytes], up[tables.nbytes:]
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    maps = torch.empty(map_floats, dtype=torch.float32, device=dev) if return_maps else None
    boxes = torch.empty((n, k, 4), dtype=torch.int32, device=dev)
    d = torch.empty((n, k), dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    feats = torch.empty((n, k, E), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_clipmine_rank(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _p(packed), _p(text), E, _p(desc_d), n,
                                     _p(tables_d), kx, ky, k, MODES[mode], _p(work), need, _p(maps), _p(boxes), _p(d), _p(count),
                                     _p(feats))
    if rc:
        raise EngineError(f"dm_clipmine_rank: {ERRORS.get(rc, 'error')} (code {rc})")
    out = (boxes, d, count, feats)
    if return_maps:
        out += ([maps[int(r["map_offset"]):int(r["map_offset"]) + (int(r["H"]) - kx + 1) * (int(r["W"]) - ky + 1)]
                 .view(int(r["H"]) - kx + 1, int(r["W"]) - ky + 1) for r in desc],)
    return out


def rank_patches(tokens, text, image_sizes, pw=24, k_per_image=5, kx=64, ky=64, mode="diff", images_per_call=64, return_maps=False):
    """`CLIPRankCluster.dot_text_image` (ranking.py:72-108) for a list of images, without the upsampled tensors (module docstring).

    tokens: per image the projected patch tokens [P_b, E] (a list; grids and image sizes may differ per image — or one [n, P, E]
    tensor); text [2, E] = the embeddings of [category, ""], used as given; image_sizes: per image (H, W); pw: the grid width, one
    number or one per image; mode 'diff' or 'sim'.  GPU tensors go through dm_clipmine_rank in calls of `images_per_call` images (a
    call's results do not depend on what else is in it); numpy arrays and CPU tensors take `rank_patches_host`.

    Returns (rows, features): rows = the reference's columns as numpy arrays — image (int64 index into the input list), x_start,
    y_start, x_end, y_end (int32, x = rows), D (fp32) — image order then round order, fewer than k_per_image rows for an image
    that ran out of eligible candidates; features [rows, E]: fp32 on the tokens' device for GPU input, float64 numpy otherwise.
    return_maps adds the list of per-image maps D [OH, OW]."""
    import torch
    tokens = list(tokens)
    if not (len(tokens) and all(isinstance(t, torch.Tensor) and t.is_cuda for t in tokens)):
        host = [t.numpy() if isinstance(t, torch.Tensor) else t for t in tokens]
        return rank_patches_host(host, text.cpu().numpy() if isinstance(text, torch.Tensor) else text, image_sizes, pw, k_per_image,
                                 kx, ky, mode, return_maps)
    n = len(tokens)
    if len(image_sizes) != n:
        raise ValueError(f"clipmine: {n} token grids but {len(image_sizes)} image sizes")
    if int(images_per_call) < 1:
        raise ValueError("clipmine: images_per_call < 1")
    text = torch.as_tensor(text).to(tokens[0].device)
    pws = [int(pw)] * n if np.isscalar(pw) else list(pw)
    image, boxes, Ds, feats, maps = [], [], [], [], []
    for c0 in range(0, n, int(images_per_call)):
        c1 = min(n, c0 + int(images_per_call))
        got = rank_device(tokens[c0:c1], text, image_sizes[c0:c1], pws[c0:c1], k_per_image, kx, ky, mode, return_maps)
        bx, d, count = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
        keep = np.arange(bx.shape[1])[None, :] < count[:, None]                          # [images, k], row-major = the row order
        image.append(np.repeat(np.arange(c0, c1), count))
        boxes.append(bx[keep])
        Ds.append(d[keep])
        feats.append(got[3][torch.from_numpy(keep).to(got[3].device)])
        if return_maps:
            maps += got[4]
    out = (_rows(np.concatenate(image), np.concatenate(boxes), np.concatenate(Ds)), torch.cat(feats))
    return out + (maps,) if return_maps else out


def center_crop(image, size: int = 512) -> np.ndarray:
    """torchvision's `CenterCrop(size)` (ranking.py:60) of a uint8 HWC image (or PIL image) at least `size` on both sides:
    top = int(round((H - size) / 2.0)), left likewise, with Python's rounding (halves to even: 513 -> 0, 515 -> 2).  A smaller image
    raises ValueError (torchvision would zero-pad it, which the reference's 512-px dataset never needs)."""
    from .resample import check_clip_image
    img = check_clip_image(image)
    H, W = img.shape[:2]
    size = int(size)
    if size < 1 or H < size or W < size:
        raise ValueError(f"center_crop: image {H}x{W} is smaller than the crop {size}x{size}")
    top, left = int(round((H - size) / 2.0)), int(round((W - size) / 2.0))
    return np.ascontiguousarray(img[top:top + size, left:left + size])


def rank_images(net, images, input_ids, k_per_image=5, kx=64, ky=64, mode="diff", images_per_call=64, return_maps=False):
    """The CLIP baseline from pixels (ranking.py:58-70, 110-125) on `net`, a `UNetEngineF32` holding the image tower
    (load_clip_tower_state_dict) and the text tower with its projection (load_clip_state_dict): images = square uint8 HWC arrays /
    PIL images (the reference's `center_crop(image, 512)`); input_ids [2, 77] = the tokenised [category, ""].  Device preprocessing
    -> tower -> patch tokens (clip_image_tokens), the normalised text embeddings once (clip_text_embeds), then `rank_device` per
    `images_per_call` images on tensors that never leave the GPU; (H, W) = each image's own size, the grid = the tower's.
    Returns what `rank_patches` returns."""
    import torch
    from .resample import check_clip_tower_image
    imgs = [check_clip_tower_image(a) for a in images]
    if not imgs:
        raise ValueError("clipmine: no images")
    if int(images_per_call) < 1:
        raise ValueError("clipmine: images_per_call < 1")
    text = net.clip_text_embeds(input_ids, normalize=True)
    if text.shape[0] != 2:
        raise ValueError(f"clipmine: input_ids must hold the two prompts [category, \"\"], got {text.shape[0]} rows")
    n = len(imgs)
    image, boxes, Ds, feats, maps = [], [], [], [], []
    for c0 in range(0, n, int(images_per_call)):
        c1 = min(n, c0 + int(images_per_call))
        tokens = net.clip_image_tokens(imgs[c0:c1])                                     # [m, G^2, E]
        pw = int(round(tokens.shape[1] ** 0.5))
        got = rank_device(list(tokens), text, [a.shape[:2] for a in imgs[c0:c1]], pw, k_per_image, kx, ky, mode, return_maps)
        bx, d, count = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
        keep = np.arange(bx.shape[1])[None, :] < count[:, None]
        image.append(np.repeat(np.arange(c0, c1), count))
        boxes.append(bx[keep])
        Ds.append(d[keep])
        feats.append(got[3][torch.from_numpy(keep).to(got[3].device)])
        if return_maps:
            maps += got[4]
    out = (_rows(np.concatenate(image), np.concatenate(boxes), np.concatenate(Ds)), torch.cat(feats))
    return out + (maps,) if return_maps else out


def rank_and_cluster(rows, feats, k: int = 1000, num_clusters: int = 32):
    """`CLIPRankCluster.clustering`'s data path for one category (ranking.py:166-172, 131-149): `get_top_k(df, key='D', k=k)`, then
    KMeans(num_clusters, random_state=10) on those rows' features, members ordered by distance to their centre, clusters by the
    median D.  rows, feats: `rank_patches`' result.  Returns (top, clusters): top = the k best rows in order, with `index` = their
    row in `rows`; clusters = `clustering.cluster_patches`' dict, its row ids counting into `top`.  Device features stay on the
    device."""
    from . import clustering
    from .typicality import TypicalityScorer
    n = len(rows["D"])
    if feats.shape[0] != n:
        raise ValueError(f"clipmine: {n} rows but {feats.shape[0]} features")
    top = TypicalityScorer.top_k(dict(rows, index=np.arange(n)), k)
    sel = feats[top["index"]] if isinstance(feats, np.ndarray) else feats[np.asarray(top["index"]).tolist()]
    return top, clustering.cluster_patches(sel, top["D"], num_clusters, aggregate="median", order_by="centroid")
