"""The X-ray application's two numbers (diffmining/applications/xray/compute.py:263-284) from heat-maps that stay on the GPU: the
mean of the per-pixel map inside the radiologist's box (`mean_typicallity`, report.json) and the area under the precision-recall
curve over 1000 thresholds (`aucpr`, auc.json).  Kernels: csrc/xray_eval.hip; C ABI: dm_xray_eval_workspace_bytes / dm_xray_eval.

`aucpr` compares every pixel with every threshold (a T x H W boolean array).  The thresholds `2 * 10 ** -linspace(2, 7, 1000)`
decrease strictly, so with bin(v) = the number of thresholds >= v = the first k with thr[k] < v,

    tp[k] = #{inside the box, v > thr[k]} = sum_{b <= k} hist_in[b]          fp[k] the same outside the box

— one pass and two histograms of T + 1 bins.  The rules, which `xray_counts_host` (numpy) and the kernel share:

  compare   the reference's: fp32 pixel against fp64 threshold, in fp64, strictly `>`.  (An fp32 comparison counts a pixel that
            sits at float32(thr[k]) differently.)  A NaN pixel exceeds nothing (bin T); +inf exceeds everything (bin 0).
  box       (x1, y1, x2, y2) selects dm[y1:y2, x1:x2]: x = COLUMNS (the mining entries have x = rows).  A box that runs past
            the map is clipped as numpy clips a slice, and may be empty.  Negative coordinates are refused (numpy would count
            them from the end; the data set has none).
  limits    1 <= T <= 4096 thresholds, strictly decreasing, no NaN; H, W >= 1; H W < 2^24 (the reference's recall divides by
            `x.sum()`, an fp32 sum of ones).

The counts are integers, so device and host agree exactly; the last four lines of `aucpr` run on the host in the reference's own
expressions (`xray_scores_from_counts`), which makes the AUC bit-equal to the reference's.  The box mean is float32(fp64 sum / n).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import random
import warnings

import numpy as np

from .engine import EngineError, UNetEngine, _p, load_library as _lib

XRAY_MAX_THRESHOLDS = 4096       # DM_XRAY_MAX_THRESHOLDS
XRAY_MAX_PIXELS = 1 << 24        # H W >= 2^24 is refused
# dm_xray_desc of include/dm_engine.h (32 bytes)
XRAY_DESC_DTYPE = np.dtype([("map_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
# dm_xray_eval return codes (include/dm_engine.h)
ERRORS = {1: "null argument", 2: "n_rows < 1", 3: f"n_thresholds outside [1, {XRAY_MAX_THRESHOLDS}]",
          4: "thresholds must decrease strictly and hold no NaN", 5: "H or W < 1", 6: "H W >= 2^24", 7: "negative box coordinate",
          8: "HIP error"}


def xray_thresholds() -> np.ndarray:
    """The reference's table (compute.py:268), float64 [1000], taken with numpy so that the bits are numpy's."""
    return 2 * 10 ** (-np.linspace(2, 7, 1000))


def _check_thresholds(thresholds) -> np.ndarray:
    thr = np.ascontiguousarray(xray_thresholds() if thresholds is None else thresholds, dtype=np.float64)
    if thr.ndim != 1 or not 1 <= thr.size <= XRAY_MAX_THRESHOLDS:
        raise ValueError(f"xray: {thr.shape} thresholds, need 1 ... {XRAY_MAX_THRESHOLDS} in one dimension")
    if np.isnan(thr).any() or not (thr[1:] < thr[:-1]).all():
        raise ValueError("xray: thresholds must decrease strictly and hold no NaN")
    return thr


def _check_row(b, H, W, box):
    if H < 1 or W < 1:
        raise ValueError(f"xray: map {b} is {H}x{W}")
    if H * W >= XRAY_MAX_PIXELS:
        raise ValueError(f"xray: map {b} has {H * W} pixels, 2^24 or more (the reference's x.sum() is an fp32 sum of ones)")
    if len(box) != 4:
        raise ValueError(f"xray: box {b} must be (x1, y1, x2, y2), got {box!r}")
    box = tuple(int(v) for v in box)
    if min(box) < 0:
        raise ValueError(f"xray: box {b} {box} has a negative coordinate (numpy would count it from the end)")
    return box


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement: the CPU-tier yardstick, and the path a numpy input takes
# ------------------------------------------------------------------------------------------------------------------------------
def xray_counts_host(maps, boxes, thresholds=None):
    """maps: a list of [H, W] arrays; boxes: per map (x1, y1, x2, y2).  Returns (tp int32 [n, T], fp int32 [n, T], n_in int32 [n],
    box_sum float64 [n]) by the rules at the top of this module; box_sum is numpy's float64 sum of the box."""
    thr = _check_thresholds(thresholds)
    if len(maps) != len(boxes) or len(maps) < 1:
        raise ValueError(f"xray: {len(maps)} maps but {len(boxes)} boxes")
    T, n = thr.size, len(maps)
    tp, fp = np.zeros((n, T), dtype=np.int32), np.zeros((n, T), dtype=np.int32)
    n_in, box_sum = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
    neg = -thr                                                        # ascending
    for b, (dm, box) in enumerate(zip(maps, boxes)):
        dm = np.asarray(dm)
        if dm.ndim != 2:
            raise ValueError(f"xray: map {b} must be [H, W], got {dm.shape}")
        dm = dm.astype(np.float32, copy=False)
        x1, y1, x2, y2 = _check_row(b, dm.shape[0], dm.shape[1], box)
        inside = np.zeros(dm.shape, dtype=bool)
        inside[y1:y2, x1:x2] = True
        # the number of thresholds >= v: thr[k] >= v  <=>  -thr[k] <= -v; a NaN sorts after everything -> T
        bins = np.searchsorted(neg, -dm.astype(np.float64).ravel(), side="right")
        m = inside.ravel()
        tp[b] = np.cumsum(np.bincount(bins[m], minlength=T + 1))[:T]
        fp[b] = np.cumsum(np.bincount(bins[~m], minlength=T + 1))[:T]
        n_in[b] = int(m.sum())
        box_sum[b] = dm[y1:y2, x1:x2].astype(np.float64).sum()
    return tp, fp, n_in, box_sum


def _trapz(y, x):
    if not hasattr(np, "trapz"):
        return np.trapezoid(y, x)
    with warnings.catch_warnings():                  # numpy 2 keeps `trapz` as a deprecated name of `trapezoid`
        warnings.simplefilter("ignore", DeprecationWarning)
        return np.trapz(y, x)


def xray_scores_from_counts(tp, fp, n_in, box_sum):
    """The reference's own last lines (compute.py:279-284, :264) from the counts of `xray_eval` / `xray_counts_host` (arrays or
    tensors, one row [T] or a batch [n, T]).  Returns (mean_typicality float32, auc float64), scalars or [n].  An empty box
    gives NaN for both, as the reference does (0 / 0)."""
    host = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)          # noqa: E731
    tp, fp, n_in, box_sum = host(tp).astype(np.int64), host(fp).astype(np.int64), host(n_in), host(box_sum).astype(np.float64)
    single = tp.ndim == 1
    tp, fp, n_in, box_sum = np.atleast_2d(tp), np.atleast_2d(fp), np.atleast_1d(n_in), np.atleast_1d(box_sum)
    mean = np.empty(len(tp), dtype=np.float32)
    auc = np.empty(len(tp), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(len(tp)):
            denominator = tp[b] + fp[b]
            precision = np.where(denominator > 0, tp[b] / denominator, 0)
            recall = tp[b] / np.float32(n_in[b])                     # x.sum() of a float32 array of ones: exact below 2^24
            auc[b] = _trapz(precision, recall)
            mean[b] = np.float32(box_sum[b] / np.float64(n_in[b]))
    return (mean[0], auc[0]) if single else (mean, auc)


# ------------------------------------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------------------------------------
def workspace_bytes(n_rows: int, n_thresholds: int, max_pixels: int) -> int:
    need = _lib().dm_xray_eval_workspace_bytes(int(n_rows), int(n_thresholds), int(max_pixels))
    if not need:
        raise ValueError(f"xray: no workspace for {n_rows} rows, {n_thresholds} thresholds, {max_pixels} pixels")
    return need


def xray_eval(maps, boxes, thresholds=None, work=None):
    """The counts of `aucpr` and the box sums for a batch of heat-maps in ONE call (dm_xray_eval), on the device the maps live on.
    maps: a list of fp32 [H, W] torch tensors on the GPU, sizes free; contiguous views of one buffer (`typicality_image_batched`'s
    output) are read where they lie, and one map may appear under several boxes (one image, two findings).  boxes: per map
    (x1, y1, x2, y2) with x = columns.  thresholds: float64, strictly decreasing (default `xray_thresholds()`); the table is built
    with numpy and uploaded once.  work: a uint8 workspace of at least `workspace_bytes(n, T, max H W)` to reuse (its contents do
    not matter).  Returns device tensors (tp int32 [n, T], fp int32 [n, T], n_in int32 [n], box_sum float64 [n]); bit-reproducible.
    A list of numpy arrays takes `xray_counts_host` and returns numpy arrays; anything else that is not on a GPU raises."""
    import torch
    if len(maps) and all(isinstance(m, np.ndarray) for m in maps):
        return xray_counts_host(maps, boxes, thresholds)
    thr = _check_thresholds(thresholds)
    if len(maps) != len(boxes) or len(maps) < 1:
        raise ValueError(f"xray: {len(maps)} maps but {len(boxes)} boxes")
    if not all(isinstance(m, torch.Tensor) and m.is_cuda for m in maps):
        raise EngineError("xray_eval: maps must be torch tensors on the GPU (xray_counts_host is the numpy restatement)")
    dev = maps[0].device
    n, T = len(maps), thr.size
    desc = np.zeros(n, dtype=XRAY_DESC_DTYPE)
    for b, (m, box) in enumerate(zip(maps, boxes)):
        if m.dim() != 2:
            raise ValueError(f"xray: map {b} must be [H, W], got {tuple(m.shape)}")
        desc[b]["H"], desc[b]["W"] = m.shape
        desc[b]["x1"], desc[b]["y1"], desc[b]["x2"], desc[b]["y2"] = _check_row(b, m.shape[0], m.shape[1], box)
    packed, offsets, _ = UNetEngine._place_maps(torch, list(maps), dev)
    desc["map_offset"] = offsets
    need = workspace_bytes(n, T, int((desc["H"].astype(np.int64) * desc["W"]).max()))
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    elif work.numel() * work.element_size() < need:
        raise ValueError(f"xray: workspace of {work.numel() * work.element_size()} bytes, {need} needed")
    up = torch.from_numpy(np.concatenate([thr.view(np.uint8), desc.view(np.uint8)])).to(dev)          # both tables in one upload
    thr_d, desc_d = up[:thr.nbytes], up[thr.nbytes:]
    tp = torch.empty((n, T), dtype=torch.int32, device=dev)
    fp = torch.empty((n, T), dtype=torch.int32, device=dev)
    n_in = torch.empty(n, dtype=torch.int32, device=dev)
    box_sum = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_xray_eval(_p(packed), _p(desc_d), n, _p(thr_d), T, _p(work), _p(tp), _p(fp), _p(n_in), _p(box_sum),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc:
        raise EngineError(f"dm_xray_eval: {ERRORS.get(rc, 'error')} (code {rc})")
    return tp, fp, n_in, box_sum


# ------------------------------------------------------------------------------------------------------------------------------
# the application's bookkeeping: `load_paths` (compute.py:170-205) and `compare_json_files` (:350-389)
# ------------------------------------------------------------------------------------------------------------------------------
def load_boxes(metadata_rows, bbox_rows, diseases, seed: int = 42, image_folder: str = ""):
    """`load_paths` without pandas.  metadata_rows: (fname, label) per line of metadata.csv ('Image Index', 'Finding Labels'; the
    labels of an image joined by '|'); bbox_rows: (fname, label, x, y, w, h) per line of BBox_List_2017.csv.  Returns the
    reference's `parent`: {finding: [(join(image_folder, fname), (x1, y1, x2, y2)), ...]} with every box halved by `int(v / 2)`
    (the images are scored at half size) and each finding's list ordered by (number of labels of the image, random.random())
    under `random.seed(seed)`.  A later box of the same (fname, label) replaces an earlier one; only images that have a box are
    kept; the findings appear in the order the reference's dict meets them.  Reseeds Python's global `random`, as the reference
    does."""
    bbox = {}
    for fname, label, x, y, w, h in bbox_rows:
        bbox[(fname, label)] = tuple(map(lambda v: int(v / 2), (x, y, x + w, y + h)))
    fnames = {k[0] for k in bbox}
    parent = {}
    for fname, label in metadata_rows:
        if fname not in fnames:
            continue
        labels = label.split("|")
        for disease in diseases:
            if disease in labels and (fname, disease) in bbox:
                parent.setdefault(disease, []).append((os.path.join(image_folder, fname), labels, bbox[(fname, disease)]))
    random.seed(seed)
    for k, v in parent.items():
        v = sorted(v, key=lambda e: (len(e[1]), random.random()))
        parent[k] = [(a, c) for a, _, c in v]
    return parent


def compare_reports(pt_dir: str, ft_dir: str) -> dict:
    """The tables `compare_json_files` prints, as a dict (no plot): per finding of the pre-trained run's auc.json / report.json,
    over ITS image names, {'auc': {finding: {'ft': (mean, std), 'pt': (mean, std), 'delta': mean(ft - pt)}}, 'typicality':
    {finding: {'ft': (mean, std), 'pt': (mean, std)}}} with numpy's population std."""
    def load(d, name):
        with open(os.path.join(d, name)) as f:
            return json.load(f)

    def stats(v):
        return float(np.mean(v)), float(np.std(v))
    out = {"auc": {}, "typicality": {}}
    pt, ft = load(pt_dir, "auc.json"), load(ft_dir, "auc.json")
    for k, vs in pt.items():
        out["auc"][k] = {"ft": stats([ft[k][kp] for kp in vs]), "pt": stats([pt[k][kp] for kp in vs]),
                         "delta": float(np.mean([ft[k][kp] - pt[k][kp] for kp in vs]))}
    pt, ft = load(pt_dir, "report.json"), load(ft_dir, "report.json")
    for k, vs in pt.items():
        out["typicality"][k] = {"ft": stats([ft[k][kp] for kp in vs]), "pt": stats([pt[k][kp] for kp in vs])}
    return out


def write_reports(output_path: str, diseases, names_by_disease, mean_by_disease, auc_by_disease):
    """report.json and auc.json with `main`'s structure and key order (compute.py:286-332): {finding: {file name: float}}, findings
    in `diseases` order, a finding without entries dropped, indent 4."""
    report, auc = {}, {}
    for disease in diseases:
        names = names_by_disease.get(disease, [])
        if not len(names):
            continue
        report[disease] = {n: float(v) for n, v in zip(names, mean_by_disease[disease])}
        auc[disease] = {n: float(v) for n, v in zip(names, auc_by_disease[disease])}
    os.makedirs(output_path, exist_ok=True)
    with open(os.path.join(output_path, "report.json"), "w") as f:
        json.dump(report, f, indent=4)
    with open(os.path.join(output_path, "auc.json"), "w") as f:
        json.dump(auc, f, indent=4)
    return report, auc
