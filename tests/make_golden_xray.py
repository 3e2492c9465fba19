#!/usr/bin/env python
"""Golden vectors for the X-ray evaluation, produced by the reference's own code (needs the reference checkout that
tests/make_golden_consumers.py reads, and pandas).

    Typicallity.mean_typicallity   diffmining/applications/xray/compute.py:263-264
    Typicallity.aucpr              diffmining/applications/xray/compute.py:266-284
    Typicallity.compute            diffmining/applications/xray/compute.py:210-218   (the end-to-end case's map)
    Typicallity.load_paths         diffmining/applications/xray/compute.py:170-205

The four methods are compiled from the reference's text with `ast` (never written anywhere) and run on the maps of
tests/xray_cases.py, which are regenerated from seeds; the sha256 of each map is stored.  `aucpr` returns the area only, so the
counts come from a line-by-line restatement of its lines 268-276 (`counts` below), and the generator asserts that the
restatement's AUC equals the compiled function's bit for bit before it stores them.  Only results are stored:
tests/golden/xray_ref.npz.

    python tests/make_golden_xray.py
"""
import csv
import json
import os
import sys
import tempfile
import types
import warnings
from collections import defaultdict
from os.path import join

import numpy as np
import pandas as pd
import torch
from torch.nn.functional import interpolate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests import xray_cases as XC  # noqa: E402
from tests.make_golden_consumers import REF, ref_function  # noqa: E402

XR = "diffmining/applications/xray/compute.py"
E2E_ATOL, E2E_RTOL = 2e-5, 1e-4          # what tests/test_gpu_e2e.py holds typicality_image at kx = ky = 1 to


def counts(bbox, dm, thresholds):
    """compute.py:271-276 with the table as an argument; plus x.sum()."""
    x = np.zeros_like(dm)
    x[bbox[1]:bbox[3], bbox[0]:bbox[2]] = 1
    dm_flattened = dm.flatten()
    x_flattened = x.flatten()
    tp = np.sum(dm_flattened[x_flattened == 1] > thresholds[:, np.newaxis], axis=1)
    fp = np.sum(dm_flattened[x_flattened == 0] > thresholds[:, np.newaxis], axis=1)
    return tp, fp, x.sum()


def area(tp, fp, xsum):
    """compute.py:279-284"""
    denominator = tp + fp
    precision = np.where(denominator > 0, tp / denominator, 0)
    recall = tp / xsum
    return np.trapz(precision, recall)


def ulps32(a, b):
    """distance of two float32 in units in the last place (0 when both are NaN)"""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) and np.isnan(b):
        return 0
    assert np.isfinite(a) and np.isfinite(b), (a, b)

    def ordered(v):
        i = int(np.array(v, dtype=np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(ordered(a) - ordered(b))


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    warnings.simplefilter("ignore")
    ns = {"np": np, "pd": pd, "torch": torch, "interpolate": interpolate, "join": join, "defaultdict": defaultdict,
          "random": __import__("random")}
    aucpr = ref_function(XR, ("Typicallity", "aucpr"), ns)
    mean_typicallity = ref_function(XR, ("Typicallity", "mean_typicallity"), ns)
    compute = ref_function(XR, ("Typicallity", "compute"), ns)
    load_paths = ref_function(XR, ("Typicallity", "load_paths"), ns)
    thr = XC.thresholds()
    out = {"thresholds_sha256": np.array(XC.digest(thr))}

    def case(tag, dm, box, table=None):
        with np.errstate(all="ignore"):
            tp, fp, xsum = counts(box, dm, thr if table is None else table)
            auc = area(tp, fp, xsum)
            mean = np.float32(mean_typicallity(None, box, dm))
            if table is None:
                ref_auc = aucpr(None, box, dm)
                assert same(ref_auc, auc), (tag, ref_auc, auc)              # the restatement IS the reference
        fs, fabs = XC.box_fsum(dm, box)
        n_in = int(xsum)
        with np.errstate(all="ignore"):
            fs_mean = np.float32(np.float64(fs) / np.float64(n_in))
        assert np.isnan(mean) == np.isnan(fs_mean), (tag, mean, fs_mean)
        out[f"{tag}_sha256"] = np.array(XC.digest(dm))
        out[f"{tag}_box"] = np.array(box, dtype=np.int32)
        out[f"{tag}_tp"], out[f"{tag}_fp"] = tp.astype(np.int32), fp.astype(np.int32)
        out[f"{tag}_n_in"] = np.array(n_in, dtype=np.int32)
        out[f"{tag}_auc"] = np.array(auc, dtype=np.float64)
        out[f"{tag}_mean"] = np.array(mean, dtype=np.float32)
        out[f"{tag}_fsum"] = np.array(fs, dtype=np.float64)
        out[f"{tag}_mean_ulps"] = np.array(ulps32(mean, fs_mean), dtype=np.int64)
        print(f"{tag}: {dm.shape} box {tuple(box)} n_in {n_in} auc {auc!r} mean {mean!r} distinct tp {len(np.unique(tp))} "
              f"mean ulps {int(out[f'{tag}_mean_ulps'])}")
        return tp, fp

    for tag in XC.ORDER:
        dm, box = XC.case_map(tag), XC.case_box(tag)
        tp, fp = case(tag, dm, box)
        if tag == "a":
            assert len(np.unique(tp)) >= 200, len(np.unique(tp))            # the bins are in use
        if tag == "c":
            assert not fp.any()
        if tag == "d":
            assert np.isnan(out["d_auc"]) and np.isnan(out["d_mean"])
        if tag == "e":
            t32 = np.array([np.float32(thr[k]) for k in XC.E_TIES]).astype(np.float64)
            above = t32 > thr[list(XC.E_TIES)]
            assert above.any() and (~above).any() and not (t32 == thr[list(XC.E_TIES)]).any(), above
            print("   e: float32(thr[k]) above its fp64 threshold for", int(above.sum()), "of", len(above))
            assert np.isnan(out["e_mean"]) and np.isfinite(out["e_auc"])
        if tag == "f":
            assert (tp == tp[0]).all() and tp[0] == out["f_n_in"]
        if tag == "g":
            assert not tp.any() and not fp.any()
    for tag in XC.SHORT_TABLES:
        case(tag, XC.case_map(tag), XC.case_box(tag), XC.short_table(tag))

    # ---- end to end: the reference's own map (Typicallity.compute) from seeded fp16 grids, then its aucpr ---------------------------------
    for j in range(XC.E2E_N):
        grid, size, box = XC.e2e_grid(j), XC.E2E_SIZE, XC.E2E_BOXES[j]
        _, dm = compute(types.SimpleNamespace(), grid, size)
        assert dm.dtype == np.float32 and dm.shape == size
        tp, fp = case(f"e2e{j}", dm, box)
        out[f"e2e{j}_sha256"] = np.array(XC.digest(grid.numpy()))           # of the grid: the map is the reference's, not regenerated
        # per k: the reference pixels that an error of atol + rtol |v| can move across thr[k], inside and outside the box
        x1, y1, x2, y2 = box
        inside = np.zeros(dm.shape, dtype=bool)
        inside[y1:y2, x1:x2] = True
        v = dm.astype(np.float64).ravel()
        near = np.abs(v[None, :] - thr[:, None]) <= (E2E_ATOL + E2E_RTOL * np.abs(v))[None, :]
        out[f"e2e{j}_band_in"] = near[:, inside.ravel()].sum(axis=1).astype(np.int32)
        out[f"e2e{j}_band_out"] = near[:, ~inside.ravel()].sum(axis=1).astype(np.int32)
        worst = (out[f"e2e{j}_band_in"] + out[f"e2e{j}_band_out"]).max() / v.size
        print(f"   e2e{j}: widest band holds {worst:.3%} of the pixels; pixels in (thr[-1], thr[0]]: "
              f"{((v > thr[-1]) & (v <= thr[0])).mean():.1%}")
        assert worst < 0.01, worst
    out["e2e_tol"] = np.array([E2E_ATOL, E2E_RTOL])

    # ---- load_paths on a ten-line CSV pair ----------------------------------------------------------------------------------------
    diseases = ["Atelectasis", "Mass", "Nodule", "Effusion"]
    meta = [(f"{i:08d}_000.png", lab) for i, lab in enumerate(
        ["Mass", "Atelectasis|Mass", "No Finding", "Nodule|Mass|Atelectasis", "Mass", "Atelectasis", "Mass|Nodule", "Cardiomegaly",
         "Atelectasis|Effusion", "Mass|Infiltration"])]
    bbox = [(meta[0][0], "Mass", 225.1, 547.0, 86.8, 79.2), (meta[1][0], "Mass", 100.0, 200.5, 301.0, 55.5),
            (meta[1][0], "Atelectasis", 686.1, 131.5, 185.5, 313.5), (meta[3][0], "Nodule", 11.0, 13.0, 99.0, 101.0),
            (meta[3][0], "Mass", 500.0, 400.0, 300.0, 201.0), (meta[4][0], "Mass", 7.9, 9.9, 1001.5, 333.3),
            (meta[5][0], "Atelectasis", 64.0, 64.0, 128.0, 128.0), (meta[6][0], "Mass", 300.5, 310.5, 40.2, 60.7),
            (meta[6][0], "Mass", 302.5, 312.5, 44.2, 64.7), (meta[9][0], "Infiltration", 1.0, 2.0, 3.0, 4.0)]
    with tempfile.TemporaryDirectory() as td:
        with open(join(td, "metadata.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Image Index", "Finding Labels", "Follow-up #"])
            w.writerows([(a, b, 0) for a, b in meta])
        with open(join(td, "BBox_List_2017.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Image Index", "Finding Label", "x", "y", "w", "h"])
            w.writerows(bbox)
        me = types.SimpleNamespace(diseases=diseases, seed=42)
        load_paths(me, td)
        parent = {k: [(os.path.relpath(a, join(td, "images")), [int(c) for c in b]) for a, b in v] for k, v in me.parent.items()}
    print("load_paths:", parent)
    assert len(parent["Mass"]) >= 5
    out["load_paths"] = np.array(json.dumps({"diseases": diseases, "metadata": meta, "bbox": bbox, "seed": 42,
                                             "parent": list(parent.items())}))
    p = os.path.join(HERE, "golden", "xray_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
