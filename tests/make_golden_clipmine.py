#!/usr/bin/env python
"""Golden vectors for the CLIP baseline's mining stage, produced by the reference's own code (needs the reference checkout that
tests/make_golden_consumers.py reads, torch on the CPU and pandas).

    CLIPRankCluster.dot_text_image   clipmining/ranking.py:72-108
    pool                             clipmining/utils.py:75-81
    get_non_overlapping              clipmining/utils.py:86-94

The three functions are compiled from the reference's text with `ast` (never written anywhere) and run on synthetic tokens with a
stub `self` that carries `mode`.  Only arrays are stored: tests/golden/clipmine_ref.npz.

`torch.topk` and pandas leave the order among equal keys undefined and the reference computes in fp32, so a case is pinned only where
neither can decide it.  With the float64 restatement's map D (diff_mining_amd.clipmine.rank_patches_host) the generator records, and
REFUSES the case (trying the next seed) when a rule fails:
  (a) leads: per round, (winner - best other alive eligible candidate) / max|D|; refused below 1e-5;
  (b) the host selection must be the same when eligibility is cut at v_n -+ 1e-5 max|D| (v_n = the n-th largest value) instead of
      at rank n = min(100 k_per_image, OH OW);
  (c) restatement_D_err = max over the boxes |D_ref - D_restated| / max|D| and restatement_feat_err = max over the boxes
      |f_ref - f_restated|_2 / |f_ref|_2: the reference's own fp32 distance from float64, the yardstick of the tests.

    python tests/make_golden_clipmine.py
"""
import os
import sys
import types

import numpy as np
import pandas as pd
import torch
from torch.nn.functional import interpolate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from diff_mining_amd import clipmine as CM  # noqa: E402
from tests.make_golden_consumers import REF, ref_function  # noqa: E402

MIN_LEAD = 1e-5
# tag: (gh, pw, E, H, W, kx, ky, k_per_image, mode, planted token or None)
CASES = {
    "g45_diff": (4, 5, 48, 40, 52, 8, 8, 3, "diff", None),        # gh != pw, scale 10.4, an E tail
    "g45_sim": (4, 5, 48, 40, 52, 8, 8, 3, "sim", None),
    "g54_rect": (5, 4, 40, 37, 45, 8, 6, 5, "diff", None),        # kx != ky
    "g33_small": (3, 3, 32, 24, 24, 8, 8, 2, "diff", None),
    "all_eligible": (3, 3, 32, 16, 16, 8, 8, 2, "diff", None),    # n = OH OW = 81
    "run_out": (3, 3, 32, 48, 48, 8, 8, 2, "diff", 4),          # one dominant token: fewer than k boxes
    "real": (24, 24, 64, 512, 512, 64, 64, 5, "diff", None),    # the reference's geometry
}


def make_inputs(seed, gh, pw, E, planted):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(E)
    tokens = (rng.standard_normal((gh * pw, E)) + 0.5 * common) * rng.uniform(0.5, 2.0, size=(gh * pw, 1))
    t0 = rng.standard_normal(E)
    t1 = t0 + 0.7 * rng.standard_normal(E)                               # [category, ""]: two nearby unit vectors
    text = np.stack([t0 / np.linalg.norm(t0), t1 / np.linalg.norm(t1)])
    if planted is not None:
        tokens[planted] = 3.0 * (text[0] - text[1]) / np.linalg.norm(text[0] - text[1]) + 0.05 * tokens[planted]
    return tokens.astype(np.float32), text.astype(np.float32)


def leads(D, boxes, kx, ky, n_elig):
    order = np.argsort(-D.reshape(-1), kind="stable")[:n_elig]
    elig = np.zeros(D.size, dtype=bool)
    elig[order] = True
    alive = elig.reshape(D.shape).copy()
    out = []
    for (i, j, _, _) in boxes:
        assert alive[i, j], "the reference's winner is not an alive eligible candidate of the restated map"
        rest = alive.copy()
        rest[i, j] = False
        out.append((D[i, j] - D[rest].max()) / np.abs(D).max() if rest.any() else np.inf)
        alive[max(0, i - kx):i + kx + 1, max(0, j - ky):j + ky + 1] = False
    return np.array(out, dtype=np.float64)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    ns = {"torch": torch, "pd": pd, "np": np, "interpolate": interpolate}
    ns["pool"] = ref_function("clipmining/utils.py", ("pool",), ns)
    ns["get_non_overlapping"] = ref_function("clipmining/utils.py", ("get_non_overlapping",), ns)
    dot_text_image = ref_function("clipmining/ranking.py", ("CLIPRankCluster", "dot_text_image"), ns)
    out = {}
    for c, (tag, (gh, pw, E, H, W, kx, ky, k, mode, planted)) in enumerate(CASES.items()):
        for seed in range(20261019 + 100 * c, 20261019 + 100 * c + 40):
            tokens, text = make_inputs(seed, gh, pw, E, planted)
            with torch.no_grad():
                df, emb = dot_text_image(types.SimpleNamespace(mode=mode), "x.jpg", torch.from_numpy(text),
                                         torch.from_numpy(tokens)[None], (H, W), pw, k, kx, ky)
            boxes = df[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32).reshape(-1, 4)
            D_ref = df["D"].to_numpy().astype(np.float32)
            f_ref = np.stack(emb).astype(np.float32).reshape(len(boxes), E)
            rows, f_host, maps = CM.rank_patches_host([tokens], text, [(H, W)], pw, k, kx, ky, mode, return_maps=True)
            D = maps[0]
            n_elig, scale = min(100 * k, D.size), np.abs(D).max()
            h_boxes = np.stack([rows[n] for n in ("x_start", "y_start", "x_end", "y_end")], axis=1)
            why = None
            if h_boxes.shape != boxes.shape or (h_boxes != boxes).any():
                why = f"restatement boxes {h_boxes.tolist()} != reference {boxes.tolist()}"
            else:
                ld = leads(D, boxes, kx, ky, n_elig)
                v_n = np.sort(D.reshape(-1))[::-1][n_elig - 1]
                cuts = [CM._select_host(D, kx, ky, k, eligible=D >= v_n + sgn * MIN_LEAD * scale) for sgn in (-1.0, 1.0)]
                if (ld < MIN_LEAD).any():
                    why = f"lead {ld.min():.3g}"
                elif any(b.shape != boxes.shape or (b != boxes).any() for b in cuts):
                    why = "the eligibility boundary decides the selection"
                elif tag == "run_out" and not len(boxes) < k:
                    why = "did not run out"
            if why is None:
                break
            print(f"  {tag}: seed {seed} refused ({why})")
        else:
            sys.exit(f"{tag}: no seed accepted")
        if tag == "all_eligible":
            assert n_elig == D.size == 81
        D_err = float(np.abs(D_ref.astype(np.float64) - D[boxes[:, 0], boxes[:, 1]]).max() / scale)
        f_err = float((np.linalg.norm(f_ref.astype(np.float64) - f_host, axis=1) / np.linalg.norm(f_ref.astype(np.float64), axis=1)).max())
        out[f"{tag}_tokens"], out[f"{tag}_text"] = tokens, text
        out[f"{tag}_args"] = np.array([gh, pw, H, W, kx, ky, k, CM.MODES[mode], seed], dtype=np.int64)
        out[f"{tag}_boxes"], out[f"{tag}_D"], out[f"{tag}_feats"] = boxes, D_ref, f_ref
        out[f"{tag}_leads"] = ld
        out[f"{tag}_max_abs_D"] = np.float64(scale)
        out[f"{tag}_restatement_D_err"], out[f"{tag}_restatement_feat_err"] = np.float64(D_err), np.float64(f_err)
        print(f"{tag}: seed {seed} boxes {boxes.tolist()} count {len(boxes)}/{k} n_elig {n_elig}/{D.size} min lead {ld.min():.3g} "
              f"restatement_D_err {D_err:.3g} restatement_feat_err {f_err:.3g}")
    p = os.path.join(HERE, "golden", "clipmine_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
