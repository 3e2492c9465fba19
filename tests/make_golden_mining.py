#!/usr/bin/env python
"""Golden vectors for the patch-mining stage, produced by the reference's own code (needs the reference checkout that
tests/make_golden_consumers.py reads, and pandas).

    sort                  diffmining/typicality/utils.py:82-83
    get_non_overlapping   diffmining/typicality/utils.py:94-102
    get_top_k             diffmining/typicality/utils.py:237-252   (non-random, unfiltered branch)
    Cluster.df_D.compute  diffmining/typicality/cluster.py:188-204 (the candidate frame; restated below line by line, because the
                          nested function also loads images and grids from disk)

The three utils functions are compiled from the reference's text with `ast` (never written anywhere) and run on pandas frames
built exactly as `df_D.compute` builds them: one row `(path, i, j, i+kx, j+ky, dm[i, j], 'real')` per position of the pooled
map, row-major.  Only arrays are stored: tests/golden/mining_ref.npz.

pandas' default sort does not define an order among equal keys, so a case is pinned only where no tie can decide it: for every
selection round the generator records the winner's lead over the best remaining candidate as a fraction of max|dm| and FAILS
when one is below 1e-5.

    python tests/make_golden_mining.py
"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests.make_golden_consumers import REF, ref_function  # noqa: E402

COLUMNS = ["seed", "x_start", "y_start", "x_end", "y_end", "D", "origin"]
MIN_LEAD = 1e-5


def frame(dm, kx, ky, path="x.jpg"):
    """cluster.py:194,200"""
    df = [(path, i, j, i + kx, j + ky, dm[i, j], "real") for i in range(dm.shape[0]) for j in range(dm.shape[1])]
    return pd.DataFrame(df, columns=COLUMNS)


def leads(dm, boxes, kx, ky, ascending):
    """Per round: (winner's key - best remaining key) / max|dm| among the candidates alive at the start of the round, the
    winner excluded (inf when the winner was the last one)."""
    key = -dm.astype(np.float64) if ascending else dm.astype(np.float64)
    alive = np.ones(dm.shape, dtype=bool)
    out = []
    for (i, j, _, _) in boxes:
        assert alive[i, j]
        rest = alive.copy()
        rest[i, j] = False
        out.append((key[i, j] - key[rest].max()) / np.abs(dm).max() if rest.any() else np.inf)
        alive[max(0, i - kx):i + kx + 1, max(0, j - ky):j + ky + 1] = False
    return np.array(out, dtype=np.float64)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    UT = "diffmining/typicality/utils.py"
    ns = {"np": np, "pd": pd}
    sort = ref_function(UT, ("sort",), ns)
    get_non_overlapping = ref_function(UT, ("get_non_overlapping",), ns)
    get_top_k = ref_function(UT, ("get_top_k",), ns)
    cons = np.load(os.path.join(HERE, "golden", "consumers_ref.npz"))
    out = {}
    selected = []

    def case(tag, dm, kx, ky, k_per_image, ascending, perm=None, want_count=None):
        df = frame(dm, kx, ky)
        if perm is None:
            df = sort(df, "D", ascending=ascending)                  # cluster.py:201
        else:
            df = df.iloc[perm].reset_index(drop=True)                # the shuffled frame (cluster.py:196-198), order = perm
        got = get_non_overlapping(df, k_per_image=k_per_image)       # cluster.py:204
        boxes = got[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32).reshape(-1, 4)
        D = got["D"].to_numpy().astype(np.float32)
        assert all(dm[b[0], b[1]] == d for b, d in zip(boxes, D))
        out[f"{tag}_map"] = dm
        out[f"{tag}_args"] = np.array([kx, ky, k_per_image, int(ascending)], dtype=np.int64)
        out[f"{tag}_boxes"], out[f"{tag}_D"] = boxes, D
        if perm is None:
            ld = leads(dm, boxes, kx, ky, ascending)
            assert (ld >= MIN_LEAD).all(), (tag, ld)                 # no tie decides a round: the case may be pinned to pandas
            out[f"{tag}_leads"] = ld
        else:
            out[f"{tag}_perm"] = np.asarray(perm, dtype=np.int64)    # a permutation has no ties
        if want_count is not None:
            assert len(boxes) in want_count, (tag, len(boxes))
        if perm is None:
            selected.append(got)                                     # (the shuffled frame can repeat a sorted frame's boxes)
        print(tag, "boxes", boxes.tolist(), "min lead", None if perm is not None else float(out[f"{tag}_leads"].min()))

    for tag in ("a", "b"):
        dm = np.ascontiguousarray(cons[f"{tag}_load_typicality"], dtype=np.float32)
        k = int(cons[f"{tag}_size"][2])
        assert dm.shape == (int(cons[f"{tag}_size"][0]) - k + 1, int(cons[f"{tag}_size"][1]) - k + 1)
        case(f"{tag}_desc", dm, k, k, 5, False)
        case(f"{tag}_asc", dm, k, k, 5, True)
    rng = np.random.default_rng(20261017)
    # a map that runs out: 5 x 12 positions, 4 x 4 windows, zone +-4 -> one row band, at most 3 boxes fit, 5 asked
    case("short_desc", rng.standard_normal((5, 12)).astype(np.float32), 4, 4, 5, False, want_count=(2, 3))
    case("short_asc", out["short_desc_map"], 4, 4, 5, True, want_count=(2, 3))
    # the random arm: map `a` visited in a stored permutation's order
    dm = out["a_desc_map"]
    case("perm", dm, 5, 5, 5, False, perm=rng.permutation(dm.size))
    # get_top_k on a category's concatenated frame (cluster.py:215, 408)
    cat = pd.concat(selected, axis=0)
    D = cat["D"].to_numpy().astype(np.float32)
    gaps = np.diff(np.sort(D.astype(np.float64)))
    assert gaps.min() / np.abs(D).max() >= MIN_LEAD, gaps.min()     # distinct D: the unstable sort cannot reorder
    top = get_top_k(cat, key="D", k=8)
    out["topk_in_D"] = D
    out["topk_in_boxes"] = cat[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32)
    out["topk_k"] = np.array(8, dtype=np.int64)
    out["topk_out_D"] = top["D"].to_numpy().astype(np.float32)
    out["topk_out_boxes"] = top[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32)
    assert len(out["topk_out_D"]) == 8 < len(D)
    p = os.path.join(HERE, "golden", "mining_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
