#!/usr/bin/env python
"""Golden vectors for the parallel-dataset mining stage, produced by the reference's own code (needs the reference checkout that
tests/make_golden_consumers.py reads, pandas and scipy).

    sort                  diffmining/typicality/utils.py:82-83
    get_non_overlapping   diffmining/typicality/utils.py:94-102
    Cluster.df_PD.compute diffmining/applications/parallel-dataset/cluster.py:229-241 (restated below line by line, with np.median
                          itself, because the nested function also loads images and grids from disk)
    Typicality.load_paths diffmining/applications/parallel-dataset/compute.py:186-208

`sort`, `get_non_overlapping` and `load_paths` are compiled from the reference's text with `ast` (never written anywhere).  The
selection runs on pandas frames built exactly as `df_PD.compute` builds them: one row
`(i, j, i+kx, j+ky, origin, dm[i, j]) + (ds[c][i, j] for c in countries) + (pths[c] for c in countries)` per position of the median
map, row-major.  Only arrays are stored: tests/golden/parallel_ref.npz.

The maps are Gaussian-smoothed normal noise (sigma 2), seeded.  pandas' default sort does not define an order among equal keys,
so, as in make_golden_mining.py, the generator records every round's lead of the winner over the best remaining candidate as a
fraction of max|median| and FAILS when one is below 1e-5.

`load_paths` runs on empty files of about 20 synthetic names in a temporary directory; its groups are stored relative to that
directory, sorted by path (the reference's order is os.listdir's).

    python tests/make_golden_parallel.py
"""
import os
import sys
import tempfile
from collections import defaultdict

import numpy as np
import pandas as pd
from scipy.ndimage import gaussian_filter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests.make_golden_consumers import REF, ref_function  # noqa: E402
from tests.make_golden_mining import MIN_LEAD, leads  # noqa: E402

FILES = {
    "France": ["gt--France__001.jpg", "Japan__001.jpg", "Italy__001.jpg", "United_Kingdom__001.jpg",
               "gt--France__002__b.jpg", "Japan__002__b.jpg",
               "gt--France__003.jpg",                                   # a base without neighbours
               "Brazil__999.jpg",                                       # a neighbour without a base
               "xx--Japan__001.jpg",                                    # '--' but not 'gt--': ignored
               "gt--France__004.png", "Japan__004.png"],                # only '.jpg' leaves the sid
    "Japan": ["gt--Japan__010.jpg", "France__010.jpg", "United States__010.jpg", "Nigeria__010.jpg"],
    "United_Kingdom": ["gt--United_Kingdom__7.jpg", "France__7.jpg", "Japan_x__7.jpg"],     # 'Japan_x' pairs as 'Japan'
}


def compute(ds, countries, country_origin, kx, ky, k_per_image, ascending, sort, get_non_overlapping, perm=None):
    """cluster.py:229-241 with `ds` (the per-country pooled maps) given; the shuffled frame's order is `perm` when given"""
    column = ['x_start', 'y_start', 'x_end', 'y_end', 'origin', 'D'] + countries + ['path_' + c for c in countries]      # :226
    pths = {c: f"{c}.jpg" for c in countries}
    dm = np.median(np.stack([ds[c] for c in countries], axis=0), axis=0)                                                  # :231
    df = [(i, j, i + kx, j + ky, country_origin, dm[i, j]) + tuple([ds[c][i, j] for c in countries]) + tuple([pths[c] for c in countries])
          for i in range(dm.shape[0]) for j in range(dm.shape[1])]                                                        # :233
    df = pd.DataFrame(df, columns=column)                                                                                 # :238
    if perm is None:
        df = sort(df, 'D', ascending=ascending)                                                                           # :239
    else:
        df = df.iloc[perm].reset_index(drop=True)                                                                         # :234-236
    return dm, get_non_overlapping(df, k_per_image=k_per_image)                                                           # :241


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    UT = "diffmining/typicality/utils.py"
    ns = {"np": np, "pd": pd}
    sort = ref_function(UT, ("sort",), ns)
    get_non_overlapping = ref_function(UT, ("get_non_overlapping",), ns)
    rng = np.random.default_rng(20261018)
    out = {}

    def maps(n_sets, shape):
        return np.stack([gaussian_filter(rng.standard_normal(shape), sigma=2).astype(np.float32) for _ in range(n_sets)])

    def case(tag, stack, k, k_per_image, ascending, perm=None, want_count=None):
        countries = [f"set{c}" for c in range(len(stack))]
        ds = dict(zip(countries, stack))
        dm, got = compute(ds, countries, countries[0], k, k, k_per_image, ascending, sort, get_non_overlapping, perm)
        assert dm.dtype == np.float32 and dm.shape == stack.shape[1:]
        boxes = got[["x_start", "y_start", "x_end", "y_end"]].to_numpy().astype(np.int32).reshape(-1, 4)
        D = got["D"].to_numpy().astype(np.float32)
        set_D = got[countries].to_numpy().astype(np.float32).reshape(-1, len(countries))
        assert all(dm[b[0], b[1]] == d for b, d in zip(boxes, D))
        assert (got["origin"] == countries[0]).all() and all((got["path_" + c] == c + ".jpg").all() for c in countries)
        out[f"{tag}_maps"], out[f"{tag}_median"] = stack, dm
        out[f"{tag}_args"] = np.array([k, k, k_per_image, int(ascending)], dtype=np.int64)
        out[f"{tag}_boxes"], out[f"{tag}_D"], out[f"{tag}_set_D"] = boxes, D, set_D
        if perm is None:
            ld = leads(dm, boxes, k, k, ascending)
            assert (ld >= MIN_LEAD).all(), (tag, ld)                 # no tie decides a round: the case may be pinned to pandas
            out[f"{tag}_leads"] = ld
        else:
            out[f"{tag}_perm"] = np.asarray(perm, dtype=np.int64)
        if want_count is not None:
            assert len(boxes) in want_count, (tag, len(boxes))
        print(tag, "boxes", boxes.tolist(), "min lead", None if perm is not None else float(out[f"{tag}_leads"].min()))

    big = maps(10, (29, 41))
    case("p10_desc", big, 8, 5, False)
    case("p10_asc", big, 8, 5, True)
    case("short_desc", maps(10, (5, 12)), 4, 5, False, want_count=(2, 3))      # one row band: at most 3 boxes fit, 5 asked
    case("p3_desc", maps(3, (23, 31)), 6, 4, False)
    case("p4_desc", maps(4, (23, 31)), 6, 4, False)
    case("perm", big, 8, 5, False, perm=rng.permutation(big[0].size))
    for t in ("p10_asc", "perm"):                                              # the maps are stored once
        assert np.array_equal(out[f"{t}_maps"], out["p10_desc_maps"]) and np.array_equal(out[f"{t}_median"], out["p10_desc_median"])
        del out[f"{t}_maps"], out[f"{t}_median"]

    # Typicality.load_paths on empty files
    import os as _os
    lp_ns = {"os": _os, "join": _os.path.join, "defaultdict": defaultdict, "tqdm": lambda x, **_: x}
    load_paths = ref_function("diffmining/applications/parallel-dataset/compute.py", ("Typicality", "load_paths"), lp_ns)

    class Holder:
        pass
    with tempfile.TemporaryDirectory() as root:
        for d, names in FILES.items():
            os.makedirs(os.path.join(root, d))
            for n in names:
                open(os.path.join(root, d, n), "w").close()
        h = Holder()
        load_paths(h, root)
        rows = []
        for d in sorted(h.parallel):
            groups = sorted(([data[0]] + sorted(data[1:]) for data in h.parallel[d]), key=lambda data: data[0][0])
            for gi, data in enumerate(groups):
                for path, country in data:
                    rows.append((d, gi, os.path.relpath(path, root), country))
    out["files_dir"] = np.array([d for d, names in FILES.items() for _ in names])
    out["files_name"] = np.array([n for names in FILES.values() for n in names])
    out["groups_dir"] = np.array([r[0] for r in rows])
    out["groups_index"] = np.array([r[1] for r in rows], dtype=np.int64)
    out["groups_path"] = np.array([r[2] for r in rows])
    out["groups_country"] = np.array([r[3] for r in rows])
    for r in rows:
        print(r)
    p = os.path.join(HERE, "golden", "parallel_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
