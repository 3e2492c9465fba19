#!/usr/bin/env python
"""Golden vectors for the clustering stage's last step (needs scikit-learn and the reference checkout that
tests/make_golden_consumers.py reads).

Expected values come from scikit-learn itself and from the reference's own text:

    KMeans(n_clusters=k, random_state=10).fit(X)                      labels_, cluster_centers_, inertia_, n_iter_
    kmeans_plusplus(X - mean, k, random_state=RandomState(10))        the seed indices
    Cluster.cluster      diffmining/typicality/cluster.py:312-328                       (project=False; 'centroid' order)
    Cluster.cluster      diffmining/applications/parallel-dataset/cluster.py:268-289    ('farthest' order; `compress` stubbed: the
                         caller's reduced matrix is what gets clustered, the originals are what distances are taken in)
    median, mean         diffmining/typicality/cluster.py:50-54

The reference's functions are compiled from its text with `ast` (never written anywhere) and run with ids = row numbers, so the
returned structure reads back as arrays.  Inputs are regenerated from seeds by tests/kmeans_cases.py; only their sha256 is stored.

A case is pinned to the label only where rounding cannot decide it.  The generator scans data seeds and REFUSES a case when
  - any row's lead of its best over its second-best centre, in any assignment, is below 1e-4 of the mean nearest squared distance;
  - |shift - tol_abs| < 1e-3 tol_abs in any iteration;
  - a seeding draw falls within 1e-6 (relative to the potential) of a prefix-sum boundary — scikit-learn's potential is an fp32
    BLAS sum (about 1e-7 relative), which is why this is wider than 1e-9 — or u0 n within 1e-9 of an integer, or two distinct
    candidates' potentials are within 1e-5 of each other (the potentials are fp32 sums there too);
  - two members of one cluster have distance keys within 1e-5 of the largest key (numpy takes the norm in fp32), or a centre's
    farthest row leads the runner-up by less than 1e-5;
  - scikit-learn and the numpy restatement (clustering.kmeans_fit_host) disagree in a seed index, a label or n_iter.
The `long*` cases must also run at least 5 iterations.  Every case's leads are recorded.

    python tests/make_golden_kmeans.py
"""
import os
import sys
import types
from collections import defaultdict
import operator

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests.make_golden_consumers import REF, ref_function  # noqa: E402
from tests import kmeans_cases as KC  # noqa: E402
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import clustering as CL  # noqa: E402

MIN_LEAD, MIN_SHIFT_GAP, MIN_DRAW_GAP, MIN_POT_GAP, MIN_KEY_GAP = 1e-4, 1e-3, 1e-6, 1e-5, 1e-5


class Refuse(Exception):
    pass


def fit_case(X, k, init_index=None, min_iter=0):
    from sklearn.cluster import KMeans, kmeans_plusplus
    n = len(X)
    if init_index is None:
        km = KMeans(n_clusters=k, random_state=10).fit(X)
        _, sk_seeds = kmeans_plusplus(X - X.mean(axis=0), k, random_state=np.random.RandomState(10))
    else:
        km = KMeans(n_clusters=k, init=X[init_index], n_init=1).fit(X)
        sk_seeds = np.asarray(init_index)
    trace = []
    labels, centers, seeds, inertia, n_iter = CL.kmeans_fit_host(X, k, init_index=init_index, trace=trace)
    if not np.array_equal(seeds, sk_seeds):
        raise Refuse(f"seed indices differ: {seeds} vs {sk_seeds}")
    if n_iter != km.n_iter_ or not np.array_equal(labels, km.labels_):
        raise Refuse(f"labels / n_iter differ ({n_iter} vs {km.n_iter_})")
    if n_iter < min_iter:
        raise Refuse(f"only {n_iter} iterations")
    Xc = X - X.mean(axis=0)
    xn = (Xc.astype(np.float64) ** 2).sum(axis=1)
    lead, shift_gap, draw_gap, pot_gap = np.inf, np.inf, np.inf, np.inf
    for it, tr in enumerate(trace):
        if "scores" in tr and k > 1:
            S = tr["scores"].astype(np.float64)
            if init_index is not None and it == 0:                  # a centre given twice ties exactly with itself: the lowest
                S = S[:, np.unique(init_index, return_index=True)[1]]     # index takes the rows by rule, not by rounding
            part = np.partition(S, 1, axis=1)
            lead = min(lead, float((part[:, 1] - part[:, 0]).min() / (part[:, 0] + xn).mean()))
        if "shift" in tr:
            shift_gap = min(shift_gap, abs(float(tr["shift"]) - float(tr["tol_abs"])) / float(tr["tol_abs"]))
        if "rand" in tr:
            draw_gap = min(draw_gap, float(np.abs(tr["cum"][None, :] - tr["rand"][:, None]).min() / tr["pot"]))
            for a in range(len(tr["cand"])):
                for b in range(a):
                    if tr["cand"][a] != tr["cand"][b]:
                        pot_gap = min(pot_gap, abs(tr["pots"][a] - tr["pots"][b]) / tr["pots"].max())
    if init_index is None:
        u0n = CL.kmeans_uniforms(k)[0] * n
        if abs(u0n - round(u0n)) < 1e-9:
            raise Refuse("u0 n at an integer")
    if lead < MIN_LEAD:
        raise Refuse(f"assignment lead {lead:.2e}")
    if shift_gap < MIN_SHIFT_GAP:
        raise Refuse(f"shift within {shift_gap:.2e} of tol")
    if draw_gap < MIN_DRAW_GAP:
        raise Refuse(f"draw within {draw_gap:.2e} of a boundary")
    if pot_gap < MIN_POT_GAP:
        raise Refuse(f"potentials within {pot_gap:.2e}")
    err = float(np.abs(centers - km.cluster_centers_).max())
    return {"seed_index": np.asarray(sk_seeds, dtype=np.int32), "labels": km.labels_.astype(np.int32),
            "centers": km.cluster_centers_.astype(np.float32), "inertia": np.float64(km.inertia_), "n_iter": np.int64(km.n_iter_),
            "leads": np.array([lead, shift_gap, draw_gap, pot_gap]), "restatement_center_err": np.float64(err)}


def key_gaps(Xr, ref, labels):
    key = np.sqrt(((Xr.astype(np.float64) - ref[labels].astype(np.float64)) ** 2).sum(axis=1))
    gap = np.inf
    for j in np.unique(labels):
        ks = np.sort(key[labels == j])
        if len(ks) > 1:
            gap = min(gap, float(np.diff(ks).min() / key.max()))
    return gap


def as_arrays(result, labels, n, k):
    """The reference's [(members, aggregate)] with ids = row numbers -> rank_clusters' arrays"""
    order = np.array([v[2] for vs, _ in result for v in vs], dtype=np.int32)
    cor = np.full(k, -1, dtype=np.int32)
    off = np.full(k + 1, n, dtype=np.int32)
    agg = np.full(k, np.nan, dtype=np.float32)
    pos = 0
    for r, (vs, a) in enumerate(result):
        cor[r], off[r], agg[r] = labels[vs[0][2]], pos, a
        assert all(labels[v[2]] == cor[r] for v in vs)
        pos += len(vs)
    assert pos == n
    return {"order": order, "cluster_of_rank": cor, "offsets": off, "aggregate": agg, "n_nonempty": np.int64(len(result))}


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    from sklearn.cluster import KMeans
    TY, PD = "diffmining/typicality/cluster.py", "diffmining/applications/parallel-dataset/cluster.py"
    ns = {"np": np, "KMeans": KMeans, "defaultdict": defaultdict, "operator": operator, "umap": None}
    aggs = {"median": ref_function(TY, ("median",), dict(ns)), "mean": ref_function(TY, ("mean",), dict(ns))}
    cluster_ty = ref_function(TY, ("Cluster", "cluster"), dict(ns))
    cluster_pd = ref_function(PD, ("Cluster", "cluster"), dict(ns))
    out = {}

    def ranking(tag, X, k, fit, d_seed, nan=False):
        n = len(X)
        labels = fit["labels"]
        D, Xr = KC.rank_inputs(labels, d_seed, nan)
        ds = list(D)
        ids = list(range(n))
        far = []
        for c in fit["centers"]:
            dist = ((X.astype(np.float64) - c.astype(np.float64)) ** 2).sum(axis=1)
            top = np.sort(dist)[-2:]
            if n > 1 and (top[1] - top[0]) / top[1] < MIN_KEY_GAP:
                raise Refuse("farthest-row lead")
            far.append(int(np.argmax(dist)))
        gaps = (key_gaps(X, fit["centers"], labels), key_gaps(Xr, Xr[far], labels))
        if min(gaps) < MIN_KEY_GAP:
            raise Refuse(f"member key gaps {gaps}")
        for agg in ("median", "mean"):
            me = types.SimpleNamespace(aggregate=aggs[agg], compress=lambda X_, **kw: X)
            res = cluster_ty(me, list(X), ids, ids, ds, ids, "c", num_clusters=k, project=False)
            for key, v in as_arrays(res, labels, n, k).items():
                out[f"{tag}_rank_centroid_{agg}{'_nan' if nan else ''}_{key}"] = v
            res = cluster_pd(me, list(Xr), ids, ids, ds, ids, num_clusters=k)
            for key, v in as_arrays(res, labels, n, k).items():
                out[f"{tag}_rank_farthest_{agg}{'_nan' if nan else ''}_{key}"] = v
        counts = np.bincount(labels, minlength=k)
        assert (counts[counts > 0] % 2 == 0).any() and (counts % 2 == 1).any(), counts
        out[f"{tag}_rank{'_nan' if nan else ''}_d_seed"] = np.int64(d_seed)
        out[f"{tag}_rank_key_gaps"] = np.array(gaps)

    for tag, (n, d, k, nb, noise) in KC.CASES.items():
        first = KC.FIRST_SEED.get(tag, 1)
        for attempt in range(3):
            for seed in range(first, first + 64):
                X = KC.blobs(n, d, nb, noise, seed)
                try:
                    fit = fit_case(X, k, min_iter=5 if tag.startswith("long") else 0)
                    stash = dict(out)
                    if tag in ("long257", "k32"):
                        try:
                            ranking(tag, X, k, fit, 100 + seed)
                            ranking(tag, X, k, fit, 200 + seed, nan=True)
                        except Refuse:
                            out.clear()
                            out.update(stash)
                            raise
                    break
                except Refuse as e:
                    print(f"  {tag} seed {seed} noise {noise}: refused ({e})")
            else:
                noise *= 0.8                                           # 64 seeds gave none: lower the noise
                continue
            break
        else:
            sys.exit(f"{tag}: no seed found")
        for key, v in fit.items():
            out[f"{tag}_{key}"] = v
        out[f"{tag}_data_seed"], out[f"{tag}_noise"], out[f"{tag}_sha256"] = np.int64(seed), np.float64(noise), np.array(KC.digest(X))
        print(tag, "seed", seed, "noise", noise, "n_iter", int(fit["n_iter"]), "leads", fit["leads"], "err", fit["restatement_center_err"])

    # the empty cluster: explicit initial rows, the first given twice, so the higher index starts empty and is relocated
    n, d, k, nb, noise = KC.EMPTY_CASE
    for seed in range(1, 65):
        X = KC.blobs(n, d, nb, noise, seed)
        init = np.array([3, 3, 40, 77][:k], dtype=np.int32)
        try:
            fit = fit_case(X, k, init_index=init)
            break
        except Refuse as e:
            print(f"  empty seed {seed}: refused ({e})")
    else:
        sys.exit("empty: no seed found")
    for key, v in fit.items():
        out[f"empty_{key}"] = v
    out["empty_data_seed"], out["empty_noise"], out["empty_sha256"] = np.int64(seed), np.float64(noise), np.array(KC.digest(X))
    print("empty seed", seed, "n_iter", int(fit["n_iter"]), "counts", np.bincount(fit["labels"], minlength=k))
    out["restatement_center_err"] = np.float64(max(float(out[f"{t}_restatement_center_err"]) for t in list(KC.CASES) + ["empty"]))
    p = os.path.join(HERE, "golden", "kmeans_ref.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes; restatement_center_err", float(out["restatement_center_err"]))


if __name__ == "__main__":
    main()
