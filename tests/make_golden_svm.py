#!/usr/bin/env python
"""Golden vectors for the Doersch baseline's detector SVMs (needs scikit-learn).

Expected values come from scikit-learn itself, as the reference calls it (doersch/doersch.py:66-79):

    SVC(C=cost, kernel='linear', shrinking=False[, max_iter=7]).fit(X, [1] * n_pos + [-1] * n_neg)
                                               coef_, intercept_, n_iter_, fit_status_, the alphas (|dual_coef_| at support_)
    the same with shrinking=True               `<key>_shrink_same`: whether the reference's default gives the same bits
    decision_function(X[n_pos:])               `<key>_score`; `<key>_hard` = the positions with a score > 0, highest first

Inputs are regenerated from seeds by tests/svm_cases.py; only their sha256 is stored.  Recorded once, each the largest over the fits:

    restatement_{w,b,alpha,score}_err   doersch.svm_fit_host / hard_negatives_host against scikit-learn: |dw| / |w| (L2), |db| / |b|,
                                        |dalpha| / |alpha| (L2), max |ds| / max |s|
    order_{w,b,alpha,score}_err         the restatement on the rows with their features in REVERSED order (another fixed summation
                                        order of QD and of every dot) against itself: what a different order does to the iterate

A case is pinned exactly, not statistically.  The generator scans data seeds and REFUSES a seed when
  - two neighbouring admitted scores differ by less than 1e-9, or a searched row scores within 1e-9 of 0;
  - the two leading candidates of a selection step (i or j, any iteration) differ by less than 1e-9 relative — unless they are equal
    bit for bit and the rows are duplicates of each other, or nothing has moved yet (iteration 0: every G is -1);
  - scikit-learn, the restatement and the restatement on reversed features disagree in n_iter, the status or the support set, or the
    restatement and scikit-learn in the hard-negative list;
  - a `hard*` case admits fewer hard negatives than svm_cases.MIN_HARD, the `sep` case any; `long` stops before n iterations.

    python tests/make_golden_svm.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests import svm_cases as SC  # noqa: E402
import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import doersch as D  # noqa: E402

MIN_GAP = 1e-9
ERRS = ("w", "b", "alpha", "score")


class Refuse(Exception):
    pass


def errors(w, b, alpha, score, w0, b0, alpha0, score0):
    return {"w": np.linalg.norm(w - w0) / np.linalg.norm(w0), "b": abs(b - b0) / abs(b0),
            "alpha": np.linalg.norm(alpha - alpha0) / np.linalg.norm(alpha0), "score": np.abs(score - score0).max() / np.abs(score0).max()}


def checked_fit(X, n_pos, cost, max_iter):
    """svm_fit_host with the selection-lead check."""
    n_neg = len(X) - n_pos
    Z = np.concatenate([X[n_pos:], X[:n_pos]])

    def trace(n_iter, kind, values, chosen):
        rest = values.copy()
        rest[chosen] = -np.inf
        second = int(np.argmax(rest))
        if rest[second] == -np.inf:
            return
        if rest[second] == values[chosen]:
            if (n_iter == 0 and kind == "i") or Z[second].tobytes() == Z[chosen].tobytes():
                return
            raise Refuse(f"iteration {n_iter}, {kind}: rows {chosen} and {second} tie without being duplicates")
        if values[chosen] - rest[second] < MIN_GAP * abs(values[chosen]):
            raise Refuse(f"iteration {n_iter}, {kind}: lead {values[chosen] - rest[second]:.3g} of {values[chosen]:.3g}")
    return D.svm_fit_host(X, n_pos, cost, 1e-3, max_iter, trace=trace)


def one_fit(tag, X, cost):
    from sklearn.svm import SVC
    c = SC.CASES[tag]
    n_pos, n = c["n_pos"], len(X)
    y = [1] * n_pos + [-1] * (n - n_pos)
    X64 = X.astype(np.float64)
    fits = []
    for shrinking in (False, True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fits.append(SVC(C=cost, kernel="linear", shrinking=shrinking, max_iter=c["max_iter"]).fit(X64, y))
    ref, shrunk = fits
    alpha0 = np.zeros(n)
    alpha0[ref.support_] = np.abs(ref.dual_coef_[0])
    w0, b0, score0 = ref.coef_[0].copy(), float(ref.intercept_[0]), ref.decision_function(X64[n_pos:])
    hard0 = np.flatnonzero(score0 > 0)
    hard0 = hard0[np.argsort(-score0[hard0], kind="stable")] + n_pos
    # the pin is exact only with clear gaps
    admitted = np.sort(score0[score0 > 0])
    if len(admitted) > 1 and np.diff(admitted).min() < MIN_GAP:
        raise Refuse("two admitted scores closer than 1e-9")
    if np.abs(score0).min() < MIN_GAP:
        raise Refuse("a score within 1e-9 of 0")
    if len(hard0) < SC.MIN_HARD.get(tag, 0) or (tag == "sep" and len(hard0)):
        raise Refuse(f"{len(hard0)} hard negatives")
    if tag == "long" and int(ref.n_iter_[0]) <= n:
        raise Refuse(f"n_iter {int(ref.n_iter_[0])} <= n")
    w, b, n_iter, alpha, status = checked_fit(X, n_pos, cost, c["max_iter"])
    hard, score = D.hard_negatives_host(X, w, b, n_pos, n)
    if n_iter != int(ref.n_iter_[0]) or status != int(ref.fit_status_) or not np.array_equal(alpha > 0, alpha0 > 0):
        raise Refuse("the restatement leaves scikit-learn's trajectory")
    if not np.array_equal(hard, hard0):
        raise Refuse("the restatement's hard negatives differ")
    Xr = np.ascontiguousarray(X[:, ::-1])
    wr, br, n_iter_r, alpha_r, status_r = D.svm_fit_host(Xr, n_pos, cost, 1e-3, c["max_iter"])
    hard_r, score_r = D.hard_negatives_host(Xr, wr, br, n_pos, n)
    if n_iter_r != n_iter or status_r != status or not np.array_equal(alpha_r > 0, alpha > 0) or not np.array_equal(hard_r, hard):
        raise Refuse("the trajectory depends on the summation order")
    rec = {"coef": w0, "intercept": np.float64(b0), "n_iter": np.int32(n_iter), "alpha": alpha0, "status": np.int32(status),
           "shrink_same": np.bool_(np.array_equal(ref.coef_, shrunk.coef_) and np.array_equal(ref.intercept_, shrunk.intercept_)
                                   and np.array_equal(ref.n_iter_, shrunk.n_iter_)),
           "hard": hard0.astype(np.int32), "score": score0}
    return rec, errors(w, b, alpha, score, w0, b0, alpha0, score0), errors(wr[::-1], br, alpha_r, score_r, w, b, alpha, score)


def main():
    import sklearn
    out = {"sklearn_version": np.array(sklearn.__version__)}
    worst = {f"{kind}_{e}_err": 0.0 for kind in ("restatement", "order") for e in ERRS}
    for tag, c in SC.CASES.items():
        data = SC.DATA_OF.get(tag, tag)
        seeds = [int(out[f"{data}_data_seed"])] if c["seed"] is None else range(c["seed"], c["seed"] + 200)
        for seed in seeds:
            X = SC.rows(tag, seed)
            try:
                fits = [(key, one_fit(tag, X, cost)) for key, cost in SC.keys(tag)]
            except Refuse as e:
                print(f"{tag}: seed {seed} refused: {e}")
                continue
            break
        else:
            raise SystemExit(f"{tag}: no seed passes")
        out[f"{tag}_data_seed"], out[f"{tag}_sha256"] = np.int64(seed), np.array(SC.digest(X))
        for key, (rec, err, order) in fits:
            for name, v in rec.items():
                out[f"{key}_{name}"] = v
            for e in ERRS:
                worst[f"restatement_{e}_err"] = max(worst[f"restatement_{e}_err"], float(err[e]))
                worst[f"order_{e}_err"] = max(worst[f"order_{e}_err"], float(order[e]))
            print(f"{key}: seed {seed}, n_iter {int(rec['n_iter'])}, status {int(rec['status'])}, {int((rec['alpha'] > 0).sum())} SVs, "
                  f"{len(rec['hard'])} hard, shrink_same {bool(rec['shrink_same'])}, restatement "
                  + " ".join(f"{e} {err[e]:.1e}" for e in ERRS) + ", order " + " ".join(f"{e} {order[e]:.1e}" for e in ERRS))
    for name, v in worst.items():
        out[name] = np.float64(v)
        print(f"{name} = {v:.3e}")
    path = os.path.join(HERE, "golden", "svm_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
