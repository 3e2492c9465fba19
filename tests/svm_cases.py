"""Inputs of the SVM tests, regenerated from their seeds.  Shared by tests/make_golden_svm.py, which records each input's sha256 in
tests/golden/svm_ref.npz, and by the tests, which check it.

`rows` uses only operations whose result is fixed: the legacy `RandomState` stream (frozen by numpy), elementwise float64
arithmetic, `math.fsum` (exact) for the row norms and the correctly rounded cast to fp16."""
import hashlib
import math

import numpy as np

# tag -> n_pos, n_neg, C (features), costs, norm of a row, near = negatives drawn from the positives' distribution (spread evenly
# over the negatives: `near_places`), spread = the noise of a row around its centre, dup = (copy, original) pairs among the
# negatives (the originals are near ones), max_iter, first seed the generator tries.
# The data seed itself is in the fixture (`<tag>_data_seed`), found by the generator.
CASES = {
    "sep": dict(n_pos=5, n_neg=257, C=2112, costs=(0.1,), norm=1.0, near=0, spread=0.5, dup=(), max_iter=-1, seed=1),
    "hard264": dict(n_pos=33, n_neg=257, C=264, costs=(1.0,), norm=2.0, near=12, spread=0.5, dup=(), max_iter=-1, seed=1),
    "hard2112": dict(n_pos=40, n_neg=600, C=2112, costs=(1.0,), norm=2.0, near=16, spread=0.5, dup=(), max_iter=-1, seed=1),
    "ties": dict(n_pos=3, n_neg=70, C=40, costs=(0.1, 1.0, 10.0), norm=2.0, near=6, spread=0.5,
                 dup=((20, 11), (41, 23), (60, 11), (69, 46)), max_iter=-1, seed=1),
    "cap": dict(n_pos=3, n_neg=70, C=40, costs=(0.1, 1.0, 10.0), norm=2.0, near=6, spread=0.5,
                dup=((20, 11), (41, 23), (60, 11), (69, 46)), max_iter=7, seed=None),          # `ties`' data
    "one": dict(n_pos=1, n_neg=64, C=40, costs=(0.1,), norm=2.0, near=6, spread=0.5, dup=(), max_iter=-1, seed=1),
    "wide": dict(n_pos=16, n_neg=30, C=8192, costs=(1.0,), norm=2.0, near=6, spread=0.5, dup=(), max_iter=-1, seed=1),   # the feature limit
    "long": dict(n_pos=8, n_neg=30, C=40, costs=(100.0,), norm=2.0, near=15, spread=1.5, dup=(), max_iter=-1, seed=1),
}
DATA_OF = {"cap": "ties"}                    # a case that reuses another one's rows
# the hard-negative runs of a case beyond the plain one (n_hn = 0, max_samples = n): (n_hn, max_samples)
HARD_VARIANTS = {"hard264": ((20, 290), (0, 5))}
MIN_HARD = {"hard264": 3, "hard2112": 3, "wide": 3}     # what the generator demands of a seed


def keys(tag):
    """The fit keys of a case, one per cost: `<tag>` or `<tag>_c<cost>`."""
    costs = CASES[tag]["costs"]
    return [(tag if len(costs) == 1 else f"{tag}_c{cost:g}", cost) for cost in costs]


def near_places(tag):
    """The negatives (counted from the first negative) that are drawn from the positives' distribution."""
    c = CASES[DATA_OF.get(tag, tag)]
    return (np.arange(c["near"]) * c["n_neg"]) // max(c["near"], 1)


def rows(tag, seed):
    """fp16 [n_pos + n_neg, C]: non-negative rows of norm `norm` (before the cast), the positives first.  The positives and the
    `near` negatives scatter around one centre, every other negative around one of eight other centres."""
    c = CASES[DATA_OF.get(tag, tag)]
    n_pos, n_neg, C_ = c["n_pos"], c["n_neg"], c["C"]
    rs = np.random.RandomState(seed)
    centres = np.abs(rs.standard_normal((9, C_)))
    which = np.concatenate([np.zeros(n_pos, dtype=np.int64), 1 + rs.randint(0, 8, size=n_neg)])
    which[n_pos + near_places(tag)] = 0
    X = np.abs(centres[which] + c["spread"] * rs.standard_normal((n_pos + n_neg, C_)))
    norms = np.array([math.sqrt(math.fsum((row * row).tolist())) for row in X])
    X = (X * (c["norm"] / norms[:, None])).astype(np.float16)
    for copy, original in c["dup"]:
        X[n_pos + copy] = X[n_pos + original]
    return np.ascontiguousarray(X)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_ref.npz"))


def case_rows(tag, ref):
    """The rows of a case, checked against the fixture's sha256."""
    data = DATA_OF.get(tag, tag)
    X = rows(tag, int(ref[f"{data}_data_seed"]))
    assert digest(X) == str(ref[f"{data}_sha256"]), f"{tag}: the regenerated input differs from the one the fixture was made from"
    return X


def expected_hard(hard_all, first, max_samples):
    """The list of a run that searches from `first` and keeps `max_samples`, from the plain run's list: the order is kept."""
    return np.asarray([p for p in hard_all if p >= first][:max_samples], dtype=np.int64)


def fit_runs():
    """(key, tag, cost) of every fit."""
    return [(key, tag, cost) for tag in CASES for key, cost in keys(tag)]


def hard_runs():
    """(key, tag, cost, n_hn, max_samples) of every hard-negative run: the plain one of every fit, then the variants."""
    out = [(key, tag, cost, 0, CASES[tag]["n_pos"] + CASES[tag]["n_neg"]) for key, tag, cost in fit_runs()]
    for tag, variants in HARD_VARIANTS.items():
        out += [(key, tag, cost, n_hn, m) for key, cost in keys(tag) for n_hn, m in variants]
    return out
