"""Inputs of the k-means tests, regenerated from their seeds (the 1000 x 512 case alone would be 2 MB as a file).  Shared by
tests/make_golden_kmeans.py, which records each input's sha256 in tests/golden/kmeans_ref.npz, and by the tests, which check it.

`blobs` uses only operations whose result is fixed: the legacy `RandomState` stream (frozen by numpy), elementwise float64
arithmetic, and `math.fsum` (exact) for the row norms."""
import hashlib
import math

import numpy as np

# tag -> (n, d, k, blobs, noise); the data seed is in the fixture (`<tag>_data_seed`), found by the generator
CASES = {
    "long257": (257, 40, 7, 20, 0.6),
    "long300": (300, 64, 8, 30, 0.5),
    "k32": (600, 96, 32, 12, 0.2),
    "ref": (1000, 512, 32, 40, 0.08),
    "nk5": (5, 12, 5, 5, 0.3),
    "k1": (33, 9, 1, 3, 0.4),
}
# the empty-cluster case: `long300`'s kind of data, started from explicit rows with row EMPTY_INIT[0] given twice
EMPTY_CASE = (90, 16, 4, 6, 0.4)
FIRST_SEED = {"long257": 14, "long300": 7}


def blobs(n, d, n_blobs, noise, seed):
    """Row-normalised Gaussian blobs with noise, fp32 [n, d]."""
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((n_blobs, d))
    which = rs.randint(0, n_blobs, size=n)
    X = centres[which] + noise * rs.standard_normal((n, d))
    norms = np.array([math.sqrt(math.fsum((row * row).tolist())) for row in X])
    return np.ascontiguousarray((X / norms[:, None]).astype(np.float32))


def typicality(n, seed):
    """A `D` column: fp32 [n], distinct values."""
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


def rank_inputs(labels, d_seed, nan=False):
    """(D, rank_features) of a ranking case.  Python's `sorted` leaves the place of a NaN key to its algorithm, except in one
    spot: the cluster whose label appears last is the head of the reversed list, where nothing ever moves it, so it ends last.
    The NaN goes to a member of that cluster."""
    n = len(labels)
    D = typicality(n, d_seed)
    if nan:
        first = {int(j): int(np.flatnonzero(labels == j)[0]) for j in np.unique(labels)}
        last = max(first, key=first.get)
        members = np.flatnonzero(labels == last)
        D[members[1 % len(members)]] = np.nan
    return D, blobs(n, 24, 9, 0.5, d_seed + 1)         # the "un-reduced" features of the parallel-dataset variant


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
