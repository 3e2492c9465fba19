"""CPU tier of the detectors' SVMs (diff-mining_amd/doersch.py, csrc/svm.hip): the numpy restatement against the scikit-learn
fixture tests/golden/svm_ref.npz (and against scikit-learn itself where it is installed), the refusals that need no GPU, and the
host paths of `train_svm`, `svm_round` and `sample_negatives`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from diff_mining_amd import doersch as D
from diff_mining_amd import engine as E
from tests import svm_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 16                                  # times the recorded error of the restatement, as the k-means tests do


@pytest.fixture(scope="module")
def ref():
    return SC.fixture()


_fits = {}


def host_fit(key, tag, cost, ref):
    """One restatement run per fit, shared by the tests."""
    if key not in _fits:
        X = SC.case_rows(tag, ref)
        _fits[key] = (X,) + D.svm_fit_host(X, SC.CASES[tag]["n_pos"], cost, 1e-3, SC.CASES[tag]["max_iter"])
    return _fits[key]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("key,tag,cost", SC.fit_runs(), ids=[r[0] for r in SC.fit_runs()])
def test_host_fit_matches_the_fixture(ref, key, tag, cost):
    X, w, b, n_iter, alpha, status = host_fit(key, tag, cost, ref)
    assert n_iter == int(ref[f"{key}_n_iter"]) and status == int(ref[f"{key}_status"])
    assert np.array_equal(alpha > 0, ref[f"{key}_alpha"] > 0)                                  # the support set
    assert rel(w, ref[f"{key}_coef"]) <= FACTOR * float(ref["restatement_w_err"])
    assert abs(b - float(ref[f"{key}_intercept"])) <= FACTOR * float(ref["restatement_b_err"]) * abs(float(ref[f"{key}_intercept"]))
    assert rel(alpha, ref[f"{key}_alpha"]) <= FACTOR * float(ref["restatement_alpha_err"])
    assert status == (D.SVM_MAX_ITER if tag == "cap" else D.SVM_CONVERGED)


@pytest.mark.parametrize("key,tag,cost,n_hn,max_samples", SC.hard_runs(), ids=[f"{r[0]}-hn{r[3]}-m{r[4]}" for r in SC.hard_runs()])
def test_host_hard_negatives_match_the_fixture(ref, key, tag, cost, n_hn, max_samples):
    X, w, b, _, _, _ = host_fit(key, tag, cost, ref)
    n_pos = SC.CASES[tag]["n_pos"]
    hard, score = D.hard_negatives_host(X, w, b, n_pos + n_hn, max_samples)
    assert np.array_equal(hard, SC.expected_hard(ref[f"{key}_hard"], n_pos + n_hn, max_samples))
    want = ref[f"{key}_score"][n_hn:]
    assert np.abs(score - want).max() <= FACTOR * float(ref["restatement_score_err"]) * np.abs(ref[f"{key}_score"]).max()


def test_the_cases_reach_their_branches(ref):
    assert len(ref["sep_hard"]) == 0 and abs(float(ref["sep_intercept"]) + 1) < 0.05             # the reference's regime
    assert len(ref["hard264_hard"]) >= 3 and len(ref["hard2112_hard"]) >= 3
    assert 3 <= len(SC.expected_hard(ref["hard264_hard"], 33 + 20, 290)) < len(ref["hard264_hard"])   # n_hn = 20 hides some
    assert int(ref["long_n_iter"]) > 38                                                          # past libsvm's first shrink step
    assert all(int(ref[f"cap_c{c}_status"]) == 1 and int(ref[f"cap_c{c}_n_iter"]) == 7 for c in ("0.1", "1", "10"))
    X = SC.case_rows("ties", ref)
    assert X[3 + 20].tobytes() == X[3 + 11].tobytes() and X[3 + 69].tobytes() == X[3 + 46].tobytes()
    for name in ("restatement_w_err", "restatement_score_err", "order_w_err", "order_b_err", "order_alpha_err", "order_score_err"):
        assert 0 <= float(ref[name]) < 1e-12, name


@pytest.mark.parametrize("key,tag,cost", SC.fit_runs(), ids=[r[0] for r in SC.fit_runs()])
def test_host_fit_matches_live_scikit_learn(ref, key, tag, cost):
    svm = pytest.importorskip("sklearn.svm")
    import warnings
    X, w, b, n_iter, alpha, status = host_fit(key, tag, cost, ref)
    n_pos = SC.CASES[tag]["n_pos"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = svm.SVC(C=cost, kernel="linear", shrinking=False, max_iter=SC.CASES[tag]["max_iter"]).fit(
            X.astype(np.float64), [1] * n_pos + [-1] * (len(X) - n_pos))
    assert n_iter == int(s.n_iter_[0]) and status == int(s.fit_status_)
    assert np.array_equal(np.flatnonzero(alpha > 0), np.sort(s.support_))
    assert rel(w, s.coef_[0]) <= FACTOR * float(ref["restatement_w_err"])
    assert abs(b - s.intercept_[0]) <= FACTOR * float(ref["restatement_b_err"]) * abs(s.intercept_[0])
    hard, score = D.hard_negatives_host(X, w, b, n_pos, len(X))
    want = s.decision_function(X[n_pos:].astype(np.float64))
    assert np.abs(score - want).max() <= FACTOR * float(ref["restatement_score_err"]) * np.abs(want).max()
    assert np.array_equal(hard - n_pos, np.flatnonzero(want > 0)[np.argsort(-want[want > 0], kind="stable")])


def test_host_refusals(ref):
    X = SC.case_rows("one", ref)
    for bad in (lambda: D.svm_fit_host(X, 0), lambda: D.svm_fit_host(X, len(X)), lambda: D.svm_fit_host(X[:, :36], 1),
                lambda: D.svm_fit_host(X[:, :4], 1), lambda: D.svm_fit_host(X.astype(np.float32), 1), lambda: D.svm_fit_host(X, 1, C=0.0),
                lambda: D.svm_fit_host(X, 1, tol=-1.0), lambda: D.hard_negatives_host(X, np.zeros(40), 0.0, len(X) + 1, 5)):
        with pytest.raises(ValueError):
            bad()
    for v in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[7, 3] = v
        with pytest.raises(ValueError, match="NaN or infinity"):
            D.svm_fit_host(Y, 1)
    table = np.arange(len(X), dtype=np.int32)[None]
    with pytest.raises(ValueError):
        D.train_svms(X, np.repeat(table, 129, axis=0), len(X), 1, 0, 5)                       # more than 128 detectors
    with pytest.raises(ValueError, match="outside the pool"):
        D.train_svms(X[:10], table, len(X), 1, 0, 5)
    with pytest.raises(ValueError, match="no positive, no negative"):
        D._svm_raise(np.array([D.SVM_CONVERGED, D.SVM_BAD_LIST]))
    with pytest.raises(ValueError, match="NaN or infinity"):
        D._svm_raise(np.array([D.SVM_NAN, D.SVM_BAD_LIST]))
    D._svm_raise(np.array([D.SVM_CONVERGED, D.SVM_MAX_ITER]))


def test_error_table_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    codes = {name: int(v) for name, v in re.findall(r"#define DM_SVM_E_(\w+) (\d+)", hdr)}
    assert sorted(codes.values()) == sorted(D.SVM_ERRORS) == list(range(1, len(codes) + 1))
    consts = dict(re.findall(r"#define (DM_SVM_[A-Z_]+) (\d+)", hdr))
    assert (int(consts["DM_SVM_MAX_DETECTORS"]), int(consts["DM_SVM_MAX_FEATURES"])) == (D.SVM_MAX_DETECTORS, D.SVM_MAX_FEATURES)
    assert [int(consts[f"DM_SVM_{n}"]) for n in ("CONVERGED", "MAX_ITER", "NAN", "BAD_LIST")] == \
        [D.SVM_CONVERGED, D.SVM_MAX_ITER, D.SVM_NAN, D.SVM_BAD_LIST]
    for name in ("dm_svm_workspace_bytes", "dm_svm_fit", "dm_svm_hard_negatives"):
        assert name in E.SYMBOLS


def test_abi_refusals_need_no_gpu():
    """Every refusal comes before the first launch: the pointers only have to be non-null (and aligned, until that is the point)."""
    lib = E.load_library()
    assert lib.dm_svm_workspace_bytes(1, 2) > 0
    big, small = lib.dm_svm_workspace_bytes(64, 25005), lib.dm_svm_workspace_bytes(64, 1000)
    assert big > small > 0 and big < 2 ** 31                                                  # 64 x 25 005: well under 2 GiB
    for K, n in ((0, 10), (129, 10), (1, 1), (1, 1 << 24)):
        assert lib.dm_svm_workspace_bytes(K, n) == 0
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def fit(rows=p, R=10, C_=40, ld=10, K=1, cost=0.1, eps=1e-3, work=p, work_bytes=1 << 30, w=p):
        return lib.dm_svm_fit(None, rows, R, C_, p, ld, p, p, K, cost, eps, -1, work, work_bytes, w, p, p, p, None)

    def hard(rows=p, R=10, C_=40, ld=10, K=1, work=p, work_bytes=1 << 30, count=p):
        return lib.dm_svm_hard_negatives(None, rows, R, C_, p, ld, p, p, p, K, p, p, work, work_bytes, p, p, count)
    assert fit(w=None) == 1 and fit(rows=None) == 1 and hard(count=None) == 1
    for call in (fit, hard):
        assert call(K=0) == 2 and call(K=129) == 2
        assert call(C_=4) == 3 and call(C_=44) == 3 and call(C_=8200) == 3 and call(C_=8192, work_bytes=64) == 8    # 8192 passes the check
        assert call(R=0) == 4
        assert call(ld=1) == 5
        assert call(ld=1 << 24) == 6
        assert call(work_bytes=64) == 8
        assert call(rows=p + 8) == 9 and call(work=p + 4) == 9
    assert fit(cost=0.0) == 7 and fit(eps=0.0) == 7 and fit(cost=float("nan")) == 7


def test_train_svm_returns_what_the_reference_returns(ref):
    X = SC.case_rows("hard264", ref)
    n_pos = SC.CASES["hard264"]["n_pos"]
    coef, hard = D.train_svm([row for row in X], (n_pos, 4, len(X) - n_pos - 4), 4)
    assert isinstance(coef, np.ndarray) and coef.shape == (264,) and coef.dtype == np.float64
    assert isinstance(hard, list) and len(hard) == 4 and all(isinstance(h, list) and len(h) == 264 for h in hard)
    w, b, _, _, _ = D.svm_fit_host(X, n_pos)                                                    # C = 0.1, the intercept dropped
    assert np.array_equal(coef, w)
    want, _ = D.hard_negatives_host(X, w, b, n_pos + 4, 4)
    assert hard == X[want].tolist()
    with pytest.raises(ValueError):
        D.train_svm(X, (n_pos, 0, 3), 4)


def keyed_chunks(shards=3, keys=(2, 3, 1), B=2, W=3, H=5, C_=8):
    """Shards of keys whose rows name themselves: feature 0 = shard, 1 = key, 2 = the cell's flat position."""
    out = []
    for s in range(shards):
        shard = []
        for q in range(keys[s]):
            data = np.zeros((B, W, H, C_), dtype=np.float16)
            data[..., 0], data[..., 1] = s, q
            data[..., 2] = np.arange(B * W * H).reshape(B, W, H)
            shard.append(data)
        out.append(shard)
    return out


def test_sample_negatives_counts_pool_and_determinism():
    chunks = keyed_chunks()
    rows = D.sample_negatives(chunks, 40, rng=np.random.default_rng(5))
    assert rows.dtype == np.float16 and rows.shape == (2 * 6 + 3 * 4 + 13, 8)                  # 40 // 3 = 13 per shard, // keys per key
    per_key = {(0, 0): 6, (0, 1): 6, (1, 0): 4, (1, 1): 4, (1, 2): 4, (2, 0): 13}
    for (s, q), want in per_key.items():
        mine = rows[(rows[:, 0] == s) & (rows[:, 1] == q)]
        assert len(mine) == want and len(set(mine[:, 2].tolist())) == want                      # without replacement
    again = D.sample_negatives(chunks, 40, rng=np.random.default_rng(5))
    assert rows.tobytes() == again.tobytes()
    assert rows.tobytes() != D.sample_negatives(chunks, 40, rng=np.random.default_rng(6)).tobytes()
    assert len(D.sample_negatives(chunks, 2)) == 6                                              # at least one row per key
    # the fold pool: the first i n // l entries of the CPU randperm under seed 0
    import torch
    torch.manual_seed(0)
    pool = torch.randperm(30)[:(2 * 30) // 3].numpy()
    assert np.array_equal(D.fold_pool(30, (2, 3)), pool) and len(pool) == 20
    rows = D.sample_negatives(chunks, 60, fold=(2, 3), rng=np.random.default_rng(1))
    assert set(rows[:, 2].astype(int).tolist()) <= set(pool.tolist())
    assert len(rows) == 2 * 10 + 3 * 6 + 20 and set(rows[rows[:, 0] == 2][:, 2].astype(int).tolist()) == set(pool.tolist())
    with pytest.raises(ValueError):
        D.sample_negatives(chunks, 90, fold=(1, 3))                                             # 30 rows from a pool of 10
    with pytest.raises(ValueError):
        D.sample_negatives([], 10)


def test_svm_round_on_numpy_rows(ref):
    X = SC.case_rows("hard264", ref)
    n_pos = SC.CASES["hard264"]["n_pos"]
    positives = [[(1.0, (0, 0), f"p{j}", X[j]) for j in range(n_pos)], [(1.0, (8, 8), f"p{j}", X[j]) for j in range(5)]]
    negatives = [X[n_pos:], X[n_pos:]]                                                          # one array for both: pooled once
    hard = [[], [X[n_pos + 3]]]
    ws = D.svm_round(positives, negatives, hard, C=1.0)
    assert ws.shape == (2, 264) and ws.dtype == np.float64
    assert rel(ws[0], ref["hard264_coef"]) <= FACTOR * float(ref["restatement_w_err"])
    assert [r.tobytes() for r in hard[0]] == [X[p].tobytes() for p in ref["hard264_hard"]]
    Y = np.concatenate([X[:5], X[n_pos + 3][None], X[n_pos:]])
    w1, b1, _, _, _ = D.svm_fit_host(Y, 5, 1.0)
    assert np.array_equal(ws[1], w1)
    want, _ = D.hard_negatives_host(Y, w1, b1, 6, 25000 - 1)
    assert hard[1][0].tobytes() == X[n_pos + 3].tobytes() and [r.tobytes() for r in hard[1][1:]] == [Y[p].tobytes() for p in want]
    with pytest.raises(ValueError):
        D.svm_round([[]], [X[n_pos:]], [[]])
