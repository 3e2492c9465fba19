"""GPU tier of the detectors' SVMs (csrc/svm.hip): dm_svm_fit and dm_svm_hard_negatives on every case of tests/svm_cases.py against
the scikit-learn fixture tests/golden/svm_ref.npz, and the batch property — a detector's outputs do not depend on K, on its place in
the call or on the other detectors.

n_iter, status, the support set and the hard-negative positions must be EQUAL; w, b, alpha and the scores agree within 16 x
max(restatement error, order error) of the fixture: what the numpy restatement itself shows against scikit-learn, and what another
fixed summation order does to the iterate (for b and alpha both are 0: they must agree bit for bit)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import svm_cases as SC  # noqa: E402
from tests.gpu_util import dev  # noqa: E402

FACTOR = 16


@pytest.fixture(scope="module")
def ref():
    return SC.fixture()


def bound(ref, what):
    return FACTOR * max(float(ref[f"restatement_{what}_err"]), float(ref[f"order_{what}_err"]))


_fits = {}


def device_fit(key, tag, cost, ref):
    """One single-detector fit per key (the pool is the case's rows, the list 0 ... n - 1), shared by the tests: numpy copies of
    (w, b, n_iter, status, alpha) and the device operands."""
    if key not in _fits:
        X = SC.case_rows(tag, ref)
        pool = torch.from_numpy(X).to(dev())
        table = torch.arange(len(X), dtype=torch.int32, device=dev())[None]
        out = D.svm_fit(pool, table, len(X), SC.CASES[tag]["n_pos"], cost, 1e-3, SC.CASES[tag]["max_iter"], want_alpha=True)
        _fits[key] = (pool, table, out) + tuple(t.cpu().numpy()[0] for t in out)
    return _fits[key]


@pytest.mark.parametrize("key,tag,cost", SC.fit_runs(), ids=[r[0] for r in SC.fit_runs()])
def test_fit_matches_the_fixture(ref, key, tag, cost):
    _, _, _, w, b, n_iter, status, alpha = device_fit(key, tag, cost, ref)
    w0, b0, a0 = ref[f"{key}_coef"], float(ref[f"{key}_intercept"]), ref[f"{key}_alpha"]
    w_err = float(np.linalg.norm(w - w0) / np.linalg.norm(w0))
    b_err = abs(float(b) - b0) / abs(b0)
    a_err = float(np.linalg.norm(alpha - a0) / np.linalg.norm(a0))
    print(f"{key}: n_iter {int(n_iter)} (fixture {int(ref[f'{key}_n_iter'])}), status {int(status)}, {int((alpha > 0).sum())} support "
          f"vectors (fixture {int((a0 > 0).sum())}), w {w_err:.3e} (bound {bound(ref, 'w'):.3e}), b {b_err:.3e} (bound "
          f"{bound(ref, 'b'):.3e}), alpha {a_err:.3e} (bound {bound(ref, 'alpha'):.3e})")
    assert int(n_iter) == int(ref[f"{key}_n_iter"]) and int(status) == int(ref[f"{key}_status"])
    assert np.array_equal(alpha > 0, a0 > 0)
    assert w_err <= bound(ref, "w") and b_err <= bound(ref, "b") and a_err <= bound(ref, "alpha")


@pytest.mark.parametrize("key,tag,cost,n_hn,max_samples", SC.hard_runs(), ids=[f"{r[0]}-hn{r[3]}-m{r[4]}" for r in SC.hard_runs()])
def test_hard_negatives_match_the_fixture(ref, key, tag, cost, n_hn, max_samples):
    pool, table, out = device_fit(key, tag, cost, ref)[:3]
    n, n_pos = pool.shape[0], SC.CASES[tag]["n_pos"]
    score, hard, count = (t.cpu().numpy()[0] for t in D.svm_hard_negatives(pool, table, n, n_pos + n_hn, max_samples, out[0], out[1]))
    want = SC.expected_hard(ref[f"{key}_hard"], n_pos + n_hn, max_samples)
    s0 = ref[f"{key}_score"]
    s_err = float(np.abs(score[n_pos + n_hn:] - s0[n_hn:]).max() / np.abs(s0).max())
    print(f"{key} n_hn {n_hn} max_samples {max_samples}: {int(count)} hard negatives (fixture {len(want)}), score {s_err:.3e} "
          f"(bound {bound(ref, 'score'):.3e})")
    assert int(count) == len(want) and np.array_equal(hard[:len(want)], want) and (hard[len(want):] == -1).all()
    assert np.isnan(score[:n_pos + n_hn]).all()
    assert s_err <= bound(ref, "score")


def batch_inputs(ref):
    """Every C = 40 data set as a detector of one call — `ties` twice, at both ends — over one shuffled pool that holds every row once:
    ragged n, ld > n."""
    sets = [("ties", SC.case_rows("ties", ref)), ("one", SC.case_rows("one", ref)), ("long", SC.case_rows("long", ref))]
    rows = np.concatenate([X for _, X in sets])
    perm = np.random.RandomState(3).permutation(len(rows))
    pool = np.empty_like(rows)
    pool[perm] = rows                                       # row r of the union lives at pool[perm[r]]
    starts = np.cumsum([0] + [len(X) for _, X in sets])
    order = (0, 1, 2, 0)
    ld = 80
    table = np.full((len(order), ld), -7, dtype=np.int32)   # past n: never read
    for k, s in enumerate(order):
        table[k, :len(sets[s][1])] = perm[starts[s]:starts[s + 1]]
    n = np.array([len(sets[s][1]) for s in order])
    n_pos = np.array([SC.CASES[sets[s][0]]["n_pos"] for s in order])
    return [sets[s] for s in order], pool, table, n, n_pos


def run_batch(pool, table, n, n_pos, cost, max_iter, first, max_samples):
    pool, table = torch.from_numpy(pool).to(dev()), torch.from_numpy(table).to(dev())
    w, b, n_iter, status, alpha = D.svm_fit(pool, table, n, n_pos, cost, 1e-3, max_iter, want_alpha=True)
    score, hard, count = D.svm_hard_negatives(pool, table, n, first, max_samples, w, b)
    return [t.cpu().numpy() for t in (w, b, n_iter, status, alpha, score, hard, count)]


@pytest.mark.parametrize("cost,max_iter", ((0.1, -1), (1.0, 7), (10.0, -1)), ids=("c0.1", "c1-cap7", "c10"))
def test_a_detector_does_not_depend_on_its_batch(ref, cost, max_iter):
    sets, pool, table, n, n_pos = batch_inputs(ref)
    first, max_samples = n_pos + 2, np.array([3, 80, 80, 80])
    got = run_batch(pool, table, n, n_pos, cost, max_iter, first, max_samples)
    again = run_batch(pool, table, n, n_pos, cost, max_iter, first, max_samples)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()                                                      # the same bits on every run
    names = ("w", "b", "n_iter", "status", "alpha", "score", "hard", "count")
    for k, (tag, X) in enumerate(sets):
        own = run_batch(X, np.arange(len(X), dtype=np.int32)[None], n[k:k + 1], n_pos[k:k + 1], cost, max_iter, first[k:k + 1],
                        max_samples[k:k + 1])
        for name, a, b in zip(names, got, own):
            a, b = a[k], b[0]
            if name in ("alpha", "score", "hard"):
                assert (a[n[k]:] == (-1 if name == "hard" else 0)).all() if name != "score" else np.isnan(a[n[k]:]).all(), (k, name)
                a = a[:n[k]]
            assert a.tobytes() == b.tobytes(), (k, tag, name)
    assert got[0][0].tobytes() == got[0][3].tobytes()                                          # `ties` at both ends of the call
    key = {(0.1, -1): "ties_c0.1", (1.0, 7): "cap_c1", (10.0, -1): "ties_c10"}[(cost, max_iter)]
    assert int(got[2][0]) == int(ref[f"{key}_n_iter"]) and int(got[3][0]) == int(ref[f"{key}_status"])
    assert np.array_equal(got[4][0][:n[0]], ref[f"{key}_alpha"])                               # bit for bit (the bound is 0)


def test_statuses_of_rows_that_cannot_be_used(ref):
    """A NaN row, an infinite row, a sample outside the pool and a list without negatives stop their own detector alone."""
    X = SC.case_rows("one", ref).copy()
    good = len(X)
    X = np.concatenate([X, X[5:7]])
    X[good, 3], X[good + 1, 9] = np.nan, np.inf
    table = np.tile(np.arange(good, dtype=np.int32), (5, 1))
    table[1, 10], table[2, 64], table[3, 20] = good, good + 1, len(X)
    n, n_pos = np.full(5, good), np.array([1, 1, 1, 1, 1])
    pool, table_d = torch.from_numpy(X).to(dev()), torch.from_numpy(table).to(dev())
    n_pos_d = torch.tensor([1, 1, 1, 1, good], dtype=torch.int32, device=dev())
    n_d = torch.from_numpy(n.astype(np.int32)).to(dev())
    K, ld, C_ = 5, good, 40
    work = torch.empty(D.svm_workspace_bytes(K, ld), dtype=torch.uint8, device=dev())
    w = torch.empty((K, C_), dtype=torch.float64, device=dev())
    b = torch.empty(K, dtype=torch.float64, device=dev())
    n_iter, status = torch.empty(K, dtype=torch.int32, device=dev()), torch.empty(K, dtype=torch.int32, device=dev())
    rc = D._lib().dm_svm_fit(D._stream(torch, dev()), D._p(pool), len(X), C_, D._p(table_d), ld, D._p(n_d), D._p(n_pos_d), K, 0.1, 1e-3,
                             -1, D._p(work), work.numel(), D._p(w), D._p(b), D._p(n_iter), D._p(status), None)
    assert rc == 0
    assert status.cpu().tolist() == [D.SVM_CONVERGED, D.SVM_NAN, D.SVM_NAN, D.SVM_BAD_LIST, D.SVM_BAD_LIST]
    w, b = w.cpu().numpy(), b.cpu().numpy()
    assert np.isnan(w[1:]).all() and np.isnan(b[1:]).all()
    assert int(n_iter[0]) == int(ref["one_n_iter"]) and abs(b[0] - float(ref["one_intercept"])) <= bound(ref, "b")
    with pytest.raises(ValueError, match="NaN or infinity"):
        D.train_svms(pool, table_d[:2], n[:2], n_pos[:2], 0, 5)
    with pytest.raises(ValueError, match="outside the pool"):
        D.train_svms(pool, table_d[3:4], n[:1], n_pos[:1], 0, 5)


def test_round_on_the_device_equals_the_host_round(ref):
    """`svm_round` and `train_svm` with rows on the GPU: the same detectors and the same hard negatives as the numpy path."""
    X = SC.case_rows("hard264", ref)
    n_pos = SC.CASES["hard264"]["n_pos"]
    positives = [[(1.0, (0, 0), f"p{j}", X[j]) for j in range(n_pos)], [(1.0, (8, 8), f"p{j}", X[j]) for j in range(5)]]
    neg_h, neg_d = X[n_pos:], torch.from_numpy(X[n_pos:]).to(dev())
    hard_h, hard_d = [[], [X[n_pos + 3]]], [[], [X[n_pos + 3]]]
    ws_h = D.svm_round(positives, [neg_h, neg_h], hard_h, C=1.0)
    ws_d = D.svm_round(positives, [neg_d, neg_d], hard_d, C=1.0)
    assert ws_d.is_cuda and ws_d.dtype == torch.float64
    assert np.linalg.norm(ws_d.cpu().numpy() - ws_h) <= bound(ref, "w") * np.linalg.norm(ws_h)
    for k in range(2):
        assert [np.asarray(r.cpu() if hasattr(r, "cpu") else r).tobytes() for r in hard_d[k]] == [r.tobytes() for r in hard_h[k]]
    assert len(hard_d[0]) == len(ref["hard264_hard"])
    coef_h, hn_h = D.train_svm(X, (n_pos, 4, len(X) - n_pos - 4), 4)
    coef_d, hn_d = D.train_svm(torch.from_numpy(X).to(dev()), (n_pos, 4, len(X) - n_pos - 4), 4)
    assert np.linalg.norm(coef_d - coef_h) <= bound(ref, "w") * np.linalg.norm(coef_h) and hn_d == hn_h and len(hn_d) == 4


def test_sample_negatives_on_the_device_fetches_the_host_rows():
    rng = np.random.RandomState(0)
    chunks = [[rng.random_sample((2, 3, 5, 16)).astype(np.float16) for _ in range(2)] for _ in range(2)]
    on_dev = [[torch.from_numpy(a).to(dev()) for a in shard] for shard in chunks]
    for fold in (None, (1, 3)):
        host = D.sample_negatives(chunks, 17, fold=fold, rng=np.random.default_rng(4))
        got = D.sample_negatives(on_dev, 17, fold=fold, rng=np.random.default_rng(4))
        assert got.is_cuda and got.dtype == torch.float16 and got.cpu().numpy().tobytes() == host.tobytes()


def test_three_rounds_on_one_running_list_equal_the_host_rounds(ref):
    """The reference's loop (doersch.py:449-471): three folds extend ONE running hard-negative list per detector.  From the second
    round on a list holds device rows of the rounds before next to the numpy rows a search returns for the positives."""
    X = SC.case_rows("hard264", ref)
    n_pos = SC.CASES["hard264"]["n_pos"]
    positives = [[(1.0, (0, 0), f"p{j}", X[j]) for j in range(n_pos)], [(1.0, (8, 8), f"p{j}", X[j]) for j in range(16)]]
    folds = [X[n_pos:], X[n_pos + 40:], X[n_pos:n_pos + 200]]                                # the negatives each round draws
    hard_h, hard_d = [[], []], [[], []]
    for r, neg in enumerate(folds):
        neg_d = torch.from_numpy(neg).to(dev())
        ws_h = D.svm_round(positives, [neg, neg], hard_h, C=1.0)
        ws_d = D.svm_round(positives, [neg_d, neg_d], hard_d, C=1.0)
        err = float(np.linalg.norm(ws_d.cpu().numpy() - ws_h) / np.linalg.norm(ws_h))
        print(f"round {r}: lists of {[len(h) for h in hard_d]} rows (host {[len(h) for h in hard_h]}), ws {err:.3e} (bound {bound(ref, 'w'):.3e})")
        assert err <= bound(ref, "w")
        for k in range(2):
            assert all(isinstance(row, torch.Tensor) and row.is_cuda for row in hard_d[k])
            assert [row.cpu().numpy().tobytes() for row in hard_d[k]] == [row.tobytes() for row in hard_h[k]]
        if r == 0:
            assert len(hard_d[0]) == len(ref["hard264_hard"]) and len(hard_d[1]) > 0          # the later rounds start from device rows
