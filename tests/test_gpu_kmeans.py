"""The clustering stage's last step on the GPU (dm_kmeans_fit, dm_cluster_rank) against scikit-learn's own fit and the
reference's own cluster() tail, recorded in tests/golden/kmeans_ref.npz (tests/make_golden_kmeans.py: every case there has leads
that keep rounding from deciding a label, a draw or a place).

Centres: within 16 x restatement_center_err of scikit-learn's (restatement_center_err = what the numpy restatement differs from
scikit-learn by, 6.0e-8; the factor is for another summation order over clusters of up to a few hundred members).  Each case
prints its figures before it asserts (-s)."""
import os

import numpy as np
import pytest
import torch

from diff_mining_amd import clustering as CL
from tests import kmeans_cases as KC
from tests.test_kmeans import RANK_ARMS, case_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(KC.CASES) + ["empty"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "kmeans_ref.npz"))


@pytest.fixture(scope="module")
def inputs(gold):
    return {tag: case_input(gold, tag) for tag in ALL}


@pytest.fixture(scope="module")
def fits(gold, inputs):
    """one device fit per case, shared and left unchanged"""
    out = {}
    for tag in ALL:
        X, k = inputs[tag]
        out[tag] = CL.kmeans_fit(torch.from_numpy(X).cuda(), k, init_index=gold["empty_seed_index"] if tag == "empty" else None)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", ALL)
def test_fit_equals_sklearn(gold, inputs, fits, tag):
    labels, centers, seeds, inertia, n_iter = fits[tag]
    k = inputs[tag][1]
    err = np.abs(centers.cpu().numpy() - gold[f"{tag}_centers"]).max()
    want = float(gold[f"{tag}_inertia"])        # 0 where every row is its own centre (n = k): the bound is then exact
    diff = abs(float(inertia) - want)
    print(f"{tag}: n_iter {int(n_iter)} centre err {err:.3e} inertia {float(inertia):.6e} against {want:.6e} (diff {diff:.3e})")
    assert np.array_equal(seeds.cpu().numpy(), gold[f"{tag}_seed_index"])
    assert int(n_iter) == int(gold[f"{tag}_n_iter"])
    assert np.array_equal(labels.cpu().numpy(), gold[f"{tag}_labels"])
    assert err <= 16 * float(gold["restatement_center_err"])
    assert diff <= 1e-5 * want
    if tag == "empty":      # scikit-learn's relocation: the duplicated start's empty cluster was filled
        assert np.bincount(labels.cpu().numpy(), minlength=k).min() > 0


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("tag", ["long300", "ref", "empty"])
def test_fit_is_bit_reproducible_on_any_stream_and_workspace(gold, inputs, fits, tag):
    X, k = inputs[tag]
    init = gold["empty_seed_index"] if tag == "empty" else None
    Xd = torch.from_numpy(X).cuda()
    assert _same(CL.kmeans_fit(Xd, k, init_index=init), fits[tag])
    need = CL.workspace_bytes(*X.shape, k)
    work = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")      # nothing relies on zeroed scratch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = CL.kmeans_fit(Xd, k, init_index=init, work=work)
        labels = fits[tag][0]
        D = torch.from_numpy(KC.typicality(len(X), 5)).cuda()
        r1 = CL.rank_clusters(Xd, labels, again[1], D, work=work.fill_(0xFF))
    side.synchronize()
    assert (work[need:] == 0xFF).all(), "the 64 bytes behind the workspace were written"
    assert _same(again, fits[tag])
    assert _same(r1, CL.rank_clusters(Xd, labels, fits[tag][1], D))


@pytest.mark.parametrize("tag,mode,agg,nan", RANK_ARMS)
def test_ranking_equals_reference(gold, inputs, tag, mode, agg, nan):
    X, k = inputs[tag]
    labels, centers = gold[f"{tag}_labels"], gold[f"{tag}_centers"]
    D, Xr = KC.rank_inputs(labels, int(gold[f"{tag}_rank{'_nan' if nan else ''}_d_seed"]), nan)
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    got = CL.rank_clusters(dev(X), dev(labels), dev(centers), dev(D), agg, mode, dev(Xr) if mode == "farthest" else None)
    pre = f"{tag}_rank_{mode}_{agg}{'_nan' if nan else ''}_"
    for name, g in zip(("order", "cluster_of_rank", "offsets", "aggregate", "n_nonempty"), got):
        np.testing.assert_array_equal(g.cpu().numpy(), gold[pre + name], err_msg=name)


def test_ranking_leaves_empty_clusters_out():
    """labels that never name cluster 1 or 3: two ranked clusters, the rest -1 / n / NaN; an even count takes the mean of the two
    middle values; equal keys keep row order"""
    X = torch.zeros(6, 2, device="cuda")
    X[:, 0] = torch.tensor([3., 1., 1., 2., 5., 4.])
    labels = torch.tensor([2, 0, 0, 2, 0, 2], dtype=torch.int32, device="cuda")
    centers = torch.zeros(4, 2, device="cuda")
    D = torch.tensor([1., 8., 2., 3., 4., 7.], device="cuda")
    order, cor, off, agg, nn = (t.cpu().numpy() for t in CL.rank_clusters(X, labels, centers, D))
    assert int(nn) == 2 and cor.tolist() == [0, 2, -1, -1] and off.tolist() == [0, 3, 6, 6, 6]
    assert order.tolist() == [1, 2, 4, 3, 0, 5] and agg[:2].tolist() == [4.0, 3.0] and np.isnan(agg[2:]).all()
    D[5] = 5.
    labels[4] = 2
    order, cor, off, agg, nn = (t.cpu().numpy() for t in CL.rank_clusters(X, labels, centers, D, "median"))
    assert cor.tolist() == [0, 2, -1, -1] and agg[:2].tolist() == [5.0, 3.5] and order.tolist() == [1, 2, 3, 0, 5, 4]


def test_scorer_clusters_patches_end_to_end(gold, inputs):
    from diff_mining_amd.typicality import TypicalityScorer
    X, k = inputs["k32"]
    labels = gold["k32_labels"]
    D, Xr = KC.rank_inputs(labels, int(gold["k32_rank_d_seed"]))
    for mode, rf in (("centroid", None), ("farthest", torch.from_numpy(Xr).cuda())):
        res = TypicalityScorer.cluster_patches(torch.from_numpy(X).cuda(), torch.from_numpy(D).cuda(), num_clusters=k, order_by=mode,
                                               rank_features=rf)
        pre = f"k32_rank_{mode}_median_"
        off = gold[pre + "offsets"]
        assert len(res["clusters"]) == int(gold[pre + "n_nonempty"]) and np.array_equal(res["labels"].cpu().numpy(), labels)
        for r, c in enumerate(res["clusters"]):
            assert c["cluster"] == gold[pre + "cluster_of_rank"][r] and c["aggregate"] == gold[pre + "aggregate"][r]
            assert np.array_equal(c["rows"], gold[pre + "order"][off[r]:off[r + 1]])


def test_refusals_on_the_device():
    from diff_mining_amd.engine import EngineError
    X = torch.zeros(4, 3, device="cuda")
    for k, kw in ((5, {}), (0, {}), (257, {}), (2, {"max_iter": 0})):
        with pytest.raises(EngineError):
            CL.kmeans_fit(X, k, **kw)
    with pytest.raises(EngineError):
        CL.kmeans_fit(X, 2, work=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(EngineError):
        CL.rank_clusters(X, torch.zeros(4, dtype=torch.int32, device="cuda"), X[:2], X[:, 0], order_by="nearest")
