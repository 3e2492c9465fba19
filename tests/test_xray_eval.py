"""CPU tier of the X-ray evaluation (diff-mining_amd/xray.py): the numpy restatement against the reference's own results
(tests/golden/xray_ref.npz, written by tests/make_golden_xray.py from the reference's `aucpr`, `mean_typicallity` and `load_paths`)."""
import json
import os

import numpy as np
import pytest

from diff_mining_amd import xray as X
from tests import xray_cases as XC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xray_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if np.isnan(a) and np.isnan(b) else 1 << 40

    def ordered(v):
        i = int(np.array(v, dtype=np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(ordered(a) - ordered(b))


def check_against_fixture(gold, tag, tp, fp, n_in, box_sum):
    assert np.array_equal(tp, gold[f"{tag}_tp"]) and np.array_equal(fp, gold[f"{tag}_fp"]), tag
    assert int(n_in) == int(gold[f"{tag}_n_in"]), tag
    mean, auc = X.xray_scores_from_counts(tp, fp, n_in, box_sum)
    assert auc.dtype == np.float64 and mean.dtype == np.float32
    assert same(auc, gold[f"{tag}_auc"]), (tag, auc, gold[f"{tag}_auc"])                  # bit for bit
    assert ulps32(mean, gold[f"{tag}_mean"]) <= int(gold[f"{tag}_mean_ulps"]) + 1, (tag, mean, gold[f"{tag}_mean"])


def test_thresholds_are_the_references(gold):
    thr = X.xray_thresholds()
    assert thr.dtype == np.float64 and thr.shape == (1000,) and (thr[1:] < thr[:-1]).all()
    assert XC.digest(thr) == str(gold["thresholds_sha256"]) == XC.digest(XC.thresholds())


@pytest.mark.parametrize("tag", XC.ORDER + XC.SHORT_TABLES)
def test_case_inputs_are_the_fixtures(gold, tag):
    assert XC.digest(XC.case_map(tag)) == str(gold[f"{tag}_sha256"])
    assert tuple(gold[f"{tag}_box"]) == tuple(XC.case_box(tag))


def test_host_counts_and_scores_equal_the_reference(gold):
    tags = list(XC.ORDER)
    tp, fp, n_in, box_sum = X.xray_counts_host([XC.case_map(t) for t in tags], [XC.case_box(t) for t in tags])
    assert tp.dtype == fp.dtype == n_in.dtype == np.int32 and box_sum.dtype == np.float64 and tp.shape == (len(tags), 1000)
    for b, tag in enumerate(tags):
        check_against_fixture(gold, tag, tp[b], fp[b], n_in[b], box_sum[b])
        fs = float(gold[f"{tag}_fsum"])
        if np.isnan(fs):
            assert np.isnan(box_sum[b]), tag
        else:
            assert abs(box_sum[b] - fs) <= max(int(n_in[b]), 1) * 2.0 ** -53 * XC.box_fsum(XC.case_map(tag), XC.case_box(tag))[1], tag
    assert np.isnan(X.xray_scores_from_counts(tp, fp, n_in, box_sum)[1][tags.index("d")])
    # a batch of rows and the rows one by one give the same scores
    mean, auc = X.xray_scores_from_counts(tp, fp, n_in, box_sum)
    assert mean.shape == auc.shape == (len(tags),)
    assert same(auc[0], X.xray_scores_from_counts(tp[0], fp[0], n_in[0], box_sum[0])[1])


@pytest.mark.parametrize("tag", XC.SHORT_TABLES)
def test_short_threshold_tables(gold, tag):
    tp, fp, n_in, box_sum = X.xray_counts_host([XC.case_map(tag)], [XC.case_box(tag)], XC.short_table(tag))
    assert tp.shape == (1, len(XC.short_table(tag)))
    check_against_fixture(gold, tag, tp[0], fp[0], n_in[0], box_sum[0])


def test_numpy_maps_take_the_host_path():
    dm, box = XC.case_map("b"), XC.case_box("b")
    got = X.xray_eval([dm], [box])
    want = X.xray_counts_host([dm], [box])
    assert all(isinstance(g, np.ndarray) and same(g, w) for g, w in zip(got, want))


def test_fp32_comparison_would_count_the_ties_differently(gold):
    """Case `e` holds pixels at float32(thr[k]); the rule is the reference's fp64 comparison, and the fixture can tell the two apart."""
    dm, box, thr = XC.case_map("e"), XC.case_box("e"), XC.thresholds()
    x1, y1, x2, y2 = box
    v = dm[y1:y2, x1:x2].ravel()
    tp32 = np.array([(v > np.float32(t)).sum() for t in thr])
    assert (tp32 != gold["e_tp"]).any()


def test_refusals():
    dm = XC.case_map("i")
    ok_box = (0, 0, 1, 1)
    with pytest.raises(ValueError, match="thresholds"):
        X.xray_counts_host([dm], [ok_box], np.zeros(0))
    with pytest.raises(ValueError, match="thresholds"):
        X.xray_counts_host([dm], [ok_box], np.linspace(1, 0.5, X.XRAY_MAX_THRESHOLDS + 1))
    with pytest.raises(ValueError, match="decrease"):
        X.xray_counts_host([dm], [ok_box], np.array([0.1, 0.1]))
    with pytest.raises(ValueError, match="decrease"):
        X.xray_counts_host([dm], [ok_box], np.array([0.1, 0.2]))
    with pytest.raises(ValueError, match="NaN"):
        X.xray_counts_host([dm], [ok_box], np.array([0.1, np.nan]))
    for bad in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1), (0, 0, 1, -1)):
        with pytest.raises(ValueError, match="negative"):
            X.xray_counts_host([dm], [bad])
    with pytest.raises(ValueError, match="2\\^24"):
        X.xray_counts_host([np.broadcast_to(np.float32(0), (4096, 4096))], [ok_box])
    with pytest.raises(ValueError):
        X.xray_counts_host([np.zeros((0, 5), np.float32)], [ok_box])
    with pytest.raises(ValueError):
        X.xray_counts_host([dm, dm], [ok_box])


def test_load_boxes_equals_the_references_load_paths(gold):
    ref = json.loads(str(gold["load_paths"]))
    meta = [tuple(r) for r in ref["metadata"]]
    bbox = [tuple(r) for r in ref["bbox"]]
    got = X.load_boxes(meta, bbox, ref["diseases"], seed=ref["seed"])
    want = [(k, [(a, tuple(b)) for a, b in v]) for k, v in ref["parent"]]
    assert list(got.items()) == want
    assert X.load_boxes(meta, bbox, ref["diseases"], seed=ref["seed"], image_folder="data/images")["Nodule"][0][0] == \
        os.path.join("data/images", want[[k for k, _ in want].index("Nodule")][1][0][0])


def test_xray_report_writes_the_references_files(tmp_path):
    from diff_mining_amd.typicality import TypicalityScorer
    sc = object.__new__(TypicalityScorer)                   # no engine: the evaluation is replaced by the host path on stored maps
    maps = {"/x/a.png": ("a", XC.case_box("a")), "/x/b.png": ("b", XC.case_box("b")), "/x/d.jpg": ("d", XC.case_box("d"))}
    calls = []

    def evaluate(paths, sizes, boxes, images_per_call=8):
        calls.append((list(paths), list(sizes)))
        tp, fp, n_in, s = X.xray_counts_host([XC.case_map(maps[p][0]) for p in paths], boxes)
        mean, auc = X.xray_scores_from_counts(tp, fp, n_in, s)
        return {"mean_typicality": mean, "auc": auc}
    sc.xray_evaluate = evaluate
    parent = {"Mass": [("/x/b.png", maps["/x/b.png"][1]), ("/x/a.png", maps["/x/a.png"][1])], "Nodule": [],
              "Effusion": [("/x/d.jpg", maps["/x/d.jpg"][1])]}
    sizes = {p: XC.case_map(t).shape for p, (t, _) in maps.items()}
    report, auc = sc.xray_report(parent, str(tmp_path / "out"), image_sizes=sizes)
    assert calls[0] == (["/x/b.png", "/x/a.png"], [(33, 47), (96, 80)])
    on_disk = json.load(open(tmp_path / "out" / "report.json")), json.load(open(tmp_path / "out" / "auc.json"))
    for got, disk in zip((report, auc), on_disk):
        assert list(got) == list(disk) == ["Mass", "Effusion"]                       # a finding without entries is dropped
        assert list(disk["Mass"]) == ["b.png", "a.png"] and list(disk["Effusion"]) == ["d.jpg"]
        assert all(type(v) is float for d in got.values() for v in d.values())
    gold = np.load(GOLDEN)
    assert on_disk[1]["Mass"]["a.png"] == float(gold["a_auc"]) and on_disk[1]["Mass"]["b.png"] == float(gold["b_auc"])
    assert np.isnan(on_disk[0]["Effusion"]["d.jpg"]) and np.isnan(on_disk[1]["Effusion"]["d.jpg"])
    assert open(tmp_path / "out" / "auc.json").read().startswith('{\n    "Mass": {\n        "b.png": ')      # indent=4


def test_compare_reports(tmp_path):
    pt, ft = tmp_path / "pt", tmp_path / "ft"
    X.write_reports(str(pt), ["Mass", "Nodule"], {"Mass": ["a", "b"], "Nodule": ["c"]},
                    {"Mass": [1.0, 3.0], "Nodule": [0.5]}, {"Mass": [0.25, 0.75], "Nodule": [0.125]})
    X.write_reports(str(ft), ["Mass", "Nodule"], {"Mass": ["a", "b", "extra"], "Nodule": ["c"]},
                    {"Mass": [2.0, 6.0, 100.0], "Nodule": [1.5]}, {"Mass": [0.5, 1.0, 9.0], "Nodule": [0.625]})
    got = X.compare_reports(str(pt), str(ft))
    assert got["auc"]["Mass"] == {"ft": (0.75, 0.25), "pt": (0.5, 0.25), "delta": 0.25}        # over the pre-trained run's names only
    assert got["auc"]["Nodule"] == {"ft": (0.625, 0.0), "pt": (0.125, 0.0), "delta": 0.5}
    assert got["typicality"]["Mass"] == {"ft": (4.0, 2.0), "pt": (2.0, 1.0)}
    assert list(got["auc"]) == ["Mass", "Nodule"]
