"""CPU tier of the detector initialisation (diff-mining_amd/doersch.py): the host restatement of the greedy ranking
against the reference's own run (tests/golden/detector_init_ref.json, tests/make_golden_detector_init.py), the integer IoU predicate,
`sample_patches` against the reference's `init_patches`, the host side of `CandidateSearch`, and the ABI of the new entries."""
import os
import random
import re

import numpy as np
import pytest

from diff_mining_amd import doersch as D
from diff_mining_amd import engine as E
from tests import detector_init_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dm_dense_wide_workspace_bytes", "dm_dense_wide_winners", "dm_dense_wide_topk", "dm_detector_rank_workspace_bytes",
               "dm_detector_rank")


@pytest.fixture(scope="module")
def gold():
    return IC.golden()


@pytest.mark.parametrize("tag", list(IC.RANKING))
def test_host_ranking_equals_the_reference(gold, tag):
    arrays = IC.ranking(tag)
    patches = IC.patches_of(arrays)
    got = D.rank_init_detectors_host(IC.RANKING[tag]["num_detectors"], IC.stats_of(arrays), patches)
    want = gold["ranking"][tag]["accepted"]
    assert [k for k, _, _ in got] == want
    assert all(p == patches[k] and w == k for k, p, w in got)                        # (index, patches[index], stats['w'][index])
    assert D.rank_init_detectors(IC.RANKING[tag]["num_detectors"], IC.stats_of(arrays), patches) == got    # no device arrays: the host


def test_the_fixture_exercises_the_rules(gold):
    """what tests/make_golden_detector_init.py asserted of the reference's run when it wrote the fixture"""
    ends = set()
    for tag in IC.RICH:
        f = gold["ranking"][tag]
        assert 4 * f["rejected"] >= f["visited"] and len(f["accepted"]) >= 8
        assert f["reject_at_6"] >= 1 and f["accept_at_5"] >= 1 and f["inter_1792"] >= 1 and f["inter_1920"] >= 1
        ends.add(f["ends"])
    assert ends == {"full", "exhausted"}


def test_integer_iou_equals_the_float_predicate():
    """every overlap of two 64-pixel boxes on the 8-pixel grid, and every inter 0 ... box^2 for the boxes the docstring covers"""
    for dx in range(0, 72, 8):
        for dy in range(0, 72, 8):
            inter = max(0, 64 - dx) * max(0, 64 - dy)
            area = 64 * 64
            assert D.iou_above_03(inter, 64) == (inter / (area + area - inter) > 0.3), (dx, dy)
    assert not D.iou_above_03(1792, 64) and D.iou_above_03(1920, 64)
    for box in (1, 7, 10, 64, 65, 130, 2048):
        inter = np.arange(0, box * box + 1, dtype=np.int64) if box <= 130 else \
            np.unique(np.clip(np.int64(6 * box * box // 13) + np.arange(-2000, 2001), 0, box * box))
        want = inter / (2.0 * box * box - inter) > 0.3
        assert np.array_equal(13 * inter > 6 * box * box, want), box


def test_exact_three_tenths_is_not_above():
    """inter / (2 A - inter) = 3 / 10 exactly when 13 inter = 6 A: A = 13^2 (box 13), inter = 78: the float quotient is the double 0.3"""
    assert 13 * 78 == 6 * 169 and 78 / (2 * 169 - 78) == 0.3 and not D.iou_above_03(78, 13)
    assert D.iou_above_03(79, 13) and 79 / (2 * 169 - 79) > 0.3


def test_sample_patches_reproduces_the_reference(gold):
    g = gold["sample"]
    random.seed(g["seed"])
    np.random.seed(g["seed"])
    got = D.sample_patches(IC.sample_sizes(), g["how_many"], g["num_trials"], IC.sample_accept)
    assert [[list(b), p] for b, p in got] == g["patches"]
    assert all(type(v) is int for b, _ in got for v in b)
    # a generator of the caller's: the same loop, another stream; accept=None takes the first position of every visit
    a = D.sample_patches(IC.sample_sizes(), 12, rng=np.random.RandomState(3))
    b = D.sample_patches(IC.sample_sizes(), 12, rng=np.random.RandomState(3))
    assert a == b and len(a) == 12 and len({p for _, p in a[:5]}) == 5                # round-robin over the five images
    for (x0, y0, x1, y1), path in a:
        W, H = IC.sample_sizes()[path]
        assert x1 - x0 == y1 - y0 == 64 and x0 % 8 == y0 % 8 == 0 and x0 // 8 < W // 8 - 8 and y0 // 8 < H // 8 - 8
    with pytest.raises(ValueError):
        D.sample_patches({"tiny.jpg": (64, 200)}, 1)


def test_candidate_search_host_equals_the_narrow_host_search():
    """the host path of `CandidateSearch` (blocks of 128 through `winners_host`) against `DenseSearch` on the same detectors, K = 130
    split 128 + 2; boxes, d20 and the arrays the ranking takes"""
    w, chunks = IC.wide_inputs("W3")
    w, chunks = w[:, :72].copy(), [(p, np.ascontiguousarray(d[..., :72]), m) for p, d, m in chunks]
    positive = [chunks[0][0][1]]
    cs = D.CandidateSearch(w, positive, top_k=2)
    for paths, data, mask in chunks:
        cs.add(paths, data, mask)
    stats = cs.result()
    score, cell = cs.tables()
    for k0 in (0, 128):
        ds = D.DenseSearch(w[k0:k0 + 128], top_k=2, scores="f32")
        for paths, data, mask in chunks:
            ds.add(paths, data, mask)
        s, c = ds.tables()
        assert s.tobytes() == score[k0:k0 + 128].tobytes() and c.tobytes() == cell[k0:k0 + 128].tobytes()
        lists = ds.result()
        for k, entries in enumerate(lists):
            assert stats["neighbors"][k0 + k] == [(bbox, path) for _, bbox, path in entries]
        assert [stats["discriminative-20"][k0 + k] for k in range(len(lists))] == D.discriminative_20(lists, positive)
    a = stats["arrays"]
    assert a["key"].dtype == a["nb_image"].dtype == a["nb_x"].dtype == a["nb_count"].dtype == np.int32
    assert a["nb_image"].shape == (130, 2) and (a["nb_count"] == 2).all()
    assert stats["w"][129].tobytes() == w[129].tobytes()
    with pytest.raises(ValueError):
        D.CandidateSearch(np.zeros((D.DENSE_WIDE_MAX_DETECTORS + 1, 8), dtype=np.float16), [])


def test_initialize_classifier_composes_the_three_stages(tmp_path):
    """host path end to end on three small image files: the patches are `sample_patches`' under the same generator, the result is
    `rank_init_detectors` of `init_detectors_images`' stats, and every accepted row is the feature row under its patch"""
    from PIL import Image
    names = []
    for j, im in enumerate(IC.compose_images(3)[:3]):
        names.append(str(tmp_path / f"s{j}.png"))
        Image.fromarray(im).save(names[-1])
    patches, init = D.initialize_classifier(names, names, names[:1], how_many=6, num_detectors=4, rng=np.random.RandomState(5), batch=2,
                                            top_k=2, device_id="cpu")
    sizes = {n: (W, H) for n, (H, W) in zip(names, IC.COMPOSE["sizes"])}
    assert patches == D.sample_patches(sizes, 6, rng=np.random.RandomState(5))
    stats = D.init_detectors_images(patches, names, names[:1], batch=2, top_k=2, device_id="cpu")
    assert [(k, p) for k, p, _ in init] == [(k, p) for k, p, _ in D.rank_init_detectors_host(4, stats, patches)] and 1 <= len(init) <= 4
    for k, (bbox, path), w in init:
        feat = D.hoglab(np.asarray(Image.open(path))[None])[0]
        assert patches[k] == (bbox, path) and w.tobytes() == feat[bbox[0] // 8, bbox[1] // 8].tobytes()
        assert stats["neighbors"][k][0] == ((bbox[0], bbox[1]), path)                # a candidate finds itself first
    with pytest.raises(ValueError):
        D.init_detectors_images([((0, 0, 64, 64), "elsewhere.png")], names, [], device_id="cpu")


def test_abi_names_the_new_entries():
    """fails on the parent commit: the table and the header carry the wide search and the ranking"""
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in E.SIGNATURES and name in declared, name
    assert re.search(r"#define\s+DM_DENSE_WIDE_MAX_DETECTORS\s+32768\b", hdr) and D.DENSE_WIDE_MAX_DETECTORS == 32768
    for name, value in (("N", D.RANK_MAX_N), ("L", D.RANK_MAX_L), ("DETECTORS", D.RANK_MAX_DETECTORS), ("BOX", D.RANK_MAX_BOX)):
        assert re.search(rf"#define\s+DM_DETECTOR_RANK_MAX_{name}\s+{value}\b", hdr), name
    assert E.SIGNATURES["dm_dense_wide_winners"] == E.SIGNATURES["dm_dense_search_winners"]
    lib = E.load_library()
    assert lib.dm_dense_wide_workspace_bytes(16, 3249, 32768) == 16 * 32768 * 8
    assert lib.dm_dense_wide_workspace_bytes(16, 3249, 32769) == 0 and lib.dm_dense_wide_workspace_bytes(0, 1, 1) == 0
    assert lib.dm_detector_rank_workspace_bytes(25000, 50, 1000) == 4 * (25000 + 3 * 50 * 1000)
    for bad in ((0, 1, 1), (32769, 1, 1), (1, 0, 1), (1, 129, 1), (1, 1, 0), (1, 1, 4097)):
        assert lib.dm_detector_rank_workspace_bytes(*bad) == 0, bad
