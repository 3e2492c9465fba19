#!/usr/bin/env python
"""Golden vectors for the detector initialisation, produced by the reference's own functions run on the build machine.

`doersch/doersch.py` cannot be imported here (its imports are absent), but `iou` (doersch/utils.py), `accept_patch_neighbor` and
`Doersch.rank_init_detectors` are plain Python, and so is `Doersch.init_patches` once PIL and the contrast filter are stubbed.  This
script parses the two files with `ast`, compiles those four (their text, unmodified, written nowhere) with `tqdm` stubbed, runs
`rank_init_detectors` on the ranking cases of tests/detector_init_cases.py and `init_patches` under seeded global generators.
Output: tests/golden/detector_init_ref.json — per ranking case the accepted indices in acceptance order and the figures below, the
recorded patch sequence, and the seed of the composition case.  Needs /root/reference (the build machine only).

Per rich ranking case (detector_init_cases.RICH) the script replays the reference's visit with the reference's `iou` and asserts
that the case exercises the rules, so that a fixture which the kernel could meet by accident is not written:
  (a) at least a quarter of the visited candidates are rejected,        (b) at least eight are accepted,
  (c) one case ends by reaching num_detectors and another by exhausting the candidates,
  (d) a rejection is decided by exactly max_pairs + 1 pairs and an acceptance happens with exactly max_pairs pairs against some
      accepted detector,
  (e) a tested pair has 13 inter one step on either side of 6 A: overlaps of 32 x 56 = 1792 (below) and 40 x 48 = 1920 (above).

The composition case (images -> features -> wide search -> ranking, device against host): the seed is the first whose host run has
every gap the comparison relies on — winner against runner-up cell of every listed (candidate, image), and the consecutive scores of
a candidate's first top_k + 1 images — at least GAP_FACTOR x the distance between the host path in fp64 and the same path with the
features computed in fp32 arithmetic (what the device does), as tests/make_golden_dense_search.py does for its cases.

    python tests/make_golden_detector_init.py
"""
import ast
import json
import os
import sys
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_mining_amd import doersch as D  # noqa: E402
from tests import detector_init_cases as IC  # noqa: E402

REF = "/root/reference/doersch/doersch.py"
REF_UTILS = "/root/reference/doersch/utils.py"
GAP_FACTOR = 16
MAX_SEEDS = 200


class _Bar:
    def __init__(self, *a, **k):
        pass

    def update(self, n=1):
        pass


def reference_functions():
    ns = {"defaultdict": defaultdict, "tqdm": _Bar}
    body = [n for n in ast.parse(open(REF_UTILS).read()).body if isinstance(n, ast.FunctionDef) and n.name == "iou"]
    for node in ast.parse(open(REF).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == "accept_patch_neighbor":
            body.append(node)
        if isinstance(node, ast.ClassDef) and node.name == "Doersch":
            body += [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "rank_init_detectors"]
    assert [n.name for n in body] == ["iou", "accept_patch_neighbor", "rank_init_detectors"], [n.name for n in body]
    exec(compile(ast.Module(body=body, type_ignores=[]), REF, "exec"), ns)
    return ns["iou"], ns["rank_init_detectors"]


def reference_init_patches(sizes, how_many, num_trials, accept, seed):
    """`Doersch.init_patches` itself with PIL, the contrast filter and the progress bar stubbed, under seeded global generators"""
    import random
    import types

    class Img:
        def __init__(self, path):
            self.path, self.size = path, sizes[path]

        def crop(self, bbox):
            return self.path, tuple(int(v) for v in bbox)
    ns = {"np": np, "random": random, "tqdm": _Bar, "Image": types.SimpleNamespace(open=Img),
          "filter_by_contrast": lambda crop, threshold: accept(*crop)}
    for node in ast.parse(open(REF).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == "Doersch":
            body = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "init_patches"]
    exec(compile(ast.Module(body=body, type_ignores=[]), REF, "exec"), ns)
    me = types.SimpleNamespace(get_seeds=lambda c: list(sizes), threshold=None)
    random.seed(seed)
    np.random.seed(seed)
    return [[[int(v) for v in bbox], path] for bbox, path in ns["init_patches"](me, "c", how_many, num_trials)]


def replay(tag, arrays, accepted, iou):
    """the visit again, with the reference's accepted list as given and its `iou`: the figures of assertions (a) ... (e)"""
    s = IC.RANKING[tag]
    order = sorted(range(s["N"]), key=lambda k: int(arrays["key"][k]), reverse=True)           # stable, as the reference's sorted()
    taken, inside = [], set(accepted)
    fig = dict(visited=0, rejected=0, reject_at_6=0, accept_at_5=0, inter_1792=0, inter_1920=0)
    entries = lambda k: [(int(arrays["nb_image"][k, j]), int(arrays["nb_x"][k, j]), int(arrays["nb_y"][k, j]))   # noqa: E731
                         for j in range(int(arrays["nb_count"][k]))]
    for k in order:
        if len(taken) == s["num_detectors"]:
            break
        fig["visited"] += 1
        counts = []
        for d in taken:
            count = 0
            for im, x, y in entries(k):
                for imd, xd, yd in entries(d):
                    if im != imd:
                        continue
                    inter = max(0, 64 - abs(x - xd)) * max(0, 64 - abs(y - yd))
                    fig["inter_1792"] += inter == 1792
                    fig["inter_1920"] += inter == 1920
                    over = iou((x, y, x + 64, y + 64), (xd, yd, xd + 64, yd + 64)) > 0.3
                    assert over == D.iou_above_03(inter, 64)
                    count += over
            counts.append(count)
        ok = all(c <= IC.MAX_PAIRS for c in counts)
        assert ok == (k in inside), (tag, k, counts)
        if ok:
            assert accepted[len(taken)] == k
            fig["accept_at_5"] += IC.MAX_PAIRS in counts
            taken.append(k)
        else:
            fig["rejected"] += 1
            fig["reject_at_6"] += next(c for c in counts if c > IC.MAX_PAIRS) == IC.MAX_PAIRS + 1
    assert taken == list(accepted)
    fig["n_accepted"] = len(taken)
    fig["ends"] = "full" if len(taken) == s["num_detectors"] else "exhausted"
    return fig


def compose_gaps(seed):
    """-> (smallest gap the comparison relies on, distance of the fp32-feature path from the fp64-feature path), host arithmetic only"""
    images = IC.compose_images(seed)
    names = [f"c{j}.png" for j in range(len(images))]
    patches = IC.compose_patches(seed, names)
    top_k = IC.COMPOSE["top_k"]
    tables = []
    for dt in (np.float64, np.float32):
        feats = [D.hoglab_host(im, dtype=dt).astype(np.float16) for im in images]
        w = np.stack([feats[names.index(p)][b[0] // 8, b[1] // 8] for b, p in patches])
        full = [(f.reshape(-1, f.shape[-1]).astype(np.float64) @ w.astype(np.float64).T).T for f in feats]       # [K, cells] per image
        tables.append(full)
    dist = max(float(np.abs(a - b).max()) for a, b in zip(*tables))
    full = tables[0]
    best = np.stack([f.max(axis=1) for f in full], axis=1)                                                      # [K, n]
    gap = np.inf
    for k in range(len(patches)):
        ranked = np.argsort(-best[k], kind="stable")
        head = best[k, ranked[:top_k + 1]]
        gap = min(gap, float(np.min(head[:-1] - head[1:])))
        for b in ranked[:top_k]:
            two = np.sort(full[b][k])[-2:]
            gap = min(gap, float(two[1] - two[0]))
    return gap, dist


def main():
    if not os.path.isfile(REF):
        sys.exit("needs /root/reference")
    iou, rank = reference_functions()
    out = {"ranking": {}, "box": IC.BOX, "max_pairs": IC.MAX_PAIRS}
    ends = set()
    for tag, s in IC.RANKING.items():
        arrays = IC.ranking(tag)
        got = rank(None, s["num_detectors"], "c", IC.stats_of(arrays), IC.patches_of(arrays))
        accepted = [int(k) for k, _, _ in got]
        fig = replay(tag, arrays, accepted, iou)
        print(tag, fig)
        if tag in IC.RICH:
            assert 4 * fig["rejected"] >= fig["visited"], (tag, "a", fig)
            assert fig["n_accepted"] >= 8, (tag, "b", fig)
            assert fig["ends"] == s["ends"], (tag, "c", fig)
            assert fig["reject_at_6"] >= 1 and fig["accept_at_5"] >= 1, (tag, "d", fig)
            assert fig["inter_1792"] >= 1 and fig["inter_1920"] >= 1, (tag, "e", fig)
            ends.add(fig["ends"])
        out["ranking"][tag] = {"accepted": accepted, **{k: int(v) if not isinstance(v, str) else v for k, v in fig.items()}}
    assert ends == {"full", "exhausted"}, ends
    sample = dict(IC.SAMPLE)
    sample["patches"] = reference_init_patches(IC.sample_sizes(), sample["how_many"], sample["num_trials"], IC.sample_accept, sample["seed"])
    assert len(sample["patches"]) == sample["how_many"] and len({p for _, p in sample["patches"]}) == len(IC.sample_sizes())
    out["sample"] = sample
    for seed in range(MAX_SEEDS):
        gap, dist = compose_gaps(seed)
        print(f"compose seed {seed}: gap {gap:.3g}, fp32-vs-fp64 distance {dist:.3g}")
        if gap >= GAP_FACTOR * dist:
            out["compose"] = {"seed": seed, "gap": gap, "distance": dist, "gap_factor": GAP_FACTOR}
            break
    else:
        sys.exit(f"no composition seed below {MAX_SEEDS}")
    with open(IC.JSON, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", IC.JSON, os.path.getsize(IC.JSON), "bytes")


if __name__ == "__main__":
    main()
