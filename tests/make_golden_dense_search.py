#!/usr/bin/env python
"""Golden vectors for the dense detector search (needs the reference checkout that tests/make_golden_consumers.py reads).

    dense_search_cuda      doersch/hog.py:124-185
    accumulate, make_bbox  doersch/hog.py:111-122

Exact side.  Per case of tests/dense_search_cases.py the expectation is computed here in fp64 (products and sums of the fp16
operands, rounded to fp32 once; mask -> 0 unless NaN; NaN never wins; lowest cell / lowest image among equals), with

    tol32 = 8 x max |numpy fp32 matmul - fp64|          (8: the other summation order of the MFMA tree)

and the assertion that every gap the tests rely on is >= 16 tol32: winner against runner-up of every (detector, image),
consecutive ranks of every detector down to top_k + 1, and every winner against the `only_pos` threshold 0.  Two masked cells tie
at exactly 0 on every side; such ties are decided by the index rule and are part of the expectation.  A seed that fails the
assertion is replaced by the next one.  tol32, the gaps and the seed go to tests/golden/dense_search_ref.json.

Reference side (S1, S2 and S4 without its NaN; S3's broadcast would be 1.7 GB per image).  The reference's `dense_search_cuda`,
compiled from its text with `ast` (never written anywhere), runs with device_id="cpu" on safetensors shards in a temporary directory,
one shard per chunk.  If its loky / Manager machinery does not run, the function's own score, mask and top-1 statements and
`accumulate`'s merge statement are compiled and executed the same way; the json records the route.  Those statements also give
the reference's full fp16 score tensor, from which `ref_err` = max |reference fp16 score - exact| and the reference's score of any
cell (tests/test_dense_search.py) come.  Only results are stored: tests/golden/dense_search_ref.npz.

    python tests/make_golden_dense_search.py
"""
import ast
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from tests import dense_search_cases as DC  # noqa: E402
from tests.make_golden_consumers import REF, ref_function  # noqa: E402

HOG = "doersch/hog.py"
GAP_FACTOR = 16
MAX_SEEDS = 40


# ---- the exact side ------------------------------------------------------------------------------------------------------------------
def exact_case(tag, seed):
    """-> dict of arrays (the expectation), dict of figures (tol32, gaps), or None when a gap is too narrow"""
    s = DC.SHAPES[tag]
    K, top_k, cells = s["K"], s["top_k"], s["W"] * s["H"]
    w = DC.detectors(tag, seed)
    w64 = w.astype(np.float64)
    score = np.empty((K, 0), dtype=np.float32)
    cell = np.empty((K, 0), dtype=np.int32)
    full, dev32, win_gap = [], 0.0, np.inf
    for _, data, mask in DC.chunks(tag, seed):
        for b in range(len(data)):
            x = data[b].reshape(cells, -1)
            with np.errstate(all="ignore"):
                e64 = x.astype(np.float64) @ w64.T                                   # [cells, K]
                m32 = x.astype(np.float32) @ w.astype(np.float32).T
            ok = ~np.isnan(e64)
            if ok.any():
                dev32 = max(dev32, float(np.abs(m32.astype(np.float64) - e64)[ok].max()))
            masked = np.zeros(cells, dtype=bool) if mask is None else mask[b] == 0
            e64 = np.where(masked[:, None] & ~np.isnan(e64), 0.0, e64)               # NaN * 0 stays NaN
            full.append(e64.T.copy())
            sc, ce = np.empty(K, dtype=np.float32), np.empty(K, dtype=np.int32)
            for k in range(K):
                col = e64[:, k]
                live = [i for i in range(cells) if not np.isnan(col[i])] if cells <= 64 or np.isnan(col).any() else None
                if live is not None and not live:
                    sc[k], ce[k] = -np.inf, -1
                    continue
                c32 = col.astype(np.float32)
                if live is None:
                    i = int(np.argmax(c32))                                          # the first among equal fp32 values
                    others = np.delete(col, i)
                else:
                    i = max(live, key=lambda j: (c32[j], -j))
                    others = np.array([col[j] for j in live if j != i and not (masked[j] and masked[i])])
                sc[k], ce[k] = c32[i], i
                if len(others):
                    win_gap = min(win_gap, float(col[i] - others.max()))
            score = np.concatenate([score, sc[:, None]], axis=1)
            cell = np.concatenate([cell, ce[:, None]], axis=1)
    tol32 = 8 * dev32
    out = {"score": score, "cell": cell, "full64": np.stack(full, axis=1)}          # full64 [K, n, cells], not stored
    rank_gap, zero_gap = np.inf, np.inf
    n = score.shape[1]
    for only_pos in ((False, True) if tag.startswith("S4") else (False,)):
        ts = np.full((K, top_k), np.nan, dtype=np.float32)
        ti, tc = np.full((K, top_k), -1, dtype=np.int32), np.full((K, top_k), -1, dtype=np.int32)
        cnt = np.zeros(K, dtype=np.int32)
        for k in range(K):
            adm = [b for b in range(n) if score[k, b] != -np.inf and not np.isnan(score[k, b]) and (not only_pos or score[k, b] > 0)]
            order = sorted(adm, key=lambda b: (-float(score[k, b]), b))
            for a, b in zip(order[:top_k], order[1:top_k + 1]):
                if not (score[k, a] == 0 and score[k, b] == 0):                      # two masked zeros tie exactly everywhere
                    rank_gap = min(rank_gap, float(score[k, a]) - float(score[k, b]))
            cnt[k] = min(len(order), top_k)
            for j, b in enumerate(order[:top_k]):
                ts[k, j], ti[k, j], tc[k, j] = score[k, b], b, cell[k, b]
        sfx = "_pos" if only_pos else ""
        out.update({f"top_score{sfx}": ts, f"top_image{sfx}": ti, f"top_cell{sfx}": tc, f"count{sfx}": cnt})
    if tag.startswith("S4"):
        fin = score[np.isfinite(score) & (score != 0)]
        zero_gap = float(np.abs(fin).min())
    figures = {"seed": seed, "tol32": tol32, "fp32_matmul_dev": dev32, "winner_gap": win_gap, "rank_gap": rank_gap}
    if tag.startswith("S4"):
        figures["zero_gap"] = zero_gap
    if min(win_gap, rank_gap, zero_gap) < GAP_FACTOR * tol32:
        print(f"   {tag} seed {seed}: gaps {win_gap:.3g} / {rank_gap:.3g} / {zero_gap:.3g} against {GAP_FACTOR} x tol32 = {GAP_FACTOR * tol32:.3g}: next seed")
        return None
    if tag == "S4clean":
        # Among exactly equal scores `torch.topk` may return any cell, so every masked-zero winner in the reference's lists can name
        # another cell than the index rule does.  The case keeps them at or below 1 % of the entries: the 2 % the test grants the
        # second branch then still measures near-ties of the reference's fp16 arithmetic, not its unspecified tie order.
        zeros_listed = int((out["top_score"] == 0).sum())
        figures["masked_zero_entries_in_lists"] = zeros_listed
        if zeros_listed > 0.01 * out["top_score"].size:
            print(f"   {tag} seed {seed}: {zeros_listed} masked-zero winners in the lists the reference is compared on: next seed")
            return None
    if tag == "S4":                                                                  # the planted rules are really in the case
        zero_wins = (score == 0) & (cell >= 0)                                       # a masked zero over a negative maximum
        ties = sum(int((np.diff(out["top_score"][k][:out["count"][k]]) == 0).any()) for k in range(K))
        if not (zero_wins.any() and (out["count_pos"] < top_k).any() and (out["count_pos"] == top_k).any() and ties):
            print(f"   {tag} seed {seed}: a planted rule does not occur: next seed")
            return None
        assert (score[:, DC.S4_NAN_IMAGE] == -np.inf).all() and (cell[:, DC.S4_NAN_IMAGE] == -1).all()
        assert not (out["top_image"] == DC.S4_NAN_IMAGE).any()
        assert not (cell[:, DC.S4_NAN_ROW[0]] == DC.S4_NAN_ROW[1]).any()
        figures.update({"detectors_with_tied_ranks": ties, "masked_zero_winners": int(zero_wins.sum()),
                        "detectors_with_count_below_top_k": int((out["count_pos"] < top_k).sum())})
    return out, figures


# ---- the reference side --------------------------------------------------------------------------------------------------------------
def ref_namespace():
    from multiprocessing import Manager
    from joblib.externals.loky.backend.context import get_context
    from safetensors import safe_open
    from tqdm import tqdm
    ns = {"np": np, "torch": torch, "Manager": Manager, "get_context": get_context, "safe_open": safe_open, "tqdm": tqdm, "time": time}
    ref_function(HOG, ("accumulate",), ns)
    ref_function(HOG, ("make_bbox",), ns)
    return ns


def ref_statements():
    """The statements of dense_search_cuda's key loop from `data = data.reshape(B, W*H, C)` to `indexes = torch.topk(...)` (score,
    mask, top-1) and accumulate's merge statement, as code objects compiled from the reference's text."""
    path = os.path.join(REF, HOG)
    tree = ast.parse(open(path).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "dense_search_cuda")
    loop = next(n for n in ast.walk(fn) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "key")
    names = [ast.unparse(st.targets[0]) if isinstance(st, ast.Assign) else type(st).__name__ for st in loop.body]
    first = names.index("data", next(i for i, n in enumerate(names) if "B, W, H, C" in n))
    last = names.index("indexes")
    assert "If" in names[first:last], names
    body = ast.Module(body=loop.body[first:last + 1], type_ignores=[])
    acc = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "accumulate")
    merge = next(n for n in ast.walk(acc) if isinstance(n, ast.Assign) and "sorted(" in ast.unparse(n))
    return compile(body, path, "exec"), compile(ast.Module(body=[merge], type_ignores=[]), path, "exec")


def ref_by_statements(tag, seed, top_k):
    """-> (lists per detector [(score, bbox, path)], the reference's masked score tensor [K, n, cells] float32, its masks [n, cells] or None)"""
    s = DC.SHAPES[tag]
    K = s["K"]
    score_code, merge_code = ref_statements()
    device = torch.device("cpu")
    w = torch.from_numpy(DC.detectors(tag, seed)).to(device).half()
    sorted_buffer = [[] for _ in range(K)]
    full, masks = [], []
    ns0 = ref_namespace()
    for path_id, (paths, data, _) in enumerate(DC.chunks(tag, seed)):
        data = torch.from_numpy(data).to(device).half()
        B, W, H, C = data.shape
        ns = dict(ns0, data=data, w=w, K=K, B=B, W=W, H=H, C=C, fold=s["fold"], path_id=path_id, device=device)
        with torch.no_grad():
            exec(score_code, ns)
        scores, indexes = ns["scores"], ns["indexes"]
        full.append(scores.reshape(K, B, W * H).float().numpy())
        if s["fold"] is not None:
            masks.append(ns["mask"].numpy().astype(np.uint8))                        # the reference's own draw (hog.py:149-152)
        idx, val = indexes.indices.reshape(K, B, 1).numpy(), indexes.values.reshape(K, B, 1).numpy()
        obj = [[(val[k, b, 0], ns0["make_bbox"](idx[k, b, 0], (W, H)), paths[b]) for b in range(B)] for k in range(K)]
        for i in range(K):
            exec(merge_code, dict(sorted_buffer=sorted_buffer, obj=obj, i=i, top_k=top_k))
    return sorted_buffer, np.concatenate(full, axis=1), (np.concatenate(masks, axis=0) if masks else None)


def ref_by_function(tag, seed, top_k):
    from safetensors.torch import save_file
    ns = ref_namespace()
    fn = ref_function(HOG, ("dense_search_cuda",), ns)
    with tempfile.TemporaryDirectory() as td:
        shards = []
        for j, (paths, data, _) in enumerate(DC.chunks(tag, seed)):
            shards.append(os.path.join(td, f"{j}.safetensors"))
            save_file({";;".join(paths): torch.from_numpy(data)}, shards[-1])
        return fn(DC.detectors(tag, seed).astype(np.float32), shards, top_k=top_k, fold=DC.SHAPES[tag]["fold"], device_id="cpu")


def lists_equal(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(float(p[0]) == float(q[0]) and tuple(p[1]) == tuple(q[1]) and p[2] == q[2]
                                                              for p, q in zip(x, y)) for x, y in zip(a, b))


def main():
    if not os.path.isdir(REF):
        sys.exit("needs the reference checkout")
    arrays, report = {}, {"cases": {}, "gap_factor": GAP_FACTOR}
    groups = (("S1",), ("S2", "S4", "S4clean"), ("S3",))
    exact = {}
    for group in groups:
        for seed in range(MAX_SEEDS):
            got = [exact_case(tag, seed) for tag in group]
            if all(g is not None for g in got):
                break
        else:
            sys.exit(f"no seed below {MAX_SEEDS} for {group}")
        for tag, (out, figures) in zip(group, got):
            exact[tag] = out
            report["cases"][tag] = figures
            print(tag, figures)
            for name, a in out.items():
                if name != "full64":
                    arrays[f"{tag}_{name}"] = a

    route = None
    for tag, ref_tag in (("S1", "S1"), ("S2", "S2"), ("S4", "S4clean")):
        s, seed = DC.SHAPES[ref_tag], report["cases"][ref_tag]["seed"]
        lists, full, ref_mask = ref_by_statements(ref_tag, seed, s["top_k"])
        if ref_mask is not None:
            arrays[f"{tag}_ref_mask"] = ref_mask
        try:
            by_fn = [list(x) for x in ref_by_function(ref_tag, seed, s["top_k"])]
            assert lists_equal(by_fn, lists), "the statements do not restate the function"
            lists, this = by_fn, "dense_search_cuda(device_id='cpu') through its own loky / Manager machinery"
        except AssertionError:
            raise
        except Exception as e:                                                       # the process machinery did not run here
            this = f"the function's score, mask, top-1 and merge statements ({type(e).__name__}: the loky / Manager route did not run)"
        assert route in (None, this), (route, this)
        route = this
        K, top_k = s["K"], s["top_k"]
        names = DC.paths(ref_tag)
        arrays[f"{tag}_ref_score"] = np.array([[np.float32(e[0]) for e in lists[k]] for k in range(K)], dtype=np.float32)
        arrays[f"{tag}_ref_bbox"] = np.array([[e[1] for e in lists[k]] for k in range(K)], dtype=np.int32)
        arrays[f"{tag}_ref_image"] = np.array([[names.index(e[2]) for e in lists[k]] for k in range(K)], dtype=np.int32)
        arrays[f"{tag}_ref_full"] = full.astype(np.float16)
        assert np.array_equal(arrays[f"{tag}_ref_full"].astype(np.float32), full)   # fp16 values, whatever the mask promoted them to
        e64 = exact[ref_tag]["full64"]
        ref_err = float(np.abs(full.astype(np.float64) - e64).max())
        pick = full.argmax(axis=2)
        other = float((pick != exact[ref_tag]["cell"]).mean())
        report["cases"][tag].update({"ref_err": ref_err, "ref_other_cell_share": other})
        arrays[f"{tag}_ref_err"] = np.array(ref_err)
        print(f"{tag}: reference lists {arrays[f'{tag}_ref_score'].shape}, ref_err {ref_err:.3g}, the first maximum of its fp16 scores is another cell than the exact "
              f"winner in {other:.2%} of the pairs")
    report["reference_route"] = route
    os.makedirs(DC.GOLDEN_DIR, exist_ok=True)
    np.savez_compressed(DC.NPZ, **arrays)
    with open(DC.JSON, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("route:", route)
    print("wrote", DC.NPZ, os.path.getsize(DC.NPZ), "bytes;", DC.JSON)


if __name__ == "__main__":
    main()
