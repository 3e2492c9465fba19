"""The Doersch-2012 HOG+SVM baseline's dense detector search (doersch/hog.py:124-185, `dense_search_cuda`) on the GPU: every
detector against every cell of every image of the data set, keeping per detector the `top_k` images by their best cell.  Kernels:
csrc/dense_search.hip; C ABI: dm_dense_search_workspace_bytes / _winners / _topk / _gather (include/dm_engine.h).

The reference forms `(data.reshape(B*W*H, C).unsqueeze(1) * w.unsqueeze(0)).sum(-1)`, a [B W H, K, C] fp16 tensor, takes
`torch.topk(..., 1)` per (detector, image) and merges Python tuples on the host.  Here the product is an fp16 GEMM on the matrix
cores whose output never leaves the registers; what grows with the data set is two [K][n_images] tables.  The rules, which
`dense_search_host` (numpy) and the kernels share:

  score     s(k, b, i) = the sum over c of the exact products data[b, i, c] * w[k, c] of the fp16 operands, in fp32 (the device: MFMA
            fp32 accumulation; the host: fp64 products and sum, rounded to fp32).  -0 counts as +0.
  mask      a cell whose mask byte is 0 scores +0 exactly (the reference multiplies by the mask, hog.py:153: a masked cell beats
            every negative score), unless its score is NaN, which stays NaN (NaN * 0).
  winner    per (detector, image): the largest score, the lowest cell index among equal scores.  A NaN score never wins (the
            reference's `normalize` divides an all-zero cell by its zero norm, so NaN rows occur in real caches); an image with no
            non-NaN cell has score -inf and cell -1.
  top-k     per detector: descending score, ascending image index among equal scores (the reference's stable `sorted(...,
            reverse=True)` over entries in image order); -inf is never admitted; `only_pos` admits score > 0 only (hog.py:177).
  limits    1 <= K <= 128 detectors, 1 <= top_k <= 128, C >= 8 and C % 8 == 0, W H < 2^24.

An entry of the result is the reference's tuple `(score, (a * 8, b * 8), path)` with cell = a * H + b, plus the cell's feature row
with `ret_ws`.  Ranking is always by the fp32 score.  What an entry SHOWS is, with scores="f32", that fp32 score; by default
(scores="f16") a numpy.float16 scalar in the reference's own arithmetic, `reference_score_f16`: every product rounded to fp16, the
products summed, the sum rounded to fp16 — computed on the host from the winning cell's feature row, for the K top_k listed entries
only.  (Rounding the fp32 score instead would land one fp16 unit beside the reference's value wherever the exact sum lies near the
middle between two fp16 numbers.)  A masked winner shows 0.  Because the shown value is another sum than the ranked one, two
neighbours of a list that are closer than the reference's own error can show in ascending order.  (With `fold` the reference's
scores are float32 scalars that hold fp16 values, because its float32 mask promotes them; here the type does not depend on `fold`.)

The features themselves come from pixels by csrc/hoglab.hip (`hoglab`, `dense_search_images` below; C ABI dm_hoglab_*);
`dense_search` still takes the cached, normalised features the reference writes.

Between two searches the baseline fits one linear SVM per detector (`train_svm`, doersch/doersch.py:66-79: scikit-learn's
`SVC(C=0.1, kernel='linear')` on 5 positives and 10 000 - 25 000 negatives) and mines hard negatives.  Kernels: csrc/svm.hip; C ABI:
dm_svm_workspace_bytes / _fit / _hard_negatives; here `train_svms`, `train_svm`, `svm_round`, `sample_negatives`
(`random_sample`, hog.py:187-212).  The pin is scikit-learn's own iterate, not "an SVM optimum": at tol 1e-3 libsvm stops after a few
dozen steps, 6 - 35 % (rel-L2) short of the optimum.  The rules, which `svm_fit_host` (numpy) and the kernels share:

  problem   one detector: n_pos >= 1 rows labelled +1, then n_neg >= 1 rows labelled -1; fp16 rows, converted exactly; cost C
            (0.1), eps 1e-3, max_iter = libsvm's max(10 000 000, 100 n) unless given.
  order     libsvm sees the classes in ascending order: the negatives first, in their own order, as y = +1, then the positives as
            y = -1.  Ties are broken in that order; the sign is flipped at the end: w = -sum alpha_t y_t x_t, b = rho.
  state     alpha = 0 and G = -1 in fp64; QD[t] = x_t . x_t in fp64; Q_i[t] = (float)(y_i y_t (x_i . x_t)): libsvm's Qfloat is fp32
            and that rounding is part of the trajectory.  A dot is the sum of the exact products of the fp16 values in fp64 in a
            fixed order that depends on the feature count alone: lane l of 64 adds the products of the 8-feature chunks l, l + 64,
            ... one by one, then the 64 partials meet in an xor tree (`_svm_dots`).
  select i  the largest of -G[t] over y = +1 rows below the upper bound and G[t] over y = -1 rows above the lower bound; the LAST
            index among equals (libsvm compares with >=).
  select j  over y = +1 rows above the lower bound and y = -1 rows below the upper bound: grad_diff = Gmax + G[t] (y = +1) or
            Gmax - G[t] (y = -1); Gmax2 = the largest G[t] (y = +1) or -G[t] (y = -1); among those with grad_diff > 0 the lowest
            -grad_diff^2 / quad, quad = QD[i] + QD[t] - 2 y_i y_t Q_i[t], 1e-12 where that is not > 0; the LAST index among equals
            (libsvm compares with <=).
  stop      iter >= max_iter (status 1), else Gmax + Gmax2 < eps or no j (status 0).
  update    libsvm's two-variable update with its four clipping branches (Solver::Solve, one C for both classes), then
            G[t] += Q_i[t] d_alpha_i + Q_j[t] d_alpha_j in fp64 without fused multiply-add.
  rho       the mean of y_t G[t] over the free variables, summed in index order; with none free, the midpoint of libsvm's ub / lb.
  w         over the support vectors in ascending index, in fp64.
  shrinking not restated: the trajectory is SVC(shrinking=False)'s, which equals the default's at least while n_iter < min(n, 1000)
            (libsvm's first shrinking step); tests/golden/svm_ref.npz records per case whether it does.
  hard neg. over rows first = n_pos + n_hn ... n - 1 only: s = x . w + b in fp64 over all features in the fixed order (its own
            pass: y (G + 1) would carry the fp32 rounding of Q); admitted: s > 0; descending s, ascending position among equals (the
            reference's argsort leaves ties open); at most max_samples, as positions in the detector's sample list.
  refused   NaN / inf rows (status 2, w = NaN; the wrapper raises ValueError as scikit-learn does); n_pos < 1 or n_neg < 1; more
            than 128 detectors; a feature count below 8, above 8192 (the score pass stages w in 64 KB of LDS) or not a multiple of 8;
            n >= 2^24.

Before the first SVM round the baseline initialises its detectors (`initialize_classifier`, doersch/doersch.py:387-400): it samples
25 000 candidate patches (`init_patches`, :248-276; here `sample_patches`), turns every candidate into a detector and searches the
whole data set with all of them (`init_detectors`, :317-369; here `CandidateSearch`, `init_detectors`, `init_detectors_images`), and
greedily keeps the 1000 best whose neighbour lists do not overlap an accepted one's (`rank_init_detectors` / `accept_patch_neighbor`,
:371-385 and :46-64; here `rank_init_detectors`).  Kernels: csrc/dense_search_wide.hip; C ABI: dm_dense_wide_workspace_bytes /
_winners / _topk, dm_detector_rank_workspace_bytes / dm_detector_rank.  The wide search obeys the search rules above
with 1 <= K <= 32768, and its tables are bit-equal to the narrow search's over blocks of 128 detectors.  The ranking's rules, which
`rank_init_detectors_host` (plain Python) and the kernel share:

  order     candidates are taken by descending key (the discriminative-20 count; any int32), among equal keys by ascending index:
            Python's stable `sorted(..., reverse=True)` over a dict filled in index order.
  test      candidate k against accepted detector d: count = the number of pairs (entry i of k, entry j of d) with the same image and
            IoU > 0.3 of the boxes (x, y, x + box, y + box); k is rejected when count > max_pairs (5) for SOME d.  The count starts
            from zero for every d: pairs from different accepted detectors never add up.
  IoU       in integers: with inter = max(0, dx) max(0, dy) and A = box^2, the reference's float64 `inter / (2 A - inter) > 0.3` is
            the same predicate as 13 inter > 6 A for box <= 2048: a ratio of exactly 3 / 10 rounds to the very double the literal
            0.3 denotes (correct rounding of one rational), and any other ratio p / q, q <= 2 A, differs from 3 / 10 by at least
            1 / (10 * 2 A) >= 2^-27, far more than the rounding of the division (2^-53 relative), so it stays on its side.
  accept    append k; stop at num_detectors accepted or when the candidates run out.  accepted[0 ... n) are candidate indices in
            acceptance order; slots past n hold -1.
  contract  of the device entry: within one candidate's list every image occurs at most once (what a top-k over per-image winners
            yields); `detector_rank` checks it when the lists come from the host.  The host restatement counts all pairs and so
            covers the general case.
  limits    1 <= N <= 32768 candidates, 1 <= L <= 128 entries, 1 <= num_detectors <= 4096, 1 <= box <= 2048.

Not here: `filter_by_contrast` (skimage's `is_low_contrast`; `sample_patches` takes the caller's `accept`), the plots.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import EngineError, _p, load_library as _lib

DENSE_MAX_DETECTORS = 128        # DM_DENSE_MAX_DETECTORS
DENSE_MAX_TOPK = 128             # DM_DENSE_MAX_TOPK
DENSE_MAX_CELLS = 1 << 24        # W H >= 2^24 is refused
# DM_DENSE_E_* (include/dm_engine.h)
ERRORS = {1: "null argument", 2: "B, n_images or n < 1", 3: "cells < 1", 4: "cells >= 2^24", 5: f"K outside [1, {DENSE_MAX_DETECTORS}]",
          6: f"top_k outside [1, {DENSE_MAX_TOPK}]", 7: "C < 8 or not a multiple of 8", 8: "ld < image_offset + B", 9: "workspace too small",
          10: "misaligned pointer", 11: "HIP error"}


def _check(rc: int, what: str):
    if rc:
        raise EngineError(f"{what}: {ERRORS.get(rc, 'error')} (code {rc})")


def _check_shape(B, cells, C_, K, top_k=1):
    if B < 1 or cells < 1:
        raise ValueError(f"dense search: {B} images of {cells} cells")
    if cells >= DENSE_MAX_CELLS:
        raise ValueError(f"dense search: {cells} cells per image, 2^24 or more")
    if not 1 <= K <= DENSE_MAX_DETECTORS:
        raise ValueError(f"dense search: {K} detectors, need 1 ... {DENSE_MAX_DETECTORS}")
    if not 1 <= top_k <= DENSE_MAX_TOPK:
        raise ValueError(f"dense search: top_k {top_k}, need 1 ... {DENSE_MAX_TOPK}")
    if C_ < 8 or C_ % 8:
        raise ValueError(f"dense search: {C_} channels, need a multiple of 8 (2112 = 8 * 264)")


def fold_mask(path_id: int, B: int, cells: int, fold, device="cpu"):
    """The reference's fold mask of one shard key (hog.py:149-152) by its own calls: `torch.manual_seed(path_id)`, then one
    `torch.randperm(cells, device=device)[: i * cells // l]` per image, fold = (i, l); uint8 [B, cells] on `device`, 1 = the cell
    takes part.  Reseeds torch's global generators, as the reference does.  The bits of a permutation drawn on a GPU are
    torch-ROCm's: they equal neither the CPU's nor CUDA's, so a fold drawn on the device selects other cells than the reference did
    on its machine (the same share of them); draw on "cpu" where the cells themselves have to agree."""
    import torch
    i, l = int(fold[0]), int(fold[1])
    torch.manual_seed(int(path_id))
    indices = torch.stack([torch.randperm(cells, device=device)[:(i * cells) // l] for _ in range(B)])
    return torch.zeros(B, cells, dtype=torch.uint8, device=device).scatter_(1, indices, 1)


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement: the CPU-tier yardstick, and the path a numpy input takes
# ------------------------------------------------------------------------------------------------------------------------------
def winners_host(data, w, mask=None):
    """data fp16 [B, cells, C] (or [B, W, H, C]), w fp16 [K, C], mask [B, cells] or None -> (score float32 [K, B], cell int32
    [K, B]) by the rules at the top of this module."""
    data, w = np.asarray(data), np.asarray(w)
    if data.dtype != np.float16 or w.dtype != np.float16:
        raise ValueError("dense search: data and w must be float16")
    data = data.reshape(data.shape[0], -1, data.shape[-1])
    B, cells, C_ = data.shape
    K = w.shape[0]
    _check_shape(B, cells, C_, K)
    if w.ndim != 2 or w.shape[1] != C_:
        raise ValueError(f"dense search: w {w.shape} against {C_} channels")
    score, cell = np.empty((K, B), dtype=np.float32), np.empty((K, B), dtype=np.int32)
    w64 = w.astype(np.float64).T
    with np.errstate(all="ignore"):
        for b in range(B):
            s = (data[b].astype(np.float64) @ w64).astype(np.float32) + np.float32(0)      # [cells, K]; -0 -> +0
            valid = ~np.isnan(s)
            if mask is not None:
                s[np.asarray(mask)[b].reshape(-1) == 0] = 0
            t = np.where(valid, s, -np.inf)
            best = t.max(axis=0)                                                            # [K]
            first = (valid & (t == best[None, :])).argmax(axis=0)                          # the lowest cell among equals
            none = ~valid.any(axis=0)
            score[:, b] = np.where(none, -np.inf, best)
            cell[:, b] = np.where(none, -1, first)
    return score, cell


def reference_score_f16(row, w_k, score_f32=None):
    """The reference's fp16 value of one (cell, detector) pair (hog.py:144): `(row * w_k).sum()` with fp16 products (each the
    correctly rounded product of two fp16 numbers) and an fp16 result; the products are summed in fp64 here, in fp32 by torch on a
    CPU, which differ only where the sum lies within an fp32 rounding of the middle between two fp16 numbers.  A winner whose fp32
    score is exactly 0 is a masked cell (`scores * mask`): 0."""
    if score_f32 is not None and score_f32 == 0:
        return np.float16(0)
    with np.errstate(all="ignore"):
        return np.float16((np.asarray(row, dtype=np.float16) * np.asarray(w_k, dtype=np.float16)).astype(np.float64).sum())


def topk_host(score, cell, top_k: int, only_pos: bool = False):
    """score float32 [K, n], cell int32 [K, n] -> (top_score float32 [K, top_k], top_image int32, top_cell int32, count int32
    [K]); slots from count on hold NaN / -1 / -1."""
    score, cell = np.asarray(score, dtype=np.float32), np.asarray(cell, dtype=np.int32)
    K, n = score.shape
    top_score = np.full((K, top_k), np.nan, dtype=np.float32)
    top_image, top_cell = np.full((K, top_k), -1, dtype=np.int32), np.full((K, top_k), -1, dtype=np.int32)
    count = np.zeros(K, dtype=np.int32)
    for k in range(K):
        s = score[k]
        ok = ~np.isnan(s) & (s != -np.inf)
        if only_pos:
            ok &= s > 0
        idx = np.nonzero(ok)[0]
        idx = idx[np.argsort(-s[idx].astype(np.float64), kind="stable")][:top_k]            # stable: ascending image among equals
        count[k] = len(idx)
        top_score[k, :len(idx)], top_image[k, :len(idx)], top_cell[k, :len(idx)] = s[idx], idx, cell[k, idx]
    return top_score, top_image, top_cell, count


# ------------------------------------------------------------------------------------------------------------------------------
# the device calls
# ------------------------------------------------------------------------------------------------------------------------------
def workspace_bytes(B: int, cells: int, K: int) -> int:
    need = _lib().dm_dense_search_workspace_bytes(int(B), int(cells), int(K))
    if not need:
        raise ValueError(f"dense search: no workspace for {B} images of {cells} cells and {K} detectors")
    return need


def _stream(torch, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def winners(data, w, score, cell, image_offset: int = 0, mask=None, work=None):
    """dm_dense_search_winners on the current stream: data fp16 [B, cells, C] and w fp16 [K, C] on the GPU, contiguous; writes
    column image_offset + b of the tables score fp32 / cell int32 [K, ld].  work: a uint8 workspace of at least
    `workspace_bytes(B, cells, K)` to reuse."""
    import torch
    B, cells, C_ = data.shape
    K, ld = score.shape
    dev = data.device
    need = workspace_bytes(B, cells, K)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_dense_search_winners(_stream(torch, dev), _p(data), _p(w), _p(mask), B, cells, C_, K, int(image_offset), ld,
                                            _p(work), work.numel() * work.element_size(), _p(score), _p(cell))
    _check(rc, "dm_dense_search_winners")
    return work


def topk(score, cell, n_images: int, top_k: int, only_pos: bool = False):
    """dm_dense_search_topk on the current stream over columns [0, n_images) of the tables -> device tensors (top_score fp32
    [K, top_k], top_image int32, top_cell int32, count int32 [K])."""
    import torch
    K, ld = score.shape
    dev = score.device
    top_score = torch.empty((K, top_k), dtype=torch.float32, device=dev)
    top_image = torch.empty((K, top_k), dtype=torch.int32, device=dev)
    top_cell = torch.empty((K, top_k), dtype=torch.int32, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_dense_search_topk(_stream(torch, dev), _p(score), _p(cell), K, int(n_images), ld, int(top_k), int(bool(only_pos)),
                                         _p(top_score), _p(top_image), _p(top_cell), _p(count))
    _check(rc, "dm_dense_search_topk")
    return top_score, top_image, top_cell, count


def gather(data, pairs):
    """dm_dense_search_gather: data fp16 [B, cells, C] on the GPU, pairs int32 [n, 2] = (image in the chunk, cell) on the GPU ->
    fp16 [n, C], bit copies."""
    import torch
    B, cells, C_ = data.shape
    n = pairs.shape[0]
    out = torch.empty((n, C_), dtype=torch.float16, device=data.device)
    with torch.cuda.device(data.device):
        rc = _lib().dm_dense_search_gather(_stream(torch, data.device), _p(data), B, cells, C_, _p(pairs), n, _p(out))
    _check(rc, "dm_dense_search_gather")
    return out


class DenseSearch:
    """The search of one set of detectors over a data set that arrives in chunks.

        ds = DenseSearch(w, top_k=50)
        for paths, data in chunks: ds.add(paths, data)          # data: fp16 [B, W, H, C] on the GPU
        lists = ds.result()                                     # per detector [(score, (a * 8, b * 8), path), ...], score descending

    w: [K, C], any float type, rounded to fp16 as the reference does.  State that grows with the data set: the two [K][n_images]
    tables of winners (grown by doubling) and the list of paths.  The winning rows are kept when `result(ret_ws=True)` needs them
    (keep_rows=True) or the shown scores do (scores="f16", the default): after every chunk the running top-k is taken and the
    feature rows of this chunk's entries in it are gathered, rows that fell out are dropped — at most K top_k rows are alive, never
    [K][n_images][C]; it costs one top-k launch and one small device-to-host copy per chunk.  scores="f32" without keep_rows keeps
    no rows and never synchronises before `result`.
    A numpy `data` takes the host restatement (`winners_host` / `topk_host`); chunks must be all numpy or all on one GPU."""

    def __init__(self, w, top_k: int = 50, only_pos: bool = False, keep_rows: bool = False, scores: str = "f16"):
        if scores not in ("f16", "f32"):
            raise ValueError(f"dense search: scores={scores!r}, need 'f16' or 'f32'")
        w = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
        if w.ndim != 2:
            raise ValueError(f"dense search: w must be [K, C], got {w.shape}")
        self.w = np.ascontiguousarray(w.astype(np.float16))
        self.K, self.C = self.w.shape
        self.top_k, self.only_pos, self.keep_rows, self.scores = int(top_k), bool(only_pos), bool(keep_rows) or scores == "f16", scores
        _check_shape(1, 1, self.C, self.K, self.top_k)
        self.paths, self.dims = [], []           # per image: its path and (W, H)
        self.n = 0
        self._host = None                        # True: numpy chunks; False: device chunks
        self._score = self._cell = self._w_dev = self._work = None
        self._rows = {}                          # (detector, image) -> feature row, while the entry is inside the running top-k

    # -- chunks ----------------------------------------------------------------------------------------------------------------
    def add(self, paths, data, mask=None):
        """One chunk: `paths` of its B images, data fp16 [B, W, H, C], mask [B, W H] (0 = the cell scores 0) or None."""
        if data.ndim != 4 or data.shape[0] != len(paths) or data.shape[3] != self.C:
            raise ValueError(f"dense search: chunk {tuple(data.shape)} for {len(paths)} paths and {self.C} channels")
        B, W, H, _ = data.shape
        _check_shape(B, W * H, self.C, self.K, self.top_k)
        if mask is not None and tuple(mask.shape) != (B, W * H):
            raise ValueError(f"dense search: mask {tuple(mask.shape)}, need {(B, W * H)}")
        host = isinstance(data, np.ndarray)
        if self._host is None:
            self._host = host
        elif self._host != host:
            raise ValueError("dense search: numpy and device chunks in one search")
        (self._add_host if host else self._add_device)(data, mask, B, W * H)
        self.paths += list(paths)
        self.dims += [(W, H)] * B
        self.n += B

    def _grow(self, B, empty, copy):
        cap = 0 if self._score is None else self._score.shape[1]
        if self.n + B <= cap:
            return
        cap = max(2 * cap, self.n + B, 64)
        score, cell = empty((self.K, cap), "float32"), empty((self.K, cap), "int32")
        if self.n:
            copy(score, self._score)
            copy(cell, self._cell)
        self._score, self._cell = score, cell

    def _add_host(self, data, mask, B, cells):
        if data.dtype != np.float16:
            raise ValueError("dense search: data must be float16")

        def copy(dst, src):
            dst[:, :self.n] = src[:, :self.n]
        self._grow(B, lambda s, dt: np.empty(s, dtype=dt), copy)
        data = data.reshape(B, cells, self.C)
        s, c = winners_host(data, self.w, None if mask is None else np.asarray(mask))
        self._score[:, self.n:self.n + B], self._cell[:, self.n:self.n + B] = s, c
        if self.keep_rows:
            _, img, cell, count = topk_host(self._score[:, :self.n + B], self._cell[:, :self.n + B], self.top_k, self.only_pos)
            self._keep(img, cell, count, lambda pairs: data[pairs[:, 0], pairs[:, 1]].copy())

    def _add_device(self, data, mask, B, cells):
        import torch
        if not (isinstance(data, torch.Tensor) and data.is_cuda):
            raise EngineError("DenseSearch.add: data must be a torch tensor on the GPU, or numpy for the host restatement")
        if data.dtype != torch.float16:
            raise ValueError("dense search: data must be float16")
        dev = data.device
        if self._w_dev is None:
            self._w_dev = torch.from_numpy(self.w).to(dev)
        elif self._w_dev.device != dev:
            raise ValueError(f"dense search: a chunk on {dev}, earlier ones on {self._w_dev.device}")
        data = data.contiguous().view(B, cells, self.C)
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.uint8).contiguous()

        def copy(dst, src):
            dst[:, :self.n].copy_(src[:, :self.n])
        self._grow(B, lambda s, dt: torch.empty(s, dtype=getattr(torch, dt), device=dev), copy)
        need = workspace_bytes(B, cells, self.K)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=dev)
        winners(data, self._w_dev, self._score, self._cell, self.n, mask, self._work)
        if self.keep_rows:
            _, img, cell, count = topk(self._score, self._cell, self.n + B, self.top_k, self.only_pos)
            img, cell, count = img.cpu().numpy(), cell.cpu().numpy(), count.cpu().numpy()
            self._keep(img, cell, count,
                       lambda pairs: gather(data, torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev)).cpu().numpy())

    def _keep(self, img, cell, count, rows_of):
        """The running top-k after a chunk: fetch the rows of its entries that lie in this chunk, drop the rows that fell out."""
        alive, want = set(), []
        for k in range(self.K):
            for j in range(int(count[k])):
                key = (k, int(img[k, j]))
                alive.add(key)
                if key[1] >= self.n:
                    want.append((key, (key[1] - self.n, int(cell[k, j]))))
        self._rows = {key: row for key, row in self._rows.items() if key in alive}
        if want:
            rows = rows_of(np.array([p for _, p in want], dtype=np.int64))
            for (key, _), row in zip(want, rows):
                self._rows[key] = row

    # -- the answer ------------------------------------------------------------------------------------------------------------
    def tables(self):
        """(score float32 [K, n_images], cell int32 [K, n_images]) as numpy arrays: the winner of every (detector, image) so far."""
        if not self.n:
            raise ValueError("dense search: no chunk yet")
        if self._host:
            return self._score[:, :self.n].copy(), self._cell[:, :self.n].copy()
        return self._score[:, :self.n].cpu().numpy(), self._cell[:, :self.n].cpu().numpy()

    def topk(self):
        """(top_score float32 [K, top_k], top_image int32, top_cell int32, count int32 [K]) as numpy arrays."""
        if not self.n:
            raise ValueError("dense search: no chunk yet")
        if self._host:
            return topk_host(self._score[:, :self.n], self._cell[:, :self.n], self.top_k, self.only_pos)
        return tuple(t.cpu().numpy() for t in topk(self._score, self._cell, self.n, self.top_k, self.only_pos))

    def result(self, ret_ws: bool = False):
        """The reference's return value: per detector a list, score descending, of (score, (a * 8, b * 8), path), with the winning
        cell's feature row (numpy float16 [C]) appended under ret_ws (needs keep_rows=True or scores="f16").  Unlike the reference, a detector
        without an admissible entry gives an empty list instead of a failed assertion."""
        if ret_ws and not self.keep_rows:
            raise ValueError("dense search: result(ret_ws=True) with scores='f32' needs DenseSearch(..., keep_rows=True)")
        top_score, top_image, top_cell, count = self.topk()
        out = []
        for k in range(self.K):
            entries = []
            for j in range(int(count[k])):
                img, cell = int(top_image[k, j]), int(top_cell[k, j])
                W, H = self.dims[img]
                s = top_score[k, j] if self.scores == "f32" else reference_score_f16(self._rows[(k, img)], self.w[k], top_score[k, j])
                bbox = ((cell // H) * 8, (cell % H) * 8)                 # make_bbox: np.unravel_index(cell, (W, H)) * 8
                entries.append((s, bbox, self.paths[img]) + ((self._rows[(k, img)],) if ret_ws else ()))
            out.append(entries)
        return out


def dense_search_host(w, chunks, top_k: int = 50, ret_ws: bool = False, only_pos: bool = False, scores: str = "f16"):
    """The numpy restatement of the whole search.  chunks: an iterable of (paths, data fp16 [B, W, H, C]) or (paths, data, mask).
    Returns what `DenseSearch.result` returns."""
    ds = DenseSearch(w, top_k=top_k, only_pos=only_pos, keep_rows=ret_ws, scores=scores)
    for chunk in chunks:
        paths, data = chunk[0], np.asarray(chunk[1])
        mask = None if len(chunk) < 3 or chunk[2] is None else np.asarray(chunk[2])
        ds.add(paths, data, mask)
    return ds.result(ret_ws=ret_ws)


def dense_search(w, sft_paths, top_k: int = 50, ret_ws: bool = False, fold=None, only_pos: bool = False, device_id: str = "cuda",
                 scores: str = "f16"):
    """`dense_search_cuda(w, sft_paths, top_k, ret_ws=, fold=, only_pos=, device_id=)` of doersch/hog.py: w [K, C] numpy; sft_paths:
    the reference's safetensors shards, each key `';;'.join(paths)` with a tensor [B, W, H, C] (read with `safetensors.safe_open`
    straight onto the device).  fold = (i, l) masks each key as the reference does — `fold_mask(path_id, ...)` with path_id the
    shard's position in sft_paths, drawn on the device the data is on.  The bits of a mask drawn on a GPU are torch-ROCm's, not
    CUDA's: the fold holds the same share of cells as the reference's but not the same cells.  device_id "cpu" takes the numpy
    restatement.  Returns the reference's list of K lists."""
    import torch
    from safetensors import safe_open
    host = device_id == "cpu"
    ds = DenseSearch(w, top_k=top_k, only_pos=only_pos, keep_rows=ret_ws, scores=scores)
    device = torch.device(device_id)
    for path_id, sft_path in enumerate(sft_paths):
        with safe_open(sft_path, framework="pt", device=device_id if device_id in ("cuda", "cpu") else device.index) as f:
            for key in f.keys():
                paths = key.split(";;")
                data = f.get_tensor(key).to(device).half()
                B, W, H, _ = data.shape
                mask = None if fold is None else fold_mask(path_id, B, W * H, fold, device)
                if host:
                    ds.add(paths, data.numpy(), None if mask is None else mask.numpy())
                else:
                    ds.add(paths, data, mask)
    return ds.result(ret_ws=ret_ws)


# ------------------------------------------------------------------------------------------------------------------------------
# HOG-LAB features from pixels (csrc/hoglab.hip): `get_hoglab_single` + `normalize` of doersch/hog.py:24-87
# ------------------------------------------------------------------------------------------------------------------------------
HOGLAB_BINS = 31                 # DM_HOGLAB_BINS
HOGLAB_FEATURE = 2112            # DM_HOGLAB_FEATURE: 8 * 8 * 31 HOG values, then 2 * 8 * 8 Lab values
HOGLAB_MAX_SIDE = 65535          # DM_HOGLAB_MAX_SIDE
# DM_HOGLAB_E_* (include/dm_engine.h)
HOGLAB_ERRORS = {1: "null argument", 2: "B < 1, or a batch of 2^23 or more workgroups", 3: f"H or W outside [64, {HOGLAB_MAX_SIDE}]",
                 4: "2^24 or more blocks per image", 5: "workspace too small", 6: "misaligned pointer", 7: "HIP error"}
_XYZ_FROM_RGB = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
_WHITE_D65_2 = (0.95047, 1.0, 1.08883)
_bin_table = None
_bin_table_dev = {}


def _check_hoglab(rc: int, what: str):
    if rc:
        raise EngineError(f"{what}: {HOGLAB_ERRORS.get(rc, 'error')} (code {rc})")


def hoglab_bin_table():
    """uint8 [511, 511], entry [g_row + 255, g_col + 255] = the orientation bin of an integer gradient, by skimage's rule in fp64:
    o = rad2deg(arctan2(g_row, g_col)) % 180, bin i iff (180.0 / 31) i <= o < (180.0 / 31) (i + 1).  Read-only, built once.  The
    kernels and `hoglab_host` both bin by this table: integer gradients come as close as 3e-6 degrees to a bin edge, which fp32
    arctan2 does not resolve."""
    global _bin_table
    if _bin_table is None:
        g = np.arange(-255, 256, dtype=np.float64)
        o = np.rad2deg(np.arctan2(g[:, None], g[None, :])) % 180
        per = 180.0 / HOGLAB_BINS
        t = np.full(o.shape, 255, dtype=np.uint8)
        for i in range(HOGLAB_BINS):
            t[(per * i <= o) & (o < per * (i + 1))] = i
        if t.max() >= HOGLAB_BINS:
            raise AssertionError("hoglab: an integer gradient without a bin")
        t.setflags(write=False)
        _bin_table = t
    return _bin_table


def _hoglab_image(image):
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"hoglab: an image must be uint8 [H, W, 3], got {image.dtype} {image.shape}")
    H, W = image.shape[:2]
    if not (64 <= H <= HOGLAB_MAX_SIDE and 64 <= W <= HOGLAB_MAX_SIDE):
        raise ValueError(f"hoglab: {H} x {W} pixels, sides must lie in [64, {HOGLAB_MAX_SIDE}]")
    if (H // 8 - 7) * (W // 8 - 7) >= DENSE_MAX_CELLS:
        raise ValueError(f"hoglab: {H} x {W} pixels give 2^24 or more blocks")
    return image


def hoglab_shape(H: int, W: int):
    """(bc, br) = (W // 8 - 7, H // 8 - 7): the first two dimensions of one image's features (block column first)."""
    return W // 8 - 7, H // 8 - 7


def _lab_ab(rgb_u8, dt):
    """(a, b) of skimage's rgb2lab (D65, 2 degree observer) of uint8 pixels [..., 3], every operation in `dt`."""
    x = rgb_u8.astype(dt) / dt(255)
    lin = np.where(x > dt(0.04045), ((x + dt(0.055)) / dt(1.055)) ** dt(2.4), x / dt(12.92))
    xyz = lin @ np.array(_XYZ_FROM_RGB, dtype=dt).T
    xyz = xyz / np.array(_WHITE_D65_2, dtype=dt)
    f = np.where(xyz > dt(0.008856), np.cbrt(xyz), dt(7.787) * xyz + dt(16.0 / 116.0))
    return dt(500) * (f[..., 0] - f[..., 1]), dt(200) * (f[..., 1] - f[..., 2])


def hoglab_cells_host(image, dtype=np.float64):
    """Stage one in numpy: image uint8 [H, W, 3] -> (hog cells `dtype` [nr, nc, 31], lab cells `dtype` [2, nr, nc]); nr = H // 8,
    nc = W // 8.  Gradients, the channel choice and the bin are integer work; magnitudes, sums and Lab run in `dtype`."""
    image = _hoglab_image(image)
    dt = np.dtype(dtype).type
    H, W = image.shape[:2]
    nr, nc = H // 8, W // 8
    I = image.astype(np.int32)
    g_row, g_col = np.zeros_like(I), np.zeros_like(I)
    g_row[1:-1] = I[2:] - I[:-2]
    g_col[:, 1:-1] = I[:, 2:] - I[:, :-2]
    m2 = g_row * g_row + g_col * g_col
    ch = m2.argmax(axis=2)[..., None]                                          # the lowest channel among equal magnitudes
    g_row, g_col, m2 = (np.take_along_axis(a, ch, 2)[:8 * nr, :8 * nc, 0] for a in (g_row, g_col, m2))
    mag = np.sqrt(m2.astype(dt))
    bins = hoglab_bin_table()[g_row + 255, g_col + 255]
    hist = np.zeros((nr, nc, HOGLAB_BINS), dtype=dt)
    for i in range(HOGLAB_BINS):
        hist[:, :, i] = np.where(bins == i, mag, dt(0)).reshape(nr, 8, nc, 8).sum(axis=(1, 3), dtype=dt)
    hist = hist / dt(64)
    rows = (8 * np.arange(nr)[:, None] + np.array([3, 4])).reshape(-1)
    cols = (8 * np.arange(nc)[:, None] + np.array([3, 4])).reshape(-1)
    ab = np.stack(_lab_ab(image[rows][:, cols], dt)).reshape(2, nr, 2, nc, 2)
    lab = ((ab[:, :, 0, :, 0] + ab[:, :, 0, :, 1]) + (ab[:, :, 1, :, 0] + ab[:, :, 1, :, 1])) * dt(0.25)
    return hist, lab


def hoglab_blocks_host(hog_cells, lab_cells, normalized=True):
    """Stage two in numpy, in the dtype of the maps: cell maps -> [bc, br, 2112]; L2-Hys (eps 1e-5, clip 0.2) on the 8 x 8 x 31
    HOG values of a block, ((a, b) + 128) / 255 of its 64 cells, and with `normalized` the division by the norm over all 2112."""
    from numpy.lib.stride_tricks import sliding_window_view
    dt = hog_cells.dtype.type
    nr, nc = hog_cells.shape[:2]
    br, bc = nr - 7, nc - 7
    eps2 = dt(1e-5) * dt(1e-5)
    v = sliding_window_view(hog_cells, (8, 8), axis=(0, 1)).transpose(0, 1, 3, 4, 2).reshape(br, bc, 64 * HOGLAB_BINS)
    v = v / np.sqrt((v * v).sum(-1, keepdims=True) + eps2)
    v = np.minimum(v, dt(0.2))
    v = v / np.sqrt((v * v).sum(-1, keepdims=True) + eps2)
    l = sliding_window_view(lab_cells, (8, 8), axis=(1, 2)).transpose(1, 2, 0, 3, 4).reshape(br, bc, 128)
    x = np.concatenate([v, (l + dt(128)) / dt(255)], axis=-1)
    if normalized:
        x = x / np.sqrt((x * x).sum(-1, keepdims=True))
    return np.ascontiguousarray(x.transpose(1, 0, 2))


def hoglab_host(image, normalized=True, dtype=np.float64):
    """The numpy restatement of `get_hoglab_single` (normalized=False: what the reference's .npy cache holds) and of
    `normalize(get_hoglab_single(...))` (normalized=True: what the search reads, before the fp16 cast): image uint8 [H, W, 3] ->
    `dtype` [bc, br, 2112].  With dtype=np.float32 every floating-point operation runs in fp32."""
    return hoglab_blocks_host(*hoglab_cells_host(image, dtype), normalized=normalized)


def _hoglab_batch(images):
    images = np.asarray(images)
    if images.ndim == 3:
        images = images[None]
    if images.ndim != 4 or images.shape[0] < 1:
        raise ValueError(f"hoglab: images must be uint8 [B, H, W, 3], got {images.shape}")
    return images


def hoglab_workspace_bytes(B: int, H: int, W: int) -> int:
    need = _lib().dm_hoglab_workspace_bytes(int(B), int(H), int(W))
    if not need:
        raise ValueError(f"hoglab: no workspace for {B} images of {H} x {W} pixels")
    return need


def _hoglab_device_args(images):
    import torch
    if not (isinstance(images, torch.Tensor) and images.is_cuda):
        raise EngineError("hoglab: images must be a uint8 torch tensor on the GPU, or numpy for the host restatement")
    if images.ndim == 3:
        images = images[None]
    if images.dtype != torch.uint8 or images.ndim != 4 or images.shape[3] != 3 or images.shape[0] < 1:
        raise ValueError(f"hoglab: images must be uint8 [B, H, W, 3], got {images.dtype} {tuple(images.shape)}")
    images = images.contiguous()
    dev = images.device
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _bin_table_dev:
        _bin_table_dev[key] = torch.from_numpy(hoglab_bin_table().copy()).to(dev)
    return torch, images, dev, _bin_table_dev[key]


def hoglab_cells(images):
    """dm_hoglab_cells on the current stream: uint8 [B, H, W, 3] on the GPU -> device tensors (hog cells fp32 [B, nr, nc, 31], lab
    cells fp32 [B, 2, nr, nc]).  A numpy input takes `hoglab_cells_host` per image (fp64 arithmetic, fp32 result)."""
    if isinstance(images, np.ndarray):
        maps = [hoglab_cells_host(im) for im in _hoglab_batch(images)]
        return np.stack([m[0] for m in maps]).astype(np.float32), np.stack([m[1] for m in maps]).astype(np.float32)
    torch, images, dev, bins = _hoglab_device_args(images)
    B, H, W, _ = images.shape
    hoglab_workspace_bytes(B, H, W)                      # the shape check
    hog = torch.empty((B, H // 8, W // 8, HOGLAB_BINS), dtype=torch.float32, device=dev)
    lab = torch.empty((B, 2, H // 8, W // 8), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_hoglab_cells(_stream(torch, dev), _p(images), B, H, W, _p(bins), _p(hog), _p(lab))
    _check_hoglab(rc, "dm_hoglab_cells")
    return hog, lab


def hoglab_features(images, normalized=True, raw=False, work=None):
    """dm_hoglab_features on the current stream: uint8 [B, H, W, 3] on the GPU -> (fp16 [B, bc, br, 2112] or None, fp32 of the same
    shape or None): the normalised features the search reads and / or the raw ones `get_hoglab_single` returns.  work: a uint8
    workspace of at least `hoglab_workspace_bytes(B, H, W)` to reuse."""
    if not (normalized or raw):
        raise ValueError("hoglab: neither output asked for")
    torch, images, dev, bins = _hoglab_device_args(images)
    B, H, W, _ = images.shape
    need = hoglab_workspace_bytes(B, H, W)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    bc, br = hoglab_shape(H, W)
    out = torch.empty((B, bc, br, HOGLAB_FEATURE), dtype=torch.float16, device=dev) if normalized else None
    rawt = torch.empty((B, bc, br, HOGLAB_FEATURE), dtype=torch.float32, device=dev) if raw else None
    with torch.cuda.device(dev):
        rc = _lib().dm_hoglab_features(_stream(torch, dev), _p(images), B, H, W, _p(bins), _p(out), _p(rawt), _p(work),
                                       work.numel() * work.element_size())
    _check_hoglab(rc, "dm_hoglab_features")
    return out, rawt


def hoglab(images, normalized=True):
    """HOG-LAB features of a batch of same-sized images: uint8 [B, H, W, 3] on the GPU -> fp16 [B, bc, br, 2112] (normalized: ready
    for `DenseSearch.add`) or fp32 of the same shape (normalized=False: the raw features).  A numpy input takes `hoglab_host` per
    image and gives numpy arrays of the same types."""
    if isinstance(images, np.ndarray):
        x = np.stack([hoglab_host(im, normalized=normalized) for im in _hoglab_batch(images)])
        return x.astype(np.float16) if normalized else x.astype(np.float32)
    out, raw = hoglab_features(images, normalized=normalized, raw=not normalized)
    return out if normalized else raw


def read_images(paths):
    """The images of `paths` as the reference's `imread` delivers them for 8-bit RGB JPEG / PNG files: PIL, `convert("RGB")`, no
    resize.  (A grey or RGBA file comes out of `imread` with another shape, on which the reference's `hog(channel_axis=-1)` fails
    or treats alpha as a colour; here it is converted to RGB.)  -> [(indices into paths, uint8 [n, H, W, 3]), ...], one entry per
    image size in order of first appearance."""
    from PIL import Image
    groups = {}
    for j, path in enumerate(paths):
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        groups.setdefault(a.shape, ([], []))
        groups[a.shape][0].append(j)
        groups[a.shape][1].append(a)
    return [(idx, np.stack(arrs)) for idx, arrs in groups.values()]


def detector_from_patch(features, bbox):
    """The reference's initial detector of a patch (doersch/doersch.py:337): `normalize(feat)[bbox[0] // 8, bbox[1] // 8]`, the row
    of the NORMALISED features [bc, br, C] (or [1, bc, br, C]) of the patch's image at block (bbox[0] // 8, bbox[1] // 8) — what
    `hoglab(image)` gives.  Device features: one row by dm_dense_search_gather -> fp16 [C] on the device; numpy: a copy of the row."""
    if features.ndim == 4 and features.shape[0] == 1:
        features = features[0]
    if features.ndim != 3:
        raise ValueError(f"detector_from_patch: features of ONE image [bc, br, C], got {tuple(features.shape)}")
    bc, br, C_ = features.shape
    a, b = int(bbox[0]) // 8, int(bbox[1]) // 8
    if not (0 <= a < bc and 0 <= b < br):
        raise ValueError(f"detector_from_patch: bbox {tuple(bbox)} outside {bc} x {br} blocks")
    if isinstance(features, np.ndarray):
        return features[a, b].copy()
    import torch
    pairs = torch.tensor([[0, a * br + b]], dtype=torch.int32, device=features.device)
    return gather(features.contiguous().view(1, bc * br, C_), pairs)[0]


def dense_search_images(w, image_paths, top_k: int = 50, ret_ws: bool = False, fold=None, only_pos: bool = False, batch: int = 16,
                        device_id: str = "cuda", scores: str = "f16"):
    """`dense_search`, fed from image files instead of the reference's feature shards: per batch of `batch` paths the images are
    read (`read_images`), their features computed on the device (`hoglab`) and handed to `DenseSearch.add` — no cache, no
    safetensors, no skimage.  Images of a batch that differ in size are added size by size (order of first appearance), so with
    mixed sizes the image order that breaks score ties is that order.  fold = (i, l): `fold_mask(path_id, ...)` with path_id = the
    batch's index, drawn on the device the features are on, once per size group: every group of a batch reseeds with the same
    path_id, so the masks of two size groups of one batch come from the same permutation stream and are correlated (equal where the
    cell counts are equal).  The reference's batches hold one size, where this is its own draw.  device_id "cpu" takes the numpy
    restatements.
    Returns what `dense_search` returns."""
    import torch
    if batch < 1:
        raise ValueError(f"dense search: batch {batch}")
    host = device_id == "cpu"
    ds = DenseSearch(w, top_k=top_k, only_pos=only_pos, keep_rows=ret_ws, scores=scores)
    device = torch.device(device_id)
    image_paths = list(image_paths)
    for path_id, at in enumerate(range(0, len(image_paths), batch)):
        names = image_paths[at:at + batch]
        for idx, images in read_images(names):
            data = hoglab(images) if host else hoglab(torch.from_numpy(images).to(device))
            B, W_, H_, _ = data.shape
            mask = None if fold is None else fold_mask(path_id, B, W_ * H_, fold, device)
            if host and mask is not None:
                mask = mask.numpy()
            ds.add([names[j] for j in idx], data, mask)
    return ds.result(ret_ws=ret_ws)


def discriminative_20(result, positive_paths):
    """`search_batch`'s d20 (doersch/doersch.py:95): per detector, how many of its first 20 entries name a path of the positive
    set.  result: what `dense_search` returns; -> list of K ints."""
    positive = set(positive_paths)
    return [sum(1 for entry in entries[:20] if entry[2] in positive) for entries in result]


# ------------------------------------------------------------------------------------------------------------------------------
# the detectors' SVMs (csrc/svm.hip): `train_svm` of doersch/doersch.py:66-79 and `random_sample` of hog.py:187-212
# ------------------------------------------------------------------------------------------------------------------------------
SVM_MAX_DETECTORS = 128          # DM_SVM_MAX_DETECTORS
SVM_MAX_FEATURES = 8192          # DM_SVM_MAX_FEATURES
SVM_MAX_SAMPLES = 1 << 24        # n >= 2^24 is refused
SVM_CONVERGED, SVM_MAX_ITER, SVM_NAN, SVM_BAD_LIST = 0, 1, 2, 3          # DM_SVM_* status
SVM_TAU = 1e-12                  # libsvm's TAU
# DM_SVM_E_* (include/dm_engine.h)
SVM_ERRORS = {1: "null argument", 2: f"K outside [1, {SVM_MAX_DETECTORS}]", 3: f"C < 8, not a multiple of 8 or above {SVM_MAX_FEATURES}",
              4: "R < 1", 5: "ld < 2", 6: "ld >= 2^24", 7: "cost or eps not > 0", 8: "workspace too small", 9: "misaligned pointer",
              10: "HIP error"}


def _check_svm(rc: int, what: str):
    if rc:
        raise EngineError(f"{what}: {SVM_ERRORS.get(rc, 'error')} (code {rc})")


def _check_svm_shape(n, n_pos, C_, K=1):
    if not 1 <= K <= SVM_MAX_DETECTORS:
        raise ValueError(f"svm: {K} detectors, need 1 ... {SVM_MAX_DETECTORS}")
    if C_ < 8 or C_ % 8 or C_ > SVM_MAX_FEATURES:
        raise ValueError(f"svm: {C_} features, need a multiple of 8 in [8, {SVM_MAX_FEATURES}] (2112 = 8 * 264)")
    if n >= SVM_MAX_SAMPLES:
        raise ValueError(f"svm: {n} samples, 2^24 or more")
    if n_pos < 1 or n - n_pos < 1:
        raise ValueError(f"svm: {n_pos} positives and {n - n_pos} negatives, need at least one of each")


def _svm_default_max_iter(n: int) -> int:
    return max(10_000_000, 100 * n)


def _svm_dots(Z, x):
    """The kernels' dot: Z float64 [n, C] times x float64 [C] (or row by row, [n, C]) -> [n].  Lane l of 64 adds the products of the
    8-feature chunks l, l + 64, ... one by one in ascending order, then the 64 partials meet in an xor tree (32, 16, ... 1)."""
    n, C_ = Z.shape
    J = -(-(C_ // 8) // 64)
    lanes = np.arange(64)
    out = np.empty(n)
    for r0 in range(0, n, 1024):
        Zr = Z[r0:r0 + 1024]
        P = np.zeros((len(Zr), J * 512))
        P[:, :C_] = Zr * (x if x.ndim == 1 else x[r0:r0 + 1024])
        P = P.reshape(len(Zr), J, 64, 8)
        a = np.zeros((len(Zr), 64))
        for j in range(J):
            for e in range(8):
                a = a + P[:, j, :, e]
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[:, lanes ^ o]
        out[r0:r0 + 1024] = a[:, 0]
    return out


def svm_fit_host(X, n_pos: int, C: float = 0.1, tol: float = 1e-3, max_iter: int = -1, trace=None):
    """The numpy restatement of SVC(C=C, kernel='linear', tol=tol, shrinking=False).fit(X, [1] * n_pos + [-1] * (n - n_pos)) by the
    rules at the top of this module: X fp16 [n, C] -> (w float64 [C], b float, n_iter int, alpha float64 [n] in the order of X's
    rows, status).  Raises ValueError on a NaN or an infinity, as scikit-learn does.  trace(n_iter, "i" or "j", values, chosen) sees
    every selection step: the candidates' values in libsvm's order (-inf: no candidate; the largest wins) and the index chosen."""
    X = np.asarray(X)
    if X.dtype != np.float16 or X.ndim != 2:
        raise ValueError(f"svm: X must be float16 [n, C], got {X.dtype} {X.shape}")
    n, C_ = X.shape
    n_pos = int(n_pos)
    _check_svm_shape(n, n_pos, C_)
    cost, eps = float(C), float(tol)
    if not (cost > 0 and eps > 0):
        raise ValueError(f"svm: C {C} and tol {tol} must be positive")
    if not np.isfinite(X).all():
        raise ValueError("svm: X contains NaN or infinity")
    max_iter = _svm_default_max_iter(n) if max_iter <= 0 else int(max_iter)
    n_neg = n - n_pos
    Z = np.concatenate([X[n_pos:], X[:n_pos]]).astype(np.float64)          # libsvm's order: the negatives as y = +1, the positives as -1
    y = np.concatenate([np.ones(n_neg), -np.ones(n_pos)])
    pos_y = y > 0
    alpha, G = np.zeros(n), -np.ones(n)
    QD = _svm_dots(Z, Z)
    cache = {}

    def column(i):
        if i not in cache:
            cache[i] = (y[i] * y * _svm_dots(Z, Z[i])).astype(np.float32)
        return cache[i]

    def last_argmax(v):
        return n - 1 - int(np.argmax(v[::-1]))

    n_iter, status = 0, SVM_CONVERGED
    while True:
        if n_iter >= max_iter:
            status = SVM_MAX_ITER
            break
        up = np.where(pos_y, alpha < cost, alpha > 0)                      # candidates for i
        if not up.any():
            break
        viol = np.where(up, np.where(pos_y, -G, G), -np.inf)
        i = last_argmax(viol)
        Gmax = viol[i]
        if trace is not None:
            trace(n_iter, "i", viol, i)
        Qi = column(i)
        low = np.where(pos_y, alpha > 0, alpha < cost)                     # candidates for j
        if not low.any():
            break
        Gmax2 = np.where(low, np.where(pos_y, G, -G), -np.inf).max()
        grad_diff = np.where(pos_y, Gmax + G, Gmax - G)
        quad = QD[i] + QD - 2.0 * (y[i] * y) * Qi.astype(np.float64)
        quad = np.where(quad > 0, quad, SVM_TAU)
        ok = low & (grad_diff > 0)
        if Gmax + Gmax2 < eps or not ok.any():
            break
        gain = np.where(ok, (grad_diff * grad_diff) / quad, -np.inf)
        j = last_argmax(gain)                                              # the lowest -grad_diff^2 / quad, the last among equals
        if trace is not None:
            trace(n_iter, "j", gain, j)
        n_iter += 1
        Qj = column(j)
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            q = QD[i] + QD[j] + 2.0 * float(Qi[j])
            if q <= 0:
                q = SVM_TAU
            delta = (-G[i] - G[j]) / q
            diff = ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0:
                if aj < 0:
                    aj, ai = 0.0, diff
            elif ai < 0:
                ai, aj = 0.0, -diff
            if diff > 0:                                                   # C_i - C_j = 0
                if ai > cost:
                    ai, aj = cost, cost - diff
            elif aj > cost:
                aj, ai = cost, cost + diff
        else:
            q = QD[i] + QD[j] - 2.0 * float(Qi[j])
            if q <= 0:
                q = SVM_TAU
            delta = (G[i] - G[j]) / q
            total = ai + aj
            ai, aj = ai - delta, aj + delta
            if total > cost:
                if ai > cost:
                    ai, aj = cost, total - cost
            elif aj < 0:
                aj, ai = 0.0, total
            if total > cost:
                if aj > cost:
                    aj, ai = cost, total - cost
            elif ai < 0:
                ai, aj = 0.0, total
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        G = G + (Qi.astype(np.float64) * dai + Qj.astype(np.float64) * daj)
    upper, lower = alpha >= cost, alpha <= 0
    free = ~upper & ~lower
    yG = y * G
    if free.any():
        s = 0.0
        for v in yG[free]:
            s += float(v)
        rho = s / int(free.sum())
    else:
        ub_set = (upper & ~pos_y) | (lower & ~upper & pos_y)
        lb_set = (upper & pos_y) | (lower & ~upper & ~pos_y)
        ub = yG[ub_set].min() if ub_set.any() else np.inf
        lb = yG[lb_set].max() if lb_set.any() else -np.inf
        rho = (ub + lb) / 2
    w = np.zeros(C_)
    for t in np.flatnonzero(alpha > 0):
        w = w - (alpha[t] * y[t]) * Z[t]
    return w, float(rho), n_iter, np.concatenate([alpha[n_neg:], alpha[:n_neg]]), status


def hard_negatives_host(X, w, b, first: int, max_samples: int):
    """doersch.py:75-78 by the rules at the top of this module: X fp16 [n, C] -> (positions int64 [count] in X, score float64
    [n - first] of rows first ... n - 1)."""
    X = np.asarray(X)
    first = int(first)
    if X.dtype != np.float16 or X.ndim != 2 or not 0 <= first <= len(X):
        raise ValueError(f"svm: X must be float16 [n, C] and first in [0, n], got {X.dtype} {X.shape}, {first}")
    s = _svm_dots(X[first:].astype(np.float64), np.asarray(w, dtype=np.float64)) + float(b)
    idx = np.flatnonzero(s > 0)
    idx = idx[np.argsort(-s[idx], kind="stable")][:max(int(max_samples), 0)]
    return idx + first, s


def svm_workspace_bytes(K: int, ld: int) -> int:
    need = _lib().dm_svm_workspace_bytes(int(K), int(ld))
    if not need:
        raise ValueError(f"svm: no workspace for {K} detectors of up to {ld} samples")
    return need


def _svm_counts(K, ld, **named):
    """Per-detector counts as int64 numpy [K]: an int stands for every detector; a device tensor is read back."""
    out = []
    for name, v in named.items():
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        v = np.broadcast_to(v, (K,)) if v.ndim == 0 else v
        if v.shape != (K,) or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"svm: {name} must be an int or {K} ints, got {v.dtype} {v.shape}")
        out.append(v.astype(np.int64))
    return out


def _svm_table(pool, table):
    if pool.ndim != 2 or table.ndim != 2:
        raise ValueError(f"svm: pool must be [R, C] and table [K, ld], got {tuple(pool.shape)} and {tuple(table.shape)}")
    (R, C_), (K, ld) = pool.shape, table.shape
    _check_svm_shape(2, 1, C_, K)
    if R < 1 or ld < 2:
        raise ValueError(f"svm: a pool of {R} rows and a table of {ld} columns")
    if ld >= SVM_MAX_SAMPLES:
        raise ValueError(f"svm: {ld} samples, 2^24 or more")
    return R, C_, K, ld


def _svm_device_args(pool, table):
    import torch
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda):
        raise EngineError("svm: pool must be a float16 torch tensor on the GPU, or numpy for the host restatement")
    if pool.dtype != torch.float16:
        raise ValueError("svm: pool must be float16")
    dev = pool.device
    table = torch.as_tensor(table).to(device=dev, dtype=torch.int32).contiguous()
    return torch, pool.contiguous(), table, dev


def svm_fit(pool, table, n, n_pos, C: float = 0.1, tol: float = 1e-3, max_iter: int = -1, work=None, want_alpha: bool = False):
    """dm_svm_fit on the current stream: pool fp16 [R, C] and table int32 [K, ld] on the GPU, n / n_pos ints or [K] -> device tensors
    (w float64 [K, C], b float64 [K], n_iter int32 [K], status int32 [K], alpha float64 [K, ld] or None).  Does not raise on a
    status; `train_svms` does.  Synchronises the stream."""
    torch, pool, table, dev = _svm_device_args(pool, table)
    R, C_, K, ld = _svm_table(pool, table)
    n, n_pos = _svm_counts(K, ld, n=n, n_pos=n_pos)
    for k in range(K):
        _check_svm_shape(int(n[k]), int(n_pos[k]), C_, K)
        if n[k] > ld:
            raise ValueError(f"svm: detector {k} lists {n[k]} samples in a table of {ld} columns")
    if not (C > 0 and tol > 0):
        raise ValueError(f"svm: C {C} and tol {tol} must be positive")
    need = svm_workspace_bytes(K, ld)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    n_d, n_pos_d = (torch.from_numpy(v.astype(np.int32)).to(dev) for v in (n, n_pos))
    w = torch.empty((K, C_), dtype=torch.float64, device=dev)
    b = torch.empty(K, dtype=torch.float64, device=dev)
    n_iter, status = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
    alpha = torch.empty((K, ld), dtype=torch.float64, device=dev) if want_alpha else None
    with torch.cuda.device(dev):
        rc = _lib().dm_svm_fit(_stream(torch, dev), _p(pool), R, C_, _p(table), ld, _p(n_d), _p(n_pos_d), K, float(C), float(tol),
                               int(max_iter), _p(work), work.numel() * work.element_size(), _p(w), _p(b), _p(n_iter), _p(status), _p(alpha))
    _check_svm(rc, "dm_svm_fit")
    return w, b, n_iter, status, alpha


def svm_hard_negatives(pool, table, n, first, max_samples, w, b, work=None):
    """dm_svm_hard_negatives on the current stream -> device tensors (score float64 [K, ld], hard int32 [K, ld], count int32 [K])."""
    torch, pool, table, dev = _svm_device_args(pool, table)
    R, C_, K, ld = _svm_table(pool, table)
    n, first, max_samples = _svm_counts(K, ld, n=n, first=first, max_samples=max_samples)
    if tuple(w.shape) != (K, C_) or tuple(b.shape) != (K,) or w.dtype != torch.float64 or b.dtype != torch.float64:
        raise ValueError(f"svm: w must be float64 [{K}, {C_}] and b float64 [{K}]")
    need = svm_workspace_bytes(K, ld)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    n_d, first_d, max_d = (torch.from_numpy(np.clip(v, -1, 2 ** 31 - 1).astype(np.int32)).to(dev) for v in (n, first, max_samples))
    score = torch.empty((K, ld), dtype=torch.float64, device=dev)
    hard = torch.empty((K, ld), dtype=torch.int32, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_svm_hard_negatives(_stream(torch, dev), _p(pool), R, C_, _p(table), ld, _p(n_d), _p(first_d), _p(max_d), K,
                                          _p(w.contiguous()), _p(b.contiguous()), _p(work), work.numel() * work.element_size(),
                                          _p(score), _p(hard), _p(count))
    _check_svm(rc, "dm_svm_hard_negatives")
    return score, hard, count


def _svm_raise(status):
    bad = np.flatnonzero(np.asarray(status) >= SVM_NAN)
    if len(bad):
        k = int(bad[0])
        if int(np.asarray(status)[k]) == SVM_NAN:
            raise ValueError(f"svm: the samples of detector {k} contain NaN or infinity")
        raise ValueError(f"svm: the sample list of detector {k} cannot be used: no positive, no negative, more samples than the table "
                         f"has columns, or a sample outside the pool")


def train_svms(pool, table, n, n_pos, n_hn, max_samples, C: float = 0.1, tol: float = 1e-3, max_iter: int = -1):
    """`train_svm` for K detectors at once.  pool fp16 [R, C]; row k of table int32 [K, ld] lists detector k's n[k] samples as pool
    rows: n_pos[k] positives, n_hn[k] hard negatives of earlier rounds, then the new negatives, among which at most max_samples[k]
    hard negatives are mined (n, n_pos, n_hn, max_samples: an int or K ints).  Returns (w float64 [K, C], b float64 [K], n_iter
    int32 [K], status int32 [K], hard int32 [K, ld] — positions in the detector's list, -1 from count on —, count int32 [K]):
    device tensors for a pool on the GPU, numpy arrays (by `svm_fit_host` / `hard_negatives_host`) for a numpy pool.  Raises
    ValueError where a detector's samples hold a NaN or an infinity, as scikit-learn does."""
    if isinstance(pool, np.ndarray):
        table = np.asarray(table)
        R, C_, K, ld = _svm_table(pool, table)
        n, n_pos, n_hn, max_samples = _svm_counts(K, ld, n=n, n_pos=n_pos, n_hn=n_hn, max_samples=max_samples)
        w, b = np.empty((K, C_)), np.empty(K)
        n_iter, status, count = (np.zeros(K, dtype=np.int32) for _ in range(3))
        hard = np.full((K, ld), -1, dtype=np.int32)
        for k in range(K):
            if n[k] > ld or table[k, :n[k]].min() < 0 or table[k, :n[k]].max() >= R:
                raise ValueError(f"svm: detector {k} names a sample outside the pool")
            X = pool[table[k, :n[k]]]
            w[k], b[k], n_iter[k], _, status[k] = svm_fit_host(X, n_pos[k], C, tol, max_iter)
            idx, _ = hard_negatives_host(X, w[k], b[k], n_pos[k] + n_hn[k], max_samples[k])
            count[k] = len(idx)
            hard[k, :len(idx)] = idx
        return w, b, n_iter, status, hard, count
    torch, pool, table, dev = _svm_device_args(pool, table)
    K, ld = table.shape
    n, n_pos, n_hn, max_samples = _svm_counts(K, ld, n=n, n_pos=n_pos, n_hn=n_hn, max_samples=max_samples)
    work = torch.empty(svm_workspace_bytes(K, ld), dtype=torch.uint8, device=dev)
    w, b, n_iter, status, _ = svm_fit(pool, table, n, n_pos, C, tol, max_iter, work)
    _svm_raise(status.cpu().numpy())
    _, hard, count = svm_hard_negatives(pool, table, n, n_pos + n_hn, max_samples, w, b, work)
    return w, b, n_iter, status, hard, count


def train_svm(X, split, max_samples):
    """`train_svm(X, split, max_samples)` of doersch/doersch.py:66-79: X = the rows of len_p positives, len_hn earlier hard negatives
    and len_n new negatives, split = (len_p, len_hn, len_n) -> (coef float64 [C], hard_negatives.tolist()): the new negatives that
    score above 0, highest first, at most max_samples.  The intercept is dropped, as the reference drops it.  Rows are taken as
    fp16 (what the reference's caches hold).  A numpy X (or a list of rows) takes the host restatement, a torch tensor on the GPU
    the kernels."""
    len_p, len_hn, len_n = (int(v) for v in split)
    if hasattr(X, "is_cuda") and X.is_cuda:
        import torch
        if X.shape[0] != len_p + len_hn + len_n:
            raise ValueError(f"svm: {X.shape[0]} rows for split {tuple(split)}")
        X = X.to(torch.float16).contiguous()
        table = torch.arange(max(X.shape[0], 2), dtype=torch.int32, device=X.device)[None]
        w, _, _, _, hard, count = train_svms(X, table, X.shape[0], len_p, len_hn, max_samples)
        return w[0].cpu().numpy(), X[hard[0, :int(count[0])].long()].cpu().numpy().tolist()
    X = np.stack([np.asarray(x) for x in X], axis=0).astype(np.float16)
    if len(X) != len_p + len_hn + len_n:
        raise ValueError(f"svm: {len(X)} rows for split {tuple(split)}")
    w, b, _, _, _ = svm_fit_host(X, len_p)
    idx, _ = hard_negatives_host(X, w, b, len_p + len_hn, max_samples)
    return w, X[idx].tolist()


def svm_round(positives, negatives, hard_negatives, C: float = 0.1, tol: float = 1e-3, max_iter: int = -1, max_samples=None):
    """One batch of doersch/doersch.py:462-471.  positives: what `DenseSearch.result(ret_ws=True)` returns (per detector its entries
    (score, bbox, path, row)); negatives: per detector the rows `sample_negatives` drew, fp16 [m, C] — all numpy or all on one GPU,
    and one array may serve several detectors (it enters the pool once); hard_negatives: per detector the running list of rows,
    extended here by the round's new hard negatives (numpy rows on the host path, rows of a device tensor on the GPU).
    max_samples: per detector, default the reference's max(25000 - len(hard_negatives[k]), 10000).  Builds the pool and the index
    table, calls `train_svms` and returns ws float64 [K, C] (numpy / a device tensor): the next search's detectors."""
    K = len(positives)
    if not (K == len(negatives) == len(hard_negatives)) or K < 1:
        raise ValueError(f"svm: {K} detectors, {len(negatives)} negative sets and {len(hard_negatives)} hard-negative lists")
    host = isinstance(negatives[0], np.ndarray)
    if host:
        to_rows = lambda rows: np.stack([np.asarray(r, dtype=np.float16) for r in rows])                      # noqa: E731
        cat = np.concatenate
    else:
        import torch
        dev = negatives[0].device

        def to_rows(rows):
            """numpy rows (a search's `ret_ws` rows) and device rows (earlier rounds' hard negatives) in their order -> fp16 [m, C] on
            `dev`: the numpy rows travel in one copy."""
            out = torch.empty((len(rows), len(rows[0])), dtype=torch.float16, device=dev)
            on_dev = [j for j, r in enumerate(rows) if isinstance(r, torch.Tensor)]
            on_host = [j for j, r in enumerate(rows) if not isinstance(r, torch.Tensor)]
            if on_dev:
                out[torch.tensor(on_dev, device=dev)] = torch.stack([rows[j].to(device=dev, dtype=torch.float16) for j in on_dev])
            if on_host:
                out[torch.tensor(on_host, device=dev)] = torch.from_numpy(np.stack([np.asarray(rows[j], dtype=np.float16) for j in on_host])).to(dev)
            return out
        cat = torch.cat
    parts, at, shared = [], 0, {}
    lists, n, n_pos, n_hn = [], [], [], []
    for k in range(K):
        pos = [entry[3] for entry in positives[k]]
        if not pos:
            raise ValueError(f"svm: detector {k} has no positive")
        own = to_rows(pos + list(hard_negatives[k]))
        idx = [np.arange(at, at + len(own))]
        parts.append(own)
        at += len(own)
        if id(negatives[k]) not in shared:
            shared[id(negatives[k])] = at
            parts.append(negatives[k].reshape(-1, negatives[k].shape[-1]))
            at += len(parts[-1])
        idx.append(shared[id(negatives[k])] + np.arange(negatives[k].reshape(-1, negatives[k].shape[-1]).shape[0]))
        lists.append(np.concatenate(idx))
        n.append(len(lists[-1]))
        n_pos.append(len(pos))
        n_hn.append(len(hard_negatives[k]))
    pool = cat(parts)
    table = np.zeros((K, max(max(n), 2)), dtype=np.int32)
    for k in range(K):
        table[k, :n[k]] = lists[k]
    if max_samples is None:
        max_samples = [max(25000 - h, 10000) for h in n_hn]
    w, _, _, _, hard, count = train_svms(pool, table, np.array(n), np.array(n_pos), np.array(n_hn), np.asarray(max_samples), C, tol, max_iter)
    if host:
        for k in range(K):
            hard_negatives[k] += list(pool[table[k, hard[k, :count[k]]]])
    else:
        count_h = count.cpu().numpy()
        if count_h.any():
            table_d = torch.from_numpy(table).to(dev)
            for k in np.flatnonzero(count_h):
                hard_negatives[k] += list(pool[table_d[k, hard[k, :int(count_h[k])].long()].long()])
    return w


def fold_pool(n: int, fold):
    """The positions `random_sample` draws from under fold = (i, l) (hog.py:206-207): the first i n // l entries of the CPU
    `torch.randperm(n)` under `torch.manual_seed(0)`, as a numpy int64 array.  Reseeds torch's global generator, as the reference does."""
    import torch
    i, l = int(fold[0]), int(fold[1])
    torch.manual_seed(0)
    return torch.randperm(n, device="cpu")[:(i * n) // l].numpy()


def sample_negatives(chunks, num_samples: int, fold=None, rng=None):
    """`random_sample(sft_paths, fold, num_samples)` of doersch/hog.py:187-212.  chunks: the shards, each a sequence of the shard's
    keys' tensors fp16 [B, W, H, C] — all numpy or all on one GPU.  Every shard gives num_samples // len(chunks) rows, spread over its
    keys as max(1, that // keys) rows per key, drawn without replacement from the key's B W H cells or, with fold, from `fold_pool`
    of them; shards and keys are visited in a shuffled order.  The positions are drawn on the host from `rng` (a numpy Generator;
    default a fresh unseeded one, as the reference draws from Python's unseeded `random`); the rows are fetched by `gather` on the
    device.  Returns fp16 [total, C], numpy or on the device of the chunks."""
    rng = np.random.default_rng() if rng is None else rng
    chunks = [list(shard) for shard in chunks]
    if not chunks or any(not shard for shard in chunks):
        raise ValueError("sample_negatives: no shard, or a shard without a key")
    per_shard = int(num_samples) // len(chunks)
    out = []
    for s in rng.permutation(len(chunks)):
        shard = chunks[s]
        per_key = max(1, per_shard // len(shard))
        for q in rng.permutation(len(shard)):
            data = shard[q]
            if data.ndim != 4:
                raise ValueError(f"sample_negatives: a key's tensor must be [B, W, H, C], got {tuple(data.shape)}")
            B, cells, C_ = data.shape[0], data.shape[1] * data.shape[2], data.shape[3]
            population = np.arange(B * cells) if fold is None else fold_pool(B * cells, fold)
            if per_key > len(population):
                raise ValueError(f"sample_negatives: {per_key} rows from a key of {len(population)} cells")
            at = rng.choice(population, size=per_key, replace=False)
            if isinstance(data, np.ndarray):
                out.append(data.reshape(B * cells, C_)[at].astype(np.float16))
            else:
                import torch
                pairs = torch.from_numpy(np.stack([at // cells, at % cells], axis=1).astype(np.int32)).to(data.device)
                out.append(gather(data.half().contiguous().view(B, cells, C_), pairs))
    if isinstance(out[0], np.ndarray):
        return np.concatenate(out)
    import torch
    return torch.cat(out)


# ------------------------------------------------------------------------------------------------------------------------------
# detector initialisation (csrc/dense_search_wide.hip): `init_patches`, `init_detectors`, `rank_init_detectors` and
# `accept_patch_neighbor` of doersch/doersch.py:46-64, 248-276, 317-400
# ------------------------------------------------------------------------------------------------------------------------------
DENSE_WIDE_MAX_DETECTORS = 32768     # DM_DENSE_WIDE_MAX_DETECTORS
RANK_MAX_N = 32768                   # DM_DETECTOR_RANK_MAX_N
RANK_MAX_L = 128                     # DM_DETECTOR_RANK_MAX_L
RANK_MAX_DETECTORS = 4096            # DM_DETECTOR_RANK_MAX_DETECTORS
RANK_MAX_BOX = 2048                  # DM_DETECTOR_RANK_MAX_BOX
# DM_RANK_E_* (include/dm_engine.h)
RANK_ERRORS = {1: "null argument", 2: f"N outside [1, {RANK_MAX_N}]", 3: f"L outside [1, {RANK_MAX_L}]",
               4: f"num_detectors outside [1, {RANK_MAX_DETECTORS}]", 5: f"box outside [1, {RANK_MAX_BOX}]", 6: "max_pairs < 0",
               7: "workspace too small", 8: "misaligned pointer", 9: "HIP error"}


def _check_rank(rc: int, what: str):
    if rc:
        raise EngineError(f"{what}: {RANK_ERRORS.get(rc, 'error')} (code {rc})")


def _check_wide_shape(B, cells, C_, K, top_k=1):
    _check_shape(B, cells, C_, 1, top_k)
    if not 1 <= K <= DENSE_WIDE_MAX_DETECTORS:
        raise ValueError(f"wide search: {K} detectors, need 1 ... {DENSE_WIDE_MAX_DETECTORS}")


def wide_workspace_bytes(B: int, cells: int, K: int) -> int:
    need = _lib().dm_dense_wide_workspace_bytes(int(B), int(cells), int(K))
    if not need:
        raise ValueError(f"wide search: no workspace for {B} images of {cells} cells and {K} detectors")
    return need


def wide_winners(data, w, score, cell, image_offset: int = 0, mask=None, work=None):
    """dm_dense_wide_winners on the current stream: `winners` for 1 <= K <= 32768 detectors, bit-equal to it over blocks of 128."""
    import torch
    B, cells, C_ = data.shape
    K, ld = score.shape
    dev = data.device
    need = wide_workspace_bytes(B, cells, K)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_dense_wide_winners(_stream(torch, dev), _p(data), _p(w), _p(mask), B, cells, C_, K, int(image_offset), ld,
                                          _p(work), work.numel() * work.element_size(), _p(score), _p(cell))
    _check(rc, "dm_dense_wide_winners")
    return work


def wide_topk(score, cell, n_images: int, top_k: int, image_h, positive=None, only_pos: bool = False):
    """dm_dense_wide_topk on the current stream over columns [0, n_images) of the tables; image_h int32 [n_images] (the H of every
    image's [W, H] block grid) and positive uint8 [n_images] or None on the device -> device tensors (top_score fp32 [K, top_k],
    top_image int32, top_x int32, top_y int32, count int32 [K], d20 int32 [K] or None)."""
    import torch
    K, ld = score.shape
    dev = score.device
    top_score = torch.empty((K, top_k), dtype=torch.float32, device=dev)
    top_image, top_x, top_y = (torch.empty((K, top_k), dtype=torch.int32, device=dev) for _ in range(3))
    count = torch.empty(K, dtype=torch.int32, device=dev)
    d20 = None if positive is None else torch.empty(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_dense_wide_topk(_stream(torch, dev), _p(score), _p(cell), K, int(n_images), ld, int(top_k), int(bool(only_pos)),
                                       _p(positive), _p(image_h), _p(top_score), _p(top_image), _p(top_x), _p(top_y), _p(count), _p(d20))
    _check(rc, "dm_dense_wide_topk")
    return top_score, top_image, top_x, top_y, count, d20


def iou_above_03(inter: int, box: int) -> bool:
    """`iou(a, b) > 0.3` of two box x box squares that share `inter` pixels, in integers (the module docstring says why it is the
    reference's float64 predicate for box <= 2048)."""
    return 13 * int(inter) > 6 * int(box) * int(box)


def _overlap(a, b, box):
    return max(0, box - abs(int(a[0]) - int(b[0]))) * max(0, box - abs(int(a[1]) - int(b[1])))


def rank_init_detectors_host(num_detectors: int, stats, patches, box: int = 64, max_pairs: int = 5):
    """`rank_init_detectors` (doersch/doersch.py:371-385) with `accept_patch_neighbor` (:46-64) in plain Python, by the rules at the
    top of this module.  stats: {'discriminative-20': {index: key}, 'neighbors': {index: [((x, y), path), ...]}, 'w': {index: row}}
    -> [(index, patches[index], stats['w'][index]), ...] in acceptance order.  Counts all pairs: a path may occur more than once in
    a list."""
    if not 1 <= box <= RANK_MAX_BOX:
        raise ValueError(f"rank: box {box}, need 1 ... {RANK_MAX_BOX}")
    out, lists = [], {}
    for k, _ in sorted(stats["discriminative-20"].items(), key=lambda x: x[1], reverse=True):
        if len(out) == num_detectors:
            break
        mine = {}
        for bbox, path in stats["neighbors"][k]:
            mine.setdefault(path, []).append(bbox)
        ok = True
        for d, _, _ in out:
            count = 0
            for path, theirs in lists[d].items():
                for bbox in mine.get(path, ()):
                    for other in theirs:
                        count += iou_above_03(_overlap(bbox, other, box), box)
            if count > max_pairs:
                ok = False
                break
        if ok:
            out.append((k, patches[k], stats["w"][k]))
            lists[k] = mine
    return out


def detector_rank_workspace_bytes(N: int, L: int, num_detectors: int) -> int:
    need = _lib().dm_detector_rank_workspace_bytes(int(N), int(L), int(num_detectors))
    if not need:
        raise ValueError(f"rank: no workspace for {N} candidates of {L} entries and {num_detectors} detectors")
    return need


def detector_rank(key, nb_image, nb_x, nb_y, nb_count, num_detectors: int, box: int = 64, max_pairs: int = 5, device=None):
    """dm_detector_rank on the current stream: key int32 [N], nb_image / nb_x / nb_y int32 [N, L], nb_count int32 [N] ->
    (accepted int32 [num_detectors] on the device, -1 past the end; n_accepted int32 [1] on the device).  Device tensors are taken as
    they are (the contract — an image at most once per list — is the caller's: a top-k over per-image winners keeps it).  numpy
    arrays are checked against the contract and copied to `device`."""
    import torch
    if isinstance(key, np.ndarray):
        if device is None:
            raise ValueError("rank: numpy lists need the device to run on")
        key, nb_image, nb_x, nb_y, nb_count = (np.ascontiguousarray(a, dtype=np.int32) for a in (key, nb_image, nb_x, nb_y, nb_count))
        for k in range(len(key)):
            row = nb_image[k, :max(0, min(int(nb_count[k]), nb_image.shape[1]))]
            row = row[row >= 0]
            if len(np.unique(row)) != len(row):
                raise ValueError(f"rank: candidate {k} lists an image twice; the device entry needs every image at most once per list")
        key, nb_image, nb_x, nb_y, nb_count = (torch.from_numpy(a).to(device) for a in (key, nb_image, nb_x, nb_y, nb_count))
    tensors = (key, nb_image, nb_x, nb_y, nb_count)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 for t in tensors):
        raise EngineError("rank: the lists must be int32 torch tensors on the GPU, or numpy arrays")
    key, nb_image, nb_x, nb_y, nb_count = (t.contiguous() for t in tensors)
    if nb_image.ndim != 2 or not (nb_image.shape == nb_x.shape == nb_y.shape) or key.shape != (nb_image.shape[0],) or nb_count.shape != key.shape:
        raise ValueError(f"rank: key {tuple(key.shape)}, lists {tuple(nb_image.shape)}, counts {tuple(nb_count.shape)}")
    N, L = nb_image.shape
    dev = key.device
    work = torch.empty(detector_rank_workspace_bytes(N, L, num_detectors), dtype=torch.uint8, device=dev)
    accepted = torch.empty(int(num_detectors), dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib().dm_detector_rank(_stream(torch, dev), _p(key), _p(nb_image), _p(nb_x), _p(nb_y), _p(nb_count), N, L, int(box),
                                     int(max_pairs), int(num_detectors), _p(work), work.numel(), _p(accepted), _p(n))
    _check_rank(rc, "dm_detector_rank")
    return accepted, n


def rank_init_detectors(num_detectors: int, stats, patches, box: int = 64, max_pairs: int = 5):
    """`rank_init_detectors(num_detectors, c, stats, patches)` of doersch/doersch.py:371-385 -> [(index, patch, w), ...].  stats: what
    `CandidateSearch.result` returns.  Where stats['arrays'] holds device tensors (a search that ran on the GPU) the greedy loop runs
    there by `detector_rank`, on the lists as the search left them; otherwise it is `rank_init_detectors_host`."""
    arrays = stats.get("arrays")
    if arrays is None or isinstance(arrays["key"], np.ndarray):
        return rank_init_detectors_host(num_detectors, stats, patches, box, max_pairs)
    accepted, n = detector_rank(arrays["key"], arrays["nb_image"], arrays["nb_x"], arrays["nb_y"], arrays["nb_count"], num_detectors, box,
                                max_pairs)
    accepted = accepted.cpu().numpy()[:int(n.cpu()[0])]
    return [(int(k), patches[int(k)], stats["w"][int(k)]) for k in accepted]


class CandidateSearch:
    """The search of `init_detectors` (doersch/doersch.py:317-369): the wide twin of `DenseSearch` for any K <= 32768 candidates.

        cs = CandidateSearch(w, positive_paths, top_k=50)
        for paths, data in chunks: cs.add(paths, data)          # data: fp16 [B, W, H, C], on the GPU or numpy
        stats = cs.result()

    The two [K][n_images] tables and the path list grow as `DenseSearch`'s do; chunks may differ in (W, H).  `result()` gives the
    reference's metadata {'discriminative-20': {index: d20}, 'neighbors': {index: [((x, y), path), ...]}, 'w': {index: fp16 row}}
    plus 'arrays': key (the d20 counts) int32 [K], nb_image / nb_x / nb_y int32 [K, top_k], nb_count int32 [K] — device tensors after
    a search on the GPU (`rank_init_detectors` takes them where they are), numpy arrays after the host restatement
    (`winners_host` over blocks of 128 detectors, `topk_host`, `discriminative_20`)."""

    def __init__(self, w, positive_paths, top_k: int = 50):
        w = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
        if w.ndim != 2:
            raise ValueError(f"wide search: w must be [K, C], got {w.shape}")
        self.w = np.ascontiguousarray(w.astype(np.float16))
        self.K, self.C = self.w.shape
        self.top_k = int(top_k)
        _check_wide_shape(1, 1, self.C, self.K, self.top_k)
        self.positive = set(positive_paths)
        self.paths, self.dims = [], []
        self.n = 0
        self._host = None
        self._score = self._cell = self._w_dev = self._work = None

    def add(self, paths, data, mask=None):
        """One chunk: `paths` of its B images, data fp16 [B, W, H, C], mask [B, W H] (0 = the cell scores 0) or None."""
        if data.ndim != 4 or data.shape[0] != len(paths) or data.shape[3] != self.C:
            raise ValueError(f"wide search: chunk {tuple(data.shape)} for {len(paths)} paths and {self.C} channels")
        B, W, H, _ = data.shape
        _check_wide_shape(B, W * H, self.C, self.K, self.top_k)
        if mask is not None and tuple(mask.shape) != (B, W * H):
            raise ValueError(f"wide search: mask {tuple(mask.shape)}, need {(B, W * H)}")
        host = isinstance(data, np.ndarray)
        if self._host is None:
            self._host = host
        elif self._host != host:
            raise ValueError("wide search: numpy and device chunks in one search")
        (self._add_host if host else self._add_device)(data, mask, B, W * H)
        self.paths += list(paths)
        self.dims += [(W, H)] * B
        self.n += B

    _grow = DenseSearch._grow

    def _add_host(self, data, mask, B, cells):
        if data.dtype != np.float16:
            raise ValueError("wide search: data must be float16")

        def copy(dst, src):
            dst[:, :self.n] = src[:, :self.n]
        self._grow(B, lambda s, dt: np.empty(s, dtype=dt), copy)
        data = data.reshape(B, cells, self.C)
        mask = None if mask is None else np.asarray(mask)
        for k0 in range(0, self.K, DENSE_MAX_DETECTORS):
            s, c = winners_host(data, self.w[k0:k0 + DENSE_MAX_DETECTORS], mask)
            self._score[k0:k0 + len(s), self.n:self.n + B], self._cell[k0:k0 + len(s), self.n:self.n + B] = s, c

    def _add_device(self, data, mask, B, cells):
        import torch
        if not (isinstance(data, torch.Tensor) and data.is_cuda):
            raise EngineError("CandidateSearch.add: data must be a torch tensor on the GPU, or numpy for the host restatement")
        if data.dtype != torch.float16:
            raise ValueError("wide search: data must be float16")
        dev = data.device
        if self._w_dev is None:
            self._w_dev = torch.from_numpy(self.w).to(dev)
        elif self._w_dev.device != dev:
            raise ValueError(f"wide search: a chunk on {dev}, earlier ones on {self._w_dev.device}")
        data = data.contiguous().view(B, cells, self.C)
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.uint8).contiguous()

        def copy(dst, src):
            dst[:, :self.n].copy_(src[:, :self.n])
        self._grow(B, lambda s, dt: torch.empty(s, dtype=getattr(torch, dt), device=dev), copy)
        need = wide_workspace_bytes(B, cells, self.K)
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.uint8, device=dev)
        wide_winners(data, self._w_dev, self._score, self._cell, self.n, mask, self._work)

    def tables(self):
        """(score float32 [K, n_images], cell int32 [K, n_images]) as numpy arrays."""
        if not self.n:
            raise ValueError("wide search: no chunk yet")
        if self._host:
            return self._score[:, :self.n].copy(), self._cell[:, :self.n].copy()
        return self._score[:, :self.n].cpu().numpy(), self._cell[:, :self.n].cpu().numpy()

    def result(self):
        """The reference's `metadata` plus 'arrays' (the class docstring).  A candidate without an admissible image has an empty
        neighbour list and d20 0."""
        if not self.n:
            raise ValueError("wide search: no chunk yet")
        image_h = np.array([H for _, H in self.dims], dtype=np.int32)
        positive = np.array([p in self.positive for p in self.paths], dtype=np.uint8)
        if self._host:
            _, img, cell, count = topk_host(self._score[:, :self.n], self._cell[:, :self.n], self.top_k)
            h = image_h[np.maximum(img, 0)]
            x, y = np.where(img >= 0, (cell // h) * 8, -1).astype(np.int32), np.where(img >= 0, (cell % h) * 8, -1).astype(np.int32)
            lists = [[(None, (int(x[k, j]), int(y[k, j])), self.paths[img[k, j]]) for j in range(int(count[k]))] for k in range(self.K)]
            d20 = np.array(discriminative_20(lists, self.positive), dtype=np.int32)
            arrays = dict(key=d20, nb_image=img, nb_x=x, nb_y=y, nb_count=count)
        else:
            import torch
            dev = self._score.device
            _, img_d, x_d, y_d, count_d, d20_d = wide_topk(self._score, self._cell, self.n, self.top_k, torch.from_numpy(image_h).to(dev),
                                                           torch.from_numpy(positive).to(dev))
            arrays = dict(key=d20_d, nb_image=img_d, nb_x=x_d, nb_y=y_d, nb_count=count_d)
            img, x, y, count, d20 = (t.cpu().numpy() for t in (img_d, x_d, y_d, count_d, d20_d))
        neighbors = {k: [((int(x[k, j]), int(y[k, j])), self.paths[img[k, j]]) for j in range(int(count[k]))] for k in range(self.K)}
        return {"discriminative-20": {k: int(d20[k]) for k in range(self.K)}, "neighbors": neighbors,
                "w": {k: self.w[k] for k in range(self.K)}, "arrays": arrays}


def sample_patches(image_sizes, how_many: int, num_trials: int = 100, accept=None, rng=None):
    """The loop of `init_patches` (doersch/doersch.py:248-276).  image_sizes: {path: (width, height)} of the seed images (PIL's
    `Image.size`) in the reference's insertion order -> [((x, y, x + 64, y + 64), path), ...], how_many of them.  Every image keeps
    a grid [width // 8 - 8, height // 8 - 8] of positions; the paths are shuffled once and visited round-robin; a visit permutes the
    free positions (`rng.permutation`), tries the first num_trials and takes the first that `accept(path, bbox)` admits (None: the
    first); every trial marks position (X[0], Y[1]) of the permuted lists — the reference's line as written, which marks neither the
    tried nor the taken position (with one free position left, where the reference's Y[1] fails, Y[0]).  The reference's accept is
    skimage's `is_low_contrast` on the crop, which is not restated here.  rng: anything with `shuffle(list)` and `permutation(n)` — a
    numpy Generator or RandomState; None draws as the reference does, from Python's `random.shuffle` and `numpy.random.permutation`."""
    import random
    shuffle = random.shuffle if rng is None else rng.shuffle
    permutation = np.random.permutation if rng is None else rng.permutation
    elems = {}
    for path, (width, height) in image_sizes.items():
        if width // 8 - 8 < 1 or height // 8 - 8 < 1:
            raise ValueError(f"sample_patches: {path} of {width} x {height} pixels has no patch position")
        elems[path] = np.zeros((width // 8 - 8, height // 8 - 8))
    if not elems or how_many < 0:
        raise ValueError("sample_patches: no seed image, or how_many < 0")
    keys = list(elems.keys())
    key_id, patches, idle = 0, [], 0
    shuffle(keys)
    while len(patches) < how_many:
        path = keys[key_id]
        X, Y = np.where(elems[path] == 0)
        idx = permutation(len(X))
        X, Y = X[idx][:num_trials], Y[idx][:num_trials]
        before = len(patches)
        for j in range(len(X)):
            elems[path][X[0], Y[min(1, len(Y) - 1)]] = 1
            bbox = (int(X[j]) * 8, int(Y[j]) * 8, int(X[j]) * 8 + 64, int(Y[j]) * 8 + 64)
            if accept is None or accept(path, bbox):
                patches.append((bbox, path))
                break
        idle = 0 if len(patches) > before or len(X) else idle + 1
        if idle >= len(keys):
            raise ValueError(f"sample_patches: no free position left after {len(patches)} of {how_many} patches")
        key_id = (key_id + 1) % len(keys)
    return patches


def _patch_rows(data, picks):
    """The detectors of one chunk's patches: data fp16 [B, W, H, C]; picks [(image in the chunk, bbox), ...] -> fp16 numpy [n, C],
    row (bbox[0] // 8, bbox[1] // 8) of each image's features (`detector_from_patch`, one gather for the chunk)."""
    B, W, H, C_ = data.shape
    pairs = []
    for b, bbox in picks:
        a, c = int(bbox[0]) // 8, int(bbox[1]) // 8
        if not (0 <= a < W and 0 <= c < H):
            raise ValueError(f"init_detectors: bbox {tuple(bbox)} outside {W} x {H} blocks")
        pairs.append((b, a * H + c))
    pairs = np.array(pairs, dtype=np.int32)
    if isinstance(data, np.ndarray):
        return data.reshape(B, W * H, C_)[pairs[:, 0], pairs[:, 1]].copy()
    import torch
    return gather(data.contiguous().view(B, W * H, C_), torch.from_numpy(pairs).to(data.device)).cpu().numpy()


def _init_from_chunks(patches, positive_paths, top_k, chunks_from, cache_bytes):
    """chunks_from(start) yields (paths, data fp16 [B, W, H, C]) from chunk `start` on.  Pass one takes every candidate's own row
    and keeps the chunks themselves while they fit `cache_bytes`; pass two searches the kept chunks and produces only the rest again."""
    want = {}
    for index, (bbox, path) in enumerate(patches):
        want.setdefault(path, []).append((index, bbox))
    rows, kept, held, full = [None] * len(patches), [], 0, False
    for names, data in chunks_from(0):
        picks = [(b, index, bbox) for b, name in enumerate(names) for index, bbox in want.get(name, ())]
        if picks:
            for (_, index, _), row in zip(picks, _patch_rows(data, [(b, bbox) for b, _, bbox in picks])):
                rows[index] = row
        size = int(np.prod(data.shape)) * 2
        if not full and held + size <= cache_bytes:
            kept.append((names, data))
            held += size
        else:
            full = True
    missing = [patches[i][1] for i, r in enumerate(rows) if r is None]
    if missing:
        raise ValueError(f"init_detectors: {len(missing)} patches of images outside the data set, e.g. {missing[0]}")
    cs = CandidateSearch(np.stack(rows), positive_paths, top_k=top_k)
    for names, data in kept:
        cs.add(names, data)
    if full:
        for names, data in chunks_from(len(kept)):
            cs.add(names, data)
    return cs.result()


def init_detectors(patches, sft_paths, positive_paths, top_k: int = 50, device_id: str = "cuda", cache_bytes: int = 8 << 30):
    """`init_detectors(c, patches)` of doersch/doersch.py:317-369 on the reference's safetensors shards (each key `';;'.join(paths)`
    with a tensor [B, W, H, C] of normalised features, as `dense_search` reads them): candidate `index` of patches = [(bbox, path),
    ...] becomes the detector `features(path)[bbox[0] // 8, bbox[1] // 8]` (:337) and all of them search every key of every shard.
    The shards are read once where all of them fit `cache_bytes` of device (or host) memory, twice otherwise.  device_id "cpu" takes
    the numpy restatements.  Returns what `CandidateSearch.result` returns."""
    import torch
    from safetensors import safe_open
    host = device_id == "cpu"
    device = torch.device(device_id)

    def chunks_from(start):
        at = 0
        for sft_path in sft_paths:
            with safe_open(sft_path, framework="pt", device=device_id if device_id in ("cuda", "cpu") else device.index) as f:
                for key in f.keys():
                    at += 1
                    if at <= start:
                        continue
                    data = f.get_tensor(key).to(device).half()
                    yield key.split(";;"), (data.numpy() if host else data)
    return _init_from_chunks(patches, positive_paths, top_k, chunks_from, cache_bytes)


def init_detectors_images(patches, image_paths, positive_paths, batch: int = 16, top_k: int = 50, device_id: str = "cuda",
                          cache_bytes: int = 8 << 30):
    """`init_detectors`, fed from image files: per batch of `batch` paths the images are read (`read_images`) and their features
    computed (`hoglab`), size group by size group as in `dense_search_images`.  The candidates' own rows are gathered from the same
    features, so a data set whose features fit `cache_bytes` is read once for both purposes; past that the remaining batches are
    read and computed a second time for the search.  Returns what `CandidateSearch.result` returns."""
    import torch
    if batch < 1:
        raise ValueError(f"init_detectors: batch {batch}")
    host = device_id == "cpu"
    device = torch.device(device_id)
    image_paths = list(image_paths)

    group_counts = []                                # size groups per batch, known once the batch has been read

    def chunks_from(start):
        n = 0
        for bi, at in enumerate(range(0, len(image_paths), batch)):
            names = image_paths[at:at + batch]
            if bi < len(group_counts) and n + group_counts[bi] <= start:
                n += group_counts[bi]
                continue
            groups = read_images(names)
            if bi == len(group_counts):
                group_counts.append(len(groups))
            for g, (idx, images) in enumerate(groups):
                if n + g >= start:
                    data = hoglab(images) if host else hoglab(torch.from_numpy(images).to(device))
                    yield [names[j] for j in idx], data
            n += len(groups)
    return _init_from_chunks(patches, positive_paths, top_k, chunks_from, cache_bytes)


def initialize_classifier(seed_paths, image_paths, positive_paths, how_many: int = 25000, num_detectors: int = 1000,
                          num_trials: int = 100, accept=None, rng=None, batch: int = 16, top_k: int = 50, device_id: str = "cuda"):
    """`initialize_classifier` (doersch/doersch.py:387-400) without its cache files: `sample_patches` over the seed images' sizes,
    `init_detectors_images` over the data set, `rank_init_detectors` -> (patches, [(index, patch, w), ...])."""
    from PIL import Image
    sizes = {}
    for path in seed_paths:
        with Image.open(path) as im:
            sizes[path] = im.size
    patches = sample_patches(sizes, how_many, num_trials=num_trials, accept=accept, rng=rng)
    stats = init_detectors_images(patches, image_paths, positive_paths, batch=batch, top_k=top_k, device_id=device_id)
    return patches, rank_init_detectors(num_detectors, stats, patches)
