"""The clustering stage's last step on the GPU: scikit-learn's `KMeans(n_clusters=k, random_state=10).fit(X)` and the tail of
the reference's `cluster()` (typicality/cluster.py:312-328, applications/parallel-dataset/cluster.py:268-289,
clipmining/ranking.py:131-149) — members ordered by distance to their cluster's reference point, clusters ranked by the median
or mean `D` of their members.  Kernels: csrc/kmeans.hip; C ABI: dm_kmeans_workspace_bytes / dm_kmeans_fit / dm_cluster_rank.

What scikit-learn does on this call (1.4.2 and 1.7.2 alike: n_init='auto' -> one k-means++ run, algorithm='lloyd',
max_iter=300, tol=1e-4), restated here in numpy (`kmeans_fit_host`) with the rules the kernels follow:

  centre    mean = X.mean(0) (fp32), Xc = X - mean, tol_abs = tol * mean(var(X, 0)).
  seeding   distances in fp64 (xx_i + xx_c - 2 xc_i.xc_c on the upcast rows), rounded to fp32 and clamped at 0; the first index
            is searchsorted(cdf, u0, 'right') = floor(u0 n); then per centre t = 2 + int(ln k) candidates by searchsorted(cumsum
            (closest), u * potential) clipped to n - 1, potential of each = sum min(closest, distance), lowest potential wins, first
            among equals.  The uniforms come from the host (`kmeans_uniforms`): the device needs no generator.
  Lloyd     fp32: score = |c|^2 - 2 xc.c, argmin with the lowest index among equals; new centres = member sums in ascending row
            order times 1/count; empty clusters, in ascending id, take the rows farthest from their own centre, in descending
            distance (each leaves its old cluster's sum and count); shift = sum_j |c_new - c_old|^2; stop strictly when the labels
            repeat, else when shift <= tol_abs; after a non-strict stop (or max_iter) one more assignment.

UMAP (umapfit.py, csrc/umap.hip and, from 4096 rows up to 65535, csrc/umap_sparse.hip; parity with umap-learn unpinned) is `cluster_patches(project=...)`: `project=5` is the main
stage's project=True, `project=('groups', G, 32)` the parallel dataset's compress(); the default None is the reference's
project=False.  One call clusters one category; several categories are several calls (no batched entry yet).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from .engine import EngineError, _p, load_library as _lib

KMEANS_MAX_K = 256           # DM_KMEANS_MAX_K
KMEANS_MAX_N = 1 << 24       # n >= 2^24 is refused
RANK_CENTROID, RANK_FARTHEST = 0, 1
AGG_MEDIAN, AGG_MEAN = 0, 1
_MODES = {"centroid": RANK_CENTROID, "farthest": RANK_FARTHEST}
_AGGS = {"median": AGG_MEDIAN, "mean": AGG_MEAN}
# dm_kmeans_fit / dm_cluster_rank return codes (include/dm_engine.h)
ERRORS = {1: "null argument", 2: "n < k", 3: f"k outside [1, {KMEANS_MAX_K}]", 4: "d < 1", 5: "n >= 2^24", 6: "max_iter < 1",
          7: "wrong number of uniforms", 8: "workspace too small", 9: "bad mode / aggregate", 10: "HIP error"}


def n_local_trials(k: int) -> int:
    return 2 + int(math.log(k))


def kmeans_uniforms(k: int, seed: int = 10) -> np.ndarray:
    """The draws scikit-learn's k-means++ consumes from `np.random.RandomState(seed)`: `choice`'s single uniform, then
    `uniform(size=t)` per later centre, t = 2 + int(ln k).  float64 [1 + (k - 1) t]."""
    rs = np.random.RandomState(seed)
    t = n_local_trials(k)
    out = [np.atleast_1d(rs.random_sample())]
    for _ in range(1, k):
        out.append(rs.uniform(size=t))
    return np.concatenate(out).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# the numpy restatement: the CPU-tier yardstick, and what runs where no GPU is present
# ------------------------------------------------------------------------------------------------------------------------------
def _seed_host(Xc: np.ndarray, k: int, uniforms: np.ndarray, trace=None) -> np.ndarray:
    n = Xc.shape[0]
    t = n_local_trials(k)
    Xd = Xc.astype(np.float64)
    xx = (Xd * Xd).sum(axis=1)

    def dist(c):
        return np.maximum((xx + xx[c] - 2.0 * (Xd @ Xd[c])).astype(np.float32), np.float32(0))

    idx = np.empty(k, dtype=np.int32)
    idx[0] = min(n - 1, int(math.floor(uniforms[0] * n)))
    closest = dist(idx[0])
    pot = closest.astype(np.float64).sum()
    for c in range(1, k):
        rand = uniforms[1 + (c - 1) * t: 1 + c * t] * pot
        cum = np.cumsum(closest, dtype=np.float64)
        cand = np.minimum(np.searchsorted(cum, rand), n - 1)
        m = np.minimum(closest[None, :], np.stack([dist(ci) for ci in cand]))
        pots = m.astype(np.float64).sum(axis=1)
        b = int(np.argmin(pots))
        if trace is not None:
            trace.append({"rand": rand, "cum": cum, "cand": cand, "pots": pots, "pot": pot})
        idx[c], closest, pot = cand[b], m[b], pots[b]
    return idx


def _assign_host(Xc, Cn):
    cn = (Cn * Cn).sum(axis=1, dtype=np.float32)
    S = cn[None, :] - np.float32(2) * (Xc @ Cn.T)
    return S.argmin(axis=1).astype(np.int32), S


def kmeans_fit_host(X, k: int = 32, seed: int = 10, max_iter: int = 300, tol: float = 1e-4, init_index=None, trace=None):
    """float64 seeding and fp32 Lloyd on mean-centred rows, by the rules at the top of this module.  Returns (labels int32 [n],
    centers fp32 [k, d], seed_index int32 [k], inertia, n_iter).  init_index: k row indices to start from instead of seeding
    (`KMeans(init=X[init_index], n_init=1)`).  trace: a list that receives one dict per seeding step and per iteration."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    _check_args(n, d, k, max_iter)
    mean = X.mean(axis=0)
    tol_abs = np.float32(np.mean(np.var(X, axis=0)) * tol)
    Xc = X - mean
    if init_index is None:
        seeds = _seed_host(Xc, k, kmeans_uniforms(k, seed), trace)
    else:
        seeds = np.asarray(init_index, dtype=np.int32)
        assert seeds.shape == (k,)
    Cn = Xc[seeds].copy()
    prev = np.full(n, -1, dtype=np.int32)
    strict = False
    for it in range(max_iter):
        labels, S = _assign_host(Xc, Cn)
        sums = np.zeros((k, d), dtype=np.float32)
        counts = np.zeros(k, dtype=np.int64)
        for j in range(k):
            rows = Xc[labels == j]
            counts[j] = len(rows)
            if len(rows):
                sums[j] = np.add.reduce(rows, axis=0)            # ascending row order, fp32
        empty = np.flatnonzero(counts == 0)
        if len(empty):
            dist = ((Xc - Cn[labels]) ** 2).sum(axis=1)
            for j in empty:
                far = int(np.argmax(dist))                       # descending distance, lowest row among equals
                dist[far] = -1
                sums[labels[far]] -= Xc[far]
                counts[labels[far]] -= 1
                sums[j] = Xc[far]
                counts[j] = 1
        new = sums.copy()
        nz = counts > 0
        new[nz] *= (np.float32(1) / counts[nz].astype(np.float32))[:, None]
        shift = np.float32((np.sqrt(((new - Cn) ** 2).sum(axis=1)) ** 2).sum())
        if trace is not None:
            trace.append({"scores": S, "shift": shift, "tol_abs": tol_abs})
        Cn = new
        if np.array_equal(labels, prev):
            strict = True
            break
        if shift <= tol_abs:
            break
        prev = labels
    if not strict:
        labels, S = _assign_host(Xc, Cn)
        if trace is not None:
            trace.append({"scores": S})
    inertia = float(((Xc - Cn[labels]) ** 2).sum(axis=1).astype(np.float64).sum())
    return labels, Cn + mean, seeds, inertia, it + 1


def _check_args(n, d, k, max_iter):
    if k < 1 or k > KMEANS_MAX_K:
        raise ValueError(f"kmeans: k {k} outside [1, {KMEANS_MAX_K}]")
    if n < k:
        raise ValueError(f"kmeans: n {n} < k {k}")
    if d < 1:
        raise ValueError("kmeans: d < 1")
    if n >= KMEANS_MAX_N:
        raise ValueError(f"kmeans: n {n} >= 2^24")
    if max_iter < 1:
        raise ValueError("kmeans: max_iter < 1")


def rank_clusters_host(X, labels, centers, D, aggregate: str = "median", order_by: str = "centroid", rank_features=None):
    """The tail of the reference's `cluster()` as arrays.  Returns (order int32 [n], cluster_of_rank int32 [k], offsets int32
    [k + 1], aggregate fp32 [k], n_nonempty): ranked cluster r is cluster id cluster_of_rank[r], its rows in order are
    order[offsets[r]:offsets[r + 1]]; slots past n_nonempty hold -1 / n / NaN.  A NaN aggregate ranks after every number
    (Python's `sorted` leaves the place of a NaN key to its algorithm)."""
    X = np.asarray(X, dtype=np.float32)
    labels = np.asarray(labels)
    centers = np.asarray(centers, dtype=np.float32)
    D = np.asarray(D, dtype=np.float32)
    n, k = len(labels), len(centers)
    Xr = X if rank_features is None else np.asarray(rank_features, dtype=np.float32)
    if _MODES[order_by] == RANK_FARTHEST:
        far = [int(np.argmax(((X.astype(np.float64) - c.astype(np.float64)) ** 2).sum(axis=1))) for c in centers]
        ref = Xr[far]
    else:
        ref = centers
    key = np.sqrt(((Xr.astype(np.float64) - ref[labels].astype(np.float64)) ** 2).sum(axis=1))
    found = []
    for j in range(k):
        rows = np.flatnonzero(labels == j)
        if not len(rows):
            continue
        rows = rows[np.argsort(key[rows], kind="stable")]
        if _AGGS[aggregate] == AGG_MEDIAN:
            agg = np.float32(np.median(D[rows]))
        else:
            s = np.float32(0)
            for v in D[rows]:
                s = np.float32(s + v)
            agg = np.float32(s / np.float32(len(rows)))
        found.append((j, rows, agg, int(np.flatnonzero(labels == j)[0])))
    found.sort(key=lambda f: f[3])                                              # dict insertion order: first appearance by row
    ranked = sorted(found, key=lambda f: (math.isnan(f[2]), -f[2] if not math.isnan(f[2]) else 0.0))     # stable
    order = np.concatenate([f[1] for f in ranked]).astype(np.int32) if ranked else np.zeros(0, np.int32)
    cluster_of_rank = np.full(k, -1, dtype=np.int32)
    offsets = np.full(k + 1, n, dtype=np.int32)
    agg_out = np.full(k, np.nan, dtype=np.float32)
    pos = 0
    for r, f in enumerate(ranked):
        cluster_of_rank[r], offsets[r], agg_out[r] = f[0], pos, f[2]
        pos += len(f[1])
    return order, cluster_of_rank, offsets, agg_out, len(ranked)


# ------------------------------------------------------------------------------------------------------------------------------
# the device path
# ------------------------------------------------------------------------------------------------------------------------------
def _fail(what, rc):
    raise EngineError(f"{what}: {ERRORS.get(rc, 'error')} (code {rc})")


def workspace_bytes(n: int, d: int, k: int) -> int:
    out = C.c_size_t(0)
    rc = _lib().dm_kmeans_workspace_bytes(int(n), int(d), int(k), C.byref(out))
    if rc:
        _fail("dm_kmeans_workspace_bytes", rc)
    return out.value


def _dev_f32(x, device=None):
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if device is not None and x.device != device:
        x = x.to(device)
    return x.to(torch.float32).contiguous()


def kmeans_fit(X, k: int = 32, seed: int = 10, max_iter: int = 300, tol: float = 1e-4, init_index=None, work=None):
    """`KMeans(n_clusters=k, random_state=seed).fit(X)` on the device X lives on (dm_kmeans_fit) — fp32 [n, d] torch tensor.
    Returns device tensors (labels int32 [n], centers fp32 [k, d], seed_index int32 [k], inertia fp32 [], n_iter int32 []).
    Bit-reproducible: no floating-point atomics, every sum in a fixed order.  init_index: start from these k rows instead of
    seeding.  work: a uint8 workspace of at least `workspace_bytes(n, d, k)` to reuse (its contents do not matter).
    There is no host path behind this call: without a GPU it raises; `kmeans_fit_host` is the numpy restatement."""
    import torch
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise EngineError("kmeans_fit: X must be a torch tensor on the GPU (kmeans_fit_host is the numpy restatement)")
    if X.dim() != 2:
        raise EngineError(f"kmeans_fit: X must be [n, d], got {tuple(X.shape)}")
    X = _dev_f32(X)
    n, d = X.shape
    lib = _lib()
    dev = X.device
    need = workspace_bytes(n, d, k)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    centers = torch.empty((k, d), dtype=torch.float32, device=dev)
    inertia = torch.empty((), dtype=torch.float32, device=dev)
    n_iter = torch.empty((), dtype=torch.int32, device=dev)
    if init_index is None:
        u = kmeans_uniforms(k, seed)
        u_dev = torch.from_numpy(u).to(dev)
        seed_index = torch.empty(k, dtype=torch.int32, device=dev)
    else:
        u, u_dev = np.zeros(0), None
        seed_index = torch.as_tensor(np.asarray(init_index, dtype=np.int32)).to(dev)
        if seed_index.shape != (k,) or int(seed_index.min()) < 0 or int(seed_index.max()) >= n:
            raise EngineError("kmeans_fit: init_index must be k row indices")
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.dm_kmeans_fit(stream, _p(X), n, d, int(k), _p(u_dev), len(u), int(max_iter), float(tol), _p(work), work.numel(),
                               _p(labels), _p(centers), _p(seed_index), _p(inertia), _p(n_iter))
    if rc:
        _fail("dm_kmeans_fit", rc)
    return labels, centers, seed_index, inertia, n_iter


def rank_clusters(X, labels, centers, D, aggregate: str = "median", order_by: str = "centroid", rank_features=None, work=None):
    """The tail of the reference's `cluster()` on the device (dm_cluster_rank); arguments and results as `rank_clusters_host`,
    as device tensors (n_nonempty: int32 [])."""
    import torch
    if order_by not in _MODES or aggregate not in _AGGS:
        raise EngineError(f"rank_clusters: order_by {order_by!r} / aggregate {aggregate!r}")
    if not (isinstance(X, torch.Tensor) and X.is_cuda):
        raise EngineError("rank_clusters: X must be a torch tensor on the GPU (rank_clusters_host is the numpy restatement)")
    X = _dev_f32(X)
    dev = X.device
    n, d = X.shape
    Xr = _dev_f32(rank_features, dev) if rank_features is not None else None
    if Xr is not None and (Xr.dim() != 2 or Xr.shape[0] != n):
        raise EngineError("rank_clusters: rank_features must be [n, d_rank]")
    if Xr is not None and order_by == "centroid":
        raise EngineError("rank_clusters: rank_features go with order_by='farthest' (a centre lives in the clustered space)")
    centers = _dev_f32(centers, dev)
    k = centers.shape[0]
    labels = labels.to(device=dev, dtype=torch.int32).contiguous()
    D = _dev_f32(D, dev)
    if labels.shape != (n,) or D.shape != (n,) or centers.shape != (k, d):
        raise EngineError("rank_clusters: labels [n], D [n], centers [k, d] expected")
    need = workspace_bytes(n, max(d, Xr.shape[1] if Xr is not None else 1), k)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    cluster_of_rank = torch.empty(k, dtype=torch.int32, device=dev)
    offsets = torch.empty(k + 1, dtype=torch.int32, device=dev)
    agg = torch.empty(k, dtype=torch.float32, device=dev)
    n_nonempty = torch.empty((), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = _lib().dm_cluster_rank(stream, _p(X), _p(Xr), n, d, Xr.shape[1] if Xr is not None else d, _p(labels), _p(centers), k,
                                    _p(D), _MODES[order_by], _AGGS[aggregate], _p(work), work.numel(), _p(order),
                                    _p(cluster_of_rank), _p(offsets), _p(agg), _p(n_nonempty))
    if rc:
        _fail("dm_cluster_rank", rc)
    return order, cluster_of_rank, offsets, agg, n_nonempty


def cluster_patches(features, D, num_clusters: int = 32, aggregate: str = "median", seed: int = 10, order_by: str = "centroid",
                    rank_features=None, max_iter: int = 300, tol: float = 1e-4, *, project=None, project_seed: int = 42,
                    project_solver: str = "host", project_disconnected: str = "random"):
    """`cluster()` of the reference as arrays: fit, then rank.  On a GPU tensor both run on the device and only the small result
    comes back; a numpy array (or a CPU tensor) takes the numpy restatement.  Returns a dict: 'clusters' = a list, best first, of
    {'cluster': id, 'rows': row ids in order (int32), 'aggregate': float}, plus 'labels', 'centers', 'seed_index', 'inertia',
    'n_iter'.  ids, paths and images stay the caller's, keyed by row.

    project: None = no projection.  An int c = the main stage's project=True with `umap.UMAP(n_components=c)` (typicality/cluster.py:
    314-317; the reference uses 5): k-means and the ranking both run on the embedding.  ('groups', G, c) = the parallel dataset's
    cluster() (cluster.py:268-289): k-means on `umapfit.compress(features, G, c)`, members ranked with order_by='farthest' on the
    original features.  project_seed seeds the projection (umap-learn is unseeded at both call sites).  project_solver: 'host' or 'device', `umapfit.umap_fit`'s
    init_solver (where the spectral initialisation runs; a numpy input ignores it).  project_disconnected: `umapfit.umap_fit`'s
    disconnected ('random', the default, or 'components': a k-NN graph that falls into several components gets one spectral embedding
    per component instead of a random start).  With a projection the dict also holds 'embedding'."""
    import torch
    embedding = None
    if project is not None:
        from . import umapfit
        if isinstance(project, (tuple, list)):
            if len(project) != 3 or project[0] != "groups":
                raise ValueError(f"cluster_patches: project {project!r} (None, an int, or ('groups', G, n_components))")
            embedding = umapfit.compress(features, int(project[1]), int(project[2]), seed=project_seed, init_solver=project_solver,
                                         disconnected=project_disconnected)
            features, rank_features, order_by = embedding, features if rank_features is None else rank_features, "farthest"
        else:
            on_dev = isinstance(features, torch.Tensor) and features.is_cuda
            if on_dev:
                embedding = umapfit.umap_fit(features, int(project), seed=project_seed, init_solver=project_solver,
                                             disconnected=project_disconnected)["embedding"]
            else:
                embedding = umapfit.umap_fit_host(features.numpy() if isinstance(features, torch.Tensor) else np.asarray(features),
                                                  int(project), seed=project_seed,
                                                  route=umapfit.pick_route("auto", len(features)),
                                                  disconnected=project_disconnected)["embedding"]
            features = embedding
    on_gpu = isinstance(features, torch.Tensor) and features.is_cuda
    if on_gpu:
        labels, centers, seeds, inertia, n_iter = kmeans_fit(features, num_clusters, seed, max_iter, tol)
        order, cor, off, agg, nn = rank_clusters(features, labels, centers, D, aggregate, order_by, rank_features)
        order, cor, off, agg, nn = order.cpu().numpy(), cor.cpu().numpy(), off.cpu().numpy(), agg.cpu().numpy(), int(nn)
        inertia, n_iter = float(inertia), int(n_iter)
    else:
        f = features.numpy() if isinstance(features, torch.Tensor) else np.asarray(features)
        r = rank_features.numpy() if isinstance(rank_features, torch.Tensor) else rank_features
        Dh = D.cpu().numpy() if isinstance(D, torch.Tensor) else D
        labels, centers, seeds, inertia, n_iter = kmeans_fit_host(f, num_clusters, seed, max_iter, tol)
        order, cor, off, agg, nn = rank_clusters_host(f, labels, centers, Dh, aggregate, order_by, r)
    clusters = [{"cluster": int(cor[r]), "rows": order[off[r]:off[r + 1]].copy(), "aggregate": float(agg[r])} for r in range(nn)]
    out = {"clusters": clusters, "labels": labels, "centers": centers, "seed_index": seeds, "inertia": inertia, "n_iter": n_iter}
    if embedding is not None:
        out["embedding"] = embedding
    return out
