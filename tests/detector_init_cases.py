"""The cases of the detector initialisation (tests/test_detector_init.py, tests/test_gpu_detector_init.py): generated from
`numpy.random.default_rng(seed)`, never stored.  tests/make_golden_detector_init.py runs the reference's `rank_init_detectors` on the
ranking cases and records the accepted indices in tests/golden/detector_init_ref.json.

    ranking    groups of near-duplicate neighbour lists: a group has a base list of L distinct images with corners on the 8-pixel
               grid; a member copies it, replaces each entry's image with probability `swap` by one the list does not hold, moves
               each corner by 8 * (-2 ... 2) in x and y, and keeps the first `count` entries (count < L for some: `ragged`).  Keys
               are small integers, so ties are common.  Members of one group overlap in many images and mostly reject each other;
               groups rarely meet.  In front of them sit five planted candidates with the largest keys, 104 ... 100 (A, C, D, B, E;
               box 64, max_pairs 5, entries a0 ... a11 of A's list):
                 A  the list itself: accepted first
                 C  a0 ... a4 where A has them: 5 pairs with A, accepted
                 D  a5 ... a8 where A has them, a9 moved by (32, 8): overlap 32 x 56 = 1792, 13 * 1792 < 6 * 4096, no pair, a10 moved by
                    (24, 16): overlap 40 x 48 = 1920, 13 * 1920 > 6 * 4096, a pair: 5 pairs, accepted
                 B  a0 ... a2, a5 ... a7 where A has them: 6 pairs with A (3 with C, 3 with D), rejected by A
                 E  a0 ... a2, a5, a6 where A has them and a11 moved by (24, 16): 6 pairs with A, rejected by A
               the other entries of C, D, B and E name images that no other list holds.
    edge       small cases without planted candidates: L = 1 (the reference's max_pairs of 5 rejects nothing there; the GPU test also
               runs it with max_pairs 0 against the host restatement), num_detectors = 1, all keys equal.
"""
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLDEN_DIR, "detector_init_ref.json")
BOX, MAX_PAIRS = 64, 5

#            candidates, entries, groups, images, detectors asked for, how the reference's visit ends
RANKING = {
    "R1": dict(seed=101, N=150, L=12, groups=10, images=300, num_detectors=12, ragged=False, planted=True, ends="full"),
    "R2": dict(seed=102, N=120, L=50, groups=15, images=600, num_detectors=64, ragged=True, planted=True, ends="exhausted"),
    "R3": dict(seed=103, N=1025, L=12, groups=25, images=900, num_detectors=48, ragged=True, planted=True, ends="full"),   # N = 1024 + 1
    "E1": dict(seed=104, N=40, L=1, groups=8, images=30, num_detectors=16, ragged=False, planted=False, ends=None),
    "E2": dict(seed=105, N=30, L=8, groups=5, images=60, num_detectors=1, ragged=False, planted=False, ends=None),
    "E3": dict(seed=106, N=60, L=8, groups=10, images=80, num_detectors=20, ragged=True, planted=False, ends=None, equal_keys=True),
}
RICH = ("R1", "R2", "R3")        # the cases the generator holds to its assertions (a) ... (e)


def ranking(tag):
    """-> dict(key int32 [N], nb_image / nb_x / nb_y int32 [N, L], nb_count int32 [N]); unused slots hold -1"""
    s = RANKING[tag]
    rng = np.random.default_rng(s["seed"])
    N, L, n_img = s["N"], s["L"], s["images"]
    img = np.full((N, L), -1, dtype=np.int32)
    x, y = np.full((N, L), -1, dtype=np.int32), np.full((N, L), -1, dtype=np.int32)
    count = np.full(N, L, dtype=np.int32)
    key = rng.integers(0, 21, size=N).astype(np.int32)
    at = 0
    if s["planted"]:
        fresh = iter(range(n_img, n_img + 1000))          # images no generated list holds
        a_img = rng.choice(n_img, size=12, replace=False)
        a_x, a_y = 8 * rng.integers(4, 40, size=12), 8 * rng.integers(4, 40, size=12)

        def plant(entries, k):
            rows = [(a_img[j], a_x[j] + dx, a_y[j] + dy) for j, dx, dy in entries]
            while len(rows) < min(L, 12):
                rows.append((next(fresh), 8 * int(rng.integers(4, 40)), 8 * int(rng.integers(4, 40))))
            rows = [rows[j] for j in rng.permutation(len(rows))]
            n = len(rows)
            img[at, :n], x[at, :n], y[at, :n] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
            count[at], key[at] = n, k
        same = lambda js: [(j, 0, 0) for j in js]          # noqa: E731
        for entries, k in ((same(range(12)), 104), (same(range(5)), 103), (same((5, 6, 7, 8)) + [(9, 32, 8), (10, 24, 16)], 102),
                           (same((0, 1, 2, 5, 6, 7)), 101), (same((0, 1, 2, 5, 6)) + [(11, 24, 16)], 100)):
            plant(entries, k)
            at += 1
    members = np.array_split(np.arange(at, N), s["groups"])
    for group in members:
        base = rng.choice(n_img, size=L, replace=False)
        bx, by = 8 * rng.integers(4, 40, size=L), 8 * rng.integers(4, 40, size=L)
        for k in group:
            row = base.copy()
            for j in np.flatnonzero(rng.random(L) < 0.25):
                other = int(rng.integers(0, n_img))
                while other in row:
                    other = int(rng.integers(0, n_img))
                row[j] = other
            img[k], x[k], y[k] = row, bx + 8 * rng.integers(-2, 3, size=L), by + 8 * rng.integers(-2, 3, size=L)
            if s["ragged"] and rng.random() < 0.5:
                count[k] = int(rng.integers((L + 1) // 2, L + 1))
                img[k, count[k]:], x[k, count[k]:], y[k, count[k]:] = -1, -1, -1
    if s.get("equal_keys"):
        key[:] = 7
    return dict(key=key, nb_image=img, nb_x=x, nb_y=y, nb_count=count)


def path_of(image):
    return f"img{int(image):05d}.jpg"


def stats_of(arrays):
    """the reference's metadata of a ranking case: {'discriminative-20', 'neighbors', 'w'} keyed by candidate index"""
    N = len(arrays["key"])
    neighbors = {k: [((int(arrays["nb_x"][k, j]), int(arrays["nb_y"][k, j])), path_of(arrays["nb_image"][k, j]))
                     for j in range(int(arrays["nb_count"][k]))] for k in range(N)}
    return {"discriminative-20": {k: int(arrays["key"][k]) for k in range(N)}, "neighbors": neighbors, "w": {k: k for k in range(N)}}


def patches_of(arrays):
    return [((8 * k, 0, 8 * k + 64, 64), f"seed{k:05d}.jpg") for k in range(len(arrays["key"]))]


def golden():
    with open(JSON) as f:
        return json.load(f)


# ---- `sample_patches`: the reference's `init_patches` under seeded global generators and a stub contrast filter ---------------------
SAMPLE = dict(seed=7, how_many=40, num_trials=5)


def sample_sizes():
    """{path: (width, height)}"""
    return {f"seed{j}.jpg": (96 + 8 * j, 120 - 8 * (j % 3)) for j in range(5)}


def sample_accept(path, bbox):
    return (bbox[0] // 8 + 3 * (bbox[1] // 8) + len(path) + int(path[4])) % 3 != 0


# ---- the search: tables the wide kernel must reproduce bit for bit (the narrow kernel over blocks of 128 is the reference) -----------
#            images per chunk, W, H, C, K, density, fold, NaN rows as in dense_search_cases.S4
WIDE = {
    "W1": dict(chunks=(3, 4), W=9, H=7, C=72, K=300, density=0.3, fold=(1, 3), nan=False, seed=201),
    "W2": dict(chunks=(3, 4), W=9, H=7, C=72, K=200, density=0.3, fold=(2, 3), nan=True, seed=202),
    "W3": dict(chunks=(2,), W=9, H=7, C=2112, K=130, density=0.1, fold=None, nan=False, seed=203),
    "W4": dict(chunks=(3, 4), W=9, H=7, C=72, K=1, density=0.3, fold=None, nan=False, seed=204),
    "W5": dict(chunks=(1,), W=23, H=13, C=136, K=260, density=0.3, fold=None, nan=False, seed=205),       # 299 cells: two cell tiles of 256
}
NAN_ROW, NAN_IMAGE = (1, 17), 5


def to_f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float16)


def wide_inputs(tag):
    """-> (w fp16 [K, C], [(paths, data fp16 [B, W, H, C], mask uint8 [B, W H] or None), ...]).  Features as dense_search_cases':
    sparse squares of uniforms, L2-normalised per cell; detectors: scaled copies of cells plus noise whose
    entries are negated with a probability drawn per detector from [0.5, 0.95): winners of both signs, masked zeros that win."""
    from diff_mining_amd.doersch import fold_mask
    s = WIDE[tag]
    rng = np.random.default_rng(s["seed"])
    n = sum(s["chunks"])
    shape = (n, s["W"], s["H"], s["C"])
    f = rng.random(shape) ** 2 * (rng.random(shape) < s["density"])
    f[..., 0] += 1e-3
    f = to_f16(f / np.linalg.norm(f, axis=-1, keepdims=True))
    rows = f.reshape(-1, s["C"]).astype(np.float64)
    w = rows[rng.integers(0, len(rows), size=s["K"])] + 0.05 * np.abs(rng.normal(size=(s["K"], s["C"])))
    w = to_f16(w * np.where(rng.random((s["K"], s["C"])) < rng.uniform(0.5, 0.95, size=(s["K"], 1)), -1.0, 1.0) * 3)
    if s["nan"]:
        f[NAN_ROW[0]].reshape(-1, s["C"])[NAN_ROW[1]] = np.nan
        f[NAN_IMAGE] = np.nan
    out, at = [], 0
    for j, B in enumerate(s["chunks"]):
        mask = None if s["fold"] is None else fold_mask(j, B, s["W"] * s["H"], s["fold"], "cpu").numpy()
        out.append(([f"img{i:03d}.jpg" for i in range(at, at + B)], np.ascontiguousarray(f[at:at + B]), mask))
        at += B
    return w, out


# ---- the composition: a handful of synthetic images on disk, candidates on them, the device path against the host path ---------------
COMPOSE = dict(sizes=((96, 104), (96, 104), (96, 104), (112, 96), (112, 96), (96, 104), (96, 104)), n_patches=24, top_k=3,
               num_detectors=6, positives=(0, 2, 3), batch=4)


def compose_images(seed):
    """[uint8 [H, W, 3], ...]: noise over a smooth ramp, a different mix per image"""
    rng = np.random.default_rng(seed)
    out = []
    for H, W in COMPOSE["sizes"]:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ramp = np.stack([127 + 100 * np.sin(xx / rng.uniform(4, 20) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(4, 20)) for _ in range(3)], -1)
        noise = rng.normal(0, rng.uniform(5, 40), size=(H, W, 3))
        out.append(np.clip(ramp + noise, 0, 255).astype(np.uint8))
    return out


def compose_patches(seed, names):
    """[(bbox, path), ...]: COMPOSE['n_patches'] positions by `sample_patches` over the images' sizes"""
    from diff_mining_amd.doersch import sample_patches
    sizes = {name: (W, H) for name, (H, W) in zip(names, COMPOSE["sizes"])}
    return sample_patches(sizes, COMPOSE["n_patches"], rng=np.random.default_rng(seed + 1))
