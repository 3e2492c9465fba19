"""The cases of the HOG-LAB features (tests/test_hoglab.py, tests/test_gpu_hoglab*.py, tests/make_golden_hoglab.py): images generated
from `numpy.random.default_rng(seed)`, never stored; host references computed once per process and shared.

    noise    uint8 noise: every orientation bin, every channel wins somewhere
    smooth   sinusoids of another frequency and phase per channel: small gradients, long runs of one bin
    flat     flat regions of one colour (zero gradients: bin 0, nothing added), saturated 0 / 255 patches (the largest gradients) and a
             band with R = G = B (the three channels tie at every pixel: the lowest wins)
    probe    512 x 512: the 16 384 integer gradients (g_row != 0) that lie closest to an orientation-bin edge, each planted as a
             plus-shaped stencil around one point of a 4-pixel grid, the same in all three channels
"""
import numpy as np

from diff_mining_amd import doersch as D

#         H, W, kinds of its images (B = their number)
SHAPES = {
    "A": (64, 64, ("noise",)),                         # one block
    "B": (72, 88, ("noise", "smooth", "flat")),        # 2 x 4 blocks: the transposition shows
    "C": (67, 93, ("flat", "noise")),                  # ragged: pixels past the 8-grid feed gradients
    "D": (200, 136, ("smooth", "noise")),              # 18 block rows x 10 block columns: more blocks per tile than waves
    "E": (512, 512, ("noise", "flat")),                # the real size: 57 block columns = 3 full column tiles and one of 9
}
ORDER = ("A", "B", "C", "D", "E")
SEEDS = {"A": 11, "B": 12, "C": 13, "D": 14, "E": 15}
GOLDEN_CASES = ("B", "C")                              # tests/make_golden_hoglab.py: the first image of each (72 x 88, 67 x 93)
PROBES = 16384


def noise(H, W, rng):
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def smooth(H, W, rng):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((H, W, 3), dtype=np.uint8)
    for ch in range(3):
        fy, fx, ph = rng.uniform(0.02, 0.15), rng.uniform(0.02, 0.15), rng.uniform(0, 2 * np.pi)
        out[..., ch] = np.round(127.5 + 120 * np.sin(fy * y + ph) * np.cos(fx * x - ph)).astype(np.uint8)
    return out


def flat(H, W, rng):
    out = np.empty((H, W, 3), dtype=np.uint8)
    out[...] = rng.integers(0, 256, size=3, dtype=np.uint8)                          # one colour
    for _ in range(6):                                                               # flat rectangles of other colours
        y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
        out[y0:y0 + rng.integers(4, H // 2), x0:x0 + rng.integers(4, W // 2)] = rng.integers(0, 256, size=3, dtype=np.uint8)
    for v in (0, 255, 0, 255):                                                       # saturated patches
        y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
        out[y0:y0 + rng.integers(3, 20), x0:x0 + rng.integers(3, 20)] = v
    y0 = H // 3                                                                      # a grey band of noise: R = G = B
    out[y0:y0 + 12] = rng.integers(0, 256, size=(12, W, 1), dtype=np.uint8)
    return out


KINDS = {"noise": noise, "smooth": smooth, "flat": flat}
_images, _host, _probe = {}, {}, {}


def images(tag):
    """uint8 [B, H, W, 3] of the case"""
    if tag not in _images:
        H, W, kinds = SHAPES[tag]
        rng = np.random.default_rng(SEEDS[tag])
        _images[tag] = np.stack([KINDS[k](H, W, rng) for k in kinds])
        _images[tag].setflags(write=False)
    return _images[tag]


def _reference(imgs, blocks=True):
    """fp64 references of a batch and the tolerances of its fp32 arithmetic: tol = 8 x max |host fp32 - host fp64|"""
    names = ("hog", "lab") + (("raw", "out") if blocks else ())
    ref, dev = {n: [] for n in names}, {n: 0.0 for n in names}
    for im in imgs:
        c64, c32 = D.hoglab_cells_host(im), D.hoglab_cells_host(im, np.float32)
        assert c32[0].dtype == np.float32 and c32[1].dtype == np.float32
        got = {"hog": (c64[0], c32[0]), "lab": (c64[1], c32[1])}
        for name, normalized in ((("raw", False), ("out", True)) if blocks else ()):
            got[name] = (D.hoglab_blocks_host(*c64, normalized=normalized), D.hoglab_blocks_host(*c32, normalized=normalized))
            assert got[name][1].dtype == np.float32
        for name, (a, b) in got.items():
            ref[name].append(a)
            dev[name] = max(dev[name], float(np.abs(a - b.astype(np.float64)).max()))
    out = {name: np.stack(v) for name, v in ref.items()}
    for v in out.values():
        v.setflags(write=False)
    out["tol"] = {name: 8 * d for name, d in dev.items()}
    return out


def host(tag):
    """{"hog" [B, nr, nc, 31], "lab" [B, 2, nr, nc], "raw" / "out" [B, bc, br, 2112]: fp64 host references; "tol": {name: tolN}};
    tag "P": the probe image, cell maps only"""
    if tag not in _host:
        _host[tag] = _reference(probe_image()[None], blocks=False) if tag == "P" else _reference(images(tag))
    return _host[tag]


def edge_distance():
    """float64 [511, 511]: the distance in degrees of the orientation of integer gradient [g_row + 255, g_col + 255] from the nearest
    bin edge (the edges at 0 / 180 included)"""
    g = np.arange(-255, 256, dtype=np.float64)
    o = np.rad2deg(np.arctan2(g[:, None], g[None, :])) % 180
    edges = (180.0 / 31) * np.arange(32)
    return np.abs(o[..., None] - edges).min(axis=-1)


def probe_pairs():
    """int [PROBES, 2]: the (g_row, g_col) with g_row != 0 closest to a bin edge, closest first"""
    d = edge_distance()
    d[255, :] = np.inf                                                               # g_row = 0: bin 0 whatever the arithmetic
    idx = np.argsort(d.reshape(-1), kind="stable")[:PROBES]
    return np.stack([idx // 511 - 255, idx % 511 - 255], axis=1)


def probe_image():
    """uint8 [512, 512, 3]: probe n sits at pixel (4 (n // 128) + 1, 4 (n % 128) + 1); its four neighbours carry the gradient:
    below - above = g_row, right - left = g_col, one of each pair 0.  The stencils do not touch: rows / columns 4 i + 3 stay 0."""
    if "image" not in _probe:
        pairs = probe_pairs()
        im = np.zeros((512, 512, 3), dtype=np.uint8)
        n = np.arange(PROBES)
        y, x = 4 * (n // 128) + 1, 4 * (n % 128) + 1
        gr, gc = pairs[:, 0], pairs[:, 1]
        im[y + 1, x] = np.maximum(gr, 0)[:, None]
        im[y - 1, x] = np.maximum(-gr, 0)[:, None]
        im[y, x + 1] = np.maximum(gc, 0)[:, None]
        im[y, x - 1] = np.maximum(-gc, 0)[:, None]
        im.setflags(write=False)
        _probe["image"] = im
    return _probe["image"]
