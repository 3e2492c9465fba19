"""CPU tier of the mixed-size work-list path: PIL's LANCZOS coefficient tables restated on the host (resample.lanczos_axis),
the packed descriptors of one batched dm_resize_lanczos launch (resample.resize_plan), and `compute_worklist`'s shape
buckets and flush plan over a fake engine."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

from diff_mining_amd import resample as RS
from diff_mining_amd.typicality import TypicalityScorer

# (source w, h) -> target (w, h): the cars / places rules on landscape, portrait and square images, upscaling, long sides that
# are not multiples of 8, 1-pixel-thin images and a few free-form pairs
PAIRS = []
for _src in [(1024, 768), (640, 480), (480, 640), (333, 500), (300, 300), (67, 50), (50, 67), (2000, 257), (256, 341), (1, 37), (37, 1)]:
    for _which in ("cars", "places"):
        PAIRS.append((_src, TypicalityScorer.rescale_size(_which, *_src)))
PAIRS += [((3, 2), (7, 5)), ((100, 37), (100, 256)), ((100, 37), (33, 37)), ((1, 1), (5, 3)), ((9, 9), (1, 1)), ((513, 257), (341, 256))]
PAIRS = [p for p in PAIRS if p[1][0] * p[1][1] <= 300_000]        # keeps the host restatement fast


def _rand_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pil(a, w, h):
    return np.asarray(PIL.Image.fromarray(a).resize((w, h), PIL.Image.LANCZOS))


@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in PAIRS])
def test_host_tables_are_pils(src, dst):
    a = _rand_image(*src, seed=src[0] * 7 + src[1])
    assert np.array_equal(RS.resize_numpy(a, *dst), _pil(a, *dst))


def test_host_tables_random_pairs():
    rng = np.random.default_rng(5)
    for _ in range(40):
        w, h = int(rng.integers(1, 600)), int(rng.integers(1, 600))
        ow, oh = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        a = _rand_image(w, h, seed=w * 1000 + h)
        assert np.array_equal(RS.resize_numpy(a, ow, oh), _pil(a, ow, oh)), (w, h, ow, oh)


def test_identity_axis_is_a_copy():
    b, k = RS.lanczos_axis(37, 37)
    assert k.shape == (37, 1) and (k == 1 << RS.PRECISION_BITS).all() and (b[:, 0] == np.arange(37)).all()
    a = _rand_image(37, 20, seed=1)
    assert np.array_equal(RS.resize_numpy(a, 37, 20), a)


def _emulate_launch(src, desc, tables, n, out_w, out_h, tmp_rows_max):
    """resize_h_kernel + resize_v_kernel (csrc/resize.hip) in numpy, reading only the packed buffers a launch gets."""
    out = np.empty((n, 3, out_h, out_w), dtype=np.float32)
    half = 1 << (RS.PRECISION_BITS - 1)
    for b in range(n):
        d = desc[b]
        w, h, y0, rows = int(d["src_w"]), int(d["src_h"]), int(d["ybox_first"]), int(d["tmp_rows"])
        assert rows <= tmp_rows_max
        img = src[int(d["src_offset"]):int(d["src_offset"]) + w * h * 3].reshape(h, w, 3).astype(np.int64)
        tmp = np.empty((rows, out_w, 3), dtype=np.int64)
        for x in range(out_w):
            s, m = tables[d["xb_off"] + 2 * x], tables[d["xb_off"] + 2 * x + 1]
            k = tables[d["xk_off"] + x * d["kx"]:][:m].astype(np.int64)
            tmp[:, x] = np.clip((half + (img[y0:y0 + rows, s:s + m] * k[None, :, None]).sum(1)) >> RS.PRECISION_BITS, 0, 255)
        for y in range(out_h):
            s, m = tables[d["yb_off"] + 2 * y], tables[d["yb_off"] + 2 * y + 1]
            k = tables[d["yk_off"] + y * d["ky"]:][:m].astype(np.int64)
            v = np.clip((half + (tmp[s:s + m] * k[:, None, None]).sum(0)) >> RS.PRECISION_BITS, 0, 255)
            out[b, :, y] = torch.from_numpy(v.astype(np.uint8).T.copy()).float().numpy() / 255.0 * 2 - 1
    return out


def test_batched_plan_mixed_sources():
    """One launch, one target size, four source sizes: the descriptors and shared tables give PIL + load_image per image."""
    out_w, out_h = 341, 256
    imgs = [_rand_image(w, h, seed=i) for i, (w, h) in enumerate([(1024, 768), (683, 512), (343, 257), (341, 256)])]
    desc, tables, tmp_rows = RS.resize_plan([(a.shape[1], a.shape[0]) for a in imgs], out_w, out_h)
    assert desc.dtype.itemsize == 48 and tables.dtype == np.int32
    src = np.concatenate([a.reshape(-1) for a in imgs])
    got = _emulate_launch(src, desc, tables, len(imgs), out_w, out_h, tmp_rows)
    for b, a in enumerate(imgs):
        ref = TypicalityScorer.load_image(PIL.Image.fromarray(a).resize((out_w, out_h), PIL.Image.LANCZOS))
        assert np.array_equal(got[b], ref[0].numpy()), b


def test_decode_threads(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert TypicalityScorer.decode_threads() == 3
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert TypicalityScorer.decode_threads() == 4


def test_worklist_plan():
    shapes = [(32, 42), (32, 40), (32, 42), (64, 32), (32, 42), (32, 40), (32, 42)]
    plan = TypicalityScorer.worklist_plan(shapes, images_per_call=2)
    assert plan == [[0, 2], [4, 6], [1, 5], [3]]


class _FakeEngine:
    """The three engine calls `compute_worklist` makes, on the host: the resize is the numpy restatement + `to_tensor * 2 - 1`,
    the VAE "encode" records its pixels and returns a latent of the right shape."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.resize_launches, self.encoded = [], []

    def resize_lanczos(self, images, out_w, out_h, resample=True):
        self.resize_launches.append((len(images), out_w, out_h, resample))
        outs = [RS.resize_numpy(a, out_w, out_h) if resample else a for a in images]
        return torch.stack([torch.from_numpy(o.copy()).permute(2, 0, 1).float() / 255.0 * 2 - 1 for o in outs])

    def vae_encode(self, image, noise=None, scaling_factor=0.18215, out_dtype=None):
        B, _, H, W = image.shape
        self.encoded.append(image.clone())
        return image.mean(1, keepdim=True)[:, :, : H // 8 * 8 : 8, : W // 8 * 8 : 8].repeat(1, 4, 1, 1).to(out_dtype)


def _write_list(tmp_path, specs):
    lines = []
    for i, (cat, (w, h), mode) in enumerate(specs):
        a = _rand_image(w, h, seed=100 + i)
        im = PIL.Image.fromarray(a)
        if mode == "L":
            im = im.convert("L")
        elif mode == "RGBA":
            im = PIL.Image.fromarray(np.dstack([a, a[:, :, :1]]), "RGBA")
        path = str(tmp_path / f"{cat}__img_{i:03d}.png")
        im.save(path)
        lines.append(f"{path},{cat}")
    return lines


@pytest.mark.parametrize("images_per_call", [1, 2, 3, 8])
def test_compute_worklist_buckets_with_a_fake_engine(tmp_path, images_per_call):
    # cars: 60 x 45 -> 341 x 256 and 67 x 50 -> 343 x 256 share latent 32 x 42, so a call holds two pixel sizes; 45 x 60 is the
    # portrait twin, 90 x 45 -> 512 x 256, 40 x 40 -> 256 x 256
    sizes = [(60, 45), (67, 50), (45, 60), (90, 45), (60, 45), (67, 50), (40, 40), (90, 45), (67, 50), (45, 60), (60, 45), (64, 48)]
    cats = ["1970", "1985", "2000", "2015"]
    modes = ["RGB"] * 12
    modes[3], modes[7] = "L", "RGBA"
    specs = [(cats[i % 4], sizes[i], modes[i]) for i in range(12)]
    lines = _write_list(tmp_path, specs)
    eng = _FakeEngine()
    g = torch.Generator().manual_seed(0)
    embeds = {c: torch.randn(77, 768, generator=g).half() for c in cats + [""]}
    sc = TypicalityScorer(eng, seed=42, N=2, typicality_path=str(tmp_path / "typ"), which="cars", country_embeds=embeds)
    calls = []

    def fake_batch(xs, emb, *a, **k):
        calls.append((tuple(xs.shape), tuple(emb.shape)))
        n, _, h, w = xs.shape
        return torch.zeros(n, sc.N, 2, 4, h, w, dtype=torch.float16)
    sc.compute_losses_batch = fake_batch
    outs = sc.compute_worklist(lines, images_per_call=images_per_call)
    # every line written exactly once, returned in list order
    assert len(outs) == len(lines) and len(set(outs)) == len(lines)
    for line, out in zip(lines, outs):
        assert out == sc.get_path(sc.typicality_path, line.split(",")[0]) and os.path.isfile(out)
    assert sorted(i for c in sc.last_worklist_calls for i in c) == list(range(len(lines)))
    # calls hold at most images_per_call images of one latent shape, as many calls as the buckets need
    latents = [(TypicalityScorer.rescale_size("cars", w, h)[1] // 8, TypicalityScorer.rescale_size("cars", w, h)[0] // 8) for w, h in sizes]
    buckets = {}
    for s in latents:
        buckets[s] = buckets.get(s, 0) + 1
    assert len(calls) == sum(-(-n // images_per_call) for n in buckets.values())
    for c, (xs_shape, emb_shape) in zip(sc.last_worklist_calls, calls):
        assert 1 <= len(c) <= images_per_call and xs_shape[0] == len(c) and emb_shape[:2] == (len(c), 2)
        assert len({latents[i] for i in c}) == 1 and xs_shape[2:] == latents[c[0]]
    # every encoded pixel tensor is load_image(rescale(img)), whichever path (device resize or the RGBA host path) made it
    pix = [e[k] for e in eng.encoded for k in range(e.shape[0])]
    assert len(pix) == len(lines)
    order = []
    for call in sc.last_worklist_calls:          # per call, images grouped by pixel size in first-appearance order
        by = {}
        for i in call:
            by.setdefault(TypicalityScorer.rescale_size("cars", *sizes[i]), []).append(i)
        for js in by.values():
            order += js
    for i, p in zip(order, pix):
        ref = sc.load_image(sc.rescale(PIL.Image.open(lines[i].split(",")[0])))[0]
        assert torch.equal(p, ref), i
    assert all(r[3] for r in eng.resize_launches)      # cars: every launch resamples
    assert sum(r[0] for r in eng.resize_launches) == len(lines) - 1   # the RGBA image took the host path


def test_compute_worklist_without_rescale_rule_only_normalises(tmp_path):
    lines = _write_list(tmp_path, [("a", (16, 24), "RGB"), ("b", (24, 16), "RGB"), ("a", (16, 24), "L")])
    eng = _FakeEngine()
    embeds = {c: torch.zeros(77, 768).half() for c in ("a", "b", "")}
    sc = TypicalityScorer(eng, seed=42, N=1, typicality_path=str(tmp_path / "typ"), which="geo", country_embeds=embeds)
    sc.compute_losses_batch = lambda xs, emb, *a, **k: torch.zeros(xs.shape[0], 1, 2, 4, *xs.shape[2:], dtype=torch.float16)
    outs = sc.compute_worklist(lines)
    assert len(set(outs)) == 3
    assert sorted((n, w, h, r) for n, w, h, r in eng.resize_launches) == [(1, 24, 16, False), (2, 16, 24, False)]
    assert sc.last_worklist_calls == [[0, 2], [1]]
