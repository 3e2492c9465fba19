"""Mixed-size work lists on the GPU: dm_resize_lanczos against PIL, the batched VAE encode against per-image encodes, and
`compute_worklist` against per-image `compute()` — all bit-equal."""
import os

import numpy as np
import PIL.Image
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_util as U  # noqa: E402
from diff_mining_amd.typicality import TypicalityScorer  # noqa: E402


@pytest.fixture(scope="module")
def engine():
    from diff_mining_amd import synth
    from diff_mining_amd.engine import UNetEngine
    assert torch.cuda.is_available()
    eng = UNetEngine(0)
    eng.load_vae_state_dict(synth.synth_vae_state_dict(seed=0, dtype=np.float16))
    yield eng
    eng.close()


def _rand_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pil_unit(a, w, h):
    return TypicalityScorer.load_image(PIL.Image.fromarray(a).resize((w, h), PIL.Image.LANCZOS))


# target size -> source sizes batched into ONE launch (cars / places rules, landscape, portrait, square, upscaling, odd long
# sides, 1-pixel-thin sources)
GROUPS = [
    ((341, 256), [(1024, 768), (640, 480), (683, 512), (67, 50), (341, 256), (342, 257)]),
    ((256, 341), [(768, 1024), (480, 640), (50, 67)]),
    ((683, 512), [(640, 480), (1024, 768), (2048, 1536)]),
    ((512, 683), [(480, 640), (333, 444)]),
    ((256, 256), [(300, 300), (1000, 1000), (40, 40)]),
    ((9472, 256), [(37, 1)]),
    ((256, 9472), [(1, 37)]),
    ((7, 5), [(3, 2), (1, 1), (100, 37)]),
]


@pytest.mark.parametrize("dst,srcs", GROUPS, ids=[f"{d[0]}x{d[1]}" for d, _ in GROUPS])
def test_resize_lanczos_is_pil(engine, dst, srcs):
    imgs = [_rand_image(w, h, seed=i * 131 + w + h) for i, (w, h) in enumerate(srcs)]
    got = engine.resize_lanczos(imgs, *dst).cpu()
    assert got.shape == (len(imgs), 3, dst[1], dst[0]) and got.dtype == torch.float32
    for b, a in enumerate(imgs):
        assert torch.equal(got[b:b + 1], _pil_unit(a, *dst)), f"image {b} ({a.shape[1]}x{a.shape[0]}) -> {dst}"


def test_resize_lanczos_is_load_image_of_rescale(engine):
    """The tensor the work list encodes is `load_image(rescale(img))` of `compute`, for both rescale rules."""
    for which in ("cars", "places"):
        sc = TypicalityScorer(engine, which=which)
        for w, h in [(500, 375), (375, 500), (401, 299)]:
            a = _rand_image(w, h, seed=w * h)
            tw, th = sc.rescale_size(which, w, h)
            ref = sc.load_image(sc.rescale(PIL.Image.fromarray(a)))
            assert torch.equal(engine.resize_lanczos([a], tw, th).cpu(), ref), (which, w, h)


def test_normalisation_only_covers_every_byte(engine):
    a = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3).astype(np.uint8)
    b = _rand_image(16, 16, seed=3)
    got = engine.resize_lanczos([a, b], 16, 16, resample=False).cpu()
    assert torch.equal(got, torch.cat([TypicalityScorer.load_image(a), TypicalityScorer.load_image(b)]))


def test_batched_vae_encode_is_per_image(engine):
    """`compute_worklist` encodes a call's images of one pixel size in one dm_vae_encode (batched_vae_encode): that is only
    allowed because a batched encode is bit-equal to per-image encodes."""
    assert TypicalityScorer.batched_vae_encode
    sc = TypicalityScorer(engine, which="cars")
    for w, h in [(341, 256), (256, 256)]:
        x = torch.cat([TypicalityScorer.load_image(_rand_image(w, h, seed=s)) for s in range(3)]).to(engine.device)
        nz = U.f16_randn(3, 4, h // 8, w // 8, seed=11)
        batched = sc.encode_vae(x, nz)
        single = torch.cat([sc.encode_vae(x[i:i + 1], nz[i:i + 1]) for i in range(3)])
        assert torch.equal(batched, single), (w, h)


def test_compute_worklist_is_compute(engine, sd15_weights_f16, tmp_path):
    """A shuffled list of 12 images over 4 categories and 4 latent shapes (two pixel widths share one), with fixed
    posterior draws: every `.npy` is bit-equal to the file `compute(country, path)` writes for the image alone."""
    from diff_mining_amd import synth
    if not engine._finalized:
        engine.load_state_dict(sd15_weights_f16)
    _, _, _, c = synth.synth_inputs(1, 1, 8, 8)
    g = torch.Generator().manual_seed(3)
    cats = ["1970", "1985", "2000", "2015"]
    embeds = {k: torch.randn(77, 768, generator=g).half() for k in cats}
    embeds["1970"], embeds[""] = torch.from_numpy(c[0]), torch.from_numpy(c[1])
    sizes = [(60, 45), (67, 50), (45, 60), (90, 45), (60, 45), (67, 50), (40, 40), (90, 45), (67, 50), (45, 60), (60, 45), (64, 48)]
    order = np.random.default_rng(7).permutation(len(sizes))
    work, vnoise = [], {}
    for k, i in enumerate(order):
        w, h = sizes[i]
        cat = cats[k % 4]
        path = str(tmp_path / f"{cat}__car_{k:03d}.jpg")
        im = PIL.Image.fromarray(_rand_image(w, h, seed=50 + k))
        im = im.convert("L") if k == 5 else im
        im.save(path, quality=90)
        work.append(f"{path},{cat}")
        tw, th = TypicalityScorer.rescale_size("cars", w, h)
        vnoise[path] = U.f16_randn(1, 4, th // 8, tw // 8, seed=200 + k)
    a = TypicalityScorer(engine, seed=42, N=2, t_min=0.1, t_max=0.7, typicality_path=str(tmp_path / "list"), which="cars", country_embeds=embeds)
    b = TypicalityScorer(engine, seed=42, N=2, t_min=0.1, t_max=0.7, typicality_path=str(tmp_path / "single"), which="cars", country_embeds=embeds)
    outs = a.compute_worklist(work, images_per_call=3, vae_noise=vnoise)
    shapes = {tuple(np.load(o).shape[-2:]) for o in outs}
    assert len(outs) == 12 and len(set(outs)) == 12 and len(shapes) >= 3
    assert max(len(call) for call in a.last_worklist_calls) == 3
    for line, out in zip(work, outs):
        path, cat = line.split(",")
        assert out == a.get_path(a.typicality_path, path)
        b.compute(cat, path, vae_noise=vnoise[path])
        ga, gb = np.load(out), b(path)
        assert ga.dtype == np.float16 and ga.shape == gb.shape and ga.shape[:3] == (2, 2, 4)
        assert np.array_equal(ga, gb), f"{os.path.basename(path)}: the work list wrote a different grid"
