"""CLIP ViT-B/32 image tower on the fp32 net (dm_f32_clip_*): the device preprocessing against its host restatement
(resample.clip_preprocess_numpy, itself bit-equal to transformers' CLIPImageProcessorPil on the CPU tier), the tower against the
fixture `transformers.CLIPVisionModelWithProjection` produced (tests/golden/clip_vision.npz), normalisation, determinism and batch
independence, the fused patch path and the feature_which dispatch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vision.npz")


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _img(h, w, seed):
    """A smooth image with texture (closer to a photo than uniform noise, so the tower's features are not all alike)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, 3)
    base = 127.5 + 90.0 * np.sin(xx[..., None] / (7.0 + seed % 5) + yy[..., None] / 11.0 + ph)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def net():
    from diff_mining_amd import synth
    from diff_mining_amd.engine import UNetEngineF32
    assert torch.cuda.is_available()
    e = UNetEngineF32(0)
    e.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
    yield e
    e.close()


def _mixed_batch():
    imgs = [_img(512, 512, 0), _img(333, 517, 1), _img(517, 333, 2), _img(224, 300, 3), _img(90, 70, 4)]
    boxes = [[(0, 0, 64, 64), (448, 448, 512, 512), (100, 37, 150, 87), (0, 462, 50, 512)],
             [None, (10, 453, 74, 517), (283, 0, 333, 50)],
             [None],
             [None, (0, 0, 224, 300)],
             [(0, 0, 90, 70), (40, 20, 90, 70)]]
    return imgs, boxes


def test_preprocess_bit_equal_to_host(net):
    from diff_mining_amd import resample as RS
    imgs, boxes = _mixed_batch()
    pv = net.clip_preprocess(imgs, boxes).cpu()
    ref = [torch.from_numpy(RS.clip_preprocess_numpy(im, b)) for im, bl in zip(imgs, boxes) for b in bl]
    assert pv.shape == (len(ref), 3, 224, 224) and pv.dtype == torch.float32
    for i, r in enumerate(ref):
        assert torch.equal(pv[i], r), f"patch {i}: max |diff| {(pv[i] - r).abs().max().item()}"
    # whole images without a box list, and PIL input
    import PIL.Image
    pv2 = net.clip_preprocess([PIL.Image.fromarray(imgs[1]), imgs[2]]).cpu()
    assert torch.equal(pv2[0], ref[4]) and torch.equal(pv2[1], ref[7])


def test_preprocess_rejects_bad_input(net):
    img = _img(100, 120, 0)
    for box in [(0, 0, 0, 10), (0, 0, 101, 10), (-1, 0, 10, 10), (0, 110, 10, 121)]:
        with pytest.raises(ValueError):
            net.clip_preprocess([img], [[box]])
    with pytest.raises(ValueError):
        net.clip_preprocess([img.astype(np.float32)], [[(0, 0, 10, 10)]])
    with pytest.raises(ValueError):
        net.clip_preprocess([np.zeros((10, 10, 4), np.uint8)], [[(0, 0, 10, 10)]])


def test_tower_matches_transformers_fixture(net):
    from diff_mining_amd import synth
    g = np.load(GOLDEN)
    pv = torch.from_numpy(synth.synth_clip_pixel_values(3))
    emb = net.clip_image_features(pv, normalize=False)
    hid = net.clip_vision_hidden(pv)
    assert emb.shape == (3, 512) and hid.shape == (3, 50, 768) and emb.dtype == hid.dtype == torch.float32
    r_emb = _rel(emb, torch.from_numpy(g["image_embeds"]))
    r_hid = _rel(hid, torch.from_numpy(g["last_hidden_state"]))
    print(f"\nclip vision vs transformers {g['transformers_version']}: image_embeds rel-L2 {r_emb:.2e}, last_hidden_state rel-L2 {r_hid:.2e}")
    assert r_emb <= 1e-5 and r_hid <= 1e-5, (r_emb, r_hid)


def test_normalized_output(net):
    imgs, boxes = _mixed_batch()
    pv = net.clip_preprocess(imgs, boxes)
    raw = net.clip_image_features(pv, normalize=False).double()
    nrm = net.clip_image_features(pv, normalize=True).double()
    assert (nrm.norm(dim=1) - 1).abs().max().item() <= 1e-6
    ref = raw / raw.norm(dim=1, keepdim=True)
    assert ((nrm - ref).norm(dim=1) / ref.norm(dim=1)).max().item() <= 1e-6
    # distinct patches give distinct features (patches 8 and 9 are the same 224 x 300 image, whole and as a full box)
    cos = nrm @ nrm.T
    assert torch.equal(nrm[8], nrm[9])
    cos[8, 9] = cos[9, 8] = 0
    assert (cos - torch.eye(len(nrm), dtype=cos.dtype, device=cos.device)).abs().max().item() < 0.9999


def test_determinism_and_batch_independence(net):
    imgs = [_img(256, 256, s) for s in range(37)]
    boxes = [[(s % 190, (3 * s) % 190, s % 190 + 64, (3 * s) % 190 + 64)] for s in range(37)]
    pv = net.clip_preprocess(imgs, boxes)
    full = net.clip_image_features(pv)
    again = net.clip_image_features(pv)
    assert torch.equal(full, again)
    alone = net.clip_image_features(pv[11:12])
    assert torch.equal(alone[0], full[11])
    perm = torch.randperm(37, generator=torch.Generator().manual_seed(3))
    permuted = net.clip_image_features(pv[perm.to(pv.device)])
    assert torch.equal(permuted, full[perm.to(full.device)])


def test_large_call_is_chunked_bit_exactly(net):
    imgs = [_img(200, 200, s) for s in range(13)]
    boxes = [[(r, c, r + 50, c + 50) for r, c in ((0, 0), (150, 150), (20, 90), (75, 10), (100, 100))] * 8 for _ in range(13)]
    pv = net.clip_preprocess(imgs, boxes)
    assert pv.shape[0] == 520                          # more than the 512-image runs of one call
    big = net.clip_image_features(pv)
    small = torch.cat([net.clip_image_features(pv[i:i + 100]) for i in range(0, 520, 100)])
    assert torch.equal(big, small)


def test_fused_patch_features_equal_two_step(net):
    imgs, boxes = _mixed_batch()
    fused = net.clip_patch_features(imgs, boxes)
    two = net.clip_image_features(net.clip_preprocess(imgs, boxes))
    assert fused.shape == (sum(len(b) for b in boxes), 512)
    assert torch.equal(fused, two)
    assert torch.equal(net.clip_patch_features(imgs, boxes, normalize=False), net.clip_image_features(net.clip_preprocess(imgs, boxes), normalize=False))


def test_feature_which_dispatch(net):
    from diff_mining_amd import dift
    from diff_mining_amd.engine import UNetEngine
    aux = UNetEngine(0)                                # the DIFT patch kernel only: no weights needed
    try:
        fz = dift.SDFeaturizer(net, aux=aux)
        img = _img(256, 320, 9)
        boxes = [(0, 0, 64, 64), (192, 256, 256, 320), (100, 40, 164, 104)]
        feat = torch.from_numpy(np.random.default_rng(0).normal(size=(1, 1280, 16, 20)).astype(np.float32)).to(net.device)
        a = dift.patch_features("clip", img, boxes, clip_net=net)
        b = dift.patch_features("dift-261", img, boxes, featurizer=fz, feat=feat)
        ab = dift.patch_features("clip+dift-261", img, boxes, featurizer=fz, clip_net=net, feat=feat)
        assert a.shape == (3, 512) and b.shape == (3, 1280) and ab.shape == (3, 1792)
        assert torch.equal(ab, torch.cat([a, b], 1))
        assert torch.equal(a, net.clip_patch_features([img], [boxes]))
        with pytest.raises(ValueError):
            dift.patch_features("clip", img, boxes)
    finally:
        aux.close()


def test_errors_without_weights():
    from diff_mining_amd import synth
    from diff_mining_amd.engine import EngineError, UNetEngineF32
    e = UNetEngineF32(0)
    try:
        pv = torch.zeros(1, 3, 224, 224, device=e.device)
        with pytest.raises(EngineError):
            e.clip_image_features(pv)
        with pytest.raises(EngineError):
            e.clip_patch_features([_img(64, 64, 0)], [None])
        sd = synth.synth_clip_vision_state_dict(0)
        del sd["vision_model.encoder.layers.5.self_attn.q_proj.bias"]
        with pytest.raises(EngineError):
            e.load_clip_vision_state_dict(sd)
        sd = synth.synth_clip_vision_state_dict(0)
        sd["visual_projection.weight"] = sd["visual_projection.weight"][:256]
        with pytest.raises(EngineError):
            e.load_clip_vision_state_dict(sd)
        with pytest.raises(EngineError):
            e.clip_image_features(pv)
    finally:
        e.close()
