"""The CLIP baseline from pixels on the fp32 net (clipmining/ranking.py:58-70): the head_dim-64 route of the fp32 flash attention, the
tower's device preprocessing against its host restatement (itself bit-equal to transformers' processor on the CPU tier), the
configurable image tower and the text embeddings against the fixture `transformers` produced (tests/golden/clip_tower.npz), determinism,
chunking, the fused path, `clipmine.rank_images`, the error paths, and the ViT-B/32 tower's bits after the new tower is loaded.

Every tower test runs the TEST config (336 px, patch 14, 577 tokens, heads of 64; hidden 128, 3 layers): the shape properties of
ViT-L/14-336 at 1/200 of its weights.  The 304 M-parameter size is tools/clip_tower_rate.py's."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import clip_spec as S  # noqa: E402
from diff_mining_amd import clipmine  # noqa: E402
from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import resample as RS  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from tests import gpu_util as U  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_CFG = S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=336, patch_size=14,
                              projection_dim=64)
# the ranking test's variant: 56 px -> a 4 x 4 grid, 17 tokens (less than one key tile); its projection is as wide as the text embeddings
CFG56 = S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=56, patch_size=14,
                           projection_dim=768)
TOL_OP = 2e-6          # tests/test_gpu_f32.py: the fp32 attention against float64 at head_dim 40 / 80 / 160
TOL_TOWER = 1e-5       # tests/test_gpu_clip_vision.py: the 12-layer ViT-B/32 tower against its transformers fixture


def _img(side, seed):
    """A smooth square image with texture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    ph = rng.uniform(0, 6.28, 3)
    base = 127.5 + 90.0 * np.sin(xx[..., None] / (7.0 + seed % 5) + yy[..., None] / 11.0 + ph)
    return np.clip(base + rng.normal(0, 25, (side, side, 3)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def text_sd():
    sd = {"text_model." + k: v for k, v in synth.synth_clip_state_dict(seed=0).items()}
    sd["text_projection.weight"] = synth.synth_clip_text_projection(0)
    return sd


@pytest.fixture(scope="module")
def b32():
    """A net with the ViT-B/32 tower and its features of one fixture image BEFORE anything else is loaded into it."""
    assert torch.cuda.is_available()
    e = E.UNetEngineF32(0)
    e.load_clip_vision_state_dict(synth.synth_clip_vision_state_dict(0))
    pv = torch.from_numpy(synth.synth_clip_pixel_values(3)[1:2])
    before = (e.clip_image_features(pv, normalize=False).clone(), e.clip_vision_hidden(pv).clone())
    yield e, pv, before
    e.close()


@pytest.fixture(scope="module")
def net(b32, text_sd):
    """The same net with the test tower and the text tower (with its projection) beside the ViT-B/32 one."""
    e = b32[0]
    e.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, TEST_CFG), TEST_CFG)
    e.load_clip_state_dict(text_sd)
    return e


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "clip_tower.npz"))


@pytest.fixture(scope="module")
def pixels():
    return torch.from_numpy(synth.synth_clip_pixel_values(2, size=336))


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _attention64(q, k, v, heads):
    B, Tq, Cc = q.shape
    D = Cc // heads
    out = torch.empty(B, Tq, Cc, dtype=torch.float64)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            qh, kh, vh = q[b, :, sl].double(), k[b, :, sl].double(), v[b, :, sl].double()
            out[b, :, sl] = torch.softmax(qh @ kh.T * D ** -0.5, dim=-1) @ vh
    return out


@pytest.mark.parametrize("T", [577, 17])
def test_attention32_head_dim_64(T):
    """dm_f32_op_attention at D = 64 on the tower's stacked q|k|v rows (ld = 3 hidden, scale 1/8): 577 = 9 * 64 + 1 — the last key tile
    holds one real key, the last query block 65 of 128 queries; 17 (a 56-px image) is less than one key tile."""
    lib = E.load_library()
    B, heads, D = 2, 2, 64
    Cc = heads * D
    qkv = torch.randn(B, T, 3 * Cc, generator=torch.Generator().manual_seed(T))
    ref = _attention64(qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:], heads)
    X = qkv.cuda()
    O = torch.full((B, T, Cc), float("nan"), device=X.device)
    base = X.data_ptr()
    rc = lib.dm_f32_op_attention(U.stream(), E.C.c_void_p(base), E.C.c_void_p(base + 4 * Cc), E.C.c_void_p(base + 8 * Cc), U.ptr(O),
                                 3 * Cc, 3 * Cc, 3 * Cc, Cc, T * 3 * Cc, T * 3 * Cc, T * 3 * Cc, T * Cc, None, 0, B, heads, T, T, D, 0.125)
    assert rc == 0, "dm_f32_op_attention refuses head_dim 64"
    torch.cuda.synchronize()
    assert torch.isfinite(O).all()
    r = U.rel_l2(O.cpu(), ref)
    print(f"\nattention32 B{B} heads{heads} T{T} D64 on q|k|v rows: rel-L2 vs float64 {r:.2e}")
    assert r < TOL_OP


# ---- preprocessing --------------------------------------------------------------------------------------------------------------
def test_tower_preprocess_bit_equal_to_host(net):
    sides = (512, 336, 337, 200, 512)                    # a downscale, both passes skipped, a one-pixel downscale, an upscale
    imgs = [_img(s, i) for i, s in enumerate(sides)]
    pv = net.clip_tower_preprocess(imgs).cpu()
    assert pv.shape == (5, 3, 336, 336) and pv.dtype == torch.float32
    for i, im in enumerate(imgs):
        ref = torch.from_numpy(RS.clip_tower_preprocess_numpy(im, 336))
        assert torch.equal(pv[i], ref), f"image {i} ({sides[i]} px): max |diff| {(pv[i] - ref).abs().max().item()}"
    import PIL.Image
    assert torch.equal(net.clip_tower_preprocess([PIL.Image.fromarray(imgs[3])]).cpu()[0], pv[3])
    for bad in ([np.zeros((336, 300, 3), np.uint8)], [np.zeros((336, 336, 3), np.float32)], []):
        with pytest.raises(ValueError):
            net.clip_tower_preprocess(bad)
    with pytest.raises(TypeError):
        net.clip_tower_preprocess(imgs[0])


# ---- towers against transformers --------------------------------------------------------------------------------------------------
def test_tower_matches_transformers_fixture(net, golden, pixels):
    tok, hid = net.clip_patch_tokens(pixels, return_hidden=True)
    assert tok.shape == (2, 576, 64) and hid.shape == (2, 577, 128) and tok.dtype == hid.dtype == torch.float32
    r_hid = U.rel_l2(hid[0], torch.from_numpy(golden["last_hidden_state"]))
    r_tok = U.rel_l2(tok, torch.from_numpy(golden["tokens"]))
    print(f"\nclip tower vs transformers {golden['transformers_version']}: last_hidden_state rel-L2 {r_hid:.2e}, tokens rel-L2 {r_tok:.2e} "
          f"(the reference's own fp32-vs-float64: {float(golden['floor_hidden']):.2e}, {float(golden['floor_tokens']):.2e})")
    assert r_hid <= TOL_TOWER and r_tok <= TOL_TOWER, (r_hid, r_tok)
    assert torch.equal(net.clip_patch_tokens(pixels), tok)


def test_text_embeds_match_transformers_fixture(net, golden):
    ids = synth.synth_token_ids(3)
    raw = net.clip_text_embeds(ids, normalize=False)
    assert raw.shape == (3, 768) and raw.dtype == torch.float32
    r = U.rel_l2(raw, torch.from_numpy(golden["text_embeds"]))
    print(f"\nclip text_embeds vs transformers {golden['transformers_version']}: rel-L2 {r:.2e}")
    assert r <= TOL_TOWER
    nrm = net.clip_text_embeds(ids).double()
    assert (nrm.norm(dim=1) - 1).abs().max().item() <= 1e-6
    ref = raw.double() / raw.double().norm(dim=1, keepdim=True)
    assert ((nrm - ref).norm(dim=1) / ref.norm(dim=1)).max().item() <= 1e-6
    # the pooled row is the EOS row of the hidden states the existing entry returns
    hidden = net.clip_encode(ids)
    pos = torch.from_numpy(np.argmax(ids, axis=1)).to(hidden.device)
    pooled = hidden[torch.arange(3, device=hidden.device), pos]
    w = torch.from_numpy(synth.synth_clip_text_projection(0)).to(hidden.device)
    assert U.rel_l2(raw, pooled.double() @ w.double().T) <= TOL_OP
    with pytest.raises(ValueError):
        net.clip_text_embeds(ids[:, :50])


def test_text_embeds_need_the_projection():
    e = E.UNetEngineF32(0)
    try:
        ids = synth.synth_token_ids(2)
        with pytest.raises(E.EngineError):
            e.clip_text_embeds(ids)                      # no text weights at all
        e.load_clip_state_dict(synth.synth_clip_state_dict(seed=0))          # the 196 tensors of CLIPTextModel: as before
        assert e.clip_encode(ids).shape == (2, 77, 768)
        with pytest.raises(E.EngineError, match="text_projection"):
            e.clip_text_embeds(ids)
    finally:
        e.close()


# ---- determinism, chunking, the fused path ------------------------------------------------------------------------------------------
def test_determinism_and_batch_independence(net):
    imgs = [_img(336, s) for s in range(5)]
    pv = net.clip_tower_preprocess(imgs)
    full = net.clip_patch_tokens(pv)
    assert torch.equal(net.clip_patch_tokens(pv), full)
    assert torch.equal(net.clip_patch_tokens(pv[3:4])[0], full[3])
    perm = torch.tensor([4, 2, 0, 3, 1], device=pv.device)
    assert torch.equal(net.clip_patch_tokens(pv[perm]), full[perm])
    assert (full[0] - full[1]).abs().max().item() > 1e-3          # different images, different tokens


def test_large_call_is_chunked_bit_exactly(net):
    n = E.CLIP_TOWER_CHUNK + 1
    base = net.clip_tower_preprocess([_img(336, s) for s in range(3)])
    pv = base[torch.arange(n, device=base.device) % 3].contiguous()
    pv[-1] = base[1].flip(-1)                              # the image behind the chunk boundary is none of the others
    big, big_h = net.clip_patch_tokens(pv, return_hidden=True)
    small = [net.clip_patch_tokens(pv[i:i + 24], return_hidden=True) for i in range(0, n, 24)]
    assert torch.equal(big, torch.cat([t for t, _ in small])) and torch.equal(big_h, torch.cat([h for _, h in small]))
    assert torch.equal(big[3], big[0]) and not torch.equal(big[-1], big[1])


def test_fused_image_tokens_equal_two_step(net):
    imgs = [_img(s, i) for i, s in enumerate((512, 336, 200, 337))]
    fused = net.clip_image_tokens(imgs)
    two = net.clip_patch_tokens(net.clip_tower_preprocess(imgs))
    assert fused.shape == (4, 576, 64)
    assert torch.equal(fused, two)


def test_patch_ln_equals_layernorm_of_the_patch_rows():
    """The patch-token head's LayerNorm (rows 1..T-1 of every image, CLS skipped) against the plain LayerNorm kernel on the gathered
    rows — the same arithmetic in the same order — and against float64."""
    lib = E.load_library()
    n, T, Cc = 3, 17, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, T, Cc, generator=g) * 2 + 0.3
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    X, G, Bt = x.cuda(), gamma.cuda(), beta.cuda()
    Y = torch.full((n * (T - 1), Cc), float("nan"), device=X.device)
    assert lib.dm_f32_op_clip_patch_ln(U.stream(), U.ptr(X), n, T, Cc, U.ptr(G), U.ptr(Bt), 1e-5, U.ptr(Y)) == 0
    rows = X[:, 1:, :].reshape(-1, Cc).contiguous()
    Y2 = torch.empty_like(Y)
    assert lib.dm_f32_op_layernorm(U.stream(), U.ptr(rows), rows.shape[0], Cc, U.ptr(G), U.ptr(Bt), 1e-5, U.ptr(Y2)) == 0
    torch.cuda.synchronize()
    assert torch.equal(Y, Y2)
    ref = torch.nn.functional.layer_norm(x[:, 1:, :].double().reshape(-1, Cc), (Cc,), gamma.double(), beta.double(), 1e-5)
    assert U.rel_l2(Y, ref) < TOL_OP


# ---- ranking from pixels ----------------------------------------------------------------------------------------------------------------
def test_rank_images_composes_the_device_path(text_sd):
    e = E.UNetEngineF32(0)
    try:
        e.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, CFG56), CFG56)
        e.load_clip_state_dict(text_sd)
        imgs = [_img(112, s) for s in range(3)]
        ids = synth.synth_token_ids(2)
        rows, feats = clipmine.rank_images(e, imgs, ids, k_per_image=5, kx=16, ky=16)
        tokens = e.clip_image_tokens(imgs)
        text = e.clip_text_embeds(ids)
        assert tokens.shape == (3, 16, 768) and text.shape == (2, 768)
        boxes, d, count, f = clipmine.rank_device(list(tokens), text, [(112, 112)] * 3, 4, 5, 16, 16, "diff")
        count = count.cpu().numpy()
        assert (count > 0).all()
        keep = np.arange(5)[None, :] < count[:, None]
        assert np.array_equal(rows["image"], np.repeat(np.arange(3), count))
        bx = boxes.cpu().numpy()[keep]
        for c, name in enumerate(("x_start", "y_start", "x_end", "y_end")):
            assert np.array_equal(rows[name], bx[:, c])
        assert np.array_equal(rows["D"], d.cpu().numpy()[keep])
        assert torch.equal(feats, f[torch.from_numpy(keep).to(f.device)])
        # one image per call: the same rows
        rows1, feats1 = clipmine.rank_images(e, imgs, ids, k_per_image=5, kx=16, ky=16, images_per_call=1)
        assert all(np.array_equal(rows[k], rows1[k]) for k in rows) and torch.equal(feats, feats1)
        with pytest.raises(ValueError):
            clipmine.rank_images(e, [np.zeros((112, 100, 3), np.uint8)], ids, kx=16, ky=16)
        with pytest.raises(ValueError):
            clipmine.rank_images(e, imgs, synth.synth_token_ids(3), kx=16, ky=16)
    finally:
        e.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    e = E.UNetEngineF32(0)
    try:
        with pytest.raises(E.EngineError):
            e.clip_patch_tokens(torch.zeros(1, 3, 336, 336))                 # before the weights are loaded
        with pytest.raises(E.EngineError):
            e.clip_image_tokens([_img(336, 0)])
        with pytest.raises(E.EngineError):
            e.clip_tower_preprocess([_img(336, 0)])
        lib, dummy = E.load_library(), torch.zeros(64, device="cuda")
        assert lib.dm_f32_clip_tower_tokens(e._h, U.ptr(dummy), 1, U.ptr(dummy), None, U.stream()) != 0          # the C entry itself refuses
        sd = synth.synth_clip_vision_state_dict(0, TEST_CFG)
        bad = dict(sd)
        del bad["vision_model.encoder.layers.1.self_attn.q_proj.bias"]
        with pytest.raises(E.EngineError, match="q_proj.bias"):
            e.load_clip_tower_state_dict(bad, TEST_CFG)
        bad = dict(sd)
        bad["visual_projection.weight"] = bad["visual_projection.weight"][:32]
        with pytest.raises(E.EngineError, match="visual_projection"):
            e.load_clip_tower_state_dict(bad, TEST_CFG)
        with pytest.raises(E.EngineError):
            e.load_clip_tower_state_dict(sd)                                 # the L/14-336 config against the test tensors
        # configs the tower refuses: heads of 32, an intermediate size off the GEMM's k step, a projection of 66
        for cfg in (S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4, image_size=336,
                                       patch_size=14, projection_dim=64),
                    S.CLIPVisionConfig(hidden_size=128, intermediate_size=520, num_hidden_layers=3, num_attention_heads=2, image_size=336,
                                       patch_size=14, projection_dim=64),
                    S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=336,
                                       patch_size=14, projection_dim=66)):
            with pytest.raises(E.EngineError):
                e.load_clip_tower_state_dict(synth.synth_clip_vision_state_dict(0, cfg), cfg)
        # the C finalize checks the config itself
        c = (E.C.c_int32 * 7)(128, 512, 3, 4, 336, 14, 64)
        assert lib.dm_f32_finalize_clip_tower(e._h, E.C.cast(c, E.C.c_void_p)) != 0
        assert b"heads" in lib.dm_f32_last_error(e._h)
        # ... and every tensor against it (the Python loader's own check bypassed): a missing tensor, then a misshapen one
        good = (E.C.c_int32 * 7)(128, 512, 3, 2, 336, 14, 64)
        bad = dict(sd)
        del bad["vision_model.post_layernorm.bias"]
        with pytest.raises(E.EngineError, match="post_layernorm.bias"):
            e._load("_clip_tower", bad, E.C.cast(good, E.C.c_void_p))
        bad = dict(sd)
        bad["vision_model.embeddings.patch_embedding.weight"] = np.zeros((128, 3, 16, 16), np.float32)
        with pytest.raises(E.EngineError, match="patch_embedding"):
            e._load("_clip_tower", bad, E.C.cast(good, E.C.c_void_p))
        with pytest.raises(E.EngineError):
            e.clip_patch_tokens(torch.zeros(1, 3, 336, 336))                 # still nothing loaded
        e.load_clip_tower_state_dict(sd, TEST_CFG)
        for shape in ((1, 3, 224, 224), (1, 3, 336, 335), (3, 336, 336), (0, 3, 336, 336)):
            with pytest.raises(ValueError):
                e.clip_patch_tokens(torch.zeros(*shape))
        assert e.clip_patch_tokens(torch.zeros(1, 3, 336, 336)).shape == (1, 576, 64)
    finally:
        e.close()


# ---- the ViT-B/32 tower's bits --------------------------------------------------------------------------------------------------------------
def test_b32_tower_untouched(b32, net):
    e, pv, (emb0, hid0) = b32
    assert e is net and getattr(e, "_clip_tower_cfg", None) is TEST_CFG
    e.clip_patch_tokens(torch.from_numpy(synth.synth_clip_pixel_values(1, size=336)))            # the new tower has run in this net
    assert torch.equal(e.clip_image_features(pv, normalize=False), emb0)
    assert torch.equal(e.clip_vision_hidden(pv), hid0)
    g = np.load(os.path.join(HERE, "golden", "clip_vision.npz"))
    assert U.rel_l2(emb0, torch.from_numpy(g["image_embeds"][1:2])) <= TOL_TOWER
