"""CPU tier of the CLIP baseline's towers on the fp32 net: the ViT-L/14-336 tensor inventory and config checks, the weight-name
mapping, `clip_tower_preprocess_numpy` against transformers' PIL-backend processor without the center crop, `clipmine.center_crop`
against torchvision's rounding rule, the fixture (tests/golden/clip_tower.npz, tests/make_golden_clip_tower.py) and the argmax
pooling rule of the text embeddings."""
import os

import numpy as np
import PIL.Image
import pytest

from diff_mining_amd import clip_spec as S
from diff_mining_amd import clipmine
from diff_mining_amd import resample as RS
from diff_mining_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_tower.npz")
# the fixture's image tower: 336 px / patch 14 / heads of 64 as ViT-L/14-336, at 1/200 of its weights
TEST_CFG = S.CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=336, patch_size=14,
                              projection_dim=64)
# the tower tolerance of tests/test_gpu_clip_tower.py (the project's own for the 12-layer B/32 tower); the reference's own fp32
# uncertainty must stay within a quarter of it
TOL_TOWER = 1e-5


def _rand_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_l14_336_spec():
    spec = S.clip_vision_tensor_spec(S.CLIP_L14_336_VISION)
    assert len(spec) == 392 == 8 + 16 * 24
    assert S.clip_vision_param_count(S.CLIP_L14_336_VISION) == 304_293_888
    d = dict(spec)
    assert d["embeddings.patch_embedding.weight"] == (1024, 3, 14, 14)
    assert d["embeddings.position_embedding.weight"] == (577, 1024)
    assert d["encoder.layers.23.mlp.fc1.weight"] == (4096, 1024)
    assert d["visual_projection.weight"] == (768, 1024)
    S.check_clip_tower_geometry(S.CLIP_L14_336_VISION)
    S.check_clip_tower_geometry(TEST_CFG)
    assert len(S.clip_vision_tensor_spec(TEST_CFG)) == 8 + 16 * 3
    # the B/32 inventory is what it was
    assert len(S.clip_vision_tensor_spec()) == 200 and S.clip_vision_param_count() == 87_849_216


def test_name_mapping_both_layouts():
    sd = synth.synth_clip_vision_state_dict(0, TEST_CFG)                       # CLIPVisionModelWithProjection names
    canon = S.map_clip_vision_state_dict(sd, TEST_CFG)
    assert set(canon) == {n for n, _ in S.clip_vision_tensor_spec(TEST_CFG)}
    full = dict(sd)                                                             # a full CLIPModel state dict: text half, scale, buffers
    full["text_model.embeddings.token_embedding.weight"] = np.zeros((4, 4), np.float32)
    full["text_projection.weight"] = np.zeros((4, 4), np.float32)
    full["logit_scale"] = np.zeros((), np.float32)
    full["vision_model.embeddings.position_ids"] = np.arange(577)[None]
    canon2 = S.map_clip_vision_state_dict(full, TEST_CFG)
    assert set(canon2) == set(canon) and all(canon2[k] is canon[k] for k in canon)
    bare = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}     # canonical names
    assert set(S.map_clip_vision_state_dict(bare, TEST_CFG)) == set(canon)
    # refused: the wrong config, a missing tensor, a misshapen one, an unexpected one
    with pytest.raises(ValueError, match="shape mismatch"):
        S.map_clip_vision_state_dict(sd)
    bad = dict(sd)
    del bad["vision_model.encoder.layers.2.mlp.fc2.bias"]
    with pytest.raises(ValueError, match="encoder.layers.2.mlp.fc2.bias"):
        S.map_clip_vision_state_dict(bad, TEST_CFG)
    bad = dict(sd)
    bad["vision_model.embeddings.position_embedding.weight"] = bad["vision_model.embeddings.position_embedding.weight"][:50]
    with pytest.raises(ValueError, match="position_embedding"):
        S.map_clip_vision_state_dict(bad, TEST_CFG)
    bad = dict(sd)
    bad["vision_model.encoder.layers.3.layer_norm1.weight"] = np.zeros(128, np.float32)
    with pytest.raises(ValueError, match="unexpected"):
        S.map_clip_vision_state_dict(bad, TEST_CFG)


def _streetclip_config():
    """The vision half and projection of a StreetCLIP-style (CLIP ViT-L/14-336) CLIPModel config.json."""
    return {"model_type": "clip", "projection_dim": 768, "logit_scale_init_value": 2.6592,
            "text_config": {"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12, "num_attention_heads": 12},
            "vision_config": {"model_type": "clip_vision_model", "hidden_size": 1024, "intermediate_size": 4096, "num_hidden_layers": 24,
                              "num_attention_heads": 16, "image_size": 336, "patch_size": 14, "hidden_act": "quick_gelu", "projection_dim": 768}}


def test_config_check():
    S.check_clip_tower_config(_streetclip_config())
    for key, val in (("hidden_size", 768), ("intermediate_size", 3072), ("num_hidden_layers", 12), ("num_attention_heads", 12),
                     ("image_size", 224), ("patch_size", 32)):
        cfg = _streetclip_config()
        cfg["vision_config"][key] = val
        with pytest.raises(ValueError, match=key):
            S.check_clip_tower_config(cfg)
    cfg = _streetclip_config()
    cfg["projection_dim"] = 512
    with pytest.raises(ValueError, match="projection_dim"):
        S.check_clip_tower_config(cfg)
    cfg = _streetclip_config()
    cfg["vision_config"]["hidden_act"] = "gelu"
    with pytest.raises(ValueError, match="hidden_act"):
        S.check_clip_tower_config(cfg)
    # a bare CLIPVisionModelWithProjection config, and another tower config as the yardstick
    S.check_clip_tower_config(dict(_streetclip_config()["vision_config"]))
    with pytest.raises(ValueError, match="hidden_size"):
        S.check_clip_tower_config(_streetclip_config(), TEST_CFG)
    # the geometry the kernels need
    with pytest.raises(ValueError, match="64"):
        S.check_clip_tower_geometry(S.CLIPVisionConfig(hidden_size=768, num_attention_heads=8, image_size=336, patch_size=14))
    with pytest.raises(ValueError, match="intermediate_size"):
        S.check_clip_tower_geometry(S.CLIPVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=500, image_size=336, patch_size=14))
    with pytest.raises(ValueError, match="projection_dim"):
        S.check_clip_tower_geometry(S.CLIPVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=512, projection_dim=66))
    with pytest.raises(ValueError, match="patch_size"):
        S.check_clip_tower_geometry(S.CLIPVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=512, image_size=336, patch_size=32))


@pytest.mark.parametrize("side", [512, 336, 337, 200])
def test_tower_preprocess_numpy_equals_transformers(side):
    """The reference's processor call (ranking.py:66) on its 512 x 512 center crop; 336 = both passes skipped, 337 = a one-pixel
    downscale, 200 = an upscale."""
    import transformers
    proc = transformers.CLIPImageProcessorPil(size={"shortest_edge": 336}, do_center_crop=False)
    a = _rand_image(side, side, seed=side)
    ref = np.asarray(proc(images=[PIL.Image.fromarray(a)])["pixel_values"][0])
    got = RS.clip_tower_preprocess_numpy(a, size=336)
    assert got.dtype == np.float32 and got.shape == (3, 336, 336) and ref.dtype == np.float32
    assert np.array_equal(got, ref)
    assert np.array_equal(RS.clip_tower_preprocess_numpy(PIL.Image.fromarray(a)), got)


def test_tower_preprocess_rejects_non_square():
    for shape in ((336, 337), (512, 300), (1, 2)):
        with pytest.raises(ValueError, match="square"):
            RS.clip_tower_preprocess_numpy(_rand_image(*shape, seed=1))
        with pytest.raises(ValueError, match="square"):
            RS.clip_tower_plan([_rand_image(*shape, seed=1)])
    with pytest.raises(ValueError):
        RS.clip_tower_preprocess_numpy(np.zeros((8, 8, 3), np.float32))


def test_tower_plan_descriptors():
    imgs = [_rand_image(s, s, s) for s in (512, 336, 200, 512)]
    desc, tables = RS.clip_tower_plan(imgs, 336)
    assert desc.dtype == RS.CLIP_DESC_DTYPE and len(desc) == 4 and tables.dtype == np.int32
    assert list(desc["src_offset"]) == [0, 512 * 512 * 3, 512 * 512 * 3 + 336 * 336 * 3, 512 * 512 * 3 + 336 * 336 * 3 + 200 * 200 * 3]
    assert (desc["left"] == 0).all() and (desc["top"] == 0).all() and (desc["crop_w"] == desc["src_w"]).all()
    assert list(desc["flags"]) == [3, 0, 3, 3]
    assert desc["xb_off"][0] == desc["xb_off"][3] and desc["xk_off"][0] == desc["xk_off"][3]          # one copy per distinct side
    for d in desc:
        b, k = RS.bicubic_axis(int(d["src_w"]), 336)
        assert np.array_equal(tables[d["xb_off"]:d["xb_off"] + b.size].reshape(b.shape), b)
        assert np.array_equal(tables[d["xk_off"]:d["xk_off"] + k.size].reshape(k.shape), k) and d["kx"] == k.shape[1] == d["ky"]
        assert d["yb_off"] == d["xb_off"] and d["yk_off"] == d["xk_off"]


def test_center_crop_offsets():
    """torchvision's CenterCrop: top = int(round((H - 512) / 2.0)) with Python's rounding — halves go to even."""
    for side, off in ((512, 0), (513, 0), (514, 1), (515, 2)):
        a = _rand_image(side, side + 2, seed=side)
        got = clipmine.center_crop(a, 512)
        left = int(round((side + 2 - 512) / 2.0))
        assert got.shape == (512, 512, 3) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, a[off:off + 512, left:left + 512]), side
    assert np.array_equal(clipmine.center_crop(PIL.Image.fromarray(_rand_image(515, 515, 0)), 512), _rand_image(515, 515, 0)[2:514, 2:514])
    for shape in ((511, 600), (600, 511), (100, 100)):
        with pytest.raises(ValueError, match="smaller"):
            clipmine.center_crop(_rand_image(*shape, seed=0), 512)


def test_fixture():
    g = np.load(GOLDEN)
    assert set(g.files) == {"tokens", "last_hidden_state", "floor_hidden", "floor_tokens", "text_embeds", "transformers_version"}
    assert g["tokens"].shape == (2, 576, 64) and g["tokens"].dtype == np.float32
    assert g["last_hidden_state"].shape == (577, 128) and g["last_hidden_state"].dtype == np.float32
    assert g["text_embeds"].shape == (3, 768) and g["text_embeds"].dtype == np.float32
    assert all(np.isfinite(g[k]).all() for k in ("tokens", "last_hidden_state", "text_embeds"))
    assert str(g["transformers_version"])
    print(f"\nclip tower fixture (transformers {g['transformers_version']}): fp32 vs float64 rel-L2 hidden {float(g['floor_hidden']):.2e}, "
          f"tokens {float(g['floor_tokens']):.2e}")
    assert 0.0 < float(g["floor_hidden"]) <= TOL_TOWER / 4 and 0.0 < float(g["floor_tokens"]) <= TOL_TOWER / 4
    assert os.path.getsize(GOLDEN) < 658_082               # below the largest fixture committed before it (clip_text.npz)
    # the rows of different images and prompts differ (a fixture of identical rows would pin nothing)
    assert np.abs(g["tokens"][0] - g["tokens"][1]).max() > 1e-2 and np.abs(g["text_embeds"][0] - g["text_embeds"][1]).max() > 1e-2


def _pool_position(ids):
    """The numpy restatement of the pooling rule dm_f32_clip_text_embeds implements: the first position of the largest id."""
    return np.argmax(np.asarray(ids), axis=-1)


def test_argmax_pooling_rule():
    ids = synth.synth_token_ids(3)
    eos = S.CLIP_L14_TEXT.eos_token_id
    pos = _pool_position(ids)
    assert list(pos) == [1, 6, 2]                          # EOS at three different positions (prompts of 2, 7 and 3 tokens)
    for r, p in zip(ids, pos):
        assert r[p] == eos == r.max() and (r[:p] != eos).all() and (r[p:] == eos).all()          # the first EOS; EOS padding behind it
    # transformers' other rule (eos_token_id != 2): the first position that EQUALS eos_token_id — the same position
    assert np.array_equal(pos, (ids == eos).argmax(axis=-1))
    # ties: argmax returns the first maximum
    assert _pool_position(np.array([[5, 9, 3, 9, 9]])) == 1
