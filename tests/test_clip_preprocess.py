"""CPU tier of the CLIP ViT-B/32 image path: PIL's BICUBIC tables restated on the host (resample.bicubic_axis) against PIL itself,
`clip_preprocess_numpy` against transformers' `CLIPImageProcessorPil`, the packed descriptors of one dm_f32_clip_preprocess launch,
the image-tower fixture and the weight-name mapping of both checkpoint layouts."""
import os

import numpy as np
import PIL.Image
import pytest

from diff_mining_amd import clip_spec as S
from diff_mining_amd import resample as RS
from diff_mining_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vision.npz")


def _rand_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _full_tables(w, h, ow, oh):
    return RS.bicubic_axis(w, ow), RS.bicubic_axis(h, oh)


# (source h, w) -> (out h, w): the 50^2 / 64^2 patch upscales, odd crops, a downscale from a 256-short-side image,
# sizes that keep one axis, and the no-op size
RESIZES = [((50, 50), (224, 224)), ((64, 64), (224, 224)), ((37, 91), (224, 550)), ((91, 37), (550, 224)), ((61, 53), (258, 224)),
           ((256, 384), (224, 336)), ((300, 256), (262, 224)), ((224, 100), (224, 501)), ((100, 224), (501, 224)), ((224, 224), (224, 224)),
           ((7, 3), (224, 96))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in RESIZES])
def test_bicubic_tables_are_pils(src, dst):
    a = _rand_image(*src, seed=src[0] * 31 + src[1])
    (h, w), (oh, ow) = src, dst
    xt, yt = _full_tables(w, h, ow, oh)
    got = RS.resize_numpy_tables(a, xt, yt, ow != w, oh != h)
    ref = np.asarray(PIL.Image.fromarray(a).resize((ow, oh), PIL.Image.BICUBIC))
    assert np.array_equal(got, ref)


def test_bicubic_windows_equal_full_resize():
    """The center-crop window of the tables (what the device computes) gives the crop of the full resize."""
    for (h, w) in [(333, 517), (517, 333), (180, 1000), (256, 300)]:
        a = _rand_image(h, w, seed=h + w)
        need_h, need_v, left, top, xt, yt = RS.clip_patch_tables(w, h)
        nw, nh = RS.clip_resize_size(w, h)
        full = np.asarray(PIL.Image.fromarray(a).resize((nw, nh), PIL.Image.BICUBIC))
        got = RS.resize_numpy_tables(a, xt, yt, need_h, need_v, left, top)
        assert np.array_equal(got, full[top:top + 224, left:left + 224])


def test_bicubic_identity_axis():
    b, k = RS.bicubic_axis(224, 224)
    assert (b[:, 0] == np.arange(224)).all() and (b[:, 1] == 1).all() and (k == 1 << RS.PRECISION_BITS).all()


# whole images (box None) and boxes in the reference's convention (x_start, y_start, x_end, y_end; x = rows)
CASES = [((512, 512), (10, 20, 74, 84)), ((512, 512), (0, 0, 64, 64)), ((512, 512), (462, 462, 512, 512)), ((300, 400), (3, 100, 53, 150)),
         ((300, 400), (0, 0, 300, 400)), ((333, 517), None), ((517, 333), None), ((224, 400), None), ((400, 224), None), ((224, 224), None),
         ((180, 1000), None), ((257, 256), None), ((300, 300), (100, 3, 171, 60))]


@pytest.mark.parametrize("shape,box", CASES, ids=[f"{s[0]}x{s[1]}-{b}" for s, b in CASES])
def test_preprocess_numpy_equals_transformers(shape, box):
    pytest.importorskip("transformers")
    import transformers
    if not hasattr(transformers, "CLIPImageProcessorPil"):
        pytest.skip("this transformers has no CLIPImageProcessorPil")
    proc = transformers.CLIPImageProcessorPil()
    a = _rand_image(*shape, seed=shape[0] * 3 + shape[1])
    pil = PIL.Image.fromarray(a)
    if box is not None:
        x0, y0, x1, y1 = box
        pil = pil.crop((y0, x0, y1, x1))
    ref = np.asarray(proc(images=[pil])["pixel_values"][0])
    got = RS.clip_preprocess_numpy(a, box)
    assert got.dtype == np.float32 and got.shape == (3, 224, 224)
    assert ref.dtype == np.float32
    assert np.array_equal(got, ref)


def test_preprocess_numpy_accepts_pil():
    a = _rand_image(90, 70, 1)
    assert np.array_equal(RS.clip_preprocess_numpy(PIL.Image.fromarray(a), (5, 6, 55, 56)), RS.clip_preprocess_numpy(a, (5, 6, 55, 56)))
    rgba = PIL.Image.fromarray(np.dstack([a, np.full(a.shape[:2], 200, np.uint8)]))
    assert np.array_equal(RS.clip_preprocess_numpy(rgba, None), RS.clip_preprocess_numpy(a, None))


def test_plan_descriptors_are_consistent():
    imgs = [_rand_image(100, 120, 0), _rand_image(300, 200, 1), _rand_image(224, 224, 2)]
    boxes = [[(0, 0, 64, 64), (36, 56, 100, 120), (10, 10, 60, 60)], None, [None, (0, 0, 224, 224)]]
    desc, tables, owner = RS.clip_plan(imgs, boxes)
    assert desc.dtype.itemsize == 72 and len(desc) == 6
    assert owner.tolist() == [0, 0, 0, 1, 2, 2]
    offs = [0, 100 * 120 * 3, 100 * 120 * 3 + 300 * 200 * 3]
    assert desc["src_offset"].tolist() == [offs[i] for i in owner]
    assert desc["src_w"].tolist() == [120, 120, 120, 200, 224, 224] and desc["src_h"].tolist() == [100, 100, 100, 300, 224, 224]
    assert desc["crop_row0"].tolist()[:3] == [0, 36, 10] and desc["crop_col0"].tolist()[:3] == [0, 56, 10]
    assert desc["crop_w"].tolist() == [64, 64, 50, 200, 224, 224] and desc["crop_h"].tolist() == [64, 64, 50, 300, 224, 224]
    assert desc["flags"].tolist() == [3, 3, 3, RS.CLIP_NEED_H | RS.CLIP_NEED_V, 0, 0]
    # equal crop sizes share one table window
    assert desc["xk_off"][0] == desc["xk_off"][1] and desc["xk_off"][0] != desc["xk_off"][2]
    for d in desc:
        need_h, need_v, left, top, (xb, xk), (yb, yk) = RS.clip_patch_tables(int(d["crop_w"]), int(d["crop_h"]))
        assert (d["left"], d["top"], d["kx"], d["ky"]) == (left, top, xk.shape[1], yk.shape[1])
        assert np.array_equal(tables[d["xb_off"]:d["xb_off"] + 448].reshape(224, 2), xb)
        assert np.array_equal(tables[d["xk_off"]:d["xk_off"] + 224 * d["kx"]].reshape(224, -1), xk)
        assert np.array_equal(tables[d["yb_off"]:d["yb_off"] + 448].reshape(224, 2), yb)
        assert np.array_equal(tables[d["yk_off"]:d["yk_off"] + 224 * d["ky"]].reshape(224, -1), yk)
        assert (xb[:, 0] >= 0).all() and (xb.sum(1) <= d["crop_w"]).all() and (yb.sum(1) <= d["crop_h"]).all()
        assert d["crop_row0"] + d["crop_h"] <= d["src_h"] and d["crop_col0"] + d["crop_w"] <= d["src_w"]


@pytest.mark.parametrize("box", [(0, 0, 0, 10), (5, 5, 5, 9), (10, 0, 5, 10), (-1, 0, 10, 10), (0, 0, 101, 10), (0, 0, 10, 121),
                                 (0, 120, 10, 130), (100, 0, 110, 10)])
def test_plan_rejects_bad_boxes(box):
    with pytest.raises(ValueError):
        RS.clip_plan([_rand_image(100, 120, 0)], [[box]])
    with pytest.raises(ValueError):
        RS.clip_preprocess_numpy(_rand_image(100, 120, 0), box)


def test_plan_rejects_bad_images():
    with pytest.raises(ValueError):
        RS.check_clip_image(np.zeros((10, 10, 3), np.float32))
    with pytest.raises(ValueError):
        RS.check_clip_image(np.zeros((10, 10, 4), np.uint8))
    with pytest.raises(ValueError):
        RS.check_clip_image(np.zeros((10, 10), np.uint8))
    with pytest.raises(TypeError):
        RS.check_clip_image([[1, 2, 3]])
    with pytest.raises(ValueError):
        RS.clip_plan([_rand_image(10, 10, 0)], [None, None])


def test_fixture_keys_shapes_dtypes():
    d = np.load(GOLDEN)
    assert set(d.files) == {"last_hidden_state", "image_embeds", "transformers_version"}
    assert d["last_hidden_state"].shape == (3, 50, 768) and d["last_hidden_state"].dtype == np.float32
    assert d["image_embeds"].shape == (3, 512) and d["image_embeds"].dtype == np.float32
    assert d["transformers_version"].dtype.kind == "U" and str(d["transformers_version"])
    assert np.isfinite(d["last_hidden_state"]).all() and np.isfinite(d["image_embeds"]).all()
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_spec_counts():
    spec = S.clip_vision_tensor_spec()
    assert len(spec) == 200 and len({n for n, _ in spec}) == 200
    assert S.clip_vision_param_count() == 87_849_216


def test_name_mapping_both_layouts():
    vis = synth.synth_clip_vision_state_dict(0)
    assert len(vis) == 200
    m = S.map_clip_vision_state_dict(vis)
    assert set(m) == {n for n, _ in S.clip_vision_tensor_spec()}
    # a full CLIPModel state dict: text half, text projection, logit scale and position_ids buffers are skipped
    full = dict(vis)
    full["vision_model.embeddings.position_ids"] = np.arange(50)[None]
    full["text_model.embeddings.position_ids"] = np.arange(77)[None]
    full["text_model.final_layer_norm.weight"] = np.ones(512, np.float32)
    full["text_projection.weight"] = np.zeros((512, 512), np.float32)
    full["logit_scale"] = np.array(2.6592, np.float32)
    m2 = S.map_clip_vision_state_dict(full)
    assert set(m2) == set(m) and all(m2[k] is m[k] for k in m)
    assert S.canonical_clip_vision_name("vision_model.encoder.layers.3.mlp.fc1.weight") == "encoder.layers.3.mlp.fc1.weight"
    assert S.canonical_clip_vision_name("visual_projection.weight") == "visual_projection.weight"
    assert S.canonical_clip_vision_name("vision_model.embeddings.position_ids") is None


def test_name_mapping_rejects_bad_dicts():
    vis = synth.synth_clip_vision_state_dict(0)
    missing = dict(vis)
    del missing["vision_model.encoder.layers.11.mlp.fc2.bias"]
    with pytest.raises(ValueError, match="missing"):
        S.map_clip_vision_state_dict(missing)
    bad = dict(vis)
    bad["vision_model.post_layernorm.weight"] = np.ones(512, np.float32)
    with pytest.raises(ValueError, match="shape"):
        S.map_clip_vision_state_dict(bad)
    extra = dict(vis)
    extra["vision_model.encoder.layers.12.mlp.fc1.bias"] = np.ones(3072, np.float32)
    with pytest.raises(ValueError, match="unexpected"):
        S.map_clip_vision_state_dict(extra)


def test_config_check():
    S.check_clip_vision_config({"projection_dim": 512, "vision_config": {"hidden_size": 768, "patch_size": 32, "hidden_act": "quick_gelu"}})
    with pytest.raises(ValueError):
        S.check_clip_vision_config({"vision_config": {"patch_size": 14}})
    with pytest.raises(ValueError):
        S.check_clip_vision_config({"projection_dim": 768, "vision_config": {}})


def test_feature_which_parsing():
    from diff_mining_amd.dift import parse_feature_which
    assert parse_feature_which("clip") == (True, False, None)
    assert parse_feature_which("dift-261") == (False, True, 261)
    assert parse_feature_which("clip+dift-101") == (True, True, 101)
    for bad in ("dift", "clip+clip", "dift-261+clip", "sift-3", "clip+dift-x", ""):
        with pytest.raises(ValueError):
            parse_feature_which(bad)
