"""Tensor inventories of the CLIP ViT-L/14 text tower (`CLIPTextModel`) the reference conditions on, and of the CLIP ViT-B/32
image tower its clustering stage describes patches with (`CLIP_B32_VISION`, at the end).

`CategoryFeatures.embed` (diffmining/typicality/compute.py:39-51) tokenises one prompt per category and
takes `self.clip(tokens)[0]` = `last_hidden_state` [n, 77, 768] of `openai/clip-vit-large-patch14-336`
(or `geolocal/StreetCLIP`, same architecture; compute.py:60-68).  The model lives in the `transformers`
dependency; this module restates the names and shapes of its state dict (123,060,480 parameters, 196
tensors) so a checkpoint can be checked before packing and synthetic weights can be generated offline.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple


@dataclass(frozen=True)
class CLIPTextConfig:
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5          # hidden_act = quick_gelu: x * sigmoid(1.702 x)
    bos_token_id: int = 49406
    eos_token_id: int = 49407


CLIP_L14_TEXT = CLIPTextConfig()


def clip_text_tensor_spec(cfg: CLIPTextConfig = CLIP_L14_TEXT) -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (name, shape) list; names are relative to `text_model.` (see `canonical_clip_name`)."""
    h, f = cfg.hidden_size, cfg.intermediate_size
    t: List[Tuple[str, Tuple[int, ...]]] = [
        ("embeddings.token_embedding.weight", (cfg.vocab_size, h)),
        ("embeddings.position_embedding.weight", (cfg.max_position_embeddings, h)),
    ]
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}"
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            t += [(f"{p}.self_attn.{proj}.weight", (h, h)), (f"{p}.self_attn.{proj}.bias", (h,))]
        t += [(f"{p}.layer_norm1.weight", (h,)), (f"{p}.layer_norm1.bias", (h,))]
        t += [(f"{p}.mlp.fc1.weight", (f, h)), (f"{p}.mlp.fc1.bias", (f,))]
        t += [(f"{p}.mlp.fc2.weight", (h, f)), (f"{p}.mlp.fc2.bias", (h,))]
        t += [(f"{p}.layer_norm2.weight", (h,)), (f"{p}.layer_norm2.bias", (h,))]
    t += [("final_layer_norm.weight", (h,)), ("final_layer_norm.bias", (h,))]
    return t


def clip_text_param_count(cfg: CLIPTextConfig = CLIP_L14_TEXT) -> int:
    n = 0
    for _, shp in clip_text_tensor_spec(cfg):
        k = 1
        for s in shp:
            k *= s
        n += k
    return n


def canonical_clip_name(name: str):
    """Key of a `CLIPTextModel` / pipeline state dict -> name used here; None for buffers off the path."""
    for pre in ("text_encoder.", "text_model."):
        if name.startswith(pre):
            name = name[len(pre):]
    if name.startswith("text_model."):
        name = name[len("text_model."):]
    if name.endswith("position_ids"):
        return None
    return name


# ---- CLIP ViT-B/32 image tower (`CLIPModel("openai/clip-vit-base-patch32").get_image_features`, cluster.py:218-231) ------------
@dataclass(frozen=True)
class CLIPVisionConfig:
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    image_size: int = 224
    patch_size: int = 32
    num_channels: int = 3
    projection_dim: int = 512
    layer_norm_eps: float = 1e-5          # hidden_act = quick_gelu


CLIP_B32_VISION = CLIPVisionConfig()


def clip_vision_tensor_spec(cfg: CLIPVisionConfig = CLIP_B32_VISION) -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (name, shape) list of `CLIPVisionModelWithProjection` (200 tensors, 87,849,216 parameters for ViT-B/32); names are
    relative to `vision_model.`, except `visual_projection.weight` (see `canonical_clip_vision_name`)."""
    h, f, p = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    n_pos = (cfg.image_size // p) ** 2 + 1
    t: List[Tuple[str, Tuple[int, ...]]] = [
        ("embeddings.class_embedding", (h,)),
        ("embeddings.patch_embedding.weight", (h, cfg.num_channels, p, p)),
        ("embeddings.position_embedding.weight", (n_pos, h)),
        ("pre_layrnorm.weight", (h,)), ("pre_layrnorm.bias", (h,)),
    ]
    for i in range(cfg.num_hidden_layers):
        q = f"encoder.layers.{i}"
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            t += [(f"{q}.self_attn.{proj}.weight", (h, h)), (f"{q}.self_attn.{proj}.bias", (h,))]
        t += [(f"{q}.layer_norm1.weight", (h,)), (f"{q}.layer_norm1.bias", (h,))]
        t += [(f"{q}.mlp.fc1.weight", (f, h)), (f"{q}.mlp.fc1.bias", (f,))]
        t += [(f"{q}.mlp.fc2.weight", (h, f)), (f"{q}.mlp.fc2.bias", (h,))]
        t += [(f"{q}.layer_norm2.weight", (h,)), (f"{q}.layer_norm2.bias", (h,))]
    t += [("post_layernorm.weight", (h,)), ("post_layernorm.bias", (h,))]
    t += [("visual_projection.weight", (cfg.projection_dim, h))]
    return t


def clip_vision_param_count(cfg: CLIPVisionConfig = CLIP_B32_VISION) -> int:
    n = 0
    for _, shp in clip_vision_tensor_spec(cfg):
        k = 1
        for s in shp:
            k *= s
        n += k
    return n


def canonical_clip_vision_name(name: str):
    """Key of a `CLIPVisionModelWithProjection` or full `CLIPModel` state dict -> name used here; None for what the image tower does
    not use (`text_model.*`, `text_projection.weight`, `logit_scale`, `position_ids` buffers).  The C loader
    (dm_f32_load_clip_vision_weight) applies the same rule."""
    if name.startswith("text_model.") or name in ("text_projection.weight", "logit_scale") or name.endswith("position_ids"):
        return None
    if name.startswith("vision_model."):
        name = name[len("vision_model."):]
    return name


def map_clip_vision_state_dict(sd, cfg: CLIPVisionConfig = CLIP_B32_VISION) -> dict:
    """The image tower's tensors of `sd` under their canonical names, checked against the spec: a missing, unexpected or misshapen
    tensor raises ValueError naming it."""
    spec = dict(clip_vision_tensor_spec(cfg))
    out = {}
    for k, v in sd.items():
        c = canonical_clip_vision_name(k)
        if c is None:
            continue
        if c not in spec:
            raise ValueError(f"unexpected tensor in the CLIP vision state dict: {k}")
        if tuple(v.shape) != spec[c]:
            raise ValueError(f"shape mismatch for {k}: {tuple(v.shape)} vs {spec[c]}")
        if c in out:
            raise ValueError(f"duplicate tensor {k}")
        out[c] = v
    missing = [k for k in spec if k not in out]
    if missing:
        raise ValueError(f"missing {len(missing)} CLIP vision tensor(s), e.g. {missing[0]}")
    return out


def check_clip_vision_config(cfg: dict) -> None:
    """`config.json` of a CLIPModel or CLIPVisionModelWithProjection directory: the ViT-B/32 image tower, else ValueError."""
    v = cfg.get("vision_config", cfg)
    want = CLIP_B32_VISION
    for key in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size"):
        if key in v and v[key] != getattr(want, key):
            raise ValueError(f"vision {key} = {v[key]}, ViT-B/32 has {getattr(want, key)}")
    if v.get("hidden_act", "quick_gelu") != "quick_gelu":
        raise ValueError(f"hidden_act {v['hidden_act']!r}: the tower implements quick_gelu")
    proj = cfg.get("projection_dim", want.projection_dim)
    if proj != want.projection_dim:
        raise ValueError(f"projection_dim = {proj}, ViT-B/32 has {want.projection_dim}")


# ---- the CLIP baseline's image tower (`CLIPModel.from_pretrained("geolocal/StreetCLIP")`, clipmining/ranking.py:58-70): ViT-L/14-336 -------
# 577 tokens, 392 tensors, 304,293,888 parameters (vision_model + visual_projection)
CLIP_L14_336_VISION = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                                       image_size=336, patch_size=14, projection_dim=768)


def check_clip_tower_geometry(cfg: CLIPVisionConfig) -> None:
    """What the fp32 net's configurable tower accepts (dm_f32_finalize_clip_tower applies the same rule), else ValueError: heads of 64
    (the flash kernel's head_dim), widths the fp32 GEMM tiles (k a multiple of 32, outputs of 4), whole patches."""
    if cfg.num_attention_heads < 1 or cfg.hidden_size != 64 * cfg.num_attention_heads:
        raise ValueError(f"hidden_size {cfg.hidden_size} != 64 * num_attention_heads {cfg.num_attention_heads}")
    if cfg.hidden_size % 32 or cfg.intermediate_size < 32 or cfg.intermediate_size % 32:
        raise ValueError(f"hidden_size {cfg.hidden_size} and intermediate_size {cfg.intermediate_size} must be multiples of 32")
    if cfg.projection_dim < 4 or cfg.projection_dim % 4:
        raise ValueError(f"projection_dim {cfg.projection_dim} must be a multiple of 4")
    if cfg.patch_size < 1 or cfg.image_size < cfg.patch_size or cfg.image_size % cfg.patch_size:
        raise ValueError(f"image_size {cfg.image_size} is not a multiple of patch_size {cfg.patch_size}")
    if cfg.num_hidden_layers < 1 or cfg.num_channels != 3:
        raise ValueError(f"num_hidden_layers {cfg.num_hidden_layers} / num_channels {cfg.num_channels}")


def check_clip_tower_config(cfg: dict, want: CLIPVisionConfig = CLIP_L14_336_VISION) -> None:
    """`config.json` of a CLIPModel (e.g. StreetCLIP) or CLIPVisionModelWithProjection directory against the tower config `want`:
    ValueError naming the first key that differs.  A CLIPModel config that leaves a vision key out means transformers' default for it."""
    check_clip_tower_geometry(want)
    v = cfg.get("vision_config", cfg)
    for key in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size"):
        if key in v and v[key] != getattr(want, key):
            raise ValueError(f"vision {key} = {v[key]}, the tower config has {getattr(want, key)}")
    if v.get("hidden_act", "quick_gelu") != "quick_gelu":
        raise ValueError(f"hidden_act {v['hidden_act']!r}: the tower implements quick_gelu")
    proj = cfg.get("projection_dim", v.get("projection_dim", want.projection_dim))
    if proj != want.projection_dim:
        raise ValueError(f"projection_dim = {proj}, the tower config has {want.projection_dim}")
