"""Generates tests/golden/clip_vision.npz: the REAL `transformers.CLIPVisionModelWithProjection` (ViT-B/32 configuration, the
image tower of `openai/clip-vit-base-patch32` that the reference's clustering stage loads, cluster.py:218-231) in fp32 on the
CPU, with the synthetic weights `synth.synth_clip_vision_state_dict(0)` and the synthetic pixel values
`synth.synth_clip_pixel_values(3)`.

    python tests/make_golden_clip_vision.py

Weights and inputs are regenerated deterministically, not stored; the file holds last_hidden_state [3, 50, 768],
image_embeds [3, 512] (get_image_features, not normalised) and the transformers version that produced them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.clip_spec import CLIP_B32_VISION  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "clip_vision.npz")
N_IMAGES = 3


def main():
    import transformers
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = CLIP_B32_VISION
    cfg = CLIPVisionConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, image_size=c.image_size, patch_size=c.patch_size,
                           num_channels=c.num_channels, projection_dim=c.projection_dim, hidden_act="quick_gelu",
                           layer_norm_eps=c.layer_norm_eps)
    cfg._attn_implementation = "eager"
    model = CLIPVisionModelWithProjection(cfg).eval().float()
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_clip_vision_state_dict(0).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    pv = torch.from_numpy(synth.synth_clip_pixel_values(N_IMAGES))
    with torch.no_grad():
        out = model(pixel_values=pv)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, last_hidden_state=out.last_hidden_state.numpy().astype(np.float32),
                        image_embeds=out.image_embeds.numpy().astype(np.float32), transformers_version=np.array(transformers.__version__))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
