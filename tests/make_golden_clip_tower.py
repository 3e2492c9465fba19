"""Generates tests/golden/clip_tower.npz: the CLIP baseline's two towers (clipmining/ranking.py:58-70) as `transformers` itself
computes them, in fp32 on the CPU with eager attention, on synthetic weights.

    python tests/make_golden_clip_tower.py

Image tower: the REAL `transformers.CLIPVisionModelWithProjection` at the TEST config below — 336 px, patch 14 (577 tokens, patch rows
of 588 values), heads of 64: every shape property of ViT-L/14-336 that can go wrong, at 1/200 of its weights — with
`synth.synth_clip_vision_state_dict(0, TEST_CFG)` on `synth.synth_clip_pixel_values(2, size=336)`.  Stored: tokens [2, 576, 64] =
`visual_projection(post_layernorm(last_hidden_state[:, 1:, :]))` exactly as the reference's `project_image` forms them,
last_hidden_state of image 0 [577, 128], and floor_hidden / floor_tokens = the rel-L2 of that fp32 run against the same model in
float64 (what the reference itself is uncertain by).

Text tower: the REAL `transformers.CLIPTextModelWithProjection` (ViT-L/14 text config, projection 768) with
`synth.synth_clip_state_dict(seed=0)` + `synth.synth_clip_text_projection(0)` on `synth.synth_token_ids(3)` (EOS at positions 1, 6, 2)
-> text_embeds [3, 768], not normalised.

Weights and inputs are regenerated deterministically, never stored."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.clip_spec import CLIP_L14_TEXT, CLIPVisionConfig as SpecVisionConfig  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "clip_tower.npz")
TEST_CFG = SpecVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=336, patch_size=14,
                            projection_dim=64)
N_IMAGES = 2


def _rel(a, b):
    return float(((a.double() - b.double()).norm() / b.double().norm()).item())


def vision():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    c = TEST_CFG
    cfg = CLIPVisionConfig(hidden_size=c.hidden_size, intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                           num_attention_heads=c.num_attention_heads, image_size=c.image_size, patch_size=c.patch_size,
                           num_channels=c.num_channels, projection_dim=c.projection_dim, hidden_act="quick_gelu",
                           layer_norm_eps=c.layer_norm_eps)
    cfg._attn_implementation = "eager"
    model = CLIPVisionModelWithProjection(cfg).eval().float()
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_clip_vision_state_dict(0, c).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    pv = torch.from_numpy(synth.synth_clip_pixel_values(N_IMAGES, size=c.image_size))

    def run(m, x):
        with torch.no_grad():
            h = m.vision_model(pixel_values=x).last_hidden_state
            return h, m.visual_projection(m.vision_model.post_layernorm(h[:, 1:, :]))
    h32, t32 = run(model, pv)
    h64, t64 = run(model.double(), pv.double())
    return {"tokens": t32.numpy().astype(np.float32), "last_hidden_state": h32[0].numpy().astype(np.float32),
            "floor_hidden": np.array(_rel(h32, h64)), "floor_tokens": np.array(_rel(t32, t64))}


def text():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    t = CLIP_L14_TEXT
    cfg = CLIPTextConfig(vocab_size=t.vocab_size, hidden_size=t.hidden_size, intermediate_size=t.intermediate_size,
                         num_hidden_layers=t.num_hidden_layers, num_attention_heads=t.num_attention_heads,
                         max_position_embeddings=t.max_position_embeddings, hidden_act="quick_gelu", layer_norm_eps=t.layer_norm_eps,
                         bos_token_id=t.bos_token_id, eos_token_id=t.eos_token_id, pad_token_id=1, projection_dim=768)
    cfg._attn_implementation = "eager"
    model = CLIPTextModelWithProjection(cfg).eval().float()
    sd = {"text_model." + k: torch.from_numpy(v) for k, v in synth.synth_clip_state_dict(seed=0).items()}
    sd["text_projection.weight"] = torch.from_numpy(synth.synth_clip_text_projection(0))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
    ids = synth.synth_token_ids(3)
    with torch.no_grad():
        emb = model(input_ids=torch.from_numpy(ids)).text_embeds
    return {"text_embeds": emb.numpy().astype(np.float32)}


def main():
    import transformers
    out = {**vision(), **text(), "transformers_version": np.array(transformers.__version__)}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; floors", float(out["floor_hidden"]), float(out["floor_tokens"]))


if __name__ == "__main__":
    main()
