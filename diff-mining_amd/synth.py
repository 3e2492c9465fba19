"""Deterministic synthetic weights for the SDv1.5 U-Net (no checkpoint is reachable offline).

The generator is counter based and uses only integer arithmetic plus one IEEE
double multiply, so the same (seed, name, index) gives the same fp32 value on any
machine and any NumPy build:

    key   = fnv1a64(name) ^ splitmix64(seed)
    bits  = splitmix64(key + index * GOLDEN)
    value = (sum of the four 16-bit fields of bits - 131070) / sqrt(4*(2^32-1)/12)

i.e. an Irwin-Hall(4) approximation of N(0,1) with support +-3.46 sigma, which keeps
fp16 activations bounded.  Scales are fan-in normalised so every pre-norm
activation of the U-Net stays O(1) (SURVEY.md §7 hard part 6).

Values are finally rounded to fp16 and returned as fp32 holding fp16-representable
numbers: the reference loads its pipeline with `torch_dtype=torch.float16`
(`diffmining/typicality/compute.py:65-70`), so the engine and the oracle must see
the *same* fp16 weights.
"""
from __future__ import annotations

import os

import numpy as np

from .unet_spec import SD15, UNetConfig, unet_tensor_spec

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_IH_MEAN = 2.0 * 65535.0
_IH_STD = float(np.sqrt(4.0 * (65536.0 ** 2 - 1.0) / 12.0))


def _splitmix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def fnv1a64(s: str) -> int:
    h = 0xCBF29CE484222325
    for b in s.encode("utf-8"):
        h ^= b
        h = (h * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _hash_normal_range(key, lo, hi):
    with np.errstate(over="ignore"):
        idx = np.arange(lo, hi, dtype=np.uint64)
        bits = _splitmix64(key + idx * _GOLDEN)
    s = (bits & np.uint64(0xFFFF)).astype(np.float64)
    s += ((bits >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.float64)
    s += ((bits >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.float64)
    s += (bits >> np.uint64(48)).astype(np.float64)
    s -= _IH_MEAN
    s /= _IH_STD
    return s


_CHUNK = 1 << 20
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))
    return _POOL


def hash_normal(name: str, n: int, seed: int = 0) -> np.ndarray:
    """n pseudo-normal fp64 values for tensor `name` (see module docstring).  NumPy ufuncs release
    the GIL, so large tensors are generated chunk-wise on a thread pool (same values either way)."""
    with np.errstate(over="ignore"):
        key = np.uint64(fnv1a64(name)) ^ _splitmix64(np.array([seed], dtype=np.uint64) + _GOLDEN)[0]
    if n <= _CHUNK:
        return _hash_normal_range(key, 0, n)
    out = np.empty(n, dtype=np.float64)
    bounds = [(lo, min(n, lo + _CHUNK)) for lo in range(0, n, _CHUNK)]

    def work(b):
        out[b[0]:b[1]] = _hash_normal_range(key, b[0], b[1])
    list(_pool().map(work, bounds))
    return out


def _scale_for(name: str, shape) -> tuple:
    """(kind, scale, offset) for a tensor: value = offset + scale * z."""
    leaf = name.rsplit(".", 1)[1]
    mod = name.rsplit(".", 2)[-2]                              # norm1, group_norm, conv_norm_out, ...
    is_norm = "norm" in mod and len(shape) == 1
    if is_norm:
        return (1.0, 0.1) if leaf == "weight" else (0.0, 0.05)   # gamma ~ 1 +- .1, beta ~ +-.05
    if leaf == "bias":
        return (0.0, 0.02)
    fan_in = 1
    for s in shape[1:]:
        fan_in *= s
    return (0.0, 1.0 / np.sqrt(float(fan_in)))


def synth_tensor(name: str, shape, seed: int = 0) -> np.ndarray:
    n = int(np.prod(shape))
    off, sc = _scale_for(name, shape)
    z = hash_normal(name, n, seed)
    v = (off + sc * z).astype(np.float32)
    return v.astype(np.float16).astype(np.float32).reshape(shape)


def hash_uniform(name: str, n: int, seed: int = 0) -> np.ndarray:
    """n values in [0, 1) for tensor `name` from the same integer hash (top 53 bits)."""
    with np.errstate(over="ignore"):
        key = np.uint64(fnv1a64(name)) ^ _splitmix64(np.array([seed], dtype=np.uint64) + _GOLDEN)[0]
        bits = _splitmix64(key + np.arange(n, dtype=np.uint64) * _GOLDEN)
    return (bits >> np.uint64(11)).astype(np.float64) / float(1 << 53)


# ---- "stress" weights: the same architecture OFF the benign operating point -------------------------------------
# The default weights give zero-mean O(1) activations everywhere.  Real SD-1.5 checkpoints do not: channel scales spread over
# decades, normalisation inputs carry |mean| >> std, a few channels are outliers.  mode="stress" builds that on the same hash:
#   * every conv / linear: output-channel scales log-uniform over two decades (10^U(-1,1), RMS-normalised so the layer's output
#     stays O(1) overall); attention q / k / v projections are left alone (outlier q.k products only saturate the softmax);
#   * the layers that WRITE a normalisation input (conv_in, conv1, conv2, conv_shortcut, proj_in, proj_out, to_out, ff.net.2,
#     down / up samplers): a common-sign bias of STRESS_BIAS x the layer's output RMS (sign per tensor) + three x50 outlier
#     output channels per tensor;
#   * norm gammas log-uniform over one decade, betas +-0.5.
# tests/test_gpu_stress.py::test_stress_operating_point_is_off_benign measures what the calibrated form (tests/stress_weights.py) does at every GroupNorm / LayerNorm input
# (|mean| / std per group or token, max |activation| < 65504).
STRESS_BIAS = 10.0
STRESS_OUTLIER = 50.0
_NORM_WRITERS = ("conv_in", "conv1", "conv2", "conv_shortcut", "proj_in", "proj_out", "to_out.0", "ff.net.2", "downsamplers.0.conv",
                 "upsamplers.0.conv")
# x50 outlier channels only where the layer's INPUT is normalised (the transformer's inner stream feeds proj_out un-normalised, the
# residual stream feeds conv_shortcut and the samplers un-normalised: outliers there compound to 50^2 ... and overflow fp16)
_OUTLIER_WRITERS = ("conv_in", "conv1", "conv2", "proj_in")


def _stress_tensor(name: str, shape, seed: int, stress_bias: float) -> np.ndarray:
    leaf = name.rsplit(".", 1)[1]
    mod = name.rsplit(".", 1)[0]
    short = mod.split(".")[-1] if not mod.endswith(("to_out.0", "ff.net.2", "downsamplers.0.conv", "upsamplers.0.conv")) else \
        next(w for w in _NORM_WRITERS if mod.endswith(w))
    is_norm = "norm" in mod.rsplit(".", 1)[-1] and len(shape) == 1
    n = int(np.prod(shape))
    if is_norm:
        if leaf == "weight":
            v = 10.0 ** (hash_uniform(name + "#g", n, seed) - 0.5)                       # 0.32 .. 3.2
            sign = np.where(hash_uniform(name + "#s", n, seed) < 0.15, -1.0, 1.0)       # a few negative gammas, as in real nets
            v = v * sign
        else:
            v = 0.5 * hash_normal(name, n, seed)
        return v.astype(np.float32).astype(np.float16).astype(np.float32).reshape(shape)
    writer = short in _NORM_WRITERS
    scaled = writer or short in ("proj", "linear_1", "linear_2", "time_emb_proj", "conv_out")      # not to_q / to_k / to_v
    cout = shape[0]
    sc = np.ones(cout)
    if scaled and cout >= 32:
        sc = 10.0 ** (2.0 * hash_uniform(mod + "#scale", cout, seed) - 1.0)
        sc /= np.sqrt(np.mean(sc * sc))
        if short in _OUTLIER_WRITERS:
            idx = (hash_uniform(mod + "#outlier", 3, seed) * cout).astype(np.int64)
            sc[idx] = STRESS_OUTLIER / np.sqrt(10.86)          # x50 the typical (median = 1 / 3.3) channel
    if leaf == "bias":
        v = 0.02 * hash_normal(name, n, seed) * sc
        if writer:
            sign = 1.0 if (short != "conv1" or hash_uniform(mod + "#sign", 1, seed)[0] < 0.5) else -1.0
            v = v + sign * stress_bias * (1.0 + 0.05 * hash_normal(name + "#b", n, seed))
        return v.astype(np.float32).astype(np.float16).astype(np.float32).reshape(shape)
    fan_in = 1
    for d in shape[1:]:
        fan_in *= d
    z = hash_normal(name, n, seed).reshape(cout, -1)
    v = z * (sc / np.sqrt(float(fan_in)))[:, None]
    return v.astype(np.float32).astype(np.float16).astype(np.float32).reshape(shape)


def synth_state_dict(cfg: UNetConfig = SD15, seed: int = 0, dtype=np.float32, mode: str = "benign",
                     stress_bias: float = STRESS_BIAS) -> dict:
    """name -> ndarray (fp16-representable values stored as `dtype`).  mode "benign": fan-in-scaled zero-mean weights (O(1)
    activations everywhere); "stress": per-channel scales over two decades, biased normalisation inputs, outlier channels
    (`stress_bias`: the common-sign offset of the norm-writing layers' biases; tests/stress_weights.py passes 0 and calibrates
    every offset against the measured spread of the normalisation input it feeds)."""
    assert mode in ("benign", "stress"), mode
    out = {}
    for name, shape in unet_tensor_spec(cfg):
        t = synth_tensor(name, shape, seed) if mode == "benign" else _stress_tensor(name, shape, seed, stress_bias)
        out[name] = t if dtype == np.float32 else t.astype(dtype)
    return out


# ---- one slab for the ranks of a node (bench.py --gpus N; VERDICT r05 #8b) ---------------------------------------------------------
# The 686 tensors take ~50 s of host arithmetic to synthesise; N ranks doing it side by side cost N x the cores and N x 1.7 GB of
# transient memory for identical bytes.  Rank 0 writes them once as ONE flat file (tensor bytes back to back, 256-byte aligned) with a
# JSON index beside it; the other ranks map the file read-only and hand the engine views into it.  /dev/shm is memory: the writer
# removes the pair once every rank has loaded (remove_slab).
def save_slab(sd: dict, path: str) -> None:
    """Writes {name: ndarray} to `path` (+ `path`.json) atomically (temporary name, then rename: a reader never sees a partial file)."""
    import json
    index, off = {}, 0
    tmp, jtmp = path + ".tmp%d" % os.getpid(), path + ".json.tmp%d" % os.getpid()
    try:
        with open(tmp, "wb") as f:
            for name, a in sd.items():
                a = np.asarray(a)                              # (tobytes() below is C order whatever the strides; 0-d stays 0-d)
                pad = (-off) % 256
                if pad:
                    f.write(b"\0" * pad)
                    off += pad
                f.write(a.tobytes())
                index[name] = {"dtype": a.dtype.str, "shape": list(a.shape), "offset": off}
                off += a.nbytes
        with open(jtmp, "w") as f:
            json.dump({"bytes": off, "tensors": index}, f)
        os.replace(jtmp, path + ".json")
        os.replace(tmp, path)
    except OSError:                                            # a full or absent mount: leave nothing behind, the caller decides
        for q in (tmp, jtmp):
            try:
                os.remove(q)
            except OSError:
                pass
        raise


def load_slab(path: str) -> dict:
    """{name: read-only ndarray view} over a file written by save_slab (np.memmap: pages are shared between the ranks)."""
    import json
    with open(path + ".json") as f:
        meta = json.load(f)
    if os.path.getsize(path) != meta["bytes"]:
        raise RuntimeError(f"{path}: {os.path.getsize(path)} bytes on disk, the index says {meta['bytes']}")
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    out = {}
    for name, m in meta["tensors"].items():
        dt = np.dtype(m["dtype"])
        n = int(np.prod(m["shape"])) if m["shape"] else 1
        out[name] = raw[m["offset"]:m["offset"] + n * dt.itemsize].view(dt).reshape(m["shape"])
    return out


def remove_slab(path: str) -> None:
    for p in (path, path + ".json"):
        try:
            os.remove(p)
        except FileNotFoundError:
            pass


def synth_vae_state_dict(cfg=None, seed: int = 0, dtype=np.float32) -> dict:
    """Synthetic `encoder.*` / `quant_conv.*` tensors of the SDv1.5 VAE (see vae_spec.py)."""
    from .vae_spec import SD15_VAE, vae_encoder_tensor_spec
    out = {}
    for name, shape in vae_encoder_tensor_spec(cfg or SD15_VAE):
        t = synth_tensor("vae." + name, shape, seed)
        out[name] = t if dtype == np.float32 else t.astype(dtype)
    return out


def synth_vae_decoder_state_dict(cfg=None, seed: int = 0, dtype=np.float32) -> dict:
    """Synthetic `post_quant_conv.*` / `decoder.*` tensors of the SDv1.5 VAE (see vae_spec.py)."""
    from .vae_spec import SD15_VAE, vae_decoder_tensor_spec
    out = {}
    for name, shape in vae_decoder_tensor_spec(cfg or SD15_VAE):
        t = synth_tensor("vae." + name, shape, seed)
        out[name] = t if dtype == np.float32 else t.astype(dtype)
    return out


def synth_clip_state_dict(cfg=None, seed: int = 0, dtype=np.float32) -> dict:
    """Synthetic CLIP text-tower tensors (see clip_spec.py).  Embeddings ~ N(0, 0.02) like the real model's
    initialiser range; linear layers fan-in scaled."""
    from .clip_spec import CLIP_L14_TEXT, clip_text_tensor_spec
    out = {}
    for name, shape in clip_text_tensor_spec(cfg or CLIP_L14_TEXT):
        if "embedding" in name:
            z = hash_normal("clip." + name, int(np.prod(shape)), seed)
            t = (0.02 * z).astype(np.float32).astype(np.float16).astype(np.float32).reshape(shape)
        else:
            t = synth_tensor("clip." + name, shape, seed)
        out[name] = t if dtype == np.float32 else t.astype(dtype)
    return out


def synth_clip_vision_state_dict(seed: int = 0, cfg=None, dtype=np.float32) -> dict:
    """Synthetic CLIP ViT-B/32 image-tower tensors (`CLIPVisionModelWithProjection` names, see clip_spec.py).  Class and position
    embeddings ~ N(0, 0.02) like synth_clip_state_dict's embeddings; the patch embedding, linear layers and projection fan-in
    scaled; norms near identity."""
    from .clip_spec import CLIP_B32_VISION, clip_vision_tensor_spec
    out = {}
    for name, shape in clip_vision_tensor_spec(cfg or CLIP_B32_VISION):
        if name in ("embeddings.class_embedding", "embeddings.position_embedding.weight"):
            z = hash_normal("clipv." + name, int(np.prod(shape)), seed)
            t = (0.02 * z).astype(np.float32).astype(np.float16).astype(np.float32).reshape(shape)
        else:
            t = synth_tensor("clipv." + name, shape, seed)
        key = name if name == "visual_projection.weight" else "vision_model." + name
        out[key] = t if dtype == np.float32 else t.astype(dtype)
    return out


def synth_clip_pixel_values(n: int, seed: int = 0, size: int = 224) -> np.ndarray:
    """Deterministic processor-like input [n, 3, size, size] fp32: a smooth per-image pattern plus noise, in the range the processor
    produces ((x - mean) / std of x in [0, 1], about [-1.8, 2.2])."""
    u = hash_uniform("input.clip_pixels", n * 3 * size * size, seed).reshape(n, 3, size, size)
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, size), np.linspace(0.0, 1.0, size), indexing="ij")
    base = 0.5 + 0.4 * np.sin(3.0 * xx + 5.0 * yy + np.arange(n * 3).reshape(n, 3, 1, 1))
    x = np.clip(0.7 * base + 0.3 * u, 0.0, 1.0).astype(np.float32)
    mean = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32).reshape(1, 3, 1, 1)
    std = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32).reshape(1, 3, 1, 1)
    return np.ascontiguousarray((x - mean) / std)


def synth_clip_text_projection(seed: int = 0, dim: int = 768) -> np.ndarray:
    """Synthetic `text_projection.weight` [dim, dim] of `CLIPTextModelWithProjection`, fan-in scaled like the other linear layers."""
    return synth_tensor("clip.text_projection.weight", (dim, dim), seed)


def synth_token_ids(n: int, cfg=None, seed: int = 3) -> np.ndarray:
    """[n, 77] int64 prompts shaped like the tokenizer's output (compute.py:35-37): BOS, a few random
    tokens, EOS, then EOS padding (`padding="max_length"` pads CLIP prompts with the EOS id)."""
    from .clip_spec import CLIP_L14_TEXT
    cfg = cfg or CLIP_L14_TEXT
    with np.errstate(over="ignore"):
        key = np.uint64(fnv1a64("input.tokens")) ^ _splitmix64(np.array([seed], dtype=np.uint64) + _GOLDEN)[0]
        bits = _splitmix64(key + np.arange(n * cfg.max_position_embeddings, dtype=np.uint64) * _GOLDEN)
    ids = (bits % np.uint64(cfg.bos_token_id)).astype(np.int64).reshape(n, cfg.max_position_embeddings)
    for i in range(n):
        length = 2 + (i * 5) % 9                 # prompt "" -> BOS EOS; longer ones for the categories
        ids[i, 0] = cfg.bos_token_id
        ids[i, length - 1:] = cfg.eos_token_id
    return ids


def synth_image(n: int, H: int, W: int, seed: int = 5) -> np.ndarray:
    """Smooth synthetic RGB images in [-1, 1] (`to_tensor(img) * 2 - 1`, compute.py:126-132), fp16-representable."""
    z = hash_normal("input.image", n * 3 * H * W, seed).reshape(n, 3, H, W)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    base = np.stack([np.sin(3 * xx + k) * np.cos(2 * yy - k) for k in range(3)])[None]
    img = np.clip(0.6 * base + 0.25 * z, -1.0, 1.0)
    return img.astype(np.float32).astype(np.float16)


def synth_inputs(n_img: int, n_draws: int, h: int, w: int, n_prompts: int = 2,
                 t_min: int = 100, t_max: int = 700, ctx_len: int = 77, ctx_dim: int = 768, latent_dtype=np.float16):
    """Synthetic scoring inputs of SURVEY.md §8d: latents x~N(0,1), eps~N(0,1), t~U{t_min..t_max-1},
    prompt embeddings c~N(0,1), generated by the same integer hash.  `latent_dtype` np.float16: x / eps are
    fp16 arrays; np.float32: the unrounded fp32 values of the same draws (the reference's latents and
    `randn_like` draws are fp32, compute.py:91-93,116).  c is always fp16."""
    x = hash_normal("input.x", n_img * 4 * h * w, 1234).reshape(n_img, 4, h, w)
    eps = hash_normal("input.eps", n_draws * 4 * h * w, 42).reshape(n_draws, 4, h, w)
    with np.errstate(over="ignore"):
        key = np.uint64(fnv1a64("input.t")) ^ _splitmix64(np.array([42], dtype=np.uint64) + _GOLDEN)[0]
        bits = _splitmix64(key + np.arange(n_draws, dtype=np.uint64) * _GOLDEN)
    t = (t_min + (bits >> np.uint64(33)) % np.uint64(t_max - t_min)).astype(np.int64)
    c = hash_normal("input.c", n_prompts * ctx_len * ctx_dim, 7).reshape(n_prompts, ctx_len, ctx_dim)
    f16 = lambda a: a.astype(np.float32).astype(np.float16)
    if latent_dtype == np.float32:
        return x.astype(np.float32), eps.astype(np.float32), t, f16(c)
    return f16(x), f16(eps), t, f16(c)
