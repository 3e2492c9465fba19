"""Shared by tests/test_train_net_cases.py (CPU) and tests/test_gpu_train_net.py, and read by the operator and guard tests of the training
kernels: a miniature U-Net of the training blocks, its float64 yardstick, and the shapes at which a real training step takes the slab
branches of wgrad32, attention backward and LayerNorm backward.

The net composes the existing references only (train_cases.resnet_ref, train_tfm_cases.tfm_ref, F.conv2d stride 2, F.interpolate to a size
+ F.conv2d); parameters live under prefixed diffusers names ("r0.norm1.weight", "a0.transformer_blocks.0.attn1.to_q.weight", ...).

    r0  Resnet 160 -> 160                 a0  Transformer 160, 4 heads (D 40)      s0 = h
    down  Downsample 160 (9 x 7 -> 5 x 4)                                         s1 = h
    r1  Resnet 160 -> 320 (conv_shortcut)  a1  Transformer 320, 4 heads (D 80)      s2 = h
    rm  Resnet 320 -> 320                 am  Transformer 320, 2 heads (D 160)
    u2  Resnet 320 + skip s2 (320) -> 320
    u1  Resnet 320 + skip s1 (160) -> 320     (480 channels / 32 groups = 15 per group: group 21 = channels 315 .. 329 straddles the sources)
    up  Upsample 320 to (9, 7)                (not 2 x the 5 x 4 input)
    u0  Resnet 320 + skip s0 (160) -> 160  a3  Transformer 160, 4 heads

So one temb feeds six time_emb_proj layers, one context four attn2.to_k / to_v pairs, every skip tensor is consumed by the next block and by
an up block, and the residual gradient of a convolution meets a second gradient on the same tensor.  The tolerance rule is
tests/train_cases.py's (float64 autograd the yardstick, CPU fp32 autograd the scale, the device within max(floor, 4 x cpu)); nothing new is
introduced.  Every reference is computed once (lru_cache) and never written to."""
import functools

import torch
import torch.nn.functional as F

from tests.train_cases import MARGIN, TOL_E2E, TOL_OP, check, nchw, nhwc, randn, rel_l2, resnet_ref, resnet_sd  # noqa: F401
from tests.train_tfm_cases import tfm_ref, tfm_sd

N, H, W, H2, W2 = 2, 9, 7, 5, 4
C_LO, C_HI, TEMB, TK, CTX, GROUPS = 160, 320, 128, 77, 96, 32

# name -> ("resnet", in, skip, out) | ("tfm", channels, heads) | ("down", channels) | ("up", channels), in forward order
LAYOUT = [("r0", ("resnet", C_LO, 0, C_LO)), ("a0", ("tfm", C_LO, 4)), ("down", ("down", C_LO)),
          ("r1", ("resnet", C_LO, 0, C_HI)), ("a1", ("tfm", C_HI, 4)),
          ("rm", ("resnet", C_HI, 0, C_HI)), ("am", ("tfm", C_HI, 2)),
          ("u2", ("resnet", C_HI, C_HI, C_HI)), ("u1", ("resnet", C_HI, C_LO, C_HI)), ("up", ("up", C_HI)),
          ("u0", ("resnet", C_HI, C_LO, C_LO)), ("a3", ("tfm", C_LO, 4))]
HEADS = {name: spec[2] for name, spec in LAYOUT if spec[0] == "tfm"}
N_PARAMS, N_LEAVES = 176, 179

# the wiring errors tests/test_train_net_cases.py shows the yardstick to catch
WIRINGS = ("s1_detached_before_u1", "temb_grad_from_r0_alone", "ctx_detached_in_am", "up_to_10x8_and_cropped", "u0_conv2_residual_detached")


def make_block(T, spec):
    """the module of diff_mining_amd.train (passed as `T`) for one LAYOUT entry, on the CPU with its default initialisation"""
    if spec[0] == "resnet":
        return T.ResnetBlock32(spec[1], spec[3], TEMB, skip_channels=spec[2], groups=GROUPS)
    if spec[0] == "tfm":
        return T.Transformer2D32(spec[1], spec[2], CTX, GROUPS)
    return T.Downsample32(spec[1]) if spec[0] == "down" else T.Upsample32(spec[1])


def sub(sd, name):
    """the parameters of block `name` under the block's own (diffusers) names"""
    return {k[len(name) + 1:]: v for k, v in sd.items() if k.startswith(name + ".")}


@functools.lru_cache(maxsize=None)
def net_sd():
    sd = {}
    for i, (name, spec) in enumerate(LAYOUT):
        if spec[0] == "resnet":
            blk = resnet_sd(spec[1] + spec[2], spec[3], TEMB, seed=100 + i)
        elif spec[0] == "tfm":
            blk = tfm_sd(spec[1], CTX, seed=100 + i)
        else:
            c = spec[1]
            blk = {"conv.weight": randn(c, c, 3, 3, seed=100 + i, scale=(9 * c) ** -0.5), "conv.bias": randn(c, seed=200 + i, scale=0.1)}
        sd.update({f"{name}.{k}": v for k, v in blk.items()})
    return sd


def net_ref(sd, x, temb, ctx, wiring=None):
    """the miniature net, NCHW, on parameters of any float dtype.  `wiring`: None, or one of WIRINGS — the same net with that one wiring
    error in its gradient flow (and, for the up-sampler's, in its values)"""
    assert wiring is None or wiring in WIRINGS
    blk = lambda n: sub(sd, n)          # noqa: E731
    t_rest = temb.detach() if wiring == "temb_grad_from_r0_alone" else temb
    h = resnet_ref(blk("r0"), x, temb, None, GROUPS)
    s0 = h = tfm_ref(blk("a0"), h, ctx, HEADS["a0"], GROUPS)
    s1 = h = F.conv2d(h, sd["down.conv.weight"], sd["down.conv.bias"], stride=2, padding=1)
    h = resnet_ref(blk("r1"), h, t_rest, None, GROUPS)
    s2 = h = tfm_ref(blk("a1"), h, ctx, HEADS["a1"], GROUPS)
    h = resnet_ref(blk("rm"), h, t_rest, None, GROUPS)
    h = tfm_ref(blk("am"), h, ctx.detach() if wiring == "ctx_detached_in_am" else ctx, HEADS["am"], GROUPS)
    h = resnet_ref(blk("u2"), h, t_rest, s2, GROUPS)
    h = resnet_ref(blk("u1"), h, t_rest, s1.detach() if wiring == "s1_detached_before_u1" else s1, GROUPS)
    if wiring == "up_to_10x8_and_cropped":
        h = F.conv2d(F.interpolate(h, size=(H + 1, W + 1), mode="nearest"), sd["up.conv.weight"], sd["up.conv.bias"], padding=1)[:, :, :H, :W]
    else:
        h = F.conv2d(F.interpolate(h, size=(H, W), mode="nearest"), sd["up.conv.weight"], sd["up.conv.bias"], padding=1)
    y = resnet_ref(blk("u0"), h, t_rest, s0, GROUPS)
    if wiring == "u0_conv2_residual_detached":          # the same values, without the gradient that conv2's residual input carries
        res = F.conv2d(torch.cat([h, s0], dim=1), sd["u0.conv_shortcut.weight"], sd["u0.conv_shortcut.bias"])
        y = (y - res) + res.detach()
    return tfm_ref(blk("a3"), y, ctx, HEADS["a3"], GROUPS)


@functools.lru_cache(maxsize=None)
def net_inputs():
    return {"x": randn(N, C_LO, H, W, seed=301), "temb": randn(N, TEMB, seed=302), "ctx": randn(N, TK, CTX, seed=303), "dy": randn(N, C_LO, H, W, seed=304)}


def net_grads(dtype, wiring=None):
    """(y, {"x", "temb", "ctx", <176 prefixed parameter names>: gradient}) by autograd in `dtype` for the seeded upstream gradient"""
    k = net_inputs()
    leaves = {n: v.to(dtype, copy=True).requires_grad_() for n, v in {"x": k["x"], "temb": k["temb"], "ctx": k["ctx"], **net_sd()}.items()}
    y = net_ref({n: leaves[n] for n in net_sd()}, leaves["x"], leaves["temb"], leaves["ctx"], wiring)
    grads = torch.autograd.grad(y, list(leaves.values()), k["dy"].to(dtype), allow_unused=wiring is not None)
    return y.detach(), {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in zip(leaves, grads)}


@functools.lru_cache(maxsize=None)
def net_case():
    """sd, x, temb, ctx, dy (fp32-valued, NCHW, CPU) and g64 / g32 = the gradients of all 179 leaves, y64 / y32 = the output"""
    out = {"sd": net_sd(), **net_inputs()}
    out["y64"], out["g64"] = net_grads(torch.float64)
    out["y32"], out["g32"] = net_grads(torch.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the partition rules of DESIGN 4ab / 4ac, restated in plain Python: (slabs, slab length, population of every slab)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _populations(total, slabs, length):
    return [max(0, min(total, (s + 1) * length) - s * length) for s in range(slabs)]


def wgrad_slab_rule(M):
    """M < 8192: min(4, ceil(M / 128)); from 8192 on: min(16, floor(M / 2048)); slab length ceil(M / slabs) rounded up to 32"""
    slabs = max(1, min(4, -(-M // 128)) if M < 8192 else min(16, M // 2048))
    length = -(-(-(-M // slabs)) // 32) * 32
    return slabs, length, _populations(M, slabs, length)


def attn_slab_rule(Tq, Tk):
    """Tk > 128: 1; otherwise min(16, ceil(Tq / 512)); slab length ceil(Tq / slabs) rounded up to 64 (a trailing slab may be empty)"""
    slabs = 1 if Tk > 128 else max(1, min(16, -(-Tq // 512)))
    length = -(-(-(-Tq // slabs)) // 64) * 64
    return slabs, length, _populations(Tq, slabs, length)


def ln_slab_rule(rows):
    """min(64, ceil(rows / 256)) slabs of ceil(rows / slabs) rows"""
    slabs = max(1, min(64, -(-rows // 256)))
    length = -(-rows // slabs)
    return slabs, length, _populations(rows, slabs, length)


def conv_pixels(c):
    """M = N OH OW of a CONV_CASES tuple"""
    mode, n, h, w, _, _, _, out_hw = c
    oh, ow = (h, w) if mode in (0, 1) else ((h + 1) // 2, (w + 1) // 2) if mode == 2 else out_hw
    return n * oh * ow


# (mode, N, H, W, C1, C2, Cout, out_hw) -> (slabs, slab length, population of the last slab): the branches of wgrad_slabs a training step
# takes and tests/train_cases.py's CONV_CASES (at most 512 pixels) stay below
NET_CONV_PARTITIONS = {
    (0, 1, 1, 8191, 32, 0, 32, None): (4, 2048, 2047),           # the last M of the small branch
    (0, 1, 1, 8197, 32, 0, 36, None): (4, 2080, 1957),           # M >= 8192, a slab length that was rounded up, Cout no multiple of 32
    (0, 1, 1, 16384, 64, 0, 32, None): (8, 2048, 2048),          # the 64^2 level of a batch of 4
    (0, 1, 1, 32805, 32, 0, 32, None): (16, 2080, 1605),         # the cap of 16 binds
    (1, 2, 64, 65, 32, 32, 32, None): (4, 2080, 2080),           # M = 8320: taps cross the slab and the sample boundaries; two sources
    (2, 2, 128, 130, 32, 0, 32, None): (4, 2080, 2080),          # M = 8320, stride 2
    (3, 2, 32, 33, 32, 0, 32, (64, 65)): (4, 2080, 2080),        # M = 8320, nearest up-sampling
}
NET_CONV_CASES = list(NET_CONV_PARTITIONS)
CONV_16_SLABS = NET_CONV_CASES[3]

# (B, heads, Tq, Tk, D, q-scale) -> (slabs, slab length, {slab: population} for the slabs the case is about)
NET_ATTN_PARTITIONS = {
    (1, 1, 8200, 77, 40, 1): (16, 576, {13: 576, 14: 136, 15: 0}),      # the cap binds: slab 15 starts past Tq and must write zeros
    (1, 1, 4097, 77, 80, 1): (9, 512, {7: 512, 8: 1}),                  # a slab that holds one query
    (4, 8, 70, 70, 40, 1): (1, 128, {0: 70}),                           # the real B * heads = 32
}
NET_ATTN_CASES = list(NET_ATTN_PARTITIONS)
ATTN_EMPTY_SLAB = NET_ATTN_CASES[0]

# (rows, C, constant row) -> (slabs, slab length, population of the last slab): the cap of 64 (rows > 16 384)
NET_LN_PARTITIONS = {(16391, 320, False): (64, 257, 200)}
NET_LN_CASES = list(NET_LN_PARTITIONS)

# (N, H, W, C1, C2, G, silu, const): the up blocks' norm1 — channels per group that do not divide the block's 256 threads, and a group
# across the C1 | C2 boundary
NET_GN_CASES = [
    (1, 2, 3, 1280, 640, 32, True, False),        # 60 per group (4 pixel lanes, 16 threads idle); group 21 = channels 1260 .. 1319
    (1, 2, 3, 640, 320, 32, True, False),         # 30 per group; group 21 = channels 630 .. 659
    (2, 1, 2, 1280, 1280, 32, True, False),       # 80 per group: 3 pixel lanes, 240 live threads
    (1, 3, 3, 320, 320, 32, False, False),        # 20 per group, without SiLU
]
