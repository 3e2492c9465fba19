"""Shared by the GPU tests of the training operators (test_gpu_train_ops / _blocks / _guards): the cases, the float64 yardstick and the
tolerance rule.

Yardstick: torch.autograd on the CPU in float64 over plain F.conv2d / F.interpolate / F.group_norm / F.silu / F.linear on fp32-valued
inputs from seeded generators.  Rule: the same autograd runs in CPU fp32 too, and the device result must lie within
max(floor, 4 x rel-L2(CPU fp32, float64)) of float64 — floor = 2e-6 for one operator (TOL_OP of tests/test_gpu_f32.py), 2e-5 for a chained
block (TOL_E2E); 4 = the margin tests/umap_cases.py gives a device kernel over the restatement's own fp32-vs-float64 distance.
Every reference is computed once (lru_cache) and never written to."""
import functools

import torch
import torch.nn.functional as F

TOL_OP = 2e-6
TOL_E2E = 2e-5
MARGIN = 4.0


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def check(what, got, ref64, ref32, floor=TOL_OP):
    """prints the three figures (device vs float64, CPU fp32 vs float64, the bound), then asserts the rule"""
    dev, cpu = rel_l2(got, ref64), rel_l2(ref32, ref64)
    bound = max(floor, MARGIN * cpu)
    print(f"TRAIN_OPS {what}: device {dev:.3e}  cpu-fp32 {cpu:.3e}  bound {bound:.3e}")
    assert torch.isfinite(got).all().item(), f"{what}: non-finite values"
    assert dev <= bound, f"{what}: device rel-L2 {dev:.3e} > bound {bound:.3e} (CPU fp32 {cpu:.3e})"
    return dev, cpu, bound


def conv_ref(x, w, b, mode, out_hw):
    if mode == 0:
        return F.conv2d(x, w, b)
    if mode == 1:
        return F.conv2d(x, w, b, padding=1)
    if mode == 2:
        return F.conv2d(x, w, b, stride=2, padding=1)
    return F.conv2d(F.interpolate(x, size=out_hw, mode="nearest"), w, b, padding=1)


# (mode, N, H, W, C1, C2, Cout, out_hw): the smallest shapes that reach each hazard of wgrad32 (and, the same shapes, of the data gradient)
CONV_CASES = [
    (1, 3, 9, 7, 64, 32, 196, None),         # ragged pixel count, odd image, split source, Cout no multiple of any tile
    (1, 1, 1, 1, 32, 0, 32, None),           # eight of nine taps read only halo
    (1, 2, 16, 16, 320, 0, 320, None),       # a real ResNet shape: several slabs, three channel tiles
    (0, 1, 1, 5, 320, 0, 1280, None),        # time_emb_proj: M = 5
    (0, 1, 1, 231, 768, 0, 64, None),        # M = 231: two slabs, the second ragged
    (2, 2, 16, 16, 64, 0, 96, None),
    (2, 1, 9, 7, 32, 0, 36, None),           # stride 2 on an odd image
    (3, 2, 4, 4, 64, 0, 64, (8, 8)),
    (3, 1, 5, 4, 32, 0, 68, (9, 7)),         # upsample_size: not 2x
]


def case_id(c):
    mode, N, H, W, C1, C2, Cout, out_hw = c
    return f"m{mode}-{N}x{H}x{W}-{C1}+{C2}-{Cout}" + (f"-to{out_hw[0]}x{out_hw[1]}" if out_hw else "")


@functools.lru_cache(maxsize=None)
def conv_case(mode, N, H, W, C1, C2, Cout, out_hw):
    """fp32-valued x, w, b, dy (NCHW / diffusers layouts, CPU) and autograd's (dx, dw, db) in float64 and in fp32"""
    cin, k = C1 + C2, 1 if mode == 0 else 3
    x = randn(N, cin, H, W, seed=11)
    w = randn(Cout, cin, k, k, seed=12, scale=(k * k * cin) ** -0.5)
    b = randn(Cout, seed=13)
    out = {"x": x, "w": w, "b": b}
    for name, dt in (("g64", torch.float64), ("g32", torch.float32)):
        xs, ws, bs = (t.to(dt, copy=True).requires_grad_() for t in (x, w, b))
        y = conv_ref(xs, ws, bs, mode, out_hw)
        if "dy" not in out:
            out["dy"] = randn(*y.shape, seed=14)
        out[name] = torch.autograd.grad(y, (xs, ws, bs), out["dy"].to(dt))
    return out


@functools.lru_cache(maxsize=None)
def gn_case(N, H, W, Cc, G, silu, const):
    """x (NCHW; `const`: group 0 of sample 0 holds one value, var = 0), gamma, beta, dy and r64 / r32 = (y, dx, dgamma, dbeta) of
    F.group_norm (+ F.silu) by autograd in float64 / fp32"""
    x = randn(N, Cc, H, W, seed=41) * 2 + 0.5
    if const:
        x[0, : Cc // G] = 1.25
    gamma, beta, dy = 1 + 0.3 * randn(Cc, seed=42), 0.3 * randn(Cc, seed=43), randn(N, Cc, H, W, seed=44)
    out = {"x": x, "gamma": gamma, "beta": beta, "dy": dy}
    for name, dt in (("r64", torch.float64), ("r32", torch.float32)):
        xs, gs, bs = (t.to(dt, copy=True).requires_grad_() for t in (x, gamma, beta))
        y = F.group_norm(xs, G, gs, bs, 1e-5)
        y = F.silu(y) if silu else y
        out[name] = (y.detach(),) + torch.autograd.grad(y, (xs, gs, bs), dy.to(dt))
    return out


def resnet_ref(sd, x, temb, skip, groups=32, eps=1e-5):
    """diffusers ResnetBlock2D (SD 1.5 settings) in plain F.* ops, NCHW; sd in the diffusers names"""
    xc = x if skip is None else torch.cat([x, skip], dim=1)
    h = F.silu(F.group_norm(xc, groups, sd["norm1.weight"], sd["norm1.bias"], eps))
    h = F.conv2d(h, sd["conv1.weight"], sd["conv1.bias"], padding=1)
    h = h + F.linear(F.silu(temb), sd["time_emb_proj.weight"], sd["time_emb_proj.bias"])[:, :, None, None]
    h = F.silu(F.group_norm(h, groups, sd["norm2.weight"], sd["norm2.bias"], eps))
    h = F.conv2d(h, sd["conv2.weight"], sd["conv2.bias"], padding=1)
    res = F.conv2d(xc, sd["conv_shortcut.weight"], sd["conv_shortcut.bias"]) if "conv_shortcut.weight" in sd else xc
    return res + h


def resnet_sd(cin, cout, temb, seed=0):
    """seeded fp32 parameters of one block under the diffusers names (norm weights around 1)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale          # noqa: E731
    sd = {"norm1.weight": 1 + 0.2 * r(cin), "norm1.bias": 0.2 * r(cin), "conv1.weight": r(cout, cin, 3, 3, scale=(9 * cin) ** -0.5),
          "conv1.bias": 0.1 * r(cout), "time_emb_proj.weight": r(cout, temb, scale=temb ** -0.5), "time_emb_proj.bias": 0.1 * r(cout),
          "norm2.weight": 1 + 0.2 * r(cout), "norm2.bias": 0.2 * r(cout), "conv2.weight": r(cout, cout, 3, 3, scale=(9 * cout) ** -0.5),
          "conv2.bias": 0.1 * r(cout)}
    if cin != cout:
        sd["conv_shortcut.weight"], sd["conv_shortcut.bias"] = r(cout, cin, 1, 1, scale=cin ** -0.5), 0.1 * r(cout)
    return sd


# (in, skip, out, N, H, W, temb channels, groups).  16 groups at the 32- and 64-channel shapes: with 32 groups over 32 output channels every
# channel is a group of its own, norm2 then removes any per-sample channel offset, and the float64 gradients of temb, time_emb_proj and
# conv1.bias are exactly zero (round-off of 1e-17 in autograd) — nothing a relative bound can be held against.
RESNET_CASES = [(32, 0, 32, 2, 9, 7, 128, 16), (32, 0, 64, 2, 9, 7, 128, 16), (64, 32, 64, 2, 9, 7, 128, 16), (320, 0, 640, 1, 8, 8, 1280, 32)]


@functools.lru_cache(maxsize=None)
def resnet_case(cin, cskip, cout, N, H, W, tch, groups):
    """inputs, parameters, a seeded upstream gradient and autograd's gradients of everything in float64 and fp32:
    g64 / g32 = {"x", "skip" (or absent), "temb", <parameter names>}; y64 = the float64 output"""
    sd = resnet_sd(cin + cskip, cout, tch, seed=21)
    x, temb = randn(N, cin, H, W, seed=22), randn(N, tch, seed=23)
    skip = randn(N, cskip, H, W, seed=24) if cskip else None
    dy = randn(N, cout, H, W, seed=25)
    out = {"sd": sd, "x": x, "temb": temb, "skip": skip, "dy": dy}
    for name, dt in (("g64", torch.float64), ("g32", torch.float32)):
        leaves = {"x": x, "temb": temb, **sd}
        if skip is not None:
            leaves["skip"] = skip
        leaves = {k: v.to(dt, copy=True).requires_grad_() for k, v in leaves.items()}
        y = resnet_ref({k: leaves[k] for k in sd}, leaves["x"], leaves["temb"], leaves.get("skip"), groups)
        grads = torch.autograd.grad(y, list(leaves.values()), dy.to(dt))
        out[name] = dict(zip(leaves, grads))
        out["y" + name[1:]] = y.detach()
    return out
