"""Differentiable blocks of the fp32 net: ResnetBlock2D, Downsample2D, Upsample2D (part 1) and, further down, the transformer blocks
(part 2: LayerNorm, self- and cross-attention, GEGLU, proj_in / proj_out; BasicTransformerBlock32, Transformer2D32), with gradients.

PyTorch does the plumbing — autograd orders the calls, allocates the tensors and adds into `.grad` —, every FLOP runs in the library:
the forward pass is the inference operators (dm_f32_op_gemm, dm_f32_op_groupnorm, dm_f32_op_silu: the same bits), the backward pass

  weight gradient   dm_f32_op_gemm_wgrad: dWp[co][tap Cin + ci] = sum over output pixels of dY (x) im2col(X), in gemm32's weight layout
  data gradient     dm_f32_op_gemm again, on repacked weights (dgrad_weights): W'[ci][8 - tap][co] = W[co][tap][ci]
                      mode 0 (linear / 1x1)      mode 0 with W^T
                      mode 1 (3x3, pad 1)        mode 1 on dY
                      mode 2 (3x3, stride 2)     dm_f32_op_zero_insert2 (Z[2 oy][2 ox] = dY[oy][ox]), then mode 1
                      mode 3 (nearest + 3x3)     mode 1 at (OH, OW), then dm_f32_op_nearest_bwd
                    a concatenated input X | X2 gets its two gradients from the two row ranges of W', one launch each
  bias, temb        dm_f32_op_colsum (all rows / per sample)
  GroupNorm (+SiLU) dm_f32_op_groupnorm_bwd from the forward pass's (mean, rstd); SiLU: dm_f32_op_silu_bwd

All tensors are NHWC fp32 on the GPU.  The pure-torch helpers at the end (dgrad_weights, zero_insert2_host, nearest_bwd_host,
wgrad_host, groupnorm_bwd_host) restate the rules on any device, so a machine without a GPU can check them against autograd.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .engine import EngineError, _p, load_library as _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise EngineError(f"{what} refused its arguments")


def _f32c(t: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda:
        raise EngineError(f"{what}: an fp32 CUDA tensor is required (got {t.dtype} on {t.device})")
    return t.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# pure-torch rules (any device, any float dtype)
# ---------------------------------------------------------------------------------------------------------------------------------------
def taps_of(mode: int) -> int:
    if mode not in (0, 1, 2, 3):
        raise ValueError(f"mode {mode}: 0 (dense / 1x1), 1 (3x3), 2 (3x3 stride 2) or 3 (nearest + 3x3)")
    return 1 if mode == 0 else 9


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """diffusers [Cout,Cin,kh,kw] (or a Linear's [Cout,Cin]) -> gemm32's [Cout][taps*Cin], k = (tap, cin)"""
    if w.dim() == 2:
        return w.contiguous()
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def unpack_conv(wp: torch.Tensor, taps: int) -> torch.Tensor:
    """the inverse of pack_conv: [Cout][taps*Cin] -> [Cout,Cin,3,3] (taps = 9) or [Cout,Cin,1,1] (taps = 1)"""
    k = 3 if taps == 9 else 1
    return wp.reshape(wp.shape[0], k, k, wp.shape[1] // taps).permute(0, 3, 1, 2).contiguous()


def dgrad_weights(wp: torch.Tensor, mode: int, pad_to: int = 1) -> torch.Tensor:
    """The weights that turn the data gradient into a forward convolution of dY: packed [Cout][taps*Cin] -> packed [Cin][taps*CoutP],
    W'[ci][8 - tap][co] = W[co][tap][ci] (mode 0: the transpose).  CoutP = Cout rounded up to `pad_to` with zero columns: gemm32 reads
    its input channels in chunks of 32, so a dY of another width is zero-padded to match."""
    taps = taps_of(mode)
    cout, cin = wp.shape[0], wp.shape[1] // taps
    coutp = (cout + pad_to - 1) // pad_to * pad_to
    w3 = wp.reshape(cout, taps, cin).flip(1).permute(2, 1, 0)          # [ci][8 - tap][co]
    out = wp.new_zeros(cin, taps, coutp)
    out[:, :, :cout] = w3
    return out.reshape(cin, taps * coutp)


def nearest_index(out: int, inp: int, device=None) -> torch.Tensor:
    """src = min(floor(dst * (float)in / (float)out), in - 1) in fp32: F.interpolate(mode="nearest") and gemm32's mode 3"""
    scale = torch.tensor(float(inp), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    idx = (torch.arange(out, dtype=torch.float32) * scale).floor().long().clamp(max=inp - 1)
    return idx.to(device) if device is not None else idx


def zero_insert2_host(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """dY [N,OH,OW,C] of a stride-2 pad-1 3x3 convolution of an H x W image -> Z [N,H,W,C] with Z[2 oy][2 ox] = dY[oy][ox]"""
    N, OH, OW, Cc = dy.shape
    assert OH == (H + 1) // 2 and OW == (W + 1) // 2, (OH, OW, H, W)
    z = dy.new_zeros(N, H, W, Cc)
    z[:, ::2, ::2] = dy
    return z


def nearest_bwd_host(du: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """dU [N,OH,OW,C] -> dS [N,H,W,C]: every source pixel sums its pre-image under nearest_index (rows, then columns, ascending)"""
    N, OH, OW, Cc = du.shape
    rows = du.new_zeros(N, H, OW, Cc).index_add_(1, nearest_index(OH, H, du.device), du)
    return du.new_zeros(N, H, W, Cc).index_add_(2, nearest_index(OW, W, du.device), rows)


def _im2col_tap(x: torch.Tensor, tap: int, mode: int, OH: int, OW: int) -> torch.Tensor:
    """x [N,H,W,C] -> the pixels tap (dy, dx) of a mode-`mode` convolution reads, [N,OH,OW,C], zeros outside the image"""
    N, H, W, Cc = x.shape
    if mode == 0:
        return x
    dy, dx = tap // 3, tap % 3
    if mode == 3:
        x = x[:, nearest_index(OH, H, x.device)][:, :, nearest_index(OW, W, x.device)]
        H, W = OH, OW
    st = 2 if mode == 2 else 1
    iy = torch.arange(OH, device=x.device) * st + dy - 1
    ix = torch.arange(OW, device=x.device) * st + dx - 1
    oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
    g = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
    return g * (oky[:, None] & okx[None, :]).to(x.dtype)[None, :, :, None]


def wgrad_host(x: torch.Tensor, x2: Optional[torch.Tensor], dy: torch.Tensor, mode: int, out_hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The weight gradient in float64 by plain indexing (no autograd): dWp [Cout][taps*Cin], k = (tap, cin), of the convolution
    dm_f32_op_gemm computes in `mode` on cat([x, x2], channels) with upstream gradient dy [N,OH,OW,Cout] (mode 0: any [..., Cout])."""
    xs = (x if x2 is None else torch.cat([x, x2], dim=-1)).double()
    dyd = dy.double()
    cout = dyd.shape[-1]
    if mode == 0:
        return dyd.reshape(-1, cout).t() @ xs.reshape(-1, xs.shape[-1])
    OH, OW = (dyd.shape[1], dyd.shape[2]) if out_hw is None else out_hw
    assert dyd.shape[1:3] == (OH, OW)
    cols = [torch.einsum("nyxo,nyxi->oi", dyd, _im2col_tap(xs, tap, mode, OH, OW)) for tap in range(9)]
    return torch.stack(cols, dim=1).reshape(cout, -1)


def groupnorm_bwd_host(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool):
    """GroupNorm (+ SiLU) backward restated in float64 on NHWC x, dy [N,H,W,C] -> (dx, dgamma, dbeta): the formula of the device kernels,
    dx = rstd (dz gamma - mean(dz gamma) - xhat mean(dz gamma xhat)) with the means over each (sample, group)"""
    x, dy, gamma, beta = x.double(), dy.double(), gamma.double(), beta.double()
    N, H, W, Cc = x.shape
    xg = x.reshape(N, H * W, groups, Cc // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = ((xg - mean) * rstd).reshape(N, H, W, Cc)
    dz = dy
    if silu:
        z = xh * gamma + beta
        s = torch.sigmoid(z)
        dz = dy * (s * (1 + z * (1 - s)))
    dgamma, dbeta = (dz * xh).sum(dim=(0, 1, 2)), dz.sum(dim=(0, 1, 2))
    dzg = (dz * gamma).reshape(N, H * W, groups, Cc // groups)
    xhg = xh.reshape(N, H * W, groups, Cc // groups)
    dx = rstd * (dzg - dzg.mean(dim=(1, 3), keepdim=True) - xhg * (dzg * xhg).mean(dim=(1, 3), keepdim=True))
    return dx.reshape(N, H, W, Cc), dgamma, dbeta


# ---------------------------------------------------------------------------------------------------------------------------------------
# device operators (thin calls of the C ABI on the current stream)
# ---------------------------------------------------------------------------------------------------------------------------------------
def gemm32(x, x2, wp, bias, temb, res, mode: int, out_hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """dm_f32_op_gemm: x [N,H,W,C1] (| x2 [N,H,W,C2]), wp [Cout][taps*(C1+C2)] -> [N,OH,OW,Cout] (+ bias, + temb[n], + res)"""
    N, H, W, C1 = x.shape
    cin = C1 + (x2.shape[3] if x2 is not None else 0)
    cout = wp.shape[0]
    if wp.shape[1] != taps_of(mode) * cin:
        raise EngineError(f"conv32: weights {tuple(wp.shape)} do not fit mode {mode} on {cin} channels")
    OH, OW = (H, W) if mode in (0, 1) else ((H + 1) // 2, (W + 1) // 2) if mode == 2 else (out_hw if out_hw is not None else (2 * H, 2 * W))
    y = torch.empty(N, OH, OW, cout, dtype=torch.float32, device=x.device)
    if temb is not None and (temb.stride(1) != 1 or temb.shape[0] != N):
        raise EngineError("conv32: temb must be [N, Cout] with unit channel stride")
    _check(_lib().dm_f32_op_gemm(_stream(), _p(x), _p(x2), _p(wp), _p(bias), _p(temb), _p(res), _p(y), N, H, W, OH, OW, cin, C1, cout, mode,
                                 temb.stride(0) if temb is not None else 0), "dm_f32_op_gemm")
    return y


def wgrad32(x, x2, dy, mode: int, out_hw: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """dm_f32_op_gemm_wgrad: the packed weight gradient [Cout][taps*Cin]; `out` + accumulate adds into an existing gradient"""
    lib = _lib()
    N, H, W, C1 = x.shape
    cin = C1 + (x2.shape[3] if x2 is not None else 0)
    cout = dy.shape[-1]
    OH, OW = (H, W) if mode in (0, 1) else (dy.shape[1], dy.shape[2])
    if out_hw is not None and mode == 3 and tuple(out_hw) != (OH, OW):
        raise EngineError("wgrad32: dy does not have the given output size")
    nbytes = lib.dm_f32_op_gemm_wgrad_workspace(N, H, W, OH, OW, cin, cout, mode)
    if nbytes == 0:
        raise EngineError("dm_f32_op_gemm_wgrad_workspace refused its arguments")
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    if out is None:
        out = torch.empty(cout, taps_of(mode) * cin, dtype=torch.float32, device=x.device)
        accumulate = False
    _check(lib.dm_f32_op_gemm_wgrad(_stream(), _p(x), _p(x2), _p(dy), _p(out), _p(work), nbytes, N, H, W, OH, OW, cin, C1, cout, mode,
                                    1 if accumulate else 0), "dm_f32_op_gemm_wgrad")
    return out


def colsum32(dy: torch.Tensor, per_sample: bool) -> torch.Tensor:
    """dy [N, ..., C] -> [N, C] (per sample) or [C] (all rows)"""
    Cc = dy.shape[-1]
    n = dy.shape[0] if per_sample else 1
    hw = dy.numel() // (n * Cc)
    out = torch.empty(n, Cc, dtype=torch.float32, device=dy.device)
    _check(_lib().dm_f32_op_colsum(_stream(), _p(dy), n, hw, Cc, 0, _p(out)), "dm_f32_op_colsum")
    return out if per_sample else out[0]


def zero_insert2(dy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    N, OH, OW, Cc = dy.shape
    if OH != (H + 1) // 2 or OW != (W + 1) // 2:
        raise EngineError("zero_insert2: dy is not the stride-2 output of an H x W image")
    z = torch.empty(N, H, W, Cc, dtype=torch.float32, device=dy.device)
    _check(_lib().dm_f32_op_zero_insert2(_stream(), _p(dy), N, H, W, Cc, _p(z)), "dm_f32_op_zero_insert2")
    return z


def nearest_bwd(du: torch.Tensor, H: int, W: int) -> torch.Tensor:
    N, OH, OW, Cc = du.shape
    ds = torch.empty(N, H, W, Cc, dtype=torch.float32, device=du.device)
    _check(_lib().dm_f32_op_nearest_bwd(_stream(), _p(du), N, H, W, OH, OW, Cc, _p(ds)), "dm_f32_op_nearest_bwd")
    return ds


def dgrad32(dy: torch.Tensor, wp: torch.Tensor, mode: int, x_shape, C1: int):
    """The data gradient of dm_f32_op_gemm in `mode`: (dX [N,H,W,C1], dX2 [N,H,W,Cin-C1] or None), each one forward gemm32 launch on
    the row range of dgrad_weights(wp) that belongs to it."""
    N, H, W = x_shape[0], x_shape[1], x_shape[2]
    cout = dy.shape[-1]
    wd = dgrad_weights(wp, mode, pad_to=32)
    cin = wd.shape[0]
    coutp = wd.shape[1] // taps_of(mode)
    if coutp != cout:
        dy = F.pad(dy, (0, coutp - cout))
    if mode == 2:
        dy = zero_insert2(dy, H, W)
    outs = []
    for lo, hi in ((0, C1), (C1, cin)):
        if hi == lo:
            outs.append(None)
            continue
        g = gemm32(dy, None, wd[lo:hi], None, None, None, 0 if mode == 0 else 1)
        outs.append(nearest_bwd(g, H, W) if mode == 3 else g)
    return outs[0], outs[1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Conv32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, wp, bias, temb, res, mode, out_hw):
        x, x2, wp, bias, res = (_f32c(t, "conv32") for t in (x, x2, wp, bias, res))
        if temb is not None and temb.stride(-1) != 1:
            temb = temb.contiguous()
        y = gemm32(x, x2, wp, bias, temb, res, mode, out_hw)
        ctx.save_for_backward(x, x2, wp)
        ctx.mode, ctx.has = mode, (bias is not None, temb is not None, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, x2, wp = ctx.saved_tensors
        dy = dy.contiguous()
        need = ctx.needs_input_grad
        dx = dx2 = dw = db = dt = dr = None
        if need[0] or (x2 is not None and need[1]):
            dx, dx2 = dgrad32(dy, wp, ctx.mode, x.shape, x.shape[3])
        if need[2]:
            dw = wgrad32(x, x2, dy, ctx.mode)
        if ctx.has[0] and need[3]:
            db = colsum32(dy, per_sample=False)
        if ctx.has[1] and need[4]:
            dt = colsum32(dy, per_sample=True)
        if ctx.has[2] and need[5]:
            dr = dy
        return dx, dx2, dw, db, dt, dr, None, None


def conv32(x, x2, w_packed, bias, temb, res, mode: int, out_hw: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """y = conv(cat([x, x2])) + bias + temb[n] + res as dm_f32_op_gemm computes it, differentiable in every tensor argument.
    x [N,H,W,C1], x2 [N,H,W,C2] or None, w_packed [Cout][taps*Cin], bias [Cout], temb [N,Cout], res [N,OH,OW,Cout]."""
    return _Conv32.apply(x, x2, w_packed, bias, temb, res, mode, out_hw)


def linear32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """F.linear on x [M, Cin] with w [Cout, Cin] (mode 0)"""
    M, cin = x.shape
    return conv32(x.reshape(1, 1, M, cin), None, w, bias, None, None, 0).reshape(M, w.shape[0])


class _GroupNormSilu32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, gamma, beta, groups, eps, silu):
        x, x2, gamma, beta = (_f32c(t, "groupnorm_silu32") for t in (x, x2, gamma, beta))
        N, H, W, C1 = x.shape
        Cc = C1 + (x2.shape[3] if x2 is not None else 0)
        stats = torch.empty(N * groups, 2, dtype=torch.float32, device=x.device)
        y = torch.empty(N, H, W, Cc, dtype=torch.float32, device=x.device)
        _check(_lib().dm_f32_op_groupnorm(_stream(), _p(x), _p(x2), N, H * W, Cc, C1, groups, eps, _p(gamma), _p(beta), 1 if silu else 0,
                                          _p(stats), _p(y)), "dm_f32_op_groupnorm")
        ctx.save_for_backward(x, x2, gamma, beta, stats)
        ctx.groups, ctx.silu = groups, silu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, x2, gamma, beta, stats = ctx.saved_tensors
        dy = dy.contiguous()
        N, H, W, C1 = x.shape
        Cc = dy.shape[3]
        G = ctx.groups
        work = torch.empty(2 * (N * Cc + N * G), dtype=torch.float64, device=x.device)
        dx = torch.empty_like(x)
        dx2 = torch.empty_like(x2) if x2 is not None else None
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        _check(_lib().dm_f32_op_groupnorm_bwd(_stream(), _p(x), _p(x2), _p(dy), N, H * W, Cc, C1, G, _p(gamma), _p(beta), _p(stats),
                                              1 if ctx.silu else 0, _p(work), work.numel() * 8, _p(dx), _p(dx2), _p(dg), _p(db)),
               "dm_f32_op_groupnorm_bwd")
        return dx, dx2, dg, db, None, None, None


def groupnorm_silu32(x, x2, gamma, beta, groups: int, eps: float, silu: bool) -> torch.Tensor:
    """GroupNorm over cat([x, x2], channels) (+ SiLU), NHWC, as dm_f32_op_groupnorm; differentiable in x, x2, gamma, beta"""
    return _GroupNormSilu32.apply(x, x2, gamma, beta, groups, eps, silu)


class _Silu32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x, "silu32")
        y = torch.empty_like(x)
        _check(_lib().dm_f32_op_silu(_stream(), _p(x), _p(y), x.numel()), "dm_f32_op_silu")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _check(_lib().dm_f32_op_silu_bwd(_stream(), _p(x), _p(dy), _p(dx), x.numel()), "dm_f32_op_silu_bwd")
        return dx


def silu32(x: torch.Tensor) -> torch.Tensor:
    return _Silu32.apply(x)


# ---------------------------------------------------------------------------------------------------------------------------------------
# modules: parameters live in the packed layout, state dicts speak the diffusers names and shapes of one block
# ---------------------------------------------------------------------------------------------------------------------------------------
class _Block32(nn.Module):
    """_convs: diffusers conv name -> taps.  Every other parameter keeps its diffusers shape; a conv / linear `name` is held as the
    parameters `name_weight` (packed) and `name_bias`, a norm as `name_weight` / `name_bias`."""
    _convs: dict = {}

    def _names(self):
        for pname, _ in self.named_parameters(recurse=False):
            layer, kind = pname.rsplit("_", 1)
            yield pname, f"{layer}.{kind}", (self._convs.get(layer) if kind == "weight" else None)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for pname, key, taps in self._names():
            t = getattr(self, pname)
            t = t if keep_vars else t.detach()
            out[prefix + key] = unpack_conv(t, taps) if taps in (1, 9) else t if keep_vars else t.clone()
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        want = {key: (pname, taps) for pname, key, taps in self._names()}
        missing, unexpected = sorted(set(want) - set(state_dict)), sorted(set(state_dict) - set(want))
        if strict and (missing or unexpected):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing}, unexpected {unexpected}")
        with torch.no_grad():
            for key, (pname, taps) in want.items():
                if key not in state_dict:
                    continue
                p = getattr(self, pname)
                v = torch.as_tensor(state_dict[key])
                v = pack_conv(v) if taps in (1, 9) else v
                if tuple(v.shape) != tuple(p.shape):
                    raise RuntimeError(f"{key}: shape {tuple(state_dict[key].shape)} does not fit this block")
                p.copy_(v.to(p.dtype))
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def grad_dict(self) -> "OrderedDict[str, Optional[torch.Tensor]]":
        """the parameters' `.grad` under the diffusers names and shapes"""
        out = OrderedDict()
        for pname, key, taps in self._names():
            g = getattr(self, pname).grad
            out[key] = None if g is None else unpack_conv(g, taps) if taps in (1, 9) else g
        return out

    def _conv_params(self, name: str, cout: int, cin: int, taps: int) -> None:
        w = torch.empty(cout, taps * cin)
        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
        bound = (taps * cin) ** -0.5
        self.register_parameter(f"{name}_weight", nn.Parameter(w))
        self.register_parameter(f"{name}_bias", nn.Parameter(torch.empty(cout).uniform_(-bound, bound)))

    def _norm_params(self, name: str, c: int) -> None:
        self.register_parameter(f"{name}_weight", nn.Parameter(torch.ones(c)))
        self.register_parameter(f"{name}_bias", nn.Parameter(torch.zeros(c)))


class ResnetBlock32(_Block32):
    """diffusers ResnetBlock2D (SD 1.5 settings: SiLU, time embedding added after conv1, output scale 1) on NHWC fp32:
    forward(x [N,H,W,in], temb [N,temb_channels], skip [N,H,W,skip_channels] or None) -> [N,H,W,out].  `skip` is the up block's
    second source: the block normalises and convolves cat([x, skip]) without building it.  conv_shortcut exists when
    in + skip != out (state-dict keys norm1.weight ... conv_shortcut.bias)."""
    _convs = {"conv1": 9, "conv2": 9, "conv_shortcut": 1, "time_emb_proj": 0}

    def __init__(self, in_channels: int, out_channels: int, temb_channels: int, skip_channels: int = 0, groups: int = 32, eps: float = 1e-5):
        super().__init__()
        cin = in_channels + skip_channels
        self.in_channels, self.skip_channels, self.out_channels, self.groups, self.eps = in_channels, skip_channels, out_channels, groups, eps
        self._norm_params("norm1", cin)
        self._conv_params("conv1", out_channels, cin, 9)
        self._conv_params("time_emb_proj", out_channels, temb_channels, 1)
        self._norm_params("norm2", out_channels)
        self._conv_params("conv2", out_channels, out_channels, 9)
        self.has_shortcut = cin != out_channels
        if self.has_shortcut:
            self._conv_params("conv_shortcut", out_channels, cin, 1)

    def forward(self, x, temb, skip=None):
        if (skip is None) != (self.skip_channels == 0):
            raise EngineError("ResnetBlock32: a skip source is expected exactly when skip_channels > 0")
        h = groupnorm_silu32(x, skip, self.norm1_weight, self.norm1_bias, self.groups, self.eps, True)
        t = linear32(silu32(temb), self.time_emb_proj_weight, self.time_emb_proj_bias)
        h = conv32(h, None, self.conv1_weight, self.conv1_bias, t, None, 1)
        h = groupnorm_silu32(h, None, self.norm2_weight, self.norm2_bias, self.groups, self.eps, True)
        res = conv32(x, skip, self.conv_shortcut_weight, self.conv_shortcut_bias, None, None, 0) if self.has_shortcut else x
        return conv32(h, None, self.conv2_weight, self.conv2_bias, None, res, 1)


class Downsample32(_Block32):
    """diffusers Downsample2D (conv 3x3, stride 2, pad 1): [N,H,W,C] -> [N,(H+1)/2,(W+1)/2,C]; state-dict keys conv.weight, conv.bias"""
    _convs = {"conv": 9}

    def __init__(self, channels: int):
        super().__init__()
        self._conv_params("conv", channels, channels, 9)

    def forward(self, x):
        return conv32(x, None, self.conv_weight, self.conv_bias, None, None, 2)


class Upsample32(_Block32):
    """diffusers Upsample2D (nearest to 2x, or to `out_hw` = upsample_size, then conv 3x3 pad 1); state-dict keys conv.weight, conv.bias"""
    _convs = {"conv": 9}

    def __init__(self, channels: int):
        super().__init__()
        self._conv_params("conv", channels, channels, 9)

    def forward(self, x, out_hw: Optional[Tuple[int, int]] = None):
        return conv32(x, None, self.conv_weight, self.conv_bias, None, None, 3, out_hw)


# =======================================================================================================================================
# part 2: the transformer blocks — LayerNorm, self- and cross-attention, GEGLU, proj_in / proj_out
# =======================================================================================================================================
# The linear layers are linear32 (conv32 in mode 0): forward dm_f32_op_gemm, weight gradient dm_f32_op_gemm_wgrad, data gradient
# dm_f32_op_gemm on W^T, bias dm_f32_op_colsum.  Three gradients have kernels of their own:
#   attention  dm_f32_op_attention_bwd: dQ, dK, dV on the stacked q|k|v rows [tokens][3C] (self) or q [tokens][C] and k|v [B Tk][2C] (cross)
#              in place, so one weight-gradient call serves a stacked projection
#   LayerNorm  dm_f32_op_layernorm_bwd (mean / rstd recomputed: the forward pass saves nothing)
#   GEGLU      the training forward pass of ff.net.0 is the plain GEMM on the [2F][C] weight (P = h | g, kept for the backward pass), then
#              dm_f32_op_geglu; dm_f32_op_geglu_bwd gives dP
LOG2E = 1.4426950408889634


def attention_host(q, k, v, heads: int):
    """softmax(q k^T / sqrt(D)) v per head with plain torch ops: q [B,Tq,C], k, v [B,Tk,C] -> [B,Tq,C]"""
    B, Tq, Cc = q.shape
    D = Cc // heads
    qh, kh, vh = (t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, Tq, Cc)


def attention_bwd_host(q, k, v, do, heads: int):
    """The device kernels' rule without autograd, on any device and float dtype: (dq, dk, dv, L, delta) with
    L [B,heads,Tq] = log2 sum_k 2^(s scale log2 e), delta = sum_d dO O, P = 2^(s' - L), dS = P (dP - delta), dQ = dS K scale,
    dK = dS^T Q scale, dV = P^T dO"""
    B, Tq, Cc = q.shape
    D = Cc // heads
    scale = D ** -0.5
    qh, kh, vh, doh = (t.reshape(B, t.shape[1], heads, D).transpose(1, 2) for t in (q, k, v, do))
    s2 = qh @ kh.transpose(-1, -2) * (scale * LOG2E)
    L = torch.logsumexp(s2 / LOG2E, dim=-1) * LOG2E
    p = torch.exp2(s2 - L[..., None])
    o = p @ vh
    delta = (doh * o).sum(-1)
    ds = p * (doh @ vh.transpose(-1, -2) - delta[..., None])
    dq, dk, dv = ds @ kh * scale, ds.transpose(-1, -2) @ qh * scale, p.transpose(-1, -2) @ doh
    back = lambda t: t.transpose(1, 2).reshape(B, t.shape[2], Cc)          # noqa: E731
    return back(dq), back(dk), back(dv), L, delta


def layernorm_bwd_host(x, dy, gamma, eps: float):
    """LayerNorm backward over the last axis: dx = rstd (dy gamma - mean(dy gamma) - xhat mean(dy gamma xhat)), dgamma = sum dy xhat,
    dbeta = sum dy over all rows"""
    mean = x.mean(-1, keepdim=True)
    rstd = (((x - mean) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    rows = tuple(range(x.dim() - 1))
    return dx, (dy * xh).sum(rows), dy.sum(rows)


def _gelu_parts(g):
    cdf = 0.5 * (1 + torch.erf(g * 0.7071067811865476))
    return g * cdf, cdf + g * torch.exp(-0.5 * g * g) * 0.3989422804014327


def geglu_host(p):
    """P [..., 2F] = (h | g) -> h gelu(g) (erf GELU)"""
    h, g = p.chunk(2, dim=-1)
    return h * _gelu_parts(g)[0]


def geglu_bwd_host(p, dy):
    """dP = (dy gelu(g) | dy h (Phi(g) + g phi(g)))"""
    h, g = p.chunk(2, dim=-1)
    gelu, dgelu = _gelu_parts(g)
    return torch.cat([dy * gelu, dy * h * dgelu], dim=-1)


# ---- device operators ------------------------------------------------------------------------------------------------------------------
def _attn_args(ts, B):
    """row and batch strides (elements) of [B, T, width] views with a unit last stride"""
    for t in ts:
        if t.dim() != 3 or t.shape[0] != B or t.stride(2) != 1 or (B > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise EngineError("attention32: operands must be [B, T, C] views of row-major rows")
    return [t.stride(1) for t in ts], [t.shape[1] * t.stride(1) for t in ts]


def attention_fwd32(q, k, v, heads: int) -> torch.Tensor:
    """dm_f32_op_attention on [B,T,C] views (slices of stacked rows are read in place) -> O [B,Tq,C]"""
    B, Tq, Cc = q.shape
    Tk, D = k.shape[1], Cc // heads
    o = torch.empty(B, Tq, Cc, dtype=torch.float32, device=q.device)
    ld, bs = _attn_args((q, k, v, o), B)
    _check(_lib().dm_f32_op_attention(_stream(), _p(q), _p(k), _p(v), _p(o), *ld, *bs, None, 0, B, heads, Tq, Tk, D, D ** -0.5), "dm_f32_op_attention")
    return o


def attention_bwd32(q, k, v, o, do, dq, dk, dv, heads: int, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dm_f32_op_attention_bwd into the views dq, dk, dv; returns the workspace (it starts with (L, delta) [B,heads,Tq,2])"""
    lib = _lib()
    B, Tq, Cc = q.shape
    Tk, D = k.shape[1], Cc // heads
    nbytes = lib.dm_f32_op_attention_bwd_workspace(B, heads, Tq, Tk, D)
    if nbytes == 0:
        raise EngineError("dm_f32_op_attention_bwd_workspace refused its arguments")
    if work is None:
        work = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    ld, bs = _attn_args((q, k, v, o, do, dq, dk, dv), B)
    _check(lib.dm_f32_op_attention_bwd(_stream(), _p(q), _p(k), _p(v), _p(o), _p(do), _p(dq), _p(dk), _p(dv), (C.c_int32 * 8)(*ld), (C.c_int64 * 8)(*bs), None,
                                       B, heads, Tq, Tk, D, D ** -0.5, _p(work), work.numel() * work.element_size()), "dm_f32_op_attention_bwd")
    return work


class _Attention32(torch.autograd.Function):
    """layout 0: (q, k, v) separate [B,T,C]; 1: a = stacked q|k|v [B,T,3C]; 2: a = q [B,Tq,C], b = stacked k|v [B,Tk,2C]"""
    @staticmethod
    def _views(layout, a, b, c):
        if layout == 0:
            return a, b, c
        Cc = a.shape[-1] // 3 if layout == 1 else a.shape[-1]
        if layout == 1:
            return a[..., :Cc], a[..., Cc:2 * Cc], a[..., 2 * Cc:]
        return a, b[..., :Cc], b[..., Cc:]

    @staticmethod
    def forward(ctx, a, b, c, heads, layout):
        a, b, c = (_f32c(t, "attention32") for t in (a, b, c))
        q, k, v = _Attention32._views(layout, a, b, c)
        o = attention_fwd32(q, k, v, heads)
        ctx.save_for_backward(a, b, c, o)
        ctx.heads, ctx.layout = heads, layout
        return o

    @staticmethod
    def backward(ctx, do):
        a, b, c, o = ctx.saved_tensors
        do = do.contiguous()
        da, db, dc = (None if t is None else torch.empty_like(t) for t in (a, b, c))
        q, k, v = _Attention32._views(ctx.layout, a, b, c)
        dq, dk, dv = _Attention32._views(ctx.layout, da, db, dc)
        attention_bwd32(q, k, v, o, do, dq, dk, dv, ctx.heads)
        return da, db, dc, None, None


def attention32(q, k, v, heads: int) -> torch.Tensor:
    """softmax(q k^T / sqrt(D)) v per head, q [B,Tq,C], k, v [B,Tk,C], C = heads * D, D in {40, 80, 160}; differentiable in q, k, v"""
    return _Attention32.apply(q, k, v, heads, 0)


def attention32_qkv(qkv, heads: int) -> torch.Tensor:
    """self-attention on stacked rows q|k|v [B,T,3C], read in place; the gradient comes back stacked, one buffer for to_q|to_k|to_v"""
    return _Attention32.apply(qkv, None, None, heads, 1)


def attention32_q_kv(q, kv, heads: int) -> torch.Tensor:
    """cross-attention of q [B,Tq,C] on stacked rows k|v [B,Tk,2C]"""
    return _Attention32.apply(q, kv, None, heads, 2)


class _LayerNorm32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x, gamma, beta = (_f32c(t, "layernorm32") for t in (x, gamma, beta))
        Cc = x.shape[-1]
        y = torch.empty_like(x)
        _check(_lib().dm_f32_op_layernorm(_stream(), _p(x), x.numel() // Cc, Cc, _p(gamma), _p(beta), eps, _p(y)), "dm_f32_op_layernorm")
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        dy = dy.contiguous()
        lib = _lib()
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        nbytes = lib.dm_f32_op_layernorm_bwd_workspace(rows, Cc)
        if nbytes == 0:
            raise EngineError("dm_f32_op_layernorm_bwd_workspace refused its arguments")
        work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        _check(lib.dm_f32_op_layernorm_bwd(_stream(), _p(x), _p(dy), rows, Cc, _p(gamma), ctx.eps, _p(work), work.numel() * 8, _p(dx), _p(dg), _p(db)),
               "dm_f32_op_layernorm_bwd")
        return dx, dg, db, None


def layernorm32(x, gamma, beta, eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm over the last axis as dm_f32_op_layernorm; differentiable in x, gamma, beta"""
    return _LayerNorm32.apply(x, gamma, beta, eps)


class _Geglu32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p):
        p = _f32c(p, "geglu32")
        Fh = p.shape[-1] // 2
        y = torch.empty(*p.shape[:-1], Fh, dtype=torch.float32, device=p.device)
        _check(_lib().dm_f32_op_geglu(_stream(), _p(p), p.numel() // (2 * Fh), Fh, _p(y)), "dm_f32_op_geglu")
        ctx.save_for_backward(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        (p,) = ctx.saved_tensors
        dy = dy.contiguous()
        Fh = p.shape[-1] // 2
        dp = torch.empty_like(p)
        _check(_lib().dm_f32_op_geglu_bwd(_stream(), _p(p), _p(dy), p.numel() // (2 * Fh), Fh, _p(dp)), "dm_f32_op_geglu_bwd")
        return dp


def geglu32(p: torch.Tensor) -> torch.Tensor:
    """P [..., 2F] = (h | g) -> h gelu(g) [..., F]; differentiable"""
    return _Geglu32.apply(p)


def _linear_res(x, w, bias, res):
    """F.linear(x, w, bias) + res on rows [M, Cin]: one dm_f32_op_gemm with its residual epilogue"""
    M, cin = x.shape
    return conv32(x.reshape(1, 1, M, cin), None, w, bias, None, res.reshape(1, 1, M, w.shape[0]), 0).reshape(M, w.shape[0])


# ---- modules ---------------------------------------------------------------------------------------------------------------------------
class _Tfm32(nn.Module):
    """_keys(): (diffusers key, owner module, parameter name, row range or None, as a 1x1 convolution).  A stacked parameter appears
    under several keys, one row range each."""
    def _keys(self):
        raise NotImplementedError

    @staticmethod
    def _view(t, rows, conv):
        t = t if rows is None else t[rows[0]:rows[1]]
        return t[:, :, None, None] if conv else t

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for key, mod, pname, rows, conv in self._keys():
            t = self._view(getattr(mod, pname), rows, conv)
            out[prefix + key] = t if keep_vars else t.detach().clone()
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        want = {key: rest for key, *rest in self._keys()}
        missing, unexpected = sorted(set(want) - set(state_dict)), sorted(set(state_dict) - set(want))
        if strict and (missing or unexpected):
            raise RuntimeError(f"{type(self).__name__}.load_state_dict: missing {missing}, unexpected {unexpected}")
        with torch.no_grad():
            for key, (mod, pname, rows, conv) in want.items():
                if key not in state_dict:
                    continue
                dst = self._view(getattr(mod, pname), rows, conv)
                v = torch.as_tensor(state_dict[key])
                if tuple(v.shape) != tuple(dst.shape):
                    raise RuntimeError(f"{key}: shape {tuple(v.shape)} does not fit this block ({tuple(dst.shape)})")
                dst.copy_(v.to(dst.dtype))
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def grad_dict(self) -> "OrderedDict[str, Optional[torch.Tensor]]":
        """the parameters' `.grad` under the diffusers names and shapes"""
        out = OrderedDict()
        for key, mod, pname, rows, conv in self._keys():
            g = getattr(mod, pname).grad
            out[key] = None if g is None else self._view(g, rows, conv)
        return out

    def _linear_params(self, name: str, cout: int, cin: int, bias: bool) -> None:
        w = torch.empty(cout, cin)
        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
        self.register_parameter(f"{name}_weight", nn.Parameter(w))
        if bias:
            self.register_parameter(f"{name}_bias", nn.Parameter(torch.empty(cout).uniform_(-cin ** -0.5, cin ** -0.5)))

    def _norm_params(self, name: str, c: int) -> None:
        self.register_parameter(f"{name}_weight", nn.Parameter(torch.ones(c)))
        self.register_parameter(f"{name}_bias", nn.Parameter(torch.zeros(c)))


class BasicTransformerBlock32(_Tfm32):
    """diffusers BasicTransformerBlock (SD 1.5: LayerNorm eps 1e-5, bias-free q/k/v, GEGLU feed-forward of 4 dim) on fp32 tokens:
    forward(x [B,T,dim], context [B,Tk,ctx_dim]) -> [B,T,dim].  attn1's to_q | to_k | to_v live in one parameter [3 dim][dim], attn2's
    to_k | to_v in one [2 dim][ctx_dim]; the state dict speaks the diffusers names (norm1.weight ... ff.net.2.bias)."""
    def __init__(self, dim: int, heads: int, ctx_dim: int):
        super().__init__()
        if dim % heads or dim // heads not in (40, 80, 160):
            raise EngineError(f"BasicTransformerBlock32: head_dim {dim / heads:g} is not 40, 80 or 160")
        self.dim, self.heads, self.ctx_dim = dim, heads, ctx_dim
        self._norm_params("norm1", dim)
        self._linear_params("attn1_to_qkv", 3 * dim, dim, False)
        self._linear_params("attn1_to_out", dim, dim, True)
        self._norm_params("norm2", dim)
        self._linear_params("attn2_to_q", dim, dim, False)
        self._linear_params("attn2_to_kv", 2 * dim, ctx_dim, False)
        self._linear_params("attn2_to_out", dim, dim, True)
        self._norm_params("norm3", dim)
        self._linear_params("ff_proj", 8 * dim, dim, True)
        self._linear_params("ff_out", dim, 4 * dim, True)

    def _keys(self):
        d = self.dim
        yield "norm1.weight", self, "norm1_weight", None, False
        yield "norm1.bias", self, "norm1_bias", None, False
        for i, n in enumerate("qkv"):
            yield f"attn1.to_{n}.weight", self, "attn1_to_qkv_weight", (i * d, (i + 1) * d), False
        yield "attn1.to_out.0.weight", self, "attn1_to_out_weight", None, False
        yield "attn1.to_out.0.bias", self, "attn1_to_out_bias", None, False
        yield "norm2.weight", self, "norm2_weight", None, False
        yield "norm2.bias", self, "norm2_bias", None, False
        yield "attn2.to_q.weight", self, "attn2_to_q_weight", None, False
        for i, n in enumerate("kv"):
            yield f"attn2.to_{n}.weight", self, "attn2_to_kv_weight", (i * d, (i + 1) * d), False
        yield "attn2.to_out.0.weight", self, "attn2_to_out_weight", None, False
        yield "attn2.to_out.0.bias", self, "attn2_to_out_bias", None, False
        yield "norm3.weight", self, "norm3_weight", None, False
        yield "norm3.bias", self, "norm3_bias", None, False
        yield "ff.net.0.proj.weight", self, "ff_proj_weight", None, False
        yield "ff.net.0.proj.bias", self, "ff_proj_bias", None, False
        yield "ff.net.2.weight", self, "ff_out_weight", None, False
        yield "ff.net.2.bias", self, "ff_out_bias", None, False

    def forward(self, x, context):
        B, Tq, d = x.shape
        if d != self.dim or context.dim() != 3 or context.shape[0] != B or context.shape[2] != self.ctx_dim:
            raise EngineError("BasicTransformerBlock32: x [B,T,dim] and context [B,Tk,ctx_dim] are expected")
        Tk = context.shape[1]
        x = x.reshape(B * Tq, d)
        h = layernorm32(x, self.norm1_weight, self.norm1_bias)
        a = attention32_qkv(linear32(h, self.attn1_to_qkv_weight, None).reshape(B, Tq, 3 * d), self.heads)
        x = _linear_res(a.reshape(B * Tq, d), self.attn1_to_out_weight, self.attn1_to_out_bias, x)
        h = layernorm32(x, self.norm2_weight, self.norm2_bias)
        q = linear32(h, self.attn2_to_q_weight, None).reshape(B, Tq, d)
        kv = linear32(context.reshape(B * Tk, self.ctx_dim), self.attn2_to_kv_weight, None).reshape(B, Tk, 2 * d)
        a = attention32_q_kv(q, kv, self.heads)
        x = _linear_res(a.reshape(B * Tq, d), self.attn2_to_out_weight, self.attn2_to_out_bias, x)
        h = layernorm32(x, self.norm3_weight, self.norm3_bias)
        y = geglu32(linear32(h, self.ff_proj_weight, self.ff_proj_bias))
        return _linear_res(y, self.ff_out_weight, self.ff_out_bias, x).reshape(B, Tq, d)


class Transformer2D32(_Tfm32):
    """diffusers Transformer2DModel as SD 1.5 uses it (GroupNorm eps 1e-6, proj_in 1x1, one BasicTransformerBlock, proj_out 1x1 + the
    input) on NHWC fp32: forward(x [N,H,W,C], context [N,Tk,ctx_dim]) -> [N,H,W,C]; state-dict keys norm.weight, proj_in.weight [C,C,1,1],
    transformer_blocks.0.*, proj_out.*"""
    def __init__(self, channels: int, heads: int, ctx_dim: int, groups: int = 32):
        super().__init__()
        self.channels, self.groups = channels, groups
        self._norm_params("norm", channels)
        self._linear_params("proj_in", channels, channels, True)
        self.block = BasicTransformerBlock32(channels, heads, ctx_dim)
        self._linear_params("proj_out", channels, channels, True)

    def _keys(self):
        yield "norm.weight", self, "norm_weight", None, False
        yield "norm.bias", self, "norm_bias", None, False
        yield "proj_in.weight", self, "proj_in_weight", None, True
        yield "proj_in.bias", self, "proj_in_bias", None, False
        for key, *rest in self.block._keys():
            yield ("transformer_blocks.0." + key, *rest)
        yield "proj_out.weight", self, "proj_out_weight", None, True
        yield "proj_out.bias", self, "proj_out_bias", None, False

    def forward(self, x, context):
        N, H, W, Cc = x.shape
        h = groupnorm_silu32(x, None, self.norm_weight, self.norm_bias, self.groups, 1e-6, False)
        h = conv32(h, None, self.proj_in_weight, self.proj_in_bias, None, None, 0)
        t = self.block(h.reshape(N, H * W, Cc), context)
        return conv32(t.reshape(N, H, W, Cc), None, self.proj_out_weight, self.proj_out_bias, None, x, 0)
