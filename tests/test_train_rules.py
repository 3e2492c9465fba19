"""CPU tier of the training operators (diff-mining_amd/train.py): the rules the device path is built from, pinned to torch.autograd in
float64 on a machine without a GPU.

  * the data gradient of every convolution mode is a FORWARD convolution of dY with dgrad_weights(w) (mode 2 after zero_insert2_host,
    mode 3 followed by nearest_bwd_host)
  * wgrad_host (the plain-indexing restatement the device weight gradient is compared with) equals autograd's dW
  * the GroupNorm (+ SiLU) backward formula of the device kernels equals autograd
  * the modules' state dicts speak the diffusers names and shapes and round-trip exactly

Everything is float64, so the bound is round-off of sums of a few thousand terms: 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

from diff_mining_amd import train as T

TOL64 = 1e-12


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).double()


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def conv_ref(x, w, mode, out_hw):
    """the convolution dm_f32_op_gemm computes in `mode`, NCHW, plain F.* ops"""
    if mode == 0:
        return F.conv2d(x, w)
    if mode == 1:
        return F.conv2d(x, w, padding=1)
    if mode == 2:
        return F.conv2d(x, w, stride=2, padding=1)
    return F.conv2d(F.interpolate(x, size=out_hw, mode="nearest"), w, padding=1)


# (mode, N, H, W, C1, C2, Cout, out_hw): odd images, a split source, upsample_size targets that are not 2x (one of them shrinking a side)
CASES = [
    (0, 2, 3, 5, 8, 0, 12, None), (0, 1, 4, 4, 8, 4, 6, None),
    (1, 3, 9, 7, 8, 4, 12, None), (1, 1, 1, 1, 4, 0, 4, None),
    (2, 2, 16, 16, 4, 0, 8, None), (2, 1, 9, 7, 8, 0, 4, None), (2, 1, 8, 5, 4, 4, 4, None),
    (3, 2, 4, 4, 4, 0, 8, (8, 8)), (3, 1, 5, 4, 8, 0, 4, (9, 7)), (3, 1, 5, 4, 4, 4, 4, (11, 3)), (3, 1, 3, 3, 4, 0, 4, (10, 7)),
]


def _case(mode, N, H, W, C1, C2, Cout, out_hw):
    cin = C1 + C2
    k = 1 if mode == 0 else 3
    x = _randn(N, cin, H, W, seed=1).requires_grad_()
    w = _randn(Cout, cin, k, k, seed=2, scale=(k * k * cin) ** -0.5).requires_grad_()
    y = conv_ref(x, w, mode, out_hw)
    dy = _randn(*y.shape, seed=3)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    return x.detach(), w.detach(), dy, dx, dw


@pytest.mark.parametrize("mode,N,H,W,C1,C2,Cout,out_hw", CASES)
def test_data_gradient_is_a_forward_convolution(mode, N, H, W, C1, C2, Cout, out_hw):
    x, w, dy, dx, _ = _case(mode, N, H, W, C1, C2, Cout, out_hw)
    taps = T.taps_of(mode)
    wd = T.unpack_conv(T.dgrad_weights(T.pack_conv(w), mode), taps)          # [Cin, Cout, k, k]
    assert wd.shape == (C1 + C2, Cout, w.shape[2], w.shape[3])
    g = _nhwc(dy)
    if mode == 2:
        g = T.zero_insert2_host(g, H, W)
    got = _nhwc(F.conv2d(_nchw(g), wd, padding=0 if mode == 0 else 1))
    if mode == 3:
        got = T.nearest_bwd_host(got, H, W)
    assert got.shape == (N, H, W, C1 + C2)
    assert _rel(got, _nhwc(dx)) < TOL64
    # the two row ranges of W' give the two sources' gradients
    if C2:
        lo = _nhwc(F.conv2d(_nchw(g), wd[:C1], padding=0 if mode == 0 else 1))
        lo = T.nearest_bwd_host(lo, H, W) if mode == 3 else lo
        assert _rel(lo, _nhwc(dx)[..., :C1]) < TOL64


def test_dgrad_weights_pads_with_zero_columns():
    w = _randn(6, 4, 3, 3, seed=5)
    a, b = T.dgrad_weights(T.pack_conv(w), 1), T.dgrad_weights(T.pack_conv(w), 1, pad_to=32)
    assert a.shape == (4, 9 * 6) and b.shape == (4, 9 * 32)
    b3 = b.reshape(4, 9, 32)
    assert torch.equal(b3[:, :, :6], a.reshape(4, 9, 6)) and not b3[:, :, 6:].any()
    assert torch.equal(T.dgrad_weights(T.pack_conv(w[:, :, 0, 0]), 0), w[:, :, 0, 0].t())
    with pytest.raises(ValueError):
        T.dgrad_weights(T.pack_conv(w), 4)


@pytest.mark.parametrize("mode,N,H,W,C1,C2,Cout,out_hw", CASES)
def test_wgrad_host_is_autograd_dw(mode, N, H, W, C1, C2, Cout, out_hw):
    x, w, dy, _, dw = _case(mode, N, H, W, C1, C2, Cout, out_hw)
    xn = _nhwc(x)
    xa, xb = (xn[..., :C1].contiguous(), xn[..., C1:].contiguous()) if C2 else (xn, None)
    got = T.wgrad_host(xa, xb, _nhwc(dy), mode, out_hw)
    assert got.dtype == torch.float64 and got.shape == (Cout, T.taps_of(mode) * (C1 + C2))
    assert _rel(got, T.pack_conv(dw)) < TOL64


def test_nearest_rule_is_interpolates():
    for inp, out in ((4, 8), (5, 9), (4, 7), (5, 11), (4, 3), (3, 10), (64, 85), (1, 5)):
        x = torch.arange(inp, dtype=torch.float64).reshape(1, 1, inp, 1)
        ref = F.interpolate(x, size=(out, 1), mode="nearest").reshape(-1).long()
        assert torch.equal(T.nearest_index(out, inp), ref), (inp, out)


@pytest.mark.parametrize("N,H,W,C,G,silu,const", [(2, 9, 7, 96, 32, True, False), (2, 3, 3, 64, 4, True, False), (1, 1, 1, 64, 32, True, False),
                                                 (2, 9, 7, 64, 4, False, False), (2, 4, 4, 32, 4, True, True)])
def test_groupnorm_backward_formula(N, H, W, C, G, silu, const):
    x = _randn(N, C, H, W, seed=1) * 2 + 0.5
    if const:
        x[0, : C // G] = 1.25          # a group without variance: rstd = eps^-1/2, xhat = 0
    x.requires_grad_()
    gamma, beta = _randn(C, seed=2).requires_grad_(), _randn(C, seed=3).requires_grad_()
    y = F.group_norm(x, G, gamma, beta, 1e-5)
    y = F.silu(y) if silu else y
    dy = _randn(*y.shape, seed=4)
    dx, dg, db = torch.autograd.grad(y, (x, gamma, beta), dy)
    gx, gg, gb = T.groupnorm_bwd_host(_nhwc(x.detach()), _nhwc(dy), gamma.detach(), beta.detach(), G, 1e-5, silu)
    assert _rel(_nchw(gx), dx) < 1e-10 and _rel(gg, dg) < TOL64 and _rel(gb, db) < TOL64      # dx: rstd = 316 amplifies round-off when var = 0


def _diffusers_resnet_sd(cin, cout, temb, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    sd = {"norm1.weight": r(cin), "norm1.bias": r(cin), "conv1.weight": r(cout, cin, 3, 3), "conv1.bias": r(cout),
          "time_emb_proj.weight": r(cout, temb), "time_emb_proj.bias": r(cout), "norm2.weight": r(cout), "norm2.bias": r(cout),
          "conv2.weight": r(cout, cout, 3, 3), "conv2.bias": r(cout)}
    if cin != cout:
        sd["conv_shortcut.weight"], sd["conv_shortcut.bias"] = r(cout, cin, 1, 1), r(cout)
    return sd


@pytest.mark.parametrize("cin,skip,cout", [(32, 0, 32), (32, 0, 64), (64, 32, 64)])
def test_resnet_state_dict_round_trip(cin, skip, cout):
    sd = _diffusers_resnet_sd(cin + skip, cout, 128)
    blk = T.ResnetBlock32(cin, cout, 128, skip_channels=skip)
    assert blk.has_shortcut == (cin + skip != cout)
    blk.load_state_dict(sd)
    out = blk.state_dict()
    assert list(out) == list(sd)                          # the diffusers names, in diffusers' order
    for k, v in sd.items():
        assert out[k].shape == v.shape and torch.equal(out[k], v), k
    assert torch.equal(blk.conv1_weight.detach(), T.pack_conv(sd["conv1.weight"]))      # held packed: [Cout][9 Cin], k = (tap, cin)
    assert set(blk.state_dict(prefix="down.0.")) == {"down.0." + k for k in sd}
    bad = dict(sd)
    del bad["norm2.bias"]
    with pytest.raises(RuntimeError):
        blk.load_state_dict(bad)
    bad = dict(sd, **{"conv1.weight": sd["conv1.weight"][:, :-1]})
    with pytest.raises(RuntimeError):
        blk.load_state_dict(bad)


def test_sampler_state_dict_round_trip():
    g = torch.Generator().manual_seed(3)
    for cls in (T.Downsample32, T.Upsample32):
        sd = {"conv.weight": torch.randn(64, 64, 3, 3, generator=g), "conv.bias": torch.randn(64, generator=g)}
        m = cls(64)
        m.load_state_dict(sd)
        out = m.state_dict()
        assert list(out) == list(sd) and all(torch.equal(out[k], sd[k]) for k in sd)


def test_device_operators_refuse_cpu_tensors():
    with pytest.raises(T.EngineError):
        T.conv32(torch.zeros(1, 2, 2, 32), None, torch.zeros(32, 32), None, None, None, 0)
