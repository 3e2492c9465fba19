"""A miniature U-Net of the training blocks (tests/train_net_cases.py: six ResnetBlock32, four Transformer2D32, Downsample32, Upsample32 to an
odd size, three skip tensors each consumed twice) against float64 autograd of the same net written with F.* ops.

The single-block tests cannot see what the whole-net step relies on: one temb feeding six time_emb_proj layers and one context feeding
four attn2.to_kv layers (autograd must sum their gradients), a residual gradient meeting a second gradient on the same tensor, an
up-sampler returning to 9 x 7 from a stride-2 output of that size, and an up block's GroupNorm with a group across its two sources.
Here: y, dx, dtemb, dcontext and all 176 parameter gradients within TOL_E2E of float64 (tests/test_train_net_cases.py asserts that CPU
fp32 autograd is within TOL_E2E / 4 for every one, so the floor is the bound throughout); the same bits from a second build, from a side
stream whose inputs arrive late, and from every needs_input_grad arm; `.grad` accumulation over two live graphs."""
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import train as T  # noqa: E402
from tests import train_cases as TC  # noqa: E402
from tests import train_net_cases as TN  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


class _Net:
    """the blocks of TN.LAYOUT, each loaded through its own load_state_dict, NHWC on the device"""
    def __init__(self):
        sd = TN.net_sd()
        self.blocks = OrderedDict()
        for name, spec in TN.LAYOUT:
            blk = TN.make_block(T, spec)
            blk.load_state_dict(TN.sub(sd, name))
            self.blocks[name] = blk.cuda()

    def __call__(self, x, temb, ctx):
        b = self.blocks
        h = b["r0"](x, temb)
        s0 = h = b["a0"](h, ctx)
        s1 = h = b["down"](h)
        h = b["r1"](h, temb)
        s2 = h = b["a1"](h, ctx)
        h = b["am"](b["rm"](h, temb), ctx)
        h = b["u2"](h, temb, s2)
        h = b["u1"](h, temb, s1)
        h = b["up"](h, (TN.H, TN.W))
        return b["a3"](b["u0"](h, temb, s0), ctx)

    def named_parameters(self):
        for name, blk in self.blocks.items():
            for pname, p in blk.named_parameters():
                yield f"{name}.{pname}", p

    def grad_dict(self):
        """every parameter's `.grad` under the prefixed diffusers names and shapes (the stacked projections come back split)"""
        return OrderedDict((f"{name}.{k}", g) for name, blk in self.blocks.items() for k, g in blk.grad_dict().items())


def _inputs(req=(True, True, True)):
    k = TN.net_case()
    x, temb, ctx = TC.nhwc(k["x"]).cuda().requires_grad_(req[0]), k["temb"].cuda().requires_grad_(req[1]), k["ctx"].cuda().requires_grad_(req[2])
    return x, temb, ctx, TC.nhwc(k["dy"]).cuda()


def _run(net, req=(True, True, True)):
    x, temb, ctx, dy = _inputs(req)
    y = net(x, temb, ctx)
    y.backward(dy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "x": x.grad, "temb": temb.grad, "ctx": ctx.grad, "params": {n: p.grad for n, p in net.named_parameters()}, "named": net.grad_dict()}


@pytest.fixture(scope="module")
def full():
    """one forward and backward pass of a freshly built net on the default stream, everything trainable: what the other runs are compared with"""
    out = _run(_Net())
    assert len(out["params"]) == 6 * 10 + 4 * 2 + 4 * 23 + 2 * 2 and all(g is not None for g in out["params"].values())
    return out


def _same_inputs(run, full, which=("x", "temb", "ctx")):
    for n in which:
        assert torch.equal(run[n], full[n]), n


def test_gradients(full):
    k = TN.net_case()
    g64, g32 = k["g64"], k["g32"]
    figures = [TN.check("net y", TC.nchw(full["y"]).cpu(), k["y64"], k["y32"], TN.TOL_E2E)]
    figures.append(TN.check("net dX", TC.nchw(full["x"]).cpu(), g64["x"], g32["x"], TN.TOL_E2E))
    figures.append(TN.check("net dtemb", full["temb"].cpu(), g64["temb"], g32["temb"], TN.TOL_E2E))
    figures.append(TN.check("net dcontext", full["ctx"].cpu(), g64["ctx"], g32["ctx"], TN.TOL_E2E))
    named = full["named"]
    assert list(named) == list(TN.net_sd()) and len(named) == TN.N_PARAMS == 176
    for name, g in named.items():
        assert g is not None and g.shape == k["sd"][name].shape, name
        figures.append(TN.check(f"net d{name}", g.cpu(), g64[name], g32[name], TN.TOL_E2E))
    assert len(figures) == 1 + TN.N_LEAVES and all(bound == TN.TOL_E2E for _, _, bound in figures)          # the floor, never 4 x cpu
    print(f"TRAIN_OPS net worst of {len(figures)}: device {max(f[0] for f in figures):.3e}  cpu-fp32 {max(f[1] for f in figures):.3e}  bound {TN.TOL_E2E:.3e}")


def test_a_second_build_gives_the_same_bits(full):
    again = _run(_Net())
    assert torch.equal(again["y"], full["y"])
    _same_inputs(again, full)
    for n, g in full["params"].items():
        assert torch.equal(again["params"][n], g), n


def test_side_stream_with_late_inputs(full):
    """every call passes torch.cuda.current_stream(): the inputs sit in buffers that hold NaN until copies queued on the side stream — behind
    tens of milliseconds of unrelated work — fill them, so a kernel issued on any other stream would read NaN"""
    net = _Net()
    src = dict(zip(("x", "temb", "ctx", "dy"), (t.detach() for t in _inputs())))
    buf = {n: torch.full_like(t, float("nan")) for n, t in src.items()}
    busy = torch.ones(1 << 27, device="cuda")                     # 512 MiB: every pass over it moves 1 GiB
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        t0.record()
        for _ in range(150):
            busy.mul_(1.0000001)
        t1.record()
        for n in src:
            buf[n].copy_(src[n])
        x, temb, ctx = (buf[n].requires_grad_() for n in ("x", "temb", "ctx"))
        y = net(x, temb, ctx)
        y.backward(buf["dy"])
    side.synchronize()
    print(f"TRAIN_OPS net side stream: {t0.elapsed_time(t1):.1f} ms of unrelated work ahead of the inputs")
    assert t0.elapsed_time(t1) > 10.0
    run = {"y": y.detach(), "x": x.grad, "temb": temb.grad, "ctx": ctx.grad}
    for n, t in run.items():
        assert torch.isfinite(t).all().item(), n
        assert torch.equal(t, full[n]), n
    for n, p in net.named_parameters():
        assert torch.isfinite(p.grad).all().item(), n
        assert torch.equal(p.grad, full["params"][n]), n


def test_inputs_without_requires_grad_get_none(full):
    net = _Net()
    run = _run(net, req=(False, False, False))
    assert run["x"] is None and run["temb"] is None and run["ctx"] is None
    assert torch.equal(run["y"], full["y"])
    for n, g in full["params"].items():
        assert torch.equal(run["params"][n], g), n


def test_only_to_kv_and_the_norms_trainable(full):
    net = _Net()
    trainable = []
    for n, p in net.named_parameters():
        keep = n.endswith("attn2_to_kv_weight") or "norm" in n.rsplit(".", 1)[-1]
        p.requires_grad_(keep)
        trainable += [n] * keep
    # per ResNet norm1, norm2; per transformer norm and the block's norm1 .. norm3; weight and bias each; and four stacked to_k | to_v
    assert len(trainable) == 6 * 4 + 4 * 8 + 4
    run = _run(net)
    for n, g in run["params"].items():
        if n in trainable:
            assert torch.equal(g, full["params"][n]), n
        else:
            assert g is None, n
    _same_inputs(run, full, ("x",))


def test_weights_frozen_biases_trainable(full):
    net = _Net()
    for n, p in net.named_parameters():
        p.requires_grad_(n.endswith("_bias"))
    run = _run(net)
    biases = [n for n in run["params"] if n.endswith("_bias")]
    assert len(biases) == 6 * 5 + 4 + 4 * 10 + 2          # five per ResNet, four conv_shortcuts, ten per transformer, the two samplers
    for n, g in run["params"].items():
        if n in biases:
            assert torch.equal(g, full["params"][n]), n
        else:
            assert g is None, n
    _same_inputs(run, full)


def test_no_grad_forward_is_the_same_bits(full):
    net = _Net()
    x, temb, ctx, _ = _inputs()
    with torch.no_grad():
        y = net(x, temb, ctx)
    torch.cuda.synchronize()
    assert y.grad_fn is None and not y.requires_grad and torch.equal(y, full["y"])


def test_two_live_graphs_accumulate_like_torch(full):
    """two forward passes share the parameters and the inputs; their backward passes add into `.grad` as torch does: g + g, bit for bit"""
    net = _Net()
    x, temb, ctx, dy = _inputs()
    y1, y2 = net(x, temb, ctx), net(x, temb, ctx)
    y1.backward(dy)
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, full["params"][n]), n
    y2.backward(dy)
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        assert torch.equal(p.grad, full["params"][n] + full["params"][n]), n
    for n, t in (("x", x), ("temb", temb), ("ctx", ctx)):
        assert torch.equal(t.grad, full[n] + full[n]), n
