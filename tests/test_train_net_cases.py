"""CPU tier of the miniature U-Net of the training blocks (tests/train_net_cases.py), runnable without a device.

  * the yardstick's conditions: 179 leaves, every float64 gradient finite and far from zero, and CPU fp32 autograd within TOL_E2E / MARGIN
    of float64 for every gradient — so the bound the device is held to (tests/test_gpu_train_net.py) is the floor TOL_E2E for every
    tensor and no case rests on a loose 4 x cpu
  * the rule has teeth at this depth: five wiring errors each move a named gradient by more than 10 x TOL_E2E
  * the slab rules of wgrad32, attention backward and LayerNorm backward, restated in plain Python, give the tabulated partitions of the
    shapes the operator tests run on the device (the cap of 16 / 64, an empty trailing slab, a slab of one query)
  * wgrad_host at a 4-slab shape equals autograd, and losing the last slab's pixels would show"""
import pytest
import torch

from diff_mining_amd import train as T
from tests import train_cases as TC
from tests import train_net_cases as TN


def test_yardstick_conditions():
    k = TN.net_case()
    g64, g32 = k["g64"], k["g32"]
    assert len(TN.net_sd()) == TN.N_PARAMS == 176 and len(g64) == TN.N_LEAVES == 179 and list(g64) == list(g32)
    assert k["y64"].shape == (TN.N, TN.C_LO, TN.H, TN.W) and k["y64"].dtype == torch.float64 and k["y32"].dtype == torch.float32
    worst, small = ("", 0.0), ("", float("inf"))
    rels = []
    for name, g in g64.items():
        assert g.dtype == torch.float64 and torch.isfinite(g).all().item(), name
        rms = g.pow(2).mean().sqrt().item()
        assert rms > 1e-3, f"{name}: RMS {rms:.3e} — nothing a relative bound can be held against"
        rel = TN.rel_l2(g32[name], g)
        assert rel <= TN.TOL_E2E / TN.MARGIN, f"{name}: CPU fp32 at {rel:.3e} of float64: the device bound would rest on 4 x cpu"
        rels.append(rel)
        worst, small = max(worst, (name, rel), key=lambda t: t[1]), min(small, (name, rms), key=lambda t: t[1])
    rel_y = TN.rel_l2(k["y32"], k["y64"])
    assert rel_y <= TN.TOL_E2E / TN.MARGIN
    print(f"TRAIN_NET cpu-fp32 vs float64: y {rel_y:.3e}, gradients median {sorted(rels)[len(rels) // 2]:.3e}, worst {worst[1]:.3e} ({worst[0]}); "
          f"smallest gradient RMS {small[1]:.3e} ({small[0]})")


def test_the_yardstick_is_cheap():
    """float64 forward and backward of the whole net: well under the minute the CPU tier may add (measured 0.2 - 0.8 s on 16 cores)"""
    import time
    t0 = time.perf_counter()
    y, grads = TN.net_grads(torch.float64)
    dt = time.perf_counter() - t0
    print(f"TRAIN_NET float64 forward + backward: {dt:.2f} s")
    assert len(grads) == 179 and TN.rel_l2(y, TN.net_case()["y64"]) < 1e-12 and dt < 20.0


def test_prefixed_names_are_the_blocks_state_dicts():
    """every block of the device net loads its slice of the state dict strictly: the names and shapes are the modules' own"""
    sd = TN.net_sd()
    seen = 0
    for name, spec in TN.LAYOUT:
        blk = TN.make_block(T, spec)
        part = TN.sub(sd, name)
        blk.load_state_dict(part)
        assert list(blk.grad_dict()) == list(part), name
        seen += len(part)
    assert seen == len(sd) == 176


# the error -> a tensor it must move (asserted), beside the one it moves most (printed)
TEETH = {"s1_detached_before_u1": "down.conv.weight", "temb_grad_from_r0_alone": "temb", "ctx_detached_in_am": "ctx",
         "up_to_10x8_and_cropped": "up.conv.weight", "u0_conv2_residual_detached": "u0.conv_shortcut.weight"}


@pytest.mark.parametrize("wiring", TN.WIRINGS)
def test_the_rule_has_teeth(wiring):
    """a yardstick earns trust when a wiring error moves it far past the bound: float64 gradients of the net with one error each"""
    right = TN.net_case()["g64"]
    _, wrong = TN.net_grads(torch.float64, wiring)
    moved = {name: TN.rel_l2(wrong[name], right[name]) for name in right}
    most = max(moved, key=moved.get)
    named = TEETH[wiring]
    print(f"TRAIN_NET teeth {wiring}: {named} moves {moved[named]:.3e}, most {most} {moved[most]:.3e}, "
          f"{sum(v > 10 * TN.TOL_E2E for v in moved.values())} of {len(moved)} past 10 x TOL_E2E = {10 * TN.TOL_E2E:.0e}")
    assert moved[named] > 10 * TN.TOL_E2E, f"{wiring}: {named} moves only {moved[named]:.3e}"


def test_wiring_errors_but_one_keep_the_forward_values():
    """four of the five are errors of the backward pass alone: the output is the right one, so only a gradient check can see them"""
    y = TN.net_case()["y64"]
    for wiring in TN.WIRINGS:
        yw, _ = TN.net_grads(torch.float64, wiring)
        if wiring == "up_to_10x8_and_cropped":
            assert TN.rel_l2(yw, y) > 10 * TN.TOL_E2E
        else:
            assert TN.rel_l2(yw, y) < 1e-12, wiring


def test_slab_rules_give_the_tabulated_partitions():
    for c, (slabs, length, last) in TN.NET_CONV_PARTITIONS.items():
        s, ln, pop = TN.wgrad_slab_rule(TN.conv_pixels(c))
        assert (s, ln, pop[-1]) == (slabs, length, last) and sum(pop) == TN.conv_pixels(c) and ln % 32 == 0, c
    assert [TN.conv_pixels(c) for c in TN.NET_CONV_CASES] == [8191, 8197, 16384, 32805, 8320, 8320, 8320]
    assert max(TN.conv_pixels(c) for c in TC.CONV_CASES) <= 512                       # what the older cases stop at
    assert TN.wgrad_slab_rule(8192)[:2] == (4, 2048) and TN.wgrad_slab_rule(1)[:2] == (1, 32) and TN.wgrad_slab_rule(231)[:2] == (2, 128)
    assert TN.wgrad_slab_rule(4 * 64 * 64)[0] == 8 and TN.wgrad_slab_rule(2 * 64 * 64)[0] == 4 and TN.wgrad_slab_rule(10 ** 6)[0] == 16
    for c, (slabs, length, pops) in TN.NET_ATTN_PARTITIONS.items():
        s, ln, pop = TN.attn_slab_rule(c[2], c[3])
        assert (s, ln) == (slabs, length) and sum(pop) == c[2] and ln % 64 == 0, c
        assert {i: pop[i] for i in pops} == pops, c
    s, ln, pop = TN.attn_slab_rule(8200, 77)
    assert pop[15] == 0 and 15 * ln > 8200 and pop[14] == 136                          # slab 15 is empty: it begins past the last query
    assert TN.attn_slab_rule(4097, 77)[2][-1] == 1                                     # the last slab holds one query
    assert TN.attn_slab_rule(1030, 77)[:2] == (3, 384) and TN.attn_slab_rule(4096, 4096)[0] == 1 and TN.attn_slab_rule(513, 129)[0] == 1
    for c, (slabs, length, last) in TN.NET_LN_PARTITIONS.items():
        s, ln, pop = TN.ln_slab_rule(c[0])
        assert (s, ln, pop[-1]) == (slabs, length, last) and sum(pop) == c[0], c
    assert TN.ln_slab_rule(600)[:2] == (3, 200) and TN.ln_slab_rule(16384)[:2] == (64, 256) and TN.ln_slab_rule(5)[:2] == (1, 5)
    for (n, h, w, c1, c2, g, _, _), straddles in zip(TN.NET_GN_CASES, (True, True, False, False)):
        cpg = (c1 + c2) // g
        assert (c1 + c2) % g == 0 and cpg <= 256 and (c1 % cpg != 0) == straddles
    assert [(c[3] + c[4]) // c[5] for c in TN.NET_GN_CASES] == [60, 30, 80, 20] and 256 // 80 * 80 == 240


def test_wgrad_host_at_a_four_slab_shape():
    """wgrad_host, which the device weight gradient is compared with, equals autograd's dW at M = 8197; without the last slab's 1957 pixels
    it would be far outside what the operator test allows"""
    c = TN.NET_CONV_CASES[1]
    assert c[:7] == (0, 1, 1, 8197, 32, 0, 36)
    k = TC.conv_case(*c)
    x, dy, ref = TC.nhwc(k["x"]), TC.nhwc(k["dy"]), T.pack_conv(k["g64"][1])
    assert TN.rel_l2(T.wgrad_host(x, None, dy, 0), ref) < 1e-12
    last = TN.wgrad_slab_rule(8197)[2][-1]
    assert last == 1957
    short = T.wgrad_host(x[:, :, :-last], None, dy[:, :, :-last], 0)
    moved = TN.rel_l2(short, ref)
    print(f"TRAIN_NET wgrad_host without the last slab: {moved:.3e}")
    assert moved > 10 * TN.TOL_OP
