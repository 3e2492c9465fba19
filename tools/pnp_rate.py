#!/usr/bin/env python
"""Rates of the parallel-dataset generator on the fp32 net (diff_mining_amd.pnp; reference: applications/parallel-dataset/pnp.py) at the
reference's shapes: a 64 x 64 latent (512 x 512 images), B = 10 target countries, synthetic weights.

    python tools/pnp_rate.py [--steps 6] [--repeat 3] [--out profiles/pnp_rate.txt]

  inversion    ms per DDIM step (U-Net forward + update, dm_f32_ddim_run) at batch 1 — the reference inverts one image at a time — and at
               batch 8
  PnP          ms per Plug-and-Play step (dm_f32_pnp_run, every injection on) at 1 + 2 B = 21 samples, against 3 B = 30 plain forwards —
               the reference's batch layout — in one dm_f32_unet_forward
  decode       ms per decoded 512 x 512 image (dm_f32_vae_decode, uint8 out), and the tail alone on its [1,512,512,128] input: statistics
               + the fused kernel, against statistics + GroupNorm apply + conv_out (the two-kernel tail, which writes and re-reads 134 MB)
  gemm32       its time, FLOP and share of the 157 TFLOP/s fp32 MFMA peak inside one decode (the net's event profile)

Times are host clocks around work that ends in a device synchronise, after a warm-up of every shape.  The tail's three figures are host-clock
means over --tail-launches back-to-back launches per window on ONE input tensor, which the 256 MB last-level cache can keep between launches:
warm-cache launch-to-launch times, not kernel times from a trace.  Prints a table and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_mining_amd  # noqa: E402,F401
from diff_mining_amd import pnp as P  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.engine import UNetEngineF32, _p  # noqa: E402

PEAK_F32_MFMA = 157.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--tail-launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    net = UNetEngineF32(0)
    net.load_state_dict(synth.synth_state_dict(seed=0, dtype=np.float16))
    net.load_vae_decoder_state_dict(synth.synth_vae_decoder_state_dict())
    B, h, w, n = a.targets, 64, 64, a.steps
    g = torch.Generator().manual_seed(0)
    net.set_prompts(torch.randn(B + 2, 77, 768, generator=g))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.repeat):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.repeat * 1e3, out

    ts = P.ddim_timesteps(50)[:n]
    inv = P.ddim_timesteps(999)[::-1][:n].copy()
    c_inv, c_step = P.ddim_coefficients(inv, "invert"), P.ddim_coefficients(ts, "step")
    res = {"latent": [h, w], "targets": B, "steps_timed": n, "repeat": a.repeat, "device": torch.cuda.get_device_name(0)}
    for bs in (1, 8):
        x = torch.randn(bs, 4, h, w, generator=g).cuda()
        ms, _ = timed(lambda: net.ddim_run(x, inv, c_inv, [0] * bs))
        res[f"inversion_ms_per_step_batch{bs}"] = round(ms / n, 2)
        res[f"inversion_ms_per_step_per_image_batch{bs}"] = round(ms / n / bs, 2)
    conv_on, attn_on, conv_mask, attn_mask = P.injection_plan(n, 1.0, 1.0)
    x = torch.randn(B, 4, h, w, generator=g).cuda()
    src = torch.randn(n, 4, h, w, generator=g).cuda()
    slots = [0] + [1] * B + list(range(2, 2 + B))
    ms, _ = timed(lambda: net.pnp_run(x, src, ts, c_step, conv_on, attn_on, conv_mask, attn_mask, slots))
    res["pnp_ms_per_step_1_plus_2B"] = round(ms / n, 2)
    x3 = torch.randn(3 * B, 4, h, w, generator=g).cuda()
    ms, _ = timed(lambda: net.unet(x3, 501, [0] * B + slots[1:]))
    res["plain_forward_ms_3B"] = round(ms, 2)
    lat = torch.randn(2, 4, h, w, generator=g).cuda()
    ms, _ = timed(lambda: net.vae_decode(lat, want="u8"))
    res["decode_ms_per_512_image"] = round(ms / 2, 2)
    net.prof_enable(True)
    net.vae_decode(lat, want="u8")
    torch.cuda.synchronize()
    prof = net.prof_read()
    net.prof_enable(False)
    tf = prof["igemm_flops"] / (prof["igemm_ms"] * 1e-3) / 1e12
    res.update(decoder_gemm32_ms_per_image=round(prof["igemm_ms"] / 2, 2), decoder_gemm32_tflops=round(tf, 2),
               decoder_gemm32_fraction_of_peak=round(tf * 1e12 / PEAK_F32_MFMA, 3), decoder_gemm32_launches=prof["igemm_launches"])
    # the tail alone, on the tensor it reads
    lib, H = net.lib, 512
    X = torch.randn(1, H, H, 128, generator=g).cuda()
    gam, bet = torch.ones(128).cuda(), torch.zeros(128).cuda()
    Wp, bias = (torch.randn(3, 9 * 128, generator=g) / 34).cuda(), torch.zeros(3).cuda()
    st, Y = torch.empty(32, 2).cuda(), torch.empty(1, H, H, 128).cuda()
    o1, o2, u8 = torch.empty(1, 3, H, H).cuda(), torch.empty(1, 3, H, H).cuda(), torch.empty(1, H, H, 3, dtype=torch.uint8).cuda()
    s = net._stream()

    def stats_and_apply():
        assert lib.dm_f32_op_groupnorm(s, _p(X), None, 1, H * H, 128, 128, 32, 1e-6, _p(gam), _p(bet), 1, _p(st), _p(Y)) == 0

    def tail_fused():
        assert lib.dm_f32_op_decoder_tail(s, _p(X), _p(st), _p(gam), _p(bet), _p(Wp), _p(bias), 1, H, H, 128, 1, _p(o1), _p(u8)) == 0

    def conv_out():
        assert lib.dm_f32_op_conv_out(s, _p(Y), _p(Wp), _p(bias), 1, H, H, 128, 3, _p(o2)) == 0
    K = a.tail_launches                                   # one launch is far below a millisecond: a window holds K of them

    def many(fn):
        def run():
            for _ in range(K):
                fn()
        return run
    t_gn, t_tail, t_conv = (timed(many(f))[0] / K for f in (stats_and_apply, tail_fused, conv_out))
    res.update(tail_launches_per_window=K, groupnorm_stats_plus_apply_ms=round(t_gn, 3), fused_tail_kernel_ms=round(t_tail, 3), conv_out_kernel_ms=round(t_conv, 3),
               tail_rel_l2_fused_vs_two_kernel=float(((o1 - o2).double().norm() / o2.double().norm()).item()))
    lines = [
        f"parallel-dataset generator, fp32 ({res['device']}), latent {h}x{w}, B = {B} targets, synthetic weights; {n} steps timed, {a.repeat} repeats",
        f"  inversion step (forward + update): batch 1 {res['inversion_ms_per_step_batch1']:8.2f} ms; batch 8 {res['inversion_ms_per_step_batch8']:8.2f} ms "
        f"= {res['inversion_ms_per_step_per_image_batch8']:.2f} ms per image",
        f"  PnP step at 1 + 2B = {1 + 2 * B} samples, all injections on: {res['pnp_ms_per_step_1_plus_2B']:8.2f} ms; one plain forward of 3B = {3 * B} samples: "
        f"{res['plain_forward_ms_3B']:8.2f} ms",
        f"  decode of one 512x512 image (uint8 out): {res['decode_ms_per_512_image']:8.2f} ms; gemm32 in it {res['decoder_gemm32_ms_per_image']:.2f} ms, "
        f"{res['decoder_gemm32_tflops']:.2f} TFLOP/s = {res['decoder_gemm32_fraction_of_peak']:.3f} of the 157 TFLOP/s fp32 MFMA peak "
        f"({res['decoder_gemm32_launches']} launches for 2 images)",
        f"  tail on [1,512,512,128] (host clock, {K} back-to-back launches per window, warm cache): fused kernel {res['fused_tail_kernel_ms']:.3f} ms (fp32 + uint8 out); two-kernel tail: GroupNorm statistics + apply "
        f"{res['groupnorm_stats_plus_apply_ms']:.3f} ms (the statistics are common to both) + conv_out {res['conv_out_kernel_ms']:.3f} ms; "
        f"fused vs two-kernel rel-L2 {res['tail_rel_l2_fused_vs_two_kernel']:.2e}",
        json.dumps(res),
    ]
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    net.close()


if __name__ == "__main__":
    main()
