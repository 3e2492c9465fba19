#!/usr/bin/env python
"""Rates of text-to-image sampling on the fp16 engine (diff_mining_amd.sample; reference: `Trainer.sample`, finetuning/cars.py:235-255) at the
reference's shapes: a 64 x 64 latent (512 x 512 images), B = 5 samples (`num_samples`), synthetic weights.

    python tools/sample_rate.py [--steps 6] [--repeat 3] [--out profiles/sample_rate.txt]

  guided step  ms per guided DDIM step (U-Net forward at batch 2B + the update, dm_sample_run)
  decode       ms per decoded 512 x 512 image (uint8 out) on the fp16 engine (dm_vae_decode) and, in the same process, on the fp32 net
               (dm_f32_vae_decode): the pair that counts is this same-run pair
  tail         the fused tail (statistics + affine + the conv_out kernel, dm_op_decoder_tail) on its [1,512,512,128] input, against the
               unfused GroupNorm(silu) alone (statistics + apply, which writes and re-reads 67 MB before any convolution)
  igemm        the igemm family's time, FLOP and share of one decode (the engine's event profile), and the attention's

Times are host clocks around work that ends in a device synchronise, after a warm-up of every shape.  The tail's figures are host-clock means
over --tail-launches back-to-back launches per window on ONE input tensor, which the 256 MB last-level cache can keep between launches:
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
from diff_mining_amd import sample as S  # noqa: E402
from diff_mining_amd import synth  # noqa: E402
from diff_mining_amd.engine import UNetEngine, UNetEngineF32, _p  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--tail-launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_rate.py measures on the GPU: no device visible")
    torch.cuda.init()
    dec_sd = synth.synth_vae_decoder_state_dict()
    eng = UNetEngine(0)
    eng.load_state_dict(synth.synth_state_dict(seed=0, dtype=np.float16))
    eng.load_vae_decoder_state_dict(dec_sd)
    net32 = UNetEngineF32(0)
    net32.load_vae_decoder_state_dict(dec_sd)
    B, h, w, n = a.samples, 64, 64, a.steps
    g = torch.Generator().manual_seed(0)
    eng.set_prompts(torch.randn(B + 1, 77, 768, generator=g).half())

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.repeat):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.repeat * 1e3, out

    ts = S.sample_timesteps(50)[:n]
    tab = S.sample_coefficients(S.sample_timesteps(50))[:n]
    res = {"latent": [h, w], "samples": B, "steps_timed": n, "repeat": a.repeat, "device": torch.cuda.get_device_name(0)}
    x = torch.randn(B, 4, h, w, generator=g).cuda()
    slots = [0] * B + list(range(1, 1 + B))
    ms, lat = timed(lambda: eng.sample_run(x, ts, tab, slots, 7.5))
    res["guided_step_ms"] = round(ms / n, 2)
    res["guided_step_ms_per_sample"] = round(ms / n / B, 2)
    lat = torch.randn(B, 4, h, w, generator=g).cuda()
    # the same-run pair, alternating: fp16 engine, fp32 net, fp16 engine, fp32 net
    pair = []
    for _ in range(2):
        pair.append((timed(lambda: eng.vae_decode(lat, want="u8"))[0] / B, timed(lambda: net32.vae_decode(lat, want="u8"))[0] / B))
    res["decode_ms_per_512_image_fp16"] = [round(p[0], 2) for p in pair]
    res["decode_ms_per_512_image_fp32_net"] = [round(p[1], 2) for p in pair]
    eng.prof_enable(True)
    eng.vae_decode(lat, want="u8")
    torch.cuda.synchronize()
    prof = eng.prof_read()
    eng.prof_enable(False)
    ms_prof, _ = timed(lambda: eng.vae_decode(lat, want="u8"))
    res.update(decoder_igemm_ms_per_image=round(prof["igemm_ms"] / B, 2), decoder_igemm_tflops=round(prof["igemm_flops"] / (prof["igemm_ms"] * 1e-3) / 1e12, 1),
               decoder_igemm_launches=prof["igemm_launches"], decoder_attn_ms_per_image=round(prof["attn_ms"] / B, 3),
               decoder_igemm_share_of_decode=round(prof["igemm_ms"] / ms_prof, 3))
    # the tail alone, on the tensor it reads
    lib, H = eng.lib, 512
    X = torch.randn(1, H, H, 128, generator=g).half().cuda()
    gam, bet = torch.ones(128).cuda(), torch.zeros(128).cuda()
    Wp, bias = (torch.randn(3, 9 * 128, generator=g) / 34).half().cuda(), torch.zeros(3).half().cuda()
    nb = lib.dm_op_decoder_tail_workspace_bytes(1, H, H)
    work = torch.empty(nb, dtype=torch.uint8).cuda()
    Y = torch.empty(1, H, H, 128, dtype=torch.float16).cuda()
    raw, u8 = torch.empty(1, 3, H, H, dtype=torch.float16).cuda(), torch.empty(1, H, H, 3, dtype=torch.uint8).cuda()
    s = eng._stream()

    def tail_fused():
        assert lib.dm_op_decoder_tail(s, _p(X), _p(gam), _p(bet), _p(Wp), _p(bias), 1, H, H, 1e-6, _p(work), nb, _p(raw), _p(u8)) == 0

    def groupnorm_unfused():           # dm_op_groupnorm synchronises and allocates per call: timed in windows of its own, as it is
        assert lib.dm_op_groupnorm(s, _p(X), None, 1, H * H, 128, 128, 32, 1e-6, _p(gam), _p(bet), 1, _p(Y)) == 0
    K = a.tail_launches

    def many(fn):
        def run():
            for _ in range(K):
                fn()
        return run
    t_tail, t_gn = (timed(many(f))[0] / K for f in (tail_fused, groupnorm_unfused))
    res.update(tail_launches_per_window=K, fused_tail_ms=round(t_tail, 3), groupnorm_silu_unfused_ms=round(t_gn, 3))
    lines = [
        f"text-to-image sampling, fp16 engine ({res['device']}), latent {h}x{w}, B = {B} samples, synthetic weights; {n} steps timed, {a.repeat} repeats",
        f"  guided step (U-Net at batch 2B = {2 * B} + update): {res['guided_step_ms']:8.2f} ms = {res['guided_step_ms_per_sample']:.2f} ms per sample",
        f"  decode of one 512x512 image (uint8 out), batch {B}, alternating: fp16 engine {res['decode_ms_per_512_image_fp16']} ms; fp32 net "
        f"{res['decode_ms_per_512_image_fp32_net']} ms",
        f"  inside one fp16 decode (event profile): igemm {res['decoder_igemm_ms_per_image']:.2f} ms per image at {res['decoder_igemm_tflops']:.1f} TFLOP/s "
        f"({res['decoder_igemm_launches']} launches for {B} images) = {res['decoder_igemm_share_of_decode']:.3f} of the decode's host-clock time; attention "
        f"{res['decoder_attn_ms_per_image']:.3f} ms per image",
        f"  tail on [1,512,512,128] (host clock, {K} back-to-back launches per window, warm cache): statistics + affine + fused kernel "
        f"{res['fused_tail_ms']:.3f} ms (fp16 + uint8 out); the unfused GroupNorm(silu) alone, with its per-call allocation and synchronise: "
        f"{res['groupnorm_silu_unfused_ms']:.3f} ms",
        json.dumps(res),
    ]
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    eng.close()
    net32.close()


if __name__ == "__main__":
    main()
