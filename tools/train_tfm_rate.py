#!/usr/bin/env python
"""Rates of the transformer half of the training operators at the U-Net's shapes: a training batch of 4 at 64^2, 32^2, 16^2 and 8^2 tokens.

Per level, for self-attention (stacked q|k|v rows) and cross-attention (77 keys, stacked k|v rows), in ONE process: the forward attn32
kernel and the four backward kernels one by one (statistics, dQ, dK / dV partials, their sum: dm_f32_op_attention_bwd_phases on a workspace
one full call has filled), device events, median of 20.  TFLOP/s count 4 B heads Tq Tk D per PAIR of matrix products: the forward pass is
one pair, the statistics half a pair, dQ one and a half, dK / dV two.  The backward pass is compared only with the forward kernel at the
same shape in the same process.  Also LayerNorm backward and GEGLU backward in GB/s against 5 rows C (x, dy read twice, dx written) and
5 M F (P = h | g and dy read, dP written) fp32.  Writes the table to --out (default profiles/train_tfm_rate.txt).  Records; gates nothing.

    python tools/train_tfm_rate.py [--batch 4] [--reps 20] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402

LEVELS = [(64, 320, 8), (32, 640, 8), (16, 1280, 8), (8, 1280, 8)]          # (latent side, channels, heads) of the SD 1.5 U-Net's attention levels
CTX = 77


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_tfm_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = E.load_library()
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)          # noqa: E731
    B = a.batch
    lines = [f"# tools/train_tfm_rate.py: batch {B}, median of {a.reps}, device events, one process, one run; {torch.cuda.get_device_name(0)}",
             "# attention: forward attn32 and the backward kernels; TF/s per pair of products = 4 B heads Tq Tk D (stats 0.5, dQ 1.5, dK/dV 2 pairs)",
             f"{'kind':>5} {'Tq':>5} {'Tk':>5} {'D':>4} {'slabs':>5} | {'fwd ms':>8} {'TF/s':>6} | {'stats ms':>8} {'TF/s':>6} | {'dQ ms':>8} {'TF/s':>6} | {'dKdV ms':>8} {'TF/s':>6} |"
             f" {'sum ms':>7} | {'bwd ms':>8} {'bwd/fwd':>7}"]
    for side, Cc, heads in LEVELS:
        Tq, D = side * side, Cc // heads
        for kind, Tk in (("self", Tq), ("cross", CTX)):
            if kind == "self":
                qkv, dqkv = rn(B, Tq, 3 * Cc), torch.empty(B, Tq, 3 * Cc, device=d)
                q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
                dq, dk, dv = dqkv[..., :Cc], dqkv[..., Cc:2 * Cc], dqkv[..., 2 * Cc:]
            else:
                q, kv, dq, dkv = rn(B, Tq, Cc), rn(B, Tk, 2 * Cc), torch.empty(B, Tq, Cc, device=d), torch.empty(B, Tk, 2 * Cc, device=d)
                k, v, dk, dv = kv[..., :Cc], kv[..., Cc:], dkv[..., :Cc], dkv[..., Cc:]
            do = rn(B, Tq, Cc)
            o = T.attention_fwd32(q, k, v, heads)
            nbytes = lib.dm_f32_op_attention_bwd_workspace(B, heads, Tq, Tk, D)
            work = torch.empty(nbytes // 4, device=d)
            ts = (q, k, v, o, do, dq, dk, dv)
            ld, bs = T._attn_args(ts, B)
            ld8, bs8, s = (C.c_int32 * 8)(*ld), (C.c_int64 * 8)(*bs), T._stream()

            def bwd(phases):
                assert lib.dm_f32_op_attention_bwd_phases(s, *(T._p(t) for t in ts), ld8, bs8, None, B, heads, Tq, Tk, D, D ** -0.5, T._p(work), nbytes, phases) == 0
            bwd(15)
            pair = 4.0 * B * heads * Tq * Tk * D
            f = median_ms(lambda: T.attention_fwd32(q, k, v, heads), a.reps)
            ms = [median_ms(lambda ph=ph: bwd(ph), a.reps) for ph in (1, 2, 4, 8, 15)]
            tf = lambda pairs, m: pairs * pair / (m * 1e9)          # noqa: E731
            lines.append(f"{kind:>5} {Tq:>5} {Tk:>5} {D:>4} {lib.dm_f32_op_attention_bwd_slabs(Tq, Tk):>5} | {f:>8.3f} {tf(1, f):>6.1f} | {ms[0]:>8.3f} {tf(0.5, ms[0]):>6.1f} |"
                         f" {ms[1]:>8.3f} {tf(1.5, ms[1]):>6.1f} | {ms[2]:>8.3f} {tf(2, ms[2]):>6.1f} | {ms[3]:>7.3f} | {ms[4]:>8.3f} {ms[4] / f:>7.2f}")
    lines += ["", "# LayerNorm backward (three kernels), GB/s against 5 rows C fp32; GEGLU backward (F = 4 C), GB/s against 5 rows F fp32",
              f"{'rows':>6} {'C':>5} | {'ln ms':>8} {'GB/s':>7} | {'geglu ms':>8} {'GB/s':>7}"]
    for side, Cc, _ in LEVELS:
        rows, Fh = B * side * side, 4 * Cc
        x, dy, ga = rn(rows, Cc), rn(rows, Cc), rn(Cc)
        nbytes = lib.dm_f32_op_layernorm_bwd_workspace(rows, Cc)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=d)
        dx, dg, db = torch.empty_like(x), torch.empty_like(ga), torch.empty_like(ga)
        s = T._stream()

        def ln():
            assert lib.dm_f32_op_layernorm_bwd(s, T._p(x), T._p(dy), rows, Cc, T._p(ga), 1e-5, T._p(work), nbytes, T._p(dx), T._p(dg), T._p(db)) == 0
        p, dyg = rn(rows, 2 * Fh), rn(rows, Fh)
        dp = torch.empty_like(p)

        def gg():
            assert lib.dm_f32_op_geglu_bwd(s, T._p(p), T._p(dyg), rows, Fh, T._p(dp)) == 0
        m1, m2 = median_ms(ln, a.reps), median_ms(gg, a.reps)
        lines.append(f"{rows:>6} {Cc:>5} | {m1:>8.3f} {5.0 * rows * Cc * 4 / (m1 * 1e6):>7.1f} | {m2:>8.3f} {5.0 * rows * Fh * 4 / (m2 * 1e6):>7.1f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
