#!/usr/bin/env python
"""Rates of the training operators at the U-Net's ResNet shapes: a training batch of 4 at a 64 x 64 latent.

For every 3x3 convolution shape of the ResNet blocks, in ONE process: the forward gemm32, the data-gradient launch (gemm32 on dgrad_weights)
and wgrad32 (both kernels: slabs + the ascending sum), device events, median of 20.  Also the GroupNorm backward in GB/s against its bytes
(x and dy read twice, dx written once) and what the zero-insert route costs the three down-samplers over a convolution of the stride-2
multiply-add count.  Writes the table to --out (default profiles/train_ops_rate.txt).  Records; gates nothing.

    python tools/train_ops_rate.py [--batch 4] [--latent 64] [--reps 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from diff_mining_amd import engine as E  # noqa: E402
from diff_mining_amd import train as T  # noqa: E402

# (level divisor, Cin, Cout) of every distinct 3x3 convolution of the ResNet blocks of the SD 1.5 U-Net (conv1 of each block, and conv2 = Cout -> Cout)
RESNET_CONVS = [(1, 320, 320), (1, 640, 320), (1, 960, 320), (2, 320, 640), (2, 640, 640), (2, 960, 640), (2, 1280, 640), (2, 1920, 640),
                (4, 640, 1280), (4, 1280, 1280), (4, 1920, 1280), (4, 2560, 1280), (8, 1280, 1280), (8, 2560, 1280)]
DOWNSAMPLERS = [(1, 320), (2, 640), (4, 1280)]
GROUPNORMS = [(1, 320, 0), (1, 640, 320), (2, 640, 0), (2, 1280, 640), (4, 1280, 0), (8, 1280, 1280)]


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
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_ops_rate.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = E.load_library()
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)          # noqa: E731
    N = a.batch
    lines = [f"# tools/train_ops_rate.py: batch {N}, latent {a.latent} x {a.latent}, median of {a.reps}, device events, one process; {torch.cuda.get_device_name(0)}",
             "# 3x3 convolutions of the ResNet blocks (mode 1): TFLOP/s of the forward gemm32, the data gradient (gemm32 on dgrad_weights) and wgrad32",
             f"{'HxW':>7} {'Cin':>5} {'Cout':>5} {'slabs':>5} | {'fwd ms':>8} {'TF/s':>6} | {'dgrad ms':>8} {'TF/s':>6} | {'wgrad ms':>8} {'TF/s':>6} | {'wgrad/fwd':>9}"]
    tot = [0.0, 0.0, 0.0]
    for div, cin, cout in RESNET_CONVS:
        H = a.latent // div
        x, dy, wp = rn(N, H, H, cin), rn(N, H, H, cout), rn(cout, 9 * cin) * (9 * cin) ** -0.5
        wd = T.dgrad_weights(wp, 1, pad_to=32)
        flops = 2.0 * N * H * H * 9 * cin * cout
        nbytes = lib.dm_f32_op_gemm_wgrad_workspace(N, H, H, H, H, cin, cout, 1)
        slabs = nbytes // (4 * cout * 9 * cin)
        work, dw = torch.empty(nbytes // 4, device=d), torch.empty(cout, 9 * cin, device=d)
        s = T._stream()

        def wgrad():
            assert lib.dm_f32_op_gemm_wgrad(s, T._p(x), None, T._p(dy), T._p(dw), T._p(work), nbytes, N, H, H, H, H, cin, cin, cout, 1, 0) == 0
        ms = [median_ms(lambda: T.gemm32(x, None, wp, None, None, None, 1), a.reps), median_ms(lambda: T.gemm32(dy, None, wd, None, None, None, 1), a.reps),
              median_ms(wgrad, a.reps)]
        tf = [flops / (m * 1e9) for m in ms]
        tot = [t + m for t, m in zip(tot, ms)]
        lines.append(f"{H:>3}x{H:<3} {cin:>5} {cout:>5} {slabs:>5} | {ms[0]:>8.3f} {tf[0]:>6.1f} | {ms[1]:>8.3f} {tf[1]:>6.1f} | {ms[2]:>8.3f} {tf[2]:>6.1f} | {tf[2] / tf[0]:>9.2f}")
        del x, dy, wp, wd, work, dw
    lines.append(f"{'sum':>25} | {tot[0]:>8.3f} {'':>6} | {tot[1]:>8.3f} {'':>6} | {tot[2]:>8.3f} {'':>6} | {tot[0] / tot[2]:>9.2f}")
    lines += ["", "# Downsample2D (3x3 stride 2): data gradient = zero_insert2 + a mode-1 gemm32 on the H x W grid (4x the multiply-adds of the stride-2 convolution);",
              "# 'extra' = that route minus the forward mode-2 gemm32 of the same layer (the time a gradient kernel of the stride-2 multiply-add count would take)",
              f"{'HxW':>7} {'C':>5} | {'fwd ms':>8} | {'insert ms':>9} {'gemm ms':>8} {'route ms':>8} | {'extra ms':>8} | {'wgrad ms':>8}"]
    for div, c in DOWNSAMPLERS:
        H = a.latent // div
        x, dy, wp = rn(N, H, H, c), rn(N, H // 2, H // 2, c), rn(c, 9 * c) * (9 * c) ** -0.5
        wd = T.dgrad_weights(wp, 2, pad_to=32)
        z = T.zero_insert2(dy, H, H)
        f = median_ms(lambda: T.gemm32(x, None, wp, None, None, None, 2), a.reps)
        zi = median_ms(lambda: T.zero_insert2(dy, H, H), a.reps)
        gm = median_ms(lambda: T.gemm32(z, None, wd, None, None, None, 1), a.reps)
        route = median_ms(lambda: T.dgrad32(dy, wp, 2, x.shape, c), a.reps)          # includes the weight repack, as a training step pays it
        wg = median_ms(lambda: T.wgrad32(x, None, dy, 2), a.reps)
        lines.append(f"{H:>3}x{H:<3} {c:>5} | {f:>8.3f} | {zi:>9.3f} {gm:>8.3f} {route:>8.3f} | {zi + gm - f:>8.3f} | {wg:>8.3f}")
        del x, dy, wp, wd, z
    lines += ["", "# GroupNorm(32) + SiLU backward (three kernels), GB/s against 5 N HW C fp32 (x and dy read by both passes, dx written once)",
              f"{'HxW':>7} {'C1':>5} {'C2':>5} | {'ms':>8} {'GB/s':>7}"]
    for div, c1, c2 in GROUPNORMS:
        H = a.latent // div
        c = c1 + c2
        xa, xb = rn(N, H, H, c1), (rn(N, H, H, c2) if c2 else None)
        dy, ga, be = rn(N, H, H, c), rn(c), rn(c)
        st, y = torch.empty(N * 32, 2, device=d), torch.empty(N, H, H, c, device=d)
        s = T._stream()
        assert lib.dm_f32_op_groupnorm(s, T._p(xa), T._p(xb), N, H * H, c, c1, 32, 1e-5, T._p(ga), T._p(be), 1, T._p(st), T._p(y)) == 0
        work = torch.empty(2 * (N * c + N * 32), dtype=torch.float64, device=d)
        dxa, dxb, dg, db = torch.empty_like(xa), (torch.empty_like(xb) if c2 else None), torch.empty_like(ga), torch.empty_like(be)

        def gn():
            assert lib.dm_f32_op_groupnorm_bwd(s, T._p(xa), T._p(xb), T._p(dy), N, H * H, c, c1, 32, T._p(ga), T._p(be), T._p(st), 1, T._p(work), work.numel() * 8,
                                               T._p(dxa), T._p(dxb), T._p(dg), T._p(db)) == 0
        ms = median_ms(gn, a.reps)
        lines.append(f"{H:>3}x{H:<3} {c1:>5} {c2:>5} | {ms:>8.3f} {5.0 * N * H * H * c * 4 / (ms * 1e6):>7.1f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
