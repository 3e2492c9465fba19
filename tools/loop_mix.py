#!/usr/bin/env python
"""Instruction mix of a kernel's tile loop, from the device assembly (no GPU needed):
    python tools/loop_mix.py diff-mining_amd/csrc/attention_qk64.hip attn_qk64_kernel
Compiles with build.FLAGS plus -S --cuda-device-only into a temporary directory and counts, per basic block of the kernel's
loop (the blocks the compiler tags `in Loop` / `Loop Header`), MFMAs, v_exp, packs, v_max, permlanes, ds_read, LDS-DMA issues
and s_nop.  Blocks that only run on a lazy rescale are the small ones that multiply O; read them off the per-block lines."""
import importlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CATS = [("mfma", r"v_mfma"), ("v_exp", r"v_exp_f32"), ("cvt_pk", r"v_cvt_pk"), ("v_max", r"v_max"), ("permlane", r"v_permlane"),
        ("ds_read", r"ds_read"), ("global_load_lds", r"global_load_lds"), ("s_nop", r"s_nop"), ("ds_bpermute", r"ds_bpermute")]


def main():
    src, kernel = sys.argv[1], sys.argv[2]
    b = importlib.import_module("diff-mining_amd.build")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([b._hipcc()] + b.FLAGS + ["-S", "--cuda-device-only", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    sym = next(m.group(1) for m in re.finditer(r"^(\S+):\s*;\s*@", text, re.M) if kernel in m.group(1))
    body = text[text.index(sym + ":"):text.index(".Lfunc_end", text.index(sym + ":"))]
    blocks, cur = [], None
    for line in body.split("\n"):
        s = line.strip()
        m = re.match(r"^(\.LBB\w+):(.*)", s)
        if m:
            cur = [m.group(1), "Loop" in m.group(2), []]
            blocks.append(cur)
        elif cur is not None and s and not s.startswith((".", ";", "//")):
            cur[2].append(s)
    for name, in_loop, ins in blocks:
        if in_loop:
            c = {k: sum(1 for i in ins if re.match(p, i)) for k, p in CATS}
            print(f"{name}: {len(ins)} instructions; " + ", ".join(f"{k} {v}" for k, v in c.items() if v))


if __name__ == "__main__":
    main()
