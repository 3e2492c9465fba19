#!/usr/bin/env python
"""Instruction mix of a kernel's tile loop, from the device assembly (no GPU needed):
    python tools/loop_mix.py diff-mining_amd/csrc/attention_qk64.hip attn_qk64_kernel
Compiles with build.FLAGS plus -S --cuda-device-only into a temporary directory and counts, per basic block of the kernel's
loop (the blocks the compiler tags `in Loop` / `Loop Header`), MFMAs, v_exp, packs, v_max, permlanes, ds_read, LDS-DMA issues
and s_nop.  Blocks that only run on a lazy rescale are the small ones that multiply O; read them off the per-block lines.

    python tools/loop_mix.py --classes diff-mining_amd/csrc/igemm_pers.hip igemm_pers_kernel [-DNAME ...]
counts the WHOLE body of every basic block of a loop that holds MFMAs (blocks entered by falling through, which carry no
label, are split off: the code after a k step's MFMAs that runs once per tile is not part of the step), for every kernel
whose symbol contains the name; with --all-blocks instead of --classes also the loop blocks without MFMAs, one line each, so that
the path of a steady-state step can be added up by following the branches: MFMA / other VALU /
SALU / ds_ / LDS-DMA / other memory / waits (s_waitcnt, s_barrier, s_nop), the kernel's registers and spills from the code-object
metadata, and the run-length order string of the classes (M v s d L g w).  A plain classifier by instruction-name prefix:
everything that starts with v_ and is no MFMA is "other VALU", everything that starts with s_ and is no wait is SALU."""
import importlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CATS = [("mfma", r"v_mfma"), ("v_exp", r"v_exp_f32"), ("cvt_pk", r"v_cvt_pk"), ("v_max", r"v_max"), ("permlane", r"v_permlane"),
        ("ds_read", r"ds_read"), ("global_load_lds", r"global_load_lds"), ("s_nop", r"s_nop"), ("ds_bpermute", r"ds_bpermute")]
# first match wins: (class, letter of the order string, prefix)
CLASSES = [("mfma", "M", r"v_mfma"), ("lds_dma", "L", r"global_load_lds|buffer_load\S*\s.*\blds\b"), ("ds", "d", r"ds_"),
           ("wait", "w", r"s_waitcnt|s_barrier|s_nop"), ("valu", "v", r"v_"), ("salu", "s", r"s_"), ("mem", "g", r"global_|buffer_|flat_|scratch_")]


def assembly(src, extra=()):
    b = importlib.import_module("diff-mining_amd.build")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([b._hipcc()] + b.FLAGS + ["-S", "--cuda-device-only", "-o", out, src] + list(extra), check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def loop_blocks(text, sym, split_fallthrough=False):
    body = text[text.index(sym + ":"):text.index(".Lfunc_end", text.index(sym + ":"))]
    blocks, cur = [], None
    for line in body.split("\n"):
        s = line.strip()
        m = re.match(r"^(\.LBB\w+):(.*)", s)
        if m is None and split_fallthrough:          # "; %bb.7:   in Loop: ..." — a block entered by falling through has no label
            m = re.match(r"^; (%bb\.\d+):(.*)", s)
        if m:
            cur = [m.group(1), "Loop" in m.group(2), []]
            blocks.append(cur)
        elif cur is not None and s and not s.startswith((".", ";", "//")):
            cur[2].append(s)
    return blocks


def classify(ins):
    for name, letter, pat in CLASSES:
        if re.match(pat, ins):
            return name, letter
    return "other", "?"


def order_string(letters):
    out, i = [], 0
    while i < len(letters):
        j = i
        while j < len(letters) and letters[j] == letters[i]:
            j += 1
        out.append(letters[i] + (str(j - i) if j - i > 1 else ""))
        i = j
    return " ".join(out)


def demangled(sym):
    r = subprocess.run(["c++filt", sym], capture_output=True, text=True)
    name = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else sym
    return re.sub(r"^void dm::\(anonymous namespace\)::|\(dm::IGemmParams.*$", "", name)


def classes_main(argv, all_blocks=False):
    src, kernel, extra = argv[0], argv[1], argv[2:]
    text = assembly(src, extra)
    meta = {m.group(1): (int(m.group(3)), int(m.group(4)), int(m.group(2)))
            for m in re.finditer(r"\.name:\s+(\S+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)}
    syms = [m.group(1) for m in re.finditer(r"^(\S+):\s*;\s*@", text, re.M) if kernel in m.group(1)]
    for sym in syms:
        vg, vs, ss = meta.get(sym, (-1, -1, -1))
        print(f"{demangled(sym)}: vgpr {vg}, vgpr spills {vs}, sgpr spills {ss}")
        for name, in_loop, ins in loop_blocks(text, sym, True):
            cl = [classify(i) for i in ins]
            n = {k: sum(1 for c, _ in cl if c == k) for k in [c[0] for c in CLASSES] + ["other"]}
            if not in_loop or (n["mfma"] == 0 and not all_blocks) or not ins:
                continue
            if n["mfma"] == 0:
                print(f"  {name}: valu {n['valu']}, salu {n['salu']}, ds {n['ds']}, lds_dma {n['lds_dma']}, mem {n['mem']}, wait {n['wait']}; ends {ins[-1].split()[0]} {ins[-1].split()[-1] if 'branch' in ins[-1] else ''}")
                continue
            print(f"  {name}: {len(ins)} instructions; mfma {n['mfma']}, valu {n['valu']}, salu {n['salu']}, ds {n['ds']}, lds_dma {n['lds_dma']}, "
                  f"mem {n['mem']}, wait {n['wait']}" + (f", other {n['other']}" if n["other"] else ""))
            print("    order: " + order_string([l for _, l in cl]))


def main():
    if sys.argv[1] in ("--classes", "--all-blocks"):
        return classes_main(sys.argv[2:], sys.argv[1] == "--all-blocks")
    src, kernel = sys.argv[1], sys.argv[2]
    text = assembly(src)
    sym = next(m.group(1) for m in re.finditer(r"^(\S+):\s*;\s*@", text, re.M) if kernel in m.group(1))
    for name, in_loop, ins in loop_blocks(text, sym):
        if in_loop:
            c = {k: sum(1 for i in ins if re.match(p, i)) for k, p in CATS}
            print(f"{name}: {len(ins)} instructions; " + ", ".join(f"{k} {v}" for k, v in c.items() if v))


if __name__ == "__main__":
    main()
