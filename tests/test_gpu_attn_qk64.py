"""attention_qk64.hip: head_dim-40 self-attention with two 32-query sets per wave sharing each tile's K / V^T fragments.

The kernel keeps attention_qk32.hip's arithmetic per query (score chain, per-set max and rescale decisions, exp2 inputs, PV
order), so on the GPU its output must be bit-identical to qk32's (attn_pipe 6 vs 5), besides being close to fp32 SDPA.
One CPU test checks the compiled kernel's register budget: no spills, no scratch, at most 256 VGPRs (two waves per SIMD)."""
import importlib
import os
import re
import subprocess

import pytest
import torch

from tests import gpu_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS, D = 8, 40


def _lib():
    from diff_mining_amd import engine as E
    return E.load_library()


def _ref_fp32(q, k, v, slots=None):
    """softmax(q k^T / sqrt(D)) v per head in fp32 on the device, from the same fp16 inputs."""
    B, Tq, C = q.shape
    if slots is not None:
        k, v = k[slots.long()], v[slots.long()]
    Tk = k.shape[1]

    def split(t, T):
        return t.float().view(B, T, HEADS, D).transpose(1, 2)
    s = torch.matmul(split(q, Tq), split(k, Tk).transpose(-1, -2)) * D ** -0.5
    return torch.matmul(torch.softmax(s, dim=-1), split(v, Tk)).transpose(1, 2).reshape(B, Tq, C)


def _run(opt, q, k, v, slots=None):
    lib = _lib()
    try:
        assert lib.dm_set_option(b"attn_pipe", opt) == 0
        return U.op_attention(q, k, v, HEADS, slots=slots)
    finally:
        lib.dm_set_option(b"attn_pipe", 1)


def _inputs(B, Tq, Tk, seed, Bk=None):
    d = U.dev()
    C = HEADS * D
    q = U.f16_randn(B, Tq, C, seed=seed)
    k = U.f16_randn(Bk or B, Tk, C, seed=seed + 1)
    v = U.f16_randn(Bk or B, Tk, C, seed=seed + 2)
    return q.to(d), k.to(d), v.to(d)


def _check(q, k, v, what, slots=None):
    o64 = _run(6, q, k, v, slots)
    o32 = _run(5, q, k, v, slots)
    assert torch.equal(o64, o32), f"{what}: qk64 differs from qk32 in {(o64 != o32).sum().item()} elements"
    ref = _ref_fp32(q, k, v, slots)
    U.assert_close_fp16(o64, ref.cpu(), what, rel=3e-3, abs_frac=4e-3)
    return o64


@pytest.mark.gpu
@pytest.mark.parametrize("Tk", [256, 384, 512, 1024, 4096])
@pytest.mark.parametrize("Tq", [4096, 300, 256, 1000, 130, 64])
def test_qk64_bit_equal_to_qk32(Tq, Tk):
    """Ragged 256-query blocks, a last wave whose second set is empty (Tq % 64 <= 32), the minimum of four tiles."""
    q, k, v = _inputs(2, Tq, Tk, seed=41)
    _check(q, k, v, f"qk64 Tq={Tq} Tk={Tk}")


@pytest.mark.gpu
@pytest.mark.parametrize("Tq,Tk", [(4096, 4096), (300, 384), (130, 512)])
def test_qk64_rescale_in_one_set_only(Tq, Tk):
    """A late dominating key correlated with a query of set 0 only (query 7 of wave 0) and another, one tile earlier, with a
    query of set 1 only (query 40 of wave 0 = query 8 of its second set): each set's ballot fires on its own tile."""
    q, k, v = _inputs(2, Tq, Tk, seed=51)
    late = Tk - 90
    k[:, late] = q[:, 7] * 4.0
    k[:, late - 70] = q[:, 40] * 4.0
    k[:, 200, :D] = q[:, 100, :D] * 3.0      # head 0 only: query 100 = wave 1, set 1
    _check(q, k, v, f"qk64 one-set rescale Tq={Tq} Tk={Tk}")


@pytest.mark.gpu
@pytest.mark.parametrize("Tq,Tk", [(512, 1024), (300, 256)])
def test_qk64_all_negative_logits(Tq, Tk):
    """Every logit negative: the first tile must set each set's running max."""
    q, k, v = _inputs(2, Tq, Tk, seed=61)
    _check(q.abs(), -k.abs(), v, f"qk64 negative logits Tq={Tq} Tk={Tk}")


@pytest.mark.gpu
def test_qk64_prompt_slots():
    """K / V of the prompt slot of each sample (the bench's slot batch: samples share a prompt's K / V rows)."""
    q, k, v = _inputs(6, 1000, 512, seed=71, Bk=2)
    slots = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32, device=U.dev())
    _check(q, k, v, "qk64 prompt slots", slots=slots)


@pytest.mark.gpu
def test_qk64_deterministic_and_batch_independent():
    q, k, v = _inputs(3, 1000, 1024, seed=81)
    o = _run(6, q, k, v)
    o2 = _run(6, q, k, v)
    o1 = _run(6, q[1:2].contiguous(), k[1:2].contiguous(), v[1:2].contiguous())
    assert torch.equal(o, o2)
    assert torch.equal(o1[0], o[1])


@pytest.mark.gpu
def test_qk64_option_value():
    lib = _lib()
    try:
        assert lib.dm_set_option(b"attn_pipe", 6) == 0
        assert lib.dm_set_option(b"attn_pipe", 7) == 2
        assert lib.dm_set_option(b"attn_pipe", 4) == 2
    finally:
        lib.dm_set_option(b"attn_pipe", 1)


def test_qk64_registers_no_spills(tmp_path):
    """The kernel's code-object metadata: no VGPR / SGPR spills, no scratch, at most 256 VGPRs (two waves per SIMD)."""
    b = importlib.import_module("diff-mining_amd.build")
    out = tmp_path / "attention_qk64.s"
    src = os.path.join(b.CSRC, "attention_qk64.hip")
    subprocess.run([b._hipcc()] + b.FLAGS + ["-S", "--cuda-device-only", "-o", str(out), src], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    kern = [m for m in re.finditer(r"\.name:\s+(\S+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                                   text, re.S) if "attn_qk64_kernel" in m.group(1)]
    assert len(kern) == 1, "attn_qk64_kernel metadata not found"
    m = kern[0]
    assert int(m.group(4)) == 0, f"VGPR spills: {m.group(4)}"
    assert int(m.group(2)) == 0, f"SGPR spills: {m.group(2)}"
    assert int(m.group(3)) <= 256, f"{m.group(3)} VGPRs"
    scratch = re.findall(r"ScratchSize:\s*(\d+)", text)
    assert scratch and all(int(s) == 0 for s in scratch), f"scratch: {scratch}"
