"""CPU tier: the C-ABI library builds, loads and exports every symbol include/dm_engine.h declares;
host-only entry points agree with the oracle; the product path fails loudly without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from diff_mining_amd import engine as E
from oracle import unet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        from diff_mining_amd import build
        build.build()
    return E.load_library()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(E.SYMBOLS), declared ^ set(E.SYMBOLS)
    for s in declared:
        assert hasattr(lib, s), f"{s} declared in include/dm_engine.h but not exported"
    assert b"gfx950" in lib.dm_version()


def _header_signatures():
    """name -> (return kind, [argument kinds]) of every dm_* declaration of include/dm_engine.h (plain C, comments stripped)."""
    hdr = open(os.path.join(ROOT, "include", "dm_engine.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    scalar = {"float": "f32", "double": "f64", "int64_t": "i64", "size_t": "size", "int": "i32", "int32_t": "i32"}
    out = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(dm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M):
        ret = {"const char *": "char_p", "size_t": "size", "void": "void", "int": "i32"}[" ".join(ret.replace("*", " * ").split())]
        args = [] if args.strip() == "void" else args.split(",")
        out[name] = (ret, ["ptr" if "*" in a else scalar[" ".join(a.split()[:-1])] for a in args])
    return out


def _ctypes_kind(t):
    C = E.C
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if t in (C.c_float, C.c_double, C.c_size_t):
        return {C.c_float: "f32", C.c_double: "f64", C.c_size_t: "size"}[t]
    assert t._type_ in "ilq", t                   # a signed integer: told apart by its width
    return {4: "i32", 8: "i64"}[C.sizeof(t)]


def _signature_mismatches(table):
    """Every way `table` (name -> (restype, argtypes)) disagrees with the header: count, kind per argument, kind of the return."""
    bad = []
    declared = _header_signatures()
    if set(declared) != set(table):
        bad.append(("symbols", sorted(set(declared) ^ set(table))))
    for name, (ret, kinds) in declared.items():
        if name not in table:
            continue
        restype, argtypes = table[name]
        got_ret = "char_p" if restype is E.C.c_char_p else _ctypes_kind(restype)
        got = [_ctypes_kind(t) for t in argtypes]
        if got_ret != ret:
            bad.append((name, "returns", got_ret, ret))
        if got != kinds:
            bad.append((name, got, kinds))
    return bad


def test_signature_table_matches_the_header():
    """Argument count, the kind of every argument (pointer / fp32 / fp64 / 32-bit / 64-bit integer / size_t) and the return kind of
    every symbol, table against header.  (Checked the same way, the lists the binding carried before the table had no mismatch; two
    symbols, dm_version and dm_op_igemm_head_rows, had no list at all.)"""
    declared = _header_signatures()
    assert len(declared) >= 92 and declared["dm_version"] == ("char_p", [])
    assert declared["dm_xray_eval_workspace_bytes"] == ("size", ["i32", "i32", "i64"])
    assert declared["dm_kmeans_fit"][1][8:11] == ["f32", "ptr", "size"] and declared["dm_engine_destroy"][0] == "void"
    assert E.SYMBOLS == list(E.SIGNATURES)
    assert _signature_mismatches(E.SIGNATURES) == []


def test_signature_check_sees_a_wrong_entry():
    """The comparison itself: one i32 too few, an i32 where the header says int64_t, a pointer for a float, a wrong return type."""
    C = E.C
    for name, edit in (("dm_score", lambda r, a: (r, a[:-3] + a[-2:])),
                       ("dm_normalize_map", lambda r, a: (r, a[:2] + [C.c_int] + a[3:])),
                       ("dm_op_attention", lambda r, a: (r, a[:9] + [C.c_int] + a[10:])),
                       ("dm_op_layernorm", lambda r, a: (r, a[:6] + [C.c_void_p] + a[7:])),
                       ("dm_xray_eval_workspace_bytes", lambda r, a: (C.c_int, a)),
                       ("dm_f32_destroy", lambda r, a: (C.c_int, a))):
        table = dict(E.SIGNATURES)
        table[name] = edit(table[name][0], list(table[name][1]))
        bad = _signature_mismatches(table)
        assert len(bad) == 1 and bad[0][0] == name, (name, bad)
    table = dict(E.SIGNATURES)
    del table["dm_mine_parallel"]
    assert _signature_mismatches(table) == [("symbols", ["dm_mine_parallel"])]


def test_load_library_applies_the_whole_table(lib):
    """Every symbol carries its table entry once the library is loaded — the k-means and X-ray ones too, whether or not the modules
    that call them have been imported."""
    for name, (restype, argtypes) in E.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name
    for name in ("dm_kmeans_workspace_bytes", "dm_kmeans_fit", "dm_cluster_rank", "dm_xray_eval_workspace_bytes", "dm_xray_eval"):
        assert name in E.SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.dm_xray_eval_workspace_bytes.restype is E.C.c_size_t


def test_scheduler_table_matches_oracle(lib):
    a = E.scheduler_alphas_cumprod()
    b = R.alphas_cumprod().numpy()
    assert np.abs(a - b).max() < 1e-7
    assert np.array_equal(a.astype(np.float16), b.astype(np.float16))     # identical after the fp16 cast (R3)
    for t, v in {0: 0.99914998, 161: 0.81210744, 261: 0.65566903, 500: 0.27633247, 999: 0.00466010}.items():
        assert abs(float(a[t]) - v) < 2e-7


def test_sinusoid_matches_oracle(lib):
    worst = 0.0
    for t in (0, 1, 161, 261, 500, 999):
        s = E.timestep_sinusoid(t)
        r = R.timestep_sinusoid(torch.tensor([t]))[0].numpy()
        worst = max(worst, float(np.abs(s - r).max()))
    assert worst < 1e-4      # fp32 argument rounding at t*f ~ 1e3; fp16 ulp near 1 is 4.9e-4
    np.testing.assert_allclose(E.timestep_sinusoid(161)[:2], [-0.71177477, 0.36481935], atol=2e-5)


def test_dift_shape(lib):
    assert E.dift_shape(64, 64, 1) == (1280, 32, 32)       # DIFT-161 tap: up_blocks[1] incl. its upsampler
    assert E.dift_shape(64, 64, 0) == (1280, 16, 16)
    assert E.dift_shape(64, 64, 2) == (640, 64, 64)
    assert E.dift_shape(64, 64, 3) == (320, 64, 64)
    assert E.dift_shape(32, 42, 1) == (1280, 16, 21)       # odd sizes follow the skip tensor (upsample_size)


def test_engine_fails_loudly_without_gpu(lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(E.EngineError):
        E.UNetEngine(0)
    h = E.C.c_void_p()
    assert lib.dm_engine_create(0, E.C.byref(h)) != 0
    assert b"no HIP device" in lib.dm_last_error(None) or b"fallback" in lib.dm_last_error(None)


def test_missing_library_is_an_error(tmp_path):
    with pytest.raises(E.EngineError):
        E.load_library(str(tmp_path / "nope.so"))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "diff-mining_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("the oracle", "").replace("CPU oracle", ""), f


def test_tap_reuse_kernels_do_not_spill():
    """igemm_pers_tr.hip picks, per instantiation, the unrolled or the run-time-dx form of its k loop by whether the register
    allocator handles it without spilling (a spilled accumulator is reloaded inside the k loop, behind the LDS-DMA on vmcnt).
    That list is a property of the compiler, so it is checked against the compiled ISA: every instantiation of the kernel that
    the library ships must have no spilled VGPR."""
    import importlib
    import re
    import subprocess
    import tempfile
    b = importlib.import_module("diff-mining_amd.build")
    src = os.path.join(os.path.dirname(b.__file__), "csrc", "igemm_pers_tr.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "tr.s")
        subprocess.run([b._hipcc()] + b.FLAGS + ["-S", "--cuda-device-only", "-o", out, src], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*igemm_pers_tr_kernel\S*).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert len(found) == 13, found
    spilled = [(n, int(c)) for n, c in found if int(c) != 0]
    assert not spilled, f"tap-reuse kernels with spilled registers (move them to the run-time-dx loop: TrUnroll): {spilled}"
    # the folded up-sampler (igemm_pers_up.hip, template parameter UP4 of the persistent tile) carries a parity class and a scattering
    # epilogue on top of the plain kernel's state: same check
    src = os.path.join(os.path.dirname(b.__file__), "csrc", "igemm_pers_up.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "up.s")
        subprocess.run([b._hipcc()] + b.FLAGS + ["-S", "--cuda-device-only", "-o", out, src], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    found = re.findall(r"\.name:\s+(\S*igemm_pers_kernelILi0ELb0ELi0ELb0ELb0ELb1E\S*).*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert len(found) == 1 and int(found[0][1]) == 0, found


# The attention route of every product shape (the table of DESIGN.md 4m): (latent h, w) -> the self-attention layers at head_dim 40 / 80
# / 160 (the mid block is head_dim 160 one level further down) and the 77-key cross-attention of the same query counts.
def _levels(h, w):
    out = [(h, w)]
    for _ in range(3):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return [a * b for a, b in out]        # tokens at head_dim 40, 80, 160 and the mid block (160)


ATTN_ROUTE_TABLE = [
    # latent, self D40, D80, D160 (down / up and mid)
    ((64, 64), "qk64", "pipe80", "d160", "d160"),
    ((64, 85), "generic40", "generic80", "generic160", "generic160"),
    ((85, 64), "generic40", "generic80", "generic160", "generic160"),
    ((32, 42), "generic40", "generic80", "generic160", "generic160"),
    ((42, 32), "generic40", "generic80", "generic160", "generic160"),
    ((32, 40), "qk64", "generic80", "d160_cross", "generic160"),      # 1280 / 320 / 80 / 20: 80 keys are inside the resident-K/V range
    ((32, 56), "qk64", "generic80", "generic160", "generic160"),      # 1792 / 448 / 112 / 28
]


def _route(lib, B, heads, Tq, Tk, D, q_mod=0):
    from tests.gpu_util import ATTN_ROUTES
    return ATTN_ROUTES[lib.dm_op_attention_route(B, heads, Tq, Tk, D, q_mod)]


@pytest.fixture
def default_attn_options(lib):
    for name in (b"attn_pipe", b"attn_cross"):
        v = E.C.c_int(-99)
        assert lib.dm_get_option(name, E.C.byref(v)) == 0 and v.value == 1, (name, v.value)
    yield
    assert lib.dm_set_option(b"attn_pipe", 1) == 0 and lib.dm_set_option(b"attn_cross", 1) == 0


@pytest.mark.parametrize("latent,r40,r80,r160,rmid", ATTN_ROUTE_TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_attention_route_of_the_work_list_shapes(lib, default_attn_options, latent, r40, r80, r160, rmid):
    """dm_op_attention_route is the one decision launch_attention switches on.  At the work list's latents (compute_worklist: 32 x
    40...56 landscapes and 42 x 32 portraits of the cars rule, 64 x 85 / 85 x 64 of the places rule) Tk % 128 != 0 keeps the fast
    self-attention kernels off, so the generic kernel runs there: a predicate change that moves any of these shapes shows here."""
    t40, t80, t160, tmid = _levels(*latent)
    B = 20
    assert _route(lib, B, 8, t40, t40, 40) == r40
    assert _route(lib, B, 8, t80, t80, 80) == r80
    assert _route(lib, B, 8, t160, t160, 160) == r160
    assert _route(lib, B, 8, tmid, tmid, 160) == rmid
    # cross-attention (77 keys): the resident-K/V kernels from 256 queries at head_dim 40 / 80, at every query count at 160
    assert _route(lib, B, 8, t40, 77, 40) == ("cross" if t40 >= 256 else "generic40")
    assert _route(lib, B, 8, t80, 77, 80) == ("cross" if t80 >= 256 else "generic80")
    assert _route(lib, B, 8, t160, 77, 160) == "d160_cross"
    assert _route(lib, B, 8, tmid, 77, 160) == "d160_cross"
    # shared-draw mode (q_mod > 0): the Q-modulo layout is read by the cross kernels and the generic kernel only
    assert _route(lib, B, 8, t40, 77, 40, q_mod=10) == ("cross" if t40 >= 256 else "generic40")
    assert _route(lib, B, 8, t160, 77, 160, q_mod=10) == "d160_cross"
    assert _route(lib, B, 8, t40, t40, 40, q_mod=10) == "generic40"
    assert _route(lib, B, 8, t160, t160, 160, q_mod=10) == ("d160_cross" if r160 == "d160_cross" else "generic160")
    # attn_cross = 0: every cross-attention on the generic kernel
    assert lib.dm_set_option(b"attn_cross", 0) == 0
    for T, D in ((t40, 40), (t80, 80), (t160, 160), (tmid, 160)):
        assert _route(lib, B, 8, T, 77, D) == f"generic{D}"


def test_attention_route_options_move_routes_as_documented(lib, default_attn_options):
    """The A/B values of attn_pipe at the 64 x 64 shapes and at 16384 keys (the 128 x 128 level): 9 = the r04 dispatch (attn_pipe_kernel
    / pipe80, the generic kernel at head_dim 160), 5 = qk32, 6 = qk64, 10 / 12 = the anti-phase kernel, 2 = head_dim-40 pipelining only,
    0 = the generic kernel everywhere; Tk = 65 / 80 are inside the resident-K/V kernels' (64, 80] range, 64 and 81 outside it."""
    r = lambda Tq, Tk, D, B=2: _route(lib, B, 8, Tq, Tk, D)        # noqa: E731
    assert (r(16384, 16384, 40), r(4096, 4096, 40), r(1024, 1024, 80), r(256, 256, 160), r(64, 64, 160)) == \
        ("pp12", "qk64", "pipe80", "d160", "d160")
    assert (r(5440, 5440, 40), r(1376, 1376, 80), r(352, 352, 160)) == ("generic40", "generic80", "generic160")
    assert (r(256, 65, 40), r(256, 80, 80), r(24, 65, 160), r(352, 80, 160)) == ("cross", "cross", "d160_cross", "d160_cross")
    assert (r(255, 77, 40), r(256, 64, 40), r(256, 81, 80), r(88, 64, 160), r(88, 81, 160)) == \
        ("generic40", "generic40", "generic80", "d160", "generic160")
    expect = {9: ("pipe", "pipe", "pipe80", "generic160", "generic160"), 5: ("qk32", "qk32", "pipe80", "d160", "d160"),
              6: ("qk64", "qk64", "pipe80", "d160", "d160"), 10: ("pp10", "pp10", "pipe80", "generic160", "generic160"),
              12: ("pp12", "pp12", "pipe80", "generic160", "generic160"), 2: ("pipe", "pipe", "generic80", "generic160", "generic160"),
              3: ("pipe", "pipe", "pipe80", "generic160", "generic160"),
              0: ("generic40", "generic40", "generic80", "generic160", "generic160")}
    for pipe, routes in expect.items():
        assert lib.dm_set_option(b"attn_pipe", pipe) == 0
        got = (r(16384, 16384, 40), r(4096, 4096, 40), r(1024, 1024, 80), r(256, 256, 160), r(64, 64, 160))
        assert got == routes, (pipe, got)
        assert (r(4096, 77, 40), r(352, 77, 160)) == ("cross", "d160_cross")       # attn_pipe does not move cross-attention
    assert lib.dm_set_option(b"attn_pipe", 1) == 0
    assert r(0, 77, 40) == "none" and r(64, 64, 64) == "none" and r(64, 64, 40, B=0) == "none"
