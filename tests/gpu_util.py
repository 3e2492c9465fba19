"""Helpers shared by the GPU parity tests: packing to the engine's layouts and error metrics."""
import ctypes as C

import numpy as np
import torch

from diff_mining_amd import engine as E


def dev():
    return torch.device("cuda", 0)


def f16_randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def to_nhwc(x):          # [N,C,H,W] -> [N,H,W,C] contiguous
    return x.permute(0, 2, 3, 1).contiguous()


def to_nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def pack_conv3(w):       # [Cout,Cin,3,3] -> [Cout, 9*Cin], k = (tap, cin)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def pack_geglu(w, b):    # [8C, C] -> quad-interleaved rows (see engine_pack.hip pack_geglu)
    c8 = w.shape[0]
    c4 = c8 // 2
    rho = torch.arange(c8)
    F, q, r = rho // 16, (rho % 16) // 4, rho % 4
    src = torch.where(r < 2, 8 * F + 2 * q + r, c4 + 8 * F + 2 * q + (r - 2))
    return w[src].contiguous(), b[src].contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def op_igemm(X, W, bias=None, X2=None, temb=None, res=None, mode=0, epi=0, OH=None, OW=None, sync=True):
    """X [N,H,W,C1] fp16 cuda; W packed [Cout, taps*Cin] fp16 cuda -> Y [N,OH,OW,Cout(/2)]"""
    lib = E.load_library()
    N, H, Wd, C1 = X.shape
    C2 = X2.shape[3] if X2 is not None else 0
    Cout = W.shape[0]
    OH = H if OH is None else OH
    OW = Wd if OW is None else OW
    cy = Cout // 2 if epi == 1 else Cout
    Y = torch.empty(N, OH, OW, cy, dtype=torch.float16, device=X.device)
    rc = lib.dm_op_igemm(stream(), ptr(X), ptr(X2), ptr(W), ptr(bias), ptr(temb), ptr(res), ptr(Y),
                         N, H, Wd, C1, C2, Cout, OH, OW, mode, epi, temb.stride(0) if temb is not None else 0)
    assert rc == 0, "dm_op_igemm failed"
    if sync:
        torch.cuda.synchronize()
    return Y


def attention_route(B, heads, Tq, Tk, D, q_mod=0):
    """the kernel dm_op_attention takes for this shape under the current options (name of ATTN_ROUTES)"""
    return ATTN_ROUTES[E.load_library().dm_op_attention_route(B, heads, Tq, Tk, D, q_mod)]


# enum AttnRoute (dm_kernels.h; the numbers of dm_op_attention_route in include/dm_engine.h)
ATTN_ROUTES = ["none", "generic40", "generic80", "generic160", "qk32", "qk64", "pipe", "pipe80", "pp10", "pp12", "d160",
               "d160_cross", "cross", "pp_ablate"]


def op_attention(Q, K, V, heads, slots=None, B=None, slot_div=0, n_slots=0, q_mod=0):
    """Q [Bq,Tq,C], K/V [Bk,Tk,C] fp16 cuda -> O [B,Tq,C] (B = Bq unless given: with q_mod > 0, sample b reads Q[b % q_mod]);
    K/V of sample b: slots[b], else b // slot_div if slot_div > 0, else b; clamped to [0, n_slots) if n_slots > 0"""
    lib = E.load_library()
    Bq, Tq, Cc = Q.shape
    B = Bq if B is None else B
    Tk = K.shape[1]
    D = Cc // heads
    O = torch.empty(B, Tq, Cc, dtype=Q.dtype, device=Q.device)
    if slot_div or n_slots or q_mod:
        rc = lib.dm_op_attention_slots(stream(), ptr(Q), ptr(K), ptr(V), ptr(O), Q.stride(1), K.stride(1), V.stride(1), Cc,
                                       Q.stride(0), K.stride(0), V.stride(0), Tq * Cc, ptr(slots), slot_div, n_slots, q_mod,
                                       B, heads, Tq, Tk, D, float(D) ** -0.5)
    else:
        assert B == Bq
        rc = lib.dm_op_attention(stream(), ptr(Q), ptr(K), ptr(V), ptr(O), Q.stride(1), K.stride(1), V.stride(1), Cc,
                                 Q.stride(0), K.stride(0), V.stride(0), Tq * Cc, ptr(slots), B, heads, Tq, Tk, D,
                                 float(D) ** -0.5)
    assert rc == 0, "dm_op_attention failed"
    torch.cuda.synchronize()
    return O


def op_groupnorm(X, gamma, beta, G, eps, silu, X2=None):
    lib = E.load_library()
    N, H, Wd, C1 = X.shape
    Ct = C1 + (X2.shape[3] if X2 is not None else 0)
    Y = torch.empty(N, H, Wd, Ct, dtype=torch.float16, device=X.device)
    rc = lib.dm_op_groupnorm(stream(), ptr(X), ptr(X2), N, H * Wd, Ct, C1, G, eps, ptr(gamma), ptr(beta),
                             1 if silu else 0, ptr(Y))
    assert rc == 0
    torch.cuda.synchronize()
    return Y


def op_layernorm(X, gamma, beta, eps=1e-5):
    lib = E.load_library()
    rows, Cc = X.shape
    Y = torch.empty_like(X)
    rc = lib.dm_op_layernorm(stream(), ptr(X), rows, Cc, ptr(gamma), ptr(beta), eps, ptr(Y))
    assert rc == 0
    torch.cuda.synchronize()
    return Y


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def max_abs(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def assert_close_fp16(got, ref, what, rel=2e-3, abs_frac=2e-3):
    """fp16-output op vs fp32 reference: rel-L2 and max-abs (as a fraction of max|ref|) bounds."""
    r = rel_l2(got, ref)
    m = max_abs(got, ref) / max(ref.abs().max().item(), 1e-30)
    assert not torch.isnan(got.float()).any().item(), f"{what}: NaN in output"
    assert r < rel and m < abs_frac, f"{what}: rel_l2={r:.3e} (<{rel}) max_abs/max_ref={m:.3e} (<{abs_frac})"
    return r, m


# Tolerances that more than one test module asserts (the parity tests and tests/test_gpu_guards.py): one definition, so they cannot drift.
TOL_FP16_CHAIN = dict(rel=3e-3, abs_frac=4e-3)      # fp16 output behind more than one rounding point: attention (P rounded to fp16 before P V), folded norm -> linear
TOL_GEGLU = dict(rel=3e-3, abs_frac=3e-3)           # GEGLU epilogue: projection, gate and product each rounded to fp16
TOL_ATTN512 = dict(rel=2e-3, abs_frac=3e-3)         # the VAE's single 512-wide head
TOL_UPFOLD_OWN = dict(rel=4e-4, abs_frac=1.2e-3)    # folded up-sampler against its own arithmetic in fp32 (fp32 accumulation distance)
TOL_TYPICALITY_SCALAR = 1e-6                        # T(x|c) of the batched reduction, relative to max(1, |T|)
TOL_PATCH_EMBED = 2e-6                              # DIFT patch descriptor (unit vector) against float64


def assert_splitk_matches_unsplit(y, ref):
    """split-K against the fused single-pass kernel: identical except where the fp32 summation order flips an fp16 rounding (1 ulp, rare)"""
    diff = (y.float() - ref.float()).abs()
    assert (diff > 0).float().mean().item() < 0.02 and diff.max().item() <= 2e-3 * ref.float().abs().max().item()


def assert_block_sums(blocks, ref, scale):
    """GroupNorm block sums (fp32) against the fp64 sums `ref` of the fp16 tensor; `scale` = the same sums of |x|"""
    assert ((blocks.double() - ref).abs() <= 4e-6 * scale + 1e-6).all()


def assert_conv_out_pred(pred, ref, what=""):
    """conv_out's fp16 prediction against F.conv2d in fp64 `ref`: the fp16 rounding of an fp32 sum of 2880 exact products"""
    err = (pred.double().cpu() - ref).abs()
    ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -14, dtype=torch.float64)) * 2.0 ** -10
    assert (err <= 0.5 * ulp + 1e-5).all(), (what, (err / ulp).max().item())


def fold_upconv_torch(w):
    """Upsample2D (nearest 2x) + conv3x3 folded onto the source grid, built with torch: w [Cout,Cin,3,3] ->
    [4 = py*2+px][Cout][(a*2+b)*Cin + ci] fp16; the 3x3 taps that read the same source pixel are summed in fp32, rounded once."""
    sel = {0: ([0], [1, 2]), 1: ([0, 1], [2])}          # parity -> 3x3 taps feeding 2x2 tap a = 0 / 1
    wf = w.float()
    out = []
    for py in (0, 1):
        for px in (0, 1):
            taps = []
            for a in (0, 1):
                for b in (0, 1):
                    taps.append(wf[:, :, sel[py][a], :][:, :, :, sel[px][b]].sum(dim=(2, 3)))     # [Cout, Cin]
            out.append(torch.cat(taps, dim=1))
    return torch.stack(out, 0).half().contiguous()


def op_upconv_folded(X, W4, bias):
    """X [N,H,W,Cin] fp16 cuda, W4 [4][Cout][4*Cin] fp16 cuda -> Y [N,2H,2W,Cout]"""
    lib = E.load_library()
    N, H, Wd, Cin = X.shape
    Cout = W4.shape[1]
    Y = torch.empty(N, 2 * H, 2 * Wd, Cout, dtype=torch.float16, device=X.device)
    rc = lib.dm_op_upconv_folded(stream(), ptr(X), ptr(W4), ptr(bias), ptr(Y), N, H, Wd, Cin, Cout)
    assert rc == 0, "dm_op_upconv_folded failed"
    torch.cuda.synchronize()
    return Y


def op_attention512(q, k, v):
    """the VAE mid block's single-head attention (head_dim 512): q / k / v [B,T,512] fp16 -> O [B,T,512] fp16 cuda.
    Q / K / V go in as one [B,T,1536] row per token, as the engine's fused projection lays them out."""
    lib = E.load_library()
    B, T, Cc = q.shape
    qkv = torch.cat([q, k, v], dim=2).contiguous().to(dev())
    o = torch.empty(B, T, Cc, dtype=torch.float16, device=dev())
    rc = lib.dm_op_attention512(stream(), ptr(qkv), C.c_void_p(qkv.data_ptr() + Cc * 2),
                                C.c_void_p(qkv.data_ptr() + 2 * Cc * 2), ptr(o), B, T, 3 * Cc, Cc, float(Cc) ** -0.5)
    assert rc == 0
    torch.cuda.synchronize()
    return o


class GuardViolation(AssertionError):
    """Raised by Guarded.check(): `name` of the tensor, `side` ("front" / "back" guard, or "payload" for a written input), `first` / `last`
    changed byte offset relative to the payload edge (front and payload: relative to the payload's first byte, so a front offset is
    negative; back: relative to the first byte after the payload) and the `count` of changed bytes."""

    def __init__(self, name, side, first, last, count):
        self.name, self.side, self.first, self.last, self.count = name, side, first, last, count
        super().__init__(f"{name}: {count} byte(s) changed in its {side}{'' if side == 'payload' else ' guard'}, "
                         f"offsets {first} ... {last} relative to the payload's {'end' if side == 'back' else 'start'}")


def _round256(n):
    return (int(n) + 255) // 256 * 256


class Guarded:
    """All device operands of one operator call inside ONE uint8 allocation, [guard | payload | guard | guard | payload | guard ...]: an
    access outside a tensor that is shorter than the guard stays inside memory the test owns, and shows — a store as a changed guard byte
    (check()), a load that reaches the result as a result that depends on the fill byte.

    inputs   {name: host tensor}: copied in; check() also verifies they come back unchanged (an operator must not write its inputs)
    outputs  {name: (shape, dtype)}: outputs and workspaces, pre-filled with the fill byte (0xFF: NaN in fp16 / fp32, -1 in int32)
    fill     the byte every guard and every output payload holds before the call
    Every payload starts at an odd multiple of 256 bytes (256 = the engine arena's granularity, the only alignment its kernels get).  The
    guard on either side of a tensor is `tile_rows` (256) rows of its row pitch (last dimension; vectors and scalars have no rows), at
    least `min_guard` (64 KiB), rounded up to 256; a payload's own padding to 256 belongs to its back guard."""

    def __init__(self, inputs, outputs=None, fill=0xFF, device="cpu", tile_rows=256, min_guard=64 * 1024):
        self.fill = int(fill)
        specs = [(n, tuple(t.shape), t.dtype, t.contiguous()) for n, t in inputs.items()]
        specs += [(n, tuple(int(v) for v in s), dt, None) for n, (s, dt) in (outputs or {}).items()]
        assert len({s[0] for s in specs}) == len(specs), "operand names must be unique"
        self.layout = {}            # name -> (front guard start, payload start, payload end, back guard end, shape, dtype, is_input)
        off = 0                     # offsets from an even multiple of 256 (`origin` below)
        for name, shape, dt, host in specs:
            es = torch.empty(0, dtype=dt).element_size()
            nbytes = es * int(np.prod(shape, dtype=np.int64))
            guard = _round256(max(tile_rows * shape[-1] * es if len(shape) >= 2 else 0, min_guard))
            start = off + guard
            if (start // 256) % 2 == 0:
                start += 256
            back = _round256(start + nbytes) + guard
            self.layout[name] = (off, start, start + nbytes, back, shape, dt, host is not None)
            off = back
        raw = torch.full((off + 512,), self.fill, dtype=torch.uint8, device=device)
        origin = -raw.data_ptr() % 512
        self.buf = raw[origin:origin + off]
        for name, _, _, host in specs:
            _, start, end, _, _, _, _ = self.layout[name]
            assert (self.buf.data_ptr() + start) % 512 == 256
            if host is not None and end > start:
                self.buf[start:end] = host.reshape(-1).view(torch.uint8).to(device)
        self.guard_bytes = {n: (L[1] - L[0], L[3] - L[2]) for n, L in self.layout.items()}
        self._inputs = {n: self.view(n).clone() for n, _, _, h in specs if h is not None}      # (output payloads are not kept)

    def view(self, name):
        _, start, end, _, shape, dt, _ = self.layout[name]
        return self.buf[start:end].view(dt).view(shape)

    def views(self):
        return {n: self.view(n) for n in self.layout}

    def offset(self, name):
        """byte address of the payload: an odd multiple of 256"""
        return self.buf.data_ptr() + self.layout[name][1]

    def _regions(self):
        for name, (front, start, end, back, _, _, is_input) in self.layout.items():
            yield name, "front", front, start, start
            if is_input:
                yield name, "payload", start, end, start
            yield name, "back", end, back, end

    def _changed(self, name, side, a, b):
        if side == "payload":
            return self.buf[a:b] != self._inputs[name].reshape(-1).view(torch.uint8)
        return self.buf[a:b] != self.fill

    def check(self):
        """every guard still holds the fill and every input its bytes, else GuardViolation for the first damaged region in layout order"""
        flags = torch.stack([self._changed(n, side, a, b).any() for n, side, a, b, _ in self._regions() if b > a])
        if not bool(flags.any()):
            return
        for name, side, a, b, origin in self._regions():
            idx = self._changed(name, side, a, b).nonzero().flatten() if b > a else torch.empty(0)
            if idx.numel():
                raise GuardViolation(name, side, int(idx[0]) + a - origin, int(idx[-1]) + a - origin, int(idx.numel()))


def line_rel_l2(got, ref):
    """per latent row and per latent column: rel-L2 over the channels (and images) of `got` vs `ref` [B,C,h,w] ->
    (rows [h], cols [w]) float64.  A global rel-L2 hides one wrong row or column of a wide grid; these do not."""
    a, b = got.double().cpu(), ref.double().cpu()
    d2, r2 = (a - b) ** 2, b ** 2
    rows = (d2.sum(dim=(0, 1, 3)) / r2.sum(dim=(0, 1, 3)).clamp_min(1e-60)).sqrt()
    cols = (d2.sum(dim=(0, 1, 2)) / r2.sum(dim=(0, 1, 2)).clamp_min(1e-60)).sqrt()
    return rows, cols
