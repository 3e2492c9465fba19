"""The VAE encoder at the image sizes it really encodes, against the CPU oracle (`oracle/vae_ref.py`) computed live.

test_gpu_vae.py / test_gpu_f32.py compare the encoder with the oracle at 64²…128² px only.  The work list's images are far
larger (compute.py:165-180: places short side 512, e.g. 512×683 -> latent 64×85; cars short side 256, e.g. 256×341 / 256×343 ->
32×42; the BASELINE 512²; configs[4] X-ray 1024²), and there the encoder takes paths the small sizes never reach: the mid
block's head_dim-512 attention over 1344…16384 tokens (hundreds of 32-key tiles), the 64-channel-wave igemm and the pad-0
stride-2 downsampler at widths 683 / 341 / 170 / 85 / 1024, GroupNorm over 349,696 px per sample, and the workspace chunking of
a call into groups of 8·512²/(H·W) images.

Bounds.  End to end the global bounds of test_gpu_vae.py stay as they are.  A global rel-L2 cannot see one wrong latent row or
column of an 85-wide grid (1 % on one column adds ~1e-3), so every latent row and every latent column is measured on its own
(rel-L2 over the 8 moment channels) against the fp32 oracle, and bounded by LINE_K x the same metric between the autocast
oracle and the fp32 oracle on the same image: the noise floor of fp16 autocast itself.  Op rows compare
with float64 references on what a check needs: sampled query rows, bands of output rows over the full width."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import gpu_util as U  # noqa: E402

TOL_E2E = 2e-5                    # the fp32 net against the fp32 oracle (test_gpu_f32.py)
LINE_K = 1.5                      # worst row / column of the engine <= LINE_K x the autocast oracle's worst row / column
# H x W px: BASELINE 512²; places 512×683 (landscape) / 683×512 (portrait) -> 64×85 / 85×64; cars 256×341, 341×256,
# 256×343 -> 32×42 / 42×32; configs[4] X-ray 1024² (one image, 16384 attention tokens)
SIZES = [(512, 512), (512, 683), (683, 512), (256, 341), (341, 256), (256, 343), (1024, 1024)]

_ORACLE = {}                      # (H, W, autocast) -> moments [1,8,h,w]: each oracle encode runs once per module


@pytest.fixture(scope="module")
def vae_sd():
    from diff_mining_amd import synth
    return synth.synth_vae_state_dict(seed=0, dtype=np.float16)


@pytest.fixture(scope="module")
def vae_sdt(vae_sd):
    return {k: torch.from_numpy(v).float() for k, v in vae_sd.items()}


@pytest.fixture(scope="module")
def vae16(vae_sd):
    from diff_mining_amd.engine import UNetEngine
    eng = UNetEngine(0)
    eng.load_vae_state_dict(vae_sd)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def vae32(vae_sd):
    from diff_mining_amd.engine import UNetEngineF32
    eng = UNetEngineF32(0)
    eng.load_vae_state_dict(vae_sd)             # fp16-valued weights widened exactly: the oracle sees the same values
    yield eng
    eng.close()


def _image(H, W):
    from diff_mining_amd import synth
    return torch.from_numpy(synth.synth_image(1, H, W))


def _noise(H, W, n=1):
    return U.f16_randn(n, 4, H // 8, W // 8, seed=H * 7 + W)


def _oracle(vae_sdt, H, W, autocast):
    from oracle import vae_ref
    key = (H, W, autocast)
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = vae_ref.vae_moments(vae_sdt, _image(H, W).float(), autocast=autocast)
    return _ORACLE[key]


def _check_fp16_encode(vae_sdt, H, W, lat, mom, noise, what):
    """one image's fp16-engine latents / moments vs both oracles: the global bounds of test_gpu_vae.py plus the per-row /
    per-column bound; returns the measured numbers"""
    from oracle import vae_ref
    m32, mac = _oracle(vae_sdt, H, W, False), _oracle(vae_sdt, H, W, True)
    assert mom.shape == m32.shape and lat.shape == (1, 4, H // 8, W // 8)
    r_ac, r_32, base = U.rel_l2(mom, mac), U.rel_l2(mom, m32), U.rel_l2(mac, m32)
    r_lat = U.rel_l2(lat, vae_ref.posterior_sample(mac, noise))
    rows, cols = U.line_rel_l2(mom, m32)
    frows, fcols = U.line_rel_l2(mac, m32)
    wr, wc, fr, fc = rows.max().item(), cols.max().item(), frows.max().item(), fcols.max().item()
    print(f"vae {what}: moments rel-L2 vs autocast-oracle {r_ac:.2e}, vs fp32 {r_32:.2e} (oracle ac-vs-fp32 {base:.2e}); "
          f"latents {r_lat:.2e}; worst row {wr:.2e} (row {rows.argmax().item()}; oracle floor {fr:.2e}), "
          f"worst column {wc:.2e} (column {cols.argmax().item()}; oracle floor {fc:.2e}); "
          f"first / last row {rows[0]:.2e} / {rows[-1]:.2e}, first / last column {cols[0]:.2e} / {cols[-1]:.2e}")
    assert torch.isfinite(mom).all() and torch.isfinite(lat).all()
    assert r_ac < 3e-3 and r_32 < 2.7e-3, (r_ac, r_32)
    assert r_lat < 1.8e-3, r_lat
    assert wr <= LINE_K * fr, f"{what}: latent row {rows.argmax().item()} rel-L2 {wr:.3e} > {LINE_K} x oracle floor {fr:.3e}"
    assert wc <= LINE_K * fc, f"{what}: latent column {cols.argmax().item()} rel-L2 {wc:.3e} > {LINE_K} x oracle floor {fc:.3e}"
    return r_ac, r_32, wr, wc


# ---- 1. the fp16 encoder end to end ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_vae_encode_at_real_image_sizes(vae16, vae_sdt, H, W):
    img, noise = _image(H, W), _noise(H, W)
    lat, mom = vae16.vae_encode(img, noise, return_moments=True, out_dtype=torch.float32)
    _check_fp16_encode(vae_sdt, H, W, lat.cpu(), mom.cpu(), noise, f"{H}x{W}")


# ---- 2. the fp32 net's encoder (the featuriser's pixel path) -----------------------------------------------------------------
@pytest.mark.parametrize("H,W,draws", [(512, 683, 1), (683, 512, 1), (256, 341, 1), (256, 343, 3)])
def test_vae32_at_real_image_sizes(vae32, vae_sdt, H, W, draws):
    from oracle import vae_ref
    img = _image(H, W).float()
    g = torch.Generator().manual_seed(H + W + draws)
    noise = torch.randn(draws, 4, H // 8, W // 8, generator=g)
    lat, mom = vae32.vae_encode(img, noise, return_moments=True, draws_per_image=draws)
    m32 = _oracle(vae_sdt, H, W, False)
    l_ref = vae_ref.posterior_sample(m32.repeat_interleave(draws, 0), noise)
    rm, rl = U.rel_l2(mom, m32), U.rel_l2(lat, l_ref)
    rows, cols = U.line_rel_l2(mom, m32)
    print(f"vae32 {H}x{W} draws {draws}: moments rel-L2 {rm:.2e}, latents {rl:.2e}; worst row {rows.max():.2e}, "
          f"worst column {cols.max():.2e}")
    assert mom.shape == m32.shape and lat.shape == l_ref.shape
    assert rm < TOL_E2E and rl < TOL_E2E, (rm, rl)
    # every latent row and column on its own at the same bound (measured <= 5.2e-6 where the global figure is 3.2e-6)
    assert rows.max() < TOL_E2E and cols.max() < TOL_E2E, (rows.max(), cols.max())


# ---- 3. op rows at the shapes the encodes reach, against float64 -------------------------------------------------------------
def _softmax_rows(q, k, v, rows):
    """exact single-head softmax attention (float64) of the query rows `rows`: q / k / v [B,T,512] -> [B,len(rows),512]"""
    s = q[:, rows].double() @ k.double().transpose(1, 2) * q.shape[2] ** -0.5
    return torch.softmax(s, dim=-1) @ v.double()


@pytest.mark.parametrize("B,T", [(2, 4096), (1, 5440), (1, 5440 - 7), (1, 1344), (1, 16384)])
def test_attention512_at_encoder_token_counts(B, T):
    """attn512_kernel over 42…512 key tiles of 32 (4096 = 512², 5440 = 512×683, 1344 = 256×341, 16384 = 1024²), and a ragged
    count whose last tile holds 25 keys and 7 zero-filled rows.  A key that dominates query 7 mid-sequence, a larger one in the
    last tile and one at the very last key for a last-block query move the running max late.  At the ragged count every real
    key leans along one direction and some first- and last-block queries point against it: all their real logits are about
    -11, so a zero-filled key that escaped the `key < T` mask (logit 0) would outweigh all of them."""
    q = U.f16_randn(B, T, 512, seed=81, scale=1.5)
    k = U.f16_randn(B, T, 512, seed=82, scale=1.5)
    v = U.f16_randn(B, T, 512, seed=83)
    k[:, T // 2] = q[:, 7] * 2.0
    k[:, T - 3] = q[:, 7] * 4.0
    k[:, T - 1] = q[:, T - 5] * 3.0
    if T % 32:
        k = (k.float() + 0.5).half()
        q[:, 0:4] = -1.0
        q[:, T - 4:T - 1] = -1.0
    o = U.op_attention512(q, k, v).cpu()
    rows = torch.cat([torch.arange(0, 64), torch.randperm(T - 128, generator=torch.Generator().manual_seed(T))[:256] + 64,
                      torch.arange(T - 64, T)])
    ref = _softmax_rows(q, k, v, rows)
    r, m = U.assert_close_fp16(o[:, rows], ref, f"attention512 B={B} T={T}", rel=2e-3, abs_frac=3e-3)
    print(f"attention512 B={B} T={T} ({len(rows)} rows): rel-L2 {r:.2e}, max|err|/max|ref| {m:.2e}")


def _bands(n, rows=8):
    """first, one interior and last band of `rows` output rows"""
    mid = n // 2 - rows // 2
    return [(0, rows), (mid, mid + rows), (n - rows, n)]


# (H, W, Cin -> Cout) of the encoder's 3x3 convolutions per level at 512×683 (683 -> 341 -> 170 -> 85 px wide) and 1024²
@pytest.mark.parametrize("H,W,Cin,Cout", [(512, 683, 128, 128), (256, 341, 128, 256), (256, 341, 256, 256), (128, 170, 256, 512),
                                          (64, 85, 512, 512), (1024, 1024, 128, 128), (512, 512, 128, 256)])
def test_igemm64_conv3x3_at_encoder_sizes(H, W, Cin, Cout):
    """the 64-channel-wave 3x3 convolution (mode 1) on whole encoder activations; float64 reference on bands of output rows
    (first, interior, last) over the full width, so the first and the last (odd) column are always checked"""
    x = U.f16_randn(1, Cin, H, W, seed=H + W + Cin)
    w = U.f16_randn(Cout, Cin, 3, 3, seed=6, scale=(9 * Cin) ** -0.5)
    b = U.f16_randn(Cout, seed=7, scale=0.1)
    d = U.dev()
    y = U.op_igemm(U.to_nhwc(x).to(d), U.pack_conv3(w).to(d), b.to(d), mode=1).cpu()
    got, ref = [], []
    for r0, r1 in _bands(H):
        lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
        xb = F.pad(x[:, :, lo:hi].double(), (1, 1, lo - (r0 - 1), (r1 + 1) - hi))
        ref.append(F.conv2d(xb, w.double(), b.double()))
        got.append(U.to_nchw(y[:, r0:r1]))
    r, m = U.assert_close_fp16(torch.cat(got, 2), torch.cat(ref, 2), f"conv3x3 {H}x{W} {Cin}->{Cout}")
    print(f"igemm64 conv3x3 {H}x{W} {Cin}->{Cout}: rel-L2 {r:.2e}, max|err|/max|ref| {m:.2e}")


@pytest.mark.parametrize("H,W,C", [(512, 683, 128), (683, 512, 128), (256, 341, 256), (128, 170, 512), (1024, 1024, 128),
                                   (512, 512, 256), (256, 256, 512)])
def test_igemm64_downsample_pad0_at_encoder_sizes(H, W, C):
    """`Downsample2D(padding=0)` (F.pad(x, (0,1,0,1)) + 3x3 stride 2, mode 4) at the encoder's real sizes, odd widths and
    heights included (683 -> 341, 341 -> 170); float64 reference on bands of output rows over the full width"""
    x = U.f16_randn(1, C, H, W, seed=H * 3 + W + C)
    w = U.f16_randn(C, C, 3, 3, seed=12, scale=(9 * C) ** -0.5)
    b = U.f16_randn(C, seed=13, scale=0.1)
    OH, OW = H // 2, W // 2
    d = U.dev()
    y = U.op_igemm(U.to_nhwc(x).to(d), U.pack_conv3(w).to(d), b.to(d), mode=4, OH=OH, OW=OW).cpu()
    assert y.shape == (1, OH, OW, C)
    got, ref = [], []
    for r0, r1 in _bands(OH):
        need = 2 * (r1 - r0) + 1                                   # input rows 2 r0 ... 2 r1, row H is the pad row
        xb = x[:, :, 2 * r0:2 * r1 + 1].double()
        xb = F.pad(xb, (0, 1, 0, need - xb.shape[2]))
        ref.append(F.conv2d(xb, w.double(), b.double(), stride=2))
        got.append(U.to_nchw(y[:, r0:r1]))
    ref = torch.cat(ref, 2)
    assert ref.shape[3] == OW
    r, m = U.assert_close_fp16(torch.cat(got, 2), ref, f"downsample {H}x{W} C={C}")
    print(f"igemm64 downsample pad0 {H}x{W} -> {OH}x{OW} C={C}: rel-L2 {r:.2e}, max|err|/max|ref| {m:.2e}")


@pytest.mark.parametrize("N,HW,C,silu", [(1, 512 * 683, 128, True), (2, 256 * 341, 256, True), (1, 64 * 85, 512, False),
                                         (2, 32 * 42, 512, True), (1, 512 * 683 - 203, 128, True)])
def test_groupnorm_at_encoder_sizes(N, HW, C, silu):
    """GroupNorm(32, eps 1e-6) at the encoder's pixel counts per sample (512×683 at 128 channels: 4 channels per group, 16
    column threads; 256×341 at 256; the mid block's 64×85 / 32×42 at 512, whose last 256-px statistics chunk is partial) and
    a ragged count; per-channel |mean| / std of a few and a ramp along the pixels (the sums cannot be right by symmetry);
    against float64 statistics"""
    G, eps = 32, 1e-6
    g = torch.Generator().manual_seed(HW + C)
    mu = 3.0 * torch.randn(N, 1, C, generator=g)
    sd = 0.5 + torch.rand(N, 1, C, generator=g)
    ramp = torch.linspace(-1.0, 1.0, HW)[None, :, None]
    x = (mu + sd * (torch.randn(N, HW, C, generator=g) + 1.5 * ramp)).half()          # NHWC, one row per pixel
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    d = U.dev()
    y = U.op_groupnorm(x.view(N, 1, HW, C).to(d), gamma.to(d), beta.to(d), G, eps, silu).cpu().view(N, HW, C)
    xd = x.double().view(N, HW, G, C // G)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    ref = ((xd - mean) / (var + eps).sqrt()).view(N, HW, C) * gamma.double() + beta.double()
    if silu:
        ref = F.silu(ref)
    r, m = U.assert_close_fp16(y, ref, f"groupnorm N={N} HW={HW} C={C}")
    print(f"groupnorm N={N} HW={HW} C={C}: rel-L2 {r:.2e}, max|err|/max|ref| {m:.2e}")


# ---- 4. workspace chunking: a call is split into groups of 8·512²/(H·W) images -------------------------------------------------
def _batch(H, W, n):
    """n images whose LAST one is the image (and draw) the end-to-end tests above use"""
    from diff_mining_amd import synth
    img = torch.cat([torch.from_numpy(synth.synth_image(n - 1, H, W, seed=11)), _image(H, W)])
    noise = torch.cat([U.f16_randn(n - 1, 4, H // 8, W // 8, seed=91), _noise(H, W)])
    return img, noise


@pytest.mark.parametrize("H,W,n", [(512, 683, 7), (1024, 1024, 3)])
def test_vae_chunked_call_is_per_image(vae16, vae_sdt, H, W, n):
    """7 images at 512×683 run as chunks of 5 + 2, 3 images at 1024² as 2 + 1: bit-equal to one call per image; the last
    image (in the last chunk) meets the end-to-end bounds"""
    img, noise = _batch(H, W, n)
    lat, mom = vae16.vae_encode(img, noise, return_moments=True, out_dtype=torch.float32)
    lat, mom = lat.cpu(), mom.cpu()
    for i in range(n):
        l1, m1 = vae16.vae_encode(img[i:i + 1], noise[i:i + 1], return_moments=True, out_dtype=torch.float32)
        assert torch.equal(lat[i:i + 1], l1.cpu()) and torch.equal(mom[i:i + 1], m1.cpu()), f"image {i} of {n} at {H}x{W}"
    _check_fp16_encode(vae_sdt, H, W, lat[-1:], mom[-1:], noise[-1:], f"{H}x{W} image {n - 1} of a {n}-image call")


@pytest.mark.parametrize("H,W,n", [(512, 683, 7), (1024, 1024, 3)])
def test_vae32_chunked_call_is_per_image(vae32, vae_sdt, H, W, n):
    img, noise = _batch(H, W, n)
    img, noise = img.float(), noise.float()
    lat, mom = vae32.vae_encode(img, noise, return_moments=True)
    lat, mom = lat.cpu(), mom.cpu()
    for i in range(n):
        l1, m1 = vae32.vae_encode(img[i:i + 1], noise[i:i + 1], return_moments=True)
        assert torch.equal(lat[i:i + 1], l1.cpu()) and torch.equal(mom[i:i + 1], m1.cpu()), f"image {i} of {n} at {H}x{W}"
    rm = U.rel_l2(mom[-1:], _oracle(vae_sdt, H, W, False))
    print(f"vae32 {H}x{W} image {n - 1} of a {n}-image call: moments rel-L2 {rm:.2e}")
    assert rm < TOL_E2E, rm
