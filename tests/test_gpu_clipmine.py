"""The CLIP baseline's mining on the GPU (dm_clipmine_rank, csrc/clipmine.hip) against the reference's own `dot_text_image`
(tests/golden/clipmine_ref.npz, tests/make_golden_clipmine.py): the boxes exactly, D and the features within 4 x the distance the
reference itself keeps from the float64 restatement.  Then what a batch must not change: image b's bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import clipmine as CM  # noqa: E402
from tests import clipmine_cases as CC  # noqa: E402
from tests.gpu_util import dev  # noqa: E402

# The batch tests put every case's grid and image size into ONE call, which has one E, one window, one k and one mode: the first
# MIX_E channels of each case's tokens and of the first case's text, 8 x 8 windows, k = 3, diff.
MIX_E, MIX_KW = 32, dict(k_per_image=3, kx=8, ky=8, mode="diff")


def _run(c, **kw):
    out = CM.rank_device([torch.from_numpy(c.tokens).to(dev())], torch.from_numpy(c.text).to(dev()), [c.size], **dict(CC.kwargs(c), **kw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tag", CC.CASES)
def test_reference_pin(tag):
    """Boxes, order and count exactly the reference's (the run-out and the all-eligible case included); D and features within
    4 x the recorded restatement errors; unused slots -1 / NaN."""
    c = CC.case(tag)
    boxes, D, count, feats = (t.cpu().numpy() for t in _run(c))
    E = c.tokens.shape[1]
    assert boxes.shape == (1, c.k, 4) and boxes.dtype == np.int32 and D.shape == (1, c.k) and D.dtype == np.float32
    assert feats.shape == (1, c.k, E) and feats.dtype == np.float32 and count.shape == (1,) and count.dtype == np.int32
    n = int(count[0])
    assert n == len(c.boxes), (n, boxes[0].tolist(), c.boxes.tolist())
    CC.check_against_reference(c, boxes[0, :n], D[0, :n], feats[0, :n], "gpu")
    assert (boxes[0, n:] == -1).all() and np.isnan(D[0, n:]).all() and np.isnan(feats[0, n:]).all()
    assert np.abs(np.linalg.norm(feats[0, :n].astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("tag", CC.CASES)
def test_returned_map_against_the_restatement(tag):
    """return_maps: the whole map D [OH][OW] against rank_patches_host's float64 map, within the bound of D; the D column is the
    map at the winners, bit for bit."""
    c = CC.case(tag)
    boxes, D, count, _, maps = _run(c, return_maps=True)
    _, _, host = CM.rank_patches_host([c.tokens], c.text, [c.size], return_maps=True, **CC.kwargs(c))
    got = maps[0].cpu().numpy()
    assert got.shape == host[0].shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - host[0]).max() / np.abs(host[0]).max())
    print(f"map {tag}: {got.shape} err {err:.3g} of max|D| (bound {CC.TOL_FACTOR * c.D_err:.3g})")
    assert err <= CC.TOL_FACTOR * c.D_err
    n = int(count[0])
    b = boxes[0, :n].cpu().numpy()
    assert D[0, :n].cpu().numpy().tobytes() == got[b[:, 0], b[:, 1]].tobytes()


@pytest.fixture(scope="module")
def mix():
    """(tokens, text, sizes, pws, alone): every case's geometry at MIX_E channels, and image b's results from a call of its own."""
    cs = [CC.case(t) for t in CC.CASES]
    tokens = [torch.from_numpy(np.ascontiguousarray(c.tokens[:, :MIX_E])).to(dev()) for c in cs]
    text = torch.from_numpy(np.ascontiguousarray(cs[0].text[:, :MIX_E])).to(dev())
    sizes, pws = [c.size for c in cs], [c.pw for c in cs]
    alone = [_bytes(CM.rank_device([t], text, [s], [q], return_maps=True, **MIX_KW)) for t, s, q in zip(tokens, sizes, pws)]
    assert len({a[2] for a in alone}) > 1                       # the counts differ: some images run out, some do not
    return tokens, text, sizes, pws, alone


def _bytes(out, b=0):
    """image b of a rank_device result as bytes: boxes, D, count, features, map"""
    torch.cuda.synchronize()
    return tuple(out[i][b].cpu().numpy().tobytes() for i in range(5))


def test_image_is_bit_equal_alone_in_a_batch_and_at_a_permuted_position(mix):
    tokens, text, sizes, pws, alone = mix
    n = len(tokens)
    for order in (list(range(n)), [3, 6, 0, 5, 2, 1, 4]):
        out = CM.rank_device([tokens[i] for i in order], text, [sizes[i] for i in order], [pws[i] for i in order], return_maps=True, **MIX_KW)
        for at, i in enumerate(order):
            assert _bytes(out, at) == alone[i], (order, at, i)
    again = CM.rank_device(tokens, text, sizes, pws, return_maps=True, **MIX_KW)             # a repeated call
    assert all(_bytes(again, b) == alone[b] for b in range(n))


def test_images_per_call_split_changes_no_bit(mix):
    tokens, text, sizes, pws, alone = mix
    whole = CM.rank_patches(tokens, text, sizes, pws, images_per_call=64, return_maps=True, **MIX_KW)
    split = CM.rank_patches(tokens, text, sizes, pws, images_per_call=3, return_maps=True, **MIX_KW)
    for (rows, feats, maps) in (whole, split):
        assert set(rows) == set(CM.COLUMNS) and feats.shape == (len(rows["D"]), MIX_E) and feats.is_cuda
    assert all(whole[0][k].tobytes() == split[0][k].tobytes() for k in CM.COLUMNS)
    assert whole[1].cpu().numpy().tobytes() == split[1].cpu().numpy().tobytes()
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(whole[2], split[2]))
    # the rows are the images' own results, image order then round order
    at = 0
    for b, a in enumerate(alone):
        cnt = int(np.frombuffer(a[2], dtype=np.int32)[0])
        assert (whole[0]["image"][at:at + cnt] == b).all()
        assert whole[0]["D"][at:at + cnt].tobytes() == a[1][:4 * cnt]
        assert np.stack([whole[0][k][at:at + cnt] for k in CM.COLUMNS[1:5]], 1).tobytes() == a[0][:16 * cnt]
        assert whole[1][at:at + cnt].cpu().numpy().tobytes() == a[3][:4 * MIX_E * cnt]
        at += cnt
    assert at == len(whole[0]["D"])


def test_device_entry_refuses_what_the_c_entry_refuses():
    c = CC.case("g33_small")
    t, x = torch.from_numpy(c.tokens).to(dev()), torch.from_numpy(c.text).to(dev())
    for bad in (dict(kx=25), dict(pw=2), dict(k_per_image=0), dict(k_per_image=CM.MINE_MAX_K + 1), dict(mode="x"), dict(ky=1)):
        with pytest.raises(ValueError):
            CM.rank_device([t], x, [c.size], **dict(CC.kwargs(c), **bad))
    with pytest.raises(CM.EngineError):
        CM.rank_device([c.tokens], x, [c.size], **CC.kwargs(c))
