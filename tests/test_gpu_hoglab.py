"""The HOG-LAB features on the GPU (csrc/hoglab.hip through diff-mining_amd/doersch.py) against the fp64 numpy restatement
`hoglab_host`.  Per case tolN = 8 x max |hoglab_host(fp32) - hoglab_host(fp64)| (tests/hoglab_cases.host: 8 x is the margin the dense
search took for the same construction), separately for the two cell maps, the raw features and the normalised ones; the fp16 output
may add half an fp16 unit.  The probe image is the test a kernel that bins with fp32 atan2 fails."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diff_mining_amd import doersch as D  # noqa: E402
from tests import hoglab_cases as HC  # noqa: E402
from tests.gpu_util import dev  # noqa: E402
from tests.hoglab_gpu_run import on_device, run  # noqa: E402

def assert_cells(tag):
    got, want = run(tag), HC.host(tag)
    for name in ("hog", "lab"):
        assert got[name].dtype == np.float32 and got[name].shape == want[name].shape
        assert not np.isnan(got[name]).any()
        err = float(np.abs(got[name].astype(np.float64) - want[name]).max())
        print(f"{tag} {name} cells: max |device - host64| = {err:.3g}, tolN = {want['tol'][name]:.3g}")
        assert err <= want["tol"][name], (tag, name, err, want["tol"][name])


@pytest.mark.parametrize("tag", HC.ORDER)
def test_cell_maps(tag):
    assert_cells(tag)


def test_probe_image_every_gradient_next_to_a_bin_edge_lands_in_its_bin():
    """The device and the host reference read the same table, Python's `hoglab_bin_table()`: this pins the kernel's use of the table
    (a kernel that bins with fp32 atan2 fails here), not the table.  A wrong table is caught on the CPU tier, where
    `dm_hoglab_bin_table` (C, atan2 / fmod) must equal the numpy statement on every entry (tests/test_hoglab.py)."""
    pairs = HC.probe_pairs()
    tol = HC.host("P")["tol"]["hog"]
    assert len(pairs) == HC.PROBES and (pairs[:, 0] != 0).all()
    # one misplaced probe moves its magnitude / 64 from one bin of its cell to another: that cannot hide under the tolerance
    assert (np.hypot(pairs[:, 0], pairs[:, 1]) / 64 >= 1000 * tol).all()
    d = HC.edge_distance()[pairs[:, 0] + 255, pairs[:, 1] + 255]
    assert d.min() < 3.1e-6 and (np.diff(d) >= 0).all()                              # the closest: 3.0e-6 degrees
    assert_cells("P")


@pytest.mark.parametrize("tag", HC.ORDER)
def test_features(tag):
    got, want = run(tag), HC.host(tag)
    H, W, kinds = HC.SHAPES[tag]
    shape = (len(kinds),) + D.hoglab_shape(H, W) + (2112,)
    assert got["raw"].dtype == np.float32 and got["out"].dtype == np.float16 and got["raw"].shape == got["out"].shape == shape
    assert not np.isnan(got["raw"]).any() and not np.isnan(got["out"]).any()
    tol = want["tol"]
    err = float(np.abs(got["raw"].astype(np.float64) - want["raw"]).max())
    print(f"{tag} raw: max |device - host64| = {err:.3g}, tolN = {tol['raw']:.3g}")
    assert err <= tol["raw"], (tag, err, tol["raw"])
    x = want["out"]
    diff = np.abs(got["out"].astype(np.float64) - x)
    normal = np.abs(x) >= 2.0 ** -14
    # half an fp16 unit (2^-11 relative; 2^-25 below the normal range) plus the fp32 error
    excess = np.where(normal, diff - 2.0 ** -11 * np.abs(x), diff - 2.0 ** -25)
    print(f"{tag} out: max (|device - host64| - half an fp16 unit) = {float(excess.max()):.3g}, tolN = {tol['out']:.3g}; "
          f"max |device - host64| = {float(diff.max()):.3g}, {int((~normal).sum())} values below 2^-14")
    assert (excess <= tol["out"]).all(), (tag, float(excess.max()), tol["out"])


@pytest.mark.parametrize("tag", ("B", "D"))
def test_two_runs_are_bit_equal(tag):
    a, b = run(tag), run(tag, fresh=True)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_an_image_does_not_depend_on_its_batch():
    """image 2 of case B alone against image 2 inside the batch of three: the same bits in every output"""
    batch = run("B")
    images = on_device("B")[2:3].contiguous()
    hog, lab = D.hoglab_cells(images)
    out, raw = D.hoglab_features(images, normalized=True, raw=True)
    torch.cuda.synchronize()
    for name, t in (("hog", hog), ("lab", lab), ("out", out), ("raw", raw)):
        assert t.shape[0] == 1 and t[0].cpu().numpy().tobytes() == batch[name][2].tobytes(), name


@pytest.mark.parametrize("tag", ("C", "D"))
def test_each_output_alone_equals_both_together(tag):
    both = run(tag)
    images = on_device(tag)
    out, none = D.hoglab_features(images, normalized=True, raw=False)
    assert none is None
    none, raw = D.hoglab_features(images, normalized=False, raw=True)
    assert none is None
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == both["out"].tobytes() and raw.cpu().numpy().tobytes() == both["raw"].tobytes()
    assert D.hoglab(images).cpu().numpy().tobytes() == both["out"].tobytes()
    assert D.hoglab(images, normalized=False).cpu().numpy().tobytes() == both["raw"].tobytes()


# ---- from image files to ranked detections -------------------------------------------------------------------------------------
# (image of case B, bbox): K = 5 detectors, the patches of the 24 whose host-side winner gaps are widest (>= 1.1e-3, tol32 = 1.5e-6)
PATCHES = ((0, (16, 8)), (1, (8, 0)), (2, (8, 8)), (0, (24, 8)), (1, (24, 0)))


def assert_gaps(feats, w, masks):
    """on the host: every winner against the runner-up cell, and every image against the next in a detector's list, is at least
    16 x the search's own tol32 (8 x the deviation of a numpy fp32 matmul from fp64) apart, so the device must agree exactly"""
    B, cells = feats.shape[0], feats.shape[1] * feats.shape[2]
    x = feats.reshape(B, cells, -1)
    e64 = np.einsum("bic,kc->kbi", x.astype(np.float64), w.astype(np.float64))
    m32 = np.einsum("bic,kc->kbi", x.astype(np.float32), w.astype(np.float32))
    tol32 = 8 * float(np.abs(m32 - e64).max())
    if masks is not None:
        e64 = np.where(masks[None] == 0, 0.0, e64)
    top = np.sort(e64, axis=2)
    best, second = top[:, :, -1], top[:, :, -2]
    tied_zeros = (best == 0) & (second == 0)                                          # two masked cells: decided by the index rule
    win_gap = float((best - second)[~tied_zeros].min())
    ranked = -np.sort(-best, axis=1)
    rank_gap = float((ranked[:, :-1] - ranked[:, 1:]).min())
    print(f"tol32 = {tol32:.3g}, winner gap {win_gap:.3g}, rank gap {rank_gap:.3g}")
    assert min(win_gap, rank_gap) >= 16 * tol32, (win_gap, rank_gap, tol32)


def test_from_png_files_to_ranked_detections(tmp_path):
    from PIL import Image
    imgs = HC.images("B")
    paths = []
    for j, im in enumerate(imgs):
        paths.append(str(tmp_path / f"img{j}.png"))
        Image.fromarray(im).save(paths[-1])
    host_feats = D.hoglab(imgs)                                                      # numpy fp16 [3, 4, 2, 2112]
    w_host = np.stack([D.detector_from_patch(host_feats[b], bbox) for b, bbox in PATCHES])
    dev_feats = D.hoglab(on_device("B"))
    w_dev = torch.stack([D.detector_from_patch(dev_feats[b], bbox) for b, bbox in PATCHES])
    for k, (b, bbox) in enumerate(PATCHES):                                          # a bit copy of the row
        assert torch.equal(w_dev[k], dev_feats[b, bbox[0] // 8, bbox[1] // 8])
    assert_gaps(host_feats, w_host, None)
    got = D.dense_search_images(w_dev, paths, top_k=3, batch=2, scores="f32")
    want = D.dense_search_host(w_host, [(paths, host_feats)], top_k=3, scores="f32")
    assert len(got) == 5 and all(len(entries) == 3 for entries in got)
    for k, (b, bbox) in enumerate(PATCHES):
        assert [e[1:] for e in got[k]] == [e[1:] for e in want[k]], k              # the same cells, the same image order
        assert got[k][0][1:] == (bbox, paths[b]) and abs(float(got[k][0][0]) - 1.0) <= 2e-3       # a patch finds itself
    # the default scores (the reference's fp16 arithmetic) and ret_ws: bit copies of the device's rows
    shown = D.dense_search_images(w_dev, paths, top_k=3, batch=2, ret_ws=True)
    flat = dev_feats.cpu().numpy()
    for k in range(5):
        assert [e[1:3] for e in shown[k]] == [e[1:] for e in want[k]]
        for score, bbox, path, row in shown[k]:
            assert type(score) is np.float16 and row.tobytes() == flat[paths.index(path), bbox[0] // 8, bbox[1] // 8].tobytes()
    # fold (1, 3): the masks are drawn on the device, per batch of two paths; the same draws, taken to the host, give the same lists
    got = D.dense_search_images(w_dev, paths, top_k=3, fold=(1, 3), batch=2, scores="f32")
    masks = [D.fold_mask(j, len(p), 8, (1, 3), dev()).cpu().numpy() for j, p in enumerate((paths[:2], paths[2:]))]
    assert all(int(m.sum()) == 2 * len(m) for m in masks)
    assert_gaps(host_feats, w_host, np.concatenate(masks))
    want = D.dense_search_host(w_host, [(paths[:2], host_feats[:2], masks[0]), (paths[2:], host_feats[2:], masks[1])], top_k=3,
                               scores="f32")
    for k in range(5):
        assert [e[1:] for e in got[k]] == [e[1:] for e in want[k]], k
