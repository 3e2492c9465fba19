"""The device runs of the HOG-LAB cases, shared by tests/test_gpu_hoglab.py and tests/test_gpu_hoglab_guards.py: one run per case and
process, whichever module asks first."""
import torch

from diff_mining_amd import doersch as D
from tests import hoglab_cases as HC
from tests.gpu_util import dev

_runs = {}


def on_device(tag):
    return torch.from_numpy((HC.probe_image()[None] if tag == "P" else HC.images(tag)).copy()).to(dev())


def run(tag, fresh=False):
    """{"hog", "lab": dm_hoglab_cells; "out", "raw": dm_hoglab_features with both outputs} as numpy arrays; once per case unless fresh"""
    if fresh or tag not in _runs:
        images = on_device(tag)
        hog, lab = D.hoglab_cells(images)
        got = {"hog": hog, "lab": lab}
        if tag != "P":
            got["out"], got["raw"] = D.hoglab_features(images, normalized=True, raw=True)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        if fresh:
            return got
        _runs[tag] = got
    return _runs[tag]
