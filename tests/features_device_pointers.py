"""Child process of tests/test_gpu_features.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first (of two
HIP runtimes in one process only the first to start sees it), then lifcal_features_detect takes the image and the status map from
torch tensors on the device (dense and with a row pitch), and the chain raw image -> raw depth -> depth map -> total focus ->
features runs without the pictures leaving the device.  Compared byte for byte with the host-pointer path."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("x", "y", "ix", "iy", "score", "desc")


def to_device(a: np.ndarray, extra: int = 0):
    """a 2-D array as a tensor on the device, 16-bit as int16 bits; extra: columns of row pitch beyond the image"""
    src = a.view(np.int16) if a.dtype == np.uint16 else a
    wide = torch.full((a.shape[0], a.shape[1] + extra), 77, dtype=torch.from_numpy(src[:1, :1].copy()).dtype, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    return wide[:, :a.shape[1]]


def same(a, b, what):
    assert a.n == b.n, (what, a.n, b.n)
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import MicroLensGrid, features
    from tests import features_reference as fref
    from tests import rawdepth_reference as ref
    for name in fref.CHAIN_CASES:
        g = MicroLensGrid(*ref.grid_arguments(name))
        raw = np.array(fref.chain_raw(name, 1))
        # from the raw image to the features on the device: estimateRawDepth -> depth_map -> total_focus -> detectFeatures
        est = g.estimateRawDepth(to_device(raw), device_out=True, patch_radius=ref.CASES[name][6], max_baseline=2.1)
        tf = est.depth_map(device_out=True, scale=1).total_focus(g, to_device(raw, 3))
        assert tf.image.is_cuda and tf.status.is_cuda
        got = features.detectFeatures(tf.image, tf.status)
        img = tf.image.cpu().numpy(); st = tf.status.cpu().numpy()
        img = img.view(np.uint16) if img.dtype == np.int16 else img
        host = features.detectFeatures(img, st)
        same(got, host, (name, "chain"))
        same(host, fref.detect(img, st), (name, "restatement"))
        assert host.n >= 10, (name, host.n)
        # a device image with a row pitch, without a status map; mixing pointer kinds is refused
        same(features.detectFeatures(to_device(img, 5)), features.detectFeatures(img), (name, "pitch"))
        for bad in ((tf.image, st), (img, tf.status)):
            try:
                features.detectFeatures(*bad)
            except ValueError:
                pass
            else:
                raise AssertionError("image and status of different pointer kinds were accepted")
    print("device pointers ok")


if __name__ == "__main__":
    main()
