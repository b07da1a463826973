"""Child process of tests/test_gpu_markers.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first (of two
HIP runtimes in one process only the first to start sees it), then lifcal_markers_detect and lifcal_markers_components take the
image and the status map from torch tensors on the device (dense and with a row pitch, 8 and 16 bit).  Compared byte for byte
with the host-pointer path and the restatement."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("id", "rotation", "hamming", "refined", "label", "area", "corners", "x", "y")


def to_device(a: np.ndarray, extra: int = 0):
    """a 2-D array as a tensor on the device, 16-bit as int16 bits; extra: columns of row pitch beyond the image"""
    src = a.view(np.int16) if a.dtype == np.uint16 else a
    wide = torch.full((a.shape[0], a.shape[1] + extra), 77, dtype=torch.from_numpy(src[:1, :1].copy()).dtype, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    return wide[:, :a.shape[1]]


def same(a, b, what):
    assert a.n == b.n and a.n_candidates == b.n_candidates, (what, a.n, b.n)
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import markers
    from tests import markers_reference as mr
    from tests.test_gpu_markers import scene_203
    words, _ = mr.dictionary()
    d = markers.Dictionary(4, words)
    for bits in (8, 16):
        img, status, _ = scene_203(bits)
        img = np.ascontiguousarray(img)
        host = markers.detectMarkers(img, d, status)
        want, _ = mr.detect(img, words, 4, status)
        assert host.n == len(want) == 3 and host.x.tobytes() == want["x"].tobytes() and host.corners.tobytes() == want["corners"].tobytes()
        st = torch.from_numpy(status).cuda()
        same(markers.detectMarkers(to_device(img), d, st), host, (bits, "dense"))
        same(markers.detectMarkers(to_device(img, 5), d, st), host, (bits, "pitch"))
        same(markers.detectMarkers(to_device(img, 5), d), markers.detectMarkers(img, d), (bits, "no status"))
        a, b = markers.markerComponents(to_device(img, 3), st), markers.markerComponents(img, status)
        assert a.dark.tobytes() == b.dark.tobytes() and a.labels.tobytes() == b.labels.tobytes() and a.candidates.tobytes() == b.candidates.tobytes()
        for bad in ((to_device(img), status), (img, st)):
            try:
                markers.detectMarkers(bad[0], d, bad[1])
            except ValueError:
                pass
            else:
                raise AssertionError("image and status of different pointer kinds were accepted")
    print("device pointers ok")


if __name__ == "__main__":
    main()
