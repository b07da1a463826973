"""Child process of tests/test_gpu_rawdepth.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first (of two
HIP runtimes in one process only the first to start sees it), then lifcal_rawdepth_estimate takes the raw image from a torch
tensor on the device and writes its maps into torch tensors.  Compared byte for byte with the host-pointer path."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import MicroLensGrid
    from tests import rawdepth_reference as ref
    for name in ref.CASES:
        g = MicroLensGrid(*ref.grid_arguments(name))
        img = np.array(ref.make_case(name, "mid", ref.NOISE))
        opts = dict(patch_radius=ref.CASES[name][6], max_baseline=2.1)
        host = g.estimateRawDepth(img, **opts)
        t = torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()   # int16 carries a 16-bit image
        wide = torch.zeros((img.shape[0], img.shape[1] + 5), dtype=t.dtype, device="cuda")  # a device image with a row pitch
        wide[:, :img.shape[1]] = t
        for dev_img in (t, wide[:, :img.shape[1]]):
            got = g.estimateRawDepth(dev_img, device_out=True, **opts)
            for f in ("inv_depth", "cost", "status", "n_neighbours"):
                a, b = getattr(got, f), getattr(host, f)
                assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes(), (name, f)
            assert np.array_equal(got.counts, host.counts) and host.counts[0] > 0
            pts_dev, pts_host = got.points(), host.points()
            assert np.array_equal(pts_dev.src, pts_host.src) and pts_dev.x.tobytes() == pts_host.x.tobytes() and len(pts_host.src) == host.counts[0]
        try:
            g.estimateRawDepth(t.float())
        except ValueError:
            pass
        else:
            raise AssertionError("a float tensor was accepted as a raw image")
    print("device pointers ok")


if __name__ == "__main__":
    main()
