"""Child process of tests/test_gpu_depthmap.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first (of two
HIP runtimes in one process only the first to start sees it), then lifcal_depthmap_from_raw takes inv_depth from a torch tensor on
the device (as estimateRawDepth(device_out=True) leaves it) and writes its maps into torch tensors, and to_depth_maps hands
depth16 to a lifcal_depth handle device to device.  Compared byte for byte with the host-pointer path."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import MicroLensGrid, depth, depth_map
    from tests import rawdepth_reference as ref
    for name in ref.CASES:
        g = MicroLensGrid(*ref.grid_arguments(name))
        img = np.array(ref.make_case(name, "near", ref.NOISE))
        est = g.estimateRawDepth(img, device_out=True, patch_radius=ref.CASES[name][6], max_baseline=2.1)
        assert est.inv_depth.is_cuda
        for scale in (1, 2):
            host = depth_map.depthMapFromRaw(g, est.inv_depth.cpu().numpy(), scale=scale)
            got = est.depth_map(device_out=True, scale=scale)
            mixed = depth_map.depthMapFromRaw(g, est.inv_depth, scale=scale)          # device in, host out
            for f in ("inv_depth", "depth16", "status", "support"):
                a, b = getattr(got, f), getattr(host, f)
                assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes(), (name, scale, f)
                assert getattr(mixed, f).tobytes() == b.tobytes(), (name, scale, f)
            assert np.array_equal(got.counts, host.counts) and got.n_samples == host.n_samples and host.counts[0] > 0 and host.counts[1] > 0
            oh, ow = host.status.shape
            Y, X = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
            with depth.DepthMaps(ow, oh, 2) as dm:
                got.to_depth_maps(dm, 0)        # device to device
                host.to_depth_maps(dm, 1)
                v0, c0 = dm.sample(X.ravel(), Y.ravel(), 0)
                v1, c1 = dm.sample(X.ravel(), Y.ravel(), 1)
            assert v0.tobytes() == v1.tobytes() and c0.direct == c1.direct == int((host.depth16 > 0).sum())
        try:
            depth_map.depthMapFromRaw(g, est.inv_depth.double())
        except ValueError:
            pass
        else:
            raise AssertionError("a double tensor was accepted as inv_depth")
    print("device pointers ok")


if __name__ == "__main__":
    main()
