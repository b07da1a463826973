"""Child process of tests/test_gpu_depth.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first, then the
library takes the maps from a torch tensor on the device and writes its outputs into torch tensors.  Compared with the host path."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import depth
    from tests import depth_reference as dr
    rs = np.random.default_rng(9)
    raw = dr.encode_vdepth(rs.uniform(2.3, 12.0, (3, 37, 250)))
    raw[rs.random(raw.shape) < 0.2] = 0
    cam = np.array([35.0, 34.15, 0.40, 511.3, 513.9, 5e-5, -2e-7, 1e-5, -1e-5] + [0.0] * 8)
    views = np.column_stack([rs.uniform(-0.4, 0.4, (2, 3)), rs.uniform(-300, 300, (2, 3))])
    frames = np.array([1, 0, 1])
    G = np.zeros((17, 17)); G[0, 0], G[1, 1], G[2, 2] = 1e-4, 4e-4, 1e-6
    with depth.DepthMaps(250, 37, 3) as host, depth.DepthMaps(250, 37, 3) as dev:
        host.setMaps(raw)
        t = torch.from_numpy(raw.view(np.int16)).cuda()          # the maps never touch the host on their way in
        dev.setMaps(t)
        for dbl in (True, False):
            for ev in (0, 1):
                kw = dict(eval=ev, out_double=dbl, frames=frames, views=views, want_z=True, want_sigma_z=True, cam_cov=G, sigma_v=0.01)
                h = host.backProjectMaps(cam, 0x6, 0.011, **kw)
                d = dev.backProjectMaps(cam, 0x6, 0.011, device_out=True, **kw)
                assert d.xyz.is_cuda and d.xyz.dtype == (torch.float64 if dbl else torch.float32) and d.n_invalid == h.n_invalid > 0
                for a, b in ((d.xyz, h.xyz), (d.z, h.z), (d.sigma_z, h.sigma_z)):
                    assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)
        try:
            dev.setMaps(t.float())
        except depth.LifcalError:
            pass
        else:
            raise AssertionError("a float tensor was accepted as depth maps")
    print("device pointers ok")


if __name__ == "__main__":
    main()
