"""Child process of tests/test_gpu_depth_views.py::test_device_pointer_outputs_equal_host_outputs: torch initialises the GPU first,
then checkMaps and fuseMaps write into torch tensors on the device.  Compared with the host-pointer path of the same calls."""
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
    from tests import depth_views_reference as vr
    raw, cam, views = vr.views_fixture()
    frames = np.arange(vr.N_FIX)
    with depth.DepthMaps(vr.W_FIX, vr.H_FIX, vr.N_FIX) as dm:
        dm.setMaps(torch.from_numpy(np.array(raw).view(np.int16)).cuda())
        for span in (1, 2):
            h = dm.checkMaps(cam, vr.CONFIG_FIX, vr.SPX_FIX, frames, views, span=span, tol_steps=vr.TOL_STEPS_FIX)
            d = dm.checkMaps(cam, vr.CONFIG_FIX, vr.SPX_FIX, frames, views, span=span, tol_steps=vr.TOL_STEPS_FIX, device_out=True)
            assert d.support.is_cuda and d.support.dtype == torch.uint8 and h.pair["n_consistent"].sum() > 0
            assert np.array_equal(d.support.cpu().numpy(), h.support) and np.array_equal(d.conflict.cpu().numpy(), h.conflict)
            assert d.pair.tobytes() == h.pair.tobytes()
            for dbl in (True, False):
                hf = dm.fuseMaps(cam, vr.CONFIG_FIX, vr.SPX_FIX, frames, views, span=span, tol_steps=vr.TOL_STEPS_FIX, out_double=dbl)
                df = dm.fuseMaps(cam, vr.CONFIG_FIX, vr.SPX_FIX, frames, views, span=span, tol_steps=vr.TOL_STEPS_FIX, out_double=dbl, device_out=True)
                assert df.xyz.is_cuda and df.n_points == hf.n_points > 0
                assert df.xyz.cpu().numpy().tobytes() == hf.xyz.tobytes()
                assert np.array_equal(df.src.cpu().numpy().view(np.uint32), hf.src) and np.array_equal(df.n_merged.cpu().numpy(), hf.n_merged)
    print("device pointers ok")


if __name__ == "__main__":
    main()
