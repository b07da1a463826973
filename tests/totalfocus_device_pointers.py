"""Child process of tests/test_gpu_totalfocus.py::test_device_pointers_through_torch_tensors: torch initialises the GPU first (of two
HIP runtimes in one process only the first to start sees it), then lifcal_totalfocus_render takes the raw image, the white image
and the depth map from torch tensors on the device (dense and with a row pitch) and writes its maps into torch tensors, and
VirtualDepthMap.total_focus goes from the raw image to the picture without leaving the device.  Compared byte for byte with the
host-pointer path."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("image", "n_lenses", "status")


def to_device(a: np.ndarray, extra: int = 0):
    """a 2-D array as a tensor on the device, 16-bit as int16 bits; extra: columns of row pitch beyond the image"""
    src = a.view(np.int16) if a.dtype == np.uint16 else a
    wide = torch.full((a.shape[0], a.shape[1] + extra), 77, dtype=torch.from_numpy(src[:1, :1].copy()).dtype, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    return wide[:, :a.shape[1]]


def main():
    torch.cuda.init()
    torch.zeros(1, device="cuda"); torch.cuda.synchronize()
    from lifcal_amd import MicroLensGrid, total_focus
    from tests import rawdepth_reference as ref
    from tests import totalfocus_reference as tref
    for name in ref.CASES:
        g = MicroLensGrid(*ref.grid_arguments(name))
        img, white = tref.vignetted_case(name, "step", ref.NOISE), tref.white_case(name)
        kw = dict(white_level=tref.white_level(name))
        for scale in (1, 2):
            iv = np.array(tref.true_depth(name, "step", scale))
            iv[3:9, 4:20] = np.nan
            host = total_focus.totalFocusImage(g, img, iv, white=white, scale=scale, **kw)
            assert host.counts[0] > 0 and host.counts[1] == 6 * 16
            t_img, t_white, t_iv = to_device(img, 5), to_device(white, 11), torch.from_numpy(iv).cuda()
            assert t_img.stride(0) == img.shape[1] + 5 and t_white.stride(0) == img.shape[1] + 11
            got = total_focus.totalFocusImage(g, t_img, t_iv, white=t_white, device_out=True, scale=scale, **kw)        # all on the device
            mixed = total_focus.totalFocusImage(g, to_device(img), iv, white=white, scale=scale, **kw)                # device image, host rest
            mixed2 = total_focus.totalFocusImage(g, img, t_iv, white=to_device(white), scale=scale, **kw)             # host image, device rest
            for f in FIELDS:
                a, b = getattr(got, f), getattr(host, f)
                assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes(), (name, scale, f)
                assert getattr(mixed, f).tobytes() == b.tobytes() and getattr(mixed2, f).tobytes() == b.tobytes(), (name, scale, f)
            assert np.array_equal(got.counts, host.counts) and np.array_equal(mixed.counts, host.counts)
            plain = total_focus.totalFocusImage(g, t_img, t_iv, device_out=True, scale=scale)                         # without a white image
            assert plain.image.cpu().numpy().tobytes() == total_focus.totalFocusImage(g, img, iv, scale=scale).image.tobytes()
        # from the raw image to the picture on the device: estimateRawDepth -> depth_map -> total_focus
        raw = np.array(ref.make_case(name, "mid", ref.NOISE))
        est = g.estimateRawDepth(to_device(raw), device_out=True, patch_radius=ref.CASES[name][6], max_baseline=2.1)
        for scale in (1, 2):
            dm = est.depth_map(device_out=True, scale=scale)
            tf = dm.total_focus(g, to_device(raw, 3))
            assert tf.image.is_cuda and tf.status.is_cuda and tf.scale == scale
            host = total_focus.totalFocusImage(g, raw, dm.inv_depth.cpu().numpy(), scale=scale)
            for f in FIELDS:
                assert getattr(tf, f).cpu().numpy().tobytes() == getattr(host, f).tobytes(), (name, scale, f)
            assert np.array_equal(tf.counts, host.counts) and host.counts[0] > 0.9 * host.status.size
        try:
            total_focus.totalFocusImage(g, raw, est.inv_depth.double())
        except ValueError:
            pass
        else:
            raise AssertionError("a double tensor was accepted as inv_depth")
    print("device pointers ok")


if __name__ == "__main__":
    main()
