"""Times lifcal_markers_components and lifcal_markers_detect (include/lifcal_markers.h) at one realistic size:
2048 x 1536, 8 bit, twelve markers of 120 to 200 pixels under rotation and perspective with blur, noise and shading, the
generator's 50-word 4-bit dictionary.  Prints the device times (`seconds`: HIP events around the kernels), median and minimum of
six calls after a warm-up call, and what was found.  The figures of section 7y's table come from this script.

usage: markers_timing.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lifcal_amd import marker_image as mi, markers  # noqa: E402
from tests import markers_reference as mr  # noqa: E402

words, dmin = mr.dictionary()
d = markers.Dictionary(4, words)
placed = []
for k in range(12):
    cx, cy = 260 + 500 * (k % 4) + 13.3 * k, 260 + 500 * (k // 4) + 7.1 * k
    placed.append(mi.place(k, mr.word_bits(words[k], 4), cx, cy, 120 + 20 * (k % 5), 7.5 * k + 90 * (k % 4), 0.15 * (k % 2), 30.0 * k))
img = mi.render_markers((1536, 2048), placed, supersample=1, blur=0.8, noise=2.0, shading=0.3, seed=5)
comp_s, det_s = [], []
for rep in range(7):
    c = markers.markerComponents(img)
    m = markers.detectMarkers(img, d)
    comp_s.append(c.seconds); det_s.append(m.seconds)
found = sorted(m.id.tolist())
err = [float(np.hypot(m.x[i] - placed[int(m.id[i])].centre[0], m.y[i] - placed[int(m.id[i])].centre[1])) for i in range(m.n)]
print(f"markers found {found} of 12, refined {int(m.refined.sum())}, candidates {m.n_candidates}, dark pixels {int(c.dark.sum())}, "
      f"max centre error {max(err):.3f} px")
print(f"components (steps 1-3) median {1e3 * np.median(comp_s[1:]):.3f} ms, min {1e3 * min(comp_s[1:]):.3f} ms")
print(f"detect (steps 1-7) median {1e3 * np.median(det_s[1:]):.3f} ms, min {1e3 * min(det_s[1:]):.3f} ms; "
      f"decode (steps 4-7) about {1e3 * (np.median(det_s[1:]) - np.median(comp_s[1:])):.3f} ms")
