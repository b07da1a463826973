"""lifcal_rawdepth_estimate with its options away from their defaults (include/lifcal_rawdepth.h): every
option at the ends of its range and at values that are no multiple of anything in the kernel, against the numpy restatement byte
for byte.  Each option set comes with a condition on the counts showing that the option acts; the condition is checked on the
restatement's counts and on the kernel's.  The cases are d14 (8 bit, patch radius 1) and d23_16 (16 bit, patch radius 2) of
rawdepth_reference.CASES on the step scene with noise, and d6, a grid of lenses so small that at patch radius 2 no pair counts."""
import numpy as np
import pytest

from lifcal_amd import MicroLensGrid
from tests import rawdepth_reference as ref

pytestmark = pytest.mark.gpu

_GRIDS = {}
NAMES = ("d14", "d23_16")
# option set: (scene, options); "radius" and "contrast_mid" depend on the case (see options_of)
OPTION_SETS = {
    "default": ("step", dict()),
    "default_18": ("step", dict(max_baseline=2.1)),
    "default_mid": ("mid", dict()),
    "n_hyp_8": ("step", dict(n_hyp=8)),                                   # the minimum
    "n_hyp_37": ("step", dict(n_hyp=37)),                                 # a multiple of nothing in the kernel
    "n_hyp_256": ("step", dict(n_hyp=256)),                               # the maximum: many local minima
    "n_hyp_256_ratio_4": ("step", dict(n_hyp=256, ambiguity_ratio=4.0)),  # and many of them below the threshold: the four slots
    "ratio_1": ("step", dict(ambiguity_ratio=1.0)),                       # no cost is below c0: nothing is ambiguous
    "ratio_4": ("step", dict(ambiguity_ratio=4.0)),
    "ratio_1e6": ("step", dict(ambiguity_ratio=1.0e6)),                   # every second distant minimum is ambiguous
    "min_nb_1": ("step", dict(min_neighbours=1)),
    "min_nb_5": ("step", dict(min_neighbours=5)),
    "min_nb_6_of_6": ("step", dict(min_neighbours=6)),
    "min_nb_18_of_18": ("step", dict(min_neighbours=18, max_baseline=2.1)),
    "min_nb_7_of_6": ("step", dict(min_neighbours=7)),                    # allowed, and no hypothesis has a finite cost
    "contrast_1": ("step", dict(min_contrast=1)),
    "contrast_mid": ("step", None),                                       # 60 of 255 (8 bit, 3 x 3) and 30000 of 65535 (16 bit, 5 x 5)
    "contrast_max": ("step", dict(min_contrast=65535)),
    "iv_narrow_step": ("step", dict(iv_min=0.2, iv_max=0.3, n_hyp=8)),    # the true depths (1 / 3.2, 1 / 5.5) lie at or beyond the ends
    "iv_narrow_mid": ("mid", dict(iv_min=0.2, iv_max=0.3, n_hyp=8)),      # 1 / 4 lies inside
    "iv_upper_end_mid": ("mid", dict(iv_min=0.04, iv_max=0.26)),          # 1 / 4 lies three steps below the upper end
    "radius_swapped": ("step", None),                                     # 8 bit with radius 2, 16 bit with radius 1
}


def setup(name):
    """(grid, its data for the restatement), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def options_of(name, key):
    """(scene, options with patch_radius) of an option set on a case"""
    bits, pr = ref.case(name)[5:7]
    scn, o = OPTION_SETS[key]
    if key == "contrast_mid":
        o = dict(min_contrast=60 if bits == 8 else 30000)
    elif key == "radius_swapped":
        o = dict(patch_radius=3 - pr)
    return scn, {"patch_radius": pr, **o}


def restatement(name, key, gd):
    scn, o = options_of(name, key)
    return ref.run(name, scn, ref.NOISE, gd, **o)


def check_option_acts(name, key, counts, gd):
    """the condition of an option set on `counts` (of the restatement or of the kernel), where it compares, against the
    restatement's counts of another set on the same image"""
    c = [int(v) for v in counts]
    other = lambda k: [int(v) for v in restatement(name, k, gd).counts]
    with_lens = sum(c) - c[1]
    if key in ("n_hyp_8", "n_hyp_37"):
        assert c[0] > 0.3 * with_lens
    elif key == "n_hyp_256":
        assert c[4] > other("default")[4] and c[0] > 0          # status 4 grows with the number of minima
    elif key == "n_hyp_256_ratio_4":
        assert c[4] > other("n_hyp_256")[4] and c[0] > 0
    elif key == "ratio_1":
        assert c[4] == 0 and c[0] == other("default")[0] + other("default")[4]
    elif key == "ratio_4":
        assert c[4] > other("default")[4] and c[0] + c[4] == other("default")[0] + other("default")[4]
    elif key == "ratio_1e6":
        assert c[4] > other("ratio_4")[4] and c[4] > c[0] and c[0] + c[4] == other("default")[0] + other("default")[4]
    elif key == "min_nb_1":
        assert c[3] < other("default")[3]
    elif key == "min_nb_5":
        assert c[3] > other("default")[3] and c[3] > c[0] > 0          # status 3 dominates
    elif key == "min_nb_6_of_6":
        assert c[3] > other("min_nb_5")[3] and c[0] > 0
    elif key == "min_nb_18_of_18":
        assert c[3] > other("default_18")[3] and c[0] > 0
    elif key == "min_nb_7_of_6":
        assert c[0] == 0 and c[4] == 0 and c[3] == with_lens - c[2] > 0
    elif key == "contrast_1":
        assert c[2] <= other("default")[2] and c[0] >= other("default")[0]
    elif key == "contrast_mid":
        assert c[2] > 0.1 * with_lens and c[2] > other("default")[2] and c[0] > 0.1 * with_lens          # a real share is flat
    elif key == "contrast_max":
        assert c[2] == with_lens > 0 and c[0] == c[3] == c[4] == 0
    elif key == "iv_narrow_step":
        assert c[3] > c[0] and c[3] > other("default")[3]          # status 3 dominates
    elif key == "iv_narrow_mid":
        assert c[0] > c[3] and c[0] > 0.5 * with_lens          # it still measures
    elif key == "iv_upper_end_mid":
        assert 0 < c[0] and c[3] != other("default_mid")[3]
    elif key == "radius_swapped":
        assert (c[1] > other("default")[1]) == (options_of(name, key)[1]["patch_radius"] == 2) and c[1] != other("default")[1] and c[0] > 0


def assert_equal(got, want, what):
    bad = np.flatnonzero(got.status.ravel() != want.status.ravel())
    assert bad.size == 0, (what, bad.size, bad[:8], got.status.ravel()[bad[:8]], want.status.ravel()[bad[:8]])
    assert np.array_equal(got.n_neighbours, want.n_neighbours), what
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (what, got.counts, want.counts)
    for f in ("inv_depth", "cost"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape
        bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
        assert bad.size == 0, (what, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])


@pytest.mark.parametrize("key", [k for k in OPTION_SETS if not k.startswith("default")])
@pytest.mark.parametrize("name", NAMES)
def test_option_equals_restatement(built, name, key):
    """status, n_neighbours and the counts equal, inv_depth and cost the same bytes, and the option acts"""
    g, gd = setup(name)
    scn, o = options_of(name, key)
    want = restatement(name, key, gd)
    check_option_acts(name, key, want.counts, gd)
    got = g.estimateRawDepth(ref.make_case(name, scn, ref.NOISE), **o)
    print(f"{name} {key} {scn} {o}: counts {got.counts.tolist()} (defaults {restatement(name, 'default_mid' if scn == 'mid' else 'default', gd).counts.tolist()}), "
          f"{got.seconds * 1e3:.3f} ms")
    assert_equal(got, want, (name, key))
    check_option_acts(name, key, got.counts, gd)
    if key == "iv_narrow_mid":
        a = ref.accuracy(name, "mid", got, gd.cx, gd.cy, gd.map_ml)
        print(f"{name} {key}: coverage {a['coverage']:.3f}, outliers {a['outliers']:.4f}, inlier rms {a['rms']:.5f}")
        assert a["outliers"] <= ref.CONDITIONS["mid"][1]
    if key == "min_nb_18_of_18":
        assert np.all(got.n_neighbours[(got.status == 0) | (got.status == 4)] == 18)


@pytest.mark.parametrize("radius", (1, 2))
def test_lenses_too_small_for_the_patch(built, radius):
    """d6: 6.5-pixel lenses, valid_r = 2.25.  At patch radius 2, r0 = 0.25 and r1 < 0: no pair counts, so nothing is measured or
    ambiguous, and status 1, 2 and 3 equal the restatement.  At radius 1, r1 = 0.25: what the restatement measures, if anything,
    the kernel measures bit for bit."""
    name = "d6"
    g, gd = setup(name)
    want = ref.run(name, "step", ref.NOISE, gd, patch_radius=radius)
    got = g.estimateRawDepth(ref.make_case(name, "step", ref.NOISE), patch_radius=radius)
    print(f"{name} radius {radius}: counts {got.counts.tolist()}, restatement {want.counts.tolist()}, {got.seconds * 1e3:.3f} ms")
    assert_equal(got, want, (name, radius))
    assert want.counts[1] < want.status.size          # some pixels pass the r0 test: the kernel's pair loop runs
    if radius == 2:
        assert got.counts[0] == 0 and got.counts[4] == 0 and got.counts[3] > 0
        assert np.all(np.isnan(got.inv_depth)) and np.all(np.isnan(got.cost)) and not got.n_neighbours.any()
