"""lifcal_depthmap_from_raw with its options away from their defaults and on inputs lifcal_rawdepth_estimate never writes
(include/lifcal_depthmap.h): all four maps, the counts and n_samples against the numpy restatement byte for
byte, each option set with a condition on the counts showing that the option acts, checked on the restatement's counts and on
the kernel's.  The inputs are the raw-depth restatement's inv_depth of d14 and d9_pitch of rawdepth_reference.CASES."""
import numpy as np
import pytest

from lifcal_amd import MicroLensGrid, depth_map
from tests import depthmap_reference as dref
from tests import rawdepth_reference as ref

pytestmark = pytest.mark.gpu

_GRIDS = {}
NAMES = ("d14", "d9_pitch")
FIELDS = ("inv_depth", "depth16", "status", "support")


def case(name):
    """(grid, its data for the restatements), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def raw_depth_of(name, scn):
    """the raw-depth restatement's inv_depth with noise: the comparison does not depend on the sweep kernel"""
    _, gd = case(name)
    return ref.run(name, scn, ref.NOISE, gd, max_baseline=dref.MAX_BASELINE).inv_depth


def both(name, iv, **kw):
    """(the library's map, the restatement's) of one input, compared byte for byte"""
    g, gd = case(name)
    want = dref.depth_map(iv, gd.map_ml, gd.cx, gd.cy, **kw)
    got = depth_map.depthMapFromRaw(g, iv, **kw)
    print(f"{name} {kw}: counts {got.counts.tolist()}, {got.n_samples} samples, {got.seconds * 1e3:.3f} ms")
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (kw, f, a.dtype, a.shape, b.shape)
        bits = "u%d" % a.itemsize
        bad = np.flatnonzero(a.ravel().view(bits) != b.ravel().view(bits))
        assert bad.size == 0, (kw, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (kw, got.counts, want.counts)
    assert got.n_samples == want.n_samples, kw
    return got, want


@pytest.mark.parametrize("name", NAMES)
def test_fill_rounds_odd_and_largest(built, name):
    """1, 3 and 64 rounds (the fill ping-pongs two buffers, so an odd count ends in the other one; 64 is the maximum) on the near
    scene: the filled cells do not decrease with the rounds and are strictly more at 3 than at 1"""
    iv = raw_depth_of(name, "near")
    filled = {}
    for rounds in (1, 2, 3, 64):
        got, want = both(name, iv, fill_rounds=rounds)
        filled[rounds] = (int(want.counts[1]), int(got.counts[1]))
    for k in (0, 1):
        assert filled[1][k] <= filled[2][k] <= filled[3][k] <= filled[64][k] and 0 < filled[1][k] < filled[3][k], filled


def test_fill_closes_an_isolated_hole(built):
    """the mid scene of d14 with the raw depth of a 70 x 70 block removed: a cell is seen through lenses within valid_r v = 24.6 px
    of it, so the middle of the block has no sample.  Two rounds leave a hole, 64 close it"""
    name = "d14"
    iv = np.array(raw_depth_of(name, "mid"))
    iv[45:115, 65:135] = np.nan
    inner = (slice(30, 130), slice(50, 150))
    two, want2 = both(name, iv, fill_rounds=2)
    all_, want64 = both(name, iv, fill_rounds=64)
    for m in (want2, two):
        assert (m.status[inner] >= 2).sum() > 25
    for m in (want64, all_):
        assert not (m.status[inner] >= 2).any() and (m.status[inner] == 1).sum() > 25


@pytest.mark.parametrize("name", NAMES)
def test_fill_min_neighbours_at_both_ends(built, name):
    iv = raw_depth_of(name, "near")
    _, base = both(name, iv)
    got1, want1 = both(name, iv, fill_min_neighbours=1)
    got8, want8 = both(name, iv, fill_min_neighbours=8)
    for one, eight in ((want1, want8), (got1, got8)):
        assert one.counts[1] > base.counts[1] > eight.counts[1] and one.counts[0] == base.counts[0] == eight.counts[0]


@pytest.mark.parametrize("name", NAMES)
def test_min_support_above_the_default(built, name):
    """5, and one more than the largest support of any cell: then no cell is measured, nothing can be filled, and without fill
    every cell that a sample reaches is status 3"""
    iv = raw_depth_of(name, "near")
    _, base = both(name, iv)
    got5, want5 = both(name, iv, min_support=5)
    for m in (want5, got5):
        assert 0 < m.counts[0] < base.counts[0] and m.counts[3] > base.counts[3]
    _, plain = both(name, iv, min_support=1, fill_rounds=-1)
    top = int(plain.support.max()) + 1
    assert 5 < top < 65535
    got, want = both(name, iv, min_support=top)
    for m in (want, got):
        assert m.counts[0] == 0 and m.counts[1] == 0
    got, want = both(name, iv, min_support=top, fill_rounds=-1)
    for m in (want, got):
        assert m.counts[0] == 0 and m.counts[1] == 0 and np.array_equal(m.status == 3, plain.support > 0) and np.array_equal(m.status == 2, plain.support == 0)
    _, under = both(name, iv, min_support=top - 1, fill_rounds=-1)
    assert under.counts[0] > 0          # the value above is the first that no cell reaches


@pytest.mark.parametrize("name", NAMES)
def test_tol_iv_narrow_and_wide(built, name):
    """0.001 and 0.5 (the maximum) on the step scene, where the front rule decides which samples a cell averages"""
    iv = raw_depth_of(name, "step")
    gotn, narrow = both(name, iv, tol_iv=0.001)
    gotw, wide = both(name, iv, tol_iv=0.5)
    for n, w in ((narrow, wide), (gotn, gotw)):
        assert n.inv_depth.tobytes() != w.inv_depth.tobytes() and n.counts[0] > 0 and w.counts[0] > 0
        assert n.counts[3] >= w.counts[3] and n.support.astype(np.int64).sum() < w.support.astype(np.int64).sum()


@pytest.mark.parametrize("name", NAMES)
def test_scale_four(built, name):
    w, h = ref.case(name)[:2]
    for scn in ("near", "step"):
        got, want = both(name, raw_depth_of(name, scn), scale=4)
        assert got.status.shape == (h // 4, w // 4) and got.scale == 4 and want.counts[0] > 0.3 * want.status.size


def test_hand_made_values_at_the_limits_of_a_sample(built):
    """the mid scene's inv_depth of d14 with blocks of pixels inside lenses overwritten by values lifcal_rawdepth_estimate never
    writes: above 0.5, exactly 1 (q = Q), the float above 1, the float below iv_min, zero, negative, both infinities and a NaN of
    another payload.  n_samples is what the header's rule counts; the float map keeps a value above 0.5 that the PNG encoding
    refuses"""
    name = "d14"
    _, gd = case(name)
    iv = np.array(raw_depth_of(name, "mid"))
    iv_min = dref.DEFAULTS["iv_min"]
    other_nan = np.array([0xffc00123], np.uint32).view(np.float32)[0]          # quiet, with a sign and a payload numpy's NaN has not
    below = np.float32(iv_min) if float(np.float32(iv_min)) < iv_min else np.nextafter(np.float32(iv_min), np.float32(0))
    first = np.nextafter(below, np.float32(1))                                  # the smallest float that is a sample
    values = [0.75, 1.0, np.nextafter(np.float32(1), np.float32(2)), below, first, 0.0, -0.2, np.inf, -np.inf, other_nan]
    assert np.isnan(other_nan) and float(below) < iv_min <= float(first) and float(values[2]) > 1.0
    # 5 x 5 pixels about the centre of a lens: inside the lens (valid_r = 6.15), so that the map alone would make them samples.
    # A cell keeps a value behind the scene (iv 0.25) only where no other sample lands, so for 0.75 and 1.0 the raw depth of a
    # 60 x 60 block about the lens is removed first: a cell is seen through lenses within valid_r v = 24.6 px of it, so nothing
    # else reaches the 5 px about the block's middle, where those samples land (v <= 4 / 3)
    w, h = ref.case(name)[:2]
    nearest = lambda x, y: int(np.argmin((gd.cx.astype(np.float64) - x) ** 2 + (gd.cy.astype(np.float64) - y) ** 2))
    alone = [nearest(50.0, 80.0), nearest(150.0, 80.0)]
    for j in alone:
        y, x = int(round(float(gd.cy[j]))), int(round(float(gd.cx[j])))
        iv[y - 30:y + 30, x - 30:x + 30] = np.nan
    rest = [j for j in range(len(gd.cx)) if 20 <= gd.cx[j] <= w - 21 and (20 <= gd.cy[j] <= 34 or h - 35 <= gd.cy[j] <= h - 21)]
    lenses = alone + rest[::2][:len(values) - 2]
    assert len(lenses) == len(values) == len(set(lenses))
    for j, v in zip(lenses, values):
        y, x = int(round(float(gd.cy[j]))) - 2, int(round(float(gd.cx[j]))) - 2
        assert np.all(gd.map_ml[y:y + 5, x:x + 5] == j)
        iv[y:y + 5, x:x + 5] = v
    with np.errstate(invalid="ignore"):
        ivd = iv.astype(np.float64)
        n_rule = int(((gd.map_ml >= 0) & (ivd >= iv_min) & (ivd <= 1.0)).sum())
    for kw in (dict(fill_rounds=-1, min_support=1), dict()):
        got, want = both(name, iv, **kw)
        assert got.n_samples == n_rule == want.n_samples
        for m in (want, got):
            above = (m.status <= (0 if kw else 1)) & (m.inv_depth > 0.5)          # one sample per cell at v <= 4 / 3: min_support 2 rejects them
            assert not m.depth16[above].any() and above.any() == bool(kw)
            assert (m.inv_depth == 1.0).any() == (want.inv_depth == 1.0).any() == bool(kw)
            assert np.array_equal(m.depth16 > 0, (m.status <= 1) & (m.inv_depth <= 0.5))
        print(f"{kw}: {n_rule} samples, {int(above.sum())} cells above 0.5, {int((want.inv_depth == 1.0).sum())} cells at exactly 1")
