"""lifcal_totalfocus_render with its options away from their defaults and on depth maps and white images the other tests never
give it (include/lifcal_totalfocus.h): image, n_lenses, status and the counts against the numpy restatement
byte for byte, each option set with a condition showing that the option acts, checked on the restatement and on the kernel's
output.  The cases are d14 (8 bit) and d23_16 (16 bit) of rawdepth_reference.CASES on the step scene with noise."""
import numpy as np
import pytest

from lifcal_amd import MicroLensGrid
from tests import rawdepth_reference as ref
from tests import totalfocus_reference as tref

pytestmark = pytest.mark.gpu

_GRIDS = {}
NAMES = ("d14", "d23_16")
FIELDS = ("image", "n_lenses", "status")


def case(name):
    """(grid, its data for the restatements), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def both(name, img, iv, white=None, **kw):
    """(the library's picture, the restatement's) of one input, compared byte for byte"""
    g, gd = case(name)
    want = tref.render(img, iv, gd.cx, gd.cy, ref.case(name)[2], white=white, **kw)
    got = g.totalFocusImage(img, iv, white=white, **kw)
    print(f"{name} {kw}: counts {got.counts.tolist()}, at most {int(want.n.max())} lenses, {got.seconds * 1e3:.3f} ms")
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (kw, f, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a.ravel() != b.ravel())
        assert bad.size == 0, (kw, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (kw, got.counts, want.counts)
    return got, want


def step(name, scale=1):
    return ref.make_case(name, "step", ref.NOISE), tref.true_depth(name, "step", scale)


@pytest.mark.parametrize("name", NAMES)
def test_margin_at_both_ends(built, name):
    """margin 0 (the whole valid disc) and 3 px: more and fewer lenses per cell than with the default 1.5"""
    img, iv = step(name)
    got0, want0 = both(name, img, iv, margin=0.0)          # 0.0 selects the default in the struct: the same picture as no option
    _, base = both(name, img, iv)
    assert np.array_equal(want0.n, base.n)
    gots, small = both(name, img, iv, margin=0.25)
    gotl, large = both(name, img, iv, margin=3.0)
    assert small.n.max() > base.n.max() > large.n.max() >= 1 and small.n.sum() > base.n.sum() > large.n.sum()
    assert gots.n_lenses.max() > got0.n_lenses.max() > gotl.n_lenses.max() >= 1
    assert large.counts[0] > 0.9 * large.status.size


@pytest.mark.parametrize("name", NAMES)
def test_max_reach_at_both_ends(built, name):
    """0.4 d: only lenses whose centre lies within 0.4 d of the cell, three at the most (the closest three centres form a
    triangle of side d, whose circumradius is 0.577 d, so a disc of radius 0.4 d holds one; the bound of the issue is three);
    8 d, the maximum, on a map at iv = 0.045, where the disc test alone admits r_use / iv = 7.2 d (d14) and more than 8 d
    (d23_16): more lenses than with the default 4 d"""
    img, iv = step(name)
    got, want = both(name, img, iv, max_reach=0.4)
    assert 1 <= want.n.max() <= 3 and got.n_lenses.max() <= 3 and want.counts[2] > 0 and want.counts[0] > 0
    deep = np.full(iv.shape, 0.045, np.float32)
    got4, want4 = both(name, img, deep)
    got8, want8 = both(name, img, deep, max_reach=8.0)
    assert want8.n.max() > want4.n.max() > 7 and got8.n_lenses.max() > got4.n_lenses.max()
    assert want8.counts[0] == want8.status.size


@pytest.mark.parametrize("name", NAMES)
def test_iv_min_at_both_ends(built, name):
    """the step scene's map (1 / 3.2 and 1 / 5.5) with a block at 0.02: iv_min 0.001 makes the block cells with a depth (status 1
    by default), iv_min 0.3 leaves only the near side of the step"""
    img, iv = step(name)
    iv = np.array(iv); iv[10:30, 10:40] = 0.02
    _, base = both(name, img, iv)
    got_lo, lo = both(name, img, iv, iv_min=0.001)
    got_hi, hi = both(name, img, iv, iv_min=0.3)
    assert base.counts[1] == 600 and np.all(base.status[10:30, 10:40] == 1)
    for m in (lo, got_lo):
        assert m.counts[1] == 0 and not np.any(m.status[10:30, 10:40] == 1)
    for m in (hi, got_hi):
        assert np.array_equal(m.status == 1, iv < 0.3) and 0.2 * iv.size < m.counts[1] < 0.8 * iv.size and m.counts[0] > 0


@pytest.mark.parametrize("name", NAMES)
def test_min_lenses_two_and_the_largest(built, name):
    """2: the cells one lens sees lose their pixel; 255: every cell with a depth is status 2, its n_lenses kept"""
    img, iv = step(name)
    _, base = both(name, img, iv)
    got2, two = both(name, img, iv, min_lenses=2)
    got255, most = both(name, img, iv, min_lenses=255)
    assert np.array_equal(two.status == 2, base.n < 2) and (base.n == 1).any() and two.counts[0] > 0
    for m in (most, got255):
        assert m.counts.tolist() == [0, 0, iv.size, 0] and not m.image.any() and np.array_equal(m.n_lenses, base.n_lenses)
    assert np.array_equal(got2.status == 2, base.n < 2)


@pytest.mark.parametrize("how", ("value", "default_iv"))
@pytest.mark.parametrize("name", NAMES)
def test_one_deep_cell_per_tile_changes_no_other_cell(built, name, how):
    """a map at 0.4 except one cell in every 16 x 16 tile, which is at 0.045 or NaN with default_iv = 0.045: the tile's bin range
    is set by that one cell (r_use / 0.045 against r_use / 0.4), and the other cells must come out as in the all-0.4 map"""
    img, iv = step(name)
    flat = np.full(iv.shape, 0.4, np.float32)
    mixed = flat.copy()
    mixed[5::16, 11::16] = 0.045 if how == "value" else np.nan
    deep = mixed != flat
    assert deep.sum() == len(range(5, iv.shape[0], 16)) * len(range(11, iv.shape[1], 16)) >= 80
    kw = dict(default_iv=0.045) if how == "default_iv" else dict()
    got_flat, want_flat = both(name, img, flat, **kw)
    got, want = both(name, img, mixed, **kw)
    for m, f in ((want, want_flat), (got, got_flat)):
        for field in FIELDS:
            assert np.array_equal(getattr(m, field)[~deep], getattr(f, field)[~deep]), field
        assert np.all(m.status[deep] == (0 if how == "value" else 3)) and m.n_lenses[deep].min() > m.n_lenses[~deep].max()


@pytest.mark.parametrize("name", NAMES)
def test_white_image_with_dark_lenses(built, name):
    """a white image with a block of zeros that covers whole lenses: a cell all of whose lenses lie in the block has den = 0 and
    is status 2 with its n_lenses kept"""
    iv = tref.true_depth(name, "step", 1)
    img = tref.vignetted_case(name, "step", ref.NOISE)
    white = np.array(tref.white_case(name))
    h, w = white.shape
    white[h // 4:3 * h // 4, w // 4:3 * w // 4] = 0
    got, want = both(name, img, iv, white=white, white_level=tref.white_level(name))
    for m in (want, got):
        dark = (m.status == 2) & (m.n_lenses > 0)
        assert dark.sum() > 100 and not m.image[dark].any() and m.counts[0] > 0.3 * m.status.size


@pytest.mark.parametrize("name", NAMES)
def test_white_level_above_the_white_image_clamps_at_full_scale(built, name):
    """the white image at a quarter of its brightness under the same white_level (white_level four times the white image's own
    level): the quotient is four times the picture, and min(full, ...) acts wherever that exceeds full scale"""
    iv = tref.true_depth(name, "step", 1)
    img = tref.vignetted_case(name, "step", ref.NOISE)
    white = (tref.white_case(name) // 4).astype(img.dtype)
    full = 255 if ref.case(name)[5] == 8 else 65535
    got, want = both(name, img, iv, white=white, white_level=tref.white_level(name))
    for m in (want, got):
        ok = m.status == 0
        assert (m.image[ok] == full).sum() > 0.05 * ok.sum() and (m.image[ok] < full).sum() > 0.05 * ok.sum()
