"""lifcal_ba_residual_report / lifcal_ba_residual_groups: the per-observation errors against the oracle and the
existing projection, the lens ids against the caller's centres, the weights against their formula, every table against numpy on the
GPU's own per-observation arrays (only the order of summation differs), the totals against calcReprojectionError, caller keys,
bitwise reproducibility, rejections, side effects and two uses of the report (a bad frame, a shifted lens)."""
import functools

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, scene
from tests.helpers import SMALL_CASES, problem

pytestmark = pytest.mark.gpu

CASES = list(SMALL_CASES[::2])
if "constraints" not in [n for n, _ in CASES]:
    CASES.append(next(c for c in SMALL_CASES if c[0] == "constraints"))
CASES.append(("cfg2", scene.baseline_spec("cfg2")))
U = 2.0 ** -53   # unit roundoff of fp64
SUMS = ("sum_x", "sum_y", "sum_xx", "sum_yy", "sum_w")


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return scene.make_scene(dict(CASES)[name])


def options(**kw):
    o = capi.default_options_py()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def terms_of(ex, ey, w):
    return {"sum_x": ex, "sum_y": ey, "sum_xx": ex * ex, "sum_yy": ey * ey, "sum_w": w}


def check_table(table, key, n_keys, ex, ey, w, thr, what):
    """a table against numpy on the same ex, ey, weight: counts and maxima exact, every sum within the first-order bound of two
    orderings of an n-term sum, |s - numpy| <= 2 n 2^-53 sum |t_i|"""
    rows = table.rows
    assert len(rows) == n_keys, what
    cnt = np.bincount(key, minlength=n_keys)
    assert np.array_equal(rows["n"], cnt), what
    sq = ex * ex + ey * ey   # numpy rounds every operation on its own, as the kernel does (contraction off)
    thr2 = thr * thr
    assert np.all(np.abs(sq - thr2) > 1e-12 * thr2), "an |e|^2 lies on the inlier threshold: choose another threshold"
    assert np.array_equal(rows["n_inliers"], np.bincount(key, weights=(sq <= thr2), minlength=n_keys).astype(np.uint32)), what
    for col, v in (("max_abs_x", ex), ("max_abs_y", ey)):
        m = np.zeros(n_keys)
        np.maximum.at(m, key, np.abs(v))
        assert np.array_equal(rows[col], m), (what, col)
    for col, t in terms_of(ex, ey, w).items():
        ref = np.bincount(key, weights=t, minlength=n_keys)
        bound = 2.0 * cnt * U * np.bincount(key, weights=np.abs(t), minlength=n_keys)
        err = np.abs(rows[col] - ref)
        print(f"{what} {col}: max |s - numpy| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert np.all(err <= bound), (what, col, float(np.max(err - bound)))
    empty = cnt == 0
    assert not rows[empty].tobytes().strip(b"\0"), what   # an empty group is an all-zero row


def check_report(ba, pa, robust, thr):
    n = pa.struct.n_obs
    rep = ba.residualReport(thr)
    ex, ey, w, lens = rep.ex, rep.ey, rep.weight, rep.lens
    # errors against the oracle, input order (the bar of test_gpu_project_observations)
    _, err = oracle.reproj_stats(pa, thr, want_errors=True)
    d_or = max(np.max(np.abs(ex - err[:, 0])), np.max(np.abs(ey - err[:, 1])))
    # ... and against the existing projection: x_proj = fl(e + u), so x_proj - u is e to the rounding of that sum
    x, y = ba.projectObservations()
    tol = 2.0 * np.spacing(max(np.max(np.abs(pa.u)), np.max(np.abs(pa.v))))
    d_pr = max(np.max(np.abs(ex - (x - pa.u))), np.max(np.abs(ey - (y - pa.v))))
    print(f"errors: max |e - oracle| = {d_or:.3g} (1e-9), max |e - (proj - obs)| = {d_pr:.3g} ({tol:.3g})")
    assert d_or < 1e-9
    assert d_pr <= tol
    # lens ids
    info = ba.info()
    assert rep.lens_xy.shape == (info.n_lenses, 2) and len(rep.per_lens) == info.n_lenses
    assert lens.max() < info.n_lenses
    assert np.array_equal(bits(rep.lens_xy[lens, 0]), bits(pa.mcx)) and np.array_equal(bits(rep.lens_xy[lens, 1]), bits(pa.mcy))
    assert len(np.unique(bits(rep.lens_xy).reshape(-1, 2), axis=0)) == info.n_lenses
    # weights
    if robust:
        ls = ba.options.loss_scale
        ref = 1.0 / (1.0 + (ex * ex + ey * ey) / (ls * ls))
        d_w = np.max(np.abs(w - ref) / ref)
        print(f"weights: max relative difference {d_w:.3g} (1e-15)")
        assert d_w <= 1e-15
    else:
        assert np.all(w == 1.0)
    # tables
    check_table(rep.per_frame, pa.fr, pa.struct.n_frames, ex, ey, w, thr, "per_frame")
    check_table(rep.per_point, pa.pt, pa.struct.n_points, ex, ey, w, thr, "per_point")
    check_table(rep.per_lens, lens, info.n_lenses, ex, ey, w, thr, "per_lens")
    check_table(rep.total, np.zeros(n, np.uint32), 1, ex, ey, w, thr, "total")
    # totals against the existing call: both are sums of n positive terms, each within n 2^-53 (relative) of the exact sum of ITS
    # terms; the square root halves that, and the division and the root of either side round once each
    st = ba.calcReprojectionError(thr)
    tot = rep.total
    rel = 2.0 * n * U + 4.0 * U
    for a, b in ((tot.rms_x[0], st.std_x), (tot.rms_y[0], st.std_y)):
        print(f"total rms {a!r} against calcReprojectionError {b!r}: relative {abs(a - b) / b:.3g} ({rel:.3g})")
        assert abs(a - b) <= rel * b
    assert tot["max_abs_x"][0] == st.mae_x and tot["max_abs_y"][0] == st.mae_y
    assert tot.n[0] == st.num_points == n and tot.n_inliers[0] == st.num_inliers
    return rep


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_report_before_and_after_the_solve(built, name):
    sc = scene_of(name)
    pa = problem(sc)
    robust = bool(sc.config & 0x200)
    with BundleAdjustment(pa) as ba:
        check_report(ba, pa, robust, 1.0)
        ba.performBundleAdjustment()
        rep = check_report(ba, pa, robust, 0.25)
        # without the per-observation arrays the tables are the same
        small = ba.residualReport(0.25, per_observation=False)
        assert small.ex is None and small.per_frame.rows.tobytes() == rep.per_frame.rows.tobytes() and small.total.rows.tobytes() == rep.total.rows.tobytes()


def test_caller_keys(built):
    sc = scene_of("r2_tan_full")
    pa = problem(sc)
    n = pa.struct.n_obs
    sizes = [1, 63, 0, 0, 64, 65, 129]   # one entry, one short of a wave, two empty keys, a wave, one more, two waves and one
    assert n > sum(sizes)
    key = np.searchsorted(np.cumsum(sizes), np.arange(n), side="right").astype(np.uint32)   # the rest: key 7
    n_keys = len(sizes) + 2   # key 8 stays empty
    with BundleAdjustment(pa) as ba:
        rep = ba.residualReport(1.0)
        tab = ba.residualGroups(key, n_keys, 1.0)
        assert list(tab.n) == sizes + [n - sum(sizes), 0]
        check_table(tab, key, n_keys, rep.ex, rep.ey, rep.weight, 1.0, "caller keys")
        assert not tab.rows[[2, 3, 8]].tobytes().strip(b"\0")
        one = ba.residualGroups(np.zeros(n, np.uint32), 1, 1.0)
        assert one.rows.tobytes() == rep.total.rows.tobytes()
        bad = key.copy(); bad[n // 2] = n_keys
        with pytest.raises(LifcalError) as ei:
            ba.residualGroups(bad, n_keys, 1.0)
        assert ei.value.code == -1 and "lifcal_ba_residual_groups" in str(ei.value)
        again = ba.residualGroups(key, n_keys, 1.0)
        assert again.rows.tobytes() == tab.rows.tobytes()
        lib = capi.load_library()
        rows = np.zeros(n_keys, capi.GROUP_STATS_DTYPE)
        assert lib.lifcal_ba_residual_groups(ba._h, 1.0, n_keys, None, rows.ctypes.data) == -1
        assert lib.lifcal_ba_residual_groups(ba._h, 1.0, n_keys, capi.as_uptr(key), None) == -1


def report_bytes(rep):
    return [a.tobytes() for a in (rep.ex, rep.ey, rep.weight, rep.lens, rep.lens_xy, rep.per_frame.rows, rep.per_point.rows, rep.per_lens.rows, rep.total.rows)]


def test_report_is_bitwise_reproducible(built):
    sc = scene_of("constraints")
    with BundleAdjustment(problem(sc), options(deterministic=0)) as ba:
        a = report_bytes(ba.residualReport(1.0))
        b = report_bytes(ba.residualReport(1.0))
    with BundleAdjustment(problem(sc), options(deterministic=0)) as ba2:
        c = report_bytes(ba2.residualReport(1.0))
    assert a == b and a == c
    # the options that change how the SOLVE sums and evaluates do not reach the report: fp64 from the stored parameters, one order
    with BundleAdjustment(problem(sc), options(deterministic=1)) as ba3:
        assert report_bytes(ba3.residualReport(1.0)) == a
    with BundleAdjustment(problem(sc), options(precision=1)) as ba4:
        assert report_bytes(ba4.residualReport(1.0)) == a


def test_rejections(built):
    sc = scene_of("r2_tan_full")
    pa = problem(sc)
    with BundleAdjustment(pa, options(world_size=2, rank=0)) as ba:
        for call in (lambda: ba.residualReport(1.0), lambda: ba.residualGroups(np.zeros(pa.struct.n_obs, np.uint32), 1)):
            with pytest.raises(LifcalError) as ei:
                call()
            assert ei.value.code == -1 and "world_size" in str(ei.value)
    with BundleAdjustment(pa) as ba:
        lib = capi.load_library()
        assert lib.lifcal_ba_residual_report(ba._h, None) == -1
        assert lib.lifcal_ba_residual_report(None, None) == -1


def test_report_leaves_the_handle_as_it_was(built):
    """deterministic = 1 here: only then are calcReprojectionError and the sweep cost themselves reproducible to the bit"""
    sc = scene_of("constraints")

    def run(with_report):
        with BundleAdjustment(problem(sc), options(deterministic=1)) as ba:
            ba.sweep(1e4)
            if with_report:
                ba.residualReport(1.0)
                ba.residualGroups(np.zeros(sc.n_obs, np.uint32), 1)
            st = ba.calcReprojectionError(1.0)
            cost = ba.sweep(1e4).cost
            s = ba.performBundleAdjustment()
            return (st.std_x, st.std_y, st.mae_x, st.mae_y, st.num_points, st.num_inliers, cost, s.final_cost, s.iterations)

    assert run(True) == run(False)


def test_a_corrupted_frame_is_named(built):
    sc = scene_of("r2_tan_full")
    pa0 = problem(sc, initial=False)   # the true parameters: the errors are the observation noise
    bad = 3
    u = pa0.u.copy(); u[pa0.fr == bad] += 3.0
    pa = capi.ProblemArrays(u, pa0.v, pa0.mcx, pa0.mcy, pa0.pt, pa0.fr, pa0.cam, pa0.views, pa0.pts, sc.spx, sc.scale, sc.config)
    with BundleAdjustment(pa) as ba:
        rep = ba.residualReport(1.0, per_observation=False)
    assert int(np.argmax(rep.per_frame.rms_x)) == bad
    assert rep.per_frame.mean_x[bad] == pytest.approx(-3.0, abs=0.1)   # e = projected - observed


def test_a_shifted_lens_is_named(built):
    sc = scene_of("r2_tan_full")   # no robust loss
    pa0 = problem(sc, initial=False)
    centres, inverse, counts = np.unique(np.stack([pa0.mcx, pa0.mcy], 1), axis=0, return_inverse=True, return_counts=True)
    sel = inverse.reshape(-1) == int(np.argmax(counts))   # the lens with the most observations
    u = pa0.u.copy(); u[sel] += 0.5                       # e_x = projected - observed of these moves by -0.5 (noise: 0.1 px)
    pa = capi.ProblemArrays(u, pa0.v, pa0.mcx, pa0.mcy, pa0.pt, pa0.fr, pa0.cam, pa0.views, pa0.pts, sc.spx, sc.scale, sc.config)
    with BundleAdjustment(pa) as ba:
        rep = ba.residualReport(1.0)
    ids = np.unique(rep.lens[sel])
    assert len(ids) == 1
    assert int(np.argmax(np.abs(rep.per_lens.mean_x))) == int(ids[0])   # the largest mean offset
    assert rep.per_lens.mean_x[ids[0]] == pytest.approx(-0.5, abs=0.1)
    assert rep.per_lens.n[ids[0]] == np.count_nonzero(sel)
