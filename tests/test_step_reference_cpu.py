"""tests/step_reference.py pinned without a GPU: the matrix-free normal equations against the dense ones of test_oracle_schur.py, the
CPU reference step against an independent dense solve, and the proof that the measure moves when one block of the step is wrong."""
import numpy as np
import pytest

from lifcal_amd import scene
from tests import step_reference as sr
from tests.helpers import S, problem
from tests.test_oracle_schur import dense_system

BOUND = 32.0   # the margin tests/test_gpu_step.py gives the kernels over the reference (reasoned there)

DENSE_CASES = [
    S(5, 25, None, 0x506, 401),
    S(5, 25, None, 0xF06, 402, outlier_fraction=0.05),
    S(5, 25, None, 0x506, 403, n_constraints=3),
    S(6, 30, None, 0xF06, 404, recalib=True),
]


@pytest.mark.parametrize("spec", DENSE_CASES, ids=["plain", "robust_adj", "constraints", "recalib_fixed"])
def test_matrix_free_system_equals_the_dense_one(spec):
    sc = scene.make_scene(spec)
    pa = problem(sc)
    radius = 3e3
    cost, H, g, delta, live = dense_system(sc, pa, radius)
    ne = sr.NormalEquations(pa, radius)
    n = ne.n
    assert ne.check_dead_rows() == int(np.sum(~live)) and np.array_equal(ne.live, live)
    assert abs(ne.cost - cost) <= 1e-13 * cost
    # g, h and lambda: sums of at most 2 N + M products, compared with numpy's double sums of the same terms
    tol = 8 * (2 * ne.N + 8) * sr.EPS
    g_scale = ne._JT(np.abs(ne.r), np.abs(ne.rc), ne._absA).astype(np.float64)   # sum of the |terms| of every g_i
    assert np.all(np.abs(ne.g.astype(np.float64) - g) <= tol * g_scale)
    h = np.diag(H)
    assert np.allclose(ne.h.astype(np.float64), h, rtol=tol, atol=0)
    sig = 1.0 / (1.0 + np.sqrt(h))
    lam = np.where(live, np.clip(h * sig * sig, 1e-6, 1e32) / (radius * sig * sig), 0.0)
    assert np.allclose(ne.lam.astype(np.float64), lam, rtol=4 * tol, atol=0)
    # the products, on a vector with entries of every sign and size class
    x = scene.Stream(spec.seed, 9).normal(n) * np.where(np.arange(n) % 3 == 0, 1e-3, 1.0)
    scale = np.abs(H) @ np.abs(x)
    assert np.all(np.abs(ne.JtJ(x).astype(np.float64) - H @ x) <= tol * scale)
    assert np.all(ne.JtJ(np.abs(x), absolute=True).astype(np.float64) >= scale * (1 - tol))   # |J|^T |J| >= |J^T J| entry by entry
    # the dense solution is a solution of the matrix-free system, and the reference step is as good as it, by the bound the kernels get
    eB_dense, eP_dense = ne.eta(delta)
    sw = sr.oracle_sweep(pa, radius)
    ref = sr.reference_step(ne, sw)
    eB, eP = ne.eta(ref)
    print(f"{spec.seed}: dense eta_B {eB_dense:.2e} eta_P {eP_dense:.2e} | reference step eta_B {eB:.2e} eta_P {eP:.2e} | floor {n * sr.EPS:.2e}")
    assert eB <= BOUND * max(eB_dense, n * sr.EPS) and eP <= BOUND * max(eP_dense, n * sr.EPS)
    # and the two steps agree where dense_system's own test compares them
    nb = ne.nb
    assert np.abs(ref[:nb].astype(np.float64) - delta[:nb]).max() <= 1e-7 * np.abs(delta[:nb]).max()


def test_dead_rows_are_counted_by_cause():
    """every class of dead column at once: absent camera slots (0x501: 11), fixed_mask (2), two constant frames (12), and a point
    that loses its observations (3); a row that left the maximum for any other reason would change the count"""
    sc = scene.make_scene(S(6, 30, None, 0xD01, 404, recalib=True))
    keep = sc.pt != 7
    from lifcal_amd import _capi as capi
    pa = capi.ProblemArrays(sc.u[keep], sc.v[keep], sc.mcx[keep], sc.mcy[keep], sc.pt[keep], sc.fr[keep], sc.cam0, sc.views0, sc.pts0, sc.spx, sc.scale,
                            sc.config, fixed_mask=sc.fixed_mask, use_constraints=0)
    fixed = np.zeros(6, bool); fixed[[1, 4]] = True
    ne = sr.NormalEquations(pa, 1e4, fixed_frames=fixed)
    assert ne.expected_dead() == 11 + 2 + 12 + 3
    assert ne.check_dead_rows() == 28
    e = ne.eta_rows(np.zeros(ne.n))
    assert int(np.sum(np.isnan(e))) == 28 and np.all(e[ne.live] == 1.0)   # delta = 0: y = g, every live row reads exactly 1
    # poses not refined: all pose and point blocks are dead
    pa2 = problem(scene.make_scene(S(6, 40, None, 0x006, 113)))
    ne2 = sr.NormalEquations(pa2, 1e4)
    assert ne2.check_dead_rows() == 8 + 36 + 120


@pytest.fixture(scope="module")
def windowed():
    sc = scene.make_scene(S(24, 120, 6, 0xF06, 6101))
    pa = problem(sc)
    ne = sr.NormalEquations(pa, 1e4)
    ne.check_dead_rows()
    return pa, ne


@pytest.mark.parametrize("radius", [1e4, 7.0])
def test_reference_step_stands_clear_of_a_1e9_block_error(windowed, radius):
    """A relative error of 1e-6 in one block raises eta to ~4e-7 (next test), linearly: one of 1e-9 gives ~4e-10.  The reference must
    stay below that for the GPU test to see such an error; a quarter of it is asked."""
    pa, ne = windowed
    ne.set_radius(radius)
    ref = sr.reference_step(ne, sr.oracle_sweep(pa, radius))
    eB, eP = ne.eta(ref)
    print(f"radius {radius:g}: reference eta_B {eB:.2e} eta_P {eP:.2e}")
    assert eB < 1e-10 and eP < 1e-10


@pytest.mark.parametrize("radius", [1e4, 7.0])
def test_one_wrong_block_raises_eta_a_hundredfold(windowed, radius):
    """the proof that the assertion on the kernels can fail: one pose block, or one point's step, scaled by 1 + 1e-6"""
    pa, ne = windowed
    ne.set_radius(radius)
    ref = sr.reference_step(ne, sr.oracle_sweep(pa, radius))
    eB0, eP0 = ne.eta(ref)
    pose = ref.copy(); pose[17 + 6 * 11:17 + 6 * 11 + 6] *= 1.0 + 1e-6
    eB1, eP1 = ne.eta(pose)
    point = ref.copy(); point[ne.nb + 3 * 57:ne.nb + 3 * 57 + 3] *= 1.0 + 1e-6
    eB2, eP2 = ne.eta(point)
    print(f"radius {radius:g}: eta_B / eta_P  unperturbed {eB0:.2e} / {eP0:.2e}  pose block {eB1:.2e} / {eP1:.2e}  point {eB2:.2e} / {eP2:.2e}")
    assert eB1 >= 100 * eB0 and eP1 >= 100 * eP0
    assert eP2 >= 100 * eP0 and eB2 >= 100 * eB0
    # row-wise: the perturbed blocks are where the measure points
    rows = ne.eta_rows(point)
    assert int(np.nanargmax(rows)) in range(ne.nb + 3 * 57, ne.nb + 3 * 57 + 3)


def test_solve_eta_skips_identity_rows_only_while_they_are_zero():
    S_ = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.0], [0.0, 0.0, 1.0]]); b = np.array([1.0, 2.0, 0.0])
    x = np.linalg.solve(S_, b)
    assert sr.solve_eta(S_, b, x) <= 4 * sr.EPS
    x2 = x.copy(); x2[1] *= 1 + 1e-6
    assert sr.solve_eta(S_, b, x2) > 1e-7
    assert sr.solve_eta(S_, b, np.array([x[0], x[1], 1e-3])) == 1.0   # a dead slot that moved is a row with nothing right, not a row to skip
