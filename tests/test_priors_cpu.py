"""Gaussian priors without a GPU (include/lifcal_prior.h): exported symbols and struct layout, every rejection of
lifcal_ba_check_priors, lifcal_prior_from_covariance against numpy's pinv, and the reference helpers of tests/prior_reference.py
against the oracle's sweep."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import lifcal_amd
from lifcal_amd import LifcalError, _capi as capi, scene
from tests import prior_reference as pr
from tests.helpers import problem, scaled_max_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = -1, -4


def spd(rng, n, scale=1.0):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T + 0.1 * np.eye(n))


def test_symbols_prototypes_and_layout(built):
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "lifcal_prior.h")).read()
    declared = set(re.findall(r"\b(lifcal_(?:ba_)?[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(capi.PRIOR_PROTOTYPES), declared ^ set(capi.PRIOR_PROTOTYPES)
    assert not (declared & set(capi.PROTOTYPES))
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/lifcal_prior.h but not exported"
    # LP64: two pointers, two uint32, three pointers
    assert C.sizeof(capi.Priors) == 48
    fields = re.search(r"typedef struct lifcal_ba_priors \{(.*?)\} lifcal_ba_priors;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in capi.Priors._fields_], names
    assert (capi.Priors.n_pose_priors.offset, capi.Priors.pose_frame.offset, capi.Priors.pose_info.offset) == (16, 24, 40)
    for name in ("check_priors", "prior_from_covariance"):
        assert hasattr(lifcal_amd, name)
    for name in ("set_priors", "clear_priors", "prior_cost"):
        assert hasattr(lifcal_amd.BundleAdjustment, name)
    assert hasattr(lifcal_amd.Covariance, "camera_information") and hasattr(lifcal_amd.ResectionResult, "pose_information")


def good_priors(rng, n=3):
    cam = (rng.normal(size=17), spd(rng, 17))
    poses = (np.array([0, 2, 5])[:n], rng.normal(size=(n, 6)), np.array([spd(rng, 6) for _ in range(n)]))
    return cam, poses


def rejected(code, n_frames, camera=None, poses=None):
    with pytest.raises(LifcalError) as e:
        lifcal_amd.check_priors(n_frames, camera, poses)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_check_priors_accepts_sound_priors(built):
    rng = np.random.default_rng(1)
    cam, poses = good_priors(rng)
    lifcal_amd.check_priors(6, cam, poses)
    lifcal_amd.check_priors(6, cam, None)
    lifcal_amd.check_priors(6, None, poses)
    lifcal_amd.check_priors(6)                                   # no prior at all
    lifcal_amd.check_priors(6, (cam[0], np.zeros((17, 17))))     # a zero matrix is positive semi-definite
    semi = np.zeros((17, 17)); semi[2, 2] = 4.0                  # rank one
    lifcal_amd.check_priors(6, (cam[0], semi))
    # asymmetric inside the tolerance 1e-12 sqrt(a_ii a_jj)
    A = cam[1].copy(); A[3, 7] += 0.5e-12 * np.sqrt(A[3, 3] * A[7, 7])
    lifcal_amd.check_priors(6, (cam[0], A))


def test_check_priors_null_pointer_where_a_count_says_otherwise(built):
    lib = capi.load_library()
    p = capi.Priors(); p.n_pose_priors = 2
    assert lib.lifcal_ba_check_priors(6, C.byref(p)) == INVALID_ARG
    assert lib.lifcal_ba_check_priors(6, None) == INVALID_ARG
    rng = np.random.default_rng(2)
    arrs = capi.PriorArrays(*good_priors(rng))
    arrs.struct.cam_info = None                                  # a mean without its matrix
    assert lib.lifcal_ba_check_priors(6, C.byref(arrs.struct)) == INVALID_ARG
    arrs = capi.PriorArrays(*good_priors(rng))
    arrs.struct.pose_mean = None
    assert lib.lifcal_ba_check_priors(6, C.byref(arrs.struct)) == INVALID_ARG


def test_check_priors_non_finite_entry(built):
    rng = np.random.default_rng(3)
    cam, poses = good_priors(rng)
    A = cam[1].copy(); A[4, 4] = np.nan
    assert "finite" in rejected(INVALID_ARG, 6, (cam[0], A))
    m = cam[0].copy(); m[1] = np.inf
    assert "finite" in rejected(INVALID_ARG, 6, (m, cam[1]))
    I = poses[2].copy(); I[1, 2, 3] = I[1, 3, 2] = np.inf
    assert "finite" in rejected(INVALID_ARG, 6, None, (poses[0], poses[1], I))
    pm = poses[1].copy(); pm[2, 5] = np.nan
    assert "finite" in rejected(INVALID_ARG, 6, None, (poses[0], pm, poses[2]))


def test_check_priors_asymmetric_matrix(built):
    rng = np.random.default_rng(4)
    cam, poses = good_priors(rng)
    A = cam[1].copy(); A[3, 7] += 4e-12 * np.sqrt(A[3, 3] * A[7, 7])
    assert "symmetric" in rejected(INVALID_ARG, 6, (cam[0], A))
    I = poses[2].copy(); I[0, 0, 1] += 1e-6
    assert "symmetric" in rejected(INVALID_ARG, 6, None, (poses[0], poses[1], I))


def test_check_priors_negative_diagonal(built):
    rng = np.random.default_rng(5)
    cam, _ = good_priors(rng)
    A = np.diag(np.ones(17)); A[6, 6] = -1e-3
    assert "diagonal" in rejected(INVALID_ARG, 6, (cam[0], A))


def test_check_priors_negative_eigenvalue(built):
    rng = np.random.default_rng(6)
    cam, poses = good_priors(rng)
    A = np.eye(17); A[0, 1] = A[1, 0] = 1.0 + 1e-6                # eigenvalue -1e-6 with a positive diagonal
    assert "semi-definite" in rejected(INVALID_ARG, 6, (cam[0], A))
    I = poses[2].copy(); I[2] = np.eye(6); I[2, 4, 5] = I[2, 5, 4] = 2.0
    assert "semi-definite" in rejected(INVALID_ARG, 6, None, (poses[0], poses[1], I))
    # an eigenvalue of -1e-13 lambda_max is rounding, not a defect
    w = np.ones(17); w[0] = -1e-13
    Q, _ = np.linalg.qr(rng.normal(size=(17, 17)))
    B = (Q * w) @ Q.T
    B = 0.5 * (B + B.T)
    assert np.all(np.diag(B) >= 0)
    lifcal_amd.check_priors(6, (cam[0], B))


def test_check_priors_frames(built):
    rng = np.random.default_rng(7)
    _, poses = good_priors(rng)
    assert "ascending" in rejected(INVALID_ARG, 6, None, (np.array([0, 5, 2]), poses[1], poses[2]))
    assert "ascending" in rejected(INVALID_ARG, 6, None, (np.array([0, 2, 2]), poses[1], poses[2]))
    rejected(OUT_OF_RANGE, 5, None, poses)                       # frame 5 of 5
    lifcal_amd.check_priors(6, None, poses)


def pinv_bar(A):
    """relative error in the Frobenius norm of numpy's own pinv(pinv(A)) round trip, times 10"""
    back = np.linalg.pinv(np.linalg.pinv(A))
    return 10.0 * np.linalg.norm(back - A) / np.linalg.norm(A)


def test_prior_from_covariance_full_rank(built):
    rng = np.random.default_rng(8)
    A = spd(rng, 17)
    mask = 0x1FFFF & ~((1 << 4) | (1 << 11))
    sel = [i for i in range(17) if (mask >> i) & 1]
    info, rank = lifcal_amd.prior_from_covariance(A, mask)
    ref = np.linalg.pinv(A[np.ix_(sel, sel)])
    err = np.linalg.norm(info[np.ix_(sel, sel)] - ref) / np.linalg.norm(ref)
    bar = pinv_bar(A[np.ix_(sel, sel)])
    print(f"full rank: relative error {err:.3e}  bar {bar:.3e}")
    assert rank == len(sel)
    assert err <= bar
    out = np.ones((17, 17), bool); out[np.ix_(sel, sel)] = False
    assert np.all(info[out] == 0.0) and np.array_equal(info, info.T)


def test_prior_from_covariance_rank_deficient(built):
    rng = np.random.default_rng(9)
    G = rng.normal(size=(17, 12))
    A = G @ G.T                                                    # rank 12
    info, rank = lifcal_amd.prior_from_covariance(A, 0x1FFFF)
    ref = np.linalg.pinv(A)
    err = np.linalg.norm(info - ref) / np.linalg.norm(ref)
    bar = pinv_bar(A)
    print(f"rank deficient: rank {rank}  relative error {err:.3e}  bar {bar:.3e}")
    assert rank == 12 == np.linalg.matrix_rank(A)
    assert err <= bar


def test_prior_from_covariance_empty_mask_and_arguments(built):
    rng = np.random.default_rng(10)
    A = spd(rng, 6)
    info, rank = lifcal_amd.prior_from_covariance(A, 0)
    assert rank == 0 and np.all(info == 0.0)
    info, rank = lifcal_amd.prior_from_covariance(A, 0x3F)
    assert rank == 6
    lib = capi.load_library()
    out = np.zeros((6, 6))
    assert lib.lifcal_prior_from_covariance(None, 6, 0x3F, 1e-9, capi.as_dptr(out), None) == INVALID_ARG
    assert lib.lifcal_prior_from_covariance(capi.as_dptr(A), 6, 0x3F, 1e-9, capi.as_dptr(out), None) == 0   # rank may be NULL
    assert np.array_equal(out, info)


def test_set_priors_needs_a_handle(built):
    lib = capi.load_library()
    assert lib.lifcal_ba_set_priors(None, None) == INVALID_ARG
    assert lib.lifcal_ba_prior_cost(None, None, None) == INVALID_ARG


def test_augmented_equations_against_the_oracle_sweep(built):
    """on `tiny` at the oracle's parameters: S and rhs of the equations with the prior rows appended = the oracle's S + embed(Lambda)
    and rhs - Lambda d, to the sweep bars of DESIGN.md section 2 (1e-9 block-scaled); the undamped radius, where Lambda does not
    move the LM diagonal"""
    sc = scene.make_scene(scene.baseline_spec("tiny"))
    pa = problem(sc)
    oracle.solve(pa, threads=oracle.hardware_threads())
    rng = np.random.default_rng(11)
    F = pa.struct.n_frames
    d = np.concatenate([np.abs(pa.cam[:9]) + 1e-3, np.ones(8)])
    cam = (pa.cam + 1e-3 * d * rng.normal(size=17), spd(rng, 17) / np.outer(d, d))
    poses = (np.array([0, 3, F - 1]), pa.views.reshape(F, 6)[[0, 3, F - 1]] + 1e-3 * rng.normal(size=(3, 6)), np.array([spd(rng, 6, 50.0) for _ in range(3)]))
    Lam, mean = pr.embed(F, 0, cam, poses)
    radius = 1e30
    o = capi.default_options_py()
    sw = oracle.sweep(pa, radius=radius, options=o, threads=oracle.hardware_threads())
    live = pr.live_slots(sc.config, sc.fixed_mask, F)
    assert not np.all(live[:17]) and np.all(live[17:])            # nine structural slots, every pose free
    cost_p, Ld = pr.prior_terms(Lam, mean, np.concatenate([pa.cam, pa.views]), live)
    ne = pr.PriorEquations(pa, radius, Lam, mean)
    S, rhs = pr.dense_reduced(ne)
    ref_S = sw.S + pr.masked(Lam, live)
    err_S = scaled_max_err(S, ref_S)
    dg = np.sqrt(np.abs(np.diag(ref_S)))
    err_rhs = float(np.max(np.abs(rhs - (sw.rhs - Ld)) / dg) / np.max(np.abs(sw.rhs - Ld) / dg))
    print(f"S {err_S:.3e}  rhs {err_rhs:.3e}  cost {ne.cost:.12e} = {sw.cost:.12e} + {cost_p:.6e}")
    assert err_S <= 1e-9 and err_rhs <= 1e-9
    assert abs(ne.cost - (sw.cost + cost_p)) <= 1e-12 * ne.cost
    assert abs(ne.cost_prior - cost_p) <= 1e-12 * cost_p and cost_p > 0
    # the prior-free equations of the same helper reproduce the oracle's S as they stand: the comparison above measures the prior
    S0, _ = pr.dense_reduced(pr.sr.NormalEquations(pa, radius))
    assert scaled_max_err(S0, sw.S) <= 1e-9
