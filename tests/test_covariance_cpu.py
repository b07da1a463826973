"""Covariance of the parameters without a GPU: the C ABI additions (symbols, struct layout, defaults, argument checks) and the dense
reference algebra of tests/cov_reference.py on the ORACLE's undamped reduced matrix at the oracle's solution."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from lifcal_amd import _capi as capi, scene
from tests import cov_reference as cr
from tests.helpers import SMALL_CASES, problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dict(SMALL_CASES)


def test_covariance_symbols_are_exported(built):
    lib = capi.load_library()
    for name in ("lifcal_ba_covariance", "lifcal_ba_default_covariance_options"):
        assert hasattr(lib, name) and name in capi.PROTOTYPES


def test_covariance_defaults_and_argument_checks(built):
    lib = capi.load_library()
    o = capi.CovarianceOptions()
    lib.lifcal_ba_default_covariance_options(C.byref(o))
    assert (o.gauge_frame, o.want_pose_blocks, o.scale_by_residual_variance) == (-1, 1, 0)
    assert o.null_rcond == 1e-9 and o.estimable_tol == 1e-3
    out = capi.CovarianceOut()
    assert lib.lifcal_ba_covariance(None, C.byref(o), C.byref(out)) == -1
    assert lib.lifcal_ba_last_error()


_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "lifcal_ba.h"
#define F(T, m) printf("%s %s %zu\n", #T, #m, offsetof(T, m))
int main(void) {
  F(lifcal_ba_covariance_options, gauge_frame); F(lifcal_ba_covariance_options, want_pose_blocks);
  F(lifcal_ba_covariance_options, scale_by_residual_variance); F(lifcal_ba_covariance_options, reserved);
  F(lifcal_ba_covariance_options, null_rcond); F(lifcal_ba_covariance_options, estimable_tol);
  F(lifcal_ba_covariance_out, camera); F(lifcal_ba_covariance_out, pose); F(lifcal_ba_covariance_out, pose_band);
  F(lifcal_ba_covariance_out, camera_null); F(lifcal_ba_covariance_out, estimable_mask); F(lifcal_ba_covariance_out, null_rank);
  F(lifcal_ba_covariance_out, gauge_frame_used); F(lifcal_ba_covariance_out, live_mask); F(lifcal_ba_covariance_out, sigma2);
  F(lifcal_ba_covariance_out, cost); F(lifcal_ba_covariance_out, seconds);
  printf("lifcal_ba_covariance_options sizeof %zu\n", sizeof(lifcal_ba_covariance_options));
  printf("lifcal_ba_covariance_out sizeof %zu\n", sizeof(lifcal_ba_covariance_out));
  return 0;
}
"""


def test_covariance_structs_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        # no C compiler: the sizes alone, from the field list of the header
        assert C.sizeof(capi.CovarianceOptions) == 4 * 4 + 2 * 8
        assert C.sizeof(capi.CovarianceOut) == 4 * 8 + 4 * 4 + 3 * 8
        return
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().split("\n"):
        if line:
            t, m, v = line.split()
            got[(t, m)] = int(v)
    for ctype, cname in ((capi.CovarianceOptions, "lifcal_ba_covariance_options"), (capi.CovarianceOut, "lifcal_ba_covariance_out")):
        assert C.sizeof(ctype) == got[(cname, "sizeof")]
        for field, _ in ctype._fields_:
            assert getattr(ctype, field).offset == got[(cname, field)], (cname, field)


def oracle_system(name, spec=None):
    """the oracle's undamped, unscaled reduced matrix at the oracle's solution, with its live mask"""
    sc = scene.make_scene(spec if spec is not None else CASES[name])
    pa = problem(sc)
    oracle.solve(pa, threads=oracle.hardware_threads())
    o = capi.default_options_py()
    o.jacobi_scaling = 0
    sw = oracle.sweep(pa, radius=1e30, options=o, threads=oracle.hardware_threads())
    F = pa.struct.n_frames
    used = np.bincount(sc.fr, minlength=F) > 0
    live = cr.live_mask(sc.config, sc.fixed_mask, F, sw.n_promoted, frame_used=used)
    full = bool(sc.config & 0x100) and bool(sc.config & 0x400)
    return sc, pa, sw, live, F, (cr.first_observed_frame(sc.fr) if full else -1)


# (case, null rank of C after the gauge frame, null directions of the full H): measured spectra — the null eigenvalues of the
# scaled C lie at <= 1e-11 of the largest, the smallest kept ones at >= 4e-7 (the constraint cases): null_rcond = 1e-9 sits in the gap
EXPECTED = [("r2_tan_full", 1, 7), ("r2_adj_robust", 1, 7), ("constraints", 0, 6), ("recalib", 0, 6), ("poses_only", 0, 0),
            ("camera_only", 0, 0), ("windowed", 1, 7)]


@pytest.mark.parametrize("name,null_c,null_h", EXPECTED)
def test_reference_algebra_on_the_oracle_matrix(built, name, null_c, null_h):
    sc, pa, sw, live, F, gauge = oracle_system(name)
    H = sw.S
    ref = cr.covariance(H, live, F, gauge, null_rcond=1e-9)
    l = np.flatnonzero(live)
    Hl = H[np.ix_(l, l)]
    Gl = ref.G[np.ix_(l, l)]
    d = np.sqrt(np.abs(np.diag(Hl)))
    # (1) G is a g-inverse of H: H G H = H, block-scaled, to round-off (measured <= 3e-9 on these cases)
    err = np.abs(Hl @ Gl @ Hl - Hl) / np.outer(d, d)
    assert err.max() < 1e-7, err.max()
    # (2) estimable camera variances are those of the Moore-Penrose inverse (any g-inverse gives them).  Bar 1e-6 relative, measured
    # <= 1.2e-7: the null direction of C is known to ~1e-7 only (an eigenvalue at C's cancellation floor, 1e-12 of the largest, against
    # a gap of ~5e-6), and a slot whose null component sits at that floor (fL of r2_tan_full: 5e-8) inherits an error of that order
    ds = np.sqrt(np.abs(np.diag(Hl)))
    Hp = np.linalg.pinv(Hl / np.outer(ds, ds), rcond=1e-9, hermitian=True) / np.outer(ds, ds)
    cam_l = [k for k, j in enumerate(l) if j < 17]
    cam_j = [j for j in l if j < 17]
    for k, j in zip(cam_l, cam_j):
        if ref.estimable[j]:
            assert abs(Gl[k, k] - Hp[k, k]) <= 1e-6 * Hp[k, k], (j, Gl[k, k], Hp[k, k])
    # (3) null rank of C + the six rigid directions the gauge frame removes = null directions of the scaled full H
    n_h, w = cr.scaled_null_count(H, live, 1e-9)
    assert ref.null_rank == null_c, ref.eig[:4]
    assert n_h == null_h, w[:10]
    assert ref.null_rank + (6 if gauge >= 0 else 0) == n_h
    # the undetermined direction of the unconstrained full arity lies in B and bL0: those two slots are not estimable, cx / cy are
    if null_c:
        assert not ref.estimable[1] and not ref.estimable[2] and ref.estimable[3] and ref.estimable[4]
    else:
        assert np.all(ref.estimable[live[:17]])


def test_gauge_frame_choice_leaves_estimable_entries(built):
    sc, pa, sw, live, F, gauge = oracle_system("r2_tan_full")
    a = cr.covariance(sw.S, live, F, 0, null_rcond=1e-9)
    b = cr.covariance(sw.S, live, F, F // 2, null_rcond=1e-9)
    e = np.flatnonzero(a.estimable)
    assert np.array_equal(a.estimable, b.estimable) and a.null_rank == b.null_rank == 1
    ce, cb = a.camera[np.ix_(e, e)], b.camera[np.ix_(e, e)]
    # (measured 4.9e-7: the same floor as above, through two different Schur complements)
    assert np.max(np.abs(ce - cb) / np.sqrt(np.outer(np.diag(ce), np.diag(ce)))) < 5e-6
    assert np.all(a.poses[0] == 0) and np.all(b.poses[F // 2] == 0) and np.abs(a.poses[F // 2]).max() > 0
