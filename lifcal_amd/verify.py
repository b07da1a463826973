"""Geometric verification of feature matches, over include/lifcal_verify.h: every feature of a plenoptic
camera is a metric point in its camera's frame, so the matches of a pair of frames of a rigid scene obey one rigid motion; a
batched RANSAC finds it and keeps the matches that agree with it.

The scoring of the hypotheses and the classification of the matches run inside liblifcal_ba.so on the GPU; there is no Python
or CPU fallback for them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError
from .depth import backProjectPoints
from .features import Matches, _check, _options

OPTION_NAMES = tuple(n for n, _ in capi.VerifyOptions._fields_)
STATUS_OK, STATUS_FEW, STATUS_DEGENERATE, STATUS_REJECTED = 0, 1, 2, 3
PAIR_DTYPE = np.dtype([("status", "<u4"), ("n_matches", "<u4"), ("n_usable", "<u4"), ("best_hypothesis", "<u4"), ("n_inliers_hypothesis", "<u4"),
                       ("n_inliers", "<u4"), ("rounds_used", "<u4"), ("reserved", "<u4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("rms", "<f8")])
_u64ptr = C.POINTER(C.c_uint64)


def make_verify_options(**options) -> capi.VerifyOptions:
    """lifcal_verify_options from keywords (hypotheses, seed, min_inliers, refine, min_ratio); what is not given takes the default"""
    return _options(capi.VerifyOptions, OPTION_NAMES, "verifyMatches", options)


@dataclass
class FeaturePoints:
    """Per feature of the concatenated list of some frames.  offset: (F + 1,) uint32; xyz: (N, 3) camera-frame coordinates in mm;
    tol_lat, tol_dep: (N,) tolerances across and along the viewing ray in mm.  A feature without a depth holds NaN."""
    offset: np.ndarray
    xyz: np.ndarray
    tol_lat: np.ndarray
    tol_dep: np.ndarray


@dataclass
class Verification:
    """keep: (n,) uint8 per match; e_par, e_perp: (n,) float64, the error of the match along and across the ray under its pair's
    motion (NaN where the match is not usable); pair: (P,) records of PAIR_DTYPE (lifcal_verify_pair); seconds: device time of
    the kernels."""
    keep: np.ndarray
    e_par: np.ndarray
    e_perp: np.ndarray
    pair: np.ndarray
    seconds: float = 0.0


def _arguments(points: FeaturePoints, matches: Matches):
    offset = np.ascontiguousarray(points.offset, np.uint32).reshape(-1)
    xyz = np.ascontiguousarray(points.xyz, np.float64).reshape(-1, 3)
    tol_lat = np.ascontiguousarray(points.tol_lat, np.float64).reshape(-1); tol_dep = np.ascontiguousarray(points.tol_dep, np.float64).reshape(-1)
    if len(offset) < 1 or not (len(xyz) == len(tol_lat) == len(tol_dep)) or len(xyz) < int(offset[-1]):
        raise LifcalError("verifyMatches: offset does not describe the point arrays")
    pairs = np.ascontiguousarray(matches.pairs, np.uint32).reshape(-1, 2)
    start = np.ascontiguousarray(matches.pair_start, np.uint64).reshape(-1)
    mi = np.ascontiguousarray(matches.i, np.uint32); mj = np.ascontiguousarray(matches.j, np.uint32)
    if len(start) != len(pairs) + 1 or len(mi) != len(mj) or int(start.max(initial=0)) > len(mi):
        raise LifcalError("verifyMatches: pair_start does not describe the match arrays")
    vp = capi.VerifyPoints(len(offset) - 1, 0, capi.as_uptr(offset), capi.as_dptr(xyz), capi.as_dptr(tol_lat), capi.as_dptr(tol_dep))
    return vp, pairs, start, mi, mj, (offset, xyz, tol_lat, tol_dep)


def checkVerify(points: FeaturePoints, matches: Matches, **options) -> capi.VerifyOptions:
    """lifcal_matches_verify_check: the argument checks of verifyMatches; returns the resolved options.  Needs no device."""
    vp, pairs, start, mi, mj, keep_alive = _arguments(points, matches)
    opt, res = make_verify_options(**options), capi.VerifyOptions()
    _check(capi.load_library().lifcal_matches_verify_check(C.byref(vp), len(pairs), capi.as_uptr(pairs), start.ctypes.data_as(_u64ptr), capi.as_uptr(mi),
                                                           capi.as_uptr(mj), C.byref(opt), C.byref(res)), "lifcal_matches_verify_check")
    del keep_alive
    return res


def verifyMatches(points: FeaturePoints, matches: Matches, device: int = 0, **options) -> Verification:
    """lifcal_matches_verify: per pair of frames the rigid motion that most matches obey, and per match whether it does."""
    vp, pairs, start, mi, mj, keep_alive = _arguments(points, matches)
    opt = make_verify_options(**options)
    n = int(start[-1]) if len(pairs) else 0
    keep = np.zeros(n, np.uint8); e_par = np.full(n, np.nan); e_perp = np.full(n, np.nan)
    rows = np.zeros(len(pairs), PAIR_DTYPE)
    res = capi.VerifyResult(keep.ctypes.data_as(C.POINTER(C.c_uint8)), capi.as_dptr(e_par), capi.as_dptr(e_perp),
                            C.cast(rows.ctypes.data, C.POINTER(capi.VerifyPair)), 0.0)
    _check(capi.load_library().lifcal_matches_verify(C.byref(vp), len(pairs), capi.as_uptr(pairs), start.ctypes.data_as(_u64ptr), capi.as_uptr(mi),
                                                     capi.as_uptr(mj), int(device), C.byref(opt), C.byref(res)), "lifcal_matches_verify")
    del keep_alive
    return Verification(keep, e_par, e_perp, rows, float(res.seconds))


def featurePoints(features, depth_maps, cam, config: int, spx: float, spy=None, tol_px: float = 1.0, tol_iv: float = 4.0 / 65535.0,
                  device: int = 0) -> FeaturePoints:
    """The metric point and the tolerances of every feature.  features: the Features of the frames; depth_maps: a DepthMaps whose
    map f is the virtual-depth map of frame f.  The virtual depth v is sampled at (x, y) (DepthMaps.sample) and back-projected
    (backProjectPoints).  tol_dep = |d p_c / d v| tol_iv v^2: tol_iv steps of inverse virtual depth; tol_lat = tol_px
    |p_c(x + 1, y, v) - p_c(x, y, v)|: tol_px pixels across the ray.  A feature whose sample failed gets NaN."""
    features = list(features)
    offset = np.zeros(len(features) + 1, np.uint32)
    offset[1:] = np.cumsum([f.n for f in features])
    x = np.concatenate([f.x for f in features]) if features else np.zeros(0)
    y = np.concatenate([f.y for f in features]) if features else np.zeros(0)
    fr = np.repeat(np.arange(len(features), dtype=np.int32), [f.n for f in features])
    n = len(x)
    if n == 0:
        return FeaturePoints(offset, np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    v, _ = depth_maps.sample(x, y, fr)
    good = np.isfinite(v) & (v > 0.0)
    xyz = np.full((n, 3), np.nan); tol_lat = np.full(n, np.nan); tol_dep = np.full(n, np.nan)
    if good.any():
        here = backProjectPoints(x[good], y[good], v[good], cam, config, spx, spy, want_jacobian=True, device=device)
        beside = backProjectPoints(x[good] + 1.0, y[good], v[good], cam, config, spx, spy, device=device)
        xyz[good] = here.p_c
        tol_dep[good] = np.linalg.norm(here.dpc_dv, axis=1) * float(tol_iv) * v[good] * v[good]
        tol_lat[good] = float(tol_px) * np.linalg.norm(beside.p_c - here.p_c, axis=1)
    return FeaturePoints(offset, xyz, tol_lat, tol_dep)
