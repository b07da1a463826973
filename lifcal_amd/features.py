"""Feature tracks from total-focus images, over include/lifcal_features.h: image points in every
total-focus image, their correspondences between frames, and the tracks (x, y, fr, pt) that DepthMaps.sample,
MicroLensGrid.projectPointsToRawImage, registerScene and BundleAdjustment take.

Detection and matching run inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for them.  The linker is host
code of the same library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError
from .raw_depth import _image

DETECT_OPTION_NAMES = tuple(n for n, _ in capi.FeaturesOptions._fields_)
MATCH_OPTION_NAMES = tuple(n for n, _ in capi.MatchOptions._fields_)
MORE = 1   # LIFCAL_MLA_MORE


def _check(rc: int, what: str):
    if rc < 0:
        lib = capi.load_library()
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc
        raise err


def _options(cls, names, who, options):
    o = cls()
    for k, v in options.items():
        if k not in names:
            raise TypeError(f"{who}: unknown option {k!r}")
        setattr(o, k, v)
    return o


def make_options(**options) -> capi.FeaturesOptions:
    """lifcal_features_options from keywords (win_r, nms_r, cell, per_cell, min_score); what is not given takes the default"""
    return _options(capi.FeaturesOptions, DETECT_OPTION_NAMES, "detectFeatures", options)


def make_match_options(**options) -> capi.MatchOptions:
    """lifcal_match_options from keywords (max_dist, ratio_num, ratio_den, max_shift)"""
    return _options(capi.MatchOptions, MATCH_OPTION_NAMES, "matchFeatures", options)


@dataclass
class Features:
    """The features of one image, buckets row-major and each bucket best first.  x, y: (n,) float64 sub-pixel positions (pixel
    centres at integers, the image points of the total-focus image); ix, iy: (n,) int32, the pixel of the maximum; score: (n,)
    float64; desc: (n, 8) uint32; seconds: device time of the kernels."""
    x: np.ndarray
    y: np.ndarray
    ix: np.ndarray
    iy: np.ndarray
    score: np.ndarray
    desc: np.ndarray
    seconds: float = 0.0

    @property
    def n(self) -> int:
        return len(self.x)


@dataclass
class Matches:
    """pairs: (P, 2) uint32 frames (a, b); pair_start: (P + 1,) uint64; i, j: indices within frame a and frame b; dist: Hamming
    distances.  Per pair ascending in i."""
    pairs: np.ndarray
    pair_start: np.ndarray
    i: np.ndarray
    j: np.ndarray
    dist: np.ndarray
    seconds: float = 0.0

    def of_pair(self, p: int):
        s = slice(int(self.pair_start[p]), int(self.pair_start[p + 1]))
        return self.i[s], self.j[s], self.dist[s]

    def filtered(self, keep) -> "Matches":
        """the matches with a true `keep` (one entry per match, Verification.keep as it is), pair_start recomputed; linkTracks
        takes the result as it takes this"""
        keep = np.asarray(keep).astype(bool).reshape(-1)
        if len(keep) != len(self.i):
            raise ValueError("Matches.filtered: one entry per match")
        start = np.asarray(self.pair_start, np.int64)
        kept = np.concatenate([[0], np.cumsum(keep)])
        return Matches(self.pairs, kept[start].astype(np.uint64), self.i[keep], self.j[keep], self.dist[keep], self.seconds)


@dataclass
class Tracks:
    """The observations of the tracks, by frame and then feature index.  fr, pt: (n,) uint32; feature: (n,) uint32 index into the
    concatenated features; x, y: (n,) float64 positions of those features."""
    fr: np.ndarray
    pt: np.ndarray
    feature: np.ndarray
    x: np.ndarray
    y: np.ndarray
    n_tracks: int
    n_conflicts: int

    def image_points(self):
        """x, y, fr, pt as MicroLensGrid.projectPointsToRawImage(x, y, vdepth, scale, fr=fr, pt=pt) takes them"""
        return self.x, self.y, self.fr, self.pt


def checkFeatures(image_shape, bits: int, **options) -> capi.FeaturesPlan:
    """lifcal_features_check: the argument checks of detectFeatures for an image of image_shape = (height, width); needs no device"""
    lib = capi.load_library()
    stand_in = np.zeros(1, np.uint16)
    img = capi.RawDepthImage(stand_in.ctypes.data, int(bits), int(image_shape[1]), int(image_shape[0]), 0, int(image_shape[1]))
    plan = capi.FeaturesPlan()
    opt = make_options(**options)
    _check(lib.lifcal_features_check(C.byref(img), C.byref(opt), C.byref(plan)), "lifcal_features_check")
    return plan


def pattern() -> np.ndarray:
    """the descriptor's 256 point pairs as (256, 4) int8: ax, ay, bx, by"""
    out = np.zeros((256, 4), np.int8)
    _check(capi.load_library().lifcal_features_pattern(out.ctypes.data_as(C.POINTER(C.c_int8))), "lifcal_features_pattern")
    return out


def detectFeatures(image, status=None, device: int = 0, **options) -> Features:
    """lifcal_features_detect.  image: (H, W) uint8 / uint16, a numpy array (rows may be strided) or a torch tensor on `device`;
    status: None or (H, W) uint8 of the same kind, contiguous (TotalFocusImage.status as it is)."""
    lib = capi.load_library()
    img, keep = _image(image)
    opt = make_options(**options)
    plan = capi.FeaturesPlan()
    _check(lib.lifcal_features_check(C.byref(img), C.byref(opt), C.byref(plan)), "lifcal_features_check")
    shape = (int(img.height), int(img.width))
    ptr_st, keep_st = None, None
    if status is not None:
        if tuple(status.shape) != shape:
            raise ValueError("status: the image's shape")
        if hasattr(status, "data_ptr"):
            import torch
            if not img.on_device or status.dtype != torch.uint8 or not status.is_cuda or not status.is_contiguous():
                raise ValueError("status: a contiguous uint8 tensor on the device, like the image")
            torch.cuda.synchronize(status.device)
            keep_st = status
            ptr_st = status.data_ptr()
        else:
            if img.on_device:
                raise ValueError("status: a tensor on the device, like the image")
            keep_st = np.ascontiguousarray(status, np.uint8)
            ptr_st = keep_st.ctypes.data
    cap = int(plan.max_features)
    x = np.zeros(cap); y = np.zeros(cap); score = np.zeros(cap)
    ix = np.zeros(cap, np.int32); iy = np.zeros(cap, np.int32); desc = np.zeros((cap, 8), np.uint32)
    lst = capi.FeaturesList(cap, 0, capi.as_dptr(x), capi.as_dptr(y), ix.ctypes.data_as(capi._iptr), iy.ctypes.data_as(capi._iptr), capi.as_dptr(score),
                            capi.as_uptr(desc), 0.0)
    _check(lib.lifcal_features_detect(C.byref(img), ptr_st, int(device), C.byref(opt), C.byref(lst)), "lifcal_features_detect")
    del keep, keep_st
    n = int(lst.n)
    return Features(x[:n].copy(), y[:n].copy(), ix[:n].copy(), iy[:n].copy(), score[:n].copy(), desc[:n].copy(), float(lst.seconds))


def _concatenate(features):
    offset = np.zeros(len(features) + 1, np.uint32)
    offset[1:] = np.cumsum([f.n for f in features])
    cat = lambda name, dtype, tail=(): (np.ascontiguousarray(np.concatenate([getattr(f, name) for f in features]), dtype) if len(features)
                                        else np.zeros((0,) + tail, dtype))
    return offset, cat("desc", np.uint32, (8,)).reshape(-1, 8), cat("ix", np.int32), cat("iy", np.int32)


def sequence_pairs(n_frames: int, window: int = 2) -> np.ndarray:
    """every frame with the next `window` frames"""
    return np.array([(a, b) for a in range(n_frames) for b in range(a + 1, min(n_frames, a + 1 + int(window)))], np.uint32).reshape(-1, 2)


def matchFeatures(features, pairs=None, window: int = 2, device: int = 0, **options) -> Matches:
    """lifcal_features_match on the Features of some frames.  pairs: (P, 2) frames (a, b); None: sequence_pairs(len(features),
    window)."""
    lib = capi.load_library()
    features = list(features)
    pairs = sequence_pairs(len(features), window) if pairs is None else np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    offset, desc, ix, iy = _concatenate(features)
    fs = capi.FeaturesSet(len(features), 0, capi.as_uptr(offset), capi.as_uptr(desc), ix.ctypes.data_as(capi._iptr), iy.ctypes.data_as(capi._iptr))
    opt = make_match_options(**options)
    P = len(pairs)
    start = np.zeros(P + 1, np.uint64)
    cap = 0
    while True:
        mi = np.zeros(cap, np.uint32); mj = np.zeros(cap, np.uint32); md = np.zeros(cap, np.uint32)
        lst = capi.MatchList(cap, 0, start.ctypes.data_as(C.POINTER(C.c_uint64)), capi.as_uptr(mi), capi.as_uptr(mj), capi.as_uptr(md), 0.0)
        rc = lib.lifcal_features_match(C.byref(fs), P, capi.as_uptr(pairs), int(device), C.byref(opt), C.byref(lst))
        _check(rc, "lifcal_features_match")
        if rc != MORE:
            break
        cap = int(lst.n)   # count, then fill
    n = int(lst.n)
    return Matches(pairs, start, mi[:n], mj[:n], md[:n], float(lst.seconds))


def linkTracks(features, matches: Matches, min_length: int = 2) -> Tracks:
    """lifcal_tracks_link: the tracks of the matches.  Host only."""
    lib = capi.load_library()
    features = list(features)
    offset = np.zeros(len(features) + 1, np.uint32)
    offset[1:] = np.cumsum([f.n for f in features])
    pairs = np.ascontiguousarray(matches.pairs, np.uint32).reshape(-1, 2)
    start = np.ascontiguousarray(matches.pair_start, np.uint64)
    mi = np.ascontiguousarray(matches.i, np.uint32); mj = np.ascontiguousarray(matches.j, np.uint32)
    if len(start) != len(pairs) + 1 or len(mi) != len(mj) or (len(start) and int(start[-1]) > len(mi)):
        raise LifcalError("linkTracks: pair_start does not describe the match arrays")
    cap = 0
    while True:
        fr = np.zeros(cap, np.uint32); pt = np.zeros(cap, np.uint32); ft = np.zeros(cap, np.uint32)
        t = capi.Tracks(int(min_length), 0, 0, cap, 0, capi.as_uptr(fr), capi.as_uptr(pt), capi.as_uptr(ft))
        rc = lib.lifcal_tracks_link(len(features), capi.as_uptr(offset), len(pairs), capi.as_uptr(pairs), start.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    capi.as_uptr(mi), capi.as_uptr(mj), C.byref(t))
        _check(rc, "lifcal_tracks_link")
        if rc != MORE:
            break
        cap = int(t.n)
    x = np.concatenate([f.x for f in features]) if features else np.zeros(0)
    y = np.concatenate([f.y for f in features]) if features else np.zeros(0)
    return Tracks(fr, pt, ft, x[ft], y[ft], int(t.n_tracks), int(t.n_conflicts))


def trackSequence(images, statuses=None, window: int = 2, min_length: int = 2, device: int = 0, detect=None, match=None, verify=None):
    """detectFeatures on every image (with its status map when statuses is given), matchFeatures over every frame and the next
    `window`, linkTracks.  detect, match: dicts of options.  Returns (features, matches, tracks).

    verify: None, or a dict that asks for the geometric verification of the matches (lifcal_amd.verify) before they are linked.
    It holds either `points`, a callable that takes the features and returns their FeaturePoints (or the FeaturePoints
    themselves), or the arguments of featurePoints after `features` (depth_maps, cam, config, spx, ...); `options`: a dict of
    verifyMatches options.  Then the tracks are those of the kept matches and the return value is (features, matches, tracks,
    verification), with `matches` still the unfiltered ones (matches.filtered(verification.keep) are the linked ones)."""
    images = list(images)
    statuses = [None] * len(images) if statuses is None else list(statuses)
    if len(statuses) != len(images):
        raise ValueError("trackSequence: one status map per image, or none")
    feats = [detectFeatures(im, st, device=device, **(detect or {})) for im, st in zip(images, statuses)]
    m = matchFeatures(feats, window=window, device=device, **(match or {}))
    if verify is None:
        return feats, m, linkTracks(feats, m, min_length)
    from . import verify as _verify
    args = dict(verify)
    options = args.pop("options", None) or {}
    if "points" in args:
        points = args.pop("points")
        if args:
            raise TypeError(f"trackSequence: verify holds `points` and also {sorted(args)}")
        points = points(feats) if callable(points) else points
    else:
        points = _verify.featurePoints(feats, device=device, **args)
    v = _verify.verifyMatches(points, m, device=device, **options)
    return feats, m, linkTracks(feats, m.filtered(v.keep), min_length), v
