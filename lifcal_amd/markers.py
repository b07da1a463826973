"""Fiducial markers in total-focus images, over include/lifcal_markers.h: square binary markers of a
caller's dictionary are detected, decoded and centred on the GPU; a marker's id then serves as a point id and its centre as an
image point, which is what the distance constraints and control points of BundleAdjustment need (the reference's
doCalibration_aruco_calib).  With it the host pieces of that mode: the constraints file, start values for the marker points and
the scale of the scene from the first constraint.

Detection runs inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .bundle_adjustment import Alignment, LifcalError, alignApply
from .features import Tracks, _check, _options
from .raw_depth import _image

OPTION_NAMES = tuple(n for n, _ in capi.MarkersOptions._fields_)
MORE = 1   # LIFCAL_MLA_MORE
NO_FEATURE = 0xffffffff   # Tracks.feature of a marker observation
FIRST_CAPACITY = 1024     # entries the first call offers; count-then-fill only beyond that
_u64p = C.POINTER(C.c_uint64)


def make_options(**options) -> capi.MarkersOptions:
    """lifcal_markers_options from keywords (w, contrast, cell_contrast, min_area, min_side, max_side, max_border_errors,
    max_correction, refine_max); what is not given takes the default"""
    return _options(capi.MarkersOptions, OPTION_NAMES, "detectMarkers", options)


class Dictionary:
    """A marker dictionary: marker_bits (3 .. 7) and n words of marker_bits^2 bits, bit r * marker_bits + c = cell (r, c), 1 =
    white.  The reference's indexDictionary names one of OpenCV's predefined tables; those are not part of this package and have
    to be brought in through from_bits."""

    def __init__(self, marker_bits: int, words):
        self.marker_bits = int(marker_bits)
        self.words = np.ascontiguousarray(np.asarray(words, np.uint64).reshape(-1))
        self.min_distance = self._distance()

    def _struct(self) -> capi.MarkerDictionary:
        return capi.MarkerDictionary(self.marker_bits, len(self.words), self.words.ctypes.data_as(_u64p))

    def _distance(self) -> int:
        d = C.c_int32(0)
        s = self._struct()
        _check(capi.load_library().lifcal_marker_dictionary_distance(C.byref(s), C.byref(d)), "lifcal_marker_dictionary_distance")
        return int(d.value)

    @property
    def n(self) -> int:
        return len(self.words)

    @classmethod
    def generate(cls, marker_bits: int, n: int, seed: int = 1) -> "Dictionary":
        """lifcal_marker_dictionary_generate: n words drawn deterministically, as far apart as the draw allows"""
        out = np.zeros(max(int(n), 0), np.uint64)
        _check(capi.load_library().lifcal_marker_dictionary_generate(int(marker_bits), int(n), int(seed), out.ctypes.data_as(_u64p), None),
               "lifcal_marker_dictionary_generate")
        return cls(marker_bits, out)

    @classmethod
    def from_bits(cls, bits) -> "Dictionary":
        """bits: (n, m, m) array of 0 / 1, bits[j, r, c] = cell (r, c) of marker j (1 = white)"""
        b = np.asarray(bits)
        if b.ndim != 3 or b.shape[1] != b.shape[2]:
            raise ValueError("Dictionary.from_bits: an (n, m, m) array")
        m = b.shape[1]
        weights = (np.uint64(1) << np.arange(m * m, dtype=np.uint64))
        words = ((b.reshape(len(b), -1) != 0).astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)
        return cls(m, words)

    def bits(self) -> np.ndarray:
        """(n, m, m) uint8, the inverse of from_bits"""
        m = self.marker_bits
        k = np.arange(m * m, dtype=np.uint64)
        return ((self.words[:, None] >> k[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1, m, m)


@dataclass
class Markers:
    """The markers of one image by ascending label.  id, rotation, hamming, refined, label, area: (n,) int32; corners: (n, 4, 2)
    float64, corner 0 the marker's own top-left, clockwise, as (x, y); x, y: (n,) float64 centres (pixel centres at integers)."""
    id: np.ndarray
    rotation: np.ndarray
    hamming: np.ndarray
    refined: np.ndarray
    label: np.ndarray
    area: np.ndarray
    corners: np.ndarray
    x: np.ndarray
    y: np.ndarray
    n_candidates: int = 0
    seconds: float = 0.0

    @property
    def n(self) -> int:
        return len(self.id)

    def take(self, keep) -> "Markers":
        return Markers(self.id[keep], self.rotation[keep], self.hamming[keep], self.refined[keep], self.label[keep], self.area[keep], self.corners[keep],
                       self.x[keep], self.y[keep], self.n_candidates, self.seconds)

    def unique(self, warn: bool = True) -> "Markers":
        """the reference's rule: of an id found more than once the first is kept, with a warning"""
        _, first = np.unique(self.id, return_index=True)
        if len(first) != self.n and warn:
            twice = sorted(set(int(i) for i in self.id[np.setdiff1d(np.arange(self.n), first)]))
            warnings.warn(f"detectMarkers: marker ids {twice} were found more than once; the first of each is kept")
        return self.take(np.sort(first))


@dataclass
class MarkerComponents:
    """markerComponents: dark (H, W) uint8, labels (H, W) int32 (-1: not dark) and the candidate table as a record array
    (label, area, x0, y0, x1, y1, ext[8][2])"""
    dark: np.ndarray
    labels: np.ndarray
    candidates: np.ndarray
    seconds: float = 0.0


def _stand_in(image_shape, bits):
    stand_in = np.zeros(1, np.uint16)
    return capi.RawDepthImage(stand_in.ctypes.data, int(bits), int(image_shape[1]), int(image_shape[0]), 0, int(image_shape[1])), stand_in


def checkMarkers(image_shape, bits: int, dictionary: Dictionary = None, **options) -> capi.MarkersPlan:
    """lifcal_markers_check: the argument checks of detectMarkers for an image of image_shape = (height, width); needs no device"""
    img, keep = _stand_in(image_shape, bits)
    plan = capi.MarkersPlan()
    opt = make_options(**options)
    d = dictionary._struct() if dictionary is not None else None
    _check(capi.load_library().lifcal_markers_check(C.byref(img), C.byref(d) if d is not None else None, C.byref(opt), C.byref(plan)), "lifcal_markers_check")
    del keep
    return plan


def _status_pointer(status, img, shape):
    if status is None:
        return None, None
    if tuple(status.shape) != shape:
        raise ValueError("status: the image's shape")
    if hasattr(status, "data_ptr"):
        import torch
        if not img.on_device or status.dtype != torch.uint8 or not status.is_cuda or not status.is_contiguous():
            raise ValueError("status: a contiguous uint8 tensor on the device, like the image")
        torch.cuda.synchronize(status.device)
        return status.data_ptr(), status
    if img.on_device:
        raise ValueError("status: a tensor on the device, like the image")
    keep = np.ascontiguousarray(status, np.uint8)
    return keep.ctypes.data, keep


def detectMarkers(image, dictionary: Dictionary, status=None, device: int = 0, **options) -> Markers:
    """lifcal_markers_detect.  image: (H, W) uint8 / uint16, a numpy array (rows may be strided) or a torch tensor on `device`;
    status: None or (H, W) uint8 of the same kind, contiguous (TotalFocusImage.status as it is)."""
    lib = capi.load_library()
    img, keep = _image(image)
    opt = make_options(**options)
    d = dictionary._struct()
    plan = capi.MarkersPlan()
    _check(lib.lifcal_markers_check(C.byref(img), C.byref(d), C.byref(opt), C.byref(plan)), "lifcal_markers_check")
    ptr_st, keep_st = _status_pointer(status, img, (int(img.height), int(img.width)))
    cap = min(int(plan.max_candidates), FIRST_CAPACITY)   # one run of the device unless an image holds more than that
    while True:
        rec = np.zeros(cap, capi.MARKER_DTYPE)
        lst = capi.MarkerList(cap, 0, rec.ctypes.data, 0, 0.0)
        rc = lib.lifcal_markers_detect(C.byref(img), ptr_st, int(device), C.byref(d), C.byref(opt), C.byref(lst))
        _check(rc, "lifcal_markers_detect")
        if rc != MORE:
            break
        cap = int(lst.n)   # count, then fill
    del keep, keep_st
    rec = rec[:int(lst.n)]
    return Markers(rec["id"].copy(), rec["rotation"].copy(), rec["hamming"].copy(), rec["refined"].copy(), rec["label"].copy(), rec["area"].copy(),
                   rec["corners"].copy(), rec["x"].copy(), rec["y"].copy(), int(lst.n_candidates), float(lst.seconds))


def markerComponents(image, status=None, device: int = 0, **options) -> MarkerComponents:
    """lifcal_markers_components: the dark map, the label map and the candidate table (steps 1 to 3)"""
    lib = capi.load_library()
    img, keep = _image(image)
    opt = make_options(**options)
    shape = (int(img.height), int(img.width))
    ptr_st, keep_st = _status_pointer(status, img, shape)
    dark = np.zeros(shape, np.uint8)
    labels = np.zeros(shape, np.int32)
    cap = FIRST_CAPACITY
    while True:
        rec = np.zeros(cap, capi.MARKER_COMPONENT_DTYPE)
        out = capi.MarkerComponents(dark.ctypes.data, labels.ctypes.data, cap, 0, rec.ctypes.data, 0.0)
        rc = lib.lifcal_markers_components(C.byref(img), ptr_st, int(device), C.byref(opt), C.byref(out))
        _check(rc, "lifcal_markers_components")
        if rc != MORE:
            break
        cap = int(out.n)
    del keep, keep_st
    return MarkerComponents(dark, labels, rec[:int(out.n)], float(out.seconds))


def detectMarkerSequence(images, dictionary: Dictionary, statuses=None, device: int = 0, unique: bool = True, **options):
    """detectMarkers on every image (one image per call), each list reduced by Markers.unique() unless unique is False"""
    images = list(images)
    statuses = [None] * len(images) if statuses is None else list(statuses)
    if len(statuses) != len(images):
        raise ValueError("detectMarkerSequence: one status map per image, or none")
    out = [detectMarkers(im, dictionary, st, device=device, **options) for im, st in zip(images, statuses)]
    return [m.unique() for m in out] if unique else out


@dataclass
class ConstraintList:
    """readConstraints: id1, id2 (n,) uint32, distance, sigma (n,) float64, ids: the distinct ids in order of first appearance"""
    id1: np.ndarray
    id2: np.ndarray
    distance: np.ndarray
    sigma: np.ndarray
    ids: np.ndarray

    @property
    def n(self) -> int:
        return len(self.id1)


def readConstraints(path) -> ConstraintList:
    """lifcal_constraints_read: the reference's constraints file, lines `id1 id2 distance sigma`; empty lines and # lines are skipped"""
    lib = capi.load_library()
    cap, cap_ids = 0, 0
    while True:
        a = np.zeros(cap, np.uint32); b = np.zeros(cap, np.uint32); dist = np.zeros(cap); sig = np.zeros(cap); ids = np.zeros(cap_ids, np.uint32)
        io = capi.Constraints(cap, 0, capi.as_uptr(a), capi.as_uptr(b), capi.as_dptr(dist), capi.as_dptr(sig), cap_ids, 0, capi.as_uptr(ids))
        rc = lib.lifcal_constraints_read(str(path).encode(), C.byref(io))
        _check(rc, "lifcal_constraints_read")
        if rc != MORE:
            break
        cap, cap_ids = int(io.n), int(io.n_ids)
    return ConstraintList(a, b, dist, sig, ids)


def _marker_observations(markers_per_frame):
    mx, my, mfr, mid = [], [], [], []
    for f, m in enumerate(markers_per_frame):
        if m is None:
            continue
        mx.append(m.x); my.append(m.y); mid.append(np.asarray(m.id, np.uint32)); mfr.append(np.full(m.n, f, np.uint32))
    cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate(parts), dtype) if parts else np.zeros(0, dtype)
    return cat(mx, np.float64), cat(my, np.float64), cat(mfr, np.uint32), cat(mid, np.uint32)


@dataclass
class MarkedTracks(Tracks):
    """addMarkers: Tracks (marker observations in front) and the bookkeeping that goes with them.  track_ids[t]: the point id
    that the feature track t (the old tracks.pt) has now; marker_ids: the marker ids, ascending; n_points: highest point id + 1,
    the number of rows of the point array (mergePoints builds it)."""
    track_ids: np.ndarray = None
    marker_ids: np.ndarray = None
    n_points: int = 0


def addMarkers(tracks: Tracks, features, markers_per_frame) -> MarkedTracks:
    """The tracks with the marker observations in front (the reference's addArucoMarkersToData): a marker's id is its point id.
    The reference removes the points whose ids clash with marker ids; here no track is lost: a track whose id is a marker's id
    is moved, in ascending order, onto the first ids above every track id and marker id; every other track keeps its id.
    features: the frames' Features (one per frame; the marker lists must be as many).  markers_per_frame: one Markers (or None)
    per frame, each id at most once (Markers.unique()).  The marker observations carry feature = NO_FEATURE."""
    if len(markers_per_frame) != len(features):
        raise ValueError("addMarkers: one marker list per frame")
    for m in markers_per_frame:
        if m is not None and len(np.unique(m.id)) != m.n:
            raise ValueError("addMarkers: a marker id occurs twice in one frame; use Markers.unique()")
    mx, my, mfr, mid = _marker_observations(markers_per_frame)
    used = np.unique(mid).astype(np.int64)
    n_tracks = int(tracks.pt.max()) + 1 if len(tracks.pt) else 0
    track_ids = np.arange(n_tracks, dtype=np.int64)
    clash = used[used < n_tracks]
    top = max(n_tracks, int(used.max()) + 1 if len(used) else 0)
    track_ids[clash] = top + np.arange(len(clash))
    pt = track_ids[np.asarray(tracks.pt, np.int64)].astype(np.uint32) if n_tracks else np.zeros(0, np.uint32)
    all_pt = np.concatenate([mid, pt])
    return MarkedTracks(np.concatenate([mfr, np.asarray(tracks.fr, np.uint32)]), all_pt,
                        np.concatenate([np.full(len(mid), NO_FEATURE, np.uint32), np.asarray(tracks.feature, np.uint32)]),
                        np.concatenate([mx, tracks.x]), np.concatenate([my, tracks.y]), len(np.unique(all_pt)), tracks.n_conflicts,
                        track_ids.astype(np.uint32), used.astype(np.uint32), top + len(clash))


def mergePoints(marked: MarkedTracks, pts, ids, xyz) -> np.ndarray:
    """The point array that goes with addMarkers' tracks: (marked.n_points, 3), row = point id.  pts[T, 3]: the points of the
    feature tracks, indexed by the old tracks.pt; ids, xyz: seedMarkerPoints' start values of the markers.  A row whose id
    neither a track nor a seeded marker has (marker ids above the track ids leave such gaps) is NaN."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    if len(p) != len(marked.track_ids):
        raise ValueError("mergePoints: one point per feature track")
    ids = np.asarray(ids, np.int64).reshape(-1)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if len(ids) != len(xyz) or not np.all(np.isin(ids, marked.marker_ids)):
        raise ValueError("mergePoints: ids and xyz are seedMarkerPoints' of the same markers")
    out = np.full((marked.n_points, 3), np.nan)
    out[marked.track_ids.astype(np.int64)] = p
    out[ids] = xyz
    return out


def seedMarkerPoints(markers_per_frame, tracks: Tracks, pts):
    """lifcal_markers_seed_points: (ids, xyz, seeded).  A marker's 3D start value is the 3D point of the nearest tracked image
    point in the first frame that shows the marker.  tracks: the feature tracks alone (before addMarkers), pts[P, 3] their
    points, indexed by tracks.pt.  seeded[k] = False: that frame holds no tracked point."""
    lib = capi.load_library()
    mx, my, mfr, mid = _marker_observations(markers_per_frame)
    tx = np.ascontiguousarray(tracks.x, np.float64); ty = np.ascontiguousarray(tracks.y, np.float64)
    tfr = np.ascontiguousarray(tracks.fr, np.uint32); tpt = np.ascontiguousarray(tracks.pt, np.uint32)
    p = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
    cap = 0
    while True:
        ids = np.zeros(cap, np.uint32); xyz = np.zeros((cap, 3)); seeded = np.zeros(cap, np.uint8)
        io = capi.MarkerSeeds(cap, 0, 0, capi.as_uptr(ids), capi.as_dptr(xyz), seeded.ctypes.data_as(C.POINTER(C.c_uint8)))
        rc = lib.lifcal_markers_seed_points(len(mx), capi.as_dptr(mx), capi.as_dptr(my), capi.as_uptr(mfr), capi.as_uptr(mid), len(tx), capi.as_dptr(tx),
                                            capi.as_dptr(ty), capi.as_uptr(tfr), capi.as_uptr(tpt), len(p), capi.as_dptr(p), C.byref(io))
        _check(rc, "lifcal_markers_seed_points")
        if rc != MORE:
            break
        cap = int(io.n_ids)
    return ids, xyz, seeded.astype(bool)


def sceneScaleFactor(p1, p2, distance: float) -> float:
    """lifcal_scene_scale_factor: distance / |p1 - p2|"""
    a = np.ascontiguousarray(np.asarray(p1, np.float64).reshape(3)); b = np.ascontiguousarray(np.asarray(p2, np.float64).reshape(3))
    f = C.c_double(0.0)
    _check(capi.load_library().lifcal_scene_scale_factor(capi.as_dptr(a), capi.as_dptr(b), float(distance), C.byref(f)), "lifcal_scene_scale_factor")
    return float(f.value)


def scaleScene(views, pts, id1: int, id2: int, distance: float):
    """The reference's scaleData: the scene scaled so that the points id1 and id2 (rows of pts[P, 3]: row = point id, as mergePoints builds it) are `distance` apart, poses
    and points through lifcal_align_apply.  Returns (views', pts', factor)."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    factor = sceneScaleFactor(p[int(id1)], p[int(id2)], distance)
    v, q = alignApply(Alignment(factor, np.eye(3), np.zeros(3), 0.0, 0), views, p)
    return v, q, factor
