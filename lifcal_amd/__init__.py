"""lifcal_amd — MI355X-native plenoptic bundle adjustment behind LiFCal's performBundleAdjustment seam.

Only what the hot path needs: csrc/ (HIP kernels + C ABI), the ctypes view of include/lifcal_ba.h,
the host mirror of the reference entry points and the synthetic scene generator.
"""
from . import _capi, scene  # noqa: F401
from .bundle_adjustment import (BundleAdjustment, Covariance, LifcalError, make_config, plan, plan_stats, plan_shape, comm_unique_id, initPlenopticParameters,  # noqa: F401
                                performBundleAdjustmentWindowed, GroupTable, ResidualReport, sensor_cells, check_priors, prior_from_covariance,
                                check_point_priors, alignFit, alignApply, alignScene, Alignment)
from .mla import MicroLensGrid, RawObservations  # noqa: F401
from .depth import DepthMaps, backProjectPoints, projectPoints, readDepthData, read_png16, depth_is_estimable  # noqa: F401
from .resection import resectFrames, ResectionResult  # noqa: F401
from .intersection import intersectPoints, IntersectionResult  # noqa: F401
from .start import startPoses, startPoints, StartPosesResult, StartPointsResult  # noqa: F401
from .register import registerScene, RegisterResult  # noqa: F401
from .grid_fit import detectLensCentres, fitGridCentres, fitGrid, GridFit, GridReport  # noqa: F401
from .raw_depth import estimateRawDepth, checkRawDepth, RawDepth, RawPoints  # noqa: F401
from .depth_map import depthMapFromRaw, checkDepthMap, VirtualDepthMap  # noqa: F401
from .total_focus import totalFocusImage, checkTotalFocus, TotalFocusImage  # noqa: F401
from .features import detectFeatures, matchFeatures, linkTracks, trackSequence, checkFeatures, Features, Matches, Tracks  # noqa: F401
from .verify import featurePoints, verifyMatches, checkVerify, FeaturePoints, Verification  # noqa: F401
from .markers import (Dictionary, Markers, MarkerComponents, ConstraintList, checkMarkers, detectMarkers, markerComponents, detectMarkerSequence,  # noqa: F401
                      readConstraints, addMarkers, mergePoints, MarkedTracks, seedMarkerPoints, sceneScaleFactor, scaleScene)
