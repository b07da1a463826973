/* lifcal_io.h — C ABI of LiFCal's result files, so that consumers of the reference's output read the
 * new solver's results unchanged.  Host code only (no GPU needed), same shared library as include/lifcal_ba.h.
 *
 * Replaces, in the reference (src/CameraCalibration.cpp):
 *   storeCameraModel               :1296-1383   CameraModel.xml            (pugixml default formatting, boost::lexical_cast numbers)
 *   storeExtrinsicOrientations     :1385-1438   extrinsicOrientations.xml
 *   storeExtrinsicOrientationsTxt  :1440-1481   ExtrinsicOrientations.txt  ("%05d" + 16 x " %16.10f", frames sorted by id)
 *   storeRawImagePointsCsv         :1483-1543   rawImagePoints.csv         ("%d,%d,%f,%f,%f,%f,%d")
 *   storeProtocol                  :1545-1617   calibrationProtocol.txt
 *   storeResults                   :1131-1287   objectCoordinates.ply, objectCoordinatesWithCOLMAPIDs.txt, cameraOrientations.ply and the
 *                                               per-frame clouds of refCameraCoordinates/ and projectedCameraCoordinates/ (numbers as
 *                                               std::ofstream << double prints them: %g, six significant digits)
 * All functions return 0, LIFCAL_BA_ERR_INVALID_ARG (-1: null argument / file cannot be opened) or LIFCAL_BA_ERR_OUT_OF_RANGE (-4).
 */
#ifndef LIFCAL_IO_H
#define LIFCAL_IO_H
#include <stdint.h>
#include "lifcal_ba.h"   /* lifcal_ba_group_stats */
#ifdef __cplusplus
extern "C" {
#endif

/* What the reference keeps as members after performBundleAdjustment copied camera[] back (:965-988). */
typedef struct lifcal_camera_model {
  int32_t image_width, image_height;   /* imageSize */
  double pixel_size;                   /* pixelSize [mm] */
  double fL, bL0, B, cx, cy;
  int32_t n_radial;                    /* radialDist.rows() */
  double radial[8];
  int32_t tangential;                  /* tangentialDistParam */
  double tangential_dist[2];
  int32_t ml_center_adjustment;
} lifcal_camera_model;

int lifcal_write_camera_model(const char* path, const lifcal_camera_model* m);
/* views: [6 n_frames] (three angles, three translations per frame); frame_ids: frame.id per frame */
int lifcal_write_extrinsic_orientations_xml(const char* path, uint32_t n_frames, const int32_t* frame_ids, const double* views);
int lifcal_write_extrinsic_orientations_txt(const char* path, uint32_t n_frames, const int32_t* frame_ids, const double* views);
/* One line per observation, frames in order, observations in their order inside the frame (fr must be non-decreasing, as
 * projectPointsToRawImage produces it, and below n_frames): frame id, index inside the frame, u, v, x_proj, y_proj (lifcal_ba_project_observations),
 * object-point index. */
int lifcal_write_raw_image_points_csv(const char* path, uint64_t n_obs, uint32_t n_frames, const int32_t* frame_ids, const uint32_t* fr, const double* u,
                                      const double* v, const double* x_proj, const double* y_proj, const uint32_t* pt);

typedef struct lifcal_protocol {
  lifcal_camera_model model;
  int32_t refine_poses, refine_points, robust_cost;
  double std_x, std_y, mae_x, mae_y;   /* lifcal_ba_stats */
} lifcal_protocol;
int lifcal_write_protocol(const char* path, const lifcal_protocol* p);

/* objectCoordinates.ply (:1131-1144): the object points p3d_w, [3 n_points], each line "x y z 0" */
int lifcal_write_object_coordinates_ply(const char* path, uint64_t n_points, const double* pts);
/* objectCoordinatesWithCOLMAPIDs.txt (:1146-1152): "id x y z" per point, colmap_ids[i] = getCorrespondingCOLMAPID of point i */
int lifcal_write_object_coordinates_colmap_ids(const char* path, uint64_t n_points, const int32_t* colmap_ids, const double* pts);
/* cameraOrientations.ply (:1154-1216): per frame the projection centre and the four image corners at three focal lengths, moved to
 * world coordinates by the inverse pose, and four triangles.  The frustum is built in float as the reference builds it (:1170-1180)
 * from c (cx, cy), fL and pixelSize_totFoc. */
int lifcal_write_camera_orientations_ply(const char* path, uint32_t n_frames, const double* views, int32_t image_width, int32_t image_height,
                                         double cx, double cy, double fL, double pixel_size_tot_foc);
/* <dir>/cameraCoordinates_%04d.ply of one frame (:1244-1286), frame_id = frame.id: serves refCameraCoordinates/ (ref_c of
 * lifcal_ba_object_space_stats) and projectedCameraCoordinates/ (proj_c); xyz: [3 n_points] of the frame.  The directory must exist. */
int lifcal_write_camera_coordinates_ply(const char* dir, int32_t frame_id, uint64_t n_points, const double* xyz);

/* One table of lifcal_ba_residual_report (or of lifcal_ba_residual_groups) as CSV; no reference counterpart.  A header line, then one
 * line per NON-EMPTY group k < n: "id[,x,y],n,n_inliers,mean_x,mean_y,rms_x,rms_y,max_abs_x,max_abs_y,mean_weight", floats as %.6f.
 * id = ids[k], or k when ids is NULL (id_header names the column: "frame", "point", "lens", ...); the x,y columns are xy[2k], xy[2k + 1]
 * (the lens centres of the per-lens table) and are left out when xy is NULL. */
int lifcal_write_group_stats_csv(const char* path, const char* id_header, uint64_t n, const int32_t* ids, const double* xy,
                                 const lifcal_ba_group_stats* rows);

#ifdef __cplusplus
}
#endif
#endif
