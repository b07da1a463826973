// register.hpp — lifcal_register_scene (include/lifcal_register.h): its kernels, then the host driver (included at the end of
// lifcal_ba.hip, behind start.hpp).  DESIGN.md section 7o.
//
// The chain is device-resident.  One staging upload carries the observations in three orders ((fr, pt)-major for the groups,
// frame-major and point-major for the two solvers), their CSRs, the group CSRs by frame and by point and the start rows.  Poses,
// points, the two masks (fstate per frame, pmask per point), the group table and the rows stay in HBM until the one download at
// the end; per round the host reads one word (the frames registered in that round).
//
//   k_start_groups   (start.hpp) the group table, once
//   k_reg_counts     one workgroup per frame: its used groups
//   k_reg_anchor     one thread: the anchor's pose, state and row
//   k_reg_frontier   one workgroup per unregistered frame: n_shared; from min_shared on the alignment of k_start_align over the used
//                    groups on mapped points, the pose, fstate = NEW, the round's counter
//   k_resect<MASKED> (resection.hpp) the pose solve of the frames in one state over their observations of mapped points
//   k_reg_frames     one thread per frame: NEW -> REGISTERED, the frame_eval table of every registered pose
//   k_reg_extend     one wave64 per unmapped point: the weighted mean of its used groups carried into the world
//   k_intersect<MASKED> (intersection.hpp) the point solve of the mapped points over their observations in registered frames
//   k_reg_frame_stats, k_reg_point_stats   the error sums of the rows at the returned parameters
// Every sum has ONE order: a lane adds in ascending position, lanes are folded by wave_sum / rs_fold.  The only atomic is the
// integer counter of a round, which is no result.  No kernel waits for another workgroup.
#pragma once
#include "../../include/lifcal_register.h"

namespace lifcal {

enum : uint32_t { REG_UNREGISTERED = 0, REG_REGISTERED = 1, REG_NEW = 2 };

struct RegArgs {
  const uint32_t *off, *fgoff, *fpt;            // frame-major: [F + 1] CSR of the observations | of the groups, [N] point of an observation
  const uint32_t *poff, *pgoff, *pgidx, *pfr;   // point-major: [P + 1] CSR of the observations | of the groups, [G] group ids (ascending frame), [N] frame
  const double *fu, *fv, *fmx, *fmy, *fcus;     // frame-major observations, c_u for the parameters as stored
  const double *pu, *pv, *pmx, *pmy, *pcus;     // point-major likewise
  const CamConsts* camc;                        // [2] folded | as stored
  const lifcal_start_group* groups;             // [G]
  double *views, *pts, *ft;                     // [6F], [3P], [F][FRAME_STRIDE]
  uint32_t *fstate, *pmask, *counters;          // [F], [P], [F + 2] frames registered by round
  lifcal_register_frame* frows;                 // [F]
  lifcal_register_point* prows;                 // [P]
  double anchor_view[6];
  double thr2;
  uint32_t n_frames, n_points, min_shared, anchor;
  int32_t round;                                // k_reg_frontier: < 0 counts only, for the frames that were never aligned
};

__global__ __launch_bounds__(ST_THREADS) void k_reg_counts(RegArgs a) {
  __shared__ double s_red[ST_WAVES], s_out[1];
  const uint32_t f = blockIdx.x;
  double acc[1] = {0.0};
  for (uint32_t g = a.fgoff[f] + threadIdx.x; g < a.fgoff[f + 1]; g += ST_THREADS)
    if (a.groups[g].status == LIFCAL_START_GROUP_USED) acc[0] += 1.0;
  rs_fold<1>(acc, s_red, s_out);
  if (threadIdx.x == 0) a.frows[f].n_used = (uint32_t)s_out[0];
}

__global__ void k_reg_anchor(RegArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int k = 0; k < 6; ++k) a.views[6 * (size_t)a.anchor + k] = a.anchor_view[k];
  a.fstate[a.anchor] = REG_REGISTERED;
  lifcal_register_frame* row = a.frows + a.anchor;
  row->status = LIFCAL_REGISTER_FRAME_OK; row->round = 0; row->termination = 0;
}

__global__ __launch_bounds__(ST_THREADS) void k_reg_frontier(RegArgs a) {
  __shared__ double s_red[ST_WAVES * 9], s_out[9], s_eig[2];
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  lifcal_register_frame* row = a.frows + f;
  if (a.round < 0 ? row->round > 0 : a.fstate[f] != REG_UNREGISTERED) return;   // (the same in every thread)
  const uint32_t gb = a.fgoff[f], ge = a.fgoff[f + 1];
  if (gb == ge) return;
  double acc[9];
  st_centroid_sums<true>(a.groups, gb, ge, a.pts, a.pmask, acc);
  rs_fold<8>(acc, s_red, s_out);
  const double sw = s_out[0];
  const uint32_t n_shared = (uint32_t)s_out[7];
  if (tid == 0) row->n_shared = n_shared;
  if (a.round < 0 || n_shared < a.min_shared) return;
  double Pm[3], cm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { Pm[k] = s_out[1 + k] / sw; cm[k] = s_out[4 + k] / sw; }
  st_moment_sums<true>(a.groups, gb, ge, a.pts, a.pmask, Pm, cm, acc);
  rs_fold<9>(acc, s_red, s_out);
  if (tid == 0) {
    double view[6];
    if (start_pose(s_out, Pm, cm, view, s_eig) == LIFCAL_START_FRAME_OK) {
#pragma unroll
      for (int k = 0; k < 6; ++k) a.views[6 * (size_t)f + k] = view[k];
      a.fstate[f] = REG_NEW;
      row->status = LIFCAL_REGISTER_FRAME_OK; row->round = a.round;
      atomicAdd(a.counters + a.round, 1u);
    } else {
      row->status = LIFCAL_REGISTER_FRAME_DEGENERATE;   // (tried again in the next round)
    }
  }
}

__global__ __launch_bounds__(256) void k_reg_frames(RegArgs a) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n_frames) return;
  uint32_t st = a.fstate[f];
  if (st == REG_NEW) { st = REG_REGISTERED; a.fstate[f] = st; }
  if (st == REG_REGISTERED) {
    double o[FRAME_STRIDE];
    frame_eval(a.views + 6 * (size_t)f, o);
#pragma unroll
    for (int k = 0; k < FRAME_STRIDE; ++k) a.ft[(size_t)f * FRAME_STRIDE + k] = o[k];
  }
}

__global__ __launch_bounds__(ST_THREADS) void k_reg_extend(RegArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * ST_WAVES + (threadIdx.x >> 6)));
  if (p >= a.n_points || a.pmask[p]) return;
  double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (uint32_t k = a.pgoff[p] + lane; k < a.pgoff[p + 1]; k += 64u) {
    const lifcal_start_group* r = a.groups + a.pgidx[k];
    if (r->status != LIFCAL_START_GROUP_USED || a.fstate[r->fr] != REG_REGISTERED) continue;
    const double* __restrict__ ft = a.ft + (size_t)r->fr * FRAME_STRIDE;
    const double w = 1.0 / (r->xyz[2] * r->xyz[2]);
    const double d0 = r->xyz[0] - ft[9], d1 = r->xyz[1] - ft[10], d2 = r->xyz[2] - ft[11];
    sw += w;
    s0 += w * (ft[0] * d0 + ft[3] * d1 + ft[6] * d2);
    s1 += w * (ft[1] * d0 + ft[4] * d1 + ft[7] * d2);
    s2 += w * (ft[2] * d0 + ft[5] * d1 + ft[8] * d2);
  }
  sw = wave_sum(sw); s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
  if (!(sw > 0.0)) return;   // no used group in a registered frame
  if (lane == 0) {
    double* out = a.pts + 3 * (size_t)p;
    out[0] = s0 / sw; out[1] = s1 / sw; out[2] = s2 / sw;
    a.pmask[p] = 1u;
    lifcal_register_point* row = a.prows + p;
    row->status = LIFCAL_REGISTER_POINT_OK; row->round = a.round;
  }
}

template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(ST_THREADS) void k_reg_frame_stats(RegArgs a) {
  __shared__ double s_red[ST_WAVES * 4], s_out[4];
  const uint32_t f = blockIdx.x;
  if (a.fstate[f] != REG_REGISTERED) return;
  const double* __restrict__ ft = a.ft + (size_t)f * FRAME_STRIDE;
  const CamConsts& cs = a.camc[1];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t i = a.off[f] + threadIdx.x; i < a.off[f + 1]; i += ST_THREADS) {
    const uint32_t q = a.fpt[i];
    if (!a.pmask[q]) continue;
    const double* P = a.pts + 3 * (size_t)q;
    const double2 w = *reinterpret_cast<const double2*>(a.fcus + 2 * (size_t)i);
    GroupConsts gc;
    group_prepare(cs, ft[0] * P[0] + ft[1] * P[1] + ft[2] * P[2] + ft[9], ft[3] * P[0] + ft[4] * P[1] + ft[5] * P[2] + ft[10],
                  ft[6] * P[0] + ft[7] * P[1] + ft[8] * P[2] + ft[11], gc);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(cs, gc, a.fmx[i], a.fmy[i], w.x, w.y, a.fu[i], a.fv[i], rx, ry);
    acc[0] += rx * rx; acc[1] += ry * ry; acc[3] += 1.0;
    if (rx * rx + ry * ry <= a.thr2) acc[2] += 1.0;
  }
  rs_fold<4>(acc, s_red, s_out);
  if (threadIdx.x == 0) {
    lifcal_register_frame* row = a.frows + f;
    row->sum_xx = s_out[0]; row->sum_yy = s_out[1]; row->n_inliers = (uint32_t)s_out[2]; row->n_obs_used = (uint32_t)s_out[3];
  }
}

template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(ST_THREADS) void k_reg_point_stats(RegArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * ST_WAVES + (threadIdx.x >> 6)));
  if (p >= a.n_points || !a.pmask[p]) return;
  const CamConsts& cs = a.camc[1];
  const double P0 = a.pts[3 * (size_t)p], P1 = a.pts[3 * (size_t)p + 1], P2 = a.pts[3 * (size_t)p + 2];
  double sxx = 0.0, syy = 0.0, inl = 0.0, cnt = 0.0, nfr = 0.0;
  for (uint32_t i = a.poff[p] + lane; i < a.poff[p + 1]; i += 64u) {
    const uint32_t f = a.pfr[i];
    if (a.fstate[f] != REG_REGISTERED) continue;
    const double* __restrict__ ft = a.ft + (size_t)f * FRAME_STRIDE;
    const double2 w = *reinterpret_cast<const double2*>(a.pcus + 2 * (size_t)i);
    GroupConsts gc;
    group_prepare(cs, ft[0] * P0 + ft[1] * P1 + ft[2] * P2 + ft[9], ft[3] * P0 + ft[4] * P1 + ft[5] * P2 + ft[10],
                  ft[6] * P0 + ft[7] * P1 + ft[8] * P2 + ft[11], gc);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(cs, gc, a.pmx[i], a.pmy[i], w.x, w.y, a.pu[i], a.pv[i], rx, ry);
    sxx += rx * rx; syy += ry * ry; cnt += 1.0;
    if (rx * rx + ry * ry <= a.thr2) inl += 1.0;
  }
  for (uint32_t k = a.pgoff[p] + lane; k < a.pgoff[p + 1]; k += 64u)
    if (a.fstate[a.groups[a.pgidx[k]].fr] == REG_REGISTERED) nfr += 1.0;
  sxx = wave_sum(sxx); syy = wave_sum(syy); inl = wave_sum(inl); cnt = wave_sum(cnt); nfr = wave_sum(nfr);
  if (lane == 0) {
    lifcal_register_point* row = a.prows + p;
    row->sum_xx = sxx; row->sum_yy = syy; row->n_inliers = (uint32_t)inl; row->n_obs_used = (uint32_t)cnt; row->n_frames_used = (uint32_t)nfr;
  }
}

}  // namespace lifcal

extern "C" void lifcal_register_default_options(lifcal_register_options* r) {
  if (!r) return;
  r->gate_px = 1.0; r->inlier_threshold = 1.0; r->min_shared = 6; r->anchor_frame = -1; r->anchor_view = nullptr; r->max_rounds = 0; r->reserved = 0;
}

namespace {

int register_impl(const lifcal_register_problem* p, const lifcal_ba_options* o, const lifcal_register_options* r, lifcal_register_frame* per_frame,
                  lifcal_register_point* per_point, lifcal_register_summary* summary, double* seconds) {
  if (!r || !per_point || !summary) { g_last_error = "lifcal_register_scene: null register options, point rows or summary"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (!(r->gate_px > 0.0)) { g_last_error = "lifcal_register_scene: gate_px must be > 0 (+infinity: no gate)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (r->min_shared < 3u) { g_last_error = "lifcal_register_scene: min_shared must be >= 3"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (int rc = batch_checks("lifcal_register_scene", p, o, per_frame, true)) return rc;
  if (r->anchor_frame >= 0 && (uint32_t)r->anchor_frame >= p->n_frames) { g_last_error = "lifcal_register_scene: anchor_frame names no frame"; return LIFCAL_BA_ERR_INVALID_ARG; }
  const uint32_t N = p->n_obs, F = p->n_frames, P = p->n_points;

  // the three orders of the observations, each stable in the caller's order: point-major, frame-major, (fr, pt)-major
  std::vector<uint32_t> poff((size_t)P + 1, 0u), pidx(N), off((size_t)F + 1, 0u), fidx(N), gidx(N);
  if (N) {
    if (int rc = lifcal_group_index(N, P, p->pt, poff.data(), pidx.data())) return rc;
    if (int rc = lifcal_group_index(N, F, p->fr, off.data(), fidx.data())) return rc;
    if (int rc = frame_point_order(N, F, p->fr, pidx, off.data(), gidx)) return rc;   // (off once more: the same counts)
  }
  // the groups: runs of equal (fr, pt); per frame its run of groups, per point its groups in ascending frame order
  const Groups g = build_groups(N, F, p->fr, p->pt, gidx);
  const uint32_t G = g.G;
  std::vector<uint32_t> pgoff((size_t)P + 1, 0u), pgidx(G);
  if (G) { if (int rc = lifcal_group_index(G, P, g.gpt.data(), pgoff.data(), pgidx.data())) return rc; }

  // the rows every frame and point starts with
  std::vector<lifcal_register_frame> frows(F);
  std::vector<lifcal_register_point> prows(P);
  if (F) std::memset(frows.data(), 0, (size_t)F * sizeof(lifcal_register_frame));
  if (P) std::memset(prows.data(), 0, (size_t)P * sizeof(lifcal_register_point));
  for (uint32_t f = 0; f < F; ++f) {
    frows[f].n_obs = off[(size_t)f + 1] - off[f]; frows[f].n_groups = g.fgoff[(size_t)f + 1] - g.fgoff[f]; frows[f].round = -1;
    frows[f].status = frows[f].n_obs ? LIFCAL_REGISTER_FRAME_UNREACHED : LIFCAL_REGISTER_FRAME_EMPTY;
  }
  for (uint32_t k = 0; k < P; ++k) {
    prows[k].n_obs = poff[(size_t)k + 1] - poff[k]; prows[k].round = -1;
    prows[k].status = prows[k].n_obs ? LIFCAL_REGISTER_POINT_UNREACHED : LIFCAL_REGISTER_POINT_EMPTY;
  }
  lifcal_register_summary sum;
  std::memset(&sum, 0, sizeof sum);
  sum.anchor_frame = -1; sum.n_groups = G;
  auto answer = [&]() {   // rows and summary to the caller
    if (F) std::memcpy(per_frame, frows.data(), (size_t)F * sizeof(lifcal_register_frame));
    if (P) std::memcpy(per_point, prows.data(), (size_t)P * sizeof(lifcal_register_point));
    *summary = sum;
    return 0;
  };
  if (seconds) *seconds = 0.0;
  if (!N) return answer();   // nothing to register: no device is needed

  ByteLayout L;
  const size_t W = (size_t)N * 8;
  const size_t at_gu = L.take(W), at_gv = L.take(W), at_gmx = L.take(W), at_gmy = L.take(W),
               at_fu = L.take(W), at_fv = L.take(W), at_fmx = L.take(W), at_fmy = L.take(W), at_fpt = L.take((size_t)N * 4),
               at_pu = L.take(W), at_pv = L.take(W), at_pmx = L.take(W), at_pmy = L.take(W), at_pfr = L.take((size_t)N * 4),
               at_off = L.take(((size_t)F + 1) * 4), at_fgoff = L.take(((size_t)F + 1) * 4), at_poff = L.take(((size_t)P + 1) * 4), at_pgoff = L.take(((size_t)P + 1) * 4),
               at_pgidx = L.take((size_t)G * 4), at_goff = L.take(((size_t)G + 1) * 4), at_gfr = L.take((size_t)G * 4), at_gpt = L.take((size_t)G * 4),
               at_cam = L.take(LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8), at_frows = L.take((size_t)F * sizeof(lifcal_register_frame)),
               at_prows = L.take((size_t)P * sizeof(lifcal_register_point));
  const size_t in_bytes = L.bytes;
  const size_t at_zero = L.bytes;   // (zeroed: poses, points, tables, states, counters)
  const size_t at_views = L.take((size_t)F * 48), at_pts = L.take((size_t)P * 24), at_ft = L.take((size_t)F * FRAME_STRIDE * 8), at_fstate = L.take((size_t)F * 4),
               at_pmask = L.take((size_t)P * 4), at_cnt = L.take(((size_t)F + 2) * 4);
  const size_t zero_bytes = L.bytes - at_zero;
  const size_t at_gcu = L.take((size_t)N * 16), at_fcu = L.take((size_t)N * 16), at_fcus = L.take((size_t)N * 16), at_pcu = L.take((size_t)N * 16), at_pcus = L.take((size_t)N * 16),
               at_camc = L.take(2 * sizeof(CamConsts)), at_grp = L.take((size_t)G * sizeof(lifcal_start_group));
  std::vector<unsigned char> host(in_bytes);
  stage_observations(host, gidx, N, p, at_gu, at_gv, at_gmx, at_gmy, 0, nullptr);
  stage_observations(host, fidx, N, p, at_fu, at_fv, at_fmx, at_fmy, at_fpt, p->pt);
  stage_observations(host, pidx, N, p, at_pu, at_pv, at_pmx, at_pmy, at_pfr, p->fr);
  std::memcpy(host.data() + at_off, off.data(), off.size() * 4);
  std::memcpy(host.data() + at_fgoff, g.fgoff.data(), g.fgoff.size() * 4);
  std::memcpy(host.data() + at_poff, poff.data(), poff.size() * 4);
  std::memcpy(host.data() + at_pgoff, pgoff.data(), pgoff.size() * 4);
  std::memcpy(host.data() + at_pgidx, pgidx.data(), (size_t)G * 4);
  std::memcpy(host.data() + at_goff, g.goff.data(), g.goff.size() * 4);
  std::memcpy(host.data() + at_gfr, g.gfr.data(), (size_t)G * 4);
  std::memcpy(host.data() + at_gpt, g.gpt.data(), (size_t)G * 4);
  std::memcpy(host.data() + at_cam, p->cam, LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8);
  std::memcpy(host.data() + at_frows, frows.data(), (size_t)F * sizeof(lifcal_register_frame));
  std::memcpy(host.data() + at_prows, prows.data(), (size_t)P * sizeof(lifcal_register_point));
  std::vector<double> views_out((size_t)F * 6), pts_out((size_t)P * 3);   // (p->views, p->pts are output only: nothing of them goes to the device)

  if (int rc = mla::select_device(o->device, "lifcal_register_scene")) return rc;
  // (every return below leaves through D, which waits for the stream if anything is queued: the copies read and write the vectors above)
  BatchCall D(o->device, "lifcal_register_scene");
  D.open(L.bytes);
  D.upload(host.data(), in_bytes);
  D.zero(at_zero, zero_bytes);
  D.begin();
  if (!D.ok()) return D.fail();
  unsigned char* const dev = D.dev;
  hipStream_t const stream = D.stream;

  const double* d_cam = (const double*)(dev + at_cam);
  StartGroupArgs ga{};
  ga.goff = (const uint32_t*)(dev + at_goff); ga.gfr = (const uint32_t*)(dev + at_gfr); ga.gpt = (const uint32_t*)(dev + at_gpt);
  ga.u = (const double*)(dev + at_gu); ga.v = (const double*)(dev + at_gv); ga.mcx = (const double*)(dev + at_gmx); ga.mcy = (const double*)(dev + at_gmy);
  ga.cu = (const double*)(dev + at_gcu); ga.camc = (const CamConsts*)(dev + at_camc); ga.groups = (lifcal_start_group*)(dev + at_grp);
  ga.gate_px = r->gate_px; ga.n_groups = G;
  RegArgs a{};
  a.off = (const uint32_t*)(dev + at_off); a.fgoff = (const uint32_t*)(dev + at_fgoff); a.fpt = (const uint32_t*)(dev + at_fpt);
  a.poff = (const uint32_t*)(dev + at_poff); a.pgoff = (const uint32_t*)(dev + at_pgoff); a.pgidx = (const uint32_t*)(dev + at_pgidx); a.pfr = (const uint32_t*)(dev + at_pfr);
  a.fu = (const double*)(dev + at_fu); a.fv = (const double*)(dev + at_fv); a.fmx = (const double*)(dev + at_fmx); a.fmy = (const double*)(dev + at_fmy); a.fcus = (const double*)(dev + at_fcus);
  a.pu = (const double*)(dev + at_pu); a.pv = (const double*)(dev + at_pv); a.pmx = (const double*)(dev + at_pmx); a.pmy = (const double*)(dev + at_pmy); a.pcus = (const double*)(dev + at_pcus);
  a.camc = ga.camc; a.groups = ga.groups;
  a.views = (double*)(dev + at_views); a.pts = (double*)(dev + at_pts); a.ft = (double*)(dev + at_ft);
  a.fstate = (uint32_t*)(dev + at_fstate); a.pmask = (uint32_t*)(dev + at_pmask); a.counters = (uint32_t*)(dev + at_cnt);
  a.frows = (lifcal_register_frame*)(dev + at_frows); a.prows = (lifcal_register_point*)(dev + at_prows);
  for (int k = 0; k < 6; ++k) a.anchor_view[k] = r->anchor_view ? r->anchor_view[k] : 0.0;
  a.thr2 = r->inlier_threshold * r->inlier_threshold;
  a.n_frames = F; a.n_points = P; a.min_shared = r->min_shared; a.anchor = 0; a.round = 0;
  // the two solvers, as lifcal_resect_frames and lifcal_intersect_points set them up, with the masks
  const LmOpts lo{o->function_tolerance, o->parameter_tolerance, o->gradient_tolerance, o->min_relative_decrease, o->max_radius, o->min_radius, o->max_iterations};
  const uint32_t robust = (p->config & LIFCAL_BA_CFG_ROBUST) ? 1u : 0u, jacobi = o->jacobi_scaling ? 1u : 0u;
  ResectArgs ra{};
  ra.off = a.off; ra.pt = a.fpt; ra.u = a.fu; ra.v = a.fv; ra.mcx = a.fmx; ra.mcy = a.fmy;
  ra.cu = (const double*)(dev + at_fcu); ra.cu_stats = a.fcus; ra.camc = a.camc; ra.cam = d_cam; ra.pts = a.pts; ra.views = a.views; ra.rows = nullptr;
  ra.lo = lo; ra.initial_radius = o->initial_radius; ra.lm_min = o->min_lm_diagonal; ra.lm_max = o->max_lm_diagonal; ra.thr2 = a.thr2; ra.robust = robust; ra.jacobi = jacobi;
  ra.pmask = a.pmask; ra.fstate = a.fstate; ra.reg_rows = a.frows; ra.fwant = REG_NEW; ra.skip_frame = 0xFFFFFFFFu;
  IntersectArgs ia{};
  ia.off = a.poff; ia.fr = a.pfr; ia.u = a.pu; ia.v = a.pv; ia.mcx = a.pmx; ia.mcy = a.pmy;
  ia.cu = (const double*)(dev + at_pcu); ia.cu_stats = a.pcus; ia.camc = a.camc; ia.cam = d_cam; ia.ft = a.ft; ia.pts = a.pts; ia.rows = nullptr;
  ia.lo = lo; ia.initial_radius = o->initial_radius; ia.lm_min = o->min_lm_diagonal; ia.lm_max = o->max_lm_diagonal; ia.thr2 = a.thr2;
  ia.n_points = P; ia.robust = robust; ia.jacobi = jacobi;
  ia.fstate = a.fstate; ia.pmask = a.pmask; ia.reg_rows = a.prows;

  const uint32_t lens_grid = (N + 255u) / 256u, group_grid = (G + (uint32_t)ST_THREADS - 1u) / (uint32_t)ST_THREADS, frame_grid = (F + 255u) / 256u,
                 point_grid = (P + (uint32_t)ST_WAVES - 1u) / (uint32_t)ST_WAVES, solve_grid = (P + (uint32_t)IS_WAVES - 1u) / (uint32_t)IS_WAVES;
  const ModelCfg cfg = model_cfg(p->config);
  auto lens = [&](int fold, const double* mx, const double* my, size_t at_out) -> int {
    return launch_lens_pass(cfg, stream, lens_grid, d_cam, p->spx, p->spy, p->scale, o->loss_scale, fold, N, mx, my, (CamConsts*)(dev + at_camc), (double*)(dev + at_out));
  };
  auto groups = [&]() -> int {
#define CALL_REG_GROUPS(NR, TAN, ADJ) hipLaunchKernelGGL((k_start_groups<NR, TAN, ADJ>), dim3(group_grid), dim3(ST_THREADS), 0, stream, ga)
    DISPATCH_CFG(&cfg, CALL_REG_GROUPS);
#undef CALL_REG_GROUPS
    return 0;
  };
  auto solve_poses = [&](uint32_t want, uint32_t skip) -> int {
    ra.fwant = want; ra.skip_frame = skip;
#define CALL_REG_RESECT(NR, TAN, ADJ) hipLaunchKernelGGL((k_resect<NR, TAN, ADJ, true>), dim3(F), dim3(RS_THREADS), 0, stream, ra)
    DISPATCH_CFG(&cfg, CALL_REG_RESECT);
#undef CALL_REG_RESECT
    return 0;
  };
  auto solve_points = [&]() -> int {
#define CALL_REG_INTERSECT(NR, TAN, ADJ) hipLaunchKernelGGL((k_intersect<NR, TAN, ADJ, true>), dim3(solve_grid), dim3(IS_THREADS), 0, stream, ia)
    DISPATCH_CFG(&cfg, CALL_REG_INTERSECT);
#undef CALL_REG_INTERSECT
    return 0;
  };
  auto stats = [&]() -> int {
#define CALL_REG_STATS(NR, TAN, ADJ) do { \
    hipLaunchKernelGGL((k_reg_frame_stats<NR, TAN, ADJ>), dim3(F), dim3(ST_THREADS), 0, stream, a); \
    hipLaunchKernelGGL((k_reg_point_stats<NR, TAN, ADJ>), dim3(point_grid), dim3(ST_THREADS), 0, stream, a); } while (0)
    DISPATCH_CFG(&cfg, CALL_REG_STATS);
#undef CALL_REG_STATS
    return 0;
  };
  auto extend_and_refine_points = [&]() -> int {
    hipLaunchKernelGGL(k_reg_frames, dim3(frame_grid), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_reg_extend, dim3(point_grid), dim3(ST_THREADS), 0, stream, a);
    return solve_points();
  };

  // the lens passes, the group table, the used groups of every frame -> the anchor
  int rc = lens(1, ga.mcx, ga.mcy, at_gcu);
  if (!rc) rc = lens(1, a.fmx, a.fmy, at_fcu);
  if (!rc) rc = lens(0, a.fmx, a.fmy, at_fcus);
  if (!rc) rc = lens(1, a.pmx, a.pmy, at_pcu);
  if (!rc) rc = lens(0, a.pmx, a.pmy, at_pcus);
  if (!rc) rc = groups();
  if (rc) return rc;
  hipLaunchKernelGGL(k_reg_counts, dim3(F), dim3(ST_THREADS), 0, stream, a);
  D.launched();
  D.download(frows.data(), at_frows, (size_t)F * sizeof(lifcal_register_frame));
  if ((rc = D.wait())) return rc;
  int64_t anchor = -1;
  for (uint32_t f = 0; f < F; ++f) {
    sum.n_groups_used += frows[f].n_used;
    if (frows[f].n_used && (anchor < 0 || frows[f].n_used > frows[(size_t)anchor].n_used)) anchor = f;
  }
  if (!sum.n_groups_used) return answer();   // no used group: nothing can be registered
  if (r->anchor_frame >= 0) anchor = r->anchor_frame;
  sum.anchor_frame = (int32_t)anchor;
  a.anchor = (uint32_t)anchor;

  // round 0
  a.round = 0;
  hipLaunchKernelGGL(k_reg_anchor, dim3(1), dim3(64), 0, stream, a);
  if ((rc = extend_and_refine_points())) return rc;
  // rounds r >= 1: every round registers a frame or ends the loop
  for (uint32_t round = 1; round <= F && (r->max_rounds == 0 || round <= r->max_rounds); ++round) {
    a.round = (int32_t)round;
    hipLaunchKernelGGL(k_reg_frontier, dim3(F), dim3(ST_THREADS), 0, stream, a);
    if ((rc = solve_poses(REG_NEW, 0xFFFFFFFFu))) return rc;
    uint32_t n_new = 0;
    D.launched();
    D.download(&n_new, at_cnt + (size_t)round * 4, 4);
    if ((rc = D.wait())) return rc;
    if (!n_new) break;
    sum.n_rounds = round;
    if ((rc = extend_and_refine_points())) return rc;
    if ((rc = solve_poses(REG_REGISTERED, a.anchor))) return rc;
  }
  // the rows at the returned parameters; n_shared of the frames that were never aligned
  a.round = -1;
  hipLaunchKernelGGL(k_reg_frames, dim3(frame_grid), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_reg_frontier, dim3(F), dim3(ST_THREADS), 0, stream, a);
  if ((rc = stats())) return rc;
  D.end();
  D.download(views_out.data(), at_views, (size_t)F * 48);
  if (P) D.download(pts_out.data(), at_pts, (size_t)P * 24);
  D.download(frows.data(), at_frows, (size_t)F * sizeof(lifcal_register_frame));
  if (P) D.download(prows.data(), at_prows, (size_t)P * sizeof(lifcal_register_point));
  if ((rc = D.finish(seconds))) return rc;
  for (uint32_t f = 0; f < F; ++f)
    if (frows[f].status == LIFCAL_REGISTER_FRAME_OK) { std::memcpy(p->views + 6 * (size_t)f, views_out.data() + 6 * (size_t)f, 48); ++sum.n_frames_registered; }
  for (uint32_t k = 0; k < P; ++k)
    if (prows[k].status == LIFCAL_REGISTER_POINT_OK) { std::memcpy(p->pts + 3 * (size_t)k, pts_out.data() + 3 * (size_t)k, 24); ++sum.n_points_mapped; }
  return answer();
}

}  // namespace

extern "C" int lifcal_register_scene(const lifcal_register_problem* p, const lifcal_ba_options* o, const lifcal_register_options* r,
                                     lifcal_register_frame* per_frame, lifcal_register_point* per_point, lifcal_register_summary* summary, double* seconds) {
  return guard_abi("lifcal_register_scene", [&] { return register_impl(p, o, r, per_frame, per_point, summary, seconds); });
}
