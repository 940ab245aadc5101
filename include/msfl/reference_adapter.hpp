// msfl/reference_adapter.hpp — the reference-side binding of libmsfl_hip.so as templates over the CALLER's types.
//
// One set of function bodies that compiles unchanged on both sides of the boundary:
//   * inside MSF_LOAM, instantiated with pcl::PointCloud<pcl::PointXYZI / PointXYZIRT> (32-byte points, common/common.h:44-62),
//     TimestampedPointCloud<T> (common/timestamped_pointcloud.h:11-42), Rigid3d = Rigid3<double> over Eigen
//     (common/rigid_transform.h:36-128), IntegrationBase (slam/imu_fusion/integration_base.h:62-69), Eigen::Vector3d;
//   * in this repository, instantiated with the dependency-free mirror PODs of msfl/scan_matcher.hpp (whose classes are now thin
//     wrappers of these functions) and, in tests/cpp/adapter_check.cpp, with PCL/Eigen-SHAPED test types that have the reference's
//     32-byte point layout and Eigen's accessor style — both run on the GPU and must agree bit for bit
//     (tests/test_cpp_host_mirror.py).
//
// What a type has to offer (duck-typed; nothing here includes PCL or Eigen):
//   cloud        size(), operator[](i) -> point, push_back(point); points with .x .y .z .intensity (and .ring, .time for the
//                sensor cloud)                                              pcl::PointCloud<T>
//   stamped      members cloud_full_res, cloud_corner_sharp, cloud_corner_less_sharp, cloud_surf_flat, cloud_surf_less_flat that
//                dereference (*p) to a cloud                                TimestampedPointCloud<T>
//   rigid        ToVector7() -> something indexable [0..6] = [t, qx qy qz qw] and default-constructible; a constructor from that
//                same vector type (NO normalisation, rigid_transform.h:47-49) Rigid3d
//   vec3         operator[](0..2) readable / writable                       Eigen::Vector3d, std::array<double, 3>
//   quaternion   .x() .y() .z() .w()  OR  operator[](0..3) in [x y z w] order Eigen::Quaterniond, std::array<double, 4>
//   integration  members sum_dt_buf_ (vector<double>), delta_q_buf_ (vector<quaternion>), delta_p_buf_ (vector<vec3>)
//
// Call sites in the reference (INTEGRATION.md has the three of them):
//   msfl::adapter::Extract(h, laser_cloud_in, g_lidar2imu_transfrom, &scan)            msf_loam_node.cc:170-371
//   msfl::adapter::MatchScan2Scan(h, scan_last, scan_curr, pose_estimate_curr2last)    odometry_scan_matcher.cc:43-285
//   msfl::adapter::MatchScan2Map(h, cloud_map, scan_curr, is_initialized, preintegration, gravity_vector,
//                                pose_estimate_map_scan2world, velocity)               mapping_scan_matcher.cc:61-278 (after :28-59)
// and, for the covariance block of the odometry message (common/rigid_transform.h ToROS leaves it zero):
//   msfl::adapter::SetUncertaintySink(h, &record, min_eigenvalue)  once;  msfl::adapter::CovarianceInParentFrame(pose, record, scale, out36)
// and, where the reference's IMUFactor on the scan-to-map problem is commented out (mapping_scan_matcher.cc:84-94):
//   msfl::adapter::SetPosePrior(h, &prior_record, predicted_pose, sqrt_information)  before MatchScan2Map;  ClearPosePrior(h) after
// and, for the degenerate geometry the reference steps through ("lidar trajectory will drift in illed situation", :84):
//   msfl::adapter::SetDegeneracy(h, &degeneracy_record, min_eigenvalue)  once;  ClearDegeneracy(h) to switch it off
// and, against correspondences that are simply wrong (moved objects; the reference's commented-out RefineByRejectOutliersWithThreshold):
//   msfl::adapter::SetOutlierRejection(h, &rejection_record, MSFL_REJECT_THRESHOLD, 0.2)  once;  ClearOutlierRejection(h) to switch it off
// and, for a health figure of a registration or the verification of a candidate pose against the map of the last MatchScan2Map:
//   msfl::adapter::ScorePoses(h, scan_curr, poses, max_dist) -> std::vector<PoseScore> (Fitness(n_features), Rmse())
// and, for P loop-closure candidates against their P submaps, the submaps indexed once:
//   msfl::adapter::SetPairMaps(h, maps);  ScorePairs(h, scans, poses_per_scan, max_dist);  MatchPairsResident(h, scans, &poses)
// and, where the reference's src/slam/loop_closure is an empty class: which earlier scan looks like this one, and at which yaw
//   msfl::PlaceDatabase places;  places.Add(cloud) per scan;  places.Query(cloud, max_index, n_prefilter, k) -> std::vector<PlaceMatch> (Yaw())
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../msfl_c_api.h"

namespace msfl {
namespace adapter {

template <class...> struct voider { using type = void; };

// the reference aborts through glog CHECK on invariant violations; here: an exception naming the call and the library's message
inline void Check(msfl_status s, msfl_handle* h, const char* what) {
  if (s != MSFL_OK) throw std::runtime_error(std::string(what) + ": " + msfl_status_string(s) + " " + (h ? msfl_last_error(h) : ""));
}

// ---- quaternion -> [x y z w] (Eigen::Quaterniond::coeffs() order)
template <class Q, class = void>
struct QuatXYZW {
  static void Get(const Q& q, double o[4]) { for (int k = 0; k < 4; ++k) o[k] = static_cast<double>(q[k]); }
};
template <class Q>
struct QuatXYZW<Q, typename voider<decltype(std::declval<const Q&>().w())>::type> {
  static void Get(const Q& q, double o[4]) { o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w(); }
};

// ---- rigid <-> 7 doubles.  The reference's ToVector7() is not const-qualified (rigid_transform.h:59): work on a copy.
template <class RigidT>
inline void RigidToArray(const RigidT& r, double o[7]) {
  RigidT c = r;
  const auto v = c.ToVector7();
  for (int k = 0; k < 7; ++k) o[k] = static_cast<double>(v[k]);
}
template <class RigidT>
inline RigidT RigidFromArray(const double a[7]) {
  using V7 = typename std::decay<decltype(std::declval<RigidT&>().ToVector7())>::type;
  V7 v;
  for (int k = 0; k < 7; ++k) v[k] = a[k];
  return RigidT(v);                                                     // no normalisation: an un-stepped pose round-trips bit for bit
}

// ---- clouds -> 16-byte msfl_point {x, y, z, t = intensity} (the reference keeps the relative time in `intensity`, msf_loam_node.cc:152-153)
template <class CloudT>
inline std::vector<msfl_point> Pack(const CloudT& c) {
  std::vector<msfl_point> o(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) { const auto& p = c[i]; o[i] = msfl_point{p.x, p.y, p.z, p.intensity}; }
  return o;
}
template <class CloudT>
inline void PackWithRing(const CloudT& c, std::vector<msfl_point>* pts, std::vector<std::uint16_t>* ring) {
  pts->resize(c.size()); ring->resize(c.size());
  for (std::size_t i = 0; i < c.size(); ++i) {
    const auto& p = c[i];
    (*pts)[i] = msfl_point{p.x, p.y, p.z, p.intensity};
    (*ring)[i] = static_cast<std::uint16_t>(p.ring);
  }
}
// the point type of a cloud, and a point of it from a library point (ring / time only where the type has them)
template <class CloudT>
using PointOf = typename std::decay<decltype(std::declval<const CloudT&>()[0])>::type;
template <class P, class = void>
struct HasRing : std::false_type {};
template <class P>
struct HasRing<P, typename voider<decltype(std::declval<P&>().ring)>::type> : std::true_type {};
template <class P>
inline typename std::enable_if<HasRing<P>::value, P>::type MakePoint(const msfl_point& q, std::uint16_t ring) {
  P p{};
  p.x = q.x; p.y = q.y; p.z = q.z; p.intensity = q.t; p.ring = ring; p.time = q.t;       // time == intensity, msf_loam_node.cc:152-153
  return p;
}
template <class P>
inline typename std::enable_if<!HasRing<P>::value, P>::type MakePoint(const msfl_point& q, std::uint16_t) {
  P p{};
  p.x = q.x; p.y = q.y; p.z = q.z; p.intensity = q.t;
  return p;
}

// ---- RealHandleLaserCloudMessage between pcl::fromROSMsg and AddLaserScan (msf_loam_node.cc:170-371): fills the five clouds of
// `scan` (cleared first); `scan->time`, `frame_id` and the poses stay the caller's.
template <class CloudT, class RigidT, class StampedT>
inline void Extract(msfl_handle* h, const CloudT& laser_cloud_in, const RigidT& lidar2imu, StampedT* scan) {
  std::vector<msfl_point> p; std::vector<std::uint16_t> r;
  PackWithRing(laser_cloud_in, &p, &r);
  const std::size_t n = p.size();
  std::vector<msfl_point> full(n); std::vector<std::uint16_t> ring(n); std::vector<float> curv(n); std::vector<std::uint8_t> label(n);
  std::vector<int> idx[4];
  for (auto& v : idx) v.resize(n);
  msfl_features f{};
  f.full_pts = full.data(); f.full_ring = ring.data(); f.curvature = curv.data(); f.label = label.data();
  f.sharp_idx = idx[0].data(); f.less_sharp_idx = idx[1].data(); f.flat_idx = idx[2].data(); f.less_flat_idx = idx[3].data();
  double ext[7];
  RigidToArray(lidar2imu, ext);
  Check(msfl_extract_features(h, p.data(), r.data(), static_cast<int>(n), ext, &f, MSFL_MEM_HOST), h, "msfl_extract_features");
  using P = PointOf<typename std::decay<decltype(*scan->cloud_full_res)>::type>;
  auto fill = [&](decltype(*scan->cloud_full_res)& out, const int* list, int m) {
    out = typename std::decay<decltype(out)>::type();
    for (int k = 0; k < m; ++k) { const int i = list ? list[k] : k; out.push_back(MakePoint<P>(full[i], ring[i])); }
  };
  fill(*scan->cloud_full_res, nullptr, f.n_full);
  fill(*scan->cloud_corner_sharp, idx[0].data(), f.n_sharp);                 // msf_loam_node.cc:360-364
  fill(*scan->cloud_corner_less_sharp, idx[1].data(), f.n_less_sharp);
  fill(*scan->cloud_surf_flat, idx[2].data(), f.n_flat);
  fill(*scan->cloud_surf_less_flat, idx[3].data(), f.n_less_flat);
}

// ---- scan segmentation in front of Extract (msfl_segment_scan; not in the reference): ground by the slope between neighbouring
// beams, range-image clusters, the small ones dropped.  classes: one MSFL_SEG_* per point of `cloud`; masked: the cloud with the
// points outside cfg.keep_classes set to NaN (x, y, z; everything else as it was) -- hand it to Extract, whose invalid-point pass
// removes them.  Either output may be null.  cfg == nullptr: msfl_segment_default_config.
template <class CloudT>
inline msfl_segment_info Segment(msfl_handle* h, const CloudT& cloud, const msfl_segment_config* cfg, std::vector<std::uint8_t>* classes,
                                 CloudT* masked) {
  std::vector<msfl_point> p; std::vector<std::uint16_t> r;
  PackWithRing(cloud, &p, &r);
  const std::size_t n = p.size();
  std::vector<std::uint8_t> cls(n + 1);
  std::vector<msfl_point> m(masked ? n + 1 : 0);
  msfl_segment_info info{};
  Check(msfl_segment_scan(h, p.data(), r.data(), static_cast<int>(n), cfg, cls.data(), nullptr, masked ? m.data() : nullptr, &info, MSFL_MEM_HOST), h,
        "msfl_segment_scan");
  cls.resize(n);
  if (masked) {
    *masked = cloud;
    for (std::size_t i = 0; i < n; ++i) { auto& q = (*masked)[i]; q.x = m[i].x; q.y = m[i].y; q.z = m[i].z; }
  }
  if (classes) classes->swap(cls);
  return info;
}

// ---- OdometryScanMatcher::MatchScan2Scan (odometry_scan_matcher.cc:43-285).  Returns false exactly where the reference does
// (< 10 correspondences, :262-267); the pose then holds the outer iterations completed so far.
template <class StampedT, class RigidT>
inline bool MatchScan2Scan(msfl_handle* h, const StampedT& scan_last, const StampedT& scan_curr, RigidT* pose_estimate_curr2last,
                           msfl_match_info* info = nullptr) {
  std::vector<msfl_point> p[4]; std::vector<std::uint16_t> r[4];
  PackWithRing(*scan_last.cloud_corner_less_sharp, &p[0], &r[0]);
  PackWithRing(*scan_last.cloud_surf_less_flat, &p[1], &r[1]);
  PackWithRing(*scan_curr.cloud_corner_sharp, &p[2], &r[2]);
  PackWithRing(*scan_curr.cloud_surf_flat, &p[3], &r[3]);
  msfl_ring_cloud c[4];
  for (int k = 0; k < 4; ++k) c[k] = msfl_ring_cloud{p[k].data(), r[k].data(), static_cast<int>(p[k].size())};
  double v[7];
  RigidToArray(*pose_estimate_curr2last, v);
  const msfl_status s = msfl_match_scan2scan(h, &c[0], &c[1], &c[2], &c[3], v, info, MSFL_MEM_HOST);
  if (s != MSFL_OK && s != MSFL_TOO_FEW_CORRESPONDENCES) Check(s, h, "msfl_match_scan2scan");
  *pose_estimate_curr2last = RigidFromArray<RigidT>(v);
  return s == MSFL_OK;
}

// ---- what GetDeltaQP reads of an IntegrationBase (scan_undistortion.cc:22-42), flattened for msfl_preintegration
struct PreintegrationView {
  std::vector<double> dq, dp;
  msfl_preintegration pre{};
  template <class IntegrationT>
  explicit PreintegrationView(const IntegrationT& ib) {
    const std::size_t n = ib.sum_dt_buf_.size();
    if (n < 2 || ib.delta_q_buf_.size() != n || ib.delta_p_buf_.size() != n)
      throw std::invalid_argument("pre-integration needs >= 2 samples and buffers of equal length");
    dq.resize(4 * n); dp.resize(3 * n);
    for (std::size_t i = 0; i < n; ++i) {
      using Q = typename std::decay<decltype(ib.delta_q_buf_[i])>::type;
      QuatXYZW<Q>::Get(ib.delta_q_buf_[i], &dq[4 * i]);
      for (int k = 0; k < 3; ++k) dp[3 * i + k] = static_cast<double>(ib.delta_p_buf_[i][k]);
    }
    pre.sum_dt = ib.sum_dt_buf_.data(); pre.delta_q = dq.data(); pre.delta_p = dp.data(); pre.n = static_cast<int>(n);
  }
};

// ---- MappingScanMatcher::MatchScan2Map (mapping_scan_matcher.cc:61-278).
// Only cloud_corner_less_sharp and cloud_surf_less_flat of both arguments are read (:71-72,109,179).
//   !is_initialized : the LiDAR-only branch (:96,123); preintegration / gravity_vector / velocity are not read.
//    is_initialized : the caller has ALREADY run its IMU-only pre-solve (:28-59, a 15-residual Ceres problem that stays on the
//                     maintainer's side) and stored pose_j / bias_j.head<3>() in *pose / *velocity (:58-59); GetDeltaQP per
//                     feature point (:112-116,182-186) runs on the GPU, then the Deskew factors with the velocity block held
//                     constant (:94).  A feature time outside the pre-integration span aborts in the reference (CHECK,
//                     scan_undistortion.cc:26-30): exception here.
// Always returns true like the reference (:277) unless the map is unusable (MAP_TOO_SMALL: the caller's gate
// laser_mapping.cc:284-285 normally prevents that) -> false, pose untouched.
template <class StampedT, class IntegrationT, class Vec3T, class RigidT>
inline bool MatchScan2Map(msfl_handle* h, const StampedT& cloud_map, const StampedT& scan_curr, const bool is_initialized,
                          const std::shared_ptr<IntegrationT>& preintegration, const Vec3T& gravity_vector,
                          RigidT* pose_estimate_map_scan2world, Vec3T* velocity, msfl_match_info* info = nullptr) {
  const std::vector<msfl_point> mc = Pack(*cloud_map.cloud_corner_less_sharp);
  const std::vector<msfl_point> ms = Pack(*cloud_map.cloud_surf_less_flat);
  Check(msfl_set_map(h, mc.data(), static_cast<int>(mc.size()), ms.data(), static_cast<int>(ms.size()), MSFL_MEM_HOST), h,
        "msfl_set_map");                                                 // the two kd-tree builds, :66-73
  const std::vector<msfl_point> c = Pack(*scan_curr.cloud_corner_less_sharp);
  const std::vector<msfl_point> s = Pack(*scan_curr.cloud_surf_less_flat);
  double v[7];
  RigidToArray(*pose_estimate_map_scan2world, v);
  msfl_status st;
  if (!is_initialized) {
    st = msfl_match_scan2map(h, c.data(), static_cast<int>(c.size()), s.data(), static_cast<int>(s.size()), v, info, MSFL_MEM_HOST);
  } else {
    if (!preintegration || !velocity) throw std::invalid_argument("MatchScan2Map: is_initialized needs a pre-integration and a velocity");
    const PreintegrationView pv(*preintegration);
    std::vector<double> cdq(4 * c.size()), cdp(3 * c.size()), sdq(4 * s.size()), sdp(3 * s.size());
    if (!c.empty()) Check(msfl_delta_qp(h, &pv.pre, c.data(), static_cast<int>(c.size()), cdq.data(), cdp.data(), MSFL_MEM_HOST), h, "msfl_delta_qp (corner)");
    if (!s.empty()) Check(msfl_delta_qp(h, &pv.pre, s.data(), static_cast<int>(s.size()), sdq.data(), sdp.data(), MSFL_MEM_HOST), h, "msfl_delta_qp (surf)");
    msfl_deskew d;
    d.corner_dq = c.empty() ? nullptr : cdq.data(); d.corner_dp = c.empty() ? nullptr : cdp.data();
    d.surf_dq = s.empty() ? nullptr : sdq.data(); d.surf_dp = s.empty() ? nullptr : sdp.data();
    for (int a = 0; a < 3; ++a) { d.velocity[a] = static_cast<double>((*velocity)[a]); d.gravity[a] = static_cast<double>(gravity_vector[a]); }
    st = msfl_match_scan2map_deskew(h, c.data(), static_cast<int>(c.size()), s.data(), static_cast<int>(s.size()), &d, v, info);
  }
  if (st == MSFL_MAP_TOO_SMALL) return false;
  Check(st, h, "msfl_match_scan2map");
  *pose_estimate_map_scan2world = RigidFromArray<RigidT>(v);               // :271 / :268 (velocity unchanged: its block is constant, :94)
  return true;
}

// ---- fitness of a scan at candidate poses against the map the handle holds (msfl_score_poses; not in the reference, whose only
// health figures are the solver's own).  Call it after MatchScan2Map (the map of that call is still resident) with the returned
// pose to grade the registration, or with a candidate pose (a loop closure, a GPS fix) before accepting it.  Only
// cloud_corner_less_sharp and cloud_surf_less_flat of `scan` are read; `poses` is any container of rigids (size(), operator[]).
struct PoseScore : msfl_pose_score {
  // inlier fraction over n_features = corner + surf features of the scan
  double Fitness(std::size_t n_features) const {
    return n_features ? (static_cast<double>(inliers[0]) + static_cast<double>(inliers[1])) / static_cast<double>(n_features) : 0.0;
  }
  // root mean squared inlier distance in metres (NaN without inliers)
  double Rmse() const {
    const double n = static_cast<double>(inliers[0]) + static_cast<double>(inliers[1]);
    const double sum = (static_cast<double>(sum_sq_q32[0]) + static_cast<double>(sum_sq_q32[1])) / 4294967296.0;
    return n > 0 ? std::sqrt(sum / n) : std::nan("");
  }
};
template <class StampedT, class RigidVecT>
inline std::vector<PoseScore> ScorePoses(msfl_handle* h, const StampedT& scan, const RigidVecT& poses, double max_dist) {
  const std::vector<msfl_point> c = Pack(*scan.cloud_corner_less_sharp);
  const std::vector<msfl_point> s = Pack(*scan.cloud_surf_less_flat);
  std::vector<double> v(7 * poses.size());
  for (std::size_t i = 0; i < poses.size(); ++i) RigidToArray(poses[i], v.data() + 7 * i);
  std::vector<PoseScore> out(poses.size());
  static_assert(sizeof(PoseScore) == sizeof(msfl_pose_score), "PoseScore adds no member");
  Check(msfl_score_poses(h, c.data(), static_cast<int>(c.size()), s.data(), static_cast<int>(s.size()), v.data(), static_cast<int>(poses.size()),
                         max_dist, out.data(), nullptr, nullptr, MSFL_MEM_HOST), h, "msfl_score_poses");
  return out;
}

// ---- where in the resident map is this scan, given only a rough guess (msfl_search_poses, msfl_relocalize; not in the reference,
// whose matcher needs a guess inside its basin).  SearchPoses: the best `capacity` peaks of the hit-count lattice round `guess`,
// best first.  Relocalize: those candidates scored exactly, the best n_refine registered and scored again, best first; a record's
// `accepted` says whether its refined inlier fraction reaches min_fitness.  Call them after MatchScan2Map (its map is resident).
inline msfl_search_config SearchDefaultConfig() {
  msfl_search_config c;
  msfl_search_default_config(&c);
  return c;
}
template <class StampedT, class RigidT>
inline std::vector<msfl_pose_candidate> SearchPoses(msfl_handle* h, const StampedT& scan, const RigidT& guess, const msfl_search_config& cfg,
                                                    int capacity) {
  const std::vector<msfl_point> c = Pack(*scan.cloud_corner_less_sharp);
  const std::vector<msfl_point> s = Pack(*scan.cloud_surf_less_flat);
  double g[7];
  RigidToArray(guess, g);
  std::vector<msfl_pose_candidate> out(static_cast<std::size_t>(capacity > 0 ? capacity : 0));
  int n = 0;
  Check(msfl_search_poses(h, c.data(), static_cast<int>(c.size()), s.data(), static_cast<int>(s.size()), g, &cfg, out.data(), capacity, &n, nullptr,
                          MSFL_MEM_HOST), h, "msfl_search_poses");
  out.resize(static_cast<std::size_t>(n));
  return out;
}
template <class StampedT, class RigidT>
inline std::vector<msfl_reloc_result> Relocalize(msfl_handle* h, const StampedT& scan, const RigidT& guess, const msfl_search_config& cfg,
                                                 int n_candidates, double max_dist, int n_refine, double min_fitness) {
  const std::vector<msfl_point> c = Pack(*scan.cloud_corner_less_sharp);
  const std::vector<msfl_point> s = Pack(*scan.cloud_surf_less_flat);
  double g[7];
  RigidToArray(guess, g);
  std::vector<msfl_reloc_result> out(static_cast<std::size_t>(n_refine > 0 ? n_refine : 0));
  int n = 0;
  Check(msfl_relocalize(h, c.data(), static_cast<int>(c.size()), s.data(), static_cast<int>(s.size()), g, &cfg, n_candidates, max_dist, n_refine,
                        min_fitness, out.data(), n_refine, &n, MSFL_MEM_HOST), h, "msfl_relocalize");
  out.resize(static_cast<std::size_t>(n));
  return out;
}

// ---- P (map, scan) pairs with the pairs' maps kept resident (msfl_set_pair_maps, msfl_score_pairs, msfl_match_pairs_resident; not in
// the reference, which registers one scan against one map per call): loop-closure candidates against their submaps.  `maps` / `scans`
// are containers (size(), operator[]) of stamped clouds, of which cloud_corner_less_sharp and cloud_surf_less_flat are read.
template <class StampedVecT>
inline void PackPairs(const StampedVecT& clouds, std::vector<msfl_point>* corner, std::vector<int>* corner_off, std::vector<msfl_point>* surf,
                      std::vector<int>* surf_off) {
  corner->clear(); surf->clear(); corner_off->assign(1, 0); surf_off->assign(1, 0);
  for (std::size_t p = 0; p < clouds.size(); ++p) {
    const std::vector<msfl_point> c = Pack(*clouds[p].cloud_corner_less_sharp);
    const std::vector<msfl_point> s = Pack(*clouds[p].cloud_surf_less_flat);
    corner->insert(corner->end(), c.begin(), c.end()); surf->insert(surf->end(), s.begin(), s.end());
    corner_off->push_back(static_cast<int>(corner->size())); surf_off->push_back(static_cast<int>(surf->size()));
  }
}
// The P maps indexed, one grid per pair; they stay resident until the next MatchScan2Map (msfl_set_map) or SetPairMaps.
template <class StampedVecT>
inline void SetPairMaps(msfl_handle* h, const StampedVecT& maps) {
  std::vector<msfl_point> mc, ms; std::vector<int> mco, mso;
  PackPairs(maps, &mc, &mco, &ms, &mso);
  Check(msfl_set_pair_maps(h, static_cast<int>(maps.size()), mc.data(), mco.data(), ms.data(), mso.data(), MSFL_MEM_HOST), h, "msfl_set_pair_maps");
}
// scans[p] at each of poses[p] (a container of rigids, may be empty) against pair map p: out[p][k] grades poses[p][k].
template <class StampedVecT, class RigidVecVecT>
inline std::vector<std::vector<PoseScore>> ScorePairs(msfl_handle* h, const StampedVecT& scans, const RigidVecVecT& poses, double max_dist) {
  if (poses.size() != scans.size()) throw std::invalid_argument("ScorePairs: one pose list per scan");
  std::vector<msfl_point> c, s; std::vector<int> co, so, po(1, 0);
  PackPairs(scans, &c, &co, &s, &so);
  std::vector<double> v;
  for (std::size_t p = 0; p < poses.size(); ++p) {
    for (std::size_t k = 0; k < poses[p].size(); ++k) { v.resize(v.size() + 7); RigidToArray(poses[p][k], v.data() + v.size() - 7); }
    po.push_back(static_cast<int>(v.size() / 7));
  }
  std::vector<PoseScore> flat(v.size() / 7);
  Check(msfl_score_pairs(h, static_cast<int>(scans.size()), c.data(), co.data(), s.data(), so.data(), v.data(), po.data(), max_dist, flat.data(),
                         nullptr, nullptr, MSFL_MEM_HOST), h, "msfl_score_pairs");
  std::vector<std::vector<PoseScore>> out(scans.size());
  for (std::size_t p = 0; p < scans.size(); ++p) out[p].assign(flat.begin() + po[p], flat.begin() + po[p + 1]);
  return out;
}
// SearchPoses against the pair index: scans[p] round guesses[p] against pair map p, all pairs in one call (msfl_search_pairs);
// out[p]: the best `capacity` peaks of pair p's lattice, best first.  One cfg serves all pairs (a pair's yaw goes into its guess).
template <class StampedVecT, class RigidVecT>
inline std::vector<std::vector<msfl_pose_candidate>> SearchPairs(msfl_handle* h, const StampedVecT& scans, const RigidVecT& guesses,
                                                                 const msfl_search_config& cfg, int capacity) {
  if (guesses.size() != scans.size()) throw std::invalid_argument("SearchPairs: one guess per scan");
  std::vector<msfl_point> c, s; std::vector<int> co, so;
  PackPairs(scans, &c, &co, &s, &so);
  std::vector<double> g(7 * scans.size());
  for (std::size_t p = 0; p < scans.size(); ++p) RigidToArray(guesses[p], g.data() + 7 * p);
  const std::size_t K = static_cast<std::size_t>(capacity > 0 ? capacity : 0);
  std::vector<msfl_pose_candidate> flat(K * scans.size());
  std::vector<int> n(scans.size(), 0);
  Check(msfl_search_pairs(h, static_cast<int>(scans.size()), c.data(), co.data(), s.data(), so.data(), g.data(), &cfg, flat.data(), capacity, n.data(),
                          nullptr, MSFL_MEM_HOST), h, "msfl_search_pairs");
  std::vector<std::vector<msfl_pose_candidate>> out(scans.size());
  for (std::size_t p = 0; p < scans.size(); ++p) out[p].assign(flat.begin() + p * K, flat.begin() + p * K + n[p]);
  return out;
}
// scans[p] registered against pair map p from (*poses)[p], which it replaces; per pair MSFL_OK or MSFL_MAP_TOO_SMALL (pose untouched).
// The index is not consumed: call it again, or ScorePairs on the result.  `info`: null or one record per pair.
template <class StampedVecT, class RigidVecT>
inline std::vector<int> MatchPairsResident(msfl_handle* h, const StampedVecT& scans, RigidVecT* poses, msfl_match_info* info = nullptr) {
  if (!poses || poses->size() != scans.size()) throw std::invalid_argument("MatchPairsResident: one pose per scan");
  std::vector<msfl_point> c, s; std::vector<int> co, so;
  PackPairs(scans, &c, &co, &s, &so);
  std::vector<double> v(7 * scans.size());
  for (std::size_t p = 0; p < scans.size(); ++p) RigidToArray((*poses)[p], v.data() + 7 * p);
  std::vector<int> status(scans.size(), 0);
  Check(msfl_match_pairs_resident(h, static_cast<int>(scans.size()), c.data(), co.data(), s.data(), so.data(), v.data(), status.data(), info,
                                  MSFL_MEM_HOST), h, "msfl_match_pairs_resident");
  using RigidT = typename std::decay<decltype((*poses)[0])>::type;
  for (std::size_t p = 0; p < scans.size(); ++p) (*poses)[p] = RigidFromArray<RigidT>(v.data() + 7 * p);
  return status;
}

// ---- HybridGrid::GetSurroundedCloud / InsertScan (hybrid_grid.cc:462-534; callers laser_mapping.cc:273-278,330-338) on a
// device-resident store created with msfl_grid_create(h, resolution, leaf, &g)
template <class CloudT, class RigidT>
inline void GetSurroundedCloud(msfl_handle* h, msfl_grid* g, const CloudT& scan, const RigidT& pose, CloudT* out) {
  const std::vector<msfl_point> in = Pack(scan);
  int n_pts = 0, n_cells = 0;
  Check(msfl_grid_size(g, &n_pts, &n_cells), h, "msfl_grid_size");
  std::vector<msfl_point> buf(static_cast<std::size_t>(n_pts > 0 ? n_pts : 1));
  int n_out = 0;
  double v[7];
  RigidToArray(pose, v);
  Check(msfl_grid_get_surrounded(g, in.data(), static_cast<int>(in.size()), v, buf.data(), n_pts, &n_out, MSFL_MEM_HOST), h,
        "msfl_grid_get_surrounded");
  *out = CloudT();
  for (int i = 0; i < n_out; ++i) out->push_back(MakePoint<PointOf<CloudT>>(buf[i], 0));
}
template <class CloudT>
inline void InsertScan(msfl_handle* h, msfl_grid* g, const CloudT& scan) {
  if (scan.size() == 0) return;                                           // hybrid_grid.cc:504
  const std::vector<msfl_point> in = Pack(scan);
  Check(msfl_grid_insert_scan(g, in.data(), static_cast<int>(in.size()), MSFL_MEM_HOST), h, "msfl_grid_insert_scan");
}

// ---- DoUndistort of LaserMapping::Run (laser_mapping.cc:197-211) and ScanUndistortionUtils::DoUndistort
// (scan_undistortion.cc:5-19) on one cloud in place (x, y, z rewritten; intensity / ring / time kept)
template <class CloudT, class IntegrationT, class QuatT, class Vec3T>
inline void DeskewCloud(msfl_handle* h, const IntegrationT& preintegration, const QuatT& rot_odom_scan2world, const Vec3T& velocity,
                        const Vec3T& gravity, CloudT* cloud) {
  std::vector<msfl_point> pts = Pack(*cloud);
  const PreintegrationView pv(preintegration);
  double q[4], vel[3], g[3];
  QuatXYZW<QuatT>::Get(rot_odom_scan2world, q);
  for (int a = 0; a < 3; ++a) { vel[a] = static_cast<double>(velocity[a]); g[a] = static_cast<double>(gravity[a]); }
  Check(msfl_deskew_cloud(h, &pv.pre, pts.data(), static_cast<int>(pts.size()), q, vel, g, MSFL_MEM_HOST), h, "msfl_deskew_cloud");
  for (std::size_t i = 0; i < pts.size(); ++i) { auto& p = (*cloud)[i]; p.x = pts[i].x; p.y = pts[i].y; p.z = pts[i].z; }
}
template <class CloudT, class IntegrationT>
inline void UndistortCloud(msfl_handle* h, const IntegrationT& preintegration, CloudT* cloud) {
  std::vector<msfl_point> pts = Pack(*cloud);
  const PreintegrationView pv(preintegration);
  Check(msfl_undistort_cloud(h, &pv.pre, pts.data(), static_cast<int>(pts.size()), MSFL_MEM_HOST), h, "msfl_undistort_cloud");
  for (std::size_t i = 0; i < pts.size(); ++i) { auto& p = (*cloud)[i]; p.x = pts[i].x; p.y = pts[i].y; p.z = pts[i].z; }
}

// ---- uncertainty of the last registration (msfl_match_uncertainty).  `record` must outlive the handle's matcher calls (one
// registration per call on this side of the boundary, so a sink of one record); nullptr turns the output off again.
inline void SetUncertaintySink(msfl_handle* h, msfl_match_uncertainty* record, double min_eigenvalue = 0.0) {
  Check(msfl_set_uncertainty(h, record, record ? 1 : 0, MSFL_MEM_HOST, min_eigenvalue), h, "msfl_set_uncertainty");
}

// ---- Gaussian prior on the pose of the handle's NEXT registrations (msfl_pose_prior; docs/kernels/prior.md): what the reference's
// commented-out IMUFactor on the scan-to-map problem (mapping_scan_matcher.cc:84-94) was for.  `record` must outlive the handle's
// matcher calls (the library keeps the pointer; one registration per call on this side, so one record); nullptr turns it off.
// sqrt_information: row-major 6 x 6 L with information = L^T L, in the tangent order [dt, dtheta] of msfl_match_uncertainty; a
// matrix type with operator()(i, j) (Eigen::Matrix<double, 6, 6>) or a flat row-major operator[](6 * i + j).
template <class M, class = void>
struct Mat6 {
  static double Get(const M& m, int i, int j) { return static_cast<double>(m[static_cast<std::size_t>(6 * i + j)]); }
};
template <class M>
struct Mat6<M, typename voider<decltype(std::declval<const M&>()(0, 0))>::type> {
  static double Get(const M& m, int i, int j) { return static_cast<double>(m(i, j)); }
};
template <class RigidT, class M>
inline void SetPosePrior(msfl_handle* h, msfl_pose_prior* record, const RigidT& mean, const M& sqrt_information) {
  RigidToArray(mean, record->pose);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) record->sqrt_information[6 * i + j] = Mat6<M>::Get(sqrt_information, i, j);
  Check(msfl_set_pose_prior(h, record, 1, MSFL_MEM_HOST), h, "msfl_set_pose_prior");
}
inline void ClearPosePrior(msfl_handle* h) { Check(msfl_set_pose_prior(h, nullptr, 0, MSFL_MEM_HOST), h, "msfl_set_pose_prior"); }

// ---- degeneracy-aware solve (msfl_set_degeneracy): eigen-directions of a solve's entry matrix below min_eigenvalue stay at the guess.
// `record` (may be null) receives the last call's msfl_degeneracy_record and must outlive the handle's matcher calls.
inline void SetDegeneracy(msfl_handle* h, msfl_degeneracy_record* record, double min_eigenvalue) {
  Check(msfl_set_degeneracy(h, 1, min_eigenvalue, record, record ? 1 : 0, MSFL_MEM_HOST), h, "msfl_set_degeneracy");
}
inline void ClearDegeneracy(msfl_handle* h) { Check(msfl_set_degeneracy(h, 0, 0.0, nullptr, 0, MSFL_MEM_HOST), h, "msfl_set_degeneracy"); }

// ---- outlier rejection in front of the solve (msfl_set_outlier_rejection).  mode MSFL_REJECT_THRESHOLD: `value` is the residual norm
// above which a correspondence goes (the reference's constant: 0.2); MSFL_REJECT_FRACTION: the fraction of a scan's correspondences
// that goes.  `record` (may be null) receives the last call's msfl_rejection_record and must outlive the handle's matcher calls.
inline void SetOutlierRejection(msfl_handle* h, msfl_rejection_record* record, int mode, double value, int which = MSFL_REJECT_LAST_OUTER) {
  msfl_outlier_rejection cfg{};
  cfg.mode = mode;
  cfg.threshold = mode == MSFL_REJECT_THRESHOLD ? value : 0.0;
  cfg.fraction = mode == MSFL_REJECT_FRACTION ? value : 0.0;
  cfg.which = which;
  Check(msfl_set_outlier_rejection(h, &cfg, record, record ? 1 : 0, MSFL_MEM_HOST), h, "msfl_set_outlier_rejection");
}
inline void ClearOutlierRejection(msfl_handle* h) {
  Check(msfl_set_outlier_rejection(h, nullptr, nullptr, 0, MSFL_MEM_HOST), h, "msfl_set_outlier_rejection");
}

// covariance (row-major 6 x 6, symmetric positive definite, tangent order [dt, dtheta]) -> L with L^T L = covariance^-1: the
// inverse of the lower Cholesky factor C of the covariance (covariance = C C^T, so its inverse is C^-T C^-1).  Host side, a few
// hundred flops.  Returns false (out untouched) when the matrix is not positive definite.
inline bool SqrtInformationFromCovariance(const double covariance[36], double out[36]) {
  double C[6][6] = {};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = covariance[6 * i + j];
      for (int k = 0; k < j; ++k) s -= C[i][k] * C[j][k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        C[i][i] = std::sqrt(s);
      } else {
        C[i][j] = s / C[j][j];
      }
    }
  double L[6][6] = {};                                                   // L = C^-1, lower triangular, column by column
  for (int j = 0; j < 6; ++j) {
    L[j][j] = 1.0 / C[j][j];
    for (int i = j + 1; i < 6; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= C[i][k] * L[k][j];
      L[i][j] = s / C[i][i];
    }
  }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) out[6 * i + j] = L[i][j];
  return true;
}

// out (row-major 6 x 6) = scale * A * unc.covariance * A^T with A = diag(I, R(pose)): the tangent space of the solve rotates about
// the BODY axes (q = q * dq), geometry_msgs::PoseWithCovariance wants rotations about the fixed parent axes, in the same
// [x y z, rot x y z] order.  `scale`: unc.sigma2, or the variance of the caller's own sensor model (the covariance is for
// unit-variance residuals).  This is the array to copy into PoseWithCovariance::covariance.
template <class RigidT>
inline void CovarianceInParentFrame(const RigidT& pose, const msfl_match_uncertainty& unc, double scale, double out[36]) {
  double v[7];
  RigidToArray(pose, v);
  const double x = v[3], y = v[4], z = v[5], w = v[6];
  const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                          {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                          {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
  const double* S = unc.covariance;
  double M[6][6];                                                        // A * S: the rotation rows turned
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
      M[i][j] = i < 3 ? S[6 * i + j] : R[i - 3][0] * S[18 + j] + R[i - 3][1] * S[24 + j] + R[i - 3][2] * S[30 + j];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
      out[6 * i + j] = scale * (j < 3 ? M[i][j] : M[i][3] * R[j - 3][0] + M[i][4] * R[j - 3][1] + M[i][5] * R[j - 3][2]);
}

}  // namespace adapter

// ---- place recognition (msfl_places_*): a database of polar scan descriptors on the device, independent of every matcher handle.
struct PlaceMatch : msfl_place_match {
  bool Valid() const { return index >= 0; }
  // the yaw between the two visits that `shift` stands for, radians in (-pi, pi]
  double Yaw(int n_sector) const {
    const double two_pi = 6.283185307179586476925286766559;
    const double a = two_pi * static_cast<double>(((shift % n_sector) + n_sector) % n_sector) / static_cast<double>(n_sector);
    return a > 0.5 * two_pi ? a - two_pi : a;
  }
};

class PlaceDatabase {
 public:
  explicit PlaceDatabase(int device = 0, const msfl_place_config* config = nullptr) {
    if (config) cfg_ = *config; else msfl_places_default_config(&cfg_);
    Check(msfl_places_create(&cfg_, device, &p_), "msfl_places_create");
  }
  ~PlaceDatabase() { msfl_places_destroy(p_); }
  PlaceDatabase(const PlaceDatabase&) = delete;
  PlaceDatabase& operator=(const PlaceDatabase&) = delete;

  const msfl_place_config& config() const { return cfg_; }
  int size() const { return msfl_places_size(p_); }
  msfl_places* get() const { return p_; }

  // describes the cloud (any point type with x, y, z, intensity) and appends it; returns its index
  template <class CloudT>
  int Add(const CloudT& cloud) {
    const std::vector<msfl_point> pts = adapter::Pack(cloud);
    const int off[2] = {0, static_cast<int>(pts.size())};
    int first = -1;
    Check(msfl_places_add(p_, pts.data(), off, 1, MSFL_MEM_HOST, &first), "msfl_places_add");
    return first;
  }

  // the k best entries below max_index (negative: every entry) for the cloud, ordered by (distance, index); n_prefilter as in the C ABI
  template <class CloudT>
  std::vector<PlaceMatch> Query(const CloudT& cloud, int max_index = -1, int n_prefilter = 0, int k = 1) {
    const std::vector<msfl_point> pts = adapter::Pack(cloud);
    const int off[2] = {0, static_cast<int>(pts.size())};
    std::vector<PlaceMatch> out(static_cast<std::size_t>(k > 0 ? k : 0));
    static_assert(sizeof(PlaceMatch) == sizeof(msfl_place_match), "PlaceMatch adds no member");
    Check(msfl_places_query(p_, pts.data(), off, 1, max_index >= 0 ? &max_index : nullptr, n_prefilter, k, out.data(), MSFL_MEM_HOST),
          "msfl_places_query");
    return out;
  }

  // as Query, for an entry that is stored already (entry i against max_index = i - 50: the loop-closure search)
  std::vector<PlaceMatch> QueryEntry(int entry, int max_index = -1, int n_prefilter = 0, int k = 1) {
    std::vector<PlaceMatch> out(static_cast<std::size_t>(k > 0 ? k : 0));
    Check(msfl_places_query_entries(p_, &entry, 1, max_index >= 0 ? &max_index : nullptr, n_prefilter, k, out.data(), MSFL_MEM_HOST),
          "msfl_places_query_entries");
    return out;
  }

  double Yaw(const msfl_place_match& m) const { return static_cast<const PlaceMatch&>(m).Yaw(cfg_.n_sector); }

 private:
  void Check(msfl_status s, const char* what) const {
    if (s != MSFL_OK) throw std::runtime_error(std::string(what) + ": " + msfl_status_string(s) + " " + (p_ ? msfl_places_last_error(p_) : ""));
  }
  msfl_place_config cfg_{};
  msfl_places* p_ = nullptr;
};

}  // namespace msfl
