// msfl/pose_graph.hpp — C++ face of msfl_graph_* (include/msfl_c_api.h, docs/kernels/graph.md):
//   msfl::PoseGraph      RAII over the C ABI
//   msfl::PoseGraphEdge  the record of a loop-closure edge, the role of PoseGraphEdgeFactor (loop_closure/pose_graph_factor.h)
//   msfl::PoseGraphEdgeInfo  the same edge weighted by the information matrix of the registration that measured it
//   msfl::PoseGraph::Marginals, msfl::RelativeCovariance  covariance blocks of the solved poses and of a relative pose between two
//   msfl::GpsFusion      the reference's class (slam/gps_fusion/gps_fusion.h, gps_fusion.cc:16-97): AddFixedPoint, AddLocalPose, Optimize
// Header only, C++14.
#ifndef MSFL_POSE_GRAPH_HPP_
#define MSFL_POSE_GRAPH_HPP_

#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "scan_matcher.hpp"

namespace msfl {

// A relative-pose edge between nodes i and j whose measurement is pose_i^-1 * pose_j (RelativePoseFactor's constructor,
// gps_factor.h:32-34), weighted by scalar sigmas for rotation and translation.
inline msfl_graph_edge PoseGraphEdge(int i, int j, const Rigid3d& pose_i, const Rigid3d& pose_j, double sr, double st) {
  msfl_graph_edge e{};
  e.i = i; e.j = j;
  const std::array<double, 7> z = (pose_i.inverse() * pose_j).ToVector7();
  std::copy(z.begin(), z.end(), e.z);
  e.sr = sr; e.st = st;
  return e;
}
// The same from a measured relative pose (what a verified and refined loop closure delivers).
inline msfl_graph_edge PoseGraphEdge(int i, int j, const Rigid3d& pose_ij, double sr, double st) {
  msfl_graph_edge e{};
  e.i = i; e.j = j;
  const std::array<double, 7> z = pose_ij.ToVector7();
  std::copy(z.begin(), z.end(), e.z);
  e.sr = sr; e.st = st;
  return e;
}

// The information-weighted edge a registration gives: pose_j is the registered pose, `unc` its record (msfl_set_uncertainty), `scale` the
// variance factor (unc.sigma2, or a sensor model's); pose_i is taken as exact.  Directions the record counts degenerate get no weight.
inline msfl_graph_edge_info PoseGraphEdgeInfo(int i, int j, const Rigid3d& pose_i, const Rigid3d& pose_j, const msfl_match_uncertainty& unc,
                                              double scale) {
  msfl_graph_edge_info e{};
  const std::array<double, 7> a = pose_i.ToVector7(), b = pose_j.ToVector7();
  const msfl_status st = msfl_graph_edge_from_uncertainty(i, j, a.data(), b.data(), &unc, scale, &e);
  if (st != MSFL_OK) throw std::invalid_argument(std::string("msfl_graph_edge_from_uncertainty: ") + msfl_status_string(st));
  return e;
}

// Covariance of pose_a^-1 * pose_b in the tangent of an information edge, from the joint marginal PoseGraph::Marginals delivers for
// (a, a), (a, b), (b, b): what a loop-candidate gate adds to the candidate's own (L^T L)^-1.
inline std::array<double, 36> RelativeCovariance(const Rigid3d& pose_a, const Rigid3d& pose_b, const std::array<double, 36>& S_aa,
                                                 const std::array<double, 36>& S_ab, const std::array<double, 36>& S_bb) {
  const std::array<double, 7> a = pose_a.ToVector7(), b = pose_b.ToVector7();
  std::array<double, 36> out{};
  const msfl_status st = msfl_graph_relative_covariance(a.data(), b.data(), S_aa.data(), S_ab.data(), S_bb.data(), out.data());
  if (st != MSFL_OK) throw std::invalid_argument(std::string("msfl_graph_relative_covariance: ") + msfl_status_string(st));
  return out;
}

class PoseGraph {
 public:
  explicit PoseGraph(const msfl_graph_config* config = nullptr, int device = 0) {
    const msfl_status st = msfl_graph_create(config, device, &g_);
    if (st != MSFL_OK) throw std::runtime_error(std::string("msfl_graph_create: ") + msfl_status_string(st));
  }
  ~PoseGraph() { msfl_graph_destroy(g_); }
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;
  static msfl_graph_config DefaultConfig() { msfl_graph_config c; msfl_graph_default_config(&c); return c; }

  int AddNode(const Rigid3d& pose) {
    const std::array<double, 7> v = pose.ToVector7();
    int first = -1;
    Check(msfl_graph_add_nodes(g_, v.data(), 1, MSFL_MEM_HOST, &first), "msfl_graph_add_nodes");
    return first;
  }
  int AddNodes(const std::vector<Rigid3d>& poses) {
    std::vector<double> v;
    for (const Rigid3d& p : poses) { const std::array<double, 7> a = p.ToVector7(); v.insert(v.end(), a.begin(), a.end()); }
    int first = -1;
    Check(msfl_graph_add_nodes(g_, v.data(), static_cast<int>(poses.size()), MSFL_MEM_HOST, &first), "msfl_graph_add_nodes");
    return first;
  }
  // n poses of 7 doubles already on the device (msfl_slam results)
  int AddDeviceNodes(const double* device_poses, int n) {
    int first = -1;
    Check(msfl_graph_add_nodes(g_, device_poses, n, MSFL_MEM_DEVICE, &first), "msfl_graph_add_nodes");
    return first;
  }
  void AddEdges(const std::vector<msfl_graph_edge>& e) { Check(msfl_graph_add_edges(g_, e.data(), static_cast<int>(e.size())), "msfl_graph_add_edges"); }
  void AddEdge(const msfl_graph_edge& e) { Check(msfl_graph_add_edges(g_, &e, 1), "msfl_graph_add_edges"); }
  void AddFixes(const std::vector<msfl_graph_fix>& f) { Check(msfl_graph_add_fixes(g_, f.data(), static_cast<int>(f.size())), "msfl_graph_add_fixes"); }
  void AddEdgesInfo(const std::vector<msfl_graph_edge_info>& e) {
    Check(msfl_graph_add_edges_info(g_, e.data(), static_cast<int>(e.size())), "msfl_graph_add_edges_info");
  }
  void AddFixesInfo(const std::vector<msfl_graph_fix_info>& f) {
    Check(msfl_graph_add_fixes_info(g_, f.data(), static_cast<int>(f.size())), "msfl_graph_add_fixes_info");
  }
  // |r|^2 of n factors of one kind (MSFL_GRAPH_FACTOR_*) from `first` on, at the current poses, before the loss
  std::vector<double> Chi2(int kind, int first, int n) {
    std::vector<double> out(static_cast<std::size_t>(n > 0 ? n : 0));
    Check(msfl_graph_factor_chi2(g_, kind, first, n, out.data()), "msfl_graph_factor_chi2");
    return out;
  }
  // A loss per factor (msfl_graph_set_losses): factors first .. first + n of one kind get `losses` (n records, or one for all of them);
  // a closure under MSFL_GRAPH_LOSS_GEMAN_MCCLURE is switched off by the solve when it contradicts the rest.
  void SetLosses(int factor_kind, int first, int n, const std::vector<msfl_graph_loss>& losses) {
    Check(msfl_graph_set_losses(g_, factor_kind, first, n, losses.data(), static_cast<int>(losses.size())), "msfl_graph_set_losses");
  }
  void SetLosses(int factor_kind, int first, int n, int loss_kind, double a) { SetLosses(factor_kind, first, n, {msfl_graph_loss{loss_kind, 0, a}}); }
  std::vector<msfl_graph_loss> Losses(int factor_kind, int first, int n) {
    std::vector<msfl_graph_loss> out(static_cast<std::size_t>(n > 0 ? n : 0));
    Check(msfl_graph_get_losses(g_, factor_kind, first, n, out.data()), "msfl_graph_get_losses");
    return out;
  }
  // rho'(|r|^2) of the same factors at the current poses, each under its own loss: near 0 for a factor the loss has switched off
  std::vector<double> FactorWeights(int factor_kind, int first, int n) {
    std::vector<double> out(static_cast<std::size_t>(n > 0 ? n : 0));
    Check(msfl_graph_factor_weights(g_, factor_kind, first, n, out.data()), "msfl_graph_factor_weights");
    return out;
  }
  // Covariance blocks Sigma_ab of the node pairs at the current poses (Covariance::GetCovarianceBlockInTangentSpace): blocks[k] is
  // row-major 6 x 6 in [dt ; dtheta], world frame, rotation on the left; a == b gives a node's marginal.  summary.singular: all NaN.
  struct MarginalBlocks { std::vector<std::array<double, 36>> blocks; msfl_graph_marginals_summary summary; };
  MarginalBlocks Marginals(const std::vector<std::pair<int, int>>& pairs, const msfl_graph_marginals_options* options = nullptr) {
    std::vector<int> flat;
    for (const std::pair<int, int>& p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
    MarginalBlocks out;
    out.blocks.resize(pairs.size());
    out.summary = msfl_graph_marginals_summary{};
    Check(msfl_graph_marginals_with(g_, flat.data(), static_cast<int>(pairs.size()), pairs.empty() ? nullptr : out.blocks[0].data(), MSFL_MEM_HOST,
                                    options, &out.summary), "msfl_graph_marginals");
    return out;
  }
  void SetFixed(int node, bool fixed = true) { Check(msfl_graph_set_fixed(g_, node, fixed ? 1 : 0), "msfl_graph_set_fixed"); }   // SetParameterBlockConstant
  int size() const { return msfl_graph_num_nodes(g_); }
  void Clear() { Check(msfl_graph_clear(g_), "msfl_graph_clear"); }
  double Cost() { double c = 0; Check(msfl_graph_cost(g_, &c), "msfl_graph_cost"); return c; }
  msfl_graph_summary Optimize() {
    msfl_graph_summary s{};
    Check(msfl_graph_optimize(g_, &s), "msfl_graph_optimize");
    return s;
  }
  std::vector<Rigid3d> Poses() {
    const int n = size();
    std::vector<double> v(static_cast<std::size_t>(n) * 7);
    Check(msfl_graph_get_poses(g_, 0, n, v.data(), MSFL_MEM_HOST), "msfl_graph_get_poses");
    std::vector<Rigid3d> out;
    for (int i = 0; i < n; ++i) {
      const double* p = v.data() + 7 * static_cast<std::size_t>(i);
      out.emplace_back(std::array<double, 7>{{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}});
    }
    return out;
  }
  void SetPoses(const std::vector<Rigid3d>& poses, int first = 0) {
    std::vector<double> v;
    for (const Rigid3d& p : poses) { const std::array<double, 7> a = p.ToVector7(); v.insert(v.end(), a.begin(), a.end()); }
    Check(msfl_graph_set_poses(g_, first, static_cast<int>(poses.size()), v.data(), MSFL_MEM_HOST), "msfl_graph_set_poses");
  }
  msfl_graph* handle() { return g_; }

 private:
  void Check(msfl_status st, const char* what) {
    if (st != MSFL_OK) throw std::runtime_error(std::string(what) + ": " + msfl_status_string(st) + " " + msfl_graph_last_error(g_));
  }
  msfl_graph* g_ = nullptr;
};

// gps_fusion.h / gps_fusion.cc.  Times are seconds.  Optimize() builds what gps_fusion.cc:41-85 builds: one relative-pose edge per
// consecutive pair of local poses, measured by those poses themselves, sr = 0.01, st = 0.1 (:73-83); one position fix per fixed point
// between the two local poses that bracket it (upper_bound, :59-65), st = 0.01 (:67); HuberLoss(1.0), 10 iterations (:45,48); and
// writes the optimised poses back into the local poses.
// One deliberate difference: for a fixed point stamped exactly at the last local pose, upper_bound returns end() and the reference
// dereferences it (:62).  Here that fix becomes (N - 2, N - 1, t = 1).
class GpsFusion {
 public:
  struct FixedPoint { double timestamp; Vector3d translation; };
  struct LocalPose { double timestamp; Rigid3d pose; };

  void AddFixedPoint(double time, const Vector3d& translation) {      // gps_fusion.cc:16-20
    if (!fixed_points_.empty() && !(fixed_points_.back().timestamp < time)) throw std::invalid_argument("AddFixedPoint: time not increasing");
    fixed_points_.push_back({time, translation});
  }
  void AddLocalPose(double time, const Rigid3d& pose) {                // gps_fusion.cc:22-25
    if (!local_poses_.empty() && !(local_poses_.back().timestamp < time)) throw std::invalid_argument("AddLocalPose: time not increasing");
    local_poses_.push_back({time, pose});
  }
  // false: fewer than two fixed points, nothing done (gps_fusion.cc:28-31)
  bool Optimize() {
    if (fixed_points_.size() < 2) return false;
    if (!(local_poses_.size() > 2)) throw std::logic_error("GpsFusion::Optimize: needs more than two local poses");                           // :32
    if (!(local_poses_.front().timestamp <= fixed_points_.front().timestamp)) throw std::logic_error("GpsFusion::Optimize: a fixed point before the first local pose");   // :33
    if (!(fixed_points_.back().timestamp <= local_poses_.back().timestamp)) throw std::logic_error("GpsFusion::Optimize: a fixed point after the last local pose");       // :34
    const int n = static_cast<int>(local_poses_.size());
    fixes_.clear(); edges_.clear();
    for (const FixedPoint& fp : fixed_points_) {
      int j = static_cast<int>(std::upper_bound(local_poses_.begin(), local_poses_.end(), fp,
                                                [](const FixedPoint& l, const LocalPose& r) { return l.timestamp < r.timestamp; }) - local_poses_.begin());
      msfl_graph_fix f{};
      if (j >= n) { f.i = n - 2; f.j = n - 1; f.t = 1.0; }            // stamped at the last pose: see above
      else {
        f.i = j - 1; f.j = j;
        f.t = (fp.timestamp - local_poses_[f.i].timestamp) / (local_poses_[f.j].timestamp - local_poses_[f.i].timestamp);
      }
      f.p[0] = fp.translation[0]; f.p[1] = fp.translation[1]; f.p[2] = fp.translation[2];
      f.st = 0.01;
      fixes_.push_back(f);
    }
    std::vector<Rigid3d> poses;
    for (const LocalPose& lp : local_poses_) poses.push_back(lp.pose);
    for (int i = 0; i + 1 < n; ++i) edges_.push_back(PoseGraphEdge(i, i + 1, poses[i], poses[i + 1], 0.01, 0.1));
    msfl_graph_config c = PoseGraph::DefaultConfig();
    c.max_nodes = n; c.max_edges = n; c.max_fixes = static_cast<int>(fixes_.size());
    c.max_num_iterations = 10; c.huber_delta = 1.0;
    PoseGraph graph(&c, device_);
    graph.AddNodes(poses);
    graph.AddEdges(edges_);
    graph.AddFixes(fixes_);
    summary_ = graph.Optimize();
    const std::vector<Rigid3d> out = graph.Poses();
    for (int i = 0; i < n; ++i) local_poses_[i].pose = out[i];
    return true;
  }
  const std::vector<LocalPose>& local_poses() const { return local_poses_; }
  const std::vector<FixedPoint>& fixed_points() const { return fixed_points_; }
  const msfl_graph_summary& summary() const { return summary_; }
  const std::vector<msfl_graph_edge>& edges() const { return edges_; }   // what the last Optimize() built
  const std::vector<msfl_graph_fix>& fixes() const { return fixes_; }
  void set_device(int device) { device_ = device; }

 private:
  std::vector<FixedPoint> fixed_points_;
  std::vector<LocalPose> local_poses_;
  std::vector<msfl_graph_edge> edges_;
  std::vector<msfl_graph_fix> fixes_;
  msfl_graph_summary summary_{};
  int device_ = 0;
};

}  // namespace msfl
#endif  // MSFL_POSE_GRAPH_HPP_
