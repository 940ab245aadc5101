// msfl/keyframes.hpp — C++ face of msfl_keyframes_* (include/msfl_c_api.h, docs/kernels/keyframes.md):
//   msfl::KeyframeStore   RAII over the C ABI: the scans' corner / surf lists kept on the device, laid down at any poses as submaps
//                         (ComposeSubmaps) or into map stores (InsertInto)
//   msfl::Submaps         what ComposeSubmaps delivers: per kind the clouds back to back and their boundaries
// A loop closer registers scan k against the submap of the scans around j, expressed in j's frame: members j-w .. j+w at
// pose_j.inverse() * pose_i, and the registration's result is the measured pose_j^-1 pose_k itself.  Header only, C++14.
#ifndef MSFL_KEYFRAMES_HPP_
#define MSFL_KEYFRAMES_HPP_

#include <array>
#include <cstddef>
#include <vector>

#include "scan_matcher.hpp"

namespace msfl {

struct Submaps {
  std::vector<msfl_point> corner, surf;   // submap b owns [corner_off[b], corner_off[b + 1]) of corner; the same for surf
  std::vector<int> corner_off, surf_off;  // n_submaps + 1 each, starting at 0
};

class KeyframeStore {
 public:
  // The store works on the stream of `handle` (a ScanMatcher's handle(), so that composed submaps feed that matcher without a
  // copy) and must be destroyed before it.  handle == nullptr: the store creates and owns a handle of its own.
  explicit KeyframeStore(msfl_handle* handle = nullptr, const msfl_keyframes_config* config = nullptr, int device = 0) : h_(handle) {
    if (!h_) { detail::Check(msfl_create(nullptr, device, &h_), nullptr, "msfl_create"); own_ = true; }
    const msfl_status st = msfl_keyframes_create(h_, config, &k_);
    if (st != MSFL_OK && own_) { msfl_destroy(h_); h_ = nullptr; }
    detail::Check(st, own_ ? nullptr : h_, "msfl_keyframes_create");
  }
  ~KeyframeStore() { msfl_keyframes_destroy(k_); if (own_) msfl_destroy(h_); }
  KeyframeStore(const KeyframeStore&) = delete;
  KeyframeStore& operator=(const KeyframeStore&) = delete;
  static msfl_keyframes_config DefaultConfig() { msfl_keyframes_config c; msfl_keyframes_default_config(&c); return c; }
  msfl_handle* handle() const { return h_; }
  msfl_keyframes* get() const { return k_; }
  int size() const { return msfl_keyframes_size(k_); }

  // One keyframe from host lists (filtered by the store's leaves; a leaf of 0 stores the list as given).  Returns its index.
  int Add(const std::vector<msfl_point>& corner, const std::vector<msfl_point>& surf) {
    int index = -1;
    detail::Check(msfl_keyframes_add(k_, corner.data(), nullptr, static_cast<int>(corner.size()), surf.data(), nullptr, static_cast<int>(surf.size()),
                                     MSFL_MEM_HOST, &index), h_, "msfl_keyframes_add");
    return index;
  }
  // The same from device memory, each list given as an index list into a cloud (nullptr: the array itself): the shape of
  // msfl_slam_get_clouds, full_scan with less_sharp_idx / less_flat_idx.
  int AddDevice(const msfl_point* corner, const int* corner_idx, int n_corner, const msfl_point* surf, const int* surf_idx, int n_surf) {
    int index = -1;
    detail::Check(msfl_keyframes_add(k_, corner, corner_idx, n_corner, surf, surf_idx, n_surf, MSFL_MEM_DEVICE, &index), h_, "msfl_keyframes_add");
    return index;
  }

  // {corner points, surf points} of keyframes [first, first + n); n < 0: all from `first` on
  std::array<std::vector<int>, 2> Sizes(int first = 0, int n = -1) const {
    if (n < 0) n = size() - first;
    std::array<std::vector<int>, 2> out{{std::vector<int>(static_cast<std::size_t>(n > 0 ? n : 0)), std::vector<int>(static_cast<std::size_t>(n > 0 ? n : 0))}};
    detail::Check(msfl_keyframes_sizes(k_, first, n, out[0].data(), out[1].data()), h_, "msfl_keyframes_sizes");
    return out;
  }

  void Get(int index, std::vector<msfl_point>* corner, std::vector<msfl_point>* surf) const {
    const std::array<std::vector<int>, 2> n = Sizes(index, 1);
    if (corner) corner->resize(static_cast<std::size_t>(n[0][0]));
    if (surf) surf->resize(static_cast<std::size_t>(n[1][0]));
    detail::Check(msfl_keyframes_get(k_, index, corner ? corner->data() : nullptr, n[0][0], surf ? surf->data() : nullptr, n[1][0], MSFL_MEM_HOST), h_,
                  "msfl_keyframes_get");
  }

  // Submap b = the keyframes keys[m] at poses[m] (keyframe frame -> submap frame), m in [member_off[b], member_off[b + 1]); a leaf
  // of 0 delivers the concatenation, otherwise its voxel filter.  One launch of the gather kernel whatever the number of members.
  Submaps ComposeSubmaps(const std::vector<int>& member_off, const std::vector<int>& keys, const std::vector<Rigid3d>& poses, float leaf_corner,
                         float leaf_surf) {
    Submaps out;
    const int n_submaps = static_cast<int>(member_off.size()) - 1;
    if (n_submaps < 0) throw std::invalid_argument("ComposeSubmaps: member_off needs n_submaps + 1 entries");
    const std::vector<double> p = Pack(poses);
    const std::array<std::vector<int>, 2> n = Sizes();
    std::size_t total[2] = {0, 0};
    for (int m = member_off.front(); m < member_off.back() && m < static_cast<int>(keys.size()); ++m)
      if (keys[static_cast<std::size_t>(m)] >= 0 && keys[static_cast<std::size_t>(m)] < size())
        for (int c = 0; c < 2; ++c) total[c] += static_cast<std::size_t>(n[static_cast<std::size_t>(c)][static_cast<std::size_t>(keys[static_cast<std::size_t>(m)])]);
    out.corner.resize(total[0] + 1); out.surf.resize(total[1] + 1);
    out.corner_off.assign(static_cast<std::size_t>(n_submaps) + 1, 0); out.surf_off.assign(static_cast<std::size_t>(n_submaps) + 1, 0);
    if (static_cast<int>(keys.size()) < member_off.back() || poses.size() < keys.size()) throw std::invalid_argument("ComposeSubmaps: fewer keys or poses than members");
    detail::Check(msfl_keyframes_compose(k_, n_submaps, member_off.data(), keys.data(), p.data(), leaf_corner, leaf_surf, out.corner.data(),
                                         static_cast<int>(total[0]), out.corner_off.data(), out.surf.data(), static_cast<int>(total[1]),
                                         out.surf_off.data(), MSFL_MEM_HOST), h_, "msfl_keyframes_compose");
    out.corner.resize(static_cast<std::size_t>(out.corner_off.back()));
    out.surf.resize(static_cast<std::size_t>(out.surf_off.back()));
    return out;
  }

  // Keyframes keys[i] at poses[i] (keyframe frame -> map frame) into the given map stores of handle() (msfl_grid_create; nullptr: that
  // kind is skipped), in order: the map rebuilt at corrected poses.  Returns how many keyframes went in; a keyframe a store refuses
  // (a point beyond +-8192 cells) ends the call there; its status goes to *status, or is thrown when status == nullptr.
  int InsertInto(const std::vector<int>& keys, const std::vector<Rigid3d>& poses, msfl_grid* grid_corner, msfl_grid* grid_surf, msfl_status* status = nullptr) {
    if (poses.size() < keys.size()) throw std::invalid_argument("InsertInto: fewer poses than keys");
    const std::vector<double> p = Pack(poses);
    int n_done = 0;
    const msfl_status st = msfl_keyframes_insert(k_, keys.data(), p.data(), static_cast<int>(keys.size()), grid_corner, grid_surf, &n_done);
    if (status) *status = st;
    else detail::Check(st, h_, "msfl_keyframes_insert");
    return n_done;
  }

 private:
  static std::vector<double> Pack(const std::vector<Rigid3d>& poses) {
    std::vector<double> v;
    v.reserve(7 * poses.size());
    for (const Rigid3d& q : poses) { const std::array<double, 7> a = q.ToVector7(); v.insert(v.end(), a.begin(), a.end()); }
    return v;
  }
  msfl_handle* h_ = nullptr;
  msfl_keyframes* k_ = nullptr;
  bool own_ = false;
};

}  // namespace msfl

#endif  // MSFL_KEYFRAMES_HPP_
