// The device-resident per-scan SLAM step (BASELINE configs[2]) — C-ABI entry points msfl_slam_*.
// Included at the end of msfl_api.hip (shares its handle, DevBuf, PinBuf and helper macros); kernels: msfl_slam.cuh
// plus every stage's own.  Reference control flow being replaced, per scan:
//   odometry thread   msf_loam_node.cc:160-378 -> laser_odometry.cc:69-95
//   mapping thread    laser_mapping.cc:138-258 (Run) -> :260-338 (MatchScan2Map, InsertScan2Map)
// Two HIP streams play the two threads: the odometry chain of scan k + 1 runs under the mapping chain of scan k.  All sizes
// between the raw scan and the result record are device-side; launches are sized by host-known upper bounds.

#include "msfl_slam.cuh"

namespace {

struct SlamScanBuf {                    // everything derived from ONE scan that a later stage reads (two sets, by scan parity)
  DevBuf in_pts, in_ring;               // raw scan (host-memory calls)
  DevBuf full, fring, curv, label, idx; // extraction outputs; idx = 4 lists of n_cap ints
  DevBuf cnt;                           // SC_WORDS ints
  DevBuf ex_off;                        // [0, n]
  DevBuf sharp, ls, ls_ring, flat, lf, lf_ring;   // gathered feature clouds (what the odometry thread keeps as scan_last_)
  DevBuf map_ls, map_lf;                // the mapping thread's less-sharp / less-flat clouds: copies, undistorted / deskewed when IMU data came with the scan
  DevBuf full_scan, full_map;           // msfl_slam_config.keep_clouds: cloud_full_res after the IMU passes, and in the map frame
  DevBuf imu;                           // SlamImuDev: this scan's IMU inputs
  int imu_mode = 0;                     // mode of the block on the device (0 = LiDAR-only: not uploaded again while it stays 0)
  DevBuf dqp;                           // is_initialized branch: dq (4) + dp (3) doubles per down-sampled corner, then per surf feature
  DevBuf odo_off, odo_status;           // scan-to-scan offset pairs (10 ints), status word
  DevBuf poses;                         // pose_odom_k[7] | pose_map_k[7] | c2l_k[7]
  PinBuf upload;                        // pinned staging of the raw scan
  int n = 0;
  hipEvent_t ev_odo = nullptr;          // the odometry chain of the scan in this set has been enqueued up to here
  hipEvent_t ev_pose = nullptr, ev_cready = nullptr, ev_match = nullptr, ev_cdone = nullptr;   // mapping <-> corner-side hand-overs
  // voxel-filtered scan clouds (staging of voxel_cloud_lds_kernel) + its run sums, per buffer set: the filters of scan k + 1 run
  // (on a stream of their own, next to its scan-to-scan match) while the mapping thread still reads those of scan k
  DevBuf vox_c, vox_s, vsum_c, vsum_s;
  DevBuf vmeta;                         // ints: m_c, flag_c, m_s, flag_s
  hipEvent_t ev_feat = nullptr, ev_vox = nullptr;   // feature lists gathered (odometry stream) -> both lists filtered (voxel stream)
};

constexpr int kSlamSlots = 4;
// What the msfl_slam_set_* calls said when a scan was fed: read once, at the top of slam_add_scan_impl; scans already fed keep theirs.
struct SlamScanOptions {
  RegOptions odo, map;                  // the two matchers' knobs
  bool unc = false, degen_any = false, rej_any = false;   // the slot's record pairs travel with its result
  bool prior_odo = false, prior_map = false;              // msfl_slam_set_next_prior gave this scan a record
  bool crop = false;                    // msfl_slam_set_map_window: the stores are cropped after this scan's inserts
  int half[3] = {};
};
struct SlamJob { int k = 0, n = 0, imu_mode = 0; SlamScanOptions o; };  // one scan's mapping chain, handed to the mapping thread once its odometry chain is enqueued

// One optional feature's records: a pair per slot ({odometry, mapping}; the map window's: {corner, surf}) that the scan's chains
// write on the device and that travels to the host with the slot's result copy.
struct SlotRecords {
  DevBuf dev[kSlamSlots];
  PinBuf host;                          // kSlamSlots pairs
  bool held[kSlamSlots] = {};           // the scan in this slot was fed with the feature on (the window: a crop ran on it)
  size_t bytes = 0;                     // of one pair
  hipError_t ensure(size_t pair_bytes) {                   // reserved when the feature is first turned on
    if (host.p) return hipSuccess;
    bytes = pair_bytes;
    for (auto& b : dev) { const hipError_t e = b.reserve(bytes); if (e != hipSuccess) return e; }
    return host.reserve(kSlamSlots * bytes);
  }
  hipError_t arm(int slot, bool on, bool zero, hipStream_t st) {   // a scan takes the slot; zero: a slice stays zero where no solve runs
    held[slot] = on;
    return on && zero ? hipMemsetAsync(dev[slot].p, 0, bytes, st) : hipSuccess;
  }
  hipError_t fetch(int slot, hipStream_t st) const {
    return held[slot] ? hipMemcpyAsync(host.as<char>() + slot * bytes, dev[slot].p, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  }
  template <class T> const T* host_at(int slot) const { return reinterpret_cast<const T*>(host.as<char>() + slot * bytes); }
};

// MSFL_SLAM_HOST_PROFILE: the wall clock of one thread's enqueue, by segment of the chain in order of first appearance.
struct SegClock {
  bool on;                              // (the first scans allocate: left out)
  std::vector<std::pair<const char*, double>>* into;
  std::chrono::steady_clock::time_point t;
  void operator()(const char* what) {   // close the segment that ends here
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    const double dt = std::chrono::duration<double>(now - t).count();
    t = now;
    for (auto& e : *into) if (e.first == what) { e.second += dt; return; }
    into->emplace_back(what, dt);
  }
};
constexpr int kSlamProfileSkip = 20;                    // MSFL_SLAM_HOST_PROFILE leaves the first scans (allocations) out
#ifndef MSFL_SLAM_ODOM_LANES
#define MSFL_SLAM_ODOM_LANES 64
#endif
#ifndef MSFL_SLAM_LM_BLOCK
#define MSFL_SLAM_LM_BLOCK 512
#endif
constexpr int kSlamLmBlock = MSFL_SLAM_LM_BLOCK;       // threads of the scan-to-map solve of the SLAM step
#ifndef MSFL_SLAM_ODOM_LM_BLOCK
#define MSFL_SLAM_ODOM_LM_BLOCK 128
#endif
constexpr int kSlamOdomLmBlock = MSFL_SLAM_ODOM_LM_BLOCK;   // threads of its scan-to-scan solve
constexpr int kSlamOdomLanes = MSFL_SLAM_ODOM_LANES;   // lanes per scan-to-scan query in the one-pair-per-call SLAM step

}  // namespace

struct msfl_slam_s {
  msfl_handle* ho = nullptr;            // odometry thread: stream + scratch of stage A and stage B
  msfl_handle* hm = nullptr;            // mapping thread: voxel filters, map stores, stage C
  msfl_handle* hc = nullptr;            // mapping thread, corner side: its surrounded cloud, index build and map insert run on a
                                        // stream of their own next to the (ten times larger) surf side; joined before the match and at the end
  msfl_handle* hv = nullptr;            // the two voxel filters of the mapping thread: they need the feature lists only, not the odometry
                                        // pose, so they run on this stream while the odometry thread matches the same scan
  msfl_grid* gc = nullptr;              // hybrid_grid_map_corner_
  msfl_grid* gs = nullptr;              // hybrid_grid_map_surf_
  msfl_slam_config cfg{};
  int n_cap = 0;
  SlamCaps caps{};
  SlamScanBuf sb[2];
  DevBuf chain;                         // c2l[7] | odo_cur[7] | odom2map[7]
  DevBuf vox_scratch;                   // run records of the global-scratch form of the voxel kernel
  DevBuf vox_big;                       // point-sort scratch of the > 65 535-point form
  DevBuf meta;                          // ints: n_map_c, n_map_s, map_status, in_off[6]
  DevBuf map_c, map_s;                  // surrounded map clouds
  DevBuf rec[kSlamSlots];               // device result records
  PinBuf rec_host;                      // kSlamSlots records
  // msfl_slam_set_uncertainty / _set_degeneracy / _set_outlier_rejection: the knobs of the two matchers {odometry, mapping} (both get the
  // uncertainty's min_eigenvalue) and a record pair per slot and feature
  bool unc_on = false;
  RegOptions opt[2];
  SlotRecords unc, degen, rej;
  // msfl_slam_set_next_prior: {odometry, mapping} records for the NEXT scan only.  They are copied to the slot of the scan that
  // consumes them (on its odometry stream, ahead of ev_odo), so a later msfl_slam_add_scan cannot overwrite what a queued
  // mapping chain has not read yet: a slot is reused only after its scan's record is out.
  msfl_pose_prior next_prior[2] = {};
  bool next_prior_set[2] = {};
  DevBuf prior[kSlamSlots];
  // msfl_slam_set_map_window: both stores are cropped to +-win_half cells around pose_map after the inserts of every win_every-th scan.
  // Two msfl_grid_crop_info {corner, surf} per slot; they travel with the slot's result copy.
  bool win_on = false;
  int win_half[3] = {}, win_every = 1;
  SlotRecords win;
  hipEvent_t ev_done[kSlamSlots] = {};
  long long seq_c[kSlamSlots] = {}, seq_s[kSlamSlots] = {};   // map-store insert sequence numbers of the scan in each slot
  bool applied[kSlamSlots] = {};        // the slot's grid reports have been folded into the stores' host-side bounds
  int n_scans = 0;                      // scans fed
  bool enqueueing = false;              // msfl_slam_add_scan has put work of the current scan on a stream
  bool poisoned = false;                // a call failed after that point: streams, buffer sets and the stores' host-side bounds no longer
  msfl_status poison_status = MSFL_OK;  // agree; every later call returns the stored error until destroy
  int adding_scan = -1;                 // index of the scan msfl_slam_add_scan is working on (n_scans moves in the middle of the call)
  int poison_scan = -1;                 // the scan whose chain failed: results of EARLIER scans stay fetchable (ADVICE r04)
  std::mutex mu_err;                    // last_error is written by the caller's thread and, with MSFL_SLAM_THREADS=1, by the mapping thread
  std::vector<double> imu_stage;        // host staging of one SlamImuDev upload
  // ---- the mapping thread.  Like the reference (LaserMapping::Run on its own std::thread, laser_mapping.cc:86), the mapping chain
  // of a scan is ENQUEUED by a second host thread: the step is host-enqueue bound (~70 launches per scan), and with one thread
  // the odometry chain of scan k + 1 cannot be put on its stream before the ~50 launches of scan k's mapping chain are out.
  // MEASURED (profiles/r04_slam_threads.md): moving the ~240 us of mapping enqueue off the calling thread did NOT shorten the period
  // (0.57 vs 0.49-0.51 ms per scan on the same box): the step is bound by the GPU-side span of the mapping stream's dependent
  // kernel chain, not by the host.  Default off; MSFL_SLAM_THREADS=1 turns it on (identical results: the GPU-side order is fixed
  // by events).
  bool threaded = false;
  std::thread worker;
  std::mutex mu;                        // job hand-over, mapped_upto, worker status
  std::condition_variable cv_job, cv_done;
  bool has_job = false, stop = false;
  SlamJob job{};
  int mapped_upto = -1;                 // scans [0, mapped_upto] have their mapping chain (and ev_done) on the streams
  std::mutex mu_grid;                   // the map stores' host-side bounds + slot bookkeeping: mapping enqueue vs. harvest on the caller's side
  std::vector<std::pair<const char*, double>> host_seg_map;   // host profile of the mapping enqueue (its own thread's clock)
  double host_map_s = 0.0;
  int fail_at = -1;                     // MSFL_SLAM_FAIL_AT=k (fault injection for the tests of the poisoning contract): the mapping chain of scan k fails
  bool host_profile = false;            // MSFL_SLAM_HOST_PROFILE=1: wall clock inside msfl_slam_add_scan, split into waiting for a free buffer
  std::vector<std::pair<const char*, double>> host_seg;   // enqueue time by segment of the chain, in order of first appearance
  double host_wait_s = 0.0, host_enqueue_s = 0.0;   // set (scan k - 2 still running: the GPU is the limit) and enqueueing (the host is); printed at destroy
  std::string last_error;
};

namespace {

void slam_worker_main(msfl_slam* s);
msfl_status slam_wait_mapped(msfl_slam* s, int k);
msfl_status slam_enqueue_mapping(msfl_slam* s, const SlamJob& jb);

enum { META_NMC = 0, META_NMS, META_STATUS, META_OFF, META_WORDS = 12 };
enum { VM_MC = 0, VM_FC, VM_MS, VM_FS, VM_WORDS = 4 };

msfl_status sfail(msfl_slam* s, msfl_status st, const std::string& msg) {
  if (s) { std::lock_guard<std::mutex> lk(s->mu_err); s->last_error = msg; }
  return st;
}
#define SHIP(s, expr)                                                                                              \
  do { hipError_t e__ = (expr); if (e__ != hipSuccess) return sfail(s, MSFL_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(e__)); } while (0)
#define SCHK(s, h, expr) do { msfl_status st__ = (expr); if (st__) return sfail(s, st__, (h)->last_error); } while (0)

// The getters' preamble.  slam_slot_of: the slot that holds the record of scan `scan_index`, or the error of `who` when the record is
// no longer (or not yet) held.  slam_slot_ready: wait until that record, and what travels with it, is on the host.
msfl_status slam_slot_of(msfl_slam* s, int scan_index, const char* who, int* slot) {
  if (scan_index < 0 || scan_index >= s->n_scans || scan_index < s->n_scans - kSlamSlots)
    return sfail(s, MSFL_BAD_ARG, std::string(who) + ": that scan's record is no longer (or not yet) held");
  *slot = scan_index % kSlamSlots;
  return MSFL_OK;
}
msfl_status slam_slot_ready(msfl_slam* s, int scan_index) {
  SHIP(s, hipSetDevice(s->ho->device));
  { const msfl_status ws = slam_wait_mapped(s, scan_index); if (ws) return ws; }
  SHIP(s, hipEventSynchronize(s->ev_done[scan_index % kSlamSlots]));
  return MSFL_OK;
}
// The getter `who` of a feature's record pair; refused for a scan that was fed while `setter` had the feature off.
template <class T>
msfl_status slam_get_pair(msfl_slam* s, SlotRecords msfl_slam_s::*feature, int scan_index, const char* who, const char* setter, T* odometry, T* mapping) {
  if (!s) return MSFL_BAD_ARG;
  const SlotRecords& r = s->*feature;
  int slot;
  { const msfl_status rs = slam_slot_of(s, scan_index, who, &slot); if (rs) return rs; }
  if (!r.held[slot]) return sfail(s, MSFL_BAD_ARG, std::string(who) + ": that scan was fed with " + setter + " off");
  { const msfl_status rs = slam_slot_ready(s, scan_index); if (rs) return rs; }
  const T* d = r.host_at<T>(slot);
  if (odometry) *odometry = d[0];
  if (mapping) *mapping = d[1];
  return MSFL_OK;
}

// What matcher m (0 odometry, 1 mapping) of the scan in `slot` carries: the slot's first / second records.  A matcher whose feature is
// off gets no record pointer even where the other matcher holds the pair.  (The prior was uploaded ahead of the scan's ev_odo.)
RegSinks slam_sinks(msfl_slam* s, int slot, int m, const SlamScanOptions& o) {
  msfl_slam_result* rec = s->rec[slot].as<msfl_slam_result>();
  RegSinks k;
  k.opt = m ? o.map : o.odo;
  k.info = reinterpret_cast<DevMatchInfo*>(m ? &rec->mapping : &rec->odometry);
  if (o.unc) k.unc = s->unc.dev[slot].as<UncRecord>() + m;
  if (m ? o.prior_map : o.prior_odo) k.prior = s->prior[slot].as<PosePrior>() + m;
  if (k.opt.degen_on) k.degen = s->degen.dev[slot].as<DegenRecord>() + m;
  if (k.opt.rej.mode != MSFL_REJECT_OFF) k.rej = s->rej.dev[slot].as<RejectRecord>() + m;
  return k;
}

__global__ void slam_result_kernel(msfl_slam_result* __restrict__ r, int scan_index, int* __restrict__ cnt, const double* __restrict__ poses_k,
                                   const double* __restrict__ odom2map, const int* __restrict__ meta, const int* __restrict__ vmeta,
                                   const int* __restrict__ odo_status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < 7; k++) { r->pose_odom[k] = poses_k[k]; r->pose_map[k] = poses_k[7 + k]; r->pose_curr2last[k] = poses_k[14 + k]; r->pose_odom2map[k] = odom2map[k]; }
  r->scan_index = scan_index;
  r->status_extract = cnt[SC_STATUS] ? cnt[SC_STATUS] : (cnt[SC_OVERFLOW] ? MSFL_CAPACITY : 0);
  r->status_mapping = meta[META_STATUS];
  r->n_full = cnt[SC_FULL]; r->n_sharp = cnt[SC_SHARP]; r->n_less_sharp = cnt[SC_LESS_SHARP]; r->n_flat = cnt[SC_FLAT]; r->n_less_flat = cnt[SC_LESS_FLAT];
  r->n_corner_ds = vmeta[VM_MC]; r->n_surf_ds = vmeta[VM_MS];
  r->n_map_corner = meta[META_NMC]; r->n_map_surf = meta[META_NMS];
  r->status_imu = cnt[SC_IMU_BAD] ? MSFL_BAD_ARG : 0;
  cnt[SC_IMU_BAD] = 0;                                           // raised by lanes of the gather kernel: cleared for the scan after next
  r->status_clouds = cnt[SC_CLOUD_BAD] ? MSFL_BAD_ARG : 0;
  cnt[SC_CLOUD_BAD] = 0;
  r->reserved_ = 0;
  r->status_insert = (r->grid_corner[3] | r->grid_corner[4] | r->grid_surf[3] | r->grid_surf[4]) ? MSFL_CAPACITY : 0;
  // a scan that was not matched at all (failed extraction, a list beyond the launch bounds) is not a successful MatchScan2Scan
  if (r->odometry.status == 0 && *odo_status != 0) r->odometry.status = *odo_status;
}

// MatchScan2Scan on device-resident clouds whose sizes live on the device: the column-grid path of scan2scan_batch_impl for
// one pair, launches sized by the per-scan caps.  d_off = [ls | lf | sharp | flat | rec] offset pairs.
msfl_status scan2scan_dyn(msfl_handle* h, const SlamScanBuf& last, const SlamScanBuf& cur, const SlamCaps& caps, double* d_pose, const RegSinks& sinks) {
  hipStream_t st = h->stream;
  const int B = 1;
  const int* d_off = cur.odo_off.as<int>();
  int* d_status = cur.odo_status.as<int>();
  const int n_rec_cap = caps.sharp + caps.flat;
  HIPCHK(h, h->records.reserve((rec_buffer_doubles((size_t)caps.sharp, (size_t)caps.flat) + 8) * sizeof(double)));
  const BatchView bv = batch_view(cur.sharp.as<float4>(), cur.flat.as<float4>(), d_off + 4, 2, B, n_rec_cap, 0, 0, caps.flat, 1);
  OdomView ov;
  ov.last_ls = last.ls.as<float4>(); ov.last_ls_ring = last.ls_ring.as<uint16_t>(); ov.last_ls_off = d_off;
  ov.last_lf = last.lf.as<float4>(); ov.last_lf_ring = last.lf_ring.as<uint16_t>(); ov.last_lf_off = d_off + 2;
  ov.dist_sq_threshold = h->prm.odom_distance_sq_threshold;
  ov.nearby_scan = h->prm.odom_nearby_scan;
  const SolverParams sp = solver_params(h->prm, h->prm.odom_min_correspondences);
  const bool gate_fits_grid = h->prm.odom_distance_sq_threshold <= 35.9;      // see scan2scan_batch_impl
  const bool use_grid = gate_fits_grid && !h->odom_force_brute;
  // one pair per call: the machine is empty, so a query gets a whole wavefront (kSlamOdomLanes lanes walk its column runs;
  // the minima are order-free lexicographic keys, results do not depend on the lane count) instead of the batch's 16 lanes
  OdomIndex oix, oie;
  { msfl_status is = odom_index(h, h->od.planes, use_grid, B, (size_t)caps.less_flat, caps.flat, kOdomBlock / kSlamOdomLanes, &oix); if (is) return is;
    is = odom_index(h, h->od.edges, use_grid, B, (size_t)caps.less_sharp, caps.sharp, kOdomBlock / kSlamOdomLanes, &oie); if (is) return is; }
  if (use_grid) {
    ScopedTimer timer(h, T_ODOM);
    // a LAST scan of more than 32 768 points (a 64-beam sensor) takes the several-workgroups form of the index build (three more launches).
    // Decided by the points that scan actually had (known on the host since its msfl_slam_add_scan; its less-flat list is a subset), not by
    // the session's capacity: with the default max_scan_points = 200 000 every 16-beam scan used to take the split form too (ADVICE r05).
    // Both forms build the same index bit for bit (test_binning_a_64_beam_sized_cloud_...), so the choice cannot change a result.
    msfl_status bs = launch_odom_bin(h, st, odom_bin_job(ov.last_lf, ov.last_lf_ring, ov.last_lf_off, oix),
                                     odom_bin_job(ov.last_ls, ov.last_ls_ring, ov.last_ls_off, oie), 2 * B, B, std::min<long long>(caps.less_flat, last.n));
    if (bs != MSFL_OK) return bs;
  }
  // one solve on an empty machine: the wide workgroup of the mapping solve (~570 records: one per thread and pass)
  return solve_outer<kSlamOdomLmBlock>(h, B, bv, nullptr, d_pose, d_status, sinks, sp, h->prm.outer_iterations, [&](int) {
    ScopedTimer timer(h, T_ODOM);
    // pairs the column grid cannot take (mode != 0) and, without the grid, everything
    hipLaunchKernelGGL(assoc_scan2scan_kernel, dim3(div_up(n_rec_cap, 256), B), dim3(256), 0, st, bv, ov, (const double*)d_pose,
                       (const int*)d_status, h->records.as<double>(), oix.mode, oie.mode);
    if (use_grid) {
      const int plane_blocks = div_up(B, 8) * 8 * oix.tiles, edge_blocks = div_up(B, 8) * 8 * oie.tiles;
      hipLaunchKernelGGL((assoc_scan2scan_grid_kernel<kSlamOdomLanes>), dim3(plane_blocks + edge_blocks), dim3(kOdomBlock), 0, st, bv, ov, oix, oie,
                         plane_blocks, (const double*)d_pose, (const int*)d_status, h->records.as<double>());
    }
    return MSFL_OK;
  });
}

// MatchScan2Map against the index in h->map_c / map_s, scan clouds and their (device-side) sizes given by in_off.
// deskew != nullptr: the is_initialized branch (Deskew factors; dq / dp / V / G all device-side, pprime provided here).
msfl_status scan2map_dyn(msfl_handle* h, const float4* d_corner, const float4* d_surf, const int* d_in_off, int cap_corner, int cap_surf,
                         double* d_pose, int* d_status, const RegSinks& sinks, const DeskewView* deskew = nullptr) {
  const int n_rec_cap = cap_corner + cap_surf;
  HIPCHK(h, h->records.reserve((rec_buffer_doubles((size_t)cap_corner, (size_t)cap_surf) + 8) * sizeof(double)));
  HIPCHK(h, h->nn.reserve(std::max<size_t>(1, (size_t)n_rec_cap) * 5 * sizeof(int)));
  const BatchView bv = batch_view(d_corner, d_surf, d_in_off, 2, 1, n_rec_cap, 0, 0, cap_surf, 1);
  DeskewView dv{};
  if (deskew) {
    dv = *deskew;
    HIPCHK(h, h->pprime.reserve(std::max<size_t>(1, (size_t)n_rec_cap) * 3 * sizeof(double)));
    dv.pprime = h->pprime.as<double>();
  }
  // one solve on an empty machine: 512 threads share its ~4 600 records (the batch kernel's 128 threads per solve are sized
  // for 1 024 concurrent solves); the per-thread summation order differs from the batch kernel's, the result by rounding
  return solve_outer<kSlamLmBlock>(h, 1, bv, dv.pprime, d_pose, d_status, sinks, solver_params(h->prm, 0), h->prm.outer_iterations, [&](int) {
    s_launch_assoc(h, bv, d_pose, d_status, deskew != nullptr, dv, n_rec_cap);
    return MSFL_OK;
  });
}

// one list through the one-workgroup voxel filter: the 256-thread form, escalating on the device to the 1024-thread one
// and, for a list with more runs than its LDS holds, to the same kernel over a global scratch area (d_scratch:
// kVoxScratchBytes).  Only a list beyond 65 535 points or +-8 191 voxels is refused (flag 4 -> MSFL_CAPACITY in the record).
constexpr size_t kVoxScratchBytes = (size_t)65536 * 8 + (size_t)2 * 65536 * 2;
msfl_status voxel_dyn(msfl_handle* h, const float4* d_full, const int* d_idx, const int* d_off, const int* d_count, int n_cap, float leaf,
                      float4* d_out, float4* d_sums, int* d_m, int* d_flag, void* d_scratch, DevBuf* big) {
  VoxelBatchView v;
  v.pts = d_full; v.idx = d_idx; v.off = d_off; v.count = d_count; v.n_clouds = 1; v.n_total = n_cap; v.inv_leaf = 1.0f / leaf;
  hipLaunchKernelGGL((voxel_cloud_lds_kernel<4, 512>), dim3(1), dim3(256), 0, h->stream, v, d_out, d_sums, d_m, d_flag, 0);
  if (n_cap > 2048) {          // a list of up to 2 048 points always fits the small form (512 run slots per 512-point slice)
    hipLaunchKernelGGL((voxel_cloud_lds_kernel<16, 768>), dim3(1), dim3(1024), 0, h->stream, v, d_out, d_sums, d_m, d_flag, 1);
    hipLaunchKernelGGL((voxel_cloud_lds_kernel<16, 4096, true>), dim3(1), dim3(1024), 0, h->stream, v, d_out, d_sums, d_m, d_flag, 2,
                       reinterpret_cast<unsigned long long*>(d_scratch), reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(d_scratch) + (size_t)65536 * 8));
  }
  if (n_cap > kVoxMaxPoints) {   // the scan capacity allows a list the one-workgroup forms cannot address: plain point sort, on refusal only
    const size_t n = (size_t)n_cap;
    HIPCHK(h, big->reserve(n * (4 * sizeof(unsigned) + 2 * sizeof(int)) + 256 + kVoxBigBoxGroups * sizeof(VoxBigPart)));
    unsigned* k1 = big->as<unsigned>(); unsigned* k2 = k1 + n; unsigned* v1 = k2 + n; unsigned* v2 = v1 + n;
    int* head = reinterpret_cast<int*>(v2 + n); int* pos = head + n;
    VoxBigDesc* desc = reinterpret_cast<VoxBigDesc*>(pos + n);
    VoxBigPart* part = reinterpret_cast<VoxBigPart*>(desc + 1);
    const dim3 grid(div_up(n_cap, 256)), block(256);
    const float4* pts = d_full + 0;                                    // the list's region starts at off[0] = 0
    hipLaunchKernelGGL(vox_big_bbox_kernel, dim3(kVoxBigBoxGroups), dim3(256), 0, h->stream, pts, d_idx, d_count, n_cap, v.inv_leaf, (const int*)d_flag, part);
    hipLaunchKernelGGL(vox_big_desc_kernel, dim3(1), dim3(64), 0, h->stream, (const VoxBigPart*)part, d_count, n_cap, d_flag, d_m, desc);
    hipLaunchKernelGGL(vox_big_key_kernel, grid, block, 0, h->stream, pts, d_idx, n_cap, v.inv_leaf, (const VoxBigDesc*)desc, k1, v1);
    size_t tb = 0;
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, k1, k2, v1, v2, n, 0u, 32u, h->stream));
    HIPCHK(h, h->idx_cub.reserve(tb));
    HIPCHK(h, rocprim::radix_sort_pairs(h->idx_cub.p, tb, k1, k2, v1, v2, n, 0u, 32u, h->stream));
    hipLaunchKernelGGL(vox_big_head_kernel, grid, block, 0, h->stream, (const unsigned*)k2, n_cap, (const VoxBigDesc*)desc, head);
    size_t tb2 = 0;
    HIPCHK(h, rocprim::inclusive_scan(nullptr, tb2, head, pos, n, rocprim::plus<int>(), h->stream));
    HIPCHK(h, h->idx_cub.reserve(tb2));
    HIPCHK(h, rocprim::inclusive_scan(h->idx_cub.p, tb2, head, pos, n, rocprim::plus<int>(), h->stream));
    hipLaunchKernelGGL(vox_big_centroid_kernel, grid, block, 0, h->stream, pts, d_idx, (const unsigned*)k2, (const unsigned*)v2, (const int*)head,
                       (const int*)pos, n_cap, (const VoxBigDesc*)desc, d_out, d_m, d_flag);
  }
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// fold the grid reports of every finished slot into the stores' host-side bounds
void slam_harvest(msfl_slam* s, bool wait_all) {
  for (int back = std::min(s->n_scans, kSlamSlots); back >= 1; back--) {
    const int k = s->n_scans - back, slot = k % kSlamSlots;
    if (s->applied[slot]) continue;
    if (wait_all) (void)hipEventSynchronize(s->ev_done[slot]);
    else if (hipEventQuery(s->ev_done[slot]) != hipSuccess) break;                 // in order: later slots are not done either
    const msfl_slam_result* r = s->rec_host.as<msfl_slam_result>() + slot;
    if (s->seq_c[slot]) (void)grid_apply_report(s->gc, r->grid_corner, s->seq_c[slot]);
    if (s->seq_s[slot]) (void)grid_apply_report(s->gs, r->grid_surf, s->seq_s[slot]);
    s->applied[slot] = true;
  }
}

}  // namespace

extern "C" {

void msfl_slam_default_config(msfl_slam_config* c) {
  if (!c) return;
  c->map_resolution = 3.0f; c->leaf_corner = 0.2f; c->leaf_surf = 0.4f;
  c->min_map_corner = 10; c->min_map_surf = 50;
  c->max_scan_points = 200000; c->max_rings = 128;
  c->reference_quirks = 0;
  c->keep_clouds = 0;
  for (int k = 0; k < 7; k++) c->pose_odom2map[k] = k == 6 ? 1.0 : 0.0;
}

// The text is copied under the lock into a buffer of the CALLING thread: the mapping thread (MSFL_SLAM_THREADS=1) may reassign last_error
// at any time, and a pointer into the string itself could dangle.  Valid until the same thread's next call of this function.
const char* msfl_slam_last_error(const msfl_slam* s) {
  if (!s) return "";
  static thread_local std::string copy;
  msfl_slam* m = const_cast<msfl_slam*>(s);
  { std::lock_guard<std::mutex> lk(m->mu_err); copy = m->last_error; }
  return copy.c_str();
}

void msfl_slam_destroy(msfl_slam* s) {
  if (!s) return;
  if (s->worker.joinable()) {
    { std::lock_guard<std::mutex> lk(s->mu); s->stop = true; }
    s->cv_job.notify_all();
    s->worker.join();                                              // finishes the job it holds, if any
  }
  if (s->host_profile && s->n_scans > kSlamProfileSkip) {
    const int np = s->n_scans - kSlamProfileSkip;
    std::fprintf(stderr, "msfl_slam host profile: scans %d..%d, per scan %.1f us waiting for a free buffer set, %.1f us enqueueing\n", kSlamProfileSkip,
                 s->n_scans - 1, 1e6 * s->host_wait_s / np, 1e6 * s->host_enqueue_s / np);
    for (auto& e : s->host_seg) std::fprintf(stderr, "  %-44s %6.1f us\n", e.first, 1e6 * e.second / np);
    std::fprintf(stderr, "mapping chain (%s): %.1f us enqueueing per scan\n", s->threaded ? "its own thread" : "calling thread", 1e6 * s->host_map_s / np);
    for (auto& e : s->host_seg_map) std::fprintf(stderr, "  %-44s %6.1f us\n", e.first, 1e6 * e.second / np);
  }
  if (s->ho) (void)hipSetDevice(s->ho->device);
  if (s->ho) (void)hipStreamSynchronize(s->ho->stream);
  if (s->hm) (void)hipStreamSynchronize(s->hm->stream);
  if (s->hc) (void)hipStreamSynchronize(s->hc->stream);
  if (s->hv) (void)hipStreamSynchronize(s->hv->stream);
  for (auto& b : s->sb)
    for (hipEvent_t e : {b.ev_odo, b.ev_pose, b.ev_cready, b.ev_match, b.ev_cdone, b.ev_feat, b.ev_vox}) if (e) (void)hipEventDestroy(e);
  for (auto e : s->ev_done) if (e) (void)hipEventDestroy(e);
  if (s->gc) msfl_grid_destroy(s->gc);
  if (s->gs) msfl_grid_destroy(s->gs);
  if (s->ho) msfl_destroy(s->ho);
  if (s->hm) msfl_destroy(s->hm);
  if (s->hc) msfl_destroy(s->hc);
  if (s->hv) msfl_destroy(s->hv);
  delete s;
}

msfl_status msfl_slam_create(const msfl_params* params, const msfl_slam_config* config, int device, msfl_slam** out) {
  if (!out) return MSFL_BAD_ARG;
  *out = nullptr;
  msfl_slam_config cfg;
  if (config) cfg = *config; else msfl_slam_default_config(&cfg);
  if (!(cfg.map_resolution > 0.f) || !(cfg.leaf_corner > 0.f) || !(cfg.leaf_surf > 0.f) || cfg.max_scan_points < 1 || cfg.max_rings < 1 ||
      cfg.max_rings > kMaxRings || cfg.max_scan_points > (1 << 24))
    return MSFL_BAD_ARG;
  msfl_slam* s = new msfl_slam_s();
  s->cfg = cfg;
  if (const char* e = std::getenv("MSFL_SLAM_HOST_PROFILE")) s->host_profile = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_SLAM_FAIL_AT")) s->fail_at = std::atoi(e);
  msfl_status st = msfl_create(params, device, &s->ho);
  if (!st) st = msfl_create(params, device, &s->hm);
  if (!st) st = msfl_create(params, device, &s->hc);
  if (!st) st = msfl_create(params, device, &s->hv);
  if (!st) st = msfl_grid_create(s->hc, cfg.map_resolution, cfg.leaf_corner, &s->gc);
  if (!st) st = msfl_grid_create(s->hm, cfg.map_resolution, cfg.leaf_surf, &s->gs);
  if (st) { msfl_slam_destroy(s); return st; }
  const msfl_params& p = s->ho->prm;
  const int n = s->n_cap = cfg.max_scan_points;
  // a ring has `sectors` sectors of at most 2 sharp, 20 less-sharp (the sharp ones included) and 4 flat picks (msf_loam_node.cc:277-317)
  const long long per_ring = (long long)p.sectors_per_ring * cfg.max_rings;
  s->caps.sharp = (int)std::min<long long>(n, per_ring * std::max(p.max_sharp_per_sector, 0));
  s->caps.less_sharp = (int)std::min<long long>(n, per_ring * std::max(p.max_less_sharp_per_sector, 0));
  s->caps.flat = (int)std::min<long long>(n, per_ring * std::max(p.max_flat_per_sector, 0));
  s->caps.less_flat = n;
  auto hip_ok = [&](hipError_t e) { if (e != hipSuccess && !st) { st = MSFL_HIP_ERROR; std::lock_guard<std::mutex> le(s->mu_err); s->last_error = hipGetErrorString(e); } };
  const size_t nn = (size_t)n;
  for (auto& b : s->sb) {
    hip_ok(b.full.reserve(nn * sizeof(float4))); hip_ok(b.fring.reserve(nn * sizeof(uint16_t))); hip_ok(b.curv.reserve(nn * sizeof(float)));
    hip_ok(b.label.reserve(nn)); hip_ok(b.idx.reserve(4 * nn * sizeof(int))); hip_ok(b.cnt.reserve(SC_WORDS * sizeof(int)));
    hip_ok(b.ex_off.reserve(2 * sizeof(int)));
    hip_ok(b.sharp.reserve(std::max(1, s->caps.sharp) * sizeof(float4))); hip_ok(b.flat.reserve(std::max(1, s->caps.flat) * sizeof(float4)));
    hip_ok(b.ls.reserve(std::max(1, s->caps.less_sharp) * sizeof(float4))); hip_ok(b.ls_ring.reserve(std::max(1, s->caps.less_sharp) * sizeof(uint16_t)));
    hip_ok(b.lf.reserve(nn * sizeof(float4))); hip_ok(b.lf_ring.reserve(nn * sizeof(uint16_t)));
    hip_ok(b.map_ls.reserve(std::max(1, s->caps.less_sharp) * sizeof(float4))); hip_ok(b.map_lf.reserve(nn * sizeof(float4)));
    hip_ok(b.imu.reserve(sizeof(SlamImuDev)));
    if (cfg.keep_clouds) { hip_ok(b.full_scan.reserve(nn * sizeof(float4))); hip_ok(b.full_map.reserve(nn * sizeof(float4))); }
    hip_ok(b.odo_off.reserve(10 * sizeof(int))); hip_ok(b.odo_status.reserve(sizeof(int))); hip_ok(b.poses.reserve(21 * sizeof(double)));
    hip_ok(b.vox_c.reserve(nn * sizeof(float4))); hip_ok(b.vox_s.reserve(nn * sizeof(float4)));
    hip_ok(b.vsum_c.reserve(nn * sizeof(float4))); hip_ok(b.vsum_s.reserve(nn * sizeof(float4)));
    hip_ok(b.vmeta.reserve(VM_WORDS * sizeof(int)));
    for (hipEvent_t* e : {&b.ev_odo, &b.ev_pose, &b.ev_cready, &b.ev_match, &b.ev_cdone, &b.ev_feat, &b.ev_vox}) hip_ok(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (!st) {
      hip_ok(hipMemsetAsync(b.cnt.p, 0, SC_WORDS * sizeof(int), s->ho->stream)); hip_ok(hipMemsetAsync(b.odo_off.p, 0, 10 * sizeof(int), s->ho->stream));
      hip_ok(hipMemsetAsync(b.vmeta.p, 0, VM_WORDS * sizeof(int), s->ho->stream));
      hip_ok(hipMemsetAsync(b.imu.p, 0, offsetof(SlamImuDev, data), s->ho->stream));          // mode 0: LiDAR-only
    }
  }
  hip_ok(s->chain.reserve(21 * sizeof(double)));
  // the buffers whose size follows the (slowly growing) surrounded clouds: start them where a re-allocation is years away
  const size_t floor_c = (size_t)1 << 20, floor_s = (size_t)1 << 22;
  hip_ok(s->map_c.reserve(floor_c * sizeof(float4))); hip_ok(s->map_s.reserve(floor_s * sizeof(float4)));
  hip_ok(s->hc->idx_cell_of.reserve(floor_c * sizeof(int))); hip_ok(s->hm->idx_cell_of.reserve(floor_s * sizeof(int)));
  hip_ok(s->hm->map_c.sorted.reserve(floor_c * sizeof(float4))); hip_ok(s->hm->map_c.pos_of.reserve(floor_c * sizeof(int)));
  hip_ok(s->hm->map_s.sorted.reserve(floor_s * sizeof(float4))); hip_ok(s->hm->map_s.pos_of.reserve(floor_s * sizeof(int)));
  hip_ok(s->meta.reserve(META_WORDS * sizeof(int)));
  hip_ok(s->vox_scratch.reserve(kVoxScratchBytes));
  hip_ok(s->rec_host.reserve(kSlamSlots * sizeof(msfl_slam_result)));
  for (int k = 0; k < kSlamSlots; k++) {
    hip_ok(s->rec[k].reserve(sizeof(msfl_slam_result)));
    hip_ok(hipEventCreateWithFlags(&s->ev_done[k], hipEventDisableTiming));
  }
  if (!st) {
    double init[21];
    for (int k = 0; k < 7; k++) { init[k] = init[7 + k] = k == 6 ? 1.0 : 0.0; init[14 + k] = cfg.pose_odom2map[k]; }   // pose_curr2last_, pose_scan2world_ = identity
    hip_ok(hipMemcpy(s->chain.p, init, sizeof(init), hipMemcpyHostToDevice));
    hip_ok(hipMemset(s->meta.p, 0, META_WORDS * sizeof(int)));
    hip_ok(hipStreamSynchronize(s->ho->stream));
  }
  if (st) { msfl_slam_destroy(s); return st; }
  if (const char* e = std::getenv("MSFL_SLAM_THREADS")) s->threaded = std::atoi(e) != 0;
  if (s->threaded) s->worker = std::thread(slam_worker_main, s);
  *out = s;
  return MSFL_OK;
}

msfl_status msfl_slam_get_result(msfl_slam* s, int scan_index, msfl_slam_result* result) {
  if (!s || !result) return MSFL_BAD_ARG;
  int slot;
  { const msfl_status rs = slam_slot_of(s, scan_index, "msfl_slam_get_result", &slot); if (rs) return rs; }
  { const msfl_status rs = slam_slot_ready(s, scan_index); if (rs) return rs; }
  { std::lock_guard<std::mutex> gl(s->mu_grid); slam_harvest(s, false); }
  *result = s->rec_host.as<msfl_slam_result>()[slot];
  return MSFL_OK;
}

msfl_status msfl_slam_set_uncertainty(msfl_slam* s, int enabled, double min_eigenvalue) {
  if (!s) return MSFL_BAD_ARG;
  if (enabled && !(min_eigenvalue >= 0.0)) return sfail(s, MSFL_BAD_ARG, "msfl_slam_set_uncertainty: negative or NaN min_eigenvalue");
  SHIP(s, hipSetDevice(s->ho->device));
  if (enabled) SHIP(s, s->unc.ensure(2 * sizeof(UncRecord)));
  s->unc_on = enabled != 0;             // read once per msfl_slam_add_scan: scans already fed keep what they were fed with
  s->opt[0].unc_min_eig = s->opt[1].unc_min_eig = enabled ? min_eigenvalue : 0.0;
  return MSFL_OK;
}

msfl_status msfl_slam_set_degeneracy(msfl_slam* s, int odometry, int mapping, double min_eig_odometry, double min_eig_mapping) {
  if (!s) return MSFL_BAD_ARG;
  if ((odometry && !(min_eig_odometry >= 0.0 && std::isfinite(min_eig_odometry))) || (mapping && !(min_eig_mapping >= 0.0 && std::isfinite(min_eig_mapping))))
    return sfail(s, MSFL_BAD_ARG, "msfl_slam_set_degeneracy: a threshold is negative or not finite");
  SHIP(s, hipSetDevice(s->ho->device));
  if (odometry || mapping) SHIP(s, s->degen.ensure(2 * sizeof(DegenRecord)));
  s->opt[0].degen_on = odometry != 0;   // read once per msfl_slam_add_scan, like msfl_slam_set_uncertainty
  s->opt[1].degen_on = mapping != 0;
  s->opt[0].degen_min_eig = odometry ? min_eig_odometry : 0.0;
  s->opt[1].degen_min_eig = mapping ? min_eig_mapping : 0.0;
  return MSFL_OK;
}

msfl_status msfl_slam_get_degeneracy(msfl_slam* s, int scan_index, msfl_degeneracy_record* odometry, msfl_degeneracy_record* mapping) {
  return slam_get_pair(s, &msfl_slam_s::degen, scan_index, "msfl_slam_get_degeneracy", "msfl_slam_set_degeneracy", odometry, mapping);
}

msfl_status msfl_slam_set_outlier_rejection(msfl_slam* s, const msfl_outlier_rejection* odometry, const msfl_outlier_rejection* mapping) {
  if (!s) return MSFL_BAD_ARG;
  const msfl_outlier_rejection* in[2] = {odometry, mapping};
  RejectOptions rej[2];
  for (int a = 0; a < 2; a++) {
    std::string err;
    const msfl_status rs = reject_options(in[a], a ? "msfl_slam_set_outlier_rejection (mapping)" : "msfl_slam_set_outlier_rejection (odometry)", &rej[a], &err);
    if (rs) return sfail(s, rs, err);
  }
  SHIP(s, hipSetDevice(s->ho->device));
  if (rej[0].mode || rej[1].mode) SHIP(s, s->rej.ensure(2 * sizeof(RejectRecord)));
  s->opt[0].rej = rej[0];               // read once per msfl_slam_add_scan, like msfl_slam_set_degeneracy
  s->opt[1].rej = rej[1];
  return MSFL_OK;
}

msfl_status msfl_slam_get_rejection(msfl_slam* s, int scan_index, msfl_rejection_record* odometry, msfl_rejection_record* mapping) {
  return slam_get_pair(s, &msfl_slam_s::rej, scan_index, "msfl_slam_get_rejection", "msfl_slam_set_outlier_rejection", odometry, mapping);
}

msfl_status msfl_slam_set_next_prior(msfl_slam* s, const msfl_pose_prior* odometry, const msfl_pose_prior* mapping) {
  if (!s) return MSFL_BAD_ARG;
  const msfl_pose_prior* in[2] = {odometry, mapping};
  for (int a = 0; a < 2; a++) {
    if (!in[a]) continue;
    const double* w = reinterpret_cast<const double*>(in[a]);
    for (int k = 0; k < kPriorWords; k++)
      if (!std::isfinite(w[k]))
        return sfail(s, MSFL_BAD_ARG, std::string("msfl_slam_set_next_prior: the ") + (a ? "mapping" : "odometry") + " prior has a non-finite entry");
  }
  SHIP(s, hipSetDevice(s->ho->device));
  if ((odometry || mapping) && !s->prior[0].p)
    for (auto& b : s->prior) SHIP(s, b.reserve(2 * sizeof(PosePrior)));
  for (int a = 0; a < 2; a++) {
    s->next_prior_set[a] = in[a] != nullptr;
    if (in[a]) s->next_prior[a] = *in[a];
  }
  return MSFL_OK;
}

msfl_status msfl_slam_set_map_window(msfl_slam* s, const int half_cells[3], int every_n_scans) {
  if (!s) return MSFL_BAD_ARG;
  if (!half_cells) { s->win_on = false; return MSFL_OK; }          // read once per msfl_slam_add_scan, like msfl_slam_set_uncertainty
  if (half_cells[0] < 0 || half_cells[1] < 0 || half_cells[2] < 0 || every_n_scans < 1)
    return sfail(s, MSFL_BAD_ARG, "msfl_slam_set_map_window: negative half_cells or every_n_scans < 1");
  SHIP(s, hipSetDevice(s->ho->device));
  SHIP(s, s->win.ensure(2 * CROP_WORDS * sizeof(int)));
  for (int a = 0; a < 3; a++) s->win_half[a] = half_cells[a];
  s->win_every = every_n_scans;
  s->win_on = true;
  return MSFL_OK;
}

msfl_status msfl_slam_get_map_window(msfl_slam* s, int scan_index, msfl_grid_crop_info* corner, msfl_grid_crop_info* surf) {
  if (!s) return MSFL_BAD_ARG;
  int slot;
  { const msfl_status rs = slam_slot_of(s, scan_index, "msfl_slam_get_map_window", &slot); if (rs) return rs; }
  if (corner) std::memset(corner, 0, sizeof(*corner));
  if (surf) std::memset(surf, 0, sizeof(*surf));
  if (!s->win.held[slot]) return MSFL_OK;                           // no crop ran on that scan
  { const msfl_status rs = slam_slot_ready(s, scan_index); if (rs) return rs; }
  const msfl_grid_crop_info* w = s->win.host_at<msfl_grid_crop_info>(slot);
  if (corner) *corner = w[0];
  if (surf) *surf = w[1];
  return MSFL_OK;
}

msfl_status msfl_slam_get_uncertainty(msfl_slam* s, int scan_index, msfl_match_uncertainty* odometry, msfl_match_uncertainty* mapping) {
  return slam_get_pair(s, &msfl_slam_s::unc, scan_index, "msfl_slam_get_uncertainty", "msfl_slam_set_uncertainty", odometry, mapping);
}

msfl_status msfl_slam_get_clouds(msfl_slam* s, int scan_index, msfl_slam_clouds* c, msfl_mem mem) {
  if (!s || !c) return MSFL_BAD_ARG;
  if (!s->cfg.keep_clouds) return sfail(s, MSFL_BAD_ARG, "msfl_slam_get_clouds: the pipeline was created without msfl_slam_config.keep_clouds");
  if (scan_index < 0 || scan_index >= s->n_scans || scan_index < s->n_scans - 2)
    return sfail(s, MSFL_BAD_ARG, "msfl_slam_get_clouds: the clouds of a scan are held until the scan after next is fed");
  const int slot = scan_index % kSlamSlots;                         // (its own window: the clouds live in the two buffer sets)
  { const msfl_status rs = slam_slot_ready(s, scan_index); if (rs) return rs; }
  const SlamScanBuf& b = s->sb[scan_index & 1];
  const msfl_slam_result& r = s->rec_host.as<msfl_slam_result>()[slot];
  const bool ok = r.status_extract == MSFL_OK;
  c->n_full = ok ? r.n_full : 0; c->n_sharp = ok ? r.n_sharp : 0; c->n_less_sharp = ok ? r.n_less_sharp : 0;
  c->n_flat = ok ? r.n_flat : 0; c->n_less_flat = ok ? r.n_less_flat : 0;
  const size_t nn = (size_t)s->n_cap;
  int* idx = const_cast<int*>(b.idx.as<int>());
  if (mem == MSFL_MEM_DEVICE) {
    c->full_scan = reinterpret_cast<msfl_point*>(b.full_scan.p); c->full_map = reinterpret_cast<msfl_point*>(b.full_map.p);
    c->ring = reinterpret_cast<uint16_t*>(b.fring.p);
    c->sharp_idx = idx; c->less_sharp_idx = idx + nn; c->flat_idx = idx + 2 * nn; c->less_flat_idx = idx + 3 * nn;
    return MSFL_OK;
  }
  hipStream_t st = s->ho->stream;
  if (c->full_scan && c->n_full) SHIP(s, hipMemcpyAsync(c->full_scan, b.full_scan.p, (size_t)c->n_full * sizeof(float4), hipMemcpyDeviceToHost, st));
  if (c->full_map && c->n_full) SHIP(s, hipMemcpyAsync(c->full_map, b.full_map.p, (size_t)c->n_full * sizeof(float4), hipMemcpyDeviceToHost, st));
  if (c->ring && c->n_full) SHIP(s, hipMemcpyAsync(c->ring, b.fring.p, (size_t)c->n_full * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
  int* dst[4] = {c->sharp_idx, c->less_sharp_idx, c->flat_idx, c->less_flat_idx};
  const int cnts[4] = {c->n_sharp, c->n_less_sharp, c->n_flat, c->n_less_flat};
  for (int l = 0; l < 4; l++)
    if (dst[l] && cnts[l]) SHIP(s, hipMemcpyAsync(dst[l], idx + (size_t)l * nn, (size_t)cnts[l] * sizeof(int), hipMemcpyDeviceToHost, st));
  SHIP(s, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_slam_grids(msfl_slam* s, msfl_grid** corner, msfl_grid** surf) {
  if (!s) return MSFL_BAD_ARG;
  SHIP(s, hipSetDevice(s->ho->device));
  if (s->n_scans > 0) {
    const msfl_status ws = slam_wait_mapped(s, s->n_scans - 1);
    bool poisoned;
    { std::lock_guard<std::mutex> lk(s->mu); poisoned = s->poisoned; }
    if (ws && !poisoned) return ws;
  }
  { std::lock_guard<std::mutex> gl(s->mu_grid); slam_harvest(s, true); }
  SHIP(s, hipStreamSynchronize(s->hm->stream));
  SHIP(s, hipStreamSynchronize(s->hc->stream));
  SHIP(s, hipStreamSynchronize(s->hv->stream));
  if (corner) *corner = s->gc;
  if (surf) *surf = s->gs;
  return MSFL_OK;
}

}  // extern "C"

namespace {

// Block until the mapping chain of scan `k` is on the streams (its ev_done recorded).  A failure inside the mapping thread
// poisons the pipeline: reported here to whoever waits next.
msfl_status slam_wait_mapped(msfl_slam* s, int k) {
  std::unique_lock<std::mutex> lk(s->mu);
  s->cv_done.wait(lk, [&] { return s->mapped_upto >= k || s->poisoned; });
  // a scan whose whole chain was enqueued before the failing one keeps its result (msfl_slam_add_scan_imu's contract)
  if (s->poisoned && !(s->mapped_upto >= k && k < s->poison_scan)) return s->poison_status;
  return MSFL_OK;
}

void slam_worker_main(msfl_slam* s) {
  for (;;) {
    SlamJob jb;
    {
      std::unique_lock<std::mutex> lk(s->mu);
      s->cv_job.wait(lk, [&] { return s->has_job || s->stop; });
      if (!s->has_job) return;                                    // stop, nothing queued
      jb = s->job;
    }
    const msfl_status st = slam_enqueue_mapping(s, jb);
    {
      std::lock_guard<std::mutex> lk(s->mu);
      s->has_job = false;
      s->mapped_upto = jb.k;
      if (st != MSFL_OK && !s->poisoned) {
        s->poisoned = true; s->poison_status = st; s->poison_scan = jb.k;
        std::lock_guard<std::mutex> le(s->mu_err);
        s->last_error = "msfl_slam: pipeline stopped by a failure in the mapping chain of scan " + std::to_string(jb.k) + " (" + s->last_error + ")";
      }
    }
    s->cv_done.notify_all();
  }
}

// The mapping chain of one scan (LaserMapping::Run, laser_mapping.cc:138-258), enqueued on the mapping / corner streams.  Runs on
// the mapping thread (or inline with MSFL_SLAM_THREADS=0); holds mu_grid: it advances the map stores' host-side bounds.
msfl_status slam_enqueue_mapping(msfl_slam* s, const SlamJob& jb) {
  std::lock_guard<std::mutex> grid_lock(s->mu_grid);
  const int k = jb.k, n = jb.n, imu_mode = jb.imu_mode, p = k & 1, slot = k % kSlamSlots;
  msfl_handle* hm = s->hm;
  SHIP(s, hipSetDevice(hm->device));
  if (k == s->fail_at) return sfail(s, MSFL_HIP_ERROR, "injected failure (MSFL_SLAM_FAIL_AT)");
  SlamScanBuf& cur = s->sb[p];
  hipStream_t sm = hm->stream;
  const auto t_start = std::chrono::steady_clock::now();
  SegClock seg{s->host_profile && k >= kSlamProfileSkip, &s->host_seg_map, t_start};   // host profile of this thread
  slam_harvest(s, false);
  msfl_slam_result* rec = s->rec[slot].as<msfl_slam_result>();
  const RegSinks map_sinks = slam_sinks(s, slot, 1, jb.o);
  const SlamImuDev* d_imu = cur.imu.as<SlamImuDev>();
  const int cap_ls = std::min(n, s->caps.less_sharp), cap_lf = std::min(n, s->caps.less_flat);
  double* chain = s->chain.as<double>();
  double* poses_k = cur.poses.as<double>();
  SHIP(s, hipStreamWaitEvent(sm, cur.ev_odo, 0));
  int* meta = s->meta.as<int>();
  int* cnt = cur.cnt.as<int>();
  double* odom2map = chain + 14;
  double* pose_map = poses_k + 7;
  hipLaunchKernelGGL(slam_map_pose_kernel, dim3(1), dim3(1), 0, sm, odom2map, (const double*)poses_k, pose_map, 0);          // TransformAssociateToMap
  SHIP(s, hipEventRecord(cur.ev_pose, sm));
  seg("  wait ev_odo + map pose kernel + record");
  msfl_handle* hc = s->hc;
  hipStream_t sc = hc->stream;
  const long long cap_c = std::max<long long>(s->gc->ub_points, 1), cap_s = std::max<long long>(s->gs->ub_points, 1);
  // generous floors (16 MB / 64 MB of 288 GB): growing a buffer is a hipFree + hipMalloc, i.e. a device synchronisation in the
  // middle of the pipeline, and the bounds creep up with the map
  SHIP(s, s->map_c.reserve(std::max<size_t>((size_t)cap_c, (size_t)1 << 20) * sizeof(float4)));
  SHIP(s, s->map_s.reserve(std::max<size_t>((size_t)cap_s, (size_t)1 << 22) * sizeof(float4)));
  // ---- corner side (own stream): GetSurroundedCloud (laser_mapping.cc:273-275), its kd-tree equivalent
  //      (mapping_scan_matcher.cc:66-69) into the mapping handle's corner index
  SHIP(s, hipStreamWaitEvent(sc, cur.ev_pose, 0));
  seg("  reserve + wait ev_pose");
  SCHK(s, hc, grid_surround_enqueue(s->gc, cur.map_ls.as<float4>(), nullptr, cap_ls, cnt + SC_USE_LS, pose_map,
                                    s->map_c.as<float4>(), (int)std::min<long long>(cap_c, INT32_MAX), meta + META_NMC));
  seg("  corner surround (3 kernels)");
  SCHK(s, hc, build_index(hc, s->map_c.as<float4>(), (int)std::min<long long>(cap_c, INT32_MAX), hm->map_c, meta + META_NMC));
  SHIP(s, hipEventRecord(cur.ev_cready, sc));
  seg("corner surround + index");
  // ---- surf side (mapping stream): GetSurroundedCloud (:276-278), index (:70-72)
  SCHK(s, hm, grid_surround_enqueue(s->gs, cur.map_lf.as<float4>(), nullptr, cap_lf, cnt + SC_USE_LF, pose_map,
                                    s->map_s.as<float4>(), (int)std::min<long long>(cap_s, INT32_MAX), meta + META_NMS));
  hm->have_map = false; hm->pr.resident = false;
  SCHK(s, hm, build_index(hm, s->map_s.as<float4>(), (int)std::min<long long>(cap_s, INT32_MAX), hm->map_s, meta + META_NMS));
  hm->have_map = true;
  seg("surf surround + index");
  SHIP(s, hipStreamWaitEvent(sm, cur.ev_cready, 0));
  SHIP(s, hipStreamWaitEvent(sm, cur.ev_vox, 0));
  const int* vm = cur.vmeta.as<int>();
  hipLaunchKernelGGL(slam_map_gate_kernel, dim3(1), dim3(1), 0, sm, (const int*)(meta + META_NMC), (const int*)(meta + META_NMS), s->cfg.min_map_corner,
                     s->cfg.min_map_surf, vm + VM_MC, vm + VM_MS, vm + VM_FC, vm + VM_FS, cnt, meta + META_OFF, meta + META_STATUS, d_imu, pose_map);
  if (imu_mode == 2) {
    // is_initialized (mapping_scan_matcher.cc:100-121,154-166,183-191,224-236): GetDeltaQP per down-sampled feature, Deskew factors
    const size_t n_c = (size_t)std::max(1, cap_ls), n_s = (size_t)n;
    SHIP(s, cur.dqp.reserve(7 * (n_c + n_s) * sizeof(double)));
    double* dq_c = cur.dqp.as<double>(); double* dp_c = dq_c + 4 * n_c; double* dq_s = dp_c + 3 * n_c; double* dp_s = dq_s + 4 * n_s;
    hipLaunchKernelGGL(slam_delta_qp_kernel, dim3(std::max(1, div_up(std::max(cap_ls, n), 256)), 2), dim3(256), 0, sm, d_imu, (const float4*)cur.vox_c.as<float4>(),
                       (const float4*)cur.vox_s.as<float4>(), (const int*)(meta + META_OFF), cap_ls, n, dq_c, dp_c, dq_s, dp_s);
    DeskewView dv{};
    dv.corner_dq = dq_c; dv.corner_dp = dp_c; dv.surf_dq = dq_s; dv.surf_dp = dp_s;
    dv.V = d_imu->velocity; dv.G_dev = d_imu->gravity;
    SCHK(s, hm, scan2map_dyn(hm, cur.vox_c.as<float4>(), cur.vox_s.as<float4>(), meta + META_OFF, cap_ls, n, pose_map, meta + META_STATUS, map_sinks, &dv));
  } else {
    SCHK(s, hm, scan2map_dyn(hm, cur.vox_c.as<float4>(), cur.vox_s.as<float4>(), meta + META_OFF, cap_ls, n, pose_map, meta + META_STATUS, map_sinks));
  }
  hipLaunchKernelGGL(slam_map_pose_kernel, dim3(1), dim3(1), 0, sm, odom2map, (const double*)poses_k, pose_map, 1);          // TransformUpdate
  if (imu_mode == 2)    // DoUndistort (laser_mapping.cc:197-211) on the clouds InsertScan2Map is about to insert
    hipLaunchKernelGGL(slam_deskew_kernel, dim3(std::max(1, div_up(std::max(cap_ls, cap_lf), 256)), 2), dim3(256), 0, sm, d_imu, (const double*)poses_k,
                       (const int*)cnt, cur.map_ls.as<float4>(), cap_ls, cur.map_lf.as<float4>(), cap_lf);
  if (s->cfg.keep_clouds)   // cloud_full_res after this scan's IMU passes + TransformPointCloud by pose_map_scan2world_ (laser_mapping.cc:206,214-217)
    hipLaunchKernelGGL(slam_full_cloud_kernel, dim3(std::max(1, div_up(n, 256))), dim3(256), 0, sm, d_imu, (const double*)poses_k, (const double*)pose_map, cnt,
                       (const float4*)cur.full.as<float4>(), n, cur.full_scan.as<float4>(), cur.full_map.as<float4>());
  SHIP(s, hipEventRecord(cur.ev_match, sm));
  seg("gate + scan-to-map");
  // InsertScan2Map (:330-338): TransformPointCloud by the refined pose inside the insert's key kernel; corner store on its
  // own stream again, joined before the record is assembled
  const long long seq_c0 = s->gc->last_seq, seq_s0 = s->gs->last_seq;
  SHIP(s, hipStreamWaitEvent(sc, cur.ev_match, 0));
  SCHK(s, hc, grid_insert_enqueue(s->gc, cur.map_ls.as<float4>(), cap_ls, cnt + SC_USE_LS, pose_map, rec->grid_corner));
  int* win = jb.o.crop ? s->win.dev[slot].as<int>() : nullptr;          // msfl_slam_set_map_window: each store forgets what lies outside the window
  if (jb.o.crop) SCHK(s, hc, grid_crop_enqueue(s->gc, pose_map, jb.o.half, nullptr, 0, win, rec->grid_corner, true));
  SHIP(s, hipEventRecord(cur.ev_cdone, sc));
  seg("corner insert");
  SCHK(s, hm, grid_insert_enqueue(s->gs, cur.map_lf.as<float4>(), cap_lf, cnt + SC_USE_LF, pose_map, rec->grid_surf));
  if (jb.o.crop) SCHK(s, hm, grid_crop_enqueue(s->gs, pose_map, jb.o.half, nullptr, 0, win + CROP_WORDS, rec->grid_surf, true));
  SHIP(s, hipStreamWaitEvent(sm, cur.ev_cdone, 0));
  seg("surf insert");
  s->seq_c[slot] = s->gc->last_seq != seq_c0 ? s->gc->last_seq : 0;
  s->seq_s[slot] = s->gs->last_seq != seq_s0 ? s->gs->last_seq : 0;
  hipLaunchKernelGGL(slam_result_kernel, dim3(1), dim3(1), 0, sm, rec, k, cnt, (const double*)poses_k, (const double*)odom2map, (const int*)meta, vm,
                     (const int*)cur.odo_status.as<int>());
  SHIP(s, hipGetLastError());
  SHIP(s, hipMemcpyAsync(s->rec_host.as<msfl_slam_result>() + slot, rec, sizeof(msfl_slam_result), hipMemcpyDeviceToHost, sm));
  for (const SlotRecords* r : {&s->unc, &s->degen, &s->rej, &s->win}) SHIP(s, r->fetch(slot, sm));   // what the scan was fed with travels along
  SHIP(s, hipEventRecord(s->ev_done[slot], sm));
  seg("record");
  s->applied[slot] = false;
  if (s->host_profile && k >= kSlamProfileSkip) s->host_map_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  return MSFL_OK;
}

msfl_status slam_add_scan_impl(msfl_slam* s, const msfl_point* pts, const uint16_t* ring, int n, msfl_mem mem, const msfl_slam_imu* imu,
                               msfl_slam_result* result) {
  if (n < 1 || !pts || !ring) return sfail(s, MSFL_BAD_ARG, "msfl_slam_add_scan: empty scan or null array");
  if (n > s->n_cap) return sfail(s, MSFL_CAPACITY, "msfl_slam_add_scan: more points than msfl_slam_config.max_scan_points");
  // this scan's IMU inputs: 0 none (LiDAR-only), 1 UndistortScan (estimator not initialised), 2 is_initialized
  const msfl_preintegration* pre = imu ? imu->pre : nullptr;
  const int imu_mode = pre ? (imu->is_initialized ? 2 : 1) : 0;
  if (pre) {
    if (pre->n < 2 || !pre->sum_dt || !pre->delta_q || !pre->delta_p)
      return sfail(s, MSFL_BAD_ARG, "msfl_slam_add_scan_imu: a pre-integration needs at least 2 samples");
    if (pre->n > kSlamImuMaxSamples) return sfail(s, MSFL_CAPACITY, "msfl_slam_add_scan_imu: more than 2048 pre-integration samples");
    for (int i = 1; i < pre->n; i++)
      if (!(pre->sum_dt[i] >= pre->sum_dt[i - 1])) return sfail(s, MSFL_BAD_ARG, "msfl_slam_add_scan_imu: sum_dt must be non-decreasing");
  }
  msfl_handle* ho = s->ho;
  SHIP(s, hipSetDevice(ho->device));
  const int k = s->n_scans, p = k & 1, q = 1 - p, slot = k % kSlamSlots;
  s->adding_scan = k;
  SlamScanBuf& cur = s->sb[p];
  SlamScanBuf& last = s->sb[q];
  hipStream_t so = ho->stream;
  // at most two scans in flight: scan k - 2 used this buffer set (and this pinned staging), its record must be out
  const auto t_call = std::chrono::steady_clock::now();
  if (k >= 2) {
    { const msfl_status ws = slam_wait_mapped(s, k - 2); if (ws) return ws; }   // its ev_done must have been RECORDED before it can be waited for
    SHIP(s, hipEventSynchronize(s->ev_done[(k - 2) % kSlamSlots]));
  }
  const auto t_free = std::chrono::steady_clock::now();
  SegClock seg{s->host_profile && k >= kSlamProfileSkip, &s->host_seg, t_free};
  msfl_slam_result* rec = s->rec[slot].as<msfl_slam_result>();
  s->enqueueing = true;                 // from here on a failure leaves work of this scan on the streams: the pipeline is poisoned
  SHIP(s, hipMemsetAsync(rec, 0, sizeof(msfl_slam_result), so));
  SlamScanOptions o;
  o.odo = s->opt[0]; o.map = s->opt[1];
  o.unc = s->unc_on;
  o.degen_any = o.odo.degen_on || o.map.degen_on;
  o.rej_any = o.odo.rej.mode != MSFL_REJECT_OFF || o.map.rej.mode != MSFL_REJECT_OFF;
  o.prior_odo = s->next_prior_set[0]; o.prior_map = s->next_prior_set[1];   // msfl_slam_set_next_prior: consumed by this scan, whatever becomes of it
  s->next_prior_set[0] = s->next_prior_set[1] = false;
  o.crop = s->win_on && (k + 1) % s->win_every == 0;
  for (int a = 0; a < 3; a++) o.half[a] = s->win_half[a];
  SHIP(s, s->unc.arm(slot, o.unc, true, so));         // scan 0 has no odometry match, a closed gate no mapping match
  SHIP(s, s->degen.arm(slot, o.degen_any, true, so));
  SHIP(s, s->rej.arm(slot, o.rej_any, true, so));
  SHIP(s, s->win.arm(slot, o.crop, false, so));       // (a crop will run on this scan; its reports are not cleared first)
  if (o.prior_odo || o.prior_map) SHIP(s, ho->pin.upload(s->prior[slot].p, s->next_prior, 2 * sizeof(PosePrior), so));
  if (imu_mode != 0 || cur.imu_mode != 0) {
    // SlamImuDev header + [sum_dt n | delta_q 4n | delta_p 3n] in one copy (pinned ring slot: the caller's arrays are free on return)
    const size_t np = pre ? (size_t)pre->n : 0, head = offsetof(SlamImuDev, data) / sizeof(double);
    s->imu_stage.assign(head + 8 * np, 0.0);
    SlamImuDev* hd = reinterpret_cast<SlamImuDev*>(s->imu_stage.data());
    hd->mode = imu_mode; hd->n = (int)np;
    if (imu_mode) {
      for (int a = 0; a < 3; a++) { hd->velocity[a] = imu->velocity[a]; hd->gravity[a] = imu->gravity[a]; }
      for (int a = 0; a < 7; a++) hd->presolved[a] = imu->presolved_pose[a];
      std::memcpy(hd->data, pre->sum_dt, np * sizeof(double));
      std::memcpy(hd->data + np, pre->delta_q, 4 * np * sizeof(double));
      std::memcpy(hd->data + 5 * np, pre->delta_p, 3 * np * sizeof(double));
    }
    SHIP(s, ho->pin.upload(cur.imu.p, s->imu_stage.data(), s->imu_stage.size() * sizeof(double), so));
    cur.imu_mode = imu_mode;
  }
  const SlamImuDev* d_imu = cur.imu.as<SlamImuDev>();
  // ---------------- odometry thread: stage A, feature clouds, stage B, pose chain ----------------
  const float4* d_pts = reinterpret_cast<const float4*>(pts);
  const uint16_t* d_ring = ring;
  if (mem == MSFL_MEM_HOST) {
    const size_t bp = (size_t)n * sizeof(float4), br = (size_t)n * sizeof(uint16_t);
    SHIP(s, cur.upload.reserve(bp + br));
    SHIP(s, cur.in_pts.reserve(bp)); SHIP(s, cur.in_ring.reserve(br));
    std::memcpy(cur.upload.p, pts, bp);
    std::memcpy(cur.upload.as<char>() + bp, ring, br);
    SHIP(s, hipMemcpyAsync(cur.in_pts.p, cur.upload.p, bp, hipMemcpyHostToDevice, so));
    SHIP(s, hipMemcpyAsync(cur.in_ring.p, cur.upload.as<char>() + bp, br, hipMemcpyHostToDevice, so));
    d_pts = cur.in_pts.as<float4>(); d_ring = cur.in_ring.as<uint16_t>();
  }
  cur.n = n;
  seg("harvest + staging + upload");
  {
    ExtractView v{};
    int* idx = cur.idx.as<int>(); int* cnt = cur.cnt.as<int>();
    const size_t nc = (size_t)s->n_cap;
    v.full_pts = cur.full.as<float4>(); v.full_ring = cur.fring.as<uint16_t>(); v.curvature = cur.curv.as<float>(); v.label = cur.label.as<uint8_t>();
    v.sharp_idx = idx; v.less_sharp_idx = idx + nc; v.flat_idx = idx + 2 * nc; v.less_flat_idx = idx + 3 * nc;
    v.n_full = cnt + SC_FULL; v.n_sharp = cnt + SC_SHARP; v.n_less_sharp = cnt + SC_LESS_SHARP; v.n_flat = cnt + SC_FLAT; v.n_less_flat = cnt + SC_LESS_FLAT;
    v.status = cnt + SC_STATUS;
    const int h_off[2] = {0, n};
    SCHK(s, ho, extract_device(ho, 1, d_pts, d_ring, h_off, nullptr, v));
    seg("  extract_device (2 small copies, 4 kernels)");
    SCHK(s, ho, (ho->pin.upload(cur.ex_off.p, h_off, sizeof(h_off), so) == hipSuccess ? MSFL_OK : fail(ho, MSFL_HIP_ERROR, "offset upload")));   // the mapping thread's copy of [0, n]
    const int gather_blocks = div_up(std::max(std::max(s->caps.sharp, s->caps.less_sharp), std::max(s->caps.flat, std::min(n, s->caps.less_flat))), 256);
    hipLaunchKernelGGL(slam_gather_kernel, dim3(std::max(1, gather_blocks), 4), dim3(256), 0, so, (const float4*)v.full_pts, (const uint16_t*)v.full_ring,
                       (const int*)v.sharp_idx, (const int*)v.less_sharp_idx, (const int*)v.flat_idx, (const int*)v.less_flat_idx, cnt, s->caps,
                       cur.sharp.as<float4>(), cur.ls.as<float4>(), cur.ls_ring.as<uint16_t>(), cur.flat.as<float4>(), cur.lf.as<float4>(),
                       cur.lf_ring.as<uint16_t>(), k > 0 ? (const int*)last.cnt.as<int>() : (const int*)nullptr, s->caps, cur.odo_off.as<int>(), cur.odo_status.as<int>(),
                       d_imu, cur.map_ls.as<float4>(), cur.map_lf.as<float4>(), s->cfg.reference_quirks ? 1 : 0);
    SHIP(s, hipGetLastError());
    SHIP(s, hipEventRecord(cur.ev_feat, so));
  }
  seg("extraction + gather");
  const int cap_ls = std::min(n, s->caps.less_sharp);
  // ---------------- mapping thread, ahead of its turn: the voxel filters 0.2 m / 0.4 m of the scan's less-sharp / less-flat lists
  //                  (laser_mapping.cc:264-270) depend on the feature lists alone; they run next to the scan-to-scan match
  {
    msfl_handle* hv = s->hv;
    const int* cnt = cur.cnt.as<int>(); int* vm = cur.vmeta.as<int>();
    SHIP(s, hipStreamWaitEvent(hv->stream, cur.ev_feat, 0));
    // on the mapping thread's copies of the two lists (the same points in the same order as full[idx[k]]; undistorted when IMU data came)
    SCHK(s, hv, voxel_dyn(hv, cur.map_ls.as<float4>(), nullptr, cur.ex_off.as<int>(), cnt + SC_USE_LS, cap_ls, s->cfg.leaf_corner, cur.vox_c.as<float4>(),
                          cur.vsum_c.as<float4>(), vm + VM_MC, vm + VM_FC, s->vox_scratch.p, &s->vox_big));
    SCHK(s, hv, voxel_dyn(hv, cur.map_lf.as<float4>(), nullptr, cur.ex_off.as<int>(), cnt + SC_USE_LF, n, s->cfg.leaf_surf, cur.vox_s.as<float4>(),
                          cur.vsum_s.as<float4>(), vm + VM_MS, vm + VM_FS, s->vox_scratch.p, &s->vox_big));
    SHIP(s, hipEventRecord(cur.ev_vox, hv->stream));
  }
  seg("voxel filters");
  double* chain = s->chain.as<double>();
  double* poses_k = cur.poses.as<double>();
  if (k > 0) {                                                   // laser_odometry.cc:72-75: the first scan only initialises
    SCHK(s, ho, scan2scan_dyn(ho, last, cur, s->caps, chain, slam_sinks(s, slot, 0, o)));
  }
  hipLaunchKernelGGL(slam_odom_pose_kernel, dim3(1), dim3(1), 0, so, (const double*)chain, chain + 7, poses_k, poses_k + 14,
                     (const int*)cur.cnt.as<int>(), k == 0 ? 1 : 0);
  SHIP(s, hipGetLastError());
  SHIP(s, hipEventRecord(cur.ev_odo, so));
  seg("scan-to-scan + pose");
  // ---------------- hand the mapping chain to the mapping thread (or run it here) ----------------
  s->n_scans = k + 1;
  if (s->host_profile && k >= kSlamProfileSkip) {
    s->host_wait_s += std::chrono::duration<double>(t_free - t_call).count();
    s->host_enqueue_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_free).count();
  }
  SlamJob job;
  job.k = k; job.n = n; job.imu_mode = imu_mode; job.o = o;
  if (s->threaded) {
    std::unique_lock<std::mutex> lk(s->mu);
    s->cv_done.wait(lk, [&] { return !s->has_job; });            // the mapping thread is at most one scan behind
    s->job = job; s->has_job = true;
    lk.unlock();
    s->cv_job.notify_one();
  } else {
    const msfl_status ms = slam_enqueue_mapping(s, job);
    { std::lock_guard<std::mutex> lk(s->mu); s->mapped_upto = k; }
    if (ms) return ms;
  }
  s->enqueueing = false;
  if (result) return msfl_slam_get_result(s, k, result);
  return MSFL_OK;
}

}  // namespace

extern "C" {

msfl_status msfl_slam_add_scan_imu(msfl_slam* s, const msfl_point* pts, const uint16_t* ring, int n, msfl_mem mem, const msfl_slam_imu* imu,
                                   msfl_slam_result* result) {
  if (!s) return MSFL_BAD_ARG;
  { std::lock_guard<std::mutex> lk(s->mu); if (s->poisoned) return s->poison_status; }   // last_error keeps the original failure
  s->enqueueing = false;
  const msfl_status st = slam_add_scan_impl(s, pts, ring, n, mem, imu, result);
  if (st != MSFL_OK && s->enqueueing) {
    std::lock_guard<std::mutex> lk(s->mu);
    // part of this scan's chain is on the streams, the stores' host-side bounds and table parity may have advanced, the slot's
    // events and sequence numbers have not: nothing consistent can follow.  Refuse every later scan (msfl_slam_get_result of
    // earlier scans and msfl_slam_destroy still work).
    // (with MSFL_SLAM_THREADS=1 the mapping thread may have poisoned the pipeline at an EARLIER scan while this call was under way: the first
    // failure keeps its scan number, status and text, so that slam_wait_mapped goes on refusing that earlier scan's result -- ADVICE r05)
    if (!s->poisoned) {
      s->poisoned = true; s->poison_status = st; s->poison_scan = s->adding_scan;
      std::lock_guard<std::mutex> le(s->mu_err);
      s->last_error = "msfl_slam: pipeline stopped by a failure in the middle of scan " + std::to_string(s->adding_scan) + " (" + s->last_error + ")";
    }
  }
  return st;
}

msfl_status msfl_slam_add_scan(msfl_slam* s, const msfl_point* pts, const uint16_t* ring, int n, msfl_mem mem, msfl_slam_result* result) {
  return msfl_slam_add_scan_imu(s, pts, ring, n, mem, nullptr, result);
}

}  // extern "C"
