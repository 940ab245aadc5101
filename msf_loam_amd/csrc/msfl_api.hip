// msfl_api.hip — C-ABI implementation (include/msfl_c_api.h) over the HIP kernels.
//
// One handle = one HIP stream + all device scratch; no global state, so the reference's two
// matcher instances (odometry thread / mapping thread) map to two independent handles.
// There is NO CPU fallback: every entry point either runs the gfx950 kernels or returns an
// error status.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <utility>
#include <chrono>
#include <string>
#include <vector>

#include <condition_variable>
#include <mutex>
#include <thread>

#include "../../include/msfl_c_api.h"
#include "msfl_kernels.cuh"
#include "msfl_extract.cuh"
#include "msfl_odom.cuh"
#include "msfl_grid.cuh"
#include "msfl_carve.cuh"
#include "msfl_keyframes.cuh"   // includes msfl_keyframes_host.h
#include "msfl_deskew.cuh"
#include "msfl_uncertainty.cuh"
#include "msfl_degeneracy.cuh"
#include "msfl_reject.cuh"

using namespace msfl;

namespace {

// The three buffer kinds own what they hold: destroying a handle, a map store or a SLAM session frees every one of their members
// (the owner makes its device current first).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }   // grow_keep
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    size_t want = std::max(bytes, cap + cap / 2);          // geometric growth: a buffer that grows a little per call
    want = (want + 255) & ~size_t(255);                    // (the map store's) is not reallocated on every call
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Ring of pinned host staging slots for small metadata uploads (offset tables, init words).
// hipMemcpyAsync from PAGEABLE memory may read the source after the call returns when the stream
// is busy, so metadata must live in pinned memory that stays untouched until its copy has run.
struct PinSlot { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
struct PinRing {
  static constexpr int kSlots = 8;
  PinSlot slot[kSlots];
  int next = 0;
  PinRing() = default;
  PinRing(const PinRing&) = delete;
  PinRing& operator=(const PinRing&) = delete;
  ~PinRing() { release(); }
  hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t st) {
    PinSlot& s = slot[next];
    next = (next + 1) % kSlots;
    hipError_t e;
    if (s.pending) { e = hipEventSynchronize(s.ev); if (e != hipSuccess) return e; s.pending = false; }
    if (bytes > s.cap) {
      // generous floor and geometric growth: growing a slot costs a hipHostFree + hipHostMalloc (tens of milliseconds, and
      // it happened once per slot as soon as a (B+1)-int offset table of a 1 024-scan batch met a 4 KB slot)
      const size_t want = (std::max<size_t>(std::max(bytes, s.cap + s.cap / 2), 256 * 1024) + 4095) & ~size_t(4095);
      if (s.p) { e = hipHostFree(s.p); if (e != hipSuccess) return e; s.p = nullptr; s.cap = 0; }
      e = hipHostMalloc(&s.p, want, hipHostMallocDefault); if (e != hipSuccess) return e;
      s.cap = want;
    }
    if (!s.ev) { e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming); if (e != hipSuccess) return e; }
    std::memcpy(s.p, src, bytes);
    e = hipMemcpyAsync(dst, s.p, bytes, hipMemcpyHostToDevice, st); if (e != hipSuccess) return e;
    e = hipEventRecord(s.ev, st); if (e != hipSuccess) return e;
    s.pending = true;
    return hipSuccess;
  }
  void release() {
    for (auto& s : slot) {
      if (s.pending) (void)hipEventSynchronize(s.ev);
      if (s.ev) (void)hipEventDestroy(s.ev);
      if (s.p) (void)hipHostFree(s.p);
      s = PinSlot{};
    }
  }
};

// Pinned host buffer for small synchronous read-backs (counts, offsets, descriptors): a D2H copy into pageable
// memory goes through the runtime's staging path, which stalls for tens of milliseconds once in a while.
struct PinBuf {
  void* p = nullptr; size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    const size_t want = (std::max<size_t>(std::max(bytes, cap + cap / 2), 4096) + 4095) & ~size_t(4095);
    if (p) { hipError_t e = hipHostFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct MapIndex {
  DevBuf gdesc;        // GridDesc, computed on the device (no host round trip in msfl_set_map)
  DevBuf bbox;         // 6 ordered ints, armed once and re-armed by every build's last launch (grid_build_done)
  int cap_cells = 0;   // capacity of cell_start / count (cells)
  PinBuf want;         // one int the build's last launch writes: the table size the bounding box wanted, feedback for the span of the
  int span = 0;        // NEXT build's table (read whenever the next build starts, never waited for)
  DevBuf sorted;      // float4[n]
  DevBuf pos_of;      // int[n]: original index -> position in `sorted`
  DevBuf cell_start;  // int[n_cells + 1]
  int n_input = 0;    // points handed to msfl_set_map
};

// ---- The handle's scratch, one set per family of calls.  Host-memory calls stage their arrays into these (stage_in / stage_out);
// device-memory calls use only the tables and work areas.  A buffer keeps its contents only until the next call that reserves it.
struct ExtractScratch {      // msfl_extract_features*: extract_device / extract_batch_impl
  DevBuf in_pts;             // float4[n_total]: staged input points (host mode)
  DevBuf in_ring;            // u16[n_total]: staged input rings (host mode)
  DevBuf off;                // int[B + 1]: scan offsets relative to the first scan, uploaded by extract_device
  DevBuf pack;               // bytes: ALL outputs of a host-mode call, carved by extract_batch_impl (one read-back for a small call)
  DevBuf status;             // int[B]: per-scan status of a device-mode call whose caller passed none
  DevBuf gap;                // u8[n_total]: neighbour-gap flags, written by the prepare kernels
  DevBuf ring_tab;           // int[B x (kMaxRings + 1)]: ring starts per scan, written by the prepare kernels
  DevBuf tmp_idx;            // int[4 n_total]: candidate lists of the pick kernel
  DevBuf ring_cnt;           // int[B x kMaxRings x 4]: picks per ring and list
  DevBuf split;              // bytes: PrepSplitView of the several-workgroups ring split (prep_split_bytes)
};
struct OdomIndexBufs {       // the column index over the previous scans of one feature family (OdomIndex, built by launch_odom_bin)
  DevBuf tab;                // unsigned[B x kOdomTabStride]: column tables
  DevBuf sorted;             // float4[points]: the clouds in column order
  DevBuf desc;               // OdomPairDesc[B]
  DevBuf mode;               // int[B]: 0 = the pair's queries walk the index, else they stay on the brute-force kernel
};
struct OdomScratch {         // msfl_match_scan2scan*, and the index sets of the SLAM step's scan-to-scan
  DevBuf pts[4];             // float4: staged last less-sharp, last less-flat, current sharp, current flat (host mode)
  DevBuf ring[2];            // u16: staged rings of the two last-scan clouds (host mode)
  DevBuf offs;               // int[5 (B + 1)]: [less-sharp | less-flat | sharp | flat | record] offsets
  DevBuf poses;              // double[7 B]: staged poses (host mode)
  DevBuf status;             // int[B]: status of a host-mode call, or of a device-mode call whose caller passed none
  DevBuf split;              // the several-workgroups index build: unsigned cursors [jobs x kOdomTabStride], then int partials [jobs x G x 8]
  OdomIndexBufs planes;      // over the last less-flat clouds
  OdomIndexBufs edges;       // over the last less-sharp clouds
};
struct VoxelLdsSet {         // what one list of the per-cloud LDS form (and the big form behind it) works in
  DevBuf staging;            // float4[n_total]: centroids per cloud before compaction.  Device-wide form (`set` only): int[3 runs], voxel-head
                             // flags, their scan, head positions
  DevBuf run_sums;           // float4[n_total]: per-run sums.  Device-wide form (`set` only): int[runs + 1], first slot of every run (run_first)
  DevBuf tables;             // int[3 B + 3]: [voxels per cloud B | flags B | out_off B + 1].  Device-wide form (`set` only):
                             // [n_valid B | in_off B + 1 | out_off B + 1 | max_cells 1]
};
struct VoxelScratch {        // msfl_voxel_downsample*
  DevBuf pts, idx, cnt;      // float4[n_total], int[n_total], int[B]: staged points, index list, per-cloud counts (host mode)
  DevBuf off;                // int[B + 1]: cloud offsets
  DevBuf desc;               // VoxelCloudDesc[B]: device-wide form
  DevBuf keys[2], vals[2];   // u64[runs], unsigned[runs], in and out of the radix sort: device-wide form
  DevBuf flag;               // int[2 n_valid]: run-head flags and their scan: device-wide form
  DevBuf out;                // float4: filtered points of a host-mode call before they go back
  VoxelLdsSet set;           // the single-list call, and list b of the pair form
  VoxelLdsSet set_a;         // list a of the pair form
  DevBuf off_a;              // int[B + 1]: the pair form's cloud offsets
  DevBuf big_scratch;        // the one-workgroup form for lists of 65 536 .. 131 071 points: per-workgroup record areas, then order areas
  DevBuf big_list;           // int[refused clouds]: the clouds that form walks
};
struct PointPassScratch {    // msfl_delta_qp, msfl_deskew_cloud, msfl_undistort_cloud, msfl_transform_cloud; msfl_voxel_downsample's fallback
  DevBuf pre;                // double[8 n]: pre-integration samples [sum_dt | dq | dp] (stage_preintegration); msfl_transform_cloud: its pose, double[7]
  DevBuf pts;                // float4[n]: staged points (host mode); the fallback's compacted finite points
  DevBuf dq;                 // double[4 n]: msfl_delta_qp's staged output (host mode); the fallback's filtered points, float4[n]
  DevBuf dp;                 // double[3 n]: msfl_delta_qp's staged output (host mode)
  DevBuf flag;               // one int: a time outside the pre-integration span was seen; the fallback's count of finite points
};
struct DeskewScratch {       // msfl_match_scan2map_deskew*: the staged msfl_deskew_batch arrays (host mode)
  DevBuf corner_dq, corner_dp, surf_dq, surf_dp;   // double[4 n_corner], [3 n_corner], [4 n_surf], [3 n_surf]
  DevBuf velocity;           // double[3 B]
};
struct PairScratch {         // msfl_set_pair_maps / msfl_match_pairs_batch: build_pair_index, and what the host remembers of the index
  DevBuf off_c, base_c;      // int[P + 1] each: corner-map offsets and cell-table bases
  DevBuf off_s, base_s;      // ... of the surf maps
  DevBuf bbox;               // int[6 P]: per-pair bounding boxes (not MapIndex::bbox: that one is the single-map build's)
  bool resident = false;     // h->map_c / map_s and the four tables above hold a pair index (every other writer of the maps clears it)
  std::vector<int> n_c, n_s; // its P pairs' map point counts per kind
};
struct ScoreScratch {        // msfl_score_poses*: no other call touches these, so a matcher call after it finds the handle as it left it
  DevBuf corner, surf;       // float4: staged clouds (host mode)
  DevBuf poses;              // double[7 H]: staged hypotheses (host mode)
  DevBuf off;                // int[3 (n_scans + 1)]: [corner | surf | pose] offsets; msfl_score_pairs: then int[2 P], where the pairs' map clouds begin
  DevBuf rec;                // ScoreRec[H]: staged results (host mode)
  DevBuf d2, nn;             // float / int [H x features]: staged per-feature outputs (host mode, single scan)
  DevBuf scan;               // int[H]: scan of every hypothesis (batch form), written by score_init_kernel
  DevBuf out0;               // u64[P]: msfl_score_pairs' first d2_out / nn_out element of every pair (ScorePairsView::out0)
};
struct SearchScratch {       // msfl_search_poses / msfl_search_pairs / msfl_relocalize: no other call touches these.  msfl_search_pairs holds
                             // every array below C times, C the pairs of one chunk (SearchPairsView), and qtab for all its pairs
  DevBuf corner, surf;       // float4: staged clouds (host mode)
  DevBuf vol;                // u64: the raw volumes [corner | surf], then with dilate = 1 the dilated ones
  DevBuf tab;                // int4[n_yaw x features]: voxel of every feature at every yaw sample
  DevBuf hits;               // int[2 H]: the counts when the caller gave no device array for them
  DevBuf peaks;              // u64[H]: keys of the peaks
  DevBuf ctr;                // int[2]: peaks appended, candidates written
  DevBuf qtab;               // double[4 n_yaw + 7]: the yaw samples' quaternions, then the guess
  DevBuf cand;               // SearchCand[1024]: the select kernel's records
  DevBuf pair;               // SearchPair[P]: msfl_search_pairs' per-pair table
  DevBuf rl_cand, rl_poses, rl_scores, rl_status, rl_corner, rl_surf;   // msfl_relocalize on device clouds: what its chained calls read and write
};
struct SegmentScratch {      // msfl_segment_scan*: allocated by the first call, no other call touches these
  DevBuf in_pts, in_ring;    // float4[n_total], u16[n_total]: staged sensor clouds (host mode)
  DevBuf out_cls, out_seg, out_masked;   // u8 / int / float4 [n_total]: the outputs before they go back (host mode)
  DevBuf off;                // int[n_scans + 1]: scan offsets into the arrays the kernels see
  DevBuf tab;                // float: cc, cs [n_col / 2 each], vs, vc [n_row - 1 each] (msfl_segment_tables)
  DevBuf img;                // the images of one chunk of scans (SegImages; kSegPixelBytes per pixel)
  DevBuf ctr;                // int[SEG_CTR_WORDS x chunk scans]: the counters of the chunk in flight
  DevBuf info;               // int[SEG_INFO_WORDS x n_scans]: the info records before they are read back
};
struct NoveltyScratch {      // msfl_grid_render / msfl_scan_novelty / msfl_grids_scan_novelty: allocated by the first call, no other call touches these
  DevBuf img;                // u32[n_col x n_row]: the map image of a host-memory call, and of a composite call without map_img_out
  DevBuf win;                // u32 mlim[npix], then int support[npix]: the window's minimum and support per pixel
  DevBuf tab;                // float: cc, cs [n_col / 2 each], ec, es [n_row + 1 each] (msfl_carve_tables) of tab_cfg
  DevBuf ctr;                // int[NOV_CTR_WORDS]: msfl_novelty_info, then msfl_grid_render_info, as the kernels count them
  DevBuf pose;               // double[8]: the pose of a host-memory call
  DevBuf in_scan, out_cls, out_masked;   // float4 / u8 / float4 [n]: the staged scan and the outputs before they go back (host mode)
  msfl_carve_config tab_cfg{};           // the configuration `tab` was built from; the tables are rebuilt when the geometry differs
  bool tab_valid = false;
};

enum TimerClass { T_ASSOC = 0, T_SOLVE, T_INDEX, T_EXTRACT, T_ODOM, T_FIT, T_ASSOC_SEEDED /* a subset of T_ASSOC */, T_COUNT };

struct TimedSpan { hipEvent_t a, b; int cls; };

// ---- What a registration call carries besides its clouds.  RegOptions: the value knobs of the optional features (the handle keeps one,
// the SLAM session one per matcher).  RecordSink: where the handle's caller wants one record per registration (or, for the prior, gives
// one).  RegSinks, below the handle: the options plus the device pointers one call's kernels use.  A new optional feature adds one member
// to RegOptions, one RecordSink to the handle and one SlotRecords to the SLAM session (msfl_api_slam.inc).
struct RejectOptions {               // msfl_set_outlier_rejection, normalised (reject_options): the inactive mode's parameter is zero
  int mode = MSFL_REJECT_OFF;        // MSFL_REJECT_OFF = feature off
  double thr2 = 0.0, fraction = 0.0; // threshold squared; fraction
  int which = MSFL_REJECT_LAST_OUTER;
};
struct RegOptions {
  double unc_min_eig = 0.0;
  int degen_on = 0;                  // msfl_set_degeneracy: 0 = feature off
  double degen_min_eig = 0.0;
  RejectOptions rej;
};
struct RecordSink {
  void* out = nullptr;               // the caller's array (the prior: its records, read only); null: none
  int capacity = 0;                  // records it holds
  msfl_mem mem = MSFL_MEM_HOST;
  DevBuf dev;                        // device staging of a host array
  void set(const void* p, int n, msfl_mem m) { out = const_cast<void*>(p); capacity = p ? n : 0; mem = m; }
  bool host() const { return out && mem == MSFL_MEM_HOST; }
};

}  // namespace

struct msfl_handle_s {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  msfl_params prm{};
  std::string last_error;

  bool have_map = false;
  MapIndex map_c, map_s;
  int grid_cap_cells = 64 * 1024 * 1024;  // hard limit of the dense cell table (MSFL_GRID_CAP_CELLS)
  int h2d_chunk_scans = 512;              // MSFL_H2D_CHUNK_SCANS: scans per PCIe chunk of a host-buffer batch (>= 2 chunks to pipeline)
  int h2d_sub_chunks = 2;                 // MSFL_H2D_SUB_CHUNKS: pieces a chunk arrives in (its first association pass follows them)
  int solve_records_block = 0;            // MSFL_SOLVE_RECORDS_BLOCK: kSlamLmBlock = msfl_solve_records runs the SLAM step's solve kernels; anything else: kLmBlock
  // set by msfl_voxel_downsample_batch when it refuses a cloud for a non-finite point: the cloud's number (-1: none) and where its
  // points are on the device (the staged copy of a host batch, or the caller's device array).  msfl_voxel_downsample reads these,
  // not the error text, to run PCL's drop-the-non-finite-points path.
  int vox_nonfinite_cloud = -1;
  const float4* vox_staged_pts = nullptr;
  bool voxel_no_big = false;              // MSFL_VOXEL_NO_BIG=1: lists beyond the LDS forms go straight to the device-wide form (A/B of the round-5 big form)
  int odom_bin_split = -1;         // the scan-to-scan index build: -1 = several workgroups per cloud when the call holds few pairs with long clouds, 0 / 1 = never / always (MSFL_ODOM_BIN_SPLIT)
  int prep_split = -1;             // workgroups per scan of the extraction's ring split: -1 = by batch size, 1 = the one-workgroup kernel (MSFL_PREP_SPLIT)
  bool voxel_force_global = false;        // MSFL_VOXEL_GLOBAL=1: the batched voxel filter keeps the device-wide radix-sort form (A/B testing)
  long long odom_wave_max_targets = -1;   // MSFL_ODOM_WAVE_MAX_TARGETS: previous-scan points up to which a small batch takes the one-wavefront-per-query kernel (default 4096 per pair)
  bool odom_force_brute = false;          // MSFL_ODOM_BRUTE=1: stage B plane queries stay on the brute-force kernel (A/B testing)
  int knn_form = 0;                       // MSFL_KNN_FORM: 0 auto (row-parallel latency form for launches of <= kKnnRowsMaxRecords queries),
                                          // 1 "lane" (one lane per query always), 2 "rows" (row-parallel always); results are identical
  bool knn_defer = true;                  // MSFL_KNN_DEFER=0|1: the whole-batch 5-NN kernel (and the candidate counter) caps every row visit and walks
                                          // the deferred tails after the ninth row (knn5_grid_k32<.., DEFER>); results are identical

  // scratch of the map matchers (scan-to-map, pairs, records): staged feature clouds, offset table, poses, per-registration status and
  // info, association records, deskewed points / host-format records, 5-NN lists.  `poses` also holds msfl_extract_features' extrinsic.
  DevBuf in_corner, in_surf, in_off, poses, status, info, records, pprime, nn;
  std::vector<int> in_off_host; const void* in_off_host_ptr = nullptr;   // what in_off holds on the device (upload_in_off)
  DevBuf idx_cell_of, idx_count, idx_scanned, idx_bbox, idx_cub, idx_stage;
  bool index_single = false;   // MSFL_INDEX_SINGLE=1: msfl_set_map builds its two indexes one after the other (the rounds 1-5 form; A/B and parity of the pair build)
  DevBuf knn_count;            // one u64: candidates evaluated by the counting 5-NN instantiation (timing mode 3)
  size_t idx_count_zero = 0;   // leading ints of idx_count known to be zero on the stream
  DeskewScratch dk;
  ExtractScratch ex;
  OdomScratch od;
  VoxelScratch vox;
  PointPassScratch pp;
  PairScratch pr;
  ScoreScratch sc;
  SearchScratch se;
  SegmentScratch sg;
  NoveltyScratch nv;
  int seg_chunk_scans = 0;                // MSFL_SEG_CHUNK_SCANS: scans per chunk of msfl_segment_scans (0 = what the scratch budget holds)
  int search_chunk_pairs = 0;             // MSFL_SEARCH_CHUNK_PAIRS: pairs per chunk of msfl_search_pairs (0 = what the scratch budget holds)

  // msfl_set_uncertainty / msfl_set_degeneracy / msfl_set_outlier_rejection: the knobs, and where every matcher call writes one
  // record per registration.  The uncertainty feature is on while its sink is set; a degeneracy or rejection sink is optional and
  // null while its feature is off.  msfl_set_pose_prior: prior.out[b] joins the problem of registration b (null: feature off).
  RegOptions opt;
  RecordSink unc, degen, rej, prior;
  DevBuf rej_keys;                        // fraction mode: one u64 per record of the call

  PinRing pin;
  PinBuf readback;
  hipStream_t copy_stream = nullptr;      // host-buffer batches: H2D of chunk k+1 under the compute of chunk k
  hipEvent_t copy_ev[9] = {};             // [8] = fork event

  // timing
  int timing = 0;            // 0 off, 1 every kernel class, 2 the association (5-NN) kernel only
  std::vector<TimedSpan> spans;
  std::vector<hipEvent_t> free_events;
  double t_ms[T_COUNT] = {0};
  int t_n[T_COUNT] = {0};
};

namespace {

msfl_status fail(msfl_handle* h, msfl_status s, const std::string& msg) {
  if (h) h->last_error = msg;
  return s;
}

#define HIPCHK(h, expr)                                                                            \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(h, MSFL_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(e__));          \
  } while (0)

msfl_status fail(msfl_places* p, msfl_status s, const std::string& msg);   // msfl_api_place.inc

// The two halves of a host-memory call's staging (`h`: the handle or the places object).  stage_in: where the kernels read the n
// elements of `src` -- a host array is copied into `buf` on `st` (which holds one element at least), a device array is read in place.
// The caller's array is typed by the pointer the kernels take (msfl_point arrives as float4).
template <class H, class T>
msfl_status stage_in(H* h, DevBuf& buf, const void* src, size_t n, msfl_mem mem, hipStream_t st, T** d) {
  if (mem != MSFL_MEM_HOST) { *d = static_cast<T*>(const_cast<void*>(src)); return MSFL_OK; }
  HIPCHK(h, buf.reserve(std::max<size_t>(1, n) * sizeof(T)));
  if (n > 0) HIPCHK(h, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
  *d = buf.as<T>();
  return MSFL_OK;
}
// stage_out: the n elements the kernels left at `d_src` go back to a host array on `st`; a device array was written in place.
template <class H, class T>
msfl_status stage_out(H* h, void* dst, const T* d_src, size_t n, msfl_mem mem, hipStream_t st) {
  if (mem == MSFL_MEM_HOST && n > 0) HIPCHK(h, hipMemcpyAsync(dst, d_src, n * sizeof(T), hipMemcpyDeviceToHost, st));
  return MSFL_OK;
}

hipEvent_t get_event(msfl_handle* h) {
  if (!h->free_events.empty()) { hipEvent_t e = h->free_events.back(); h->free_events.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

struct ScopedTimer {
  msfl_handle* h; TimedSpan s{}; bool on;
  ScopedTimer(msfl_handle* h_, int cls) : h(h_), on(h_->timing == 1 || h_->timing == 3 || (h_->timing == 2 && (cls == T_ASSOC || cls == T_ASSOC_SEEDED))) {
    if (on) { s.a = get_event(h); s.b = get_event(h); s.cls = cls; (void)hipEventRecord(s.a, h->stream); }
  }
  ~ScopedTimer() {
    if (on) { (void)hipEventRecord(s.b, h->stream); h->spans.push_back(s); }
  }
};

void collect_timing(msfl_handle* h) {
  for (auto& s : h->spans) {
    (void)hipEventSynchronize(s.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      h->t_ms[s.cls] += ms; h->t_n[s.cls]++;
      if (s.cls == T_ASSOC_SEEDED) { h->t_ms[T_ASSOC] += ms; h->t_n[T_ASSOC]++; }
    }
    h->free_events.push_back(s.a); h->free_events.push_back(s.b);
  }
  h->spans.clear();
}

// The offset table of a batch on the device (h->in_off).  Registering the same batch layout again (a replayed or re-registered batch: the
// bench step, a retry after msfl_set_map) skips the copy: it is one more dependent operation on the stream in front of the first kernel.
msfl_status upload_in_off(msfl_handle* h, const int* data, size_t count, hipStream_t st) {
  HIPCHK(h, h->in_off.reserve(count * sizeof(int)));
  if (h->in_off_host.size() == count && h->in_off_host_ptr == h->in_off.p && std::memcmp(h->in_off_host.data(), data, count * sizeof(int)) == 0)
    return MSFL_OK;
  h->in_off_host.clear();                       // (stays empty if the upload fails)
  HIPCHK(h, h->pin.upload(h->in_off.p, data, count * sizeof(int), st));
  h->in_off_host.assign(data, data + count); h->in_off_host_ptr = h->in_off.p;
  return MSFL_OK;
}

SolverParams solver_params(const msfl_params& p, int min_corr) {
  SolverParams s;
  s.max_iterations = p.max_lm_iterations;
  s.huber = p.huber_delta;
  s.radius0 = p.initial_trust_region_radius;
  s.radius_max = p.max_trust_region_radius;
  s.radius_min = p.min_trust_region_radius;
  s.min_relative_decrease = p.min_relative_decrease;
  s.min_diag = p.min_lm_diagonal;
  s.max_diag = p.max_lm_diagonal;
  s.ftol = p.function_tolerance;
  s.gtol = p.gradient_tolerance;
  s.ptol = p.parameter_tolerance;
  s.max_invalid = p.max_consecutive_invalid_steps;
  s.min_correspondences = min_corr;
  return s;
}

inline int div_up(int a, int b) { return (a + b - 1) / b; }

// ---- What a registration call carries besides its clouds: the info record, the msfl_set_uncertainty sink and the msfl_set_pose_prior
// records, all on the device.  Every solve site runs reg_check -> reg_open -> solve_outer -> reg_close (the SLAM step fills its
// RegSinks from the scan's slot instead of reg_open / reg_close).
static_assert(sizeof(UncRecord) == sizeof(msfl_match_uncertainty), "uncertainty record layout");
static_assert(sizeof(PosePrior) == sizeof(msfl_pose_prior), "pose prior record layout");
static_assert(sizeof(DevMatchInfo) == sizeof(msfl_match_info), "info layout");
static_assert(sizeof(DegenRecord) == sizeof(msfl_degeneracy_record), "degeneracy record layout");
static_assert(sizeof(RejectRecord) == sizeof(msfl_rejection_record) && sizeof(RejectRecord) == 56, "rejection record layout");
struct RegSinks {
  RegOptions opt;
  DevMatchInfo* info = nullptr;      // never null when `unc` is not: the uncertainty record takes sigma2 from the solve's own final cost
  UncRecord* unc = nullptr;          // null: feature off
  const PosePrior* prior = nullptr;  // null: feature off
  DegenRecord* degen = nullptr;      // optional record sink of the feature (zeroed before the first solve)
  RejectRecord* rej = nullptr;       // optional record sink of the feature (zeroed before the first solve)
  RegSinks at(int b) const {         // a part of a batch
    RegSinks k = *this;
    if (info) k.info += b;
    if (unc) k.unc += b;
    if (prior) k.prior += b;
    if (degen) k.degen += b;
    if (rej) k.rej += b;
    return k;
  }
};

// msfl_outlier_rejection as the solve takes it, for msfl_set_outlier_rejection and each matcher of msfl_slam_set_outlier_rejection
// (`who`: the caller's name).  Null or MSFL_REJECT_OFF gives the defaults; a bad field gives MSFL_BAD_ARG and *err says which.
msfl_status reject_options(const msfl_outlier_rejection* cfg, const char* who, RejectOptions* out, std::string* err) {
  *out = RejectOptions{};
  if (!cfg || cfg->mode == MSFL_REJECT_OFF) return MSFL_OK;
  const char* bad = nullptr;
  if (cfg->mode != MSFL_REJECT_THRESHOLD && cfg->mode != MSFL_REJECT_FRACTION) bad = "unknown mode";
  else if (cfg->which != MSFL_REJECT_LAST_OUTER && cfg->which != MSFL_REJECT_EVERY_OUTER)
    bad = "`which` is neither MSFL_REJECT_LAST_OUTER nor MSFL_REJECT_EVERY_OUTER";
  else if (cfg->mode == MSFL_REJECT_THRESHOLD && !(cfg->threshold >= 0.0 && std::isfinite(cfg->threshold))) bad = "threshold negative or not finite";
  else if (cfg->mode == MSFL_REJECT_FRACTION && !(cfg->fraction >= 0.0 && cfg->fraction <= 1.0)) bad = "fraction outside [0, 1]";
  if (bad) { *err = std::string(who) + ": " + bad; return MSFL_BAD_ARG; }
  out->mode = cfg->mode;
  out->which = cfg->which;
  if (cfg->mode == MSFL_REJECT_THRESHOLD) out->thr2 = cfg->threshold * cfg->threshold;
  else out->fraction = cfg->fraction;
  return MSFL_OK;
}

// The three RecordSink helpers of reg_check / reg_open / reg_close.  sink_fits: does the sink hold n records (`what`: how the error
// names it)?
msfl_status sink_fits(msfl_handle* h, const RecordSink& k, int n, const char* who, const char* what) {
  if (!k.out || n <= k.capacity) return MSFL_OK;
  return fail(h, MSFL_CAPACITY, std::string(who) + ": " + std::to_string(n) + " registrations, " + what + std::to_string(k.capacity));
}
// Where the kernels write the n records: the caller's device array, or device staging of its host one (null: no sink); zero = cleared on st.
template <class T>
msfl_status sink_open(msfl_handle* h, RecordSink& k, int n, hipStream_t st, bool zero, T** d) {
  *d = nullptr;
  if (!k.out) return MSFL_OK;
  if (k.mem == MSFL_MEM_DEVICE) *d = static_cast<T*>(k.out);
  else {
    HIPCHK(h, k.dev.reserve(std::max<size_t>(1, (size_t)n) * sizeof(T)));
    *d = k.dev.as<T>();
  }
  if (zero && n > 0) HIPCHK(h, hipMemsetAsync(*d, 0, (size_t)n * sizeof(T), st));
  return MSFL_OK;
}
// The n records go back to a host sink.
template <class T>
msfl_status sink_close(msfl_handle* h, const RecordSink& k, const T* d, int n, hipStream_t st) {
  if (k.host() && d && n > 0) HIPCHK(h, hipMemcpyAsync(k.out, d, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
  return MSFL_OK;
}

// First thing a matcher call does, before it stages or launches anything: refuse a call with more registrations than the sink holds or
// than there are prior records, and host prior records with a non-finite entry (device records are checked by the solve kernel:
// per-scan status MSFL_BAD_ARG).
msfl_status reg_check(msfl_handle* h, int n, const char* who) {
  msfl_status s = sink_fits(h, h->unc, n, who, "the msfl_set_uncertainty sink holds "); if (s) return s;
  s = sink_fits(h, h->degen, n, who, "the msfl_set_degeneracy sink holds "); if (s) return s;
  s = sink_fits(h, h->rej, n, who, "the msfl_set_outlier_rejection sink holds "); if (s) return s;
  if (!h->prior.out) return MSFL_OK;
  if (n > h->prior.capacity)
    return fail(h, MSFL_CAPACITY, std::string(who) + ": " + std::to_string(n) + " registrations, msfl_set_pose_prior gave " +
                                      std::to_string(h->prior.capacity) + " records");
  if (h->prior.mem == MSFL_MEM_HOST) {
    for (int b = 0; b < n; b++) {
      const double* w = reinterpret_cast<const double*>(static_cast<const msfl_pose_prior*>(h->prior.out) + b);
      for (int k = 0; k < kPriorWords; k++)
        if (!std::isfinite(w[k]))
          return fail(h, MSFL_BAD_ARG, std::string(who) + ": the pose prior of registration " + std::to_string(b) + " has a non-finite entry (" +
                                           (k < 7 ? "pose[" + std::to_string(k) : "sqrt_information[" + std::to_string(k - 7)) + "])");
    }
  }
  return MSFL_OK;
}

// Where the kernels of this call of n registrations find their sinks: the caller's device pointers, or device staging of its host ones
// (the prior records are copied on stream st, ahead of the clearing of the info records).  want_info: the caller asked for the info records.
msfl_status reg_open(msfl_handle* h, int n, hipStream_t st, bool want_info, RegSinks* k) {
  *k = RegSinks{};
  k->opt = h->opt;
  msfl_status s = sink_open(h, h->unc, n, st, false, &k->unc); if (s) return s;
  if (n > 0) {
    PosePrior* prior;
    s = sink_open(h, h->prior, n, st, false, &prior); if (s) return s;
    if (h->prior.host()) HIPCHK(h, h->pin.upload(prior, h->prior.out, (size_t)n * sizeof(PosePrior), st));
    k->prior = prior;
  }
  // the kernels write a degeneracy or rejection slice only where they solve: every other slice stays all zero (valid = 0)
  s = sink_open(h, h->degen, n, st, true, &k->degen); if (s) return s;
  s = sink_open(h, h->rej, n, st, true, &k->rej); if (s) return s;
  if (want_info || k->unc) {
    HIPCHK(h, h->info.reserve((size_t)n * sizeof(DevMatchInfo)));
    HIPCHK(h, hipMemsetAsync(h->info.p, 0, (size_t)n * sizeof(DevMatchInfo), st));
    k->info = h->info.as<DevMatchInfo>();
  }
  return MSFL_OK;
}

// What goes back to the caller: poses and status of a host-memory call, the info records, the host record sinks; then the stream is
// waited for if anything went to host memory.
msfl_status reg_close(msfl_handle* h, int n, msfl_mem mem, double* poses_io, const double* d_poses, int* status, const int* d_status,
                      msfl_match_info* info, const RegSinks& k) {
  hipStream_t st = h->stream;
  msfl_status s = stage_out(h, poses_io, d_poses, (size_t)n * 7, mem, st); if (s) return s;
  if (status) { s = stage_out(h, status, d_status, (size_t)n, mem, st); if (s) return s; }
  if (info) HIPCHK(h, hipMemcpyAsync(info, k.info, (size_t)n * sizeof(DevMatchInfo), hipMemcpyDeviceToHost, st));
  s = sink_close(h, h->unc, k.unc, n, st); if (s) return s;
  s = sink_close(h, h->degen, k.degen, n, st); if (s) return s;
  s = sink_close(h, h->rej, k.rej, n, st); if (s) return s;
  if (mem == MSFL_MEM_HOST || info || h->unc.host() || h->degen.host() || h->rej.host()) HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

// The outer loop of every registration: per outer iteration the site's own association launches (`assoc(it)`, which may fail), then the
// LM solve of all n problems; after the last one the uncertainty records, if asked for.  BLOCK: the site's solve workgroup.
// With msfl_set_outlier_rejection the selected solves are preceded by the rejection launch over the records association just wrote
// (msfl_reject.cuh); longest: records of the call's longest scan, for that launch's grid (< 0: bv.n_records, a bound).
template <int BLOCK, class Assoc>
msfl_status solve_outer(msfl_handle* h, int n, const BatchView& bv, const double* pprime, double* d_poses, int* d_status, const RegSinks& k,
                        const SolverParams& sp, int n_outer, Assoc&& assoc, int longest = -1) {
  hipStream_t st = h->stream;
  const double* records = h->records.as<double>();
  if (k.opt.rej.mode == MSFL_REJECT_FRACTION) HIPCHK(h, h->rej_keys.reserve(std::max<size_t>(1, (size_t)bv.n_records) * sizeof(unsigned long long)));
  for (int it = 0; it < n_outer; it++) {
    { const msfl_status as = assoc(it); if (as) return as; }
    if (k.opt.rej.mode != MSFL_REJECT_OFF && (k.opt.rej.which == MSFL_REJECT_EVERY_OUTER || it == n_outer - 1))
      launch_reject(st, k.opt.rej.mode, n, longest < 0 ? bv.n_records : longest, bv, pprime, h->records.as<double>(), d_poses, d_status, k.rej, it,
                    k.opt.rej.thr2, k.opt.rej.fraction, h->rej_keys.as<unsigned long long>());
    ScopedTimer timer(h, T_SOLVE);
    launch_lm_solve<BLOCK>(st, n, bv, pprime, records, d_poses, d_status, k.info, it, sp, k.prior, k.opt.degen_on, k.opt.degen_min_eig, k.degen);
  }
  launch_uncertainty<BLOCK>(st, n, bv, pprime, records, d_poses, d_status, k.info, n_outer - 1, sp, k.opt.unc_min_eig, k.unc, k.prior);
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// [corner_off | surf_off | rec_off] (n + 1 ints each) of a batch of n scans from its host offsets, into h->in_off; *n_rec: its records.
msfl_status upload_batch_offsets(msfl_handle* h, int n, const int* corner_off, const int* surf_off, int* n_rec) {
  std::vector<int> offs(3 * (size_t)(n + 1));
  for (int b = 0; b <= n; b++) {
    offs[b] = corner_off[b];
    offs[(n + 1) + b] = surf_off[b];
    offs[2 * (n + 1) + b] = corner_off[b] - corner_off[0] + surf_off[b] - surf_off[0];
    if (b > 0 && (corner_off[b] < corner_off[b - 1] || surf_off[b] < surf_off[b - 1]))
      return fail(h, MSFL_BAD_ARG, "offset arrays must be non-decreasing");
  }
  *n_rec = offs[2 * (n + 1) + n];
  return upload_in_off(h, offs.data(), offs.size(), h->stream);
}

// Bytes of the record buffer of a batch of n_rec records, n_surf of them planes (msfl_record_tiles.h: the plane tiles, padded to whole
// tiles, then the edge records).
size_t record_bytes(size_t n_rec, size_t n_surf) { return rec_reserve_doubles(n_rec, n_surf) * sizeof(double); }

// The view over a device offset table whose rows corner_off, surf_off and rec_off lie `stride` ints apart.  dyn = 1: the SLAM step's
// device-written table (BatchView::dyn: n_records and n_surf_total are then capacities, c0 = s0 = 0).
BatchView batch_view(const float4* d_corner, const float4* d_surf, const int* d_table, int stride, int n_scans, int n_records, int c0, int s0,
                     int n_surf_total, int dyn = 0) {
  BatchView bv;
  bv.corner = d_corner; bv.corner_off = d_table;
  bv.surf = d_surf; bv.surf_off = d_table + stride;
  bv.rec_off = d_table + 2 * stride;
  bv.n_scans = n_scans; bv.n_records = n_records;
  bv.c0 = c0; bv.s0 = s0; bv.n_surf_total = n_surf_total; bv.dyn = dyn;
  return bv;
}

__global__ void __launch_bounds__(256) zero_ints_kernel(int* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}

// What every index build does on the host before its launches: the size check, the span of the dense cell table, the buffers
// that belong to the map, the bbox armed.  The span is what the previous build of this map said it needs (+25 %), else 1 M
// cells (MSFL_GRID_CAP_CELLS bounds it).  The device grows the cell edge when the bounding box needs more than the span, or
// more than kGridMaxDim cells along one axis (larger cells stay exact, just more candidates per cell: tested to 12 km extents,
// docs/kernels/scan2map.md "Index geometry"), and reports the wanted size for the next build.
msfl_status index_prepare(msfl_handle* h, MapIndex& mi, int n) {
  // the 5-NN walk addresses candidates by 32-bit byte offsets into the sorted copy (knn5_grid_k32)
  if (n >= (1 << 28)) return fail(h, MSFL_BAD_ARG, "map cloud of 2^28 points or more (the index addresses 16-byte points by 32-bit byte offsets)");
  mi.n_input = n;
  if (!mi.want.p) { HIPCHK(h, mi.want.reserve(sizeof(int))); *mi.want.as<int>() = 0; }
  const int seen = *(volatile int*)mi.want.as<int>();
  if (seen > 0) mi.span = (int)std::min<long long>(std::max<long long>((long long)seen + seen / 4 + 1024, 65536), h->grid_cap_cells);
  if (mi.span <= 0) mi.span = std::min(1 << 20, h->grid_cap_cells);
  mi.cap_cells = mi.span;
  HIPCHK(h, mi.gdesc.reserve(sizeof(GridDesc)));
  HIPCHK(h, mi.cell_start.reserve(((size_t)mi.span + 1) * sizeof(int)));
  HIPCHK(h, mi.sorted.reserve(std::max<size_t>(1, (size_t)n) * sizeof(float4)));
  HIPCHK(h, mi.pos_of.reserve(std::max<size_t>(1, (size_t)n) * sizeof(int)));
  if (!mi.bbox.p) {                       // armed once; every build re-arms it after the last read
    HIPCHK(h, mi.bbox.reserve(6 * sizeof(int)));
    const int init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
    HIPCHK(h, h->pin.upload(mi.bbox.p, init, sizeof(init), h->stream));
  }
  return MSFL_OK;
}

// Build the exact-kNN grid over `pts` (device pointer, n points; n_dev: the SLAM step's device-side count, n is then its bound).
// Fully asynchronous: the grid descriptor is computed and kept on the device.
msfl_status build_index(msfl_handle* h, const float4* pts, int n, MapIndex& mi, const int* n_dev = nullptr) {
  ScopedTimer timer(h, T_INDEX);
  msfl_status ps = index_prepare(h, mi, n); if (ps) return ps;
  hipStream_t st = h->stream;
  const int cap = mi.span;
  HIPCHK(h, h->idx_cell_of.reserve(std::max<size_t>(1, (size_t)n) * sizeof(int)));
  const void* count_before = h->idx_count.p;
  HIPCHK(h, h->idx_count.reserve(((size_t)cap + 1) * sizeof(int)));
  if (h->idx_count.p != count_before) h->idx_count_zero = 0;
  if (n > 0) {
    const int blocks = std::min(div_up(n, 1024), 256);   // 6 atomics per workgroup, all on one line: four points per lane and pass
    hipLaunchKernelGGL(grid_bbox_kernel, dim3(blocks), dim3(256), 0, st, pts, n, mi.bbox.as<int>(), n_dev);
  }
  const double radius = std::sqrt((double)h->prm.map_knn_max_sq_dist);
  if (n == 0)
    hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(1), 0, st, mi.bbox.as<int>(), radius, cap, mi.gdesc.as<GridDesc>(), mi.want.as<int>());
  // the table is cleared / scanned over the cells actually used last time (+ margin) when known,
  // else over the full capacity; the device never indexes beyond n_cells <= cap.
  const size_t span = (size_t)cap + 1;
  // the scatter kernel counts every cell back down to zero, so the table only needs clearing when it
  // is new or larger than what has been cleared before
  const size_t zeroed = h->idx_count_zero;
  h->idx_count_zero = 0;                  // unknown until this build has been enqueued completely
  if (span > zeroed) HIPCHK(h, hipMemsetAsync(h->idx_count.p, 0, span * sizeof(int), st));
  if (n > 0)
    hipLaunchKernelGGL(grid_count_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, pts, n, (const int*)mi.bbox.as<int>(), radius, cap,
                       mi.gdesc.as<GridDesc>(), h->idx_cell_of.as<int>(), h->idx_count.as<int>(), n_dev);
  size_t tmp_bytes = 0;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tmp_bytes, h->idx_count.as<int>(), mi.cell_start.as<int>(), 0, (size_t)((int)span), rocprim::plus<int>(), st));
  HIPCHK(h, h->idx_cub.reserve(tmp_bytes));
  HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tmp_bytes, h->idx_count.as<int>(), mi.cell_start.as<int>(), 0, (size_t)((int)span), rocprim::plus<int>(), st));
  if (n > 0)
    hipLaunchKernelGGL(grid_scatter_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, pts, n, h->idx_cell_of.as<int>(),
                       mi.cell_start.as<int>(), h->idx_count.as<int>(), mi.sorted.as<float4>(), mi.pos_of.as<int>(),
                       mi.gdesc.as<GridDesc>(), mi.bbox.as<int>(), mi.want.as<int>(), n_dev);
  HIPCHK(h, hipGetLastError());
  h->idx_count_zero = std::max(zeroed, span);
  return MSFL_OK;
}

// Both maps of msfl_set_map through one chain of five launches (msfl_knn_index.cuh: GridPairJob).  Same results as two build_index calls;
// used when both clouds are non-empty and their sizes are host-side numbers (the per-scan SLAM step builds its maps on streams of their own).
msfl_status build_index_pair(msfl_handle* h, const float4* pts_c, int n_c, const float4* pts_s, int n_s) {
  ScopedTimer timer(h, T_INDEX);
  hipStream_t st = h->stream;
  MapIndex* mi[2] = {&h->map_c, &h->map_s};
  const float4* pts[2] = {pts_c, pts_s};
  const int n[2] = {n_c, n_s};
  GridPairJob j;
  for (int m = 0; m < 2; m++) {
    MapIndex& x = *mi[m];
    msfl_status ps = index_prepare(h, x, n[m]); if (ps) return ps;
    j.pts[m] = pts[m]; j.n[m] = n[m]; j.bbox[m] = x.bbox.as<int>(); j.gdesc[m] = x.gdesc.as<GridDesc>(); j.cap[m] = x.span;
    j.cell_start[m] = x.cell_start.as<int>(); j.sorted[m] = x.sorted.as<float4>(); j.pos_of[m] = x.pos_of.as<int>();
    j.want_host[m] = x.want.as<int>();
  }
  const size_t span = (size_t)j.cap[0] + 1 + (size_t)j.cap[1] + 1;
  HIPCHK(h, h->idx_cell_of.reserve(((size_t)n_c + (size_t)n_s) * sizeof(int)));
  const void* count_before = h->idx_count.p;
  HIPCHK(h, h->idx_count.reserve(span * sizeof(int)));
  if (h->idx_count.p != count_before) h->idx_count_zero = 0;
  HIPCHK(h, h->idx_scanned.reserve(span * sizeof(int)));
  j.cell_of = h->idx_cell_of.as<int>(); j.count = h->idx_count.as<int>(); j.scanned = h->idx_scanned.as<int>();
  j.blocks0 = div_up(n_c, 256); j.bbox_blocks0 = std::min(div_up(n_c, 1024), 256);
  j.radius = std::sqrt((double)h->prm.map_knn_max_sq_dist);
  const int bbox_blocks1 = std::min(div_up(n_s, 1024), 256), blocks1 = div_up(n_s, 256);
  hipLaunchKernelGGL(grid_bbox_pair_kernel, dim3(j.bbox_blocks0 + bbox_blocks1), dim3(256), 0, st, j);
  // the scatter launch counts every cell back down to zero: the table only needs clearing when it is new or larger than what has been cleared
  const size_t zeroed = h->idx_count_zero;
  h->idx_count_zero = 0;
  if (span > zeroed) HIPCHK(h, hipMemsetAsync(h->idx_count.p, 0, span * sizeof(int), st));
  hipLaunchKernelGGL(grid_count_pair_kernel, dim3(j.blocks0 + blocks1), dim3(256), 0, st, j);
  size_t tmp_bytes = 0;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tmp_bytes, j.count, j.scanned, 0, span, rocprim::plus<int>(), st));
  HIPCHK(h, h->idx_cub.reserve(tmp_bytes));
  HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tmp_bytes, j.count, j.scanned, 0, span, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(grid_scatter_pair_kernel, dim3(j.blocks0 + blocks1), dim3(256), 0, st, j);
  HIPCHK(h, hipGetLastError());
  h->idx_count_zero = std::max(zeroed, span);
  return MSFL_OK;
}

// A 5-NN launch: batch, poses and status, then the eight map arguments (descriptor, sorted points and cell table of the corner
// map, the same of the surf map, the two position tables) and the acceptance gate that every form takes, then the form's own.
template <class Kernel, class... Tail>
void launch_knn5(msfl_handle* h, Kernel kernel, dim3 grid, dim3 block, const BatchView& bv, const double* d_poses, const int* d_status,
                 Tail... tail) {
  hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, bv, d_poses, d_status,
                     (const GridDesc*)h->map_c.gdesc.as<GridDesc>(), h->map_c.sorted.as<float4>(), h->map_c.cell_start.as<int>(),
                     (const GridDesc*)h->map_s.gdesc.as<GridDesc>(), h->map_s.sorted.as<float4>(), h->map_s.cell_start.as<int>(),
                     (const int*)h->map_c.pos_of.as<int>(), (const int*)h->map_s.pos_of.as<int>(), h->prm.map_knn_max_sq_dist, tail...);
}

// Does an association pass over ALL n_rec records of this batch take the whole-batch kernels?  They number `nn` by corner feature and
// keep a surf feature's list in its record tile; the per-record kernels number `nn` by record (msfl_kernels.cuh: corner_slot, plane_nn_store).
bool assoc_whole_batch(const msfl_handle* h, const BatchView& bv, bool deskew, int n_rec, const double* full) {
  return !deskew && !bv.dyn && n_rec >= 65536 && !full && h->timing != 3;
}

// one data-association pass = kNN kernel + fit kernel
// (records [rec_begin, rec_end) of the batch; rec_end < 0: all of them)
void s_launch_assoc(msfl_handle* h, const BatchView& bv_all, const double* d_poses, const int* d_status, bool deskew,
                    const DeskewView& dv, int n_rec, double* full = nullptr, int rec_begin = 0, int rec_end = -1, bool second_pass = false) {
  const bool whole_batch = rec_end < 0 && assoc_whole_batch(h, bv_all, deskew, n_rec, full);
  hipStream_t st = h->stream;
  int* nn = h->nn.as<int>();
  BatchView bv = bv_all;
  if (rec_end >= 0) { bv.rec_begin = rec_begin; bv.n_records = rec_end; n_rec = rec_end - rec_begin; }
  if (n_rec <= 0) return;
  const dim3 grid(div_up(n_rec, kAssocBlock)), block(kAssocBlock);
  {
    ScopedTimer timer(h, second_pass ? T_ASSOC_SEEDED : T_ASSOC);      // second-pass launches are timed (and counted) on their own
    if (h->timing == 3) {
      unsigned long long* cnt = h->knn_count.as<unsigned long long>();
      if (deskew) launch_knn5(h, knn5_scan2map_kernel<true, true>, grid, block, bv, d_poses, d_status, dv, nn, cnt, nullptr, nullptr);
      else if (h->knn_defer) launch_knn5(h, knn5_scan2map_kernel<false, true, false, true>, grid, block, bv, d_poses, d_status, dv, nn, cnt + (second_pass ? 1 : 0), nullptr, nullptr);
      else launch_knn5(h, knn5_scan2map_kernel<false, true>, grid, block, bv, d_poses, d_status, dv, nn, cnt + (second_pass ? 1 : 0), nullptr, nullptr);
    } else if (whole_batch) {       // a whole large batch: one body per feature kind (-2 %)
      const int n_s = bv.n_surf_total, n_c = n_rec - n_s;
      const int edge_blocks = div_up(n_c, kAssocBlock), plane_blocks = div_up(n_s, kAssocBlock);
      const dim3 blocks(edge_blocks + plane_blocks);
      if (h->knn_defer) launch_knn5(h, knn5_scan2map_split_kernel<true>, blocks, block, bv, d_poses, d_status, nn, h->records.as<double>(), edge_blocks);
      else launch_knn5(h, knn5_scan2map_split_kernel<false>, blocks, block, bv, d_poses, d_status, nn, h->records.as<double>(), edge_blocks);
    } else if (!deskew && (h->knn_form == 2 || (h->knn_form == 0 && (n_rec <= kKnnRowsMaxRecords ||
                                                                       // the SLAM step launches over the list CAPACITIES (device-side counts): a 64-beam scan's ~11-17 k
                                                                       // queries sit in a ~150 k-slot launch whose surplus workgroups leave at once
                                                                       (bv.dyn && n_rec <= 8 * kKnnRowsMaxRecords)))))
      launch_knn5(h, knn5_scan2map_rows_kernel, dim3(div_up(n_rec, kKnnRowsBlock / kKnnRowLanes)), dim3(kKnnRowsBlock), bv, d_poses, d_status, nn);
    else if (deskew)
      launch_knn5(h, knn5_scan2map_kernel<true>, grid, block, bv, d_poses, d_status, dv, nn, nullptr, nullptr, nullptr);
    else
      launch_knn5(h, knn5_scan2map_kernel<false>, grid, block, bv, d_poses, d_status, dv, nn, nullptr, nullptr, nullptr);
  }
  {
    ScopedTimer timer(h, T_FIT);
    if (deskew)
      hipLaunchKernelGGL(fit_scan2map_kernel<true>, grid, block, 0, st, bv, h->map_c.sorted.as<float4>(),
                         h->map_s.sorted.as<float4>(), (const int*)nn, h->prm.line_eigen_ratio, h->prm.plane_tolerance, dv,
                         h->records.as<double>(), full);
    else
      if (whole_batch) {    // (the same condition as the 5-NN launch above: the two share a numbering of `nn`)
        // a whole large batch: corner and surf features through their own specialisations of the fit (msfl_kernels.cuh)
        const int n_c = n_rec - bv.n_surf_total, n_s = bv.n_surf_total;
        const int edge_blocks = div_up(n_c, kAssocBlock), plane_blocks = div_up(n_s, kAssocBlock);
        hipLaunchKernelGGL(fit_scan2map_split_kernel, dim3(edge_blocks + plane_blocks), block, 0, st, bv, h->map_c.sorted.as<float4>(),
                           h->map_s.sorted.as<float4>(), (const int*)nn, h->prm.line_eigen_ratio, h->prm.plane_tolerance, dv,
                           h->records.as<double>(), full, edge_blocks);
      } else
      hipLaunchKernelGGL(fit_scan2map_kernel<false>, grid, block, 0, st, bv, h->map_c.sorted.as<float4>(),
                         h->map_s.sorted.as<float4>(), (const int*)nn, h->prm.line_eigen_ratio, h->prm.plane_tolerance, dv,
                         h->records.as<double>(), full);
  }
}

// Core of stage C.  All pointers are device pointers except the offsets (host).
// `n_chunks` > 1: the features of scans [chunk_b[c], chunk_b[c + 1]) are valid on the device once `chunk_ev[c]` has
// fired (host-buffer batches: they arrive over PCIe on another stream).  The first association pass then runs chunk by
// chunk behind the copies; everything after it sees the whole batch.
msfl_status match_scan2map_device(msfl_handle* h, int B, const float4* d_corner, const int* h_corner_off, const float4* d_surf,
                                  const int* h_surf_off, double* d_poses, int* d_status, const RegSinks& sinks, const DeskewView* deskew,
                                  int n_chunks = 1, const int* chunk_b = nullptr, hipEvent_t* chunk_ev = nullptr,
                                  const std::function<hipError_t(int)>* enqueue_chunk = nullptr) {
  int n_rec = 0;
  { const msfl_status us = upload_batch_offsets(h, B, h_corner_off, h_surf_off, &n_rec); if (us) return us; }
  HIPCHK(h, h->records.reserve(record_bytes((size_t)n_rec, (size_t)(h_surf_off[B] - h_surf_off[0]))));
  const BatchView bv = batch_view(d_corner, d_surf, h->in_off.as<int>(), B + 1, B, n_rec, h_corner_off[0], h_surf_off[0], h_surf_off[B] - h_surf_off[0]);
  // every pass through the whole-batch kernels: `nn` holds the corner features' lists only (the surf lists live in the record tiles)
  const bool nn_corner_only = n_chunks == 1 && !enqueue_chunk && assoc_whole_batch(h, bv, deskew != nullptr, n_rec, nullptr);
  HIPCHK(h, h->nn.reserve(std::max<size_t>(1, (size_t)(nn_corner_only ? n_rec - bv.n_surf_total : n_rec)) * 5 * sizeof(int)));
  DeskewView dv{};
  if (deskew) {
    dv = *deskew;
    HIPCHK(h, h->pprime.reserve(std::max<size_t>(1, (size_t)n_rec) * 3 * sizeof(double)));
    dv.pprime = h->pprime.as<double>();
  }
  const auto rec_at = [&](int b) { return h_corner_off[b] - h_corner_off[0] + h_surf_off[b] - h_surf_off[0]; };   // rec_off[b]
  int longest = 0;
  for (int b = 0; b < B; b++) longest = std::max(longest, rec_at(b + 1) - rec_at(b));
  return solve_outer<kLmBlock>(h, B, bv, dv.pprime, d_poses, d_status, sinks, solver_params(h->prm, 0), h->prm.outer_iterations, [&](int it) -> msfl_status {
    if (it == 0 && (n_chunks > 1 || enqueue_chunk)) {
      for (int c = 0; c < n_chunks; c++) {
        // the copy of chunk c is ENQUEUED here, right before the kernels that wait for it: a copy from pageable memory
        // holds the calling thread until it is staged, and the kernels of chunk c - 1 must be in the queue by then
        if (enqueue_chunk) HIPCHK(h, (*enqueue_chunk)(c));
        HIPCHK(h, hipStreamWaitEvent(h->stream, chunk_ev[c], 0));
        s_launch_assoc(h, bv, d_poses, d_status, deskew != nullptr, dv, n_rec, nullptr, rec_at(chunk_b[c]), rec_at(chunk_b[c + 1]));
      }
    } else if (n_rec > 0) {
      s_launch_assoc(h, bv, d_poses, d_status, deskew != nullptr, dv, n_rec, nullptr, 0, -1, it > 0);
    }
    return MSFL_OK;
  }, longest);
}

msfl_status check_map(msfl_handle* h) {
  if (!h->have_map) return fail(h, MSFL_NO_MAP, "msfl_set_map has not been called on this handle");
  // host-known input sizes; non-finite map points only ever reduce the candidate set (a query
  // with fewer than 5 finite neighbours is rejected on the device like any other)
  if (h->map_c.n_input < 5 || h->map_s.n_input < 5)
    return fail(h, MSFL_MAP_TOO_SMALL, "map corner/surf cloud has fewer than 5 points (mapping_scan_matcher.cc:128,198 would read out of bounds)");
  return MSFL_OK;
}

msfl_status enter(msfl_handle* h) {
  if (!h) return MSFL_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  return MSFL_OK;
}

}  // namespace

// =============================================================================================
// lifecycle
// =============================================================================================

extern "C" {

void msfl_default_params(msfl_params* p) {
  if (!p) return;
  p->scan_period = 0.1;
  p->min_range = 0.3;
  p->curvature_threshold = 0.1f;
  p->neighbor_gap_sq = 0.05f;
  p->sectors_per_ring = 6;
  p->max_sharp_per_sector = 2;
  p->max_less_sharp_per_sector = 20;
  p->max_flat_per_sector = 4;
  p->odom_distance_sq_threshold = 25.0;
  p->odom_nearby_scan = 2.5;
  p->odom_min_correspondences = 10;
  p->map_knn = 5;
  p->map_knn_max_sq_dist = 1.0f;
  p->line_eigen_ratio = 3.0;
  p->plane_tolerance = 0.2;
  p->outer_iterations = 2;
  p->max_lm_iterations = 6;
  p->huber_delta = 0.1;
  p->initial_trust_region_radius = 1e4;
  p->max_trust_region_radius = 1e16;
  p->min_trust_region_radius = 1e-32;
  p->min_relative_decrease = 1e-3;
  p->min_lm_diagonal = 1e-6;
  p->max_lm_diagonal = 1e32;
  p->function_tolerance = 1e-6;
  p->gradient_tolerance = 1e-10;
  p->parameter_tolerance = 1e-8;
  p->max_consecutive_invalid_steps = 5;
}

int msfl_api_version(void) { return MSFL_API_VERSION; }

msfl_status msfl_create(const msfl_params* params, int device, msfl_handle** out) {
  if (!out) return MSFL_BAD_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSFL_HIP_ERROR;   // no GPU: fail loudly, no fallback
  if (device < 0 || device >= ndev) return MSFL_BAD_ARG;
  msfl_handle* h = new msfl_handle_s();
  h->device = device;
  if (params) h->prm = *params; else msfl_default_params(&h->prm);
  if (h->prm.map_knn != 5 || h->prm.outer_iterations < 1 || h->prm.outer_iterations > 2 ||
      h->prm.max_lm_iterations < 0 || !(h->prm.map_knn_max_sq_dist > 0.f) ||
      h->prm.sectors_per_ring < 1 || h->prm.sectors_per_ring > 16) {
    delete h;
    return MSFL_BAD_ARG;
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return MSFL_HIP_ERROR;
  }
  h->stream = h->own_stream;
  if (const char* e = std::getenv("MSFL_GRID_CAP_CELLS")) { const int c = std::atoi(e); if (c >= 8 && c <= (1 << 28)) h->grid_cap_cells = c; }
  if (const char* e = std::getenv("MSFL_H2D_CHUNK_SCANS")) { const int c = std::atoi(e); if (c >= 1) h->h2d_chunk_scans = c; }
  if (const char* e = std::getenv("MSFL_H2D_SUB_CHUNKS")) { const int c = std::atoi(e); if (c >= 1) h->h2d_sub_chunks = c; }
  if (const char* e = std::getenv("MSFL_SOLVE_RECORDS_BLOCK")) h->solve_records_block = std::atoi(e);
  if (const char* e = std::getenv("MSFL_ODOM_BRUTE")) h->odom_force_brute = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_INDEX_SINGLE")) h->index_single = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_KNN_DEFER")) h->knn_defer = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_KNN_FORM")) h->knn_form = !std::strcmp(e, "lane") ? 1 : !std::strcmp(e, "rows") ? 2 : 0;
  if (const char* e = std::getenv("MSFL_ODOM_WAVE_MAX_TARGETS")) h->odom_wave_max_targets = std::atoll(e);
  if (const char* e = std::getenv("MSFL_VOXEL_GLOBAL")) h->voxel_force_global = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_VOXEL_NO_BIG")) h->voxel_no_big = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSFL_ODOM_BIN_SPLIT")) h->odom_bin_split = std::atoi(e) != 0 ? 1 : 0;
  if (const char* e = std::getenv("MSFL_SEG_CHUNK_SCANS")) { const int c = std::atoi(e); if (c >= 1) h->seg_chunk_scans = c; }
  if (const char* e = std::getenv("MSFL_SEARCH_CHUNK_PAIRS")) { const int c = std::atoi(e); if (c >= 1) h->search_chunk_pairs = c; }
  if (const char* e = std::getenv("MSFL_PREP_SPLIT")) { const int g = std::atoi(e); if (g == 1 || g == 2 || g == 4 || g == 8 || g == 16) h->prep_split = g; }
  *out = h;
  return MSFL_OK;
}

void msfl_destroy(msfl_handle* h) {
  if (!h) return;
#ifdef MSFL_LM_PROFILE
  {
    unsigned long long v[8] = {0};
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(v, HIP_SYMBOL(msfl::g_lm_prof), sizeof(v));
    if (v[5]) fprintf(stderr, "[lm profile] per solve (100 MHz ticks): eval %.0f reduce %.0f serial %.0f total %.0f passes %.2f solves %llu\n",
                      (double)v[0] / v[5], (double)v[1] / v[5], (double)v[2] / v[5], (double)v[3] / v[5], (double)v[4] / v[5], v[5]);
    if (v[5]) fprintf(stderr, "[lm profile] lane-0 logic: tr_decide %.0f tr_propose %.0f ticks per solve\n", (double)v[6] / v[5], (double)v[7] / v[5]);
  }
#endif
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  collect_timing(h);
  for (auto e : h->free_events) (void)hipEventDestroy(e);
  if (h->copy_stream) { (void)hipStreamDestroy(h->copy_stream); for (auto e : h->copy_ev) if (e) (void)hipEventDestroy(e); }
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;                               // every DevBuf / PinBuf member and the pinned ring free themselves
}

msfl_status msfl_set_stream(msfl_handle* h, void* hip_stream) {
  msfl_status s = enter(h); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = HIP null stream
  return MSFL_OK;
}

msfl_status msfl_reset_stream(msfl_handle* h) {
  msfl_status s = enter(h); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = h->own_stream;
  return MSFL_OK;
}

msfl_status msfl_synchronize(msfl_handle* h) {
  msfl_status s = enter(h); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MSFL_OK;
}

msfl_status msfl_set_uncertainty(msfl_handle* h, msfl_match_uncertainty* out, int capacity, msfl_mem mem, double min_eigenvalue) {
  msfl_status s = enter(h); if (s) return s;
  if (out && (capacity < 1 || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE) || !(min_eigenvalue >= 0.0)))
    return fail(h, MSFL_BAD_ARG, "msfl_set_uncertainty: capacity < 1, unknown memory kind or a negative / NaN min_eigenvalue");
  h->unc.set(out, capacity, mem);
  h->opt.unc_min_eig = out ? min_eigenvalue : 0.0;
  return MSFL_OK;
}

msfl_status msfl_set_degeneracy(msfl_handle* h, int enabled, double min_eigenvalue, msfl_degeneracy_record* out, int capacity, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (enabled && (!(min_eigenvalue >= 0.0) || !std::isfinite(min_eigenvalue)))
    return fail(h, MSFL_BAD_ARG, "msfl_set_degeneracy: min_eigenvalue negative or not finite");
  if (enabled && out && (capacity < 1 || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE)))
    return fail(h, MSFL_BAD_ARG, "msfl_set_degeneracy: capacity < 1 or unknown memory kind");
  h->opt.degen_on = enabled != 0;
  h->opt.degen_min_eig = enabled ? min_eigenvalue : 0.0;
  h->degen.set(enabled ? out : nullptr, capacity, mem);
  return MSFL_OK;
}

msfl_status msfl_set_outlier_rejection(msfl_handle* h, const msfl_outlier_rejection* cfg, msfl_rejection_record* out, int capacity, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  RejectOptions rej;
  std::string err;
  s = reject_options(cfg, "msfl_set_outlier_rejection", &rej, &err); if (s) return fail(h, s, err);
  const bool on = rej.mode != MSFL_REJECT_OFF;
  if (on && out && (capacity < 1 || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE)))
    return fail(h, MSFL_BAD_ARG, "msfl_set_outlier_rejection: capacity < 1 or unknown memory kind");
  h->opt.rej = rej;
  h->rej.set(on ? out : nullptr, capacity, mem);
  return MSFL_OK;
}

msfl_status msfl_set_pose_prior(msfl_handle* h, const msfl_pose_prior* priors, int count, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (priors && (count < 1 || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE)))
    return fail(h, MSFL_BAD_ARG, "msfl_set_pose_prior: count < 1 or unknown memory kind");
  h->prior.set(priors, count, mem);
  return MSFL_OK;
}

const char* msfl_status_string(int status) {
  switch (status) {
    case MSFL_OK: return "OK";
    case MSFL_TOO_FEW_CORRESPONDENCES: return "TOO_FEW_CORRESPONDENCES";
    case MSFL_MAP_TOO_SMALL: return "MAP_TOO_SMALL";
    case MSFL_BAD_ARG: return "BAD_ARG";
    case MSFL_HIP_ERROR: return "HIP_ERROR";
    case MSFL_BAD_RING: return "BAD_RING";
    case MSFL_NO_MAP: return "NO_MAP";
    case MSFL_CAPACITY: return "CAPACITY";
    default: return "UNKNOWN";
  }
}

const char* msfl_last_error(const msfl_handle* h) { return h ? h->last_error.c_str() : ""; }

msfl_status msfl_set_timing(msfl_handle* h, int enabled) {
  msfl_status s = enter(h); if (s) return s;
  h->timing = enabled < 0 ? 0 : (enabled > 3 ? 1 : enabled);
  if (h->timing == 3 && !h->knn_count.p) {
    HIPCHK(h, h->knn_count.reserve(2 * sizeof(unsigned long long)));     // [first-pass launches, second-pass launches]
    HIPCHK(h, hipMemsetAsync(h->knn_count.p, 0, 2 * sizeof(unsigned long long), h->stream));
  }
  return MSFL_OK;
}

msfl_status msfl_get_timing(msfl_handle* h, msfl_timing* out, int reset) {
  msfl_status s = enter(h); if (s) return s;
  if (!out) return MSFL_BAD_ARG;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  collect_timing(h);
  out->launches_assoc = h->t_n[T_ASSOC];     out->ms_assoc = h->t_ms[T_ASSOC];
  out->launches_solve = h->t_n[T_SOLVE];     out->ms_solve = h->t_ms[T_SOLVE];
  out->launches_index = h->t_n[T_INDEX];     out->ms_index = h->t_ms[T_INDEX];
  out->launches_extract = h->t_n[T_EXTRACT]; out->ms_extract = h->t_ms[T_EXTRACT];
  out->launches_odom = h->t_n[T_ODOM];       out->ms_odom = h->t_ms[T_ODOM];
  out->launches_fit = h->t_n[T_FIT];         out->ms_fit = h->t_ms[T_FIT];
  out->launches_assoc_seeded = h->t_n[T_ASSOC_SEEDED]; out->ms_assoc_seeded = h->t_ms[T_ASSOC_SEEDED];
  out->knn_candidates = 0; out->knn_candidates_seeded = 0;
  if (h->knn_count.p) {
    unsigned long long c2[2] = {0, 0};
    HIPCHK(h, hipMemcpy(c2, h->knn_count.p, sizeof(c2), hipMemcpyDeviceToHost));
    out->knn_candidates = c2[0]; out->knn_candidates_seeded = c2[1];
    if (reset) HIPCHK(h, hipMemset(h->knn_count.p, 0, sizeof(c2)));
  }
  if (reset) for (int i = 0; i < T_COUNT; i++) { h->t_ms[i] = 0; h->t_n[i] = 0; }
  return MSFL_OK;
}

// =============================================================================================
// stage C
// =============================================================================================

msfl_status msfl_set_map(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf,
                         msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || (n_corner > 0 && !corner) || (n_surf > 0 && !surf))
    return fail(h, MSFL_BAD_ARG, "msfl_set_map: null cloud with positive size");
  h->have_map = false;
  h->pr.resident = false;                 // the single map takes the arrays a pair index lived in
  const float4* dc = reinterpret_cast<const float4*>(corner);
  const float4* ds = reinterpret_cast<const float4*>(surf);
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, h->idx_stage.reserve(std::max<size_t>(1, (size_t)n_corner + (size_t)n_surf) * sizeof(float4)));
    float4* stage = h->idx_stage.as<float4>();
    if (n_corner) HIPCHK(h, hipMemcpyAsync(stage, corner, (size_t)n_corner * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    if (n_surf) HIPCHK(h, hipMemcpyAsync(stage + n_corner, surf, (size_t)n_surf * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    dc = stage; ds = stage + n_corner;
  }
  if (n_corner > 0 && n_surf > 0 && !h->index_single) {
    s = build_index_pair(h, dc, n_corner, ds, n_surf); if (s) return s;
  } else {
    s = build_index(h, dc, n_corner, h->map_c); if (s) return s;
    s = build_index(h, ds, n_surf, h->map_s); if (s) return s;
  }
  // host arrays were staged with asynchronous copies from pageable memory: they must have been read
  // before the caller may touch them again.  Device-resident maps stay fully asynchronous.
  if (mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  h->have_map = true;
  return MSFL_OK;
}

static msfl_status match_batch_impl(msfl_handle* h, int B, const msfl_point* corner, const int* corner_off,
                                    const msfl_point* surf, const int* surf_off, double* poses_io, int* status,
                                    msfl_match_info* info, msfl_mem mem, const msfl_deskew_batch* deskew) {
  if (B < 0 || (B > 0 && (!corner_off || !surf_off || !poses_io)))
    return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map_batch: null argument");
  if (B == 0) return MSFL_OK;
  msfl_status s = reg_check(h, B, "msfl_match_scan2map"); if (s) return s;
  s = check_map(h); if (s) return s;
  hipStream_t st = h->stream;
  const int c0 = corner_off[0], s0 = surf_off[0];
  const int ncp = corner_off[B] - c0, nsp = surf_off[B] - s0;
  if (ncp < 0 || nsp < 0 || (ncp > 0 && !corner) || (nsp > 0 && !surf))
    return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map_batch: bad offsets or null feature array");
  const float4* d_corner; const float4* d_surf; double* d_poses; int* d_status;
  std::vector<int> co(corner_off, corner_off + B + 1), so(surf_off, surf_off + B + 1);
  // Host buffers, large batch, plain branch: the features go over PCIe in chunks of >= 512 scans on a second
  // stream while the previous chunk is being registered (82 MB per 1 024 scans is as long as the compute).
  const int n_chunks = (mem == MSFL_MEM_HOST && !deskew && B >= 2 * h->h2d_chunk_scans) ? std::min(8, B / h->h2d_chunk_scans) : 1;   // copy_ev[8] is the fork event
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, h->in_corner.reserve(std::max<size_t>(1, (size_t)ncp) * sizeof(float4)));
    HIPCHK(h, h->in_surf.reserve(std::max<size_t>(1, (size_t)nsp) * sizeof(float4)));
    HIPCHK(h, h->poses.reserve((size_t)B * 7 * sizeof(double)));
    if (n_chunks == 1) {
      if (ncp) HIPCHK(h, hipMemcpyAsync(h->in_corner.p, corner + c0, (size_t)ncp * sizeof(float4), hipMemcpyHostToDevice, st));
      if (nsp) HIPCHK(h, hipMemcpyAsync(h->in_surf.p, surf + s0, (size_t)nsp * sizeof(float4), hipMemcpyHostToDevice, st));
    }
    HIPCHK(h, hipMemcpyAsync(h->poses.p, poses_io, (size_t)B * 7 * sizeof(double), hipMemcpyHostToDevice, st));
    for (int b = 0; b <= B; b++) { co[b] -= c0; so[b] -= s0; }
    d_corner = h->in_corner.as<float4>(); d_surf = h->in_surf.as<float4>(); d_poses = h->poses.as<double>();
  } else {
    d_corner = reinterpret_cast<const float4*>(corner); d_surf = reinterpret_cast<const float4*>(surf);
    d_poses = poses_io;
  }
  if (mem == MSFL_MEM_DEVICE && status) {
    d_status = status;
  } else {
    HIPCHK(h, h->status.reserve((size_t)B * sizeof(int)));
    d_status = h->status.as<int>();
  }
  // (a kernel, not hipMemsetAsync: replayed from a captured HIP graph the memset node of a 24-byte status array wrote host-pointer
  // patterns into it from the second replay on -- ROCm 7.2, tests/test_gpu_scan2map.py::test_the_batch_step_replays_from_a_captured_graph)
  hipLaunchKernelGGL(zero_ints_kernel, dim3(div_up(B, 256)), dim3(256), 0, st, d_status, B);
  RegSinks sinks;
  s = reg_open(h, B, st, info != nullptr, &sinks); if (s) return s;
  DeskewView dv{}; const DeskewView* dvp = nullptr;
  if (deskew) {
    // the four per-feature arrays are indexed like the feature arrays (corner_off / surf_off), velocity per scan
    const double* src[5] = {deskew->corner_dq, deskew->corner_dp, deskew->surf_dq, deskew->surf_dp, deskew->velocity};
    const size_t nb[5] = {(size_t)ncp * 4, (size_t)ncp * 3, (size_t)nsp * 4, (size_t)nsp * 3, (size_t)B * 3};
    const size_t skip[5] = {(size_t)c0 * 4, (size_t)c0 * 3, (size_t)s0 * 4, (size_t)s0 * 3, 0};
    DevBuf* const buf[5] = {&h->dk.corner_dq, &h->dk.corner_dp, &h->dk.surf_dq, &h->dk.surf_dp, &h->dk.velocity};
    const double* dev[5];
    for (int k = 0; k < 5; k++) {
      if (nb[k] && !src[k]) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map_deskew: null deskew array");
      const double* used = mem == MSFL_MEM_HOST && src[k] ? src[k] + skip[k] : src[k];   // a host array's used part is what is staged
      s = stage_in(h, *buf[k], used, nb[k], mem, st, &dev[k]); if (s) return s;
    }
    dv.corner_dq = dev[0]; dv.corner_dp = dev[1]; dv.surf_dq = dev[2]; dv.surf_dp = dev[3]; dv.V = dev[4];
    for (int a = 0; a < 3; a++) dv.G[a] = deskew->gravity[a];
    dvp = &dv;
  }
  if (n_chunks == 1) {
    s = match_scan2map_device(h, B, d_corner, co.data(), d_surf, so.data(), d_poses, d_status, sinks, dvp);
    if (s) return s;
  } else {
    if (!h->copy_stream) {
      HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
      for (auto& e : h->copy_ev) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // the staging buffers may still be read by work queued earlier on the compute stream
    HIPCHK(h, hipEventRecord(h->copy_ev[8], st));
    HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->copy_ev[8], 0));
    // Two levels.  PARTS of >= h2d_chunk_scans scans are registered one after the other, each completely (a solve over a
    // fraction of the batch takes as long as one over all of it, so there are few parts): part p + 1 crosses PCIe while
    // part p is being registered.  Inside a part the FIRST association pass follows its SUB-chunks as they land, so a
    // part's kernels do not wait for all of its features either.
    const int n_sub = std::max(1, std::min(h->h2d_sub_chunks, 8));
    for (int p = 0; p < n_chunks; p++) {
      const int pb0 = (int)((long long)B * p / n_chunks), pb1 = (int)((long long)B * (p + 1) / n_chunks), Bp = pb1 - pb0;
      const int ns_p = std::max(1, std::min(n_sub, Bp / 32));
      int sub_b[9];
      for (int c = 0; c <= ns_p; c++) sub_b[c] = (int)((long long)Bp * c / ns_p);
      const std::function<hipError_t(int)> enqueue_chunk = [&](int c) -> hipError_t {
        const int b0 = pb0 + sub_b[c], b1 = pb0 + sub_b[c + 1];
        const size_t nc = (size_t)(co[b1] - co[b0]), ns = (size_t)(so[b1] - so[b0]);
        hipError_t e = hipSuccess;
        if (nc) e = hipMemcpyAsync(h->in_corner.as<float4>() + co[b0], corner + c0 + co[b0], nc * sizeof(float4), hipMemcpyHostToDevice, h->copy_stream);
        if (ns && e == hipSuccess) e = hipMemcpyAsync(h->in_surf.as<float4>() + so[b0], surf + s0 + so[b0], ns * sizeof(float4), hipMemcpyHostToDevice, h->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(h->copy_ev[c], h->copy_stream);
        return e;
      };
      s = match_scan2map_device(h, Bp, d_corner, co.data() + pb0, d_surf, so.data() + pb0, d_poses + 7 * (size_t)pb0, d_status + pb0,
                                sinks.at(pb0), nullptr, ns_p, sub_b, h->copy_ev, &enqueue_chunk);
      if (s) return s;
    }
  }
  return reg_close(h, B, mem, poses_io, d_poses, status, d_status, info, sinks);
}

msfl_status msfl_match_scan2map_batch(msfl_handle* h, int n_scans, const msfl_point* corner, const int* corner_off,
                                      const msfl_point* surf, const int* surf_off, double* poses_io, int* status,
                                      msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  return match_batch_impl(h, n_scans, corner, corner_off, surf, surf_off, poses_io, status, info, mem, nullptr);
}

msfl_status msfl_match_scan2map(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf,
                                int n_surf, double pose_io[7], msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose_io) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map: bad argument");
  const int co[2] = {0, n_corner}, so[2] = {0, n_surf};
  int st = 0;
  int* stp = (mem == MSFL_MEM_HOST) ? &st : nullptr;
  s = match_batch_impl(h, 1, corner, co, surf, so, pose_io, stp, info, mem, nullptr);
  if (s) return s;
  return (msfl_status)st;
}

msfl_status msfl_match_scan2map_deskew(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf,
                                       int n_surf, const msfl_deskew* deskew, double pose_io[7], msfl_match_info* info) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose_io || !deskew) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map_deskew: bad argument");
  const int co[2] = {0, n_corner}, so[2] = {0, n_surf};
  int st = 0;
  msfl_deskew_batch db;
  db.corner_dq = deskew->corner_dq; db.corner_dp = deskew->corner_dp; db.surf_dq = deskew->surf_dq; db.surf_dp = deskew->surf_dp;
  db.velocity = deskew->velocity;
  for (int a = 0; a < 3; a++) db.gravity[a] = deskew->gravity[a];
  s = match_batch_impl(h, 1, corner, co, surf, so, pose_io, &st, info, MSFL_MEM_HOST, &db);
  if (s) return s;
  return (msfl_status)st;
}

msfl_status msfl_match_scan2map_deskew_batch(msfl_handle* h, int n_scans, const msfl_point* corner, const int* corner_off,
                                             const msfl_point* surf, const int* surf_off, const msfl_deskew_batch* deskew,
                                             double* poses_io, int* status, msfl_match_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  if (!deskew) return fail(h, MSFL_BAD_ARG, "msfl_match_scan2map_deskew_batch: null deskew");
  return match_batch_impl(h, n_scans, corner, corner_off, surf, surf_off, poses_io, status, info, mem, deskew);
}

static msfl_status stage_single(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf,
                                const double* pose, BatchView& bv) {
  hipStream_t st = h->stream;
  HIPCHK(h, h->poses.reserve(7 * sizeof(double)));
  HIPCHK(h, h->status.reserve(sizeof(int)));
  HIPCHK(h, h->records.reserve(record_bytes((size_t)n_corner + (size_t)n_surf, (size_t)n_surf)));
  HIPCHK(h, h->nn.reserve(std::max<size_t>(1, (size_t)(n_corner + n_surf)) * 5 * sizeof(int)));
  const float4 *d_corner, *d_surf;
  msfl_status s = stage_in(h, h->in_corner, corner, (size_t)n_corner, MSFL_MEM_HOST, st, &d_corner); if (s) return s;
  s = stage_in(h, h->in_surf, surf, (size_t)n_surf, MSFL_MEM_HOST, st, &d_surf); if (s) return s;
  HIPCHK(h, hipMemcpyAsync(h->poses.p, pose, 7 * sizeof(double), hipMemcpyHostToDevice, st));     // (the callers read h->poses and h->status)
  HIPCHK(h, hipMemsetAsync(h->status.p, 0, sizeof(int), st));
  const int co[2] = {0, n_corner}, so[2] = {0, n_surf};
  int n_rec = 0;
  s = upload_batch_offsets(h, 1, co, so, &n_rec); if (s) return s;
  bv = batch_view(d_corner, d_surf, h->in_off.as<int>(), 2, 1, n_rec, 0, 0, n_surf);
  return MSFL_OK;
}

msfl_status msfl_associate_scan2map(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf,
                                    int n_surf, const double pose[7], double* records_out) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose || (n_corner + n_surf > 0 && !records_out) || (n_corner && !corner) || (n_surf && !surf))
    return fail(h, MSFL_BAD_ARG, "msfl_associate_scan2map: bad argument");
  s = check_map(h); if (s) return s;
  const int n = n_corner + n_surf;
  if (n == 0) return MSFL_OK;
  BatchView bv;
  s = stage_single(h, corner, n_corner, surf, n_surf, pose, bv); if (s) return s;
  DeskewView dv{};
  HIPCHK(h, h->pprime.reserve((size_t)n * 6 * sizeof(double)));   // {C,N} staging for the host-format output
  s_launch_assoc(h, bv, h->poses.as<double>(), h->status.as<int>(), false, dv, n, h->pprime.as<double>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(records_out, h->pprime.p, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MSFL_OK;
}

// The de-skew form of msfl_associate_scan2map: the launch pair msfl_match_scan2map_deskew takes, at a fixed pose.  h->pprime holds
// the {C', N} staging in its first 6 n doubles and p' in the 3 n doubles behind them.
msfl_status msfl_associate_scan2map_deskew(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf,
                                           int n_surf, const msfl_deskew* deskew, const double pose[7], double* records_out,
                                           double* points_out) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose || !deskew || (n_corner + n_surf > 0 && (!records_out || !points_out)) ||
      (n_corner && (!corner || !deskew->corner_dq || !deskew->corner_dp)) || (n_surf && (!surf || !deskew->surf_dq || !deskew->surf_dp)))
    return fail(h, MSFL_BAD_ARG, "msfl_associate_scan2map_deskew: bad argument");
  s = check_map(h); if (s) return s;
  const int n = n_corner + n_surf;
  if (n == 0) return MSFL_OK;
  BatchView bv;
  s = stage_single(h, corner, n_corner, surf, n_surf, pose, bv); if (s) return s;
  DeskewView dv{};
  s = stage_in(h, h->dk.corner_dq, deskew->corner_dq, (size_t)n_corner * 4, MSFL_MEM_HOST, h->stream, &dv.corner_dq); if (s) return s;
  s = stage_in(h, h->dk.corner_dp, deskew->corner_dp, (size_t)n_corner * 3, MSFL_MEM_HOST, h->stream, &dv.corner_dp); if (s) return s;
  s = stage_in(h, h->dk.surf_dq, deskew->surf_dq, (size_t)n_surf * 4, MSFL_MEM_HOST, h->stream, &dv.surf_dq); if (s) return s;
  s = stage_in(h, h->dk.surf_dp, deskew->surf_dp, (size_t)n_surf * 3, MSFL_MEM_HOST, h->stream, &dv.surf_dp); if (s) return s;
  s = stage_in(h, h->dk.velocity, deskew->velocity, (size_t)3, MSFL_MEM_HOST, h->stream, &dv.V); if (s) return s;
  for (int a = 0; a < 3; a++) dv.G[a] = deskew->gravity[a];
  HIPCHK(h, h->pprime.reserve((size_t)n * 9 * sizeof(double)));
  double* full = h->pprime.as<double>();
  dv.pprime = full + 6 * (size_t)n;
  s_launch_assoc(h, bv, h->poses.as<double>(), h->status.as<int>(), true, dv, n, full);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(records_out, full, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(points_out, dv.pprime, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MSFL_OK;
}

}  // extern "C"

namespace {
// One solve of the records already in h->records, in the workgroup MSFL_SOLVE_RECORDS_BLOCK chose; pprime: the de-skew branch's f64
// points (device, n x 3) or null.  Defined at the end of this file: kSlamLmBlock and the SLAM step's <kSlamLmBlock> instantiations,
// which this only reuses, come with msfl_api_slam.inc.
msfl_status solve_given_records(msfl_handle* h, const BatchView& bv, const RegSinks& sinks, const double* pprime);

// msfl_solve_records (points == nullptr) and msfl_solve_records_deskew: h->pprime holds the {C, N} staging in its first 6 n doubles
// and, for the de-skew form, the points in the 3 n doubles behind them.
msfl_status solve_records_impl(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf,
                               const double* records, const double* points, double pose_io[7], msfl_match_info* info, const char* who) {
  const int n = n_corner + n_surf;
  msfl_status s = reg_check(h, 1, who); if (s) return s;
  BatchView bv;
  s = stage_single(h, corner, n_corner, surf, n_surf, pose_io, bv); if (s) return s;
  RegSinks sinks;
  s = reg_open(h, 1, h->stream, info != nullptr, &sinks); if (s) return s;
  if (n || points) HIPCHK(h, h->pprime.reserve(std::max<size_t>(1, (size_t)n * (points ? 9 : 6)) * sizeof(double)));
  // (an empty problem too: the solve kernels take the de-skew branch on the pointer alone)
  const double* d_points = points ? h->pprime.as<double>() + 6 * (size_t)n : nullptr;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(h->pprime.p, records, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (points) HIPCHK(h, hipMemcpyAsync(h->pprime.as<double>() + 6 * (size_t)n, points, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(pack_records_kernel, dim3(div_up(n, 256)), dim3(256), 0, h->stream, bv, (const double*)h->pprime.as<double>(),
                       h->records.as<double>());
  }
  s = solve_given_records(h, bv, sinks, d_points);
  if (s) return s;
  return reg_close(h, 1, MSFL_MEM_HOST, pose_io, h->poses.as<double>(), nullptr, nullptr, info, sinks);   // (host memory: always waited for)
}
}  // namespace

extern "C" {

msfl_status msfl_solve_records(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf,
                               const double* records, double pose_io[7], msfl_match_info* info) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose_io || (n_corner + n_surf > 0 && !records) || (n_corner && !corner) || (n_surf && !surf))
    return fail(h, MSFL_BAD_ARG, "msfl_solve_records: bad argument");
  return solve_records_impl(h, corner, n_corner, surf, n_surf, records, nullptr, pose_io, info, "msfl_solve_records");
}

msfl_status msfl_solve_records_deskew(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf,
                                      const double* records, const double* points, double pose_io[7], msfl_match_info* info) {
  msfl_status s = enter(h); if (s) return s;
  if (n_corner < 0 || n_surf < 0 || !pose_io || !points || (n_corner + n_surf > 0 && !records) || (n_corner && !corner) || (n_surf && !surf))
    return fail(h, MSFL_BAD_ARG, "msfl_solve_records_deskew: bad argument");
  return solve_records_impl(h, corner, n_corner, surf, n_surf, records, points, pose_io, info, "msfl_solve_records_deskew");
}

}  // extern "C"

#include "msfl_api_stage_ab.inc"
#include "msfl_api_grid.inc"
#include "msfl_api_deskew.inc"
#include "msfl_api_slam.inc"
#include "msfl_api_pairs.inc"
#include "msfl_api_score.inc"
#include "msfl_api_search.inc"
#include "msfl_api_segment.inc"
#include "msfl_api_novelty.inc"
#include "msfl_api_place.inc"

namespace {

msfl_status solve_given_records(msfl_handle* h, const BatchView& bv, const RegSinks& sinks, const double* pprime) {
  const auto no_assoc = [](int) { return MSFL_OK; };        // the records are given: nothing to associate
  const SolverParams sp = solver_params(h->prm, 0);
  if (h->solve_records_block == kSlamLmBlock)                // (any other value, kLmBlock included: the default workgroup)
    return solve_outer<kSlamLmBlock>(h, 1, bv, pprime, h->poses.as<double>(), h->status.as<int>(), sinks, sp, 1, no_assoc);
  return solve_outer<kLmBlock>(h, 1, bv, pprime, h->poses.as<double>(), h->status.as<int>(), sinks, sp, 1, no_assoc);
}

}  // namespace
#include "msfl_api_graph.inc"
#include "msfl_api_keyframes.inc"
