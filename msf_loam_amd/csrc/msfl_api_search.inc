// Pose search over the resident single map — C-ABI entry points msfl_search_default_config, msfl_search_geometry, msfl_search_poses
// and msfl_relocalize — and over the resident pair index, scan p round guess p against pair map p — msfl_search_pairs.  Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros); kernels:
// msfl_search.cuh.  The search stages into scratch of its own (h->se) and reads only the sorted point arrays of the map index: a
// matcher or scoring call after it finds the handle as it left it.  msfl_relocalize is a chain of the public calls.

#include "msfl_search.cuh"

namespace {

static_assert(sizeof(SearchCand) == sizeof(msfl_pose_candidate) && sizeof(msfl_pose_candidate) == 88, "pose candidate record layout");
static_assert(sizeof(msfl_reloc_result) == 216, "relocalisation record layout");
static_assert(kSearchSelectBlock == kSearchMaxK, "the select kernel sorts one key per thread");

constexpr long long kSearchMaxHyp = 1ll << 24;        // hypothesis indices and totals share a 64-bit key; one workgroup selects
constexpr int kSearchMaxDim = 1 << 20;                // voxels per axis (and half-extent) of the volume
constexpr long long kSearchMaxTable = 1ll << 26;      // (yaw, feature) table entries

// The geometry rule (msfl_c_api.h).  *why: what a refusal says.
msfl_status search_geometry(const double* guess, const msfl_search_config* c, int n_corner, int n_surf, msfl_search_geom* out, std::string* why) {
  if (!guess || !c || !out) { *why = "null pointer"; return MSFL_BAD_ARG; }
  std::memset(out, 0, sizeof(*out));
  for (int k = 0; k < 7; k++) if (!std::isfinite(guess[k])) { *why = "the guess has a non-finite entry"; return MSFL_BAD_ARG; }
  const char* bad = nullptr;
  if (!(c->step > 0.0) || !std::isfinite(c->step)) bad = "step must be positive and finite";
  else if (!(c->range > 0.0) || !std::isfinite(c->range)) bad = "range must be positive and finite";
  else if (c->half[0] < 0 || c->half[1] < 0 || c->half[2] < 0) bad = "negative half-extent";
  else if (c->n_yaw < 1) bad = "n_yaw below 1";
  else if (!std::isfinite(c->yaw_min) || !std::isfinite(c->yaw_step)) bad = "yaw_min / yaw_step not finite";
  else if ((c->dilate != 0 && c->dilate != 1) || (c->yaw_wraps != 0 && c->yaw_wraps != 1)) bad = "dilate and yaw_wraps are 0 or 1";
  else if (c->nms_cells < 0 || c->nms_yaws < 0) bad = "negative peak window";
  else if (c->max_volume_bytes <= 0) bad = "max_volume_bytes must be positive";
  else if (n_corner < 0 || n_surf < 0) bad = "negative feature count";
  if (bad) { *why = bad; return MSFL_BAD_ARG; }
  const double inv = 1.0 / c->step;
  out->inv_step = (float)inv;
  if (!std::isfinite(out->inv_step) || !(out->inv_step > 0.f)) { *why = "1 / step is not a finite positive float"; return MSFL_BAD_ARG; }
  const double reach = std::ceil(c->range / c->step);
  const char* cap = nullptr;
  if (!(reach <= (double)kSearchMaxDim)) cap = "range / step above 2^20 cells";
  for (int a = 0; a < 3 && !cap; a++) if (c->half[a] > kSearchMaxDim) cap = "a half-extent above 2^20 cells";
  if (cap) { *why = cap; return MSFL_CAPACITY; }
  double words = 1.0;
  for (int a = 0; a < 3; a++) {
    const long long ext = (long long)c->half[a] + (long long)reach + c->dilate + 1;
    const long long dim = 2 * ext + 1;
    const double o = (std::floor(guess[a] / c->step) - (double)ext) * c->step;
    out->origin[a] = (float)o;
    if (!std::isfinite(out->origin[a])) { *why = "the box origin is not a finite float"; return MSFL_BAD_ARG; }
    out->n[a] = 2 * c->half[a] + 1;
    if (dim > kSearchMaxDim) { cap = "a volume dimension above 2^20 voxels"; out->dims[a] = kSearchMaxDim; continue; }
    out->dims[a] = (int)dim;
  }
  out->n_yaw = c->n_yaw;
  out->words_per_row = (out->dims[0] + 63) / 64 + 1;
  words = (double)out->words_per_row * (double)out->dims[1] * (double)out->dims[2];
  double hyp = (double)c->n_yaw * (double)out->n[0] * (double)out->n[1] * (double)out->n[2];
  out->n_hypotheses = hyp < 9.0e18 ? (long long)hyp : (long long)9.0e18;       // (exact below 2^53; only compared above)
  out->volume_bytes = words * 8.0 < 9.0e18 ? (long long)(words * 8.0) : (long long)9.0e18;
  const long long F = (long long)n_corner + n_surf;
  if (!cap && out->volume_bytes > c->max_volume_bytes) cap = "a volume above max_volume_bytes";
  if (!cap && out->n_hypotheses > kSearchMaxHyp) cap = "more than 2^24 hypotheses";
  if (!cap && (n_corner >= (1 << 24) || n_surf >= (1 << 24))) cap = "2^24 features or more of a kind";
  if (!cap && (long long)c->n_yaw * F > kSearchMaxTable) cap = "more than 2^26 (yaw, feature) table entries";
  if (cap) { *why = cap; return MSFL_CAPACITY; }
  out->scratch_bytes = 2ll * (1 + c->dilate) * out->volume_bytes + 16ll * c->n_yaw * F + 16ll * out->n_hypotheses + 32ll * c->n_yaw + 56 +
                       (long long)sizeof(SearchCand) * kSearchMaxK + 8;
  return MSFL_OK;
}

// q = normalised(qz(yaw) * q_guess): the host computes it once per yaw sample (libm's sin and cos, IEEE sqrt and division), the
// kernels and the candidate records copy it
void search_yaw_quat(const double* guess, double yaw, double* q) {
  const double hy = yaw * 0.5;
  const double az = std::sin(hy), aw = std::cos(hy);                    // a = (0, 0, az, aw)
  const double bx = guess[3], by = guess[4], bz = guess[5], bw = guess[6];
  const double x = aw * bx - az * by, y = aw * by + az * bx, z = aw * bz + az * bw, w = aw * bw - az * bz;
  const double n = std::sqrt(((x * x + y * y) + z * z) + w * w);
  q[0] = x; q[1] = y; q[2] = z; q[3] = w;
  if (n > 0.0) { q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = w / n; }
}

// what the kernels take of the geometry
SearchGeom search_kernel_geom(const msfl_search_geom& gm, const msfl_search_config* c) {
  SearchGeom g{};
  g.ox = gm.origin[0]; g.oy = gm.origin[1]; g.oz = gm.origin[2]; g.inv = gm.inv_step;
  g.dx = gm.dims[0]; g.dy = gm.dims[1]; g.dz = gm.dims[2]; g.W = gm.words_per_row;
  g.nx = gm.n[0]; g.ny = gm.n[1]; g.nz = gm.n[2]; g.n_yaw = gm.n_yaw;
  g.hx = c->half[0]; g.hy = c->half[1]; g.hz = c->half[2];
  return g;
}

// The search on the stream: candidates in h->se.cand (device), their count in h->se.ctr[1]; d_n_out / d_hits: device pointers the
// kernels also write (null: none; without d_hits the counts live in h->se.hits).  corner / surf are device pointers.
msfl_status search_run(msfl_handle* h, const float4* d_corner, int n_corner, const float4* d_surf, int n_surf, const double* guess,
                       const msfl_search_config* c, const msfl_search_geom& gm, int K, int* d_n_out, int* d_hits, int** hits_used) {
  hipStream_t st = h->stream;
  const SearchGeom g = search_kernel_geom(gm, c);
  const int H = (int)gm.n_hypotheses, F = n_corner + n_surf;
  const size_t vol_words = (size_t)gm.volume_bytes / 8;
  const size_t all_words = 2 * (size_t)(1 + c->dilate) * vol_words;

  HIPCHK(h, h->se.vol.reserve(all_words * 8));
  HIPCHK(h, h->se.tab.reserve(std::max<size_t>(1, (size_t)gm.n_yaw * F) * sizeof(int4)));
  if (!d_hits) { HIPCHK(h, h->se.hits.reserve(2 * (size_t)H * sizeof(int))); d_hits = h->se.hits.as<int>(); }
  HIPCHK(h, h->se.peaks.reserve((size_t)H * sizeof(unsigned long long)));
  HIPCHK(h, h->se.cand.reserve(kSearchMaxK * sizeof(SearchCand)));
  HIPCHK(h, h->se.ctr.reserve(2 * sizeof(int)));
  HIPCHK(h, h->se.qtab.reserve(((size_t)gm.n_yaw * 4 + 7) * sizeof(double)));
  std::vector<double> qt((size_t)gm.n_yaw * 4 + 7);
  for (int a = 0; a < gm.n_yaw; a++) search_yaw_quat(guess, c->yaw_min + (double)a * c->yaw_step, &qt[4 * (size_t)a]);
  for (int k = 0; k < 7; k++) qt[(size_t)gm.n_yaw * 4 + k] = guess[k];
  HIPCHK(h, h->pin.upload(h->se.qtab.p, qt.data(), qt.size() * sizeof(double), st));
  const double* d_qtab = h->se.qtab.as<double>();
  const double* d_guess = d_qtab + (size_t)gm.n_yaw * 4;

  unsigned long long* raw_c = h->se.vol.as<unsigned long long>();
  unsigned long long* raw_s = raw_c + vol_words;
  unsigned long long *use_c = raw_c, *use_s = raw_s;
  int* ctr = h->se.ctr.as<int>();
  hipLaunchKernelGGL(search_clear_kernel, dim3((unsigned)((std::max<size_t>(all_words, 2) + kSearchBlock - 1) / kSearchBlock)), dim3(kSearchBlock), 0, st,
                     raw_c, all_words, ctr, 2);
  const int n_mc = h->map_c.n_input, n_ms = h->map_s.n_input;
  if (n_mc > 0)
    hipLaunchKernelGGL(search_fill_kernel, dim3(div_up(n_mc, kSearchBlock)), dim3(kSearchBlock), 0, st, g, (const GridDesc*)h->map_c.gdesc.as<GridDesc>(),
                       (const float4*)h->map_c.sorted.as<float4>(), raw_c);
  if (n_ms > 0)
    hipLaunchKernelGGL(search_fill_kernel, dim3(div_up(n_ms, kSearchBlock)), dim3(kSearchBlock), 0, st, g, (const GridDesc*)h->map_s.gdesc.as<GridDesc>(),
                       (const float4*)h->map_s.sorted.as<float4>(), raw_s);
  if (c->dilate) {
    use_c = raw_s + vol_words; use_s = use_c + vol_words;
    const unsigned blocks = (unsigned)((vol_words + kSearchBlock - 1) / kSearchBlock);
    hipLaunchKernelGGL(search_dilate_kernel, dim3(blocks), dim3(kSearchBlock), 0, st, g, (const unsigned long long*)raw_c, use_c);
    hipLaunchKernelGGL(search_dilate_kernel, dim3(blocks), dim3(kSearchBlock), 0, st, g, (const unsigned long long*)raw_s, use_s);
  }
  int4* tab = h->se.tab.as<int4>();
  if (F > 0)
    hipLaunchKernelGGL(search_table_kernel, dim3((unsigned)(((size_t)gm.n_yaw * F + kSearchBlock - 1) / kSearchBlock)), dim3(kSearchBlock), 0, st, g,
                       d_corner, n_corner, d_surf, n_surf, d_qtab, d_guess, tab);
  const int chunks = div_up(g.nx, 64);
  hipLaunchKernelGGL(search_correlate_kernel, dim3((unsigned)((size_t)gm.n_yaw * g.nz * g.ny * chunks)), dim3(64), 0, st, g, (const int4*)tab, n_corner,
                     n_surf, (const unsigned long long*)use_c, (const unsigned long long*)use_s, chunks, d_hits, H);
  hipLaunchKernelGGL(search_peaks_kernel, dim3(div_up(H, kSearchBlock)), dim3(kSearchBlock), 0, st, g, (const int*)d_hits, H, c->nms_cells, c->nms_yaws,
                     c->yaw_wraps, h->se.peaks.as<unsigned long long>(), ctr);
  hipLaunchKernelGGL(search_select_kernel, dim3(1), dim3(kSearchSelectBlock), 0, st, g, (const unsigned long long*)h->se.peaks.as<unsigned long long>(), ctr,
                     K, (const int*)d_hits, H, d_qtab, d_guess, c->step, h->se.cand.as<SearchCand>(), d_n_out);
  HIPCHK(h, hipGetLastError());
  if (hits_used) *hits_used = d_hits;
  return MSFL_OK;
}

// What both entry points refuse before anything is staged or launched.
msfl_status search_check(msfl_handle* h, const std::string& w, const void* corner, int n_corner, const void* surf, int n_surf, const double* guess,
                         const msfl_search_config* c, int capacity, msfl_mem mem, msfl_search_geom* gm) {
  if (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE) return fail(h, MSFL_BAD_ARG, w + ": unknown memory kind");
  if (n_corner < 0 || n_surf < 0 || (n_corner > 0 && !corner) || (n_surf > 0 && !surf)) return fail(h, MSFL_BAD_ARG, w + ": negative count or null cloud");
  if (capacity < 1 || capacity > kSearchMaxK) return fail(h, MSFL_BAD_ARG, w + ": the candidate capacity must be 1 .. 1024");
  std::string why;
  const msfl_status s = search_geometry(guess, c, n_corner, n_surf, gm, &why);
  if (s) return fail(h, s, w + ": " + why);
  if (!h->have_map || h->pr.resident)
    return fail(h, MSFL_NO_MAP, w + ": no resident single map (msfl_set_map has not been called, or a pair index replaced it)");
  return MSFL_OK;
}

// msfl_search_pairs: device scratch the pairs of one chunk may take together (volumes, table, counts, keys, records).  A pair
// needs 2 (1 + dilate) volume_bytes + 16 n_yaw F + 16 H + 88 K; one pair always runs, whatever it needs (max_volume_bytes bounds it).
constexpr long long kSearchPairsBudget = 256ll << 20;
constexpr int kSearchPairsMaxChunk = 65535;          // gridDim.y

// The P searches on the stream, chunk by chunk.  Checked arguments; gms[p]: the geometry of pair p (they differ in origin only);
// co / so: P + 1 offsets into d_corner / d_surf.  Host memory: every chunk is waited for and its results copied out.
msfl_status search_pairs_run(msfl_handle* h, int P, const float4* d_corner, const int* co, const float4* d_surf, const int* so, const double* guesses,
                             const msfl_search_config* c, const std::vector<msfl_search_geom>& gms, int K, msfl_pose_candidate* candidates, int* n_out,
                             int* hits_out, bool dev) {
  hipStream_t st = h->stream;
  const msfl_search_geom& gm = gms[0];
  const SearchGeom g = search_kernel_geom(gm, c);              // (the origin is pair 0's: the pairs kernels take theirs from the table)
  const int H = (int)gm.n_hypotheses, n_yaw = gm.n_yaw;
  const size_t vol_words = (size_t)gm.volume_bytes / 8;
  const size_t pair_words = 2 * (size_t)(1 + c->dilate) * vol_words;
  const size_t q_stride = 4 * (size_t)n_yaw + 7;
  int f_max = 0;
  for (int p = 0; p < P; p++) f_max = std::max(f_max, (co[p + 1] - co[p]) + (so[p + 1] - so[p]));
  const long long per_pair = (long long)pair_words * 8 + 16ll * n_yaw * f_max + 16ll * H + (long long)sizeof(SearchCand) * K + 8;
  long long C_ll = h->search_chunk_pairs > 0 ? h->search_chunk_pairs : std::max<long long>(1, kSearchPairsBudget / per_pair);
  const int C = (int)std::min<long long>(std::min<long long>(C_ll, kSearchPairsMaxChunk), P);

  // the tables of all P pairs, uploaded once: yaw quaternions and guess, origin, feature ranges, table offsets (inside the pair's chunk)
  std::vector<double> qt((size_t)P * q_stride);
  std::vector<SearchPair> pt((size_t)P);
  size_t tab_max = 1;
  for (int p0 = 0; p0 < P; p0 += C) {
    size_t at = 0;
    for (int p = p0; p < std::min(P, p0 + C); p++) {
      const double* guess = guesses + 7 * (size_t)p;
      double* q = &qt[(size_t)p * q_stride];
      for (int a = 0; a < n_yaw; a++) search_yaw_quat(guess, c->yaw_min + (double)a * c->yaw_step, q + 4 * (size_t)a);
      for (int k = 0; k < 7; k++) q[4 * (size_t)n_yaw + k] = guess[k];
      SearchPair& e = pt[p];
      e.ox = gms[p].origin[0]; e.oy = gms[p].origin[1]; e.oz = gms[p].origin[2];
      e.n_corner = co[p + 1] - co[p]; e.n_surf = so[p + 1] - so[p];
      e.corner0 = co[p]; e.surf0 = so[p];
      e.reserved_ = 0;
      e.tab0 = at;
      at += (size_t)n_yaw * (size_t)(e.n_corner + e.n_surf);
    }
    tab_max = std::max(tab_max, at);
  }
  const bool own_hits = !(dev && hits_out);
  HIPCHK(h, h->se.vol.reserve((size_t)C * pair_words * 8));
  HIPCHK(h, h->se.tab.reserve(tab_max * sizeof(int4)));
  if (own_hits) HIPCHK(h, h->se.hits.reserve(2 * (size_t)C * H * sizeof(int)));
  HIPCHK(h, h->se.peaks.reserve((size_t)C * H * sizeof(unsigned long long)));
  if (!dev) HIPCHK(h, h->se.cand.reserve((size_t)C * K * sizeof(SearchCand)));
  HIPCHK(h, h->se.ctr.reserve(2 * (size_t)C * sizeof(int)));
  HIPCHK(h, h->se.qtab.reserve(qt.size() * sizeof(double)));
  HIPCHK(h, h->se.pair.reserve(pt.size() * sizeof(SearchPair)));
  HIPCHK(h, h->pin.upload(h->se.qtab.p, qt.data(), qt.size() * sizeof(double), st));
  HIPCHK(h, h->pin.upload(h->se.pair.p, pt.data(), pt.size() * sizeof(SearchPair), st));
  std::vector<SearchCand> got;                                  // host memory: a chunk's records before the first n of every pair go out
  if (!dev) { got.resize((size_t)C * K); HIPCHK(h, h->readback.reserve(2 * (size_t)C * sizeof(int))); }

  const int chunks = div_up(g.nx, 64);
  for (int p0 = 0; p0 < P; p0 += C) {
    const int n = std::min(C, P - p0);
    SearchPairsView v{};
    v.pair = h->se.pair.as<SearchPair>() + p0;
    v.qtab = h->se.qtab.as<double>() + (size_t)p0 * q_stride;
    v.vol = h->se.vol.as<unsigned long long>(); v.vol_words = vol_words;
    v.tab = h->se.tab.as<int4>();
    v.hits = own_hits ? h->se.hits.as<int>() : hits_out + 2 * (size_t)p0 * H;
    v.peaks = h->se.peaks.as<unsigned long long>();
    v.ctr = h->se.ctr.as<int>();
    v.cand = dev ? reinterpret_cast<SearchCand*>(candidates) + (size_t)p0 * K : h->se.cand.as<SearchCand>();
    v.n_out = dev ? n_out + p0 : nullptr;
    v.n_pairs = n; v.dilate = c->dilate; v.H = H; v.K = K;
    int map_c = 0, map_s = 0, f_most = 0;                       // the chunk's longest map of each kind, its scan with the most features
    for (int p = p0; p < p0 + n; p++) {
      map_c = std::max(map_c, h->pr.n_c[p]); map_s = std::max(map_s, h->pr.n_s[p]);
      f_most = std::max(f_most, pt[p].n_corner + pt[p].n_surf);
    }
    const size_t all_words = (size_t)n * pair_words;
    hipLaunchKernelGGL(search_clear_kernel, dim3((unsigned)((std::max<size_t>(all_words, 2 * (size_t)n) + kSearchBlock - 1) / kSearchBlock)), dim3(kSearchBlock), 0,
                       st, v.vol, all_words, v.ctr, 2 * n);
    if (map_c > 0)
      hipLaunchKernelGGL(search_fill_pairs_kernel, dim3(div_up(map_c, kSearchBlock), n), dim3(kSearchBlock), 0, st, g, v, 0, (const int*)h->map_c.cell_start.as<int>(),
                         (const int*)h->pr.base_c.as<int>() + p0, (const float4*)h->map_c.sorted.as<float4>());
    if (map_s > 0)
      hipLaunchKernelGGL(search_fill_pairs_kernel, dim3(div_up(map_s, kSearchBlock), n), dim3(kSearchBlock), 0, st, g, v, 1, (const int*)h->map_s.cell_start.as<int>(),
                         (const int*)h->pr.base_s.as<int>() + p0, (const float4*)h->map_s.sorted.as<float4>());
    if (c->dilate)
      hipLaunchKernelGGL(search_dilate_pairs_kernel, dim3((unsigned)((2 * (size_t)n * vol_words + kSearchBlock - 1) / kSearchBlock)), dim3(kSearchBlock), 0, st, g, v);
    if (f_most > 0)
      hipLaunchKernelGGL(search_table_pairs_kernel, dim3((unsigned)(((size_t)n_yaw * f_most + kSearchBlock - 1) / kSearchBlock), n), dim3(kSearchBlock), 0, st, g, v,
                         d_corner, d_surf);
    hipLaunchKernelGGL(search_correlate_pairs_kernel, dim3((unsigned)((size_t)n_yaw * g.nz * g.ny * chunks), n), dim3(64), 0, st, g, v, chunks);
    hipLaunchKernelGGL(search_peaks_pairs_kernel, dim3(div_up(H, kSearchBlock), n), dim3(kSearchBlock), 0, st, g, v, c->nms_cells, c->nms_yaws, c->yaw_wraps);
    hipLaunchKernelGGL(search_select_pairs_kernel, dim3(1, n), dim3(kSearchSelectBlock), 0, st, g, v, c->step);
    HIPCHK(h, hipGetLastError());
    if (dev) continue;
    HIPCHK(h, hipMemcpyAsync(h->readback.p, v.ctr, 2 * (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (hits_out) HIPCHK(h, hipMemcpyAsync(hits_out + 2 * (size_t)p0 * H, v.hits, 2 * (size_t)n * H * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(got.data(), v.cand, (size_t)n * K * sizeof(SearchCand), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int p = 0; p < n; p++) {
      const int k = h->readback.as<int>()[2 * p + 1];
      if (k > 0) std::memcpy(candidates + (size_t)(p0 + p) * K, &got[(size_t)p * K], (size_t)k * sizeof(SearchCand));
      n_out[p0 + p] = k;
    }
  }
  return MSFL_OK;
}

inline long long score_inliers(const msfl_pose_score& r) { return (long long)r.inliers[0] + r.inliers[1]; }
// (each sum is below 2^63, their sum below 2^64)
inline unsigned long long score_sum(const msfl_pose_score& r) { return r.sum_sq_q32[0] + r.sum_sq_q32[1]; }
// exact inliers descending, fixed-point sum ascending, then the order they came in
void score_order(const std::vector<msfl_pose_score>& sc, std::vector<int>* order) {
  order->resize(sc.size());
  for (size_t i = 0; i < sc.size(); i++) (*order)[i] = (int)i;
  std::stable_sort(order->begin(), order->end(), [&](int a, int b) {
    if (score_inliers(sc[a]) != score_inliers(sc[b])) return score_inliers(sc[a]) > score_inliers(sc[b]);
    return score_sum(sc[a]) < score_sum(sc[b]);
  });
}

}  // namespace

extern "C" {

void msfl_search_default_config(msfl_search_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->step = 0.5;
  cfg->half[0] = 6; cfg->half[1] = 6; cfg->half[2] = 0;
  cfg->n_yaw = 24;
  cfg->yaw_min = 0.0;
  cfg->yaw_step = 2.0 * 3.14159265358979323846 / 24.0;
  cfg->yaw_wraps = 1;
  cfg->dilate = 1;
  cfg->range = 100.0;
  cfg->nms_cells = 1; cfg->nms_yaws = 1;
  cfg->max_volume_bytes = 64ll << 20;
}

msfl_status msfl_search_geometry(const double guess[7], const msfl_search_config* cfg, int n_corner, int n_surf, msfl_search_geom* out) {
  std::string why;
  return search_geometry(guess, cfg, n_corner, n_surf, out, &why);
}

msfl_status msfl_search_poses(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, const double guess[7],
                              const msfl_search_config* cfg, msfl_pose_candidate* candidates, int capacity, int* n_out, int* hits_out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string w("msfl_search_poses");
  if (!candidates || !n_out) return fail(h, MSFL_BAD_ARG, w + ": null candidates or n_out");
  msfl_search_geom gm;
  s = search_check(h, w, corner, n_corner, surf, n_surf, guess, cfg, capacity, mem, &gm); if (s) return s;
  hipStream_t st = h->stream;
  const float4 *d_corner, *d_surf;
  s = stage_in(h, h->se.corner, corner, (size_t)n_corner, mem, st, &d_corner); if (s) return s;
  s = stage_in(h, h->se.surf, surf, (size_t)n_surf, mem, st, &d_surf); if (s) return s;
  const bool dev = mem == MSFL_MEM_DEVICE;
  int* d_hits = nullptr;
  s = search_run(h, d_corner, n_corner, d_surf, n_surf, guess, cfg, gm, capacity, dev ? n_out : nullptr, dev ? hits_out : nullptr, &d_hits); if (s) return s;
  if (dev) {
    // the records the select kernel left in scratch go to the caller's array on the stream (all `capacity` slots: the kernel
    // zeroed those past *n_out)
    HIPCHK(h, hipMemcpyAsync(candidates, h->se.cand.p, (size_t)capacity * sizeof(SearchCand), hipMemcpyDeviceToDevice, st));
    return MSFL_OK;
  }
  HIPCHK(h, h->readback.reserve(2 * sizeof(int)));
  HIPCHK(h, hipMemcpyAsync(h->readback.p, h->se.ctr.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (hits_out) HIPCHK(h, hipMemcpyAsync(hits_out, d_hits, 2 * (size_t)gm.n_hypotheses * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  const int n = h->readback.as<int>()[1];
  if (n > 0) HIPCHK(h, hipMemcpy(candidates, h->se.cand.p, (size_t)n * sizeof(SearchCand), hipMemcpyDeviceToHost));
  *n_out = n;
  return MSFL_OK;
}

msfl_status msfl_relocalize(msfl_handle* h, const msfl_point* corner, int n_corner, const msfl_point* surf, int n_surf, const double guess[7],
                            const msfl_search_config* cfg, int n_candidates, double max_dist, int n_refine, double min_fitness,
                            msfl_reloc_result* results, int capacity, int* n_out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string w("msfl_relocalize");
  if (!results || !n_out) return fail(h, MSFL_BAD_ARG, w + ": null results or n_out");
  if (n_candidates < 1 || n_candidates > kSearchMaxK || n_refine < 1 || n_refine > n_candidates || capacity < n_refine || std::isnan(min_fitness))
    return fail(h, MSFL_BAD_ARG, w + ": n_candidates must be 1 .. 1024, n_refine 1 .. n_candidates, capacity >= n_refine, min_fitness a number");
  if (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE) return fail(h, MSFL_BAD_ARG, w + ": unknown memory kind");
  *n_out = 0;
  const bool dev = mem == MSFL_MEM_DEVICE;
  const int F = n_corner + n_surf;
  // 1. the candidates (device clouds: into device scratch of this call, then read back)
  std::vector<msfl_pose_candidate> cand((size_t)n_candidates);
  int n_cand = 0;
  if (dev) {
    HIPCHK(h, h->se.rl_cand.reserve((size_t)n_candidates * sizeof(SearchCand) + sizeof(int)));
    int* d_n = reinterpret_cast<int*>(h->se.rl_cand.as<SearchCand>() + n_candidates);
    s = msfl_search_poses(h, corner, n_corner, surf, n_surf, guess, cfg, h->se.rl_cand.as<msfl_pose_candidate>(), n_candidates, d_n, nullptr, mem); if (s) return s;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&n_cand, d_n, sizeof(int), hipMemcpyDeviceToHost));
    if (n_cand > 0) HIPCHK(h, hipMemcpy(cand.data(), h->se.rl_cand.p, (size_t)n_cand * sizeof(SearchCand), hipMemcpyDeviceToHost));
  } else {
    s = msfl_search_poses(h, corner, n_corner, surf, n_surf, guess, cfg, cand.data(), n_candidates, &n_cand, nullptr, mem); if (s) return s;
  }
  if (n_cand == 0) return MSFL_OK;
  // the scoring and the registration take their poses, scores and status where the clouds are
  auto score = [&](const std::vector<double>& poses, int n, std::vector<msfl_pose_score>* sc) -> msfl_status {
    sc->resize((size_t)n);
    if (!dev) return msfl_score_poses(h, corner, n_corner, surf, n_surf, poses.data(), n, max_dist, sc->data(), nullptr, nullptr, mem);
    HIPCHK(h, h->se.rl_poses.reserve((size_t)n * 7 * sizeof(double)));
    HIPCHK(h, h->se.rl_scores.reserve((size_t)n * sizeof(msfl_pose_score)));
    HIPCHK(h, hipMemcpyAsync(h->se.rl_poses.p, poses.data(), (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));               // (the source is pageable)
    const msfl_status r = msfl_score_poses(h, corner, n_corner, surf, n_surf, h->se.rl_poses.as<double>(), n, max_dist, h->se.rl_scores.as<msfl_pose_score>(),
                                           nullptr, nullptr, mem);
    if (r) return r;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(sc->data(), h->se.rl_scores.p, (size_t)n * sizeof(msfl_pose_score), hipMemcpyDeviceToHost));
    return MSFL_OK;
  };
  // 2. exact scores of the candidates, and their order
  std::vector<double> poses((size_t)n_cand * 7);
  for (int i = 0; i < n_cand; i++) std::memcpy(&poses[7 * (size_t)i], cand[i].pose, 7 * sizeof(double));
  std::vector<msfl_pose_score> coarse;
  s = score(poses, n_cand, &coarse); if (s) return s;
  std::vector<int> order;
  score_order(coarse, &order);
  // 3. the registration of the best few, every one a scan of its own in one batch
  const int R = std::min(n_refine, n_cand);
  std::vector<double> refined((size_t)R * 7);
  std::vector<int> co((size_t)R + 1), so((size_t)R + 1), status((size_t)R, 0);
  for (int r = 0; r <= R; r++) { co[r] = r * n_corner; so[r] = r * n_surf; }
  for (int r = 0; r < R; r++) std::memcpy(&refined[7 * (size_t)r], cand[order[r]].pose, 7 * sizeof(double));
  if (!dev) {
    std::vector<msfl_point> tc((size_t)R * n_corner), ts((size_t)R * n_surf);
    for (int r = 0; r < R; r++) {
      if (n_corner) std::memcpy(&tc[(size_t)r * n_corner], corner, (size_t)n_corner * sizeof(msfl_point));
      if (n_surf) std::memcpy(&ts[(size_t)r * n_surf], surf, (size_t)n_surf * sizeof(msfl_point));
    }
    s = msfl_match_scan2map_batch(h, R, tc.data(), co.data(), ts.data(), so.data(), refined.data(), status.data(), nullptr, mem); if (s) return s;
  } else {
    hipStream_t st = h->stream;
    HIPCHK(h, h->se.rl_corner.reserve(std::max<size_t>(1, (size_t)R * n_corner) * sizeof(msfl_point)));
    HIPCHK(h, h->se.rl_surf.reserve(std::max<size_t>(1, (size_t)R * n_surf) * sizeof(msfl_point)));
    HIPCHK(h, h->se.rl_poses.reserve((size_t)R * 7 * sizeof(double)));
    HIPCHK(h, h->se.rl_status.reserve((size_t)R * sizeof(int)));
    for (int r = 0; r < R; r++) {
      if (n_corner) HIPCHK(h, hipMemcpyAsync(h->se.rl_corner.as<msfl_point>() + (size_t)r * n_corner, corner, (size_t)n_corner * sizeof(msfl_point), hipMemcpyDeviceToDevice, st));
      if (n_surf) HIPCHK(h, hipMemcpyAsync(h->se.rl_surf.as<msfl_point>() + (size_t)r * n_surf, surf, (size_t)n_surf * sizeof(msfl_point), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(h, hipMemcpyAsync(h->se.rl_poses.p, refined.data(), (size_t)R * 7 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));
    s = msfl_match_scan2map_batch(h, R, h->se.rl_corner.as<msfl_point>(), co.data(), h->se.rl_surf.as<msfl_point>(), so.data(), h->se.rl_poses.as<double>(),
                                  h->se.rl_status.as<int>(), nullptr, mem);
    if (s) return s;
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipMemcpy(refined.data(), h->se.rl_poses.p, (size_t)R * 7 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(status.data(), h->se.rl_status.p, (size_t)R * sizeof(int), hipMemcpyDeviceToHost));
  }
  // 4. exact scores of the refined poses, and the records in their order
  std::vector<msfl_pose_score> fine;
  s = score(refined, R, &fine); if (s) return s;
  std::vector<int> order2;
  score_order(fine, &order2);
  for (int i = 0; i < R; i++) {
    const int r = order2[i];
    msfl_reloc_result o;
    std::memset(&o, 0, sizeof(o));
    std::memcpy(o.pose, &refined[7 * (size_t)r], 7 * sizeof(double));
    o.candidate = cand[order[r]];
    o.coarse = coarse[order[r]];
    o.refined = fine[r];
    o.status = status[r];
    o.accepted = F > 0 && (double)score_inliers(fine[r]) / (double)F >= min_fitness ? 1 : 0;
    results[i] = o;
  }
  *n_out = R;
  return MSFL_OK;
}

msfl_status msfl_search_pairs(msfl_handle* h, int n_pairs, const msfl_point* corner, const int* corner_off, const msfl_point* surf, const int* surf_off,
                              const double* guesses, const msfl_search_config* cfg, msfl_pose_candidate* candidates, int capacity, int* n_out,
                              int* hits_out, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  const std::string w("msfl_search_pairs");
  const int P = n_pairs;
  // 1. the arguments
  if (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE) return fail(h, MSFL_BAD_ARG, w + ": unknown memory kind");
  if (P < 0 || (P > 0 && (!corner_off || !surf_off || !guesses || !cfg || !candidates || !n_out))) return fail(h, MSFL_BAD_ARG, w + ": negative count or null argument");
  if (capacity < 1 || capacity > kSearchMaxK) return fail(h, MSFL_BAD_ARG, w + ": the candidate capacity must be 1 .. 1024");
  std::vector<int> co((size_t)P + 1, 0), so((size_t)P + 1, 0);
  if (P > 0) {
    const int c0 = corner_off[0], s0 = surf_off[0];
    if (c0 < 0 || s0 < 0) return fail(h, MSFL_BAD_ARG, w + ": negative offset");
    for (int p = 0; p <= P; p++) {
      co[p] = corner_off[p] - c0; so[p] = surf_off[p] - s0;
      if (p > 0 && (co[p] < co[p - 1] || so[p] < so[p - 1])) return fail(h, MSFL_BAD_ARG, w + ": offset arrays must be non-decreasing");
    }
    if ((co[P] > 0 && !corner) || (so[P] > 0 && !surf)) return fail(h, MSFL_BAD_ARG, w + ": null cloud");
  }
  // 2. the geometry rule, pair by pair (with one cfg the results differ in origin only)
  std::vector<msfl_search_geom> gms((size_t)P);
  for (int p = 0; p < P; p++) {
    std::string why;
    s = search_geometry(guesses + 7 * (size_t)p, cfg, co[p + 1] - co[p], so[p + 1] - so[p], &gms[p], &why);
    if (s) return fail(h, s, w + ": pair " + std::to_string(p) + ": " + why);
  }
  // 3. the pair index
  s = pairs_resident(h, w, P); if (s) return s;
  if (P == 0) return MSFL_OK;
  hipStream_t st = h->stream;
  const bool dev = mem == MSFL_MEM_DEVICE;
  // (both memory kinds read from the first used element on: the offsets are relative to it)
  const float4 *d_corner, *d_surf;
  s = stage_in(h, h->se.corner, co[P] ? corner + corner_off[0] : corner, (size_t)co[P], mem, st, &d_corner); if (s) return s;
  s = stage_in(h, h->se.surf, so[P] ? surf + surf_off[0] : surf, (size_t)so[P], mem, st, &d_surf); if (s) return s;
  s = search_pairs_run(h, P, d_corner, co.data(), d_surf, so.data(), guesses, cfg, gms, capacity, candidates, n_out, hits_out, dev); if (s) return s;
  // host clouds were staged with asynchronous copies from pageable memory; every chunk was waited for
  return MSFL_OK;
}

}  // extern "C"
