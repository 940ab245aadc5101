// N1: device-resident local map store (HybridGrid) — C-ABI entry points and the stream-ordered building blocks the
// per-scan SLAM step (msfl_api_slam.inc) chains.  Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing
// and helper macros).  Layout and algorithm: msfl_grid.cuh.

struct msfl_grid_s {
  msfl_handle* h = nullptr;
  GridStoreDesc d{};
  DevBuf state;                                   // GridState
  DevBuf pool[2];                                 // point pool (float4), the live one is pool[cur_pool]
  int cur_pool = 0;
  DevBuf ckey[2], cstart[2], ccnt[2], cstamp[2];  // cell table, ping-pong per insert
  int cur_tab = 0;
  int cell_cap = 0;                               // entries every table buffer holds
  // insert scratch (sized by the largest scan seen)
  DevBuf keys, keys_s, vals, vals_s, head, tpos, xf, xs, t_key, t_ns, t_old, t_woff, t_rank, t_cnt;
  // surround / dump scratch
  DevBuf cnt, off, stage, pose, report_dev;
  DevBuf crop;                                    // crop scratch: keep flag and rank per cell (cnt / off hold the evicted counts and offsets)
  DevBuf crop_cells;                              // msfl_grid_crop_tiles: {ix, iy, iz, count} of the evicted cells
  DevBuf load;                                    // load scratch: the staged cell list, then key, position, conflict flag, count and slab offset per listed cell
  // carve scratch, allocated by the first msfl_grid_carve: the range and limit images, keep flag / rank / removed count / offset per
  // cell, the bisection tables of carve_cfg (rebuilt when the configuration changes), the counters of the call in flight
  DevBuf carve_img, carve_cells, carve_tab, carve_ctr;
  msfl_carve_config carve_cfg{};
  bool carve_tab_valid = false;
  PinBuf report;                                  // int[8] read-back: {points, cells, pool_top, bad, overflow, touched, work, surround_total}, then the int[8] crop info
  // What the host knows: exact sizes as of the newest insert whose report it has seen, plus the inserts enqueued since
  // (sequence number, point capacity).  Every launch bound and capacity decision derives from these upper bounds, so
  // inserts and queries can be enqueued without waiting for the ones before them.
  int n_points = 0, n_cells = 0, pool_top = 0;
  long long ub_points = 0, ub_cells = 0, ub_top = 0;
  std::vector<std::pair<long long, int>> inflight;
  long long next_seq = 1, last_seq = 0, top_valid_from = 0;   // reports of inserts before top_valid_from carry a pool top from before a compaction
  bool pending = false;                           // the newest insert went to the grid's own report buffer and has not been read
  long long min_pool = 1 << 20;                   // smallest point pool (16 MB); MSFL_GRID_MIN_POOL overrides it (tests: forces frequent compaction)
};

namespace {

constexpr int kGridMinCells = 1 << 16;

size_t pool_capacity(const msfl_grid* g) { return g->pool[g->cur_pool].cap / sizeof(float4); }
// pool slots one insert can take at most: every live point touched, every cell beyond the LDS capacity (+ 50 % sort scratch)
long long grid_work_bound(long long points_before, int n_cap) { return (points_before + n_cap) + (points_before + n_cap) / 2 + 64; }

// a buffer that must keep its first `keep` bytes when it grows
msfl_status grow_keep(msfl_handle* h, DevBuf& b, size_t bytes, size_t keep) {
  if (bytes <= b.cap) return MSFL_OK;
  DevBuf nb;
  HIPCHK(h, nb.reserve(std::max(bytes, b.cap + b.cap / 2)));
  if (b.p && keep) HIPCHK(h, hipMemcpyAsync(nb.p, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  b = std::move(nb);
  return MSFL_OK;
}

msfl_status grid_init_state(msfl_grid* g) {
  msfl_handle* h = g->h;
  HIPCHK(h, g->state.reserve(sizeof(GridState)));
  GridState init{};
  init.epoch = 1;
  HIPCHK(h, h->pin.upload(g->state.p, &init, sizeof(init), h->stream));
  HIPCHK(h, g->report_dev.reserve(16 * sizeof(int)));
  HIPCHK(h, g->report.reserve(16 * sizeof(int)));
  std::memset(g->report.p, 0, 16 * sizeof(int));
  return MSFL_OK;
}

// the live cells back to back into `out` (device, `capacity` points), table order.  into_pool: `out` is the other pool
// buffer, the table's starts are rewritten and the pool top drops to the live count.
msfl_status grid_pack(msfl_grid* g, float4* out, long long capacity, bool into_pool) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  const int bound = (int)std::min<long long>(g->ub_cells, g->cell_cap);
  if (bound <= 0) return MSFL_OK;
  GridState* gs = g->state.as<GridState>();
  int* cnt = g->ccnt[g->cur_tab].as<int>();
  HIPCHK(h, g->off.reserve((size_t)bound * sizeof(int)));
  hipLaunchKernelGGL(grid_zero_tail_kernel, dim3(div_up(bound, 256)), dim3(256), 0, st, cnt, bound, (const GridState*)gs);
  size_t tb = 0;
  HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, cnt, g->off.as<int>(), 0, (size_t)bound, rocprim::plus<int>(), st));
  HIPCHK(h, h->idx_cub.reserve(tb));
  HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, cnt, g->off.as<int>(), 0, (size_t)bound, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(grid_compact_kernel, dim3(std::min(bound, 4096)), dim3(256), 0, st, (const float4*)g->pool[g->cur_pool].as<float4>(),
                     (const int*)g->cstart[g->cur_tab].as<int>(), (const int*)cnt, (const int*)g->off.as<int>(), out,
                     (int)std::min<long long>(capacity, INT32_MAX), (int*)nullptr, bound, gs, into_pool ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  if (into_pool) HIPCHK(h, hipMemcpyAsync(g->cstart[g->cur_tab].p, g->off.p, (size_t)bound * sizeof(int), hipMemcpyDeviceToDevice, st));
  return MSFL_OK;
}

// Capacity planning from host-known upper bounds only (never a device round trip): room for `add_cells` more table entries and
// `add_pool` more pool slots above the bounds; the pool is compacted into the other buffer (grown if need be) when they do not fit.
msfl_status grid_reserve(msfl_grid* g, long long add_cells, long long add_pool) {
  msfl_handle* h = g->h;
  const long long need_cells = g->ub_cells + add_cells;
  if (need_cells > g->cell_cap) {
    const long long want = std::max<long long>(std::max<long long>(need_cells + need_cells / 2, kGridMinCells), 2LL * g->cell_cap);
    if (want > (1LL << 30)) return fail(h, MSFL_CAPACITY, "msfl_grid: cell table beyond 2^30 entries");
    for (int k = 0; k < 2; k++) {
      msfl_status s;
      if ((s = grow_keep(h, g->ckey[k], (size_t)want * sizeof(unsigned long long), (size_t)g->cell_cap * sizeof(unsigned long long)))) return s;
      if ((s = grow_keep(h, g->cstart[k], (size_t)want * sizeof(int), (size_t)g->cell_cap * sizeof(int)))) return s;
      if ((s = grow_keep(h, g->ccnt[k], (size_t)want * sizeof(int), (size_t)g->cell_cap * sizeof(int)))) return s;
      if ((s = grow_keep(h, g->cstamp[k], (size_t)want * sizeof(int), (size_t)g->cell_cap * sizeof(int)))) return s;
    }
    g->cell_cap = (int)want;
  }
  const long long work = add_pool;
  if (g->ub_top + work > (long long)pool_capacity(g)) {
    // compact into the other buffer (grown if the live points plus one worst-case insert would not leave it half empty)
    const long long want = std::max<long long>(std::max<long long>(2 * (g->ub_points + work), g->min_pool), (long long)pool_capacity(g));
    if (want * (long long)sizeof(float4) > (64LL << 30)) return fail(h, MSFL_CAPACITY, "msfl_grid: point pool beyond 64 GB");
    DevBuf& other = g->pool[1 - g->cur_pool];
    if ((size_t)want * sizeof(float4) > other.cap) {
      HIPCHK(h, hipStreamSynchronize(h->stream));            // the buffer may still be read by queued work
      other.release();
      HIPCHK(h, other.reserve((size_t)want * sizeof(float4)));
    }
    if (g->ub_points > 0) { msfl_status s = grid_pack(g, other.as<float4>(), (long long)(other.cap / sizeof(float4)), true); if (s) return s; }
    else HIPCHK(h, hipMemsetAsync(&g->state.as<GridState>()->pool_top, 0, sizeof(int), h->stream));
    g->cur_pool = 1 - g->cur_pool;
    g->ub_top = g->ub_points;
    g->top_valid_from = g->next_seq;
  }
  return MSFL_OK;
}

// before an insert of up to n_cap points: the cell tables take every new point as a new cell, the pool takes every live point as
// touched and every cell as large
msfl_status grid_reserve_for_insert(msfl_grid* g, int n_cap) { return grid_reserve(g, n_cap, grid_work_bound(g->ub_points, n_cap)); }

// Stream-ordered InsertScan: `d_pts` (device, up to n_cap points, the first *n_dev of them valid when n_dev != null) ->
// optional rigid transform by the device pose `d_pose` -> merged into the touched cells.  No host synchronisation; the
// outcome is published to the pinned report by the copy enqueued at the end (grid_read_report after a synchronisation).
// report_dst: device int[8] that receives the report (the SLAM step's result record); null = the grid's own buffer, copied
// to its pinned mirror.
msfl_status grid_insert_enqueue(msfl_grid* g, const float4* d_pts, int n_cap, const int* n_dev, const double* d_pose, int* report_dst = nullptr) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  if (n_cap <= 0) return MSFL_OK;
  msfl_status s = grid_reserve_for_insert(g, n_cap); if (s) return s;
  const size_t n = (size_t)n_cap;
  HIPCHK(h, g->keys.reserve(n * sizeof(unsigned long long)));
  HIPCHK(h, g->keys_s.reserve(n * sizeof(unsigned long long)));
  HIPCHK(h, g->vals.reserve(n * sizeof(int)));
  HIPCHK(h, g->vals_s.reserve(n * sizeof(int)));
  HIPCHK(h, g->xs.reserve(n * sizeof(float4)));
  HIPCHK(h, g->head.reserve(n * sizeof(int)));
  HIPCHK(h, g->tpos.reserve(n * sizeof(int)));
  HIPCHK(h, g->t_key.reserve((n + 1) * sizeof(unsigned long long)));
  for (DevBuf* b : {&g->t_ns, &g->t_old, &g->t_woff, &g->t_rank, &g->t_cnt}) HIPCHK(h, b->reserve((n + 1) * sizeof(int)));
  const float4* xf = d_pts;
  if (d_pose) { HIPCHK(h, g->xf.reserve(n * sizeof(float4))); xf = g->xf.as<float4>(); }
  GridState* gs = g->state.as<GridState>();
  const int cur = g->cur_tab, nxt = 1 - cur;
  const dim3 grid(div_up(n_cap, 256)), block(256);
  if (n_cap <= kGridSortSmall) {
    // a short list (the corner side of a scan): keys and their stable sort in one workgroup
    hipLaunchKernelGGL(grid_key_sort_small_kernel, dim3(1), dim3(1024), 0, st, d_pts, n_cap, n_dev, d_pose, g->xf.as<float4>(), g->d,
                       g->keys_s.as<unsigned long long>(), g->vals_s.as<int>(), g->xs.as<float4>(), gs);
  } else {
    hipLaunchKernelGGL(grid_key_kernel, grid, block, 0, st, d_pts, n_cap, n_dev, d_pose, g->xf.as<float4>(), g->d,
                       g->keys.as<unsigned long long>(), g->vals.as<int>(), gs);
    size_t tb = 0;
    const unsigned key_bits = 64;                                        // the bad key (padding, out-of-range points) is all ones
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, g->keys.as<unsigned long long>(), g->keys_s.as<unsigned long long>(), g->vals.as<int>(),
                                        g->vals_s.as<int>(), n, 0u, key_bits, st));
    HIPCHK(h, h->idx_cub.reserve(tb));
    HIPCHK(h, rocprim::radix_sort_pairs(h->idx_cub.p, tb, g->keys.as<unsigned long long>(), g->keys_s.as<unsigned long long>(), g->vals.as<int>(),
                                        g->vals_s.as<int>(), n, 0u, key_bits, st));
    hipLaunchKernelGGL(grid_gather_sorted_kernel, grid, block, 0, st, xf, (const int*)g->vals_s.as<int>(), n_cap, n_dev, g->xs.as<float4>());
  }
  if (n_cap <= kGridTouchOneBlockMax) {
    hipLaunchKernelGGL(grid_touch_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long*)g->keys_s.as<unsigned long long>(), n_cap, n_dev,
                       g->t_key.as<unsigned long long>(), g->t_ns.as<int>(), gs);
  } else {
    hipLaunchKernelGGL(grid_touch_flag_kernel, grid, block, 0, st, (const unsigned long long*)g->keys_s.as<unsigned long long>(), n_cap, n_dev,
                       g->head.as<int>());
    size_t tb2 = 0;
    HIPCHK(h, rocprim::inclusive_scan(nullptr, tb2, g->head.as<int>(), g->tpos.as<int>(), n, rocprim::plus<int>(), st));
    HIPCHK(h, h->idx_cub.reserve(tb2));
    HIPCHK(h, rocprim::inclusive_scan(h->idx_cub.p, tb2, g->head.as<int>(), g->tpos.as<int>(), n, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(grid_touch_list_kernel, grid, block, 0, st, (const unsigned long long*)g->keys_s.as<unsigned long long>(),
                       (const int*)g->head.as<int>(), (const int*)g->tpos.as<int>(), n_cap, n_dev, g->t_key.as<unsigned long long>(),
                       g->t_ns.as<int>(), gs);
  }
  hipLaunchKernelGGL(grid_plan_kernel, dim3(1), dim3(1024), 0, st, (const unsigned long long*)g->ckey[cur].as<unsigned long long>(),
                     (const int*)g->ccnt[cur].as<int>(), (const unsigned long long*)g->t_key.as<unsigned long long>(), (const int*)g->t_ns.as<int>(),
                     g->t_old.as<int>(), g->t_woff.as<int>(), g->t_rank.as<int>(), (int)std::min<size_t>(pool_capacity(g), INT32_MAX), g->cell_cap, gs);
  float4* pool = g->pool[g->cur_pool].as<float4>();
  const int small_blocks = std::min(n_cap, 2048), large_blocks = std::min(n_cap, 256);
  const float4* xs = g->xs.as<float4>();
  hipLaunchKernelGGL((grid_rebuild_kernel<kGridSmallThreads, kGridSmallCap, false>), dim3(small_blocks), dim3(kGridSmallThreads), 0, st, (const float4*)pool, pool,
                     (const int*)g->cstart[cur].as<int>(), (const int*)g->ccnt[cur].as<int>(), xs,
                     (const unsigned long long*)g->keys_s.as<unsigned long long>(),
                     (const unsigned long long*)g->t_key.as<unsigned long long>(), (const int*)g->t_ns.as<int>(), (const int*)g->t_old.as<int>(),
                     (const int*)g->t_woff.as<int>(), g->t_cnt.as<int>(), g->d, gs);
  hipLaunchKernelGGL((grid_rebuild_kernel<1024, kGridLargeCap, true>), dim3(large_blocks), dim3(1024), 0, st, (const float4*)pool, pool,
                     (const int*)g->cstart[cur].as<int>(), (const int*)g->ccnt[cur].as<int>(), xs,
                     (const unsigned long long*)g->keys_s.as<unsigned long long>(),
                     (const unsigned long long*)g->t_key.as<unsigned long long>(), (const int*)g->t_ns.as<int>(), (const int*)g->t_old.as<int>(),
                     (const int*)g->t_woff.as<int>(), g->t_cnt.as<int>(), g->d, gs);
  const int bound = (int)std::min<long long>(g->ub_cells + n_cap, g->cell_cap);
  hipLaunchKernelGGL(grid_commit_kernel, dim3(div_up(bound, 256)), dim3(256), 0, st, (const unsigned long long*)g->ckey[cur].as<unsigned long long>(),
                     (const int*)g->cstart[cur].as<int>(), (const int*)g->ccnt[cur].as<int>(), (const int*)g->cstamp[cur].as<int>(),
                     g->ckey[nxt].as<unsigned long long>(), g->cstart[nxt].as<int>(), g->ccnt[nxt].as<int>(), g->cstamp[nxt].as<int>(),
                     (const unsigned long long*)g->t_key.as<unsigned long long>(), (const int*)g->t_old.as<int>(), (const int*)g->t_woff.as<int>(),
                     (const int*)g->t_rank.as<int>(), (const int*)g->t_cnt.as<int>(), bound, (const GridState*)gs);
  hipLaunchKernelGGL(grid_finish_kernel, dim3(1), dim3(1), 0, st, gs, report_dst ? report_dst : g->report_dev.as<int>());
  HIPCHK(h, hipGetLastError());
  if (!report_dst) { HIPCHK(h, hipMemcpyAsync(g->report.p, g->report_dev.p, 8 * sizeof(int), hipMemcpyDeviceToHost, st)); g->pending = true; }
  g->cur_tab = nxt;
  g->ub_top += grid_work_bound(g->ub_points, n_cap);
  g->ub_points += n_cap;
  g->ub_cells += n_cap;
  g->last_seq = g->next_seq++;
  g->inflight.emplace_back(g->last_seq, n_cap);
  return MSFL_OK;
}

// The report of insert `seq` has reached the host (its stream position has been synchronised with): exact sizes as of
// that insert, the bounds of the inserts enqueued after it on top.  MSFL_CAPACITY when that insert was dropped.
msfl_status grid_apply_report(msfl_grid* g, const int* r, long long seq) {
  while (!g->inflight.empty() && g->inflight.front().first <= seq) g->inflight.erase(g->inflight.begin());
  g->n_points = r[0]; g->n_cells = r[1];
  long long pts = r[0], cells = r[1], top = seq >= g->top_valid_from ? (long long)r[2] : -1;
  if (top >= 0) g->pool_top = r[2];
  for (auto& f : g->inflight) { if (top >= 0) top += grid_work_bound(pts, f.second); pts += f.second; cells += f.second; }
  g->ub_points = pts; g->ub_cells = cells;
  if (top >= 0) g->ub_top = top;
  if (r[3]) return fail(g->h, MSFL_CAPACITY, "msfl_grid_insert_scan: a point falls outside +-8192 cells (hybrid_grid.cc:460) or is not finite; map unchanged");
  if (r[4]) return fail(g->h, MSFL_CAPACITY, "msfl_grid_insert_scan: internal capacity exceeded; map unchanged");
  return MSFL_OK;
}

// after a synchronisation of the stream: take the report of the newest insert from the grid's own buffer
msfl_status grid_read_report(msfl_grid* g) {
  if (!g->pending) return MSFL_OK;
  g->pending = false;
  return grid_apply_report(g, g->report.as<int>(), g->last_seq);
}

// Stream-ordered crop to the window of +-half cells around the cell of the device-resident `d_center` (3 doubles).  d_evicted:
// device buffer of `capacity` points for the evicted points, or null (dropped).  d_ev_cells: device buffer for {ix, iy, iz, count} of
// the evicted cells (min(cell_capacity, live cells) x 4 ints), or null.  info_dst: device int[8] (msfl_grid_crop_info).
// report_dst as in grid_insert_enqueue; with sizes_only only its first three words are rewritten (the SLAM step's record keeps
// what the insert before the crop published in the others).  Takes a sequence number like an insert of zero points: the bounds
// come down when the report is applied.
msfl_status grid_crop_enqueue(msfl_grid* g, const double* d_center, const int half[3], float4* d_evicted, int capacity, int* info_dst,
                              int* report_dst = nullptr, bool sizes_only = false, int* d_ev_cells = nullptr, int cell_capacity = 0) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  GridState* gs = g->state.as<GridState>();
  const int bound = (int)std::min<long long>(g->ub_cells, g->cell_cap);
  const GridWindow w{half[0], half[1], half[2]};
  int *keep = nullptr, *rank = nullptr, *ecnt = nullptr, *eoff = nullptr;
  if (bound > 0) {
    const int cur = g->cur_tab, nxt = 1 - cur;
    HIPCHK(h, g->crop.reserve(2 * (size_t)bound * sizeof(int)));
    HIPCHK(h, g->cnt.reserve((size_t)bound * sizeof(int)));
    HIPCHK(h, g->off.reserve((size_t)bound * sizeof(int)));
    keep = g->crop.as<int>(); rank = keep + bound; ecnt = g->cnt.as<int>(); eoff = g->off.as<int>();
    const unsigned long long* keys = g->ckey[cur].as<unsigned long long>();
    const int* ccnt = g->ccnt[cur].as<int>();
    if (bound <= kGridOneBlockMax) {
      hipLaunchKernelGGL(grid_crop_scan_kernel, dim3(1), dim3(1024), 0, st, keys, ccnt, bound, d_center, g->d.resolution, w, keep, rank, ecnt, eoff,
                         (const GridState*)gs);
    } else {
      hipLaunchKernelGGL(grid_crop_flag_kernel, dim3(div_up(bound, 256)), dim3(256), 0, st, keys, ccnt, bound, d_center, g->d.resolution, w, keep, ecnt,
                         (const GridState*)gs);
      size_t tb = 0;
      HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, keep, rank, 0, (size_t)bound, rocprim::plus<int>(), st));
      HIPCHK(h, h->idx_cub.reserve(tb));
      HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, keep, rank, 0, (size_t)bound, rocprim::plus<int>(), st));
      HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, ecnt, eoff, 0, (size_t)bound, rocprim::plus<int>(), st));
    }
    hipLaunchKernelGGL(grid_crop_commit_kernel, dim3(std::min(bound, 4096)), dim3(256), 0, st, keys, (const int*)g->cstart[cur].as<int>(), ccnt,
                       (const int*)g->cstamp[cur].as<int>(), g->ckey[nxt].as<unsigned long long>(), g->cstart[nxt].as<int>(), g->ccnt[nxt].as<int>(),
                       g->cstamp[nxt].as<int>(), (const float4*)g->pool[g->cur_pool].as<float4>(), (const int*)keep, (const int*)rank, (const int*)ecnt,
                       (const int*)eoff, bound, d_evicted, capacity, d_ev_cells, cell_capacity, (const GridState*)gs);
    g->cur_tab = nxt;
  }
  hipLaunchKernelGGL(grid_crop_finish_kernel, dim3(1), dim3(1), 0, st, gs, (const int*)keep, (const int*)rank, (const int*)ecnt, (const int*)eoff, bound, d_center,
                     g->d.resolution, d_evicted ? 1 : 0, capacity, d_ev_cells ? 1 : 0, cell_capacity, info_dst,
                     report_dst ? report_dst : g->report_dev.as<int>(), sizes_only ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  if (!report_dst) { HIPCHK(h, hipMemcpyAsync(g->report.p, g->report_dev.p, 16 * sizeof(int), hipMemcpyDeviceToHost, st)); g->pending = true; }
  g->last_seq = g->next_seq++;
  g->inflight.emplace_back(g->last_seq, 0);
  return MSFL_OK;
}

// Stream-ordered load of `n_cells` listed cells with `n_points` points (both exact: the host validated the list).  d_cells: the
// staged list at the head of g->load; d_pts: the points on the device.  info_dst: device int[8] (msfl_grid_load_info).  Takes a
// sequence number like an insert; the bounds rise by the exact sizes and come down again with the report when the load was refused.
msfl_status grid_load_enqueue(msfl_grid* g, const int* d_cells, int n_cells, const float4* d_pts, int n_points, int* info_dst, int* report_dst = nullptr) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  msfl_status s = grid_reserve(g, n_cells, n_points); if (s) return s;
  GridState* gs = g->state.as<GridState>();
  const int cur = g->cur_tab, nxt = 1 - cur;
  const size_t n = (size_t)n_cells;
  // scratch behind the staged list (16 bytes per cell): key (8), position, conflict flag, count, offset (4 each)
  unsigned long long* lkey = reinterpret_cast<unsigned long long*>(g->load.as<char>() + 16 * n);
  int* lpos = reinterpret_cast<int*>(lkey + n);
  int *lconf = lpos + n, *lcnt = lconf + n, *loff = lcnt + n;
  const unsigned long long* keys = g->ckey[cur].as<unsigned long long>();
  const int pool_cap = (int)std::min<size_t>(pool_capacity(g), INT32_MAX);
  if (n_cells <= kGridOneBlockMax) {
    hipLaunchKernelGGL(grid_load_plan_kernel, dim3(1), dim3(1024), 0, st, d_cells, n_cells, keys, lkey, lpos, lconf, loff, gs);
  } else {
    hipLaunchKernelGGL(grid_load_flag_kernel, dim3(div_up(n_cells, 256)), dim3(256), 0, st, d_cells, n_cells, keys, lkey, lpos, lconf, lcnt, gs);
    size_t tb = 0;
    HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, lcnt, loff, 0, n, rocprim::plus<int>(), st));
    HIPCHK(h, h->idx_cub.reserve(tb));
    HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, lcnt, loff, 0, n, rocprim::plus<int>(), st));
  }
  hipLaunchKernelGGL(grid_load_copy_kernel, dim3(div_up(n_points, 256)), dim3(256), 0, st, d_pts, n_points, g->pool[g->cur_pool].as<float4>(), pool_cap, gs);
  const int bound = (int)std::min<long long>(g->ub_cells + n_cells, g->cell_cap);
  hipLaunchKernelGGL(grid_load_commit_kernel, dim3(div_up(bound, 256)), dim3(256), 0, st, keys, (const int*)g->cstart[cur].as<int>(),
                     (const int*)g->ccnt[cur].as<int>(), (const int*)g->cstamp[cur].as<int>(), g->ckey[nxt].as<unsigned long long>(),
                     g->cstart[nxt].as<int>(), g->ccnt[nxt].as<int>(), g->cstamp[nxt].as<int>(), d_cells, (const unsigned long long*)lkey,
                     (const int*)lpos, (const int*)loff, n_cells, n_points, bound, pool_cap, g->cell_cap, (const GridState*)gs);
  hipLaunchKernelGGL(grid_load_finish_kernel, dim3(1), dim3(1), 0, st, gs, n_cells, n_points, pool_cap, g->cell_cap, info_dst,
                     report_dst ? report_dst : g->report_dev.as<int>());
  HIPCHK(h, hipGetLastError());
  if (!report_dst) { HIPCHK(h, hipMemcpyAsync(g->report.p, g->report_dev.p, 16 * sizeof(int), hipMemcpyDeviceToHost, st)); g->pending = true; }
  g->cur_tab = nxt;
  g->ub_top += n_points;
  g->ub_points += n_points;
  g->ub_cells += n_cells;
  g->last_seq = g->next_seq++;
  g->inflight.emplace_back(g->last_seq, 0);
  return MSFL_OK;
}

// Stream-ordered GetSurroundedCloud.  scan = d_scan[idx ? idx[k] : k], k < min(n_cap, *n_dev); pose on the device.
// The cloud goes to d_out (capacity points), its size to *d_n_out (device, optional) and to GridState::surround_total.
msfl_status grid_surround_enqueue(msfl_grid* g, const float4* d_scan, const int* d_idx, int n_cap, const int* n_dev, const double* d_pose,
                                  float4* d_out, int capacity, int* d_n_out) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  GridState* gs = g->state.as<GridState>();
  const int bound = (int)std::min<long long>(g->ub_cells, g->cell_cap);
  if (bound <= 0 || n_cap <= 0) {
    if (d_n_out) HIPCHK(h, hipMemsetAsync(d_n_out, 0, sizeof(int), st));
    HIPCHK(h, hipMemsetAsync(&gs->surround_total, 0, sizeof(int), st));
    return MSFL_OK;
  }
  const int cur = g->cur_tab;
  HIPCHK(h, g->cnt.reserve((size_t)bound * sizeof(int)));
  HIPCHK(h, g->off.reserve((size_t)bound * sizeof(int)));
  hipLaunchKernelGGL(grid_mark_kernel, dim3(div_up(n_cap, 256)), dim3(256), 0, st, d_scan, d_idx, n_cap, n_dev, d_pose, g->d.resolution,
                     (const unsigned long long*)g->ckey[cur].as<unsigned long long>(), g->cstamp[cur].as<int>(), (const GridState*)gs);
  if (bound <= kGridOneBlockMax) {
    hipLaunchKernelGGL(grid_emit_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)g->cstamp[cur].as<int>(), (const int*)g->ccnt[cur].as<int>(),
                       bound, g->cnt.as<int>(), g->off.as<int>(), (const GridState*)gs);
  } else {
    hipLaunchKernelGGL(grid_emit_count_kernel, dim3(div_up(bound, 256)), dim3(256), 0, st, (const int*)g->cstamp[cur].as<int>(),
                       (const int*)g->ccnt[cur].as<int>(), bound, g->cnt.as<int>(), (const GridState*)gs);
    size_t tb = 0;
    HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, g->cnt.as<int>(), g->off.as<int>(), 0, (size_t)bound, rocprim::plus<int>(), st));
    HIPCHK(h, h->idx_cub.reserve(tb));
    HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, g->cnt.as<int>(), g->off.as<int>(), 0, (size_t)bound, rocprim::plus<int>(), st));
  }
  hipLaunchKernelGGL(grid_emit_kernel, dim3(std::min(bound, 4096)), dim3(256), 0, st, (const float4*)g->pool[g->cur_pool].as<float4>(),
                     (const int*)g->cstart[cur].as<int>(), (const int*)g->cnt.as<int>(), (const int*)g->off.as<int>(), bound, capacity, d_out, d_n_out, gs);
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// ---- Carve (msfl_carve.cuh) -----------------------------------------------------------------------------------------------------

bool carve_config_ok(const msfl_carve_config& c) {
  const float f[6] = {c.elev_low_deg, c.elev_high_deg, c.min_range, c.max_range, c.margin_abs, c.margin_rel};
  for (float v : f) if (!std::isfinite(v)) return false;
  return c.n_col >= 2 && c.n_col <= kCarveMaxCol && (c.n_col & 1) == 0 && c.n_row >= 1 && c.n_row <= kCarveMaxRow &&
         c.elev_low_deg > -90.f && c.elev_low_deg < c.elev_high_deg && c.elev_high_deg < 90.f && c.min_range >= 0.f && c.min_range < c.max_range &&
         c.margin_abs >= 0.f && c.margin_rel >= 0.f && c.window_col >= 0 && c.window_col <= kCarveMaxWindow && c.window_row >= 0 &&
         c.window_row <= kCarveMaxWindow;
}

// the tables in double, rounded to f32 (docs/kernels/grid_store.md states the two formulas)
void carve_build_tables(const msfl_carve_config& c, float* cc, float* cs, float* ec, float* es) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < c.n_col / 2; k++) {
    const double a = 2.0 * pi * (double)k / (double)c.n_col;
    cc[k] = (float)std::cos(a); cs[k] = (float)std::sin(a);
  }
  for (int k = 0; k <= c.n_row; k++) {
    const double deg = (double)c.elev_low_deg + ((double)c.elev_high_deg - (double)c.elev_low_deg) * (double)k / (double)c.n_row;
    const double e = deg * pi / 180.0;
    ec[k] = (float)std::cos(e); es[k] = (float)std::sin(e);
  }
}

// Stream-ordered carve with the scan `d_scan` (device, n points, sensor frame) taken at the device-resident `d_pose` (7 doubles).
// d_removed: device buffer of `capacity` points for the removed points, or null (dropped).  info_dst: device int[8]
// (msfl_grid_carve_info).  report_dst as in grid_insert_enqueue.  Takes a sequence number and flips the table parity like a crop:
// the bounds come down when the report is applied.  The pool is not touched: a carved slab's tail is garbage for the next grid_pack.
msfl_status grid_carve_enqueue(msfl_grid* g, const float4* d_scan, int n, const double* d_pose, const msfl_carve_config& cfg, float4* d_removed,
                               int capacity, int* info_dst, int* report_dst = nullptr) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  GridState* gs = g->state.as<GridState>();
  const int npix = cfg.n_col * cfg.n_row, half = cfg.n_col / 2;
  if (!g->carve_ctr.p) {
    HIPCHK(h, g->carve_ctr.reserve(CARVE_CTR_WORDS * sizeof(int)));
    HIPCHK(h, hipMemsetAsync(g->carve_ctr.p, 0, CARVE_CTR_WORDS * sizeof(int), st));
  }
  if (!g->carve_tab_valid || std::memcmp(&g->carve_cfg, &cfg, sizeof(cfg)) != 0) {
    float tab[kCarveMaxTab];
    carve_build_tables(cfg, tab, tab + half, tab + 2 * half, tab + 2 * half + cfg.n_row + 1);
    HIPCHK(h, g->carve_tab.reserve(kCarveMaxTab * sizeof(float)));
    HIPCHK(h, h->pin.upload(g->carve_tab.p, tab, (size_t)carve_tab_size(cfg.n_col, cfg.n_row) * sizeof(float), st));
    g->carve_cfg = cfg; g->carve_tab_valid = true;
  }
  HIPCHK(h, g->carve_img.reserve(2 * (size_t)npix * sizeof(float)));
  unsigned* near_img = g->carve_img.as<unsigned>();
  float* lim = g->carve_img.as<float>() + npix;
  int* ctr = g->carve_ctr.as<int>();
  const CarveCfg c{cfg.n_col, cfg.n_row, cfg.window_col, cfg.window_row, cfg.min_range, cfg.max_range, cfg.margin_abs, cfg.margin_rel,
                   (const float*)g->carve_tab.as<float>()};
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)near_img, (int)kCarveEmpty, (size_t)npix, st));
  if (n > 0) hipLaunchKernelGGL(carve_fill_kernel, dim3(std::min(div_up(n, kCarveBlock), 1024)), dim3(kCarveBlock), 0, st, c, d_scan, n, near_img);
  hipLaunchKernelGGL(carve_limit_kernel, dim3(div_up(npix, kCarveBlock)), dim3(kCarveBlock), 0, st, c, (const unsigned*)near_img, lim, ctr);
  const int bound = (int)std::min<long long>(g->ub_cells, g->cell_cap);
  int *keep = nullptr, *rank = nullptr, *rcnt = nullptr, *roff = nullptr;
  if (bound > 0) {
    const int cur = g->cur_tab, nxt = 1 - cur;
    HIPCHK(h, g->carve_cells.reserve(4 * (size_t)bound * sizeof(int)));
    keep = g->carve_cells.as<int>(); rank = keep + bound; rcnt = rank + bound; roff = rcnt + bound;
    const unsigned long long* keys = g->ckey[cur].as<unsigned long long>();
    const int* cstart = g->cstart[cur].as<int>();
    const int* ccnt = g->ccnt[cur].as<int>();
    float4* pool = g->pool[g->cur_pool].as<float4>();
    hipLaunchKernelGGL(carve_count_kernel, dim3(std::min(bound, 4096)), dim3(kCarveBlock), 0, st, c, d_pose, (const float*)lim, keys, cstart, ccnt,
                       (const float4*)pool, bound, g->d.resolution, keep, rcnt, ctr, (const GridState*)gs);
    if (bound <= kGridOneBlockMax) {
      hipLaunchKernelGGL(carve_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)keep, (const int*)rcnt, bound, rank, roff, (const GridState*)gs);
    } else {
      size_t tb = 0;
      HIPCHK(h, rocprim::exclusive_scan(nullptr, tb, keep, rank, 0, (size_t)bound, rocprim::plus<int>(), st));
      HIPCHK(h, h->idx_cub.reserve(tb));
      HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, keep, rank, 0, (size_t)bound, rocprim::plus<int>(), st));
      HIPCHK(h, rocprim::exclusive_scan(h->idx_cub.p, tb, rcnt, roff, 0, (size_t)bound, rocprim::plus<int>(), st));
    }
    hipLaunchKernelGGL(carve_apply_kernel, dim3(std::min(bound, 4096)), dim3(kCarveBlock), 0, st, c, d_pose, (const float*)lim, keys, cstart, ccnt,
                       (const int*)g->cstamp[cur].as<int>(), g->ckey[nxt].as<unsigned long long>(), g->cstart[nxt].as<int>(), g->ccnt[nxt].as<int>(),
                       g->cstamp[nxt].as<int>(), pool, (const int*)keep, (const int*)rank, (const int*)rcnt, (const int*)roff, bound, d_removed,
                       capacity, (const GridState*)gs);
    g->cur_tab = nxt;
  }
  hipLaunchKernelGGL(carve_finish_kernel, dim3(1), dim3(1), 0, st, gs, d_pose, (const int*)keep, (const int*)rank, (const int*)rcnt, (const int*)roff, bound,
                     d_removed ? 1 : 0, capacity, ctr, info_dst, report_dst ? report_dst : g->report_dev.as<int>());
  HIPCHK(h, hipGetLastError());
  if (!report_dst) { HIPCHK(h, hipMemcpyAsync(g->report.p, g->report_dev.p, 16 * sizeof(int), hipMemcpyDeviceToHost, st)); g->pending = true; }
  g->last_seq = g->next_seq++;
  g->inflight.emplace_back(g->last_seq, 0);
  return MSFL_OK;
}

}  // namespace

extern "C" {

void msfl_carve_default_config(msfl_carve_config* cfg) {
  if (!cfg) return;
  cfg->n_col = 720; cfg->n_row = 16;
  cfg->elev_low_deg = -16.f; cfg->elev_high_deg = 16.f;
  cfg->min_range = 0.3f; cfg->max_range = 100.f;
  cfg->margin_abs = 0.3f; cfg->margin_rel = 0.02f;
  cfg->window_col = 1; cfg->window_row = 1;
}

msfl_status msfl_carve_tables(const msfl_carve_config* cfg, float* cc, float* cs, float* ec, float* es) {
  if (!cfg || !cc || !cs || !ec || !es || !carve_config_ok(*cfg)) return MSFL_BAD_ARG;
  carve_build_tables(*cfg, cc, cs, ec, es);
  return MSFL_OK;
}

// Remove the points the scan sees through (msfl_c_api.h)
msfl_status msfl_grid_carve(msfl_grid* g, const msfl_point* scan, int n, const double pose7[7], const msfl_carve_config* cfg, msfl_point* removed,
                            int capacity, msfl_mem mem, msfl_grid_carve_info* info) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  msfl_carve_config c;
  if (cfg) c = *cfg; else msfl_carve_default_config(&c);
  if (!info || !pose7 || n < 0 || (n > 0 && !scan) || (removed && capacity < 0)) return fail(h, MSFL_BAD_ARG, "msfl_grid_carve: bad argument");
  if (!carve_config_ok(c)) return fail(h, MSFL_BAD_ARG, "msfl_grid_carve: configuration outside its limits");
  if (mem == MSFL_MEM_HOST)
    for (int k = 0; k < 7; k++) if (!std::isfinite(pose7[k])) return fail(h, MSFL_BAD_ARG, "msfl_grid_carve: a pose that is not finite");
  hipStream_t st = h->stream;
  if (g->pending) { HIPCHK(h, hipStreamSynchronize(st)); (void)grid_read_report(g); }
  const double* d_pose = pose7;
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, g->pose.reserve(8 * sizeof(double)));
    HIPCHK(h, h->pin.upload(g->pose.p, pose7, 7 * sizeof(double), st));
    d_pose = g->pose.as<double>();
  }
  // staging of a host call: the scan, then room for the removed points (no more than the live points can go)
  const float4* d_scan = reinterpret_cast<const float4*>(scan);
  float4* d_rm = reinterpret_cast<float4*>(removed);
  if (mem == MSFL_MEM_HOST) {
    const long long stage_cap = removed ? std::min<long long>(capacity, g->ub_points) : 0;
    HIPCHK(h, g->stage.reserve(((size_t)n + (size_t)std::max<long long>(stage_cap, 1)) * sizeof(float4)));
    if (n > 0) HIPCHK(h, hipMemcpyAsync(g->stage.p, scan, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, st));
    d_scan = g->stage.as<float4>();
    if (removed) d_rm = g->stage.as<float4>() + n;
  }
  int* d_info = g->report_dev.as<int>() + 8;
  s = grid_carve_enqueue(g, d_scan, n, d_pose, c, d_rm, capacity, d_info); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(st));
  s = grid_read_report(g); if (s) return s;
  static_assert(sizeof(msfl_grid_carve_info) == CARVE_WORDS * sizeof(int), "msfl_grid_carve_info is the device record");
  std::memcpy(info, g->report.as<int>() + 8, sizeof(*info));
  if (!info->applied) {
    if (removed && info->n_points_removed > capacity) return fail(h, MSFL_CAPACITY, "msfl_grid_carve: more removed points than `capacity`; map unchanged");
    return fail(h, MSFL_BAD_ARG, "msfl_grid_carve: a pose that is not finite; map unchanged");
  }
  if (removed && mem == MSFL_MEM_HOST && info->n_points_removed > 0) {
    HIPCHK(h, hipMemcpyAsync(removed, d_rm, (size_t)info->n_points_removed * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
  }
  return MSFL_OK;
}

msfl_status msfl_grid_create(msfl_handle* h, float resolution, float leaf, msfl_grid** out) {
  msfl_status s = enter(h); if (s) return s;
  if (!out || !(resolution > 0.f) || !(leaf > 0.f)) return fail(h, MSFL_BAD_ARG, "msfl_grid_create: bad argument");
  // 7 bits of voxel coordinate per axis inside a cell (+ margins)
  if ((double)resolution / (double)leaf > 120.0) return fail(h, MSFL_BAD_ARG, "msfl_grid_create: resolution / leaf must be <= 120");
  msfl_grid* g = new msfl_grid_s();
  g->h = h;
  g->d.resolution = resolution;
  g->d.inv_leaf = 1.0f / leaf;
  g->d.leaf = (double)leaf;
  if (const char* e = std::getenv("MSFL_GRID_MIN_POOL")) { const long long v = std::atoll(e); if (v >= 1024) g->min_pool = v; }
  s = grid_init_state(g);
  if (s) { delete g; return s; }
  *out = g;
  return MSFL_OK;
}

void msfl_grid_destroy(msfl_grid* g) {
  if (!g) return;
  (void)hipSetDevice(g->h->device);
  (void)hipStreamSynchronize(g->h->stream);
  delete g;
}

msfl_status msfl_grid_size(msfl_grid* g, int* n_points, int* n_cells) {
  if (!g) return MSFL_BAD_ARG;
  if (g->pending) {                                  // an insert enqueued by the SLAM step: wait for its report
    msfl_status s = enter(g->h); if (s) return s;
    HIPCHK(g->h, hipStreamSynchronize(g->h->stream));
    (void)grid_read_report(g);
  }
  if (n_points) *n_points = g->n_points;
  if (n_cells) *n_cells = g->n_cells;
  return MSFL_OK;
}

// HybridGrid::InsertScan (hybrid_grid.cc:503-521); `pts` are already in the map frame
// (laser_mapping.cc:330-338 transforms them first).
msfl_status msfl_grid_insert_scan(msfl_grid* g, const msfl_point* pts, int n, msfl_mem mem) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || (n > 0 && !pts)) return fail(h, MSFL_BAD_ARG, "msfl_grid_insert_scan: bad argument");
  if (n == 0) return MSFL_OK;                                    // :504
  const float4* d_pts;
  s = stage_in(h, g->stage, pts, (size_t)n, mem, h->stream, &d_pts); if (s) return s;
  s = grid_insert_enqueue(g, d_pts, n, nullptr, nullptr); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return grid_read_report(g);
}

// HybridGrid::GetSurroundedCloud (hybrid_grid.cc:470-501): `scan` in the scan frame, `pose` = scan -> map.
// Cells are emitted in ascending (iz, iy, ix) order (the reference's order is that of a
// boost::unordered_set of pointers, i.e. unspecified).  *n_out is the full count even if it exceeds
// `capacity` (then only `capacity` points are written and MSFL_CAPACITY is returned).
msfl_status msfl_grid_get_surrounded(msfl_grid* g, const msfl_point* scan, int n, const double pose[7], msfl_point* out,
                                     int capacity, int* n_out, msfl_mem mem) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (n < 0 || !pose || !n_out || capacity < 0 || (n > 0 && !scan) || (capacity > 0 && !out))
    return fail(h, MSFL_BAD_ARG, "msfl_grid_get_surrounded: bad argument");
  *n_out = 0;
  if (g->ub_cells == 0 || n == 0) return MSFL_OK;
  hipStream_t st = h->stream;
  HIPCHK(h, g->pose.reserve(8 * sizeof(double)));
  HIPCHK(h, h->pin.upload(g->pose.p, pose, 7 * sizeof(double), st));
  const float4* d_scan = reinterpret_cast<const float4*>(scan);
  float4* d_out = reinterpret_cast<float4*>(out);
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(h, g->stage.reserve(((size_t)n + (size_t)capacity) * sizeof(float4)));
    HIPCHK(h, hipMemcpyAsync(g->stage.p, scan, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, st));
    d_scan = g->stage.as<float4>();
    d_out = g->stage.as<float4>() + n;
  }
  int* d_total = reinterpret_cast<int*>(g->pose.as<double>() + 7);
  s = grid_surround_enqueue(g, d_scan, nullptr, n, nullptr, g->pose.as<double>(), d_out, capacity, d_total); if (s) return s;
  HIPCHK(h, h->readback.reserve(sizeof(int)));
  HIPCHK(h, hipMemcpyAsync(h->readback.p, d_total, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (g->pending) (void)grid_read_report(g);
  const int total = *h->readback.as<int>();
  *n_out = total;
  const int m = std::min(total, capacity);
  if (mem == MSFL_MEM_HOST && m > 0) {
    HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
  }
  if (total > capacity) return fail(h, MSFL_CAPACITY, "msfl_grid_get_surrounded: output capacity too small");
  return MSFL_OK;
}

// The whole map (cells ascending), e.g. for the PLY dump of laser_mapping.cc:95-113.
msfl_status msfl_grid_dump(msfl_grid* g, msfl_point* out, int capacity, int* n_out, msfl_mem mem) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (!n_out || capacity < 0 || (capacity > 0 && !out)) return fail(h, MSFL_BAD_ARG, "msfl_grid_dump: bad argument");
  if (g->pending) { HIPCHK(h, hipStreamSynchronize(h->stream)); (void)grid_read_report(g); }
  *n_out = g->n_points;
  const int m = std::min(g->n_points, capacity);
  if (m > 0) {
    float4* d_out = reinterpret_cast<float4*>(out);
    if (mem == MSFL_MEM_HOST) { HIPCHK(h, g->stage.reserve((size_t)m * sizeof(float4))); d_out = g->stage.as<float4>(); }
    s = grid_pack(g, d_out, m, false); if (s) return s;
    s = stage_out(h, out, d_out, (size_t)m, mem, h->stream); if (s) return s;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return g->n_points > capacity ? MSFL_CAPACITY : MSFL_OK;
}

// Forget every cell outside the window of +-half_cells cells around the cell of `center` (msfl_c_api.h).
static msfl_status grid_crop_sync(msfl_grid* g, const double center[3], const int half_cells[3], msfl_point* evicted, int capacity, int* evicted_cells,
                                  int cell_capacity, bool tiles, msfl_mem mem, msfl_grid_crop_info* info) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (!info || !center || !half_cells || half_cells[0] < 0 || half_cells[1] < 0 || half_cells[2] < 0 || !std::isfinite(center[0]) ||
      !std::isfinite(center[1]) || !std::isfinite(center[2]) || !std::isfinite((float)center[0]) || !std::isfinite((float)center[1]) ||
      !std::isfinite((float)center[2]) || (evicted && capacity < 0) || (tiles && (!evicted || !evicted_cells || cell_capacity < 0)))
    return fail(h, MSFL_BAD_ARG, tiles ? "msfl_grid_crop_tiles: bad argument" : "msfl_grid_crop: bad argument");
  hipStream_t st = h->stream;
  if (g->pending) { HIPCHK(h, hipStreamSynchronize(st)); (void)grid_read_report(g); }
  HIPCHK(h, g->pose.reserve(8 * sizeof(double)));
  HIPCHK(h, h->pin.upload(g->pose.p, center, 3 * sizeof(double), st));
  float4* d_ev = reinterpret_cast<float4*>(evicted);
  const int stage_cap = (int)std::min<long long>(capacity, g->ub_points);   // no more than the live points can be evicted
  if (evicted && mem == MSFL_MEM_HOST) { HIPCHK(h, g->stage.reserve((size_t)std::max(stage_cap, 1) * sizeof(float4))); d_ev = g->stage.as<float4>(); }
  int* d_info = g->report_dev.as<int>() + 8;
  int* d_cells = nullptr;
  if (tiles) {                                                               // no more than the live cells can be evicted
    HIPCHK(h, g->crop_cells.reserve((size_t)std::max<long long>(std::min<long long>(cell_capacity, g->ub_cells), 1) * 4 * sizeof(int)));
    d_cells = g->crop_cells.as<int>();
  }
  s = grid_crop_enqueue(g, g->pose.as<double>(), half_cells, d_ev, capacity, d_info, nullptr, false, d_cells, cell_capacity); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(st));
  s = grid_read_report(g); if (s) return s;
  static_assert(sizeof(msfl_grid_crop_info) == CROP_WORDS * sizeof(int), "msfl_grid_crop_info is the device record");
  std::memcpy(info, g->report.as<int>() + 8, sizeof(*info));
  if (!info->applied)
    return fail(h, MSFL_CAPACITY, tiles ? "msfl_grid_crop_tiles: more evicted points than `capacity` or more evicted cells than `cell_capacity`; map unchanged"
                                        : "msfl_grid_crop: more evicted points than `capacity`; map unchanged");
  bool copying = false;
  if (tiles && info->n_cells_evicted > 0) {
    HIPCHK(h, hipMemcpyAsync(evicted_cells, d_cells, (size_t)info->n_cells_evicted * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    copying = true;
  }
  if (evicted && mem == MSFL_MEM_HOST && info->n_points_evicted > 0) {
    HIPCHK(h, hipMemcpyAsync(evicted, d_ev, (size_t)info->n_points_evicted * sizeof(float4), hipMemcpyDeviceToHost, st));
    copying = true;
  }
  if (copying) HIPCHK(h, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_grid_crop(msfl_grid* g, const double center[3], const int half_cells[3], msfl_point* evicted, int capacity, msfl_mem mem,
                           msfl_grid_crop_info* info) {
  return grid_crop_sync(g, center, half_cells, evicted, capacity, nullptr, 0, false, mem, info);
}

// msfl_grid_crop that also delivers {ix, iy, iz, count} of the evicted cells, in the order of `evicted` (msfl_c_api.h)
msfl_status msfl_grid_crop_tiles(msfl_grid* g, const double center[3], const int half_cells[3], msfl_point* evicted, int capacity,
                                 int* evicted_cells, int cell_capacity, msfl_mem mem, msfl_grid_crop_info* info) {
  return grid_crop_sync(g, center, half_cells, evicted, capacity, evicted_cells, cell_capacity, true, mem, info);
}

// Dumped or evicted cells back into the store, verbatim (msfl_c_api.h)
msfl_status msfl_grid_load_cells(msfl_grid* g, const int* cells, int n_cells, const msfl_point* pts, int n_points, msfl_mem mem, int* conflict,
                                 msfl_grid_load_info* info) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (!info || n_cells < 0 || n_points < 0 || (n_cells > 0 && !cells) || (n_points > 0 && !pts))
    return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: bad argument");
  const int lim = 1 << (kGridCellBits - 1);
  long long sum = 0;
  unsigned long long prev = 0;
  for (int j = 0; j < n_cells; j++) {
    const int* c = cells + 4 * (size_t)j;
    if (c[3] <= 0) return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: a listed cell with a count <= 0");
    if (c[0] < -lim || c[0] >= lim || c[1] < -lim || c[1] >= lim || c[2] < -lim || c[2] >= lim)
      return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: a cell index outside [-8192, 8191]");
    const unsigned long long key = ((unsigned long long)(c[2] + lim) << (2 * kGridCellBits)) | ((unsigned long long)(c[1] + lim) << kGridCellBits) |
                                   (unsigned long long)(c[0] + lim);
    if (j > 0 && key <= prev) return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: cells not strictly ascending in (iz, iy, ix)");
    prev = key;
    sum += c[3];
  }
  if (sum != n_points) return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: the counts do not sum to n_points");
  hipStream_t st = h->stream;
  if (g->pending) { HIPCHK(h, hipStreamSynchronize(st)); (void)grid_read_report(g); }
  static_assert(sizeof(msfl_grid_load_info) == LOAD_WORDS * sizeof(int), "msfl_grid_load_info is the device record");
  if (n_cells == 0) {
    std::memset(info, 0, sizeof(*info));
    info->n_cells = g->n_cells; info->n_points = g->n_points; info->applied = 1;
    return MSFL_OK;
  }
  const size_t n = (size_t)n_cells;
  HIPCHK(h, g->load.reserve(n * (16 + 8 + 4 * 4)));
  HIPCHK(h, hipMemcpyAsync(g->load.p, cells, n * 16, hipMemcpyHostToDevice, st));
  const float4* d_pts;
  s = stage_in(h, g->stage, pts, (size_t)n_points, mem, st, &d_pts); if (s) return s;
  int* d_info = g->report_dev.as<int>() + 8;
  s = grid_load_enqueue(g, g->load.as<int>(), n_cells, d_pts, n_points, d_info); if (s) return s;
  HIPCHK(h, hipStreamSynchronize(st));
  s = grid_read_report(g); if (s) return s;
  std::memcpy(info, g->report.as<int>() + 8, sizeof(*info));
  if (conflict) {
    const int* lconf = reinterpret_cast<const int*>(g->load.as<char>() + 16 * n + 8 * n) + n;
    HIPCHK(h, hipMemcpy(conflict, lconf, n * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (info->applied) return MSFL_OK;
  if (info->n_conflicts > 0) return fail(h, MSFL_BAD_ARG, "msfl_grid_load_cells: a listed cell is live in the store already; map unchanged");
  if (info->n_bad_points > 0) return fail(h, MSFL_CAPACITY, "msfl_grid_load_cells: a point is not finite; map unchanged");
  return fail(h, MSFL_CAPACITY, "msfl_grid_load_cells: internal capacity exceeded; map unchanged");
}

// {ix, iy, iz, count} of every cell, in the order of msfl_grid_dump
msfl_status msfl_grid_dump_cells(msfl_grid* g, int* cells, int capacity, int* n_out) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  if (!n_out || capacity < 0 || (capacity > 0 && !cells)) return fail(h, MSFL_BAD_ARG, "msfl_grid_dump_cells: bad argument");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (g->pending) (void)grid_read_report(g);
  *n_out = g->n_cells;
  const int m = std::min(g->n_cells, capacity);
  if (m > 0) {
    std::vector<unsigned long long> keys((size_t)m);
    std::vector<int> cnt((size_t)m);
    HIPCHK(h, hipMemcpy(keys.data(), g->ckey[g->cur_tab].p, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(cnt.data(), g->ccnt[g->cur_tab].p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    const int lim = 1 << (kGridCellBits - 1), mask = (1 << kGridCellBits) - 1;
    for (int c = 0; c < m; c++) {
      cells[4 * c] = (int)(keys[c] & mask) - lim; cells[4 * c + 1] = (int)((keys[c] >> kGridCellBits) & mask) - lim;
      cells[4 * c + 2] = (int)(keys[c] >> (2 * kGridCellBits)) - lim; cells[4 * c + 3] = cnt[c];
    }
  }
  return g->n_cells > capacity ? MSFL_CAPACITY : MSFL_OK;
}

// {n_points, n_cells, pool_top, pool_capacity_points, cell_capacity, device_bytes}
msfl_status msfl_grid_stats(msfl_grid* g, long long out[6]) {
  if (!g || !out) return MSFL_BAD_ARG;
  if (g->pending) {
    msfl_status s = enter(g->h); if (s) return s;
    HIPCHK(g->h, hipStreamSynchronize(g->h->stream));
    (void)grid_read_report(g);
  }
  const DevBuf* bufs[] = {&g->state, &g->pool[0], &g->pool[1], &g->ckey[0], &g->ckey[1], &g->cstart[0], &g->cstart[1], &g->ccnt[0], &g->ccnt[1],
                          &g->cstamp[0], &g->cstamp[1], &g->keys, &g->keys_s, &g->vals, &g->vals_s, &g->head, &g->tpos, &g->xf, &g->xs, &g->t_key, &g->t_ns,
                          &g->t_old, &g->t_woff, &g->t_rank, &g->t_cnt, &g->cnt, &g->off, &g->stage, &g->pose, &g->report_dev, &g->crop, &g->crop_cells, &g->load,
                          &g->carve_img, &g->carve_cells, &g->carve_tab, &g->carve_ctr};
  long long bytes = 0;
  for (auto* b : bufs) bytes += (long long)b->cap;
  out[0] = g->n_points; out[1] = g->n_cells; out[2] = g->pool_top; out[3] = (long long)pool_capacity(g); out[4] = g->cell_cap; out[5] = bytes;
  return MSFL_OK;
}

}  // extern "C"

#ifdef MSFL_GRID_PROF
extern "C" int msfl_debug_vox_prof(unsigned long long* out, int n_words) {
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(msfl::g_vox_prof), (size_t)n_words * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif
#ifdef MSFL_GRID_PROF
extern "C" int msfl_debug_grid_prof(unsigned long long* out, int n_words) {
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(msfl::g_grid_prof), (size_t)n_words * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
#endif
