// Render and scan novelty — C-ABI entry points msfl_grid_render, msfl_novelty_default_config, msfl_scan_novelty and
// msfl_grids_scan_novelty.  Included at the end of msfl_api.hip after msfl_api_grid.inc and msfl_api_segment.inc (shares the handle,
// the map store, DevBuf, PinRing and the helper macros); kernels: msfl_novelty.cuh.  The calls work in scratch of their own (h->nv),
// allocated by the first call: a process that never calls them launches and allocates nothing here.  Both enqueue functions read
// launch bounds from what the host knows already (ub_cells, n), so neither waits for the device.

#include "msfl_novelty.cuh"

namespace {

static_assert(sizeof(msfl_novelty_info) == (NOV_CTR_RESERVED + 1) * sizeof(int), "msfl_novelty_info is the first 8 counter words");
static_assert(sizeof(msfl_grid_render_info) == 2 * sizeof(int) && NOV_CTR_RENDERED == NOV_CTR_TESTED + 1, "msfl_grid_render_info is the next 2");
static_assert(MSFL_NOV_NONE == NOV_NONE && MSFL_NOV_UNSEEN == NOV_UNSEEN && MSFL_NOV_COVERED == NOV_COVERED && MSFL_NOV_IN_FRONT == NOV_IN_FRONT &&
              MSFL_NOV_CLASSES == NOV_CLASSES, "the classes of the header are the kernels'");

bool novelty_config_ok(const msfl_novelty_config& c) {
  return carve_config_ok(c.image) && c.min_support >= 1 && c.min_support <= (2 * c.image.window_col + 1) * (2 * c.image.window_row + 1) &&
         c.keep_classes >= 0 && c.keep_classes < (1 << NOV_CLASSES);
}

bool pose_finite(const double pose7[7]) {
  for (int k = 0; k < 7; k++) if (!std::isfinite(pose7[k])) return false;
  return true;
}

// The configuration as the kernels see it.  The counters are allocated here; the tables are rebuilt and uploaded only when the
// geometry they depend on differs from the last call's.
msfl_status novelty_cfg(msfl_handle* h, const msfl_carve_config& cfg, CarveCfg* out) {
  NoveltyScratch& nv = h->nv;
  HIPCHK(h, nv.ctr.reserve(NOV_CTR_WORDS * sizeof(int)));
  const msfl_carve_config& o = nv.tab_cfg;
  if (!nv.tab_valid || o.n_col != cfg.n_col || o.n_row != cfg.n_row || std::memcmp(&o.elev_low_deg, &cfg.elev_low_deg, sizeof(float)) != 0 ||
      std::memcmp(&o.elev_high_deg, &cfg.elev_high_deg, sizeof(float)) != 0) {
    float tab[kCarveMaxTab];
    const int half = cfg.n_col / 2;
    carve_build_tables(cfg, tab, tab + half, tab + 2 * half, tab + 2 * half + cfg.n_row + 1);
    HIPCHK(h, nv.tab.reserve(kCarveMaxTab * sizeof(float)));
    HIPCHK(h, h->pin.upload(nv.tab.p, tab, (size_t)carve_tab_size(cfg.n_col, cfg.n_row) * sizeof(float), h->stream));
    nv.tab_cfg = cfg; nv.tab_valid = true;
  }
  *out = CarveCfg{cfg.n_col, cfg.n_row, cfg.window_col, cfg.window_row, cfg.min_range, cfg.max_range, cfg.margin_abs, cfg.margin_rel,
                  (const float*)nv.tab.as<float>()};
  return MSFL_OK;
}

// Stream-ordered render of `g` at the device-resident `d_pose` (7 doubles) into the device image `d_img` (n_col x n_row words).  The
// store is only read: no sequence number, no report, the table parity stays.
msfl_status render_enqueue(msfl_grid* g, const double* d_pose, const msfl_carve_config& cfg, unsigned* d_img, bool accumulate) {
  msfl_handle* h = g->h;
  hipStream_t st = h->stream;
  CarveCfg c;
  msfl_status s = novelty_cfg(h, cfg, &c); if (s) return s;
  int* ctr = h->nv.ctr.as<int>();
  const int npix = accumulate ? 0 : cfg.n_col * cfg.n_row;
  hipLaunchKernelGGL(render_clear_kernel, dim3(std::max(div_up(npix, kCarveBlock), 1)), dim3(kCarveBlock), 0, st, d_pose, d_img, npix, ctr);
  const int bound = (int)std::min<long long>(g->ub_cells, g->cell_cap);
  if (bound > 0) {
    const int cur = g->cur_tab;
    hipLaunchKernelGGL(render_cells_kernel, dim3(std::min(bound, 4096)), dim3(kCarveBlock), 0, st, c, d_pose,
                       (const unsigned long long*)g->ckey[cur].as<unsigned long long>(), (const int*)g->cstart[cur].as<int>(),
                       (const int*)g->ccnt[cur].as<int>(), (const float4*)g->pool[g->cur_pool].as<float4>(), bound, g->d.resolution, d_img, ctr,
                       (const GridState*)g->state.as<GridState>());
  }
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// Stream-ordered labels of the device scan against the device image.  rendered: null, or the applied word of the render before it.
msfl_status novelty_enqueue(msfl_handle* h, const float4* d_scan, int n, const unsigned* d_img, const msfl_novelty_config& cfg, uint8_t* d_cls,
                            float4* d_masked, const int* rendered) {
  hipStream_t st = h->stream;
  CarveCfg c;
  msfl_status s = novelty_cfg(h, cfg.image, &c); if (s) return s;
  const int npix = cfg.image.n_col * cfg.image.n_row;
  HIPCHK(h, h->nv.win.reserve(2 * (size_t)npix * sizeof(int)));
  unsigned* mlim = h->nv.win.as<unsigned>();
  int* support = h->nv.win.as<int>() + npix;
  int* ctr = h->nv.ctr.as<int>();
  HIPCHK(h, hipMemsetAsync(ctr, 0, NOV_CTR_APPLIED * sizeof(int), st));
  hipLaunchKernelGGL(novelty_window_kernel, dim3(div_up(npix, kCarveBlock)), dim3(kCarveBlock), 0, st, c, d_img, mlim, support, ctr);
  hipLaunchKernelGGL(novelty_label_kernel, dim3(std::max(std::min(div_up(n, kCarveBlock), 1024), 1)), dim3(kCarveBlock), 0, st, c, cfg.min_support,
                     cfg.keep_classes, d_scan, n, (const unsigned*)mlim, (const int*)support, rendered, d_cls, d_masked, ctr);
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// what the three calls refuse alike before anything is staged: the scan's arguments
const char* novelty_scan_bad(const msfl_point* scan, int n, const uint8_t* cls_out, const msfl_point* masked_out) {
  if (n < 0 || (n > 0 && (!scan || !cls_out))) return "n < 0, or scan / cls_out NULL with points to label";
  if (masked_out && scan && n > 0 && seg_overlap(scan, (size_t)n * sizeof(msfl_point), masked_out, (size_t)n * sizeof(msfl_point)))
    return "masked_out overlaps scan";
  return nullptr;
}

// the scan in, the labels, the outputs back, the info record: everything of a labelling call after the image stands at d_img
msfl_status novelty_run(msfl_handle* h, const char* who, const msfl_point* scan, int n, const unsigned* d_img, const msfl_novelty_config& c,
                        uint8_t* cls_out, msfl_point* masked_out, const int* rendered, float* img_out, msfl_novelty_info* info, msfl_mem mem) {
  hipStream_t st = h->stream;
  NoveltyScratch& nv = h->nv;
  const bool host = mem == MSFL_MEM_HOST;
  const float4* d_scan = nullptr;
  msfl_status s = stage_in(h, nv.in_scan, scan, (size_t)n, mem, st, &d_scan); if (s) return s;
  uint8_t* d_cls = cls_out;
  float4* d_masked = reinterpret_cast<float4*>(masked_out);
  if (host) {
    HIPCHK(h, nv.out_cls.reserve(std::max<size_t>(1, (size_t)n)));
    d_cls = nv.out_cls.as<uint8_t>();
    if (masked_out) { HIPCHK(h, nv.out_masked.reserve(std::max<size_t>(1, (size_t)n) * sizeof(float4))); d_masked = nv.out_masked.as<float4>(); }
  }
  s = novelty_enqueue(h, d_scan, n, d_img, c, d_cls, d_masked, rendered); if (s) return s;
  if (host) {
    s = stage_out(h, cls_out, d_cls, (size_t)n, mem, st); if (s) return s;
    if (masked_out) { s = stage_out(h, masked_out, d_masked, (size_t)n, mem, st); if (s) return s; }
    if (img_out) { s = stage_out(h, img_out, reinterpret_cast<const float*>(d_img), (size_t)c.image.n_col * c.image.n_row, mem, st); if (s) return s; }
  }
  if (info) {
    HIPCHK(h, h->readback.reserve(sizeof(msfl_novelty_info)));
    HIPCHK(h, hipMemcpyAsync(h->readback.p, nv.ctr.p, sizeof(msfl_novelty_info), hipMemcpyDeviceToHost, st));
  }
  if (host || info) HIPCHK(h, hipStreamSynchronize(st));
  if (info) {
    std::memcpy(info, h->readback.p, sizeof(*info));
    if (!info->applied) return fail(h, MSFL_BAD_ARG, std::string(who) + ": a pose that is not finite; nothing rendered, every point is NONE");
  }
  return MSFL_OK;
}

}  // namespace

extern "C" {

void msfl_novelty_default_config(msfl_novelty_config* cfg) {
  if (!cfg) return;
  msfl_carve_default_config(&cfg->image);
  cfg->image.window_col = 2; cfg->image.window_row = 1;
  cfg->min_support = 1;
  cfg->keep_classes = (1 << MSFL_NOV_NONE) | (1 << MSFL_NOV_UNSEEN) | (1 << MSFL_NOV_COVERED);
}

// The range image the store predicts for a sensor at pose7 (msfl_c_api.h)
msfl_status msfl_grid_render(msfl_grid* g, const double pose7[7], const msfl_carve_config* cfg, float* range_img, int accumulate, msfl_mem mem,
                             msfl_grid_render_info* info) {
  if (!g) return MSFL_BAD_ARG;
  msfl_handle* h = g->h;
  msfl_status s = enter(h); if (s) return s;
  msfl_carve_config c;
  if (cfg) c = *cfg; else msfl_carve_default_config(&c);
  if (!pose7 || !range_img) return fail(h, MSFL_BAD_ARG, "msfl_grid_render: bad argument");
  if (!carve_config_ok(c)) return fail(h, MSFL_BAD_ARG, "msfl_grid_render: configuration outside its limits");
  const bool host = mem == MSFL_MEM_HOST;
  if (host && !pose_finite(pose7)) return fail(h, MSFL_BAD_ARG, "msfl_grid_render: a pose that is not finite");
  hipStream_t st = h->stream;
  NoveltyScratch& nv = h->nv;
  const size_t npix = (size_t)c.n_col * c.n_row;
  const double* d_pose = pose7;
  unsigned* d_img = reinterpret_cast<unsigned*>(range_img);
  if (host) {
    HIPCHK(h, nv.pose.reserve(8 * sizeof(double)));
    HIPCHK(h, h->pin.upload(nv.pose.p, pose7, 7 * sizeof(double), st));
    d_pose = nv.pose.as<double>();
    HIPCHK(h, nv.img.reserve(npix * sizeof(unsigned)));
    d_img = nv.img.as<unsigned>();
    if (accumulate) HIPCHK(h, hipMemcpyAsync(d_img, range_img, npix * sizeof(unsigned), hipMemcpyHostToDevice, st));
  }
  s = render_enqueue(g, d_pose, c, d_img, accumulate != 0); if (s) return s;
  s = stage_out(h, range_img, reinterpret_cast<const float*>(d_img), npix, mem, st); if (s) return s;
  if (info) {
    HIPCHK(h, h->readback.reserve(sizeof(msfl_grid_render_info)));
    HIPCHK(h, hipMemcpyAsync(h->readback.p, nv.ctr.as<int>() + NOV_CTR_TESTED, sizeof(msfl_grid_render_info), hipMemcpyDeviceToHost, st));
  }
  if (host || info) HIPCHK(h, hipStreamSynchronize(st));
  if (info) {
    std::memcpy(info, h->readback.p, sizeof(*info));
    if (!info->applied) return fail(h, MSFL_BAD_ARG, "msfl_grid_render: a pose that is not finite; nothing rendered");
  }
  return MSFL_OK;
}

// One class per scan point against a map image (msfl_c_api.h)
msfl_status msfl_scan_novelty(msfl_handle* h, const msfl_point* scan, int n, const float* map_img, const msfl_novelty_config* cfg, uint8_t* cls_out,
                              msfl_point* masked_out, msfl_novelty_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  msfl_novelty_config c;
  if (cfg) c = *cfg; else msfl_novelty_default_config(&c);
  if (!map_img) return fail(h, MSFL_BAD_ARG, "msfl_scan_novelty: map_img is NULL");
  if (const char* bad = novelty_scan_bad(scan, n, cls_out, masked_out)) return fail(h, MSFL_BAD_ARG, std::string("msfl_scan_novelty: ") + bad);
  if (!novelty_config_ok(c)) return fail(h, MSFL_BAD_ARG, "msfl_scan_novelty: configuration outside its limits");
  const unsigned* d_img = nullptr;
  s = stage_in(h, h->nv.img, map_img, (size_t)c.image.n_col * c.image.n_row, mem, h->stream, &d_img); if (s) return s;
  return novelty_run(h, "msfl_scan_novelty", scan, n, d_img, c, cls_out, masked_out, nullptr, nullptr, info, mem);
}

// Render the stores into one image, then label the scan against it (msfl_c_api.h)
msfl_status msfl_grids_scan_novelty(msfl_grid* const* grids, int n_grids, const msfl_point* scan, int n, const double pose7[7],
                                    const msfl_novelty_config* cfg, uint8_t* cls_out, msfl_point* masked_out, float* map_img_out,
                                    msfl_novelty_info* info, msfl_mem mem) {
  if (!grids || n_grids < 1 || n_grids > 8 || !grids[0]) return MSFL_BAD_ARG;
  msfl_handle* h = grids[0]->h;
  msfl_status s = enter(h); if (s) return s;
  for (int k = 1; k < n_grids; k++)
    if (!grids[k] || grids[k]->h != h) return fail(h, MSFL_BAD_ARG, "msfl_grids_scan_novelty: the grids must belong to one handle");
  msfl_novelty_config c;
  if (cfg) c = *cfg; else msfl_novelty_default_config(&c);
  if (!pose7) return fail(h, MSFL_BAD_ARG, "msfl_grids_scan_novelty: pose7 is NULL");
  if (const char* bad = novelty_scan_bad(scan, n, cls_out, masked_out)) return fail(h, MSFL_BAD_ARG, std::string("msfl_grids_scan_novelty: ") + bad);
  if (!novelty_config_ok(c)) return fail(h, MSFL_BAD_ARG, "msfl_grids_scan_novelty: configuration outside its limits");
  const bool host = mem == MSFL_MEM_HOST;
  if (host && !pose_finite(pose7)) return fail(h, MSFL_BAD_ARG, "msfl_grids_scan_novelty: a pose that is not finite");
  hipStream_t st = h->stream;
  NoveltyScratch& nv = h->nv;
  const double* d_pose = pose7;
  if (host) {
    HIPCHK(h, nv.pose.reserve(8 * sizeof(double)));
    HIPCHK(h, h->pin.upload(nv.pose.p, pose7, 7 * sizeof(double), st));
    d_pose = nv.pose.as<double>();
  }
  unsigned* d_img = reinterpret_cast<unsigned*>(map_img_out);
  if (host || !map_img_out) {
    HIPCHK(h, nv.img.reserve((size_t)c.image.n_col * c.image.n_row * sizeof(unsigned)));
    d_img = nv.img.as<unsigned>();
  }
  for (int k = 0; k < n_grids; k++) { s = render_enqueue(grids[k], d_pose, c.image, d_img, k > 0); if (s) return s; }
  return novelty_run(h, "msfl_grids_scan_novelty", scan, n, d_img, c, cls_out, masked_out, nv.ctr.as<int>() + NOV_CTR_RENDERED, map_img_out, info, mem);
}

}  // extern "C"
