// Scan segmentation — C-ABI entry points msfl_segment_default_config, msfl_segment_tables, msfl_segment_scans and msfl_segment_scan.
// Included at the end of msfl_api.hip (shares its handle, DevBuf, PinRing and helper macros); kernels: msfl_segment.cuh.  The call
// works in scratch of its own (h->sg), allocated by the first call: a handle that never segments launches and allocates nothing here.

#include "msfl_segment.cuh"

namespace {

static_assert(sizeof(msfl_segment_info) == SEG_INFO_WORDS * sizeof(int), "msfl_segment_info is the device record");
static_assert(MSFL_SEG_NONE == SEG_NONE && MSFL_SEG_SHADOWED == SEG_SHADOWED && MSFL_SEG_GROUND == SEG_GROUND && MSFL_SEG_SEGMENT == SEG_SEGMENT &&
              MSFL_SEG_OUTLIER == SEG_OUTLIER && MSFL_SEG_CLASSES == SEG_CLASSES, "the classes of the header are the kernels'");

constexpr size_t kSegScratchBudgetBytes = size_t(256) << 20;      // images of one chunk of scans (kSegPixelBytes per pixel)
constexpr int kSegMaxChunkScans = 32768;                          // the scan inside a chunk is blockIdx.y

// e[k] in degrees, as a double
double seg_elev_deg(const msfl_segment_config& c, int k) {
  if (c.row_elev_deg) return (double)c.row_elev_deg[k];
  return (double)c.elev_low_deg + ((double)c.elev_high_deg - (double)c.elev_low_deg) * (double)k / (double)(c.n_row - 1);
}

const char* seg_config_bad(const msfl_segment_config& c) {
  const float f[10] = {c.elev_low_deg, c.elev_high_deg, c.min_range, c.max_range, c.ground_angle_deg, c.up[0], c.up[1], c.up[2], c.segment_angle_deg, 0.f};
  for (float v : f) if (!std::isfinite(v)) return "a field that is not finite";
  if (c.n_col < 4 || c.n_col > kSegMaxCol || (c.n_col & 1)) return "n_col must be even, 4..2048";
  if (c.n_row < 2 || c.n_row > kSegMaxRow) return "n_row must be 2..128";
  if (c.row_elev_deg) {
    for (int k = 0; k < c.n_row; k++) {
      const float e = c.row_elev_deg[k];
      if (!std::isfinite(e) || !(e > -90.f) || !(e < 90.f)) return "row_elev_deg outside (-90, 90)";
      if (k > 0 && !(e > c.row_elev_deg[k - 1])) return "row_elev_deg must ascend strictly";
    }
  } else if (!(c.elev_low_deg > -90.f && c.elev_low_deg < c.elev_high_deg && c.elev_high_deg < 90.f)) {
    return "elevations need -90 < elev_low_deg < elev_high_deg < 90";
  }
  if (!(c.min_range >= 0.f && c.min_range < c.max_range)) return "ranges need 0 <= min_range < max_range";
  if (c.ground_rows < 0 || c.ground_rows > c.n_row - 1) return "ground_rows must be 0..n_row - 1";
  if (!(c.ground_angle_deg > 0.f && c.ground_angle_deg < 90.f)) return "ground_angle_deg must lie in (0, 90)";
  if (!(c.segment_angle_deg > 0.f && c.segment_angle_deg < 90.f)) return "segment_angle_deg must lie in (0, 90)";
  const double u2 = (double)c.up[0] * c.up[0] + (double)c.up[1] * c.up[1] + (double)c.up[2] * c.up[2];
  if (!(std::fabs(u2 - 1.0) < 1e-3)) return "up must be a unit vector";
  if (c.min_points < 1 || c.min_points_tall < 1 || c.min_rows_tall < 1) return "the cluster sizes must be >= 1";
  if (c.keep_classes < 0 || c.keep_classes >= (1 << SEG_CLASSES)) return "keep_classes must be 0..31";
  return nullptr;
}

// the tables in double, rounded to f32 (docs/kernels/segment.md states the formulas)
void seg_build_tables(const msfl_segment_config& c, float* cc, float* cs, float* vs, float* vc, float* scalars) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < c.n_col / 2; k++) {
    const double a = 2.0 * pi * ((double)k - 0.5) / (double)c.n_col;
    cc[k] = (float)std::cos(a); cs[k] = (float)std::sin(a);
  }
  for (int k = 0; k + 1 < c.n_row; k++) {
    const double a = (seg_elev_deg(c, k + 1) - seg_elev_deg(c, k)) * pi / 180.0;
    vs[k] = (float)std::sin(a); vc[k] = (float)std::cos(a);
  }
  const double h = 2.0 * pi / (double)c.n_col, g = std::sin((double)c.ground_angle_deg * pi / 180.0);
  scalars[0] = (float)std::sin(h); scalars[1] = (float)std::cos(h);
  scalars[2] = (float)(g * g);
  scalars[3] = (float)std::tan((double)c.segment_angle_deg * pi / 180.0);
}

bool seg_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

void msfl_segment_default_config(msfl_segment_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->n_col = 1800; cfg->n_row = 16;
  cfg->elev_low_deg = -15.f; cfg->elev_high_deg = 15.f;
  cfg->row_elev_deg = nullptr;
  cfg->min_range = 0.3f; cfg->max_range = 100.f;
  cfg->ground_rows = 8; cfg->ground_angle_deg = 10.f;
  cfg->up[0] = 0.f; cfg->up[1] = 0.f; cfg->up[2] = 1.f;
  cfg->segment_angle_deg = 60.f;
  cfg->min_points = 30; cfg->min_points_tall = 5; cfg->min_rows_tall = 3;
  cfg->keep_classes = (1 << MSFL_SEG_GROUND) | (1 << MSFL_SEG_SEGMENT);
}

msfl_status msfl_segment_tables(const msfl_segment_config* cfg, float* cc, float* cs, float* vs, float* vc, float scalars[4]) {
  if (!cfg || !cc || !cs || !vs || !vc || !scalars || seg_config_bad(*cfg)) return MSFL_BAD_ARG;
  seg_build_tables(*cfg, cc, cs, vs, vc, scalars);
  return MSFL_OK;
}

msfl_status msfl_segment_scans(msfl_handle* h, int n_scans, const msfl_point* pts, const uint16_t* ring, const int* off,
                               const msfl_segment_config* cfg, uint8_t* cls_out, int* segment_out, msfl_point* masked_out,
                               msfl_segment_info* info, msfl_mem mem) {
  msfl_status s = enter(h); if (s) return s;
  msfl_segment_config c;
  if (cfg) c = *cfg; else msfl_segment_default_config(&c);
  if (n_scans < 0 || (n_scans > 0 && !off)) return fail(h, MSFL_BAD_ARG, "msfl_segment_scans: bad argument");
  if (const char* bad = seg_config_bad(c)) return fail(h, MSFL_BAD_ARG, std::string("msfl_segment_scans: ") + bad);
  if (n_scans == 0) return MSFL_OK;
  if (off[0] < 0) return fail(h, MSFL_BAD_ARG, "msfl_segment_scans: off[0] < 0");
  for (int b = 0; b < n_scans; b++)
    if (off[b + 1] < off[b]) return fail(h, MSFL_BAD_ARG, "msfl_segment_scans: offsets descend");
  const size_t first = (size_t)off[0], n_total = (size_t)off[n_scans] - first;
  if (n_total > 0 && (!pts || !ring || !cls_out)) return fail(h, MSFL_BAD_ARG, "msfl_segment_scans: pts, ring or cls_out is NULL");
  if (masked_out && pts && n_total > 0 && seg_overlap(pts + first, n_total * sizeof(msfl_point), masked_out + first, n_total * sizeof(msfl_point)))
    return fail(h, MSFL_BAD_ARG, "msfl_segment_scans: masked_out overlaps pts");
  hipStream_t st = h->stream;
  SegmentScratch& sg = h->sg;
  const bool host = mem == MSFL_MEM_HOST;

  // tables and offsets.  The device copy of `off` is relative to the arrays the kernels see: a host call stages only [off[0], off[n_scans]).
  const int half = c.n_col / 2, n_tab = seg_tab_size(c.n_col, c.n_row);
  float tab[kSegMaxTab], scalars[4];
  seg_build_tables(c, tab, tab + half, tab + 2 * half, tab + 2 * half + (c.n_row - 1), scalars);
  HIPCHK(h, sg.tab.reserve(kSegMaxTab * sizeof(float)));
  HIPCHK(h, h->pin.upload(sg.tab.p, tab, (size_t)n_tab * sizeof(float), st));
  std::vector<int> rel((size_t)n_scans + 1);
  for (int b = 0; b <= n_scans; b++) rel[b] = host ? off[b] - off[0] : off[b];
  HIPCHK(h, sg.off.reserve(rel.size() * sizeof(int)));
  HIPCHK(h, h->pin.upload(sg.off.p, rel.data(), rel.size() * sizeof(int), st));
  const int* d_off = sg.off.as<int>();

  // staging of a host call
  const float4* d_pts = reinterpret_cast<const float4*>(pts);
  const uint16_t* d_ring = ring;
  uint8_t* d_cls = cls_out;
  int* d_seg = segment_out;
  float4* d_masked = reinterpret_cast<float4*>(masked_out);
  if (host) {
    s = stage_in(h, sg.in_pts, pts ? pts + first : nullptr, n_total, mem, st, &d_pts); if (s) return s;
    s = stage_in(h, sg.in_ring, ring ? ring + first : nullptr, n_total, mem, st, &d_ring); if (s) return s;
    HIPCHK(h, sg.out_cls.reserve(std::max<size_t>(1, n_total)));
    d_cls = sg.out_cls.as<uint8_t>();
    if (segment_out) { HIPCHK(h, sg.out_seg.reserve(std::max<size_t>(1, n_total) * sizeof(int))); d_seg = sg.out_seg.as<int>(); }
    if (masked_out) { HIPCHK(h, sg.out_masked.reserve(std::max<size_t>(1, n_total) * sizeof(float4))); d_masked = sg.out_masked.as<float4>(); }
  }

  // the chunk: as many scans as the budget holds images of
  const int npix = c.n_col * c.n_row;
  int chunk = (int)std::min<size_t>(std::max<size_t>(kSegScratchBudgetBytes / ((size_t)npix * kSegPixelBytes), 1), (size_t)kSegMaxChunkScans);
  if (h->seg_chunk_scans > 0) chunk = std::min(h->seg_chunk_scans, kSegMaxChunkScans);
  chunk = std::min(chunk, n_scans);
  const size_t cells = (size_t)chunk * (size_t)npix;
  HIPCHK(h, sg.img.reserve(cells * kSegPixelBytes));
  HIPCHK(h, sg.ctr.reserve((size_t)chunk * SEG_CTR_WORDS * sizeof(int)));
  if (info) HIPCHK(h, sg.info.reserve((size_t)n_scans * SEG_INFO_WORDS * sizeof(int)));
  SegImages im;
  char* base = sg.img.as<char>();                                   // widest element first: every array stays aligned to its element
  im.key = reinterpret_cast<unsigned long long*>(base);
  im.rows = reinterpret_cast<unsigned*>(base + cells * 8);
  im.ground = reinterpret_cast<int*>(base + cells * 24);
  im.parent = im.ground + cells;
  im.label = im.parent + cells;
  im.count = im.label + cells;
  im.ctr = sg.ctr.as<int>();
  SegCfg k{};
  k.n_col = c.n_col; k.n_row = c.n_row; k.ground_rows = c.ground_rows;
  k.min_points = c.min_points; k.min_points_tall = c.min_points_tall; k.min_rows_tall = c.min_rows_tall; k.keep = c.keep_classes;
  k.min_range = c.min_range; k.max_range = c.max_range;
  k.up[0] = c.up[0]; k.up[1] = c.up[1]; k.up[2] = c.up[2];
  k.hs = scalars[0]; k.hc = scalars[1]; k.g2 = scalars[2]; k.t = scalars[3];
  k.tab = sg.tab.as<float>();

  const int gx_pix = div_up(npix, kSegBlock);
  for (int s0 = 0; s0 < n_scans; s0 += chunk) {
    const int ns = std::min(chunk, n_scans - s0);
    int cmax = 0;
    for (int b = s0; b < s0 + ns; b++) cmax = std::max(cmax, off[b + 1] - off[b]);
    const int gx_pts = std::min(div_up(std::max(cmax, 1), kSegBlock), 1024);
    hipLaunchKernelGGL(seg_clear_kernel, dim3(gx_pix, ns), dim3(kSegBlock), 0, st, im, npix);
    if (cmax > 0) {
      hipLaunchKernelGGL(seg_fill_kernel, dim3(gx_pts, ns), dim3(kSegBlock), 0, st, k, im, d_pts, d_ring, d_off, s0);
      if (c.ground_rows > 0)
        hipLaunchKernelGGL(seg_ground_kernel, dim3(div_up(c.ground_rows * c.n_col, kSegBlock), ns), dim3(kSegBlock), 0, st, k, im, d_pts, d_off, s0);
      hipLaunchKernelGGL(seg_union_kernel, dim3(gx_pix, ns), dim3(kSegBlock), 0, st, k, im);
      hipLaunchKernelGGL(seg_flatten_kernel, dim3(gx_pix, ns), dim3(kSegBlock), 0, st, k, im);
      hipLaunchKernelGGL(seg_classify_kernel, dim3(gx_pts, ns), dim3(kSegBlock), 0, st, k, im, d_pts, d_ring, d_off, s0, d_cls, d_seg, d_masked);
    }
    if (info)
      hipLaunchKernelGGL(seg_finish_kernel, dim3(div_up(ns, kSegBlock)), dim3(kSegBlock), 0, st, (const int*)im.ctr, ns, c.keep_classes,
                         sg.info.as<int>() + (size_t)s0 * SEG_INFO_WORDS);
  }
  HIPCHK(h, hipGetLastError());

  if (host) {
    s = stage_out(h, cls_out ? cls_out + first : nullptr, d_cls, n_total, mem, st); if (s) return s;
    if (segment_out) { s = stage_out(h, segment_out + first, d_seg, n_total, mem, st); if (s) return s; }
    if (masked_out) { s = stage_out(h, masked_out + first, d_masked, n_total, mem, st); if (s) return s; }
  }
  if (info) {
    const size_t bytes = (size_t)n_scans * sizeof(msfl_segment_info);
    HIPCHK(h, h->readback.reserve(bytes));
    HIPCHK(h, hipMemcpyAsync(h->readback.p, sg.info.p, bytes, hipMemcpyDeviceToHost, st));
  }
  if (host || info) HIPCHK(h, hipStreamSynchronize(st));
  if (info) std::memcpy(info, h->readback.p, (size_t)n_scans * sizeof(msfl_segment_info));
  return MSFL_OK;
}

msfl_status msfl_segment_scan(msfl_handle* h, const msfl_point* pts, const uint16_t* ring, int n, const msfl_segment_config* cfg,
                              uint8_t* cls_out, int* segment_out, msfl_point* masked_out, msfl_segment_info* info, msfl_mem mem) {
  if (n < 0) { msfl_status s = enter(h); if (s) return s; return fail(h, MSFL_BAD_ARG, "msfl_segment_scan: n < 0"); }
  const int off[2] = {0, n};
  return msfl_segment_scans(h, 1, pts, ring, off, cfg, cls_out, segment_out, masked_out, info, mem);
}

}  // extern "C"
