// Place recognition — C-ABI entry points msfl_places_*: a device-resident database of polar scan descriptors and its queries.
// Included at the end of msfl_api.hip (shares DevBuf, PinRing, PinBuf and the helper macros); kernels: msfl_place.cuh.
// The object owns its stream and all its memory: it knows nothing of msfl_handle or msfl_slam, and no call here touches theirs.

#include "msfl_place.cuh"

static_assert(sizeof(PlaceRec) == sizeof(msfl_place_match) && sizeof(msfl_place_match) == 24, "place match record layout");

struct msfl_places_s {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  msfl_place_config cfg{};
  std::string last_error;
  int size = 0;                 // entries added so far
  DevBuf tab;                   // e2[n_ring + 1], lo2, bc[n_sector / 2], bs[n_sector / 2]
  DevBuf desc, rkey, nrm;       // capacity x (n_ring x n_sector f32, n_ring int, n_sector f64)
  // scratch of place_describe
  DevBuf pts;                   // float4[points]: staged scans (host mode)
  DevBuf off;                   // int[2 (n_scans + 1)]: [point offsets | chunk offsets]
  DevBuf part;                  // unsigned[chunks x n_ring x n_sector]: per-chunk partial descriptors of scans longer than one chunk
  // scratch of the queries
  DevBuf q_desc, q_rkey, q_nrm; // the described query scans of msfl_places_query, laid out like desc / rkey / nrm
  DevBuf meta;                  // int[3 Q]: [entry of each query | candidates | compared candidates]
  DevBuf keys, list;            // u64[queries per launch x candidates], int[queries per launch x pitch]: the prefilter's keys and its survivors
  DevBuf rec;                   // PlaceRec[queries per launch x pitch]: one record per compared pair
  DevBuf out;                   // PlaceRec[Q x k]: staged results (host mode)
  DevBuf flag;                  // one int: msfl_places_add_descriptors saw a bad value on the device
  PinRing pin;
  PinBuf readback;
};

namespace {

msfl_status fail(msfl_places* p, msfl_status s, const std::string& msg) {
  if (p) p->last_error = msg;
  return s;
}

msfl_status enter(msfl_places* p) {
  if (!p) return MSFL_BAD_ARG;
  HIPCHK(p, hipSetDevice(p->device));
  return MSFL_OK;
}

bool place_config_ok(const msfl_place_config& c) {
  return c.n_ring >= 1 && c.n_ring <= kPlaceMaxRing && c.n_sector >= 2 && c.n_sector <= kPlaceMaxSector && c.n_sector % 2 == 0 &&
         std::isfinite(c.min_range) && std::isfinite(c.max_range) && std::isfinite(c.height_offset) && c.min_range >= 0.0 &&
         c.min_range < c.max_range && c.capacity >= 1;
}

PlaceCfg place_cfg(const msfl_places* p) {
  return PlaceCfg{p->cfg.n_ring, p->cfg.n_sector, (float)p->cfg.height_offset, p->tab.as<float>()};
}

__global__ void place_zero_kernel(int* __restrict__ p, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = 0;
}

// Describes n_scans scans into desc / rkey / nrm (slot b = scan b).  off: n_scans + 1 non-decreasing host offsets, checked by the caller.
msfl_status place_describe(msfl_places* p, const msfl_point* pts, const int* off, int n_scans, msfl_mem mem, float* desc, int* rkey, double* nrm) {
  hipStream_t st = p->stream;
  const int ds = p->cfg.n_ring * p->cfg.n_sector;
  const int p0 = off[0], total = off[n_scans] - p0;
  std::vector<int> offs(2 * (size_t)(n_scans + 1));
  int* po = offs.data(); int* co = po + (n_scans + 1);
  int widest = 1;
  co[0] = 0;
  for (int b = 0; b <= n_scans; b++) {
    po[b] = off[b] - p0;
    if (b == 0) continue;
    const int chunks = std::max(1, div_up(po[b] - po[b - 1], kPlaceChunk));
    co[b] = co[b - 1] + chunks;
    widest = std::max(widest, chunks);
  }
  HIPCHK(p, p->off.reserve(offs.size() * sizeof(int)));
  HIPCHK(p, p->pin.upload(p->off.p, offs.data(), offs.size() * sizeof(int), st));
  const float4* d_pts;
  { const msfl_status s = stage_in(p, p->pts, total ? pts + p0 : pts, (size_t)total, mem, st, &d_pts); if (s) return s; }
  if (widest > 1) HIPCHK(p, p->part.reserve((size_t)co[n_scans] * ds * sizeof(unsigned)));
  const PlaceCfg c = place_cfg(p);
  const size_t lds = ((size_t)ds + place_tab_size(c.nr, c.ns)) * sizeof(unsigned);
  const int* d_off = p->off.as<int>();
  for (int row0 = 0; row0 < n_scans; row0 += 65535)
    hipLaunchKernelGGL(place_describe_kernel, dim3(widest, std::min(65535, n_scans - row0)), dim3(kPlaceBlock), lds, st, c, d_pts, d_off, n_scans,
                       row0, desc, p->part.as<unsigned>());
  hipLaunchKernelGGL(place_finish_kernel, dim3(n_scans), dim3(kPlaceFinishBlock), (size_t)ds * sizeof(float), st, c, d_off, n_scans,
                     (const unsigned*)p->part.as<unsigned>(), desc, rkey, nrm);
  HIPCHK(p, hipGetLastError());
  return MSFL_OK;
}

msfl_status place_check_scans(msfl_places* p, const char* who, const msfl_point* pts, const int* off, int n_scans, msfl_mem mem) {
  const std::string w(who);
  if (n_scans < 0 || (n_scans > 0 && !off) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(p, MSFL_BAD_ARG, w + ": null offset array, negative count or unknown memory kind");
  if (n_scans == 0) return MSFL_OK;
  if (off[0] < 0) return fail(p, MSFL_BAD_ARG, w + ": negative offset");
  for (int b = 1; b <= n_scans; b++)
    if (off[b] < off[b - 1]) return fail(p, MSFL_BAD_ARG, w + ": offsets must be non-decreasing");
  if (off[n_scans] > off[0] && !pts) return fail(p, MSFL_BAD_ARG, w + ": null point array");
  return MSFL_OK;
}

// The query proper.  Query i is entry qidx[i] of (q_desc, q_rkey, q_nrm).
msfl_status place_query(msfl_places* p, const char* who, const float* q_desc, const int* q_rkey, const double* q_nrm, const int* qidx, int Q,
                        const int* max_index, int n_prefilter, int k, msfl_place_match* out, msfl_mem mem) {
  hipStream_t st = p->stream;
  std::vector<int> meta(3 * (size_t)Q);
  int* m_idx = meta.data(); int* m_cand = m_idx + Q; int* m_count = m_cand + Q;
  int widest = 0, most = 0;                  // compared candidates / candidates of the query with the most
  for (int i = 0; i < Q; i++) {
    m_idx[i] = qidx ? qidx[i] : i;
    m_cand[i] = max_index ? max_index[i] : p->size;
    m_count[i] = n_prefilter > 0 ? std::min(n_prefilter, m_cand[i]) : m_cand[i];
    widest = std::max(widest, m_count[i]); most = std::max(most, m_cand[i]);
  }
  HIPCHK(p, p->meta.reserve(meta.size() * sizeof(int)));
  HIPCHK(p, p->pin.upload(p->meta.p, meta.data(), meta.size() * sizeof(int), st));
  // queries per launch: the pair records (and the prefilter's keys) of one launch stay within ~4 M entries
  const int per_query = std::max(1, std::max(widest, n_prefilter > 0 ? most : 0));
  const int qb = std::max(1, std::min(std::min(Q, 65535), (1 << 22) / per_query));
  const int pitch = std::max(1, widest);
  HIPCHK(p, p->rec.reserve((size_t)qb * pitch * sizeof(PlaceRec)));
  if (n_prefilter > 0) {
    HIPCHK(p, p->keys.reserve((size_t)qb * std::max(1, most) * sizeof(unsigned long long)));
    HIPCHK(p, p->list.reserve((size_t)qb * pitch * sizeof(int)));
  }
  PlaceRec* d_out = reinterpret_cast<PlaceRec*>(out);
  if (mem == MSFL_MEM_HOST) {
    HIPCHK(p, p->out.reserve((size_t)Q * k * sizeof(PlaceRec)));
    d_out = p->out.as<PlaceRec>();
  }
  const PlaceCfg c = place_cfg(p);
  PlaceQuery j{};
  j.q_desc = q_desc; j.q_rkey = q_rkey; j.q_nrm = q_nrm;
  j.db_desc = p->desc.as<float>(); j.db_rkey = p->rkey.as<int>(); j.db_nrm = p->nrm.as<double>();
  j.qidx = p->meta.as<int>(); j.ncand = j.qidx + Q; j.count = j.ncand + Q;
  j.pitch = pitch;
  j.list = n_prefilter > 0 ? p->list.as<int>() : nullptr;
  const size_t lds = ((size_t)(2 + kPlaceShiftTile) * c.ns) * sizeof(double) + 2 * (size_t)c.nr * c.ns * sizeof(float);
  for (int q0 = 0; q0 < Q; q0 += qb) {
    const int nq = std::min(qb, Q - q0);
    j.q0 = q0;
    if (n_prefilter > 0 && widest > 0)
      hipLaunchKernelGGL(place_prefilter_kernel, dim3(nq), dim3(kPlaceBlock), 0, st, c, j, p->keys.as<unsigned long long>(), std::max(1, most),
                         p->list.as<int>());
    if (widest > 0)
      hipLaunchKernelGGL(place_match_kernel, dim3(widest, nq), dim3(kPlaceBlock), lds, st, c, j, p->rec.as<PlaceRec>());
    hipLaunchKernelGGL(place_topk_kernel, dim3(nq), dim3(kPlaceBlock), 0, st, j, (const PlaceRec*)p->rec.as<PlaceRec>(), k, d_out);
  }
  HIPCHK(p, hipGetLastError());
  { const msfl_status s = stage_out(p, out, d_out, (size_t)Q * k, mem, st); if (s) return s; }
  if (mem == MSFL_MEM_HOST) HIPCHK(p, hipStreamSynchronize(st));
  (void)who;
  return MSFL_OK;
}

msfl_status place_check_query(msfl_places* p, const char* who, int n_queries, const int* max_index, int n_prefilter, int k, const void* out,
                              msfl_mem mem) {
  const std::string w(who);
  if (n_queries < 0 || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE)) return fail(p, MSFL_BAD_ARG, w + ": negative count or unknown memory kind");
  if (k < 1 || k > kPlaceMaxK) return fail(p, MSFL_BAD_ARG, w + ": k must be in [1, 64]");
  if (n_prefilter < 0) return fail(p, MSFL_BAD_ARG, w + ": negative n_prefilter");
  if (n_queries > 0 && !out) return fail(p, MSFL_BAD_ARG, w + ": null result array");
  if (max_index)
    for (int i = 0; i < n_queries; i++)
      if (max_index[i] < 0 || max_index[i] > p->size) return fail(p, MSFL_BAD_ARG, w + ": a max_index outside [0, size]");
  return MSFL_OK;
}

}  // namespace

extern "C" {

void msfl_places_default_config(msfl_place_config* c) {
  if (!c) return;
  c->n_ring = 20; c->n_sector = 60;
  c->min_range = 0.3; c->max_range = 80.0; c->height_offset = 2.0;
  c->capacity = 16384;
}

msfl_status msfl_places_create(const msfl_place_config* cfg, int device, msfl_places** out) {
  if (!out) return MSFL_BAD_ARG;
  *out = nullptr;
  msfl_place_config c;
  if (cfg) c = *cfg; else msfl_places_default_config(&c);
  if (!place_config_ok(c)) return MSFL_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSFL_HIP_ERROR;   // no GPU: fail loudly, no fallback
  if (device < 0 || device >= ndev) return MSFL_BAD_ARG;
  msfl_places* p = new msfl_places_s();
  p->device = device; p->cfg = c;
  // the tables, in double, each entry rounded to f32 once
  const int nr = c.n_ring, ns = c.n_sector, half = ns / 2;
  std::vector<float> tab((size_t)place_tab_size(nr, ns));
  for (int k = 0; k <= nr; k++) { const double e = (double)k * c.max_range / (double)nr; tab[k] = (float)(e * e); }
  tab[nr + 1] = (float)(c.min_range * c.min_range);
  for (int k = 0; k < half; k++) {
    const double a = 2.0 * 3.141592653589793238462643383279502884 * (double)k / (double)ns;
    tab[nr + 2 + k] = (float)std::cos(a); tab[nr + 2 + half + k] = (float)std::sin(a);
  }
  const size_t ds = (size_t)nr * ns;
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && p->tab.reserve(tab.size() * sizeof(float)) == hipSuccess && p->desc.reserve((size_t)c.capacity * ds * sizeof(float)) == hipSuccess &&
       p->rkey.reserve((size_t)c.capacity * nr * sizeof(int)) == hipSuccess && p->nrm.reserve((size_t)c.capacity * ns * sizeof(double)) == hipSuccess &&
       p->flag.reserve(sizeof(int)) == hipSuccess && p->readback.reserve(sizeof(int)) == hipSuccess;
  ok = ok && hipMemcpy(p->tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { msfl_places_destroy(p); return MSFL_HIP_ERROR; }
  p->stream = p->own_stream;
  *out = p;
  return MSFL_OK;
}

void msfl_places_destroy(msfl_places* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
  delete p;                               // every DevBuf / PinBuf member and the pinned ring free themselves
}

msfl_status msfl_places_set_stream(msfl_places* p, void* hip_stream) {
  msfl_status s = enter(p); if (s) return s;
  HIPCHK(p, hipStreamSynchronize(p->stream));
  p->stream = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = HIP null stream
  return MSFL_OK;
}

msfl_status msfl_places_synchronize(msfl_places* p) {
  msfl_status s = enter(p); if (s) return s;
  HIPCHK(p, hipStreamSynchronize(p->stream));
  return MSFL_OK;
}

int msfl_places_size(const msfl_places* p) { return p ? p->size : 0; }

const char* msfl_places_last_error(const msfl_places* p) { return p ? p->last_error.c_str() : "null places object"; }

msfl_status msfl_places_add(msfl_places* p, const msfl_point* pts, const int* off, int n_scans, msfl_mem mem, int* first_index) {
  msfl_status s = enter(p); if (s) return s;
  s = place_check_scans(p, "msfl_places_add", pts, off, n_scans, mem); if (s) return s;
  if ((long long)p->size + n_scans > p->cfg.capacity) return fail(p, MSFL_CAPACITY, "msfl_places_add: the batch does not fit the capacity; nothing added");
  if (first_index) *first_index = p->size;
  if (n_scans == 0) return MSFL_OK;
  const size_t at = (size_t)p->size;
  s = place_describe(p, pts, off, n_scans, mem, p->desc.as<float>() + at * p->cfg.n_ring * p->cfg.n_sector, p->rkey.as<int>() + at * p->cfg.n_ring,
                     p->nrm.as<double>() + at * p->cfg.n_sector);
  if (s) return s;
  if (mem == MSFL_MEM_HOST) HIPCHK(p, hipStreamSynchronize(p->stream));
  p->size += n_scans;
  return MSFL_OK;
}

msfl_status msfl_places_add_descriptors(msfl_places* p, const float* desc, int n, msfl_mem mem, int* first_index) {
  msfl_status s = enter(p); if (s) return s;
  if (n < 0 || (n > 0 && !desc) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(p, MSFL_BAD_ARG, "msfl_places_add_descriptors: null array, negative count or unknown memory kind");
  if ((long long)p->size + n > p->cfg.capacity)
    return fail(p, MSFL_CAPACITY, "msfl_places_add_descriptors: the batch does not fit the capacity; nothing added");
  if (first_index) *first_index = p->size;
  if (n == 0) return MSFL_OK;
  hipStream_t st = p->stream;
  const size_t ds = (size_t)p->cfg.n_ring * p->cfg.n_sector, count = (size_t)n * ds, at = (size_t)p->size;
  if (mem == MSFL_MEM_HOST) {
    for (size_t i = 0; i < count; i++)
      if (!(desc[i] >= 0.f && std::isfinite(desc[i]))) return fail(p, MSFL_BAD_ARG, "msfl_places_add_descriptors: a value is negative or not finite; nothing added");
  } else {                                // checked on the device before anything is stored: the whole add is refused
    int* flag = p->flag.as<int>();
    hipLaunchKernelGGL(place_zero_kernel, dim3(1), dim3(64), 0, st, flag, 1);
    hipLaunchKernelGGL(place_check_kernel, dim3((unsigned)((count + kPlaceBlock - 1) / kPlaceBlock)), dim3(kPlaceBlock), 0, st, desc, count, flag);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipMemcpyAsync(p->readback.p, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(p, hipStreamSynchronize(st));
    if (*p->readback.as<int>() != 0) return fail(p, MSFL_BAD_ARG, "msfl_places_add_descriptors: a value is negative or not finite; nothing added");
  }
  float* dst = p->desc.as<float>() + at * ds;
  HIPCHK(p, hipMemcpyAsync(dst, desc, count * sizeof(float), mem == MSFL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(place_finish_kernel, dim3(n), dim3(kPlaceFinishBlock), ds * sizeof(float), st, place_cfg(p), (const int*)nullptr, n,
                     (const unsigned*)nullptr, dst, p->rkey.as<int>() + at * p->cfg.n_ring, p->nrm.as<double>() + at * p->cfg.n_sector);
  HIPCHK(p, hipGetLastError());
  if (mem == MSFL_MEM_HOST) HIPCHK(p, hipStreamSynchronize(st));
  p->size += n;
  return MSFL_OK;
}

msfl_status msfl_places_get(msfl_places* p, int first, int n, float* desc_out, int* ring_key_out, msfl_mem mem) {
  msfl_status s = enter(p); if (s) return s;
  if (first < 0 || n < 0 || (long long)first + n > p->size || (n > 0 && !desc_out) || (mem != MSFL_MEM_HOST && mem != MSFL_MEM_DEVICE))
    return fail(p, MSFL_BAD_ARG, "msfl_places_get: range outside [0, size], null array or unknown memory kind");
  if (n == 0) return MSFL_OK;
  hipStream_t st = p->stream;
  const size_t ds = (size_t)p->cfg.n_ring * p->cfg.n_sector, nr = (size_t)p->cfg.n_ring;
  const hipMemcpyKind kind = mem == MSFL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIPCHK(p, hipMemcpyAsync(desc_out, p->desc.as<float>() + (size_t)first * ds, (size_t)n * ds * sizeof(float), kind, st));
  if (ring_key_out) HIPCHK(p, hipMemcpyAsync(ring_key_out, p->rkey.as<int>() + (size_t)first * nr, (size_t)n * nr * sizeof(int), kind, st));
  if (mem == MSFL_MEM_HOST) HIPCHK(p, hipStreamSynchronize(st));
  return MSFL_OK;
}

msfl_status msfl_places_query(msfl_places* p, const msfl_point* pts, const int* off, int n_queries, const int* max_index, int n_prefilter, int k,
                              msfl_place_match* out, msfl_mem mem) {
  msfl_status s = enter(p); if (s) return s;
  s = place_check_query(p, "msfl_places_query", n_queries, max_index, n_prefilter, k, out, mem); if (s) return s;
  s = place_check_scans(p, "msfl_places_query", pts, off, n_queries, mem); if (s) return s;
  if (n_queries == 0) return MSFL_OK;
  const size_t ds = (size_t)p->cfg.n_ring * p->cfg.n_sector;
  HIPCHK(p, p->q_desc.reserve((size_t)n_queries * ds * sizeof(float)));
  HIPCHK(p, p->q_rkey.reserve((size_t)n_queries * p->cfg.n_ring * sizeof(int)));
  HIPCHK(p, p->q_nrm.reserve((size_t)n_queries * p->cfg.n_sector * sizeof(double)));
  s = place_describe(p, pts, off, n_queries, mem, p->q_desc.as<float>(), p->q_rkey.as<int>(), p->q_nrm.as<double>());
  if (s) return s;
  return place_query(p, "msfl_places_query", p->q_desc.as<float>(), p->q_rkey.as<int>(), p->q_nrm.as<double>(), nullptr, n_queries,
                     max_index, n_prefilter, k, out, mem);
}

msfl_status msfl_places_query_entries(msfl_places* p, const int* entries, int n_queries, const int* max_index, int n_prefilter, int k,
                                      msfl_place_match* out, msfl_mem mem) {
  msfl_status s = enter(p); if (s) return s;
  s = place_check_query(p, "msfl_places_query_entries", n_queries, max_index, n_prefilter, k, out, mem); if (s) return s;
  if (n_queries > 0 && !entries) return fail(p, MSFL_BAD_ARG, "msfl_places_query_entries: null entry array");
  for (int i = 0; i < n_queries; i++)
    if (entries[i] < 0 || entries[i] >= p->size) return fail(p, MSFL_BAD_ARG, "msfl_places_query_entries: an entry index outside the database");
  if (n_queries == 0) return MSFL_OK;
  return place_query(p, "msfl_places_query_entries", p->desc.as<float>(), p->rkey.as<int>(), p->nrm.as<double>(), entries, n_queries, max_index,
                     n_prefilter, k, out, mem);
}

}  // extern "C"
