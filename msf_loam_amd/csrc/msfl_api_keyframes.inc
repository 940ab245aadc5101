// Keyframe store — C-ABI entry points msfl_keyframes_*: the scans themselves kept on the device (two pools of 16-byte points, one per
// feature kind) and laid down at any poses as submaps (compose) or into map stores (insert).  Included at the end of msfl_api.hip
// (shares its handle, DevBuf, PinRing, PinBuf and helper macros; msfl_grid_s for insert).  Kernel: msfl_keyframes.cuh; the host
// bookkeeping (validation, member table, totals, launch shape): msfl_keyframes_host.h.  A store works on its handle's stream, like a
// map store, and owns every buffer it uses: the matchers' scratch on the handle is never touched.

static_assert(kKfOk == MSFL_OK && kKfBadArg == MSFL_BAD_ARG && kKfCapacity == MSFL_CAPACITY, "msfl_keyframes_host.h hands out msfl_status values");
static_assert(sizeof(KfRec) == 16 && sizeof(msfl_point) == sizeof(float4), "record layout");

struct msfl_keyframes_s {
  msfl_handle* h = nullptr;
  msfl_keyframes_config cfg{};
  KfIndex ix;                      // counts and pool positions: nothing ever reads a size back from the device
  DevBuf pool[2];                  // float4[max_corner_points], float4[max_surf_points], fixed at creation
  DevBuf gather[2];                // compose with a leaf: the kind's transformed clouds before the voxel filter.  add: [0] holds both lists
  DevBuf vout[2];                  // filtered or transformed points on their way to the host or the pool; insert: the transformed keyframe
  DevBuf table;                    // one launch's member table: double[8 M] poses, KfRec[M] corner, KfRec[M] surf
  DevBuf flag;                     // int[4]: the gather kernel's flag, then the two list counts of an add (the voxel pair form reads them)
  DevBuf iota;                     // int[iota_n] = 0, 1, 2 ...: the index lists the voxel pair form wants over an add's two lists
  size_t iota_n = 0;
  PinBuf stage;                    // host lists of an add, gathered and checked here, then copied asynchronously
  hipEvent_t stage_ev = nullptr;   // that copy has run
  bool stage_pending = false;
  PinBuf flag_rb;                  // one int
};

namespace {

msfl_status kf_fail(msfl_keyframes* k, int s, const char* who, const char* why) {
  return fail(k->h, (msfl_status)s, std::string(who) + ": " + why);
}

// upload the plan's table (one copy) and run the gather kernel over its members, both kinds
msfl_status kf_launch(msfl_keyframes* k, const KfPlan& plan, KfGatherArgs a) {
  msfl_handle* h = k->h;
  const int M = plan.n_members;
  if (M <= 0 || plan.max_count <= 0) return MSFL_OK;
  const size_t pose_bytes = (size_t)M * 8 * sizeof(double), rec_bytes = (size_t)M * sizeof(KfRec);
  std::vector<unsigned char> tab(pose_bytes + 2 * rec_bytes);
  std::memcpy(tab.data(), plan.poses.data(), pose_bytes);
  std::memcpy(tab.data() + pose_bytes, plan.rec[0].data(), rec_bytes);
  std::memcpy(tab.data() + pose_bytes + rec_bytes, plan.rec[1].data(), rec_bytes);
  HIPCHK(h, k->table.reserve(tab.size()));
  HIPCHK(h, h->pin.upload(k->table.p, tab.data(), tab.size(), h->stream));
  a.poses = k->table.as<double>();
  a.kind[0].rec = reinterpret_cast<const KfRec*>(k->table.as<unsigned char>() + pose_bytes);
  a.kind[1].rec = reinterpret_cast<const KfRec*>(k->table.as<unsigned char>() + pose_bytes + rec_bytes);
  a.bad = k->flag.as<int>();
  for (int base = 0; base < M; base += kKfMaxGridY) {
    const KfGrid g = kf_grid_shape(plan.max_count, M - base);
    a.member_base = base;
    hipLaunchKernelGGL(kf_gather_kernel, dim3(g.x, g.y, g.z), dim3(256), 0, h->stream, a);
  }
  HIPCHK(h, hipGetLastError());
  return MSFL_OK;
}

// a plan of one member whose two lists start at src[k] and hold n[k] points (a kind with n = 0 launches workgroups that leave at once)
void kf_plan_one(KfPlan* plan, const int src[2], const int n[2], int flags, const double* pose7) {
  plan->n_members = 1;
  plan->poses.assign(8, 0.0);
  if (pose7) std::copy(pose7, pose7 + 7, plan->poses.begin());
  for (int k = 0; k < 2; k++) { plan->rec[k].assign(1, KfRec{src[k], n[k], 0, flags}); plan->total[k] = n[k]; }
  plan->max_count = std::max(n[0], n[1]);
}

msfl_status kf_iota(msfl_keyframes* k, size_t n) {
  if (n <= k->iota_n) return MSFL_OK;
  msfl_handle* h = k->h;
  const size_t want = std::max(n, k->iota_n + k->iota_n / 2);
  HIPCHK(h, hipStreamSynchronize(h->stream));          // queued filters may still read the old list
  HIPCHK(h, k->iota.reserve(want * sizeof(int)));
  std::vector<int> v(want);
  for (size_t i = 0; i < want; i++) v[i] = (int)i;
  HIPCHK(h, h->pin.upload(k->iota.p, v.data(), want * sizeof(int), h->stream));
  k->iota_n = want;
  return MSFL_OK;
}

}  // namespace

extern "C" {

void msfl_keyframes_default_config(msfl_keyframes_config* c) {
  if (!c) return;
  c->max_keyframes = 4096;
  c->max_corner_points = 4194304;
  c->max_surf_points = 16777216;
  c->leaf_corner = 0.2f;
  c->leaf_surf = 0.4f;
}

msfl_status msfl_keyframes_create(msfl_handle* h, const msfl_keyframes_config* c, msfl_keyframes** out) {
  msfl_status s = enter(h); if (s) return s;
  if (!out) return fail(h, MSFL_BAD_ARG, "msfl_keyframes_create: bad argument");
  msfl_keyframes_config cfg;
  msfl_keyframes_default_config(&cfg);
  if (c) cfg = *c;
  if (cfg.max_keyframes < 1 || cfg.max_corner_points < 0 || cfg.max_surf_points < 0 || !kf_leaf_ok(cfg.leaf_corner) || !kf_leaf_ok(cfg.leaf_surf))
    return fail(h, MSFL_BAD_ARG, "msfl_keyframes_create: max_keyframes < 1, a negative pool size, or a leaf that is negative or not finite");
  msfl_keyframes* k = new msfl_keyframes_s();
  k->h = h;
  k->cfg = cfg;
  const hipError_t e[] = {k->pool[0].reserve(std::max<size_t>(1, (size_t)cfg.max_corner_points) * sizeof(float4)),
                          k->pool[1].reserve(std::max<size_t>(1, (size_t)cfg.max_surf_points) * sizeof(float4)), k->flag.reserve(4 * sizeof(int)),
                          k->flag_rb.reserve(sizeof(int)), hipEventCreateWithFlags(&k->stage_ev, hipEventDisableTiming)};
  for (hipError_t x : e)
    if (x != hipSuccess) {
      if (k->stage_ev) (void)hipEventDestroy(k->stage_ev);
      delete k;
      return fail(h, MSFL_HIP_ERROR, std::string("msfl_keyframes_create: ") + hipGetErrorString(x));
    }
  *out = k;
  return MSFL_OK;
}

void msfl_keyframes_destroy(msfl_keyframes* k) {
  if (!k) return;
  (void)hipSetDevice(k->h->device);
  (void)hipStreamSynchronize(k->h->stream);
  if (k->stage_ev) (void)hipEventDestroy(k->stage_ev);
  delete k;
}

int msfl_keyframes_size(const msfl_keyframes* k) { return k ? k->ix.size() : 0; }

msfl_status msfl_keyframes_add(msfl_keyframes* k, const msfl_point* corner, const int* corner_idx, int n_corner, const msfl_point* surf,
                               const int* surf_idx, int n_surf, msfl_mem mem, int* index) {
  if (!k) return MSFL_BAD_ARG;
  msfl_handle* h = k->h;
  msfl_status s = enter(h); if (s) return s;
  const char* who = "msfl_keyframes_add";
  if (n_corner < 0 || n_surf < 0 || (n_corner > 0 && !corner) || (n_surf > 0 && !surf)) return kf_fail(k, MSFL_BAD_ARG, who, "bad argument");
  hipStream_t st = h->stream;
  const int n[2] = {n_corner, n_surf};
  const msfl_point* pts[2] = {corner, surf};
  const int* idx[2] = {corner_idx, surf_idx};
  const float leaf[2] = {k->cfg.leaf_corner, k->cfg.leaf_surf};
  const bool filt[2] = {leaf[0] > 0.f && n[0] > 0, leaf[1] > 0.f && n[1] > 0};
  const long long pool_cap[2] = {k->cfg.max_corner_points, k->cfg.max_surf_points};
  const char* why = "";
  // lists stored as given must fit now; filtered ones are checked again at their filtered size
  int rc = kf_check_add(k->ix, k->cfg.max_keyframes, pool_cap, filt[0] ? 0 : n[0], filt[1] ? 0 : n[1], &why);
  if (rc) return kf_fail(k, rc, who, why);
  // where each list goes on the device: the pool's top (stored as given), or gather[0] = [corner | surf] (to be filtered)
  const size_t g_off[2] = {0, filt[0] ? (size_t)n[0] : 0};
  const size_t g_n = (filt[0] ? (size_t)n[0] : 0) + (filt[1] ? (size_t)n[1] : 0);
  if (g_n > 0) HIPCHK(h, k->gather[0].reserve(g_n * sizeof(float4)));
  float4* dst[2];
  for (int c = 0; c < 2; c++) dst[c] = filt[c] ? k->gather[0].as<float4>() + g_off[c] : k->pool[c].as<float4>() + k->ix.top[c];
  if (mem == MSFL_MEM_HOST) {
    // gathered and checked in pinned memory, then copied asynchronously: the caller's arrays are free when the call returns
    if (k->stage_pending) { HIPCHK(h, hipEventSynchronize(k->stage_ev)); k->stage_pending = false; }
    HIPCHK(h, k->stage.reserve(std::max<size_t>(1, (size_t)n[0] + (size_t)n[1]) * sizeof(float4)));
    float* sp[2] = {k->stage.as<float>(), k->stage.as<float>() + 4 * (size_t)n[0]};
    for (int c = 0; c < 2; c++) {
      const float* p = reinterpret_cast<const float*>(pts[c]);
      if (idx[c]) for (int i = 0; i < n[c]; i++) std::memcpy(sp[c] + 4 * (size_t)i, p + 4 * (size_t)idx[c][i], sizeof(float4));
      else if (n[c] > 0) std::memcpy(sp[c], p, (size_t)n[c] * sizeof(float4));
      if (kf_first_non_finite(sp[c], nullptr, n[c]) >= 0)
        return kf_fail(k, MSFL_BAD_ARG, who, c == 0 ? "a corner point that is not finite; nothing added" : "a surf point that is not finite; nothing added");
    }
    for (int c = 0; c < 2; c++)
      if (n[c] > 0) HIPCHK(h, hipMemcpyAsync(dst[c], sp[c], (size_t)n[c] * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipEventRecord(k->stage_ev, st));
    k->stage_pending = true;
  } else if (n[0] + (long long)n[1] > 0) {
    // one launch gathers both lists (through their index lists, if any) and checks them on the way
    HIPCHK(h, hipMemsetAsync(k->flag.p, 0, sizeof(int), st));
    KfPlan plan;
    const int zero[2] = {0, 0};
    kf_plan_one(&plan, zero, n, kKfCopy | kKfCheckFinite, nullptr);
    KfGatherArgs a{};
    for (int c = 0; c < 2; c++) { a.kind[c].src = reinterpret_cast<const float4*>(pts[c]); a.kind[c].idx = idx[c]; a.kind[c].dst = dst[c]; }
    s = kf_launch(k, plan, a); if (s) return s;
    HIPCHK(h, hipMemcpyAsync(k->flag_rb.p, k->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  int m[2] = {n[0], n[1]};
  if (g_n > 0) {
    // the stored list is what msfl_voxel_downsample returns for it; both filters share one synchronisation (the batch pair form:
    // one cloud [corner | surf] with two index lists over it)
    HIPCHK(h, k->vout[0].reserve(g_n * sizeof(float4)));
    msfl_point* g = reinterpret_cast<msfl_point*>(k->gather[0].p);
    msfl_point* vo = reinterpret_cast<msfl_point*>(k->vout[0].p);
    int oo[2][2] = {{0, 0}, {0, 0}};
    if (filt[0] && filt[1]) {
      s = kf_iota(k, g_n); if (s) return s;
      HIPCHK(h, h->pin.upload(k->flag.as<int>() + 1, n, 2 * sizeof(int), st));
      const int off[2] = {0, (int)g_n};
      const int* it = k->iota.as<int>();
      const int* cnt = k->flag.as<int>() + 1;
      s = msfl_voxel_downsample_batch_pair(h, 1, g, off, it, cnt, leaf[0], vo, oo[0], it + n[0], cnt + 1, leaf[1], vo + n[0], oo[1], MSFL_MEM_DEVICE);
    } else {
      const int c = filt[0] ? 0 : 1;
      const int off[2] = {0, n[c]};
      s = msfl_voxel_downsample_batch(h, 1, g, nullptr, off, nullptr, leaf[c], vo, oo[c], MSFL_MEM_DEVICE);
    }
    for (int c = 0; c < 2; c++) if (filt[c]) m[c] = oo[c][1];
  } else if (mem != MSFL_MEM_HOST) {
    HIPCHK(h, hipStreamSynchronize(st));
  }
  // (the filter has synchronised, whatever it returned: the gather launch's flag is on the host)
  if (mem != MSFL_MEM_HOST && n[0] + (long long)n[1] > 0 && *k->flag_rb.as<int>() != 0)
    return kf_fail(k, MSFL_BAD_ARG, who, "a point that is not finite; nothing added");
  if (s) return s;                                       // a leaf too small for the list's extent: the filter's status; nothing added
  rc = kf_check_add(k->ix, k->cfg.max_keyframes, pool_cap, m[0], m[1], &why);
  if (rc) return kf_fail(k, rc, who, why);
  for (int c = 0; c < 2; c++)
    if (filt[c] && m[c] > 0)
      HIPCHK(h, hipMemcpyAsync(k->pool[c].as<float4>() + k->ix.top[c], k->vout[0].as<float4>() + g_off[c], (size_t)m[c] * sizeof(float4),
                               hipMemcpyDeviceToDevice, st));
  if (index) *index = k->ix.size();
  kf_commit_add(&k->ix, m[0], m[1]);
  return MSFL_OK;
}

msfl_status msfl_keyframes_sizes(msfl_keyframes* k, int first, int n, int* n_corner, int* n_surf) {
  if (!k) return MSFL_BAD_ARG;
  if (first < 0 || n < 0 || (long long)first + n > k->ix.size()) return kf_fail(k, MSFL_BAD_ARG, "msfl_keyframes_sizes", "a range outside the keyframes");
  for (int i = 0; i < n; i++) {
    if (n_corner) n_corner[i] = k->ix.count[kKfCorner][first + i];
    if (n_surf) n_surf[i] = k->ix.count[kKfSurf][first + i];
  }
  return MSFL_OK;
}

msfl_status msfl_keyframes_get(msfl_keyframes* k, int index, msfl_point* corner, int cap_corner, msfl_point* surf, int cap_surf, msfl_mem mem) {
  if (!k) return MSFL_BAD_ARG;
  msfl_handle* h = k->h;
  msfl_status s = enter(h); if (s) return s;
  const char* who = "msfl_keyframes_get";
  if (index < 0 || index >= k->ix.size()) return kf_fail(k, MSFL_BAD_ARG, who, "an index that is no keyframe");
  msfl_point* out[2] = {corner, surf};
  const int cap[2] = {cap_corner, cap_surf};
  for (int c = 0; c < 2; c++)
    if (out[c] && cap[c] < k->ix.count[c][index]) return kf_fail(k, MSFL_CAPACITY, who, "an output capacity below the list's size (msfl_keyframes_sizes)");
  bool copied = false;
  for (int c = 0; c < 2; c++) {                          // a null pointer: that list is not wanted
    const int cnt = k->ix.count[c][index];
    if (!out[c] || cnt == 0) continue;
    HIPCHK(h, hipMemcpyAsync(out[c], k->pool[c].as<float4>() + k->ix.start[c][index], (size_t)cnt * sizeof(float4),
                             mem == MSFL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    copied = true;
  }
  if (copied && mem == MSFL_MEM_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  return MSFL_OK;
}

msfl_status msfl_keyframes_compose(msfl_keyframes* k, int n_submaps, const int* member_off, const int* keys, const double* poses, float leaf_corner,
                                   float leaf_surf, msfl_point* out_corner, int cap_corner, int* out_corner_off, msfl_point* out_surf, int cap_surf,
                                   int* out_surf_off, msfl_mem mem) {
  if (!k) return MSFL_BAD_ARG;
  msfl_handle* h = k->h;
  msfl_status s = enter(h); if (s) return s;
  const char* who = "msfl_keyframes_compose";
  if (!out_corner_off || !out_surf_off || cap_corner < 0 || cap_surf < 0) return kf_fail(k, MSFL_BAD_ARG, who, "bad argument");
  KfPlan plan;
  const char* why = "";
  const int rc = kf_plan_compose(k->ix, n_submaps, member_off, keys, poses, leaf_corner, leaf_surf, cap_corner, cap_surf, &plan, &why);
  if (rc) return kf_fail(k, rc, who, why);
  msfl_point* out[2] = {out_corner, out_surf};
  int* out_off[2] = {out_corner_off, out_surf_off};
  const float leaf[2] = {leaf_corner, leaf_surf};
  for (int c = 0; c < 2; c++)
    if (plan.total[c] > 0 && !out[c]) return kf_fail(k, MSFL_BAD_ARG, who, "a null output for a kind that has points");
  hipStream_t st = h->stream;
  const int B = n_submaps;
  bool filt[2];
  KfGatherArgs a{};
  for (int c = 0; c < 2; c++) {
    filt[c] = leaf[c] > 0.f && plan.total[c] > 0;
    const size_t bytes = (size_t)plan.total[c] * sizeof(float4);
    a.kind[c].src = k->pool[c].as<float4>();
    if (filt[c]) { HIPCHK(h, k->gather[c].reserve(bytes)); a.kind[c].dst = k->gather[c].as<float4>(); }
    else if (mem == MSFL_MEM_HOST) { HIPCHK(h, k->vout[c].reserve(std::max<size_t>(bytes, 1))); a.kind[c].dst = k->vout[c].as<float4>(); }
    else a.kind[c].dst = reinterpret_cast<float4*>(out[c]);
  }
  s = kf_launch(k, plan, a); if (s) return s;
  bool copying = false;
  msfl_status first_error = MSFL_OK;
  for (int c = 0; c < 2; c++) {
    if (!filt[c]) {
      std::copy(plan.off[c].begin(), plan.off[c].end(), out_off[c]);
      if (mem == MSFL_MEM_HOST && plan.total[c] > 0) {
        HIPCHK(h, hipMemcpyAsync(out[c], k->vout[c].p, (size_t)plan.total[c] * sizeof(float4), hipMemcpyDeviceToHost, st));
        copying = true;
      }
      continue;
    }
    // the existing batch filter over the gather buffer (it synchronises to deliver the boundaries)
    msfl_point* vo = out[c];
    if (mem == MSFL_MEM_HOST) { HIPCHK(h, k->vout[c].reserve((size_t)plan.total[c] * sizeof(float4))); vo = reinterpret_cast<msfl_point*>(k->vout[c].p); }
    const msfl_status sv = msfl_voxel_downsample_batch(h, B, reinterpret_cast<const msfl_point*>(k->gather[c].p), nullptr, plan.off[c].data(), nullptr,
                                                       leaf[c], vo, out_off[c], MSFL_MEM_DEVICE);
    if (sv && !first_error) first_error = sv;
    if (mem == MSFL_MEM_HOST && out_off[c][B] > 0) {
      HIPCHK(h, hipMemcpyAsync(out[c], vo, (size_t)out_off[c][B] * sizeof(float4), hipMemcpyDeviceToHost, st));
      copying = true;
    }
  }
  if (copying) HIPCHK(h, hipStreamSynchronize(st));
  return first_error;
}

msfl_status msfl_keyframes_insert(msfl_keyframes* k, const int* keys, const double* poses, int n, msfl_grid* grid_corner, msfl_grid* grid_surf,
                                  int* n_done) {
  if (n_done) *n_done = 0;
  if (!k) return MSFL_BAD_ARG;
  msfl_handle* h = k->h;
  msfl_status s = enter(h); if (s) return s;
  const char* who = "msfl_keyframes_insert";
  if (n < 0 || (n > 0 && (!keys || !poses))) return kf_fail(k, MSFL_BAD_ARG, who, "bad argument");
  msfl_grid* grids[2] = {grid_corner, grid_surf};
  for (msfl_grid* g : grids)
    if (g && g->h != h) return kf_fail(k, MSFL_BAD_ARG, who, "a map store of another handle");
  const char* why = "";
  const int rc = kf_check_members(k->ix.size(), keys, poses, 0, n, &why);
  if (rc) return kf_fail(k, rc, who, why);
  hipStream_t st = h->stream;
  for (int i = 0; i < n; i++) {
    // one member through the gather kernel into scratch, checked on the way against what each store would refuse, so that a refused
    // keyframe reaches neither store; then the existing insert, once per store
    int cnt[2], src[2];
    KfGatherArgs a{};
    for (int c = 0; c < 2; c++) {
      cnt[c] = grids[c] ? k->ix.count[c][keys[i]] : 0;
      src[c] = k->ix.start[c][keys[i]];
      HIPCHK(h, k->vout[c].reserve(std::max<size_t>(1, (size_t)cnt[c]) * sizeof(float4)));
      a.kind[c].src = k->pool[c].as<float4>();
      a.kind[c].dst = k->vout[c].as<float4>();
      if (grids[c]) a.kind[c].grid = grids[c]->d;
    }
    if (cnt[0] + (long long)cnt[1] > 0) {
      KfPlan plan;
      kf_plan_one(&plan, src, cnt, kKfCheckCell, poses + 7 * (size_t)i);
      HIPCHK(h, hipMemsetAsync(k->flag.p, 0, sizeof(int), st));
      s = kf_launch(k, plan, a); if (s) return s;
      HIPCHK(h, hipMemcpyAsync(k->flag_rb.p, k->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      if (*k->flag_rb.as<int>() != 0)
        return kf_fail(k, MSFL_CAPACITY, who, "a keyframe with a point outside +-8192 cells of a store (or not finite there); it is in neither store");
      for (int c = 0; c < 2; c++) {
        if (cnt[c] == 0) continue;
        s = msfl_grid_insert_scan(grids[c], reinterpret_cast<const msfl_point*>(k->vout[c].p), cnt[c], MSFL_MEM_DEVICE);
        if (s) return s;
      }
    }
    if (n_done) *n_done = i + 1;
  }
  return MSFL_OK;
}

}  // extern "C"
