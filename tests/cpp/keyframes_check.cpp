// The keyframe store through its C++ face (include/msfl/keyframes.hpp): Add, Sizes, Get, ComposeSubmaps against points transformed
// here, InsertInto against msfl_transform_cloud + msfl_grid_insert_scan.  Also names every new C declaration of
// include/msfl_c_api.h, so that compiling this file checks them (tests/test_keyframes_model.py compiles it on the CPU and runs it on
// the GPU; tests/cpp/Makefile does not know it).  Exit status 0: all checks hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "msfl/keyframes.hpp"

static_assert(sizeof(msfl_keyframes_config) == 5 * 4, "msfl_keyframes_config is three ints and two floats");
static void (*const kDefault)(msfl_keyframes_config*) = &msfl_keyframes_default_config;
static msfl_status (*const kCreate)(msfl_handle*, const msfl_keyframes_config*, msfl_keyframes**) = &msfl_keyframes_create;
static void (*const kDestroy)(msfl_keyframes*) = &msfl_keyframes_destroy;
static int (*const kSize)(const msfl_keyframes*) = &msfl_keyframes_size;
static msfl_status (*const kAdd)(msfl_keyframes*, const msfl_point*, const int*, int, const msfl_point*, const int*, int, msfl_mem, int*) = &msfl_keyframes_add;
static msfl_status (*const kSizes)(msfl_keyframes*, int, int, int*, int*) = &msfl_keyframes_sizes;
static msfl_status (*const kGet)(msfl_keyframes*, int, msfl_point*, int, msfl_point*, int, msfl_mem) = &msfl_keyframes_get;
static msfl_status (*const kCompose)(msfl_keyframes*, int, const int*, const int*, const double*, float, float, msfl_point*, int, int*, msfl_point*, int,
                                     int*, msfl_mem) = &msfl_keyframes_compose;
static msfl_status (*const kInsert)(msfl_keyframes*, const int*, const double*, int, msfl_grid*, msfl_grid*, int*) = &msfl_keyframes_insert;

static int fail(const char* what) { std::fprintf(stderr, "keyframes_check: %s\n", what); return 1; }

static std::vector<msfl_point> cloud(int n, float shift) {
  std::vector<msfl_point> v(static_cast<std::size_t>(n));
  for (int i = 0; i < n; ++i)
    v[static_cast<std::size_t>(i)] = msfl_point{shift + 0.37f * static_cast<float>(i % 29), 0.21f * static_cast<float>(i % 53) - 4.0f,
                                                0.05f * static_cast<float>(i % 7), 0.0001f * static_cast<float>(i)};
  return v;
}

static bool same(const std::vector<msfl_point>& a, const msfl_point* b, std::size_t n) {
  return a.size() == n && (n == 0 || std::memcmp(a.data(), b, n * sizeof(msfl_point)) == 0);
}

int main() {
  (void)kDefault; (void)kCreate; (void)kDestroy; (void)kSize; (void)kAdd; (void)kSizes; (void)kGet; (void)kCompose; (void)kInsert;
  msfl_keyframes_config cfg = msfl::KeyframeStore::DefaultConfig();
  if (!(cfg.max_keyframes == 4096 && cfg.max_corner_points == 4194304 && cfg.max_surf_points == 16777216 && cfg.leaf_corner == 0.2f &&
        cfg.leaf_surf == 0.4f))
    return fail("the default config");
  cfg.max_corner_points = 1 << 14; cfg.max_surf_points = 1 << 14; cfg.leaf_corner = 0.f; cfg.leaf_surf = 0.f;
  msfl::KeyframeStore store(nullptr, &cfg);
  const std::vector<msfl_point> c0 = cloud(1025, 0.f), s0 = cloud(2049, 1.f), c1 = cloud(65, 2.f), s1 = cloud(0, 0.f);
  if (store.Add(c0, s0) != 0 || store.Add(c1, s1) != 1 || store.size() != 2) return fail("Add");
  const std::array<std::vector<int>, 2> n = store.Sizes();
  if (n[0] != std::vector<int>{1025, 65} || n[1] != std::vector<int>{2049, 0}) return fail("Sizes");
  std::vector<msfl_point> gc, gs;
  store.Get(0, &gc, &gs);
  if (!same(gc, c0.data(), c0.size()) || !same(gs, s0.data(), s0.size())) return fail("Get");

  // two submaps: {0 at A, 1 at B}, {1 at A}; against msfl_transform_cloud on the same handle
  const msfl::Rigid3d A({{10.0, -20.0, 0.5}}, {{0.0, 0.0, 0.3826834323650898, 0.9238795325112867}}), B({{-3.0, 4.0, 0.0}}, {{0.0, 0.0, 0.0, 1.0}});
  const std::vector<int> member_off = {0, 2, 3}, keys = {0, 1, 1};
  const std::vector<msfl::Rigid3d> poses = {A, B, A};
  const msfl::Submaps sub = store.ComposeSubmaps(member_off, keys, poses, 0.f, 0.f);
  if (sub.corner_off != std::vector<int>{0, 1090, 1155} || sub.surf_off != std::vector<int>{0, 2049, 2049}) return fail("ComposeSubmaps: offsets");
  std::vector<msfl_point> want;
  const std::vector<msfl_point>* src[3] = {&c0, &c1, &c1};
  for (int m = 0; m < 3; ++m) {
    std::vector<msfl_point> t(src[m]->size());
    const std::array<double, 7> p = poses[static_cast<std::size_t>(m)].ToVector7();
    if (msfl_transform_cloud(store.handle(), src[m]->data(), static_cast<int>(t.size()), p.data(), t.data(), MSFL_MEM_HOST) != MSFL_OK)
      return fail("msfl_transform_cloud");
    want.insert(want.end(), t.begin(), t.end());
  }
  if (!same(sub.corner, want.data(), want.size())) return fail("ComposeSubmaps: corner points");
  const msfl::Submaps filtered = store.ComposeSubmaps(member_off, keys, poses, 0.2f, 0.4f);
  if (filtered.corner_off.back() <= 0 || filtered.corner_off.back() > 1155 || filtered.surf_off[2] != filtered.surf_off[1]) return fail("ComposeSubmaps: leaves");

  // InsertInto against the loop it replaces
  msfl_grid *ga = nullptr, *gc2 = nullptr;
  if (msfl_grid_create(store.handle(), 3.0f, 0.2f, &ga) != MSFL_OK || msfl_grid_create(store.handle(), 3.0f, 0.2f, &gc2) != MSFL_OK) return fail("msfl_grid_create");
  if (store.InsertInto(keys, poses, ga, nullptr) != 3) return fail("InsertInto");
  int na = 0;
  msfl_grid_size(ga, &na, nullptr);
  // (one insert per keyframe on the store's side: one per keyframe here too)
  if (msfl_grid_insert_scan(gc2, want.data(), 1025, MSFL_MEM_HOST) != MSFL_OK || msfl_grid_insert_scan(gc2, want.data() + 1025, 65, MSFL_MEM_HOST) != MSFL_OK ||
      msfl_grid_insert_scan(gc2, want.data() + 1090, 65, MSFL_MEM_HOST) != MSFL_OK)
    return fail("msfl_grid_insert_scan");
  int nc = 0;
  msfl_grid_size(gc2, &nc, nullptr);
  std::vector<msfl_point> da(static_cast<std::size_t>(na) + 1), dc(static_cast<std::size_t>(nc) + 1);
  int ma = 0, mc = 0;
  if (msfl_grid_dump(ga, da.data(), na, &ma, MSFL_MEM_HOST) != MSFL_OK || msfl_grid_dump(gc2, dc.data(), nc, &mc, MSFL_MEM_HOST) != MSFL_OK) return fail("msfl_grid_dump");
  if (na != nc || ma != mc || std::memcmp(da.data(), dc.data(), static_cast<std::size_t>(ma) * sizeof(msfl_point)) != 0) return fail("InsertInto differs from the loop");
  // a keyframe 30 km out is refused at its position
  msfl_status st = MSFL_OK;
  const std::vector<msfl::Rigid3d> far = {B, msfl::Rigid3d({{30000.0, 0.0, 0.0}}, {{0.0, 0.0, 0.0, 1.0}}), A};
  if (store.InsertInto(keys, far, ga, nullptr, &st) != 1 || st != MSFL_CAPACITY) return fail("InsertInto: the refused keyframe");
  msfl_grid_destroy(ga); msfl_grid_destroy(gc2);
  std::printf("keyframes_check ok: %d keyframes, %d + %d points composed\n", store.size(), sub.corner_off.back(), sub.surf_off.back());
  return 0;
}
