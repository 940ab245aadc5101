// Host bookkeeping of the keyframe store (msf_loam_amd/csrc/msfl_keyframes_host.h), stand-alone: the member table for the shapes of
// the GPU tests' compose cases, totals just below and at 2^31 from made-up counts with no memory behind them, every refusal, the add
// capacities and the launch shape.  Built with -fsanitize=address,undefined and run on the CPU (tests/test_keyframes_model.py).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "msfl_keyframes_host.h"

using namespace msfl;

static int g_failed = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "keyframes_host_check: line %d: %s\n", __LINE__, #cond); g_failed++; } } while (0)

static const int kSizes[9] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4097};

// the nine keyframes of tests/test_gpu_keyframes.py: keyframe i has kSizes[i] corner and kSizes[(4 i + 3) % 9] surf points
static KfIndex nine() {
  KfIndex ix;
  for (int i = 0; i < 9; i++) kf_commit_add(&ix, kSizes[i], kSizes[(4 * i + 3) % 9]);
  return ix;
}

static std::vector<double> unit_poses(int n) {
  std::vector<double> p((size_t)n * 7, 0.0);
  for (int m = 0; m < n; m++) { p[7 * m] = m; p[7 * m + 6] = 1.0; }
  return p;
}

static void check_plan(const KfIndex& ix, int B, const std::vector<int>& off, const std::vector<int>& keys) {
  const std::vector<double> poses = unit_poses((int)keys.size());
  KfPlan plan;
  const char* why = "";
  const long long big = std::numeric_limits<int>::max();
  EXPECT(kf_plan_compose(ix, B, off.data(), keys.data(), poses.data(), 0.f, 0.4f, big, big, &plan, &why) == kKfOk);
  const int first = off[0], M = off[B] - off[0];
  EXPECT(plan.n_members == M && (int)plan.poses.size() == 8 * M);
  int longest = 0;
  for (int k = 0; k < 2; k++) {
    EXPECT((int)plan.rec[k].size() == M && (int)plan.off[k].size() == B + 1 && plan.off[k][0] == 0);
    long long run = 0;
    for (int b = 0; b < B; b++) {
      EXPECT(plan.off[k][b] == run);
      for (int m = off[b]; m < off[b + 1]; m++) {
        const KfRec& r = plan.rec[k][m - first];
        EXPECT(r.src == ix.start[k][keys[m]] && r.count == ix.count[k][keys[m]] && r.dst == run && r.flags == 0);
        run += r.count;
        longest = std::max(longest, r.count);
      }
    }
    EXPECT(plan.off[k][B] == run && plan.total[k] == run);
  }
  for (int m = 0; m < M; m++) EXPECT(plan.poses[8 * m] == first + m && plan.poses[8 * m + 6] == 1.0 && plan.poses[8 * m + 7] == 0.0);
  EXPECT(plan.max_count == longest);
  // a capacity one short of either total
  for (int k = 0; k < 2; k++) {
    KfPlan p2;
    const long long cc = plan.total[0] - (k == 0), cs = plan.total[1] - (k == 1);
    if (cc < 0 || cs < 0) continue;
    EXPECT(kf_plan_compose(ix, B, off.data(), keys.data(), poses.data(), 0.f, 0.f, cc, cs, &p2, &why) == kKfCapacity);
    EXPECT(kf_plan_compose(ix, B, off.data(), keys.data(), poses.data(), 0.f, 0.f, plan.total[0], plan.total[1], &p2, &why) == kKfOk);
  }
}

int main() {
  const KfIndex ix = nine();
  EXPECT(ix.size() == 9 && ix.top[0] == 7362 && ix.top[1] == 7362 && ix.start[0][8] == 3265 && ix.start[1][1] == 64);
  // the shapes of the compose cases: B = 1 and B = 5, member_off[0] = 2, repeated keys, members of size 0, a submap without members
  check_plan(ix, 1, {2, 8}, {99, -1, 3, 0, 6, 3, 8, 1});
  check_plan(ix, 5, {2, 6, 9, 9, 12, 15}, {77, 77, 6, 8, 6, 0, 5, 8, 2, 7, 1, 3, 4, 8, 0});
  check_plan(ix, 3, {0, 0, 0, 0}, {});                      // nothing but empty submaps
  check_plan(ix, 0, {5}, {});                               // no submap at all
  check_plan(ix, 2, {0, 17, 57}, std::vector<int>(57, 8));  // the large forms: 17 and 40 times key 8

  // ---- refusals ----
  const std::vector<int> off = {2, 6, 9, 9, 12, 15}, keys = {77, 77, 6, 8, 6, 0, 5, 8, 2, 7, 1, 3, 4, 8, 0};
  const std::vector<double> poses = unit_poses(15);
  const long long big = std::numeric_limits<int>::max();
  const char* why = "";
  KfPlan plan;
  auto run = [&](const std::vector<int>& o, const std::vector<int>& k, const std::vector<double>& p, float lc, float ls) {
    return kf_plan_compose(ix, (int)o.size() - 1, o.data(), k.data(), p.data(), lc, ls, big, big, &plan, &why);
  };
  EXPECT(run(off, keys, poses, 0.2f, 0.4f) == kKfOk);
  for (int bad : {9, -1, 1 << 30}) { std::vector<int> k2 = keys; k2[7] = bad; EXPECT(run(off, k2, poses, 0.f, 0.f) == kKfBadArg); }
  { std::vector<int> k2 = keys; k2[0] = -5; k2[1] = 1 << 30; EXPECT(run(off, k2, poses, 0.f, 0.f) == kKfOk); }    // positions before member_off[0] are never read
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double bad : {nan, inf, -inf})
    for (int e = 0; e < 7; e++) { std::vector<double> p2 = poses; p2[7 * 9 + e] = bad; EXPECT(run(off, keys, p2, 0.f, 0.f) == kKfBadArg); }
  { std::vector<double> p2 = poses; p2[0] = nan; p2[13] = inf; EXPECT(run(off, keys, p2, 0.f, 0.f) == kKfOk); }
  EXPECT(run({2, 6, 5, 9, 12, 15}, keys, poses, 0.f, 0.f) == kKfBadArg);
  EXPECT(run({-1, 6, 9, 9, 12, 15}, keys, poses, 0.f, 0.f) == kKfBadArg);
  const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
  for (float leaf : {fnan, -0.2f, finf, -finf, -0.0f - 1e-30f}) {
    EXPECT(run(off, keys, poses, leaf, 0.f) == kKfBadArg);
    EXPECT(run(off, keys, poses, 0.f, leaf) == kKfBadArg);
  }
  EXPECT(kf_plan_compose(ix, -1, off.data(), keys.data(), poses.data(), 0.f, 0.f, big, big, &plan, &why) == kKfBadArg);
  EXPECT(kf_plan_compose(ix, 5, nullptr, keys.data(), poses.data(), 0.f, 0.f, big, big, &plan, &why) == kKfBadArg);
  EXPECT(kf_plan_compose(ix, 5, off.data(), nullptr, poses.data(), 0.f, 0.f, big, big, &plan, &why) == kKfBadArg);
  EXPECT(kf_plan_compose(ix, 5, off.data(), keys.data(), nullptr, 0.f, 0.f, big, big, &plan, &why) == kKfBadArg);
  EXPECT(kf_check_members(9, keys.data(), poses.data(), 2, 15, &why) == kKfOk && kf_check_members(8, keys.data(), poses.data(), 2, 15, &why) == kKfBadArg);

  // ---- totals just below and at 2^31: two made-up keyframes of 2^30 and 2^30 - 1 points, no memory behind them ----
  KfIndex huge;
  huge.start[0] = {0, 0}; huge.count[0] = {1 << 30, (1 << 30) - 1};
  huge.start[1] = {0, 0}; huge.count[1] = {5, 7};
  const std::vector<double> p2 = unit_poses(2);
  const int off2[2] = {0, 2}, below[2] = {0, 1}, at[2] = {0, 0};
  const long long cap = 1LL << 40;
  EXPECT(kf_plan_compose(huge, 1, off2, below, p2.data(), 0.f, 0.f, cap, cap, &plan, &why) == kKfOk);
  EXPECT(plan.total[0] == 2147483647LL && plan.rec[0][1].dst == (1 << 30) && plan.off[0][1] == 2147483647 && plan.max_count == (1 << 30));
  EXPECT(kf_plan_compose(huge, 1, off2, at, p2.data(), 0.f, 0.f, cap, cap, &plan, &why) == kKfCapacity);
  std::swap(huge.count[0], huge.count[1]);                  // the same on the surf side
  EXPECT(kf_plan_compose(huge, 1, off2, below, p2.data(), 0.f, 0.f, cap, cap, &plan, &why) == kKfOk && plan.total[1] == 2147483647LL);
  EXPECT(kf_plan_compose(huge, 1, off2, at, p2.data(), 0.f, 0.f, cap, cap, &plan, &why) == kKfCapacity);
  EXPECT(kf_plan_compose(huge, 1, off2, below, p2.data(), 0.f, 0.f, cap, 2147483646LL, &plan, &why) == kKfCapacity);

  // ---- add: the keyframe count and both pools, one past capacity ----
  KfIndex a;
  const long long pool[2] = {100, 50};
  EXPECT(kf_check_add(a, 2, pool, 100, 50, &why) == kKfOk && kf_check_add(a, 2, pool, 101, 0, &why) == kKfCapacity &&
         kf_check_add(a, 2, pool, 0, 51, &why) == kKfCapacity);
  kf_commit_add(&a, 60, 30);
  EXPECT(kf_check_add(a, 2, pool, 40, 20, &why) == kKfOk && kf_check_add(a, 2, pool, 41, 20, &why) == kKfCapacity &&
         kf_check_add(a, 2, pool, 40, 21, &why) == kKfCapacity);
  kf_commit_add(&a, 40, 20);
  EXPECT(a.size() == 2 && a.start[0][1] == 60 && a.start[1][1] == 30 && a.top[0] == 100 && a.top[1] == 50);
  EXPECT(kf_check_add(a, 2, pool, 0, 0, &why) == kKfCapacity && kf_check_add(a, 3, pool, 0, 0, &why) == kKfOk);

  // ---- the finite check of a host list, through an index list too ----
  std::vector<float> pts(4 * 6, 1.0f);
  const int idx[3] = {5, 0, 2};
  EXPECT(kf_first_non_finite(pts.data(), nullptr, 6) == -1 && kf_first_non_finite(pts.data(), idx, 3) == -1 && kf_first_non_finite(pts.data(), nullptr, 0) == -1);
  for (float bad : {fnan, finf, -finf})
    for (int c = 0; c < 4; c++) {
      pts[4 * 2 + c] = bad;
      EXPECT(kf_first_non_finite(pts.data(), nullptr, 6) == 2 && kf_first_non_finite(pts.data(), idx, 3) == 2 && kf_first_non_finite(pts.data(), idx, 2) == -1);
      pts[4 * 2 + c] = 1.0f;
    }

  // ---- launch shape ----
  KfGrid g = kf_grid_shape(4097, 1344);
  EXPECT(g.x == 5 && g.y == 1344 && g.z == 2);
  g = kf_grid_shape(1024, 70000);
  EXPECT(g.x == 1 && g.y == 65535 && g.z == 2);
  g = kf_grid_shape(1025, 70000 - 65535);
  EXPECT(g.x == 2 && g.y == 4465 && g.z == 2);
  g = kf_grid_shape(1 << 30, 1);
  EXPECT(g.x == (1u << 20) && g.y == 1);

  if (g_failed) return 1;
  std::printf("keyframes host ok\n");
  return 0;
}
