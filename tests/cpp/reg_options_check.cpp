// Stand-alone check of the host-side helpers of what a registration call carries (msfl_api.hip: reject_options, RegSinks::at;
// msfl_api_slam.inc: the SlotRecords bookkeeping).  They live in the library's one translation unit, so this file includes it and adds a
// main(); it launches nothing and needs no GPU.  `make -C tests/cpp reg_options_check` builds it with the host side under
// -fsanitize=address,undefined and runs it.
#include "../../msf_loam_amd/csrc/msfl_api.hip"

#include <limits>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "reg_options_check: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static bool is_default(const RejectOptions& r) {
  return r.mode == MSFL_REJECT_OFF && r.thr2 == 0.0 && r.fraction == 0.0 && r.which == MSFL_REJECT_LAST_OUTER;
}

int main() {
  const char* who = "msfl_set_outlier_rejection";
  RejectOptions r;
  std::string err;
  // ---- the normaliser: off, and each mode with the other mode's parameter set to something
  CHECK(reject_options(nullptr, who, &r, &err) == MSFL_OK && is_default(r) && err.empty());
  msfl_outlier_rejection c{MSFL_REJECT_OFF, 0.3, 0.7, MSFL_REJECT_EVERY_OUTER};
  r.mode = 7; r.thr2 = 1.0;
  CHECK(reject_options(&c, who, &r, &err) == MSFL_OK && is_default(r));
  c = {MSFL_REJECT_THRESHOLD, 0.2, 0.7, MSFL_REJECT_EVERY_OUTER};
  CHECK(reject_options(&c, who, &r, &err) == MSFL_OK);
  CHECK(r.mode == MSFL_REJECT_THRESHOLD && r.thr2 == 0.2 * 0.2 && r.fraction == 0.0 && r.which == MSFL_REJECT_EVERY_OUTER);
  c = {MSFL_REJECT_FRACTION, 9.0, 0.15, MSFL_REJECT_LAST_OUTER};
  CHECK(reject_options(&c, who, &r, &err) == MSFL_OK);
  CHECK(r.mode == MSFL_REJECT_FRACTION && r.thr2 == 0.0 && r.fraction == 0.15 && r.which == MSFL_REJECT_LAST_OUTER);
  for (double edge : {0.0, 1.0}) {
    c = {MSFL_REJECT_FRACTION, 0.0, edge, MSFL_REJECT_LAST_OUTER};
    CHECK(reject_options(&c, who, &r, &err) == MSFL_OK && r.fraction == edge);
  }
  c = {MSFL_REJECT_THRESHOLD, 0.0, 0.0, MSFL_REJECT_LAST_OUTER};
  CHECK(reject_options(&c, who, &r, &err) == MSFL_OK && r.mode == MSFL_REJECT_THRESHOLD && r.thr2 == 0.0);
  CHECK(err.empty());
  // ---- every refusal: MSFL_BAD_ARG, the defaults, a text that starts with the caller's name and names the field
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const struct { msfl_outlier_rejection cfg; const char* field; } bad[] = {
      {{9, 0.2, 0.1, MSFL_REJECT_LAST_OUTER}, "mode"},           {{-1, 0.2, 0.1, MSFL_REJECT_LAST_OUTER}, "mode"},
      {{MSFL_REJECT_THRESHOLD, 0.2, 0.0, 7}, "which"},           {{MSFL_REJECT_FRACTION, 0.0, 0.1, -1}, "which"},
      {{MSFL_REJECT_THRESHOLD, -1.0, 0.0, 0}, "threshold"},      {{MSFL_REJECT_THRESHOLD, nan, 0.0, 0}, "threshold"},
      {{MSFL_REJECT_THRESHOLD, inf, 0.0, 0}, "threshold"},       {{MSFL_REJECT_FRACTION, 0.0, -0.1, 0}, "fraction"},
      {{MSFL_REJECT_FRACTION, 0.0, 1.5, 0}, "fraction"},         {{MSFL_REJECT_FRACTION, 0.0, nan, 0}, "fraction"}};
  for (const auto& b : bad) {
    err.clear(); r.mode = 7;
    CHECK(reject_options(&b.cfg, "msfl_slam_set_outlier_rejection (mapping)", &r, &err) == MSFL_BAD_ARG && is_default(r));
    CHECK(err.rfind("msfl_slam_set_outlier_rejection (mapping): ", 0) == 0 && err.find(b.field) != std::string::npos);
  }
  // ---- RegSinks::at offsets exactly the non-null pointers and copies the options
  DevMatchInfo info[4]; UncRecord unc[4]; PosePrior prior[4]; DegenRecord degen[4]; RejectRecord rej[4];
  RegSinks k;
  k.opt.unc_min_eig = 150.0; k.opt.degen_on = 1; k.opt.degen_min_eig = 40.0;
  k.opt.rej.mode = MSFL_REJECT_FRACTION; k.opt.rej.fraction = 0.25; k.opt.rej.thr2 = 0.0; k.opt.rej.which = MSFL_REJECT_EVERY_OUTER;
  const auto same_opt = [&](const RegSinks& a) { return std::memcmp(&a.opt, &k.opt, sizeof(RegOptions)) == 0; };
  RegSinks a = k.at(3);                                                     // all null: stays null
  CHECK(same_opt(a) && !a.info && !a.unc && !a.prior && !a.degen && !a.rej);
  k.info = info; k.unc = unc; k.prior = prior; k.degen = degen; k.rej = rej;
  a = k.at(3);
  CHECK(same_opt(a) && a.info == info + 3 && a.unc == unc + 3 && a.prior == prior + 3 && a.degen == degen + 3 && a.rej == rej + 3);
  CHECK(k.info == info && k.rej == rej);                                    // (the whole batch's record is untouched)
  for (int off = 0; off < 5; off++) {                                       // one pointer null at a time
    RegSinks m = k;
    if (off == 0) m.info = nullptr; if (off == 1) m.unc = nullptr; if (off == 2) m.prior = nullptr;
    if (off == 3) m.degen = nullptr; if (off == 4) m.rej = nullptr;
    a = m.at(2).at(1);
    CHECK(a.info == (off == 0 ? nullptr : info + 3) && a.unc == (off == 1 ? nullptr : unc + 3) && a.prior == (off == 2 ? nullptr : prior + 3));
    CHECK(a.degen == (off == 3 ? nullptr : degen + 3) && a.rej == (off == 4 ? nullptr : rej + 3) && same_opt(a));
  }
  CHECK(k.at(0).unc == unc);
  // ---- SlotRecords: what `held` and the slot arithmetic do without a device (nothing is reserved, nothing is put on a stream)
  SlotRecords s;
  for (int slot = 0; slot < kSlamSlots; slot++) CHECK(!s.held[slot] && s.fetch(slot, nullptr) == hipSuccess);   // not held: no copy
  CHECK(s.arm(2, true, false, nullptr) == hipSuccess && s.held[2] && !s.held[1] && !s.held[3]);
  CHECK(s.arm(2, false, true, nullptr) == hipSuccess && !s.held[2]);       // off: no memset either
  alignas(8) static char pinned[kSlamSlots * 2 * sizeof(RejectRecord)];
  s.host.p = pinned; s.bytes = 2 * sizeof(RejectRecord);
  for (int slot = 0; slot < kSlamSlots; slot++) {
    const RejectRecord* pair = s.host_at<RejectRecord>(slot);
    CHECK(reinterpret_cast<const char*>(pair) == pinned + slot * 2 * sizeof(RejectRecord));
    CHECK(reinterpret_cast<const char*>(pair + 2) <= pinned + sizeof(pinned));
  }
  CHECK(s.ensure(64) == hipSuccess && s.bytes == 2 * sizeof(RejectRecord));   // already reserved: left as it is
  s.host.p = nullptr;                                                        // (not the buffer's to free)
  std::printf("reg_options_check ok\n");
  return 0;
}
