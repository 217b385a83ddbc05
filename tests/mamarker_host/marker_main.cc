// marker_main.cc -- TEST PROGRAM ONLY: the "not populated" marker of a macro-atom record (tables.h "ABSENT IONS") against the action filters
// populate_mafilter_level() can write, and rng_unstep() against rng_next(). physics.h compiled for x86 (ARTIS_HOST_EMU), one level without
// transitions whose record is a local buffer.
#define ARTIS_HOST_EMU 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../artis_amd/csrc/model_build.h"
#include "../../artis_amd/csrc/physics.h"

using namespace artis;

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next64() {
  g_s ^= g_s << 13;
  g_s ^= g_s >> 7;
  g_s ^= g_s << 17;
  return g_s;
}
static double unif() { return (double)(next64() >> 11) * 0x1.0p-53; }

static bool unusable(const U4 &f) { return (f.w[0] & 0xFFFFu) > (f.w[3] >> 16); }  // ma_jump_internal's test

int main() {
  long failed = 0, cases = 0;
  const U4 absent = U4{{MA_MARK_ABSENT, 0u, 0u, 0u}}, filling = U4{{MA_MARK_FILLING, 0u, 0u, 0u}};
  const U4 none = U4{{MAFILT_NONE, 0u, 0u, 0u}};  // populate_mafilter_level's "no usable filter"
  // the markers themselves
  for (const U4 &m : {absent, filling}) {
    cases++;
    if (!unusable(m) || !ma_mark_unpopulated(m.w[0]) || std::memcmp(&m, &none, sizeof(U4)) == 0) failed++;
  }
  cases++;
  if (!unusable(none) || ma_mark_unpopulated(none.w[0])) failed++;  // (the existing marker is unusable too, and is not taken for the new one)

  // one level, no transitions: record = [action filter | 3 first lines | rates]
  Env env;
  std::memset(&env, 0, sizeof(env));
  LevelPack lpk{0, 0, 0, 0};
  env.M.level_pack = &lpk;
  env.M.nlevels = 1;
  std::vector<U4> rec((size_t)marec_slots(0, 0) + MAREC_SLACK);
  env.M.nmacache = (int)rec.size();
  env.K.macache = rec.data();
  double *rates = ma_rates_of(rec.data(), 0, 0);
  auto check = [&](const char *what) {
    populate_mafilter_level(env, 0, 0);
    const U4 f = rec[0];
    cases++;
    const bool is_marker = std::memcmp(&f, &absent, sizeof(U4)) == 0 || std::memcmp(&f, &filling, sizeof(U4)) == 0 || ma_mark_unpopulated(f.w[0]);
    // a filter is either usable (sorted entries, each <= 0x7FFF) or exactly the "no usable filter" marker
    const bool is_none = std::memcmp(&f, &none, sizeof(U4)) == 0;
    if (is_marker || (unusable(f) && !is_none)) {
      failed++;
      std::printf("FAILED %s: filter %08x %08x %08x %08x\n", what, f.w[0], f.w[1], f.w[2], f.w[3]);
    }
    return is_none;
  };
  for (int t = 0; t < 200000; t++) {  // random rates over 86 decades, some of them zero
    const double scale = std::exp((unif() - 0.5) * 200.);
    for (int a = 0; a < MA_N; a++) rates[a] = (unif() < 0.3) ? 0. : unif() * unif() * scale;
    (void)check("random rates");
  }
  for (int a = 0; a < MA_N; a++) rates[a] = 0.;
  cases++;
  if (!check("zero total")) failed++;  // (must be the existing marker)
  for (int t = 0; t < 20000; t++) {  // a negative rate somewhere
    for (int a = 0; a < MA_N; a++) rates[a] = unif();
    rates[next64() % MA_N] = -unif() * ((t & 1) ? 10. : 0.1);
    (void)check("negative rate");
  }
  for (double bad : {std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::max()}) {
    for (int a = 0; a < MA_N; a++) rates[a] = unif();
    rates[3] = bad;
    (void)check("non-finite rate");
  }

  // rng_unstep() undoes rng_next(), from any state
  for (int t = 0; t < 200000; t++) {
    Pkt p;
    std::memset(&p, 0, sizeof(p));
    p.s0 = (uint32_t)next64(); p.s1 = (uint32_t)next64(); p.s2 = (uint32_t)next64(); p.s3 = (uint32_t)next64();
    if (t == 0) p.s0 = p.s1 = p.s2 = 0u, p.s3 = 1u;
    if (t == 1) p.s0 = p.s1 = p.s2 = p.s3 = 0xFFFFFFFFu;
    const Pkt q = p;
    (void)rng_u24(p);
    rng_unstep(p);
    cases++;
    if (p.s0 != q.s0 || p.s1 != q.s1 || p.s2 != q.s2 || p.s3 != q.s3) failed++;
  }
  std::printf("%ld cases, %ld failed\n", cases, failed);
  return failed == 0 ? 0 : 1;
}
