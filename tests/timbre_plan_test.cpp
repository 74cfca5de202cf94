// Stand-alone driver of csrc/timbre_plan.h (plain g++, built with -fsanitize=address,undefined by tests/test_timbre_cpu.py):
// the argument rules (each bound, NaN, inf), the identity test, and n / v / N of the breath noise at the corners of the grid the
// Python test compares with its numpy restatement.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "timbre_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static bool names(const std::string &msg, const char *field) { return msg.find(field) != std::string::npos; }

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  static_assert(sizeof(Timbre) == 20, "xdtts_timbre is 20 bytes");

  // the default: (1, 0, 1, 30, 1e-5), a setting, the identity
  const Timbre d = timbre_default();
  CHECK(d.vtl == 1.0f && d.breath == 0.0f && d.seed == 1u && d.lifter == 30 && d.log_floor == 1e-5f);
  CHECK(timbre_check(d).empty());
  CHECK(timbre_is_identity(d));

  // each bound, from both sides; NaN and inf
  auto with = [&](auto set) {
    Timbre t = d;
    set(t);
    return timbre_check(t);
  };
  for (float v : {0.5f, 0.75f, 1.0f, 2.0f}) CHECK(with([&](Timbre &t) { t.vtl = v; }).empty());
  for (float v : {std::nextafter(0.5f, 0.0f), std::nextafter(2.0f, 3.0f), 0.0f, -1.0f, nan, inf, -inf})
    CHECK(names(with([&](Timbre &t) { t.vtl = v; }), "vtl"));
  for (float v : {0.0f, 0.5f, 1.0f}) CHECK(with([&](Timbre &t) { t.breath = v; }).empty());
  for (float v : {-std::numeric_limits<float>::denorm_min(), std::nextafter(1.0f, 2.0f), -1.0f, 2.0f, nan, inf, -inf})
    CHECK(names(with([&](Timbre &t) { t.breath = v; }), "breath"));
  for (int v : {1, 30, 255}) CHECK(with([&](Timbre &t) { t.lifter = v; }).empty());
  for (int v : {0, -1, 256, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()})
    CHECK(names(with([&](Timbre &t) { t.lifter = v; }), "lifter"));
  for (float v : {std::numeric_limits<float>::denorm_min(), 1e-5f, 1e-3f, 1.0f, std::numeric_limits<float>::max()})
    CHECK(with([&](Timbre &t) { t.log_floor = v; }).empty());
  for (float v : {0.0f, -0.0f, -1e-5f, nan, inf, -inf}) CHECK(names(with([&](Timbre &t) { t.log_floor = v; }), "log_floor"));
  // the first bad field is the one named
  CHECK(names(with([&](Timbre &t) { t.vtl = nan; t.breath = nan; }), "vtl"));
  // any seed is a setting
  for (uint32_t s : {0u, 1u, 0xFFFFFFFFu}) CHECK(with([&](Timbre &t) { t.seed = s; }).empty());

  // the frame count of a request of the stage alone: 1 .. 2^20
  CHECK(names(timbre_frames_check(0), "frames"));
  CHECK(timbre_frames_check(1).empty());
  CHECK(timbre_frames_check((size_t)1 << 20).empty());
  CHECK(names(timbre_frames_check(((size_t)1 << 20) + 1), "frames"));

  // the identity: vtl == 1 and breath == 0, whatever the rest
  CHECK(timbre_is_identity(Timbre{1.0f, 0.0f, 77u, 1, 1e-3f}));
  CHECK(timbre_is_identity(Timbre{1.0f, -0.0f, 0u, 255, 1.0f}));
  CHECK(!timbre_is_identity(Timbre{std::nextafter(1.0f, 2.0f), 0.0f, 1u, 30, 1e-5f}));
  CHECK(!timbre_is_identity(Timbre{1.0f, std::numeric_limits<float>::denorm_min(), 1u, 30, 1e-5f}));

  // n, v, N at the corners of the grid: n is 23 bits of rng_u32(seed, 0x71B8, frame * 513 + bin), v an odd multiple of 2^-24
  const uint32_t seeds[] = {0u, 1u, 0xFFFFFFFFu}, frames[] = {0u, 1u, 799u, (1u << 20) - 1u}, bins[] = {0u, 1u, 511u, 512u};
  const float lo = 0.5f * std::log(std::ldexp(1.0f, -24)) + TIMBRE_NOISE_SHIFT, hi = 0.5f * std::log(24.0f * std::log(2.0f)) + TIMBRE_NOISE_SHIFT;
  for (uint32_t s : seeds)
    for (uint32_t f : frames)
      for (uint32_t b : bins) {
        const uint32_t n = timbre_noise_bits(s, f, b);
        CHECK(n == (rng_u32(s, 0x71B8u, f * 513u + b) >> 9));
        CHECK(n < (1u << 23));
        const float v = timbre_noise_v(n);
        CHECK(v > 0.0f && v < 1.0f);
        CHECK((double)v == (2.0 * n + 1.0) / 16777216.0);  // exact in fp32
        const float N = timbre_noise(v);
        CHECK(std::isfinite(N) && N >= lo - 1e-5f && N <= hi + 1e-5f);
      }
  // the ends of the range of v
  CHECK(timbre_noise_v(0u) == std::ldexp(1.0f, -24));
  CHECK(timbre_noise_v((1u << 23) - 1u) == 1.0f - std::ldexp(1.0f, -24));
  CHECK(std::isfinite(timbre_noise(timbre_noise_v(0u))) && std::isfinite(timbre_noise(timbre_noise_v((1u << 23) - 1u))));
  // the noise is a function of (seed, frame, bin): the index of the last cell of 2^20 frames does not wrap
  CHECK((uint64_t)((1u << 20) - 1u) * 513u + 512u < ((uint64_t)1 << 32));
  CHECK(timbre_noise_bits(1u, 0u, 513u) == timbre_noise_bits(1u, 1u, 0u));  // (the index is frame * 513 + bin)
  CHECK(timbre_noise_bits(1u, 0u, 0u) != timbre_noise_bits(2u, 0u, 0u));
  CHECK(std::fabs(TIMBRE_NOISE_SHIFT - 0.5 * 0.5772156649015329) < 1e-7);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
