// Stand-alone driver of xd-tts_amd/csrc/f0_plan.h (the host arithmetic of the pitch tracker and of pitch targets) at its limits:
// F = 16384, range 0 and 4 with the clamp engaging, no voiced frame, ties, one frame, and each argument rule.
// Plain g++, no HIP; prints "ok".  tests/test_f0_cpu.py builds and runs it, once more under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "f0_plan.h"

using namespace xdtts;

#define REQUIRE(x)                                                \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      return 1;                                                   \
    }                                                             \
  } while (0)

static bool names(const std::string &msg, const char *word) { return msg.find(word) != std::string::npos; }

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const F0Opts def = f0_opts_default();
  // the rules of the options and the quefrency range
  {
    int lo = 0, hi = 0;
    REQUIRE(f0_opts_check(def).empty());
    f0_quefrency(def, &lo, &hi);
    REQUIRE(lo == 56 && hi == 367);
    F0Opts o = def;
    o.fmin = 50.0f;
    o.fmax = 1000.0f;
    REQUIRE(f0_opts_check(o).empty());
    f0_quefrency(o, &lo, &hi);
    REQUIRE(lo == 23 && hi == 441 && lo >= 22);
    o.fmax = 50.1f;
    f0_quefrency(o, &lo, &hi);
    REQUIRE(lo == 441 && hi == 441 && names(f0_opts_check(o), "quefrency"));
    struct {
      float F0Opts::*field;
      float v;
      const char *name;
    } bad[] = {{&F0Opts::fmin, 49.9f, "fmin"}, {&F0Opts::fmin, nan, "fmin"}, {&F0Opts::fmin, 400.0f, "fmin"}, {&F0Opts::fmax, 1000.5f, "fmax"},
               {&F0Opts::fmax, inf, "fmax"}, {&F0Opts::threshold, -0.1f, "threshold"}, {&F0Opts::threshold, nan, "threshold"},
               {&F0Opts::octave_bias, 0.0f, "octave_bias"}, {&F0Opts::octave_bias, 1.01f, "octave_bias"}, {&F0Opts::octave_bias, nan, "octave_bias"},
               {&F0Opts::log_floor, 0.0f, "log_floor"}, {&F0Opts::log_floor, -1.0f, "log_floor"}, {&F0Opts::log_floor, inf, "log_floor"}};
    for (const auto &b : bad) {
      F0Opts x = def;
      x.*(b.field) = b.v;
      REQUIRE(names(f0_opts_check(x), b.name));
    }
    o = def;
    o.threshold = 0.0f;
    o.octave_bias = 1.0f;
    REQUIRE(f0_opts_check(o).empty());
  }
  // the rules of the target, and the identity
  {
    REQUIRE(pitch_target_check(pitch_target_default()).empty() && pitch_target_is_identity(pitch_target_default()));
    REQUIRE(pitch_target_is_identity({2, 1.0f, 1.0f}) && pitch_target_is_identity({0, 7.0f, 1.0f}));
    REQUIRE(!pitch_target_is_identity({2, 1.0f, 0.0f}) && !pitch_target_is_identity({1, 180.0f, 1.0f}) && !pitch_target_is_identity({2, 1.1f, 1.0f}));
    REQUIRE(names(pitch_target_check({3, 1.0f, 1.0f}), "mode") && names(pitch_target_check({-1, 1.0f, 1.0f}), "mode"));
    REQUIRE(names(pitch_target_check({1, 49.0f, 1.0f}), "value") && names(pitch_target_check({1, 1001.0f, 1.0f}), "value") && names(pitch_target_check({1, nan, 1.0f}), "value"));
    REQUIRE(names(pitch_target_check({2, 0.49f, 1.0f}), "value") && names(pitch_target_check({2, 2.01f, 1.0f}), "value"));
    REQUIRE(names(pitch_target_check({0, 1.0f, -0.1f}), "range") && names(pitch_target_check({0, 1.0f, 4.1f}), "range") && names(pitch_target_check({0, 1.0f, nan}), "range"));
    REQUIRE(pitch_target_check({1, 50.0f, 0.0f}).empty() && pitch_target_check({1, 1000.0f, 4.0f}).empty() && pitch_target_check({0, nan, 1.0f}).empty());
  }
  // the median of five: counts 0 .. 5, unvoiced entries skipped, the LOWER median of an even count
  {
    const uint32_t w[5] = {f0_bits(100.0f), 0u, f0_bits(300.0f), f0_bits(200.0f), f0_bits(400.0f)};
    REQUIRE(f0_median5(w, 0) == 0u && f0_median5(w + 1, 1) == 0u);
    REQUIRE(f0_float(f0_median5(w, 1)) == 100.0f && f0_float(f0_median5(w, 3)) == 100.0f);  // {100, 300} -> 100
    REQUIRE(f0_float(f0_median5(w, 4)) == 200.0f && f0_float(f0_median5(w, 5)) == 200.0f);  // {100, 200, 300(, 400)} -> 200
  }
  // F = 16384, every frame voiced, a slow sweep over an octave: the selection at full size; range 4 engages the clamp at both ends
  {
    const size_t F = F0_MAX_FRAMES;
    std::vector<float> raw(F), strength(F, 0.5f), f0(F), ratio(F);
    for (size_t i = 0; i < F; ++i) raw[i] = 100.0f * std::exp2((float)((i * 7919u) % F) / (float)F);  // a permutation: 100 .. 200 Hz
    F0Stats s;
    F0Opts o = def;
    f0_track_reference(raw.data(), strength.data(), F, o, {2, 1.0f, 4.0f}, f0.data(), ratio.data(), &s);
    REQUIRE(s.n_frames == (int)F && s.n_voiced == (int)F && s.base_ratio == 1.0f);
    REQUIRE(s.min_hz >= 100.0f && s.max_hz < 200.0f && s.median_hz > 135.0f && s.median_hz < 148.0f);
    size_t below = 0, clamped = 0;
    for (size_t i = 0; i < F; ++i) {
      REQUIRE(ratio[i] >= 0.5f && ratio[i] <= 2.0f && f0[i] > 0.0f);
      below += f0[i] < s.median_hz;
      clamped += ratio[i] == 0.5f || ratio[i] == 2.0f;
    }
    REQUIRE(below <= (F - 1) / 2);  // the lower median: at most (n - 1) / 2 values lie below it
    REQUIRE(s.n_clamped > 0 && (size_t)s.n_clamped <= clamped && clamped < F);
    // range 0 flattens: every frame lands on the median, nothing is clamped inside an octave
    f0_track_reference(raw.data(), strength.data(), F, o, {2, 1.0f, 0.0f}, f0.data(), ratio.data(), &s);
    REQUIRE(s.n_clamped == 0);
    for (size_t i = 0; i < F; ++i) REQUIRE(std::fabs(f0[i] * ratio[i] / s.median_hz - 1.0f) < 1e-6f);
    // an absolute target an octave above the median: base 2 -- at range 1 every ratio is the base itself, at range 4 the frames
    // above the median leave the range and are clamped
    f0_track_reference(raw.data(), strength.data(), F, o, {1, 2.0f * s.median_hz, 1.0f}, nullptr, ratio.data(), &s);
    REQUIRE(s.base_ratio == 2.0f && s.n_clamped == 0);  // (range 1: every ratio is the base itself)
    f0_track_reference(raw.data(), strength.data(), F, o, {1, 2.0f * s.median_hz, 4.0f}, nullptr, ratio.data(), &s);
    REQUIRE(s.n_clamped > (int)F / 4);
    // outputs are optional
    f0_track_reference(raw.data(), strength.data(), F, o, pitch_target_default(), nullptr, nullptr, nullptr);
  }
  // no voiced frame: base 1, every ratio 1, the stats' frequencies 0 -- whatever the target
  {
    const size_t F = 37;
    std::vector<float> raw(F, 123.0f), strength(F, 0.05f), f0(F, -1.0f), ratio(F, -1.0f);
    strength[3] = nan;  // NaN: unvoiced
    F0Stats s;
    f0_track_reference(raw.data(), strength.data(), F, def, {1, 300.0f, 4.0f}, f0.data(), ratio.data(), &s);
    REQUIRE(s.n_voiced == 0 && s.n_clamped == 0 && s.median_hz == 0.0f && s.min_hz == 0.0f && s.max_hz == 0.0f && s.base_ratio == 1.0f);
    for (size_t i = 0; i < F; ++i) REQUIRE(f0[i] == 0.0f && ratio[i] == 1.0f);
  }
  // one frame, and ties
  {
    const float raw1 = 222.0f, st1 = 0.3f;
    float f0 = 0.f, ratio = 0.f;
    F0Stats s;
    f0_track_reference(&raw1, &st1, 1, def, {1, 111.0f, 2.0f}, &f0, &ratio, &s);
    REQUIRE(f0 == 222.0f && ratio == 0.5f && s.n_voiced == 1 && s.median_hz == 222.0f && s.min_hz == 222.0f && s.max_hz == 222.0f && s.base_ratio == 0.5f && s.n_clamped == 0);
    std::vector<float> raw(64, 150.0f), strength(64, 0.4f), f(64), r(64);
    for (size_t i = 0; i < 64; i += 7) raw[i] = 130.0f;
    f0_track_reference(raw.data(), strength.data(), 64, def, {2, 1.0f, 2.0f}, f.data(), r.data(), &s);
    REQUIRE(s.median_hz == 150.0f && s.min_hz == 150.0f);  // the median of five removes every isolated 130
    for (size_t i = 0; i < 64; ++i) REQUIRE(f[i] == 150.0f && r[i] == 1.0f);
    // an unvoiced frame takes the base, unclamped values pass
    strength[10] = 0.0f;
    f0_track_reference(raw.data(), strength.data(), 64, def, {2, 1.5f, 1.0f}, f.data(), r.data(), &s);
    REQUIRE(f[10] == 0.0f && r[10] == 1.5f && s.n_voiced == 63);
  }
  std::printf("ok\n");
  return 0;
}
