// f0_plan.h -- the host arithmetic of the pitch tracker and of pitch targets (xdtts_f0_opts, xdtts_pitch_target; the definition:
// include/xdtts.h): the argument rules, the quefrency range, the per-value functions of the utterance stage (median of five,
// ratio of one frame) and the reference of that stage from given raw / strength arrays.
// Plain C++, no HIP and none of the library's headers: tests/f0_plan_test.cpp drives it with plain g++.  Everything the device
// shares carries F0_HD -- f0.hip's k_f0_track is the lane loops and the LDS selection around these functions.  The stage
// compares and selects; its only arithmetic is the ratio, where every operation is rounded to fp32 on its own (contraction is
// off) and log2 / exp2 are taken in double and rounded once, so that host, device and a numpy restatement agree.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define F0_HD __host__ __device__ __attribute__((always_inline))
#else
#define F0_HD
#endif
#ifdef __clang__
#define F0_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define F0_NO_CONTRACT  // (g++ on x86-64 without -mfma has no fused instruction to contract into)
#endif

namespace xdtts {

constexpr double F0_SAMPLE_RATE = 22050.0;
constexpr size_t F0_MAX_FRAMES = 16384;          // one workgroup holds an utterance's values in LDS: the contour's limit
constexpr size_t F0_MAX_ROWS = (size_t)1 << 20;  // frames of one call in all (the analysis entries' limit)
constexpr int F0_MEDIAN_HALF = 2;                // the running median spans |u - t| <= 2

struct F0Opts {  // the layout of xdtts_f0_opts
  float fmin, fmax, threshold, octave_bias, log_floor;
};
struct PitchTarget {  // the layout of xdtts_pitch_target
  int32_t mode;
  float value, range;
};
struct F0Stats {  // the layout of xdtts_f0_stats
  int32_t n_frames, n_voiced, n_clamped;
  float median_hz, min_hz, max_hz, base_ratio;
};

inline F0Opts f0_opts_default() { return {60.0f, 400.0f, 0.2f, 0.9f, 1e-5f}; }
inline PitchTarget pitch_target_default() { return {0, 1.0f, 1.0f}; }

// q_lo = ceil(22050 / fmax), q_hi = floor(22050 / fmin), in double
inline void f0_quefrency(const F0Opts &o, int *q_lo, int *q_hi) {
  *q_lo = (int)std::ceil(F0_SAMPLE_RATE / (double)o.fmax);
  *q_hi = (int)std::floor(F0_SAMPLE_RATE / (double)o.fmin);
}

// "" if the options define a tracker, else the message: it names the field
inline std::string f0_opts_check(const F0Opts &o) {
  char msg[160];
  auto say = [&](const char *field, double v, const char *rule) {
    std::snprintf(msg, sizeof msg, "f0 opts: %s %g %s", field, v, rule);
    return std::string(msg);
  };
  if (!std::isfinite(o.fmin) || o.fmin < 50.0f) return say("fmin", o.fmin, "is not in [50, fmax)");
  if (!std::isfinite(o.fmax) || o.fmax > 1000.0f) return say("fmax", o.fmax, "is not in (fmin, 1000]");
  if (!(o.fmin < o.fmax)) return say("fmin", o.fmin, "is not below fmax");
  if (!std::isfinite(o.threshold) || o.threshold < 0.0f) return say("threshold", o.threshold, "is not a number >= 0");
  if (!std::isfinite(o.octave_bias) || !(o.octave_bias > 0.0f) || o.octave_bias > 1.0f) return say("octave_bias", o.octave_bias, "is not in (0, 1]");
  if (!std::isfinite(o.log_floor) || !(o.log_floor > 0.0f)) return say("log_floor", o.log_floor, "is not a positive number");
  int lo, hi;
  f0_quefrency(o, &lo, &hi);
  if (!(lo < hi)) {
    std::snprintf(msg, sizeof msg, "f0 opts: fmin %g and fmax %g leave no quefrency range (q_lo %d, q_hi %d)", (double)o.fmin, (double)o.fmax, lo, hi);
    return msg;
  }
  return "";
}

// "" if the target may be applied, else the message: it names the field
inline std::string pitch_target_check(const PitchTarget &t) {
  char msg[160];
  if (t.mode < 0 || t.mode > 2) {
    std::snprintf(msg, sizeof msg, "pitch target: mode %d is not 0 (none), 1 (Hz) or 2 (factor)", (int)t.mode);
    return msg;
  }
  if (t.mode == 1 && (!std::isfinite(t.value) || t.value < 50.0f || t.value > 1000.0f)) {
    std::snprintf(msg, sizeof msg, "pitch target: value %g Hz is not in [50, 1000]", (double)t.value);
    return msg;
  }
  if (t.mode == 2 && (!std::isfinite(t.value) || t.value < 0.5f || t.value > 2.0f)) {
    std::snprintf(msg, sizeof msg, "pitch target: value %g (a factor) is not in [0.5, 2]", (double)t.value);
    return msg;
  }
  if (!std::isfinite(t.range) || t.range < 0.0f || t.range > 4.0f) {
    std::snprintf(msg, sizeof msg, "pitch target: range %g is not in [0, 4]", (double)t.range);
    return msg;
  }
  return "";
}

// The target that launches nothing: range 1 with no pitch, or with the factor 1 (mode 0 ignores `value`)
inline bool pitch_target_is_identity(const PitchTarget &t) { return t.range == 1.0f && (t.mode == 0 || (t.mode == 2 && t.value == 1.0f)); }

// ---- the utterance stage, value by value.  A raw F0 is a positive float, so the order of the values is the order of their
// bit patterns: every selection below works on those (0 = unvoiced). ----
F0_HD inline uint32_t f0_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}
F0_HD inline float f0_float(uint32_t u) {
  float x;
  memcpy(&x, &u, sizeof x);
  return x;
}
F0_HD inline bool f0_is_voiced(float strength, float threshold) { return strength >= threshold; }  // (NaN: unvoiced)

// The lower median of the voiced (non-zero) entries of w[0 .. n), n <= 5: index (count - 1) / 2 of the sorted; 0 if none
F0_HD inline uint32_t f0_median5(const uint32_t *w, int n) {
  uint32_t s[2 * F0_MEDIAN_HALF + 1];
  int cnt = 0;
  for (int i = 0; i < n && i < 2 * F0_MEDIAN_HALF + 1; ++i) {
    const uint32_t v = w[i];
    if (!v) continue;
    int j = cnt++;
    for (; j > 0 && s[j - 1] > v; --j) s[j] = s[j - 1];
    s[j] = v;
  }
  return cnt ? s[(cnt - 1) / 2] : 0u;
}

// log2 and exp2 of a float, correctly rounded (double, rounded once)
F0_HD inline float f0_log2(float x) { return (float)log2((double)x); }
F0_HD inline float f0_exp2(float x) { return (float)exp2((double)x); }

// What the frames of an utterance share: base, its log2 and the median's
struct F0Base {
  float base, lb, lm, rm1;  // rm1 = range - 1
};
F0_HD inline F0Base f0_base(const PitchTarget &t, int n_voiced, float median_hz) {
  F0_NO_CONTRACT
  F0Base b;
  b.base = 1.0f;
  if (n_voiced > 0) b.base = t.mode == 1 ? t.value / median_hz : (t.mode == 2 ? t.value : 1.0f);
  b.lb = f0_log2(b.base);
  b.lm = n_voiced > 0 ? f0_log2(median_hz) : 0.0f;
  b.rm1 = n_voiced > 0 ? t.range - 1.0f : 0.0f;
  return b;
}
// ratio[t] before the clamp (f0 = 0: an unvoiced frame) ...
F0_HD inline float f0_ratio_raw(const F0Base &b, float f0) {
  F0_NO_CONTRACT
  if (!(f0 > 0.0f)) return b.base;
  const float d = f0_log2(f0) - b.lm;
  const float pr = b.rm1 * d;
  const float x = b.lb + pr;
  return f0_exp2(x);
}
// ... and the clamp, of the ratio and of a table's pitch alike
F0_HD inline float f0_clamp(float r) { return fminf(fmaxf(r, 0.5f), 2.0f); }
F0_HD inline float f0_table_pitch(float contour_pitch, float ratio) {
  F0_NO_CONTRACT
  const float p = contour_pitch * ratio;
  return f0_clamp(p);
}

// The reference of the utterance stage: raw[F], strength[F] -> f0[F], ratio[F] (either may be null) and the stats.
// (checked arguments; F >= 1)
inline void f0_track_reference(const float *raw, const float *strength, size_t F, const F0Opts &o, const PitchTarget &t, float *f0_out,
                               float *ratio_out, F0Stats *stats) {
  std::vector<uint32_t> v(F), f0(F);
  for (size_t i = 0; i < F; ++i) v[i] = f0_is_voiced(strength[i], o.threshold) ? f0_bits(raw[i]) : 0u;
  std::vector<uint32_t> voiced;
  for (size_t i = 0; i < F; ++i) {
    const size_t a = i >= (size_t)F0_MEDIAN_HALF ? i - F0_MEDIAN_HALF : 0, b = std::min(F - 1, i + F0_MEDIAN_HALF);
    f0[i] = v[i] ? f0_median5(&v[a], (int)(b - a + 1)) : 0u;
    if (f0[i]) voiced.push_back(f0[i]);
  }
  F0Stats s{};
  s.n_frames = (int32_t)F;
  s.n_voiced = (int32_t)voiced.size();
  if (!voiced.empty()) {
    std::sort(voiced.begin(), voiced.end());
    s.median_hz = f0_float(voiced[(voiced.size() - 1) / 2]);
    s.min_hz = f0_float(voiced.front());
    s.max_hz = f0_float(voiced.back());
  }
  const F0Base b = f0_base(t, s.n_voiced, s.median_hz);
  s.base_ratio = b.base;
  for (size_t i = 0; i < F; ++i) {
    const float r = f0_ratio_raw(b, f0_float(f0[i])), rc = f0_clamp(r);
    if (f0_bits(rc) != f0_bits(r)) ++s.n_clamped;
    if (f0_out) f0_out[i] = f0_float(f0[i]);
    if (ratio_out) ratio_out[i] = rc;
  }
  if (stats) *stats = s;
}

}  // namespace xdtts
