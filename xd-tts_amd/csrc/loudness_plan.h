// loudness_plan.h -- the host arithmetic of the loudness stage (xdtts_griffinlim_set_loudness, include/xdtts.h): the rate rule,
// the K-weighting coefficients, the state-transition matrix of the cascade and the powers the device scan reads, the block
// plan (h, nb), the two gate constants, the true-peak taps and the gain rule.  Every caller -- the host entries, the
// measurement hooks, the request paths, loudness.hip -- gets them here.
// Plain C++, no HIP and none of the library's headers but resample_plan.h (the I0 series): tests/loudness_plan_test.cpp drives
// it with plain g++.  The two functions the device shares (the filter step, the gain rule) carry LOUD_HD.
#pragma once
#include "resample_plan.h"

#ifdef __HIPCC__
#define LOUD_HD __host__ __device__
#else
#define LOUD_HD
#endif

namespace xdtts {

constexpr int LOUD_RATE_MIN = RESAMPLE_RATE_MIN, LOUD_RATE_MAX = RESAMPLE_RATE_MAX;
constexpr int LOUD_SEG = 32;            // samples a lane runs serially: one segment
constexpr int LOUD_SEG_LOG2 = 5;
constexpr int LOUD_LANES = 64;          // segments of a workgroup (one wave): the in-wave scan needs no LDS
constexpr int LOUD_GROUP = LOUD_SEG * LOUD_LANES;  // 2048 samples of one utterance per workgroup
constexpr int LOUD_GROUP_LOG2 = 11;
constexpr int LOUD_POW = 17;            // A^(2^k), k = 0 .. 16: the scan over segments reads 5 .. 10, the scan over groups 11 .. 16
constexpr int LOUD_TP_TAPS = 24, LOUD_TP_PHASES = 3, LOUD_TP_HALF = 12;  // taps j = -12 .. 11 of a phase
constexpr double LOUD_TP_BETA = 8.0;
constexpr double LOUD_OFFSET = -0.691;  // L = LOUD_OFFSET + 10 log10 Z

// "" if the rate is supported, else the message: it names the rate and the rule
inline std::string loudness_check(long long rate) {
  char msg[160];
  if (rate < LOUD_RATE_MIN || rate > LOUD_RATE_MAX) {
    std::snprintf(msg, sizeof msg, "loudness: rate %lld is not in [%d, %d]", rate, LOUD_RATE_MIN, LOUD_RATE_MAX);
    return msg;
  }
  return "";
}

// The target (LUFS) and the ceiling (dBTP) of xdtts_griffinlim_set_loudness: NaN target = off (the ceiling is then not looked
// at beyond its own range), else finite in [-70, 0]; the ceiling NaN = none or in [-20, +6].
inline std::string loudness_target_check(float target, float ceiling) {
  char msg[160];
  if (!std::isnan(ceiling) && !(ceiling >= -20.f && ceiling <= 6.f)) {
    std::snprintf(msg, sizeof msg, "loudness: ceiling %g dBTP is not in [-20, 6] (NaN = none)", (double)ceiling);
    return msg;
  }
  if (!std::isnan(target) && !(target >= -70.f && target <= 0.f)) {
    std::snprintf(msg, sizeof msg, "loudness: target %g LUFS is not in [-70, 0] (NaN = off)", (double)target);
    return msg;
  }
  return "";
}

// coef[10]: the high-shelf's b0 b1 b2 a1 a2, then the high-pass's b0 b1 b2 a1 a2 (a0 = 1 in both), by the bilinear transform
// of the BS.1770 analogue prototypes with K = tan(pi f0 / Q).
inline void loudness_coef(int rate, double coef[10]) {
  const double PI = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Qf = 0.7071752369554196;
    const double K = std::tan(PI * f0 / (double)rate);
    const double Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Qf + K * K;
    coef[0] = (Vh + Vb * K / Qf + K * K) / a0;
    coef[1] = 2.0 * (K * K - Vh) / a0;
    coef[2] = (Vh - Vb * K / Qf + K * K) / a0;
    coef[3] = 2.0 * (K * K - 1.0) / a0;
    coef[4] = (1.0 - K / Qf + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Qf = 0.5003270373238773;
    const double K = std::tan(PI * f0 / (double)rate);
    const double a0 = 1.0 + K / Qf + K * K;
    coef[5] = 1.0;
    coef[6] = -2.0;
    coef[7] = 1.0;
    coef[8] = 2.0 * (K * K - 1.0) / a0;
    coef[9] = (1.0 - K / Qf + K * K) / a0;
  }
}

// One sample through the cascade, both biquads in the transposed direct form II; s[4] = the shelf's two states, then the
// high-pass's.  Linear in (s, x): s' = A s + B x -- what the segment scan rests on.
// (R = double everywhere but in the fp32 comparison form of loudness.hip)
template <typename R>
LOUD_HD inline R loudness_step(const R *c, R *s, R x) {
  const R y1 = c[0] * x + s[0];
  s[0] = c[1] * x - c[3] * y1 + s[1];
  s[1] = c[2] * x - c[4] * y1;
  const R y2 = c[5] * y1 + s[2];
  s[2] = c[6] * y1 - c[8] * y2 + s[3];
  s[3] = c[7] * y1 - c[9] * y2;
  return y2;
}

// A (row major, 4 x 4): column i = one step from the unit state e_i with x = 0
inline void loudness_transition(const double coef[10], double A[16]) {
  for (int i = 0; i < 4; ++i) {
    double s[4] = {0, 0, 0, 0};
    s[i] = 1.0;
    loudness_step(coef, s, 0.0);
    for (int r = 0; r < 4; ++r) A[r * 4 + i] = s[r];
  }
}

inline void loudness_matmul(const double X[16], const double Y[16], double out[16]) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a += X[r * 4 + k] * Y[k * 4 + c];
      out[r * 4 + c] = a;
    }
}

// What the device reads for one rate: the coefficients, A^(2^k) for k < LOUD_POW (by repeated squaring, in double), and the
// true-peak taps.  A segment of 2^5 samples advances a state by pw[5], a group by pw[11].
struct LoudnessTable {
  double coef[10];
  double pw[LOUD_POW][16];
  float taps[LOUD_TP_PHASES][LOUD_TP_TAPS];
  int rate, pad;
};

// taps[p - 1][j + 12] = t[4 j + p], p = 1 .. 3, j = -12 .. 11;  t[k] = sinc(k / 4) I0(8 sqrt(1 - (k / 48)^2)) / I0(8), in
// double, rounded once
inline void loudness_true_peak_taps(float taps[LOUD_TP_PHASES][LOUD_TP_TAPS]) {
  const double PI = 3.14159265358979323846;
  const double i0b = resample_i0(LOUD_TP_BETA);
  for (int p = 1; p <= LOUD_TP_PHASES; ++p)
    for (int j = -LOUD_TP_HALF; j < LOUD_TP_HALF; ++j) {
      const int k = 4 * j + p;
      const double x = (double)k / 4.0, u = (double)k / 48.0;
      const double s = std::sin(PI * x) / (PI * x);  // (k is never a multiple of 4)
      taps[p - 1][j + LOUD_TP_HALF] = (float)(s * resample_i0(LOUD_TP_BETA * std::sqrt(1.0 - u * u)) / i0b);
    }
}

inline void loudness_table(int rate, LoudnessTable &t) {
  loudness_coef(rate, t.coef);
  loudness_transition(t.coef, t.pw[0]);
  for (int k = 1; k < LOUD_POW; ++k) loudness_matmul(t.pw[k - 1], t.pw[k - 1], t.pw[k]);
  loudness_true_peak_taps(t.taps);
  t.rate = rate;
  t.pad = 0;
}

// h = (Q + 5) / 10: 100 ms; a block is 4 h samples, block j covers [j h, j h + 4 h)
inline int loudness_hop(int rate) { return (rate + 5) / 10; }
inline size_t loudness_blocks(int rate, size_t n) {
  const size_t h = (size_t)loudness_hop(rate);
  return n >= 4 * h ? (n - 4 * h) / h + 1 : 0;
}
inline size_t loudness_sub_blocks(int rate, size_t n) {  // 100 ms stretches a sample of the utterance falls into (the last may be short)
  const size_t h = (size_t)loudness_hop(rate);
  return (n + h - 1) / h;
}
inline size_t loudness_segments(size_t n) { return (n + LOUD_SEG - 1) / LOUD_SEG; }
inline size_t loudness_groups(size_t n) { return (n + LOUD_GROUP - 1) / LOUD_GROUP; }

// The gates, on z (mean squares): absolute z > 10^((-70 + 0.691) / 10), relative z > 0.1 mean(z over the absolutely gated)
inline double loudness_abs_gate() { return std::pow(10.0, (-70.0 - LOUD_OFFSET) / 10.0); }
constexpr double LOUD_REL_GATE = 0.1;

// The gain rule with its two constants in linear form: tgt = 10^((T + 0.691) / 20); ceil = 10^(C / 20), or 0 for no ceiling.
// Z = 0 (nothing passed the gates) leaves the utterance unscaled.
inline double loudness_target_lin(float target) { return std::pow(10.0, ((double)target - LOUD_OFFSET) / 20.0); }
inline double loudness_ceiling_lin(float ceiling) { return std::isnan(ceiling) ? 0.0 : std::pow(10.0, (double)ceiling / 20.0); }
LOUD_HD inline double loudness_gain(double Z, double true_peak, double tgt, double ceil) {
  if (!(Z > 0.0)) return 1.0;
#ifdef __HIP_DEVICE_COMPILE__
  double gain = tgt / __dsqrt_rn(Z);  // (IEEE square root: a function of Z alone)
#else
  double gain = tgt / std::sqrt(Z);
#endif
  if (ceil > 0.0 && gain * true_peak > ceil) gain = ceil / true_peak;
  return gain;
}

// The measurement on the host, in double, sample by sample: the plain restatement the driver and the tools compare against.
struct LoudnessHost {
  double mean_square = 0.0, true_peak = 0.0, sample_peak = 0.0;
  int blocks = 0, gated = 0;
};
inline LoudnessHost loudness_measure_host(int rate, const float *x, size_t n) {
  LoudnessHost r;
  LoudnessTable t;
  loudness_table(rate, t);
  const size_t h = (size_t)loudness_hop(rate), nb = loudness_blocks(rate, n), nsb = loudness_sub_blocks(rate, n);
  std::vector<double> sub(nsb + 1, 0.0);
  double s[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const double y = loudness_step(t.coef, s, (double)x[i]);
    sub[i / h] += y * y;
    r.sample_peak = std::fmax(r.sample_peak, std::fabs((double)x[i]));
    for (int p = 0; p < LOUD_TP_PHASES; ++p) {
      double a = 0.0;
      for (int j = -LOUD_TP_HALF; j < LOUD_TP_HALF; ++j) {
        const long long m = (long long)i - j;
        if (m >= 0 && m < (long long)n) a += (double)x[m] * (double)t.taps[p][j + LOUD_TP_HALF];
      }
      r.true_peak = std::fmax(r.true_peak, std::fabs(a));
    }
  }
  r.true_peak = std::fmax(r.true_peak, r.sample_peak);
  r.blocks = (int)nb;
  std::vector<double> z(nb);
  double sa = 0.0;
  int na = 0;
  const double abs_gate = loudness_abs_gate();
  for (size_t j = 0; j < nb; ++j) {
    z[j] = ((sub[j] + sub[j + 1]) + (sub[j + 2] + sub[j + 3])) / (double)(4 * h);
    if (z[j] > abs_gate) sa += z[j], ++na;
  }
  if (!na) return r;
  const double rel = LOUD_REL_GATE * (sa / na);
  double sg = 0.0;
  for (size_t j = 0; j < nb; ++j)
    if (z[j] > abs_gate && z[j] > rel) sg += z[j], ++r.gated;
  if (r.gated) r.mean_square = sg / r.gated;
  return r;
}

inline double loudness_lufs(double mean_square) {
  return mean_square > 0.0 ? LOUD_OFFSET + 10.0 * std::log10(mean_square) : -INFINITY;
}

}  // namespace xdtts
