// Stand-alone driver of xd-tts_amd/csrc/loudness_plan.h (plain g++, no HIP, no library): the rate rule and the argument rule,
// the BS.1770 coefficient table at 48 kHz, the block plan, the true-peak taps, the gain rule, and the three-phase scan walked
// exactly as loudness.hip walks it -- local runs from zero, the in-wave scan with A^(32 2^k), the carry over groups with
// A^(2048 2^k), the re-run from the true state into at most two sub-blocks a segment, the sub-block sums in ascending order,
// the gates -- with every index bounds-checked, against the sample-by-sample measurement of the same header.  Built with
// -fsanitize=address,undefined by tests/test_loudness_cpu.py.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loudness_plan.h"

using namespace xdtts;

#define REQUIRE(c)                                             \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                \
    }                                                          \
  } while (0)

static void apply(const double *M, double v[4]) {
  const double a = v[0], b = v[1], c = v[2], d = v[3];
  for (int r = 0; r < 4; ++r) v[r] = (M[r * 4] * a + M[r * 4 + 1] * b) + (M[r * 4 + 2] * c + M[r * 4 + 3] * d);
}

typedef std::vector<std::vector<double>> States;  // [element][4]

// wave_scan of loudness.hip on 64 states: s_{i+1} = M s_i + z_i, Hillis-Steele with pw[k0 + k]
static void wave_scan(const LoudnessTable &t, int k0, States &s) {
  for (int k = 0; k < 6; ++k) {
    States prev = s;
    for (int lane = 0; lane < LOUD_LANES; ++lane) {
      if (lane < (1 << k)) continue;
      double v[4];
      for (int i = 0; i < 4; ++i) v[i] = prev.at((size_t)(lane - (1 << k))).at((size_t)i);
      apply(t.pw[k0 + k], v);
      for (int i = 0; i < 4; ++i) s.at((size_t)lane).at((size_t)i) += v[i];
    }
  }
}

// The four measuring kernels on the host.  Returns false on an index the kernels must never form.
static bool scan_measure(int rate, const std::vector<float> &x, LoudnessHost &out) {
  LoudnessTable t;
  loudness_table(rate, t);
  const int n = (int)x.size(), h = loudness_hop(rate);
  const int G = (int)loudness_groups((size_t)n), nseg = (int)loudness_segments((size_t)n), nsb = (int)loudness_sub_blocks(rate, (size_t)n);
  const int nb = (int)loudness_blocks(rate, (size_t)n);
  if (h <= LOUD_SEG) return false;
  if (nsb > 3 * G + 1) return false;  // the scratch the handle sizes
  auto at = [&](long long i) { return (i >= 0 && i < n) ? x.at((size_t)i) : 0.f; };
  States excl((size_t)nseg, std::vector<double>(4, 0.0)), agg((size_t)G, std::vector<double>(4, 0.0)), gin = agg;
  // k_loud_local
  for (int g = 0; g < G; ++g) {
    States s((size_t)LOUD_LANES, std::vector<double>(4, 0.0));
    for (int lane = 0; lane < LOUD_LANES; ++lane)
      for (int i = 0; i < LOUD_SEG; ++i) loudness_step(t.coef, s.at((size_t)lane).data(), (double)at((long long)g * LOUD_GROUP + lane * LOUD_SEG + i));
    wave_scan(t, LOUD_SEG_LOG2, s);
    for (int lane = 0; lane < LOUD_LANES; ++lane) {
      const int seg = g * LOUD_LANES + lane;
      if (seg < nseg && lane > 0) excl.at((size_t)seg) = s.at((size_t)lane - 1);
    }
    agg.at((size_t)g) = s.at(LOUD_LANES - 1);
  }
  // k_loud_carry
  std::vector<double> carry(4, 0.0);
  for (int g0 = 0; g0 < G; g0 += LOUD_LANES) {
    States v((size_t)LOUD_LANES, std::vector<double>(4, 0.0));
    for (int lane = 0; lane < LOUD_LANES; ++lane)
      if (g0 + lane < G) v.at((size_t)lane) = agg.at((size_t)(g0 + lane));
    double pc[4] = {carry[0], carry[1], carry[2], carry[3]};
    apply(t.pw[LOUD_GROUP_LOG2], pc);
    for (int i = 0; i < 4; ++i) v.at(0).at((size_t)i) += pc[i];
    wave_scan(t, LOUD_GROUP_LOG2, v);
    for (int lane = 0; lane < LOUD_LANES; ++lane)
      if (g0 + lane < G) gin.at((size_t)(g0 + lane)) = lane ? v.at((size_t)lane - 1) : carry;
    carry = v.at(LOUD_LANES - 1);
  }
  // k_loud_energy
  std::vector<double> part((size_t)nseg * 2, 0.0);
  for (int seg = 0; seg < nseg; ++seg) {
    const int g = seg / LOUD_LANES, lane = seg % LOUD_LANES;
    double v[4], s[4];
    for (int i = 0; i < 4; ++i) v[i] = gin.at((size_t)g).at((size_t)i);
    for (int k = 0; k < 6; ++k)
      if ((lane >> k) & 1) apply(t.pw[LOUD_SEG_LOG2 + k], v);
    for (int i = 0; i < 4; ++i) s[i] = excl.at((size_t)seg).at((size_t)i) + v[i];
    const int n0 = seg * LOUD_SEG, edge = (n0 / h + 1) * h - n0, len = std::min(LOUD_SEG, n - n0);
    for (int i = 0; i < LOUD_SEG; ++i) {
      const double y = loudness_step(t.coef, s, (double)at(n0 + i));
      const double yy = i < len ? y * y : 0.0;
      part.at((size_t)seg * 2 + (i < edge ? 0 : 1)) += yy;
    }
  }
  // k_loud_final
  std::vector<double> sub((size_t)nsb, 0.0);
  for (int b = 0; b < nsb; ++b) {
    const int k_lo = (int)(((long long)b * h) >> LOUD_SEG_LOG2);
    const int k_hi = std::min((int)((((long long)(b + 1) * h) - 1) >> LOUD_SEG_LOG2), nseg - 1);
    for (int k = k_lo; k <= k_hi; ++k) {
      const int slot = b - (k * LOUD_SEG) / h;
      if (slot < 0 || slot > 1) return false;
      sub.at((size_t)b) += part.at((size_t)k * 2 + (size_t)slot);
    }
  }
  out = LoudnessHost();
  out.blocks = nb;
  const double inv = 1.0 / (double)(4 * h), abs_gate = loudness_abs_gate();
  double sa = 0.0, sg = 0.0;
  int na = 0;
  std::vector<double> z((size_t)nb);
  for (int j = 0; j < nb; ++j) {
    z.at((size_t)j) = ((sub.at((size_t)j) + sub.at((size_t)j + 1)) + (sub.at((size_t)j + 2) + sub.at((size_t)j + 3))) * inv;
    if (z[(size_t)j] > abs_gate) sa += z[(size_t)j], ++na;
  }
  if (na) {
    const double rel = LOUD_REL_GATE * (sa / na);
    for (int j = 0; j < nb; ++j)
      if (z[(size_t)j] > abs_gate && z[(size_t)j] > rel) sg += z[(size_t)j], ++out.gated;
    if (out.gated) out.mean_square = sg / out.gated;
  }
  return true;
}

static std::vector<float> signal(int rate, int n, unsigned seed) {
  std::vector<float> x((size_t)n);
  unsigned s = seed * 2654435761u + 12345u;
  for (int i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    const double noise = ((double)(s >> 8) / (double)(1u << 24) - 0.5) * 0.1;
    const double pos = (double)i / (double)n;
    double v = 0.3 * std::sin(2.0 * 3.14159265358979323846 * 220.0 * i / rate) + noise;
    if (pos >= 0.4 && pos < 0.6) v *= 0.01;
    if (pos >= 0.6 && pos < 0.8) v = 0.0;
    x[(size_t)i] = (float)v;
  }
  return x;
}

int main() {
  // the rate rule and the argument rule
  const long long bad[] = {7999, 96001, 0, -1, 1LL << 33};
  for (long long r : bad) REQUIRE(!loudness_check(r).empty());
  const int rates[] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000, 8001, 95999};
  for (int r : rates) REQUIRE(loudness_check(r).empty());
  REQUIRE(loudness_target_check(NAN, NAN).empty() && loudness_target_check(-16.f, -1.f).empty() && loudness_target_check(0.f, 6.f).empty());
  REQUIRE(loudness_target_check(-70.f, -20.f).empty() && loudness_target_check(NAN, -1.f).empty());
  REQUIRE(!loudness_target_check(0.5f, NAN).empty() && !loudness_target_check(-70.5f, NAN).empty() && !loudness_target_check(INFINITY, NAN).empty());
  REQUIRE(!loudness_target_check(-16.f, 6.5f).empty() && !loudness_target_check(-16.f, -21.f).empty() && !loudness_target_check(NAN, INFINITY).empty());

  // the coefficient table of BS.1770 at 48 kHz
  {
    double c[10];
    loudness_coef(48000, c);
    const double want[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
    for (int i = 0; i < 10; ++i) REQUIRE(std::fabs(c[i] - want[i]) < 1e-12);
  }

  // the plan
  REQUIRE(loudness_hop(11025) == 1103 && loudness_hop(8000) == 800 && loudness_hop(96000) == 9600 && loudness_hop(22050) == 2205);
  for (int r : rates) {
    const size_t h = (size_t)loudness_hop(r);
    REQUIRE(h > (size_t)LOUD_SEG);
    REQUIRE(loudness_blocks(r, 0) == 0 && loudness_blocks(r, 4 * h - 1) == 0 && loudness_blocks(r, 4 * h) == 1);
    REQUIRE(loudness_blocks(r, 5 * h - 1) == 1 && loudness_blocks(r, 5 * h) == 2 && loudness_blocks(r, 10 * h + 7) == 7);
  }

  // the powers: pw[k] = A^(2^k); a state moved by pw[5] equals 32 silent steps
  for (int r : rates) {
    LoudnessTable t;
    loudness_table(r, t);
    double s[4] = {0.3, -0.2, 0.7, 0.1}, v[4] = {0.3, -0.2, 0.7, 0.1};
    for (int i = 0; i < LOUD_SEG; ++i) loudness_step(t.coef, s, 0.0);
    apply(t.pw[LOUD_SEG_LOG2], v);
    for (int i = 0; i < 4; ++i) REQUIRE(std::fabs(s[i] - v[i]) < 1e-12);
    for (int k = 0; k < LOUD_POW; ++k)
      for (int i = 0; i < 16; ++i) REQUIRE(std::isfinite(t.pw[k][i]));
  }

  // the true-peak taps: 24 a phase, phase 2 symmetric about its centre, phases 1 and 3 mirror images, DC gain 1 within 1e-3
  {
    float taps[LOUD_TP_PHASES][LOUD_TP_TAPS];
    loudness_true_peak_taps(taps);
    for (int j = 0; j < LOUD_TP_TAPS; ++j) {
      REQUIRE(taps[1][j] == taps[1][LOUD_TP_TAPS - 1 - j]);
      REQUIRE(taps[0][j] == taps[2][LOUD_TP_TAPS - 1 - j]);
    }
    for (int p = 0; p < LOUD_TP_PHASES; ++p) {
      double dc = 0;
      for (int j = 0; j < LOUD_TP_TAPS; ++j) dc += taps[p][j];
      REQUIRE(std::fabs(dc - 1.0) < 1e-3);
    }
  }

  // the gain rule
  {
    const double tgt = loudness_target_lin(-16.f), Z = 0.01;
    REQUIRE(loudness_gain(0.0, 0.5, tgt, 0.0) == 1.0);
    const double g = loudness_gain(Z, 0.5, tgt, 0.0);
    REQUIRE(std::fabs(loudness_lufs(g * g * Z) - (-16.0)) < 1e-9);
    const double ceil = loudness_ceiling_lin(-20.f), gc = loudness_gain(Z, 0.5, tgt, ceil);
    REQUIRE(gc < g && std::fabs(gc * 0.5 - ceil) < 1e-15);
    REQUIRE(loudness_gain(Z, 0.5, tgt, loudness_ceiling_lin(6.f)) == g);
    REQUIRE(loudness_ceiling_lin(NAN) == 0.0 && std::isinf(loudness_lufs(0.0)));
  }

  // the scan against the sample-by-sample measurement: every branch of the lengths
  const int scan_rates[] = {8000, 11025, 22050, 48000, 96000};
  for (int r : scan_rates) {
    const int h = loudness_hop(r);
    const int lens[] = {1, 31, 32, 33, 2047, 2048, 2049, 4 * h - 1, 4 * h, 5 * h - 1, 5 * h + 1, 25 * h + 13};
    for (int n : lens) {
      const std::vector<float> x = signal(r, n, (unsigned)(r + n));
      LoudnessHost a, b = loudness_measure_host(r, x.data(), x.size());
      REQUIRE(scan_measure(r, x, a));
      REQUIRE(a.blocks == b.blocks && a.gated == b.gated);
      REQUIRE(std::fabs(a.mean_square - b.mean_square) <= 1e-9 * b.mean_square);
      if (n >= 25 * h) REQUIRE(b.gated > 0 && b.gated < b.blocks);
    }
  }
  {  // more than 64 groups: the carry of a step of the group scan
    const int r = 8000, n = 70 * LOUD_GROUP + 5;
    const std::vector<float> x = signal(r, n, 7u);
    LoudnessHost a, b = loudness_measure_host(r, x.data(), x.size());
    REQUIRE(scan_measure(r, x, a));
    REQUIRE(a.blocks == b.blocks && a.gated == b.gated && std::fabs(a.mean_square - b.mean_square) <= 1e-9 * b.mean_square);
  }
  std::printf("ok\n");
  return 0;
}
