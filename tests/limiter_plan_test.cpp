// Stand-alone driver of csrc/limiter_plan.h (plain g++, built with -fsanitize=address,undefined by tests/test_limiter_cpu.py):
// the argument rules, H and the window against their definitions, and the walk of k_limit -- staging with zero extension, the
// peak values, r at the sample's own slot, the vote, the doubling ping-pong, the flags, the skipped FIR rounds -- run on the
// host exactly as a workgroup runs it, tile by tile, with buffers of the exact size (the sanitizer sees every index), and
// compared bit for bit, samples and stats, with the sample-by-sample reference at every shape the GPU tests use.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "limiter_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// the features of tests/limiter_ref.py's signal: a floor at -40 dB, impulses at both ends and at both sides of the first tile
// boundary, two peaks 2 H - 1 apart, two peaks 4 H + 2 apart, a plateau longer than 2 H + 1, a burst at a quarter of the rate
static std::vector<float> signal(size_t N, int H, float floor_amp) {
  std::vector<float> x(N);
  uint32_t s = 12345u + (uint32_t)N * 2654435761u + (uint32_t)H;
  for (size_t i = 0; i < N; ++i) {
    s = s * 1664525u + 1013904223u;
    x[i] = floor_amp * ((float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f);
  }
  auto put = [&](long long i, float v) {
    if (i >= 0 && i < (long long)N) x[(size_t)i] = v;
  };
  put(0, 0.9f);
  put((long long)N - 1, -0.8f);
  put(LIM_TILE - 1, 0.7f);
  put(LIM_TILE, -0.95f);
  long long at = 40;
  put(at, 0.85f);
  put(at + 2 * H - 1, -0.6f);
  at += 2 * H - 1 + 3 * H;
  put(at, 0.75f);
  put(at + 4 * H + 2, 0.65f);
  at += 4 * H + 2 + 3 * H;
  for (long long i = at; i < at + 2 * H + 40; ++i) put(i, 0.5f);
  at += 2 * H + 40 + 3 * H;
  for (int k = 0; k < 512; ++k) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * k / 511.0);
    if (at + k < (long long)N) x[(size_t)(at + k)] += (float)(0.9 * std::sin(3.14159265358979323846 / 2.0 * k + 3.14159265358979323846 / 4.0) * w);
  }
  return x;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

struct Walk {
  LimiterStats st;
  int scale_tiles = 0, skipped = 0, run = 0;
};
static Walk walk(const std::vector<float> &x, int rate, int us, double gain0, double ceil, std::vector<float> &out) {
  const int H = limiter_half_width(rate, us);
  float taps[LOUD_TP_PHASES][LOUD_TP_TAPS];
  loudness_true_peak_taps(taps);
  std::vector<float> w((size_t)(2 * H + 1));
  limiter_window(H, w.data());
  out.assign(x.size(), -7.0f);
  Walk r;
  r.st = LimiterStats{1.0f, H, 1, 0};
  const size_t tiles = limiter_tiles(x.size());
  CHECK(tiles * LIM_TILE >= x.size() && (tiles - 1) * LIM_TILE < x.size());
  for (size_t t = 0; t < tiles; ++t) {
    const LimTileStats ts = limiter_tile_walk(x.data(), x.size(), t * LIM_TILE, H, &taps[0][0], w.data(), (float)gain0, (float)ceil, out.data());
    r.st.limited += ts.limited;
    r.st.min_gain = fminf(r.st.min_gain, ts.min_gain);
    r.scale_tiles += ts.scale_route;
    r.skipped += ts.fir_skipped;
    r.run += ts.fir_run;
  }
  return r;
}

int main() {
  // the rules
  CHECK(limiter_half_width(96000, 10000) == 960 && limiter_half_width(8000, 500) == 12 && limiter_half_width(22050, 500) == 12);
  CHECK(limiter_half_width(22050, 5000) == 110 && limiter_half_width(44100, 1500) == 66 && limiter_half_width(11025, 10000) == 110);
  CHECK(limiter_setting_check(0).empty() && limiter_setting_check(500).empty() && limiter_setting_check(10000).empty());
  CHECK(!limiter_setting_check(499).empty() && !limiter_setting_check(10001).empty() && !limiter_setting_check(-1).empty());
  CHECK(!limiter_check(22050, 0).empty() && !limiter_check(7999, 500).empty() && !limiter_check(96001, 500).empty() && limiter_check(8000, 500).empty());
  CHECK(!limiter_args_check(22050, 500, 0, 1.0, 1.0).empty() && !limiter_args_check(22050, 500, LIM_MAX_SAMPLES, 1.0, 1.0).empty());
  CHECK(!limiter_args_check(22050, 500, 1, 1.0, 0.0).empty() && !limiter_args_check(22050, 500, 1, 1.0, -1.0).empty() &&
        !limiter_args_check(22050, 500, 1, 1.0, NAN).empty() && !limiter_args_check(22050, 500, 1, NAN, 1.0).empty() &&
        limiter_args_check(22050, 500, 1, 0.0, 1.0).empty());
  CHECK(lim_lds_floats(LIM_H_MAX) * 4 + 256 <= 65536);
  for (int H : {12, 13, 40, 110, 221, 480, 960}) {
    std::vector<float> w((size_t)(2 * H + 1));
    limiter_window(H, w.data());
    double s = 0.0;
    for (float v : w) s += (double)v;
    CHECK(std::fabs(s - 1.0) < 1e-5 && w[0] > 0.f && w[(size_t)H] >= w[(size_t)H - 1] && w[0] == w[(size_t)(2 * H)]);
    const int P = lim_pow2(H);
    CHECK(P <= 2 * H + 1 && 2 * P > 2 * H + 1 && (P & (P - 1)) == 0);
  }
  // the walk against the reference, at the shapes of the GPU tests
  const double gain0 = 1.7, ceil = 0.7079457843841379;
  int scale_tiles = 0, skipped = 0, run = 0;
  for (int rate : {8000, 22050, 96000})
    for (int us : {500, 5000, 10000}) {
      const int H = limiter_half_width(rate, us);
      const size_t lens[] = {1, (size_t)H, (size_t)(2 * H + 1), LIM_TILE - 1, LIM_TILE, LIM_TILE + 1, (size_t)(2 * LIM_TILE + 2 * H + 5)};
      for (size_t N : lens) {
        const std::vector<float> x = signal(N, H, 0.01f);
        std::vector<float> ref(N), out;
        const LimiterStats a = limiter_reference(x.data(), N, rate, us, gain0, ceil, ref.data());
        const Walk b = walk(x, rate, us, gain0, ceil, out);
        CHECK(same_bits(ref, out));
        CHECK(a.limited == b.st.limited && a.min_gain == b.st.min_gain && a.half_width == H && a.engaged == 1);
        CHECK(a.limited > 0 && a.min_gain < 1.0f);
        scale_tiles += b.scale_tiles;
        skipped += b.skipped;
        run += b.run;
      }
    }
  CHECK(skipped > 0 && run > 0);
  // nothing to limit: every tile takes the scale route, every sample is fl(x G)
  {
    const std::vector<float> x = signal(2 * LIM_TILE + 77, 110, 0.01f);
    std::vector<float> ref(x.size()), out;
    const LimiterStats a = limiter_reference(x.data(), x.size(), 22050, 5000, 0.5, 1.0, ref.data());
    const Walk b = walk(x, 22050, 5000, 0.5, 1.0, out);
    CHECK(same_bits(ref, out) && a.limited == 0 && a.min_gain == 1.0f && b.st.limited == 0 && b.scale_tiles == 3);
    bool scaled = true;
    for (size_t i = 0; i < x.size(); ++i) scaled = scaled && ref[i] == x[i] * 0.5f;
    CHECK(scaled);
  }
  // one peak in a long quiet signal: its tile limits, the others scale; a peak 2 H behind a tile's end reaches into it
  {
    const int H = 110;
    std::vector<float> x(3 * LIM_TILE, 0.001f);
    x[(size_t)(LIM_TILE + 2 * H - 1)] = 1.0f;  // inside tile 1; hold and smoothing reach 2 H back, into tile 0's last sample
    x[(size_t)(2 * LIM_TILE + 5)] = -1.0f;      // inside tile 2, reaches back into tile 1
    std::vector<float> ref(x.size()), out;
    const LimiterStats a = limiter_reference(x.data(), x.size(), 22050, 5000, 1.0, 0.5, ref.data());
    const Walk b = walk(x, 22050, 5000, 1.0, 0.5, out);
    CHECK(same_bits(ref, out) && a.limited == b.st.limited && a.min_gain == b.st.min_gain && a.limited > 0);
    CHECK(b.skipped > 0);
  }
  (void)scale_tiles;
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
