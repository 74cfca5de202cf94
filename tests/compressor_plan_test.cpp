// Stand-alone driver of csrc/compressor_plan.h (plain g++, built with -fsanitize=address,undefined by
// tests/test_compressor_cpu.py): the argument rules, the host integers, lvl and 2^x at their exact points, and the two passes
// of the kernels -- the aggregates and the peak per tile, then the carries within reach, the in-lane / in-wave / cross-segment
// scans in tile-local 32-bit integers, the gain -- run on the host exactly as a workgroup runs them, tile by tile, with buffers
// of the exact size (the sanitizers see every index and every signed sum), and compared bit for bit, samples and stats, with
// the sample-by-sample reference in the serial form at the shapes the GPU tests use.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "compressor_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static std::vector<float> noise(size_t N, float amp, uint32_t seed) {
  std::vector<float> x(N);
  uint32_t s = 12345u + (uint32_t)N * 2654435761u + seed;
  for (size_t i = 0; i < N; ++i) {
    s = s * 1664525u + 1013904223u;
    x[i] = amp * ((float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f);
  }
  return x;
}
// a floor at -50 dB, impulses at both ends and at both sides of every tile boundary, a loud stretch, a stretch of exact zeros
static std::vector<float> signal(size_t N, uint32_t seed) {
  std::vector<float> x = noise(N, 0.003f, seed);
  auto put = [&](long long i, float v) {
    if (i >= 0 && i < (long long)N) x[(size_t)i] = v;
  };
  put(0, 0.9f);
  put((long long)N - 1, -0.8f);
  for (long long t = COMP_TILE; t < (long long)N; t += COMP_TILE) {
    put(t - 1, 0.7f);
    put(t, -0.95f);
  }
  for (long long i = (long long)N / 3; i < (long long)N / 3 + 300; ++i) put(i, (i & 1) ? 0.5f : -0.5f);
  for (long long i = (long long)N / 2 + 1; i < (long long)N / 2 + 501; ++i) put(i, 0.0f);
  return x;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

// the three launches on the host: pass 1 over every tile, then pass 2 over every tile
static CompressorStats walk(const std::vector<float> &x, int rate, const Compressor &c, std::vector<float> &out) {
  const CompPlan p = compressor_plan(c, rate);
  const size_t n = x.size(), tiles = compressor_tiles(n);
  out.assign(n, -7.0f);
  CHECK(tiles * COMP_TILE >= n && (tiles - 1) * COMP_TILE < n);
  std::vector<CompAgg> agg(tiles);
  uint32_t pk = 0;
  for (size_t t = 0; t < tiles; ++t) {
    const CompTile1 a = compressor_tile_pass1(x.data(), n, t * COMP_TILE, p);
    agg[t] = a.agg;
    pk = std::max(pk, a.peak_bits);
  }
  CompressorStats st{0.0f, 0, 0, 0};
  if (pk == 0) {
    out = x;
    return st;
  }
  st.peak = comp_float(pk);
  st.engaged = 1;
  st.max_over = COMP_NEG;
  for (size_t t = 0; t < tiles; ++t) {
    const CompTile2 b = compressor_tile_walk(x.data(), n, t * COMP_TILE, p, agg.data(), (int)tiles, comp_lvl(pk), out.data());
    st.compressed += b.compressed;
    st.max_over = std::max(st.max_over, b.max_over);
  }
  return st;
}

static void against_reference(const std::vector<float> &x, int rate, const Compressor &c, bool want_compressed) {
  std::vector<float> ref(x.size()), out;
  const CompressorStats a = compressor_reference(x.data(), x.size(), rate, c, ref.data());
  const CompressorStats b = walk(x, rate, c, out);
  CHECK(same_bits(ref, out));
  CHECK(a.compressed == b.compressed && a.max_over == b.max_over && a.engaged == b.engaged && comp_bits(a.peak) == comp_bits(b.peak));
  if (want_compressed) {
    CHECK(a.engaged == 1 && a.compressed > 0 && a.max_over == -compressor_plan(c, rate).T);  // (V reaches P at the peak itself)
  }
}

int main() {
  // the rules
  Compressor d = compressor_default(), drc{};
  CHECK(compressor_is_identity(d) && compressor_check(d).empty());
  CHECK(compressor_preset(1, &drc) && drc.threshold_db == -24.0f && drc.ratio == 3.0f && drc.knee_db == 6.0f && drc.attack_ms == 5.0f &&
        drc.release_ms == 100.0f && drc.makeup_db == 0.0f && !compressor_is_identity(drc) && compressor_check(drc).empty());
  CHECK(!compressor_preset(2, &d) && !compressor_preset(-1, &d));
  {
    const float lo[6] = {-60.f, 1.f, 0.f, 0.1f, 1.f, 0.f}, hi[6] = {0.f, 20.f, 24.f, 100.f, 2000.f, 24.f};
    const char *names[6] = {"threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db"};
    for (int i = 0; i < 6; ++i) {
      for (float v : {lo[i], hi[i]}) {
        Compressor c = drc;
        reinterpret_cast<float *>(&c)[i] = v;
        CHECK(compressor_check(c).empty());
      }
      for (float v : {std::nextafterf(lo[i], -INFINITY), std::nextafterf(hi[i], INFINITY), (float)NAN, (float)INFINITY, -(float)INFINITY}) {
        Compressor c = drc;
        reinterpret_cast<float *>(&c)[i] = v;
        const std::string m = compressor_check(c);
        CHECK(!m.empty() && m.find(names[i]) != std::string::npos);
      }
    }
  }
  CHECK(!compressor_args_check(drc, 7999, 1).empty() && !compressor_args_check(drc, 96001, 1).empty() && compressor_args_check(drc, 8000, 1).empty());
  CHECK(!compressor_args_check(drc, 22050, 0).empty() && !compressor_args_check(drc, 22050, COMP_MAX_SAMPLES).empty());
  // the host integers: the clamp ends, and the preset at the three rates of the tests
  {
    Compressor c = drc;
    c.attack_ms = 0.1f;
    c.release_ms = 2000.0f;
    CHECK(compressor_plan(c, 8000).alpha == 136066 && compressor_plan(c, 96000).rho == 1 && compressor_plan(c, 8000).rho == 7);
    CHECK(comp_slope(0.0001, 8000) == COMP_SLOPE_MAX && comp_slope(1e9, 96000) == 1);
    const CompPlan p = compressor_plan(drc, 22050);
    CHECK(p.T == comp_round_q16(-24.0) && p.T == -261247 && p.W == 65312 && p.alpha == 987 && p.rho == 49);
    CHECK(p.s < 0.f && p.kq < 0.f && p.half_w == 32656.0f && p.mk == 1.0f);
    CHECK(comp_reach(1) == 4080 && comp_reach(COMP_SLOPE_MAX) == 1 && comp_reach(49) == 84);
  }
  // lvl and 2^x at their exact points
  CHECK(comp_lvl(comp_abs_bits(1.0f)) == 0 && comp_lvl(comp_abs_bits(-0.5f)) == -COMP_UNIT && comp_lvl(comp_abs_bits(4.0f)) == 2 * COMP_UNIT);
  CHECK(comp_lvl(0u) == COMP_L_FLOOR && comp_lvl(comp_abs_bits(1e-40f)) == COMP_L_FLOOR && comp_lvl(comp_abs_bits(1.17549435e-38f)) == -126 * COMP_UNIT);
  CHECK(comp_lvl(comp_abs_bits(3.4028235e38f)) <= COMP_L_MAX && comp_lvl(0x7fffffffu) <= COMP_L_MAX + COMP_UNIT);
  CHECK(comp_exp2(0.0f) == 1.0f && comp_exp2(-0.0f) == 1.0f && comp_exp2(-65536.0f) == 0.5f && comp_exp2(-3.0f * 65536.0f) == 0.125f);
  CHECK(comp_exp2(-1e-30f) == 1.0f && comp_exp2(-127.0f * 65536.0f) == 0.0f && comp_exp2(-125.5f * 65536.0f) > 0.0f);
  for (float r = 0.0f; r >= -65536.0f; r -= 0.37f) CHECK(comp_exp2(r) <= 1.0f && comp_exp2(r) >= 0.5f);
  // the walk against the reference
  Compressor hard = drc, soft = drc, mk = d, slow = drc, ramp = drc;
  hard.ratio = 20.f, hard.knee_db = 0.f;
  soft.ratio = 1.5f, soft.knee_db = 24.f;
  mk.makeup_db = 6.f;
  slow.release_ms = 2000.f;
  ramp.attack_ms = 100.f;
  for (int rate : {8000, 22050, 96000})
    for (size_t N : {(size_t)1, (size_t)2, (size_t)255, (size_t)COMP_TILE - 1, (size_t)COMP_TILE, (size_t)COMP_TILE + 1, (size_t)3 * COMP_TILE + 5})
      for (const Compressor &c : {drc, hard, soft}) against_reference(signal(N, (uint32_t)rate), rate, c, true);
  against_reference(signal(3 * COMP_TILE + 5, 1), 22050, mk, false);
  {  // make-up only: every sample is fl(x mk)
    const std::vector<float> x = signal(COMP_TILE + 9, 2);
    std::vector<float> out;
    const CompressorStats st = walk(x, 22050, mk, out);
    const float m = compressor_plan(mk, 22050).mk;
    bool scaled = true;
    for (size_t i = 0; i < x.size(); ++i) scaled = scaled && out[i] == x[i] * m;
    CHECK(scaled && st.compressed == 0 && st.engaged == 1);
  }
  {  // a release tail over more than two tiles, an attack ramp over more than one
    std::vector<float> x = noise(5 * COMP_TILE, 0.0001f, 3);
    x[100] = 1.0f;
    against_reference(x, 8000, slow, true);
    std::vector<float> y = noise(4 * COMP_TILE, 0.0001f, 4);
    y[4 * COMP_TILE - 100] = -1.0f;
    against_reference(y, 96000, ramp, true);
  }
  {  // bursts at the last sample of a tile and the first of the next; a zero stretch longer than a tile that reaches the floor
    std::vector<float> x(4 * COMP_TILE + 77, 0.0f);
    x[COMP_TILE - 1] = 0.9f;
    x[3 * COMP_TILE] = -0.6f;
    against_reference(x, 22050, drc, true);
    Compressor fast = drc;
    fast.attack_ms = 0.1f, fast.release_ms = 1.0f;
    against_reference(x, 8000, fast, true);
    std::vector<int32_t> l(x.size()), V(x.size());
    compressor_level(x.data(), x.size(), l.data());
    const CompPlan p = compressor_plan(fast, 8000);
    compressor_envelope_from_level(l.data(), x.size(), p.alpha, p.rho, V.data());
    CHECK(V[2 * COMP_TILE] == COMP_L_FLOOR && V[COMP_TILE - 1] == l[COMP_TILE - 1]);
  }
  {  // all zero: not engaged, unchanged; the identity: unchanged
    std::vector<float> z(COMP_TILE + 3, 0.0f), out;
    z[5] = -0.0f;
    const CompressorStats st = walk(z, 22050, drc, out);
    CHECK(same_bits(z, out) && st.engaged == 0 && st.compressed == 0 && st.max_over == 0 && st.peak == 0.0f);
    std::vector<float> ref(z.size());
    const CompressorStats rs = compressor_reference(z.data(), z.size(), 22050, drc, ref.data());
    CHECK(same_bits(z, ref) && rs.engaged == 0 && rs.max_over == 0);
    const std::vector<float> x = signal(1000, 5);
    std::vector<float> idn(x.size());
    const CompressorStats is = compressor_reference(x.data(), x.size(), 22050, d, idn.data());
    CHECK(same_bits(x, idn) && is.engaged == 0);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
