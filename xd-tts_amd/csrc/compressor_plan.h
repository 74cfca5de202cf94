// compressor_plan.h -- the arithmetic of the dynamic range compressor in front of the level stage (xdtts_griffinlim_set_compressor;
// the definition: include/xdtts.h): the argument rules, the identity, the slopes and constants, the per-sample functions (level,
// gain computer, 2^x, output), the two passes over one tile exactly as a workgroup of k_comp_tiles / k_compress performs them,
// and the sample-by-sample reference in the serial form.
// Plain C++, no HIP and none of the library's headers: tests/compressor_plan_test.cpp drives it with plain g++.  Everything the
// device shares carries COMP_HD -- compressor.hip's kernels are the lane loops around these functions.  Every product of the
// definition is rounded to fp32 on its own: the functions that multiply switch contraction off.  No libm on the shared path:
// fmaf and fminf are single instructions there.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define COMP_HD __host__ __device__ __attribute__((always_inline))
#else
#define COMP_HD
#endif
#ifdef __clang__
#define COMP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define COMP_NO_CONTRACT  // (g++ on x86-64 without -mfma has no fused instruction to contract into)
#endif

namespace xdtts {

constexpr int COMP_TILE = 4096;                          // samples of one utterance a workgroup owns
constexpr int COMP_WG = 256;                             // lanes of a workgroup
constexpr int COMP_VEC = 4;                              // consecutive samples of a lane in one round (one 128-bit access)
constexpr int COMP_ROUND = COMP_WG * COMP_VEC;           // samples of a round
constexpr int COMP_ROUNDS = COMP_TILE / COMP_ROUND;      // 4
constexpr int COMP_WAVES = COMP_WG / 64;                 // 4
constexpr int COMP_SEGS = COMP_ROUNDS * COMP_WAVES;      // 16 segments of 256 consecutive samples: one wave's share of a round
constexpr int COMP_OWN = COMP_ROUNDS * COMP_VEC;         // 16 samples of a lane
constexpr int32_t COMP_UNIT = 65536;                     // levels are Q16 octaves
constexpr int32_t COMP_L_FLOOR = -127 * COMP_UNIT;       // zeros and denormals: one octave under the smallest normal float
constexpr int32_t COMP_L_MAX = 128 * COMP_UNIT;          // no finite float's level exceeds it
constexpr int32_t COMP_SLOPE_MAX = 1 << 18;              // Q16 octaves per sample: 4 octaves, 24 dB
constexpr int32_t COMP_NEG = INT32_MIN;                  // "no value" of a max scan; never enters arithmetic
constexpr size_t COMP_MAX_SAMPLES = (size_t)1 << 28;     // exclusive, as the loudness measurement
constexpr int COMP_RATE_MIN = 8000, COMP_RATE_MAX = 96000;
// COMP_L_FLOOR - COMP_TILE * COMP_SLOPE_MAX = -2^30 - 127 * 2^16 and COMP_L_MAX + COMP_TILE * COMP_SLOPE_MAX fit an int32: the
// tile-local scans run in 32 bits.
static_assert((long long)COMP_L_FLOOR - (long long)COMP_TILE * COMP_SLOPE_MAX > (long long)INT32_MIN + 1 &&
              (long long)COMP_L_MAX + (long long)COMP_TILE * COMP_SLOPE_MAX < (long long)INT32_MAX, "tile-local scans fit 32 bits");
static_assert(COMP_TILE % COMP_ROUND == 0 && COMP_WG % 64 == 0, "a wave's samples of a round are one segment");

struct Compressor {  // == xdtts_compressor
  float threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db;
};
struct CompressorStats {  // == xdtts_compressor_stats
  float peak;
  int32_t max_over, engaged;
  int64_t compressed;
};
// what the kernels take: the host integers and the three floats of the gain computer
struct CompPlan {
  int32_t alpha, rho, T, W;
  float s, kq, half_w, mk;  // 1/ratio - 1; s / (2 W) (0 where W = 0); W / 2; 10^(makeup_db / 20)
};
// what pass 1 leaves per tile: the forward envelope at its last sample and the backward envelope at its first, had the
// utterance consisted of the tile alone
struct CompAgg {
  int32_t fwd, bwd;
};

inline Compressor compressor_default() { return Compressor{0.0f, 1.0f, 0.0f, 5.0f, 100.0f, 0.0f}; }  // the identity
// preset 1, "drc": -24 dB re peak, 3:1, 6 dB knee, 5 ms / 100 ms, no make-up (the level stage behind supplies it)
inline bool compressor_preset(int which, Compressor *out) {
  if (which == 0) *out = compressor_default();
  else if (which == 1) *out = Compressor{-24.0f, 3.0f, 6.0f, 5.0f, 100.0f, 0.0f};
  else return false;
  return true;
}
inline bool compressor_is_identity(const Compressor &c) { return c.ratio == 1.0f && c.makeup_db == 0.0f; }

// "" if c is a setting, else the message: it names the field
inline std::string compressor_check(const Compressor &c) {
  char msg[160];
  const struct {
    const char *name;
    float v, lo, hi;
  } f[] = {{"threshold_db", c.threshold_db, -60.f, 0.f}, {"ratio", c.ratio, 1.f, 20.f},         {"knee_db", c.knee_db, 0.f, 24.f},
           {"attack_ms", c.attack_ms, 0.1f, 100.f},      {"release_ms", c.release_ms, 1.f, 2000.f}, {"makeup_db", c.makeup_db, 0.f, 24.f}};
  for (const auto &e : f)
    if (!std::isfinite(e.v) || e.v < e.lo || e.v > e.hi) {
      std::snprintf(msg, sizeof msg, "compressor: %s %g is not a finite value in [%g, %g]", e.name, (double)e.v, (double)e.lo, (double)e.hi);
      return msg;
    }
  return "";
}
inline std::string compressor_rate_check(long long rate) {
  char msg[160];
  if (rate < COMP_RATE_MIN || rate > COMP_RATE_MAX) {
    std::snprintf(msg, sizeof msg, "compressor: rate %lld is not in [%d, %d]", rate, COMP_RATE_MIN, COMP_RATE_MAX);
    return msg;
  }
  return "";
}
// the arguments of the stage alone (xdtts_griffinlim_compress, xdtts_compressor_reference)
inline std::string compressor_args_check(const Compressor &c, long long rate, size_t n) {
  char msg[160];
  std::string r = compressor_check(c);
  if (!r.empty()) return r;
  r = compressor_rate_check(rate);
  if (!r.empty()) return r;
  if (n == 0 || n >= COMP_MAX_SAMPLES) {
    std::snprintf(msg, sizeof msg, "compressor: need 1 .. 2^28 - 1 samples, got %zu", n);
    return msg;
  }
  return "";
}
inline size_t compressor_tiles(size_t n) { return (n + COMP_TILE - 1) / COMP_TILE; }

// The host integers and constants (checked arguments).  log10(2) is a literal, every step one double operation in the order
// written, rounding by floor(v + 0.5): tests/compressor_ref.py repeats them and gets the same integers.
constexpr double COMP_LOG10_2 = 0.30102999566398119521;
constexpr double COMP_UNIT_D = (double)COMP_UNIT;  // 65536
inline int32_t comp_round_q16(double db) { return (int32_t)std::floor(db * (COMP_UNIT_D / (20.0 * COMP_LOG10_2)) + 0.5); }
inline int32_t comp_slope(double ms, int rate) {
  const double oct10 = 10.0 / (20.0 * COMP_LOG10_2);
  const double v = std::floor(65536.0 * oct10 / (ms * (double)rate / 1000.0) + 0.5);
  return (int32_t)std::min(std::max(v, 1.0), (double)COMP_SLOPE_MAX);
}
inline CompPlan compressor_plan(const Compressor &c, int rate) {
  CompPlan p{};
  p.alpha = comp_slope((double)c.attack_ms, rate);
  p.rho = comp_slope((double)c.release_ms, rate);
  p.T = comp_round_q16((double)c.threshold_db);
  p.W = comp_round_q16((double)c.knee_db);
  const double s = 1.0 / (double)c.ratio - 1.0;
  p.s = (float)s;
  p.kq = p.W > 0 ? (float)(s / (2.0 * (double)p.W)) : 0.0f;
  p.half_w = (float)((double)p.W / 2.0);  // exact: W < 2^23
  p.mk = (float)std::pow(10.0, (double)c.makeup_db / 20.0);
  return p;
}
// tiles a carry can come from: a tent that starts d tiles away has fallen by d * COMP_TILE * slope, and no level lies more
// than COMP_L_MAX - COMP_L_FLOOR above another
COMP_HD inline int comp_reach(int32_t slope) {
  const long long step = (long long)COMP_TILE * slope, range = (long long)COMP_L_MAX - COMP_L_FLOOR;
  return (int)((range + step - 1) / step);
}

// ---- one sample -----------------------------------------------------------------------------------------------------------------

COMP_HD inline uint32_t comp_bits(float a) {
  uint32_t u;
  __builtin_memcpy(&u, &a, sizeof u);
  return u;
}
COMP_HD inline float comp_float(uint32_t u) {
  float a;
  __builtin_memcpy(&a, &u, sizeof a);
  return a;
}
COMP_HD inline uint32_t comp_abs_bits(float x) { return comp_bits(x) & 0x7fffffffu; }  // |x| as an integer: its order is the floats'

// lvl: 65536 log2 of the float with bits `abs_bits`, to the nearest integer within COMP_LVL_ERR.  Exponent from the bits;
// log2(1 + f) = f q(f) on the mantissa f in [0, 1), q of degree 8 (the Chebyshev interpolant of log2(1 + f) / f on [0, 1],
// coefficients rounded to fp32: |f q(f) - log2(1 + f)| <= 4e-8 in exact arithmetic), Horner with fmaf.  lvl(1) = 0 exactly.
constexpr float COMP_LOG2_Q[9] = {1.44269502f,  -0.721339524f, 0.480678886f,  -0.358299077f, 0.275221199f,
                                  -0.19623895f, 0.111832075f,  -0.0419450104f, 0.00739540206f};
COMP_HD inline int32_t comp_lvl(uint32_t abs_bits) {
  COMP_NO_CONTRACT
  const int e = (int)(abs_bits >> 23);
  if (e == 0) return COMP_L_FLOOR;
  const float f = comp_float((abs_bits & 0x7fffffu) | 0x3f800000u) - 1.0f;  // exact
  float q = COMP_LOG2_Q[8];
#ifdef __clang__
#pragma unroll
#endif
  for (int k = 7; k >= 0; --k) q = fmaf(q, f, COMP_LOG2_Q[k]);
  const float p = q * f;
  const float v = p * 65536.0f + 0.5f;  // (the product is exact)
  return (e - 127) * COMP_UNIT + (int32_t)v;
}

// 2^(r / 65536) for r <= 0, in [0, 1]: r / 65536 = i + f, f in [0, 1); 2^f = 1 + f q(f), q of degree 5 (the Chebyshev interpolant
// of (2^f - 1) / f, coefficients rounded to fp32: |1 + f q(f) - 2^f| <= 3e-8 in exact arithmetic), times 2^i through the
// exponent bits; 0 below -126 octaves.  r = 0 (either sign) gives 1 exactly.
constexpr float COMP_EXP2_Q[6] = {0.693147182f, 0.240227208f, 0.0554960221f, 0.0096521955f, 0.00126921665f, 0.000208179146f};
COMP_HD inline float comp_exp2(float r) {
  COMP_NO_CONTRACT
  const float t = r * (1.0f / 65536.0f);
  if (!(t > -126.0f)) return 0.0f;
  int i = (int)t;
  if ((float)i > t) --i;  // floor
  const float f = t - (float)i;  // in [0, 1]: exact but for a tiny |t|, which rounds to f = 1 (2^1 2^-1: the same value)
  float q = COMP_EXP2_Q[5];
#ifdef __clang__
#pragma unroll
#endif
  for (int k = 4; k >= 0; --k) q = fmaf(q, f, COMP_EXP2_Q[k]);
  const float p = fmaf(f, q, 1.0f);
  return fminf(p * comp_float((uint32_t)(i + 127) << 23), 1.0f);
}

// the gain computer: r <= 0 in Q16 octaves from o = V - (P + T); the branch is chosen in integers
COMP_HD inline float comp_gain_r(int32_t o, const CompPlan &c) {
  COMP_NO_CONTRACT
  const int32_t o2 = 2 * o;  // |o| < 2^26
  if (o2 <= -c.W) return 0.0f;
  const float of = (float)o;
  if ((o2 < 0 ? -o2 : o2) < c.W) {
    const float h = of + c.half_w;
    const float hh = h * h;
    return hh * c.kq;
  }
  return c.s * of;
}

// out = fl(x fl(g mk))
COMP_HD inline float comp_apply(float x, float g, float mk) {
  COMP_NO_CONTRACT
  const float f = g * mk;
  return x * f;
}

// one sample from its envelope: the output, and r through *r_out
COMP_HD inline float comp_sample(float x, int32_t V, int32_t PT, const CompPlan &c, int32_t *o_out, float *r_out) {
  const int32_t o = V - PT;
  const float r = comp_gain_r(o, c);
  *o_out = o;
  *r_out = r;
  return comp_apply(x, comp_exp2(r), c.mk);
}

// ---- the definition, sample by sample, in the serial form ------------------------------------------------------------------------

inline uint32_t compressor_peak_bits(const float *x, size_t n) {
  uint32_t pk = 0;
  for (size_t i = 0; i < n; ++i) pk = std::max(pk, comp_abs_bits(x[i]));
  return pk;
}
inline void compressor_level(const float *x, size_t n, int32_t *l) {
  for (size_t i = 0; i < n; ++i) l[i] = comp_lvl(comp_abs_bits(x[i]));
}
// V from l: E[n] = max(l[n], E[n - 1] - rho) forwards, its mirror image with alpha backwards, V = the larger.  64-bit.
inline void compressor_envelope_from_level(const int32_t *l, size_t n, int32_t alpha, int32_t rho, int32_t *V) {
  if (n == 0) return;
  long long e = l[0];
  V[0] = l[0];
  for (size_t i = 1; i < n; ++i) {
    e = std::max<long long>(l[i], e - rho);
    V[i] = (int32_t)e;
  }
  e = l[n - 1];
  for (size_t i = n - 1; i-- > 0;) {
    e = std::max<long long>(l[i], e - alpha);
    V[i] = std::max(V[i], (int32_t)e);
  }
}
inline CompressorStats compressor_reference(const float *x, size_t n, int rate, const Compressor &c, float *out) {
  CompressorStats st{0.0f, 0, 0, 0};
  const uint32_t pk = compressor_peak_bits(x, n);
  if (compressor_is_identity(c) || pk == 0) {
    if (out != x) std::memcpy(out, x, n * sizeof(float));
    return st;
  }
  const CompPlan p = compressor_plan(c, rate);
  std::vector<int32_t> l(n), V(n);
  compressor_level(x, n, l.data());
  compressor_envelope_from_level(l.data(), n, p.alpha, p.rho, V.data());
  const int32_t PT = comp_lvl(pk) + p.T;
  st.peak = comp_float(pk);
  st.engaged = 1;
  st.max_over = COMP_NEG;
  for (size_t i = 0; i < n; ++i) {
    int32_t o;
    float r;
    out[i] = comp_sample(x[i], V[i], PT, p, &o, &r);
    st.max_over = std::max(st.max_over, o);
    if (r < 0.0f) ++st.compressed;
  }
  return st;
}

// ---- the two passes over one tile, as a workgroup performs them ----------------------------------------------------------------
// x: the utterance's n samples; t0: the tile's first sample (a multiple of COMP_TILE below n).  Lane `tid` owns, in round r, the
// COMP_VEC samples from j0 = r COMP_ROUND + COMP_VEC tid of the tile; its wave's 256 samples of the round are segment
// r COMP_WAVES + wave.  Arrays that stand for LDS have exactly the kernel's sizes.

// sample j of the tile (0 behind the utterance's end: never used, `valid` says so)
COMP_HD inline bool comp_valid(int j, int n_here) { return j < n_here; }

// pass 1 (k_comp_tiles): the tile's aggregates and its peak
struct CompTile1 {
  CompAgg agg;
  uint32_t peak_bits;
};
inline CompTile1 compressor_tile_pass1(const float *x, size_t n, size_t t0, const CompPlan &p) {
  const int n_here = (int)std::min<size_t>(COMP_TILE, n - t0), last = n_here - 1;
  int32_t red_f[COMP_WAVES], red_b[COMP_WAVES];
  uint32_t red_p[COMP_WAVES];
  for (int w = 0; w < COMP_WAVES; ++w) red_f[w] = red_b[w] = COMP_NEG, red_p[w] = 0;
  for (int tid = 0; tid < COMP_WG; ++tid) {
    int32_t f = COMP_NEG, b = COMP_NEG;
    uint32_t pk = 0;
    for (int r = 0; r < COMP_ROUNDS; ++r)
      for (int c = 0; c < COMP_VEC; ++c) {
        const int j = r * COMP_ROUND + COMP_VEC * tid + c;
        if (!comp_valid(j, n_here)) continue;
        const uint32_t a = comp_abs_bits(x[t0 + (size_t)j]);
        const int32_t l = comp_lvl(a);
        pk = std::max(pk, a);
        f = std::max(f, l - (last - j) * p.rho);
        b = std::max(b, l - j * p.alpha);
      }
    red_f[tid >> 6] = std::max(red_f[tid >> 6], f);
    red_b[tid >> 6] = std::max(red_b[tid >> 6], b);
    red_p[tid >> 6] = std::max(red_p[tid >> 6], pk);
  }
  CompTile1 t{{COMP_NEG, COMP_NEG}, 0};
  for (int w = 0; w < COMP_WAVES; ++w) {
    t.agg.fwd = std::max(t.agg.fwd, red_f[w]);
    t.agg.bwd = std::max(t.agg.bwd, red_b[w]);
    t.peak_bits = std::max(t.peak_bits, red_p[w]);
  }
  return t;
}

// the carries of tile `tl` of an utterance of `tiles` tiles from the aggregates agg[0 .. tiles): the forward envelope at the last
// sample in front of the tile and the backward envelope at the first sample behind it, never below COMP_L_FLOOR (no level is)
COMP_HD inline int32_t comp_carry_term(int32_t a, int d, int32_t slope) {
  const long long v = (long long)a - (long long)d * COMP_TILE * slope;
  return v < COMP_L_FLOOR ? COMP_L_FLOOR : (int32_t)v;
}
inline void compressor_carries(const CompAgg *agg, int tiles, int tl, const CompPlan &p, int32_t *cin, int32_t *din) {
  int32_t ci = COMP_L_FLOOR, di = COMP_L_FLOOR;
  const int nf = std::min(tl, comp_reach(p.rho)), nb = std::min(tiles - 1 - tl, comp_reach(p.alpha));
  for (int d = 0; d < nf; ++d) ci = std::max(ci, comp_carry_term(agg[tl - 1 - d].fwd, d, p.rho));
  for (int d = 0; d < nb; ++d) di = std::max(di, comp_carry_term(agg[tl + 1 + d].bwd, d, p.alpha));
  *cin = ci;
  *din = di;
}

// pass 2 (k_compress): the tile's samples and its share of the stats (count of r < 0, the largest o)
struct CompTile2 {
  long long compressed = 0;
  int32_t max_over = COMP_NEG;
};
inline CompTile2 compressor_tile_walk(const float *x, size_t n, size_t t0, const CompPlan &p, const CompAgg *agg, int tiles, int32_t P,
                                      float *out) {
  CompTile2 st;
  const int n_here = (int)std::min<size_t>(COMP_TILE, n - t0), tl = (int)(t0 / COMP_TILE);
  const int32_t PT = P + p.T;
  int32_t cin, din;
  compressor_carries(agg, tiles, tl, p, &cin, &din);
  std::vector<int32_t> seg_f(COMP_SEGS, COMP_NEG), seg_b(COMP_SEGS, COMP_NEG);  // LDS
  std::vector<int32_t> pf((size_t)COMP_WG * COMP_OWN), sb((size_t)COMP_WG * COMP_OWN);  // registers: [tid][r * VEC + c]
  // the in-lane scans, then the scan across a wave's lanes; the wave's total of the round goes to LDS
  for (int r = 0; r < COMP_ROUNDS; ++r)
    for (int wave = 0; wave < COMP_WAVES; ++wave) {
      int32_t run = COMP_NEG;  // forwards: lanes ascending
      for (int lane = 0; lane < 64; ++lane) {
        const int tid = wave * 64 + lane;
        for (int c = 0; c < COMP_VEC; ++c) {
          const int j = r * COMP_ROUND + COMP_VEC * tid + c;
          if (comp_valid(j, n_here)) run = std::max(run, comp_lvl(comp_abs_bits(x[t0 + (size_t)j])) + j * p.rho);
          pf[(size_t)tid * COMP_OWN + (size_t)(r * COMP_VEC + c)] = run;
        }
      }
      seg_f[(size_t)(r * COMP_WAVES + wave)] = run;
      run = COMP_NEG;  // backwards: lanes descending
      for (int lane = 63; lane >= 0; --lane) {
        const int tid = wave * 64 + lane;
        for (int c = COMP_VEC - 1; c >= 0; --c) {
          const int j = r * COMP_ROUND + COMP_VEC * tid + c;
          if (comp_valid(j, n_here)) run = std::max(run, comp_lvl(comp_abs_bits(x[t0 + (size_t)j])) - j * p.alpha);
          sb[(size_t)tid * COMP_OWN + (size_t)(r * COMP_VEC + c)] = run;
        }
      }
      seg_b[(size_t)(r * COMP_WAVES + wave)] = run;
    }
  // across the segments, the carries, the gain
  for (int tid = 0; tid < COMP_WG; ++tid)
    for (int r = 0; r < COMP_ROUNDS; ++r) {
      const int seg = r * COMP_WAVES + (tid >> 6);
      int32_t ex_f = COMP_NEG, ex_b = COMP_NEG;
      for (int k = 0; k < seg; ++k) ex_f = std::max(ex_f, seg_f[(size_t)k]);
      for (int k = seg + 1; k < COMP_SEGS; ++k) ex_b = std::max(ex_b, seg_b[(size_t)k]);
      for (int c = 0; c < COMP_VEC; ++c) {
        const int j = r * COMP_ROUND + COMP_VEC * tid + c;
        if (!comp_valid(j, n_here)) continue;
        const size_t k = (size_t)tid * COMP_OWN + (size_t)(r * COMP_VEC + c);
        const int32_t e_f = std::max(std::max(pf[k], ex_f) - j * p.rho, cin - (j + 1) * p.rho);
        const int32_t e_b = std::max(std::max(sb[k], ex_b) + j * p.alpha, din - (COMP_TILE - j) * p.alpha);
        int32_t o;
        float rr;
        out[t0 + (size_t)j] = comp_sample(x[t0 + (size_t)j], std::max(e_f, e_b), PT, p, &o, &rr);
        st.max_over = std::max(st.max_over, o);
        if (rr < 0.0f) ++st.compressed;
      }
    }
  return st;
}

}  // namespace xdtts
