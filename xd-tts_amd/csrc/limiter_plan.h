// limiter_plan.h -- the arithmetic of the look-ahead true-peak limiter behind the loudness stage (xdtts_griffinlim_set_limiter;
// the definition: include/xdtts.h): the argument rules, the half width H and the tile, the smoothing window, the per-sample
// functions (peak envelope, needed gain, hold, smoothing, output), the walk of one tile exactly as a workgroup of k_limit
// performs it, and the sample-by-sample reference.
// Plain C++, no HIP and none of the library's headers but loudness_plan.h (the true-peak taps): tests/limiter_plan_test.cpp
// drives it with plain g++.  Everything the device shares carries LIM_HD -- limiter.hip's kernel is the lane loops around these
// functions.  Every product of the definition is rounded to fp32 on its own: the functions that multiply switch contraction off.
#pragma once
#include <algorithm>
#include <cstdint>

#include "loudness_plan.h"

#ifdef __HIPCC__
#define LIM_HD __host__ __device__ __attribute__((always_inline))
#else
#define LIM_HD
#endif
#ifdef __clang__
#define LIM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LIM_NO_CONTRACT  // (g++ on x86-64 without -mfma has no fused instruction to contract into)
#endif

namespace xdtts {

constexpr int LIM_US_MIN = 500, LIM_US_MAX = 10000;   // look-ahead in microseconds; 0 = off
constexpr int LIM_H_MIN = LOUD_TP_HALF;               // the hold is never shorter than the peak filter's half length
constexpr int LIM_H_MAX = 960;                        // 96 kHz, 10 ms
constexpr int LIM_TILE = 4096;                        // output samples of one utterance a workgroup owns
constexpr int LIM_WG = 256;                           // lanes of a workgroup
constexpr int LIM_ROUNDS = LIM_TILE / LIM_WG;         // outputs of a lane
constexpr int LIM_FRONT = LOUD_TP_HALF + 1;           // staged samples in front of the first needed-gain position
constexpr size_t LIM_MAX_SAMPLES = (size_t)1 << 28;   // exclusive, as the loudness measurement

struct LimiterStats {  // == xdtts_limiter_stats
  float min_gain;
  int32_t half_width, engaged;
  int64_t limited;
};

// "" if the look-ahead is a setting of xdtts_griffinlim_set_limiter (0 = off, or [500, 10000]), else the message
inline std::string limiter_setting_check(long long lookahead_us) {
  char msg[160];
  if (lookahead_us != 0 && (lookahead_us < LIM_US_MIN || lookahead_us > LIM_US_MAX)) {
    std::snprintf(msg, sizeof msg, "limiter: lookahead_us %lld is not 0 (off) or in [%d, %d]", lookahead_us, LIM_US_MIN, LIM_US_MAX);
    return msg;
  }
  return "";
}
// "" if (rate, look-ahead) define a stage that runs, else the message: it names the field
inline std::string limiter_check(long long rate, long long lookahead_us) {
  char msg[160];
  const std::string r = loudness_check(rate);
  if (!r.empty()) return "limiter: " + r;
  if (lookahead_us < LIM_US_MIN || lookahead_us > LIM_US_MAX) {
    std::snprintf(msg, sizeof msg, "limiter: lookahead_us %lld is not in [%d, %d]", lookahead_us, LIM_US_MIN, LIM_US_MAX);
    return msg;
  }
  return "";
}
// the arguments of the stage alone (xdtts_griffinlim_limit, xdtts_limiter_reference)
inline std::string limiter_args_check(long long rate, long long lookahead_us, size_t n, double gain0, double ceiling_lin) {
  char msg[160];
  const std::string r = limiter_check(rate, lookahead_us);
  if (!r.empty()) return r;
  if (n == 0 || n >= LIM_MAX_SAMPLES) {
    std::snprintf(msg, sizeof msg, "limiter: need 1 .. 2^28 - 1 samples, got %zu", n);
    return msg;
  }
  if (!(ceiling_lin > 0.0) || !std::isfinite(ceiling_lin)) {
    std::snprintf(msg, sizeof msg, "limiter: ceiling_lin %g is not a finite value above 0", ceiling_lin);
    return msg;
  }
  if (!std::isfinite(gain0) || gain0 < 0.0) {
    std::snprintf(msg, sizeof msg, "limiter: gain0 %g is not a finite value >= 0", gain0);
    return msg;
  }
  return "";
}

// H = max(12, (Q lookahead_us + 500000) / 1000000) in 64-bit integer division: 12 .. 960
inline int limiter_half_width(int rate, int lookahead_us) {
  const long long h = ((long long)rate * (long long)lookahead_us + 500000LL) / 1000000LL;
  return h < LIM_H_MIN ? LIM_H_MIN : (int)h;
}
inline size_t limiter_tiles(size_t n) { return (n + LIM_TILE - 1) / LIM_TILE; }

// w[j + H] = (0.5 + 0.5 cos(pi j / (H + 1))) / (H + 1), j = -H .. H: in double, rounded once (2 H + 1 weights, their exact sum is 1)
inline void limiter_window(int H, float *w) {
  const double PI = 3.14159265358979323846;
  for (int j = -H; j <= H; ++j) w[j + H] = (float)((0.5 + 0.5 * std::cos(PI * (double)j / (double)(H + 1))) / (double)(H + 1));
}

// ---- what a tile keeps, in floats -----------------------------------------------------------------------------------------
// A tile of outputs [t0, t0 + TILE) needs the gain's hold over [t0 - H, t0 + TILE + H), hence the needed gain r over W = TILE + 4 H
// positions from t0 - 2 H on, hence the peak values Y over W + 1 positions from t0 - 2 H - 1 on, hence the samples
// x[t0 - 2 H - 13 .. t0 + TILE + 2 H + 12] (zero outside [0, n)).
LIM_HD inline int lim_w(int H) { return LIM_TILE + 4 * H; }                   // positions of r
LIM_HD inline int lim_d(int H) { return LIM_TILE + 2 * H; }                   // positions of d = 1 - hold
LIM_HD inline int lim_xs(int H) { return lim_w(H) + 2 * LIM_FRONT; }          // staged samples; buffer A
LIM_HD inline int lim_ys(int H) { return lim_w(H) + 1; }                      // peak values; buffer B
LIM_HD inline int lim_flags(int H) { return (lim_d(H) + 63) / 64; }           // one word per 64 positions of d: any d != 0
LIM_HD inline int lim_lds_floats(int H) { return lim_xs(H) + lim_ys(H) + lim_flags(H) + 8; }
// the largest power of two <= 2 H + 1: the doubling stops there, two such windows cover the hold
LIM_HD inline int lim_pow2(int H) {
  int p = 1;
  while (2 * p <= 2 * H + 1) p *= 2;
  return p;
}

// ---- one position -----------------------------------------------------------------------------------------------------------

// sample at absolute position pos of an utterance of n samples, zero extension
LIM_HD inline float lim_sample(const float *x, long long pos, long long n) { return (pos >= 0 && pos < n) ? x[pos] : 0.f; }

// Y at peak position q of the tile (sample position t0 - 2 H - 1 + q): max over p of |y[4 n + p]|, each phase one fmaf chain over
// j ascending; xs[q + 12 - j] = x[n - j].  0 outside [0, n_utt): Y[-1] = 0, and behind the last sample nothing counts.
LIM_HD inline float lim_peak(const float *xs, int q, const float *taps, bool inside) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#ifdef __clang__
#pragma unroll
#endif
  for (int j = -LOUD_TP_HALF; j < LOUD_TP_HALF; ++j) {
    const float v = xs[q + LOUD_TP_HALF - j];
    a0 = fmaf(v, taps[j + LOUD_TP_HALF], a0);
    a1 = fmaf(v, taps[LOUD_TP_TAPS + j + LOUD_TP_HALF], a1);
    a2 = fmaf(v, taps[2 * LOUD_TP_TAPS + j + LOUD_TP_HALF], a2);
  }
  const float y = fmaxf(fabsf(a0), fmaxf(fabsf(a1), fabsf(a2)));
  return inside ? y : 0.f;
}

// r from e = max(|x[n]|, Y[n], Y[n - 1]): 1 unless fl(G e) > c, then (float)((double)c / (double)a); 1 outside the utterance
LIM_HD inline float lim_need(float G, float c, float x, float y_here, float y_before, bool inside) {
  LIM_NO_CONTRACT
  const float e = fmaxf(fabsf(x), fmaxf(y_here, y_before));
  const float a = G * e;
  if (!inside || !(a > c)) return 1.0f;
  return (float)((double)c / (double)a);
}

// d = fl(1 - m), m = the minimum of the two windows of P positions that cover [k, k + 2 H]  (mp[i] = min r[i .. i + P - 1])
LIM_HD inline float lim_hold(const float *mp, int k, int H, int P) { return 1.0f - fminf(mp[k], mp[k + 2 * H + 1 - P]); }

// sum over t = 0 .. 2 H of w[t] d[t], one fmaf chain from 0 over t ascending
LIM_HD inline float lim_fir(const float *w, const float *d, int H) {
  float acc = 0.f;
  for (int t = 0; t <= 2 * H; ++t) acc = fmaf(w[t], d[t], acc);
  return acc;
}

// ... for LIM_FIR_ROUNDS outputs `stride` apart at once: each its own chain in the same order, so the bits are lim_fir's; the
// weight is read once for the four and the chains' latencies overlap
constexpr int LIM_FIR_ROUNDS = 4;
LIM_HD inline void lim_fir_rounds(const float *w, const float *d, int stride, int H, float acc[LIM_FIR_ROUNDS]) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#ifdef __clang__
#pragma unroll 4
#endif
  for (int t = 0; t <= 2 * H; ++t) {
    const float wt = w[t];
    a0 = fmaf(wt, d[t], a0);
    a1 = fmaf(wt, d[stride + t], a1);
    a2 = fmaf(wt, d[2 * stride + t], a2);
    a3 = fmaf(wt, d[3 * stride + t], a3);
  }
  acc[0] = a0, acc[1] = a1, acc[2] = a2, acc[3] = a3;
}

// g = min(fl(1 - acc), r); out = fl(x fl(G g))
LIM_HD inline float lim_apply(float x, float G, float acc, float r, float *g_out) {
  LIM_NO_CONTRACT
  const float s = 1.0f - acc;
  const float g = fminf(s, r);
  *g_out = g;
  const float f = G * g;
  return x * f;
}
// the scale route (g = 1): fl(x fl(G 1)) = fl(x G), the bits of k_loud_scale
LIM_HD inline float lim_scale(float x, float G) {
  LIM_NO_CONTRACT
  return x * G;
}

// engaged: Z > 0 and g0 TP > c, in double, from the measurement
LIM_HD inline bool lim_engaged(double Z, double true_peak, double g0, double c) { return Z > 0.0 && c > 0.0 && g0 * true_peak > c; }

// ---- the walk of one tile, as a workgroup of k_limit performs it ---------------------------------------------------------------
// x: the utterance's n samples; t0: the tile's first output (a multiple of LIM_TILE below n); out: the utterance's output.
// Buffers A, B and the flags have exactly the sizes the kernel's LDS has.  Returns through min_gain / limited the tile's share of
// the stats (min over g, count of g < 1).
struct LimTileStats {
  float min_gain = 1.0f;
  long long limited = 0;
  bool scale_route = false;
  int fir_skipped = 0, fir_run = 0;  // (wave, round) pairs
};
inline LimTileStats limiter_tile_walk(const float *x, size_t n, size_t t0, int H, const float *taps, const float *w, float G, float c,
                                      float *out) {
  LimTileStats st;
  const int W = lim_w(H), D = lim_d(H), P = lim_pow2(H);
  std::vector<float> A((size_t)lim_xs(H)), B((size_t)lim_ys(H));
  std::vector<int> flags((size_t)lim_flags(H), 0);
  const long long N = (long long)n, X0 = (long long)t0 - 2 * H - LIM_FRONT;
  // 1 the staged samples, and each lane's own samples of the tile
  for (int i = 0; i < lim_xs(H); ++i) A[(size_t)i] = lim_sample(x, X0 + i, N);
  std::vector<float> xc(LIM_TILE), rc(LIM_TILE);
  for (int o = 0; o < LIM_TILE; ++o) xc[(size_t)o] = A[(size_t)(2 * H + LIM_FRONT + o)];
  // 2 the peak values, then r over W positions into A at the sample's own slot
  for (int q = 0; q < lim_ys(H); ++q) {
    const long long pos = (long long)t0 - 2 * H - 1 + q;
    B[(size_t)q] = lim_peak(A.data(), q, taps, pos >= 0 && pos < N);
  }
  bool any = false;
  for (int i = 0; i < W; ++i) {
    const long long pos = (long long)t0 - 2 * H + i;
    const float r = lim_need(G, c, A[(size_t)(i + LIM_FRONT)], B[(size_t)(i + 1)], B[(size_t)i], pos >= 0 && pos < N);
    A[(size_t)(i + LIM_FRONT)] = r;
    any = any || r < 1.0f;
  }
  // 3 the vote
  const int n_here = (int)std::min<size_t>(LIM_TILE, n - t0);
  if (!any) {
    st.scale_route = true;
    for (int o = 0; o < n_here; ++o) out[t0 + (size_t)o] = lim_scale(xc[(size_t)o], G);
    return st;
  }
  for (int o = 0; o < LIM_TILE; ++o) rc[(size_t)o] = A[(size_t)(LIM_FRONT + 2 * H + o)];
  // 4 the sliding minimum by doubling, ping-pong between the two buffers: after the level of width p, cur[i] = min r[i .. i + p - 1]
  const float *cur = A.data() + LIM_FRONT;
  bool in_a = true;
  for (int p = 1; p < P; p *= 2) {
    float *dst = in_a ? B.data() : A.data();
    for (int i = 0; i + 2 * p <= W; ++i) dst[i] = fminf(cur[i], cur[i + p]);
    cur = dst;
    in_a = !in_a;
  }
  float *d = in_a ? B.data() : A.data();  // (cur is in the other one)
  for (int k = 0; k < D; ++k) {
    const float v = lim_hold(cur, k, H, P);
    d[k] = v;
    if (v != 0.0f) flags[(size_t)(k >> 6)] = 1;
  }
  // 5, 6 the FIR: a wave takes its 64 consecutive outputs of LIM_FIR_ROUNDS rounds at once, and skips them where no d of
  // their windows is non-zero
  for (int r0 = 0; r0 < LIM_ROUNDS; r0 += LIM_FIR_ROUNDS)
    for (int wave0 = 0; wave0 < LIM_WG; wave0 += 64) {
      bool run = false;
      for (int q = 0; q < LIM_FIR_ROUNDS; ++q) {
        const int o0 = (r0 + q) * LIM_WG + wave0;
        for (int b = o0 >> 6; b <= (o0 + 63 + 2 * H) >> 6; ++b) run = run || flags[(size_t)b] != 0;
      }
      if (run) ++st.fir_run; else ++st.fir_skipped;
      for (int lane = wave0; lane < wave0 + 64; ++lane) {
        float acc[LIM_FIR_ROUNDS] = {0.f, 0.f, 0.f, 0.f};
        if (run) lim_fir_rounds(w, d + r0 * LIM_WG + lane, LIM_WG, H, acc);
        for (int q = 0; q < LIM_FIR_ROUNDS; ++q) {
          const int o = (r0 + q) * LIM_WG + lane;
          if (o >= n_here) continue;
          float g;
          out[t0 + (size_t)o] = lim_apply(xc[(size_t)o], G, acc[q], rc[(size_t)o], &g);
          if (g < 1.0f) ++st.limited;
          st.min_gain = fminf(st.min_gain, g);
        }
      }
    }
  return st;
}

// ---- the definition, sample by sample ----------------------------------------------------------------------------------------
inline LimiterStats limiter_reference(const float *x, size_t n, int rate, int lookahead_us, double gain0, double ceiling_lin, float *out) {
  const int H = limiter_half_width(rate, lookahead_us);
  const long long N = (long long)n;
  float taps[LOUD_TP_PHASES][LOUD_TP_TAPS];
  loudness_true_peak_taps(taps);
  std::vector<float> w((size_t)(2 * H + 1));
  limiter_window(H, w.data());
  const float G = (float)gain0, c = (float)ceiling_lin;
  // Y[n], n = -1 .. N - 1, at index n + 1
  std::vector<float> Y(n + 1, 0.f), r(n), m(n + 2 * (size_t)H);
  for (long long i = 0; i < N; ++i) {
    float xs[LOUD_TP_TAPS + 1];
    for (int k = 0; k <= LOUD_TP_TAPS; ++k) xs[k] = lim_sample(x, i - LOUD_TP_HALF + k, N);  // xs[12 - j] = x[i - j]
    Y[(size_t)(i + 1)] = lim_peak(xs, 0, &taps[0][0], true);
  }
  for (long long i = 0; i < N; ++i) r[(size_t)i] = lim_need(G, c, x[i], Y[(size_t)(i + 1)], Y[(size_t)i], true);
  // m[k], k = -H .. N - 1 + H, at index k + H: the minimum over [k - H, k + H], r = 1 outside [0, N)
  for (long long k = -H; k < N + H; ++k) {
    float v = 1.0f;
    const long long lo = std::max<long long>(k - H, 0), hi = std::min<long long>(k + H, N - 1);
    for (long long i = lo; i <= hi; ++i) v = fminf(v, r[(size_t)i]);
    m[(size_t)(k + H)] = v;
  }
  LimiterStats st{1.0f, H, 1, 0};
  std::vector<float> d((size_t)(2 * H + 1));
  for (long long i = 0; i < N; ++i) {
    for (int t = 0; t <= 2 * H; ++t) d[(size_t)t] = 1.0f - m[(size_t)(i + t)];  // m[i - H + t] of the definition
    float g;
    out[i] = lim_apply(x[i], G, lim_fir(w.data(), d.data(), H), r[(size_t)i], &g);
    if (g < 1.0f) ++st.limited;
    st.min_gain = fminf(st.min_gain, g);
  }
  return st;
}

}  // namespace xdtts
