// silence_plan.h -- the arithmetic of the silence stage, the last stage of the delivery chain (xdtts_griffinlim_set_silence; the
// definition: include/xdtts.h): the argument rules, the host integers of a rate, the per-window decisions (sound, kept, where),
// the three passes of k_sil_plan over the windows exactly as its workgroup performs them, the gather with its fades, and the
// definition as serial plain C++.
// Plain C++, no HIP: tests/silence_plan_test.cpp drives it with plain g++.  Everything the device shares carries SIL_HD --
// silence.hip's kernels are the lane loops around these functions.  All decisions are integers and comparisons; the one fp32
// product of the definition (P tfac) stands alone, and a fade is one multiply per touched sample.  The one libm call (pow, for
// tfac) is the host's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "resample_plan.h"
#include "stream_plan.h"

#ifdef __HIPCC__
#define SIL_HD __host__ __device__ __attribute__((always_inline))
#else
#define SIL_HD
#endif

namespace xdtts {

constexpr int SIL_TILE = 4096;                        // samples of one utterance a workgroup of k_sil_peaks / k_sil_gather owns
constexpr int SIL_WG = 256;                           // lanes of a workgroup of k_sil_peaks / k_sil_gather
constexpr int SIL_WAVES = SIL_WG / 64;                // 4
constexpr int SIL_PLAN_WG = 1024;                     // lanes of k_sil_plan's workgroup: the chunk of windows it walks at a time
constexpr int SIL_PLAN_WAVES = SIL_PLAN_WG / 64;      // 16
constexpr int SIL_WIN_PER_S = 200;                    // W = rate / 200: 5 ms
constexpr double SIL_WIN_MS = 5.0;
constexpr int SIL_W_MIN = RESAMPLE_RATE_MIN / SIL_WIN_PER_S, SIL_W_MAX = RESAMPLE_RATE_MAX / SIL_WIN_PER_S;  // 40 .. 480 samples
constexpr int SIL_FADE_MAX = SIL_W_MAX / 2;           // entries of the fade table at most
constexpr int32_t SIL_DROPPED = -1;                   // the mark of a dropped window where a kept one has its output offset
constexpr size_t SIL_MAX_SAMPLES = (size_t)1 << 28;   // exclusive, as the loudness measurement
static_assert(SIL_W_MIN == 40 && SIL_W_MAX == 480 && SIL_WG % 64 == 0 && SIL_PLAN_WG % 64 == 0, "the window of every supported rate");

struct Silence {  // == xdtts_silence
  float threshold_db, min_sound_ms, lead_ms, trail_ms, max_pause_ms, fade_ms;
};
struct SilenceStats {  // == xdtts_silence_stats
  uint32_t n_in, n_out, lead_cut, trail_cut, pause_cut, n_cuts;
  float peak;
  uint32_t any_sound;
};
// what the kernels take: the host integers of (setting, rate) and the threshold's factor
struct SilPlan {
  int32_t W, min_w, lead_w, trail_w, pause_w, fade;
  float tfac;
};

inline Silence silence_default() { return Silence{-40.0f, 20.0f, 50.0f, 100.0f, 0.0f, 2.0f}; }

// "" if s is a setting, else the message: it names the field
inline std::string silence_check(const Silence &s) {
  char msg[200];
  const struct {
    const char *name;
    float v, lo, hi;
  } f[] = {{"threshold_db", s.threshold_db, -96.f, -6.f}, {"min_sound_ms", s.min_sound_ms, 0.f, 500.f}, {"lead_ms", s.lead_ms, 0.f, 10000.f},
           {"trail_ms", s.trail_ms, 0.f, 10000.f},        {"fade_ms", s.fade_ms, 0.f, 2.5f}};
  for (const auto &e : f)
    if (!std::isfinite(e.v) || e.v < e.lo || e.v > e.hi) {
      std::snprintf(msg, sizeof msg, "silence: %s %g is not a finite value in [%g, %g]", e.name, (double)e.v, (double)e.lo, (double)e.hi);
      return msg;
    }
  if (!std::isfinite(s.max_pause_ms) || (s.max_pause_ms != 0.f && (s.max_pause_ms < 20.f || s.max_pause_ms > 60000.f))) {
    std::snprintf(msg, sizeof msg, "silence: max_pause_ms %g is neither 0 (off) nor a finite value in [20, 60000]", (double)s.max_pause_ms);
    return msg;
  }
  return "";
}
// the rate: what the output-rate setting accepts
inline std::string silence_rate_check(long long rate) {
  ResamplePlan p;
  const std::string r = resample_check(rate, &p);
  return r.empty() ? r : "silence: rate: " + r;
}
// the arguments of the stage alone (xdtts_griffinlim_trim, xdtts_silence_keep, xdtts_silence_reference)
inline std::string silence_args_check(const Silence &s, long long rate, size_t n) {
  char msg[160];
  std::string r = silence_check(s);
  if (!r.empty()) return r;
  r = silence_rate_check(rate);
  if (!r.empty()) return r;
  if (n == 0 || n >= SIL_MAX_SAMPLES) {
    std::snprintf(msg, sizeof msg, "silence: n: need 1 .. 2^28 - 1 samples, got %zu", n);
    return msg;
  }
  return "";
}

// The host integers (checked arguments), in double: win(ms) = floor(ms / 5 + 0.5); tests/silence_ref.py repeats them.
inline int32_t sil_win(double ms) { return (int32_t)std::floor(ms / SIL_WIN_MS + 0.5); }
inline SilPlan silence_plan(const Silence &s, int rate) {
  SilPlan p{};
  p.W = rate / SIL_WIN_PER_S;
  p.min_w = sil_win((double)s.min_sound_ms);
  p.lead_w = sil_win((double)s.lead_ms);
  p.trail_w = sil_win((double)s.trail_ms);
  p.pause_w = sil_win((double)s.max_pause_ms);
  p.fade = std::min(p.W / 2, (int32_t)std::floor((double)s.fade_ms * (double)rate / 1000.0 + 0.5));
  p.tfac = (float)std::pow(10.0, (double)s.threshold_db / 20.0);
  return p;
}
// the fade gains: the rising half of the stream stage's table, T[0 .. fade)
inline void silence_fade_table(const SilPlan &p, float *T) { stream_fade_table(p.fade, T); }

inline size_t silence_windows(size_t n, int W) { return (n + (size_t)W - 1) / (size_t)W; }
inline size_t silence_tiles(size_t n) { return (n + SIL_TILE - 1) / SIL_TILE; }

// ---- one window -------------------------------------------------------------------------------------------------------------

SIL_HD inline uint32_t sil_abs_bits(float x) {  // |x| as an integer: its order is the floats'
  uint32_t u;
  __builtin_memcpy(&u, &x, sizeof u);
  return u & 0x7fffffffu;
}
SIL_HD inline float sil_float(uint32_t u) {
  float a;
  __builtin_memcpy(&a, &u, sizeof a);
  return a;
}
SIL_HD inline int sil_win_len(int w, int nw, int n, int W) { return w == nw - 1 ? n - w * W : W; }
// a window belongs to the tile it starts in: the windows of the tile at t0 (a multiple of SIL_TILE below n) are w0 .. w1
SIL_HD inline int sil_tile_win0(int t0, int W) { return (t0 + W - 1) / W; }
SIL_HD inline int sil_tile_win1(int t0, int n, int W) { return ((t0 + SIL_TILE < n ? t0 + SIL_TILE : n) + W - 1) / W; }
// the threshold: one fp32 product; a window is a candidate where its peak is strictly above it (P == 0: none is)
SIL_HD inline float sil_threshold(float P, float tfac) { return P * tfac; }
SIL_HD inline bool sil_candidate(float pw, float thr) { return pw > thr; }
// windows kept of an utterance without sound
SIL_HD inline int sil_quiet_keep(int nw, const SilPlan &p) {
  const int k = p.lead_w + p.trail_w > 1 ? p.lead_w + p.trail_w : 1;
  return nw < k ? nw : k;
}
// is window w kept?  a: it is sound; l, r: the nearest sound window at or in front of w (-1: none) and at or behind it (nw: none)
SIL_HD inline bool sil_keep_rule(int w, bool a, int l, int r, int nw, const SilPlan &p) {
  if (a) return true;
  if (l < 0 && r >= nw) return w < sil_quiet_keep(nw, p);
  if (l < 0) return r - w <= p.lead_w;
  if (r >= nw) return w - l <= p.trail_w;
  return p.pause_w == 0 || w - l <= p.pause_w - p.pause_w / 2 || r - w <= p.pause_w / 2;
}
// where a dropped window's samples are counted: 0 lead, 1 trail (an utterance without sound: all of it), 2 pause
SIL_HD inline int sil_cut_kind(int l, int r, int nw) { return r >= nw ? 1 : (l < 0 ? 0 : 2); }
// sample k of a kept window of len samples: faded in where the window in front is dropped, out where the one behind is
SIL_HD inline float sil_sample(float x, int k, int len, bool fade_in, bool fade_out, int fade, const float *T) {
  if (fade_in && k < fade) return x * T[k];
  if (fade_out && len - 1 - k < fade) return x * T[len - 1 - k];
  return x;
}

// ---- the definition, window by window, in the serial form ---------------------------------------------------------------------

inline void silence_window_peaks(const float *x, size_t n, int W, std::vector<float> &pw, float *P) {
  const size_t nw = silence_windows(n, W);
  pw.assign(nw, 0.0f);
  uint32_t top = 0;
  for (size_t w = 0; w < nw; ++w) {
    uint32_t pk = 0;
    for (size_t i = w * (size_t)W; i < std::min(n, (w + 1) * (size_t)W); ++i) pk = std::max(pk, sil_abs_bits(x[i]));
    pw[w] = sil_float(pk);
    top = std::max(top, pk);
  }
  *P = sil_float(top);
}
// a[w]: sound; steps 2 and 3
inline void silence_sound(const std::vector<float> &pw, float P, const SilPlan &p, std::vector<uint8_t> &a) {
  const size_t nw = pw.size();
  const float thr = sil_threshold(P, p.tfac);
  const size_t need = (size_t)std::max(p.min_w, 1);
  a.assign(nw, 0);
  for (size_t w = 0; w < nw;) {
    if (!sil_candidate(pw[w], thr)) {
      ++w;
      continue;
    }
    size_t e = w;
    while (e < nw && sil_candidate(pw[e], thr)) ++e;
    if (e - w >= need) std::fill(a.begin() + (long)w, a.begin() + (long)e, (uint8_t)1);
    w = e;
  }
}
// keep[w]; steps 4 and 5.  Returns any_sound.
inline bool silence_keep_from_sound(const std::vector<uint8_t> &a, const SilPlan &p, std::vector<uint8_t> &keep, std::vector<int> *l_out = nullptr,
                                    std::vector<int> *r_out = nullptr) {
  const int nw = (int)a.size();
  std::vector<int> l((size_t)nw), r((size_t)nw);
  int at = -1;
  for (int w = 0; w < nw; ++w) l[(size_t)w] = at = a[(size_t)w] ? w : at;
  at = nw;
  for (int w = nw - 1; w >= 0; --w) r[(size_t)w] = at = a[(size_t)w] ? w : at;
  keep.assign((size_t)nw, 0);
  for (int w = 0; w < nw; ++w) keep[(size_t)w] = sil_keep_rule(w, a[(size_t)w] != 0, l[(size_t)w], r[(size_t)w], nw, p) ? 1 : 0;
  const bool any = nw > 0 && r[0] < nw;
  if (l_out) *l_out = std::move(l);
  if (r_out) *r_out = std::move(r);
  return any;
}
// the per-window decisions of one utterance (xdtts_silence_keep)
inline void silence_keep(const float *x, size_t n, const SilPlan &p, uint8_t *keep) {
  std::vector<float> pw;
  float P;
  silence_window_peaks(x, n, p.W, pw, &P);
  std::vector<uint8_t> a, k;
  silence_sound(pw, P, p, a);
  silence_keep_from_sound(a, p, k);
  std::memcpy(keep, k.data(), k.size());
}
// the whole stage (xdtts_silence_reference): out holds n floats, of which [0, n_out) are written
inline SilenceStats silence_reference(const float *x, size_t n, int rate, const Silence &s, float *out) {
  const SilPlan p = silence_plan(s, rate);
  std::vector<float> T((size_t)std::max(p.fade, 1));
  silence_fade_table(p, T.data());
  std::vector<float> pw;
  float P;
  silence_window_peaks(x, n, p.W, pw, &P);
  std::vector<uint8_t> a, keep;
  std::vector<int> l, r;
  silence_sound(pw, P, p, a);
  const bool any = silence_keep_from_sound(a, p, keep, &l, &r);
  const int nw = (int)pw.size();
  SilenceStats st{(uint32_t)n, 0, 0, 0, 0, 0, P, any ? 1u : 0u};
  size_t at = 0;
  for (int w = 0; w < nw; ++w) {
    const int len = sil_win_len(w, nw, (int)n, p.W);
    if (!keep[(size_t)w]) {
      const int kind = sil_cut_kind(l[(size_t)w], r[(size_t)w], nw);
      (kind == 0 ? st.lead_cut : (kind == 1 ? st.trail_cut : st.pause_cut)) += (uint32_t)len;
      continue;
    }
    const bool fin = w > 0 && !keep[(size_t)w - 1], fout = w < nw - 1 && !keep[(size_t)w + 1];
    st.n_cuts += (fin ? 1u : 0u) + (fout ? 1u : 0u);
    const float *xs = x + (size_t)w * (size_t)p.W;
    for (int k = 0; k < len; ++k) out[at + (size_t)k] = sil_sample(xs[k], k, len, fin, fout, p.fade, T.data());
    at += (size_t)len;
  }
  st.n_out = (uint32_t)at;
  return st;
}

// ---- the launches on the host, as the workgroups perform them ----------------------------------------------------------------
// Arrays that stand for device scratch have exactly the kernels' sizes: pw, wl, wr, woff one entry per window, tpk one per tile.

// k_sil_peaks, the tile at t0: wave v takes the tile's windows w0 + v, w0 + v + SIL_WAVES, ..., its lanes stride over the
// window's samples -- on past the tile's end where the window runs on -- and the tile's peak is the largest of its windows'.
inline void silence_tile_peaks(const float *x, int n, int t0, const SilPlan &p, float *pw, float *tpk) {
  const int nw = (int)silence_windows((size_t)n, p.W), w0 = sil_tile_win0(t0, p.W), w1 = sil_tile_win1(t0, n, p.W);
  uint32_t top = 0;
  for (int v = 0; v < SIL_WAVES; ++v)
    for (int w = w0 + v; w < w1; w += SIL_WAVES) {
      const int len = sil_win_len(w, nw, n, p.W);
      uint32_t pk = 0;
      for (int lane = 0; lane < 64; ++lane)
        for (int k = lane; k < len; k += 64) pk = std::max(pk, sil_abs_bits(x[(size_t)w * (size_t)p.W + (size_t)k]));
      pw[w] = sil_float(pk);
      top = std::max(top, pk);
    }
  tpk[t0 / SIL_TILE] = sil_float(top);
}

// k_sil_plan: P from the tiles' peaks, then three passes over the windows in chunks of SIL_PLAN_WG with integer carries --
//   1 forwards   wl[w] = the nearest window at or in front of w that is no candidate (-1: none)
//   2 backwards  the nearest one at or behind w (nw: none), from both the run's length and a[w]; wr[w] = the nearest sound
//                window at or behind w (nw: none); wl[w] = a[w]
//   3 forwards   the nearest sound window at or in front of w, keep[w], the exclusive prefix sum of the kept lengths ->
//                woff[w] (SIL_DROPPED where dropped), and the stats.
// The backward pass walks the mirrored index w' = nw - 1 - w, so that every scan is an ascending inclusive maximum.
inline SilenceStats silence_plan_walk(const float *pw, const float *tpk, int n, const SilPlan &p, int32_t *wl, int32_t *wr, int32_t *woff) {
  const int nw = (int)silence_windows((size_t)n, p.W), tiles = (int)silence_tiles((size_t)n);
  uint32_t top = 0;
  for (int t = 0; t < tiles; ++t) top = std::max(top, sil_abs_bits(tpk[t]));
  const float P = sil_float(top), thr = sil_threshold(P, p.tfac);
  const int need = p.min_w > 1 ? p.min_w : 1;
  int carry = -1;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG)
    for (int tid = 0; tid < SIL_PLAN_WG; ++tid) {
      const int w = c0 + tid;
      if (w >= nw) break;
      if (!sil_candidate(pw[w], thr)) carry = w;
      wl[w] = carry;
    }
  int carry0 = -1, carry1 = -1;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG)
    for (int tid = 0; tid < SIL_PLAN_WG; ++tid) {
      const int m = c0 + tid, w = nw - 1 - m;
      if (m >= nw) break;
      const bool a0 = sil_candidate(pw[w], thr);
      if (!a0) carry0 = m;
      const int R0 = nw - 1 - carry0;
      const bool a = a0 && R0 - wl[w] - 1 >= need;
      if (a) carry1 = m;
      wr[w] = nw - 1 - carry1;
      wl[w] = a ? 1 : 0;
    }
  SilenceStats st{(uint32_t)n, 0, 0, 0, 0, 0, P, 0};
  int l = -1, prev_keep = 0;
  uint32_t at = 0;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG)
    for (int tid = 0; tid < SIL_PLAN_WG; ++tid) {
      const int w = c0 + tid;
      if (w >= nw) break;
      const bool a = wl[w] != 0;
      if (a) l = w;
      const int r = wr[w], len = sil_win_len(w, nw, n, p.W);
      const bool keep = sil_keep_rule(w, a, l, r, nw, p);
      woff[w] = keep ? (int32_t)at : SIL_DROPPED;
      if (keep) at += (uint32_t)len;
      else {
        const int kind = sil_cut_kind(l, r, nw);
        (kind == 0 ? st.lead_cut : (kind == 1 ? st.trail_cut : st.pause_cut)) += (uint32_t)len;
      }
      if (w > 0 && (keep ? 1 : 0) != prev_keep) ++st.n_cuts;
      prev_keep = keep ? 1 : 0;
    }
  st.n_out = at;
  st.any_sound = l >= 0 ? 1u : 0u;
  return st;
}

// k_sil_gather, the tile at t0: the kept windows that start in it go to their offsets, with the fades
inline void silence_tile_gather(const float *x, int n, int t0, const SilPlan &p, const float *T, const int32_t *woff, float *out) {
  const int nw = (int)silence_windows((size_t)n, p.W), w0 = sil_tile_win0(t0, p.W), w1 = sil_tile_win1(t0, n, p.W);
  for (int w = w0; w < w1; ++w) {
    if (woff[w] == SIL_DROPPED) continue;
    const int len = sil_win_len(w, nw, n, p.W);
    const bool fin = w > 0 && woff[w - 1] == SIL_DROPPED, fout = w < nw - 1 && woff[w + 1] == SIL_DROPPED;
    for (int k = 0; k < len; ++k) out[(size_t)woff[w] + (size_t)k] = sil_sample(x[(size_t)w * (size_t)p.W + (size_t)k], k, len, fin, fout, p.fade, T);
  }
}

}  // namespace xdtts
