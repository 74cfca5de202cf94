// stream_plan.h -- the arithmetic of the stream stage (xdtts_griffinlim_join, xdtts_synthesize_document; the definition:
// include/xdtts.h): the argument rules, offsets and total of a joined sequence, the fade table, the per-sample encoders
// (fade, gain, PCM16 cast, TPDF dither, G.711 mu-law and A-law), and the tile / segment / pack walk of k_stream_join.
// Plain C++, no HIP and none of the library's headers but rng.h: tests/stream_plan_test.cpp drives it with plain g++.
// Everything the device shares carries STREAM_HD -- stream.hip's kernel is the tile loop around stream_pack() and one store.
// Every product of the definition is rounded to fp32 on its own: the functions that multiply switch contraction off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rng.h"

#ifdef __HIPCC__
#define STREAM_HD __host__ __device__ __attribute__((always_inline))
#else
#define STREAM_HD
#endif
#ifdef __clang__
#define STREAM_NO_CONTRACT _Pragma("clang fp contract(off)")
#define STREAM_UNROLL _Pragma("unroll")
#else
#define STREAM_NO_CONTRACT  // (g++ on x86-64 without -mfma has no fused instruction to contract into)
#define STREAM_UNROLL
#endif

namespace xdtts {

constexpr int STREAM_F32 = 0, STREAM_PCM16 = 1, STREAM_ULAW = 2, STREAM_ALAW = 3;
constexpr int STREAM_UTT_MAX = 4096;
constexpr int STREAM_FADE_MAX = 4800;
constexpr size_t STREAM_TOTAL_MAX = (size_t)1 << 28;  // exclusive: what the loudness measurement takes as one signal
constexpr uint32_t STREAM_DITHER_STREAM = 0x57AEA401u;  // rng.h: the stream number of the dither
constexpr int STREAM_PACK_BYTES = 16;                 // what a lane writes per step: one 128-bit store
constexpr int STREAM_WG = 256;                        // lanes of a workgroup
constexpr int STREAM_STEPS = 4;                       // packs of a lane
constexpr int STREAM_TILE_PACKS = STREAM_WG * STREAM_STEPS;  // a workgroup's tile: 16 KiB of the output stream
constexpr int STREAM_CACHE = 64;                      // utterance records a workgroup keeps in LDS

struct StreamOpts {  // == xdtts_stream_opts
  int32_t format, dither;
  uint32_t dither_seed;
  int32_t level, fade;
};
inline StreamOpts stream_opts_default() { return StreamOpts{STREAM_PCM16, 0, 0u, 0, 0}; }

STREAM_HD inline int stream_sample_bytes(int format) {
  return format == STREAM_F32 ? 4 : (format == STREAM_PCM16 ? 2 : ((format == STREAM_ULAW || format == STREAM_ALAW) ? 1 : 0));
}
STREAM_HD inline int stream_pack_samples(int format) { return STREAM_PACK_BYTES / stream_sample_bytes(format); }

// "" if the options are in range, else the message: it names the field
inline std::string stream_opts_check(const StreamOpts &o) {
  char msg[160];
  msg[0] = 0;
  if (o.format < 0 || o.format > 3) std::snprintf(msg, sizeof msg, "stream: format %d is not 0 (fp32), 1 (PCM16), 2 (mu-law) or 3 (A-law)", o.format);
  else if (o.dither != 0 && o.dither != 1) std::snprintf(msg, sizeof msg, "stream: dither %d is not 0 or 1", o.dither);
  else if (o.dither == 1 && o.format != STREAM_PCM16) std::snprintf(msg, sizeof msg, "stream: dither is defined for format 1 (PCM16) only, format is %d", o.format);
  else if (o.level != 0 && o.level != 1) std::snprintf(msg, sizeof msg, "stream: level %d is not 0 (per utterance) or 1 (programme)", o.level);
  else if (o.fade < 0 || o.fade > STREAM_FADE_MAX) std::snprintf(msg, sizeof msg, "stream: fade %d is not in [0, %d]", o.fade, STREAM_FADE_MAX);
  return msg;
}

// offset[u] = gap[0] + sum over v < u of (n[v] + gap[v + 1]);  total = offset[U - 1] + n[U - 1] + gap[U], 1 <= total < 2^28.
// "" if the layout is in range (offsets[0 .. U) and *total filled in, either may be null), else the message: it names the field
// and the index.  Every term is looked at before it is added: nothing overflows.
inline std::string stream_plan(const size_t *n, long long n_utt, const size_t *gaps, size_t *offsets, size_t *total) {
  char msg[200];
  if (total) *total = 0;
  if (n_utt < 1 || n_utt > STREAM_UTT_MAX) {
    std::snprintf(msg, sizeof msg, "stream: n_utt %lld is not in [1, %d]", n_utt, STREAM_UTT_MAX);
    return msg;
  }
  if (!n) return "stream: null n";
  size_t at = 0;
  for (long long u = 0; u <= n_utt; ++u) {
    const size_t g = gaps ? gaps[u] : 0;
    if (g >= STREAM_TOTAL_MAX || at + g >= STREAM_TOTAL_MAX) {
      std::snprintf(msg, sizeof msg, "stream: gaps[%lld] = %zu takes the stream to 2^28 samples or more", u, g);
      return msg;
    }
    at += g;
    if (u == n_utt) break;
    if (offsets) offsets[u] = at;
    if (n[u] >= STREAM_TOTAL_MAX || at + n[u] >= STREAM_TOTAL_MAX) {
      std::snprintf(msg, sizeof msg, "stream: n[%lld] = %zu takes the stream to 2^28 samples or more", u, n[u]);
      return msg;
    }
    at += n[u];
  }
  if (at == 0) return "stream: total is 0 samples (every n and every gap is zero)";
  if (total) *total = at;
  return "";
}

// T[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade), j < fade: in double, rounded once
inline void stream_fade_table(int fade, float *w) {
  const double PI = 3.14159265358979323846;
  for (int j = 0; j < fade; ++j) w[j] = (float)(0.5 - 0.5 * std::cos(PI * ((double)j + 0.5) / (double)fade));
}

// ---- one sample ------------------------------------------------------------------------------------------------------------

// Rust's `v as i16`: truncating toward zero, saturating, NaN -> 0 (xdtts_audio_to_i16)
STREAM_HD inline int stream_cast_i16(float v) {
  if (v != v) return 0;
  if (v >= 32767.0f) return 32767;
  if (v <= -32768.0f) return -32768;
  return (int)v;
}
// d = u(2 k) - u(2 k + 1): both are multiples of 2^-24 in [0, 1), the difference is exact
STREAM_HD inline float stream_dither(uint32_t seed, uint32_t k) {
  return rng_uniform(seed, STREAM_DITHER_STREAM, 2u * k) - rng_uniform(seed, STREAM_DITHER_STREAM, 2u * k + 1u);
}
// q of step 4: the cast, or with dither floor(fl(fl(v + d) + 0.5)) saturated
STREAM_HD inline int stream_quantise(float x, int dither, uint32_t seed, uint32_t k) {
  STREAM_NO_CONTRACT
  float v = x * 32767.0f;
  if (!dither) return stream_cast_i16(v);
  v = v + stream_dither(seed, k);
  const float r = std::floor(v + 0.5f);
  if (r != r) return 0;
  if (r >= 32767.0f) return 32767;
  if (r <= -32768.0f) return -32768;
  return (int)r;
}
STREAM_HD inline int stream_log2(uint32_t m) { return 31 - __builtin_clz(m); }  // floor(log2 m), m >= 1
STREAM_HD inline uint32_t stream_ulaw(int q) {
  const uint32_t a = (uint32_t)(q < 0 ? -q : q) > 32767u ? 32767u : (uint32_t)(q < 0 ? -q : q);
  const uint32_t c = a >> 2, m = (c > 8158u ? 8158u : c) + 33u;
  const int e = stream_log2(m) - 5;
  const uint32_t mant = (m >> (e + 1)) & 15u;
  return 0xFFu ^ ((q < 0 ? 0x80u : 0u) | ((uint32_t)e << 4) | mant);
}
STREAM_HD inline uint32_t stream_alaw(int q) {
  const uint32_t a = (uint32_t)(q < 0 ? -q : q) > 32767u ? 32767u : (uint32_t)(q < 0 ? -q : q);
  const uint32_t a13 = a >> 3;
  uint32_t e = 0, mant = a13 >> 1;
  if (a13 >= 32u) {
    e = (uint32_t)(stream_log2(a13) - 4);
    mant = (a13 >> e) & 15u;
  }
  return ((q < 0 ? 0u : 0x80u) | (e << 4) | mant) ^ 0x55u;
}
// steps 3 to 5 for one sample behind fade and gain: the sample's bits in the low 4, 2 or 1 bytes
STREAM_HD inline uint32_t stream_encode(float x, int format, int dither, uint32_t seed, uint32_t k) {
  if (format == STREAM_F32) {
    union {
      float f;
      uint32_t u;
    } b;
    b.f = x;
    return b.u;
  }
  if (format == STREAM_PCM16) return (uint32_t)stream_quantise(x, dither, seed, k) & 0xFFFFu;
  const int q = stream_quantise(x, 0, 0u, 0u);
  return format == STREAM_ULAW ? stream_ulaw(q) : stream_alaw(q);
}
// a gap's sample: fp32 +0, PCM16 0, mu-law 0xFF, A-law 0xD5 (dither does not reach the gaps: they are exact zeros)
STREAM_HD inline uint32_t stream_silence(int format) {
  return format == STREAM_ULAW ? 0xFFu : (format == STREAM_ALAW ? 0xD5u : 0u);
}

// steps 1 and 2: sample i of an utterance of n samples; T = the fade table (null without a fade); the gain at programme level only
STREAM_HD inline float stream_shape(float x, int i, int n, int fade, const float *T, bool levelled, float gain) {
  STREAM_NO_CONTRACT
  if (fade > 0) {
    const int f = fade < n / 2 ? fade : n / 2;
    if (i < f) x = x * T[i];
    else if (n - 1 - i < f) x = x * T[n - 1 - i];
  }
  if (levelled) x = x * gain;
  return x;
}

// ---- the walk of k_stream_join ---------------------------------------------------------------------------------------------

// One utterance of the table, ascending off: n samples at src + src0 go to stream positions [off, off + n).  Whatever lies
// between two utterances, in front of the first and behind the last is a gap.
struct StreamUtt {
  long long src0;
  uint32_t off;
  int32_t n;
};
struct alignas(16) StreamF4 {
  float v[4];
};
struct StreamJob {
  const float *src;
  const StreamUtt *tab;  // [n_utt]
  const float *fade_tab;   // [fade], null without
  const double *gain;      // the programme gain in device memory (LoudResult::gain), null at level 0
  int32_t n_utt;
  uint32_t total;
  int32_t format, dither;
  uint32_t seed;
  int32_t fade;
};

// the last utterance of tab[0 .. count) with off <= k, -1 if none: a bounded binary search (13 steps cover 4096 records)
STREAM_HD inline int stream_owner(const StreamUtt *tab, int count, uint32_t k) {
  int lo = -1, hi = count - 1;
  for (int it = 0; it < 16 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].off <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// What a workgroup keeps of the table: records [u0, u0 + cnt) -- u0 the owner of the tile's first sample (0 if a gap leads
// the stream) -- and the stream position where the first record behind them begins (2^32 - 1 where there is none: the
// whole rest of the stream is then decided by the cache).
struct StreamCache {
  int u0, cnt;
  uint32_t end;
};
STREAM_HD inline StreamCache stream_cache_plan(const StreamUtt *tab, int n_utt, uint32_t tile_k0) {
  StreamCache c;
  const int o = stream_owner(tab, n_utt, tile_k0);
  c.u0 = o < 0 ? 0 : o;
  c.cnt = n_utt - c.u0 < STREAM_CACHE ? n_utt - c.u0 : STREAM_CACHE;
  c.end = c.u0 + c.cnt < n_utt ? tab[c.u0 + c.cnt].off : 0xFFFFFFFFu;
  return c;
}
// the owner of sample k of the tile (k >= the tile's first sample): in the cache where the cache decides it, else the
// bounded search in the table
STREAM_HD inline int stream_owner_cached(const StreamUtt *cache, const StreamCache c, const StreamUtt *tab, int n_utt, uint32_t k) {
  if (k < c.end) {
    const int o = stream_owner(cache, c.cnt, k);
    return o < 0 ? -1 : c.u0 + o;  // (-1: u0 = 0 and a gap leads the stream)
  }
  return stream_owner(tab, n_utt, k);
}
STREAM_HD inline StreamUtt stream_record(const StreamUtt *cache, const StreamCache c, const StreamUtt *tab, int u) {
  return (u >= c.u0 && u < c.u0 + c.cnt) ? cache[u - c.u0] : tab[u];
}

// One pack: the P = 16 / sample_bytes samples from k0 = pack * P on, encoded into w[4] (little endian, sample j at byte
// j * sample_bytes).  Samples at or behind `total` are left as silence; the caller does not store them.
// Three routes: the pack inside one gap (constants), inside one utterance (128-bit loads where the source address is a
// multiple of 16 bytes, scalar loads otherwise), or anything else -- sample by sample, each with its own owner lookup, so a
// pack may span any number of utterances and gaps.
template <int FORMAT>
STREAM_HD inline void stream_pack(const StreamJob &J, const StreamUtt *cache, const StreamCache c, uint32_t pack, uint32_t w[4]) {
  constexpr int SB = FORMAT == STREAM_F32 ? 4 : (FORMAT == STREAM_PCM16 ? 2 : 1), P = STREAM_PACK_BYTES / SB, PER = 4 / SB;
  const uint32_t k0 = pack * (uint32_t)P;
  const uint32_t sil = stream_silence(FORMAT);
STREAM_UNROLL
  for (int q = 0; q < 4; ++q) w[q] = SB == 1 ? sil * 0x01010101u : 0u;
  const bool levelled = J.gain != nullptr;
  const float gain = levelled ? (float)*J.gain : 1.0f;
  const int o = stream_owner_cached(cache, c, J.tab, J.n_utt, k0);
  StreamUtt r{0, 0u, 0};
  if (o >= 0) r = stream_record(cache, c, J.tab, o);
  const uint32_t r_end = r.off + (uint32_t)r.n;  // (o < 0: 0)
  const uint32_t total = J.total;
  uint32_t next = total;
  if (o + 1 < J.n_utt) next = stream_record(cache, c, J.tab, o + 1).off;
  const uint32_t k1 = k0 + (uint32_t)P;  // (< 2^28 + 16)
  if (k0 >= r_end && (k1 <= next || next >= total)) return;  // a gap, or the tail behind the last utterance
  if (o >= 0 && k1 <= r_end) {  // the interior of utterance o
    const int i0 = (int)(k0 - r.off);
    const float *p = J.src + r.src0 + i0;
    float x[P];
    if ((((uintptr_t)p) & 15u) == 0) {
STREAM_UNROLL
      for (int q = 0; q < P / 4; ++q) {
        const StreamF4 v = *reinterpret_cast<const StreamF4 *>(p + 4 * q);
STREAM_UNROLL
        for (int t = 0; t < 4; ++t) x[4 * q + t] = v.v[t];
      }
    } else {
STREAM_UNROLL
      for (int j = 0; j < P; ++j) x[j] = p[j];
    }
STREAM_UNROLL
    for (int j = 0; j < P; ++j) {
      const float y = stream_shape(x[j], i0 + j, r.n, J.fade, J.fade_tab, levelled, gain);
      const uint32_t b = stream_encode(y, FORMAT, J.dither, J.seed, k0 + (uint32_t)j);
      if (SB == 4) w[j] = b;
      else w[j / PER] = (w[j / PER] & ~((SB == 2 ? 0xFFFFu : 0xFFu) << (8 * SB * (j % PER)))) | (b << (8 * SB * (j % PER)));
    }
    return;
  }
STREAM_UNROLL
  for (int j = 0; j < P; ++j) {  // sample by sample
    const uint32_t k = k0 + (uint32_t)j;
    if (k >= total) continue;
    const int u = stream_owner_cached(cache, c, J.tab, J.n_utt, k);
    if (u < 0) continue;
    const StreamUtt t = stream_record(cache, c, J.tab, u);
    const uint32_t i = k - t.off;
    if (i >= (uint32_t)t.n) continue;  // behind utterance u: a gap
    const float y = stream_shape(J.src[t.src0 + (long long)i], (int)i, t.n, J.fade, J.fade_tab, levelled, gain);
    const uint32_t b = stream_encode(y, FORMAT, J.dither, J.seed, k);
    if (SB == 4) w[j] = b;
    else w[j / PER] = (w[j / PER] & ~((SB == 2 ? 0xFFFFu : 0xFFu) << (8 * SB * (j % PER)))) | (b << (8 * SB * (j % PER)));
  }
}

inline uint32_t stream_packs(size_t total, int format) {
  const size_t P = (size_t)stream_pack_samples(format);
  return (uint32_t)((total + P - 1) / P);
}
inline uint32_t stream_tiles(size_t total, int format) {
  return (stream_packs(total, format) + STREAM_TILE_PACKS - 1) / STREAM_TILE_PACKS;
}

}  // namespace xdtts
