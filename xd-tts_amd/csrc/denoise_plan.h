// denoise_plan.h -- the host arithmetic of the clean-up stage (xdtts_denoise; the definition: include/xdtts.h): the argument
// rules, the identity test, the rank of the order statistic, the spectral floor, the tone curve, the records of the two launches
// with their index arithmetic, and the definition as serial plain C++ (denoise_reference).
// Plain C++, no HIP and none of the library's headers: tests/denoise_plan_test.cpp drives it with plain g++.  What the device
// shares carries DENOISE_HD: denoise.hip's kernels index with these functions.
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
#define DENOISE_HD __host__ __device__ __attribute__((always_inline))
#else
#define DENOISE_HD
#endif

namespace xdtts {

constexpr int DENOISE_NB = 513;                          // bins of a frame
constexpr int DENOISE_MAX_TONE = 8;                      // points of a tone curve
constexpr size_t DENOISE_MAX_FRAMES = (size_t)1 << 20;   // of one utterance of a request of the stage alone
constexpr double DENOISE_BIN_HZ = 22050.0 / 1024.0;      // f_k = k * 22050 / 1024
// k_noise_profile: a workgroup owns DENOISE_STRIP consecutive bins of one utterance; its DENOISE_LANES threads are
// DENOISE_STRIP bins x DENOISE_FSTEP frames, so a wave reads four 64-byte row segments.  33 strips: the last holds bin 512 alone.
constexpr int DENOISE_STRIP = 16;
constexpr int DENOISE_LANES = 512;
constexpr int DENOISE_FSTEP = DENOISE_LANES / DENOISE_STRIP;
constexpr int DENOISE_STRIPS = (DENOISE_NB + DENOISE_STRIP - 1) / DENOISE_STRIP;
// k_denoise: a wave per row, DENOISE_ROWS rows per workgroup; lane l holds bins l + 64 r (r < 8), lane 0 bin 512 as well
constexpr int DENOISE_ROWS = 4;

struct Denoise {  // == xdtts_denoise
  float strength, quantile, floor_db;
  int32_t n_tone;
  float tone_hz[DENOISE_MAX_TONE], tone_db[DENOISE_MAX_TONE];
};
struct DenoiseStats {  // == xdtts_denoise_stats
  uint32_t cells, floored, rank, profiled;
};

inline Denoise denoise_default() {
  Denoise d;
  std::memset(&d, 0, sizeof d);
  d.quantile = 0.5f;
  d.floor_db = -20.0f;
  return d;
}

// the setting that launches nothing: no subtraction, and every tone_db that is used is 0.  Only these decide it.
inline bool denoise_is_identity(const Denoise &d) {
  if (d.strength != 0.0f) return false;
  for (int i = 0; i < d.n_tone && i < DENOISE_MAX_TONE; ++i)
    if (d.tone_db[i] != 0.0f) return false;
  return true;
}
// ... of the tone curve alone: E = 1 in every bin, nothing is multiplied
inline bool denoise_tone_is_flat(const Denoise &d) {
  for (int i = 0; i < d.n_tone && i < DENOISE_MAX_TONE; ++i)
    if (d.tone_db[i] != 0.0f) return false;
  return true;
}

// "" if the fields are a setting, else the message: it names the field
inline std::string denoise_check(const Denoise &d) {
  char msg[200];
  if (!std::isfinite(d.strength) || d.strength < 0.0f || d.strength > 16.0f) {
    std::snprintf(msg, sizeof msg, "denoise strength %g is not in [0, 16]", (double)d.strength);
    return msg;
  }
  if (!std::isfinite(d.quantile) || d.quantile < 0.0f || d.quantile > 1.0f) {
    std::snprintf(msg, sizeof msg, "denoise quantile %g is not in [0, 1]", (double)d.quantile);
    return msg;
  }
  if (!std::isfinite(d.floor_db) || d.floor_db < -80.0f || d.floor_db > 0.0f) {
    std::snprintf(msg, sizeof msg, "denoise floor_db %g is not in [-80, 0]", (double)d.floor_db);
    return msg;
  }
  if (d.n_tone < 0 || d.n_tone > DENOISE_MAX_TONE) {
    std::snprintf(msg, sizeof msg, "denoise n_tone %d is not in [0, 8]", (int)d.n_tone);
    return msg;
  }
  for (int i = 0; i < d.n_tone; ++i) {
    if (!std::isfinite(d.tone_hz[i]) || !(d.tone_hz[i] > 0.0f) || d.tone_hz[i] > 11025.0f) {
      std::snprintf(msg, sizeof msg, "denoise tone_hz[%d] %g is not in (0, 11025]", i, (double)d.tone_hz[i]);
      return msg;
    }
    if (i > 0 && !(d.tone_hz[i] > d.tone_hz[i - 1])) {
      std::snprintf(msg, sizeof msg, "denoise tone_hz[%d] %g is not above tone_hz[%d] %g: the points are strictly ascending", i,
                    (double)d.tone_hz[i], i - 1, (double)d.tone_hz[i - 1]);
      return msg;
    }
    if (!std::isfinite(d.tone_db[i]) || d.tone_db[i] < -40.0f || d.tone_db[i] > 20.0f) {
      std::snprintf(msg, sizeof msg, "denoise tone_db[%d] %g is not in [-40, 20]", i, (double)d.tone_db[i]);
      return msg;
    }
  }
  return "";
}
// ... a caller's noise magnitude: every bin finite
inline std::string denoise_profile_check(const float *profile) {
  char msg[160];
  for (int k = 0; profile && k < DENOISE_NB; ++k)
    if (!std::isfinite(profile[k])) {
      std::snprintf(msg, sizeof msg, "denoise profile[%d] is not finite", k);
      return msg;
    }
  return "";
}
// ... and the frame count of an utterance of a request of the stage alone: 1 .. 2^20
inline std::string denoise_frames_check(size_t n_frames) {
  char msg[160];
  if (n_frames < 1 || n_frames > DENOISE_MAX_FRAMES) {
    std::snprintf(msg, sizeof msg, "denoise takes 1 .. 2^20 frames, got %zu", n_frames);
    return msg;
  }
  return "";
}
inline std::string denoise_quantile_check(float quantile) {
  char msg[160];
  if (!std::isfinite(quantile) || quantile < 0.0f || quantile > 1.0f) {
    std::snprintf(msg, sizeof msg, "denoise quantile %g is not in [0, 1]", (double)quantile);
    return msg;
  }
  return "";
}

// r = floor((double) quantile * (F - 1)): which of an utterance's F frames, in ascending order of the key, is "the noise"
inline uint32_t denoise_rank(size_t F, float quantile) {
  if (F < 1) return 0;
  const double r = std::floor((double)quantile * (double)(F - 1));
  return (uint32_t)std::min(std::max(r, 0.0), (double)(F - 1));
}
// gmin = (float) pow(10, (double) floor_db / 20): the one libm call of the gain rule, on the host
inline float denoise_floor(float floor_db) { return (float)std::pow(10.0, (double)floor_db / 20.0); }
// E[k], k = 0 .. 512: dB(k) piecewise linear in log2(f_k) between the points, constant outside them, bin 0 takes the first
// point's value; E = (float) pow(10, dB / 20), in double.  n_tone == 0: 1.
inline void denoise_tone(const Denoise &d, float *E) {
  for (int k = 0; k < DENOISE_NB; ++k) {
    if (d.n_tone <= 0) {
      E[k] = 1.0f;
      continue;
    }
    const int n = std::min<int>(d.n_tone, DENOISE_MAX_TONE);
    const double f = (double)k * DENOISE_BIN_HZ;
    double db;
    if (k == 0 || f <= (double)d.tone_hz[0]) {
      db = (double)d.tone_db[0];
    } else if (f >= (double)d.tone_hz[n - 1]) {
      db = (double)d.tone_db[n - 1];
    } else {
      int i = 0;
      while (i + 2 < n && f >= (double)d.tone_hz[i + 1]) ++i;  // hz[i] <= f < hz[i + 1]
      const double l0 = std::log2((double)d.tone_hz[i]), l1 = std::log2((double)d.tone_hz[i + 1]);
      const double a = (std::log2(f) - l0) / (l1 - l0);
      db = (double)d.tone_db[i] + a * ((double)d.tone_db[i + 1] - (double)d.tone_db[i]);
    }
    E[k] = (float)std::pow(10.0, db / 20.0);
  }
}

// key(x) = bits(x) & 0x7fffffff: a total order, the numeric one on the non-negative finite values mel -> linear produces
DENOISE_HD inline uint32_t denoise_key(float x) {
  uint32_t b;
#ifdef __HIP_DEVICE_COMPILE__
  b = __float_as_uint(x);
#else
  std::memcpy(&b, &x, sizeof b);
#endif
  return b & 0x7fffffffu;
}
inline float denoise_unkey(uint32_t key) {
  float x;
  std::memcpy(&x, &key, sizeof x);
  return x;
}

// ---- what the chain hands the plan for an utterance (magnitude_plan.h), and the record of the launches it becomes
// sub: the subtraction runs (strength != 0); profiled: N is the caller's profile (only looked at under sub); tone: the row of
// the tone table E [.][513] the utterance multiplies by, -1 = flat (nothing is multiplied)
struct DenoiseJob {
  float strength = 0.f, quantile = 0.5f, gmin = 0.1f;
  int sub = 0, profiled = 0, tone = -1;
};
inline DenoiseJob denoise_job(const Denoise &d, bool profile, int tone_row) {
  DenoiseJob j;
  j.strength = d.strength, j.quantile = d.quantile, j.gmin = denoise_floor(d.floor_db);
  j.sub = d.strength != 0.0f;
  j.profiled = j.sub && profile;
  j.tone = denoise_tone_is_flat(d) ? -1 : tone_row;
  return j;
}
// F rows from row row0 of S -> the same rows of S_clean; its N is row u of the per-utterance table (selected with `rank`) or the profile
struct DenoiseUtt {
  int row0, F, rank, sub, profiled, tone;
  float strength, gmin;
};
inline DenoiseUtt denoise_utt(const DenoiseJob &j, int row0, int F) {
  return DenoiseUtt{row0, F, (j.sub && !j.profiled) ? (int)denoise_rank((size_t)F, j.quantile) : 0, j.sub, j.profiled, j.tone, j.strength, j.gmin};
}
inline bool denoise_utt_selects(const DenoiseUtt &t) { return t.sub && !t.profiled; }

// ---- the index arithmetic of the two launches (tests/denoise_plan_test.cpp walks it on the host into buffers of the exact size)
// k_noise_profile: workgroup b of n_utt * DENOISE_STRIPS, thread tid of DENOISE_LANES
DENOISE_HD inline int denoise_profile_utt(int block) { return block / DENOISE_STRIPS; }
DENOISE_HD inline int denoise_profile_bin(int block, int tid) { return (block % DENOISE_STRIPS) * DENOISE_STRIP + (tid % DENOISE_STRIP); }  // live iff < 513
DENOISE_HD inline int denoise_profile_frame0(int tid) { return tid / DENOISE_STRIP; }  // then += DENOISE_FSTEP while < F
DENOISE_HD inline size_t denoise_cell(int row0, int frame, int bin) { return ((size_t)row0 + (size_t)frame) * DENOISE_NB + (size_t)bin; }
// k_denoise: the last utterance whose row0 <= row (row0 ascending; bounded: the index stays in [0, n_utt) whatever the table holds)
DENOISE_HD inline int denoise_row_utt(const DenoiseUtt *tab, int n_utt, int row) {
  int lo = 0, hi = n_utt - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].row0 <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}
DENOISE_HD inline int denoise_lane_bin(int lane, int r) { return r < 8 ? lane + 64 * r : 512; }  // r == 8: lane 0 only

// ---- the definition, serial: S and S_out n_bins x F in C order (bin-major, as mel -> linear returns it), profile 513 floats or
// null.  One operation per statement and contraction off: every product, quotient and difference is rounded to fp32 on its own.
#if defined(__clang__)
#define DENOISE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DENOISE_NO_CONTRACT  // (every rounded value below is a volatile fp32: nothing can be fused across it)
#endif
// the order statistic of the selection alone: N[k] = the float whose bits are the rank-th smallest key of bin k's F frames
inline void denoise_noise_reference(const float *S, size_t F, uint32_t rank, float *N) {
  std::vector<uint32_t> keys(F);
  for (int k = 0; k < DENOISE_NB; ++k) {
    for (size_t t = 0; t < F; ++t) keys[t] = denoise_key(S[(size_t)k * F + t]);
    std::nth_element(keys.begin(), keys.begin() + (ptrdiff_t)rank, keys.end());
    N[k] = denoise_unkey(keys[rank]);
  }
}
inline void denoise_reference(const float *S, size_t F, const Denoise &d, const float *profile, float *S_out, DenoiseStats *stats) {
  DENOISE_NO_CONTRACT
  const DenoiseJob j = denoise_job(d, profile != nullptr, 0);
  const DenoiseUtt t = denoise_utt(j, 0, (int)F);
  DenoiseStats st{(uint32_t)(F * (size_t)DENOISE_NB), 0u, (uint32_t)t.rank, (uint32_t)t.profiled};
  std::vector<float> N((size_t)DENOISE_NB, 0.0f), E((size_t)DENOISE_NB, 1.0f);
  if (denoise_utt_selects(t)) denoise_noise_reference(S, F, (uint32_t)t.rank, N.data());
  if (t.sub && t.profiled) std::copy(profile, profile + DENOISE_NB, N.begin());
  if (t.tone >= 0) denoise_tone(d, E.data());
  for (int k = 0; k < DENOISE_NB; ++k) {
    volatile float aN = j.strength * N[(size_t)k];  // (volatile: the statement's value is an fp32 in memory, whatever the compiler)
    for (size_t f = 0; f < F; ++f) {
      const float s = S[(size_t)k * F + f];
      float y = s;
      if (t.sub) {
        volatile float q = aN / s;
        volatile float dd = 1.0f - q;
        const float dv = dd;
        const bool above = dv > j.gmin;  // (false for a NaN: S == 0 gives gmin, and 0 comes out)
        const float G = above ? dv : j.gmin;
        st.floored += above ? 0u : 1u;
        volatile float p = s * G;
        y = p;
      }
      if (t.tone >= 0) {
        volatile float p = y * E[(size_t)k];
        y = p;
      }
      S_out[(size_t)k * F + f] = y;
    }
  }
  if (stats) *stats = st;
}

}  // namespace xdtts
