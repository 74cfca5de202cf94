// timbre_plan.h -- the host arithmetic of the timbre stage (xdtts_timbre; the definition: include/xdtts.h): the argument rules,
// the identity test, and the noise term of the breath control -- n, v and N of a cell -- with its constant.
// Plain C++, no HIP and none of the library's headers but rng.h: tests/timbre_plan_test.cpp drives it with plain g++.  What the
// device shares carries TIMBRE_HD: timbre.hip's kernel evaluates the noise with these functions.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "rng.h"

#ifdef __HIPCC__
#define TIMBRE_HD __host__ __device__ __attribute__((always_inline))
#else
#define TIMBRE_HD
#endif

namespace xdtts {

constexpr uint32_t TIMBRE_NOISE_STREAM = 0x71B8u;        // rng.h: the stream number of the breath noise
constexpr int TIMBRE_NB = 513;                           // bins of a frame: the noise index is frame * 513 + bin
constexpr size_t TIMBRE_MAX_FRAMES = (size_t)1 << 20;    // of one request of the stage alone
constexpr float TIMBRE_VTL_MIN = 0.5f, TIMBRE_VTL_MAX = 2.0f;
constexpr int TIMBRE_LIFTER_MIN = 1, TIMBRE_LIFTER_MAX = 255;
constexpr float TIMBRE_NOISE_SHIFT = 0.28860784f;        // gamma / 2: E[ln(-ln v)] = -gamma for v uniform on (0, 1)

struct Timbre {  // == xdtts_timbre
  float vtl, breath;
  uint32_t seed;
  int32_t lifter;
  float log_floor;
};

inline Timbre timbre_default() { return Timbre{1.0f, 0.0f, 1u, 30, 1e-5f}; }

// the setting that launches nothing
inline bool timbre_is_identity(const Timbre &t) { return t.vtl == 1.0f && t.breath == 0.0f; }

// "" if the fields are a setting, else the message: it names the field
inline std::string timbre_check(const Timbre &t) {
  char msg[160];
  if (!std::isfinite(t.vtl) || t.vtl < TIMBRE_VTL_MIN || t.vtl > TIMBRE_VTL_MAX) {
    std::snprintf(msg, sizeof msg, "timbre vtl %g is not in [0.5, 2]", (double)t.vtl);
    return msg;
  }
  if (!std::isfinite(t.breath) || t.breath < 0.0f || t.breath > 1.0f) {
    std::snprintf(msg, sizeof msg, "timbre breath %g is not in [0, 1]", (double)t.breath);
    return msg;
  }
  if (t.lifter < TIMBRE_LIFTER_MIN || t.lifter > TIMBRE_LIFTER_MAX) {
    std::snprintf(msg, sizeof msg, "timbre lifter %d is not in [1, 255]", (int)t.lifter);
    return msg;
  }
  if (!std::isfinite(t.log_floor) || !(t.log_floor > 0.0f)) {
    std::snprintf(msg, sizeof msg, "timbre log_floor %g is not a positive number", (double)t.log_floor);
    return msg;
  }
  return "";
}

// ... and the frame count of a request of the stage alone: 1 .. 2^20 (no time interpolation: one frame is enough)
inline std::string timbre_frames_check(size_t n_frames) {
  char msg[160];
  if (n_frames < 1 || n_frames > TIMBRE_MAX_FRAMES) {
    std::snprintf(msg, sizeof msg, "timbre takes 1 .. 2^20 frames, got %zu", n_frames);
    return msg;
  }
  return "";
}

// n of cell (frame, bin): 23 bits of the counter-based stream, a function of (seed, frame, bin) alone
TIMBRE_HD inline uint32_t timbre_noise_bits(uint32_t seed, uint32_t frame, uint32_t bin) {
  return rng_u32(seed, TIMBRE_NOISE_STREAM, frame * (uint32_t)TIMBRE_NB + bin) >> 9;
}
// v = (2 n + 1) 2^-24: an odd integer below 2^24 times a power of two, exact in fp32, 0 < v < 1
TIMBRE_HD inline float timbre_noise_v(uint32_t n) { return (float)(2u * n + 1u) * (1.0f / 16777216.0f); }
// N = 0.5 ln(-ln v) + gamma / 2: the log of a Rayleigh magnitude, shifted to zero mean
TIMBRE_HD inline float timbre_noise(float v) { return 0.5f * logf(-logf(v)) + TIMBRE_NOISE_SHIFT; }

}  // namespace xdtts
