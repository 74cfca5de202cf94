// rng.h -- the counter-based RNG (specification shared with oracle/, implemented independently).  Plain C++ with the HIP
// qualifiers only under hipcc: common.h brings it to the library, stream_plan.h to the host drivers that build with plain g++.
// Stream numbers in use: 0x47 the vocoder's initial phase, 0x1000 + ... the prenet dropout, the small row indices of the
// synthetic weights, 0x57AEA401 the TPDF dither of the stream stage (stream_plan.h), 0x71B8 the breath noise of the timbre
// stage (timbre_plan.h).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define XDTTS_RNG_HD __host__ __device__
#else
#define XDTTS_RNG_HD
#endif

namespace xdtts {

XDTTS_RNG_HD inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
XDTTS_RNG_HD inline uint32_t rng_u32(uint32_t seed, uint32_t stream, uint32_t idx) {
  return mix32(mix32(mix32(seed ^ 0x9E3779B9U) + stream) + idx);
}
XDTTS_RNG_HD inline float rng_uniform(uint32_t seed, uint32_t stream, uint32_t idx) {
  return (float)(rng_u32(seed, stream, idx) >> 8) * (1.0f / 16777216.0f);
}

}  // namespace xdtts
