// gl_fft.h -- the framed-FFT building blocks the Griffin-Lim kernels (griffinlim.hip) and the analysis kernels (analysis.hip)
// share: complex helpers, the 8-point butterfly, the in-register 512-point Stockham transform of one wave, its twiddle fetch,
// and the numpy "reflect" padding index.  Included by both translation units.
#pragma once
#include "kernels.h"

namespace xdtts {
namespace {

constexpr int NFFT = 1024, HOP = 256;  // the reference's vocoder geometry (mod.rs:453-456); checked at GriffinLim::new
constexpr int FRAMES_PER_BLOCK = 4;    // one wave per frame

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // * (-i)

// forward 8-point DFT, natural-order output
__device__ __forceinline__ void fft8(float2 (&v)[8]) {
  const float h = 0.70710678118654752440f;
  float2 b0 = cadd(v[0], v[4]), b4 = csub(v[0], v[4]);
  float2 b1 = cadd(v[1], v[5]), b5 = csub(v[1], v[5]);
  float2 b2 = cadd(v[2], v[6]), b6 = csub(v[2], v[6]);
  float2 b3 = cadd(v[3], v[7]), b7 = csub(v[3], v[7]);
  b5 = make_float2(h * (b5.x + b5.y), h * (b5.y - b5.x));   // * (1-i)/sqrt2
  b6 = mul_mi(b6);                                           // * (-i)
  b7 = make_float2(h * (b7.y - b7.x), -h * (b7.x + b7.y));  // * (-1-i)/sqrt2
  float2 d0 = cadd(b0, b2), d1 = csub(b0, b2), d2 = cadd(b1, b3), d3 = mul_mi(csub(b1, b3));
  v[0] = cadd(d0, d2);
  v[4] = csub(d0, d2);
  v[2] = cadd(d1, d3);
  v[6] = csub(d1, d3);
  d0 = cadd(b4, b6);
  d1 = csub(b4, b6);
  d2 = cadd(b5, b7);
  d3 = mul_mi(csub(b5, b7));
  v[1] = cadd(d0, d2);
  v[5] = csub(d0, d2);
  v[3] = cadd(d1, d3);
  v[7] = csub(d1, d3);
}

// Per-lane twiddles of the two twiddled passes, pulled from the table once at kernel entry (in
// the same memory round trip as the frame's data) so the FFT itself never waits on global memory.
struct Twiddles {
  float2 p8[7];   // pass Ns = 8 : e^{-2 pi i r k / 64},  k = lane & 7  -> table index r*k*16
  float2 p64[7];  // pass Ns = 64: e^{-2 pi i r k / 512}, k = lane      -> table index r*k*2
};
__device__ __forceinline__ Twiddles load_twiddles(const float2 *__restrict__ tw, int lane) {
  Twiddles t;
  const int k = lane & 7;
#pragma unroll
  for (int r = 1; r < 8; ++r) {
    t.p8[r - 1] = tw[r * k * 16];
    t.p64[r - 1] = tw[r * lane * 2];
  }
  return t;
}

// Orders a wave's LDS stores before its later LDS loads of other lanes' addresses.  DS operations
// of one wave execute in order, so only the compiler has to be held back; waves stay decoupled.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 512-point forward complex FFT of one wave.  In: v[r] = x[lane + 64 r].  Runs Stockham passes
// Ns = 1 and 8 through `buf` (512 float2 of LDS owned by this wave) and the twiddle + butterfly
// of pass Ns = 64; on return v[r] = X[lane + 64 r] (natural order), nothing left in LDS.
// buf is private to the calling wave, so the exchanges only need wave-level ordering.
__device__ __forceinline__ void fft512(float2 (&v)[8], float2 *buf, const Twiddles &t, int lane) {
  // pass Ns = 1: no twiddles; out[8 j + r]
  fft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[8 * lane + r] = v[r];
  wave_lds_sync();
  // pass Ns = 8
  {
    const int k = lane & 7;
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], t.p8[r - 1]);
    fft8(v);
    wave_lds_sync();
    const int j0 = (lane >> 3) * 64 + k;
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[j0 + 8 * r] = v[r];
  }
  wave_lds_sync();
  // pass Ns = 64; out[j + 64 r]
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[lane + 64 * r];
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], t.p64[r - 1]);
  fft8(v);
}

// numpy "reflect" padding index: mirror without repeating the edge sample; one fold for normal
// sizes, a few for signals shorter than the pad
__device__ __forceinline__ int reflect_index(int p, int N) {
  while (p < 0 || p >= N) p = p < 0 ? -p : 2 * (N - 1) - p;
  return p;
}

// the same for |overhang| < N (signals longer than the pad): branch-free
__device__ __forceinline__ int reflect_once(int p, int N) {
  p = p < 0 ? -p : p;
  return p >= N ? 2 * (N - 1) - p : p;
}

// the same for ANY N >= 1 in bounded time (a signal of two samples folds 512 times in the loop above, and one of a single
// sample never leaves it): the index modulo the period 2 (N - 1); every index of a one-sample signal is 0
__device__ __forceinline__ int reflect_fold(int p, int N) {
  if ((unsigned)p < (unsigned)N) return p;
  const int period = 2 * (N - 1);
  if (period == 0) return 0;
  p %= period;
  p = p < 0 ? p + period : p;
  return p >= N ? period - p : p;
}

}  // namespace
}  // namespace xdtts
