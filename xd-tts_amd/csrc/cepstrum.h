// cepstrum.h -- the log -> real cepstrum half of a prosody frame (prosody.hip: prosody_frame_at) as device functions of one
// wave, shared with the pitch tracker (f0.hip: k_f0_frames), so that both form a frame's cepstrum with the same arithmetic.
#pragma once
#include "gl_fft.h"

namespace xdtts {
namespace {

// DFT (1024 points) of the real EVEN sequence x[m] = e[min(m, 1024 - m)], e = the 513 floats at the start of the wave's LDS
// slice: real and even again, so the forward transform serves for both directions (the inverse differs by 1 / 1024).
// Packed as z[m] = x[2m] + i x[2m + 1], one fft512, Hermitian split with the handle's table tw[k] = e^{-2 pi i k / 1024}, real
// part kept: on return X[r] = the value of bin lane + 64 r (r < 8) and X[8] = bin 512 (the same in every lane).  The slice
// holds the transform's packed spectrum afterwards; the caller orders its next stores behind with wave_lds_sync().
__device__ __forceinline__ void even_dft(float2 *buf, const float2 *__restrict__ tw, const Twiddles &tws, int lane, float (&X)[9]) {
  const float *e = reinterpret_cast<const float *>(buf);
  float2 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int m = 2 * (lane + 64 * r);                      // 0 .. 1022, even
    v[r] = make_float2(e[min(m, NFFT - m)], e[min(m + 1, NFFT - 1 - m)]);  // indices 0 .. 512
  }
  wave_lds_sync();
  fft512(v, buf, tws, lane);
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[lane + 64 * r] = v[r];
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    const int k = r < 8 ? lane + 64 * r : 512;
    const float2 zk = buf[k & 511], zc = buf[(512 - k) & 511];
    const float2 od = make_float2(0.5f * (zk.y + zc.y), 0.5f * (zc.x - zk.x));  // (Z[k] - conj Z[512-k]) / (2i)
    const float2 twk = k == 512 ? make_float2(-1.f, 0.f) : tw[k];
    X[r] = 0.5f * (zk.x + zc.x) + fmaf(twk.x, od.x, -twk.y * od.y);  // Re((Z[k] + conj Z[512-k]) / 2 + tw[k] od)
  }
}

// The frame's magnitude in L (bins lane + 64 r, and bin 512) -> L = ln(max(., log_floor)) and X = 1024 x the real cepstrum of L
// (quefrencies lane + 64 r, and 512): the caller scales by 1 / NFFT where it keeps a value.  The slice is the wave's own.
__device__ __forceinline__ void log_cepstrum(float (&L)[9], float log_floor, const float2 *__restrict__ tw, const Twiddles &tws, float2 *buf,
                                             int lane, float (&X)[9]) {
  float *e = reinterpret_cast<float *>(buf);
#pragma unroll
  for (int r = 0; r <= 8; ++r) L[r] = logf(fmaxf(L[r], log_floor));
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = L[r];
  if (lane == 0) e[512] = L[8];
  wave_lds_sync();
  even_dft(buf, tw, tws, lane, X);
  wave_lds_sync();
}

}  // namespace
}  // namespace xdtts
