// analysis.hip -- the inverse direction of GriffinLim::infer's conventions as HIP kernels for gfx950: audio -> STFT magnitude
// (librosa.stft(y, 1024, hop 256, periodic hann, center, reflect)) -> mel basis -> compression, and the spectral convergence
// || a |STFT(y)| - S || / || S || of an audio against a target magnitude.
//
// The transform is the one of the iteration kernels (gl_fft.h: one wave per frame, 512-point complex Stockham FFT of the packed
// real frame, Hermitian split), but it reads the audio itself instead of the overlap-added frame buffer and stores magnitudes
// instead of updating a phase -- a separate entry that leaves the iteration kernels as they are.  Nothing here crosses
// workgroups inside a launch: no exchange, no polling, no atomics; the reduction is two launches in a fixed order.
#include <algorithm>

#include "gl_fft.h"
#include "kernels.h"

namespace xdtts {

namespace {

// Magnitude of frame f0 + wave of the workgroup's utterance (segs[blockIdx.x]):
//   S[row][k] = |X[k]|, k < 513;  P[row][k] = |X[k]|^e with row stride ldp and the padding columns 513 .. ldp-1 zero (the
//   A operand of the mel GEMM; P == null: not wanted).
// The exchange buffer is private to the wave, so the kernel has no workgroup barrier at all; a wave past the utterance's last
// frame computes the last frame again (clamped index) and leaves before the stores.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_stft_mag(const float *__restrict__ audio, const AnSeg *__restrict__ segs,
                                                                    const float2 *__restrict__ tw, const float *__restrict__ win_,
                                                                    float *__restrict__ S, float *__restrict__ P, int ldp, float e) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const AnSeg sg = segs[blockIdx.x];
  const int fr = sg.f0 + wave;
  const bool ok = fr < sg.F;
  const int f = ok ? fr : sg.F - 1;
  const float *y = audio + sg.abase;
  const float2 *win = reinterpret_cast<const float2 *>(win_);
  const Twiddles tws = load_twiddles(tw, lane);
  float2 v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int m = lane + 64 * r;
    const int base = f * HOP + 2 * m - NFFT / 2;
    const int p0 = reflect_fold(base, sg.n), p1 = reflect_fold(base + 1, sg.n);  // both in [0, n)
    const float2 w = win[m];
    v[r] = make_float2(y[p0] * w.x, y[p1] * w.y);
  }
  float2 *buf = lds[wave];
  fft512(v, buf, tws, lane);
  wave_lds_sync();
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[lane + 64 * r] = v[r];
  wave_lds_sync();
  if (!ok) return;
  const size_t row = (size_t)sg.row0 + (size_t)f;
  float *Sr = S + row * (NFFT / 2 + 1);
  float *Pr = P ? P + row * (size_t)ldp : nullptr;
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    const int k = lane + 64 * r;
    if (r == 8 && lane != 0) {
      if (Pr && k < ldp) Pr[k] = 0.f;  // padding columns
      break;
    }
    const float2 zk = buf[k & 511], zc = buf[(512 - k) & 511];
    const float2 ev = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));  // (Z[k] + conj Z[512-k]) / 2
    const float2 od = make_float2(0.5f * (zk.y + zc.y), 0.5f * (zc.x - zk.x));  // (Z[k] - conj Z[512-k]) / (2i)
    const float2 twk = k == 512 ? make_float2(-1.f, 0.f) : tw[k];
    const float2 x = cadd(ev, cmul(twk, od));
    const float mag = sqrtf(fmaf(x.x, x.x, x.y * x.y));
    Sr[k] = mag;
    if (Pr) Pr[k] = e == 1.0f ? mag : powf(mag, e);
  }
}

// melT [F][n_mels] -> the boundary layout (n_mels x F), compressed with the inverse of k_exp_transpose's modes:
// 0: ln(max(m, floor)), 1: m, 2: log10(max(m, floor))
__global__ void k_mel_compress(const float *__restrict__ melT, float *__restrict__ out, int n_mels, int F, int mode, float floor) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_mels * F) return;
  const int m = i / F, f = i % F;
  const float v = melT[(size_t)f * n_mels + m];
  out[i] = mode == 0 ? logf(fmaxf(v, floor)) : (mode == 2 ? log10f(fmaxf(v, floor)) : v);
}

// The three sums of the spectral convergence over n cells, x = analysed magnitude, s = target: workgroup b adds its fixed strided
// share in fp64 (lane-strided accumulation, xor-shuffle tree, the four waves in order) into parts[b][0..2] = sum x s, sum x x,
// sum s s.  Which cells a thread takes depends on n alone, so the same input gives the same bits on every call.
__global__ __launch_bounds__(256) void k_spec_distance(const float *__restrict__ X, const float *__restrict__ St, size_t n,
                                                       double *__restrict__ parts) {
  double xs = 0.0, xx = 0.0, ss = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double x = X[i], s = St[i];
    xs = fma(x, s, xs);
    xx = fma(x, x, xx);
    ss = fma(s, s, ss);
  }
  for (int o = 32; o > 0; o >>= 1) {
    xs += __shfl_xor(xs, o, 64);
    xx += __shfl_xor(xx, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  __shared__ double w[4][3];
  if ((threadIdx.x & 63) == 0) {
    w[threadIdx.x >> 6][0] = xs;
    w[threadIdx.x >> 6][1] = xx;
    w[threadIdx.x >> 6][2] = ss;
  }
  __syncthreads();
  if (threadIdx.x < 3) parts[blockIdx.x * 3 + threadIdx.x] = ((w[0][threadIdx.x] + w[1][threadIdx.x]) + w[2][threadIdx.x]) + w[3][threadIdx.x];
}
// ... and the partials added in index order, one thread per sum (one workgroup)
__global__ void k_spec_distance_sum(const double *__restrict__ parts, int nparts, double *__restrict__ sums) {
  if (threadIdx.x >= 3) return;
  double a = 0.0;
  for (int b = 0; b < nparts; ++b) a += parts[b * 3 + threadIdx.x];
  sums[threadIdx.x] = a;
}

}  // namespace

void launch_stft_mag(const float *audio, const AnSeg *segs_dev, int nblk, const float2 *tw, const float *win, float *S, float *P,
                     int ldp, float e, hipStream_t s) {
  hipLaunchKernelGGL(k_stft_mag, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, audio, segs_dev, tw, win, S, P, ldp, e);
  HIP_CHECK(hipGetLastError());
}

void launch_mel_compress(const float *melT, float *out_melsxF, int n_mels, int F, int mode, float floor, hipStream_t s) {
  const int n = n_mels * F;
  hipLaunchKernelGGL(k_mel_compress, dim3((n + 255) / 256), dim3(256), 0, s, melT, out_melsxF, n_mels, F, mode, floor);
  HIP_CHECK(hipGetLastError());
}

void launch_spec_distance(const float *X, const float *St, size_t n, double *parts, double *sums, hipStream_t s) {
  const int nparts = (int)std::min<size_t>(SPD_PARTS, (n + 255) / 256);
  hipLaunchKernelGGL(k_spec_distance, dim3(nparts), dim3(256), 0, s, X, St, n, parts);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_spec_distance_sum, dim3(1), dim3(64), 0, s, parts, nparts, sums);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
