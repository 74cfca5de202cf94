// timbre.hip -- voice timbre as a change of the STFT magnitude behind the prosody stage and in front of the initial phase
// (xdtts_timbre, include/xdtts.h): per frame, the log magnitude is split by the cepstral lifter of the prosody stage into its
// smooth envelope (the formants) and its fine structure (the harmonics).
//   vtl   : only the ENVELOPE is resampled on the frequency axis -- the formants move, the harmonics and with them F0 stay
//   breath: the fine structure fades into the log of a Rayleigh noise magnitude under the same envelope; 1 = a whisper
// The reverse of prosody_frame_at (prosody.hip), which warps the fine structure under a fixed envelope: here E goes to LDS for
// the warped read and R stays in the registers that held L.  One wave per row, FRAMES_PER_BLOCK rows per workgroup over the
// concatenated utterances (the shape of k_prosody_batch), the two transforms through cepstrum.h on a private LDS slice.
// Nothing crosses a workgroup: no barrier, no exchange, no polling, no atomics.  One kernel serves the single call (the record
// travels as a kernel argument) and the ragged batch (a table in device memory): a row leaves either with the same bits.
#include "cepstrum.h"
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int NB = NFFT / 2 + 1;  // 513 bins
static_assert(NB == TIMBRE_NB, "the noise index of timbre_plan.h counts 513 bins per frame");

// Row `jr` of Sout over the concatenated utterances.  tab[u] (TimbreUtt, kernels.h; dst0 ascending) says where utterance u lies
// and with which parameters; tab == nullptr: the one utterance of `one`.  Each wave looks its own utterance up (the bounded
// search of k_prosody_batch: the index stays in [0, n_utt) whatever the table holds) and reads no row but its utterance's.
// With j = the frame inside its utterance and s = that row of S:
//   identity (vtl == 1 and breath == 0): the row is copied, no arithmetic
//   L = ln(max(s, log_floor)); c = real cepstrum of L; E = the transform of c with c[n] = 0 for lifter < n < 1024 - lifter
//   p = k vtl;  E'[k] = p <= 512 ? lerp(E, p) : E[512];  R = L - E
//   breath != 0: R <- (1 - breath) R + breath N(seed, j, k)     (timbre_plan.h; not evaluated otherwise)
//   out[k] = exp(E'[k] + R[k])
// A wave past the last row computes the last row again and leaves before the stores, so every wave_lds_sync is wave-uniform.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_timbre(const float *__restrict__ S, float *__restrict__ Sout,
                                                                  const TimbreUtt *__restrict__ tab, int n_utt, TimbreUtt one,
                                                                  int rows_all, const float2 *__restrict__ tw) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (the same in every lane: scalar)
  const int jr = blockIdx.x * FRAMES_PER_BLOCK + wave;
  const bool ok = jr < rows_all;
  const int row = ok ? jr : rows_all - 1;
  TimbreUtt t = one;
  if (tab) {
    int lo = 0, hi = n_utt - 1;  // the last utterance with dst0 <= row
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = (lo + hi + 1) >> 1;  // lo < mid <= hi
      if (tab[mid].dst0 <= row) lo = mid; else hi = mid - 1;
    }
    t = tab[lo];
  }
  const int j = min(max(row - t.dst0, 0), max(t.F, 1) - 1);
  const float *s = S + ((size_t)t.src0 + (size_t)j) * NB;
  float *out = Sout + ((size_t)t.dst0 + (size_t)j) * NB;
  float L[9];  // bins lane + 64 r, and bin 512
#pragma unroll
  for (int r = 0; r <= 8; ++r) L[r] = s[r < 8 ? lane + 64 * r : 512];
  if (t.vtl == 1.0f && t.breath == 0.0f) {
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < 8; ++r) out[lane + 64 * r] = L[r];
    if (lane == 0) out[512] = L[8];
    return;
  }
  float2 *buf = lds[wave];
  const Twiddles tws = load_twiddles(tw, lane);
  float *e = reinterpret_cast<float *>(buf);
  float X[9];
  log_cepstrum(L, t.log_floor, tw, tws, buf, lane, X);  // (cepstrum.h: shared with the prosody stage and the pitch tracker)
  // liftered cepstrum -> envelope
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = lane + 64 * r <= t.lifter ? X[r] * (1.0f / NFFT) : 0.f;
  if (lane == 0) e[512] = 0.f;  // (lifter <= 255)
  wave_lds_sync();
  even_dft(buf, tw, tws, lane, X);  // X = E
  wave_lds_sync();
  // fine structure in the registers that held L; the envelope to LDS, read warped
#pragma unroll
  for (int r = 0; r <= 8; ++r) L[r] -= X[r];
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = X[r];
  if (lane == 0) e[512] = X[8];
  wave_lds_sync();
  if (!ok) return;
  const bool noisy = t.breath != 0.0f;  // (wave-uniform)
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    if (r == 8 && lane != 0) break;
    const int k = r < 8 ? lane + 64 * r : 512;
    const float p = (float)k * t.vtl;
    float Ew = e[512];
    if (p <= 512.0f) {
      const float fl = floorf(p);
      const int q = (int)fl;  // 0 .. 512
      const float a = p - fl;
      Ew = (1.0f - a) * e[q] + a * e[min(q + 1, 512)];
    }
    float R = L[r];
    if (noisy) {
      const float N = timbre_noise(timbre_noise_v(timbre_noise_bits(t.seed, (uint32_t)j, (uint32_t)k)));
      R = (1.0f - t.breath) * R + t.breath * N;
    }
    out[k] = expf(Ew + R);
  }
}

}  // namespace

void launch_timbre(const float *S, float *Sout, const TimbreUtt *tab, int n_utt, const TimbreUtt &one, int rows_all, const float2 *tw,
                   hipStream_t s) {
  if (n_utt <= 0 || rows_all <= 0) return;
  const int nblk = (rows_all + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  hipLaunchKernelGGL(k_timbre, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, Sout, tab, n_utt, one, rows_all, tw);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
