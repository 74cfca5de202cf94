// prosody.hip -- speaking rate and pitch as a change of the STFT magnitude between mel -> linear and the Griffin-Lim loop
// (Griffin & Lim's algorithm estimates a signal from a MODIFIED magnitude; the loop then finds a phase for it).
//   rate : the frames are resampled on the time axis, linear interpolation between the two neighbouring frames
//   pitch: per frame, the log magnitude is split by a cepstral lifter into its smooth envelope (the formants) and its fine
//          structure (the harmonics); only the fine structure is resampled on the frequency axis, the envelope stays where it is.
// One wave per OUTPUT frame, four frames per workgroup (the shape of k_stft_mag, analysis.hip); the two transforms are the
// one-wave 512-point FFT of gl_fft.h on a private LDS slice.  Nothing here crosses workgroups: no barrier, no exchange, no
// polling, no atomics.  k_prosody takes one utterance, k_prosody_batch the concatenated utterances of a batch, each with its own
// parameters; both run prosody_frame().  k_prosody_contour takes utterances whose rate, pitch and gain vary from frame to frame
// (a host-built table, prosody_contour.h); all three share prosody_frame_at().
#include "cepstrum.h"
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int NB = NFFT / 2 + 1;  // 513 bins

// One output frame from its two neighbouring input rows -- the arithmetic of all three kernels, so that a frame leaves any of
// them with the same bits.  out[k] from s0 = S[i], s1 = S[i + 1] (s1 == s0 where the row i + 1 must not be read) and w:
//   St[k] = (1 - w) s0[k] + w s1[k]
//   pitch == 1: out = St (an exact zero stays one)
//   else      : L = ln(max(St, log_floor)); c = real cepstrum of L; E = the transform of c with c[n] = 0 for lifter < n <
//               1024 - lifter; R = L - E; p = k / pitch; out[k] = exp(E[k] + (p <= 512 ? lerp(R, p) : 0))
//   GAIN      : out is multiplied by `gain` in either branch (the contour kernel; the uniform kernels carry no multiply)
// A wave with !ok computes the frame and leaves before the stores.  buf = the wave's private LDS slice.
template <bool GAIN>
__device__ __forceinline__ void prosody_frame_at(const float *__restrict__ s0, const float *__restrict__ s1, float *__restrict__ out, float w,
                                                 bool ok, float pitch, float gain, int lifter, float log_floor,
                                                 const float2 *__restrict__ tw, float2 *buf, int lane) {
  float L[9];  // bins lane + 64 r, and bin 512
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    const int k = r < 8 ? lane + 64 * r : 512;
    L[r] = (1.0f - w) * s0[k] + w * s1[k];
  }
  if (pitch == 1.0f) {
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < 8; ++r) out[lane + 64 * r] = GAIN ? gain * L[r] : L[r];
    if (lane == 0) out[512] = GAIN ? gain * L[8] : L[8];
    return;
  }
  const Twiddles tws = load_twiddles(tw, lane);
  float *e = reinterpret_cast<float *>(buf);
  float X[9];
  log_cepstrum(L, log_floor, tw, tws, buf, lane, X);  // (cepstrum.h: shared with the pitch tracker)
  // liftered cepstrum -> envelope
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = lane + 64 * r <= lifter ? X[r] * (1.0f / NFFT) : 0.f;
  if (lane == 0) e[512] = 0.f;  // (lifter <= 255)
  wave_lds_sync();
  even_dft(buf, tw, tws, lane, X);  // X = E
  wave_lds_sync();
  // fine structure, warped
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = L[r] - X[r];
  if (lane == 0) e[512] = L[8] - X[8];
  wave_lds_sync();
  if (!ok) return;
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    if (r == 8 && lane != 0) break;
    const int k = r < 8 ? lane + 64 * r : 512;
    const float p = (float)k / pitch;
    float Rw = 0.f;
    if (p <= 512.0f) {
      const float fl = floorf(p);
      const int q = (int)fl;  // 0 .. 512
      const float a = p - fl;
      Rw = (1.0f - a) * e[q] + a * e[min(q + 1, 512)];
    }
    const float y = expf(X[r] + Rw);
    out[k] = GAIN ? gain * y : y;
  }
}

// One output frame of one utterance under a uniform prosody: finds (i, w), then prosody_frame_at().
// Sout[j][k], j < Fout, from S [F][513] (F >= 2 unless rate == 1):  u = min(j rate, F - 1), i = min(floor u, F - 2), w = u - i.
// j is the wave's frame (already clamped into the utterance).
__device__ __forceinline__ void prosody_frame(const float *__restrict__ S, float *__restrict__ Sout, int F, int j, bool ok, float rate,
                                              float pitch, int lifter, float log_floor, const float2 *__restrict__ tw, float2 *buf,
                                              int lane) {
  int i = 0;
  float w = 0.f;
  if (rate != 1.0f) {
    const float u = fminf((float)j * rate, (float)(F - 1));
    i = min((int)floorf(u), F - 2);
    w = u - (float)i;
  } else {
    i = j;  // (F == Fout; the row i + 1 is not read: F may be 1)
  }
  const float *s0 = S + (size_t)i * NB, *s1 = rate != 1.0f ? s0 + NB : s0;
  prosody_frame_at<false>(s0, s1, Sout + (size_t)j * NB, w, ok, pitch, 1.0f, lifter, log_floor, tw, buf, lane);
}

// One utterance: a wave past the last frame computes the last frame again (clamped index) and leaves before the stores.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_prosody(const float *__restrict__ S, float *__restrict__ Sout, int F,
                                                                   int Fout, float rate, float pitch, int lifter, float log_floor,
                                                                   const float2 *__restrict__ tw) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jr = blockIdx.x * FRAMES_PER_BLOCK + wave;
  const bool ok = jr < Fout;
  prosody_frame(S, Sout, F, ok ? jr : Fout - 1, ok, rate, pitch, lifter, log_floor, tw, lds[wave], lane);
}

// The ragged form: the utterances of a batch lie one behind the other in S [sum F_u][513] and Sout [sum F'_u][513]; tab[u]
// (ProsodyUtt, kernels.h) says where, and with which parameters.  One wave per row of Sout, FRAMES_PER_BLOCK rows per
// workgroup over the concatenated axis, so the waves of a workgroup may belong to different utterances: each looks its own
// up (a bounded search over dst0, ascending; the index stays in [0, n_utt) whatever the table holds), takes its own branch
// and reads no row but its utterance's.  rate == pitch == 1: the row is copied, no arithmetic.  A wave past the last row
// of the batch computes the last row again and leaves before the stores.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_prosody_batch(const float *__restrict__ S, float *__restrict__ Sout,
                                                                         const ProsodyUtt *__restrict__ tab, int n_utt, int Fout_all,
                                                                         const float2 *__restrict__ tw) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (the same in every lane: scalar)
  const int jr = blockIdx.x * FRAMES_PER_BLOCK + wave;
  const bool ok = jr < Fout_all;
  const int row = ok ? jr : Fout_all - 1;
  int lo = 0, hi = n_utt - 1;  // the last utterance with dst0 <= row
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;  // lo < mid <= hi
    if (tab[mid].dst0 <= row) lo = mid; else hi = mid - 1;
  }
  const ProsodyUtt t = tab[lo];
  const int j = min(max(row - t.dst0, 0), t.Fout - 1);
  const float *Su = S + (size_t)t.src0 * NB;
  float *So = Sout + (size_t)t.dst0 * NB;
  if (t.rate == 1.0f && t.pitch == 1.0f) {
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < 8; ++r) So[(size_t)j * NB + lane + 64 * r] = Su[(size_t)j * NB + lane + 64 * r];
    if (lane == 0) So[(size_t)j * NB + 512] = Su[(size_t)j * NB + 512];
    return;
  }
  prosody_frame(Su, So, t.F, j, ok, t.rate, t.pitch, t.lifter, t.log_floor, tw, lds[wave], lane);
}

// The contour form (xdtts_prosody_contour): rate, pitch and gain vary inside an utterance.  The shape of k_prosody_batch -- one
// wave per row of Sout over the concatenated axis, each wave looks up its utterance in utt[] (dst0 ascending) -- and then a
// second bounded search, over that utterance's cumulative slowness c[0 .. F - 1] (ftab + tab0, ascending, 2^-16 output frames):
//   t = min(j 2^16, c[F - 1]);  i = the last interval with c[i] <= t, in [0, F - 2] whatever the table holds, so that the rows
//   i and i + 1 are the utterance's own;  w = (t - c[i]) / (c[i + 1] - c[i]): integers below 2^24, exact in fp32
//   pitch = fmaf(w, p[i + 1] - p[i], p[i]), gain likewise: exactly 1 wherever both neighbours are 1 (the copy branch)
// Both searches run on wave-uniform values (scalar loads).  ftab holds c, then the pitches, then the gains of all utterances,
// n_tab entries each.  An identity utterance is copied.  A wave past the last row computes the last row again and leaves
// before the stores.  Single call: n_utt = 1.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_prosody_contour(const float *__restrict__ S, float *__restrict__ Sout,
                                                                           const ContourUtt *__restrict__ utt, int n_utt,
                                                                           const unsigned *__restrict__ ftab, int n_tab, int Fout_all,
                                                                           const float2 *__restrict__ tw) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int jr = blockIdx.x * FRAMES_PER_BLOCK + wave;
  const bool ok = jr < Fout_all;
  const int row = ok ? jr : Fout_all - 1;
  int lo = 0, hi = n_utt - 1;  // the last utterance with dst0 <= row
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (utt[mid].dst0 <= row) lo = mid; else hi = mid - 1;
  }
  const ContourUtt t = utt[lo];
  const int j = min(max(row - t.dst0, 0), t.Fout - 1);
  const float *Su = S + (size_t)t.src0 * NB;
  float *So = Sout + ((size_t)t.dst0 + (size_t)j) * NB;
  if (t.identity) {
    if (!ok) return;
#pragma unroll
    for (int r = 0; r < 8; ++r) So[lane + 64 * r] = Su[(size_t)j * NB + lane + 64 * r];
    if (lane == 0) So[512] = Su[(size_t)j * NB + 512];
    return;
  }
  if (t.F < 2) return;  // (never: the host's argument rules)
  const unsigned *c = ftab + t.tab0;
  const float *pt = reinterpret_cast<const float *>(ftab + n_tab + t.tab0), *gn = reinterpret_cast<const float *>(ftab + 2 * (size_t)n_tab + t.tab0);
  const unsigned tt = min((unsigned)j << 16, c[t.F - 1]);
  int i = 0, ihi = t.F - 2;  // the last interval with c[i] <= tt
  for (int it = 0; it < 15 && i < ihi; ++it) {
    const int mid = (i + ihi + 1) >> 1;  // i < mid <= ihi <= F - 2
    if (c[mid] <= tt) i = mid; else ihi = mid - 1;
  }
  const unsigned c0 = c[i];
  const float w = (float)(tt - c0) / (float)(c[i + 1] - c0);
  const float p0 = pt[i], g0 = gn[i];
  const float pj = fmaf(w, pt[i + 1] - p0, p0), gj = fmaf(w, gn[i + 1] - g0, g0);
  const float *s0 = Su + (size_t)i * NB;
  prosody_frame_at<true>(s0, s0 + NB, So, w, ok, pj, gj, t.lifter, t.log_floor, tw, lds[wave], lane);
}

}  // namespace

void launch_prosody(const float *S, float *Sout, int F, int Fout, float rate, float pitch, int lifter, float log_floor,
                    const float2 *tw, hipStream_t s) {
  const int nblk = (Fout + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  hipLaunchKernelGGL(k_prosody, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, Sout, F, Fout, rate, pitch, lifter, log_floor, tw);
  HIP_CHECK(hipGetLastError());
}

void launch_prosody_batch(const float *S, float *Sout, const ProsodyUtt *tab, int n_utt, int Fout_all, const float2 *tw, hipStream_t s) {
  if (n_utt <= 0 || Fout_all <= 0) return;
  const int nblk = (Fout_all + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  hipLaunchKernelGGL(k_prosody_batch, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, Sout, tab, n_utt, Fout_all, tw);
  HIP_CHECK(hipGetLastError());
}

void launch_prosody_contour(const float *S, float *Sout, const ContourUtt *utt, int n_utt, const unsigned *ftab, int n_tab, int Fout_all,
                            const float2 *tw, hipStream_t s) {
  if (n_utt <= 0 || Fout_all <= 0) return;
  const int nblk = (Fout_all + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  hipLaunchKernelGGL(k_prosody_contour, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, Sout, utt, n_utt, ftab, n_tab, Fout_all, tw);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
