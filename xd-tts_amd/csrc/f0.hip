// f0.hip -- the pitch tracker on the magnitude that mel -> linear leaves (xdtts_f0_opts, xdtts_pitch_target; the definition:
// include/xdtts.h), in two kernels ordered by the stream alone:
//   k_f0_frames  one wave per frame over the concatenated rows of a call, four frames per workgroup (the shape of k_prosody):
//                the frame's real cepstrum by log_cepstrum() (cepstrum.h: the arithmetic of the prosody stage), the largest
//                value in the quefrency range by a wave max-reduction, the lowest qualifying local maximum by a wave
//                min-reduction over each lane's lowest candidate, the parabolic offset -> raw[t], strength[t].  A frame needs
//                nothing of its neighbours, so the ragged form is the single form.  No workgroup barrier, no atomics, no polling.
//   k_f0_track   one workgroup per utterance (F <= 16384, its values in 64 KiB of LDS): the running median of five, the
//                utterance's median by a radix select on the bit patterns of the positive floats (integer LDS counters: the
//                result does not depend on the order of the additions), min / max, the ratios of a pitch target, and their
//                product with the pitch slice of a contour table (prosody.hip: k_prosody_contour reads it next).  Comparisons
//                and selections only; no floating-point sum anywhere, so every output is the same on every run, and in a batch
//                the same as alone.  The per-value arithmetic is f0_plan.h's, shared with the host reference.
#include <climits>

#include "cepstrum.h"
#include "device_utils.h"
#include "f0_plan.h"
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int NB = NFFT / 2 + 1;  // 513 bins
constexpr int TRACK_WG = 1024;
constexpr int TRACK_ROUNDS = (int)F0_MAX_FRAMES / TRACK_WG;  // values of a lane

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_move_i(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_min_i(int v) {  // (the sequence of wave_max, device_utils.h)
  v = min(v, dpp_move_i<0xB1, 0xf>(v));
  v = min(v, dpp_move_i<0x4E, 0xf>(v));
  v = min(v, dpp_move_i<0x124, 0xf>(v));
  v = min(v, dpp_move_i<0x128, 0xf>(v));
  v = min(v, dpp_move_i<0x142, 0xa>(v));
  v = min(v, dpp_move_i<0x143, 0xc>(v));
  return __builtin_amdgcn_readlane(v, 63);
}

// raw[t], strength[t] of every row t < rows of S [rows][513].  1 <= q_lo < q_hi <= 510 (the host's rules give 22 .. 441): the
// neighbours n - 1 and n + 1 of a candidate lie inside the 513 cepstrum values of the slice.  A wave past the last row computes
// the last row again and leaves before its stores.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_f0_frames(const float *__restrict__ S, int rows, float log_floor, float octave_bias,
                                                                     int q_lo, int q_hi, const float2 *__restrict__ tw,
                                                                     float *__restrict__ raw, float *__restrict__ strength) {
  __shared__ float2 lds[FRAMES_PER_BLOCK][512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jr = blockIdx.x * FRAMES_PER_BLOCK + wave;
  const bool ok = jr < rows;
  const int row = ok ? jr : rows - 1;
  const float *s = S + (size_t)row * NB;
  float2 *buf = lds[wave];
  float *e = reinterpret_cast<float *>(buf);
  q_lo = max(q_lo, 1);
  q_hi = min(q_hi, 510);
  float L[9], X[9];
#pragma unroll
  for (int r = 0; r <= 8; ++r) L[r] = s[r < 8 ? lane + 64 * r : 512];
  const Twiddles tws = load_twiddles(tw, lane);
  log_cepstrum(L, log_floor, tw, tws, buf, lane, X);
#pragma unroll
  for (int r = 0; r <= 8; ++r) X[r] *= 1.0f / NFFT;  // c[lane + 64 r], c[512]
#pragma unroll
  for (int r = 0; r < 8; ++r) e[lane + 64 * r] = X[r];
  if (lane == 0) e[512] = X[8];
  wave_lds_sync();
  float top = -INFINITY;  // (NaN compares false)
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = lane + 64 * r;
    if (n >= q_lo && n <= q_hi && X[r] > top) top = X[r];
  }
  top = wave_max(top);
  const float thr = octave_bias * top;
  int first_peak = INT_MAX, first_top = INT_MAX;  // the lane's lowest qualifying n; its lowest n with c[n] == top
#pragma unroll
  for (int r = 7; r >= 0; --r) {
    const int n = lane + 64 * r;
    if (n < q_lo || n > q_hi) continue;
    const float v = X[r];
    if (v == top) first_top = n;
    if (v >= thr && v >= e[n - 1] && v >= e[n + 1]) first_peak = n;
  }
  first_peak = wave_min_i(first_peak);
  first_top = wave_min_i(first_top);
  const int ns = top > 0.0f && first_peak != INT_MAX ? first_peak : (first_top != INT_MAX ? first_top : q_lo);
  if (!ok || lane != 0) return;
  const float a = e[ns - 1], b = e[ns], c = e[ns + 1];
  const float d = (a - b) + (c - b);
  float p = d == 0.0f ? 0.0f : 0.5f * (a - c) / d;
  p = fminf(fmaxf(p, -0.5f), 0.5f);
  raw[row] = 22050.0f / ((float)ns + p);
  strength[row] = b;
}

// The utterance stage of utterance blockIdx.x: rows row0 .. row0 + F of raw / strength -> f0, ratio (the same rows), stats[u],
// and, with tab0 >= 0, the pitch slice of the contour table: ftab[n_tab + tab0 + t] = clamp(ftab[3 n_tab + tab0 + t] * ratio[t])
// -- the caller's pitches stay behind the three arrays k_prosody_contour reads, so a second run writes the same bits.
__global__ __launch_bounds__(TRACK_WG) void k_f0_track(const float *__restrict__ raw, const float *__restrict__ strength,
                                                       const F0Utt *__restrict__ utts, float threshold, float *__restrict__ f0_out,
                                                       float *__restrict__ ratio_out, F0Stats *__restrict__ stats, unsigned *ftab, int n_tab) {
  __shared__ uint32_t v[F0_MAX_FRAMES];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[8];  // n_voiced, min, max, n_clamped, the select's prefix, its remaining rank
  const F0Utt u = utts[blockIdx.x];
  const int F = min(u.F, (int)F0_MAX_FRAMES), tid = threadIdx.x;
  if (F <= 0) return;
  const size_t row0 = (size_t)u.row0;
  for (int t = tid; t < F; t += TRACK_WG) v[t] = f0_is_voiced(strength[row0 + t], threshold) ? f0_bits(raw[row0 + t]) : 0u;
  if (tid < 256) hist[tid] = 0u;
  if (tid < 8) sh[tid] = tid == 1 ? 0xffffffffu : 0u;
  __syncthreads();
  // the running median of five, then the values' counts and extremes
  uint32_t med[TRACK_ROUNDS];
#pragma unroll
  for (int i = 0; i < TRACK_ROUNDS; ++i) {
    const int t = tid + TRACK_WG * i;
    med[i] = 0u;
    if (t < F && v[t]) {
      uint32_t w[2 * F0_MEDIAN_HALF + 1];
      const int a = max(t - F0_MEDIAN_HALF, 0), b = min(t + F0_MEDIAN_HALF, F - 1);
#pragma unroll
      for (int j = 0; j < 2 * F0_MEDIAN_HALF + 1; ++j) w[j] = a + j <= b ? v[a + j] : 0u;
      med[i] = f0_median5(w, 2 * F0_MEDIAN_HALF + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TRACK_ROUNDS; ++i) {
    const int t = tid + TRACK_WG * i;
    if (t >= F) continue;
    v[t] = med[i];
    f0_out[row0 + t] = f0_float(med[i]);
    if (med[i]) {
      atomicAdd(&sh[0], 1u);
      atomicMin(&sh[1], med[i]);
      atomicMax(&sh[2], med[i]);
    }
  }
  __syncthreads();
  const int n_voiced = (int)sh[0];
  // the lower median of the voiced values: radix select, eight bits a pass from the top
  uint32_t prefix = 0u;
  if (n_voiced > 0) {  // (the same in every lane of the workgroup)
    uint32_t k = (uint32_t)(n_voiced - 1) / 2u;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t fixed = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
      for (int t = tid; t < F; t += TRACK_WG) {
        const uint32_t x = v[t];
        if (x && (x & fixed) == prefix) atomicAdd(&hist[(x >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid < 64) {  // the first wave: four bins a lane, an inclusive scan over the lanes, and the lane that holds rank k
        uint32_t c[4], incl = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c[j] = hist[4 * tid + j];
          incl += c[j];
        }
        const uint32_t own = incl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
          if (tid >= d) incl += o;
        }
        uint32_t before = incl - own;
        if (before <= k && k < incl) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (k >= before && k < before + c[j]) {
              sh[4] = prefix | ((uint32_t)(4 * tid + j) << shift);
              sh[5] = k - before;
            }
            before += c[j];
          }
        }
      }
      __syncthreads();
      prefix = sh[4];
      k = sh[5];
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
    }
  }
  const float median = f0_float(prefix);
  PitchTarget tg;
  tg.mode = u.mode;
  tg.value = u.value;
  tg.range = u.range;
  const F0Base bs = f0_base(tg, n_voiced, median);
  const bool tab = ftab && u.tab0 >= 0;
  const float *pitch0 = tab ? reinterpret_cast<const float *>(ftab + 3 * (size_t)n_tab + (size_t)u.tab0) : nullptr;
  float *pitch = tab ? reinterpret_cast<float *>(ftab + (size_t)n_tab + (size_t)u.tab0) : nullptr;
  for (int t = tid; t < F; t += TRACK_WG) {
    const float r = f0_ratio_raw(bs, f0_float(v[t])), rc = f0_clamp(r);
    if (f0_bits(rc) != f0_bits(r)) atomicAdd(&sh[3], 1u);
    ratio_out[row0 + t] = rc;
    if (tab) pitch[t] = f0_table_pitch(pitch0[t], rc);
  }
  __syncthreads();
  if (tid == 0) {
    F0Stats s;
    s.n_frames = F;
    s.n_voiced = n_voiced;
    s.n_clamped = (int)sh[3];
    s.median_hz = median;
    s.min_hz = n_voiced > 0 ? f0_float(sh[1]) : 0.0f;
    s.max_hz = n_voiced > 0 ? f0_float(sh[2]) : 0.0f;
    s.base_ratio = bs.base;
    stats[blockIdx.x] = s;
  }
}

}  // namespace

void launch_f0_frames(const float *S, int rows, const F0Opts &o, int q_lo, int q_hi, const float2 *tw, float *raw, float *strength,
                      hipStream_t s) {
  if (rows <= 0) return;
  const int nblk = (rows + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK;
  hipLaunchKernelGGL(k_f0_frames, dim3(nblk), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, rows, o.log_floor, o.octave_bias, q_lo, q_hi, tw, raw, strength);
  HIP_CHECK(hipGetLastError());
}

void launch_f0_track(const float *raw, const float *strength, const F0Utt *utts_dev, int n_utt, float threshold, float *f0, float *ratio,
                     F0Stats *stats, unsigned *ftab, int n_tab, hipStream_t s) {
  if (n_utt <= 0) return;
  hipLaunchKernelGGL(k_f0_track, dim3(n_utt), dim3(TRACK_WG), 0, s, raw, strength, utts_dev, threshold, f0, ratio, stats, ftab, n_tab);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
