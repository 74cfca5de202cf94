// phase_spsi.hip -- Single Pass Spectrogram Inversion (Beauregard, Harish, Wyse 2015) as the loop's initial phase
// (phase_init mode 1; the definition is above xdtts_griffinlim_set_phase_init in include/xdtts.h and in DESIGN.md 4.8).
//
// Frame t is a map on the 513 phases of the frame before it:  phi_t[j] = phi_{t-1}[o_t(j)] + d_t(j)  (uint32, 2^-32 turn,
// modulo 2^32).  Maps compose associatively -- (O, D) then (o, d) = (O[o[j]], D[o[j]] + d[j]) -- and integer sums are exact in
// any order, so the recurrence over F frames is cut into segments of SPSI_L frames and runs as four launches ordered by the
// stream alone:
//   k_spsi_maps     one wave per frame, every frame at once: peaks, their offsets, the owner of every bin, d   -> map [F][513]
//   k_spsi_compose  one workgroup per segment: the composite of its frames, SPSI_L dependent gathers in LDS    -> comp [nseg][513]
//   k_spsi_carry    one workgroup per utterance: walks its composites, carry <- carry[O] + D                   -> entry [nseg][513]
//   k_spsi_apply    one workgroup per segment: from its entry phase through its frames                          -> ang, tprev (, turns)
// The dependent depth is 2 SPSI_L + F / SPSI_L gathers instead of F.  No workgroup waits for another inside a launch: no
// granules, no polling, no atomics, no co-residency; every loop is bounded by a count the host passes.
//
// The gather new[j] = cur[o[j]]: neighbouring bins share their owner (a frame has a few dozen peaks), so the lanes of a wave
// read a handful of distinct LDS words, each a broadcast -- distinct owners of one wave differ by at least 2 and lie within
// a few hundred words, a few-way conflict at worst.  cur and new are different rows (history in k_spsi_apply, ping-pong in
// the others), so a step costs one barrier.
#include "gl_fft.h"
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int NB = NFFT / 2 + 1;  // 513 bins
constexpr int SPSI_THREADS = 256;
constexpr int SPSI_SLOTS = (NB + SPSI_THREADS - 1) / SPSI_THREADS;  // bins per thread of the gather kernels: tid + 256 r
constexpr int NONE_R = 1 << 20;  // "no peak at or above"

// One frame's map.  Lane l owns bins 8 l .. 8 l + 7 (contiguous, so that the nearest peak below / above is a running maximum /
// minimum inside the lane and one wave scan across lanes); lane 0 also finishes bin 512, which is never a peak.
__global__ __launch_bounds__(64 * FRAMES_PER_BLOCK) void k_spsi_maps(const float *__restrict__ S, uint2 *__restrict__ map, int F) {
  __shared__ float sm[FRAMES_PER_BLOCK][NB + 1 + 2];  // m[-1] .. m[513] (both ends: never compared for a peak decision that counts)
  __shared__ float sp[FRAMES_PER_BLOCK][NB];          // p of the peaks
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * FRAMES_PER_BLOCK + wave;
  if (row >= F) return;  // (whole waves leave; nothing below crosses waves)
  const float *m_in = S + (size_t)row * NB;
  float *m = sm[wave] + 1;
  for (int k = lane; k < NB; k += 64) m[k] = m_in[k];
  if (lane == 0) m[-1] = 0.f, m[NB] = 0.f;
  wave_lds_sync();
  float v[10];  // m[8 l - 1 .. 8 l + 8]
#pragma unroll
  for (int i = 0; i < 10; ++i) v[i] = m[8 * lane - 1 + i];
  unsigned peaks = 0;  // bit i: bin 8 l + i is a peak
  int lmax = -1, lmin = NONE_R;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = 8 * lane + i;
    const float a = v[i], b = v[i + 1], c = v[i + 2];
    if (k >= 1 && k <= NB - 2 && b > a && b >= c) {
      peaks |= 1u << i;
      lmax = k;
      lmin = min(lmin, k);
      const float d = (a - b) + (c - b);
      float p = d == 0.f ? 0.f : 0.5f * (a - c) / d;
      p = fminf(fmaxf(p, -0.5f), 0.5f);
      sp[wave][k] = p;
    }
  }
  // nearest peak in the lanes below (exclusive prefix maximum) and above (exclusive suffix minimum)
  int inc_max = lmax, inc_min = lmin;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(inc_max, o, 64), b = __shfl_down(inc_min, o, 64);
    if (lane >= o) inc_max = max(inc_max, a);
    if (lane + o < 64) inc_min = min(inc_min, b);
  }
  int left = __shfl_up(inc_max, 1, 64), right = __shfl_down(inc_min, 1, 64);
  if (lane == 0) left = -1;
  if (lane == 63) right = NONE_R;
  const int top = __shfl(inc_max, 63, 64);  // the frame's highest peak, -1: the frame has none
  wave_lds_sync();                          // (sp)
  auto cell = [&](int j, int l, int r) {
    if (top < 0) return make_uint2((unsigned)j, 0u);  // no peak: the phase is carried through
    const bool hl = l >= 0, hr = r < NONE_R;
    const int o = hl && hr ? (j - l <= r - j ? l : r) : (hl ? l : r);
    const float pp = sp[wave][o];
    const unsigned adv = ((unsigned)(o & 3) << 30) + (unsigned)(int)rintf(pp * 1073741824.0f);
    const bool flip = j != o && (pp > 0.f ? (j < o || j == o + 1) : (j > o || j == o - 1));
    return make_uint2((unsigned)o, adv + (flip ? 0x80000000u : 0u));
  };
  int rr[8];  // nearest peak at or above, per own bin
  {
    int r = right;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
      if (peaks & (1u << i)) r = 8 * lane + i;
      rr[i] = r;
    }
  }
  uint2 *out = map + (size_t)row * NB;
  int l = left;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = 8 * lane + i;
    if (peaks & (1u << i)) l = j;
    out[j] = cell(j, l, rr[i]);
  }
  if (lane == 0) out[NB - 1] = cell(NB - 1, top, NONE_R);
}

// Where a workgroup's segment lies.  segs == null: one utterance of F frames cut every SPSI_L frames.
__device__ __forceinline__ SpsiSeg spsi_seg(const SpsiSeg *__restrict__ segs, int s, int F) {
  if (segs) return segs[s];
  SpsiSeg g;
  g.row0 = s * SPSI_L;
  g.n = min(SPSI_L, F - g.row0);
  g.first = s == 0;
  g.last = g.row0 + g.n >= F;
  return g;
}

__global__ __launch_bounds__(SPSI_THREADS) void k_spsi_compose(const uint2 *__restrict__ map, const SpsiSeg *__restrict__ segs, int F,
                                                                 uint2 *__restrict__ comp) {
  __shared__ unsigned sO[2][NB], sD[2][NB];
  const SpsiSeg g = spsi_seg(segs, blockIdx.x, F);
  if (g.last) return;  // nobody enters behind an utterance's last segment (uniform: the whole workgroup leaves)
  const int n = min(max(g.n, 0), SPSI_L);
  const int tid = threadIdx.x;
  uint2 cur[SPSI_SLOTS] = {};
#pragma unroll
  for (int r = 0; r < SPSI_SLOTS; ++r) {
    const int j = tid + SPSI_THREADS * r;
    if (j < NB) {
      sO[0][j] = (unsigned)j, sD[0][j] = 0u;
      cur[r] = map[(size_t)g.row0 * NB + j];
    }
  }
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    const int a = t & 1, b = a ^ 1;
    uint2 nxt[SPSI_SLOTS] = {};  // the next frame's map: its load does not depend on the gather
#pragma unroll
    for (int r = 0; r < SPSI_SLOTS; ++r) {
      const int j = tid + SPSI_THREADS * r;
      if (j < NB) {
        if (t + 1 < n) nxt[r] = map[(size_t)(g.row0 + t + 1) * NB + j];
        const unsigned o = min(cur[r].x, (unsigned)(NB - 1));
        sO[b][j] = sO[a][o];
        sD[b][j] = sD[a][o] + cur[r].y;
        cur[r] = nxt[r];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < SPSI_SLOTS; ++r) {
    const int j = tid + SPSI_THREADS * r;
    if (j < NB) comp[(size_t)blockIdx.x * NB + j] = make_uint2(sO[n & 1][j], sD[n & 1][j]);
  }
}

// entry[s] = the phase in front of segment s, for every segment of the utterance but its first (whose entry is 0)
__global__ __launch_bounds__(SPSI_THREADS) void k_spsi_carry(const uint2 *__restrict__ comp, const SpsiUtt *__restrict__ utts, int nseg_single,
                                                               unsigned *__restrict__ entry) {
  __shared__ unsigned sC[2][NB];
  const int seg0 = utts ? utts[blockIdx.x].seg0 : 0;
  const int nseg = utts ? utts[blockIdx.x].nseg : nseg_single;
  if (nseg < 2) return;
  const int tid = threadIdx.x;
  uint2 cur[SPSI_SLOTS] = {};
#pragma unroll
  for (int r = 0; r < SPSI_SLOTS; ++r) {
    const int j = tid + SPSI_THREADS * r;
    if (j < NB) {
      sC[0][j] = 0u;
      cur[r] = comp[(size_t)seg0 * NB + j];
    }
  }
  __syncthreads();
  for (int s = 0; s + 1 < nseg; ++s) {
    const int a = s & 1, b = a ^ 1;
    uint2 nxt[SPSI_SLOTS] = {};
#pragma unroll
    for (int r = 0; r < SPSI_SLOTS; ++r) {
      const int j = tid + SPSI_THREADS * r;
      if (j < NB) {
        if (s + 2 < nseg) nxt[r] = comp[(size_t)(seg0 + s + 1) * NB + j];
        const unsigned c = sC[a][min(cur[r].x, (unsigned)(NB - 1))] + cur[r].y;
        sC[b][j] = c;
        entry[(size_t)(seg0 + s + 1) * NB + j] = c;
        cur[r] = nxt[r];
      }
    }
    __syncthreads();
  }
}

// The segment's frames from its entry phase; the phases stay in LDS (row t + 1 = frame t) until the chain is done, then every
// cell becomes an angle at once: u = (float)(phi >> 8) 2^-24, (cos, sin) 2 pi u; the previous spectrum is 0.
__global__ __launch_bounds__(SPSI_THREADS) void k_spsi_apply(const uint2 *__restrict__ map, const SpsiSeg *__restrict__ segs, int F,
                                                               const unsigned *__restrict__ entry, float2 *__restrict__ ang,
                                                               float2 *__restrict__ tprev, unsigned *__restrict__ turns) {
  __shared__ unsigned sH[SPSI_L + 1][NB];
  const SpsiSeg g = spsi_seg(segs, blockIdx.x, F);
  const int n = min(max(g.n, 0), SPSI_L);
  const int tid = threadIdx.x;
  uint2 cur[SPSI_SLOTS] = {};
#pragma unroll
  for (int r = 0; r < SPSI_SLOTS; ++r) {
    const int j = tid + SPSI_THREADS * r;
    if (j < NB) {
      sH[0][j] = g.first ? 0u : entry[(size_t)blockIdx.x * NB + j];
      if (n > 0) cur[r] = map[(size_t)g.row0 * NB + j];
    }
  }
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    uint2 nxt[SPSI_SLOTS] = {};
#pragma unroll
    for (int r = 0; r < SPSI_SLOTS; ++r) {
      const int j = tid + SPSI_THREADS * r;
      if (j < NB) {
        if (t + 1 < n) nxt[r] = map[(size_t)(g.row0 + t + 1) * NB + j];
        sH[t + 1][j] = sH[t][min(cur[r].x, (unsigned)(NB - 1))] + cur[r].y;
        cur[r] = nxt[r];
      }
    }
    __syncthreads();
  }
  const unsigned *h = &sH[1][0];
  const size_t base = (size_t)g.row0 * NB;
  for (int i = tid; i < n * NB; i += SPSI_THREADS) {
    const unsigned phi = h[i];
    const float u = (float)(phi >> 8) * 5.9604644775390625e-8f;  // 2^-24: exact
    float sn, cs;
    sincospif(2.0f * u, &sn, &cs);
    ang[base + i] = make_float2(cs, sn);
    tprev[base + i] = make_float2(0.f, 0.f);
    if (turns) turns[base + i] = phi;
  }
}

// parity hook: device [F][nb] -> the boundary's (nb x F), turns and (cos, sin) pairs
__global__ void k_spsi_export(const unsigned *__restrict__ turns, const float2 *__restrict__ ang, int F, int nb, unsigned *__restrict__ turns_out,
                              float2 *__restrict__ ang_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F * nb) return;
  const int f = i / nb, k = i % nb;
  turns_out[(size_t)k * F + f] = turns[i];
  ang_out[(size_t)k * F + f] = ang[i];
}

}  // namespace

void launch_spsi(const float *S, int F, const SpsiSeg *segs_dev, const SpsiUtt *utts_dev, int nseg, int n_utt, bool chained,
                 const SpsiBufs &b, float2 *ang, float2 *tprev, unsigned *turns, hipStream_t s) {
  if (F <= 0 || nseg <= 0 || n_utt <= 0) return;
  hipLaunchKernelGGL(k_spsi_maps, dim3((F + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK), dim3(64 * FRAMES_PER_BLOCK), 0, s, S, b.map, F);
  if (chained) {  // some utterance has more than one segment
    hipLaunchKernelGGL(k_spsi_compose, dim3(nseg), dim3(SPSI_THREADS), 0, s, b.map, segs_dev, F, b.comp);
    hipLaunchKernelGGL(k_spsi_carry, dim3(n_utt), dim3(SPSI_THREADS), 0, s, b.comp, utts_dev, nseg, b.entry);
  }
  hipLaunchKernelGGL(k_spsi_apply, dim3(nseg), dim3(SPSI_THREADS), 0, s, b.map, segs_dev, F, b.entry, ang, tprev, turns);
  HIP_CHECK(hipGetLastError());
}

void launch_spsi_export(const unsigned *turns, const float2 *ang, int F, int nb, unsigned *turns_out, float2 *ang_out, hipStream_t s) {
  const int n = F * nb;
  hipLaunchKernelGGL(k_spsi_export, dim3((n + 255) / 256), dim3(256), 0, s, turns, ang, F, nb, turns_out, ang_out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
