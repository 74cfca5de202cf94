// limiter.hip -- the look-ahead true-peak limiter that takes k_loud_scale's place where a limiter is set (the definition:
// include/xdtts.h; the half width, the window, the per-sample functions and the host walk of a tile: limiter_plan.h).
// One kernel, k_limit, for the single call, the ragged batch, the document's stream and the stage alone.  A workgroup owns
// LIM_TILE consecutive outputs of ONE utterance and keeps two LDS buffers, A (W + 26 floats, W = TILE + 4 H) and B (W + 1):
//   1  A <- x[t0 - 2 H - 13 .. t0 + TILE + 2 H + 12], zero outside the utterance; each lane keeps its 16 own samples in registers
//   2  B <- the peak values Y (3 phases x 24 taps, fmaf chains, the loudness stage's taps), then r into A at the sample's own slot
//   3  a workgroup-wide vote: no r < 1 -> out = fl(x G), done (the utterance is not engaged at all: the same, without staging)
//   4  the sliding minimum over 2 H + 1 by doubling, ping-pong between the two buffers (log2 P levels, P the largest power of two
//      <= 2 H + 1; two windows of P cover the hold), then d = 1 - hold and one flag per 64 positions: any d != 0
//   5  the smoothing FIR: w[t] wave-uniform, d at consecutive LDS addresses across the lanes, four rounds (outputs 256 apart) as
//      four chains at once; a wave skips the 2 H + 1 taps of four rounds whose windows have no flag set (limiting is sparse on
//      speech) -- the sum of zeros is +0 either way
//   6  out = fl(x fl(G min(1 - sum, r))), and the tile's share of the stats: min g by compare-and-swap on the float, the count of
//      g < 1 by an integer add -- neither depends on the order of arrival.
// No libm, no scratch, a fixed order inside every chain: out and stats are functions of (the utterance, G, c, H) alone, so a
// ragged launch has the bits of the single call and the device those of limiter_reference().
#include "kernels.h"

namespace xdtts {

namespace {

static_assert(sizeof(LimiterStats) == 24 && sizeof(xdtts_limiter_stats) == 24, "LimiterStats is xdtts_limiter_stats");
static_assert(LIM_TILE % LIM_WG == 0 && LIM_WG % 64 == 0 && LIM_TILE % 64 == 0, "a wave's outputs of a round are one 64-block");
static_assert((size_t)(LIM_TILE + 4 * LIM_H_MAX + 2 * LIM_FRONT + LIM_TILE + 4 * LIM_H_MAX + 1 + (LIM_TILE + 2 * LIM_H_MAX + 63) / 64 + 8) * 4 + 256 <= 65536,
              "the largest half width fits 64 KiB of LDS beside the 256 bytes the compiler takes for the vote");

// the utterance that owns tile `tile` of the table's numbering (ascending tile0; the index stays in [0, count) whatever the table holds)
__device__ __forceinline__ LimUtt lim_find(const LimUtt *tab, int count, int tile, const LimUtt &one, int *u) {
  *u = 0;
  if (!tab) return one;
  int lo = 0, hi = count - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  *u = lo;
  return tab[lo];
}

__device__ __forceinline__ bool lim_job_engaged(const LimJob &J, int u, double *g0) {
  if (!J.res) {
    *g0 = J.gain0;
    return true;
  }
  const LoudResult r = J.res[u];
  *g0 = r.gain;
  return lim_engaged(r.mean_square, r.true_peak, r.gain, J.ceil);
}

__global__ __launch_bounds__(64) void k_limit_init(LimJob J, int count, LimiterStats *__restrict__ stats) {
  const int u = (int)(blockIdx.x * 64 + threadIdx.x);
  if (u >= count) return;
  double g0;
  const bool engaged = lim_job_engaged(J, u, &g0);
  stats[u] = LimiterStats{1.0f, J.H, engaged ? 1 : 0, 0};
}

__global__ __launch_bounds__(LIM_WG) void k_limit(const float *__restrict__ x, float *__restrict__ out, const LimUtt *__restrict__ tab, int count,
                                                  int tile_base, LimUtt one, LimJob J, LimiterStats *__restrict__ stats) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, H = J.H, W = lim_w(H), D = lim_d(H), P = lim_pow2(H);
  float *A = lds, *B = A + lim_xs(H);
  int *flags = reinterpret_cast<int *>(B + lim_ys(H));
  float *red = reinterpret_cast<float *>(flags + lim_flags(H));  // [4] minima, [4] counts
  int u;
  const LimUtt t = lim_find(tab, count, (int)blockIdx.x + tile_base, one, &u);
  const int tl = (int)blockIdx.x + tile_base - t.tile0;
  if (tl < 0 || (long long)tl * LIM_TILE >= (long long)t.n) return;  // (never: the host's table)
  const int t0 = tl * LIM_TILE, n_here = min(LIM_TILE, t.n - t0);
  const float *xu = x + t.src0;
  float *ou = out + t.dst0;
  double g0;
  const bool engaged = lim_job_engaged(J, u, &g0);  // (uniform)
  const float G = (float)g0, c = (float)J.ceil;
  if (!engaged) {
#pragma unroll
    for (int r = 0; r < LIM_ROUNDS; ++r) {
      const int o = r * LIM_WG + tid;
      if (o < n_here) ou[t0 + o] = lim_scale(xu[t0 + o], G);
    }
    return;
  }
  // 1
  const long long N = t.n, X0 = (long long)t0 - 2 * H - LIM_FRONT;
  for (int i = tid; i < lim_xs(H); i += LIM_WG) A[i] = lim_sample(xu, X0 + i, N);
  __syncthreads();
  float xc[LIM_ROUNDS], rc[LIM_ROUNDS];
#pragma unroll
  for (int r = 0; r < LIM_ROUNDS; ++r) xc[r] = A[2 * H + LIM_FRONT + r * LIM_WG + tid];
  // 2
  for (int q = tid; q < lim_ys(H); q += LIM_WG) {
    const long long pos = (long long)t0 - 2 * H - 1 + q;
    B[q] = lim_peak(A, q, J.taps, pos >= 0 && pos < N);
  }
  __syncthreads();
  int any = 0;
  for (int i = tid; i < W; i += LIM_WG) {
    const long long pos = (long long)t0 - 2 * H + i;
    const float r = lim_need(G, c, A[i + LIM_FRONT], B[i + 1], B[i], pos >= 0 && pos < N);
    A[i + LIM_FRONT] = r;  // (the slot this lane alone read)
    any |= r < 1.0f;
  }
  // 3
  if (!__syncthreads_or(any)) {
#pragma unroll
    for (int r = 0; r < LIM_ROUNDS; ++r) {
      const int o = r * LIM_WG + tid;
      if (o < n_here) ou[t0 + o] = lim_scale(xc[r], G);
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < LIM_ROUNDS; ++r) rc[r] = A[LIM_FRONT + 2 * H + r * LIM_WG + tid];
  // 4
  const float *cur = A + LIM_FRONT;
  bool in_a = true;
  for (int p = 1; p < P; p *= 2) {
    float *dst = in_a ? B : A;
    for (int i = tid; i + 2 * p <= W; i += LIM_WG) dst[i] = fminf(cur[i], cur[i + p]);
    __syncthreads();  // (the level behind this one writes what this one read; rc was read in front of the first)
    cur = dst;
    in_a = !in_a;
  }
  float *d = in_a ? B : A;
  for (int k0 = 0; k0 < D; k0 += LIM_WG) {
    const int k = k0 + tid;
    float v = 0.f;
    if (k < D) {
      v = lim_hold(cur, k, H, P);
      d[k] = v;
    }
    const unsigned long long b = __ballot(v != 0.f);
    if ((tid & 63) == 0 && k < D) flags[k >> 6] = b != 0ull;
  }
  __syncthreads();
  // 5, 6
  float mn = 1.0f;
  int cnt = 0;
  const int wave0 = tid & ~63;
  static_assert(LIM_ROUNDS % LIM_FIR_ROUNDS == 0, "the rounds go through the FIR in whole groups");
#pragma unroll
  for (int r0 = 0; r0 < LIM_ROUNDS; r0 += LIM_FIR_ROUNDS) {  // (unrolled: xc and rc stay in registers)
    int run = 0;
#pragma unroll
    for (int q = 0; q < LIM_FIR_ROUNDS; ++q) {
      const int o0 = (r0 + q) * LIM_WG + wave0;
      for (int b = o0 >> 6; b <= (o0 + 63 + 2 * H) >> 6; ++b) run |= flags[b];
    }
    run = __builtin_amdgcn_readfirstlane(run);
    float acc[LIM_FIR_ROUNDS] = {0.f, 0.f, 0.f, 0.f};
    if (run) lim_fir_rounds(J.win, d + r0 * LIM_WG + tid, LIM_WG, H, acc);
#pragma unroll
    for (int q = 0; q < LIM_FIR_ROUNDS; ++q) {
      const int o = (r0 + q) * LIM_WG + tid;
      if (o < n_here) {
        float g;
        ou[t0 + o] = lim_apply(xc[r0 + q], G, acc[q], rc[r0 + q], &g);
        cnt += g < 1.0f;
        mn = fminf(mn, g);
      }
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, s, 64));
    cnt += __shfl_xor(cnt, s, 64);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = mn;
    reinterpret_cast<int *>(red)[4 + (tid >> 6)] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    const int *rc4 = reinterpret_cast<const int *>(red) + 4;
    cnt = (rc4[0] + rc4[1]) + (rc4[2] + rc4[3]);
    if (cnt > 0) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[u].limited), (unsigned long long)cnt);
    unsigned *p = reinterpret_cast<unsigned *>(&stats[u].min_gain);
    unsigned old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int it = 0; it < 4096 && __uint_as_float(old) > mn; ++it) {  // (a bounded compare-and-swap: the minimum whatever the order)
      const unsigned seen = atomicCAS(p, old, __float_as_uint(mn));
      if (seen == old) break;
      old = seen;
    }
  }
}

}  // namespace

void launch_limit(const float *x, float *out, const LimUtt *tab_dev, int count, int tile_base, int n_tiles, const LimUtt &one,
                  const LimJob &job, LimiterStats *stats, hipStream_t s) {
  if (count <= 0 || n_tiles <= 0) return;
  if (job.H < LIM_H_MIN || job.H > LIM_H_MAX || !(job.ceil > 0.0) || !job.taps || !job.win || !stats)
    fail(XDTTS_ERR_BAD_ARG, "limiter: half width %d, ceiling %g do not fit the kernel", job.H, job.ceil);
  hipLaunchKernelGGL(k_limit_init, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, job, count, stats);
  const size_t lds = (size_t)lim_lds_floats(job.H) * sizeof(float);
  hipLaunchKernelGGL(k_limit, dim3((unsigned)n_tiles), dim3(LIM_WG), lds, s, x, out, tab_dev, count, tile_base, one, job, stats);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
