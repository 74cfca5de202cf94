// loudness.hip -- the loudness stage behind the resampler: ITU-R BS.1770 integrated loudness and true peak of the delivered
// signal, and the linear gain to a target (the definition: include/xdtts.h; the coefficients, the powers of the transition
// matrix, the plan and the gain rule: loudness_plan.h).
// The K-weighting is a recursion; it runs as a three-phase scan over segments of LOUD_SEG samples, one lane a segment, one
// wave (LOUD_LANES segments = LOUD_GROUP samples of ONE utterance) a workgroup -- with three more waves beside it that help
// stage the tile and share the true-peak pass, so that a lane has 9 loads in flight and 8 samples of the peak filter:
//   k_loud_local   every lane runs its segment from the zero state; an in-wave scan with A^(32 2^k) turns the 64 final states
//                  into each segment's state on entry, had the group started from zero, and the group's aggregate.  The same
//                  staged tile gives the true peak (3 phases x 24 taps, fp32) and the sample peak of the group.
//   k_loud_carry   one wave per utterance: the groups' aggregates are scanned with A^(2048 2^k), 64 groups a step, the carry of
//                  a step entering at lane 0; writes every group's true state on entry, and the utterance's two peaks.
//   k_loud_energy  every lane re-runs its segment from its true state (entry state + A^(32 lane) . the group's) and adds y^2
//                  into the at most two 100 ms sub-blocks the segment touches (h >= 800 > LOUD_SEG).
//   k_loud_final   one workgroup per utterance: sub-block sums from the segments' partials in ascending order, the block
//                  means z_j, both gates, Z, the counts and the gain.
// k_loud_scale applies the gain.  State, coefficients, carry and every energy sum are fp64; samples are fp32.  No atomics,
// every reduction in a fixed order, nothing from libm: a result is a function of (rate, n, the samples, target, ceiling) alone,
// so an utterance of a ragged launch has the bits of the single call.  (The three scan kernels are templates on the type of
// the recurrences: the product runs <double>; XDTTS_LOUD=fp32 runs <float>, so that tools/loudness_check.py can say what fp64
// costs and buys.)
// A tile is staged in LDS (coalesced global reads) with one pad word per 32, so that 64 lanes reading their own contiguous
// segments hit 32 distinct banks per half wave.
#include "env.h"
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int LOUD_HALO = LOUD_TP_HALF;                   // samples in front of the group (and as many behind) the true peak reads
constexpr int LOUD_TILE = LOUD_GROUP + 2 * LOUD_HALO;     // staged samples
constexpr int LOUD_LDS = LOUD_TILE + (LOUD_TILE >> 5) + 1;  // ... with the pad words
constexpr int LOUD_WG = 256;                              // lanes of k_loud_local and k_loud_energy: all four waves stage the tile and share
                                                          // the true peak; the recursion and its scan are wave 0's
constexpr int LOUD_TP_ROUNDS = LOUD_GROUP / LOUD_WG;      // samples a lane takes in the true-peak pass
static_assert(LOUD_SEG == 32 && LOUD_LANES == 64 && (1 << LOUD_SEG_LOG2) == LOUD_SEG && (1 << LOUD_GROUP_LOG2) == LOUD_GROUP,
              "the scan's powers are indexed by log2");
static_assert(sizeof(LoudResult) == 40, "LoudResult is xdtts_loudness");

__device__ __forceinline__ int lds_at(int w) { return w + (w >> 5); }

// the utterance that owns group `grp` of the table's numbering (ascending grp0; the index stays in [0, count) whatever the table holds)
__device__ __forceinline__ LoudUtt loud_find(const LoudUtt *tab, int count, int grp, const LoudUtt &one, int *u) {
  *u = 0;
  if (!tab) return one;
  int lo = 0, hi = count - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].grp0 <= grp) lo = mid; else hi = mid - 1;
  }
  *u = lo;
  return tab[lo];
}

// the tile of group gl of utterance t: xs[lds_at(w)] = x[gl GROUP - HALO + w], zero outside [0, n)
// (LOUD_WG lanes; every lane's loads are issued before the first LDS write, so their latencies overlap)
__device__ __forceinline__ void loud_stage(const float *__restrict__ x, const LoudUtt &t, int gl, float *xs) {
  const float *xu = x + t.src0;
  const int lo = gl * LOUD_GROUP - LOUD_HALO;
  constexpr int ROUNDS = (LOUD_TILE + LOUD_WG - 1) / LOUD_WG;
  float v[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int n = lo + r * LOUD_WG + (int)threadIdx.x;
    v[r] = (n >= 0 && n < t.n && r * LOUD_WG + (int)threadIdx.x < LOUD_TILE) ? xu[n] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int w = r * LOUD_WG + (int)threadIdx.x;
    if (w < LOUD_TILE) xs[lds_at(w)] = v[r];
  }
  __syncthreads();
}

// v <- M v, M row major 4 x 4 at a wave-uniform address.  R = double; float only in the comparison form (XDTTS_LOUD=fp32).
template <typename R>
__device__ __forceinline__ void mat_apply(const double *__restrict__ M, R v[4]) {
  const R a = v[0], b = v[1], c = v[2], d = v[3];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (((R)M[r * 4] * a + (R)M[r * 4 + 1] * b) + ((R)M[r * 4 + 2] * c + (R)M[r * 4 + 3] * d));
}

// inclusive scan over the wave of s_{i+1} = M s_i + z_i:  lane i ends with the state behind element i; pw0 = M, then its squares
template <typename R>
__device__ __forceinline__ void wave_scan(const double (*__restrict__ pw)[16], int k0, R s[4]) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    R t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = __shfl_up(s[i], 1u << k, LOUD_LANES);
    mat_apply(pw[k0 + k], t);
    if (lane >= (1 << k)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] += t[i];
    }
  }
}

template <typename R>
__global__ __launch_bounds__(LOUD_WG) void k_loud_local(const float *__restrict__ x, const LoudUtt *__restrict__ tab, int count,
                                                          int grp_base, LoudUtt one, const LoudnessTable *__restrict__ T, LoudBufs B) {
  __shared__ float xs[LOUD_LDS];
  __shared__ float pk[LOUD_WG / 64][2];
  const int lane = threadIdx.x, grp = (int)blockIdx.x + grp_base;
  int u;
  const LoudUtt t = loud_find(tab, count, grp, one, &u);
  const int gl = grp - t.grp0;
  if (gl < 0 || (long long)gl * LOUD_GROUP >= (long long)t.n) return;  // (never: the host's table)
  loud_stage(x, t, gl, xs);
  // The peaks, a lane a sample in rounds of 256 consecutive samples; phase p of sample n = sum_j x[n - j] taps[p][j + 12], j
  // ascending in one fmaf chain.  The taps are the outer loop: each is read once for a lane's eight samples.
  const int n_here = min(LOUD_GROUP, t.n - gl * LOUD_GROUP);
  float a[LOUD_TP_ROUNDS][LOUD_TP_PHASES];
#pragma unroll
  for (int r = 0; r < LOUD_TP_ROUNDS; ++r) a[r][0] = a[r][1] = a[r][2] = 0.f;
#pragma unroll
  for (int j = -LOUD_TP_HALF; j < LOUD_TP_HALF; ++j) {
    const float t0 = T->taps[0][j + LOUD_TP_HALF], t1 = T->taps[1][j + LOUD_TP_HALF], t2 = T->taps[2][j + LOUD_TP_HALF];
#pragma unroll
    for (int r = 0; r < LOUD_TP_ROUNDS; ++r) {
      const float v = xs[lds_at(LOUD_HALO + r * LOUD_WG + lane - j)];
      a[r][0] = fmaf(v, t0, a[r][0]);
      a[r][1] = fmaf(v, t1, a[r][1]);
      a[r][2] = fmaf(v, t2, a[r][2]);
    }
  }
  float tp = 0.f, sp = 0.f;
#pragma unroll
  for (int r = 0; r < LOUD_TP_ROUNDS; ++r) {
    if (r * LOUD_WG + lane < n_here) {  // (behind the last sample nothing counts: the filter's tail there is not part of the signal)
      tp = fmaxf(tp, fmaxf(fabsf(a[r][0]), fmaxf(fabsf(a[r][1]), fabsf(a[r][2]))));
      sp = fmaxf(sp, fabsf(xs[lds_at(LOUD_HALO + r * LOUD_WG + lane)]));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    tp = fmaxf(tp, __shfl_xor(tp, o, 64));
    sp = fmaxf(sp, __shfl_xor(sp, o, 64));
  }
  if ((lane & 63) == 0) pk[lane >> 6][0] = tp, pk[lane >> 6][1] = sp;
  __syncthreads();
  if (lane >= LOUD_LANES) return;  // the recursion is wave 0's
  if (lane == 0) {
    tp = fmaxf(fmaxf(pk[0][0], pk[1][0]), fmaxf(pk[2][0], pk[3][0]));
    sp = fmaxf(fmaxf(pk[0][1], pk[1][1]), fmaxf(pk[2][1], pk[3][1]));
    B.peaks[grp] = make_float2(fmaxf(tp, sp), sp);
  }
  // the segment from the zero state (samples past n are zero: their segments stay at zero)
  R c[10], s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 10; ++i) c[i] = (R)T->coef[i];
  const int w0 = LOUD_HALO + lane * LOUD_SEG;
#pragma unroll 4
  for (int i = 0; i < LOUD_SEG; ++i) loudness_step<R>(c, s, (R)xs[lds_at(w0 + i)]);
  wave_scan(T->pw, LOUD_SEG_LOG2, s);
  const int seg = gl * LOUD_LANES + lane, nseg = (t.n + LOUD_SEG - 1) / LOUD_SEG;
  R e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e[i] = __shfl_up(s[i], 1, LOUD_LANES);
    if (lane == 0) e[i] = 0;
  }
  if (seg < nseg) {
    double *q = B.excl + (size_t)(t.seg0 + seg) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = e[i];
  }
  if (lane == LOUD_LANES - 1) {
    double *q = B.agg + (size_t)grp * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = s[i];
  }
}

template <typename R>
__global__ __launch_bounds__(LOUD_LANES) void k_loud_carry(const LoudUtt *__restrict__ tab, LoudUtt one, const LoudnessTable *__restrict__ T,
                                                          LoudBufs B, LoudResult *__restrict__ res) {
  const int lane = threadIdx.x;
  const LoudUtt t = tab ? tab[blockIdx.x] : one;
  const int G = (t.n + LOUD_GROUP - 1) / LOUD_GROUP;
  R carry[4] = {0, 0, 0, 0};
  float tp = 0.f, sp = 0.f;
  for (int g0 = 0; g0 < G; g0 += LOUD_LANES) {
    const int g = g0 + lane;
    R v[4] = {0, 0, 0, 0};
    if (g < G) {
      const double *q = B.agg + (size_t)(t.grp0 + g) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (R)q[i];
      const float2 pk = B.peaks[t.grp0 + g];
      tp = fmaxf(tp, pk.x);
      sp = fmaxf(sp, pk.y);
    }
    if (lane == 0) {  // the state that enters this step of 64 groups
      R pc[4] = {carry[0], carry[1], carry[2], carry[3]};
      mat_apply(T->pw[LOUD_GROUP_LOG2], pc);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += pc[i];
    }
    wave_scan(T->pw, LOUD_GROUP_LOG2, v);
    R e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      e[i] = __shfl_up(v[i], 1, LOUD_LANES);
      if (lane == 0) e[i] = carry[i];
    }
    if (g < G) {
      double *q = B.gin + (size_t)(t.grp0 + g) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = e[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) carry[i] = __shfl(v[i], LOUD_LANES - 1, LOUD_LANES);
  }
  for (int o = 32; o > 0; o >>= 1) {
    tp = fmaxf(tp, __shfl_xor(tp, o, LOUD_LANES));
    sp = fmaxf(sp, __shfl_xor(sp, o, LOUD_LANES));
  }
  if (lane == 0) {
    res[blockIdx.x].true_peak = (double)tp;
    res[blockIdx.x].sample_peak = (double)sp;
  }
}

template <typename R>
__global__ __launch_bounds__(LOUD_WG) void k_loud_energy(const float *__restrict__ x, const LoudUtt *__restrict__ tab, int count,
                                                           int grp_base, LoudUtt one, const LoudnessTable *__restrict__ T, LoudBufs B, int h) {
  __shared__ float xs[LOUD_LDS];
  const int lane = threadIdx.x, grp = (int)blockIdx.x + grp_base;
  int u;
  const LoudUtt t = loud_find(tab, count, grp, one, &u);
  const int gl = grp - t.grp0;
  if (gl < 0 || (long long)gl * LOUD_GROUP >= (long long)t.n) return;
  loud_stage(x, t, gl, xs);
  const int seg = gl * LOUD_LANES + lane, nseg = (t.n + LOUD_SEG - 1) / LOUD_SEG;
  if (lane >= LOUD_LANES || seg >= nseg) return;  // (waves 1 .. 3 only staged)
  // the true state on entry: what the group's own scan left, plus the group's entry state moved over `lane` segments
  R s[4], v[4];
  {
    const double *q = B.gin + (size_t)grp * 4, *e = B.excl + (size_t)(t.seg0 + seg) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (R)q[i], s[i] = (R)e[i];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    R m[4] = {v[0], v[1], v[2], v[3]};
    mat_apply(T->pw[LOUD_SEG_LOG2 + k], m);
    if ((lane >> k) & 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = m[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] += v[i];
  R c[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) c[i] = (R)T->coef[i];
  const int n0 = seg * LOUD_SEG, w0 = LOUD_HALO + lane * LOUD_SEG;
  const int edge = (n0 / h + 1) * h - n0;  // samples of the segment inside the first sub-block it touches (if < LOUD_SEG)
  const int len = min(LOUD_SEG, t.n - n0);
  R acc0 = 0, acc1 = 0;
#pragma unroll 4
  for (int i = 0; i < LOUD_SEG; ++i) {
    const R y = loudness_step<R>(c, s, (R)xs[lds_at(w0 + i)]);
    const R yy = i < len ? y * y : (R)0;
    if (i < edge) acc0 += yy; else acc1 += yy;
  }
  double *q = B.part + (size_t)(t.seg0 + seg) * 2;
  q[0] = acc0;
  q[1] = acc1;
}

constexpr int LOUD_FINAL = 256;

// sum over the workgroup in a fixed order: lanes' values into LDS, then a tree; every lane gets the total
__device__ __forceinline__ void wg_sum(double v, int c, double *sd, int *sc, double *out_v, int *out_c) {
  const int tid = threadIdx.x;
  __syncthreads();
  sd[tid] = v;
  sc[tid] = c;
  __syncthreads();
  for (int o = LOUD_FINAL / 2; o > 0; o >>= 1) {
    if (tid < o) sd[tid] += sd[tid + o], sc[tid] += sc[tid + o];
    __syncthreads();
  }
  *out_v = sd[0];
  *out_c = sc[0];
}

__global__ __launch_bounds__(LOUD_FINAL) void k_loud_final(const LoudUtt *__restrict__ tab, LoudUtt one, LoudBufs B, LoudResult *__restrict__ res,
                                                          int h, double abs_gate, double tgt, double ceil) {
  __shared__ double sd[LOUD_FINAL];
  __shared__ int sc[LOUD_FINAL];
  const int tid = threadIdx.x;
  const LoudUtt t = tab ? tab[blockIdx.x] : one;
  const int nseg = (t.n + LOUD_SEG - 1) / LOUD_SEG, nsb = (t.n + h - 1) / h;
  const int nb = t.n >= 4 * h ? (t.n - 4 * h) / h + 1 : 0;
  double *sub = B.sub + t.sb0;
  const double *part = B.part + (size_t)t.seg0 * 2;
  // sub-block b = samples [b h, (b + 1) h): the partials of the segments that touch it, ascending
  for (int b = tid; b < nsb; b += LOUD_FINAL) {
    const int k_lo = (int)(((long long)b * h) >> LOUD_SEG_LOG2);
    const int k_hi = min((int)((((long long)(b + 1) * h) - 1) >> LOUD_SEG_LOG2), nseg - 1);
    // (sixteen loads in flight, then their sum in ascending order: the loop is bound by the loads' latency, not by the adds)
    double a = 0.0;
    for (int k0 = k_lo; k0 <= k_hi; k0 += 16) {
      double v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = min(k0 + i, k_hi);
        v[i] = part[(size_t)k * 2 + (b - (k * LOUD_SEG) / h)];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (k0 + i <= k_hi) a += v[i];
    }
    sub[b] = a;
  }
  __syncthreads();
  const double inv = 1.0 / (double)(4 * h);
  double sa = 0.0, total;
  int na = 0, n_abs, n_gated;
  for (int j = tid; j < nb; j += LOUD_FINAL) {
    const double z = ((sub[j] + sub[j + 1]) + (sub[j + 2] + sub[j + 3])) * inv;
    if (z > abs_gate) sa += z, ++na;
  }
  wg_sum(sa, na, sd, sc, &total, &n_abs);
  double Z = 0.0;
  n_gated = 0;
  if (n_abs > 0) {  // (uniform)
    const double rel = LOUD_REL_GATE * (total / (double)n_abs);
    double sg = 0.0;
    int ng = 0;
    for (int j = tid; j < nb; j += LOUD_FINAL) {
      const double z = ((sub[j] + sub[j + 1]) + (sub[j + 2] + sub[j + 3])) * inv;
      if (z > abs_gate && z > rel) sg += z, ++ng;
    }
    wg_sum(sg, ng, sd, sc, &total, &n_gated);
    if (n_gated > 0) Z = total / (double)n_gated;
  }
  if (tid == 0) {
    LoudResult &r = res[blockIdx.x];
    r.mean_square = Z;
    r.blocks = nb;
    r.gated = n_gated;
    r.gain = tgt > 0.0 ? loudness_gain(Z, r.true_peak, tgt, ceil) : 1.0;
  }
}

__global__ __launch_bounds__(LOUD_LANES) void k_loud_scale(float *__restrict__ x, const LoudUtt *__restrict__ tab, int count, int grp_base,
                                                          LoudUtt one, const LoudResult *__restrict__ res) {
  const int grp = (int)blockIdx.x + grp_base;
  int u;
  const LoudUtt t = loud_find(tab, count, grp, one, &u);
  const int gl = grp - t.grp0;
  if (gl < 0 || (long long)gl * LOUD_GROUP >= (long long)t.n) return;
  const float gain = (float)res[u].gain;
  if (gain == 1.0f) return;
  float *p = x + t.src0;
  const int hi = min(t.n, (gl + 1) * LOUD_GROUP);
  for (int i = gl * LOUD_GROUP + threadIdx.x; i < hi; i += LOUD_LANES) p[i] *= gain;
}

}  // namespace

void launch_loudness_measure(const float *x, const LoudUtt *tab_dev, int count, int grp_base, int n_groups, const LoudUtt &one,
                             const LoudnessTable *table_dev, const LoudBufs &b, LoudResult *res, int rate, double tgt, double ceil,
                             hipStream_t s) {
  if (count <= 0 || n_groups <= 0) return;
  const int h = loudness_hop(rate);
  if (h <= LOUD_SEG) fail(XDTTS_ERR_BAD_ARG, "loudness: rate %d has sub-blocks of %d samples, a segment has %d", rate, h, LOUD_SEG);
  if (env::equals(env::LOUD, "fp32")) {  // developer comparison aid (tools/loudness_check.py): what the fp64 recurrences cost and buy
    hipLaunchKernelGGL(k_loud_local<float>, dim3((unsigned)n_groups), dim3(LOUD_WG), 0, s, x, tab_dev, count, grp_base, one, table_dev, b);
    hipLaunchKernelGGL(k_loud_carry<float>, dim3((unsigned)count), dim3(LOUD_LANES), 0, s, tab_dev, one, table_dev, b, res);
    hipLaunchKernelGGL(k_loud_energy<float>, dim3((unsigned)n_groups), dim3(LOUD_WG), 0, s, x, tab_dev, count, grp_base, one, table_dev, b, h);
  } else {
    hipLaunchKernelGGL(k_loud_local<double>, dim3((unsigned)n_groups), dim3(LOUD_WG), 0, s, x, tab_dev, count, grp_base, one, table_dev, b);
    hipLaunchKernelGGL(k_loud_carry<double>, dim3((unsigned)count), dim3(LOUD_LANES), 0, s, tab_dev, one, table_dev, b, res);
    hipLaunchKernelGGL(k_loud_energy<double>, dim3((unsigned)n_groups), dim3(LOUD_WG), 0, s, x, tab_dev, count, grp_base, one, table_dev, b, h);
  }
  hipLaunchKernelGGL(k_loud_final, dim3((unsigned)count), dim3(LOUD_FINAL), 0, s, tab_dev, one, b, res, h, loudness_abs_gate(), tgt, ceil);
  HIP_CHECK(hipGetLastError());
}

void launch_loudness_scale(float *x, const LoudUtt *tab_dev, int count, int grp_base, int n_groups, const LoudUtt &one,
                           const LoudResult *res, hipStream_t s) {
  if (count <= 0 || n_groups <= 0) return;
  hipLaunchKernelGGL(k_loud_scale, dim3((unsigned)n_groups), dim3(LOUD_LANES), 0, s, x, tab_dev, count, grp_base, one, res);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
