// compressor.hip -- the dynamic range compressor in front of the level stage (the definition: include/xdtts.h; the slopes, the
// per-sample functions and the host walk of a tile: compressor_plan.h).  Three launches for the single call, the ragged batch and
// the stage alone; a workgroup owns COMP_TILE consecutive samples of ONE utterance, a lane COMP_VEC consecutive ones per round:
//   k_comp_init   the stats' initial values
//   k_comp_tiles  per tile: the peak |x| into the utterance's stats (an integer max on the float's bits), and the tile's two
//                 aggregates -- the forward envelope at its last sample and the backward envelope at its first, had the utterance
//                 consisted of the tile alone
//   k_compress    per tile: the carries from the aggregates of the tiles within reach (a tent falls by TILE * slope per tile: a
//                 few to a few thousand tiles, strided over the lanes), l again from x, the prefix maximum of l + j rho and the
//                 suffix maximum of l - j alpha in tile-local 32-bit integers -- in the lane, across the wave by shuffles, across
//                 the 16 segments through LDS --, the gain computer, 2^x, the output, and the tile's share of the stats.
// P and `engaged` are read from the stats on the device: the host does not wait between the launches.  Integer maxima and sums
// only, so out and stats are functions of (the utterance, the plan) alone: a ragged launch has the bits of the single call and
// the device those of compressor_reference().  No libm, no scratch.
#include "kernels.h"

namespace xdtts {

namespace {

static_assert(sizeof(CompressorStats) == 24 && sizeof(xdtts_compressor_stats) == 24, "CompressorStats is xdtts_compressor_stats");
static_assert(sizeof(CompAgg) == 8, "one 64-bit store per tile");

// the utterance that owns tile `tile` of the table's numbering (ascending tile0; the index stays in [0, count) whatever the table holds)
__device__ __forceinline__ CompUtt comp_find(const CompUtt *tab, int count, int tile, const CompUtt &one, int *u) {
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

__device__ __forceinline__ int wave_max(int v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
  return v;
}

// the lane's COMP_VEC samples of a round from xs (the tile's first sample), 0 behind the utterance's end
__device__ __forceinline__ void comp_load(const float *xs, int j0, int n_here, bool vec, float v[COMP_VEC]) {
  if (vec && j0 + COMP_VEC <= n_here) {
    const float4 q = *reinterpret_cast<const float4 *>(xs + j0);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) v[c] = j0 + c < n_here ? xs[j0 + c] : 0.f;
  }
}

__global__ __launch_bounds__(64) void k_comp_init(int count, CompressorStats *stats) {
  const int u = (int)(blockIdx.x * 64 + threadIdx.x);
  if (u < count) stats[u] = CompressorStats{0.0f, COMP_NEG, 0, 0};
}

__global__ __launch_bounds__(COMP_WG) void k_comp_tiles(const float *x, const CompUtt *__restrict__ tab, int count, int tile_base, CompUtt one,
                                                        CompPlan P, CompAgg *__restrict__ agg, CompressorStats *stats) {
  __shared__ int red[3 * COMP_WAVES];
  const int tid = threadIdx.x, tile = (int)blockIdx.x + tile_base;
  int u;
  const CompUtt t = comp_find(tab, count, tile, one, &u);
  const int tl = tile - t.tile0;
  if (tl < 0 || (long long)tl * COMP_TILE >= (long long)t.n) return;  // (never: the host's table)
  const int t0 = tl * COMP_TILE, n_here = min(COMP_TILE, t.n - t0), last = n_here - 1;
  const float *xs = x + t.src0 + t0;
  const bool vec = (reinterpret_cast<uintptr_t>(xs) & 15u) == 0;
  int f = COMP_NEG, b = COMP_NEG;
  unsigned pk = 0;
#pragma unroll
  for (int r = 0; r < COMP_ROUNDS; ++r) {
    const int j0 = r * COMP_ROUND + COMP_VEC * tid;
    float v[COMP_VEC];
    comp_load(xs, j0, n_here, vec, v);
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) {
      const int j = j0 + c;
      if (!comp_valid(j, n_here)) continue;
      const unsigned a = comp_abs_bits(v[c]);
      const int l = comp_lvl(a);
      pk = max(pk, a);
      f = max(f, l - (last - j) * P.rho);
      b = max(b, l - j * P.alpha);
    }
  }
  f = wave_max(f);
  b = wave_max(b);
  pk = (unsigned)wave_max((int)pk);  // (|x| bits are below 2^31: the signed order is theirs)
  if ((tid & 63) == 0) {
    red[tid >> 6] = f;
    red[COMP_WAVES + (tid >> 6)] = b;
    red[2 * COMP_WAVES + (tid >> 6)] = (int)pk;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < COMP_WAVES; ++w) {
      f = max(f, red[w]);
      b = max(b, red[COMP_WAVES + w]);
      pk = max(pk, (unsigned)red[2 * COMP_WAVES + w]);
    }
    agg[tile] = CompAgg{f, b};
    if (pk) atomicMax(reinterpret_cast<unsigned *>(&stats[u].peak), pk);
  }
}

__global__ __launch_bounds__(COMP_WG) void k_compress(const float *x, float *out, const CompUtt *__restrict__ tab, int count, int tile_base,
                                                      CompUtt one, CompPlan P, const CompAgg *__restrict__ agg, CompressorStats *stats) {
  __shared__ int seg_f[COMP_SEGS], seg_b[COMP_SEGS], red[2 * COMP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = (int)blockIdx.x + tile_base;
  int u;
  const CompUtt t = comp_find(tab, count, tile, one, &u);
  const int tl = tile - t.tile0;
  if (tl < 0 || (long long)tl * COMP_TILE >= (long long)t.n) return;  // (never: the host's table)
  const int t0 = tl * COMP_TILE, n_here = min(COMP_TILE, t.n - t0), tiles = (t.n + COMP_TILE - 1) / COMP_TILE;
  const float *xs = x + t.src0 + t0;
  float *os = out + t.dst0 + t0;
  const bool vec = ((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(os)) & 15u) == 0;
  const unsigned pk = __hip_atomic_load(reinterpret_cast<unsigned *>(&stats[u].peak), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (uniform)
  const bool engaged = pk != 0;
  if (tl == 0 && tid == 0) {  // the one writer of these two
    stats[u].engaged = engaged ? 1 : 0;
    if (!engaged) stats[u].max_over = 0;
  }
  float xv[COMP_ROUNDS][COMP_VEC];
#pragma unroll
  for (int r = 0; r < COMP_ROUNDS; ++r) comp_load(xs, r * COMP_ROUND + COMP_VEC * tid, n_here, vec, xv[r]);
  if (!engaged) {  // an all-zero utterance: delivered unchanged
    if (os != xs) {
#pragma unroll
      for (int r = 0; r < COMP_ROUNDS; ++r)
#pragma unroll
        for (int c = 0; c < COMP_VEC; ++c) {
          const int j = r * COMP_ROUND + COMP_VEC * tid + c;
          if (comp_valid(j, n_here)) os[j] = xv[r][c];
        }
    }
    return;
  }
  // the carries: tile tl - 1 - d forwards, tl + 1 + d backwards, d strided over the lanes
  int cin = COMP_L_FLOOR, din = COMP_L_FLOOR;
  {
    const CompAgg *au = agg + t.tile0;
    const int nf = min(tl, comp_reach(P.rho)), nb = min(tiles - 1 - tl, comp_reach(P.alpha));
    for (int d = tid; d < nf; d += COMP_WG) cin = max(cin, comp_carry_term(au[tl - 1 - d].fwd, d, P.rho));
    for (int d = tid; d < nb; d += COMP_WG) din = max(din, comp_carry_term(au[tl + 1 + d].bwd, d, P.alpha));
    cin = wave_max(cin);
    din = wave_max(din);
    if (lane == 0) {
      red[wave] = cin;
      red[COMP_WAVES + wave] = din;
    }
  }
  // the scans inside the lane and across the wave
  int pf[COMP_ROUNDS][COMP_VEC], sb[COMP_ROUNDS][COMP_VEC];
#pragma unroll
  for (int r = 0; r < COMP_ROUNDS; ++r) {
    const int j0 = r * COMP_ROUND + COMP_VEC * tid;
    int run = COMP_NEG;
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) {
      const int l = comp_lvl(comp_abs_bits(xv[r][c]));
      if (comp_valid(j0 + c, n_here)) run = max(run, l + (j0 + c) * P.rho);
      pf[r][c] = run;
    }
    int inc = run;  // inclusive across the lanes, ascending
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_up(inc, s, 64);
      if (lane >= s) inc = max(inc, o);
    }
    int exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = COMP_NEG;
    if (lane == 63) seg_f[r * COMP_WAVES + wave] = inc;
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) pf[r][c] = max(pf[r][c], exc);
    run = COMP_NEG;
#pragma unroll
    for (int c = COMP_VEC - 1; c >= 0; --c) {
      const int l = comp_lvl(comp_abs_bits(xv[r][c]));
      if (comp_valid(j0 + c, n_here)) run = max(run, l - (j0 + c) * P.alpha);
      sb[r][c] = run;
    }
    inc = run;  // inclusive across the lanes, descending
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int o = __shfl_down(inc, s, 64);
      if (lane + s < 64) inc = max(inc, o);
    }
    exc = __shfl_down(inc, 1, 64);
    if (lane == 63) exc = COMP_NEG;
    if (lane == 0) seg_b[r * COMP_WAVES + wave] = inc;
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) sb[r][c] = max(sb[r][c], exc);
  }
  __syncthreads();
  cin = max(max(red[0], red[1]), max(red[2], red[3]));
  din = max(max(red[COMP_WAVES], red[COMP_WAVES + 1]), max(red[COMP_WAVES + 2], red[COMP_WAVES + 3]));
  static_assert(COMP_WAVES == 4, "the carries' reduction reads four partials");
  // across the segments, the carries, the gain
  const int PT = comp_lvl(pk) + P.T;
  int cnt = 0, mo = COMP_NEG;
#pragma unroll
  for (int r = 0; r < COMP_ROUNDS; ++r) {
    const int seg = r * COMP_WAVES + wave, j0 = r * COMP_ROUND + COMP_VEC * tid;
    int ex_f = COMP_NEG, ex_b = COMP_NEG;
    for (int k = 0; k < seg; ++k) ex_f = max(ex_f, seg_f[k]);
    for (int k = seg + 1; k < COMP_SEGS; ++k) ex_b = max(ex_b, seg_b[k]);
    float y[COMP_VEC];
#pragma unroll
    for (int c = 0; c < COMP_VEC; ++c) {
      const int j = j0 + c;
      y[c] = 0.f;
      if (!comp_valid(j, n_here)) continue;
      const int e_f = max(max(pf[r][c], ex_f) - j * P.rho, cin - (j + 1) * P.rho);
      const int e_b = max(max(sb[r][c], ex_b) + j * P.alpha, din - (COMP_TILE - j) * P.alpha);
      int o;
      float rr;
      y[c] = comp_sample(xv[r][c], max(e_f, e_b), PT, P, &o, &rr);
      mo = max(mo, o);
      cnt += rr < 0.0f;
    }
    if (vec && j0 + COMP_VEC <= n_here) {
      *reinterpret_cast<float4 *>(os + j0) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int c = 0; c < COMP_VEC; ++c)
        if (comp_valid(j0 + c, n_here)) os[j0 + c] = y[c];
    }
  }
  mo = wave_max(mo);
  for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
  __syncthreads();  // (every lane has read the carries' partials)
  if (lane == 0) {
    red[wave] = mo;
    red[COMP_WAVES + wave] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    mo = max(max(red[0], red[1]), max(red[2], red[3]));
    cnt = (red[COMP_WAVES] + red[COMP_WAVES + 1]) + (red[COMP_WAVES + 2] + red[COMP_WAVES + 3]);
    if (cnt > 0) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[u].compressed), (unsigned long long)cnt);
    atomicMax(&stats[u].max_over, mo);
  }
}

}  // namespace

void launch_compress(const float *x, float *out, const CompUtt *tab_dev, int count, int tile_base, int n_tiles, const CompUtt &one,
                     const CompPlan &plan, CompAgg *agg, CompressorStats *stats, hipStream_t s) {
  if (count <= 0 || n_tiles <= 0) return;
  if (plan.alpha < 1 || plan.alpha > COMP_SLOPE_MAX || plan.rho < 1 || plan.rho > COMP_SLOPE_MAX || plan.W < 0 || !agg || !stats)
    fail(XDTTS_ERR_BAD_ARG, "compressor: slopes %d / %d, knee %d do not fit the kernel", plan.alpha, plan.rho, plan.W);
  hipLaunchKernelGGL(k_comp_init, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, count, stats);
  hipLaunchKernelGGL(k_comp_tiles, dim3((unsigned)n_tiles), dim3(COMP_WG), 0, s, x, tab_dev, count, tile_base, one, plan, agg, stats);
  hipLaunchKernelGGL(k_compress, dim3((unsigned)n_tiles), dim3(COMP_WG), 0, s, x, out, tab_dev, count, tile_base, one, plan, agg, stats);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
