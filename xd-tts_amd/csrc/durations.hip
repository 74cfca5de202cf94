// durations.hip -- per-id durations and start marks from the decoder's cumulative attention weights (xdtts_durations_opts,
// include/xdtts.h; the definitions: durations_plan.h).  Two small launches behind a decode, nothing inside it:
//   k_durations        one wave per chunk slot: picks the slot's final row (batched mode: by the parity of the slot's own frame
//                      count), masks the padding, converts to Q16, scans, adds the frames of the utterance's earlier chunks,
//                      stores dur / dur_q16 / start_q16 at the chunk's place in the caller's order
//   k_durations_stats  one wave per utterance: the stats over the Q16 values the first launch wrote
// Ids lie across the wave (id t = lane + 64 r), so every load and store of a row is one contiguous run per instruction; the
// scan is a wave scan per r with a carry, all in 64-bit integers -- its result does not depend on its order.  No atomics, no
// floats in any sum, no LDS, no barrier, no wait on another wave: every loop is bounded by a table field the host clamped.
#include "kernels.h"

namespace xdtts {

namespace {

constexpr int DUR_ROWS = DUR_T_MAX / 64;  // ids per lane

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += shfl_xor_u64(v, m);
  return v;
}
// entry i of the slot list, index and slot kept inside [0, B) whatever the table holds
__device__ __forceinline__ int dur_slot(const int *list, int i, int B) { return min(max(list[min(max(i, 0), B - 1)], 0), B - 1); }
// inclusive scan over the 64 lanes
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = shfl_up_u64(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__global__ __launch_bounds__(64) void k_durations(const float *__restrict__ cum_a, const float *__restrict__ cum_b, int B, int T,
                                                  const int *__restrict__ nframes, const int *__restrict__ n_valid,
                                                  const DurChunk *__restrict__ tab, const int *__restrict__ list, int batched,
                                                  float *__restrict__ dur, uint32_t *__restrict__ dur_q16, uint64_t *__restrict__ start_q16) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= B) return;
  const DurChunk c = tab[j];
  const int nf = max(nframes[j], 0);
  const int nv = min(min(max(n_valid[j], 0), c.n), T);  // never past the ids the host laid out, never past the row
  const float *row = (batched && (nf & 1) ? cum_b : cum_a) + (size_t)j * T;
  // frames of the utterance's earlier chunks: at most the request's chunk count of integers
  uint64_t base = 0;
  const int k = min(max(c.k, 0), B);
  for (int i = lane; i < k; i += 64) base += (uint64_t)max(nframes[dur_slot(list, c.list0 + i, B)], 0);
  base = wave_sum_u64(base) << 16;
  uint64_t carry = 0;
#pragma unroll
  for (int r = 0; r < DUR_ROWS; ++r) {
    if (r * 64 >= nv) break;  // (wave-uniform)
    const int t = lane + 64 * r;
    const bool ok = t < nv;
    const float w = ok ? row[t] : 0.f;
    const uint32_t q = ok ? durations_q16(w) : 0u;
    const uint64_t inc = wave_scan_u64((uint64_t)q, lane);
    if (ok) {
      const size_t at = (size_t)c.out_off + t;
      dur[at] = w;
      dur_q16[at] = q;
      start_q16[at] = base + carry + inc - q;  // exclusive
    }
    carry += shfl_u64(inc, 63);  // the row's total
  }
}

// (value, index) pairs: the smaller value wins, the smaller index among equals -- and the mirror for the maximum
__global__ __launch_bounds__(64) void k_durations_stats(const uint32_t *__restrict__ dur_q16, const int *__restrict__ nframes,
                                                        const DurUtt *__restrict__ utt, const int *__restrict__ list, int n_utt, int B,
                                                        uint32_t lo, uint32_t hi, AlignmentStats *__restrict__ stats) {
  const int u = blockIdx.x, lane = threadIdx.x;
  if (u >= n_utt) return;
  const DurUtt U = utt[u];
  const uint32_t *q = dur_q16 + U.id_off;
  uint64_t sum = 0, frames = 0;
  uint32_t mn = 0xFFFFFFFFu, mni = 0xFFFFFFFFu, mx = 0u, mxi = 0xFFFFFFFFu, below = 0, above = 0;
  for (int i = lane; i < U.n_ids; i += 64) {
    const uint32_t v = q[i];
    sum += v;
    if (v < mn || mni == 0xFFFFFFFFu) mn = v, mni = (uint32_t)i;  // (ascending i: the first of equals stays)
    if (v > mx || mxi == 0xFFFFFFFFu) mx = v, mxi = (uint32_t)i;
    below += v < lo;
    above += v > hi;
  }
  const int nc = min(max(U.n_chunks, 0), B);
  for (int i = lane; i < nc; i += 64) frames += (uint64_t)max(nframes[dur_slot(list, U.list0 + i, B)], 0);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t omn = (uint32_t)__shfl_xor((int)mn, m), omni = (uint32_t)__shfl_xor((int)mni, m);
    const uint32_t omx = (uint32_t)__shfl_xor((int)mx, m), omxi = (uint32_t)__shfl_xor((int)mxi, m);
    if (omni != 0xFFFFFFFFu && (mni == 0xFFFFFFFFu || omn < mn || (omn == mn && omni < mni))) mn = omn, mni = omni;
    if (omxi != 0xFFFFFFFFu && (mxi == 0xFFFFFFFFu || omx > mx || (omx == mx && omxi < mxi))) mx = omx, mxi = omxi;
    below += (uint32_t)__shfl_xor((int)below, m);
    above += (uint32_t)__shfl_xor((int)above, m);
  }
  sum = wave_sum_u64(sum);
  frames = wave_sum_u64(frames);
  if (lane == 0) {
    AlignmentStats s;
    s.sum_q16 = sum;
    s.n_frames = frames;
    s.n_ids = (uint32_t)U.n_ids;
    s.min_q16 = mn;
    s.min_index = mni;
    s.max_q16 = mx;
    s.max_index = mxi;
    s.n_below = below;
    s.n_above = above;
    s.last_q16 = U.n_ids > 0 ? q[U.n_ids - 1] : 0u;
    stats[u] = s;
  }
}

}  // namespace

void launch_durations(const DurationsJob &job, hipStream_t s) {
  if (job.B <= 0 || job.n_utt <= 0) return;
  hipLaunchKernelGGL(k_durations, dim3(job.B), dim3(64), 0, s, job.cum_a, job.cum_b, job.B, job.T, job.nframes, job.n_valid, job.tab,
                     job.list, job.batched, job.dur, job.dur_q16, job.start_q16);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_durations_stats, dim3(job.n_utt), dim3(64), 0, s, job.dur_q16, job.nframes, job.utt, job.list, job.n_utt, job.B,
                     job.lo_q16, job.hi_q16, job.stats);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
