// silence.hip -- the silence stage, the last of the delivery chain: edge silence trimmed, pauses capped, a fade either side of
// every cut (the definition: include/xdtts.h; the integers, the per-window rules and the host walk: silence_plan.h).  Three
// launches for the single call, the ragged batch and the stage alone:
//   k_sil_peaks   per tile of SIL_TILE samples of ONE utterance: the peak |x| of every 5 ms window that starts in the tile (a
//                 wave per window, its lanes striding over the samples, on past the tile's end where the window runs on), and
//                 the tile's peak
//   k_sil_plan    per utterance: P from the tiles' peaks, then three passes over the windows in chunks of SIL_PLAN_WG lanes with
//                 integer carries -- the nearest non-candidate in front, the nearest one behind and with both the run's length
//                 and a[w], the nearest sound window behind, the nearest in front, keep[w], the exclusive prefix sum of the kept
//                 lengths -- into a per-window output offset (SIL_DROPPED where dropped) and the stats
//   k_sil_gather  per tile: every kept window that starts in it goes to its offset in the utterance's output row, faded where
//                 a neighbour is dropped
// The output's length is decided on the device: the host does not wait between the launches, and reads n_out from the stats
// behind the audio.  Integer maxima and sums and one fp32 comparison per window: out [0, n_out) and stats are functions of
// (the utterance, the plan) alone -- a ragged launch has the bits of the single call and the device those of
// silence_reference().  No atomics, no libm.
#include "kernels.h"

namespace xdtts {

namespace {

static_assert(sizeof(SilenceStats) == 32 && sizeof(xdtts_silence_stats) == 32 && sizeof(Silence) == 24 && sizeof(xdtts_silence) == 24,
              "Silence / SilenceStats are xdtts_silence / xdtts_silence_stats");
static_assert(sizeof(SilUtt) == 32, "the record of the table");

// the utterance that owns tile `tile` of the table's numbering (ascending tile0; the index stays in [0, count) whatever the table holds)
__device__ __forceinline__ SilUtt sil_find(const SilUtt *tab, int count, int tile, const SilUtt &one) {
  if (!tab) return one;
  int lo = 0, hi = count - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return tab[lo];
}

__device__ __forceinline__ int wave_max(int v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
  for (int s = 32; s > 0; s >>= 1) v += (unsigned)__shfl_xor((int)v, s, 64);
  return v;
}

// Inclusive scans over the lanes of k_sil_plan's workgroup, ascending; red: SIL_PLAN_WAVES ints of LDS; *total: the whole
// workgroup's.  Every lane of the workgroup calls them.
__device__ __forceinline__ int wg_scan_max(int v, int *red, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_up(v, s, 64);
    if (lane >= s) v = max(v, o);
  }
  __syncthreads();  // (every lane has read the partials of the scan before)
  if (lane == 63) red[wave] = v;
  __syncthreads();
  int tot = red[0];
#pragma unroll
  for (int k = 0; k < SIL_PLAN_WAVES; ++k) {
    if (k < wave) v = max(v, red[k]);
    tot = max(tot, red[k]);
  }
  *total = tot;
  return v;
}
__device__ __forceinline__ int wg_scan_sum(int v, int *red, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int o = __shfl_up(v, s, 64);
    if (lane >= s) v += o;
  }
  __syncthreads();
  if (lane == 63) red[wave] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int k = 0; k < SIL_PLAN_WAVES; ++k) {
    if (k < wave) v += red[k];
    tot += red[k];
  }
  *total = tot;
  return v;
}

__global__ __launch_bounds__(SIL_WG) void k_sil_peaks(const float *__restrict__ x, const SilUtt *__restrict__ tab, int count, int tile_base,
                                                      SilUtt one, SilPlan P, float *__restrict__ pw, float *__restrict__ tpk) {
  __shared__ int red[SIL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = (int)blockIdx.x + tile_base;
  const SilUtt t = sil_find(tab, count, tile, one);
  const int tl = tile - t.tile0;
  if (tl < 0 || (long long)tl * SIL_TILE >= (long long)t.n) return;  // (never: the host's table)
  const int t0 = tl * SIL_TILE, nw = (t.n + P.W - 1) / P.W;
  const int w0 = sil_tile_win0(t0, P.W), w1 = sil_tile_win1(t0, t.n, P.W);
  const float *xs = x + t.src0;
  unsigned top = 0;
  for (int w = w0 + wave; w < w1; w += SIL_WAVES) {  // (w1 <= nw: every sample read lies inside the utterance)
    const int len = sil_win_len(w, nw, t.n, P.W);
    const float *xw = xs + (long long)w * P.W;
    unsigned pk = 0;
    for (int k = lane; k < len; k += 64) pk = max(pk, sil_abs_bits(xw[k]));
    pk = (unsigned)wave_max((int)pk);  // (|x| bits are below 2^31: the signed order is theirs)
    if (lane == 0) pw[t.win0 + w] = sil_float(pk);
    top = max(top, pk);
  }
  if (lane == 0) red[wave] = (int)top;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < SIL_WAVES; ++v) top = max(top, (unsigned)red[v]);
    tpk[tile] = sil_float(top);
  }
}

__global__ __launch_bounds__(SIL_PLAN_WG) void k_sil_plan(const SilUtt *__restrict__ tab, SilUtt one, SilPlan P, const float *__restrict__ pw_all,
                                                          const float *__restrict__ tpk, int *__restrict__ wl_all, int *__restrict__ wr_all,
                                                          int *__restrict__ woff_all, SilenceStats *__restrict__ stats) {
  __shared__ int red[SIL_PLAN_WAVES], sk[SIL_PLAN_WG], acc[4 * SIL_PLAN_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, u = (int)blockIdx.x;
  const SilUtt t = tab ? tab[u] : one;
  const int n = t.n, nw = (n + P.W - 1) / P.W, tiles = (n + SIL_TILE - 1) / SIL_TILE;
  const float *pw = pw_all + t.win0;
  int *wl = wl_all + t.win0, *wr = wr_all + t.win0, *woff = woff_all + t.win0;
  // P: the largest of the tiles' peaks
  int top = 0;
  for (int k = tid; k < tiles; k += SIL_PLAN_WG) top = max(top, (int)sil_abs_bits(tpk[t.tile0 + k]));
  {
    int tot;
    wg_scan_max(top, red, &tot);
    top = tot;
  }
  const float Pk = sil_float((unsigned)top), thr = sil_threshold(Pk, P.tfac);
  const int need = P.min_w > 1 ? P.min_w : 1;
  // 1 forwards: the nearest window at or in front of w that is no candidate
  int carry = -1;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG) {
    const int w = c0 + tid;
    const bool valid = w < nw;
    const bool a0 = valid && sil_candidate(pw[w], thr);
    int tot;
    const int L0 = max(wg_scan_max(valid && !a0 ? w : -1, red, &tot), carry);
    carry = max(carry, tot);
    if (valid) wl[w] = L0;
  }
  __syncthreads();  // (wl: written by one lane, read by another in pass 2)
  // 2 backwards, on the mirrored index m = nw - 1 - w: the nearest non-candidate behind, a[w], the nearest sound window behind
  int carry0 = -1, carry1 = -1;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG) {
    const int m = c0 + tid, w = nw - 1 - m;
    const bool valid = m < nw;
    const bool a0 = valid && sil_candidate(pw[w], thr);
    int tot;
    const int R0m = max(wg_scan_max(valid && !a0 ? m : -1, red, &tot), carry0);
    carry0 = max(carry0, tot);
    const bool a = a0 && (nw - 1 - R0m) - wl[w] - 1 >= need;
    const int rm = max(wg_scan_max(a ? m : -1, red, &tot), carry1);
    carry1 = max(carry1, tot);
    if (valid) {
      wr[w] = nw - 1 - rm;
      wl[w] = a ? 1 : 0;
    }
  }
  __syncthreads();
  // 3 forwards: the nearest sound window in front, keep, the offsets, the stats
  int l_carry = -1, at = 0, prev_keep = 0;
  unsigned cut[3] = {0u, 0u, 0u}, cuts = 0u;
  for (int c0 = 0; c0 < nw; c0 += SIL_PLAN_WG) {
    const int w = c0 + tid;
    const bool valid = w < nw;
    const bool a = valid && wl[w] != 0;
    int tot;
    const int l = max(wg_scan_max(a ? w : -1, red, &tot), l_carry);
    l_carry = max(l_carry, tot);
    const int r = valid ? wr[w] : nw, len = valid ? sil_win_len(w, nw, n, P.W) : 0;
    const bool keep = valid && sil_keep_rule(w, a, l, r, nw, P);
    const int inc = wg_scan_sum(keep ? len : 0, red, &tot);
    if (valid) woff[w] = keep ? at + inc - len : SIL_DROPPED;
    at += tot;
    if (valid && !keep) cut[sil_cut_kind(l, r, nw)] += (unsigned)len;
    sk[tid] = keep ? 1 : 0;
    __syncthreads();
    const int before = tid > 0 ? sk[tid - 1] : prev_keep;
    if (valid && w > 0 && before != (keep ? 1 : 0)) ++cuts;
    prev_keep = sk[SIL_PLAN_WG - 1];
    // (sk is written again behind the two scans of the next chunk, each of which synchronises first)
  }
  const unsigned s0 = wave_sum(cut[0]), s1 = wave_sum(cut[1]), s2 = wave_sum(cut[2]), s3 = wave_sum(cuts);
  if (lane == 0) {
    acc[wave] = (int)s0;
    acc[SIL_PLAN_WAVES + wave] = (int)s1;
    acc[2 * SIL_PLAN_WAVES + wave] = (int)s2;
    acc[3 * SIL_PLAN_WAVES + wave] = (int)s3;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int q = 0; q < SIL_PLAN_WAVES; ++q) v[k] += (unsigned)acc[k * SIL_PLAN_WAVES + q];
    stats[u] = SilenceStats{(uint32_t)n, (uint32_t)at, v[0], v[1], v[2], v[3], Pk, l_carry >= 0 ? 1u : 0u};
  }
}

__global__ __launch_bounds__(SIL_WG) void k_sil_gather(const float *__restrict__ x, float *__restrict__ out, const SilUtt *__restrict__ tab, int count,
                                                       int tile_base, SilUtt one, SilPlan P, const float *__restrict__ T,
                                                       const int *__restrict__ woff_all) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = (int)blockIdx.x + tile_base;
  const SilUtt t = sil_find(tab, count, tile, one);
  const int tl = tile - t.tile0;
  if (tl < 0 || (long long)tl * SIL_TILE >= (long long)t.n) return;  // (never: the host's table)
  const int t0 = tl * SIL_TILE, nw = (t.n + P.W - 1) / P.W;
  const int w0 = sil_tile_win0(t0, P.W), w1 = sil_tile_win1(t0, t.n, P.W);
  const int *woff = woff_all + t.win0;
  for (int w = w0 + wave; w < w1; w += SIL_WAVES) {
    const int off = woff[w];  // (uniform over the wave)
    if (off == SIL_DROPPED) continue;
    const int len = sil_win_len(w, nw, t.n, P.W);
    const bool fin = w > 0 && woff[w - 1] == SIL_DROPPED, fout = w < nw - 1 && woff[w + 1] == SIL_DROPPED;
    const float *xw = x + t.src0 + (long long)w * P.W;
    float *ow = out + t.dst0 + off;  // (off + len <= n_out <= n: inside the utterance's row)
    const int len4 = ((reinterpret_cast<uintptr_t>(xw) | reinterpret_cast<uintptr_t>(ow)) & 15u) == 0 ? len & ~3 : 0;
    for (int k = 4 * lane; k < len4; k += 256) {
      const float4 q = *reinterpret_cast<const float4 *>(xw + k);
      *reinterpret_cast<float4 *>(ow + k) = make_float4(sil_sample(q.x, k, len, fin, fout, P.fade, T), sil_sample(q.y, k + 1, len, fin, fout, P.fade, T),
                                                        sil_sample(q.z, k + 2, len, fin, fout, P.fade, T), sil_sample(q.w, k + 3, len, fin, fout, P.fade, T));
    }
    for (int k = len4 + lane; k < len; k += 64) ow[k] = sil_sample(xw[k], k, len, fin, fout, P.fade, T);
  }
}

}  // namespace

void launch_silence(const float *x, float *out, const SilUtt *tab_dev, int count, int tile_base, int n_tiles, const SilUtt &one,
                    const SilPlan &plan, const float *fade_tab, const SilBufs &b, SilenceStats *stats, hipStream_t s) {
  if (count <= 0 || n_tiles <= 0) return;
  if (plan.W < SIL_W_MIN || plan.W > SIL_W_MAX || plan.fade < 0 || plan.fade > plan.W / 2 || (plan.fade > 0 && !fade_tab) || plan.min_w < 0 ||
      plan.lead_w < 0 || plan.trail_w < 0 || plan.pause_w < 0 || !b.pw || !b.tpk || !b.wl || !b.wr || !b.woff || !stats || x == out)
    fail(XDTTS_ERR_BAD_ARG, "silence: window %d, fade %d do not fit the kernel", plan.W, plan.fade);
  hipLaunchKernelGGL(k_sil_peaks, dim3((unsigned)n_tiles), dim3(SIL_WG), 0, s, x, tab_dev, count, tile_base, one, plan, b.pw, b.tpk);
  hipLaunchKernelGGL(k_sil_plan, dim3((unsigned)count), dim3(SIL_PLAN_WG), 0, s, tab_dev, one, plan, b.pw, b.tpk, b.wl, b.wr, b.woff, stats);
  hipLaunchKernelGGL(k_sil_gather, dim3((unsigned)n_tiles), dim3(SIL_WG), 0, s, x, out, tab_dev, count, tile_base, one, plan, fade_tab, b.woff);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
