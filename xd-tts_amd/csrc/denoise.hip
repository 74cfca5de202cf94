// denoise.hip -- the clean-up stage of the magnitude chain (xdtts_denoise, include/xdtts.h; the host arithmetic and the index
// functions: denoise_plan.h): spectral subtraction against a per-bin noise estimate with a spectral floor, and a tone curve.
//   k_noise_profile : per utterance and bin, the rank-th smallest key over the utterance's frames -- a radix select, eight bits
//                     a pass from the top, on integer LDS counters.  Counts are integers: no order of arrival changes a bit.
//   k_denoise       : the pointwise part, a wave per row, every operation rounded to fp32 on its own (__f*_rn: nothing fuses);
//                     the floored cells are counted with integer adds.
// One kernel each serves the single call (the record travels as a kernel argument) and the ragged batch (a table in device
// memory): a cell leaves either with the same bits.  Subnormal inputs are kept (the default of the compilation); nothing here
// relies on it.
#include "kernels.h"

#pragma clang fp contract(off)  // (__fmul_rn and __fsub_rn are plain operators in this toolchain: nothing in this file may fuse)

namespace xdtts {

namespace {

constexpr int NB = DENOISE_NB;
constexpr int CNT_STRIDE = 257;  // 256 buckets of a bin, skewed by one bank

// Workgroup b: strip b % 33 of utterance b / 33 (tab[u], or `one` where tab == nullptr: one utterance).  Thread tid: bin
// tid % 16 of the strip, frames tid / 16 + 32 i.  A wave's read of a step is four 64-byte row segments; the lone bin 512 has a
// strip of its own in which 15 of 16 bins are dead (they count nothing and store nothing).
// Pass p (shift 24, 16, 8, 0): the keys that agree with the prefix found so far are counted by their next eight bits; the
// bucket in which the cumulative count passes the remaining rank extends the prefix.  After four passes the prefix is the key.
// The dependent depth is 4 x (F / 32 row reads from L2 + a 32-step scan), independent of the bytes; ONE route for every F.
__global__ __launch_bounds__(DENOISE_LANES) void k_noise_profile(const float *__restrict__ S, const DenoiseUtt *__restrict__ tab, DenoiseUtt one,
                                                                 float *__restrict__ N) {
  __shared__ unsigned cnt[DENOISE_STRIP * CNT_STRIDE];
  __shared__ unsigned part[DENOISE_STRIP][16];
  __shared__ unsigned prefix[DENOISE_STRIP], rem[DENOISE_STRIP];
  const int tid = threadIdx.x, u = denoise_profile_utt((int)blockIdx.x);
  const DenoiseUtt t = tab ? tab[u] : one;
  if (!(t.sub && !t.profiled) || t.F < 1) return;  // (the whole workgroup: its utterance selects nothing)
  const int b = tid % DENOISE_STRIP, bin = denoise_profile_bin((int)blockIdx.x, tid), f0 = denoise_profile_frame0(tid);
  const bool live = bin < NB;
  if (tid < DENOISE_STRIP) {
    prefix[tid] = 0u;
    rem[tid] = (unsigned)min(max(t.rank, 0), t.F - 1);
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < DENOISE_STRIP * CNT_STRIDE; i += DENOISE_LANES) cnt[i] = 0u;
    __syncthreads();
    const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u, pfx = prefix[b];
    unsigned *mine = cnt + b * CNT_STRIDE;
    if (live) {
      int f = f0;
      for (; f + 3 * DENOISE_FSTEP < t.F; f += 4 * DENOISE_FSTEP) {  // four independent reads in flight
        unsigned k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = denoise_key(S[denoise_cell(t.row0, f + j * DENOISE_FSTEP, bin)]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((k[j] & himask) == pfx) atomicAdd(&mine[(k[j] >> shift) & 255u], 1u);
      }
      for (; f < t.F; f += DENOISE_FSTEP) {
        const unsigned k = denoise_key(S[denoise_cell(t.row0, f, bin)]);
        if ((k & himask) == pfx) atomicAdd(&mine[(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid < DENOISE_STRIP * 16) {  // sixteen threads a bin: the sums of sixteen buckets each
      const int b2 = tid >> 4, g = tid & 15;
      unsigned s = 0u;
#pragma unroll
      for (int i = 0; i < 16; ++i) s += cnt[b2 * CNT_STRIDE + 16 * g + i];
      part[b2][g] = s;
    }
    __syncthreads();
    if (tid < DENOISE_STRIP) {  // one thread a bin: the group, then the bucket in it (bounded: a dead bin ends in bucket 255)
      unsigned r = rem[tid], acc = 0u;
      int g = 15;
      bool found = false;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned c = part[tid][i];
        if (!found && acc + c > r) g = i, found = true;
        if (!found) acc += c;
      }
      int j = 15;
      found = false;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned c = cnt[tid * CNT_STRIDE + 16 * g + i];
        if (!found && acc + c > r) j = i, found = true;
        if (!found) acc += c;
      }
      prefix[tid] |= (unsigned)(16 * g + j) << shift;
      rem[tid] = found ? r - acc : 0u;
    }
    __syncthreads();
  }
  if (tid < DENOISE_STRIP && live) N[(size_t)u * NB + (size_t)bin] = __uint_as_float(prefix[tid]);  // (tid < 16: bin = strip * 16 + tid)
}

// Row `jr` of Sout over the concatenated utterances; tab[u] (row0 ascending) or `one`.  With s = S[row][k]:
//   sub : aN = strength * N[k] (N: the profile, or row u of the selected table);  q = aN / s;  d = 1 - q;
//         G = d > gmin ? d : gmin (a NaN d gives gmin);  y = s * G;  a floored cell (G == gmin) is counted
//   tone: y = y * E[tone][k]
// each rounded to fp32 on its own.  Neither: the row is copied.  The wave of an utterance's first row writes the integer
// fields of its stats; `floored` is zeroed by the host in front of the launch and added to once per wave.
__global__ __launch_bounds__(64 * DENOISE_ROWS) void k_denoise(const float *__restrict__ S, float *__restrict__ Sout,
                                                               const DenoiseUtt *__restrict__ tab, int n_utt, DenoiseUtt one, int rows_all,
                                                               const float *__restrict__ Nsel, const float *__restrict__ profile,
                                                               const float *__restrict__ tone, DenoiseStats *__restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = (int)blockIdx.x * DENOISE_ROWS + wave;
  if (row >= rows_all) return;  // (no barrier below: a wave may leave alone)
  const int u = tab ? denoise_row_utt(tab, n_utt, row) : 0;
  const DenoiseUtt t = tab ? tab[u] : one;
  const int j = min(max(row - t.row0, 0), max(t.F, 1) - 1);
  const float *s = S + denoise_cell(t.row0, j, 0);
  float *out = Sout + denoise_cell(t.row0, j, 0);
  const float *N = t.sub ? (t.profiled ? profile : Nsel + (size_t)u * NB) : nullptr;
  const float *E = t.tone >= 0 ? tone + (size_t)t.tone * NB : nullptr;
  unsigned floored = 0u;
#pragma unroll
  for (int r = 0; r <= 8; ++r) {
    const bool mine = r < 8 || lane == 0;
    const int k = denoise_lane_bin(lane, r);
    float y = 0.f;
    bool fl = false;
    if (mine) {
      const float x = s[k];
      y = x;
      if (N) {
        const float aN = __fmul_rn(t.strength, N[k]);
        const float q = __fdiv_rn(aN, x);
        const float d = __fsub_rn(1.0f, q);
        const bool above = d > t.gmin;
        fl = !above;
        y = __fmul_rn(x, above ? d : t.gmin);
      }
      if (E) y = __fmul_rn(y, E[k]);
      out[k] = y;
    }
    floored += (unsigned)__popcll(__ballot(fl));  // (wave-uniform)
  }
  if (lane == 0) {
    if (floored) atomicAdd(&stats[u].floored, floored);
    if (j == 0 && row == t.row0) {
      stats[u].cells = (unsigned)t.F * (unsigned)NB;
      stats[u].rank = (unsigned)t.rank;
      stats[u].profiled = (unsigned)t.profiled;
    }
  }
}

}  // namespace

void launch_noise_profile(const float *S, const DenoiseUtt *tab, int n_utt, const DenoiseUtt &one, float *N, hipStream_t s) {
  if (n_utt <= 0) return;
  hipLaunchKernelGGL(k_noise_profile, dim3((unsigned)n_utt * DENOISE_STRIPS), dim3(DENOISE_LANES), 0, s, S, tab, one, N);
  HIP_CHECK(hipGetLastError());
}

void launch_denoise(const float *S, float *Sout, const DenoiseUtt *tab, int n_utt, const DenoiseUtt &one, int rows_all, const float *Nsel,
                    const float *profile, const float *tone, DenoiseStats *stats, hipStream_t s) {
  if (n_utt <= 0 || rows_all <= 0) return;
  const int nblk = (rows_all + DENOISE_ROWS - 1) / DENOISE_ROWS;
  hipLaunchKernelGGL(k_denoise, dim3(nblk), dim3(64 * DENOISE_ROWS), 0, s, S, Sout, tab, n_utt, one, rows_all, Nsel, profile, tone, stats);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
