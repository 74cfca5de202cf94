// resample.hip -- the output-rate stage behind the Griffin-Lim loop: 22 050 Hz audio -> rate Q by a polyphase windowed-sinc
// filter (the definition: include/xdtts.h; the taps and the table: resample_plan.h).
//   y[m] = sum_n x[n] h[m M - n L],  |m M - n L| <= H,  x = 0 outside [0, N)
// One kernel, k_resample, for the single call and the ragged batch.  A workgroup owns RESAMPLE_BLOCK consecutive outputs of
// ONE utterance, which it finds in a small table (or takes by value: the single call uploads nothing).  It stages the input
// window those outputs read in LDS, zero outside the utterance, so the inner loop carries no bounds test; each lane then
// owns one output: its phase's row of the table (contiguous, 128-bit loads) against a descending run of the window.
// The sum runs over the T4 entries of the row in a fixed order -- four interleaved fmaf chains, combined (a0 + a1) + (a2 + a3)
// -- so an output's bits depend on (Q, m, N) and its utterance's samples alone: batch == single.
// Nothing here crosses workgroups: one barrier behind the staging, no exchange, no atomics.
#include "kernels.h"

namespace xdtts {

namespace {

__global__ __launch_bounds__(RESAMPLE_BLOCK) void k_resample(const float *__restrict__ x, float *__restrict__ y,
                                                            const ResampleUtt *__restrict__ tab, int n_utt, int blk_base,
                                                            ResampleUtt one, const float *__restrict__ rows, int L, int M, int Jn,
                                                            int T4) {
  __shared__ float xs[RESAMPLE_WINDOW];
  const int tid = threadIdx.x;
  ResampleUtt t = one;
  if (tab) {
    const int blk = (int)blockIdx.x + blk_base;
    int lo = 0, hi = n_utt - 1;  // the last utterance with blk0 <= blk (ascending; the index stays in [0, n_utt) whatever the table holds)
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    t = tab[lo];
    t.blk0 -= blk_base;
  }
  const long long m0 = (long long)((int)blockIdx.x - t.blk0) * RESAMPLE_BLOCK;  // the workgroup's first output, within the utterance
  if (m0 < 0 || m0 >= (long long)t.n_out) return;                               // (never: the host's table)
  // m0 M = q0 L + r0 in 64 bits, once per workgroup; everything per lane is 32-bit from there
  const long long p0 = m0 * (long long)M, q0 = p0 / (long long)L;
  const int r0 = (int)(p0 - q0 * (long long)L);
  // the window: x[nlo .. nlo + span), nlo = q0 + Jn - (T4 - 1); the last lane's q is q0 + (r0 + (BLOCK - 1) M) / L
  const int span = min((r0 + (RESAMPLE_BLOCK - 1) * M) / L + T4, RESAMPLE_WINDOW);
  const long long nlo = q0 + (long long)Jn - (long long)(T4 - 1);
  const float *xu = x + t.src0;
  for (int i = tid; i < span; i += RESAMPLE_BLOCK) {
    const long long n = nlo + (long long)i;
    xs[i] = (n >= 0 && n < (long long)t.n) ? xu[n] : 0.f;
  }
  __syncthreads();
  const long long m = m0 + (long long)tid;
  if (m >= (long long)t.n_out) return;
  const int pr = r0 + tid * M, dq = pr / L, r = pr - dq * L;  // m M = (q0 + dq) L + r
  // entry i of row r multiplies x[q0 + dq + Jn - i] = xs[dq + T4 - 1 - i]; dq + T4 - 1 < span
  const float4 *row = reinterpret_cast<const float4 *>(rows + (size_t)r * (size_t)T4);
  const float *xp = xs + min(dq + T4 - 1, RESAMPLE_WINDOW - 1);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int i = 0; i < T4; i += 4) {
    const float4 h = row[i >> 2];
    a0 = fmaf(xp[-i], h.x, a0);
    a1 = fmaf(xp[-i - 1], h.y, a1);
    a2 = fmaf(xp[-i - 2], h.z, a2);
    a3 = fmaf(xp[-i - 3], h.w, a3);
  }
  y[t.dst0 + m] = (a0 + a1) + (a2 + a3);
}

}  // namespace

void launch_resample(const float *x, float *y, const ResampleUtt *tab_dev, int n_utt, int blk_base, int nblk, const ResampleUtt &one,
                     const float *rows_dev, int L, int M, int Jn, int T4, hipStream_t s) {
  if (nblk <= 0) return;
  if (L < 1 || M < 1 || T4 < 4 || (T4 & 3) || (L - 1 + (RESAMPLE_BLOCK - 1) * M) / L + T4 > RESAMPLE_WINDOW)
    fail(XDTTS_ERR_BAD_ARG, "resample: L %d, M %d, %d entries per phase do not fit the kernel's window", L, M, T4);
  hipLaunchKernelGGL(k_resample, dim3((unsigned)nblk), dim3(RESAMPLE_BLOCK), 0, s, x, y, tab_dev, n_utt, blk_base, one, rows_dev, L, M, Jn, T4);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
