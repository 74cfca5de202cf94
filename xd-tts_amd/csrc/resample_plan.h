// resample_plan.h -- the host arithmetic of the output-rate stage (xdtts_griffinlim_set_output_rate, include/xdtts.h): the rate
// rule, L, M, H and N', the taps, and the phase-major table the device reads (resample.hip: k_resample).  Every caller -- the
// two host entries, the parity hooks, the request paths -- gets them here.
// Plain host C++, no HIP and none of the library's headers: tests/resample_plan_test.cpp drives it with plain g++.
// The taps are computed in double and rounded once to float; all index arithmetic is integer.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace xdtts {

constexpr int RESAMPLE_RATE_IN = 22050;  // XDTTS_SAMPLE_RATE: what the vocoder's loop produces
constexpr int RESAMPLE_RATE_MIN = 8000, RESAMPLE_RATE_MAX = 96000;
constexpr int RESAMPLE_L_MAX = 640;
constexpr int RESAMPLE_ZEROS = 32;       // H = 32 W: zero crossings of the sinc on either side
constexpr double RESAMPLE_RHO = 0.9, RESAMPLE_BETA = 10.0;
constexpr int RESAMPLE_BLOCK = 256;      // consecutive outputs of one utterance per workgroup
constexpr int RESAMPLE_WINDOW = 1024;    // floats of LDS for a workgroup's input window (resample_window() of every supported rate fits)

// Q = rate_out, R = 22050, g = gcd(Q, R): L = Q / g, M = R / g, W = max(L, M), H = 32 W.  The identity (Q == R) has no filter:
// L = M = W = 1, H = 0, one tap of 1.
struct ResamplePlan {
  int rate = RESAMPLE_RATE_IN;
  int L = 1, M = 1, W = 1, H = 0;
  bool identity = true;
};

// "" if the rate is supported (plan filled in), else the message: it names the rate and the rule.
inline std::string resample_check(long long rate, ResamplePlan *plan) {
  char msg[200];
  if (rate < RESAMPLE_RATE_MIN || rate > RESAMPLE_RATE_MAX) {
    std::snprintf(msg, sizeof msg, "output rate %lld is not in [%d, %d]", rate, RESAMPLE_RATE_MIN, RESAMPLE_RATE_MAX);
    return msg;
  }
  int a = (int)rate, b = RESAMPLE_RATE_IN;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  const int L = (int)rate / a, M = RESAMPLE_RATE_IN / a;
  if (rate != RESAMPLE_RATE_IN && L > RESAMPLE_L_MAX) {
    std::snprintf(msg, sizeof msg, "output rate %lld: L = rate / gcd(rate, %d) = %d is above %d", rate, RESAMPLE_RATE_IN, L, RESAMPLE_L_MAX);
    return msg;
  }
  if (plan) {
    ResamplePlan p;
    p.rate = (int)rate;
    p.identity = rate == RESAMPLE_RATE_IN;
    if (!p.identity) {
      p.L = L;
      p.M = M;
      p.W = L > M ? L : M;
      p.H = RESAMPLE_ZEROS * p.W;
    }
    *plan = p;
  }
  return "";
}

// N' = ceil(N L / M), without forming N L
inline size_t resample_n_out(const ResamplePlan &p, size_t n) {
  const size_t M = (size_t)p.M, L = (size_t)p.L;
  return (n / M) * L + ((n % M) * L + M - 1) / M;
}

inline double resample_i0(double x) {  // modified Bessel function of the first kind, order 0: sum ((x/2)^k / k!)^2
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

// h[k + H], k = -H .. H:  (L / W) rho sinc(rho k / W) I0(beta sqrt(1 - (k / H)^2)) / I0(beta), in double, rounded once.
// Computed for k >= 0 and mirrored: exactly symmetric.
inline void resample_taps(const ResamplePlan &p, std::vector<float> &h) {
  if (p.identity) {
    h.assign(1, 1.0f);
    return;
  }
  const double PI = 3.14159265358979323846;
  const int H = p.H;
  h.assign((size_t)2 * H + 1, 0.f);
  const double i0b = resample_i0(RESAMPLE_BETA), scale = (double)p.L / (double)p.W * RESAMPLE_RHO;
  for (int k = 0; k <= H; ++k) {
    const double x = RESAMPLE_RHO * (double)k / (double)p.W;
    const double s = k == 0 ? 1.0 : std::sin(PI * x) / (PI * x);
    const double u = (double)k / (double)H;
    const double w = resample_i0(RESAMPLE_BETA * std::sqrt(1.0 - u * u)) / i0b;
    h[(size_t)(H + k)] = h[(size_t)(H - k)] = (float)(scale * s * w);
  }
}

// The table the device reads.  With m M = q L + r (0 <= r < L) the taps that meet output m are k = r + j L, j = q - n, for
// -Jn <= j <= Jp, Jp = floor(H / L), Jn = floor((H + L - 1) / L).  Row r holds them in the order of DESCENDING n, so that
// entry t of row r multiplies x[q + Jn - t]:  rows[r][t] = h[r + (t - Jn) L] where |r + (t - Jn) L| <= H, else 0; T = Jp + Jn + 1
// entries, zero-padded to T4, a multiple of 4 (a lane reads its row with 128-bit loads).
struct ResampleTable {
  int rate = 0, L = 1, M = 1, Jn = 0, T4 = 0;
  std::vector<float> rows;  // [L][T4]
};

inline void resample_table(const ResamplePlan &p, const std::vector<float> &h, ResampleTable &t) {
  t = ResampleTable();
  t.rate = p.rate;
  t.L = p.L;
  t.M = p.M;
  const int Jp = p.H / p.L;
  t.Jn = (p.H + p.L - 1) / p.L;
  t.T4 = (Jp + t.Jn + 1 + 3) / 4 * 4;
  t.rows.assign((size_t)p.L * (size_t)t.T4, 0.f);
  for (int r = 0; r < p.L; ++r)
    for (int i = 0; i < t.T4; ++i) {
      const long long k = (long long)r + (long long)(i - t.Jn) * p.L;
      if (k >= -(long long)p.H && k <= (long long)p.H) t.rows[(size_t)r * t.T4 + i] = h[(size_t)(k + p.H)];
    }
}

// Input samples a workgroup of RESAMPLE_BLOCK consecutive outputs stages at most: the q of its outputs span
// floor((L - 1 + (BLOCK - 1) M) / L) + 1 values, and each output reads T4 samples below its q + Jn.
inline int resample_window(const ResampleTable &t) { return (t.L - 1 + (RESAMPLE_BLOCK - 1) * t.M) / t.L + t.T4; }

}  // namespace xdtts
