// Stand-alone driver of xd-tts_amd/csrc/resample_plan.h (plain g++, no HIP, no library): the rate rule, the plan, the taps, and
// the phase-major table walked exactly as k_resample walks it -- block base in 64 bits, the staged window, one row per
// output -- with every index bounds-checked, against the definition y[m] = sum x[n] h[m M - n L].  Built with
// -fsanitize=address,undefined by tests/test_resample_cpu.py.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_plan.h"

using namespace xdtts;

#define REQUIRE(c)                                             \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                \
    }                                                          \
  } while (0)

// One workgroup of k_resample on the host: outputs m0 .. m0 + BLOCK of an utterance x[0 .. N).  Returns false on an index that
// the kernel must never form.
static bool block(const ResampleTable &t, const std::vector<float> &x, long long m0, long long n_out, std::vector<double> &y) {
  const long long N = (long long)x.size();
  std::vector<float> xs((size_t)RESAMPLE_WINDOW, 0.f);
  const long long p0 = m0 * t.M, q0 = p0 / t.L;
  const int r0 = (int)(p0 - q0 * t.L);
  const int span = (r0 + (RESAMPLE_BLOCK - 1) * t.M) / t.L + t.T4;
  if (span > RESAMPLE_WINDOW) return false;
  const long long nlo = q0 + t.Jn - (t.T4 - 1);
  for (int i = 0; i < span; ++i) {
    const long long n = nlo + i;
    xs.at((size_t)i) = (n >= 0 && n < N) ? x.at((size_t)n) : 0.f;
  }
  for (int tid = 0; tid < RESAMPLE_BLOCK; ++tid) {
    const long long m = m0 + tid;
    if (m >= n_out) break;
    const int pr = r0 + tid * t.M, dq = pr / t.L, r = pr - dq * t.L;
    if (dq + t.T4 - 1 >= span) return false;
    double acc = 0;
    for (int i = 0; i < t.T4; ++i) acc += (double)xs.at((size_t)(dq + t.T4 - 1 - i)) * (double)t.rows.at((size_t)r * t.T4 + i);
    y.at((size_t)m) = acc;
  }
  return true;
}

int main() {
  // the rate rule
  const long long bad[] = {7999, 96001, 22051, 0, -1, 8003, 1LL << 33};
  for (long long q : bad) {
    ResamplePlan p;
    REQUIRE(!resample_check(q, &p).empty());
  }
  ResamplePlan id;
  REQUIRE(resample_check(22050, &id).empty() && id.identity && id.L == 1 && id.M == 1 && id.H == 0);
  REQUIRE(resample_n_out(id, 12345) == 12345);
  std::vector<float> one;
  resample_taps(id, one);
  REQUIRE(one.size() == 1 && one[0] == 1.0f);

  const int rates[] = {8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 88200, 96000};
  const int Ls[] = {160, 1, 80, 320, 160, 640, 2, 320, 4, 640}, Ms[] = {441, 2, 147, 441, 147, 441, 1, 147, 1, 147};
  unsigned seed = 12345;
  for (int c = 0; c < 10; ++c) {
    ResamplePlan p;
    REQUIRE(resample_check(rates[c], &p).empty());
    REQUIRE(!p.identity && p.L == Ls[c] && p.M == Ms[c] && p.W == (p.L > p.M ? p.L : p.M) && p.H == 32 * p.W);
    REQUIRE(resample_n_out(p, 0) == 0 && resample_n_out(p, 1) == (size_t)((p.L + p.M - 1) / p.M));
    REQUIRE(resample_n_out(p, (size_t)1 << 30) == (size_t)((((unsigned long long)1 << 30) * p.L + p.M - 1) / p.M));
    REQUIRE(resample_n_out(p, ~(size_t)0 / 1024) >= ~(size_t)0 / 1024 / 3);  // no overflow on the way
    std::vector<float> h;
    resample_taps(p, h);
    REQUIRE(h.size() == (size_t)2 * p.H + 1);
    for (int k = 0; k <= p.H; ++k) REQUIRE(h[(size_t)(p.H + k)] == h[(size_t)(p.H - k)]);
    REQUIRE(std::fabs(h[(size_t)p.H] - (float)((double)p.L / p.W * RESAMPLE_RHO)) < 1e-7f && h[0] != 0.f && std::fabs(h[0]) < 1e-4f);
    ResampleTable t;
    resample_table(p, h, t);
    REQUIRE(t.rate == rates[c] && t.T4 % 4 == 0 && t.rows.size() == (size_t)p.L * t.T4 && resample_window(t) <= RESAMPLE_WINDOW);
    // every tap sits in the table exactly once
    double sum_h = 0, sum_t = 0;
    size_t nz_h = 0, nz_t = 0;
    for (float v : h) sum_h += v, nz_h += v != 0.f;
    for (float v : t.rows) sum_t += v, nz_t += v != 0.f;
    REQUIRE(nz_h == nz_t && std::fabs(sum_h - sum_t) < 1e-9 * (double)p.L);
    // the kernel's walk against the definition, short inputs and block boundaries
    const size_t Ns[] = {1, 2, 255, 256, 257, 885, 4097};
    for (size_t N : Ns) {
      std::vector<float> x(N);
      for (float &v : x) {
        seed = seed * 1664525u + 1013904223u;
        v = (float)(seed >> 8) * (2.0f / 16777216.0f) - 1.0f;
      }
      const long long n_out = (long long)resample_n_out(p, N);
      std::vector<double> y((size_t)n_out, 0.0);
      for (long long m0 = 0; m0 < n_out; m0 += RESAMPLE_BLOCK) REQUIRE(block(t, x, m0, n_out, y));
      for (long long m = 0; m < n_out; ++m) {
        double ref = 0, mag = 0;
        const long long n_first = std::max(0LL, (m * p.M - p.H) / p.L - 1), n_last = std::min((long long)N - 1, (m * p.M + p.H) / p.L + 1);
        for (long long n = n_first; n <= n_last; ++n) {  // (a superset of the taps' reach; the test below decides)
          const long long k = m * p.M - n * p.L;
          if (k < -(long long)p.H || k > (long long)p.H) continue;
          ref += (double)x[(size_t)n] * (double)h[(size_t)(k + p.H)];
          mag += std::fabs((double)x[(size_t)n] * (double)h[(size_t)(k + p.H)]);
        }
        REQUIRE(std::fabs(ref - y[(size_t)m]) <= 1e-12 * (mag + 1.0));
      }
    }
    // a block whose m M is past 2^32: the indices stay inside a window placed by 64-bit arithmetic
    {
      const long long m0 = (((long long)1 << 33) / p.M / RESAMPLE_BLOCK + 1) * RESAMPLE_BLOCK;
      const long long p0 = m0 * p.M, q0 = p0 / p.L;
      REQUIRE(p0 > ((long long)1 << 32) && q0 * p.L <= p0 && p0 - q0 * p.L < p.L);
    }
  }
  std::printf("ok\n");
  return 0;
}
