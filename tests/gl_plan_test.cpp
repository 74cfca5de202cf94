// gl_plan_test.cpp -- the vocoder's host arithmetic (xd-tts_amd/csrc/gl_plan.h) on the host alone (no HIP, no GPU): the batch
// packing plan at CU counts, workgroups per CU and forced shapes that no GPU test reaches, and the ragged-rows table.
// Built and run by tests/test_gl_plan_cpu.py; prints "ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>

#include "gl_plan.h"

using namespace xdtts;
using Ints = std::vector<int>;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)  [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static std::string g_case;
static const int HOP = 256;

// (a) what must hold for any plan
static void check_invariants(const Ints &Fu, int n_cu, int per_cu4, int shape, int force) {
  g_case = "n_utt " + std::to_string(Fu.size()) + " F0 " + std::to_string(Fu[0]) + " n_cu " + std::to_string(n_cu) + " per_cu4 " +
           std::to_string(per_cu4) + " shape " + std::to_string(shape) + " force " + std::to_string(force);
  const GlBatchPlan P = gl_batch_plan(Fu, HOP, n_cu, per_cu4, shape, force);
  const int n_utt = (int)Fu.size(), TF = P.TF;
  CHECK(TF == 4 || TF == GLP_TF_MAX);
  CHECK(P.WG == 1 || (P.WG == 2 && per_cu4 >= 2 && TF == 4));
  if (shape == 4 && force == 0) CHECK(TF == 4);
  if (force == 8) CHECK(TF == GLP_TF_MAX && P.WG == 1);
  if (force == 41) CHECK(TF == 4 && P.WG == 1);
  if (force == 42 && per_cu4 >= 2) CHECK(TF == 4 && P.WG == 2);
  Ints fbase(n_utt), abase(n_utt), rides(n_utt, 0);
  for (int u = 0, f = 0, a = 0; u < n_utt; f += Fu[u], a += HOP * (Fu[u] - 1), ++u) fbase[u] = f, abase[u] = a;
  CHECK((int)P.batched.size() == n_utt);
  int seg = 0;
  Ints order;
  for (const GlBatchPlan::Launch &L : P.launches) {
    CHECK(L.seg0 == seg && L.nblk >= 1 && L.nblk <= n_cu * P.WG && !L.utts.empty());
    for (int u : L.utts) {
      CHECK(u >= 0 && u < n_utt && P.batched[u] && ++rides[u] == 1);
      order.push_back(u);
      const int F = Fu[u], nb = (F + TF - 1) / TF;
      CHECK(!(F < 16 || nb > n_cu || F / nb < 3));
      if (TF == 4) {  // the split of the utterance's own call: the reason batch_shape 4 gives the single call's bits
        int tf1 = 0, nb1 = 0;
        CHECK(gl_persistent_plan(F, n_cu, &tf1, &nb1) && tf1 == 4 && nb1 == nb);
      }
      int next = 0;
      for (int b = 0; b < nb; ++b, ++seg) {
        CHECK(seg < (int)P.segs.size());
        const GlSeg &s = P.segs[seg];
        CHECK(s.fbase == fbase[u] && s.abase == abase[u] && s.F == F && s.pad == 0);
        CHECK(s.f0 == next && s.f0 == gl_fstart(b, F, nb) && s.n_own >= 3 && s.n_own <= TF);
        CHECK(s.first == (b == 0) && s.last == (b + 1 == nb));
        next = s.f0 + s.n_own;
      }
      CHECK(next == F);
    }
    CHECK(seg == L.seg0 + L.nblk);
  }
  CHECK(seg == (int)P.segs.size());
  for (int u = 0; u < n_utt; ++u) {
    const int nb = (Fu[u] + TF - 1) / TF;
    CHECK(rides[u] == (P.batched[u] ? 1 : 0));
    CHECK(!P.batched[u] == (Fu[u] < 16 || nb > n_cu || Fu[u] / nb < 3));
    if (!P.batched[u]) order.push_back(u);  // behind the riders, ascending
  }
  CHECK(P.order == order && (int)order.size() == n_utt);
}

// (b) plans recorded from the lambda this header replaced (gl_batch_from_device before the move), run on the CPU
struct Recorded {
  const char *name;
  const Ints *Fu;
  int n_cu, per_cu4, shape, force, TF, WG;
  Ints nblk;
  std::vector<Ints> riders;
  Ints alone;
};
static Ints iota(int a, int b) {  // a .. b
  Ints v(b - a + 1);
  std::iota(v.begin(), v.end(), a);
  return v;
}
static Ints cat(Ints a, const Ints &b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}
static void check_recorded(const Recorded &r) {
  g_case = std::string(r.name) + " n_cu " + std::to_string(r.n_cu) + " per_cu4 " + std::to_string(r.per_cu4) + " shape " + std::to_string(r.shape) +
           " force " + std::to_string(r.force);
  const GlBatchPlan P = gl_batch_plan(*r.Fu, HOP, r.n_cu, r.per_cu4, r.shape, r.force);
  CHECK(P.TF == r.TF && P.WG == r.WG && P.launches.size() == r.nblk.size());
  for (size_t k = 0; k < r.nblk.size(); ++k) CHECK(P.launches[k].nblk == r.nblk[k] && P.launches[k].utts == r.riders[k]);
  Ints alone;
  for (size_t u = 0; u < r.Fu->size(); ++u)
    if (!P.batched[u]) alone.push_back((int)u);
  CHECK(alone == r.alone);
  check_invariants(*r.Fu, r.n_cu, r.per_cu4, r.shape, r.force);
}

static Rows gl_rows(const Ints &counts, size_t cap, const char *too_large) {
  Rows r;
  for (int c : counts) r.add((size_t)c, cap, too_large);
  return r;
}
template <class F>
static std::string thrown(F &&f) {
  try {
    f();
  } catch (const std::length_error &e) {
    return e.what();
  }
  return "(nothing)";
}

int main() {
  static_assert(GLP_TF_MAX == 8 && sizeof(GlSeg) == 32, "the kernel's segment row");
  {  // the single call's split
    int tf = 0, nb = 0;
    CHECK(!gl_persistent_plan(15, 256, &tf, &nb) && gl_persistent_plan(16, 256, &tf, &nb) && tf == 4 && nb == 4);
    CHECK(gl_persistent_plan(1025, 256, &tf, &nb) && tf == 5 && nb == 205 && !gl_persistent_plan(2049, 256, &tf, &nb));
    CHECK(gl_fstart(0, 19, 5) == 0 && gl_fstart(1, 19, 5) == 3 && gl_fstart(5, 19, 5) == 19);
    CHECK(gl_fstart(255, 1 << 24, 256) == 255 * (1 << 16));  // (the product passes 2^31)
  }

  const Ints A = {37, 16, 5, 400, 1100, 19, 2, 257, 64, 1024, 333}, B = cat(Ints(40, 37), Ints(5, 400)), C = {17, 18, 23, 16}, D(8, 200);
  const std::vector<Ints> B2 = {cat(iota(40, 44), {0}), iota(1, 39)};
  const std::vector<Recorded> recorded = {
      {"A", &A, 256, 1, 4, 0, 4, 1, {256, 254, 30}, {{9}, {3, 10, 7, 5}, {8, 0, 1}}, {2, 4, 6}},
      {"A", &A, 256, 2, 4, 0, 4, 2, {510, 30}, {{9, 3, 10, 7, 5}, {8, 0, 1}}, {2, 4, 6}},
      {"A", &A, 256, 1, 0, 0, 8, 1, {248, 161}, {{4, 3, 10, 8, 0, 5, 1}, {9, 7}}, {2, 6}},
      {"A", &A, 256, 2, 0, 0, 8, 1, {248, 161}, {{4, 3, 10, 8, 0, 5, 1}, {9, 7}}, {2, 6}},
      {"A", &A, 64, 2, 0, 0, 8, 1, {63, 47, 33}, {{3, 8, 0}, {10, 5, 1}, {7}}, {2, 4, 6, 9}},
      {"B", &B, 256, 1, 0, 0, 8, 1, {255, 195}, B2, {}},
      {"B", &B, 256, 2, 0, 0, 4, 2, {510, 390}, B2, {}},
      {"B", &B, 256, 2, 0, 41, 4, 1, {250, 250, 250, 150}, {cat({40, 41}, iota(0, 4)), cat({42, 43}, iota(5, 9)), cat({44}, iota(10, 24)), iota(25, 39)}, {}},
      {"B", &B, 256, 1, 0, 42, 8, 1, {255, 195}, B2, {}},  // (the force is ignored without per_cu4 >= 2)
      {"C", &C, 256, 1, 0, 0, 4, 1, {20}, {{2, 0, 1, 3}}, {}},
      {"C", &C, 256, 2, 0, 0, 4, 1, {20}, {{2, 0, 1, 3}}, {}},
      {"C", &C, 256, 1, 4, 0, 4, 1, {20}, {{2, 0, 1, 3}}, {}},
      {"C", &C, 256, 2, 4, 0, 4, 1, {20}, {{2, 0, 1, 3}}, {}},
      {"C", &C, 8, 1, 0, 0, 8, 1, {8, 3}, {{0, 1, 3}, {2}}, {}},
      {"D", &D, 256, 1, 0, 0, 8, 1, {200}, {iota(0, 7)}, {}},
      {"D", &D, 256, 2, 0, 0, 4, 2, {400}, {iota(0, 7)}, {}},
      {"D", &D, 256, 1, 4, 0, 4, 1, {250, 150}, {iota(0, 4), iota(5, 7)}, {}},
  };
  for (const Recorded &r : recorded) check_recorded(r);

  // (a) over the inputs above and seeded random ones
  std::vector<Ints> inputs = {A, B, C, D, {2}, {16}, {15, 15}, {2048}, {2049, 16}};
  std::mt19937 rng(20240327);
  for (int t = 0; t < 300; ++t) {
    Ints Fu(1 + rng() % 60);
    for (int &f : Fu) f = 2 + (int)(rng() % 1199);  // 2 .. 1200
    inputs.push_back(Fu);
  }
  for (const Ints &Fu : inputs)
    for (int n_cu : {8, 64, 256})
      for (int per_cu4 : {1, 2})
        for (int shape : {0, 4})
          for (int force : {0, 8, 41, 42}) check_invariants(Fu, n_cu, per_cu4, shape, force);

  {  // a handle without a usable persistent engine (n_cu = 0): nothing is launched, everything alone in index order
    g_case = "empty plan";
    const GlBatchPlan P = gl_batch_plan(A, HOP, 0, 2, 0, 8);
    CHECK(P.segs.empty() && P.launches.empty() && P.batched == std::vector<char>(A.size(), 0) && P.order == iota(0, (int)A.size() - 1));
  }

  {  // (c) the rows table: running sums, and the caller's message once the total passes the cap
    g_case = "rows";
    const Rows r = gl_rows(A, (size_t)1 << 24, "batch too large");
    CHECK(r.n() == (int)A.size() && r.F == A && r.total == 3257);
    for (int u = 0, f = 0; u < r.n(); f += A[u], ++u) CHECK(r.row0[u] == f);
    const char *m24 = "batch too large", *m20 = "batch too large: more than 2^20 frames";
    const Ints at24 = {1 << 23, 1 << 23}, over24 = {1 << 23, 1 << 23, 1}, at20 = {1 << 19, (1 << 19) - 1, 1}, over20 = {(1 << 20) + 1};
    CHECK(gl_rows(at24, (size_t)1 << 24, m24).total == (size_t)1 << 24 && thrown([&] { gl_rows(over24, (size_t)1 << 24, m24); }) == m24);
    CHECK(gl_rows(at20, (size_t)1 << 20, m20).total == (size_t)1 << 20 && thrown([&] { gl_rows(over20, (size_t)1 << 20, m20); }) == m20);
    Rows big;  // a count that would wrap the sum
    big.add(5, (size_t)1 << 20, m20);
    CHECK(thrown([&] { big.add(~(size_t)0 - 2, (size_t)1 << 20, m20); }) == m20 && big.n() == 1 && big.total == 5);
  }
  std::puts("ok");
  return 0;
}
