// Stand-alone driver of csrc/durations_plan.h (plain g++, built with -fsanitize=address,undefined by tests/test_durations_cpu.py):
// the argument rules, the Q16 rounding, the layout under a permutation, the row choice by parity, the mask, multi-chunk bases,
// 64-bit starts at 16384-frame chunks, the stats, and the two maps.
#include <cmath>
#include <cstdio>
#include <limits>

#include "durations_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static bool names(const std::string &msg, const char *field) { return msg.find(field) != std::string::npos; }

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  static_assert(sizeof(DurationsOpts) == 12, "xdtts_durations_opts is 12 bytes");
  static_assert(sizeof(AlignmentStats) == 48, "xdtts_alignment_stats is 48 bytes");
  static_assert(sizeof(DurChunk) == 24 && sizeof(DurUtt) == 16, "the kernel's tables");

  // the setting
  const DurationsOpts d = durations_default();
  CHECK(d.on == 0 && d.min_frames == 0.5f && d.max_frames == 40.0f && durations_check(d).empty());
  CHECK(names(durations_check(DurationsOpts{2, 0.5f, 40.f}), "on"));
  CHECK(names(durations_check(DurationsOpts{-1, 0.5f, 40.f}), "on"));
  for (float v : {-1.0f, nan, inf, 65536.0f}) CHECK(names(durations_check(DurationsOpts{1, v, 40.f}), "min_frames"));
  for (float v : {0.25f, nan, inf, 65536.0f}) CHECK(names(durations_check(DurationsOpts{1, 0.5f, v}), "max_frames"));
  CHECK(durations_check(DurationsOpts{1, 0.0f, 0.0f}).empty() && durations_check(DurationsOpts{1, 65535.0f, 65535.0f}).empty());

  // Q16: one exact scaling, one rounding to nearest even
  CHECK(durations_q16(0.0f) == 0u && durations_q16(-0.0f) == 0u && durations_q16(-1.0f) == 0u && durations_q16(nan) == 0u);
  CHECK(durations_q16(1.0f) == 65536u && durations_q16(0.5f) == 32768u);
  CHECK(durations_q16(std::ldexp(1.0f, -17)) == 0u);   // 0.5 -> even 0
  CHECK(durations_q16(std::ldexp(3.0f, -17)) == 2u);   // 1.5 -> even 2
  CHECK(durations_q16(std::ldexp(5.0f, -17)) == 2u);   // 2.5 -> even 2
  CHECK(durations_q16(std::ldexp(5.0f, -18)) == 1u);   // 1.25 -> 1
  CHECK(durations_q16(std::ldexp(7.0f, -18)) == 2u);   // 1.75 -> 2
  CHECK(durations_q16(65535.0f) == 65535u * 65536u && durations_q16(65536.0f) == 0xFFFFFFFFu && durations_q16(inf) == 0xFFFFFFFFu);
  CHECK(durations_q16(16384.0f) == 16384u * 65536u);

  // the argument rules
  {
    const int nv[3] = {2, 3, 1}, nf[3] = {4, 5, 6}, ord[3] = {2, 0, 1}, bad_ord[3] = {0, 0, 1}, utt[3] = {0, 0, 1}, bad_utt[3] = {0, 2, 2}, utt1[3] = {1, 1, 1};
    CHECK(durations_plan(3, 4, nf, nv, ord, 0, false, utt, nullptr).empty());
    CHECK(names(durations_plan(0, 4, nf, nv, ord, 0, false, utt, nullptr), "batch"));
    CHECK(names(durations_plan(4097, 4, nf, nv, ord, 0, false, utt, nullptr), "batch"));
    CHECK(names(durations_plan(3, 0, nf, nv, ord, 0, false, utt, nullptr), "window"));
    CHECK(names(durations_plan(3, 513, nf, nv, ord, 0, false, utt, nullptr), "window"));
    CHECK(names(durations_plan(3, 4, nf, nv, ord, 2, true, utt, nullptr), "batched"));
    CHECK(names(durations_plan(3, 4, nf, nv, ord, 1, false, utt, nullptr), "cum_b"));
    CHECK(names(durations_plan(3, 4, nf, nullptr, ord, 0, false, utt, nullptr), "n_valid"));
    CHECK(names(durations_plan(3, 4, nf, nv, bad_ord, 0, false, utt, nullptr), "order"));
    CHECK(names(durations_plan(3, 2, nf, nv, ord, 0, false, utt, nullptr), "n_valid"));  // 3 ids in a window of 2
    CHECK(names(durations_plan(3, 4, nf, nv, ord, 0, false, bad_utt, nullptr), "utt_of_chunk"));
    CHECK(names(durations_plan(3, 4, nf, nv, ord, 0, false, utt1, nullptr), "utt_of_chunk"));
    const int neg[3] = {4, -1, 6}, big[3] = {4, 100001, 6};
    CHECK(names(durations_plan(3, 4, neg, nv, ord, 0, false, utt, nullptr), "nframes"));
    CHECK(names(durations_plan(3, 4, big, nv, ord, 0, false, utt, nullptr), "nframes"));
  }

  // layout, permutation, parity, mask, bases, stats: 3 chunks, two utterances; slot j holds the caller's chunk order[j]
  {
    const int T = 4, B = 3;
    const int ord[3] = {2, 0, 1};       // slot 0 = chunk 2, slot 1 = chunk 0, slot 2 = chunk 1
    const int nv[3] = {1, 2, 3};        // by slot
    const int nf[3] = {6, 5, 4};        // by slot: slot 1 is odd
    const int utt[3] = {0, 0, 1};       // chunks 0, 1 = utterance 0; chunk 2 = utterance 1
    const float a[12] = {6.0f, 9, 9, 9, /* slot 1 */ 1.0f, 2.0f, 9, 9, /* slot 2 */ 0.25f, 3.0f, 0.75f, 9};
    const float b[12] = {7.0f, 9, 9, 9, /* slot 1 */ 1.5f, 3.5f, 9, 9, /* slot 2 */ 8, 8, 8, 8};
    DurPlan p;
    CHECK(durations_plan(B, T, nf, nv, ord, 1, true, utt, &p).empty());
    CHECK(p.n_ids == 6 && p.utt.size() == 2);
    CHECK(p.utt[0].id_off == 0 && p.utt[0].n_ids == 5 && p.utt[0].n_chunks == 2 && p.utt[1].id_off == 5 && p.utt[1].n_ids == 1);
    CHECK(p.chunk[1].out_off == 0 && p.chunk[2].out_off == 2 && p.chunk[0].out_off == 5);
    CHECK(p.chunk[2].k == 1 && p.list[p.chunk[2].list0] == 1);  // chunk 1's earlier chunk is chunk 0, in slot 1
    float dur[6];
    uint32_t q[6];
    uint64_t st[6];
    AlignmentStats s[2];
    durations_reference(p, a, b, T, nf, 1, DurationsOpts{1, 0.5f, 3.25f}, dur, q, st, s);
    // chunk 0 = slot 1, 5 frames: odd -> buffer b; chunk 1 = slot 2, 4 frames: a; chunk 2 = slot 0, 6 frames: a
    const float want[6] = {1.5f, 3.5f, 0.25f, 3.0f, 0.75f, 6.0f};
    const uint64_t want_st[6] = {0, 98304, 5 * 65536, 5 * 65536 + 16384, 5 * 65536 + 16384 + 196608, 0};
    for (int i = 0; i < 6; ++i) CHECK(dur[i] == want[i] && q[i] == durations_q16(want[i]) && st[i] == want_st[i]);
    CHECK(s[0].n_ids == 5 && s[0].n_frames == 9 && s[0].sum_q16 == 9 * 65536u && s[0].min_q16 == 16384u && s[0].min_index == 2);
    CHECK(s[0].max_q16 == 229376u && s[0].max_index == 1 && s[0].n_below == 1 && s[0].n_above == 1 && s[0].last_q16 == 49152u);
    CHECK(s[1].n_ids == 1 && s[1].n_frames == 6 && s[1].min_index == 0 && s[1].max_index == 0 && s[1].last_q16 == 6 * 65536u && s[1].n_above == 1);
    // not batched: always buffer a
    durations_reference(p, a, b, T, nf, 0, d, dur, q, st, s);
    CHECK(dur[0] == 1.0f && dur[1] == 2.0f);
    // equal values: the first index
    const float eq[12] = {1, 0, 0, 0, 2, 2, 0, 0, 2, 2, 2, 0};
    durations_reference(p, eq, nullptr, T, nf, 0, d, nullptr, nullptr, nullptr, s);
    CHECK(s[0].min_index == 0 && s[0].max_index == 0);
  }

  // 64-bit starts: 40 chunks of 16384 frames in one utterance, the last id of each holding them all
  {
    const int B = 40, T = 2;
    std::vector<int> nv(B, 2), nf(B, 16384), utt(B, 0);
    std::vector<float> a((size_t)B * T);
    for (int j = 0; j < B; ++j) a[2 * j] = 16383.5f, a[2 * j + 1] = 0.5f;
    DurPlan p;
    CHECK(durations_plan(B, T, nf.data(), nv.data(), nullptr, 0, false, utt.data(), &p).empty());
    std::vector<uint64_t> st(p.n_ids);
    AlignmentStats s;
    durations_reference(p, a.data(), nullptr, T, nf.data(), 0, d, nullptr, nullptr, st.data(), &s);
    CHECK(st[2 * 39] == (uint64_t)39 * 16384 * 65536 && st[2 * 39 + 1] == (uint64_t)39 * 16384 * 65536 + (uint64_t)16383 * 65536 + 32768);
    CHECK(st[2 * 39] > ((uint64_t)1 << 32) && s.n_frames == (uint64_t)40 * 16384 && s.sum_q16 == (uint64_t)40 * 16384 * 65536);
  }

  // the position map: integer and fractional x, 0 and n, the clamp, the rule
  {
    const uint64_t st[3] = {0, 2 * 65536, 5 * 65536};
    const uint32_t q[3] = {2 * 65536, 3 * 65536, 4 * 65536};
    CHECK(durations_position(st, q, 3, 10, 0.0) == 0.0);
    CHECK(durations_position(st, q, 3, 10, 1.0) == 2.0 / 9.0);
    CHECK(durations_position(st, q, 3, 10, 1.5) == 3.5 / 9.0);
    CHECK(durations_position(st, q, 3, 10, 3.0) == 1.0);  // x == n: the end of the last id, 9 / 9
    CHECK(durations_position(st, q, 3, 8, 3.0) == 1.0);   // clamped
    CHECK(durations_position(st, q, 3, 1, 2.0) == 0.0);
    CHECK(std::isnan(durations_position(st, q, 3, 10, -0.1)) && std::isnan(durations_position(st, q, 3, 10, 3.1)));
    CHECK(std::isnan(durations_position(st, q, 3, 10, std::nan(""))) && std::isnan(durations_position(st, q, 0, 10, 0.0)));
    CHECK(std::isnan(durations_position(nullptr, q, 3, 10, 0.0)) && std::isnan(durations_position(st, q, 3, 0, 0.0)));
  }

  // the sample map
  CHECK(durations_samples(0, 256, 22050) == 0 && durations_samples(10 * 65536, 256, 22050) == 2560);
  CHECK(durations_samples(10 * 65536 + 32768, 256, 22050) == 2688);
  CHECK(durations_samples(10 * 65536, 256, 44100) == 5120 && durations_samples(3 * 65536, 256, 8000) == (int64_t)(768LL * 160 / 441));
  CHECK(durations_samples(65536, 256, 7999) == -1 && durations_samples(65536, 0, 22050) == -1);
  CHECK(durations_samples((uint64_t)4096 * 100000 * 65536, 256, 96000) == (int64_t)((unsigned __int128)4096 * 100000 * 256 * 640 / 147));

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
