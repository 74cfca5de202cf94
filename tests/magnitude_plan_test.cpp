// magnitude_plan_test.cpp -- the magnitude chain's host arithmetic (xd-tts_amd/csrc/magnitude_plan.h) on the host alone (no HIP,
// no GPU): the request's identity() and frames(), F' and the rows of every record table against values worked out by hand from
// the rules in the records' comments, the contour frame table with three and four arrays, the tracker's records, the SPSI
// segments, frame_local, the loop's buffer in all eight combinations, and the 2^24-row failure.
// Built and run by tests/test_magnitude_plan_cpu.py (plain, and with the address and undefined-behaviour sanitizers); prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "magnitude_plan.h"

using namespace xdtts;

static std::string g_case;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)  [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static const std::vector<Timbre> NO_TIMBRE;
static const Timbre VOICE{1.12f, 0.25f, 9u, 28, 1e-4f};

static bool same(const ProsodyUtt &a, const ProsodyUtt &b) {
  return a.src0 == b.src0 && a.F == b.F && a.dst0 == b.dst0 && a.Fout == b.Fout && a.rate == b.rate && a.pitch == b.pitch && a.lifter == b.lifter &&
         a.log_floor == b.log_floor;
}
static bool same(const ContourUtt &a, const ContourUtt &b) {
  return a.src0 == b.src0 && a.F == b.F && a.dst0 == b.dst0 && a.Fout == b.Fout && a.tab0 == b.tab0 && a.lifter == b.lifter && a.log_floor == b.log_floor &&
         a.identity == b.identity;
}
static bool same(const TimbreUtt &a, const TimbreUtt &b) {
  return a.src0 == b.src0 && a.dst0 == b.dst0 && a.F == b.F && a.vtl == b.vtl && a.breath == b.breath && a.seed == b.seed && a.lifter == b.lifter &&
         a.log_floor == b.log_floor;
}
static bool same(const F0Utt &a, const F0Utt &b) {
  return a.row0 == b.row0 && a.F == b.F && a.tab0 == b.tab0 && a.mode == b.mode && a.value == b.value && a.range == b.range;
}
static bool same(const SpsiSeg &a, const SpsiSeg &b) { return a.row0 == b.row0 && a.n == b.n && a.first == b.first && a.last == b.last; }
static unsigned bits(float x) {
  unsigned u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}
static void check_frame_local(const MagnitudePlan &p) {
  CHECK(p.frame_local.size() == p.rows.total);
  for (int u = 0; u < p.rows.n(); ++u)
    for (int f = 0; f < p.rows.F[(size_t)u]; ++f) CHECK(p.frame_local[(size_t)p.rows.row0[(size_t)u] + (size_t)f] == f);  // restarts at 0
}

// F' = max(floor((F - 1) / rate + 0.5), 1) + 1: 2 -> 3 and 24 -> 47 and 25 -> 49 at rate 0.5; 24 -> 13 (11.5 + 0.5) and 25 -> 13
// (12.5 -> 12) at rate 2; 2 -> 2 at rate 2 (0.5 + 0.5 = 1)
static void test_frames() {
  g_case = "prosody_frames";
  CHECK(prosody_frames(2, 0.5f) == 3 && prosody_frames(24, 0.5f) == 47 && prosody_frames(25, 0.5f) == 49);
  CHECK(prosody_frames(24, 2.0f) == 13 && prosody_frames(25, 2.0f) == 13 && prosody_frames(2, 2.0f) == 2);
  CHECK(prosody_frames(1, 1.0f) == 1 && prosody_frames(1, 2.0f) == 0 && prosody_frames(24, 0.2f) == 0 && prosody_frames(24, 4.5f) == 0);
  CHECK(spsi_segments(1) == 1 && spsi_segments(24) == 1 && spsi_segments(25) == 2 && spsi_segments(48) == 2 && spsi_segments(49) == 3 && SPSI_L == 24);
}

static void test_request() {
  g_case = "request";
  const MagnitudeRequest none = MagnitudeRequest::none(3);
  CHECK(none.n() == 3 && none.form() == MagnitudeRequest::NONE && !none.tracked() && none.identity(1) && none.frames(2, 25) == 25);
  const Prosody pr[3] = {{0.5f, 1.2f, 30, 1e-5f}, {1.0f, 1.0f, 30, 1e-5f}, {1.0f, 0.8f, 30, 1e-5f}};
  const MagnitudeRequest uni = MagnitudeRequest::uniform(pr, 3);
  CHECK(uni.form() == MagnitudeRequest::UNIFORM && !uni.identity(0) && uni.identity(1) && !uni.identity(2));  // (a pitch alone is no identity)
  CHECK(uni.frames(0, 24) == 47 && uni.frames(1, 24) == 24 && uni.frames(2, 24) == 24);
  std::vector<ContourTable> tabs(2);
  tabs[0].F = tabs[0].Fout = 24;
  tabs[1].identity = false, tabs[1].F = 2, tabs[1].Fout = 3, tabs[1].c = {0, 131072}, tabs[1].pitch = {1, 1}, tabs[1].gain = {1, 1};
  const MagnitudeRequest con = MagnitudeRequest::contours(tabs);
  CHECK(con.form() == MagnitudeRequest::CONTOUR && !con.tracked() && con.identity(0) && !con.identity(1) && con.frames(0, 24) == 24 && con.frames(1, 2) == 3);
  F0Job job{f0_opts_default(), 56, 367};
  const MagnitudeRequest tgt = MagnitudeRequest::targets(tabs, job, {{1, 180.0f, 1.0f}, {0, 1.0f, 1.0f}});
  CHECK(tgt.form() == MagnitudeRequest::CONTOUR && tgt.tracked() && tgt.job().q_hi == 367 && tgt.target(0).mode == 1 && tgt.frames(1, 2) == 3);
  bool threw = false;
  try {
    MagnitudeRequest::targets(tabs, job, {{0, 1.0f, 1.0f}});
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw);
}

// u0: F = 24 at rate 0.5 (F' = 47 > F); u1: F = 2, the identity, in the middle; u2: F = 25 at rate 2 (F' = 13 < F)
static void test_uniform() {
  g_case = "uniform n_utt 3";
  const Prosody pr[3] = {{0.5f, 1.2f, 30, 1e-5f}, {1.0f, 1.0f, 31, 1e-5f}, {2.0f, 0.8f, 32, 2e-5f}};
  const int Fin[3] = {24, 2, 25};
  const MagnitudePlan p = magnitude_plan(MagnitudeRequest::uniform(pr, 3), Fin, std::vector<Timbre>(1, VOICE), 1);
  CHECK(p.prosody == MagnitudeRequest::UNIFORM && p.staged() && !p.track && p.spsi && p.chained && p.loop == MagnitudePlan::S_TIMBRE);
  CHECK(p.in.total == 51 && p.in.row0 == std::vector<int>({0, 24, 26}) && p.in.F == std::vector<int>({24, 2, 25}));
  CHECK(p.rows.total == 62 && p.rows.row0 == std::vector<int>({0, 47, 49}) && p.rows.F == std::vector<int>({47, 2, 13}));
  CHECK(p.loop_rows == 62);  // max(sum F, sum F')
  const ProsodyUtt want[3] = {{0, 24, 0, 47, 0.5f, 1.2f, 30, 1e-5f}, {24, 2, 47, 2, 1.0f, 1.0f, 31, 1e-5f}, {26, 25, 49, 13, 2.0f, 0.8f, 32, 2e-5f}};
  CHECK(p.pros.size() == 3 && p.contour.empty() && p.ftab.empty() && p.f0.empty() && p.n_tab == 0);
  for (int u = 0; u < 3; ++u) CHECK(same(p.pros[(size_t)u], want[u]));
  // timbre on the F' rows, src0 = dst0, the handle's one setting for every utterance
  const TimbreUtt tw[3] = {{0, 0, 47, 1.12f, 0.25f, 9u, 28, 1e-4f}, {47, 47, 2, 1.12f, 0.25f, 9u, 28, 1e-4f}, {49, 49, 13, 1.12f, 0.25f, 9u, 28, 1e-4f}};
  CHECK(p.timbre.size() == 3);
  for (int u = 0; u < 3; ++u) CHECK(same(p.timbre[(size_t)u], tw[u]));
  // SPSI on the F' rows: 47 = 24 + 23, 2, 13
  const SpsiSeg sw[4] = {{0, 24, 1, 0}, {24, 23, 0, 1}, {47, 2, 1, 1}, {49, 13, 1, 1}};
  CHECK(p.spsi_segs.size() == 4 && p.spsi_utts.size() == 3);
  for (int k = 0; k < 4; ++k) CHECK(same(p.spsi_segs[(size_t)k], sw[k]));
  CHECK(p.spsi_utts[0].seg0 == 0 && p.spsi_utts[0].nseg == 2 && p.spsi_utts[1].seg0 == 2 && p.spsi_utts[1].nseg == 1 && p.spsi_utts[2].seg0 == 3 && p.spsi_utts[2].nseg == 1);
  check_frame_local(p);
  CHECK(p.frame_local[46] == 46 && p.frame_local[47] == 0 && p.frame_local[48] == 1 && p.frame_local[49] == 0 && p.frame_local[61] == 12);

  g_case = "uniform n_utt 1, F' < F";
  const int F25 = 25;
  const MagnitudePlan q = magnitude_plan(MagnitudeRequest::uniform(&pr[2], 1), &F25, NO_TIMBRE, 0);
  CHECK(q.in.total == 25 && q.rows.total == 13 && q.loop_rows == 25 && q.loop == MagnitudePlan::S_PROS && !q.spsi && q.spsi_segs.empty() && q.timbre.empty());
  CHECK(q.pros.size() == 1 && same(q.pros[0], ProsodyUtt{0, 25, 0, 13, 2.0f, 0.8f, 32, 2e-5f}));
  check_frame_local(q);

  g_case = "uniform, every utterance the identity";
  const MagnitudePlan r = magnitude_plan(MagnitudeRequest::uniform(&pr[1], 1), &F25, NO_TIMBRE, 0);
  CHECK(r.prosody == MagnitudeRequest::NONE && r.pros.empty() && r.rows.total == 25 && r.loop == MagnitudePlan::S);  // a request path launches nothing
  const MagnitudePlan h = magnitude_plan(MagnitudeRequest::uniform(&pr[1], 1), &F25, NO_TIMBRE, 0, true);
  CHECK(h.prosody == MagnitudeRequest::UNIFORM && h.pros.size() == 1 && same(h.pros[0], ProsodyUtt{0, 25, 0, 25, 1.0f, 1.0f, 31, 1e-5f}));  // the stage's hook does
}

static void test_spsi_one() {
  const int Fs[3] = {2, 24, 25};
  for (int F : Fs) {
    g_case = "spsi n_utt 1 F " + std::to_string(F);
    const MagnitudePlan p = magnitude_plan(MagnitudeRequest::none(1), &F, NO_TIMBRE, 1);
    CHECK(p.spsi && p.spsi_utts.size() == 1 && p.spsi_utts[0].seg0 == 0 && p.loop == MagnitudePlan::S && p.rows.total == (size_t)F && p.loop_rows == (size_t)F);
    if (F <= 24) {  // one segment exactly: not chained
      CHECK(!p.chained && p.spsi_segs.size() == 1 && same(p.spsi_segs[0], SpsiSeg{0, F, 1, 1}) && p.spsi_utts[0].nseg == 1);
    } else {  // a second segment of one frame
      CHECK(p.chained && p.spsi_segs.size() == 2 && same(p.spsi_segs[0], SpsiSeg{0, 24, 1, 0}) && same(p.spsi_segs[1], SpsiSeg{24, 1, 0, 1}) && p.spsi_utts[0].nseg == 2);
    }
    check_frame_local(p);
  }
}

// u0: F = 2 -> F' = 3 with a table of 2 entries; u1: F = 24, an identity contour in the middle (no entries); u2: F = 25 -> F' = 13
// with a table of 25 entries.  n_tab = 27; the arrays c | pitch | gain (| pitch once more) lie 27 entries apart.
static std::vector<ContourTable> three_tables() {
  std::vector<ContourTable> t(3);
  t[0].identity = false, t[0].F = 2, t[0].Fout = 3, t[0].lifter = 30, t[0].log_floor = 1e-5f;
  t[0].c = {0, 131072}, t[0].pitch = {0.9f, 1.1f}, t[0].gain = {1.0f, 0.5f};
  t[1].F = t[1].Fout = 24, t[1].lifter = 20, t[1].log_floor = 2e-5f;
  t[2].identity = false, t[2].F = 25, t[2].Fout = 13, t[2].lifter = 40, t[2].log_floor = 3e-5f;
  for (int m = 0; m < 25; ++m) t[2].c.push_back(32768u * (unsigned)m), t[2].pitch.push_back(1.0f + 0.01f * (float)m), t[2].gain.push_back(2.0f - 0.01f * (float)m);
  return t;
}
static void check_three_tables(const MagnitudePlan &p, bool four) {
  CHECK(p.prosody == MagnitudeRequest::CONTOUR && p.n_tab == 27 && p.ftab.size() == (four ? 108u : 81u));
  CHECK(p.in.total == 51 && p.in.row0 == std::vector<int>({0, 2, 26}) && p.rows.total == 40 && p.rows.row0 == std::vector<int>({0, 3, 27}) && p.loop_rows == 51);
  const ContourUtt want[3] = {{0, 2, 0, 3, 0, 30, 1e-5f, 0}, {2, 24, 3, 24, 2, 20, 2e-5f, 1}, {26, 25, 27, 13, 2, 40, 3e-5f, 0}};  // the tab0 chain: 0, 2, 2
  CHECK(p.contour.size() == 3 && p.pros.empty());
  for (int u = 0; u < 3; ++u) CHECK(same(p.contour[(size_t)u], want[u]));
  CHECK(p.ftab[0] == 0 && p.ftab[1] == 131072 && p.ftab[27] == bits(0.9f) && p.ftab[28] == bits(1.1f) && p.ftab[54] == bits(1.0f) && p.ftab[55] == bits(0.5f));
  for (int m = 0; m < 25; ++m) {
    CHECK(p.ftab[2 + (size_t)m] == 32768u * (unsigned)m && p.ftab[29 + (size_t)m] == bits(1.0f + 0.01f * (float)m) && p.ftab[56 + (size_t)m] == bits(2.0f - 0.01f * (float)m));
    if (four) CHECK(p.ftab[83 + (size_t)m] == bits(1.0f + 0.01f * (float)m));
  }
  if (four) CHECK(p.ftab[81] == bits(0.9f) && p.ftab[82] == bits(1.1f));
  check_frame_local(p);
}
static void test_contour() {
  const int Fin[3] = {2, 24, 25};
  g_case = "contour, no tracker";
  const MagnitudePlan p = magnitude_plan(MagnitudeRequest::contours(three_tables()), Fin, NO_TIMBRE, 0);
  check_three_tables(p, false);
  CHECK(!p.track && p.f0.empty() && p.loop == MagnitudePlan::S_PROS);

  g_case = "contour under a tracker job";
  const F0Job job{f0_opts_default(), 56, 367};
  const MagnitudePlan q = magnitude_plan(MagnitudeRequest::targets(three_tables(), job, {{1, 180.0f, 1.0f}, {0, 1.0f, 1.0f}, {2, 1.1f, 0.5f}}), Fin, std::vector<Timbre>(1, VOICE), 0);
  check_three_tables(q, true);
  CHECK(q.track && q.job.q_lo == 56 && q.job.q_hi == 367 && q.loop == MagnitudePlan::S_TIMBRE);
  const F0Utt fw[3] = {{0, 2, 0, 1, 180.0f, 1.0f}, {2, 24, -1, 0, 1.0f, 1.0f}, {26, 25, 2, 2, 1.1f, 0.5f}};  // the rows of S; -1: an identity contour has no entry
  CHECK(q.f0.size() == 3);
  for (int u = 0; u < 3; ++u) CHECK(same(q.f0[(size_t)u], fw[u]));
  CHECK(q.timbre.size() == 3 && same(q.timbre[1], TimbreUtt{3, 3, 24, 1.12f, 0.25f, 9u, 28, 1e-4f}) && same(q.timbre[2], TimbreUtt{27, 27, 13, 1.12f, 0.25f, 9u, 28, 1e-4f}));

  g_case = "contours that are all the identity";
  std::vector<ContourTable> id(2);
  id[0].F = id[0].Fout = 24, id[1].F = id[1].Fout = 2;
  const int F2[2] = {24, 2};
  const MagnitudePlan r = magnitude_plan(MagnitudeRequest::contours(id), F2, NO_TIMBRE, 0);
  CHECK(r.prosody == MagnitudeRequest::NONE && r.contour.empty() && r.ftab.empty() && r.loop == MagnitudePlan::S && r.rows.total == 26);
  const MagnitudePlan h = magnitude_plan(MagnitudeRequest::contours(id), F2, NO_TIMBRE, 0, true);  // the hook: the kernel copies
  CHECK(h.prosody == MagnitudeRequest::CONTOUR && h.contour.size() == 2 && h.n_tab == 0 && h.ftab == std::vector<unsigned>(3, 0u) && h.contour[1].identity == 1 && h.contour[1].dst0 == 24);
}

// the tables of a target request: a target that is not the identity over no contour gets the rate-1 table
static void test_target_tables() {
  g_case = "target tables";
  const PitchTarget t[3] = {{1, 180.0f, 1.0f}, {0, 1.0f, 1.0f}, {2, 1.0f, 1.0f}};  // Hz; none; the factor 1: the identity too
  const size_t F[3] = {3, 24, 2};
  std::vector<ContourTable> tabs;
  bool active = false, any = true;
  CHECK(target_tables(t, nullptr, 3, F, tabs, &active, &any).empty() && active && !any && tabs.size() == 3);
  CHECK(!tabs[0].identity && tabs[0].F == 3 && tabs[0].Fout == 3 && tabs[0].c == std::vector<uint32_t>({0, 65536, 131072}) &&
        tabs[0].pitch == std::vector<float>(3, 1.0f) && tabs[0].gain == std::vector<float>(3, 1.0f));
  CHECK(tabs[1].identity && tabs[1].F == 24 && tabs[1].Fout == 24 && tabs[1].c.empty() && tabs[2].identity && tabs[2].Fout == 2);
  const F0Job job{f0_opts_default(), 56, 367};
  const int Fi[3] = {3, 24, 2};
  const MagnitudePlan p = magnitude_plan(MagnitudeRequest::targets(tabs, job, std::vector<PitchTarget>(t, t + 3)), Fi, NO_TIMBRE, 0);
  CHECK(p.track && p.n_tab == 3 && p.ftab.size() == 12 && p.contour[0].identity == 0 && p.contour[1].identity == 1 && p.contour[1].tab0 == 3 && p.contour[2].tab0 == 3);
  CHECK(same(p.f0[0], F0Utt{0, 3, 0, 1, 180.0f, 1.0f}) && same(p.f0[1], F0Utt{3, 24, -1, 0, 1.0f, 1.0f}) && same(p.f0[2], F0Utt{27, 2, -1, 2, 1.0f, 1.0f}));
  CHECK(p.ftab[2] == 131072 && p.ftab[3] == bits(1.0f) && p.ftab[9] == bits(1.0f) && p.rows.total == 29 && p.in.total == 29);
  // identities alone: not active; a contour is noticed; the frame rules carry the utterance
  const ContourPoint pts[2] = {{0.0f, 2.0f, 1.0f, 1.0f}, {1.0f, 2.0f, 1.0f, 1.0f}};
  const Contour c{pts, 2, 30, 1e-5f};
  const Contour *cs[2] = {nullptr, &c};
  CHECK(target_tables(&t[1], cs, 2, &F[1], tabs, &active, &any).empty() && !active && any && tabs[0].identity && !tabs[1].identity && tabs[1].F == 2);
  const size_t one = 1;
  CHECK(target_tables(t, nullptr, 1, &one, tabs, &active, &any) == "utterance 0: a pitch target that is not the identity takes 2 .. 16384 frames, got 1");
  const size_t many[2] = {24, 16385};
  CHECK(target_tables(t, nullptr, 2, many, tabs, &active, &any) == "utterance 1: the pitch tracker takes 1 .. 16384 frames, got 16385");
  CHECK(target_tables(&t[1], cs, 2, many, tabs, &active, &any).rfind("utterance 1: contour n_frames:", 0) == 0);

  g_case = "tracker alone";
  Rows rows;
  rows.add(24, 1 << 20, "x"), rows.add(2, 1 << 20, "x");
  const MagnitudePlan q = magnitude_plan_tracker(rows, job);
  CHECK(q.track && !q.staged() && q.in.total == 26 && q.f0.size() == 2 && same(q.f0[0], F0Utt{0, 24, -1, 0, 1.0f, 1.0f}) && same(q.f0[1], F0Utt{24, 2, -1, 0, 1.0f, 1.0f}));
  CHECK(q.n_tab == 0 && q.ftab.empty() && q.loop == MagnitudePlan::S && q.rows.total == 26);
}

// one Timbre per utterance: the stage's hook
static void test_timbre_each() {
  g_case = "timbre, one setting each";
  const std::vector<Timbre> ts = {timbre_default(), VOICE, {0.9f, 0.0f, 4u, 30, 1e-5f}};
  const int Fin[3] = {2, 24, 25};
  const MagnitudePlan p = magnitude_plan(MagnitudeRequest::none(3), Fin, ts, 0);
  CHECK(p.timbre.size() == 3 && p.loop == MagnitudePlan::S_TIMBRE && !p.staged());
  CHECK(same(p.timbre[0], TimbreUtt{0, 0, 2, 1.0f, 0.0f, 1u, 30, 1e-5f}) && same(p.timbre[1], TimbreUtt{2, 2, 24, 1.12f, 0.25f, 9u, 28, 1e-4f}) &&
        same(p.timbre[2], TimbreUtt{26, 26, 25, 0.9f, 0.0f, 4u, 30, 1e-5f}));
}

static void test_loop_buffer() {
  const Prosody on{0.5f, 1.0f, 30, 1e-5f};
  const int F = 24;
  for (int k = 0; k < 8; ++k) {
    const bool staged = k & 1, timbre = k & 2, spsi = k & 4;
    g_case = "loop buffer, combination " + std::to_string(k);
    const MagnitudePlan p = magnitude_plan(staged ? MagnitudeRequest::uniform(&on, 1) : MagnitudeRequest::none(1), &F, timbre ? std::vector<Timbre>(1, VOICE) : NO_TIMBRE, spsi ? 1 : 0);
    CHECK(p.loop == (timbre ? MagnitudePlan::S_TIMBRE : (staged ? MagnitudePlan::S_PROS : MagnitudePlan::S)));
    CHECK(p.staged() == staged && p.timbre.size() == (timbre ? 1u : 0u) && p.spsi == spsi && p.spsi_segs.size() == (spsi ? (staged ? 2u : 1u) : 0u));  // (F' = 47: two segments)
    CHECK(p.rows.total == (staged ? 47u : 24u) && p.loop_rows == (staged ? 47u : 24u));
  }
}

static void test_too_large() {
  g_case = "2^24 rows";
  auto message = [](const MagnitudeRequest &req, const size_t *Fin) {
    try {
      magnitude_plan(req, Fin, NO_TIMBRE, 0);
    } catch (const std::length_error &e) {
      return std::string(e.what());
    }
    return std::string();
  };
  const size_t past[2] = {((size_t)1 << 24) - 1, 2}, one_past = ((size_t)1 << 24) + 1;
  CHECK(message(MagnitudeRequest::none(1), &one_past) == "batch too large" && message(MagnitudeRequest::none(2), past) == "batch too large");
  const Prosody slow{0.25f, 1.0f, 30, 1e-5f};  // F' = 4 (F - 1) + 1: the mel fits, the frames behind the stage do not
  const size_t F = (size_t)1 << 23;
  CHECK(message(MagnitudeRequest::uniform(&slow, 1), &F) == "batch too large");
}

int main() {
  test_frames();
  test_request();
  test_uniform();
  test_spsi_one();
  test_contour();
  test_target_tables();
  test_timbre_each();
  test_loop_buffer();
  test_too_large();
  std::printf("ok\n");
  return 0;
}
