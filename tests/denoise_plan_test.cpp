// denoise_plan_test.cpp -- the clean-up stage's host arithmetic (xd-tts_amd/csrc/denoise_plan.h, magnitude_plan.h) on the host
// alone (no HIP, no GPU): the argument rules, rank / floor / tone, the two launches of denoise.hip as their workgroups perform
// them -- the same index functions, thread by thread, into buffers of the exact size (ragged tables, the lone bin 512) -- against
// the serial definition bit for bit, and magnitude_plan() with the stage on and with the argument defaulted.
// Built and run by tests/test_denoise_cpu.py with the address and undefined-behaviour sanitizers; prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "magnitude_plan.h"

using namespace xdtts;

static std::string g_case;
static void check_failed(const char *file, int line, const char *cond) {
  std::fprintf(stderr, "%s:%d: CHECK(%s)  [%s]\n", file, line, cond, g_case.c_str());
  std::exit(1);
}
#define CHECK(cond) ((cond) ? (void)0 : check_failed(__FILE__, __LINE__, #cond))  // (an expression: it stands in comma chains)

static unsigned bits(float x) {
  unsigned u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}
static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static void test_rules() {
  g_case = "rules";
  Denoise d = denoise_default();
  CHECK(sizeof(Denoise) == 80 && sizeof(DenoiseStats) == 16 && sizeof(DenoiseUtt) == 32);
  CHECK(denoise_check(d).empty() && denoise_is_identity(d) && d.quantile == 0.5f && d.floor_db == -20.0f && d.n_tone == 0);
  auto bad = [](Denoise x, const char *field) { return denoise_check(x).find(field) != std::string::npos; };
  Denoise x = d;
  x.strength = -0.5f, CHECK(bad(x, "strength")), x.strength = 16.5f, CHECK(bad(x, "strength")), x.strength = NAN, CHECK(bad(x, "strength"));
  x = d, x.strength = 16.0f, CHECK(denoise_check(x).empty() && !denoise_is_identity(x));
  x = d, x.quantile = 1.5f, CHECK(bad(x, "quantile")), x.quantile = INFINITY, CHECK(bad(x, "quantile")), x.quantile = 1.0f, CHECK(denoise_check(x).empty());
  x = d, x.floor_db = -81.0f, CHECK(bad(x, "floor_db")), x.floor_db = 1.0f, CHECK(bad(x, "floor_db")), x.floor_db = -80.0f, CHECK(denoise_check(x).empty());
  x = d, x.n_tone = 9, CHECK(bad(x, "n_tone")), x.n_tone = -1, CHECK(bad(x, "n_tone"));
  x = d, x.n_tone = 2, x.tone_hz[0] = 100.f, x.tone_hz[1] = 100.f, CHECK(bad(x, "tone_hz[1]")), x.tone_hz[1] = 11025.f, CHECK(denoise_check(x).empty());
  CHECK(denoise_is_identity(x) && denoise_tone_is_flat(x));  // both dB are 0
  x.tone_db[1] = 21.f, CHECK(bad(x, "tone_db[1]")), x.tone_db[1] = -3.f, CHECK(denoise_check(x).empty() && !denoise_is_identity(x));
  x.tone_hz[0] = 0.f, CHECK(bad(x, "tone_hz[0]"));
  x = d, x.tone_db[3] = 7.f, CHECK(denoise_is_identity(x));  // not used
  CHECK(!denoise_frames_check(0).empty() && denoise_frames_check(1).empty() && denoise_frames_check((size_t)1 << 20).empty() &&
        !denoise_frames_check(((size_t)1 << 20) + 1).empty());
  std::vector<float> prof((size_t)DENOISE_NB, 1.f);
  CHECK(denoise_profile_check(prof.data()).empty() && denoise_profile_check(nullptr).empty());
  prof[512] = NAN, CHECK(denoise_profile_check(prof.data()).find("profile[512]") != std::string::npos);

  g_case = "rank, floor, tone";
  CHECK(denoise_rank(1, 1.0f) == 0 && denoise_rank(2, 0.5f) == 0 && denoise_rank(2, 1.0f) == 1 && denoise_rank(3, 0.5f) == 1 && denoise_rank(800, 0.1f) == 79 &&
        denoise_rank(800, 0.5f) == 399 && denoise_rank(800, 1.0f) == 799 && denoise_rank(800, 0.0f) == 0 && denoise_rank(0, 0.5f) == 0);
  CHECK(denoise_floor(0.0f) == 1.0f && denoise_floor(-20.0f) == 0.1f && denoise_floor(-40.0f) == 0.01f);
  std::vector<float> E((size_t)DENOISE_NB);
  denoise_tone(d, E.data());
  for (float e : E) CHECK(e == 1.0f);
  x = d, x.n_tone = 2, x.tone_hz[0] = 1000.f, x.tone_db[0] = -20.f, x.tone_hz[1] = 4000.f, x.tone_db[1] = 0.f;
  denoise_tone(x, E.data());
  CHECK(E[0] == 0.1f && E[1] == 0.1f && E[46] == 0.1f && E[512] == 1.0f && E[186] == 1.0f);  // 46: 990 Hz; 186: 4005 Hz
  const int k2 = 93;  // 2002.6 Hz: a hair above the geometric mean 2000 -> a hair above -10 dB
  CHECK(E[k2] > 0.316f && E[k2] < 0.318f);
  for (int k = 47; k < 186; ++k) CHECK(E[k] > E[k - 1] || k == 47);
}

// ---- the launches, thread by thread ------------------------------------------------------------------------------------------

// k_noise_profile as its workgroups run it: N is written through the kernel's own index functions
static void walk_profile(const std::vector<float> &S, const std::vector<DenoiseUtt> &tab, std::vector<float> &N) {
  const int CNT = 257;
  for (int blk = 0; blk < (int)tab.size() * DENOISE_STRIPS; ++blk) {
    const int u = denoise_profile_utt(blk);
    const DenoiseUtt t = tab[(size_t)u];
    if (!denoise_utt_selects(t)) continue;
    std::vector<unsigned> cnt((size_t)DENOISE_STRIP * CNT), prefix((size_t)DENOISE_STRIP, 0u), rem((size_t)DENOISE_STRIP, (unsigned)t.rank);
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      std::fill(cnt.begin(), cnt.end(), 0u);
      const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;
      for (int tid = 0; tid < DENOISE_LANES; ++tid) {
        const int b = tid % DENOISE_STRIP, bin = denoise_profile_bin(blk, tid);
        if (bin >= DENOISE_NB) continue;
        for (int f = denoise_profile_frame0(tid); f < t.F; f += DENOISE_FSTEP) {
          const unsigned k = denoise_key(S.at(denoise_cell(t.row0, f, bin)));
          if ((k & himask) == prefix[(size_t)b]) cnt.at((size_t)b * CNT + ((k >> shift) & 255u)) += 1u;
        }
      }
      for (int b = 0; b < DENOISE_STRIP; ++b) {
        unsigned acc = 0u;
        int j = 255;
        bool found = false;
        for (int i = 0; i < 256 && !found; ++i) {
          const unsigned c = cnt[(size_t)b * CNT + (size_t)i];
          if (acc + c > rem[(size_t)b]) j = i, found = true; else acc += c;
        }
        prefix[(size_t)b] |= (unsigned)j << shift;
        rem[(size_t)b] = found ? rem[(size_t)b] - acc : 0u;
      }
    }
    for (int tid = 0; tid < DENOISE_STRIP; ++tid) {
      const int bin = denoise_profile_bin(blk, tid);
      if (bin < DENOISE_NB) N.at((size_t)u * DENOISE_NB + (size_t)bin) = denoise_unkey(prefix[(size_t)tid]);
    }
  }
}

// k_denoise as its waves run it (the arithmetic is the reference's: here the indices are what is checked)
static void walk_denoise(const std::vector<float> &S, std::vector<float> &out, const std::vector<DenoiseUtt> &tab, int rows_all, const std::vector<float> &N,
                         const float *profile, const std::vector<float> &tone, std::vector<DenoiseStats> &stats, std::vector<int> &written) {
  const int nblk = (rows_all + DENOISE_ROWS - 1) / DENOISE_ROWS;
  for (int blk = 0; blk < nblk; ++blk)
    for (int wave = 0; wave < DENOISE_ROWS; ++wave) {
      const int row = blk * DENOISE_ROWS + wave;
      if (row >= rows_all) continue;
      const int u = denoise_row_utt(tab.data(), (int)tab.size(), row);
      const DenoiseUtt t = tab[(size_t)u];
      const int j = std::min(std::max(row - t.row0, 0), std::max(t.F, 1) - 1);
      CHECK(row >= t.row0 && row < t.row0 + t.F);  // the search found the row's own utterance
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r <= 8; ++r) {
          if (r == 8 && lane != 0) continue;
          const int k = denoise_lane_bin(lane, r);
          const size_t at = denoise_cell(t.row0, j, k);
          float y = S.at(at);
          if (t.sub) {
            const float n = t.profiled ? profile[k] : N.at((size_t)u * DENOISE_NB + (size_t)k);
            volatile float aN = t.strength * n;
            volatile float q = aN / y;
            volatile float d = 1.0f - q;
            const float dv = d;
            const bool above = dv > t.gmin;
            stats.at((size_t)u).floored += above ? 0u : 1u;
            volatile float p = y * (above ? dv : t.gmin);
            y = p;
          }
          if (t.tone >= 0) {
            volatile float p = y * tone.at((size_t)t.tone * DENOISE_NB + (size_t)k);
            y = p;
          }
          out.at(at) = y;
          written.at(at) += 1;
        }
      if (j == 0) stats.at((size_t)u).cells = (unsigned)t.F * DENOISE_NB, stats[(size_t)u].rank = (unsigned)t.rank, stats[(size_t)u].profiled = (unsigned)t.profiled;
    }
}

static void test_launches() {
  g_case = "launches";
  const int Fs[] = {1, 5, 2, 300, 64, 33, 16};
  const int n_utt = (int)(sizeof Fs / sizeof Fs[0]);
  std::vector<Denoise> ds((size_t)n_utt, denoise_default());
  ds[1].n_tone = 2, ds[1].tone_hz[0] = 300.f, ds[1].tone_db[0] = -6.f, ds[1].tone_hz[1] = 3000.f, ds[1].tone_db[1] = 2.f;  // tone only
  ds[2].strength = 2.f, ds[2].quantile = 1.0f;
  ds[3].strength = 1.5f, ds[3].quantile = 0.1f, ds[3].floor_db = -12.f;
  ds[4].strength = 2.f, ds[4].n_tone = 1, ds[4].tone_hz[0] = 1000.f, ds[4].tone_db[0] = 3.f;
  ds[5].strength = 4.f, ds[5].quantile = 0.5f, ds[5].floor_db = -40.f;
  ds[6].strength = 1.f, ds[6].quantile = 0.0f;
  for (int with_profile = 0; with_profile < 2; ++with_profile) {
    std::vector<float> profile((size_t)DENOISE_NB);
    uint32_t seed = 12345u;
    for (float &p : profile) p = (float)(lcg(seed) >> 8) * (1.0f / 16777216.0f) * 0.01f;
    const float *prof = with_profile ? profile.data() : nullptr;
    std::vector<DenoiseJob> jobs;
    std::vector<float> tone;
    Rows rows;
    for (int u = 0; u < n_utt; ++u) {
      int row = -1;
      if (!denoise_tone_is_flat(ds[(size_t)u])) {
        row = (int)(tone.size() / DENOISE_NB);
        tone.resize(tone.size() + DENOISE_NB);
        denoise_tone(ds[(size_t)u], tone.data() + (size_t)row * DENOISE_NB);
      }
      jobs.push_back(denoise_job(ds[(size_t)u], prof != nullptr, row));
      rows.add((size_t)Fs[u], (size_t)1 << 24, "too large");
    }
    std::vector<size_t> Fin(Fs, Fs + n_utt);
    const MagnitudePlan plan = magnitude_plan(MagnitudeRequest::none(n_utt), Fin.data(), std::vector<Timbre>(), 0, false, jobs);
    CHECK((int)plan.clean.size() == n_utt && plan.in.total == rows.total);
    // S time-major [sum F][513], exactly as large as the rows; some exact zeros, no subnormals
    std::vector<float> S(rows.total * DENOISE_NB);
    for (float &s : S) {
      const uint32_t r = lcg(seed);
      s = (r & 63u) == 0u ? 0.0f : std::exp(-9.0f * (float)(r >> 8) * (1.0f / 16777216.0f));
    }
    std::vector<float> N((size_t)n_utt * DENOISE_NB, -1.0f), out(S.size(), -1.0f);
    std::vector<int> written(S.size(), 0);
    std::vector<DenoiseStats> stats((size_t)n_utt, DenoiseStats{0, 0, 0, 0});
    walk_profile(S, plan.clean, N);
    walk_denoise(S, out, plan.clean, (int)plan.in.total, N, prof, tone, stats, written);
    for (int w : written) CHECK(w == 1);  // every cell once, none twice
    for (int u = 0; u < n_utt; ++u) {
      g_case = "launches: utterance " + std::to_string(u) + (with_profile ? " (profile)" : "");
      const size_t F = (size_t)Fs[u], r0 = (size_t)rows.row0[(size_t)u];
      std::vector<float> Sb(F * DENOISE_NB), want(F * DENOISE_NB);  // the boundary layout: bin-major
      for (size_t f = 0; f < F; ++f)
        for (int k = 0; k < DENOISE_NB; ++k) Sb[(size_t)k * F + f] = S[(r0 + f) * DENOISE_NB + (size_t)k];
      DenoiseStats st;
      denoise_reference(Sb.data(), F, ds[(size_t)u], prof, want.data(), &st);
      for (size_t f = 0; f < F; ++f)
        for (int k = 0; k < DENOISE_NB; ++k) CHECK(bits(out[(r0 + f) * DENOISE_NB + (size_t)k]) == bits(want[(size_t)k * F + f]));
      CHECK(st.cells == stats[(size_t)u].cells && st.floored == stats[(size_t)u].floored && st.rank == stats[(size_t)u].rank && st.profiled == stats[(size_t)u].profiled);
      const bool selects = denoise_utt_selects(plan.clean[(size_t)u]);
      CHECK(selects == (ds[(size_t)u].strength != 0.f && !with_profile));
      if (selects) {
        std::vector<float> Nref((size_t)DENOISE_NB);
        denoise_noise_reference(Sb.data(), F, (uint32_t)plan.clean[(size_t)u].rank, Nref.data());
        for (int k = 0; k < DENOISE_NB; ++k) CHECK(bits(N[(size_t)u * DENOISE_NB + (size_t)k]) == bits(Nref[(size_t)k]));
      } else {
        for (int k = 0; k < DENOISE_NB; ++k) CHECK(N[(size_t)u * DENOISE_NB + (size_t)k] == -1.0f);  // untouched
      }
    }
  }
  g_case = "strips";
  CHECK(DENOISE_STRIPS == 33 && denoise_profile_bin(32, 0) == 512 && denoise_profile_bin(32, 1) == 513 && denoise_profile_bin(31, 15) == 511 &&
        denoise_profile_bin(33, 0) == 0 && denoise_profile_utt(33) == 1 && denoise_profile_utt(32) == 0 && denoise_profile_frame0(511) == 31 &&
        denoise_profile_frame0(15) == 0 && DENOISE_FSTEP == 32);
  CHECK(denoise_cell((1 << 24) - 1, 0, 512) == ((size_t)(1 << 24) - 1) * 513 + 512);  // past 2^31: size_t
}

static void test_magnitude_plan() {
  g_case = "magnitude_plan";
  const size_t Fin[3] = {7, 1, 30};
  Denoise d = denoise_default();
  d.strength = 2.f, d.quantile = 0.5f;
  const std::vector<DenoiseJob> one(1, denoise_job(d, false, 0));
  const std::vector<Timbre> voice(1, Timbre{1.12f, 0.25f, 9u, 28, 1e-4f});
  const Prosody pr[3] = {{2.0f, 1.0f, 30, 1e-5f}, {1.0f, 1.0f, 30, 1e-5f}, {0.5f, 1.2f, 30, 1e-5f}};
  for (int form = 0; form < 2; ++form)
    for (int tv = 0; tv < 2; ++tv)
      for (int ph = 0; ph < 2; ++ph) {
        const MagnitudeRequest req = form ? MagnitudeRequest::uniform(pr, 3) : MagnitudeRequest::none(3);
        const std::vector<Timbre> &tm = tv ? voice : std::vector<Timbre>();
        const MagnitudePlan off = magnitude_plan(req, Fin, tm, ph), off2 = magnitude_plan(req, Fin, tm, ph, false, std::vector<DenoiseJob>());
        const MagnitudePlan on = magnitude_plan(req, Fin, tm, ph, false, one);
        // defaulted: today's plan, no records
        CHECK(off.clean.empty() && off2.clean.empty());
        // on: the records lie on the rows of `in`; nothing else moves
        CHECK(on.clean.size() == 3);
        for (int u = 0; u < 3; ++u) {
          const DenoiseUtt &t = on.clean[(size_t)u];
          CHECK(t.row0 == on.in.row0[(size_t)u] && t.F == (int)Fin[u] && t.rank == (int)denoise_rank(Fin[u], 0.5f) && t.sub == 1 && t.profiled == 0 && t.tone == -1 &&
                t.strength == 2.f && t.gmin == 0.1f);
        }
        CHECK(on.loop == off.loop && on.loop_rows == off.loop_rows && on.rows.total == off.rows.total && on.rows.F == off.rows.F && on.rows.row0 == off.rows.row0 &&
              on.in.F == off.in.F && on.in.row0 == off.in.row0 && on.staged() == off.staged() && on.spsi == off.spsi && on.pros.size() == off.pros.size() &&
              on.timbre.size() == off.timbre.size() && on.spsi_segs.size() == off.spsi_segs.size() && on.frame_local == off.frame_local);
        CHECK(off.loop == (tv ? MagnitudePlan::S_TIMBRE : (form ? MagnitudePlan::S_PROS : MagnitudePlan::S)));
      }
  // one job per utterance, with a profile and a tone row
  Denoise t2 = d;
  t2.n_tone = 1, t2.tone_hz[0] = 500.f, t2.tone_db[0] = -3.f;
  const std::vector<DenoiseJob> each = {denoise_job(denoise_default(), true, -1), denoise_job(t2, true, 4), denoise_job(d, false, -1)};
  const MagnitudePlan p = magnitude_plan(MagnitudeRequest::none(3), Fin, std::vector<Timbre>(), 0, false, each);
  CHECK(p.clean[0].sub == 0 && p.clean[0].profiled == 0 && p.clean[0].tone == -1 && p.clean[0].rank == 0);
  CHECK(p.clean[1].sub == 1 && p.clean[1].profiled == 1 && p.clean[1].tone == 4 && p.clean[1].rank == 0 && p.clean[1].row0 == 7);
  CHECK(p.clean[2].sub == 1 && p.clean[2].profiled == 0 && p.clean[2].rank == 14 && p.clean[2].row0 == 8 && p.clean[2].F == 30);
}

int main() {
  test_rules();
  test_launches();
  test_magnitude_plan();
  std::puts("ok");
  return 0;
}
