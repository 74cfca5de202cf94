// Stand-alone driver of csrc/silence_plan.h (plain g++, built with -fsanitize=address,undefined by tests/test_silence_cpu.py):
// the argument rules, the host integers at every rate the tests use, the per-window rules at their edges, and the three launches
// of silence.hip -- the windows' peaks tile by tile, the three chunked passes of k_sil_plan with their carries, the gather tile
// by tile -- run on the host exactly as the workgroups run them, with scratch of the exact size (the sanitizers see every
// index), and compared bit for bit, samples and stats, with the serial definition.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "silence_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// bursts of a square-ish tone between stretches of exact zeros and of low noise; `seed` moves the edges off the window grid
static std::vector<float> signal(size_t N, int W, uint32_t seed) {
  std::vector<float> x(N, 0.0f);
  uint32_t s = 99991u + (uint32_t)N * 2654435761u + seed;
  size_t i = (seed % 3) * (size_t)W + seed % 7;
  int k = 0;
  while (i < N) {
    s = s * 1664525u + 1013904223u;
    const size_t burst = (size_t)W * (1 + (s >> 27)) + (s >> 13) % 5, gap = (size_t)W * (1 + ((s >> 20) & 63)) + (s >> 9) % 3;
    const float amp = 0.05f + 0.85f * (float)((s >> 5) & 15) / 15.0f;
    for (size_t j = i; j < std::min(N, i + burst); ++j) x[j] = ((j / 13) & 1) ? amp : -amp;
    i += burst;
    if (k++ & 1)
      for (size_t j = i; j < std::min(N, i + gap); ++j) {
        s = s * 1664525u + 1013904223u;
        x[j] = 0.001f * ((float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f);
      }
    i += gap;
  }
  return x;
}

// the three launches on the host
static SilenceStats walk(const std::vector<float> &x, const SilPlan &p, std::vector<float> &out) {
  const int n = (int)x.size();
  const size_t nw = silence_windows(x.size(), p.W), tiles = silence_tiles(x.size());
  std::vector<float> pw(nw, -1.0f), tpk(tiles, -1.0f), T((size_t)p.fade);
  std::vector<int32_t> wl(nw, -7), wr(nw, -7), woff(nw, -7);
  silence_fade_table(p, T.data());
  for (size_t t = 0; t < tiles; ++t) silence_tile_peaks(x.data(), n, (int)(t * SIL_TILE), p, pw.data(), tpk.data());
  for (float v : pw) CHECK(v >= 0.0f);  // every window belongs to exactly one tile
  const SilenceStats st = silence_plan_walk(pw.data(), tpk.data(), n, p, wl.data(), wr.data(), woff.data());
  out.assign((size_t)st.n_out, -7.0f);  // exactly n_out floats: a store behind them is an error
  for (size_t t = 0; t < tiles; ++t) silence_tile_gather(x.data(), n, (int)(t * SIL_TILE), p, T.data(), woff.data(), out.data());
  return st;
}

static void compare(const std::vector<float> &x, int rate, const Silence &s) {
  const SilPlan p = silence_plan(s, rate);
  std::vector<float> ref(x.size(), -3.0f), out;
  const SilenceStats a = silence_reference(x.data(), x.size(), rate, s, ref.data());
  const SilenceStats b = walk(x, p, out);
  CHECK(std::memcmp(&a, &b, sizeof a) == 0);
  CHECK(a.n_out + a.lead_cut + a.trail_cut + a.pause_cut == a.n_in && a.n_in == x.size() && a.n_out >= 1);
  CHECK(out.size() == a.n_out && std::memcmp(out.data(), ref.data(), out.size() * sizeof(float)) == 0);
  std::vector<uint8_t> keep(silence_windows(x.size(), p.W));
  silence_keep(x.data(), x.size(), p, keep.data());
  size_t kept = 0;
  for (size_t w = 0; w < keep.size(); ++w)
    if (keep[w]) kept += (size_t)sil_win_len((int)w, (int)keep.size(), (int)x.size(), p.W);
  CHECK(kept == a.n_out);
}

int main() {
  // the rules
  const Silence d = silence_default();
  CHECK(silence_check(d).empty() && d.threshold_db == -40.0f && d.min_sound_ms == 20.0f && d.lead_ms == 50.0f && d.trail_ms == 100.0f &&
        d.max_pause_ms == 0.0f && d.fade_ms == 2.0f);
  static_assert(sizeof(Silence) == 24 && sizeof(SilenceStats) == 32, "the boundary's sizes");
  {
    const struct {
      float Silence::*f;
      const char *name;
      float lo, hi;
    } fields[] = {{&Silence::threshold_db, "threshold_db", -96.f, -6.f}, {&Silence::min_sound_ms, "min_sound_ms", 0.f, 500.f},
                  {&Silence::lead_ms, "lead_ms", 0.f, 10000.f},          {&Silence::trail_ms, "trail_ms", 0.f, 10000.f},
                  {&Silence::max_pause_ms, "max_pause_ms", 20.f, 60000.f}, {&Silence::fade_ms, "fade_ms", 0.f, 2.5f}};
    for (const auto &e : fields) {
      for (float v : {e.lo, e.hi}) {
        Silence s = d;
        s.*(e.f) = v;
        CHECK(silence_check(s).empty());
      }
      for (float v : {std::nextafterf(e.lo, -INFINITY), std::nextafterf(e.hi, INFINITY), NAN, INFINITY, -INFINITY}) {
        Silence s = d;
        s.*(e.f) = v;
        CHECK(silence_check(s).find(e.name) != std::string::npos);
      }
    }
    Silence s = d;
    s.max_pause_ms = 19.9f;
    CHECK(!silence_check(s).empty());
    s.max_pause_ms = 0.0f;
    CHECK(silence_check(s).empty());
  }
  CHECK(silence_rate_check(7999).find("rate") != std::string::npos && silence_rate_check(96001).find("rate") != std::string::npos);
  CHECK(silence_rate_check(22050).empty() && silence_rate_check(8000).empty() && silence_rate_check(96000).empty());
  CHECK(!silence_args_check(d, 22050, 0).empty() && !silence_args_check(d, 22050, (size_t)1 << 28).empty() && silence_args_check(d, 22050, 1).empty());
  // the host integers
  {
    const int rates[] = {8000, 11025, 16000, 22050, 44100, 48000, 96000}, Ws[] = {40, 55, 80, 110, 220, 240, 480},
              fades[] = {16, 22, 32, 44, 88, 96, 192};
    for (int i = 0; i < 7; ++i) {
      const SilPlan p = silence_plan(d, rates[i]);
      CHECK(p.W == Ws[i] && p.min_w == 4 && p.lead_w == 10 && p.trail_w == 20 && p.pause_w == 0 && p.fade == fades[i]);
      CHECK(p.tfac == 0.01f);
      Silence s = d;
      s.fade_ms = 2.5f;
      CHECK(silence_plan(s, rates[i]).fade == std::min(Ws[i] / 2, (int)std::floor(2.5 * rates[i] / 1000.0 + 0.5)));
    }
    Silence s = d;
    s.min_sound_ms = 12.5f, s.max_pause_ms = 105.0f, s.lead_ms = 2.4f, s.trail_ms = 7.5f;
    const SilPlan p = silence_plan(s, 22050);
    CHECK(p.min_w == 3 && p.pause_w == 21 && p.lead_w == 0 && p.trail_w == 2);
  }
  // the rules of one window at their edges
  {
    SilPlan p = silence_plan(d, 22050);
    p.pause_w = 5;
    CHECK(sil_keep_rule(7, false, 4, 10, 20, p) && sil_keep_rule(8, false, 4, 10, 20, p));  // a gap of 5: all of it
    CHECK(sil_keep_rule(7, false, 4, 11, 20, p) && !sil_keep_rule(8, false, 4, 11, 20, p) && sil_keep_rule(9, false, 4, 11, 20, p));  // 6 -> 5
    CHECK(sil_keep_rule(0, false, -1, 10, 20, p) && !sil_keep_rule(0, false, -1, 11, 20, p));  // lead_w = 10
    CHECK(sil_keep_rule(20, false, 0, 40, 40, p) && !sil_keep_rule(21, false, 0, 40, 40, p));  // trail_w = 20
    CHECK(sil_quiet_keep(100, p) == 30 && sil_quiet_keep(7, p) == 7);
    p.lead_w = p.trail_w = 0;
    CHECK(sil_quiet_keep(100, p) == 1);
    CHECK(sil_tile_win0(4096, 55) == 75 && sil_tile_win1(0, 100000, 55) == 75 && sil_tile_win1(4096, 4100, 55) == 75);
  }
  // the launches against the definition
  {
    const int rates[] = {8000, 11025, 22050, 48000, 96000};
    const size_t Ns[] = {1, 39, 40, 41, 109, 110, 111, 4095, 4096, 4097, 8192, 12345, 132000};
    Silence sets[4] = {d, d, d, d};
    sets[1].max_pause_ms = 105.0f, sets[1].threshold_db = -30.0f;
    sets[2].lead_ms = sets[2].trail_ms = 0.0f, sets[2].fade_ms = 0.0f, sets[2].max_pause_ms = 20.0f, sets[2].min_sound_ms = 0.0f;
    sets[3].lead_ms = sets[3].trail_ms = 10000.0f;
    uint32_t seed = 0;
    for (int rate : rates)
      for (size_t N : Ns)
        for (const Silence &s : sets) compare(signal(N, rate / 200, seed++), rate, s);
    compare(std::vector<float>(5000, 0.0f), 22050, d);  // no sound: the first lead_w + trail_w windows
    compare(std::vector<float>(5000, 0.25f), 22050, d);  // all sound
    // max_pause 0 with lead and trail at their maxima: the input's bits
    const std::vector<float> x = signal(30000, 110, 5);
    std::vector<float> out(x.size());
    const SilenceStats st = silence_reference(x.data(), x.size(), 22050, sets[3], out.data());
    CHECK(st.n_out == x.size() && st.n_cuts == 0 && std::memcmp(out.data(), x.data(), x.size() * sizeof(float)) == 0);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
