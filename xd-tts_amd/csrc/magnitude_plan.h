// magnitude_plan.h -- the host arithmetic of the magnitude chain between mel -> linear and the Griffin-Lim loop: what a request
// asks for (nothing, a uniform prosody, a contour, a pitch target over a contour), which stages run (the clean-up stage, tracker
// and target, then the contour or the uniform prosody, then timbre, then the SPSI initial phase), the frames F'_u behind them, the per-utterance
// records of the stages' launches, the totals every buffer is sized from, and the buffer the loop reads.  Plain host C++, no
// HIP: tests/magnitude_plan_test.cpp drives it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "denoise_plan.h"
#include "f0_plan.h"
#include "gl_plan.h"
#include "prosody_contour.h"
#include "timbre_plan.h"

namespace xdtts {

// ---- the records: one utterance of a stage's launch (kernels.h: launch_prosody_batch, launch_prosody_contour, launch_timbre,
// launch_f0_track, launch_spsi).  The utterances lie back to back, in the caller's order.
// F rows from row src0 of S -> Fout = prosody_frames(F, rate) rows from row dst0 of Sout (dst0[u + 1] = dst0[u] + Fout[u])
struct ProsodyUtt {
  int src0, F, dst0, Fout;
  float rate, pitch;
  int lifter;
  float log_floor;
};
// the contour form: ... and its frame table at entry tab0 of ftab; identity != 0: the rows are copied, no table is read
struct ContourUtt {
  int src0, F, dst0, Fout, tab0, lifter;
  float log_floor;
  int identity;
};
// F rows from row src0 of S -> F rows from row dst0 of Sout, under the fields of a Timbre
struct TimbreUtt {
  int src0, dst0, F;
  float vtl, breath;
  uint32_t seed;
  int lifter;
  float log_floor;
};
// rows row0 .. row0 + F (1 <= F <= F0_MAX_FRAMES) of raw / strength / f0 / ratio; tab0 = its entry in the contour frame table whose
// pitch slice takes the ratios, -1 = none; the fields of its PitchTarget
struct F0Utt {
  int row0, F, tab0, mode;
  float value, range;
};
// The SPSI recurrence over the frames runs as a scan over segments of SPSI_L consecutive frames of one utterance: the dependent
// depth is 2 SPSI_L + F / SPSI_L LDS gathers (82 at F = 800 with 24; 20 .. 32 are within 10 % of it), against F.
constexpr int SPSI_L = 24;
struct SpsiSeg {
  int row0;   // row of the segment's first frame in S / ang / tprev (the utterances of a batch lie one behind the other)
  int n;      // its frames, 1 .. SPSI_L
  int first;  // the utterance's first segment: it starts from phase 0
  int last;   // the utterance's last segment: nothing enters behind it
};
struct SpsiUtt {
  int seg0, nseg;  // the utterance's segments in the table
};
inline size_t spsi_segments(int F) { return (size_t)((F + SPSI_L - 1) / SPSI_L); }  // of one utterance

// ---- the uniform prosody (the layout of xdtts_prosody) and F' = F at rate 1, else max(floor((F - 1) / rate + 0.5), 1) + 1, in
// double; 0 for a bad argument
struct Prosody {
  float rate, pitch;
  int32_t lifter;
  float log_floor;
};
inline size_t prosody_frames(size_t F, float rate) {
  if (!std::isfinite(rate) || rate < 0.25f || rate > 4.0f) return 0;
  if (rate == 1.0f) return F;
  if (F < 2) return 0;
  const double n = std::floor((double)(F - 1) / (double)rate + 0.5);
  return (size_t)std::max(n, 1.0) + 1;
}

struct F0Job {  // the checked options of a tracker request with their quefrency range
  F0Opts opts;
  int q_lo = 0, q_hi = 0;
};

// ---- what a request of n utterances puts between mel -> linear and the loop: nothing, one uniform prosody each (checked by
// the caller), one contour table each (built by the caller for the utterance's frame count), or tables plus a tracker job with
// one target each -- the tracker and the target then run on S in front of the contour stage and multiply their ratios into the
// tables' pitches on the device.  Only these four can be built.
class MagnitudeRequest {
 public:
  enum Form { NONE, UNIFORM, CONTOUR };
  static MagnitudeRequest none(int n) { return MagnitudeRequest(NONE, n, {}, {}); }
  static MagnitudeRequest uniform(const Prosody *p, int n) { return MagnitudeRequest(UNIFORM, n, std::vector<Prosody>(p, p + n), {}); }
  static MagnitudeRequest contours(std::vector<ContourTable> tabs) {
    const int n = (int)tabs.size();
    return MagnitudeRequest(CONTOUR, n, {}, std::move(tabs));
  }
  static MagnitudeRequest targets(std::vector<ContourTable> tabs, const F0Job &job, std::vector<PitchTarget> t) {
    if (t.size() != tabs.size()) throw std::invalid_argument("one pitch target per contour table");
    MagnitudeRequest r = contours(std::move(tabs));
    r.tracked_ = true, r.job_ = job, r.targets_ = std::move(t);
    return r;
  }
  int n() const { return n_; }
  Form form() const { return form_; }
  bool tracked() const { return tracked_; }
  // utterance u passes the stage unchanged (its rows are copied where another utterance of the request is staged)
  bool identity(int u) const { return form_ == CONTOUR ? tabs_[(size_t)u].identity : (form_ == NONE || (pros_[(size_t)u].rate == 1.0f && pros_[(size_t)u].pitch == 1.0f)); }
  // F'_u for a mel of F frames
  int frames(int u, int F) const { return form_ == CONTOUR ? tabs_[(size_t)u].Fout : (form_ == UNIFORM ? (int)prosody_frames((size_t)F, pros_[(size_t)u].rate) : F); }
  const Prosody &prosody(int u) const { return pros_[(size_t)u]; }
  const ContourTable &table(int u) const { return tabs_[(size_t)u]; }
  const PitchTarget &target(int u) const { return targets_[(size_t)u]; }
  const F0Job &job() const { return job_; }

 private:
  MagnitudeRequest(Form f, int n, std::vector<Prosody> p, std::vector<ContourTable> t) : form_(f), n_(n), pros_(std::move(p)), tabs_(std::move(t)) {}
  Form form_;
  int n_;
  bool tracked_ = false;
  std::vector<Prosody> pros_;
  std::vector<ContourTable> tabs_;
  F0Job job_;
  std::vector<PitchTarget> targets_;
};

struct Contour {  // the contour of a target request (the layout of xdtts_prosody_contour)
  const ContourPoint *points;
  int32_t n_points, lifter;
  float log_floor;
};
// What a target request runs on, once the frame counts are known (checked targets; c, or an element of it, may be null): the
// contour tables -- the caller's, or the rate-1 table where an utterance under a target that is not the identity has no contour
// of its own (its identity flag is off: the stage reads the pitches the device writes).  active = some target is not the
// identity: without it the request is that of the contours alone (any_contour) or nothing.  "" or the failure's message.
inline std::string target_tables(const PitchTarget *t, const Contour *const *c, int n_utt, const size_t *n_frames, std::vector<ContourTable> &tabs,
                                 bool *active, bool *any_contour) {
  auto at = [](int u, const std::string &msg) { return "utterance " + std::to_string(u) + ": " + msg; };
  tabs.assign((size_t)n_utt, ContourTable());
  *active = *any_contour = false;
  for (int u = 0; u < n_utt; ++u) {
    *active = *active || !pitch_target_is_identity(t[u]);
    *any_contour = *any_contour || (c && c[u]);
  }
  for (int u = 0; u < n_utt; ++u) {
    const size_t F = n_frames[u];
    ContourTable &tab = tabs[(size_t)u];
    if (c && c[u]) {
      const std::string msg = contour_check(c[u]->points, c[u]->n_points, c[u]->lifter, c[u]->log_floor, F);
      if (!msg.empty()) return at(u, msg);
      contour_build(c[u]->points, c[u]->n_points, c[u]->lifter, c[u]->log_floor, F, tab);
    } else {
      tab.F = tab.Fout = (int)F;  // (the identity: no table)
    }
    if (*active && (F < 1 || F > F0_MAX_FRAMES))
      return at(u, "the pitch tracker takes 1 .. " + std::to_string(F0_MAX_FRAMES) + " frames, got " + std::to_string(F));
    if (pitch_target_is_identity(t[u])) continue;
    if (F < 2) return at(u, "a pitch target that is not the identity takes 2 .. " + std::to_string(F0_MAX_FRAMES) + " frames, got " + std::to_string(F));
    if (tab.identity) {  // the rate-1 table: c[m] = 65536 m, pitch 1, gain 1, F' = F
      tab.identity = false;
      tab.c.resize(F);
      for (size_t m = 0; m < F; ++m) tab.c[m] = (uint32_t)(65536u * m);
      tab.pitch.assign(F, 1.0f);
      tab.gain.assign(F, 1.0f);
    }
  }
  return "";
}

// ---- everything the host decides before a launch
struct MagnitudePlan {
  Rows in, rows;  // the mel's frames F_u, and the frames behind the prosody stage, F'_u: the rows of everything from there on
  std::vector<DenoiseUtt> clean;    // the clean-up stage, on the F_u rows of `in`, in front of everything: where it runs, its
                                    // output takes S's place for every stage below and for the loop (`loop` keeps its meaning)
  MagnitudeRequest::Form prosody = MagnitudeRequest::NONE;  // the form that runs; NONE: nothing is launched, S' is S
  bool track = false;  // the tracker and the targets run in front of it
  F0Job job;
  std::vector<ProsodyUtt> pros;     // per utterance; a stage that does not run has no records
  std::vector<ContourUtt> contour;
  std::vector<unsigned> ftab;       // the contour frame table: c, pitch, gain of all utterances, n_tab entries each (float bits),
  int n_tab = 0;                    // and with the tracker a fourth array, the pitches once more (what k_f0_track multiplies into `pitch` from)
  std::vector<F0Utt> f0;            // on the rows of S: the tracker looks at all of them
  std::vector<TimbreUtt> timbre;    // on the F' rows, src0 = dst0
  bool spsi = false, chained = false;  // chained: some utterance has more than one segment
  std::vector<SpsiSeg> spsi_segs;
  std::vector<SpsiUtt> spsi_utts;
  std::vector<int> frame_local;     // row -> frame index inside its utterance (the seeded phase of a batch)
  size_t loop_rows = 0;             // max(sum F, sum F'): what the loop's arrays are sized for
  enum Source { S, S_PROS, S_TIMBRE } loop = S;  // the buffer the loop reads
  bool staged() const { return prosody != MagnitudeRequest::NONE; }
};

// Fin[u]: the frames of utterance u's mel.  timbre: empty = the stage is off, one setting = every utterance's, else one each (the
// stage's hook).  phase_init 1 = SPSI.  always: a hook of a stage alone runs the request's form even where every utterance is the
// identity (a request path then launches nothing).  denoise: as timbre -- empty = the clean-up stage is off, one job = every
// utterance's, else one each (the stage's hook).  Throws std::length_error past 2^24 rows.
template <class Int>
inline MagnitudePlan magnitude_plan(const MagnitudeRequest &req, const Int *Fin, const std::vector<Timbre> &timbre, int phase_init,
                                    bool always = false, const std::vector<DenoiseJob> &denoise = std::vector<DenoiseJob>()) {
  MagnitudePlan p;
  const int n_utt = req.n();
  bool staged = always && req.form() != MagnitudeRequest::NONE;
  for (int u = 0; u < n_utt; ++u) staged = staged || !req.identity(u);
  p.prosody = staged ? req.form() : MagnitudeRequest::NONE;
  p.track = staged && req.tracked();
  if (p.track) p.job = req.job();
  size_t ntab = 0;
  for (int u = 0; p.prosody == MagnitudeRequest::CONTOUR && u < n_utt; ++u) ntab += req.table(u).c.size();
  if (p.prosody == MagnitudeRequest::CONTOUR) p.ftab.assign((size_t)(p.track ? 4 : 3) * std::max<size_t>(ntab, 1), 0u);
  for (int u = 0; u < n_utt; ++u) {
    const size_t F = (size_t)Fin[u], Fp = staged ? (size_t)req.frames(u, (int)F) : F;
    p.in.add(F, (size_t)1 << 24, "batch too large");
    p.rows.add(Fp, (size_t)1 << 24, "batch too large");
    const int src0 = p.in.row0[(size_t)u], dst0 = p.rows.row0[(size_t)u];
    if (!denoise.empty()) p.clean.push_back(denoise_utt(denoise[denoise.size() == 1 ? 0 : (size_t)u], src0, (int)F));
    if (p.prosody == MagnitudeRequest::UNIFORM) {
      const Prosody &q = req.prosody(u);
      p.pros.push_back({src0, (int)F, dst0, (int)Fp, q.rate, q.pitch, q.lifter, q.log_floor});
    } else if (p.prosody == MagnitudeRequest::CONTOUR) {
      const ContourTable &t = req.table(u);
      p.contour.push_back({src0, (int)F, dst0, (int)Fp, p.n_tab, t.lifter, t.log_floor, t.identity ? 1 : 0});
      if (p.track) p.f0.push_back({src0, (int)F, t.identity ? -1 : p.n_tab, req.target(u).mode, req.target(u).value, req.target(u).range});
      const size_t at = (size_t)p.n_tab, n = t.c.size();
      if (n) std::memcpy(&p.ftab[at], t.c.data(), n * sizeof(unsigned));
      if (n) std::memcpy(&p.ftab[ntab + at], t.pitch.data(), n * sizeof(float));
      if (n) std::memcpy(&p.ftab[2 * ntab + at], t.gain.data(), n * sizeof(float));
      if (n && p.track) std::memcpy(&p.ftab[3 * ntab + at], t.pitch.data(), n * sizeof(float));
      p.n_tab += (int)n;
    }
    if (!timbre.empty()) {
      const Timbre &t = timbre[timbre.size() == 1 ? 0 : (size_t)u];
      p.timbre.push_back({dst0, dst0, (int)Fp, t.vtl, t.breath, t.seed, t.lifter, t.log_floor});
    }
    if (phase_init == 1) {
      const int nseg = (int)spsi_segments((int)Fp);
      p.spsi_utts.push_back({(int)p.spsi_segs.size(), nseg});
      for (int k = 0; k < nseg; ++k) p.spsi_segs.push_back({dst0 + k * SPSI_L, std::min(SPSI_L, (int)Fp - k * SPSI_L), k == 0, k + 1 == nseg});
      p.chained = p.chained || nseg > 1;
    }
    for (size_t f = 0; f < Fp; ++f) p.frame_local.push_back((int)f);
  }
  p.spsi = phase_init == 1;
  p.loop_rows = std::max(p.in.total, p.rows.total);
  p.loop = !timbre.empty() ? MagnitudePlan::S_TIMBRE : (staged ? MagnitudePlan::S_PROS : MagnitudePlan::S);
  return p;
}

// The tracker alone on the rows `rows` (the hooks of the tracker): no target, no table
inline MagnitudePlan magnitude_plan_tracker(const Rows &rows, const F0Job &job) {
  MagnitudePlan p;
  p.in = p.rows = rows;
  p.track = true, p.job = job;
  for (int u = 0; u < rows.n(); ++u) p.f0.push_back({rows.row0[(size_t)u], rows.F[(size_t)u], -1, 0, 1.0f, 1.0f});
  p.loop_rows = rows.total;
  return p;
}

}  // namespace xdtts
