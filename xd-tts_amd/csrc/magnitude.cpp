// magnitude.cpp -- the magnitude chain's state and its one runner (magnitude.h): buffers, the record tables' uploads and the
// launches of clean-up -> tracker + target -> contour | uniform prosody -> timbre, and of the SPSI initial phase, for a single request and a batch.
#include "magnitude.h"

#include "env.h"

namespace xdtts {

static_assert(sizeof(xdtts_f0_stats) == sizeof(F0Stats), "F0Stats is xdtts_f0_stats");
static_assert(sizeof(xdtts_denoise_stats) == sizeof(DenoiseStats) && sizeof(xdtts_denoise) == sizeof(Denoise) && sizeof(Denoise) == 80,
              "the layouts of denoise_plan.h");

void Magnitude::prepare(MagnitudePlan p, bool with_tables) {
  plan = std::move(p);
  tables = with_tables;
  const size_t cells = std::max<size_t>(plan.rows.total, 1) * (size_t)nb, n_utt = std::max<size_t>((size_t)plan.rows.n(), 1);
  if (!plan.clean.empty()) {
    S_clean.alloc(std::max<size_t>(plan.in.total, 1) * (size_t)nb);
    dn_N.alloc(plan.clean.size() * (size_t)nb);
    dn_stats.alloc(plan.clean.size());
    dn_host.reserve(plan.clean.size());
  }
  if (plan.staged()) S_pros.alloc(cells);
  if (!plan.timbre.empty()) S_timbre.alloc(cells);
  if (plan.prosody == MagnitudeRequest::CONTOUR) {
    contour_utts.upload(plan.contour.data(), plan.contour.size(), stream);
    contour_ftab.upload(plan.ftab.data(), plan.ftab.size(), stream);
  }
  if (plan.track) {
    const size_t n = std::max<size_t>(plan.in.total, 1);
    for (DevBuf<float> *b : {&f0_raw, &f0_strength, &f0_val, &f0_ratio}) b->alloc(n);
    f0_stats.alloc(n_utt);
    f0_host.reserve(n_utt);
    f0_utts.upload(plan.f0.data(), plan.f0.size(), stream);
  }
  if (plan.spsi) {
    spsi_map.alloc(cells);
    spsi_comp.alloc(plan.spsi_segs.size() * (size_t)nb);
    spsi_entry.alloc(plan.spsi_segs.size() * (size_t)nb);
  }
  if (!tables) return;
  frame_local.upload(plan.frame_local.data(), plan.frame_local.size(), stream);
  if (plan.prosody == MagnitudeRequest::UNIFORM) pros_tab.upload(plan.pros.data(), plan.pros.size(), stream);
  if (!plan.timbre.empty()) timbre_tab.upload(plan.timbre.data(), plan.timbre.size(), stream);
  if (!plan.clean.empty()) clean_tab.upload(plan.clean.data(), plan.clean.size(), stream);
  if (plan.spsi) {
    spsi_segs.upload(plan.spsi_segs.data(), plan.spsi_segs.size(), stream);
    spsi_utts.upload(plan.spsi_utts.data(), plan.spsi_utts.size(), stream);
  }
  HIP_CHECK(hipStreamSynchronize(stream));  // the tables are up
}

// The selection where some utterance asks for it, then the pointwise kernel over all rows; the stats' `floored` is zeroed on the
// stream in front of them, so a retry counts afresh.
void Magnitude::clean(const float *S, const float *profile, const float *tone, hipEvent_t between) {
  const int n_utt = (int)plan.clean.size();
  bool selects = false;
  for (const DenoiseUtt &t : plan.clean) selects = selects || denoise_utt_selects(t);
  HIP_CHECK(hipMemsetAsync(dn_stats.p, 0, (size_t)n_utt * sizeof(DenoiseStats), stream));
  if (selects) launch_noise_profile(S, tables ? clean_tab.p : nullptr, n_utt, tables ? DenoiseUtt{} : plan.clean[0], dn_N.p, stream);
  if (between) HIP_CHECK(hipEventRecord(between, stream));
  launch_denoise(S, S_clean.p, tables ? clean_tab.p : nullptr, n_utt, tables ? DenoiseUtt{} : plan.clean[0], (int)plan.in.total, dn_N.p, profile,
                 tone, dn_stats.p, stream);
  HIP_CHECK(hipMemcpyAsync(dn_host.p, dn_stats.p, (size_t)n_utt * sizeof(DenoiseStats), hipMemcpyDeviceToHost, stream));
}

void Magnitude::track(const float *S, hipEvent_t between) {
  const int n_utt = (int)plan.f0.size();
  launch_f0_frames(S, (int)plan.in.total, plan.job.opts, plan.job.q_lo, plan.job.q_hi, tw, f0_raw.p, f0_strength.p, stream);
  if (between) HIP_CHECK(hipEventRecord(between, stream));
  launch_f0_track(f0_raw.p, f0_strength.p, f0_utts.p, n_utt, plan.job.opts.threshold, f0_val.p, f0_ratio.p, f0_stats.p,
                  plan.prosody == MagnitudeRequest::CONTOUR ? contour_ftab.p : nullptr, plan.n_tab, stream);
  HIP_CHECK(hipMemcpyAsync(f0_host.p, f0_stats.p, (size_t)n_utt * sizeof(F0Stats), hipMemcpyDeviceToHost, stream));
}

// Both forms: the contour's one kernel reads its tables for one utterance and for many; the uniform stage is one k_prosody
// launch with the record as arguments, or the ragged k_prosody_batch over the table.
void Magnitude::prosody(const float *S) {
  const int n_utt = plan.rows.n(), rows = (int)plan.rows.total;
  if (plan.prosody == MagnitudeRequest::CONTOUR) {
    launch_prosody_contour(S, S_pros.p, contour_utts.p, n_utt, contour_ftab.p, plan.n_tab, rows, tw, stream);
  } else if (!tables || env::equals(env::PROSODY_BATCH, "loop")) {  // (loop: developer comparison aid, tools/prosody_check.py)
    for (const ProsodyUtt &t : plan.pros)
      launch_prosody(S + (size_t)t.src0 * nb, S_pros.p + (size_t)t.dst0 * nb, t.F, t.Fout, t.rate, t.pitch, t.lifter, t.log_floor, tw, stream);
  } else {
    launch_prosody_batch(S, S_pros.p, pros_tab.p, n_utt, rows, tw, stream);
  }
}

void Magnitude::voice(const float *S_in) {
  launch_timbre(S_in, S_timbre.p, tables ? timbre_tab.p : nullptr, (int)plan.timbre.size(), tables ? TimbreUtt{} : plan.timbre[0], (int)plan.rows.total,
                tw, stream);
}

void Magnitude::spsi(const float *S_in, float2 *ang, float2 *tprev, unsigned *turns) {
  launch_spsi(S_in, (int)plan.rows.total, tables ? spsi_segs.p : nullptr, tables ? spsi_utts.p : nullptr, (int)plan.spsi_segs.size(),
              (int)plan.spsi_utts.size(), plan.chained, SpsiBufs{spsi_map.p, spsi_comp.p, spsi_entry.p}, ang, tprev, turns, stream);
}

// THE magnitude order: the clean-up stage on what mel -> linear left, then on its output (or on S) the tracker and the targets,
// which write the contour table's pitches, then the contour or the uniform prosody, then the handle's timbre on what that left
// (the tracker saw the voice before prosody and timbre).
float *Magnitude::run(float *S) {
  if (!plan.clean.empty()) clean(S, dn_profile.p, dn_tone.p);
  float *B = base_S(S);
  if (plan.track) track(B);
  if (plan.staged()) prosody(B);
  if (!plan.timbre.empty()) voice(plan.staged() ? S_pros.p : B);
  return loop_S(S);
}

void Magnitude::collect() {
  if (!plan.track) return;
  last_f0.resize(plan.f0.size());
  if (!last_f0.empty()) std::memcpy(last_f0.data(), f0_host.p, last_f0.size() * sizeof(F0Stats));
}

void Magnitude::collect_clean() {
  const size_t n = plan.clean.size(), at = last_denoise.size();
  if (!n) return;
  last_denoise.resize(at + n);
  std::memcpy(last_denoise.data() + at, dn_host.p, n * sizeof(DenoiseStats));
}

}  // namespace xdtts
