// magnitude.h -- the magnitude chain between mel -> linear and the Griffin-Lim loop as one member of the vocoder handle: its
// settings, the buffers, record tables and pinned stats of the stages (denoise.hip, f0.hip, prosody.hip, timbre.hip, phase_spsi.hip), and the
// ONE runner every request path goes through.  The arithmetic is magnitude_plan.h's.
#pragma once
#include "delivery.h"

namespace xdtts {

struct Magnitude {
  hipStream_t stream = nullptr;  // the handle's, as are the bins per frame and the twiddles
  int nb = 0;
  const float2 *tw = nullptr;

  // ---- settings (the setters and getters of api_gl_magnitude.cpp) ----
  Timbre timbre = timbre_default();  // the voice of the handle; the identity (the default) launches and allocates nothing
  bool timbre_on() const { return !timbre_is_identity(timbre); }
  int phase_init = 0;  // 0 = the seeded random stream, 1 = SPSI on the magnitude that enters the loop
  std::vector<Timbre> timbres() const { return timbre_on() ? std::vector<Timbre>(1, timbre) : std::vector<Timbre>(); }  // as magnitude_plan takes them
  // the clean-up stage (denoise.hip), the first of the chain; the identity (the default) launches and allocates nothing.  The
  // setter (behind a drained stream) leaves the profile and the tone curve E on the device.
  Denoise denoise = denoise_default();
  bool denoise_profiled = false;
  std::vector<float> denoise_profile;  // the caller's, as set (the getter's)
  DevBuf<float> dn_profile, dn_tone;   // [nb] each
  bool denoise_on() const { return !denoise_is_identity(denoise); }
  std::vector<DenoiseJob> denoises() const { return denoise_on() ? std::vector<DenoiseJob>(1, denoise_job(denoise, denoise_profiled, 0)) : std::vector<DenoiseJob>(); }

  // ---- buffers: grow with the request and stay; a growth happens behind a drained stream (every request path starts there).
  // Every stage writes out of place: S stays as mel -> linear left it, S_clean, S_pros and S_timbre as their stages left them ----
  DevBuf<float> S_clean;           // [sum F][nb]
  DevBuf<float> dn_N;              // [n_utt][nb]: the selected noise magnitude of each utterance
  DevBuf<DenoiseStats> dn_stats;   // one per utterance
  PinnedArray<DenoiseStats> dn_host;  // the stats travel back behind the stage
  DevBuf<float> dn_hook_profile, dn_hook_tone;  // the hooks of the stage alone: their profile [nb] and tone curves [n_utt][nb]
  DevBuf<float> S_pros, S_timbre;  // [sum F'][nb] each
  DevBuf<float> f0_raw, f0_strength, f0_val, f0_ratio;  // per row the tracker looks at
  DevBuf<F0Stats> f0_stats;        // one per utterance
  PinnedArray<F0Stats> f0_host;    // the stats travel back behind the tracker
  DevBuf<uint2> spsi_map, spsi_comp;
  DevBuf<unsigned> spsi_entry, spsi_turns;  // spsi_turns: the parity hooks only

  // ---- the request in flight: its plan (whose vectors are the sources of the tables' uploads: they stay until the next
  // prepare(), which every path calls behind a drained stream) and the tables on the device ----
  MagnitudePlan plan;
  bool tables = false;  // the uniform, timbre and SPSI launches read the device tables; else record 0 travels as a kernel argument
  DevBuf<ProsodyUtt> pros_tab;
  DevBuf<ContourUtt> contour_utts;
  DevBuf<unsigned> contour_ftab;
  DevBuf<F0Utt> f0_utts;
  DevBuf<TimbreUtt> timbre_tab;
  DevBuf<DenoiseUtt> clean_tab;
  DevBuf<SpsiSeg> spsi_segs;
  DevBuf<SpsiUtt> spsi_utts;
  DevBuf<int> frame_local;
  // p becomes the plan in place and the buffers are sized for it.  The contour's and the tracker's tables go up on the stream
  // in either form.  with_tables: the other records and frame_local go up too and the stream is drained behind them.  Without:
  // one utterance, whose records travel as kernel arguments; nothing else is uploaded and nothing is waited for.
  void prepare(MagnitudePlan p, bool with_tables);
  // The stages of the plan in place on S [sum F][nb], in the fixed order, on the stream; returns the magnitude the loop reads
  // (S, S_pros or S_timbre; where the clean-up stage runs, S_clean stands for S).  Any number of times: a retry finds S, S_clean,
  // S_pros and S_timbre intact.  The initial phase is the loop's first step: where the plan says so it calls spsi() on what
  // run() returned.
  float *run(float *S);
  float *base_S(float *S) const { return plan.clean.empty() ? S : S_clean.p; }  // what every stage behind the clean-up reads
  float *loop_S(float *S) const { return plan.loop == MagnitudePlan::S_TIMBRE ? S_timbre.p : (plan.loop == MagnitudePlan::S_PROS ? S_pros.p : base_S(S)); }
  // ... the stages one by one, for run() and the hooks of a stage alone
  // -> S_clean, dn_stats, dn_host (profile [nb], tone [.][nb]: the setting's or a hook's; between: behind k_noise_profile)
  void clean(const float *S, const float *profile, const float *tone, hipEvent_t between = nullptr);
  void track(const float *S, hipEvent_t between = nullptr);  // -> f0_*, the table's pitches, f0_host (between: behind k_f0_frames)
  void prosody(const float *S);                               // -> S_pros
  void voice(const float *S_in);                              // -> S_timbre
  void spsi(const float *S_in, float2 *ang, float2 *tprev, unsigned *turns = nullptr);

  // ---- what the tracker of the last call found, in the caller's order (xdtts_griffinlim_last_f0) ----
  std::vector<xdtts_f0_stats> last_f0;
  void collect();  // behind a drained stream: the pinned stats -> last_f0 (nothing where the plan in place has no tracker)
  // ---- ... and what the clean-up stage did (xdtts_griffinlim_last_denoise) ----
  std::vector<xdtts_denoise_stats> last_denoise;
  void collect_clean();  // behind a drained stream: the pinned stats of the plan in place are APPENDED (a sequence: utterance by utterance)
};

}  // namespace xdtts
