// api_gl_magnitude.cpp -- the extern "C" boundary, vocoder half: the entries that work on the magnitude between mel -> linear and
// the loop -- prosody, contours, the pitch tracker and pitch targets, the SPSI initial phase, timbre, the clean-up stage.
#include <algorithm>
#include <cmath>

#include "api_gl.h"

using namespace xdtts;

// The parity hook of a magnitude stage alone: the utterances' magnitudes one behind the other on the device (rows plan.in of S),
// ev.e[3], the plan in place (with_tables: the form a batch runs -- the tables go up and the stream is drained; else the single
// request's), ev.e[0], the stage, ev.e[1], the rows plan.rows of the buffer it returns back in the boundary layout (ev.e[2]
// behind the layout change), the wait.
template <class Stage>
static void stage_hook(xdtts_griffinlim *g, const float *const *S, MagnitudePlan plan, bool with_tables, float *const *S_outs, Stage stage) {  // (the caller holds g->mu)
  HIP_CHECK(hipSetDevice(g->device));
  g->bufs((int)plan.loop_rows);  // (frames: the boundary-layout staging of both directions)
  g->upload_rows(S, plan.in);
  HIP_CHECK(hipEventRecord(g->ev.e[3], g->stream));
  g->mg.prepare(std::move(plan), with_tables);
  HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
  const float *out = stage(g->mg);
  HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));  // last_timings: ms[0] = the stage alone, ms[1] = the layout change behind it
  rows_to_host(g, out, g->mg.plan.rows, S_outs);
  g->finish_timings();  // (drains the stream: the tables and the outputs)
}
static void frames_out(const xdtts_griffinlim *g, size_t *n_frames_out) {
  for (int u = 0; n_frames_out && u < g->mg.plan.rows.n(); ++u) n_frames_out[u] = (size_t)g->mg.plan.rows.F[(size_t)u];
}
static const std::vector<Timbre> NO_TIMBRE;

extern "C" {

// ---- prosody: rate and pitch on the magnitude between mel -> linear and the loop (prosody.hip) --------------------------------

void xdtts_prosody_default(xdtts_prosody *p) {
  if (!p) return;
  p->rate = 1.0f;
  p->pitch = 1.0f;
  p->lifter = 30;  // quefrencies below 1.4 ms: under the pitch period of any voice (2.5 ms at 400 Hz), above the formant ripple
  p->log_floor = 1e-5f;
}

size_t xdtts_prosody_frames(size_t n_frames, float rate) { return prosody_frames(n_frames, rate); }

xdtts_status xdtts_griffinlim_prosody_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_prosody *p,
                                             float *S_out, size_t *n_frames_out) {
  return guard([&] {
    if (n_frames_out) *n_frames_out = 0;
    if (!g || !S || !p || !S_out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_frames == 0) fail(XDTTS_ERR_BAD_ARG, "need at least 1 frame");
    MagnitudePlan plan = magnitude_plan_checked(magnitude_request(MagnitudeAsk::prosody(p), 1, &n_frames), &n_frames, NO_TIMBRE, 0);
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, &S, std::move(plan), false, &S_out, [&](Magnitude &m) { return m.run(g->S.p); });  // (the identity launches nothing: S's bits)
    frames_out(g, n_frames_out);
  });
}

xdtts_status xdtts_griffinlim_infer_prosody(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            const xdtts_prosody *p, float **audio, size_t *n_samples) {
  return guard([&] {
    if (audio) *audio = nullptr;
    if (n_samples) *n_samples = 0;
    if (!g || !mel || !p || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    mel_check(g, n_mels, n_frames);
    infer_host_mel(g, mel, n_mels, n_frames, magnitude_request(MagnitudeAsk::prosody(p), 1, &n_frames), audio, n_samples);
  });
}

// ... for a batch, one prosody per utterance: audios[u] has hop * (F'_u - 1) samples.  The prosody array is checked first, so
// that a bad field is reported without a handle.
xdtts_status xdtts_griffinlim_infer_batch_prosody(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                                  int32_t n_utt, const xdtts_prosody *p, float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    null_outputs(audios, n_samples, n_utt);
    prosody_check_array(p, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, MagnitudeAsk::prosody(p), audios, n_samples);
}

// Parity hook of the ragged stage alone: the utterances' magnitudes one behind the other on the device, one k_prosody_batch
// launch, and back.  last_timings as after xdtts_griffinlim_prosody_linear: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_prosody_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                   const xdtts_prosody *p, float *const *S_outs, size_t *n_frames_out) {
  return guard([&] {
    for (int u = 0; n_frames_out && u < n_utt; ++u) n_frames_out[u] = 0;
    prosody_check_array(p, n_utt);
    if (!g || !S || !n_frames || !S_outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (n_frames[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 1 frame", u);
      prosody_check_at(&p[u], u, n_frames[u]);
    }
    MagnitudePlan plan = magnitude_plan_checked(magnitude_request(MagnitudeAsk::prosody(p), n_utt, nullptr), n_frames, NO_TIMBRE, 0, true);
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, S, std::move(plan), true, S_outs, [&](Magnitude &m) { return m.prosody(g->S.p), m.S_pros.p; });
    frames_out(g, n_frames_out);
  });
}

// ---- prosody contours: rate, pitch and gain that vary inside an utterance (prosody_contour.h, prosody.hip: k_prosody_contour) ----

void xdtts_prosody_contour_default(xdtts_prosody_contour *c) {
  if (!c) return;
  c->points = nullptr;
  c->n_points = 0;
  c->lifter = 30;
  c->log_floor = 1e-5f;
}

size_t xdtts_prosody_contour_frames(const xdtts_prosody_contour *c, size_t n_frames) {
  if (!c) return 0;
  return contour_frames(reinterpret_cast<const ContourPoint *>(c->points), c->n_points, c->lifter, c->log_floor, n_frames);
}

xdtts_status xdtts_prosody_contour_table(const xdtts_prosody_contour *c, size_t n_frames, uint32_t *cum, float *pitch, float *gain) {
  return guard([&] {
    contour_check(c, n_frames);
    if (n_frames < 1 || n_frames > CONTOUR_MAX_FRAMES) fail(XDTTS_ERR_BAD_ARG, "contour n_frames: the table takes 1 .. %zu frames, got %zu", CONTOUR_MAX_FRAMES, n_frames);
    contour_fill(reinterpret_cast<const ContourPoint *>(c->points), c->n_points, n_frames, cum, pitch, gain);
  });
}

// Parity hook of the stage alone: the utterances' magnitudes one behind the other on the device, the table upload and one
// k_prosody_contour launch (identity utterances are copied), and back.  last_timings: ms[0] = the launch alone, ms[1] = the
// layout change behind it, ms[2] = both and the table's upload in front of them.
xdtts_status xdtts_griffinlim_contour_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                   const xdtts_prosody_contour *c, float *const *S_outs, size_t *n_frames_out) {
  return guard([&] {
    for (int u = 0; n_frames_out && u < n_utt; ++u) n_frames_out[u] = 0;
    contour_check_array(c, n_utt);
    if (!S || !n_frames || !S_outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<ContourTable> tabs((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (n_frames[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 1 frame", u);
      contour_check_at(&c[u], u, n_frames[u]);
      contour_table(c[u], n_frames[u], tabs[(size_t)u]);
    }
    MagnitudePlan plan = magnitude_plan_checked(MagnitudeRequest::contours(std::move(tabs)), n_frames, NO_TIMBRE, 0, true);
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");  // (behind the contours and their frame counts: those need no device)
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, S, std::move(plan), false, S_outs, [&](Magnitude &m) { return m.prosody(g->S.p), m.S_pros.p; });  // (ev.e[0]: behind the table's upload)
    HIP_CHECK(hipEventElapsedTime(&g->last_ms[2], g->ev.e[3], g->ev.e[2]));  // the total takes the table's upload in
    frames_out(g, n_frames_out);
  });
}

xdtts_status xdtts_griffinlim_contour_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_prosody_contour *c,
                                             float *S_out, size_t *n_frames_out) {
  if (!c) {
    if (n_frames_out) *n_frames_out = 0;
    return guard([&] { fail(XDTTS_ERR_BAD_ARG, "null contour"); });
  }
  return xdtts_griffinlim_contour_linear_batch(g, &S, &n_frames, 1, c, &S_out, n_frames_out);
}

xdtts_status xdtts_griffinlim_infer_contour(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            const xdtts_prosody_contour *c, float **audio, size_t *n_samples) {
  return guard([&] {
    if (audio) *audio = nullptr;
    if (n_samples) *n_samples = 0;
    contour_check(c, std::max<size_t>(n_frames, 2));  // the fields first: reported without a handle
    if (!g || !mel || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    mel_check(g, n_mels, n_frames);
    infer_host_mel(g, mel, n_mels, n_frames, magnitude_request(MagnitudeAsk::contour(c), 1, &n_frames), audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch_contour(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                                  int32_t n_utt, const xdtts_prosody_contour *c, float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    null_outputs(audios, n_samples, n_utt);
    contour_check_array(c, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, MagnitudeAsk::contour(c), audios, n_samples);
}

// ---- pitch tracker and pitch targets (f0_plan.h, f0.hip: k_f0_frames, k_f0_track) ----------------------------------------------

void xdtts_f0_opts_default(xdtts_f0_opts *o) {
  if (!o) return;
  const F0Opts d = f0_opts_default();
  std::memcpy(o, &d, sizeof d);
}

void xdtts_pitch_target_default(xdtts_pitch_target *t) {
  if (!t) return;
  const PitchTarget d = pitch_target_default();
  std::memcpy(t, &d, sizeof d);
}

xdtts_status xdtts_f0_plan(const xdtts_f0_opts *o, int32_t *q_lo, int32_t *q_hi) {
  return guard([&] {
    if (q_lo) *q_lo = 0;
    if (q_hi) *q_hi = 0;
    const F0Job j = f0_job_checked(o);
    if (q_lo) *q_lo = j.q_lo;
    if (q_hi) *q_hi = j.q_hi;
  });
}

xdtts_status xdtts_f0_track_reference(const float *raw, const float *strength, size_t n_frames, const xdtts_f0_opts *o,
                                      const xdtts_pitch_target *t, float *f0_out, float *ratio_out, xdtts_f0_stats *stats) {
  return guard([&] {
    const F0Job j = f0_job_checked(o);
    xdtts_pitch_target td;
    xdtts_pitch_target_default(&td);
    pitch_target_check_array(t ? t : &td, 1);
    if (!raw || !strength) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_frames < 1 || n_frames > F0_MAX_ROWS) fail(XDTTS_ERR_BAD_ARG, "f0 reference: need 1 .. 2^20 frames, got %zu", n_frames);
    PitchTarget pt;
    std::memcpy(&pt, t ? t : &td, sizeof pt);
    F0Stats st;
    f0_track_reference(raw, strength, n_frames, j.opts, pt, f0_out, ratio_out, &st);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_last_f0(const xdtts_griffinlim *g, xdtts_f0_stats *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->mg.last_f0 : nullptr, true, out, cap, n);
}

// The tracker's results of the rows `rows` to the host (any array, and any element of one, may be null), the wait, the stats.
// Behind Magnitude::track() on g->stream; ev.e[0 .. 2] recorded by the caller.
static void f0_fetch(xdtts_griffinlim *g, const Rows &rows, float *const *raw_outs, float *const *strength_outs, float *const *f0_outs,
                     float *const *ratio_outs, xdtts_f0_stats *stats) {
  for (int u = 0; u < rows.n(); ++u) {
    const size_t r0 = (size_t)rows.row0[(size_t)u], nbytes = (size_t)rows.F[(size_t)u] * sizeof(float);
    if (raw_outs && raw_outs[u]) HIP_CHECK(hipMemcpyAsync(raw_outs[u], g->mg.f0_raw.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (strength_outs && strength_outs[u]) HIP_CHECK(hipMemcpyAsync(strength_outs[u], g->mg.f0_strength.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (f0_outs && f0_outs[u]) HIP_CHECK(hipMemcpyAsync(f0_outs[u], g->mg.f0_val.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (ratio_outs && ratio_outs[u]) HIP_CHECK(hipMemcpyAsync(ratio_outs[u], g->mg.f0_ratio.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
  }
  g->finish_timings();  // (drains the stream)
  g->clear_last();
  g->mg.collect();
  if (stats && !g->mg.last_f0.empty()) std::memcpy(stats, g->mg.last_f0.data(), g->mg.last_f0.size() * sizeof(xdtts_f0_stats));
}

// The tracker alone on S_dev [rows.total][nb]: no target, no table.  ms[0] = k_f0_frames, ms[1] = k_f0_track.
static void f0_run(xdtts_griffinlim *g, const float *S_dev, const Rows &rows, const F0Job &job, float *const *raw_outs,
                   float *const *strength_outs, float *const *f0_outs, xdtts_f0_stats *stats) {
  g->mg.prepare(magnitude_plan_tracker(rows, job), false);
  HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
  g->mg.track(S_dev, g->ev.e[1]);
  HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
  f0_fetch(g, rows, raw_outs, strength_outs, f0_outs, nullptr, stats);
}

static void f0_rows_checked(Rows &rows, const size_t *n_frames, int n_utt) {
  for (int u = 0; u < n_utt; ++u) {
    if (n_frames[u] < 1 || n_frames[u] > F0_MAX_FRAMES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: the pitch tracker takes 1 .. %zu frames, got %zu", u, F0_MAX_FRAMES, n_frames[u]);
    rows_add(rows, n_frames[u], F0_MAX_ROWS, "batch too large: more than 2^20 frames");
  }
}

xdtts_status xdtts_griffinlim_f0_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                              const xdtts_f0_opts *o, float *const *raw_outs, float *const *strength_outs,
                                              float *const *f0_outs, xdtts_f0_stats *stats) {
  return guard([&] {
    const F0Job job = f0_job_checked(o);
    if (n_utt < 1) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!S || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    Rows rows;
    for (int u = 0; u < n_utt; ++u)
      if (!S[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
    f0_rows_checked(rows, n_frames, n_utt);
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)rows.total);
    g->upload_rows(S, rows);
    f0_run(g, g->S.p, rows, job, raw_outs, strength_outs, f0_outs, stats);
  });
}

xdtts_status xdtts_griffinlim_f0_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_f0_opts *o,
                                        float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats) {
  return xdtts_griffinlim_f0_linear_batch(g, &S, &n_frames, 1, o, &raw_out, &strength_out, &f0_out, stats);
}

xdtts_status xdtts_griffinlim_f0(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames, const xdtts_f0_opts *o,
                                 float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats) {
  return guard([&] {
    const F0Job job = f0_job_checked(o);
    if (!g || !mel) fail(XDTTS_ERR_BAD_ARG, "null argument");
    mel_check(g, n_mels);
    Rows rows;
    f0_rows_checked(rows, &n_frames, 1);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)n_frames);
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    g->mel_to_linear(g->mel_in.p, (int)n_frames);
    f0_run(g, g->S.p, rows, job, &raw_out, &strength_out, &f0_out, stats);
  });
}

xdtts_status xdtts_griffinlim_f0_audio(xdtts_griffinlim *g, const float *audio, size_t n_samples, const xdtts_f0_opts *o,
                                       float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats) {
  return guard([&] {
    const F0Job job = f0_job_checked(o);
    if (!g || !audio) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_samples == 0 || n_samples >= ((size_t)1 << 28)) fail(XDTTS_ERR_BAD_ARG, "need 1 .. 2^28 - 1 samples, got %zu", n_samples);
    const size_t F = n_samples / (size_t)g->hop + 1;
    Rows rows;
    f0_rows_checked(rows, &F, 1);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    gl_analysis_enqueue(g, &audio, &n_samples, rows, false);
    f0_run(g, g->an_S.p, rows, job, &raw_out, &strength_out, &f0_out, stats);
  });
}

// Parity hook of the application: the magnitudes one behind the other on the device, the tables (with the pitches kept a second
// time), k_f0_frames, k_f0_track -- which writes the tables' pitches -- and k_prosody_contour, and back.  The hook always runs
// the tracker: under identity targets the ratios are 1 and the utterances are copied.  ms[0] = k_f0_frames, ms[1] = the rest.
xdtts_status xdtts_griffinlim_pitch_target_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames,
                                                        int32_t n_utt, const xdtts_f0_opts *o, const xdtts_pitch_target *t,
                                                        const xdtts_prosody_contour *const *c, float *const *S_outs,
                                                        float *const *ratio_outs, xdtts_f0_stats *stats) {
  return guard([&] {
    const F0Job job = f0_job_checked(o);
    pitch_target_check_array(t, n_utt);
    if (!S || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (c && c[u]) contour_check_at(c[u], u, std::max<size_t>(n_frames[u], 2));  // the fields first
    }
    Rows in;
    f0_rows_checked(in, n_frames, n_utt);
    MagnitudePlan plan = magnitude_plan_checked(magnitude_request(MagnitudeAsk::target(&job, t, c, true), n_utt, n_frames, 0), n_frames, NO_TIMBRE, 0, true);
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)plan.loop_rows);
    g->upload_rows(S, in);
    g->mg.prepare(std::move(plan), false);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->mg.track(g->S.p, g->ev.e[1]);
    g->mg.prosody(g->S.p);
    rows_to_host(g, g->mg.S_pros.p, g->mg.plan.rows, S_outs);
    f0_fetch(g, in, nullptr, nullptr, nullptr, ratio_outs, stats);
  });
}

xdtts_status xdtts_griffinlim_pitch_target_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_f0_opts *o,
                                                  const xdtts_pitch_target *t, const xdtts_prosody_contour *c, float *S_out,
                                                  float *ratio_out, xdtts_f0_stats *stats) {
  return xdtts_griffinlim_pitch_target_linear_batch(g, &S, &n_frames, 1, o, t, c ? &c : nullptr, &S_out, &ratio_out, stats);
}

xdtts_status xdtts_griffinlim_infer_pitch_target(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                                 const xdtts_f0_opts *o, const xdtts_pitch_target *t, const xdtts_prosody_contour *c,
                                                 float **audio, size_t *n_samples) {
  return guard([&] {
    if (audio) *audio = nullptr;
    if (n_samples) *n_samples = 0;
    const F0Job job = f0_job_checked(o);  // the fields first: reported without a handle
    pitch_target_check_array(t, 1);
    if (c) contour_check(c, std::max<size_t>(n_frames, 2));
    if (!g || !mel || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    mel_check(g, n_mels, n_frames);
    infer_host_mel(g, mel, n_mels, n_frames, magnitude_request(MagnitudeAsk::target(&job, t, c ? &c : nullptr), 1, &n_frames), audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch_pitch_target(xdtts_griffinlim *g, const float *const *mels, size_t n_mels,
                                                       const size_t *n_frames, int32_t n_utt, const xdtts_f0_opts *o,
                                                       const xdtts_pitch_target *t, const xdtts_prosody_contour *const *c,
                                                       float **audios, size_t *n_samples) {
  F0Job job;
  xdtts_status st = guard([&] {
    null_outputs(audios, n_samples, n_utt);
    job = f0_job_checked(o);
    pitch_target_check_array(t, n_utt);
    for (int u = 0; c && u < n_utt; ++u)
      if (c[u]) contour_check_at(c[u], u, 2);
  });
  if (st != XDTTS_OK) return st;
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, MagnitudeAsk::target(&job, t, c), audios, n_samples);
}

// ---- initial phase: the seeded random stream (0) or Single Pass Spectrogram Inversion (1; phase_spsi.hip) ---------------------

xdtts_status xdtts_griffinlim_set_phase_init(xdtts_griffinlim *g, int32_t mode) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    if (mode != 0 && mode != 1) fail(XDTTS_ERR_BAD_ARG, "phase_init must be 0 (seeded random) or 1 (SPSI), got %d", mode);
    std::lock_guard<std::mutex> lk(g->mu);
    g->mg.phase_init = mode;
  });
}

xdtts_status xdtts_griffinlim_get_phase_init(const xdtts_griffinlim *g, int32_t *mode) {
  return guard([&] {
    if (!g || !mode) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *mode = g->mg.phase_init;
  });
}

// Parity hook of the ragged stage alone: the utterances' magnitudes one behind the other on the device, the launches of
// phase_spsi.hip, and back.  last_timings: ms[0] = the stage alone, ms[1] = the layout change behind it.
xdtts_status xdtts_griffinlim_spsi_phase_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                               uint32_t *const *turns, float *const *angles) {
  return guard([&] {
    if (!g || !S || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    Rows rows;
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (n_frames[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 1 frame", u);
      if (n_frames[u] > ((size_t)1 << 20)) fail(XDTTS_ERR_BAD_ARG, "utterance %d: at most 2^20 frames, got %zu", u, n_frames[u]);
      rows_add(rows, n_frames[u], (size_t)1 << 20, "batch too large: more than 2^20 frames");
    }
    const std::vector<int> &Fu = rows.F, &row0 = rows.row0;
    const size_t Ftot = rows.total;
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const size_t nb = (size_t)g->nb, ne = Ftot * nb;
    GlBufs b = g->bufs((int)Ftot);
    g->upload_rows(S, rows);
    g->mg.prepare(magnitude_plan_checked(MagnitudeRequest::none(n_utt), n_frames, NO_TIMBRE, 1), n_utt > 1);  // (one utterance: the form the single-utterance entries run)
    g->mg.spsi_turns.alloc(ne);
    g->phase0.alloc(ne * 3);  // staging in the boundary layout: the angles, then the turns
    float2 *ang_out = reinterpret_cast<float2 *>(g->phase0.p);
    unsigned *turns_out = reinterpret_cast<unsigned *>(g->phase0.p + ne * 2);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->mg.spsi(g->S.p, b.ang, b.tprev, g->mg.spsi_turns.p);
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)row0[(size_t)u] * nb;
      launch_spsi_export(g->mg.spsi_turns.p + r0, b.ang + r0, Fu[(size_t)u], g->nb, turns_out + r0, ang_out + r0, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)row0[(size_t)u] * nb, n = (size_t)Fu[(size_t)u] * nb;
      if (turns && turns[u]) HIP_CHECK(hipMemcpyAsync(turns[u], turns_out + r0, n * sizeof(uint32_t), hipMemcpyDeviceToHost, g->stream));
      if (angles && angles[u]) HIP_CHECK(hipMemcpyAsync(angles[u], ang_out + r0, n * sizeof(float2), hipMemcpyDeviceToHost, g->stream));
    }
    g->finish_timings();  // (drains the stream)
  });
}

xdtts_status xdtts_griffinlim_spsi_phase(xdtts_griffinlim *g, const float *S, size_t n_frames, uint32_t *turns, float *angles) {
  return xdtts_griffinlim_spsi_phase_batch(g, &S, &n_frames, 1, &turns, &angles);
}

// ---- timbre: vocal-tract length and breathiness, the voice of a handle (timbre_plan.h, timbre.hip) --------------------------------

void xdtts_timbre_default(xdtts_timbre *t) {
  if (!t) return;
  const Timbre d = timbre_default();
  std::memcpy(t, &d, sizeof d);
}

uint32_t xdtts_timbre_noise_bits(uint32_t seed, uint32_t frame, uint32_t bin) { return timbre_noise_bits(seed, frame, bin); }

xdtts_status xdtts_griffinlim_set_timbre(xdtts_griffinlim *g, const xdtts_timbre *t) {
  return guard([&] {
    const Timbre s = timbre_checked(t);  // (the fields before the handle; a failure leaves the setting as it was)
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->mg.timbre = s;
  });
}

xdtts_status xdtts_griffinlim_get_timbre(xdtts_griffinlim *g, xdtts_timbre *t) {
  return guard([&] {
    if (!g || !t) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    std::memcpy(t, &g->mg.timbre, sizeof g->mg.timbre);
  });
}

// Parity hook of the stage alone: the utterances' magnitudes one behind the other on the device, ONE k_timbre launch -- with
// the table for several utterances, with the record as a kernel argument for one (the form the single-utterance entries run)
// -- and back.  A request of identities alone touches no device.  last_timings: ms[0] = the stage alone, ms[1] = the layout change.
xdtts_status xdtts_griffinlim_timbre_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                  const xdtts_timbre *t, float *const *S_outs) {
  return guard([&] {
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!t) fail(XDTTS_ERR_BAD_ARG, "null timbre");
    std::vector<Timbre> ts((size_t)n_utt);
    bool any = false;
    for (int u = 0; u < n_utt; ++u) {
      std::string msg;
      std::memcpy(&ts[(size_t)u], &t[u], sizeof(Timbre));
      msg = timbre_check(ts[(size_t)u]);
      if (msg.empty() && n_frames) msg = timbre_frames_check(n_frames[u]);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      any = any || !timbre_is_identity(ts[(size_t)u]);
    }
    if (!g || !S || !n_frames || !S_outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
    MagnitudePlan plan = magnitude_plan_checked(MagnitudeRequest::none(n_utt), n_frames, ts, 0);
    std::lock_guard<std::mutex> lk(g->mu);
    if (!any) {  // the identity: S's bits, nothing launched, nothing allocated
      for (int u = 0; u < n_utt; ++u)
        if (S_outs[u] != S[u]) std::memmove(S_outs[u], S[u], n_frames[u] * (size_t)g->nb * sizeof(float));
      return;
    }
    stage_hook(g, S, std::move(plan), n_utt > 1, S_outs, [&](Magnitude &m) { return m.voice(g->S.p), m.S_timbre.p; });
  });
}

xdtts_status xdtts_griffinlim_timbre_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_timbre *t, float *S_out) {
  return xdtts_griffinlim_timbre_linear_batch(g, &S, &n_frames, 1, t, &S_out);
}

// ---- clean-up: spectral subtraction with a floor and a tone curve, the first stage of the chain (denoise_plan.h, denoise.hip) ----

void xdtts_denoise_default(xdtts_denoise *d) {
  if (!d) return;
  const Denoise s = denoise_default();
  std::memcpy(d, &s, sizeof s);
}

uint32_t xdtts_denoise_rank(size_t n_frames, float quantile) { return denoise_rank(n_frames, quantile); }

float xdtts_denoise_floor(float floor_db) { return denoise_floor(floor_db); }

xdtts_status xdtts_denoise_tone(const xdtts_denoise *d, float *E) {
  return guard([&] {
    if (!d || !E) fail(XDTTS_ERR_BAD_ARG, "null argument");
    denoise_tone(denoise_checked(d, nullptr), E);
  });
}

xdtts_status xdtts_denoise_reference(const float *S, size_t n_frames, const xdtts_denoise *d, const float *profile, float *S_out,
                                     xdtts_denoise_stats *stats) {
  return guard([&] {
    if (!d) fail(XDTTS_ERR_BAD_ARG, "null denoise");
    const Denoise s = denoise_checked(d, profile);
    bad_arg_if(denoise_frames_check(n_frames));
    if (!S || !S_out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    DenoiseStats st;
    denoise_reference(S, n_frames, s, profile, S_out, &st);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_denoise(xdtts_griffinlim *g, const xdtts_denoise *d, const float *profile) {
  return guard([&] {
    const Denoise s = denoise_checked(d, d ? profile : nullptr);  // (the fields before the handle; a failure leaves the setting as it was)
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    const bool profiled = d && profile;
    std::vector<float> E((size_t)DENOISE_NB), P(profiled ? profile : nullptr, profiled ? profile + DENOISE_NB : nullptr);
    denoise_tone(s, E.data());
    std::lock_guard<std::mutex> lk(g->mu);
    if (!denoise_is_identity(s)) {  // (the identity allocates nothing)
      HIP_CHECK(hipSetDevice(g->device));
      HIP_CHECK(hipStreamSynchronize(g->stream));  // as a growth: nothing in flight reads what is replaced
      g->mg.dn_tone.upload(E.data(), E.size(), g->stream);
      if (profiled) g->mg.dn_profile.upload(P.data(), P.size(), g->stream);
      HIP_CHECK(hipStreamSynchronize(g->stream));
    }
    g->mg.denoise = s;
    g->mg.denoise_profiled = profiled;
    g->mg.denoise_profile = std::move(P);
  });
}

xdtts_status xdtts_griffinlim_get_denoise(xdtts_griffinlim *g, xdtts_denoise *d, float *profile_out, int32_t *profiled) {
  return guard([&] {
    if (!g || !d) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    std::memcpy(d, &g->mg.denoise, sizeof g->mg.denoise);
    if (profiled) *profiled = g->mg.denoise_profiled ? 1 : 0;
    if (profile_out && g->mg.denoise_profiled) std::memcpy(profile_out, g->mg.denoise_profile.data(), (size_t)DENOISE_NB * sizeof(float));
  });
}

xdtts_status xdtts_griffinlim_last_denoise(const xdtts_griffinlim *g, xdtts_denoise_stats *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->mg.last_denoise : nullptr, false, out, cap, n);
}

// Parity hook of the stage alone: the utterances' magnitudes one behind the other on the device, the selection where an
// utterance asks for it and ONE k_denoise launch -- with the table for several utterances, with the record as a kernel argument
// for one (the form the single-utterance entries run) -- and back.  A request of identities alone touches no device.
// last_timings: ms[0] = the stage alone, ms[1] = the layout change.
xdtts_status xdtts_griffinlim_denoise_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                   const xdtts_denoise *d, const float *profile, float *const *S_outs) {
  return guard([&] {
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!d) fail(XDTTS_ERR_BAD_ARG, "null denoise");
    std::vector<DenoiseJob> jobs((size_t)n_utt);
    std::vector<float> tones;  // one row per utterance with a curve that is not flat
    bool any = false;
    for (int u = 0; u < n_utt; ++u) {
      Denoise s;
      std::memcpy(&s, &d[u], sizeof s);
      std::string msg = denoise_check(s);
      if (msg.empty() && n_frames) msg = denoise_frames_check(n_frames[u]);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      any = any || !denoise_is_identity(s);
      int row = -1;
      if (!denoise_tone_is_flat(s)) {
        row = (int)(tones.size() / (size_t)DENOISE_NB);
        tones.resize(tones.size() + (size_t)DENOISE_NB);
        denoise_tone(s, tones.data() + (size_t)row * DENOISE_NB);
      }
      jobs[(size_t)u] = denoise_job(s, profile != nullptr, row);
    }
    bad_arg_if(denoise_profile_check(profile));
    if (!g || !S || !n_frames || !S_outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
    MagnitudePlan plan = magnitude_plan_checked(MagnitudeRequest::none(n_utt), n_frames, NO_TIMBRE, 0, false, jobs);
    std::lock_guard<std::mutex> lk(g->mu);
    if (!any) {  // the identity: S's bits, nothing launched, nothing allocated
      for (int u = 0; u < n_utt; ++u)
        if (S_outs[u] != S[u]) std::memmove(S_outs[u], S[u], n_frames[u] * (size_t)g->nb * sizeof(float));
      return;
    }
    stage_hook(g, S, std::move(plan), n_utt > 1, S_outs, [&](Magnitude &m) {
      if (profile) m.dn_hook_profile.upload(profile, (size_t)DENOISE_NB, g->stream);  // (the sources outlive the hook's final wait)
      if (!tones.empty()) m.dn_hook_tone.upload(tones.data(), tones.size(), g->stream);
      return m.clean(g->S.p, m.dn_hook_profile.p, m.dn_hook_tone.p), m.S_clean.p;
    });
    g->clear_last();
    g->mg.collect_clean();
  });
}

xdtts_status xdtts_griffinlim_denoise_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_denoise *d,
                                             const float *profile, float *S_out) {
  return xdtts_griffinlim_denoise_linear_batch(g, &S, &n_frames, 1, d, profile, &S_out);
}

// The selection alone: the magnitude on the device, ONE k_noise_profile launch in the single form, N back.  ms[0] = the launch.
xdtts_status xdtts_griffinlim_noise_profile(xdtts_griffinlim *g, const float *S, size_t n_frames, float quantile, float *out) {
  return guard([&] {
    bad_arg_if(denoise_quantile_check(quantile));
    bad_arg_if(denoise_frames_check(n_frames));
    if (!g || !S || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    Denoise s = denoise_default();
    s.strength = 1.0f, s.quantile = quantile;
    MagnitudePlan plan = magnitude_plan_checked(MagnitudeRequest::none(1), &n_frames, NO_TIMBRE, 0, false, std::vector<DenoiseJob>(1, denoise_job(s, false, -1)));
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)plan.loop_rows);
    g->upload_rows(&S, plan.in);
    g->mg.prepare(std::move(plan), false);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    launch_noise_profile(g->S.p, nullptr, 1, g->mg.plan.clean[0], g->mg.dn_N.p, g->stream);
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    HIP_CHECK(hipMemcpyAsync(out, g->mg.dn_N.p, (size_t)DENOISE_NB * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    g->finish_timings();  // (drains the stream)
  });
}

}  // extern "C"
