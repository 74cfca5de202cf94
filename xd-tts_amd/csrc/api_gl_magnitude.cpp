// api_gl_magnitude.cpp -- the extern "C" boundary, vocoder half: the entries that work on the magnitude between mel -> linear and
// the loop -- prosody, contours, the pitch tracker and pitch targets, the SPSI initial phase, timbre.
#include <algorithm>
#include <cmath>

#include "api_gl.h"

using namespace xdtts;

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
    prosody_check(p, n_frames);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const int F = (int)n_frames, Fmax = std::max(F, (int)prosody_frames(n_frames, p->rate));
    g->bufs(Fmax);
    // boundary layout (nb x F) -> device layout [F][nb], the stage, and back: (nb x F')
    g->frames.upload(S, (size_t)F * g->nb, g->stream);
    launch_transpose(g->frames.p, g->S.p, g->nb, F, g->stream);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    const int Fp = g->prosody(ProsodyArg(p), F);
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));  // last_timings: ms[0] = the stage alone, ms[1] = the layout change behind it
    launch_transpose(g->prosody_S(ProsodyArg(p)), g->frames.p, Fp, g->nb, g->stream);
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    HIP_CHECK(hipMemcpyAsync(S_out, g->frames.p, (size_t)Fp * g->nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    g->finish_timings();  // (drains the stream)
    if (n_frames_out) *n_frames_out = (size_t)Fp;
  });
}

xdtts_status xdtts_griffinlim_infer_prosody(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            const xdtts_prosody *p, float **audio, size_t *n_samples) {
  return guard([&] {
    if (audio) *audio = nullptr;
    if (n_samples) *n_samples = 0;
    if (!g || !mel || !p || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    mel_check(g, n_mels, n_frames);
    prosody_check(p, n_frames);
    infer_host_mel(g, mel, n_mels, n_frames, ProsodyArg(p), audio, n_samples);
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
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, p, nullptr, audios, n_samples);
}

// Parity hook of the ragged stage alone: the utterances' magnitudes one behind the other on the device, one k_prosody_batch
// launch, and back.  last_timings as after xdtts_griffinlim_prosody_linear: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_prosody_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                   const xdtts_prosody *p, float *const *S_outs, size_t *n_frames_out) {
  return guard([&] {
    for (int u = 0; n_frames_out && u < n_utt; ++u) n_frames_out[u] = 0;
    prosody_check_array(p, n_utt);
    if (!g || !S || !n_frames || !S_outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<ProsodyUtt> tab((size_t)n_utt);
    Rows in, out;
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (n_frames[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 1 frame", u);
      prosody_check_at(&p[u], u, n_frames[u]);
      const size_t Fp = prosody_frames(n_frames[u], p[u].rate);
      tab[(size_t)u] = {(int)in.total, (int)n_frames[u], (int)out.total, (int)Fp, p[u].rate, p[u].pitch, p[u].lifter, p[u].log_floor};
      rows_add(in, n_frames[u], (size_t)1 << 24, "batch too large");
      rows_add(out, Fp, (size_t)1 << 24, "batch too large");
    }
    const size_t Fout = out.total;
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const size_t nb = (size_t)g->nb;
    g->bufs((int)std::max(in.total, Fout));  // (frames: the boundary-layout staging of both directions)
    g->S_pros.alloc(Fout * nb);
    g->pros_tab.upload(tab.data(), tab.size(), g->stream);
    g->upload_rows(S, in);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    if (env::equals(env::PROSODY_BATCH, "loop")) {  // developer comparison aid (tools/prosody_check.py): one k_prosody launch per utterance
      for (const ProsodyUtt &t : tab)
        launch_prosody(g->S.p + (size_t)t.src0 * nb, g->S_pros.p + (size_t)t.dst0 * nb, t.F, t.Fout, t.rate, t.pitch, t.lifter, t.log_floor, g->tw.p, g->stream);
    } else {
      launch_prosody_batch(g->S.p, g->S_pros.p, g->pros_tab.p, n_utt, (int)Fout, g->tw.p, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    rows_to_host(g, g->S_pros.p, out, S_outs);
    g->finish_timings();  // (drains the stream: the table and the outputs)
    for (int u = 0; n_frames_out && u < n_utt; ++u) n_frames_out[u] = (size_t)tab[(size_t)u].Fout;
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
    Rows in, out;
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      if (n_frames[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 1 frame", u);
      contour_check_at(&c[u], u, n_frames[u]);
      contour_table(c[u], n_frames[u], tabs[(size_t)u]);
      rows_add(in, n_frames[u], (size_t)1 << 24, "batch too large");
      rows_add(out, (size_t)tabs[(size_t)u].Fout, (size_t)1 << 24, "batch too large");
    }
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");  // (behind the contours and their frame counts: those need no device)
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)std::max(in.total, out.total));  // (frames: the boundary-layout staging of both directions)
    g->upload_rows(S, in);
    HIP_CHECK(hipEventRecord(g->ev.e[3], g->stream));
    g->contour_upload(tabs.data(), n_utt);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->contour_launch();
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    rows_to_host(g, g->S_pros.p, out, S_outs);
    g->finish_timings();  // (drains the stream: the tables and the outputs)
    HIP_CHECK(hipEventElapsedTime(&g->last_ms[2], g->ev.e[3], g->ev.e[2]));  // the total takes the table's upload in
    for (int u = 0; n_frames_out && u < n_utt; ++u) n_frames_out[u] = (size_t)out.F[(size_t)u];
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
    ContourTable tab;
    contour_table(*c, n_frames, tab);
    infer_host_mel(g, mel, n_mels, n_frames, ProsodyArg(&tab), audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch_contour(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                                  int32_t n_utt, const xdtts_prosody_contour *c, float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    null_outputs(audios, n_samples, n_utt);
    contour_check_array(c, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, nullptr, c, audios, n_samples);
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
  return last_stats_out(g, g ? &g->last_f0 : nullptr, true, out, cap, n);
}

// The tracker's results of the rows `rows` to the host (any array, and any element of one, may be null), the wait, the stats.
// Behind f0_launch() on g->stream; ev.e[0 .. 2] recorded by the caller.
static void f0_fetch(xdtts_griffinlim *g, const Rows &rows, float *const *raw_outs, float *const *strength_outs, float *const *f0_outs,
                     float *const *ratio_outs, xdtts_f0_stats *stats) {
  for (int u = 0; u < rows.n(); ++u) {
    const size_t r0 = (size_t)rows.row0[(size_t)u], nbytes = (size_t)rows.F[(size_t)u] * sizeof(float);
    if (raw_outs && raw_outs[u]) HIP_CHECK(hipMemcpyAsync(raw_outs[u], g->f0_raw.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (strength_outs && strength_outs[u]) HIP_CHECK(hipMemcpyAsync(strength_outs[u], g->f0_strength.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (f0_outs && f0_outs[u]) HIP_CHECK(hipMemcpyAsync(f0_outs[u], g->f0_val.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
    if (ratio_outs && ratio_outs[u]) HIP_CHECK(hipMemcpyAsync(ratio_outs[u], g->f0_ratio.p + r0, nbytes, hipMemcpyDeviceToHost, g->stream));
  }
  g->finish_timings();  // (drains the stream)
  g->clear_last();
  g->f0_collect();
  if (stats && !g->last_f0.empty()) std::memcpy(stats, g->last_f0.data(), g->last_f0.size() * sizeof(xdtts_f0_stats));
}

// The tracker alone on S_dev [rows.total][nb]: no target, no table.  ms[0] = k_f0_frames, ms[1] = k_f0_track.
static void f0_run(xdtts_griffinlim *g, const float *S_dev, const Rows &rows, const F0Job &job, float *const *raw_outs,
                   float *const *strength_outs, float *const *f0_outs, xdtts_f0_stats *stats) {
  std::vector<F0Utt> utts;
  for (int u = 0; u < rows.n(); ++u) utts.push_back({rows.row0[(size_t)u], rows.F[(size_t)u], -1, 0, 1.0f, 1.0f});
  g->f0_prepare(utts);
  HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
  g->f0_launch(S_dev, job, nullptr, 0, g->ev.e[1]);
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
    Rows in, out;
    f0_rows_checked(in, n_frames, n_utt);
    TargetPlan plan;
    target_plan(job, t, c, n_utt, n_frames, plan);
    for (int u = 0; u < n_utt; ++u) rows_add(out, (size_t)plan.tabs[(size_t)u].Fout, (size_t)1 << 24, "batch too large");
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)std::max(in.total, out.total));
    g->upload_rows(S, in);
    g->contour_upload(plan.tabs.data(), n_utt, true);
    g->f0_prepare_contour(plan.job);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->f0_launch(g->S.p, plan.job, g->contour_ftab.p, g->contour_n_tab, g->ev.e[1]);
    g->contour_launch();
    rows_to_host(g, g->S_pros.p, out, S_outs);
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
    TargetPlan plan;
    target_plan(job, t, c ? &c : nullptr, 1, &n_frames, plan);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    gl_run_from_device_mel(g, g->mel_in.p, (int)n_frames, plan.arg(), audio, n_samples);
    if (plan.active) g->f0_collect();
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
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, nullptr, nullptr, audios, n_samples, &job, t, c);
}

// ---- initial phase: the seeded random stream (0) or Single Pass Spectrogram Inversion (1; phase_spsi.hip) ---------------------

xdtts_status xdtts_griffinlim_set_phase_init(xdtts_griffinlim *g, int32_t mode) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    if (mode != 0 && mode != 1) fail(XDTTS_ERR_BAD_ARG, "phase_init must be 0 (seeded random) or 1 (SPSI), got %d", mode);
    std::lock_guard<std::mutex> lk(g->mu);
    g->phase_init = mode;
  });
}

xdtts_status xdtts_griffinlim_get_phase_init(const xdtts_griffinlim *g, int32_t *mode) {
  return guard([&] {
    if (!g || !mode) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *mode = g->phase_init;
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
    xdtts_griffinlim::SpsiTables tab;
    g->spsi_tables(Fu, tab);
    g->spsi_turns.alloc(ne);
    g->phase0.alloc(ne * 3);  // staging in the boundary layout: the angles, then the turns
    float2 *ang_out = reinterpret_cast<float2 *>(g->phase0.p);
    unsigned *turns_out = reinterpret_cast<unsigned *>(g->phase0.p + ne * 2);
    HIP_CHECK(hipStreamSynchronize(g->stream));  // the host tables
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    if (n_utt == 1) g->spsi(g->S.p, Fu[0], b.ang, b.tprev, g->spsi_turns.p);  // (the form the single-utterance entries run)
    else g->spsi_batch(g->S.p, tab, b.ang, b.tprev, g->spsi_turns.p);
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)row0[(size_t)u] * nb;
      launch_spsi_export(g->spsi_turns.p + r0, b.ang + r0, Fu[(size_t)u], g->nb, turns_out + r0, ang_out + r0, g->stream);
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
    g->timbre = s;
  });
}

xdtts_status xdtts_griffinlim_get_timbre(xdtts_griffinlim *g, xdtts_timbre *t) {
  return guard([&] {
    if (!g || !t) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    std::memcpy(t, &g->timbre, sizeof g->timbre);
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
    Rows rows;
    for (int u = 0; u < n_utt; ++u) {
      if (!S[u] || !S_outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null magnitude", u);
      rows_add(rows, n_frames[u], (size_t)1 << 24, "batch too large");
    }
    std::lock_guard<std::mutex> lk(g->mu);
    const size_t nb = (size_t)g->nb;
    if (!any) {  // the identity: S's bits, nothing launched, nothing allocated
      for (int u = 0; u < n_utt; ++u)
        if (S_outs[u] != S[u]) std::memmove(S_outs[u], S[u], n_frames[u] * nb * sizeof(float));
      return;
    }
    HIP_CHECK(hipSetDevice(g->device));
    g->bufs((int)rows.total);  // (frames: the boundary-layout staging of both directions)
    g->S_timbre.alloc(rows.total * nb);
    g->timbre_tab_host.clear();
    for (int u = 0; u < n_utt; ++u) g->timbre_tab_host.push_back(timbre_utt(rows.row0[(size_t)u], rows.row0[(size_t)u], rows.F[(size_t)u], ts[(size_t)u]));
    if (n_utt > 1) g->timbre_tab.upload(g->timbre_tab_host.data(), g->timbre_tab_host.size(), g->stream);
    g->upload_rows(S, rows);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    if (n_utt == 1) g->timbre_one(g->S.p, rows.F[0], ts[0]);
    else g->timbre_rows(g->S.p, (int)rows.total);
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    rows_to_host(g, g->S_timbre.p, rows, S_outs);
    g->finish_timings();  // (drains the stream: the table and the outputs)
  });
}

xdtts_status xdtts_griffinlim_timbre_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_timbre *t, float *S_out) {
  return xdtts_griffinlim_timbre_linear_batch(g, &S, &n_frames, 1, t, &S_out);
}

}  // extern "C"
