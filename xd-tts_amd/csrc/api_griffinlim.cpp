// api_griffinlim.cpp -- the extern "C" boundary, vocoder half: argument checks and locking; the work is in griffinlim_handle.cpp.
// Here: filter bank, handle, options, the infer entries, the loop's parity hooks, timings, analysis.  The entries of the magnitude
// stages are in api_gl_magnitude.cpp, those of the delivery chain and the stream in api_gl_delivery.cpp.
#include <algorithm>
#include <cmath>
#include <memory>

#include "api_gl.h"

using namespace xdtts;

// GriffinLim::infer for several utterances at once (the vocoder half of a batch, BASELINE.json configs[3]):
// the utterances' frames are concatenated, mel -> linear is one GEMM over all of them, and the persistent
// kernel takes as many utterances per launch as fit one workgroup per CU.  Every utterance's audio is bit-identical to what
// xdtts_griffinlim_infer returns for it alone.  (the arguments: api_gl.h)
xdtts_status xdtts::gl_infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames, int32_t n_utt,
                                   const MagnitudeAsk &ask, float **audios, size_t *n_samples) {
  return guard([&] {
    if (!g || !mels || !n_frames || !audios || !n_samples || n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    mel_check(g, n_mels);
    Rows rows;
    for (int u = 0; u < n_utt; ++u) {
      audios[u] = nullptr;
      n_samples[u] = 0;
      if (!mels[u] || n_frames[u] < 2) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 2 frames", u);
      rows_add(rows, n_frames[u], (size_t)1 << 24, "batch too large");
    }
    const MagnitudeRequest req = magnitude_request(ask, n_utt, n_frames, 0);
    const size_t Ftot = rows.total;
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    // mel of all utterances side by side: [n_mels][Ftot], staged in pinned memory (one fast upload)
    PinnedGuard mel_all((size_t)n_mels * Ftot);
    for (int u = 0; u < n_utt; ++u)
      for (size_t m = 0; m < n_mels; ++m)
        std::memcpy(mel_all.p + m * Ftot + rows.row0[u], mels[u] + m * n_frames[u], sizeof(float) * n_frames[u]);
    g->mel_in.upload(mel_all.p, (size_t)n_mels * Ftot, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));  // the staging buffer goes back to the pool
    gl_batch_from_device(g, g->mel_in.p, rows.F, audios, n_samples, req);
  });
}

extern "C" {

xdtts_status xdtts_mel_filter_bank(float sample_rate, size_t n_fft, size_t n_mels, float fmin, float fmax_or_nan,
                                   float *out) {
  return guard([&] {
    if (!out || n_fft < 2 || n_mels == 0 || !(sample_rate > 0)) fail(XDTTS_ERR_BAD_ARG, "bad filter bank request");
    const double sr = sample_rate;
    const double fmax = std::isnan(fmax_or_nan) ? sr / 2.0 : (double)fmax_or_nan;  // Option<f32>::None
    xdtts::mel_filter_bank(sr, (int)n_fft, (int)n_mels, fmin, fmax, out);
  });
}

xdtts_status xdtts_griffinlim_new(const float *mel_basis, size_t n_mels, size_t n_bins, size_t noverlap, float power,
                                  size_t iters, float momentum, int32_t device_id, xdtts_griffinlim **out) {
  return guard([&] {
    if (!out) fail(XDTTS_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    if (!mel_basis || n_mels == 0 || n_bins < 2) fail(XDTTS_ERR_BAD_ARG, "bad mel basis");
    const size_t n_fft = 2 * (n_bins - 1);
    if (n_fft != 1024) fail(XDTTS_ERR_BAD_ARG, "n_fft %zu unsupported: the framed-FFT kernel is built for 1024", n_fft);
    if (noverlap >= n_fft) fail(XDTTS_ERR_BAD_ARG, "noverlap %zu must be < n_fft %zu", noverlap, n_fft);
    if (n_fft - noverlap != n_fft / 4)
      fail(XDTTS_ERR_BAD_ARG, "hop %zu unsupported: the framed-FFT kernels are built for hop = n_fft/4 = 256 (mod.rs:456)", n_fft - noverlap);
    if (n_mels % 16 != 0) fail(XDTTS_ERR_BAD_ARG, "n_mels %zu must be a multiple of 16", n_mels);
    // (written so that a NaN fails each test: `momentum < 0` alone is false for it)
    if (!(power > 0) || !std::isfinite(power)) fail(XDTTS_ERR_BAD_ARG, "power %g must be finite and > 0", (double)power);
    if (!(momentum >= 0) || !std::isfinite(momentum)) fail(XDTTS_ERR_BAD_ARG, "momentum %g must be finite and >= 0", (double)momentum);
    device_id = select_device(device_id);
    auto g = std::make_unique<xdtts_griffinlim>();
    g->device = device_id;
    g->n_mels = (int)n_mels;
    g->nb = (int)n_bins;
    g->n_fft = (int)n_fft;
    g->hop = (int)(n_fft - noverlap);
    g->iters = (int)iters;
    g->power = power;
    g->momentum = momentum;
    HIP_CHECK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->dl.stream = g->mg.stream = g->stream;
    g->mg.nb = g->nb;
    g->ev.create();
    g->an_ev.create();
    std::vector<float> pinv;
    host_pinv(mel_basis, (int)n_mels, (int)n_bins, pinv);
    g->pinv.upload(pinv.data(), pinv.size(), g->stream);
    {  // NNLS refinement operands: the basis and its transpose, bins zero-padded to NBP, and the step 1/L
      const int NBP = xdtts_griffinlim::NBP, nm = (int)n_mels, nbi = (int)n_bins;
      std::vector<float> bp((size_t)nm * NBP, 0.f), bt((size_t)NBP * nm, 0.f);
      for (int i = 0; i < nm; ++i)
        for (int b = 0; b < nbi; ++b) bp[(size_t)i * NBP + b] = bt[(size_t)b * nm + i] = mel_basis[(size_t)i * nbi + b];
      g->basis_p.upload(bp.data(), bp.size(), g->stream);
      g->basisT_p.upload(bt.data(), bt.size(), g->stream);
      g->nnls_step = (float)(1.0 / host_lipschitz(mel_basis, nm, nbi));
      g->dl.norm_parts.alloc(GLN_SCRATCH);
    }
    std::vector<float2> tw(n_fft);
    std::vector<float> win(n_fft);
    const double PI = 3.14159265358979323846;
    for (size_t k = 0; k < n_fft; ++k) {
      tw[k] = make_float2((float)std::cos(2.0 * PI * k / n_fft), (float)(-std::sin(2.0 * PI * k / n_fft)));
      win[k] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * k / n_fft));  // periodic hann
    }
    g->tw.upload(tw.data(), tw.size(), g->stream);
    g->win.upload(win.data(), win.size(), g->stream);
    g->mg.tw = g->tw.p;
    HIP_CHECK(hipStreamSynchronize(g->stream));
    *out = g.release();
  });
}

void xdtts_griffinlim_opts_default(xdtts_griffinlim_opts *o) {
  if (!o) return;
  o->nnls_iters = 0;
  o->power_mode = 0;
  o->mel_decompress = 0;
  o->output_normalise = 3;  // rms, never past +-1: the level of the reference's own WAV_SPEC files
  o->batch_shape = 0;
  o->rms_target = 0.1f;
}

xdtts_status xdtts_griffinlim_set_opts(xdtts_griffinlim *g, const xdtts_griffinlim_opts *o) {
  return guard([&] {
    if (!g || !o) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (o->nnls_iters < 0 || o->nnls_iters > 100000 || o->power_mode < 0 || o->power_mode > 2 || o->mel_decompress < 0 ||
        o->mel_decompress > 2 || o->output_normalise < 0 || o->output_normalise > 3 || !(o->rms_target > 0.f) || !(o->rms_target <= 1e6f) || (o->batch_shape != 0 && o->batch_shape != 4))
      fail(XDTTS_ERR_BAD_ARG, "griffin-lim option out of range");
    std::lock_guard<std::mutex> lk(g->mu);
    g->gopts = *o;
  });
}

xdtts_status xdtts_griffinlim_get_opts(const xdtts_griffinlim *g, xdtts_griffinlim_opts *o) {
  return guard([&] {
    if (!g || !o) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *o = g->gopts;
  });
}

xdtts_status xdtts_griffinlim_set_seed(xdtts_griffinlim *g, uint32_t seed) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->seed = seed;
  });
}

xdtts_status xdtts_griffinlim_infer(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                    float **audio, size_t *n_samples) {
  return guard([&] {
    if (!g || !mel || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    *audio = nullptr;
    *n_samples = 0;
    mel_check(g, n_mels, n_frames);
    infer_host_mel(g, mel, n_mels, n_frames, MagnitudeRequest::none(1), audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                          int32_t n_utt, float **audios, size_t *n_samples) {
  return gl_infer_batch(g, mels, n_mels, n_frames, n_utt, MagnitudeAsk(), audios, n_samples);
}

// Host arithmetic: gl_batch_plan on the arguments gl_batch_from_device would hand it now (gl_batch_args), nothing launched
xdtts_status xdtts_griffinlim_batch_plan(xdtts_griffinlim *g, const size_t *n_frames, int32_t n_utt, int32_t *TF, int32_t *WG,
                                         int32_t *n_launches, int32_t *launch_of, int32_t *n_cu, int32_t *per_cu4) {
  return guard([&] {
    if (!g || !n_frames || n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    Rows rows;
    for (int u = 0; u < n_utt; ++u) {
      if (n_frames[u] < 2) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 2 frames", u);
      rows_add(rows, n_frames[u], (size_t)1 << 24, "batch too large");
    }
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const GlBatchArgs a = gl_batch_args(g);
    const GlBatchPlan plan = gl_batch_plan(rows.F, g->hop, a.n_cu, a.per_cu4, a.batch_shape, a.force);
    if (TF) *TF = plan.TF;
    if (WG) *WG = plan.WG;
    if (n_launches) *n_launches = (int32_t)plan.launches.size();
    if (n_cu) *n_cu = a.n_cu;
    if (per_cu4) *per_cu4 = a.per_cu4;
    if (launch_of) {
      for (int u = 0; u < n_utt; ++u) launch_of[u] = -1;
      for (size_t k = 0; k < plan.launches.size(); ++k)
        for (int u : plan.launches[k].utts) launch_of[u] = (int32_t)k;
    }
  });
}

xdtts_status xdtts_griffinlim_mel_to_linear(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            float *S_out) {
  return guard([&] {
    if (!g || !mel || !S_out || n_frames == 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    mel_check(g, n_mels);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const int F = (int)n_frames;
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    g->bufs(F);
    g->mel_to_linear(g->mel_in.p, F);
    // S is [F][nb] on the device; the boundary layout is the crate's (nb x F)
    g->frames.alloc((size_t)F * g->n_fft);
    launch_transpose(g->S.p, g->frames.p, F, g->nb, g->stream);
    HIP_CHECK(hipMemcpyAsync(S_out, g->frames.p, (size_t)F * g->nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
  });
}

xdtts_status xdtts_griffinlim_infer_linear(xdtts_griffinlim *g, const float *S, const float *phase0, size_t n_frames,
                                           size_t iters, float **audio, size_t *n_samples) {
  return guard([&] {
    if (!g || !S || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    *audio = nullptr;
    *n_samples = 0;
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const int F = (int)n_frames;
    GlBufs b = g->bufs(F);
    // boundary layout (nb x F) -> device layout [F][nb]
    g->frames.upload(S, (size_t)F * g->nb, g->stream);
    launch_transpose(g->frames.p, g->S.p, g->nb, F, g->stream);
    const float *p0 = nullptr;
    if (phase0) {
      g->phase0.upload(phase0, (size_t)F * g->nb * 2, g->stream);
      p0 = g->phase0.p;
    }
    HIP_CHECK(hipStreamSynchronize(g->stream));
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    gl_iterate_and_fetch(g, b, p0, iters ? (int)iters : g->iters, audio, n_samples, false);  // G2..G5 + final ISTFT only
  });
}

// Parity hook: `n_iter` Griffin-Lim iterations (no final ISTFT) from a caller-held state.
xdtts_status xdtts_griffinlim_step(xdtts_griffinlim *g, const float *S, float *angles, float *rebuilt, size_t n_frames,
                                   size_t n_iter) {
  return guard([&] {
    if (!g || !S || !angles || !rebuilt) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
    if (n_iter == 0) n_iter = 1;
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    const int F = (int)n_frames;
    const size_t ne = (size_t)F * g->nb;
    GlBufs b = g->bufs(F);
    g->frames.upload(S, ne, g->stream);
    launch_transpose(g->frames.p, g->S.p, g->nb, F, g->stream);
    g->phase0.alloc(ne * 4);  // staging: angles then rebuilt, (nb x F x 2) each
    HIP_CHECK(hipMemcpyAsync(g->phase0.p, angles, ne * 2 * sizeof(float), hipMemcpyHostToDevice, g->stream));
    HIP_CHECK(hipMemcpyAsync(g->phase0.p + ne * 2, rebuilt, ne * 2 * sizeof(float), hipMemcpyHostToDevice, g->stream));
    launch_gl_state_import(b, g->phase0.p, g->phase0.p + ne * 2, g->stream);
    launch_gl_prepare(b, g->stream);
    const float alpha = g->momentum / (1.0f + g->momentum);
    std::lock_guard<ChipLock> chip(chip_mutex(g->device));
    g->probe_tick();
    for (int attempt = 0;; ++attempt) {
      const float2 *tp = nullptr;
      const float2 *fin = g->run_iterations(b, (int)n_iter, alpha, nullptr, true, &tp);
      if (!g->last_persistent) {  // the launch engine updates the state in place
        launch_gl_state_export(b, fin, b.tprev, g->phase0.p, g->phase0.p + ne * 2, g->stream);
        break;
      }
      HIP_CHECK(hipStreamSynchronize(g->stream));
      if (!g->persistent_failed()) {
        launch_gl_state_export(b, fin, tp, g->phase0.p, g->phase0.p + ne * 2, g->stream);
        break;
      }
      if (attempt) fail(XDTTS_ERR_HIP, "Griffin-Lim step: exchange failure");
    }
    HIP_CHECK(hipMemcpyAsync(angles, g->phase0.p, ne * 2 * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipMemcpyAsync(rebuilt, g->phase0.p + ne * 2, ne * 2 * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
  });
}

xdtts_status xdtts_griffinlim_last_timings(const xdtts_griffinlim *g, float ms[3]) {
  return guard([&] {
    if (!g || !ms) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int i = 0; i < 3; ++i) ms[i] = g->last_ms[i];
  });
}

// ---- analysis: the inverse direction of GriffinLim::infer's conventions (analysis.hip).  No co-resident grid: no chip lock. ----

// What one call takes: the row tiles of the mel GEMM and of the boundary transposes go into a grid dimension of at most 65535
// (32 rows each), so 2^20 frames in all (3.4 hours of audio) leave a factor two; 2^28 samples are 2^20 frames.
static constexpr size_t AN_MAX_FRAMES = (size_t)1 << 20, AN_MAX_SAMPLES = (size_t)1 << 28;

size_t xdtts_griffinlim_analysis_frames(const xdtts_griffinlim *g, size_t n_samples) {
  return n_samples / (size_t)(g ? g->hop : 256) + 1;  // (every handle's hop is 256: xdtts_griffinlim_new)
}

xdtts_status xdtts_griffinlim_analyze_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n_samples, int32_t n_utt,
                                            float mel_floor, float **S_outs, float **mel_outs, size_t *n_frames) {
  return guard([&] {
    if (!g || !audios || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_utt < 1) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    Rows rows;
    bool want_S = false, want_mel = false;
    for (int u = 0; u < n_utt; ++u) {
      if (!audios[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio", u);
      if (n_samples[u] == 0 || n_samples[u] >= AN_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need 1 .. 2^28 - 1 samples, got %zu", u, n_samples[u]);
      rows_add(rows, n_samples[u] / (size_t)g->hop + 1, AN_MAX_FRAMES, "batch too large: more than 2^20 frames");
      want_S = want_S || (S_outs && S_outs[u]);
      want_mel = want_mel || (mel_outs && mel_outs[u]);
    }
    const float floor = mel_floor > 0.f ? mel_floor : 1e-5f;  // Tacotron2's clamp
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    gl_analysis_enqueue(g, audios, n_samples, rows, want_mel);
    // boundary layouts, utterance by utterance: mel (n_mels x F) compressed, S (n_bins x F)
    const size_t mel_at = rows.total * g->nb;
    g->an_out.alloc(rows.total * (size_t)(g->nb + g->n_mels));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)rows.row0[(size_t)u];
      const int F = rows.F[(size_t)u];
      if (mel_outs && mel_outs[u])
        launch_mel_compress(g->an_melT.p + r0 * g->n_mels, g->an_out.p + mel_at + r0 * g->n_mels, g->n_mels, F, g->gopts.mel_decompress, floor, g->stream);
      if (S_outs && S_outs[u]) launch_transpose(g->an_S.p + r0 * g->nb, g->an_out.p + r0 * g->nb, F, g->nb, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->an_ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)rows.row0[(size_t)u], F = (size_t)rows.F[(size_t)u];
      if (mel_outs && mel_outs[u])
        HIP_CHECK(hipMemcpyAsync(mel_outs[u], g->an_out.p + mel_at + r0 * g->n_mels, F * g->n_mels * sizeof(float), hipMemcpyDeviceToHost, g->stream));
      if (S_outs && S_outs[u])
        HIP_CHECK(hipMemcpyAsync(S_outs[u], g->an_out.p + r0 * g->nb, F * g->nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
      if (n_frames) n_frames[u] = F;
    }
    gl_analysis_finish_timings(g);
  });
}

xdtts_status xdtts_griffinlim_analyze(xdtts_griffinlim *g, const float *audio, size_t n_samples, float mel_floor, float *S_out,
                                      float *mel_out, size_t *n_frames) {
  return xdtts_griffinlim_analyze_batch(g, &audio, &n_samples, 1, mel_floor, &S_out, &mel_out, n_frames);
}

xdtts_status xdtts_griffinlim_spectral_convergence(xdtts_griffinlim *g, const float *audio, size_t n_samples, const float *S,
                                                   size_t n_frames, int32_t fit_gain, float out[2]) {
  return guard([&] {
    if (!g || !audio || !S || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_samples == 0 || n_samples >= AN_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "need 1 .. 2^28 - 1 samples, got %zu", n_samples);
    const size_t F = n_samples / (size_t)g->hop + 1;
    if (n_frames != F) fail(XDTTS_ERR_BAD_ARG, "the target has %zu frames, %zu samples analyse to %zu", n_frames, n_samples, F);
    if (fit_gain != 0 && fit_gain != 1) fail(XDTTS_ERR_BAD_ARG, "fit_gain must be 0 or 1, got %d", fit_gain);
    const size_t ne = F * (size_t)g->nb;
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    // the target in the device layout [F][nb] first, so that the timed span holds kernels only
    g->an_out.upload(S, ne, g->stream);
    g->an_St.alloc(ne);
    launch_transpose(g->an_out.p, g->an_St.p, g->nb, (int)F, g->stream);
    g->an_sums.alloc(3 * SPD_PARTS + 3);
    Rows rows;
    rows_add(rows, F, AN_MAX_FRAMES, "batch too large: more than 2^20 frames");  // (never: the sample count was checked above)
    gl_analysis_enqueue(g, &audio, &n_samples, rows, false);
    double *sums = g->an_sums.p + 3 * SPD_PARTS;
    launch_spec_distance(g->an_S.p, g->an_St.p, ne, g->an_sums.p, sums, g->stream);
    HIP_CHECK(hipEventRecord(g->an_ev.e[2], g->stream));
    double h[3] = {0, 0, 0};  // sum x s, sum x x, sum s s  (x = analysed magnitude, s = target)
    HIP_CHECK(hipMemcpyAsync(h, sums, sizeof h, hipMemcpyDeviceToHost, g->stream));
    gl_analysis_finish_timings(g);
    if (!(h[2] > 0.0)) fail(XDTTS_ERR_BAD_ARG, "the target magnitude is all zero");
    const double a = fit_gain ? (h[1] > 0.0 ? h[0] / h[1] : 0.0) : 1.0;
    const double d2 = (a * a * h[1] - 2.0 * a * h[0]) + h[2];  // || a x - s ||^2
    out[0] = (float)std::sqrt(std::max(d2, 0.0) / h[2]);
    out[1] = (float)a;
  });
}

xdtts_status xdtts_griffinlim_analysis_timings(const xdtts_griffinlim *g, float ms[3]) {
  return guard([&] {
    if (!g || !ms) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int i = 0; i < 3; ++i) ms[i] = g->an_ms[i];
  });
}

void xdtts_griffinlim_free(xdtts_griffinlim *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  delete g;
}

}  // extern "C"
