// api_griffinlim.cpp -- the extern "C" boundary, vocoder half: argument checks and locking; the work is in griffinlim_handle.cpp.
#include <algorithm>
#include <cmath>
#include <memory>

#include "env.h"
#include "griffinlim_handle.h"

using namespace xdtts;

// GriffinLim::infer for several utterances at once (the vocoder half of a batch, BASELINE.json configs[3]):
// the utterances' frames are concatenated, mel -> linear is one GEMM over all of them, and the persistent
// kernel takes as many utterances per launch as fit one workgroup per CU.  Every utterance's audio is bit-identical to what
// xdtts_griffinlim_infer returns for it alone.  (pros == cont == null: xdtts_griffinlim_infer_batch; else one prosody or one
// contour per utterance, its fields checked by the caller; job: a pitch-target request -- checked options, one checked target
// per utterance and contours that may be null, which take the place of pros / cont)
static xdtts_status infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames, int32_t n_utt,
                                const xdtts_prosody *pros, const xdtts_prosody_contour *cont, float **audios, size_t *n_samples,
                                const F0Job *job = nullptr, const xdtts_pitch_target *tg = nullptr,
                                const xdtts_prosody_contour *const *tc = nullptr) {
  return guard([&] {
    if (!g || !mels || !n_frames || !audios || !n_samples || n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
    Rows rows;
    std::vector<ContourTable> tabs(cont ? (size_t)n_utt : 0);
    for (int u = 0; u < n_utt; ++u) {
      audios[u] = nullptr;
      n_samples[u] = 0;
      if (!mels[u] || n_frames[u] < 2) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need at least 2 frames", u);
      if (pros) prosody_check_at(&pros[u], u, n_frames[u]);
      if (cont) {
        contour_check_at(&cont[u], u, n_frames[u]);
        contour_table(cont[u], n_frames[u], tabs[(size_t)u]);
      }
      rows_add(rows, n_frames[u], (size_t)1 << 24, "batch too large");
    }
    TargetPlan plan;
    if (job) target_plan(*job, tg, tc, n_utt, n_frames, plan);
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
    gl_batch_from_device(g, g->mel_in.p, rows.F, audios, n_samples, job ? plan.arg() : (cont ? ProsodyArg(tabs.data()) : ProsodyArg(pros)));
    if (job && plan.active) g->f0_collect();
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
    if (!(power > 0) || momentum < 0) fail(XDTTS_ERR_BAD_ARG, "bad power/momentum");
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
      g->norm_parts.alloc(GLN_SCRATCH);
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
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    gl_run_from_device_mel(g, g->mel_in.p, (int)n_frames, nullptr, audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                          int32_t n_utt, float **audios, size_t *n_samples) {
  return infer_batch(g, mels, n_mels, n_frames, n_utt, nullptr, nullptr, audios, n_samples);
}

xdtts_status xdtts_griffinlim_mel_to_linear(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            float *S_out) {
  return guard([&] {
    if (!g || !mel || !S_out || n_frames == 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
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
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
    prosody_check(p, n_frames);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    gl_run_from_device_mel(g, g->mel_in.p, (int)n_frames, ProsodyArg(p), audio, n_samples);
  });
}

// ... for a batch, one prosody per utterance: audios[u] has hop * (F'_u - 1) samples.  The prosody array is checked first, so
// that a bad field is reported without a handle.
xdtts_status xdtts_griffinlim_infer_batch_prosody(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                                  int32_t n_utt, const xdtts_prosody *p, float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    for (int u = 0; u < n_utt; ++u) {
      if (audios) audios[u] = nullptr;
      if (n_samples) n_samples[u] = 0;
    }
    prosody_check_array(p, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return infer_batch(g, mels, n_mels, n_frames, n_utt, p, nullptr, audios, n_samples);
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
    for (const ProsodyUtt &t : tab) launch_transpose(g->S_pros.p + (size_t)t.dst0 * nb, g->frames.p + (size_t)t.dst0 * nb, t.Fout, g->nb, g->stream);
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const ProsodyUtt &t = tab[(size_t)u];
      HIP_CHECK(hipMemcpyAsync(S_outs[u], g->frames.p + (size_t)t.dst0 * nb, (size_t)t.Fout * nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    }
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
    const size_t nb = (size_t)g->nb;
    g->bufs((int)std::max(in.total, out.total));  // (frames: the boundary-layout staging of both directions)
    g->upload_rows(S, in);
    HIP_CHECK(hipEventRecord(g->ev.e[3], g->stream));
    g->contour_upload(tabs.data(), n_utt);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->contour_launch();
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)out.row0[(size_t)u] * nb;
      launch_transpose(g->S_pros.p + r0, g->frames.p + r0, out.F[(size_t)u], g->nb, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)out.row0[(size_t)u] * nb;
      HIP_CHECK(hipMemcpyAsync(S_outs[u], g->frames.p + r0, (size_t)out.F[(size_t)u] * nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    }
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
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
    ContourTable tab;
    contour_table(*c, n_frames, tab);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    g->mel_in.upload(mel, n_mels * n_frames, g->stream);
    HIP_CHECK(hipStreamSynchronize(g->stream));
    gl_run_from_device_mel(g, g->mel_in.p, (int)n_frames, ProsodyArg(&tab), audio, n_samples);
  });
}

xdtts_status xdtts_griffinlim_infer_batch_contour(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames,
                                                  int32_t n_utt, const xdtts_prosody_contour *c, float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    for (int u = 0; u < n_utt; ++u) {
      if (audios) audios[u] = nullptr;
      if (n_samples) n_samples[u] = 0;
    }
    contour_check_array(c, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return infer_batch(g, mels, n_mels, n_frames, n_utt, nullptr, c, audios, n_samples);
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
  return guard([&] {
    if (n) *n = 0;
    if (!g || !n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *n = g->last_f0.size();
    if (!out && cap == 0) return;  // the count alone
    if (!out || cap < g->last_f0.size()) fail(XDTTS_ERR_BAD_ARG, "the last call tracked %zu utterances, the buffer holds %zu", g->last_f0.size(), cap);
    if (!g->last_f0.empty()) std::memcpy(out, g->last_f0.data(), g->last_f0.size() * sizeof(xdtts_f0_stats));
  });
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
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
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
    const size_t nb = (size_t)g->nb;
    g->bufs((int)std::max(in.total, out.total));
    g->upload_rows(S, in);
    g->contour_upload(plan.tabs.data(), n_utt, true);
    g->f0_prepare_contour(plan.job);
    HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
    g->f0_launch(g->S.p, plan.job, g->contour_ftab.p, g->contour_n_tab, g->ev.e[1]);
    g->contour_launch();
    for (int u = 0; u < n_utt; ++u) {
      if (!S_outs || !S_outs[u]) continue;
      const size_t r0 = (size_t)out.row0[(size_t)u] * nb;
      launch_transpose(g->S_pros.p + r0, g->frames.p + r0, out.F[(size_t)u], g->nb, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      if (!S_outs || !S_outs[u]) continue;
      const size_t r0 = (size_t)out.row0[(size_t)u] * nb;
      HIP_CHECK(hipMemcpyAsync(S_outs[u], g->frames.p + r0, (size_t)out.F[(size_t)u] * nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    }
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
    if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
    if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
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
    for (int u = 0; u < n_utt; ++u) {
      if (audios) audios[u] = nullptr;
      if (n_samples) n_samples[u] = 0;
    }
    job = f0_job_checked(o);
    pitch_target_check_array(t, n_utt);
    for (int u = 0; c && u < n_utt; ++u)
      if (c[u]) contour_check_at(c[u], u, 2);
  });
  if (st != XDTTS_OK) return st;
  return infer_batch(g, mels, n_mels, n_frames, n_utt, nullptr, nullptr, audios, n_samples, &job, t, c);
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
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)rows.row0[(size_t)u] * nb;
      launch_transpose(g->S_timbre.p + r0, g->frames.p + r0, rows.F[(size_t)u], g->nb, g->stream);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
    for (int u = 0; u < n_utt; ++u) {
      const size_t r0 = (size_t)rows.row0[(size_t)u] * nb;
      HIP_CHECK(hipMemcpyAsync(S_outs[u], g->frames.p + r0, (size_t)rows.F[(size_t)u] * nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
    }
    g->finish_timings();  // (drains the stream: the table and the outputs)
  });
}

xdtts_status xdtts_griffinlim_timbre_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_timbre *t, float *S_out) {
  return xdtts_griffinlim_timbre_linear_batch(g, &S, &n_frames, 1, t, &S_out);
}

// ---- output rate: 22 050 Hz -> 8 .. 96 kHz behind the loop, in front of the output normalisation (resample_plan.h, resample.hip) ----

// The rate rule of the entries: the plan of a supported rate, else XDTTS_ERR_BAD_ARG with the rate and the rule.
static ResamplePlan resample_plan_checked(int32_t rate) {
  ResamplePlan p;
  const std::string msg = resample_check(rate, &p);
  if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s (supported: %d .. %d Hz with rate / gcd(rate, %d) <= %d)", msg.c_str(), RESAMPLE_RATE_MIN,
                         RESAMPLE_RATE_MAX, RESAMPLE_RATE_IN, RESAMPLE_L_MAX);
  return p;
}

xdtts_status xdtts_resample_plan(int32_t rate_out, size_t n_in, int32_t *L, int32_t *M, int32_t *half_len, size_t *n_out) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate_out);
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (half_len) *half_len = p.H;
    if (n_out) *n_out = resample_n_out(p, n_in);
  });
}

xdtts_status xdtts_resample_filter(int32_t rate_out, float *taps, size_t cap, size_t *n_taps) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate_out);
    const size_t n = (size_t)2 * (size_t)p.H + 1;
    if (n_taps) *n_taps = n;
    if (!taps && cap == 0) return;  // the size alone
    if (!taps || cap < n) fail(XDTTS_ERR_BAD_ARG, "rate %d has %zu taps, the buffer holds %zu", rate_out, n, cap);
    std::vector<float> h;
    resample_taps(p, h);
    std::memcpy(taps, h.data(), n * sizeof(float));
  });
}

xdtts_status xdtts_griffinlim_set_output_rate(xdtts_griffinlim *g, int32_t rate) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate);  // the rate first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->out_rate = rate;
    g->out_plan = p;
  });
}

xdtts_status xdtts_griffinlim_get_output_rate(const xdtts_griffinlim *g, int32_t *rate) {
  return guard([&] {
    if (!g || !rate) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *rate = g->out_rate;
  });
}

// What the stage takes in one call: the analysis entries' sample cap per utterance, and 2^31 - 1 output samples in all.
static constexpr size_t RS_MAX_SAMPLES = (size_t)1 << 28;

// Parity hook of the stage alone, single call and ragged batch: the audios one behind the other on the device, ONE k_resample
// launch (the single call passes its record by value, the batch uploads the table), and back.  last_timings: ms[0] = the
// launch alone.  The identity copies and launches nothing.
xdtts_status xdtts_griffinlim_resample_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate_out,
                                             float *const *outs, size_t *n_out) {
  return guard([&] {
    for (int u = 0; n_out && u < n_utt; ++u) n_out[u] = 0;
    const ResamplePlan p = resample_plan_checked(rate_out);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!g || !audios || !n || !outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<ResampleUtt> tab((size_t)n_utt);
    size_t in_tot = 0, out_tot = 0;
    int blk = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (n[u] >= RS_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: at most 2^28 - 1 samples, got %zu", u, n[u]);
      if (n[u] && (!audios[u] || !outs[u])) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio", u);
      const size_t no = resample_n_out(p, n[u]);
      tab[(size_t)u] = {(long long)in_tot, (long long)out_tot, (int)n[u], (int)no, blk, 0};
      in_tot += n[u];
      out_tot += no;
      if (out_tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples at rate %d", rate_out);
      blk += (int)((no + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK);
    }
    if (p.identity) {  // nothing to launch, no device
      for (int u = 0; u < n_utt; ++u) {
        if (n[u]) std::memcpy(outs[u], audios[u], n[u] * sizeof(float));
        if (n_out) n_out[u] = n[u];
      }
      return;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    g->rs_in.alloc(std::max<size_t>(in_tot, 1));
    g->audio_rs.alloc(std::max<size_t>(out_tot, 1));
    g->resample_prepare(rate_out);
    for (int u = 0; u < n_utt; ++u)
      if (n[u]) HIP_CHECK(hipMemcpyAsync(g->rs_in.p + tab[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_utt > 1) {
      g->rs_tab_host = tab;
      g->rs_tab.upload(g->rs_tab_host.data(), g->rs_tab_host.size(), st);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[0], st));
    if (n_utt == 1) {
      if (n[0]) g->resample_one(g->rs_in.p, n[0], g->audio_rs.p, rate_out);  // (the form the single-utterance entries run)
    } else {
      g->resample_rows(g->rs_in.p, g->audio_rs.p, 0, n_utt);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    for (int u = 0; u < n_utt; ++u)
      if (tab[(size_t)u].n_out)
        HIP_CHECK(hipMemcpyAsync(outs[u], g->audio_rs.p + tab[(size_t)u].dst0, (size_t)tab[(size_t)u].n_out * sizeof(float), hipMemcpyDeviceToHost, st));
    g->finish_timings();  // (drains the stream: the inputs, the table and the outputs)
    for (int u = 0; n_out && u < n_utt; ++u) n_out[u] = (size_t)tab[(size_t)u].n_out;
  });
}

xdtts_status xdtts_griffinlim_resample(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate_out, float *out, size_t *n_out) {
  return xdtts_griffinlim_resample_batch(g, &audio, &n, 1, rate_out, &out, n_out);
}

// ---- loudness: BS.1770 integrated loudness under a true-peak ceiling, behind the resampler (loudness_plan.h, loudness.hip) ----

static void loudness_rate_checked(int32_t rate) {
  const std::string msg = loudness_check(rate);
  if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
}

double xdtts_loudness_lufs(const xdtts_loudness *l) { return l ? loudness_lufs(l->mean_square) : -INFINITY; }

xdtts_status xdtts_loudness_plan(int32_t rate, size_t n, int32_t *hop, size_t *n_blocks) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (hop) *hop = loudness_hop(rate);
    if (n_blocks) *n_blocks = loudness_blocks(rate, n);
  });
}

xdtts_status xdtts_loudness_filter(int32_t rate, double coef[10]) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (!coef) fail(XDTTS_ERR_BAD_ARG, "null argument");
    loudness_coef(rate, coef);
  });
}

xdtts_status xdtts_true_peak_filter(float taps[3][24]) {
  return guard([&] {
    if (!taps) fail(XDTTS_ERR_BAD_ARG, "null argument");
    static_assert(LOUD_TP_PHASES == 3 && LOUD_TP_TAPS == 24, "the header's array type");
    loudness_true_peak_taps(taps);
  });
}

xdtts_status xdtts_griffinlim_set_loudness(xdtts_griffinlim *g, float target_lufs, float ceiling_dbtp) {
  return guard([&] {
    const std::string msg = loudness_target_check(target_lufs, ceiling_dbtp);  // the values first: reported without a handle
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->loud_target = target_lufs;
    g->loud_ceiling = ceiling_dbtp;
  });
}

xdtts_status xdtts_griffinlim_get_loudness(const xdtts_griffinlim *g, float *target_lufs, float *ceiling_dbtp) {
  return guard([&] {
    if (!g || !target_lufs || !ceiling_dbtp) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *target_lufs = g->loud_target;
    *ceiling_dbtp = g->loud_ceiling;
  });
}

xdtts_status xdtts_griffinlim_last_loudness(const xdtts_griffinlim *g, xdtts_loudness *out, size_t cap, size_t *n) {
  return guard([&] {
    if (n) *n = 0;
    if (!g || !n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *n = g->last_loud.size();
    if (!out && cap == 0) return;  // the count alone
    if (!out || cap < g->last_loud.size()) fail(XDTTS_ERR_BAD_ARG, "the last call delivered %zu utterances, the buffer holds %zu", g->last_loud.size(), cap);
    if (!g->last_loud.empty()) std::memcpy(out, g->last_loud.data(), g->last_loud.size() * sizeof(xdtts_loudness));
  });
}

// Measurement hook of the stage alone, single call and ragged batch: the audios one behind the other on the device, the four
// launches of launch_loudness_measure (the single call passes its record by value, the batch uploads the table), and the
// structs back.  No target, no scaling: gain = 1.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_loudness_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                             xdtts_loudness *out) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!g || !audios || !n || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<LoudUtt> tab((size_t)n_utt);
    size_t tot = 0, grp = 0, seg = 0, sb = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (n[u] == 0 || n[u] >= RS_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need 1 .. 2^28 - 1 samples, got %zu", u, n[u]);
      if (!audios[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio", u);
      tab[(size_t)u] = {(long long)tot, (int)n[u], (int)grp, (int)seg, (int)sb};
      tot += n[u];
      grp += loudness_groups(n[u]);
      seg += loudness_segments(n[u]);
      sb += loudness_sub_blocks(rate, n[u]);
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    g->rs_in.alloc(tot);
    g->loudness_prepare(rate);
    g->loudness_bufs(grp, (size_t)n_utt);
    for (int u = 0; u < n_utt; ++u)
      HIP_CHECK(hipMemcpyAsync(g->rs_in.p + tab[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_utt > 1) {
      g->loud_tab_host = tab;
      g->loud_tab.upload(g->loud_tab_host.data(), g->loud_tab_host.size(), st);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[0], st));
    if (n_utt == 1) g->loudness_one(g->rs_in.p, n[0], rate, false);  // (the form the single-utterance entries run)
    else g->loudness_rows(g->rs_in.p, 0, n_utt, rate, false);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    g->loudness_fetch(0, n_utt, st);
    g->finish_timings();  // (drains the stream: the inputs, the table and the structs)
    static_assert(sizeof(xdtts_loudness) == sizeof(LoudResult), "LoudResult is xdtts_loudness");
    std::memcpy(out, g->loud_host, (size_t)n_utt * sizeof(xdtts_loudness));
  });
}

xdtts_status xdtts_griffinlim_loudness(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, xdtts_loudness *out) {
  return xdtts_griffinlim_loudness_batch(g, &audio, &n, 1, rate, out);
}

// ---- limiter: look-ahead true-peak limiter where the loudness stage scaled (limiter_plan.h, limiter.hip) ------------------------

static_assert(sizeof(xdtts_limiter_stats) == sizeof(LimiterStats) && offsetof(xdtts_limiter_stats, limited) == offsetof(LimiterStats, limited),
              "xdtts_limiter_stats and LimiterStats share one layout");

xdtts_status xdtts_limiter_plan(int32_t rate, int32_t lookahead_us, int32_t *half_width, int32_t *tile) {
  return guard([&] {
    const std::string msg = limiter_check(rate, lookahead_us);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (half_width) *half_width = limiter_half_width(rate, lookahead_us);
    if (tile) *tile = LIM_TILE;
  });
}

xdtts_status xdtts_limiter_window(int32_t rate, int32_t lookahead_us, float *w) {
  return guard([&] {
    const std::string msg = limiter_check(rate, lookahead_us);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!w) fail(XDTTS_ERR_BAD_ARG, "null argument");
    limiter_window(limiter_half_width(rate, lookahead_us), w);
  });
}

xdtts_status xdtts_limiter_reference(const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin, int32_t lookahead_us,
                                     float *out, xdtts_limiter_stats *stats) {
  return guard([&] {
    const std::string msg = limiter_args_check(rate, lookahead_us, n, gain0, ceiling_lin);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!audio || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const LimiterStats st = limiter_reference(audio, n, rate, lookahead_us, gain0, ceiling_lin, out);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_limiter(xdtts_griffinlim *g, int32_t lookahead_us) {
  return guard([&] {
    const std::string msg = limiter_setting_check(lookahead_us);  // the value first: reported without a handle
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->lim_us = lookahead_us;
  });
}

xdtts_status xdtts_griffinlim_get_limiter(const xdtts_griffinlim *g, int32_t *lookahead_us) {
  return guard([&] {
    if (!g || !lookahead_us) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *lookahead_us = g->lim_us;
  });
}

xdtts_status xdtts_griffinlim_last_limiter(const xdtts_griffinlim *g, xdtts_limiter_stats *out, size_t cap, size_t *n) {
  return guard([&] {
    if (n) *n = 0;
    if (!g || !n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *n = g->last_lim.size();
    if (!out && cap == 0) return;  // the count alone
    if (!out || cap < g->last_lim.size()) fail(XDTTS_ERR_BAD_ARG, "the last call delivered %zu utterances, the buffer holds %zu", g->last_lim.size(), cap);
    if (!g->last_lim.empty()) std::memcpy(out, g->last_lim.data(), g->last_lim.size() * sizeof(xdtts_limiter_stats));
  });
}

// The stage alone, single call and ragged batch: the audios one behind the other on the device, the two launches of
// launch_limit (the single call passes its record by value, the batch uploads the table), the outputs and the stats back.
// Always engaged, g0 = gain0.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_limit_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                          double gain0, double ceiling_lin, int32_t lookahead_us, float *const *outs,
                                          xdtts_limiter_stats *stats) {
  return guard([&] {
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<LimUtt> tab((size_t)n_utt);
    size_t tot = 0, tile = 0;
    for (int u = 0; u < n_utt; ++u) {
      const std::string msg = limiter_args_check(rate, lookahead_us, n[u], gain0, ceiling_lin);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      tab[(size_t)u] = {(long long)tot, (long long)tot, (int)n[u], (int)tile};
      tot += n[u];
      tile += limiter_tiles(n[u]);
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    if (!g || !audios || !outs || !stats) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!audios[u] || !outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio / out", u);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    g->rs_in.alloc(tot);
    g->limiter_prepare(rate, lookahead_us);
    g->limiter_bufs(tot, (size_t)n_utt);
    for (int u = 0; u < n_utt; ++u)
      HIP_CHECK(hipMemcpyAsync(g->rs_in.p + tab[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_utt > 1) {
      g->lim_tab_host = tab;
      g->lim_tab.upload(g->lim_tab_host.data(), g->lim_tab_host.size(), st);
    }
    const LimJob job = g->limiter_job(false, 0, gain0, ceiling_lin);
    HIP_CHECK(hipEventRecord(g->ev.e[0], st));
    if (n_utt == 1) g->limit_one(g->rs_in.p, n[0], job);  // (the form the single-utterance entries run)
    else g->limit_rows(g->rs_in.p, 0, n_utt, job);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    for (int u = 0; u < n_utt; ++u)
      HIP_CHECK(hipMemcpyAsync(outs[u], g->lim_out.p + tab[(size_t)u].dst0, n[u] * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(g->lim_host, g->lim_stats.p, (size_t)n_utt * sizeof(LimiterStats), hipMemcpyDeviceToHost, st));
    g->finish_timings();  // (drains the stream: the inputs, the table, the outputs and the stats)
    std::memcpy(stats, g->lim_host, (size_t)n_utt * sizeof(xdtts_limiter_stats));
  });
}

xdtts_status xdtts_griffinlim_limit(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin,
                                    int32_t lookahead_us, float *out, xdtts_limiter_stats *stats) {
  return xdtts_griffinlim_limit_batch(g, &audio, &n, 1, rate, gain0, ceiling_lin, lookahead_us, &out, stats);
}

// ---- compressor: tent-envelope dynamic range compressor in front of the level stage (compressor_plan.h, compressor.hip) --------

static_assert(sizeof(xdtts_compressor) == sizeof(Compressor) && offsetof(xdtts_compressor, makeup_db) == offsetof(Compressor, makeup_db),
              "xdtts_compressor and Compressor share one layout");
static_assert(sizeof(xdtts_compressor_stats) == sizeof(CompressorStats) &&
                  offsetof(xdtts_compressor_stats, compressed) == offsetof(CompressorStats, compressed),
              "xdtts_compressor_stats and CompressorStats share one layout");

// the checked setting (null is an error here: the entries that take "off" look at the pointer first)
static Compressor compressor_checked(const xdtts_compressor *c) {
  if (!c) fail(XDTTS_ERR_BAD_ARG, "compressor: null settings");
  Compressor s;
  std::memcpy(&s, c, sizeof s);
  const std::string msg = compressor_check(s);
  if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
  return s;
}

void xdtts_compressor_default(xdtts_compressor *c) {
  if (!c) return;
  const Compressor d = compressor_default();
  std::memcpy(c, &d, sizeof d);
}

xdtts_status xdtts_compressor_preset(int32_t which, xdtts_compressor *out) {
  return guard([&] {
    if (!out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    Compressor p;
    if (!compressor_preset(which, &p)) fail(XDTTS_ERR_BAD_ARG, "compressor: preset %d is not 0 (default) or 1 (drc)", which);
    std::memcpy(out, &p, sizeof p);
  });
}

xdtts_status xdtts_compressor_plan(int32_t rate, const xdtts_compressor *c, int32_t *alpha, int32_t *rho, int32_t *T, int32_t *W,
                                   int32_t *tile) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    const std::string msg = compressor_rate_check(rate);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    const CompPlan p = compressor_plan(s, rate);
    if (alpha) *alpha = p.alpha;
    if (rho) *rho = p.rho;
    if (T) *T = p.T;
    if (W) *W = p.W;
    if (tile) *tile = COMP_TILE;
  });
}

xdtts_status xdtts_compressor_level(const float *audio, size_t n, int32_t *l) {
  return guard([&] {
    if (n >= COMP_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "compressor: need at most 2^28 - 1 samples, got %zu", n);
    if (n && (!audio || !l)) fail(XDTTS_ERR_BAD_ARG, "null argument");
    compressor_level(audio, n, l);
  });
}

xdtts_status xdtts_compressor_envelope(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, int32_t *V) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    const std::string msg = compressor_args_check(s, rate, n);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!audio || !V) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const CompPlan p = compressor_plan(s, rate);
    std::vector<int32_t> l(n);
    compressor_level(audio, n, l.data());
    compressor_envelope_from_level(l.data(), n, p.alpha, p.rho, V);
  });
}

xdtts_status xdtts_compressor_reference(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, float *out,
                                        xdtts_compressor_stats *stats) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    const std::string msg = compressor_args_check(s, rate, n);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!audio || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const CompressorStats st = compressor_reference(audio, n, rate, s, out);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_compressor(xdtts_griffinlim *g, const xdtts_compressor *c) {
  return guard([&] {
    Compressor s = compressor_default();
    if (c) s = compressor_checked(c);  // the fields first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->comp = s;
    g->comp_set = c != nullptr;
  });
}

xdtts_status xdtts_griffinlim_get_compressor(const xdtts_griffinlim *g, xdtts_compressor *c, int32_t *on) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    if (c) std::memcpy(c, &g->comp, sizeof g->comp);
    if (on) *on = g->comp_set ? 1 : 0;
  });
}

xdtts_status xdtts_griffinlim_last_compressor(const xdtts_griffinlim *g, xdtts_compressor_stats *out, size_t cap, size_t *n) {
  return guard([&] {
    if (n) *n = 0;
    if (!g || !n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *n = g->last_comp.size();
    if (!out && cap == 0) return;  // the count alone
    if (!out || cap < g->last_comp.size()) fail(XDTTS_ERR_BAD_ARG, "the last call delivered %zu utterances, the buffer holds %zu", g->last_comp.size(), cap);
    if (!g->last_comp.empty()) std::memcpy(out, g->last_comp.data(), g->last_comp.size() * sizeof(xdtts_compressor_stats));
  });
}

// The stage alone, single call and ragged batch: the audios one behind the other on the device, the three launches of
// launch_compress in place (the single call passes its record by value, the batch uploads the table), the outputs and the
// stats back.  The identity touches no device: the inputs' bits, stats of zeros.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_compress_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                             const xdtts_compressor *c, float *const *outs, xdtts_compressor_stats *stats) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::vector<CompUtt> tab((size_t)n_utt);
    size_t tot = 0, tile = 0;
    for (int u = 0; u < n_utt; ++u) {
      const std::string msg = compressor_args_check(s, rate, n[u]);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      tab[(size_t)u] = {(long long)tot, (long long)tot, (int)n[u], (int)tile};  // (back to back, as the batch's rows lie)
      tot += n[u];
      tile += compressor_tiles(n[u]);
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    if (!g || !audios || !outs || !stats) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!audios[u] || !outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio / out", u);
    if (compressor_is_identity(s)) {
      for (int u = 0; u < n_utt; ++u) {
        if (outs[u] != audios[u]) std::memmove(outs[u], audios[u], n[u] * sizeof(float));
        stats[u] = xdtts_compressor_stats{0.0f, 0, 0, 0};
      }
      return;
    }
    const CompPlan plan = compressor_plan(s, rate);
    std::lock_guard<std::mutex> lk(g->mu);
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    g->rs_in.alloc(tot);
    g->compressor_bufs(tile, (size_t)n_utt);
    for (int u = 0; u < n_utt; ++u)
      HIP_CHECK(hipMemcpyAsync(g->rs_in.p + tab[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_utt > 1) {
      g->comp_tab_host = tab;
      g->comp_tab.upload(g->comp_tab_host.data(), g->comp_tab_host.size(), st);
    }
    HIP_CHECK(hipEventRecord(g->ev.e[0], st));
    if (n_utt == 1) g->compress_one(g->rs_in.p, g->rs_in.p, n[0], plan);  // (the form the single-utterance entries run)
    else g->compress_rows(g->rs_in.p, g->rs_in.p, 0, n_utt, plan);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    for (int u = 0; u < n_utt; ++u)
      HIP_CHECK(hipMemcpyAsync(outs[u], g->rs_in.p + tab[(size_t)u].dst0, n[u] * sizeof(float), hipMemcpyDeviceToHost, st));
    g->compressor_fetch(0, n_utt, st);
    g->finish_timings();  // (drains the stream: the inputs, the table, the outputs and the stats)
    std::memcpy(stats, g->comp_host, (size_t)n_utt * sizeof(xdtts_compressor_stats));
  });
}

xdtts_status xdtts_griffinlim_compress(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, const xdtts_compressor *c,
                                       float *out, xdtts_compressor_stats *stats) {
  return xdtts_griffinlim_compress_batch(g, &audio, &n, 1, rate, c, &out, stats);
}

// ---- stream: the sequence joined with its gaps, faded, levelled, encoded (stream_plan.h, stream.hip) ----------------------------

static_assert(sizeof(xdtts_stream_opts) == sizeof(StreamOpts) && offsetof(xdtts_stream_opts, fade) == offsetof(StreamOpts, fade),
              "xdtts_stream_opts and StreamOpts share one layout");

void xdtts_stream_opts_default(xdtts_stream_opts *o) {
  if (!o) return;
  const StreamOpts d = stream_opts_default();
  std::memcpy(o, &d, sizeof d);
}

size_t xdtts_stream_sample_bytes(int32_t format) { return (size_t)stream_sample_bytes(format); }

xdtts_status xdtts_stream_plan(const size_t *n, int32_t n_utt, const size_t *gaps, size_t *offsets, size_t *total) {
  return guard([&] {
    const std::string msg = stream_plan(n, n_utt, gaps, offsets, total);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
  });
}

xdtts_status xdtts_stream_fade_table(int32_t fade, float *w) {
  return guard([&] {
    if (fade < 0 || fade > STREAM_FADE_MAX) fail(XDTTS_ERR_BAD_ARG, "stream: fade %d is not in [0, %d]", fade, STREAM_FADE_MAX);
    if (fade > 0 && !w) fail(XDTTS_ERR_BAD_ARG, "null argument");
    stream_fade_table(fade, w);
  });
}

xdtts_status xdtts_stream_encode_sample(float x, int32_t format, int32_t dither, uint32_t seed, size_t k, void *out) {
  return guard([&] {
    const std::string msg = stream_opts_check(StreamOpts{format, dither, seed, 0, 0});
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (k >= STREAM_TOTAL_MAX) fail(XDTTS_ERR_BAD_ARG, "stream: position %zu is not below 2^28", k);
    if (!out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const uint32_t b = stream_encode(x, format, dither, seed, (uint32_t)k);
    std::memcpy(out, &b, (size_t)stream_sample_bytes(format));  // (little endian: the low bytes)
  });
}

xdtts_status xdtts_griffinlim_join(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, const size_t *gaps,
                                   int32_t rate, const xdtts_stream_opts *o, void *out, size_t cap_bytes, size_t *offsets, size_t *total) {
  return guard([&] {
    if (total) *total = 0;
    const StreamOpts so = stream_opts_checked(o);
    if (so.level == 1) loudness_rate_checked(rate);
    std::vector<size_t> off((size_t)std::max(0, std::min(n_utt, STREAM_UTT_MAX)));
    size_t tot = 0;
    const std::string msg = stream_plan(n, n_utt, gaps, off.data(), &tot);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
    if (!audios || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (n[u] && !audios[u]) fail(XDTTS_ERR_BAD_ARG, "audios[%d] is null with n[%d] = %zu", u, u, n[u]);
    const size_t bytes = tot * (size_t)stream_sample_bytes(so.format);
    if (cap_bytes < bytes) fail(XDTTS_ERR_BAD_ARG, "cap_bytes %zu: the stream has %zu samples = %zu bytes", cap_bytes, tot, bytes);
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    if (so.level == 1 && !g->loudness_on()) fail(XDTTS_ERR_BAD_ARG, "stream: level 1 (programme) needs a loudness target on the handle");
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    HIP_CHECK(hipStreamSynchronize(st));
    g->clear_last();
    // utterance u at a multiple of four floats plus the 16-byte phase of (its host address + its offset): an interior pack of
    // the kernel then reads at the phase of the caller's buffer
    g->st_tab_host.clear();
    size_t at = 0;
    for (int u = 0; u < n_utt; ++u) {
      const size_t phase = ((reinterpret_cast<uintptr_t>(audios[u]) / sizeof(float)) + off[(size_t)u]) & 3u;
      const size_t src0 = ((at + 3) & ~(size_t)3) + phase;
      g->st_tab_host.push_back(StreamUtt{(long long)src0, (uint32_t)off[(size_t)u], (int32_t)n[u]});
      at = src0 + n[u];
    }
    g->st_used = 0;
    g->stream_reserve(std::max<size_t>(at, 1));
    for (int u = 0; u < n_utt; ++u)
      if (n[u]) HIP_CHECK(hipMemcpyAsync(g->st_src.p + g->st_tab_host[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    g->stream_join(tot, so, rate, g->ev.e[0]);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    HIP_CHECK(hipMemcpyAsync(out, g->st_out.p, bytes, hipMemcpyDeviceToHost, st));
    g->finish_timings();  // (drains the stream: the inputs, the tables, the stream and the struct)
    if (so.level == 1) g->push_last(0);
    for (int u = 0; offsets && u < n_utt; ++u) offsets[u] = off[(size_t)u];
    if (total) *total = tot;
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
