// griffinlim_handle.cpp -- the vocoder handle (GriffinLim::infer, mod.rs:441-520): mel -> linear, the iteration engines and
// their fallback, the stream stage, the request paths.  The magnitude chain in front of the loop: magnitude.cpp; the delivery
// chain behind it: delivery.cpp.
#include "griffinlim_handle.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

using namespace xdtts;

xdtts_griffinlim::~xdtts_griffinlim() {
  for (hipEvent_t e : copy_ev) (void)hipEventDestroy(e);
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
  if (host_err) (void)hipHostFree(host_err);
  if (stream) (void)hipStreamDestroy(stream);
}

GlBufs xdtts_griffinlim::bufs(int F) {
  S.alloc((size_t)F * nb);
  ang.alloc((size_t)F * nb);
  ang2.alloc((size_t)F * nb);
  tprev.alloc((size_t)F * nb);
  frames.alloc((size_t)F * n_fft);
  wss_inv.alloc((size_t)std::max(1, hop * (F - 1)));
  audio.alloc((size_t)std::max(1, hop * (F - 1)));
  GlBufs g{};
  g.F = F;
  g.n_fft = n_fft;
  g.hop = hop;
  g.nb = nb;
  g.S = S.p;
  g.ang = ang.p;
  g.ang2 = ang2.p;
  g.tprev = tprev.p;
  g.frames = frames.p;
  g.wss_inv = wss_inv.p;
  g.tw = tw.p;
  g.win = win.p;
  return g;
}

// step 1 of GriffinLim::infer: mel (device, n_mels x F) -> S [F][nb], with the convention switches of
// xdtts_griffinlim_opts: de-compression, optional projected-gradient NNLS refinement, exponent.
//   x0 = max(pinv m, 0);  x <- max(x - (1/L) A^T (A x - m), 0)  nnls_iters times, batched over the
//   frames as two MFMA GEMMs per step (residual [F][80], then the update of X [F][NBP]).
void xdtts_griffinlim::mel_to_linear(const float *mel_dev_ptr, int F) {
  melT.alloc((size_t)F * n_mels);
  launch_gl_exp_transpose(mel_dev_ptr, melT.p, n_mels, F, gopts.mel_decompress, stream);
  const float ex = gopts.power_mode == 0 ? 1.0f / power : (gopts.power_mode == 1 ? power : 1.0f);
  GemmArgs a{};
  a.A = melT.p;
  a.lda = n_mels;
  a.W = pinv.p;
  a.M = F;
  a.N = nb;
  a.K = n_mels;
  a.batch = 1;
  if (gopts.nnls_iters <= 0) {
    a.C = S.p;
    a.ldc = nb;
    a.act = ex == 1.0f ? 1 : 3;
    a.p = ex;
    launch_gemm_nt(a, stream);
    return;
  }
  nnls_x.alloc((size_t)F * NBP);
  nnls_r.alloc((size_t)F * n_mels);
  HIP_CHECK(hipMemsetAsync(nnls_x.p, 0, (size_t)F * NBP * sizeof(float), stream));  // padding columns stay 0
  a.C = nnls_x.p;
  a.ldc = NBP;
  a.act = 1;
  launch_gemm_nt(a, stream);
  for (int it = 0; it < gopts.nnls_iters; ++it) {
    GemmArgs r{};  // R = X A^T - m
    r.A = nnls_x.p;
    r.lda = NBP;
    r.W = basis_p.p;  // [n_mels][NBP]
    r.C = nnls_r.p;
    r.ldc = n_mels;
    r.M = F;
    r.N = n_mels;
    r.K = NBP;
    r.batch = 1;
    r.R = melT.p;
    r.ldr = n_mels;
    r.beta = -1.0f;
    launch_gemm_nt(r, stream);
    GemmArgs u{};  // X = max(X - (1/L) R A, 0)
    u.A = nnls_r.p;
    u.lda = n_mels;
    u.W = basisT_p.p;  // [NBP][n_mels]
    u.C = nnls_x.p;
    u.ldc = NBP;
    u.M = F;
    u.N = NBP;
    u.K = n_mels;
    u.batch = 1;
    u.alpha = -nnls_step;
    u.R = nnls_x.p;
    u.ldr = NBP;
    u.r_before_act = 1;
    u.act = 1;
    launch_gemm_nt(u, stream);
  }
  launch_gl_pow_rows(nnls_x.p, NBP, S.p, nb, F, ex, stream);
}

// The stream stage (stream.hip).
void xdtts_griffinlim::stream_reserve(size_t floats) {
  if (floats <= st_src.n) return;
  DevBuf<float> grown;
  grown.alloc(std::max(floats, 2 * st_src.n));
  if (st_used) HIP_CHECK(hipMemcpyAsync(grown.p, st_src.p, st_used * sizeof(float), hipMemcpyDeviceToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  std::swap(grown.p, st_src.p);
  std::swap(grown.n, st_src.n);
}

void xdtts_griffinlim::stream_join(size_t total, const StreamOpts &o, int rate, hipEvent_t begin) {
  const int n_utt = (int)st_tab_host.size();
  st_tab.upload(st_tab_host.data(), st_tab_host.size(), stream);
  if (o.fade > 0) {
    st_fade_host.resize((size_t)o.fade);
    stream_fade_table(o.fade, st_fade_host.data());
    st_fade.upload(st_fade_host.data(), st_fade_host.size(), stream);
  }
  st_out.alloc(total * (size_t)stream_sample_bytes(o.format));
  const bool lim = o.level == 1 && dl.limiter_on();
  if (o.level == 1) {  // the programme: ONE row of the delivery chain's level stage, the stream itself
    DeliveryStages s;
    s.rate = rate;
    s.loud = true;
    s.lim_us = lim ? dl.lim_us : 0;
    dl.prepare(delivery_plan(s, {total}, {0}, {0}), false);
    st_f32.alloc(total);
  }
  if (lim) {  // the encode then reads the limited stream: the same offsets, the utterances where they lie in it
    st_lim_tab_host = st_tab_host;
    for (StreamUtt &r : st_lim_tab_host) r.src0 = (long long)r.off;
    st_lim_tab.upload(st_lim_tab_host.data(), st_lim_tab_host.size(), stream);
  }
  if (begin) HIP_CHECK(hipEventRecord(begin, stream));
  StreamJob job{};
  job.src = st_src.p;
  job.tab = st_tab.p;
  job.fade_tab = o.fade > 0 ? st_fade.p : nullptr;
  job.n_utt = n_utt;
  job.total = (uint32_t)total;
  job.format = o.format;
  job.dither = o.dither;
  job.seed = o.dither_seed;
  job.fade = o.fade;
  if (o.level == 1) {
    StreamJob form = job;  // the stream as level 0 / format 0 delivers it: what the programme measurement is defined on
    form.format = STREAM_F32;
    form.dither = 0;
    launch_stream_join(form, st_f32.p, stream);
    dl.measure(st_f32.p, 0, 1, true);
    job.gain = &dl.loud_res.p->gain;
    if (lim) {  // fade and gain are in the limited stream already; gaps stay the encoder's constants
      dl.limit(st_f32.p, 0, 1, dl.limiter_job(true, 0, 0.0, loudness_ceiling_lin(dl.loud_ceiling)));
      job.src = dl.lim_out.p;
      job.tab = st_lim_tab.p;
      job.fade_tab = nullptr;
      job.fade = 0;
      job.gain = nullptr;
    }
  }
  launch_stream_join(job, st_out.p, stream);
  if (o.level == 1) dl.fetch_stats(0, 1, stream);
}

void xdtts_griffinlim::upload_rows(const float *const *S_host, const Rows &rows) {
  for (int u = 0; u < rows.n(); ++u) {
    const size_t r0 = (size_t)rows.row0[(size_t)u] * nb;
    HIP_CHECK(hipMemcpyAsync(frames.p + r0, S_host[u], (size_t)rows.F[(size_t)u] * nb * sizeof(float), hipMemcpyHostToDevice, stream));
    launch_transpose(frames.p + r0, S.p + r0, nb, rows.F[(size_t)u], stream);
  }
}

bool xdtts_griffinlim::persistent_usable() {
  if (env::equals(env::GL, "launch")) return false;  // developer comparison aid: launch-per-iteration engine
  gate.ensure_probed([&] { return gl_persistent_supported(device, &n_cu, &per_cu4); });
  return gate.usable();
}

void xdtts_griffinlim::persist_prepare(size_t xch_words, unsigned tags) {
  if (xch_words > xch.n || epoch > 0x7fff0000u - tags) {  // fresh (or wrapped) tags: clear every granule
    xch.alloc(xch_words);
    HIP_CHECK(hipMemsetAsync(xch.p, 0, xch.n * sizeof(unsigned long long), stream));
    epoch = 0;
  }
  if (!gl_err.p) {
    gl_err.alloc(1);
    HIP_CHECK(hipMemsetAsync(gl_err.p, 0, sizeof(int), stream));
    HIP_CHECK(hipHostMalloc((void **)&host_err, sizeof(int), hipHostMallocDefault));
  }
}
GlPersist xdtts_griffinlim::persist_args(int n_iter) {
  GlPersist p{};
  p.xch = xch.p;
  p.err = gl_err.p;
  p.epoch = epoch;
  p.poll_delay = 6;  // first poll 6 x 128 clocks after the publish (F = 1000: 4.31-4.36 us per iteration at 5..7, 4.39 behind the overlap-add, 4.45-4.53 at 2 or 10..12)
  epoch += (unsigned)n_iter + 2u;
  return p;
}

// The iteration engine on the current state (ang, tprev, S in place): n_iter iterations and, when
// audio_out is given, the final ISTFT into it.  Returns the buffer holding the final angles
// (*tprev_fin: the final rebuilt spectrum).  Small-to-medium frame counts run as ONE persistent
// launch; the caller holds the chip lock until the stream has drained and then asks
// persistent_failed().
const float2 *xdtts_griffinlim::run_iterations(const GlBufs &g, int n_iter, float alpha, float *audio_out, bool want_state,
                                               const float2 **tprev_fin, bool gen_phase) {
  int TF = 0, nblk = 0;
  last_persistent = false;
  err_fetched = false;
  if (tprev_fin) *tprev_fin = g.tprev;
  if (persistent_usable() && gl_persistent_plan(g.F, n_cu, &TF, &nblk)) {
    persist_prepare(gl_persistent_xch_words(nblk), (unsigned)n_iter);
    GlPersist p = persist_args(n_iter);
    p.nblk = nblk;
    p.TF = TF;
    env::override_int(env::GL_SPINS, &p.spins);  // test hook
    env::override_int(env::GL_SLOW, &p.slow);    // test hook: straggler workgroup
    p.gen_phase = gen_phase ? 1 : 0;
    p.seed = seed;
    if (want_state) {
      p.ang_out = g.ang2;
      tprev2.alloc((size_t)g.F * g.nb);
      p.tprev_out = tprev2.p;
      if (tprev_fin) *tprev_fin = p.tprev_out;
    }
#ifdef XDTTS_GL_PROFILE
    static DevBuf<unsigned long long> prof;
    prof.alloc(256 * 12);
    p.prof = prof.p;
#endif
    launch_gl_persistent(g, p, g.ang, g.tprev, n_iter, alpha, audio_out, stream);
#ifdef XDTTS_GL_PROFILE
    if (const char *path = env::raw(env::GL_PROFILE)) {
      std::vector<unsigned long long> hp((size_t)nblk * 12);
      HIP_CHECK(hipMemcpyAsync(hp.data(), prof.p, hp.size() * 8, hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      if (FILE *f = fopen(path, "w")) {
        fprintf(f, "%d %d\n", nblk, n_iter);
        for (int c = 0; c < nblk; ++c) {
          for (int i = 0; i < 12; ++i) fprintf(f, "%llu ", hp[(size_t)c * 12 + i]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
#endif
    last_persistent = true;
    return want_state ? g.ang2 : g.ang;
  }
  const float2 *fin = launch_gl_iterate(g, n_iter, alpha, stream);
  if (audio_out) launch_gl_final(g, fin, audio_out, stream);
  return fin;
}

// After the stream has drained: did a bounded spin of the persistent launch run out (grid not
// co-resident)?  If so the handle is demoted to the launch-per-iteration engine (and probes the
// persistent one again after PROBE_AFTER calls); the input state is intact, the caller re-runs.
// (fetch_error_word() ahead of a sync the caller needs anyway saves persistent_failed() its own round trip)
void xdtts_griffinlim::fetch_error_word() {
  if (!last_persistent) return;
  HIP_CHECK(hipMemcpyAsync(host_err, gl_err.p, sizeof(int), hipMemcpyDeviceToHost, stream));
  err_fetched = true;
}
bool xdtts_griffinlim::persistent_failed() {
  if (!last_persistent) return false;
  if (!err_fetched) {
    HIP_CHECK(hipMemcpyAsync(host_err, gl_err.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  err_fetched = false;
  if (!*host_err) return false;
  HIP_CHECK(hipMemsetAsync(gl_err.p, 0, sizeof(int), stream));
  HIP_CHECK(hipMemsetAsync(xch.p, 0, xch.n * sizeof(unsigned long long), stream));
  epoch = 0;
  gate.demote();
  std::fprintf(stderr, "libxdtts_hip: persistent Griffin-Lim exchange timed out (grid not co-resident); "
                       "this handle uses the launch-per-iteration engine for the next %d calls\n", EngineGate::PROBE_AFTER);
  return true;
}

// phase init + iterations + final ISTFT; S already in place.  Result in audio (device).
// phase_init 1 without a caller's phase0: the SPSI stage of the magnitude plan in place on g.S (what its run() returned) writes
// the angles and the zero previous spectrum, and the engines then take the route of a caller-supplied phase0.  The stage counts as preparation:
// ev.e[1] moves behind it, so last_ms[0] covers mel -> linear, prosody and the initial phase.  A retry after a demotion
// comes through here again and recomputes the phase from the intact S.
void xdtts_griffinlim::iterate(const GlBufs &g, const float *phase0_dev, int n_iter) {
  const float alpha = momentum / (1.0f + momentum);
  int TF = 0, nblk = 0;
  const bool use_spsi = !phase0_dev && mg.plan.spsi;
  if (use_spsi) {
    mg.spsi(g.S, g.ang, g.tprev);
    HIP_CHECK(hipEventRecord(ev.e[1], stream));
  }
  if (persistent_usable() && gl_persistent_plan(g.F, n_cu, &TF, &nblk)) {
    // one launch: nothing to capture; with the seeded stream the kernel draws the phase itself (no
    // phase-init launch, no window-sum table: the kernel keeps its own)
    if (phase0_dev) launch_gl_phase_init(g, seed, phase0_dev, stream);
    run_iterations(g, n_iter, alpha, audio.p, false, nullptr, !phase0_dev && !use_spsi);
    return;
  }
  if (!use_spsi) launch_gl_phase_init(g, seed, phase0_dev, stream);
  launch_gl_prepare(g, stream);
  last_persistent = false;
  // the launch-per-iteration loop is launch-bound: replay it as one hipGraph
  struct Key {
    GlBufs g;
    const float *audio;
    int n_iter;
    float alpha;
  } key;
  std::memset(&key, 0, sizeof key);
  std::memcpy(&key.g, &g, sizeof g);
  key.audio = audio.p;
  key.n_iter = n_iter;
  key.alpha = alpha;
  graph.replay(&key, sizeof key, stream, [&] { launch_gl_iterations(g, n_iter, alpha, audio.p, stream); });
}

void xdtts_griffinlim::finish_timings() {
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipEventElapsedTime(&last_ms[0], ev.e[0], ev.e[1]));
  HIP_CHECK(hipEventElapsedTime(&last_ms[1], ev.e[1], ev.e[2]));
  HIP_CHECK(hipEventElapsedTime(&last_ms[2], ev.e[0], ev.e[2]));
}

namespace xdtts {

// Slaney-scale helpers for create_mel_filter_bank (librosa.filters.mel, htk=False, norm="slaney")
static double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
  const double logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// pinv(A) = A^T (A A^T)^-1 for the full-row-rank mel basis, fp64 Cholesky.  librosa's nnls starts
// from lstsq(A, M) clipped at 0 and its L-BFGS-B refinement stops at iteration 0 for this
// objective scaling, so clip(pinv M, 0) is the inversion the vocoder performs.
void host_pinv(const float *basis, int n, int nbins, std::vector<float> &out) {
  std::vector<double> G((size_t)n * n, 0.0), z(n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0;
      for (int b = 0; b < nbins; ++b) s += (double)basis[(size_t)i * nbins + b] * basis[(size_t)j * nbins + b];
      G[(size_t)i * n + j] = G[(size_t)j * n + i] = s;
    }
  for (int j = 0; j < n; ++j) {
    double d = G[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= G[(size_t)j * n + k] * G[(size_t)j * n + k];
    if (!(d > 0)) fail(XDTTS_ERR_BAD_ARG, "mel basis is rank deficient (filter %d)", j);
    d = std::sqrt(d);
    G[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double s = G[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= G[(size_t)i * n + k] * G[(size_t)j * n + k];
      G[(size_t)i * n + j] = s / d;
    }
  }
  out.resize((size_t)nbins * n);
  for (int b = 0; b < nbins; ++b) {
    for (int i = 0; i < n; ++i) {
      double s = basis[(size_t)i * nbins + b];
      for (int k = 0; k < i; ++k) s -= G[(size_t)i * n + k] * z[k];
      z[i] = s / G[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = z[i];
      for (int k = i + 1; k < n; ++k) s -= G[(size_t)k * n + i] * z[k];
      z[i] = s / G[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i) out[(size_t)b * n + i] = (float)z[i];
  }
}

// lambda_max(A A^T) by power iteration (double): the Lipschitz constant of the NNLS gradient
double host_lipschitz(const float *basis, int n, int nbins) {
  std::vector<double> G((size_t)n * n, 0.0), v(n, 1.0 / std::sqrt((double)n)), w(n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0;
      for (int b = 0; b < nbins; ++b) s += (double)basis[(size_t)i * nbins + b] * basis[(size_t)j * nbins + b];
      G[(size_t)i * n + j] = G[(size_t)j * n + i] = s;
    }
  double lam = 0;
  for (int it = 0; it < 1000; ++it) {
    double nrm = 0;
    for (int i = 0; i < n; ++i) {
      double a = 0;
      for (int j = 0; j < n; ++j) a += G[(size_t)i * n + j] * v[j];
      w[i] = a;
      nrm += a * a;
    }
    nrm = std::sqrt(nrm);
    if (!(nrm > 0)) fail(XDTTS_ERR_BAD_ARG, "mel basis is all zero");
    for (int i = 0; i < n; ++i) v[i] = w[i] / nrm;
    const bool done = std::fabs(nrm - lam) <= 1e-13 * nrm;
    lam = nrm;
    if (done) break;
  }
  return lam;
}

void mel_filter_bank(double sr, int n_fft, int n_mels, double fmin, double fmax, float *out) {
  const int nb = (int)(n_fft / 2 + 1), nm = (int)n_mels;
  std::vector<double> mel_f(nm + 2);
  const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
  for (int i = 0; i < nm + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (nm + 1));
  for (int i = 0; i < nm; ++i) {
    const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int b = 0; b < nb; ++b) {
      const double f = (sr / 2.0) * b / (nb - 1);
      const double lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
      const double upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1]);
      const double wv = std::min(lower, upper);
      out[(size_t)i * nb + b] = (float)((wv > 0 ? wv : 0) * enorm);
    }
  }
}

// "Iterations enqueued" -> "audio on its way to a pinned buffer": phase init + iterations + final ISTFT on the S in place
// (iterate()), the delivery chain if wanted (delivery.h: one row, its records by value), ev.e[2], the copy into `host` (taken from
// the pool here unless the caller brought one, sized for what is delivered) and the engine's error word.  Nothing is waited for.
static void enqueue_run(xdtts_griffinlim *g, const GlBufs &b, const float *phase0_dev, int iters, bool deliver, PinnedGuard &host) {
  size_t N = (size_t)g->hop * (size_t)(b.F - 1);
  g->iterate(b, phase0_dev, iters);
  float *out = g->audio.p;
  if (deliver) {  // (a document at programme level takes the utterance unlevelled; sizing behind the loop's launches: growing drains the stream)
    g->dl.prepare_one(g->dl.stages(g->gopts.output_normalise, g->sink.dst && g->sink.unlevelled), N);
    out = g->dl.run(g->audio.p, 0, 1, g->gopts.rms_target);
    N = (size_t)g->dl.plan.dn[0];
  }
  HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
  if (deliver && g->sink.dst) {  // a document run: the utterance stays in HBM, at its place in the staging buffer
    HIP_CHECK(hipMemcpyAsync(g->sink.dst, out, N * sizeof(float), hipMemcpyDeviceToDevice, g->stream));
  } else {
    if (!host.p) host = PinnedGuard(N);
    HIP_CHECK(hipMemcpyAsync(host.p, out, N * sizeof(float), hipMemcpyDeviceToHost, g->stream));
  }
  if (deliver) g->dl.fetch_stats(0, 1, g->stream);  // the measurement, the gain and the stats travel back behind the audio
  g->fetch_error_word();
}
// ... and its counterpart: the wait and the engine's error word.  The persistent engine needs its grid co-resident (the
// caller holds the chip lock from enqueue_run until here); a timed-out exchange demotes the handle and the same run goes
// once more, on the launch-per-iteration engine (S, S' and the phase seed are intact until the next enqueue).
static void collect_run(xdtts_griffinlim *g, const GlBufs &b, const float *phase0_dev, int iters, bool deliver, PinnedGuard &host,
                        float **audio, size_t *n_samples) {
  g->finish_timings();  // (drains the stream)
  if (g->persistent_failed()) {
    HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));  // time the run that counts
    enqueue_run(g, b, phase0_dev, iters, deliver, host);  // (the delivery stages again: they read the loop's audio)
    g->finish_timings();
    if (g->persistent_failed()) fail(XDTTS_ERR_HIP, "Griffin-Lim: the fallback engine reported an exchange failure");
  }
  const size_t N = (size_t)g->hop * (size_t)(b.F - 1);
  if (deliver) g->dl.push_last(0);
  *audio = host.release();
  *n_samples = deliver ? g->dl.out_samples(0) : N;  // (dn, or what the silence stage decided on the device: its stats have landed)
}

// The loop alone on a state the caller has put in place (xdtts_griffinlim_infer_linear), then the audio in a pinned host buffer.
void gl_iterate_and_fetch(xdtts_griffinlim *g, const GlBufs &b, const float *phase0_dev, int iters, float **audio, size_t *n_samples,
                          bool normalise) {
  std::lock_guard<ChipLock> chip(chip_mutex(g->device));
  g->probe_tick();
  g->clear_last();
  g->mg.prepare(magnitude_plan_checked(MagnitudeRequest::none(1), &b.F, std::vector<Timbre>(), g->mg.phase_init), false);  // (the initial phase alone)
  PinnedGuard host;
  enqueue_run(g, b, phase0_dev, iters, normalise, host);
  collect_run(g, b, phase0_dev, iters, normalise, host, audio, n_samples);
}

// The loop's buffers for the magnitude plan in place: F' frames, sized for max(F, F'), reading what the chain's run() returns
static GlBufs request_bufs(xdtts_griffinlim *g) {
  GlBufs b = g->bufs((int)g->mg.plan.loop_rows);  // (sized by the enqueue in front of mel -> linear, where growing S drops no contents: nothing grows here)
  b.F = (int)g->mg.plan.rows.total;
  b.S = g->mg.loop_S(g->S.p);
  return b;
}
// GriffinLim::infer (G1..G6) from a mel in HBM, in two halves for a caller that overlaps the vocoder with other work
// (xdtts_synthesize_sequence): everything enqueued on g->stream, nothing waited for; then collect_run.  Caller holds g->mu and the
// chip lock.
// (req: checked against F -- the loop runs on what the magnitude chain returns, with F' frames.  gl_collect works from the plan
// this leaves in place: S, S' and the timbre's output are intact, a demoted engine's retry runs on them again.)
void gl_enqueue_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, PinnedGuard &host, const MagnitudeRequest &req) {
  MagnitudePlan plan = magnitude_plan_checked(req, &F, g->mg.timbres(), g->mg.phase_init, false, g->mg.denoises());
  g->bufs((int)plan.loop_rows);
  HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
  g->mg.prepare(std::move(plan), false);  // (a contour's table goes up on the stream; nothing is waited for)
  g->mel_to_linear(mel_dev_ptr, F);
  g->mg.run(g->S.p);
  HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
  g->probe_tick();
  enqueue_run(g, request_bufs(g), nullptr, g->iters, true, host);  // (the sequence hands in a buffer it took from the pool while the frame loop ran)
}
void gl_collect(xdtts_griffinlim *g, PinnedGuard &host, float **audio, size_t *n_samples) {
  collect_run(g, request_bufs(g), nullptr, g->iters, true, host, audio, n_samples);
  g->mg.collect_clean();  // (the stream is drained: the stage's stats have landed)
}

void gl_run_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, const MagnitudeRequest &req, float **audio, size_t *n_samples) {
  std::lock_guard<ChipLock> chip(chip_mutex(g->device));
  g->clear_last();
  PinnedGuard host;
  gl_enqueue_from_device_mel(g, mel_dev_ptr, F, host, req);
  gl_collect(g, host, audio, n_samples);
  g->mg.collect();
}

// The argument rules of xdtts_prosody for a request of n_frames frames; at most 2^20 frames go in (F' <= 2^22: the frame
// counts of the loop behind it are ints).
void prosody_check(const xdtts_prosody *p, size_t n_frames) {
  if (!p) fail(XDTTS_ERR_BAD_ARG, "null prosody");
  if (!std::isfinite(p->rate) || p->rate < 0.25f || p->rate > 4.0f) fail(XDTTS_ERR_BAD_ARG, "prosody rate %g is not in [0.25, 4]", (double)p->rate);
  if (!std::isfinite(p->pitch) || p->pitch < 0.5f || p->pitch > 2.0f) fail(XDTTS_ERR_BAD_ARG, "prosody pitch %g is not in [0.5, 2]", (double)p->pitch);
  if (p->lifter < 1 || p->lifter > 255) fail(XDTTS_ERR_BAD_ARG, "prosody lifter %d is not in [1, 255]", p->lifter);
  if (!std::isfinite(p->log_floor) || !(p->log_floor > 0.f)) fail(XDTTS_ERR_BAD_ARG, "prosody log_floor %g is not a positive number", (double)p->log_floor);
  if (n_frames > ((size_t)1 << 20)) fail(XDTTS_ERR_BAD_ARG, "prosody takes at most 2^20 frames, got %zu", n_frames);
  if ((p->rate != 1.0f || p->pitch != 1.0f) && n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "prosody needs at least 2 frames, got %zu", n_frames);
}

static_assert(sizeof(xdtts_prosody_point) == sizeof(ContourPoint) && offsetof(xdtts_prosody_point, gain) == offsetof(ContourPoint, gain),
              "xdtts_prosody_point and ContourPoint share one layout");
F0Job f0_job_checked(const xdtts_f0_opts *o) {
  static_assert(sizeof(xdtts_f0_opts) == sizeof(F0Opts) && sizeof(xdtts_pitch_target) == sizeof(PitchTarget), "the layouts of f0_plan.h");
  F0Job j;
  j.opts = f0_opts_default();
  if (o) std::memcpy(&j.opts, o, sizeof j.opts);
  bad_arg_if(f0_opts_check(j.opts));
  f0_quefrency(j.opts, &j.q_lo, &j.q_hi);
  return j;
}

void pitch_target_check_array(const xdtts_pitch_target *t, int n_utt) {
  if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
  if (!t) fail(XDTTS_ERR_BAD_ARG, "null pitch target");
  for (int u = 0; u < n_utt; ++u) {
    PitchTarget p;
    std::memcpy(&p, &t[u], sizeof p);
    const std::string msg = pitch_target_check(p);
    if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
  }
}

static_assert(sizeof(xdtts_prosody) == sizeof(Prosody) && offsetof(xdtts_prosody, log_floor) == offsetof(Prosody, log_floor) &&
                  sizeof(xdtts_prosody_contour) == sizeof(Contour) && offsetof(xdtts_prosody_contour, log_floor) == offsetof(Contour, log_floor),
              "the layouts of magnitude_plan.h");
MagnitudeRequest magnitude_request(const MagnitudeAsk &a, int n_utt, const size_t *n_frames, int first) {
  if (a.job) {
    std::vector<ContourTable> tabs;
    std::vector<PitchTarget> targets((size_t)n_utt);
    std::memcpy(targets.data(), a.tg, (size_t)n_utt * sizeof(PitchTarget));
    bool active = false, any_contour = false;
    bad_arg_if(target_tables(targets.data(), reinterpret_cast<const Contour *const *>(a.tc), n_utt, n_frames, tabs, &active, &any_contour));
    if (active || a.tracked) return MagnitudeRequest::targets(std::move(tabs), *a.job, std::move(targets));
    return any_contour ? MagnitudeRequest::contours(std::move(tabs)) : MagnitudeRequest::none(n_utt);  // (the bits of the contour entry, or of the plain one)
  }
  if (a.cont) {
    std::vector<ContourTable> tabs((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) {
      first < 0 ? contour_check(&a.cont[u], n_frames[u]) : contour_check_at(&a.cont[u], first + u, n_frames[u]);
      contour_table(a.cont[u], n_frames[u], tabs[(size_t)u]);
    }
    return MagnitudeRequest::contours(std::move(tabs));
  }
  if (!a.pros) return MagnitudeRequest::none(n_utt);
  for (int u = 0; n_frames && u < n_utt; ++u) first < 0 ? prosody_check(&a.pros[u], n_frames[u]) : prosody_check_at(&a.pros[u], first + u, n_frames[u]);
  return MagnitudeRequest::uniform(reinterpret_cast<const Prosody *>(a.pros), n_utt);
}

static const ContourPoint *contour_points(const xdtts_prosody_contour &c) { return reinterpret_cast<const ContourPoint *>(c.points); }

void contour_check(const xdtts_prosody_contour *c, size_t n_frames) {
  if (!c) fail(XDTTS_ERR_BAD_ARG, "null contour");
  bad_arg_if(xdtts::contour_check(contour_points(*c), c->n_points, c->lifter, c->log_floor, n_frames));
}

void contour_check_at(const xdtts_prosody_contour *c, int u, size_t n_frames) {
  try {
    contour_check(c, n_frames);
  } catch (const Error &e) {
    fail(e.code, "utterance %d: %s", u, e.what());
  }
}

void contour_check_array(const xdtts_prosody_contour *c, int n_utt) {
  if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
  if (!c) fail(XDTTS_ERR_BAD_ARG, "null contour array");
  for (int u = 0; u < n_utt; ++u) contour_check_at(&c[u], u, 2);
}

void contour_table(const xdtts_prosody_contour &c, size_t n_frames, ContourTable &t) {
  contour_build(contour_points(c), c.n_points, c.lifter, c.log_floor, n_frames, t);
}

void prosody_check_at(const xdtts_prosody *p, int u, size_t n_frames) {
  try {
    prosody_check(p, n_frames);
  } catch (const Error &e) {
    fail(e.code, "utterance %d: %s", u, e.what());
  }
}

void prosody_check_array(const xdtts_prosody *p, int n_utt) {
  if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
  if (!p) fail(XDTTS_ERR_BAD_ARG, "null prosody array");
  for (int u = 0; u < n_utt; ++u) prosody_check_at(&p[u], u, 2);
}

GlBatchArgs gl_batch_args(xdtts_griffinlim *g) {
  const int n_cu = g->persistent_usable() ? g->n_cu : 0;  // (first: the probe fills n_cu and per_cu4)
  return {n_cu, g->per_cu4, g->gopts.batch_shape, env::int_or(env::GL_BATCH_FORCE, 0)};
}

// The vocoder half of a batch from a mel that is already in HBM (on g's device): [n_mels][sum Fu], utterance u at columns
// fbase[u] .. fbase[u] + Fu[u].  mel -> linear is one GEMM over all frames, and the persistent kernel takes as many
// utterances per launch as fit one workgroup per CU (gl_plan.h: gl_batch_plan).  Caller holds g->mu.  The reads of the mel
// are enqueued on g->stream: the caller orders them behind the mel's producer (a stream sync or an event wait on g->stream).
// req: what the caller has checked against (or built for) the frame counts.  With an utterance that is not the identity the
// ragged stages (magnitude.h) follow the GEMM: S [sum F_u] -> S_pros [sum F'_u], and everything behind them -- the rows of the
// loop's arrays, the packing into launches, the audio -- works from F'_u and reads what the chain returns.  Without one,
// nothing new is launched.
void gl_batch_from_device(xdtts_griffinlim *g, const float *mel_dev_all, const std::vector<int> &Fin, float **audios, size_t *n_samples,
                          const MagnitudeRequest &req) {
  const int n_utt = (int)Fin.size();
  MagnitudePlan mplan = magnitude_plan_checked(req, Fin.data(), g->mg.timbres(), g->mg.phase_init, false, g->mg.denoises());
  HIP_CHECK(hipSetDevice(g->device));
  hipStream_t st = g->stream;
  GlBufs all = g->bufs((int)mplan.loop_rows);
  g->mg.prepare(std::move(mplan), true);  // (drains st behind the tables)
  const Rows &in = g->mg.plan.in, &rows = g->mg.plan.rows;  // the mel's frames F_u, and the frames behind the stages: F'_u
  const std::vector<int> &Fu = rows.F, &fbase = rows.row0;
  all.F = (int)rows.total;
  all.S = g->mg.loop_S(g->S.p);
  const bool use_spsi = g->mg.plan.spsi;
  std::vector<size_t> loop_n((size_t)n_utt);  // the loop's samples per utterance, back to back in its audio
  size_t Ntot = 0;
  for (int u = 0; u < n_utt; ++u) Ntot += loop_n[(size_t)u] = (size_t)g->hop * (size_t)(Fu[(size_t)u] - 1);
  const std::vector<long long> abase = delivery_bases(loop_n);
  g->audio.alloc(std::max<size_t>(Ntot, 1));
  // What is delivered (delivery_plan.h): at 22050 the loop's audio where it lies; at another rate the resampled utterances back
  // to back, and everything behind the loop works from those.  Counts, places and buffer sizes do not depend on the order of the
  // rows, which is known only with the launches: here the failure and every growth, in front of the launches.
  const DeliveryStages stages = g->dl.stages(g->gopts.output_normalise, false);
  const DeliveryPlan sized = delivery_plan_checked(stages, loop_n, abase, delivery_identity((size_t)n_utt));
  const std::vector<int> &dn = sized.dn;
  g->dl.size(sized);
  const float alpha = g->momentum / (1.0f + g->momentum);
  g->clear_last();
  std::lock_guard<ChipLock> chip(chip_mutex(g->device));
  g->probe_tick();
  for (int attempt = 0;; ++attempt) {
    // mel -> linear, the ragged stages, the initial phase: all from the mel, so a retry starts from an intact S / S'
    HIP_CHECK(hipEventRecord(g->ev.e[0], st));
    g->mel_to_linear(mel_dev_all, (int)in.total);
    g->mg.run(g->S.p);  // (out of place: a retry writes the same S_pros and S_timbre from the intact S)
    if (use_spsi) g->mg.spsi(all.S, all.ang, all.tprev);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    if (!use_spsi) launch_gl_phase_init_batch(all, g->seed, g->mg.frame_local.p, st);
    // the plan, on the host while the device works on the above.  A handle without a usable persistent engine (demoted: the
    // retry) gets the empty one: everything runs one by one on the launch-per-iteration kernels.
    const GlBatchArgs pa = gl_batch_args(g);
    const GlBatchPlan plan = gl_batch_plan(Fu, g->hop, pa.n_cu, pa.per_cu4, pa.batch_shape, pa.force);
    std::vector<PinnedGuard> out;  // each utterance straight into the buffer the caller receives
    out.reserve((size_t)n_utt);
    for (int u = 0; u < n_utt; ++u) out.emplace_back((size_t)dn[(size_t)u]);
    Drain drain(g->copy_stream);  // no buffer of `out` goes back to the pool while a copy into it may be in flight
    // The delivery stages.  The utterances of one fetch are consecutive rows of the tables (plan.order), so each fetch is
    // preceded by ONE launch per stage over exactly its utterances, in the chain's order: the level rules hold for the signal
    // the caller receives.
    g->dl.prepare(delivery_plan(stages, loop_n, abase, plan.order), true);  // (sized and checked above: nothing grows or throws; drains st)
    const DeliveryPlan &dp = g->dl.plan;
    size_t n_ev = 0;
    auto fetch_audio = [&](const std::vector<int> &utts) {  // after the work just enqueued on `st`
      const int r0 = utts.empty() ? 0 : dp.tab_pos[(size_t)utts[0]];
      const float *src = g->dl.run(g->audio.p, r0, (int)utts.size(), g->gopts.rms_target);  // where the delivered rows lie
      hipEvent_t e = g->launch_done(n_ev++);
      HIP_CHECK(hipEventRecord(e, st));
      HIP_CHECK(hipStreamWaitEvent(g->copy_stream, e, 0));
      for (int u : utts)
        HIP_CHECK(hipMemcpyAsync(out[(size_t)u].p, src + dp.dbase[(size_t)u], sizeof(float) * (size_t)dn[(size_t)u], hipMemcpyDeviceToHost,
                                 g->copy_stream));
      g->dl.fetch_stats(r0, (int)utts.size(), g->copy_stream);
    };
    // the persistent launches, each followed by the fetch of its utterances
    bool used_persistent = false;
    if (!plan.segs.empty()) {
      g->segs.upload(plan.segs.data(), plan.segs.size(), st);
      HIP_CHECK(hipStreamSynchronize(st));
      g->persist_prepare(gl_persistent_xch_words(g->n_cu * std::max(1, std::min(g->per_cu4, 2))),
                         (unsigned)plan.launches.size() * ((unsigned)g->iters + 2u));
      for (const GlBatchPlan::Launch &L : plan.launches) {
        GlPersist p = g->persist_args(g->iters);
        p.segs = g->segs.p + L.seg0;
        p.nblk = L.nblk;
        p.TF = plan.TF;
        p.per_cu = plan.WG;
        launch_gl_persistent(all, p, all.ang, all.tprev, g->iters, alpha, g->audio.p, st);
        fetch_audio(L.utts);
      }
      used_persistent = true;
    }
    // the rest one by one (tiny / very long utterances, or a demoted handle)
    for (int u = 0; u < n_utt; ++u) {
      if (plan.batched[(size_t)u]) continue;
      GlBufs v = all;
      v.F = Fu[u];
      v.S = all.S + (size_t)fbase[u] * g->nb;
      v.ang = all.ang + (size_t)fbase[u] * g->nb;
      v.ang2 = all.ang2 + (size_t)fbase[u] * g->nb;
      v.tprev = all.tprev + (size_t)fbase[u] * g->nb;
      v.frames = all.frames + (size_t)fbase[u] * g->n_fft;
      v.wss_inv = all.wss_inv + abase[(size_t)u];
      launch_gl_prepare(v, st);
      g->run_iterations(v, g->iters, alpha, g->audio.p + abase[(size_t)u]);  // the engine the single-utterance call uses
      used_persistent = used_persistent || g->last_persistent;
      fetch_audio(std::vector<int>(1, u));
    }
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    g->finish_timings();
    HIP_CHECK(hipStreamSynchronize(g->copy_stream));
    g->last_persistent = used_persistent;
    if (g->persistent_failed()) {
      if (attempt) fail(XDTTS_ERR_HIP, "Griffin-Lim batch: exchange failure on the fallback engine");
      continue;  // demoted
    }
    for (int u = 0; u < n_utt; ++u) {
      audios[u] = out[(size_t)u].release();
      n_samples[u] = g->dl.out_samples((size_t)u);  // (dn[u], or n_out of the silence stage: the buffer holds dn[u] floats)
      g->dl.push_last((size_t)dp.tab_pos[(size_t)u]);
    }
    g->mg.collect();
    g->mg.collect_clean();
    return;
  }
}

void gl_analysis_enqueue(xdtts_griffinlim *g, const float *const *audios, const size_t *n_samples, const Rows &rows, bool want_mel) {
  const int n_utt = rows.n();
  std::vector<long long> abase((size_t)n_utt);
  std::vector<AnSeg> segs;
  size_t Ntot = 0;
  for (int u = 0; u < n_utt; ++u) {
    abase[(size_t)u] = (long long)Ntot;
    for (int f0 = 0; f0 < rows.F[(size_t)u]; f0 += 4) {  // a workgroup: four consecutive frames of one utterance
      AnSeg sg{};
      sg.abase = (long long)Ntot;
      sg.n = (int)n_samples[u];
      sg.F = rows.F[(size_t)u];
      sg.f0 = f0;
      sg.row0 = rows.row0[(size_t)u];
      segs.push_back(sg);
    }
    Ntot += n_samples[u];
  }
  const size_t Ftot = rows.total;
  hipStream_t st = g->stream;
  g->an_audio.alloc(Ntot);
  for (int u = 0; u < n_utt; ++u)
    HIP_CHECK(hipMemcpyAsync(g->an_audio.p + abase[(size_t)u], audios[u], n_samples[u] * sizeof(float), hipMemcpyHostToDevice, st));
  g->an_segs.upload(segs.data(), segs.size(), st);
  g->an_S.alloc(Ftot * (size_t)g->nb);
  const int NBP = xdtts_griffinlim::NBP;
  if (want_mel) {
    g->an_P.alloc(Ftot * (size_t)NBP);
    g->an_melT.alloc(Ftot * (size_t)g->n_mels);
  }
  HIP_CHECK(hipStreamSynchronize(st));  // the host vector above
  // the handle's exponent, inverted: mel -> linear takes x^(1/power) (mode 0) / x^power (1) / x (2)
  const float e = g->gopts.power_mode == 0 ? g->power : (g->gopts.power_mode == 1 ? 1.0f / g->power : 1.0f);
  HIP_CHECK(hipEventRecord(g->an_ev.e[0], st));
  launch_stft_mag(g->an_audio.p, g->an_segs.p, (int)segs.size(), g->tw.p, g->win.p, g->an_S.p, want_mel ? g->an_P.p : nullptr, NBP, e, st);
  HIP_CHECK(hipEventRecord(g->an_ev.e[1], st));
  if (want_mel) {
    GemmArgs a{};  // melT = P basis^T (the residual GEMM of the NNLS refinement without the residual)
    a.A = g->an_P.p;
    a.lda = NBP;
    a.W = g->basis_p.p;  // [n_mels][NBP]
    a.C = g->an_melT.p;
    a.ldc = g->n_mels;
    a.M = (int)Ftot;
    a.N = g->n_mels;
    a.K = NBP;
    a.batch = 1;
    a.tile = 32;  // one tile shape whatever the row count: a frame's mel does not depend on what else is in the batch
    launch_gemm_nt(a, st);
  }
}

void gl_analysis_finish_timings(xdtts_griffinlim *g) {
  HIP_CHECK(hipStreamSynchronize(g->stream));
  HIP_CHECK(hipEventElapsedTime(&g->an_ms[0], g->an_ev.e[0], g->an_ev.e[1]));
  HIP_CHECK(hipEventElapsedTime(&g->an_ms[1], g->an_ev.e[1], g->an_ev.e[2]));
  HIP_CHECK(hipEventElapsedTime(&g->an_ms[2], g->an_ev.e[0], g->an_ev.e[2]));
}

}  // namespace xdtts
