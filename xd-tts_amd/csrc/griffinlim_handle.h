// griffinlim_handle.h -- the vocoder handle, the host-side mel-bank algebra, and the gl_* request paths the extern "C"
// functions of api_griffinlim.cpp, api_gl_magnitude.cpp, api_gl_delivery.cpp and api_synthesize.cpp share.
#pragma once
#include "delivery.h"
#include "engine_gate.h"
#include "kernels.h"
#include "magnitude.h"
#include "prosody_contour.h"
#include "runtime.h"

namespace xdtts {
// xdtts_prosody (include/xdtts.h): the argument rules.  Host arithmetic only.
void prosody_check(const xdtts_prosody *p, size_t n_frames);  // fails with XDTTS_ERR_BAD_ARG and a message
// xdtts_prosody_contour (include/xdtts.h) on top of prosody_contour.h, which knows no status codes: the argument rules for a
// request of n_frames frames (fails with XDTTS_ERR_BAD_ARG, the message names the field and the point), and the table.
void contour_check(const xdtts_prosody_contour *c, size_t n_frames);
void contour_check_at(const xdtts_prosody_contour *c, int u, size_t n_frames);  // ... for utterance u of a batch
void contour_check_array(const xdtts_prosody_contour *c, int n_utt);            // the fields of n_utt contours, before a handle is looked at
void contour_table(const xdtts_prosody_contour &c, size_t n_frames, ContourTable &t);  // (checked arguments)
// xdtts_f0_opts / xdtts_pitch_target on top of f0_plan.h, which knows no status codes: the checked options (null = the default)
// with their quefrency range, and the targets of n_utt utterances; both fail with XDTTS_ERR_BAD_ARG and need no handle.
F0Job f0_job_checked(const xdtts_f0_opts *o);
void pitch_target_check_array(const xdtts_pitch_target *t, int n_utt);
// What an entry asks for between mel -> linear and the loop, as the boundary received it (fields checked, frame counts not yet
// known): nothing, one prosody per utterance, one contour per utterance, or a tracker job with one target per utterance over
// contours that may be null (tracked: the target hook's -- the tracker runs even where every target is the identity).
struct MagnitudeAsk {
  const xdtts_prosody *pros = nullptr;
  const xdtts_prosody_contour *cont = nullptr;
  const F0Job *job = nullptr;
  const xdtts_pitch_target *tg = nullptr;
  const xdtts_prosody_contour *const *tc = nullptr;
  bool tracked = false;
  static MagnitudeAsk prosody(const xdtts_prosody *p) { return {p, nullptr, nullptr, nullptr, nullptr, false}; }
  static MagnitudeAsk contour(const xdtts_prosody_contour *c) { return {nullptr, c, nullptr, nullptr, nullptr, false}; }
  static MagnitudeAsk target(const F0Job *j, const xdtts_pitch_target *t, const xdtts_prosody_contour *const *c, bool tracked = false) { return {nullptr, nullptr, j, t, c, tracked}; }
  MagnitudeAsk at(int u) const { return {pros ? pros + u : nullptr, cont ? cont + u : nullptr, job, tg ? tg + u : nullptr, tc ? tc + u : nullptr, tracked}; }  // utterance u alone
};
// ... and the request it becomes once the frame counts are known: each utterance checked against its count (XDTTS_ERR_BAD_ARG;
// first >= 0: the utterances are first .. of a batch or sequence and the message names them), the contour tables built.
// n_frames == null (the uniform form or nothing, which need no count to be built): for frames() alone.
MagnitudeRequest magnitude_request(const MagnitudeAsk &a, int n_utt, const size_t *n_frames, int first = -1);
// The options of a stream request (stream_plan.h, which knows no status codes), before a handle is looked at; null = the default
inline StreamOpts stream_opts_checked(const xdtts_stream_opts *o) {
  StreamOpts s = stream_opts_default();
  if (o) std::memcpy(&s, o, sizeof s);
  bad_arg_if(stream_opts_check(s));
  return s;
}
// xdtts_timbre (include/xdtts.h) on top of timbre_plan.h, which knows no status codes: the checked setting (null = the default,
// the identity), before a handle is looked at.
inline Timbre timbre_checked(const xdtts_timbre *t) {
  static_assert(sizeof(xdtts_timbre) == sizeof(Timbre) && sizeof(Timbre) == 20, "Timbre is xdtts_timbre");
  Timbre s = timbre_default();
  if (t) std::memcpy(&s, t, sizeof s);
  bad_arg_if(timbre_check(s));
  return s;
}
// xdtts_denoise (include/xdtts.h) on top of denoise_plan.h: the checked setting (null = the default, the identity) and the
// caller's profile (null = none), before a handle is looked at.
inline Denoise denoise_checked(const xdtts_denoise *d, const float *profile) {
  Denoise s = denoise_default();
  if (d) std::memcpy(&s, d, sizeof s);
  bad_arg_if(denoise_check(s));
  bad_arg_if(denoise_profile_check(profile));
  return s;
}
// The *_plan.h headers know no status codes: past a cap they throw std::length_error, which inside a request fails with
// XDTTS_ERR_BAD_ARG and the text -- Rows::add (gl_plan.h), magnitude_plan (magnitude_plan.h: 2^24 rows) and delivery_plan
// (delivery_plan.h: more than 2^31 - 1 delivered samples)
template <class F>
inline auto bad_arg_past_cap(F f) -> decltype(f()) {
  try {
    return f();
  } catch (const std::length_error &e) {
    fail(XDTTS_ERR_BAD_ARG, "%s", e.what());
  }
}
inline void rows_add(Rows &r, size_t rows, size_t cap, const char *too_large) { bad_arg_past_cap([&] { r.add(rows, cap, too_large); }); }
template <class... A>
inline MagnitudePlan magnitude_plan_checked(const A &...a) { return bad_arg_past_cap([&] { return magnitude_plan(a...); }); }
template <class... A>
inline DeliveryPlan delivery_plan_checked(const A &...a) { return bad_arg_past_cap([&] { return delivery_plan(a...); }); }
}  // namespace xdtts

struct xdtts_griffinlim {
  using GlBufs = xdtts::GlBufs;
  using GlPersist = xdtts::GlPersist;
  template <class T>
  using DevBuf = xdtts::DevBuf<T>;
  int device = 0;
  hipStream_t stream = nullptr;
  mutable std::mutex mu;
  int n_mels = 0, nb = 0, n_fft = 0, hop = 0, iters = 0;
  float power = 1.f, momentum = 0.99f;
  uint32_t seed = 0;
  xdtts::Events ev;
  float last_ms[3] = {0, 0, 0};
  DevBuf<float> pinv, win, S, melT, mel_in, frames, wss_inv, audio, phase0;
  // mel->linear options (xdtts_griffinlim_opts) and the NNLS refinement's operands
  xdtts_griffinlim_opts gopts = [] { xdtts_griffinlim_opts o; xdtts_griffinlim_opts_default(&o); return o; }();  // one source for the defaults
  static constexpr int NBP = 528;  // bins padded to the GEMM's K granule
  DevBuf<float> basis_p, basisT_p, nnls_x, nnls_r;
  float nnls_step = 0.f;   // 1 / lambda_max(A A^T)
  xdtts::GraphCache graph;  // n_iter x (istft, stft) + final ISTFT for the cached (buffers, F, iterations, momentum, output)
  DevBuf<float2> tw, ang, ang2, tprev, tprev2;  // tprev2: final rebuilt spectrum of the parity hook
  // persistent engine (griffinlim.hip: k_gl_persistent)
  DevBuf<unsigned long long> xch;  // neighbour-overlap granules
  DevBuf<xdtts::GlSeg> segs;              // vocoder batch: per-workgroup segment table
  DevBuf<int> gl_err;
  int *host_err = nullptr;         // pinned
  unsigned epoch = 0;              // tag base; tags are never reused while xch lives
  xdtts::EngineGate gate;          // the persistent engine (engine_gate.h)
  int n_cu = 0;
  int per_cu4 = 1;                 // co-resident workgroups of the 4-frame shape per CU (vocoder batch)
  bool last_persistent = false;    // the last run_iterations used the persistent engine
  // vocoder batch: the audio of a finished launch goes to the host while the next launches run
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> copy_ev;
  hipEvent_t launch_done(size_t k) {
    if (!copy_stream) HIP_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    while (copy_ev.size() <= k) {
      hipEvent_t e = nullptr;
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      copy_ev.push_back(e);
    }
    return copy_ev[k];
  }

  // analysis (analysis.hip): audio -> magnitude -> mel, spectral convergence.  Buffers of its own: the iteration state
  // (S, angles, previous spectrum) of the handle is not touched.
  DevBuf<float> an_audio, an_S, an_P, an_melT, an_out, an_St;  // an_out: boundary-layout staging; an_St: a target, [F][nb]
  DevBuf<xdtts::AnSeg> an_segs;
  DevBuf<double> an_sums;  // 3 * SPD_PARTS partials, then the three sums
  xdtts::Events an_ev;
  float an_ms[3] = {0, 0, 0};

  // The magnitude chain between mel -> linear and the loop (magnitude.h): tracker and targets, prosody or contour, timbre, the SPSI
  // initial phase -- settings, tables, buffers, the tracker's stats of the last call, and the one runner of every request path.
  xdtts::Magnitude mg;

  // The delivery chain behind the loop (delivery.h): output rate, compressor, output normalisation or loudness with or without
  // the limiter -- settings, tables, buffers, the stats of the last call, and the one runner of every request path.
  xdtts::Delivery dl;
  void clear_last() { dl.clear_last(), mg.last_f0.clear(), mg.last_denoise.clear(); }

  // stream (stream.hip): the utterances of a sequence joined with their gaps, faded, levelled and encoded -- the stage behind
  // everything above (xdtts_griffinlim_join, xdtts_synthesize_document).
  DevBuf<float> st_src, st_f32, st_fade;      // the utterances' fp32 staging; the programme level's fp32 stream; the fade table
  DevBuf<unsigned char> st_out;               // the encoded stream
  DevBuf<xdtts::StreamUtt> st_tab, st_lim_tab;  // st_lim_tab: the same records with sources in the limited stream (programme level)
  std::vector<xdtts::StreamUtt> st_lim_tab_host;
  std::vector<xdtts::StreamUtt> st_tab_host;  // the uploads' sources: they stay until the next stream request of this handle,
  std::vector<float> st_fade_host;            // which starts behind a drained stream
  size_t st_used = 0;                         // floats of st_src that hold utterances of the request in flight
  // Where a document run delivers an utterance: enqueue_run copies to dst on the device instead of to a pinned host buffer (one
  // stream-ordered operation in the place of one; a demoted engine's retry writes the same place again), and with
  // `unlevelled` runs neither the loudness stage nor the output normalisation (programme level: one gain for the stream).
  struct StreamSink {
    float *dst = nullptr;
    bool unlevelled = false;
  } sink;
  // st_src with room for `floats` in all; what it holds (st_used floats) survives the growth.  Stream idle.
  void stream_reserve(size_t floats);
  // The stage on the stream, from st_tab_host (src0 into st_src) -> st_out (total * sample_bytes bytes): the table and the fade
  // table go up, then at level 0 ONE k_stream_join launch; at level 1 the fp32 stream is formed first (format 0, no gain),
  // measured once by the delivery chain's loudness stage at `rate` (with the limiter where it is on), and the encode launch reads
  // the gain from dl.loud_res[0] on the device -- the structs travel back behind it.  Checked arguments.
  // (begin: recorded behind the uploads, in front of the first launch)
  void stream_join(size_t total, const xdtts::StreamOpts &o, int rate, hipEvent_t begin = nullptr);

  ~xdtts_griffinlim();
  GlBufs bufs(int F);
  // The ragged parity hooks: utterance u's magnitude in the boundary layout (nb x F_u), uploaded through `frames` and transposed
  // into its rows of S [rows.total][nb], on the stream.  bufs(>= rows.total) first.
  void upload_rows(const float *const *S_host, const xdtts::Rows &rows);
  void mel_to_linear(const float *mel_dev_ptr, int F);
  // Once per API call (never inside a retry attempt): a demoted handle counts the call and, after PROBE_AFTER of them,
  // gives the persistent engine another try -- the cause of a timed-out exchange may have been transient.
  void probe_tick() { gate.tick(); }
  bool persistent_usable();
  // exchange granules and error word of the persistent kernel, ready for launches that consume `tags` epoch tags in all
  void persist_prepare(size_t xch_words, unsigned tags);
  GlPersist persist_args(int n_iter);  // of the next launch: exchange, error word, its epoch (advanced), the first-poll delay
  const float2 *run_iterations(const GlBufs &g, int n_iter, float alpha, float *audio_out, bool want_state = false,
                               const float2 **tprev_fin = nullptr, bool gen_phase = false);
  bool err_fetched = false;
  void fetch_error_word();
  bool persistent_failed();
  void iterate(const GlBufs &g, const float *phase0_dev, int n_iter);
  void finish_timings();
};

namespace xdtts {
void host_pinv(const float *basis, int n, int nbins, std::vector<float> &out);
double host_lipschitz(const float *basis, int n, int nbins);
void mel_filter_bank(double sr, int n_fft, int n_mels, double fmin, double fmax, float *out);

// The loop alone on the S in place (infer_linear: a caller's phase0 and iteration count, no normalisation); takes the chip lock.
void gl_iterate_and_fetch(xdtts_griffinlim *g, const GlBufs &b, const float *phase0_dev, int iters, float **audio, size_t *n_samples,
                          bool normalise);
// GriffinLim::infer from a mel in HBM, the one single-utterance request path: chip lock, gl_enqueue_from_device_mel, gl_collect,
// the tracker's stats.  (req: the magnitude chain behind mel -> linear, last_ms[0] covers both; F is the mel's frame count)
void gl_run_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, const MagnitudeRequest &req, float **audio, size_t *n_samples);
// ... and its two halves for a caller that holds the chip lock itself and works between them (the sequence entry); gl_collect
// works from the magnitude plan in place, the one of the enqueue in front of it
void gl_enqueue_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, PinnedGuard &host, const MagnitudeRequest &req);
void gl_collect(xdtts_griffinlim *g, PinnedGuard &host, float **audio, size_t *n_samples);
// (req: one utterance per element of Fu -- the ragged stages behind the one mel -> linear GEMM; audios[u] then has
// hop * (F'_u - 1) samples)
void gl_batch_from_device(xdtts_griffinlim *g, const float *mel_dev_all, const std::vector<int> &Fu, float **audios, size_t *n_samples,
                          const MagnitudeRequest &req);
// What gl_batch_plan (gl_plan.h) takes from the handle and the environment, read at the call: the probed CU count (0 without a
// usable persistent engine or under XDTTS_GL=launch: the empty plan), the co-resident 4-frame workgroups per CU, the batch_shape
// option and XDTTS_GL_BATCH_FORCE.  The one source for gl_batch_from_device and xdtts_griffinlim_batch_plan.  Caller holds g->mu;
// the first use probes the engine (device attributes only, nothing is launched).
struct GlBatchArgs {
  int n_cu, per_cu4, batch_shape, force;
};
GlBatchArgs gl_batch_args(xdtts_griffinlim *g);
// The fields of n_utt prosodies before any handle is looked at (entries that take an array): fails with XDTTS_ERR_BAD_ARG,
// the message names the field and the utterance.
void prosody_check_array(const xdtts_prosody *p, int n_utt);
void prosody_check_at(const xdtts_prosody *p, int u, size_t n_frames);  // prosody_check for utterance u of a batch or sequence

// Analysis of the audios in one k_stft_mag launch: utterance u's n_samples[u] / hop + 1 frames are its rows of `rows`;
// g->an_S [rows.total][nb] = |STFT|, and with want_mel g->an_melT [rows.total][n_mels] = an_S^e . basis^T (linear mel, before
// compression).  Everything is enqueued on g->stream behind an_ev.e[0]; an_ev.e[1] follows the magnitude kernel.  Caller holds g->mu.
void gl_analysis_enqueue(xdtts_griffinlim *g, const float *const *audios, const size_t *n_samples, const Rows &rows, bool want_mel);
void gl_analysis_finish_timings(xdtts_griffinlim *g);  // drains the stream; an_ms from an_ev.e[0..2] (e[2]: recorded by the caller behind its last kernel)
}  // namespace xdtts
