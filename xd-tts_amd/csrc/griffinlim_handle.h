// griffinlim_handle.h -- the vocoder handle, the host-side mel-bank algebra, and the gl_* request paths the extern "C"
// functions of api_griffinlim.cpp, api_gl_magnitude.cpp, api_gl_delivery.cpp and api_synthesize.cpp share.
#pragma once
#include "delivery.h"
#include "engine_gate.h"
#include "kernels.h"
#include "prosody_contour.h"
#include "runtime.h"

namespace xdtts {
// xdtts_prosody (include/xdtts.h): the argument rules, F' and the case that launches nothing.  Host arithmetic only.
inline bool prosody_is_identity(const xdtts_prosody &p) { return p.rate == 1.0f && p.pitch == 1.0f; }
size_t prosody_frames(size_t F, float rate);                   // 0 for a bad argument
void prosody_check(const xdtts_prosody *p, size_t n_frames);  // fails with XDTTS_ERR_BAD_ARG and a message
// xdtts_prosody_contour (include/xdtts.h) on top of prosody_contour.h, which knows no status codes: the argument rules for a
// request of n_frames frames (fails with XDTTS_ERR_BAD_ARG, the message names the field and the point), and the table.
void contour_check(const xdtts_prosody_contour *c, size_t n_frames);
void contour_check_at(const xdtts_prosody_contour *c, int u, size_t n_frames);  // ... for utterance u of a batch
void contour_check_array(const xdtts_prosody_contour *c, int n_utt);            // the fields of n_utt contours, before a handle is looked at
void contour_table(const xdtts_prosody_contour &c, size_t n_frames, ContourTable &t);  // (checked arguments)
// What a request path puts between mel -> linear and the loop, as ONE argument: nothing, a uniform prosody (checked by the
// caller), or the table of a contour (built by the caller once the frame count is known).  The single-utterance path reads
// element 0, the batch path one element per utterance.
// With a pitch target (f0_plan.h) the tables are a TargetPlan's and `f0` is its job: the tracker and the target run on S in
// front of the contour stage and multiply their ratios into the tables' pitches on the device.
struct F0Job {
  F0Opts opts;
  int q_lo = 0, q_hi = 0;
  const PitchTarget *targets = nullptr;  // one per utterance
};
struct ProsodyArg {
  const xdtts_prosody *uniform = nullptr;
  const ContourTable *contour = nullptr;
  const F0Job *f0 = nullptr;  // (with `contour` only)
  ProsodyArg() = default;
  ProsodyArg(std::nullptr_t) {}
  ProsodyArg(const xdtts_prosody *p) : uniform(p) {}
  ProsodyArg(const ContourTable *t, const F0Job *j = nullptr) : contour(t), f0(j) {}
  explicit operator bool() const { return uniform || contour; }
  bool identity(int u) const { return contour ? contour[u].identity : (!uniform || prosody_is_identity(uniform[u])); }
  int frames(int u, int F) const { return contour ? contour[u].Fout : (uniform ? (int)prosody_frames((size_t)F, uniform[u].rate) : F); }  // F'
};
// xdtts_f0_opts / xdtts_pitch_target on top of f0_plan.h, which knows no status codes: the checked options (null = the default)
// with their quefrency range, and the targets of n_utt utterances; both fail with XDTTS_ERR_BAD_ARG and need no handle.
F0Job f0_job_checked(const xdtts_f0_opts *o);
void pitch_target_check_array(const xdtts_pitch_target *t, int n_utt);
// What a target request runs on, built once the frame counts are known (checked options and targets): the contour tables --
// the caller's, or the rate-1 table where an utterance under a target that is not the identity has no contour of its own (its
// identity flag is off: the stage reads the pitches the device writes) -- and the job.  active = some target is not the
// identity; without it arg() is the request of the contours alone (or nothing: the bits of the plain entry).
struct TargetPlan {
  F0Job job;
  std::vector<PitchTarget> targets;
  std::vector<ContourTable> tabs;
  bool active = false, any_contour = false;
  ProsodyArg arg() const { return active ? ProsodyArg(tabs.data(), &job) : (any_contour ? ProsodyArg(tabs.data()) : ProsodyArg()); }
};
void target_plan(const F0Job &job, const xdtts_pitch_target *t, const xdtts_prosody_contour *const *c, int n_utt, const size_t *n_frames,
                 TargetPlan &p);
// The options of a stream request (stream_plan.h, which knows no status codes), before a handle is looked at; null = the default
inline StreamOpts stream_opts_checked(const xdtts_stream_opts *o) {
  StreamOpts s = stream_opts_default();
  if (o) std::memcpy(&s, o, sizeof s);
  bad_arg_if(stream_opts_check(s));
  return s;
}
// xdtts_timbre (include/xdtts.h) on top of timbre_plan.h, which knows no status codes: the checked setting (null = the default,
// the identity), before a handle is looked at; and the record of one utterance of the stage.
inline Timbre timbre_checked(const xdtts_timbre *t) {
  static_assert(sizeof(xdtts_timbre) == sizeof(Timbre) && sizeof(Timbre) == 20, "Timbre is xdtts_timbre");
  Timbre s = timbre_default();
  if (t) std::memcpy(&s, t, sizeof s);
  bad_arg_if(timbre_check(s));
  return s;
}
inline TimbreUtt timbre_utt(int src0, int dst0, int F, const Timbre &t) {
  return TimbreUtt{src0, dst0, F, t.vtl, t.breath, t.seed, t.lifter, t.log_floor};
}
// Rows::add (gl_plan.h, which knows no status codes) inside a request: past the cap it fails with XDTTS_ERR_BAD_ARG and the text
inline void rows_add(Rows &r, size_t rows, size_t cap, const char *too_large) {
  try {
    r.add(rows, cap, too_large);
  } catch (const std::length_error &e) {
    fail(XDTTS_ERR_BAD_ARG, "%s", e.what());
  }
}
// ... and delivery_plan (delivery_plan.h) likewise: more than 2^31 - 1 delivered samples fail with XDTTS_ERR_BAD_ARG and the text
inline DeliveryPlan delivery_plan_checked(const DeliveryStages &s, const std::vector<size_t> &n, const std::vector<long long> &base,
                                          const std::vector<int> &order) {
  try {
    return delivery_plan(s, n, base, order);
  } catch (const std::length_error &e) {
    fail(XDTTS_ERR_BAD_ARG, "%s", e.what());
  }
}
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
  DevBuf<int> frame_local;         // vocoder batch: row -> frame index inside its utterance
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

  // prosody (prosody.hip): the modified magnitude [F'][nb]; S itself stays as mel -> linear left it
  DevBuf<float> S_pros;
  DevBuf<xdtts::ProsodyUtt> pros_tab;  // vocoder batch: per-utterance rows and parameters of the ragged stage (k_prosody_batch)
  // ... and the contour form (k_prosody_contour), single call and batch alike: the per-utterance records and the concatenated
  // frame table {c, pitch, gain}.  The host vectors are the upload's source: they stay until the next contour request of this
  // handle, which every path starts behind a drained stream.
  DevBuf<xdtts::ContourUtt> contour_utts;
  DevBuf<unsigned> contour_ftab;
  std::vector<xdtts::ContourUtt> contour_utts_host;
  std::vector<unsigned> contour_ftab_host;
  int contour_n_tab = 0, contour_rows = 0;  // entries per array of the frame table; sum of F'
  // Uploads (on the stream) the records and tables of n_utt utterances lying back to back in S (rows F_u) and S_pros (rows
  // F'_u, allocated here); returns sum F'.  contour_launch() then runs the stage, any number of times (a retry).
  // (keep_pitch: a fourth array behind the three, the pitches once more -- what k_f0_track multiplies its ratios into `pitch` from)
  int contour_upload(const xdtts::ContourTable *tabs, int n_utt, bool keep_pitch = false);
  void contour_launch();
  // pitch tracker and pitch targets (f0.hip): raw / strength / f0 / ratio of the rows of a request, the per-utterance records
  // and stats.  f0_prepare() sizes the buffers and uploads the records (on the stream; the host vector stays until the next
  // tracker request of this handle); f0_launch() runs k_f0_frames on S_dev [rows][nb] and k_f0_track and sends the stats to
  // the pinned buffer, any number of times (a retry).  ftab: the contour table whose pitches take the ratios, or null.
  DevBuf<float> f0_raw, f0_strength, f0_val, f0_ratio;
  DevBuf<xdtts::F0Stats> f0_stats;
  DevBuf<xdtts::F0Utt> f0_utts;
  std::vector<xdtts::F0Utt> f0_utts_host;
  xdtts::PinnedArray<xdtts::F0Stats> f0_host;
  int f0_rows = 0;
  std::vector<xdtts_f0_stats> last_f0;  // xdtts_griffinlim_last_f0
  void f0_prepare(const std::vector<xdtts::F0Utt> &utts);
  void f0_prepare_contour(const xdtts::F0Job &job);  // ... from the records contour_upload() has just built
  void f0_launch(const float *S_dev, const xdtts::F0Job &job, unsigned *ftab, int n_tab, hipEvent_t between = nullptr);
  void f0_collect();  // behind a drained stream: the pinned stats -> last_f0

  // timbre (timbre.hip): the voice of this handle -- vocal-tract length and breathiness on the magnitude that would enter the
  // loop (S, or S_pros behind a prosody stage), out of place into S_timbre [F'][nb]; S and S_pros stay as their stages left them.
  // The identity (the default) launches and allocates nothing.  The table of the ragged form and its host vector, the upload's
  // source, stay until the next request of this handle, which every path starts behind a drained stream.
  xdtts::Timbre timbre = xdtts::timbre_default();
  bool timbre_on() const { return !xdtts::timbre_is_identity(timbre); }
  DevBuf<float> S_timbre;
  DevBuf<xdtts::TimbreUtt> timbre_tab;
  std::vector<xdtts::TimbreUtt> timbre_tab_host;
  // One utterance: S_in [F][nb] -> S_timbre (allocated by the caller) under t, one launch on the stream, nothing uploaded.
  void timbre_one(const float *S_in, int F, const xdtts::Timbre &t);
  // Ragged: the records of timbre_tab_host (uploaded by the caller as timbre_tab), rows_all rows, one launch; any number of
  // times (a retry).
  void timbre_rows(const float *S_in, int rows_all);

  // initial phase (phase_spsi.hip): 0 = the seeded random stream, 1 = SPSI on the magnitude that enters the loop
  int phase_init = 0;
  DevBuf<uint2> spsi_map, spsi_comp;
  DevBuf<unsigned> spsi_entry, spsi_turns;  // spsi_turns: the parity hooks only
  DevBuf<xdtts::SpsiSeg> spsi_segs;         // vocoder batch: the segments of all utterances
  DevBuf<xdtts::SpsiUtt> spsi_utts;
  // The SPSI stage on the stream: S [F][nb] -> ang, tprev (and turns, if wanted).  One utterance ...
  void spsi(const float *S_dev, int F, float2 *ang_out, float2 *tprev_out, unsigned *turns = nullptr);
  // ... and the ragged form: spsi_tables() (uploads; the caller drains the stream before the host vectors go), then any
  // number of spsi_batch() launches on the rows the tables describe.
  struct SpsiTables {
    std::vector<xdtts::SpsiSeg> segs;
    std::vector<xdtts::SpsiUtt> utts;
    int rows = 0;
    bool chained = false;
  };
  void spsi_tables(const std::vector<int> &Fu, SpsiTables &t);
  void spsi_batch(const float *S_dev, const SpsiTables &t, float2 *ang_out, float2 *tprev_out, unsigned *turns = nullptr);

  // The delivery chain behind the loop (delivery.h): output rate, compressor, output normalisation or loudness with or without
  // the limiter -- settings, tables, buffers, the stats of the last call, and the one runner of every request path.
  xdtts::Delivery dl;
  void clear_last() { dl.clear_last(), last_f0.clear(); }

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
  // S [F][nb] -> S_pros [F'][nb] in one launch on the stream; returns F'.  The identity launches nothing and returns F.
  // The caller then points GlBufs.S at prosody_S(p) with F' frames; its bufs() was sized for max(F, F').
  // (a contour: its table goes up on the stream in front of the launch of k_prosody_contour)
  int prosody(const xdtts::ProsodyArg &p, int F);
  float *prosody_S(const xdtts::ProsodyArg &p) { return p.identity(0) ? S.p : S_pros.p; }
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
// GriffinLim::infer from a mel in HBM, the one single-utterance request path: chip lock, gl_enqueue_from_device_mel, gl_collect.
// (p: nothing, a checked prosody or a contour's table -- the single-utterance stage behind mel -> linear, last_ms[0] covers
// both; F stays the mel's frame count everywhere)
void gl_run_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, const ProsodyArg &p, float **audio, size_t *n_samples);
// ... and its two halves for a caller that holds the chip lock itself and works between them (the sequence entry)
void gl_enqueue_from_device_mel(xdtts_griffinlim *g, const float *mel_dev_ptr, int F, PinnedGuard &host, const ProsodyArg &p = ProsodyArg());
void gl_collect(xdtts_griffinlim *g, int F, PinnedGuard &host, float **audio, size_t *n_samples, const ProsodyArg &p = ProsodyArg());
// (pros: nothing, or one checked prosody / one contour table per utterance -- the ragged stage behind the one mel -> linear
// GEMM; audios[u] then has hop * (F'_u - 1) samples)
void gl_batch_from_device(xdtts_griffinlim *g, const float *mel_dev_all, const std::vector<int> &Fu, float **audios, size_t *n_samples,
                          const ProsodyArg &pros = ProsodyArg());
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
