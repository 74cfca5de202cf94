// xdtts_host.hpp -- header-only C++ mirror of the reference's Rust surface for the hot path, over
// the C ABI of include/xdtts.h.  (The reference's host language is Rust; this image has no Rust
// toolchain, so the host-side mirror is C++.  INTEGRATION.md holds the equivalent Rust shim.)
//
//   xdtts::Tacotron2::load(path)            -- Tacotron2::load,  src/tacotron2/mod.rs:242
//   xdtts::Tacotron2::infer(units)          -- Tacotron2::infer, src/tacotron2/mod.rs:398
//   xdtts::create_mel_filter_bank(...)      -- griffin_lim::mel, src/tacotron2/mod.rs:453
//   xdtts::GriffinLim(basis, noverlap, power, iter, momentum) / infer(mel)
//                                           -- src/tacotron2/mod.rs:456, src/lib.rs:141
//   xdtts::create_griffin_lim()             -- src/tacotron2/mod.rs:441-458
// Errors become xdtts::Error (the shim's anyhow::Error); nothing here computes on the CPU.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "xdtts.h"

namespace xdtts {

struct Error : std::runtime_error {
  xdtts_status status;
  Error(xdtts_status s, const char *what) : std::runtime_error(what), status(s) {}
};
inline void check(xdtts_status s) {
  if (s != XDTTS_OK) throw Error(s, xdtts_last_error());
}

// Array2<f32> stand-in: row-major (rows x cols)
struct Array2 {
  size_t rows = 0, cols = 0;
  std::vector<float> data;
  float &operator()(size_t r, size_t c) { return data[r * cols + c]; }
  float operator()(size_t r, size_t c) const { return data[r * cols + c]; }
};

// A unit is carried as its token text ("IH0", " ", ".", "a"), i.e. Unit::from_str's input.
struct Unit {
  std::string token;
  bool is_character = false;  // Unit::Character(c) built directly (grapheme input)
};

class Tacotron2 {
 public:
  // (device_id: XDTTS_DEVICE_DEFAULT = the process's default GPU, environment variable XDTTS_DEVICE -- the reference's load(path) takes none)
  static Tacotron2 load(const std::string &path, int device_id = XDTTS_DEVICE_DEFAULT) {
    xdtts_tacotron2 *h = nullptr;
    check(xdtts_tacotron2_load(path.c_str(), device_id, &h));
    return Tacotron2(h);
  }
  static Tacotron2 synthetic(uint32_t seed = 20240327u, float rec_scale = 1.0f, int device_id = XDTTS_DEVICE_DEFAULT) {
    xdtts_tacotron2 *h = nullptr;
    check(xdtts_tacotron2_load_synthetic(seed, rec_scale, device_id, &h));
    return Tacotron2(h);
  }
  Tacotron2(Tacotron2 &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Tacotron2 &operator=(Tacotron2 &&o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  Tacotron2(const Tacotron2 &) = delete;
  Tacotron2 &operator=(const Tacotron2 &) = delete;
  ~Tacotron2() { xdtts_tacotron2_free(h_); }

  // src/tacotron2/mod.rs:398-437: find_splits(units, 100); units with no id are dropped (:403-406);
  // chunks are inferred independently and concatenated on the time axis.
  Array2 infer(const std::vector<Unit> &units, const xdtts_infer_opts *opts = nullptr) const {
    std::vector<int64_t> ids;
    for (const Unit &u : units) {
      const int64_t id = xdtts_unit_id(u.token.c_str(), u.is_character ? 1 : 0);
      if (id >= 0) ids.push_back(id);
    }
    xdtts_infer_opts o;
    xdtts_infer_opts_default(&o);
    if (opts) o = *opts;
    std::vector<size_t> splits(ids.size() + 2);
    size_t n_splits = 0;
    check(xdtts_find_splits(ids.data(), ids.size(), (size_t)o.max_chunk, splits.data(), splits.size(), &n_splits));
    float *mel = nullptr;
    size_t frames = 0;
    check(xdtts_tacotron2_infer_ids(h_, ids.data(), ids.size(), splits.data(), n_splits, &o, &mel, &frames));
    Array2 out;
    out.rows = 80;
    out.cols = frames;
    out.data.assign(mel, mel + 80 * frames);
    xdtts_free(mel);
    return out;
  }
  xdtts_tacotron2 *raw() const { return h_; }

  // Per-id durations and timing marks (xdtts_durations_opts): the setting, and what the last call captured per utterance
  struct Durations {
    std::vector<float> dur;
    std::vector<uint32_t> dur_q16;
    std::vector<uint64_t> start_q16;
    xdtts_alignment_stats stats;
  };
  void set_durations(const xdtts_durations_opts &o) { check(xdtts_tacotron2_set_durations(h_, &o)); }
  xdtts_durations_opts get_durations() const {
    xdtts_durations_opts o;
    check(xdtts_tacotron2_get_durations(h_, &o));
    return o;
  }
  std::vector<Durations> last_durations() const {
    size_t n_utt = 0;
    check(xdtts_tacotron2_last_durations_count(h_, &n_utt));
    std::vector<Durations> out(n_utt);
    for (size_t u = 0; u < n_utt; ++u) {
      size_t n = 0;
      check(xdtts_tacotron2_last_durations(h_, u, nullptr, nullptr, nullptr, 0, &n));
      out[u].dur.resize(n);
      out[u].dur_q16.resize(n);
      out[u].start_q16.resize(n);
      check(xdtts_tacotron2_last_durations(h_, u, out[u].dur.data(), out[u].dur_q16.data(), out[u].start_q16.data(), n, &n));
      check(xdtts_tacotron2_last_alignment(h_, u, &out[u].stats));
    }
    return out;
  }

 private:
  explicit Tacotron2(xdtts_tacotron2 *h) : h_(h) {}
  xdtts_tacotron2 *h_ = nullptr;
};

// create_mel_filter_bank(sample_rate, n_fft, n_mels, fmin, fmax: Option<f32>); NaN = None
inline Array2 create_mel_filter_bank(float sample_rate, size_t n_fft, size_t n_mels, float fmin, float fmax = NAN) {
  Array2 b;
  b.rows = n_mels;
  b.cols = n_fft / 2 + 1;
  b.data.resize(b.rows * b.cols);
  check(xdtts_mel_filter_bank(sample_rate, n_fft, n_mels, fmin, fmax, b.data.data()));
  return b;
}

class GriffinLim {
 public:
  GriffinLim(const Array2 &mel_basis, size_t noverlap, float power, size_t iter, float momentum, int device_id = XDTTS_DEVICE_DEFAULT)
      : n_mels_(mel_basis.rows), n_bins_(mel_basis.cols) {
    check(xdtts_griffinlim_new(mel_basis.data.data(), mel_basis.rows, mel_basis.cols, noverlap, power, iter, momentum,
                               device_id, &g_));
  }
  GriffinLim(GriffinLim &&o) noexcept : g_(std::exchange(o.g_, nullptr)), n_mels_(o.n_mels_), n_bins_(o.n_bins_) {}
  GriffinLim(const GriffinLim &) = delete;
  GriffinLim &operator=(const GriffinLim &) = delete;
  ~GriffinLim() { xdtts_griffinlim_free(g_); }

  std::vector<float> infer(const Array2 &mel) const {
    float *audio = nullptr;
    size_t n = 0;
    check(xdtts_griffinlim_infer(g_, mel.data.data(), mel.rows, mel.cols, &audio, &n));
    std::vector<float> out(audio, audio + n);
    xdtts_free(audio);
    return out;
  }
  // Speaking rate and pitch in the vocoder (xdtts_prosody: rate > 1 faster, pitch > 1 higher; the formants stay): infer() with the
  // stage between mel -> linear and the loop.  The audio has 256 * (xdtts_prosody_frames(mel.cols, p.rate) - 1) samples.
  std::vector<float> infer(const Array2 &mel, const xdtts_prosody &p) const {
    float *audio = nullptr;
    size_t n = 0;
    check(xdtts_griffinlim_infer_prosody(g_, mel.data.data(), mel.rows, mel.cols, &p, &audio, &n));
    std::vector<float> out(audio, audio + n);
    xdtts_free(audio);
    return out;
  }
  // ... and the stage alone (parity hook): S (n_bins x F) -> S' (n_bins x F')
  Array2 prosody_linear(const Array2 &S, const xdtts_prosody &p) const {
    const size_t Fp = xdtts_prosody_frames(S.cols, p.rate);
    Array2 out{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))};
    check(xdtts_griffinlim_prosody_linear(g_, S.data.data(), S.cols, &p, out.data.data(), nullptr));
    return out;
  }
  // infer() for several utterances in one call, one prosody per utterance (xdtts_griffinlim_infer_batch_prosody): the stage
  // runs as one ragged launch behind the batch's mel -> linear GEMM
  std::vector<std::vector<float>> infer_batch(const std::vector<Array2> &mels, const std::vector<xdtts_prosody> &p) const {
    const size_t n = mels.size();
    if (p.size() != n) throw std::runtime_error("xdtts: one prosody per utterance");
    std::vector<const float *> mp(n);
    std::vector<size_t> nf(n), ns(n, 0);
    std::vector<float *> audios(n, nullptr);
    for (size_t u = 0; u < n; ++u) {
      mp[u] = mels[u].data.data();
      nf[u] = mels[u].cols;
    }
    check(xdtts_griffinlim_infer_batch_prosody(g_, mp.data(), n ? mels[0].rows : 0, nf.data(), (int32_t)n, p.data(), audios.data(), ns.data()));
    std::vector<std::vector<float>> out(n);
    for (size_t u = 0; u < n; ++u) {
      out[u].assign(audios[u], audios[u] + ns[u]);
      xdtts_free(audios[u]);
    }
    return out;
  }
  // ... and the ragged stage alone (parity hook, xdtts_griffinlim_prosody_linear_batch)
  std::vector<Array2> prosody_linear_batch(const std::vector<Array2> &S, const std::vector<xdtts_prosody> &p) const {
    const size_t n = S.size();
    if (p.size() != n) throw std::runtime_error("xdtts: one prosody per utterance");
    std::vector<Array2> out(n);
    std::vector<const float *> sp(n);
    std::vector<float *> op(n);
    std::vector<size_t> nf(n);
    for (size_t u = 0; u < n; ++u) {
      const size_t Fp = xdtts_prosody_frames(S[u].cols, p[u].rate);
      out[u] = Array2{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))};
      sp[u] = S[u].data.data();
      op[u] = out[u].data.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_prosody_linear_batch(g_, sp.data(), nf.data(), (int32_t)n, p.data(), op.data(), nullptr));
    return out;
  }
  // Rate, pitch and gain that vary INSIDE an utterance (xdtts_prosody_contour: points (pos, rate, pitch, gain), pos a fraction of
  // the utterance's duration): infer() with the contour stage between mel -> linear and the loop.  The audio has
  // 256 * (xdtts_prosody_contour_frames(&c, mel.cols) - 1) samples.
  std::vector<float> infer(const Array2 &mel, const xdtts_prosody_contour &c) const {
    float *audio = nullptr;
    size_t n = 0;
    check(xdtts_griffinlim_infer_contour(g_, mel.data.data(), mel.rows, mel.cols, &c, &audio, &n));
    std::vector<float> out(audio, audio + n);
    xdtts_free(audio);
    return out;
  }
  // ... the stage alone (parity hooks: xdtts_griffinlim_contour_linear, and the ragged xdtts_griffinlim_contour_linear_batch)
  Array2 contour_linear(const Array2 &S, const xdtts_prosody_contour &c) const {
    const size_t Fp = xdtts_prosody_contour_frames(&c, S.cols);
    Array2 out{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))};
    check(xdtts_griffinlim_contour_linear(g_, S.data.data(), S.cols, &c, out.data.data(), nullptr));
    return out;
  }
  std::vector<Array2> contour_linear_batch(const std::vector<Array2> &S, const std::vector<xdtts_prosody_contour> &c) const {
    const size_t n = S.size();
    if (c.size() != n) throw std::runtime_error("xdtts: one contour per utterance");
    std::vector<Array2> out(n);
    std::vector<const float *> sp(n);
    std::vector<float *> op(n);
    std::vector<size_t> nf(n);
    for (size_t u = 0; u < n; ++u) {
      const size_t Fp = xdtts_prosody_contour_frames(&c[u], S[u].cols);
      out[u] = Array2{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))};
      sp[u] = S[u].data.data();
      op[u] = out[u].data.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_contour_linear_batch(g_, sp.data(), nf.data(), (int32_t)n, c.data(), op.data(), nullptr));
    return out;
  }
  // ... and for several utterances in one call, one contour per utterance (xdtts_griffinlim_infer_batch_contour)
  std::vector<std::vector<float>> infer_batch(const std::vector<Array2> &mels, const std::vector<xdtts_prosody_contour> &c) const {
    const size_t n = mels.size();
    if (c.size() != n) throw std::runtime_error("xdtts: one contour per utterance");
    std::vector<const float *> mp(n);
    std::vector<size_t> nf(n), ns(n, 0);
    std::vector<float *> audios(n, nullptr);
    for (size_t u = 0; u < n; ++u) {
      mp[u] = mels[u].data.data();
      nf[u] = mels[u].cols;
    }
    check(xdtts_griffinlim_infer_batch_contour(g_, mp.data(), n ? mels[0].rows : 0, nf.data(), (int32_t)n, c.data(), audios.data(), ns.data()));
    std::vector<std::vector<float>> out(n);
    for (size_t u = 0; u < n; ++u) {
      out[u].assign(audios[u], audios[u] + ns[u]);
      xdtts_free(audios[u]);
    }
    return out;
  }
  // Pitch tracking on the device and pitch targets (xdtts_f0_opts, xdtts_pitch_target: an absolute median pitch in Hz and / or a
  // scaled pitch range, what SSML pitch="180Hz" and range= ask for).  The tracker alone, from a
  // magnitude (xdtts_griffinlim_f0_linear), a mel (xdtts_griffinlim_f0) or audio at 22 050 Hz (xdtts_griffinlim_f0_audio);
  // o == nullptr: the default options.
  struct F0Track {
    std::vector<float> raw, strength, f0;  // per frame: raw F0 in Hz, the cepstral peak, the smoothed F0 (0 = unvoiced)
    xdtts_f0_stats stats{};
  };
  F0Track f0_linear(const Array2 &S, const xdtts_f0_opts *o = nullptr) const {
    F0Track t{std::vector<float>(S.cols), std::vector<float>(S.cols), std::vector<float>(S.cols)};
    check(xdtts_griffinlim_f0_linear(g_, S.data.data(), S.cols, o, t.raw.data(), t.strength.data(), t.f0.data(), &t.stats));
    return t;
  }
  std::vector<F0Track> f0_linear_batch(const std::vector<Array2> &S, const xdtts_f0_opts *o = nullptr) const {
    const size_t n = S.size();
    std::vector<F0Track> out(n);
    std::vector<const float *> sp(n);
    std::vector<float *> rp(n), tp(n), fp(n);
    std::vector<size_t> nf(n);
    std::vector<xdtts_f0_stats> st(n);
    for (size_t u = 0; u < n; ++u) {
      out[u] = F0Track{std::vector<float>(S[u].cols), std::vector<float>(S[u].cols), std::vector<float>(S[u].cols)};
      sp[u] = S[u].data.data();
      rp[u] = out[u].raw.data();
      tp[u] = out[u].strength.data();
      fp[u] = out[u].f0.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_f0_linear_batch(g_, sp.data(), nf.data(), (int32_t)n, o, rp.data(), tp.data(), fp.data(), st.data()));
    for (size_t u = 0; u < n; ++u) out[u].stats = st[u];
    return out;
  }
  F0Track f0(const Array2 &mel, const xdtts_f0_opts *o = nullptr) const {
    F0Track t{std::vector<float>(mel.cols), std::vector<float>(mel.cols), std::vector<float>(mel.cols)};
    check(xdtts_griffinlim_f0(g_, mel.data.data(), mel.rows, mel.cols, o, t.raw.data(), t.strength.data(), t.f0.data(), &t.stats));
    return t;
  }
  F0Track f0_audio(const std::vector<float> &audio, const xdtts_f0_opts *o = nullptr) const {
    const size_t F = xdtts_griffinlim_analysis_frames(g_, audio.size());
    F0Track t{std::vector<float>(F), std::vector<float>(F), std::vector<float>(F)};
    check(xdtts_griffinlim_f0_audio(g_, audio.data(), audio.size(), o, t.raw.data(), t.strength.data(), t.f0.data(), &t.stats));
    return t;
  }
  // ... infer() with the tracker, the target and the contour stage between mel -> linear and the loop
  // (xdtts_griffinlim_infer_pitch_target; c == nullptr: no contour), and for several utterances (one target each, contours that
  // may be null: xdtts_griffinlim_infer_batch_pitch_target).  last_f0() then returns the stats.
  std::vector<float> infer(const Array2 &mel, const xdtts_pitch_target &t, const xdtts_prosody_contour *c = nullptr,
                           const xdtts_f0_opts *o = nullptr) const {
    float *audio = nullptr;
    size_t n = 0;
    check(xdtts_griffinlim_infer_pitch_target(g_, mel.data.data(), mel.rows, mel.cols, o, &t, c, &audio, &n));
    std::vector<float> out(audio, audio + n);
    xdtts_free(audio);
    return out;
  }
  std::vector<std::vector<float>> infer_batch(const std::vector<Array2> &mels, const std::vector<xdtts_pitch_target> &t,
                                              const std::vector<const xdtts_prosody_contour *> *c = nullptr,
                                              const xdtts_f0_opts *o = nullptr) const {
    const size_t n = mels.size();
    if (t.size() != n || (c && c->size() != n)) throw std::runtime_error("xdtts: one pitch target (and contour pointer) per utterance");
    std::vector<const float *> mp(n);
    std::vector<size_t> nf(n), ns(n, 0);
    std::vector<float *> audios(n, nullptr);
    for (size_t u = 0; u < n; ++u) {
      mp[u] = mels[u].data.data();
      nf[u] = mels[u].cols;
    }
    check(xdtts_griffinlim_infer_batch_pitch_target(g_, mp.data(), n ? mels[0].rows : 0, nf.data(), (int32_t)n, o, t.data(),
                                                    c ? c->data() : nullptr, audios.data(), ns.data()));
    std::vector<std::vector<float>> out(n);
    for (size_t u = 0; u < n; ++u) {
      out[u].assign(audios[u], audios[u] + ns[u]);
      xdtts_free(audios[u]);
    }
    return out;
  }
  // ... the application alone (parity hooks: xdtts_griffinlim_pitch_target_linear and its ragged form): S' and the ratios
  std::pair<Array2, std::vector<float>> pitch_target_linear(const Array2 &S, const xdtts_pitch_target &t, const xdtts_prosody_contour *c = nullptr,
                                                            const xdtts_f0_opts *o = nullptr, xdtts_f0_stats *stats = nullptr) const {
    const size_t Fp = c ? xdtts_prosody_contour_frames(c, S.cols) : S.cols;
    std::pair<Array2, std::vector<float>> out{Array2{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))}, std::vector<float>(S.cols)};
    check(xdtts_griffinlim_pitch_target_linear(g_, S.data.data(), S.cols, o, &t, c, out.first.data.data(), out.second.data(), stats));
    return out;
  }
  std::vector<Array2> pitch_target_linear_batch(const std::vector<Array2> &S, const std::vector<xdtts_pitch_target> &t,
                                                const std::vector<const xdtts_prosody_contour *> *c = nullptr,
                                                const xdtts_f0_opts *o = nullptr) const {
    const size_t n = S.size();
    if (t.size() != n || (c && c->size() != n)) throw std::runtime_error("xdtts: one pitch target (and contour pointer) per utterance");
    std::vector<Array2> out(n);
    std::vector<const float *> sp(n);
    std::vector<float *> op(n);
    std::vector<size_t> nf(n);
    for (size_t u = 0; u < n; ++u) {
      const size_t Fp = c && (*c)[u] ? xdtts_prosody_contour_frames((*c)[u], S[u].cols) : S[u].cols;
      out[u] = Array2{n_bins_, Fp, std::vector<float>(n_bins_ * (Fp ? Fp : 1))};
      sp[u] = S[u].data.data();
      op[u] = out[u].data.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_pitch_target_linear_batch(g_, sp.data(), nf.data(), (int32_t)n, o, t.data(), c ? c->data() : nullptr, op.data(),
                                                     nullptr, nullptr));
    return out;
  }
  // The stats of the last call that ran the tracker, one per utterance (xdtts_griffinlim_last_f0)
  std::vector<xdtts_f0_stats> last_f0() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_f0(g_, nullptr, 0, &n));
    std::vector<xdtts_f0_stats> out(n);
    if (n) check(xdtts_griffinlim_last_f0(g_, out.data(), out.size(), &n));
    return out;
  }
  // The conventions of the crate's mel->linear step as switches (xdtts_griffinlim_opts)
  void set_opts(const xdtts_griffinlim_opts &o) { check(xdtts_griffinlim_set_opts(g_, &o)); }
  xdtts_griffinlim_opts opts() const {
    xdtts_griffinlim_opts o;
    check(xdtts_griffinlim_get_opts(g_, &o));
    return o;
  }
  // The rate of every delivered utterance (xdtts_griffinlim_set_output_rate): 22050 (default, nothing runs) or a supported rate
  // in 8 .. 96 kHz -- a polyphase resampler on the device behind the loop, in front of the output normalisation.  Hand the same
  // rate to write_wav.
  void set_output_rate(int32_t rate) { check(xdtts_griffinlim_set_output_rate(g_, rate)); }
  int32_t output_rate() const {
    int32_t rate = 0;
    check(xdtts_griffinlim_get_output_rate(g_, &rate));
    return rate;
  }
  // ... the stage alone (parity hook, xdtts_griffinlim_resample): audio at 22 050 Hz -> rate_out, whatever the handle's rate
  std::vector<float> resample(const std::vector<float> &audio, int32_t rate_out) const {
    size_t n = 0;
    check(xdtts_resample_plan(rate_out, audio.size(), nullptr, nullptr, nullptr, &n));
    std::vector<float> out(n ? n : 1);
    check(xdtts_griffinlim_resample(g_, audio.data(), audio.size(), rate_out, out.data(), &n));
    out.resize(n);
    return out;
  }
  // ... and the ragged form (xdtts_griffinlim_resample_batch): one launch, the single hook's bits per utterance
  std::vector<std::vector<float>> resample_batch(const std::vector<std::vector<float>> &audios, int32_t rate_out) const {
    const size_t n = audios.size();
    std::vector<std::vector<float>> out(n);
    std::vector<const float *> ip(n);
    std::vector<float *> op(n);
    std::vector<size_t> ns(n), no(n, 0);
    for (size_t u = 0; u < n; ++u) {
      check(xdtts_resample_plan(rate_out, audios[u].size(), nullptr, nullptr, nullptr, &no[u]));
      out[u].resize(no[u] ? no[u] : 1);
      ip[u] = audios[u].data();
      op[u] = out[u].data();
      ns[u] = audios[u].size();
    }
    check(xdtts_griffinlim_resample_batch(g_, ip.data(), ns.data(), (int32_t)n, rate_out, op.data(), no.data()));
    for (size_t u = 0; u < n; ++u) out[u].resize(no[u]);
    return out;
  }
  // The level rule of every delivered utterance (xdtts_griffinlim_set_loudness): a BS.1770 target in LUFS under a true-peak
  // ceiling in dBTP, NaN = off / none; when on it takes the output normalisation's place, at the delivered rate.
  void set_loudness(float target_lufs, float ceiling_dbtp) { check(xdtts_griffinlim_set_loudness(g_, target_lufs, ceiling_dbtp)); }
  std::pair<float, float> loudness_setting() const {
    float t = 0.f, c = 0.f;
    check(xdtts_griffinlim_get_loudness(g_, &t, &c));
    return {t, c};
  }
  // ... the measurement and applied gain of each utterance of the last delivering call (empty without a target)
  std::vector<xdtts_loudness> last_loudness() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_loudness(g_, nullptr, 0, &n));
    std::vector<xdtts_loudness> out(n);
    if (n) check(xdtts_griffinlim_last_loudness(g_, out.data(), out.size(), &n));
    return out;
  }
  // ... and the measurement alone on the caller's audio at `rate` (xdtts_griffinlim_loudness): gain 1, nothing scaled
  xdtts_loudness loudness(const std::vector<float> &audio, int32_t rate) const {
    xdtts_loudness l{};
    check(xdtts_griffinlim_loudness(g_, audio.data(), audio.size(), rate, &l));
    return l;
  }
  // A look-ahead true-peak limiter beside the target and the ceiling (xdtts_griffinlim_set_limiter): 500 .. 10000 microseconds,
  // 0 = off.  The gain is then formed without the ceiling and the limiter keeps it around the peaks only.
  void set_limiter(int32_t lookahead_us) { check(xdtts_griffinlim_set_limiter(g_, lookahead_us)); }
  int32_t limiter_setting() const {
    int32_t us = 0;
    check(xdtts_griffinlim_get_limiter(g_, &us));
    return us;
  }
  // ... the stats of each utterance of the last delivering call (empty unless a target, a ceiling and a limiter are set)
  std::vector<xdtts_limiter_stats> last_limiter() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_limiter(g_, nullptr, 0, &n));
    std::vector<xdtts_limiter_stats> out(n);
    if (n) check(xdtts_griffinlim_last_limiter(g_, out.data(), out.size(), &n));
    return out;
  }
  // ... and the stage alone on the caller's audio (xdtts_griffinlim_limit): always engaged, the bits of xdtts_limiter_reference
  std::vector<float> limit(const std::vector<float> &audio, int32_t rate, double gain0, double ceiling_lin, int32_t lookahead_us,
                           xdtts_limiter_stats *stats = nullptr) const {
    std::vector<float> out(audio.size());
    xdtts_limiter_stats st{};
    check(xdtts_griffinlim_limit(g_, audio.data(), audio.size(), rate, gain0, ceiling_lin, lookahead_us, out.data(), &st));
    if (stats) *stats = st;
    return out;
  }
  // A dynamic range compressor in front of the level stage (xdtts_griffinlim_set_compressor): nullptr = off, the default;
  // compressor_preset(1) is "drc".  It runs behind the output rate and in front of the normalisation / loudness target / limiter.
  static xdtts_compressor compressor_preset(int32_t which) {
    xdtts_compressor c{};
    check(xdtts_compressor_preset(which, &c));
    return c;
  }
  void set_compressor(const xdtts_compressor *c) { check(xdtts_griffinlim_set_compressor(g_, c)); }
  // ... the setting, and whether the stage is on
  bool compressor_setting(xdtts_compressor *c) const {
    int32_t on = 0;
    check(xdtts_griffinlim_get_compressor(g_, c, &on));
    return on != 0;
  }
  // ... the stats of each utterance of the last delivering call (empty unless a compressor other than the identity is set)
  std::vector<xdtts_compressor_stats> last_compressor() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_compressor(g_, nullptr, 0, &n));
    std::vector<xdtts_compressor_stats> out(n);
    if (n) check(xdtts_griffinlim_last_compressor(g_, out.data(), out.size(), &n));
    return out;
  }
  // ... and the stage alone on the caller's audio (xdtts_griffinlim_compress): the bits of xdtts_compressor_reference
  std::vector<float> compress(const std::vector<float> &audio, int32_t rate, const xdtts_compressor &c,
                              xdtts_compressor_stats *stats = nullptr) const {
    std::vector<float> out(audio.size());
    xdtts_compressor_stats st{};
    check(xdtts_griffinlim_compress(g_, audio.data(), audio.size(), rate, &c, out.data(), &st));
    if (stats) *stats = st;
    return out;
  }
  // Pause control (xdtts_griffinlim_set_silence): nullptr = off, the default.  The last stage of the delivery chain: edge silence
  // trimmed to lead_ms / trail_ms, pauses capped at max_pause_ms; every delivering entry then returns n_out samples.
  static xdtts_silence default_silence() {
    xdtts_silence s{};
    xdtts_silence_default(&s);
    return s;
  }
  void set_silence(const xdtts_silence *s) { check(xdtts_griffinlim_set_silence(g_, s)); }
  // ... the setting, and whether the stage is on
  bool silence_setting(xdtts_silence *s) const {
    int32_t on = 0;
    check(xdtts_griffinlim_get_silence(g_, s, &on));
    return on != 0;
  }
  // ... the stats of each utterance of the last delivering call (empty unless the stage is set)
  std::vector<xdtts_silence_stats> last_silence() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_silence(g_, nullptr, 0, &n));
    std::vector<xdtts_silence_stats> out(n);
    if (n) check(xdtts_griffinlim_last_silence(g_, out.data(), out.size(), &n));
    return out;
  }
  // ... and the stage alone on the caller's audio (xdtts_griffinlim_trim): the n_out samples, the bits of xdtts_silence_reference
  std::vector<float> trim(const std::vector<float> &audio, int32_t rate, const xdtts_silence &s, xdtts_silence_stats *stats = nullptr) const {
    std::vector<float> out(audio.size());
    xdtts_silence_stats st{};
    check(xdtts_griffinlim_trim(g_, audio.data(), audio.size(), rate, &s, out.data(), &st));
    out.resize(st.n_out);
    if (stats) *stats = st;
    return out;
  }
  // The voice of this handle (xdtts_griffinlim_set_timbre): vocal-tract length and breathiness on the magnitude behind the prosody
  // stage.  The default is the identity, which launches nothing; every entry that runs mel -> linear itself honours the setting.
  static xdtts_timbre default_timbre() {
    xdtts_timbre t{};
    xdtts_timbre_default(&t);
    return t;
  }
  void set_timbre(const xdtts_timbre &t) { check(xdtts_griffinlim_set_timbre(g_, &t)); }
  void clear_timbre() { check(xdtts_griffinlim_set_timbre(g_, nullptr)); }
  xdtts_timbre timbre_setting() const {
    xdtts_timbre t{};
    check(xdtts_griffinlim_get_timbre(g_, &t));
    return t;
  }
  // ... and the stage alone on the caller's magnitude (xdtts_griffinlim_timbre_linear), whatever the setting: S (n_bins x F) -> S'
  Array2 timbre_linear(const Array2 &S, const xdtts_timbre &t) const {
    Array2 out{S.rows, S.cols, std::vector<float>(S.data.size())};
    check(xdtts_griffinlim_timbre_linear(g_, S.data.data(), S.cols, &t, out.data.data()));
    return out;
  }
  // ... for several magnitudes in one launch, one setting each (xdtts_griffinlim_timbre_linear_batch): the single call's bits
  std::vector<Array2> timbre_linear_batch(const std::vector<Array2> &S, const std::vector<xdtts_timbre> &t) const {
    const size_t n = S.size();
    if (t.size() != n) throw std::runtime_error("xdtts: one timbre per utterance");
    std::vector<Array2> out(n);
    std::vector<const float *> in(n);
    std::vector<float *> op(n);
    std::vector<size_t> nf(n);
    for (size_t u = 0; u < n; ++u) {
      out[u] = Array2{S[u].rows, S[u].cols, std::vector<float>(S[u].data.size())};
      in[u] = S[u].data.data();
      op[u] = out[u].data.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_timbre_linear_batch(g_, in.data(), nf.data(), (int32_t)n, t.data(), op.data()));
    return out;
  }
  // The clean-up stage of this handle (xdtts_griffinlim_set_denoise): spectral subtraction with a floor and a tone curve on the
  // magnitude as mel -> linear left it, in front of every other stage.  The default is the identity, which launches nothing;
  // every entry that runs mel -> linear itself honours the setting.  profile: n_bins floats (e.g. noise_profile() of a silent
  // utterance of the checkpoint), or empty = none.
  static xdtts_denoise default_denoise() {
    xdtts_denoise d{};
    xdtts_denoise_default(&d);
    return d;
  }
  void set_denoise(const xdtts_denoise &d, const std::vector<float> &profile = {}) {
    if (!profile.empty() && profile.size() != 513) throw std::runtime_error("xdtts: a noise profile has 513 bins");
    check(xdtts_griffinlim_set_denoise(g_, &d, profile.empty() ? nullptr : profile.data()));
  }
  void clear_denoise() { check(xdtts_griffinlim_set_denoise(g_, nullptr, nullptr)); }
  xdtts_denoise denoise_setting(std::vector<float> *profile = nullptr) const {
    xdtts_denoise d{};
    std::vector<float> p(513);
    int32_t profiled = 0;
    check(xdtts_griffinlim_get_denoise(g_, &d, p.data(), &profiled));
    if (profile) *profile = profiled ? p : std::vector<float>();
    return d;
  }
  std::vector<xdtts_denoise_stats> last_denoise() const {
    size_t n = 0;
    check(xdtts_griffinlim_last_denoise(g_, nullptr, 0, &n));
    std::vector<xdtts_denoise_stats> out(n);
    if (n) check(xdtts_griffinlim_last_denoise(g_, out.data(), n, &n));
    return out;
  }
  // ... the stage alone on the caller's magnitude (xdtts_griffinlim_denoise_linear), whatever the setting: S (n_bins x F) -> S'
  Array2 denoise_linear(const Array2 &S, const xdtts_denoise &d, const std::vector<float> &profile = {}) const {
    Array2 out{S.rows, S.cols, std::vector<float>(S.data.size())};
    check(xdtts_griffinlim_denoise_linear(g_, S.data.data(), S.cols, &d, profile.empty() ? nullptr : profile.data(), out.data.data()));
    return out;
  }
  // ... for several magnitudes, one setting each and one shared profile (xdtts_griffinlim_denoise_linear_batch): the single call's bits
  std::vector<Array2> denoise_linear_batch(const std::vector<Array2> &S, const std::vector<xdtts_denoise> &d, const std::vector<float> &profile = {}) const {
    const size_t n = S.size();
    if (d.size() != n) throw std::runtime_error("xdtts: one denoise setting per utterance");
    std::vector<Array2> out(n);
    std::vector<const float *> in(n);
    std::vector<float *> op(n);
    std::vector<size_t> nf(n);
    for (size_t u = 0; u < n; ++u) {
      out[u] = Array2{S[u].rows, S[u].cols, std::vector<float>(S[u].data.size())};
      in[u] = S[u].data.data();
      op[u] = out[u].data.data();
      nf[u] = S[u].cols;
    }
    check(xdtts_griffinlim_denoise_linear_batch(g_, in.data(), nf.data(), (int32_t)n, d.data(), profile.empty() ? nullptr : profile.data(), op.data()));
    return out;
  }
  // ... and the selection alone (xdtts_griffinlim_noise_profile): per bin the order statistic `quantile` over S's frames
  std::vector<float> noise_profile(const Array2 &S, float quantile = 0.5f) const {
    std::vector<float> out(513);
    check(xdtts_griffinlim_noise_profile(g_, S.data.data(), S.cols, quantile, out.data()));
    return out;
  }
  // The inverse direction (xdtts_griffinlim_analyze): audio -> (S (n_bins x F), mel (n_mels x F)) under the handle's conventions,
  // F = audio.size() / 256 + 1
  std::pair<Array2, Array2> analyze(const std::vector<float> &audio, float mel_floor = 1e-5f) const {
    const size_t F = xdtts_griffinlim_analysis_frames(g_, audio.size());
    Array2 S{n_bins_, F, std::vector<float>(n_bins_ * F)}, mel{n_mels_, F, std::vector<float>(n_mels_ * F)};
    check(xdtts_griffinlim_analyze(g_, audio.data(), audio.size(), mel_floor, S.data.data(), mel.data.data(), nullptr));
    return {std::move(S), std::move(mel)};
  }
  // ... for several audios in one call (xdtts_griffinlim_analyze_batch): the single call's bits per utterance
  std::vector<std::pair<Array2, Array2>> analyze_batch(const std::vector<std::vector<float>> &audios, float mel_floor = 1e-5f) const {
    const size_t n = audios.size();
    std::vector<std::pair<Array2, Array2>> out(n);
    std::vector<const float *> ys(n);
    std::vector<size_t> ns(n), nf(n);
    std::vector<float *> Sp(n), Mp(n);
    for (size_t u = 0; u < n; ++u) {
      const size_t F = xdtts_griffinlim_analysis_frames(g_, audios[u].size());
      out[u].first = Array2{n_bins_, F, std::vector<float>(n_bins_ * F)};
      out[u].second = Array2{n_mels_, F, std::vector<float>(n_mels_ * F)};
      ys[u] = audios[u].data();
      ns[u] = audios[u].size();
      Sp[u] = out[u].first.data.data();
      Mp[u] = out[u].second.data.data();
    }
    check(xdtts_griffinlim_analyze_batch(g_, ys.data(), ns.data(), (int32_t)n, mel_floor, Sp.data(), Mp.data(), nf.data()));
    return out;
  }
  // (|| a |STFT(audio)| - S || / || S ||, a): how far `audio` is from the target magnitude S (n_bins x F)
  std::pair<float, float> spectral_convergence(const std::vector<float> &audio, const Array2 &S, bool fit_gain = false) const {
    float out[2] = {0.f, 0.f};
    check(xdtts_griffinlim_spectral_convergence(g_, audio.data(), audio.size(), S.data.data(), S.cols, fit_gain ? 1 : 0, out));
    return {out[0], out[1]};
  }
  std::array<float, 3> analysis_timings() const {  // ms: transform + magnitude, projection / distance, total
    std::array<float, 3> ms{};
    check(xdtts_griffinlim_analysis_timings(g_, ms.data()));
    return ms;
  }
  xdtts_griffinlim *raw() const { return g_; }

 private:
  xdtts_griffinlim *g_ = nullptr;
  size_t n_mels_ = 0, n_bins_ = 0;  // the basis' shape: the sizes of the analysis outputs
};

// src/tacotron2/mod.rs:441-458
inline GriffinLim create_griffin_lim(int device_id = XDTTS_DEVICE_DEFAULT) {
  const Array2 mel_basis = create_mel_filter_bank(22050.0f, 1024, 80, 0.0f, 8000.0f);
  return GriffinLim(mel_basis, 1024 - 256, 1.7f, 30, 0.99f, device_id);
}

// The output-rate stage's host arithmetic (xdtts_resample_plan, xdtts_resample_filter): no handle, no device.
struct ResamplePlan {
  int32_t L = 1, M = 1, half_len = 0;
  size_t n_out = 0;
};
inline ResamplePlan resample_plan(int32_t rate_out, size_t n_in = 0) {
  ResamplePlan p;
  check(xdtts_resample_plan(rate_out, n_in, &p.L, &p.M, &p.half_len, &p.n_out));
  return p;
}
inline std::vector<float> resample_filter(int32_t rate_out) {  // the library's own fp32 taps h[-H .. H]
  size_t n = 0;
  check(xdtts_resample_filter(rate_out, nullptr, 0, &n));
  std::vector<float> taps(n);
  check(xdtts_resample_filter(rate_out, taps.data(), taps.size(), &n));
  return taps;
}

inline xdtts_prosody default_prosody() {  // rate 1, pitch 1, lifter 30, log_floor 1e-5: the identity
  xdtts_prosody p;
  xdtts_prosody_default(&p);
  return p;
}

// A contour that owns its points (xdtts_prosody_contour borrows them): rate, pitch and gain that vary inside an utterance, what
// nested SSML <prosody> spans and contour="(0%,+20%) (40%,-10%)" attributes map to.
struct ProsodyContour {
  std::vector<xdtts_prosody_point> points;  // (pos, rate, pitch, gain), pos in [0, 1] non-decreasing
  int32_t lifter = 30;
  float log_floor = 1e-5f;
  xdtts_prosody_contour c() const {  // valid while this object lives and its points are not resized
    xdtts_prosody_contour o;
    xdtts_prosody_contour_default(&o);
    o.points = points.data();
    o.n_points = (int32_t)points.size();
    o.lifter = lifter;
    o.log_floor = log_floor;
    return o;
  }
  size_t frames(size_t n_frames) const {  // F' (xdtts_prosody_contour_frames); 0 for a bad argument
    const xdtts_prosody_contour o = c();
    return xdtts_prosody_contour_frames(&o, n_frames);
  }
  // The frame table the device reads (xdtts_prosody_contour_table): cumulative slowness c, pitch and gain per input frame
  void table(size_t n_frames, std::vector<uint32_t> &cum, std::vector<float> &pitch, std::vector<float> &gain) const {
    const xdtts_prosody_contour o = c();
    cum.assign(n_frames, 0);
    pitch.assign(n_frames, 0.f);
    gain.assign(n_frames, 0.f);
    check(xdtts_prosody_contour_table(&o, n_frames, cum.data(), pitch.data(), gain.data()));
  }
};

// XdTts::infer (src/lib.rs:110-159) for one utterance with a prosody -- what an SSML <prosody rate=".." pitch=".."> element asks
// for (src/text_normaliser.rs:41-56): units -> ids -> find_splits -> mel-gen -> vocoder with the rate / pitch stage
// (xdtts_synthesize_ids_prosody).  Returns (Tacotron2's own mel, the modified audio).
inline std::pair<Array2, std::vector<float>> infer_prosody(const Tacotron2 &model, const GriffinLim &vocoder, const std::vector<Unit> &units,
                                                            const xdtts_prosody &prosody, const xdtts_infer_opts *opts = nullptr) {
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  std::vector<int64_t> ids;
  for (const Unit &u : units) {
    const int64_t id = xdtts_unit_id(u.token.c_str(), u.is_character ? 1 : 0);
    if (id >= 0) ids.push_back(id);
  }
  std::vector<size_t> splits(ids.size() + 2);
  size_t n_splits = 0;
  check(xdtts_find_splits(ids.data(), ids.size(), (size_t)o.max_chunk, splits.data(), splits.size(), &n_splits));
  float *mel = nullptr, *audio = nullptr;
  size_t nf = 0, ns = 0;
  check(xdtts_synthesize_ids_prosody(model.raw(), vocoder.raw(), ids.data(), ids.size(), splits.data(), n_splits, &o, &prosody, &mel, &nf, &audio, &ns));
  std::pair<Array2, std::vector<float>> out;
  out.first.rows = 80;
  out.first.cols = nf;
  out.first.data.assign(mel, mel + 80 * nf);
  out.second.assign(audio, audio + ns);
  xdtts_free(mel);
  xdtts_free(audio);
  return out;
}

// ... and with a contour (xdtts_synthesize_ids_contour): one sentence synthesised whole, its <prosody> spans applied inside it.
inline std::pair<Array2, std::vector<float>> infer_contour(const Tacotron2 &model, const GriffinLim &vocoder, const std::vector<Unit> &units,
                                                            const ProsodyContour &contour, const xdtts_infer_opts *opts = nullptr,
                                                            bool at_ids = false) {  // at_ids: pos in ids (xdtts_synthesize_ids_contour_at_ids)
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  std::vector<int64_t> ids;
  for (const Unit &u : units) {
    const int64_t id = xdtts_unit_id(u.token.c_str(), u.is_character ? 1 : 0);
    if (id >= 0) ids.push_back(id);
  }
  std::vector<size_t> splits(ids.size() + 2);
  size_t n_splits = 0;
  check(xdtts_find_splits(ids.data(), ids.size(), (size_t)o.max_chunk, splits.data(), splits.size(), &n_splits));
  float *mel = nullptr, *audio = nullptr;
  size_t nf = 0, ns = 0;
  const xdtts_prosody_contour c = contour.c();
  check((at_ids ? xdtts_synthesize_ids_contour_at_ids : xdtts_synthesize_ids_contour)(model.raw(), vocoder.raw(), ids.data(), ids.size(), splits.data(),
                                                                                     n_splits, &o, &c, &mel, &nf, &audio, &ns));
  std::pair<Array2, std::vector<float>> out;
  out.first.rows = 80;
  out.first.cols = nf;
  out.first.data.assign(mel, mel + 80 * nf);
  out.second.assign(audio, audio + ns);
  xdtts_free(mel);
  xdtts_free(audio);
  return out;
}

// ... and with a pitch target (xdtts_synthesize_ids_pitch_target): the utterance's own F0 is tracked on the device and its median
// moved to an absolute pitch and / or its range scaled; contour: null or a contour to combine with; f0: null = the default options.
inline xdtts_f0_opts f0_opts_default() {
  xdtts_f0_opts o;
  xdtts_f0_opts_default(&o);
  return o;
}
inline xdtts_pitch_target pitch_target_default() {
  xdtts_pitch_target t;
  xdtts_pitch_target_default(&t);
  return t;
}
inline std::pair<int, int> f0_plan(const xdtts_f0_opts *o = nullptr) {  // (q_lo, q_hi) -- xdtts_f0_plan
  int32_t lo = 0, hi = 0;
  check(xdtts_f0_plan(o, &lo, &hi));
  return {lo, hi};
}
// The utterance stage on the host (xdtts_f0_track_reference): raw / strength -> (f0, ratio), stats if wanted
inline std::pair<std::vector<float>, std::vector<float>> f0_track_reference(const std::vector<float> &raw, const std::vector<float> &strength,
                                                                             const xdtts_pitch_target *t = nullptr, const xdtts_f0_opts *o = nullptr,
                                                                             xdtts_f0_stats *stats = nullptr) {
  if (raw.size() != strength.size()) throw std::runtime_error("xdtts: raw and strength have one length");
  std::pair<std::vector<float>, std::vector<float>> out{std::vector<float>(raw.size()), std::vector<float>(raw.size())};
  check(xdtts_f0_track_reference(raw.data(), strength.data(), raw.size(), o, t, out.first.data(), out.second.data(), stats));
  return out;
}
inline std::pair<Array2, std::vector<float>> infer_pitch_target(const Tacotron2 &model, const GriffinLim &vocoder, const std::vector<Unit> &units,
                                                                 const xdtts_pitch_target &target, const ProsodyContour *contour = nullptr,
                                                                 const xdtts_f0_opts *f0 = nullptr, const xdtts_infer_opts *opts = nullptr) {
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  std::vector<int64_t> ids;
  for (const Unit &u : units) {
    const int64_t id = xdtts_unit_id(u.token.c_str(), u.is_character ? 1 : 0);
    if (id >= 0) ids.push_back(id);
  }
  std::vector<size_t> splits(ids.size() + 2);
  size_t n_splits = 0;
  check(xdtts_find_splits(ids.data(), ids.size(), (size_t)o.max_chunk, splits.data(), splits.size(), &n_splits));
  float *mel = nullptr, *audio = nullptr;
  size_t nf = 0, ns = 0;
  xdtts_prosody_contour c;
  if (contour) c = contour->c();
  check(xdtts_synthesize_ids_pitch_target(model.raw(), vocoder.raw(), ids.data(), ids.size(), splits.data(), n_splits, &o, f0, &target,
                                          contour ? &c : nullptr, &mel, &nf, &audio, &ns));
  std::pair<Array2, std::vector<float>> out;
  out.first.rows = 80;
  out.first.cols = nf;
  out.first.data.assign(mel, mel + 80 * nf);
  out.second.assign(audio, audio + ns);
  xdtts_free(mel);
  xdtts_free(audio);
  return out;
}

// XdTts::infer (src/lib.rs:110-159) for several utterances in one call (xdtts_synthesize_batch): units -> ids
// (units with no id are dropped, mod.rs:403-406), find_splits per utterance (mod.rs:399,412-414), all chunks in one
// lock-step batch, the mel kept in HBM between mel-gen and vocoder.  Returns (mel, audio) per utterance.
// (prosody: null, or one per text -- xdtts_synthesize_batch_prosody: the mels stay Tacotron2's own, the audios are the modified ones;
// contour: null, or one per text -- xdtts_synthesize_batch_contour; not both.  target: null, or one pitch target per text --
// xdtts_synthesize_batch_pitch_target, alone or with `contour`; f0: its tracker options, null = the default)
inline std::vector<std::pair<Array2, std::vector<float>>> infer_many(const Tacotron2 &model, const GriffinLim &vocoder,
                                                                       const std::vector<std::vector<Unit>> &texts,
                                                                       const xdtts_infer_opts *opts = nullptr,
                                                                       const std::vector<xdtts_prosody> *prosody = nullptr,
                                                                       const std::vector<ProsodyContour> *contour = nullptr,
                                                                       const std::vector<xdtts_pitch_target> *target = nullptr,
                                                                       const xdtts_f0_opts *f0 = nullptr,
                                                                       bool contour_at_ids = false) {  // the contours' pos in ids: xdtts_synthesize_batch_contour_at_ids
  if (contour_at_ids && (!contour || target)) throw std::runtime_error("xdtts: contour_at_ids goes with a contour per text and no pitch target");
  if (target && (target->size() != texts.size() || prosody)) throw std::runtime_error("xdtts: one pitch target per text, and no uniform prosody beside it");
  if (prosody && prosody->size() != texts.size()) throw std::runtime_error("xdtts: one prosody per text");
  if (contour && contour->size() != texts.size()) throw std::runtime_error("xdtts: one contour per text");
  if (prosody && contour) throw std::runtime_error("xdtts: a prosody or a contour per text, not both");
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  const size_t T = (size_t)o.max_chunk;
  std::vector<int64_t> ids;      // [B][T], zero-padded
  std::vector<int32_t> lens, utt_chunks;
  for (const std::vector<Unit> &units : texts) {
    std::vector<int64_t> u;
    for (const Unit &x : units) {
      const int64_t id = xdtts_unit_id(x.token.c_str(), x.is_character ? 1 : 0);
      if (id >= 0) u.push_back(id);
    }
    std::vector<size_t> splits(u.size() + 2);
    size_t n_splits = 0;
    check(xdtts_find_splits(u.data(), u.size(), T, splits.data(), splits.size(), &n_splits));
    splits.resize(n_splits);
    if (splits.empty() || splits.back() != u.size()) splits.push_back(u.size());  // the trailing split (mod.rs:412-414)
    int32_t n = 0;
    size_t a = 0;
    for (size_t e : splits) {
      if (e <= a) continue;
      if (e - a > T) throw std::runtime_error("xdtts: a chunk exceeds the encoder window");
      ids.resize(ids.size() + T, 0);
      std::copy(u.begin() + (long)a, u.begin() + (long)e, ids.end() - (long)T);
      lens.push_back((int32_t)(e - a));
      a = e;
      ++n;
    }
    utt_chunks.push_back(n);
  }
  const size_t n_utt = texts.size();
  std::vector<float *> mels(n_utt, nullptr), audios(n_utt, nullptr);
  std::vector<size_t> nf(n_utt, 0), ns(n_utt, 0);
  if (target) {
    std::vector<xdtts_prosody_contour> cs;
    std::vector<const xdtts_prosody_contour *> cp;
    if (contour) {
      for (const ProsodyContour &c : *contour) cs.push_back(c.c());
      for (const xdtts_prosody_contour &c : cs) cp.push_back(&c);
    }
    check(xdtts_synthesize_batch_pitch_target(model.raw(), vocoder.raw(), ids.data(), lens.data(), (int32_t)lens.size(), (int32_t)T, utt_chunks.data(),
                                              (int32_t)n_utt, &o, nullptr, f0, target->data(), contour ? cp.data() : nullptr, mels.data(), nf.data(),
                                              audios.data(), ns.data()));
  } else if (contour) {
    std::vector<xdtts_prosody_contour> cs;
    for (const ProsodyContour &c : *contour) cs.push_back(c.c());
    check((contour_at_ids ? xdtts_synthesize_batch_contour_at_ids : xdtts_synthesize_batch_contour)(
        model.raw(), vocoder.raw(), ids.data(), lens.data(), (int32_t)lens.size(), (int32_t)T, utt_chunks.data(), (int32_t)n_utt, &o, nullptr, cs.data(),
        mels.data(), nf.data(), audios.data(), ns.data()));
  } else if (prosody)
    check(xdtts_synthesize_batch_prosody(model.raw(), vocoder.raw(), ids.data(), lens.data(), (int32_t)lens.size(), (int32_t)T, utt_chunks.data(),
                                         (int32_t)n_utt, &o, nullptr, prosody->data(), mels.data(), nf.data(), audios.data(), ns.data()));
  else
    check(xdtts_synthesize_batch(model.raw(), vocoder.raw(), ids.data(), lens.data(), (int32_t)lens.size(), (int32_t)T, utt_chunks.data(),
                                 (int32_t)n_utt, &o, nullptr, mels.data(), nf.data(), audios.data(), ns.data()));
  std::vector<std::pair<Array2, std::vector<float>>> out(n_utt);
  for (size_t i = 0; i < n_utt; ++i) {
    out[i].first.rows = 80;
    out[i].first.cols = nf[i];
    out[i].first.data.assign(mels[i], mels[i] + 80 * nf[i]);
    out[i].second.assign(audios[i], audios[i] + ns[i]);
    xdtts_free(mels[i]);
    xdtts_free(audios[i]);
  }
  return out;
}

// XdTts::infer for a sequence of sentences, each decoded alone as the reference does (a loop over src/lib.rs:122-141), the vocoder
// of one overlapped with the encoder of the next (xdtts_synthesize_sequence): what `app` would call for a text of several sentences.
// (prosody: null, or one per sentence -- xdtts_synthesize_sequence_prosody: one SSML <prosody> span per element)
inline std::vector<std::pair<Array2, std::vector<float>>> infer_sequence(const Tacotron2 &model, const GriffinLim &vocoder,
                                                                           const std::vector<std::vector<Unit>> &texts,
                                                                           const xdtts_infer_opts *opts = nullptr,
                                                                           const std::vector<xdtts_prosody> *prosody = nullptr) {
  if (prosody && prosody->size() != texts.size()) throw std::runtime_error("xdtts: one prosody per sentence");
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  const size_t n_utt = texts.size();
  std::vector<std::vector<int64_t>> ids(n_utt);
  std::vector<std::vector<size_t>> splits(n_utt);
  std::vector<const int64_t *> ids_p(n_utt);
  std::vector<const size_t *> sp_p(n_utt);
  std::vector<size_t> n_ids(n_utt), n_sp(n_utt);
  for (size_t u = 0; u < n_utt; ++u) {
    for (const Unit &x : texts[u]) {
      const int64_t id = xdtts_unit_id(x.token.c_str(), x.is_character ? 1 : 0);
      if (id >= 0) ids[u].push_back(id);  // units with no id are dropped, mod.rs:403-406
    }
    splits[u].resize(ids[u].size() + 2);
    size_t n = 0;
    check(xdtts_find_splits(ids[u].data(), ids[u].size(), (size_t)o.max_chunk, splits[u].data(), splits[u].size(), &n));
    splits[u].resize(n);
    ids_p[u] = ids[u].data();
    n_ids[u] = ids[u].size();
    sp_p[u] = splits[u].data();
    n_sp[u] = n;
  }
  std::vector<float *> mels(n_utt, nullptr), audios(n_utt, nullptr);
  std::vector<size_t> nf(n_utt, 0), ns(n_utt, 0);
  if (prosody)
    check(xdtts_synthesize_sequence_prosody(model.raw(), vocoder.raw(), ids_p.data(), n_ids.data(), sp_p.data(), n_sp.data(), (int32_t)n_utt, &o,
                                            prosody->data(), mels.data(), nf.data(), audios.data(), ns.data()));
  else
    check(xdtts_synthesize_sequence(model.raw(), vocoder.raw(), ids_p.data(), n_ids.data(), sp_p.data(), n_sp.data(), (int32_t)n_utt, &o, mels.data(),
                                    nf.data(), audios.data(), ns.data()));
  std::vector<std::pair<Array2, std::vector<float>>> out(n_utt);
  for (size_t i = 0; i < n_utt; ++i) {
    out[i].first.rows = 80;
    out[i].first.cols = nf[i];
    out[i].first.data.assign(mels[i], mels[i] + 80 * nf[i]);
    out[i].second.assign(audios[i], audios[i] + ns[i]);
    xdtts_free(mels[i]);
    xdtts_free(audios[i]);
  }
  return out;
}

// XdTts::generate_audio (src/lib.rs:60-108): a text cut at its <break>s -- `pieces` one after the other, breaks[u] seconds of
// silence BEHIND piece u (src/lib.rs:162-176; breaks may be shorter than pieces: the rest is 0) -- as ONE stream in the sample
// format of `stream` (default PCM16, the reference's i16 writer), joined and encoded on the device (xdtts_synthesize_document).
// The bytes of the stream: int16 little endian for format 1, one byte a sample for G.711, float for format 0.
struct Document {
  std::vector<unsigned char> bytes;
  std::vector<size_t> offsets;  // of each piece, in samples
  size_t total = 0;             // samples
  xdtts_stream_opts opts;
  std::vector<Array2> mels;
};
inline Document generate_audio(const Tacotron2 &model, const GriffinLim &vocoder, const std::vector<std::vector<Unit>> &pieces,
                               const std::vector<double> &breaks = {}, const xdtts_stream_opts *stream = nullptr,
                               const xdtts_infer_opts *opts = nullptr, const std::vector<xdtts_prosody> *prosody = nullptr) {
  if (prosody && prosody->size() != pieces.size()) throw std::runtime_error("xdtts: one prosody per piece");
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  Document doc;
  xdtts_stream_opts_default(&doc.opts);
  if (stream) doc.opts = *stream;
  const size_t n_utt = pieces.size();
  std::vector<std::vector<int64_t>> ids(n_utt);
  std::vector<std::vector<size_t>> splits(n_utt);
  std::vector<const int64_t *> ids_p(n_utt);
  std::vector<const size_t *> sp_p(n_utt);
  std::vector<size_t> n_ids(n_utt), n_sp(n_utt), gaps(n_utt + 1, 0);
  int32_t rate = XDTTS_SAMPLE_RATE;
  check(xdtts_griffinlim_get_output_rate(vocoder.raw(), &rate));
  for (size_t u = 0; u < n_utt; ++u) {
    for (const Unit &x : pieces[u]) {
      const int64_t id = xdtts_unit_id(x.token.c_str(), x.is_character ? 1 : 0);
      if (id >= 0) ids[u].push_back(id);  // units with no id are dropped, mod.rs:403-406
    }
    splits[u].resize(ids[u].size() + 2);
    size_t n = 0;
    check(xdtts_find_splits(ids[u].data(), ids[u].size(), (size_t)o.max_chunk, splits[u].data(), splits[u].size(), &n));
    splits[u].resize(n);
    ids_p[u] = ids[u].data();
    n_ids[u] = ids[u].size();
    sp_p[u] = splits[u].data();
    n_sp[u] = n;
    if (u < breaks.size()) gaps[u + 1] = xdtts_silence_samples(breaks[u], (uint32_t)rate);
  }
  std::vector<float *> mels(n_utt, nullptr);
  std::vector<size_t> nf(n_utt, 0);
  doc.offsets.assign(n_utt, 0);
  void *out = nullptr;
  check(xdtts_synthesize_document(model.raw(), vocoder.raw(), ids_p.data(), n_ids.data(), sp_p.data(), n_sp.data(), (int32_t)n_utt, &o,
                                  prosody ? prosody->data() : nullptr, gaps.data(), &doc.opts, mels.data(), nf.data(), &out,
                                  doc.offsets.data(), &doc.total));
  const unsigned char *b = static_cast<const unsigned char *>(out);
  doc.bytes.assign(b, b + doc.total * xdtts_stream_sample_bytes(doc.opts.format));
  xdtts_free(out);
  doc.mels.resize(n_utt);
  for (size_t i = 0; i < n_utt; ++i) {
    doc.mels[i].rows = 80;
    doc.mels[i].cols = nf[i];
    doc.mels[i].data.assign(mels[i], mels[i] + 80 * nf[i]);
    xdtts_free(mels[i]);
  }
  return doc;
}

// XdTts::infer's output stage (src/lib.rs:145-157): RTF, `(sample * i16::MAX as f32) as i16`,
// mono 22050 Hz 16-bit WAV (WAV_SPEC, src/lib.rs:25-30).
inline std::vector<int16_t> to_i16(const std::vector<float> &audio) {
  std::vector<int16_t> pcm(audio.size());
  check(xdtts_audio_to_i16(audio.data(), audio.size(), pcm.data()));
  return pcm;
}
inline void write_wav(const std::string &path, const std::vector<float> &audio) {
  const std::vector<int16_t> pcm = to_i16(audio);
  check(xdtts_wav_write(path.c_str(), pcm.data(), pcm.size(), XDTTS_SAMPLE_RATE));
}
inline void write_npy(const std::string &path, const Array2 &mel) {  // src/lib.rs:128-141
  check(xdtts_npy_write_f32(path.c_str(), mel.data.data(), mel.rows, mel.cols));
}

}  // namespace xdtts
