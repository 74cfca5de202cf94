// api_gl.h -- what the three files of the vocoder's extern "C" boundary (api_griffinlim.cpp, api_gl_magnitude.cpp,
// api_gl_delivery.cpp) share: the checks and the small copies every entry repeats.  Internal.
#pragma once
#include "env.h"
#include "griffinlim_handle.h"

namespace xdtts {

// A mel request against the handle's basis; with n_frames, a request that enters the loop (at least 2 frames)
inline void mel_check(const xdtts_griffinlim *g, size_t n_mels) {
  if ((int)n_mels != g->n_mels) fail(XDTTS_ERR_BAD_ARG, "mel has %zu rows, basis has %d", n_mels, g->n_mels);
}
inline void mel_check(const xdtts_griffinlim *g, size_t n_mels, size_t n_frames) {
  mel_check(g, n_mels);
  if (n_frames < 2) fail(XDTTS_ERR_BAD_ARG, "need at least 2 frames, got %zu", n_frames);
}

// The outputs of a batch entry before anything can fail (either array may be null: that is reported behind this)
inline void null_outputs(float **audios, size_t *n_samples, int n_utt) {
  for (int u = 0; u < n_utt; ++u) {
    if (audios) audios[u] = nullptr;
    if (n_samples) n_samples[u] = 0;
  }
}

// xdtts_griffinlim_last_f0 / _loudness / _limiter / _compressor: the count, and the structs where the buffer holds them
// (last: the handle's vector, or null with a null handle; tracked: the tracker's wording)
template <class T>
xdtts_status last_stats_out(const xdtts_griffinlim *g, const std::vector<T> *last, bool tracked, T *out, size_t cap, size_t *n) {
  return guard([&] {
    if (n) *n = 0;
    if (!g || !n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *n = last->size();
    if (!out && cap == 0) return;  // the count alone
    if (!out || cap < last->size())
      fail(XDTTS_ERR_BAD_ARG, tracked ? "the last call tracked %zu utterances, the buffer holds %zu" : "the last call delivered %zu utterances, the buffer holds %zu", last->size(), cap);
    if (!last->empty()) std::memcpy(out, last->data(), last->size() * sizeof(T));
  });
}

// A single mel request from the host: the handle's lock, the mel up, the one single-utterance request path
inline void infer_host_mel(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames, const MagnitudeRequest &req, float **audio, size_t *n_samples) {
  std::lock_guard<std::mutex> lk(g->mu);
  HIP_CHECK(hipSetDevice(g->device));
  g->mel_in.upload(mel, n_mels * n_frames, g->stream);
  HIP_CHECK(hipStreamSynchronize(g->stream));
  gl_run_from_device_mel(g, g->mel_in.p, (int)n_frames, req, audio, n_samples);
}

// A magnitude hook's result out: utterance u's rows of src [rows.total][nb] transposed into `frames` (the boundary layout,
// nb x F_u), ev.e[2], and copied to S_outs[u]; an utterance without an output is skipped.  bufs(>= rows.total) first.
inline void rows_to_host(xdtts_griffinlim *g, const float *src, const Rows &rows, float *const *S_outs) {
  const size_t nb = (size_t)g->nb;
  for (int u = 0; u < rows.n(); ++u) {
    if (!S_outs || !S_outs[u]) continue;
    const size_t r0 = (size_t)rows.row0[(size_t)u] * nb;
    launch_transpose(src + r0, g->frames.p + r0, rows.F[(size_t)u], g->nb, g->stream);
  }
  HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
  for (int u = 0; u < rows.n(); ++u) {
    if (!S_outs || !S_outs[u]) continue;
    const size_t r0 = (size_t)rows.row0[(size_t)u] * nb;
    HIP_CHECK(hipMemcpyAsync(S_outs[u], g->frames.p + r0, (size_t)rows.F[(size_t)u] * nb * sizeof(float), hipMemcpyDeviceToHost, g->stream));
  }
}

// GriffinLim::infer for several utterances at once (api_griffinlim.cpp).  ask: what the entry puts between mel -> linear and the
// loop, fields checked; each utterance is checked against its frame count here.
xdtts_status gl_infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels, const size_t *n_frames, int32_t n_utt,
                            const MagnitudeAsk &ask, float **audios, size_t *n_samples);

}  // namespace xdtts
