// api_synthesize.cpp -- the extern "C" boundary, both halves in one call: XdTts::infer for one utterance, a sequence, a batch.
#include <algorithm>
#include <cmath>

#include "griffinlim_handle.h"
#include "tacotron2_handle.h"

using namespace xdtts;

// ---- XdTts::infer (src/lib.rs:110-159) --------------------------------------------------------------

// The two handles of every xdtts_synthesize* entry, before a lock is taken or anything is enqueued: one device, and a vocoder
// whose basis has the model's N_MEL rows -- it reads the model's [N_MEL][F] mel where it lies in HBM as [n_mels][F] (fewer rows:
// wrong audio; more: a read past the buffer).
static void pair_check(const xdtts_tacotron2 *h, const xdtts_griffinlim *g) {
  if (h->device != g->device) fail(XDTTS_ERR_BAD_ARG, "tacotron2 and griffin-lim handles live on different devices");
  if (g->n_mels != N_MEL) fail(XDTTS_ERR_BAD_ARG, "the vocoder's basis has %d mel bands, the model's mel has %d", g->n_mels, N_MEL);
}

// ---- id-anchored contours (xdtts_synthesize_ids_contour_at_ids / _batch_contour_at_ids): a point's pos is in ids, 0 .. n ----
// The fields before a device is touched: a copy with pos / n is a contour in fractions, and the contour's own rules name the
// field and the point (dividing by n keeps the order of the points and maps [0, n] onto [0, 1]; NaN stays NaN).
static void contour_at_ids_check(const xdtts_prosody_contour *c, size_t n_ids, int u) {
  if (!c) fail(XDTTS_ERR_BAD_ARG, "null contour");
  if (n_ids == 0) fail(XDTTS_ERR_BAD_ARG, "empty id sequence");
  if (!c->points || c->n_points < 1 || c->n_points > 64) {  // (the contour's own message)
    if (u < 0) contour_check(c, 2); else contour_check_at(c, u, 2);
  }
  std::vector<xdtts_prosody_point> pts(c->points, c->points + c->n_points);
  const char *in_utt = u < 0 ? "" : "utterance ";
  char where[32] = "";
  if (u >= 0) std::snprintf(where, sizeof where, "%d: ", u);
  for (int k = 0; k < c->n_points; ++k) {  // pos in the words of this entry: ids
    const float pos = pts[(size_t)k].pos;
    if (!std::isfinite(pos) || pos < 0.0f || (double)pos > (double)n_ids)
      fail(XDTTS_ERR_BAD_ARG, "%s%scontour point %d: pos %g is not in [0, %zu] (ids)", in_utt, where, k, (double)pos, n_ids);
    if (k > 0 && pos < pts[(size_t)k - 1].pos)
      fail(XDTTS_ERR_BAD_ARG, "%s%scontour point %d: pos %g is below the point before it", in_utt, where, k, (double)pos);
  }
  for (xdtts_prosody_point &p : pts) p.pos = (float)((double)p.pos / (double)n_ids);
  xdtts_prosody_contour t = *c;
  t.points = pts.data();
  if (u < 0) contour_check(&t, 2); else contour_check_at(&t, u, 2);
}
// Behind the decode: the points of utterance u of the handle's capture mapped from ids to fractions of the utterance's F frames
// with durations_position, kept non-decreasing (at a chunk boundary the sum of a chunk's Q16 durations can pass the next chunk's
// base by a rounding: the running maximum), rounded to the fp32 pos of a point.
static void contour_at_ids_map(const xdtts_tacotron2 *h, size_t u, size_t F, const xdtts_prosody_contour &c, std::vector<xdtts_prosody_point> &out) {
  const DurUtt &U = h->dur_plan.utt[u];
  out.assign(c.points, c.points + c.n_points);
  double last = 0.0;
  for (xdtts_prosody_point &p : out) {
    const double pos = durations_position(h->dur_start() + U.id_off, h->dur_q16() + U.id_off, (size_t)U.n_ids, F, (double)p.pos);
    if (!(pos >= 0.0)) fail(XDTTS_ERR_BAD_ARG, "contour point at id position %g: outside the utterance's %d ids", (double)p.pos, (int)U.n_ids);
    last = pos > last ? pos : last;
    p.pos = (float)last;
  }
}

// (ask: nothing -- xdtts_synthesize_ids -- or the magnitude chain between mel -> linear and the loop, fields checked by the caller;
// at_ids: a contour whose pos are in ids -- the durations are captured whatever the setting says, the points mapped on the host
// once the capture has landed, and the contour machinery runs on the mapped contour)
static xdtts_status synthesize_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n, const size_t *splits,
                                   size_t n_splits, const xdtts_infer_opts *opts, const MagnitudeAsk &ask, float **mel, size_t *n_frames,
                                   float **audio, size_t *n_samples, const xdtts_prosody_contour *at_ids = nullptr) {
  return guard([&] {
    if (!h || !g || !mel || !n_frames || !audio || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    pair_check(h, g);
    *mel = nullptr;
    *audio = nullptr;
    *n_frames = *n_samples = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    std::lock_guard<std::mutex> lk2(g->mu);
    const xdtts_infer_opts o = resolve_opts(opts);
    std::vector<int64_t> padded;
    std::vector<int> lens;
    chunks_from_splits(ids, n, splits, n_splits, o.max_chunk, padded, lens);
    int total = 0;
    const std::vector<int> one_utt(lens.size(), 0);  // (durations: the chunks are one utterance)
    h->infer_batch_device(padded.data(), lens.data(), (int)lens.size(), o.max_chunk, o, nullptr, &total, false,
                          DurAsk{true, at_ids != nullptr, one_utt.data()});
    if (total < 2) fail(XDTTS_ERR_BAD_ARG, "mel has %d frame(s); the vocoder needs at least 2", total);
    std::vector<xdtts_prosody_point> mapped;
    xdtts_prosody_contour mapped_c{};
    if (at_ids) {
      h->wait_durations();  // (the capture's copy alone: the post-net may still be running)
      contour_at_ids_map(h, 0, (size_t)total, *at_ids, mapped);
      mapped_c = *at_ids;
      mapped_c.points = mapped.data();
    }
    const MagnitudeAsk ask_now = at_ids ? MagnitudeAsk::contour(&mapped_c) : ask;
    PinnedGuard mel_host((size_t)N_MEL * total);
    // the vocoder stream reads the mel behind the post-net (event 3 of infer_batch_device); the mel's copy to the host
    // follows on the mel-gen stream and overlaps the vocoder
    HIP_CHECK(hipStreamWaitEvent(g->stream, h->ev.e[3], 0));
    HIP_CHECK(hipMemcpyAsync(mel_host.p, h->mel_dev.p, (size_t)N_MEL * total * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    Drain drain(h->stream);  // the pinned buffer does not go back to the pool with the copy in flight
    const size_t total_frames = (size_t)total;  // (the frame count is known only now; nothing of the vocoder has been enqueued)
    gl_run_from_device_mel(g, h->mel_dev.p, total, magnitude_request(ask_now, 1, &total_frames), audio, n_samples);
    h->finish_timings();  // (stream sync: the mel has landed)
    h->publish_durations();
    *mel = mel_host.release();
    *n_frames = (size_t)total;
  });
}

// The outputs of a batch or sequence entry are cleared before its fields are checked, so that a rejected call returns nothing.
static void null_outputs(int32_t n_utt, float **mels, size_t *n_frames, float **audios, size_t *n_samples) {
  for (int u = 0; u < n_utt; ++u) {
    if (mels) mels[u] = nullptr;
    if (audios) audios[u] = nullptr;
    if (n_frames) n_frames[u] = 0;
    if (n_samples) n_samples[u] = 0;
  }
}
// The prosody array of the batch and sequence entries, before a handle is looked at
static xdtts_status check_prosody_array(const xdtts_prosody *p, int32_t n_utt, float **mels, size_t *n_frames, float **audios, size_t *n_samples) {
  return guard([&] {
    null_outputs(n_utt, mels, n_frames, audios, n_samples);
    prosody_check_array(p, n_utt);
  });
}

// XdTts::infer for a SEQUENCE of utterances, one after the other as the reference runs them (src/lib.rs:110-159: each utterance
// decoded alone, batch 1) -- but software-pipelined across the two halves: the frame loop owns every CU (weights in the register
// files), so nothing can run beside it; what can overlap is utterance u's vocoder (mel -> linear, Griffin-Lim, normalise: its own
// stream) with utterance u + 1's ENCODER (embedding, three convolutions, BiLSTM on 16 CUs, memory layer).  The frame loop of
// u + 1 is ordered behind the vocoder of u by an event (two grids that each want the chip co-resident never meet), and the host
// collects u's audio while u + 1 decodes.  Same bits as xdtts_synthesize_ids called once per utterance.
// (pros == null: xdtts_synthesize_sequence; else one prosody per utterance, fields checked by the caller: utterance u's vocoder
// half runs the single-utterance stage, the bits of xdtts_synthesize_ids_prosody)
// (doc: xdtts_synthesize_document -- the same run, but each utterance's delivered audio stays in HBM: doc->place() names its
// place in the handle's staging buffer in front of the vocoder's enqueue, audios[u] stays null, and doc->finish() runs the
// stream stage behind the last vocoder, under the locks of the run.)
struct DocRun {
  xdtts_griffinlim *g;
  StreamOpts o;
  const size_t *gaps;  // [n_utt + 1] or null
  int n_utt;
  size_t at = 0, src_at = 0;  // the stream position behind what has been placed; the floats of the staging buffer in use
  std::vector<size_t> off, n;
  PinnedGuard out;
  size_t total = 0;
  size_t gap(int u) const { return gaps ? gaps[u] : 0; }
  // utterance u (the next one) delivers N samples: its record, room in the staging buffer, the sink.  g->stream is idle.
  void place(int u, size_t N) {
    if (u == 0) {
      g->st_tab_host.clear();
      g->st_used = 0;
      at = gap(0);
    }
    if (at + N >= STREAM_TOTAL_MAX || at + N + gap(u + 1) >= STREAM_TOTAL_MAX)
      fail(XDTTS_ERR_BAD_ARG, "stream: utterance %d (%zu samples) and gaps[%d] take the stream to 2^28 samples or more", u, N, u + 1);
    const size_t src0 = ((src_at + 3) & ~(size_t)3) + (at & 3u);  // (an interior pack of the kernel then reads aligned 128 bits)
    g->stream_reserve(src0 + N + 4);
    g->st_tab_host.push_back(StreamUtt{(long long)src0, (uint32_t)at, (int32_t)N});
    off.push_back(at);
    n.push_back(N);
    src_at = src0 + N;
    g->st_used = src_at;
    at += N + gap(u + 1);
    g->sink.dst = g->st_src.p + src0;
    g->sink.unlevelled = o.level == 1;
  }
  // behind utterance u's collect, in front of the next place(): the silence stage decided on the device that u delivers
  // n_out <= N samples -- its record takes n_out, and the stream goes on behind them (the staging buffer keeps room for N)
  void trimmed(int u, size_t n_out) {
    if (n_out >= n[(size_t)u]) return;
    g->st_tab_host[(size_t)u].n = (int32_t)n_out;
    n[(size_t)u] = n_out;
    at = off[(size_t)u] + n_out + gap(u + 1);
  }
  // behind the last collect: the level-1 measurement if asked for, ONE k_stream_join launch, ONE copy to the host
  void finish() {
    g->sink = xdtts_griffinlim::StreamSink();
    total = at;
    if (total == 0) fail(XDTTS_ERR_BAD_ARG, "stream: total is 0 samples");
    const size_t bytes = total * (size_t)stream_sample_bytes(o.format);
    g->stream_join(total, o, g->dl.out_rate);
    out = PinnedGuard((bytes + 3) / 4);
    HIP_CHECK(hipMemcpyAsync(out.p, g->st_out.p, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_CHECK(hipStreamSynchronize(g->stream));
    if (o.level == 1) g->dl.push_last(0);
  }
};
static xdtts_status synthesize_sequence(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids, const size_t *n_ids,
                                        const size_t *const *splits, const size_t *n_splits, int32_t n_utt, const xdtts_infer_opts *opts,
                                        const xdtts_prosody *pros, float **mels, size_t *n_frames, float **audios, size_t *n_samples,
                                        DocRun *doc = nullptr) {
  return guard([&] {
    if (!h || !g || !ids || !n_ids || !n_frames || !audios || !n_samples || n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "null argument / no utterance");
    pair_check(h, g);
    for (int u = 0; u < n_utt; ++u) {
      audios[u] = nullptr;
      n_frames[u] = n_samples[u] = 0;
      if (mels) mels[u] = nullptr;
      if (!ids[u] || n_ids[u] == 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d is empty", u);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    std::lock_guard<std::mutex> lk2(g->mu);
    std::lock_guard<ChipLock> chip(chip_mutex(h->device));  // the whole sequence: co-resident launches of two streams are in flight
    g->clear_last();  // (gl_collect appends utterance by utterance)
    const MagnitudeAsk ask = pros ? MagnitudeAsk::prosody(pros) : MagnitudeAsk();
    const xdtts_infer_opts o = resolve_opts(opts);
    struct Hook {  // (the hook never outlives this call, whatever throws)
      xdtts_tacotron2 *h;
      xdtts_griffinlim *g;
      ~Hook() {
        h->before_decoder = nullptr;
        h->while_decoding = nullptr;
        g->sink = xdtts_griffinlim::StreamSink();
      }
    } unhook{h, g};
    if (doc && doc->o.level == 1 && !g->dl.loudness_on())
      fail(XDTTS_ERR_BAD_ARG, "stream: level 1 (programme) needs a loudness target on the handle");
    std::vector<PinnedGuard> mel_host(n_utt), audio_host(n_utt);
    std::vector<int> total(n_utt, 0);
    std::vector<float *> audio_out(n_utt, nullptr);
    // timing events per utterance (the post-net of u ends while the host is already enqueuing u + 1): utterance u records into a
    // fresh set, read when everything has drained; xdtts_*_last_timings then report the SUMS over the sequence
    std::vector<Events> per(n_utt);
    for (Events &e : per) e.create();
    // Declared BEHIND the pinned buffers and the event sets, i.e. destroyed BEFORE them: whatever throws (utterance u's chunking
    // fails while utterance u - 1's mel copy, vocoder and audio copy are still in flight), both streams drain first and only then
    // do the buffers go back to the shared pool and the events get destroyed.
    Drain drain(h->stream, g->stream);
    float gsum[3] = {0.f, 0.f, 0.f};
    int steps_sum = 0;
    auto add_gl = [&]() {
      for (int i = 0; i < 3; ++i) gsum[i] += g->last_ms[i];
    };
    auto release_all = [&]() {
      for (int u = 0; u < n_utt; ++u)
        if (audio_out[u]) pinned_release(audio_out[u]);
    };
    try {
      for (int u = 0; u < n_utt; ++u) {
        std::vector<int64_t> padded;
        std::vector<int> lens;
        chunks_from_splits(ids[u], n_ids[u], splits ? splits[u] : nullptr, (splits && n_splits) ? n_splits[u] : 0, o.max_chunk, padded, lens);
        if (u > 0) h->before_decoder = [&] { HIP_CHECK(hipStreamWaitEvent(h->stream, g->ev.e[2], 0)); };  // vocoder of u - 1 done (its audio copy is behind it on g->stream)
        // The pinned output buffers of utterance u are taken from the pool WHILE its frame loop runs (the host has 5.6 ms to wait there), not
        // between the vocoder's enqueue and the next encoder's: a pool miss is a hipHostMalloc of 0.8 MB -- 0.2-0.4 ms on some boxes -- and in
        // that place it made the next encoder start when the vocoder had finished instead of beside it (round 6: the sequence headline's two
        // modes, 6.15-6.25 / 6.5-6.6 ms per utterance; the kernel timeline of tools/sequence_timeline.sh shows k_embed behind k_gl_persistent
        // in the slow utterances).  Gate-less decodes only: the frame count is then known beforehand.
        long predicted = 0;
        if (o.fixed_steps > 0 || o.fixed_frames_per_id > 0.f)
          for (int len : lens) {
            const long l = o.fixed_steps > 0 ? o.fixed_steps : std::lround((double)o.fixed_frames_per_id * len);
            predicted += std::min<long>(std::max<long>(l, 1), o.max_steps);
          }
        h->while_decoding = nullptr;
        if (predicted >= 2)
          h->while_decoding = [&, u, predicted] {
            if (!mel_host[u].p) mel_host[u] = PinnedGuard((size_t)N_MEL * predicted);
            const size_t Fp = (size_t)magnitude_request(ask.at(u), 1, nullptr).frames(0, (int)predicted);  // the vocoder's frames, not the mel's
            if (!doc && !audio_host[u].p) audio_host[u] = PinnedGuard(g->dl.delivered((size_t)g->hop * (Fp - 1)));  // (at the handle's output rate)
          };
        for (int i = 0; i < 4; ++i) std::swap(h->ev.e[i], per[u].e[i]);  // (per[u] now holds what the handle had: utterance u - 1's set, or its own)
        h->infer_batch_device(padded.data(), lens.data(), (int)lens.size(), o.max_chunk, o, nullptr, &total[u]);
        h->before_decoder = nullptr;
        h->while_decoding = nullptr;
        if (predicted != total[u]) mel_host[u] = PinnedGuard(), audio_host[u] = PinnedGuard();  // (the stop rule decided otherwise: sized below)
        steps_sum += h->last_steps;
        if (total[u] < 2) fail(XDTTS_ERR_BAD_ARG, "utterance %d: mel has %d frame(s); the vocoder needs at least 2", u, total[u]);
        const size_t mel_frames = (size_t)total[u];
        const MagnitudeRequest req = magnitude_request(ask.at(u), 1, &mel_frames, u);  // (the frame count is known only now)
        // the frame loop of u has drained, and it waited for the vocoder of u - 1: collect that audio now
        if (u > 0) {
          gl_collect(g, audio_host[u - 1], &audio_out[u - 1], &n_samples[u - 1]);  // (the plan in place is still utterance u - 1's)
          if (doc) doc->trimmed(u - 1, n_samples[u - 1]);
          add_gl();
        }
        if (!mel_host[u].p) mel_host[u] = PinnedGuard((size_t)N_MEL * total[u]);
        HIP_CHECK(hipStreamWaitEvent(g->stream, h->ev.e[3], 0));  // the vocoder reads the mel behind the post-net
        HIP_CHECK(hipMemcpyAsync(mel_host[u].p, h->mel_dev.p, (size_t)N_MEL * total[u] * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (doc) doc->place(u, g->dl.delivered((size_t)g->hop * (size_t)(req.frames(0, total[u]) - 1)));
        gl_enqueue_from_device_mel(g, h->mel_dev.p, total[u], audio_host[u], req);
      }
      gl_collect(g, audio_host[n_utt - 1], &audio_out[n_utt - 1], &n_samples[n_utt - 1]);
      if (doc) doc->trimmed(n_utt - 1, n_samples[n_utt - 1]);
      add_gl();
      if (doc) doc->finish();
      h->finish_timings();  // (stream sync: every mel has landed; last_ms = the last utterance's phases)
      float hsum[4] = {h->last_ms[0], h->last_ms[1], h->last_ms[2], h->last_ms[3]};
      for (int u = 1; u < n_utt; ++u) {  // utterance u - 1's events sit in per[u]
        float ms = 0.f;
        for (int i = 0; i < 3; ++i) {
          HIP_CHECK(hipEventElapsedTime(&ms, per[u].e[i], per[u].e[i + 1]));
          hsum[i] += ms;
        }
        HIP_CHECK(hipEventElapsedTime(&ms, per[u].e[0], per[u].e[3]));
        hsum[3] += ms;
      }
      for (int i = 0; i < 4; ++i) h->last_ms[i] = hsum[i];
      for (int i = 0; i < 3; ++i) g->last_ms[i] = gsum[i];
      h->last_steps = steps_sum;
    } catch (...) {
      (void)hipStreamSynchronize(h->stream);  // (nothing in flight writes into a buffer that is handed back below)
      (void)hipStreamSynchronize(g->stream);
      release_all();
      throw;
    }
    for (int u = 0; u < n_utt; ++u) {
      audios[u] = audio_out[u];
      n_frames[u] = (size_t)total[u];
      if (mels) mels[u] = mel_host[u].release();
    }
  });
}

// XdTts::infer for several utterances in one call (BASELINE.json configs[3]; the author's "batched / parallel
// sentences" note, src/phonemes.rs:677-680): all chunks through one lock-step mel-gen batch (chunks are independent,
// src/tacotron2/mod.rs:422-434), the post-net writes every utterance's chunks side by side on the time axis
// (mod.rs:430), and the vocoder batch reads that mel where it lies in HBM -- no copy to the host and back, no
// re-staging between the two halves.  The per-utterance mels leave for the host while the vocoder runs.
// (ask: nothing -- xdtts_synthesize_batch -- or the magnitude chain's request per utterance, fields checked by the caller)
static xdtts_status synthesize_batch(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                     int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                     const int32_t *fixed_steps_per_item, const MagnitudeAsk &ask, float **mels, size_t *n_frames, float **audios,
                                     size_t *n_samples, const xdtts_prosody_contour *at_ids = nullptr) {
  return guard([&] {
    if (!h || !g || !ids || !lens || !utt_chunks || !n_frames || !audios || !n_samples) fail(XDTTS_ERR_BAD_ARG, "null argument");
    pair_check(h, g);
    if (B <= 0 || n_utt <= 0 || t_stride <= 0) fail(XDTTS_ERR_BAD_ARG, "batch %d / utterances %d / stride %d out of range", B, n_utt, t_stride);
    long nchunks = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (utt_chunks[u] <= 0) fail(XDTTS_ERR_BAD_ARG, "utterance %d has no chunk", u);
      nchunks += utt_chunks[u];
      audios[u] = nullptr;
      n_frames[u] = n_samples[u] = 0;
      if (mels) mels[u] = nullptr;
    }
    if (nchunks != B) fail(XDTTS_ERR_BAD_ARG, "utt_chunks sum to %ld, the batch has %d chunks", nchunks, B);
    std::lock_guard<std::mutex> lk(h->mu);
    std::lock_guard<std::mutex> lk2(g->mu);
    const xdtts_infer_opts o = resolve_opts(opts);
    const int T = o.max_chunk;
    const std::vector<int64_t> padded = pad_batch_ids(ids, lens, B, t_stride, T);
    int total = 0;
    std::vector<int> utt_of_chunk;  // (durations: utterance of every chunk)
    for (int u = 0; u < n_utt; ++u) utt_of_chunk.insert(utt_of_chunk.end(), (size_t)utt_chunks[u], u);
    const std::vector<int> F = h->infer_batch_device(padded.data(), lens, B, T, o, fixed_steps_per_item, &total, false,
                                                      DurAsk{true, at_ids != nullptr, utt_of_chunk.data()});
    std::vector<int> Fu(n_utt, 0), col0(n_utt, 0);
    for (int u = 0, b = 0, off = 0; u < n_utt; ++u) {
      col0[u] = off;
      for (int k = 0; k < utt_chunks[u]; ++k) Fu[u] += F[b++];
      off += Fu[u];
      if (Fu[u] < 2) fail(XDTTS_ERR_BAD_ARG, "utterance %d has %d mel frame(s); the vocoder needs at least 2", u, Fu[u]);
    }
    const std::vector<size_t> Fz(Fu.begin(), Fu.end());
    std::vector<std::vector<xdtts_prosody_point>> mapped;
    std::vector<xdtts_prosody_contour> mapped_c;
    if (at_ids) {
      h->wait_durations();  // (the capture's copy alone: the post-net may still be running)
      mapped.resize((size_t)n_utt);
      mapped_c.assign(at_ids, at_ids + n_utt);
      for (int u = 0; u < n_utt; ++u) {
        contour_at_ids_map(h, (size_t)u, Fz[(size_t)u], at_ids[u], mapped[(size_t)u]);
        mapped_c[(size_t)u].points = mapped[(size_t)u].data();
      }
    }
    const MagnitudeRequest req = magnitude_request(at_ids ? MagnitudeAsk::contour(mapped_c.data()) : ask, n_utt, Fz.data(), 0);  // (nothing of the vocoder has been enqueued)
    // the vocoder stream reads the mel behind the post-net (event 3 of infer_batch_device); the host copies of the
    // mel follow on the mel-gen stream and overlap the vocoder
    HIP_CHECK(hipStreamWaitEvent(g->stream, h->ev.e[3], 0));
    std::vector<PinnedGuard> mel_out;
    Drain drain(h->stream);  // no mel buffer goes back to the pool while a copy into it may be in flight
    if (mels) {
      mel_out.reserve((size_t)n_utt);
      for (int u = 0; u < n_utt; ++u) {
        mel_out.emplace_back((size_t)N_MEL * Fu[u]);
        HIP_CHECK(hipMemcpy2DAsync(mel_out[(size_t)u].p, sizeof(float) * (size_t)Fu[u], h->mel_dev.p + col0[u], sizeof(float) * (size_t)total,
                                   sizeof(float) * (size_t)Fu[u], N_MEL, hipMemcpyDeviceToHost, h->stream));
      }
    }
    gl_batch_from_device(g, h->mel_dev.p, Fu, audios, n_samples, req);
    try {
      h->finish_timings();  // (stream sync: the mel copies have landed)
    } catch (...) {  // the caller gets either every buffer of the call or none
      for (int u = 0; u < n_utt; ++u) {
        if (audios[u]) pinned_release(audios[u]);
        audios[u] = nullptr;
        n_samples[u] = 0;
      }
      throw;
    }
    h->publish_durations();
    for (int u = 0; u < n_utt; ++u) {
      n_frames[u] = (size_t)Fu[u];
      if (mels) mels[u] = mel_out[(size_t)u].release();
    }
  });
}

extern "C" {

xdtts_status xdtts_synthesize_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                  const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts, float **mel,
                                  size_t *n_frames, float **audio, size_t *n_samples) {
  return synthesize_ids(h, g, ids, n, splits, n_splits, opts, MagnitudeAsk(), mel, n_frames, audio, n_samples);
}

// ... with a prosody: the mel returned is Tacotron2's own, the audio has hop * (F' - 1) samples
xdtts_status xdtts_synthesize_ids_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                          const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts,
                                          const xdtts_prosody *p, float **mel, size_t *n_frames, float **audio,
                                          size_t *n_samples) {
  xdtts_status st = guard([&] {
    if (!p) fail(XDTTS_ERR_BAD_ARG, "null prosody");
    prosody_check(p, 2);  // the fields, before a device is touched
  });
  if (st != XDTTS_OK) return st;
  return synthesize_ids(h, g, ids, n, splits, n_splits, opts, MagnitudeAsk::prosody(p), mel, n_frames, audio, n_samples);
}

// ... with a contour (rate, pitch and gain that vary inside the utterance): the audio has hop * (F' - 1) samples, F' from the
// table, which is built once the frame count is known
xdtts_status xdtts_synthesize_ids_contour(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                          const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts,
                                          const xdtts_prosody_contour *c, float **mel, size_t *n_frames, float **audio,
                                          size_t *n_samples) {
  xdtts_status st = guard([&] { contour_check(c, 2); });  // the fields, before a device is touched
  if (st != XDTTS_OK) return st;
  return synthesize_ids(h, g, ids, n, splits, n_splits, opts, MagnitudeAsk::contour(c), mel, n_frames, audio, n_samples);
}

// ... with a contour whose points are anchored at ids: pos in [0, n], mapped through the durations of this very decode
xdtts_status xdtts_synthesize_ids_contour_at_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                                 const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts,
                                                 const xdtts_prosody_contour *c, float **mel, size_t *n_frames, float **audio,
                                                 size_t *n_samples) {
  xdtts_status st = guard([&] { contour_at_ids_check(c, ids ? n : 0, -1); });  // the fields, before a device is touched
  if (st != XDTTS_OK) return st;
  return synthesize_ids(h, g, ids, n, splits, n_splits, opts, MagnitudeAsk(), mel, n_frames, audio, n_samples, c);
}

xdtts_status xdtts_synthesize_sequence(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids, const size_t *n_ids,
                                       const size_t *const *splits, const size_t *n_splits, int32_t n_utt, const xdtts_infer_opts *opts,
                                       float **mels, size_t *n_frames, float **audios, size_t *n_samples) {
  return synthesize_sequence(h, g, ids, n_ids, splits, n_splits, n_utt, opts, nullptr, mels, n_frames, audios, n_samples);
}

// ... one prosody per utterance (what a text cut at its <break>s into pieces with their own <prosody> asks for): mels[u] is
// Tacotron2's own, audios[u] has hop * (xdtts_prosody_frames(n_frames[u], p[u].rate) - 1) samples
xdtts_status xdtts_synthesize_sequence_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids, const size_t *n_ids,
                                               const size_t *const *splits, const size_t *n_splits, int32_t n_utt,
                                               const xdtts_infer_opts *opts, const xdtts_prosody *p, float **mels, size_t *n_frames,
                                               float **audios, size_t *n_samples) {
  const xdtts_status st = check_prosody_array(p, n_utt, mels, n_frames, audios, n_samples);
  if (st != XDTTS_OK) return st;
  return synthesize_sequence(h, g, ids, n_ids, splits, n_splits, n_utt, opts, p, mels, n_frames, audios, n_samples);
}

// XdTts::generate_audio (src/lib.rs:60-108): the sequence, its audio kept in HBM, joined and encoded on the device
xdtts_status xdtts_synthesize_document(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids, const size_t *n_ids,
                                       const size_t *const *splits, const size_t *n_splits, int32_t n_utt, const xdtts_infer_opts *opts,
                                       const xdtts_prosody *p, const size_t *gaps, const xdtts_stream_opts *o, float **mels, size_t *n_frames,
                                       void **stream, size_t *offsets, size_t *total) {
  DocRun doc{};
  std::vector<float *> audios;
  std::vector<size_t> n_samples;
  xdtts_status st = guard([&] {  // the options, the count and the gaps: before a handle is looked at
    if (stream) *stream = nullptr;
    if (total) *total = 0;
    doc.o = stream_opts_checked(o);
    if (n_utt < 1 || n_utt > STREAM_UTT_MAX) fail(XDTTS_ERR_BAD_ARG, "stream: n_utt %d is not in [1, %d]", n_utt, STREAM_UTT_MAX);
    if (!stream || !total || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t sum = 0;
    for (int u = 0; gaps && u <= n_utt; ++u) {
      if (gaps[u] >= STREAM_TOTAL_MAX || sum + gaps[u] >= STREAM_TOTAL_MAX)
        fail(XDTTS_ERR_BAD_ARG, "stream: gaps[%d] = %zu takes the stream to 2^28 samples or more", u, gaps[u]);
      sum += gaps[u];
    }
    if (p) prosody_check_array(p, n_utt);
    for (int u = 0; u < n_utt; ++u) {
      if (mels) mels[u] = nullptr;
      n_frames[u] = 0;
    }
    audios.assign((size_t)n_utt, nullptr);
    n_samples.assign((size_t)n_utt, 0);
  });
  if (st != XDTTS_OK) return st;
  doc.g = g;
  doc.gaps = gaps;
  doc.n_utt = n_utt;
  st = synthesize_sequence(h, g, ids, n_ids, splits, n_splits, n_utt, opts, p, mels, n_frames, audios.data(), n_samples.data(), &doc);
  if (st != XDTTS_OK) return st;
  for (int u = 0; offsets && u < n_utt; ++u) offsets[u] = doc.off[(size_t)u];
  *total = doc.total;
  *stream = doc.out.release();
  return XDTTS_OK;
}

xdtts_status xdtts_synthesize_batch(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                    int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                    const int32_t *fixed_steps_per_item, float **mels, size_t *n_frames, float **audios,
                                    size_t *n_samples) {
  return synthesize_batch(h, g, ids, lens, B, t_stride, utt_chunks, n_utt, opts, fixed_steps_per_item, MagnitudeAsk(), mels, n_frames, audios, n_samples);
}

// ... one prosody per utterance: the ragged stage behind the batch's one mel -> linear GEMM
xdtts_status xdtts_synthesize_batch_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                            int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                            const int32_t *fixed_steps_per_item, const xdtts_prosody *p, float **mels, size_t *n_frames,
                                            float **audios, size_t *n_samples) {
  const xdtts_status st = check_prosody_array(p, n_utt, mels, n_frames, audios, n_samples);
  if (st != XDTTS_OK) return st;
  return synthesize_batch(h, g, ids, lens, B, t_stride, utt_chunks, n_utt, opts, fixed_steps_per_item, MagnitudeAsk::prosody(p), mels, n_frames, audios, n_samples);
}

// ... one contour per utterance: the ragged contour stage behind the batch's one mel -> linear GEMM
xdtts_status xdtts_synthesize_batch_contour(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                            int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                            const int32_t *fixed_steps_per_item, const xdtts_prosody_contour *c, float **mels, size_t *n_frames,
                                            float **audios, size_t *n_samples) {
  const xdtts_status st = guard([&] {
    null_outputs(n_utt, mels, n_frames, audios, n_samples);
    contour_check_array(c, n_utt);
  });
  if (st != XDTTS_OK) return st;
  return synthesize_batch(h, g, ids, lens, B, t_stride, utt_chunks, n_utt, opts, fixed_steps_per_item, MagnitudeAsk::contour(c), mels, n_frames, audios, n_samples);
}

// ... one id-anchored contour per utterance: pos in [0, the utterance's id count]
xdtts_status xdtts_synthesize_batch_contour_at_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                                   int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                                   const int32_t *fixed_steps_per_item, const xdtts_prosody_contour *c, float **mels, size_t *n_frames,
                                                   float **audios, size_t *n_samples) {
  xdtts_status st = guard([&] {
    null_outputs(n_utt, mels, n_frames, audios, n_samples);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!c) fail(XDTTS_ERR_BAD_ARG, "null contour array");
    if (!lens || !utt_chunks) fail(XDTTS_ERR_BAD_ARG, "null argument");
    // the fields against each utterance's id count, before a handle is looked at
    for (int u = 0, b = 0; u < n_utt; ++u) {
      size_t n_ids = 0;
      for (int k = 0; k < utt_chunks[u]; ++k, ++b) {
        if (b >= B) fail(XDTTS_ERR_BAD_ARG, "utt_chunks name more than the batch's %d chunks", B);
        n_ids += lens[b] > 0 ? (size_t)lens[b] : 0;
      }
      contour_at_ids_check(&c[u], n_ids, u);
    }
  });
  if (st != XDTTS_OK) return st;
  return synthesize_batch(h, g, ids, lens, B, t_stride, utt_chunks, n_utt, opts, fixed_steps_per_item, MagnitudeAsk(), mels, n_frames, audios, n_samples, c);
}

// ... with a pitch target (xdtts_pitch_target): tracker, target and contour stage behind mel -> linear; the table is built once
// the frame count is known
xdtts_status xdtts_synthesize_ids_pitch_target(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                               const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts,
                                               const xdtts_f0_opts *o, const xdtts_pitch_target *t, const xdtts_prosody_contour *c,
                                               float **mel, size_t *n_frames, float **audio, size_t *n_samples) {
  F0Job job;
  xdtts_status st = guard([&] {  // the fields, before a device is touched
    job = f0_job_checked(o);
    pitch_target_check_array(t, 1);
    if (c) contour_check(c, 2);
  });
  if (st != XDTTS_OK) return st;
  return synthesize_ids(h, g, ids, n, splits, n_splits, opts, MagnitudeAsk::target(&job, t, c ? &c : nullptr), mel, n_frames, audio, n_samples);
}

// ... one target per utterance, contours that may be null
xdtts_status xdtts_synthesize_batch_pitch_target(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, const int32_t *lens, int32_t B,
                                                 int32_t t_stride, const int32_t *utt_chunks, int32_t n_utt, const xdtts_infer_opts *opts,
                                                 const int32_t *fixed_steps_per_item, const xdtts_f0_opts *o, const xdtts_pitch_target *t,
                                                 const xdtts_prosody_contour *const *c, float **mels, size_t *n_frames, float **audios,
                                                 size_t *n_samples) {
  F0Job job;
  const xdtts_status st = guard([&] {
    null_outputs(n_utt, mels, n_frames, audios, n_samples);
    job = f0_job_checked(o);
    pitch_target_check_array(t, n_utt);
    for (int u = 0; c && u < n_utt; ++u)
      if (c[u]) contour_check_at(c[u], u, 2);
  });
  if (st != XDTTS_OK) return st;
  return synthesize_batch(h, g, ids, lens, B, t_stride, utt_chunks, n_utt, opts, fixed_steps_per_item, MagnitudeAsk::target(&job, t, c), mels, n_frames, audios, n_samples);
}

}  // extern "C"
