// api_tacotron2.cpp -- the extern "C" boundary of libxdtts_hip.so (declared in include/xdtts.h), mel-generator half and the
// entry points that belong to no handle.  Argument checks and locking; the work is in tacotron2_handle.cpp / tacotron2_decode.cpp.
// No CPU compute path exists: without a HIP device every entry point fails with XDTTS_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>
#include <memory>

#include "tacotron2_handle.h"

#include "edge_floor.hip"

using namespace xdtts;

extern "C" {

void xdtts_infer_opts_default(xdtts_infer_opts *o) {
  if (!o) return;
  o->gate_threshold = 0.6f;  // src/tacotron2/mod.rs:279
  o->max_steps = 1000;       // src/tacotron2/mod.rs:280
  o->fixed_steps = 0;
  o->dropout_mode = 1;
  o->dropout_seed = 0;
  o->max_chunk = 100;  // src/tacotron2/mod.rs:363,369-371,399
  o->item_base = 0;
  o->fixed_frames_per_id = 0.f;
  o->dropout_masks = nullptr;
  o->dropout_mask_steps = 0;
}

const char *xdtts_last_error(void) { return last_error(); }

int32_t xdtts_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void xdtts_free(void *p) {
  if (p) pinned_release(p);
}

int32_t xdtts_tensor_count(void) { return (int32_t)tensor_table().size(); }
const char *xdtts_tensor_name(int32_t i) {
  return i >= 0 && i < xdtts_tensor_count() ? tensor_table()[i].name : nullptr;
}
int32_t xdtts_tensor_ndim(int32_t i) { return i >= 0 && i < xdtts_tensor_count() ? tensor_table()[i].ndim : 0; }
int32_t xdtts_tensor_dim(int32_t i, int32_t d) {
  return i >= 0 && i < xdtts_tensor_count() && d >= 0 && d < 3 ? tensor_table()[i].dims[d] : 0;
}
size_t xdtts_tensor_offset(int32_t i) { return i >= 0 && i < xdtts_tensor_count() ? tensor_table()[i].offset : 0; }
size_t xdtts_tensor_total(void) { return tensor_total(); }

static xdtts_status make_handle(std::vector<float> &&blob, int32_t device_id, xdtts_tacotron2 **out) {
  return guard([&] {
    if (!out) fail(XDTTS_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    auto h = std::make_unique<xdtts_tacotron2>();
    h->blob = std::move(blob);
    h->init(device_id);
    *out = h.release();
  });
}

xdtts_status xdtts_tacotron2_load(const char *dir, int32_t device_id, xdtts_tacotron2 **out) {
  std::vector<float> blob;
  xdtts_status st = guard([&] {
    if (!dir) fail(XDTTS_ERR_BAD_ARG, "dir is null");
    device_id = select_device(device_id);
    load_model_dir(dir, blob);
  });
  if (st != XDTTS_OK) return st;
  return make_handle(std::move(blob), device_id, out);
}

int32_t xdtts_default_device(void) {
  int32_t v = 0;
  return guard([&] { v = default_device(); }) == XDTTS_OK ? v : -1;
}

xdtts_status xdtts_model_dir_read(const char *dir, float *blob, size_t n_floats) {
  return guard([&] {
    if (!dir || !blob) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n_floats != tensor_total()) fail(XDTTS_ERR_BAD_ARG, "blob has %zu floats, expected %zu", n_floats, tensor_total());
    std::vector<float> v;
    load_model_dir(dir, v);
    std::memcpy(blob, v.data(), v.size() * sizeof(float));
  });
}

xdtts_status xdtts_model_dir_describe(const char *dir, char *buf, size_t cap, size_t *needed) {
  return guard([&] {
    if (!dir || (!buf && cap)) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const std::string d = describe_onnx_dir(dir);
    if (needed) *needed = d.size() + 1;
    if (cap) {
      const size_t n = std::min(cap - 1, d.size());
      std::memcpy(buf, d.data(), n);
      buf[n] = 0;
    }
  });
}

xdtts_status xdtts_tacotron2_load_synthetic(uint32_t seed, float rec_scale, int32_t device_id,
                                            xdtts_tacotron2 **out) {
  std::vector<float> blob;
  xdtts_status st = guard([&] {
    device_id = select_device(device_id);
    synthetic_blob(seed, rec_scale, blob);
  });
  if (st != XDTTS_OK) return st;
  return make_handle(std::move(blob), device_id, out);
}

xdtts_status xdtts_tacotron2_load_blob(const float *blob, size_t n_floats, int32_t device_id,
                                       xdtts_tacotron2 **out) {
  std::vector<float> v;
  xdtts_status st = guard([&] {
    if (!blob) fail(XDTTS_ERR_BAD_ARG, "blob is null");
    if (n_floats != tensor_total()) fail(XDTTS_ERR_BAD_ARG, "blob has %zu floats, expected %zu", n_floats, tensor_total());
    device_id = select_device(device_id);
    v.assign(blob, blob + n_floats);
  });
  if (st != XDTTS_OK) return st;
  return make_handle(std::move(v), device_id, out);
}

xdtts_status xdtts_tacotron2_save(const xdtts_tacotron2 *h, const char *dir) {
  return guard([&] {
    if (!h || !dir) fail(XDTTS_ERR_BAD_ARG, "null argument");
    save_container(dir, h->blob);
  });
}

xdtts_status xdtts_tacotron2_get_tensor(const xdtts_tacotron2 *h, int32_t i, float *out) {
  return guard([&] {
    if (!h || !out || i < 0 || i >= xdtts_tensor_count()) fail(XDTTS_ERR_BAD_ARG, "bad tensor request");
    const TensorInfo &t = tensor_table()[i];
    std::memcpy(out, h->blob.data() + t.offset, t.numel * sizeof(float));
  });
}

void xdtts_tacotron2_free(xdtts_tacotron2 *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

xdtts_status xdtts_tacotron2_sync(xdtts_tacotron2 *h) {
  return guard([&] {
    if (!h) fail(XDTTS_ERR_BAD_ARG, "null handle");
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

xdtts_status xdtts_tacotron2_infer_ids(xdtts_tacotron2 *h, const int64_t *ids, size_t n, const size_t *splits,
                                       size_t n_splits, const xdtts_infer_opts *opts, float **mel,
                                       size_t *n_frames) {
  return guard([&] {
    if (!h || !mel || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    *mel = nullptr;
    *n_frames = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const xdtts_infer_opts o = resolve_opts(opts);
    std::vector<int64_t> padded;
    std::vector<int> lens;
    chunks_from_splits(ids, n, splits, n_splits, o.max_chunk, padded, lens);
    int total = 0;
    const std::vector<int> one_utt(lens.size(), 0);  // (durations: the chunks are one utterance)
    h->infer_batch_device(padded.data(), lens.data(), (int)lens.size(), o.max_chunk, o, nullptr, &total, false, DurAsk{true, false, one_utt.data()});
    PinnedGuard host((size_t)N_MEL * total);
    HIP_CHECK(hipMemcpyAsync(host.p, h->mel_dev.p, (size_t)N_MEL * total * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    h->finish_timings();
    h->publish_durations();
    *mel = host.release();
    *n_frames = (size_t)total;
  });
}

xdtts_status xdtts_tacotron2_infer_batch(xdtts_tacotron2 *h, const int64_t *ids, const int32_t *lens, int32_t B,
                                         int32_t t_stride, const xdtts_infer_opts *opts,
                                         const int32_t *fixed_steps_per_item, float **mels, size_t *n_frames) {
  return guard([&] {
    if (!h || !ids || !lens || !mels || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const xdtts_infer_opts o = resolve_opts(opts);
    if (B <= 0) fail(XDTTS_ERR_BAD_ARG, "batch %d out of range", B);
    for (int b = 0; b < B; ++b) mels[b] = nullptr;
    const int T = o.max_chunk;
    if (t_stride <= 0) fail(XDTTS_ERR_BAD_ARG, "t_stride must be positive");
    const std::vector<int64_t> padded = pad_batch_ids(ids, lens, B, t_stride, T);
    int total = 0;
    // the post-net leaves one dense (80 x F_b) matrix per chunk, back to back: ONE copy into a pinned slab whose pieces
    // are the buffers the caller receives (the (80 x F_total) layout took 4 160 strided row copies on the host for the
    // 52-chunk batch -- as long as the post-net on one thread, 0.3 ms on four; 52 pitched copies from the device 0.9 ms)
    std::vector<int> F = h->infer_batch_device(padded.data(), lens, B, T, o, fixed_steps_per_item, &total, true, DurAsk{true, false, nullptr});
    PinnedSlab slab((size_t)N_MEL * total);
    Drain drain(h->stream);  // the slab does not go back to the pool with the copy in flight
    HIP_CHECK(hipMemcpyAsync(slab.base, h->mel_dev.p, (size_t)N_MEL * total * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    h->finish_timings();
    h->publish_durations();
    size_t off = 0;
    for (int b = 0; b < B; ++b) {
      mels[b] = slab.piece(off);
      n_frames[b] = (size_t)F[b];
      off += (size_t)N_MEL * F[b];
    }
    slab.hand_over();
  });
}

xdtts_status xdtts_tacotron2_encoder(xdtts_tacotron2 *h, const int64_t *ids, int32_t T, float *memory,
                                     float *processed_memory) {
  return guard([&] {
    if (!h || !ids || !memory || !processed_memory) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (T <= 0 || T > T_MAX) fail(XDTTS_ERR_BAD_ARG, "T %d out of range", T);
    for (int t = 0; t < T; ++t)
      if (ids[t] < 0 || ids[t] >= N_SYMBOLS) fail(XDTTS_ERR_BAD_ARG, "id out of range");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    h->ids.upload(ids, T, h->stream);
    std::lock_guard<ChipLock> chip(chip_mutex(h->device));
    h->run_encoder(1, T);
    HIP_CHECK(hipMemcpyAsync(memory, h->memory.p, (size_t)T * EMB * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(processed_memory, h->pmem.p, (size_t)T * ATT_DIM * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->check_encoder_exchange();
  });
}

// Parity hook: encoder.onnx for B chunks of T ids through run_encoder(B, T), the call of infer_batch_device, with the BiLSTM
// engine the caller names.
xdtts_status xdtts_tacotron2_encoder_batch(xdtts_tacotron2 *h, int32_t engine, const int64_t *ids, int32_t B, int32_t T, float *memory,
                                           float *processed_memory) {
  return guard([&] {
    if (!h || !ids || !memory || !processed_memory) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (engine < -1 || engine > 1) fail(XDTTS_ERR_BAD_ARG, "engine %d out of range (-1 the handle's, 0 single-workgroup, 1 cooperative)", engine);
    if (B <= 0 || B > 4096) fail(XDTTS_ERR_BAD_ARG, "batch %d out of range", B);
    if (T <= 0 || T > T_MAX) fail(XDTTS_ERR_BAD_ARG, "window %d out of range (1..%d)", T, T_MAX);
    for (size_t i = 0; i < (size_t)B * T; ++i)
      if (ids[i] < 0 || ids[i] >= N_SYMBOLS) fail(XDTTS_ERR_BAD_ARG, "id %lld out of range (0..%d)", (long long)ids[i], N_SYMBOLS - 1);
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    h->ids.upload(ids, (size_t)B * T, h->stream);
    std::lock_guard<ChipLock> chip(chip_mutex(h->device));
    h->run_encoder(B, T, engine);
    HIP_CHECK(hipMemcpyAsync(memory, h->memory.p, (size_t)B * T * EMB * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipMemcpyAsync(processed_memory, h->pmem.p, (size_t)B * T * ATT_DIM * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->check_encoder_exchange();
  });
}

xdtts_status xdtts_tacotron2_decoder(xdtts_tacotron2 *h, const float *memory, const float *processed_memory,
                                     int32_t T, int32_t n_valid, const xdtts_infer_opts *opts, float *frames,
                                     float *gates, size_t *n_frames) {
  return guard([&] {
    if (!h || !memory || !processed_memory || !frames || !n_frames) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (T <= 0 || T > T_MAX || n_valid <= 0 || n_valid > T) fail(XDTTS_ERR_BAD_ARG, "bad T/n_valid");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    const xdtts_infer_opts o = resolve_opts(opts);
    h->memory.upload(memory, (size_t)T * EMB, h->stream);
    h->pmem.upload(processed_memory, (size_t)T * ATT_DIM, h->stream);
    int nv = n_valid;
    h->n_valid.upload(&nv, 1, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    std::vector<int> lim(1, std::min(o.fixed_steps > 0 ? o.fixed_steps : o.max_steps, o.max_steps));
    h->upload_dropout_masks(o, 1, lim.data());
    DecoderBufs d = h->decoder_bufs(1, T, h->memory.p, h->pmem.p, o);
    HIP_CHECK(hipEventRecord(h->ev.e[0], h->stream));
    HIP_CHECK(hipEventRecord(h->ev.e[1], h->stream));
    h->last_steps = h->run_decoder(d, lim);
    HIP_CHECK(hipEventRecord(h->ev.e[2], h->stream));
    HIP_CHECK(hipEventRecord(h->ev.e[3], h->stream));
    const int F = h->host_ctl[xdtts_tacotron2::HOST_NF];
    HIP_CHECK(hipMemcpyAsync(frames, d.frames, (size_t)F * N_MEL * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (gates) HIP_CHECK(hipMemcpyAsync(gates, d.gates, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    h->finish_timings();
    *n_frames = (size_t)F;
  });
}

// Parity hook: n_steps consecutive decoder_iter.onnx calls (mod.rs:304; each call's outputs fed back as mod.rs:328-341 does)
// for B chunks from caller-held state, through the frame-loop engine the caller names.
xdtts_status xdtts_tacotron2_decoder_steps(xdtts_tacotron2 *h, int32_t engine, int32_t B, const float *memory, const float *processed_memory,
                                           int32_t T, const int32_t *n_valid, const xdtts_infer_opts *opts, uint32_t step0, int32_t n_steps,
                                           const float *decoder_input, float *attention_hidden, float *attention_cell, float *decoder_hidden,
                                           float *decoder_cell, float *attention_weights, float *attention_weights_cum, float *attention_context,
                                           float *decoder_output, float *gate_prediction) {
  return guard([&] {
    if (!h || !memory || !processed_memory || !n_valid || !decoder_input || !attention_hidden || !attention_cell || !decoder_hidden ||
        !decoder_cell || !attention_weights || !attention_weights_cum || !attention_context || !decoder_output || !gate_prediction)
      fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (engine < 0 || engine > 3)
      fail(XDTTS_ERR_BAD_ARG, "engine %d out of range (0 launch-per-stage, 1 persistent, 2 batched MFMA, 3 persistent MFMA)", engine);
    if (engine == 3 && (B > P8_B_MAX || T > PERSIST_T_MAX))
      fail(XDTTS_ERR_BAD_ARG, "the persistent MFMA engine takes at most %d chunks of at most %d encoder steps", P8_B_MAX, PERSIST_T_MAX);
    if (B <= 0 || B > 64) fail(XDTTS_ERR_BAD_ARG, "batch %d out of range (1..64)", B);
    if (T <= 0 || T > T_MAX) fail(XDTTS_ERR_BAD_ARG, "T %d out of range", T);
    if (n_steps <= 0 || n_steps > 100000 || (uint64_t)step0 + (uint64_t)n_steps > (1u << 30)) fail(XDTTS_ERR_BAD_ARG, "bad step range");
    for (int b = 0; b < B; ++b)
      if (n_valid[b] <= 0 || n_valid[b] > T) fail(XDTTS_ERR_BAD_ARG, "chunk %d: bad n_valid %d", b, n_valid[b]);
    if (engine == 1 && (B > PERSIST_B_MAX || T > PERSIST_T_MAX))
      fail(XDTTS_ERR_BAD_ARG, "the persistent engine takes at most %d chunks of at most %d encoder steps", PERSIST_B_MAX, PERSIST_T_MAX);
    if (engine == 1) {
      // The persistent engine folds the context columns of its weights into the encoder memory and works from the attention
      // WEIGHTS (decoder_persistent.hip), so the incoming context must be the one those weights give -- true for every state
      // the graph itself produced (out_attention_context = out_attention_weights . memory, fed back at mod.rs:332-339).
      for (int b = 0; b < B; ++b)
        for (int j = 0; j < EMB; ++j) {
          double c = 0;
          for (int t = 0; t < T; ++t) c += (double)attention_weights[(size_t)b * T + t] * memory[((size_t)b * T + t) * EMB + j];
          if (std::fabs(c - attention_context[(size_t)b * EMB + j]) > 1e-4 + 1e-4 * std::fabs(c))
            fail(XDTTS_ERR_BAD_ARG, "engine 1 needs attention_context = attention_weights . memory (chunk %d, column %d: %g vs %g)", b, j,
                 (double)attention_context[(size_t)b * EMB + j], c);
        }
    }
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    xdtts_infer_opts o = resolve_opts(opts);
    const int end = (int)step0 + n_steps;
    o.max_steps = end + 1;
    hipStream_t st = h->stream;
    h->memory.upload(memory, (size_t)B * T * EMB, st);
    h->pmem.upload(processed_memory, (size_t)B * T * ATT_DIM, st);
    h->n_valid.upload(n_valid, B, st);
    std::vector<int> lim((size_t)B, end);
    h->upload_dropout_masks(o, B, lim.data());
    if (engine == 2) h->w.ensure_batched_layout(h->blob, st);
    DecoderBufs d = h->decoder_bufs(B, T, h->memory.p, h->pmem.p, o, engine == 2 ? 1 : 0);
    d.use_gate = 0;  // the caller applies the stop rule to gate_prediction (mod.rs:319)
    h->limits.upload(lim.data(), lim.size(), st);
    h->lim_on_dev = lim;
    launch_decoder_init(d, h->limits.p, st);
    h->dec_in_dev.upload(decoder_input, (size_t)B * N_MEL, st);
    // staging of the seven state tensors in the caller's row-major layout
    const size_t nh = (size_t)B * ATT_RNN, nt = (size_t)B * T, nc = (size_t)B * EMB;
    h->state_stage.alloc(4 * nh + 2 * nt + nc);
    float *s_ah = h->state_stage.p, *s_ac = s_ah + nh, *s_dh = s_ac + nh, *s_dc = s_dh + nh, *s_aw = s_dc + nh, *s_awc = s_aw + nt, *s_ctx = s_awc + nt;
    auto up = [&](float *dst, const float *src, size_t n) { HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, st)); };
    auto dd = [&](float *dst, const float *src, size_t n) { HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st)); };
    up(s_ah, attention_hidden, nh);
    up(s_ac, attention_cell, nh);
    up(s_dh, decoder_hidden, nh);
    up(s_dc, decoder_cell, nh);
    up(s_aw, attention_weights, nt);
    up(s_awc, attention_weights_cum, nt);
    up(s_ctx, attention_context, nc);
    const int s0 = (int)step0;
    HIP_CHECK(hipMemcpyAsync(d.ctl, &s0, sizeof(int), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));  // the sources above are caller memory / locals
    dd(d.aw, s_aw, nt);
    dd(d.awc, s_awc, nt);
    dd(d.ctx, s_ctx, nc);
    if (engine == 2) {  // the batched kernels keep h, c and the context in MFMA-operand order
      launch_frag_convert(s_ah, d.att_hf[0], B, d.Bpad, ATT_RNN, 0, st);
      launch_frag_convert(s_dh, d.dec_hf[0], B, d.Bpad, DEC_RNN, 0, st);
      launch_frag_convert(s_ac, d.att_c, B, d.Bpad, ATT_RNN, 0, st);
      launch_frag_convert(s_dc, d.dec_c, B, d.Bpad, DEC_RNN, 0, st);
      launch_frag_convert(s_ctx, d.ctxf, B, d.Bpad, EMB, 0, st);
    } else {
      dd(d.att_h[0], s_ah, nh);
      dd(d.att_c, s_ac, nh);
      dd(d.dec_h[0], s_dh, nh);
      dd(d.dec_c, s_dc, nh);
    }
    d.dec_in = h->dec_in_dev.p;
    int fin = 0;  // ping-pong half that holds the final hidden states
    if (engine == 1) {
      if (!decoder_persistent_supported(h->device, PERSIST_B_MAX, PERSIST_T_MAX))
        fail(XDTTS_ERR_HIP, "persistent engine not available on this device (its 256-workgroup grid cannot be co-resident)");
      std::lock_guard<ChipLock> chip(chip_mutex(h->device));
      launch_decoder_prenet(d, h->w, st);  // x(step0) = prenet(decoder_input): the persistent kernel's own prenet produces x(s + 1)
      d.dec_in = nullptr;
      h->dec_exchange.alloc(persist_granule_words(B));
      PersistBufs g = persist_bufs(h->dec_exchange.p, h->dec_err.p, B);
      launch_persist_seed_at(d, g, h->limits.p, s0, st);
      try {
        launch_decoder_persistent(d, h->w, g, n_steps, st);
      } catch (const CoopRefused &) {
        (void)hipStreamSynchronize(st);
        fail(XDTTS_ERR_HIP, "persistent engine not available on this device (cooperative launch refused)");
      }
      if (fetch_and_clear_error_word(h->dec_err.p, st)) fail(XDTTS_ERR_HIP, "persistent decoder exchange timed out (grid not co-resident)");
    } else if (engine == 3) {
      if (!decoder_p8_supported(h->device, B, PERSIST_T_MAX))
        fail(XDTTS_ERR_HIP, "persistent MFMA engine not available on this device (its 256-workgroup grid cannot be co-resident)");
      std::lock_guard<ChipLock> chip(chip_mutex(h->device));
      launch_decoder_prenet(d, h->w, st);  // x(step0) = prenet(decoder_input)
      d.dec_in = nullptr;
      h->dec_exchange.alloc(p8_exchange_words(B, n_steps));
      P8Bufs g = p8_bufs(h->dec_exchange.p, h->dec_err.p, B, n_steps);
      launch_p8_seed_at(d, g, h->limits.p, s0, st);
      try {
        launch_decoder_p8(d, h->w, g, n_steps, st);
      } catch (const CoopRefused &) {
        (void)hipStreamSynchronize(st);
        fail(XDTTS_ERR_HIP, "persistent MFMA engine not available on this device (cooperative launch refused)");
      }
      if (fetch_and_clear_error_word(h->dec_err.p, st)) fail(XDTTS_ERR_HIP, "persistent MFMA decoder exchange timed out (grid not co-resident)");
    } else {
      std::unique_lock<ChipLock> chip;
      if (d.hg) chip = std::unique_lock<ChipLock>(chip_mutex(h->device));
      if (engine == 0) launch_decoder_location(d, h->w, st);  // (the batched prenet launch computes them itself)
      launch_decoder_early(d, h->w, 0, st);  // (batched engine: the first attention-LSTM pass's early partial, from the imported state)
      launch_decoder_prologue(d, h->w, st);  // (two-launch form: x and location features of the first step; d.dec_in = decoder_input)
      for (int i = 0; i < n_steps; ++i) {
        launch_decoder_step_at(d, h->w, i, st);
        d.dec_in = nullptr;  // from the second step on the loop feeds itself
      }
      launch_decoder_advance(d, n_steps, st);
      launch_decoder_flush(d, h->w, st);  // decoder_output and gate_prediction of the last step
      fin = n_steps & 1;
      if (d.ep_g && fetch_and_clear_error_word(h->dec_err.p, st)) fail(XDTTS_ERR_HIP, "batched attention exchange timed out (grid not co-resident)");
    }
    if (engine == 2) {
      launch_frag_convert(s_ah, d.att_hf[fin], B, d.Bpad, ATT_RNN, 1, st);
      launch_frag_convert(s_dh, d.dec_hf[fin], B, d.Bpad, DEC_RNN, 1, st);
      launch_frag_convert(s_ac, d.att_c, B, d.Bpad, ATT_RNN, 1, st);
      launch_frag_convert(s_dc, d.dec_c, B, d.Bpad, DEC_RNN, 1, st);
    }
    auto down = [&](float *dst, const float *src, size_t n) { HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, st)); };
    down(attention_hidden, engine == 2 ? s_ah : d.att_h[fin], nh);
    down(attention_cell, engine == 2 ? s_ac : d.att_c, nh);
    down(decoder_hidden, engine == 2 ? s_dh : d.dec_h[fin], nh);
    down(decoder_cell, engine == 2 ? s_dc : d.dec_c, nh);
    down(attention_weights, d.aw, nt);
    down(attention_weights_cum, engine == 2 && (n_steps & 1) ? d.awc2 : d.awc, nt);  // (batched: ping-pong by step parity)
    down(attention_context, d.ctx, nc);
    for (int b = 0; b < B; ++b) {
      down(decoder_output + (size_t)b * n_steps * N_MEL, d.frames + ((size_t)b * d.max_steps + step0) * N_MEL, (size_t)n_steps * N_MEL);
      down(gate_prediction + (size_t)b * n_steps, d.gates + (size_t)b * d.max_steps + step0, (size_t)n_steps);
    }
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

// Parity hook: ONE decoder_iter.onnx call (mod.rs:304) from caller-held state, on the launch-per-stage kernels.
xdtts_status xdtts_tacotron2_decoder_step(xdtts_tacotron2 *h, const float *memory, const float *processed_memory, int32_t T,
                                          int32_t n_valid, const xdtts_infer_opts *opts, uint32_t step, const float *decoder_input,
                                          float *attention_hidden, float *attention_cell, float *decoder_hidden, float *decoder_cell,
                                          float *attention_weights, float *attention_weights_cum, float *attention_context,
                                          float *decoder_output, float *gate_prediction) {
  return xdtts_tacotron2_decoder_steps(h, 0, 1, memory, processed_memory, T, &n_valid, opts, step, 1, decoder_input, attention_hidden,
                                       attention_cell, decoder_hidden, decoder_cell, attention_weights, attention_weights_cum,
                                       attention_context, decoder_output, gate_prediction);
}

// Which engines this handle currently uses (1 = the persistent / cooperative one, 0 = demoted to the
// launch-per-stage / single-workgroup one after a timed-out exchange, -1 = not probed yet).
xdtts_status xdtts_tacotron2_engine_state(const xdtts_tacotron2 *h, int32_t *decoder_persistent, int32_t *encoder_cooperative,
                                          int32_t *batched_attention) {
  return guard([&] {
    if (!h) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (decoder_persistent) *decoder_persistent = h->pair_gate.abi_state();
    if (encoder_cooperative) *encoder_cooperative = h->enc_gate.state != EngineGate::OFF ? 1 : 0;
    if (batched_attention) *batched_attention = h->att_fused();
  });
}

xdtts_status xdtts_tacotron2_small_batch_engine_state(const xdtts_tacotron2 *h, int32_t *state) {
  return guard([&] {
    if (!h || !state) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *state = h->p8_gate.abi_state();
  });
}

// Puts a demoted handle back on the fast engines (they are probed again on the next call).
xdtts_status xdtts_tacotron2_engine_reset(xdtts_tacotron2 *h) {
  return guard([&] {
    if (!h) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    // (a launch the runtime REFUSED is a property of the device, not a transient: those engines stay off)
    h->pair_gate.reset();
    h->p8_gate.reset();
    h->enc_gate.reset();
    h->att_gate.reset();
    h->att_form = env::int_or(env::ATT_FUSED, 2);
  });
}

// Measurement aid (bench.py's roofline.latency_floor_us): the five dependent all-gather exchanges of one persistent-decoder
// step with no arithmetic between them, timed on THIS device now (csrc/edge_floor.hip).
xdtts_status xdtts_edge_floor_us(int32_t device_id, int32_t steps, int32_t T, int32_t tuned, double *us_per_step) {
  return guard([&] {
    if (!us_per_step || steps < 1 || steps > 1000000 || T < 1 || T > 128) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    device_id = select_device(device_id);
    std::lock_guard<ChipLock> chip(chip_mutex(device_id));  // its grid must be co-resident, like the engine's
    const double us = xdtts_edge_floor::measure(device_id, steps, T, xdtts_edge_floor::kernel_delays(tuned ? 1 : 0), 5, false);
    if (us < 0) fail(XDTTS_ERR_HIP, "edge-floor skeleton: grid not co-resident on this device, or an exchange failed");
    *us_per_step = us;
  });
}

xdtts_status xdtts_tacotron2_postnet(xdtts_tacotron2 *h, const float *frames, int32_t F, float *mel_out) {
  return guard([&] {
    if (!h || !frames || !mel_out || F <= 0) fail(XDTTS_ERR_BAD_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    h->frames.upload(frames, (size_t)F * N_MEL, h->stream);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    h->mel_dev.alloc((size_t)N_MEL * F);
    const long zero = 0;
    h->run_postnet(h->frames.p, 0, &F, &zero, 1, h->mel_dev.p, F);
    HIP_CHECK(hipMemcpyAsync(mel_out, h->mel_dev.p, (size_t)N_MEL * F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

// Parity hook: postnet.onnx for n chunks through postnet_groups, the group loop behind every decode of infer_batch_device.
xdtts_status xdtts_tacotron2_postnet_batch(xdtts_tacotron2 *h, const float *frames, size_t frame_stride, const int32_t *F, int32_t n,
                                           int32_t per_chunk, float *out) {
  return guard([&] {
    if (!h || !frames || !F || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    if (n <= 0 || n > 4096) fail(XDTTS_ERR_BAD_ARG, "batch %d out of range", n);
    if (frame_stride == 0 || frame_stride % N_MEL != 0 || frame_stride > ((size_t)1 << 26)) fail(XDTTS_ERR_BAD_ARG, "frame_stride must be a multiple of %d", N_MEL);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
      if (F[i] <= 0 || (size_t)F[i] * N_MEL > frame_stride) fail(XDTTS_ERR_BAD_ARG, "chunk %d: %d frames do not fit the stride", i, F[i]);
      total += (size_t)F[i];
    }
    if (total > ((size_t)1 << 24)) fail(XDTTS_ERR_BAD_ARG, "%zu frames in all", total);
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    h->frames.alloc((size_t)n * frame_stride);
    for (int i = 0; i < n; ++i)  // the rows behind F[i] keep whatever the buffer held, as behind a decode
      HIP_CHECK(hipMemcpyAsync(h->frames.p + (size_t)i * frame_stride, frames + (size_t)i * frame_stride, (size_t)F[i] * N_MEL * sizeof(float),
                               hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    const int got = h->postnet_groups(h->frames.p, frame_stride, F, nullptr, n, per_chunk != 0);
    HIP_CHECK(hipMemcpyAsync(out, h->mel_dev.p, (size_t)N_MEL * got * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  });
}

// ---- durations (durations_plan.h, durations.hip) --------------------------------------------------------------------------

static DurationsOpts dur_opts_of(const xdtts_durations_opts *o) {
  static_assert(sizeof(xdtts_durations_opts) == sizeof(DurationsOpts) && sizeof(xdtts_alignment_stats) == sizeof(AlignmentStats),
                "durations_plan.h mirrors the structs of include/xdtts.h");
  if (!o) return durations_default();
  const DurationsOpts d{o->on, o->min_frames, o->max_frames};
  const std::string bad = durations_check(d);
  if (!bad.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", bad.c_str());
  return d;
}

void xdtts_durations_default(xdtts_durations_opts *o) {
  if (!o) return;
  const DurationsOpts d = durations_default();
  o->on = d.on;
  o->min_frames = d.min_frames;
  o->max_frames = d.max_frames;
}

xdtts_status xdtts_tacotron2_set_durations(xdtts_tacotron2 *h, const xdtts_durations_opts *o) {
  return guard([&] {
    const DurationsOpts d = dur_opts_of(o);  // the fields, before the handle
    if (!h) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->dur_opts = d;
  });
}

xdtts_status xdtts_tacotron2_get_durations(const xdtts_tacotron2 *h, xdtts_durations_opts *o) {
  return guard([&] {
    if (!h || !o) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    o->on = h->dur_opts.on;
    o->min_frames = h->dur_opts.min_frames;
    o->max_frames = h->dur_opts.max_frames;
  });
}

xdtts_status xdtts_tacotron2_last_durations_count(const xdtts_tacotron2 *h, size_t *n_utterances) {
  return guard([&] {
    if (!h || !n_utterances) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *n_utterances = h->dur_n_utt;
  });
}

xdtts_status xdtts_tacotron2_last_durations(const xdtts_tacotron2 *h, size_t utterance, float *dur, uint32_t *dur_q16, uint64_t *start_q16,
                                            size_t cap, size_t *n_ids) {
  return guard([&] {
    if (!h || !n_ids) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (utterance >= h->dur_n_utt) fail(XDTTS_ERR_BAD_ARG, "utterance %zu: the last call captured durations of %zu", utterance, h->dur_n_utt);
    const DurUtt &U = h->dur_plan.utt[utterance];
    *n_ids = (size_t)U.n_ids;
    const size_t n = std::min(cap, (size_t)U.n_ids);
    if (dur) std::memcpy(dur, h->dur_f32() + U.id_off, n * sizeof(float));
    if (dur_q16) std::memcpy(dur_q16, h->dur_q16() + U.id_off, n * sizeof(uint32_t));
    if (start_q16) std::memcpy(start_q16, h->dur_start() + U.id_off, n * sizeof(uint64_t));
  });
}

xdtts_status xdtts_tacotron2_last_alignment(const xdtts_tacotron2 *h, size_t utterance, xdtts_alignment_stats *out) {
  return guard([&] {
    if (!h || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (utterance >= h->dur_n_utt) fail(XDTTS_ERR_BAD_ARG, "utterance %zu: the last call captured durations of %zu", utterance, h->dur_n_utt);
    std::memcpy(out, h->dur_stats() + utterance, sizeof(*out));
  });
}

// the outputs of the stage alone / of its host reference, cleared and checked alike
static void dur_gather_args(const float *cum_a, const float *cum_b, int32_t B, int32_t T, const int32_t *nframes, const int32_t *n_valid,
                            const int32_t *order, int32_t batched, const int32_t *utt_of_chunk, size_t *n_ids, size_t *n_utt, DurPlan *plan) {
  if (n_ids) *n_ids = 0;
  if (n_utt) *n_utt = 0;
  if (!cum_a || !nframes || !n_valid) fail(XDTTS_ERR_BAD_ARG, "null argument");
  const std::string bad = durations_plan(B, T, nframes, n_valid, order, batched, cum_b != nullptr, utt_of_chunk, plan);
  if (!bad.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", bad.c_str());
}
static void dur_gather_room(const DurPlan &plan, size_t cap_ids, size_t cap_utt, size_t *n_ids, size_t *n_utt) {
  if (n_ids) *n_ids = plan.n_ids;
  if (n_utt) *n_utt = plan.utt.size();
  if (cap_ids < plan.n_ids || cap_utt < plan.utt.size())
    fail(XDTTS_ERR_BAD_ARG, "durations: room for %zu ids and %zu utterances, the request has %zu and %zu", cap_ids, cap_utt, plan.n_ids, plan.utt.size());
}

xdtts_status xdtts_durations_reference(const float *cum_a, const float *cum_b, int32_t B, int32_t T, const int32_t *nframes, const int32_t *n_valid,
                                       const int32_t *order, int32_t batched, const int32_t *utt_of_chunk, const xdtts_durations_opts *opts,
                                       float *dur, uint32_t *dur_q16, uint64_t *start_q16, size_t cap_ids, xdtts_alignment_stats *stats,
                                       size_t cap_utt, size_t *n_ids, size_t *n_utt) {
  return guard([&] {
    const DurationsOpts o = dur_opts_of(opts);
    DurPlan plan;
    dur_gather_args(cum_a, cum_b, B, T, nframes, n_valid, order, batched, utt_of_chunk, n_ids, n_utt, &plan);
    dur_gather_room(plan, cap_ids, cap_utt, n_ids, n_utt);
    durations_reference(plan, cum_a, cum_b, T, nframes, batched, o, dur, dur_q16, start_q16, reinterpret_cast<AlignmentStats *>(stats));
  });
}

// Parity hook: the stage alone on caller arrays, through launch_durations -- the launches behind every decode.
xdtts_status xdtts_tacotron2_durations_gather(xdtts_tacotron2 *h, const float *cum_a, const float *cum_b, int32_t B, int32_t T,
                                              const int32_t *nframes, const int32_t *n_valid, const int32_t *order, int32_t batched,
                                              const int32_t *utt_of_chunk, const xdtts_durations_opts *opts, float *dur, uint32_t *dur_q16,
                                              uint64_t *start_q16, size_t cap_ids, xdtts_alignment_stats *stats, size_t cap_utt, size_t *n_ids,
                                              size_t *n_utt) {
  return guard([&] {
    const DurationsOpts o = dur_opts_of(opts);
    DurPlan plan;
    dur_gather_args(cum_a, cum_b, B, T, nframes, n_valid, order, batched, utt_of_chunk, n_ids, n_utt, &plan);
    dur_gather_room(plan, cap_ids, cap_utt, n_ids, n_utt);
    if (!h) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_CHECK(hipSetDevice(h->device));
    const size_t nt = (size_t)B * T;
    h->state_stage.alloc(2 * nt);
    DevBuf<int> counts;
    counts.alloc((size_t)2 * B);
    HIP_CHECK(hipMemcpyAsync(h->state_stage.p, cum_a, nt * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (batched) HIP_CHECK(hipMemcpyAsync(h->state_stage.p + nt, cum_b, nt * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(counts.p, nframes, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipMemcpyAsync(counts.p + B, n_valid, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));  // the sources above are caller memory
    h->enqueue_durations(h->state_stage.p, h->state_stage.p + nt, counts.p, counts.p + B, B, T, n_valid, order, batched != 0, utt_of_chunk, o);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    const size_t N = plan.n_ids, U = plan.utt.size();
    if (dur) std::memcpy(dur, h->dur_f32(), N * sizeof(float));
    if (dur_q16) std::memcpy(dur_q16, h->dur_q16(), N * sizeof(uint32_t));
    if (start_q16) std::memcpy(start_q16, h->dur_start(), N * sizeof(uint64_t));
    if (stats) std::memcpy(stats, h->dur_stats(), U * sizeof(*stats));
    h->dur_n_utt = h->dur_pending = 0;  // (a hook is no request: last_durations reports nothing of it)
  });
}

double xdtts_durations_position(const uint64_t *start_q16, const uint32_t *dur_q16, size_t n, size_t n_frames, double x) {
  return durations_position(start_q16, dur_q16, n, n_frames, x);
}

int64_t xdtts_durations_samples(uint64_t start_q16, int32_t hop, int64_t rate_out) { return durations_samples(start_q16, hop, rate_out); }

xdtts_status xdtts_tacotron2_last_timings(const xdtts_tacotron2 *h, float ms[4], int32_t *steps) {
  return guard([&] {
    if (!h || !ms) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int i = 0; i < 4; ++i) ms[i] = h->last_ms[i];
    if (steps) *steps = h->last_steps;
  });
}

}  // extern "C"
