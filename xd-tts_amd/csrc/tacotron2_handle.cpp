// tacotron2_handle.cpp -- the mel-generator handle outside the frame loop: encoder, decoder workspaces, post-net and the
// request path infer_batch_device (infer_chunk x B, mod.rs:361-393).
#include "tacotron2_handle.h"

#include <algorithm>
#include <cmath>

using namespace xdtts;

xdtts_tacotron2::~xdtts_tacotron2() {
  if (fetched) (void)hipEventDestroy(fetched);
  if (host_ctl) (void)hipHostFree(host_ctl);
  if (in_host) (void)hipHostFree(in_host);
  if (dur_tab_host) (void)hipHostFree(dur_tab_host);
  if (dur_out_host) (void)hipHostFree(dur_out_host);
  if (dur_ev) (void)hipEventDestroy(dur_ev);
  if (stream) (void)hipStreamDestroy(stream);
}

void xdtts_tacotron2::init(int dev) {
  device = dev;
  select_device(dev);
  HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  ev.create();
  HIP_CHECK(hipEventCreateWithFlags(&fetched, hipEventDisableTiming));
  HIP_CHECK(hipHostMalloc((void **)&host_ctl, sizeof(int) * CTL_INTS, hipHostMallocDefault));
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  coop_group = cus / 8 < 1 ? 1 : cus / 8;
  n_cu = cus;
  ctlblk.alloc(CTL_INTS);
  HIP_CHECK(hipMemsetAsync(ctlblk.p, 0, sizeof(int) * CTL_INTS, stream));
  ctl.p = ctlblk.p;
  enc_err.p = ctlblk.p + HOST_ENC_ERR;
  dec_err.p = ctlblk.p + HOST_DEC_ERR;
  nframes.p = ctlblk.p + HOST_NF;
  w.upload(blob, stream);
}

void xdtts_tacotron2::run_gemm(GemmArgs &g) {
  size_t wsf = 0, tiles = 0;
  int tile = 0;
  const int sk = gemm_splitk_plan(g, &wsf, &tiles, &tile);
  if (sk > 1) {
    if (tiles > gemm_cnt.n) {
      gemm_cnt.alloc(std::max<size_t>(tiles, 4096));
      HIP_CHECK(hipMemsetAsync(gemm_cnt.p, 0, gemm_cnt.n * sizeof(unsigned), stream));
    }
    gemm_ws.alloc(wsf);
    g.splitk = sk;
    g.tile = tile;
    g.ws = gemm_ws.p;
    g.cnt = gemm_cnt.p;
  }
  launch_gemm_nt(g, stream);
}

void xdtts_tacotron2::run_encoder(int B, int T, int bilstm) {
  const int pad = (ENC_K - 1) / 2, TP = T + 2 * pad;
  const size_t padded = (size_t)B * TP * EMB;
  xpadA.alloc(padded);
  xpadB.alloc(padded);
  xproj.alloc((size_t)2 * B * T * 4 * ENC_H);
  memory.alloc((size_t)B * T * EMB);
  pmem.alloc((size_t)B * T * ATT_DIM);
  // only the padding rows must read as zero, and nothing ever writes them (the embedding and the convolutions store rows
  // pad .. pad + T - 1 of every chunk): the fills are needed when the layout (or the allocation) changes, not per request
  if (xpad_zero[0] != xpadA.p || xpad_zero[1] != xpadB.p || xpad_B != B || xpad_T != T) {
    HIP_CHECK(hipMemsetAsync(xpadA.p, 0, padded * sizeof(float), stream));
    HIP_CHECK(hipMemsetAsync(xpadB.p, 0, padded * sizeof(float), stream));
    xpad_zero[0] = xpadA.p;
    xpad_zero[1] = xpadB.p;
    xpad_B = B;
    xpad_T = T;
  }
  launch_embed(ids.p, w.emb.p, xpadA.p, B, T, pad, stream);
  float *src = xpadA.p, *dst = xpadB.p;
  for (int i = 0; i < ENC_CONVS; ++i) {
    GemmArgs g{};
    g.A = src;
    g.lda = EMB;
    g.strideA = (long)TP * EMB;
    g.W = w.enc_conv[i].w.p;
    g.bias = w.enc_conv[i].b.p;
    g.C = dst + (size_t)pad * EMB;
    g.ldc = EMB;
    g.strideC = (long)TP * EMB;
    g.M = T;
    g.N = EMB;
    g.K = ENC_K * EMB;
    g.batch = B;
    g.act = 1;
    run_gemm(g);
    std::swap(src, dst);
  }
  for (int d = 0; d < 2; ++d) {  // BiLSTM input projections for all T at once
    GemmArgs g{};
    g.A = src + (size_t)pad * EMB;
    g.lda = EMB;
    g.strideA = (long)TP * EMB;
    g.W = w.enc_wih[d].p;
    g.bias = w.enc_bias[d].p;
    g.C = xproj.p + (size_t)d * B * T * 4 * ENC_H;
    g.ldc = 4 * ENC_H;
    g.strideC = (long)T * 4 * ENC_H;
    g.M = T;
    g.N = 4 * ENC_H;
    g.K = EMB;
    g.batch = B;
    run_gemm(g);
  }
  // a demoted encoder probes the cooperative recurrence again by itself (its own counter: the decoder's re-probe does not
  // depend on it, and a batched decode never passes through use_persistent)
  if (bilstm < 0) {
    enc_gate.ensure_probed([] { return true; });
    enc_gate.tick();
  }
  bool coop_ran = false;
  if (bilstm < 0 ? enc_gate.usable() : bilstm == 1) {
    // groups of four workgroups per direction, at most coop_group of them per launch; from coop_group + 1 chunks on a group
    // takes two chunks (52 chunks on 256 CUs: one launch of 26 two-chunk groups; it was 26 + 26 one-chunk groups)
    const int slots = B > coop_group ? (B + 1) / 2 : B;  // groups needed
    const int launches = (slots + coop_group - 1) / coop_group, group = B > coop_group ? coop_group : (B + launches - 1) / launches;
    enc_exchange.alloc(bilstm_coop_exchange_words(2 * group));
    try {
      launch_bilstm_coop(xproj.p, w.enc_whhT[0].p, w.enc_whhT[1].p, memory.p, enc_exchange.p, enc_err.p, B, T, group,
                         stream);
      coop_ran = true;
    } catch (const CoopRefused &) {
      if (bilstm == 1) {
        (void)hipStreamSynchronize(stream);
        fail(XDTTS_ERR_HIP, "cooperative encoder BiLSTM not available on this device (cooperative launch refused)");
      }
      // the runtime refused the cooperative grid (CU masking, a smaller part): the single-workgroup recurrence serves
      // this handle from now on -- the refusal is a property of the device, not a transient
      enc_gate.refuse();
      std::fprintf(stderr, "libxdtts_hip: cooperative encoder BiLSTM launch refused by the runtime; this handle uses the "
                           "single-workgroup recurrence\n");
    }
  }
  if (!coop_ran) launch_bilstm(xproj.p, w.enc_whhT[0].p, w.enc_whhT[1].p, memory.p, B, T, stream);
  GemmArgs g{};  // processed_memory = memory_layer(memory)
  g.A = memory.p;
  g.lda = EMB;
  g.strideA = (long)T * EMB;
  g.W = w.mem_w.p;
  g.C = pmem.p;
  g.ldc = ATT_DIM;
  g.strideC = (long)T * ATT_DIM;
  g.M = T;
  g.N = ATT_DIM;
  g.K = EMB;
  g.batch = B;
  run_gemm(g);
}

// dropout_mode 2 (SURVEY 8(b) "explicit(mask ptr)"): the caller's keep bytes [B][steps][2][256] go to the device; every
// chunk's step limit must lie inside them.  Any other mode value than 0 / 1 / 2 is refused here too.
void xdtts_tacotron2::upload_dropout_masks(const xdtts_infer_opts &o, int B, const int *lim) {
  if (o.dropout_mode < 0 || o.dropout_mode > 2) fail(XDTTS_ERR_BAD_ARG, "dropout_mode %d out of range (0 off, 1 seeded, 2 explicit)", o.dropout_mode);
  if (o.dropout_mode != 2) return;
  if (!o.dropout_masks || o.dropout_mask_steps <= 0) fail(XDTTS_ERR_BAD_ARG, "dropout_mode 2 needs dropout_masks and dropout_mask_steps");
  for (int b = 0; b < B; ++b)
    if (lim[b] > o.dropout_mask_steps)
      fail(XDTTS_ERR_BAD_ARG, "chunk %d may run %d steps, the dropout masks cover %d", b, lim[b], o.dropout_mask_steps);
  drop_dev.upload(o.dropout_masks, (size_t)B * o.dropout_mask_steps * 2 * PRENET, stream);
}

DecoderBufs xdtts_tacotron2::decoder_bufs(int B, int T, const float *mem, const float *pm, const xdtts_infer_opts &o, int force_batched) {
  const bool batched = force_batched < 0 ? B >= BATCH_MFMA_MIN : force_batched != 0;
  const int ms = o.max_steps;
  att_h.alloc((size_t)2 * B * ATT_RNN);
  att_c.alloc((size_t)((B + 15) / 16 * 16) * ATT_RNN);  // (batched mode: [256][Bpad][4])
  dec_h.alloc((size_t)2 * B * DEC_RNN);
  dec_c.alloc((size_t)((B + 15) / 16 * 16) * DEC_RNN);
  aw.alloc((size_t)B * T);
  awc.alloc((size_t)B * T);
  ctx.alloc((size_t)B * EMB);
  x.alloc((size_t)B * PRENET);
  loc.alloc((size_t)B * T * ATT_DIM);
  e_part.alloc((size_t)B * (ATT_DIM / 4) * T);
  pmel.alloc(decoder_pmel_floats(B));
  frames.alloc((size_t)B * ms * N_MEL);
  gates.alloc((size_t)B * ms);
  DecoderBufs d{};
  d.B = B;
  d.T = T;
  d.memory = mem;
  d.pmem = pm;
  d.n_valid = n_valid.p;
  d.att_h[0] = att_h.p;
  d.att_h[1] = att_h.p + (size_t)B * ATT_RNN;
  d.att_c = att_c.p;
  d.dec_h[0] = dec_h.p;
  d.dec_h[1] = dec_h.p + (size_t)B * DEC_RNN;
  d.dec_c = dec_c.p;
  d.aw = aw.p;
  d.awc = awc.p;
  d.ctx = ctx.p;
  d.x = x.p;
  d.loc = loc.p;
  d.e_part = e_part.p;
  d.pmel = pmel.p;
  d.frames = frames.p;
  d.gates = gates.p;
  d.nframes = nframes.p;
  d.ctl = ctl.p;
  d.max_steps = ms;
  d.use_gate = o.fixed_steps > 0 ? 0 : 1;
  d.gate_threshold = o.gate_threshold;
  {  // gate_fires (device_utils.h): where the verdict needs no sigmoid
    const double t = (double)o.gate_threshold;
    d.gate_lo = -INFINITY;  // (an empty band on either side = always the reference's arithmetic)
    d.gate_hi = INFINITY;
    if (t > 1e-3 && t < 1.0 - 1e-3) {
      const double L = std::log(t / (1.0 - t)), w = 1e-3 * (1.0 + std::fabs(L));
      d.gate_lo = (float)(L - w);
      d.gate_hi = (float)(L + w);
    }
  }
  d.dropout_mode = o.dropout_mode;
  d.dropout_seed = o.dropout_seed;
  d.item_base = o.item_base;
  if (o.dropout_mode == 2) {  // the caller's keep masks, uploaded by upload_dropout_masks()
    d.drop_masks = drop_dev.p;
    d.drop_steps = o.dropout_mask_steps;
  }
  if (batched) {  // MFMA B-operand copies [K/4][Bpad][4] of the vectors the LSTM GEMMs consume
    const int Bpad = (B + 15) / 16 * 16;
    frag.alloc((size_t)Bpad * (PRENET + EMB + 2 * ATT_RNN + 2 * DEC_RNN) + (size_t)B * T);
    d.Bpad = Bpad;
    d.xf = frag.p;
    d.ctxf = d.xf + (size_t)Bpad * PRENET;
    d.att_hf[0] = d.ctxf + (size_t)Bpad * EMB;
    d.att_hf[1] = d.att_hf[0] + (size_t)Bpad * ATT_RNN;
    d.dec_hf[0] = d.att_hf[1] + (size_t)Bpad * ATT_RNN;
    d.dec_hf[1] = d.dec_hf[0] + (size_t)Bpad * DEC_RNN;
    d.awc2 = d.dec_hf[1] + (size_t)Bpad * DEC_RNN;
    pmem_t.alloc((size_t)B * T * ATT_DIM);
    launch_dimgroup_transpose(pm, pmem_t.p, B, T, stream);
    d.pmem_t = pmem_t.p;
    // a timed-out exchange demoted the handle to separate kernels; the cause may be transient: try again after PROBE_AFTER batches
    att_gate.ensure_probed([] { return true; });
    if (att_gate.tick()) att_form = env::int_or(env::ATT_FUSED, 2);
    if (att_fused() > 0 && T <= T_MAX) {  // one-launch attention: partial energies cross as tagged granules
      const size_t ne = (size_t)B * ATT_EXCHANGE_BLOCKS * T;
      att_exchange.alloc(ne + (size_t)B * ATT_RNN);
      d.ep_g = att_exchange.p;
      d.att_err = dec_err.p;
      // ... and the attention LSTM in the same launch: its 256 blocks of 512 threads must be resident together, one per CU
      if (att_fused() > 1 && B <= 64 && n_cu >= ATT_RNN / 4) {
        d.hg = att_exchange.p + ne;
        if (early_partial) {  // early partial of the attention-LSTM GEMM, computed by extra blocks of the decoder-LSTM launch (kernels.h)
          att_part.alloc((size_t)(ATT_RNN / 4) * 4 * 64 * 4);
          d.att_part = att_part.p;
          if (two_launch && T <= PERSIST_T_MAX) {  // ... and the prenet as the tail of that launch (h_dec / mel cross as granules)
            tail_exchange.alloc((size_t)B * (DEC_RNN + 96));
            d.hdg = tail_exchange.p;
            d.melg = d.hdg + (size_t)B * DEC_RNN;
            dec_part.alloc((size_t)(DEC_RNN / 4) * 4 * 64 * 4);
            d.dec_part = dec_part.p;
          }
        }
      }
      env::override_int(env::ATT_SPINS, &d.att_spins);    // test hooks for the
      env::override_int(env::ATT_FAULT, &d.att_fault);    // lost-block path
      env::override_int(env::TAIL_FAULT, &d.tail_fault);  // (two-launch form: a block whose h_dec never arrives)
      env::override_int(env::ATT_SLOW, &d.att_slow);      // straggler block
    }
  }
  return d;
}

// postnet.onnx (mod.rs:345-355) for one chunk: frames_dev [F][80] (row stride 80) ->
// out[m * ldc + t] for m < 80, t < F  (the (80 x F) Array2 layout), residual included.
// postnet.onnx (mod.rs:345-355) for n <= GEMM_RAGGED_MAX chunks in one launch per layer: chunk i has
// F[i] frames at frames_dev + i * frame_stride ([F][80], row stride 80) and its (80 x F[i]) result
// goes to out + col_off[i] with row stride ldc (the (80 x F_total) Array2 layout), residual included.
// dense_items: chunk i's result is a dense (80 x F[i]) matrix of its own at out + col_off[i] (ldc unused).
void xdtts_tacotron2::run_postnet(const float *frames_dev, size_t frame_stride, const int *F, const long *col_off, int n, float *out,
                                  long ldc, bool dense_items) {
  const int pad = (POST_K - 1) / 2;
  int Fmax = 0;
  for (int i = 0; i < n; ++i) Fmax = std::max(Fmax, F[i]);
  const size_t FP = (size_t)Fmax + 2 * pad, slot = FP * POST_CH, slot0 = FP * N_MEL;
  pp0.alloc(slot0 * n);
  ppA.alloc(slot * n);
  ppB.alloc(slot * n);
  // What must read as zero -- the padding rows and, in a ragged group, the rows between a chunk's end and the longest chunk's
  // -- is never written (the copy and the convolutions store rows pad .. pad + F[z] - 1 of item z), so the three fills are
  // due when the group's layout or an allocation changes, not per request (the 80-channel input has its own buffer for that:
  // as a second view of ppB it left 80-channel rows where the 512-channel layout has its padding)
  {
    std::vector<long> sig{(long)n, (long)Fmax, (long)(size_t)pp0.p, (long)(size_t)ppA.p, (long)(size_t)ppB.p};
    for (int z = 0; z < n; ++z) sig.push_back(F[z]);
    if (sig != pp_sig) {
      HIP_CHECK(hipMemsetAsync(pp0.p, 0, slot0 * n * sizeof(float), stream));
      HIP_CHECK(hipMemsetAsync(ppA.p, 0, slot * n * sizeof(float), stream));
      HIP_CHECK(hipMemsetAsync(ppB.p, 0, slot * n * sizeof(float), stream));
      pp_sig = sig;
    }
  }
  // layer 0 input: the frames themselves in zero-padded [FP][80] buffers
  launch_copy_rows(frames_dev, frame_stride, pp0.p + (size_t)pad * N_MEL, slot0, F, n, N_MEL, stream);
  float *src = pp0.p, *dst = ppA.p;
  for (int i = 0; i < POST_CONVS; ++i) {
    const ConvGemm &c = w.post_conv[i];
    const bool last = i == POST_CONVS - 1;
    GemmArgs g{};
    g.A = src;
    g.lda = c.ci;
    g.strideA = (long)(i == 0 ? slot0 : slot);
    g.W = c.w.p;
    g.bias = c.b.p;
    g.M = Fmax;
    g.N = c.co;
    g.K = c.k * c.ci;
    g.batch = n;
    g.ragged = 1;
    for (int z = 0; z < n; ++z) {
      g.Mz[z] = F[z];
      g.Cz[z] = last ? col_off[z] : 0;
    }
    if (!last) {
      g.C = dst + (size_t)pad * c.co;
      g.ldc = c.co;
      g.strideC = (long)slot;
      g.act = 2;
    } else {
      g.C = out;
      g.ldc = ldc;
      g.transpose_out = 1;
      g.ldc_rows = dense_items ? 1 : 0;
      g.R = frames_dev;
      g.ldr = N_MEL;
      g.strideR = (long)frame_stride;
    }
    run_gemm(g);
    if (i == 0) src = ppB.p;  // (layers 1.. ping-pong between the two 512-channel buffers)
    std::swap(src, dst);
  }
}

// The post-net behind a decode, and the parity hook's (xdtts_tacotron2_postnet_batch): run_postnet per group of GEMM_RAGGED_MAX slots.
int xdtts_tacotron2::postnet_groups(const float *frames_dev, size_t frame_stride, const int *Fs, const int *order, int B, bool per_chunk) {
  std::vector<int> F(B);  // frames per caller index
  int total = 0;
  for (int j = 0; j < B; ++j) {
    F[order ? order[j] : j] = Fs[j];
    total += Fs[j];
  }
  // (In a sequence the vocoder of the PREVIOUS utterance may still be reading mel_dev on its own stream when this runs for the next
  // one.  DevBuf::alloc only ever grows: the buffer is kept unless this utterance is longer than every one before it, and then the
  // hipFree inside it synchronises the whole device before the old buffer goes -- correct, at the price of that one overlap.  The
  // post-net's own writes into a kept buffer are ordered behind the vocoder by the event the frame loop waits for, before_decoder.)
  mel_dev.alloc((size_t)N_MEL * total);
  std::vector<long> col0(B), col(B);  // the final mel keeps the caller's chunk order on the time axis (mod.rs:430)
  long off = 0;
  for (int b = 0; b < B; ++b) {
    col0[b] = off;
    off += F[b];
  }
  for (int j = 0; j < B; ++j) col[j] = (per_chunk ? N_MEL : 1) * col0[order ? order[j] : j];
  for (int b = 0; b < B; b += GEMM_RAGGED_MAX) {
    const int n = std::min(GEMM_RAGGED_MAX, B - b);
    run_postnet(frames_dev + (size_t)b * frame_stride, frame_stride, Fs + b, col.data() + b, n, mel_dev.p, total, per_chunk);
  }
  return total;
}

// infer_chunk x B (mod.rs:361-393).  ids_host [B][T] already zero-padded.  Leaves the final mel
// of chunk b at mel_dev + col_off[b] with row stride F_total; returns per-chunk frame counts.
// per_chunk: mel_dev receives one dense (80 x F_b) matrix per chunk instead, back to back in the caller's order.
std::vector<int> xdtts_tacotron2::infer_batch_device(const int64_t *ids_host, const int *lens, int B, int T, const xdtts_infer_opts &o,
                                                     const int *fixed_per_item, int *F_total, bool per_chunk, const DurAsk &dur) {
  dur_n_utt = dur_pending = 0;  // (what last_durations reports of a call that captures nothing, or fails: zero utterances)
  if (B <= 0 || B > 4096) fail(XDTTS_ERR_BAD_ARG, "batch %d out of range", B);
  if (T <= 0 || T > T_MAX) fail(XDTTS_ERR_BAD_ARG, "window %d out of range (1..%d)", T, T_MAX);
  if (o.max_steps <= 0 || o.max_steps > 100000) fail(XDTTS_ERR_BAD_ARG, "max_steps %d out of range", o.max_steps);
  for (int b = 0; b < B; ++b) {
    if (lens[b] <= 0) fail(XDTTS_ERR_BAD_ARG, "chunk %d is empty", b);
    if (lens[b] > T) fail(XDTTS_ERR_TOO_LONG, "chunk %d has %d ids, window is %d", b, lens[b], T);
    for (int t = 0; t < T; ++t) {
      const int64_t id = ids_host[(size_t)b * T + t];
      if (id < 0 || id >= N_SYMBOLS) fail(XDTTS_ERR_BAD_ARG, "id %lld out of range (0..%d)", (long long)id, N_SYMBOLS - 1);
    }
  }
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipEventRecord(ev.e[0], stream));
  // Step caps per chunk, then (batched mode) the lock-step order: longest first, so that the chunks
  // still running always fill a prefix of the 16-chunk MFMA tiles and finished tiles are skipped.
  // order[j] = caller's index of the chunk decoded in slot j; everything below works on slots.
  std::vector<int> lim0(B), order(B);
  for (int b = 0; b < B; ++b) {
    int l = o.max_steps;
    if (fixed_per_item) l = fixed_per_item[b];
    else if (o.fixed_steps > 0) l = o.fixed_steps;
    else if (o.fixed_frames_per_id > 0.f) l = (int)std::lround((double)o.fixed_frames_per_id * lens[b]);
    lim0[b] = std::min(std::max(l, 1), o.max_steps);
    order[b] = b;
  }
  upload_dropout_masks(o, B, lim0.data());  // (caller's chunk order: a sorted batch finds its masks through item_perm)
  const bool gate_off = fixed_per_item || o.fixed_steps > 0 || o.fixed_frames_per_id > 0.f;
  // (3..8 chunks on the persistent MFMA engine keep the row-major state of the small-batch engines and the caller's order)
  bool batched_mode = B >= BATCH_MFMA_MIN;
  if (batched_mode) {  // (a smaller batch asks, and counts, in run_decoder: a demoted handle counts a request once)
    const int max_lim = *std::max_element(lim0.begin(), lim0.end());
    small_batch_tick(B, T, max_lim);
    batched_mode = !small_batch_engine(B, T, max_lim);
  }
  if (batched_mode)
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) {
      return gate_off ? lim0[a] > lim0[c] : lens[a] > lens[c];  // with the gate on, length is the proxy for duration
    });
  std::vector<int64_t> ids_sorted((size_t)B * T);
  std::vector<int> lens_sorted(B), lim(B);
  for (int j = 0; j < B; ++j) {
    std::copy(ids_host + (size_t)order[j] * T, ids_host + (size_t)(order[j] + 1) * T, ids_sorted.begin() + (size_t)j * T);
    lens_sorted[j] = lens[order[j]];
    lim[j] = lim0[order[j]];
  }
  ids_host = ids_sorted.data();
  lens = lens_sorted.data();
  {  // ids, lengths, step caps and (batched mode) the dropout-stream order: one pinned block, one copy (it was four of 4-5 us
     // each, with the host's enqueue time in front of every one of them at the start of a request)
    const size_t b_ids = sizeof(int64_t) * (size_t)B * T, b_int = sizeof(int) * (size_t)B, need = b_ids + 3 * b_int;
    if (need > in_host_bytes) {
      if (in_host) (void)hipHostFree(in_host);
      in_host = nullptr;
      in_host_bytes = 0;
      HIP_CHECK(hipHostMalloc((void **)&in_host, need, hipHostMallocDefault));
      in_host_bytes = need;
    }
    std::memcpy(in_host, ids_host, b_ids);
    std::memcpy(in_host + b_ids, lens, b_int);
    std::memcpy(in_host + b_ids + b_int, lim.data(), b_int);
    std::memcpy(in_host + b_ids + 2 * b_int, order.data(), b_int);
    in_blk.alloc(need);
    HIP_CHECK(hipMemcpyAsync(in_blk.p, in_host, need, hipMemcpyHostToDevice, stream));  // (run_decoder's final wait is behind it)
    ids.p = reinterpret_cast<int64_t *>(in_blk.p);
    n_valid.p = reinterpret_cast<int *>(in_blk.p + b_ids);
    limits.p = reinterpret_cast<int *>(in_blk.p + b_ids + b_int);
    item_perm.p = reinterpret_cast<int *>(in_blk.p + b_ids + 2 * b_int);
    lim_on_dev = lim;
  }
  std::lock_guard<ChipLock> chip(chip_mutex(device));  // released after run_decoder's final wait
  run_encoder(B, T);
  HIP_CHECK(hipEventRecord(ev.e[1], stream));
  // (the cooperative BiLSTM's error word comes back with the decoder's own final fetch: same block, same copy)
  if (batched_mode) w.ensure_batched_layout(blob, stream);
  if (before_decoder) before_decoder();  // (xdtts_synthesize_sequence: the frame loop waits for the previous utterance's vocoder)
  DecoderBufs d = decoder_bufs(B, T, memory.p, pmem.p, o, batched_mode ? 1 : 0);
  if (batched_mode) d.item_perm = item_perm.p;
  if (fixed_per_item || o.fixed_frames_per_id > 0.f) d.use_gate = 0;
  // everything behind the decoder: frame counts -> column offsets -> post-net.  A gate-less decode on the persistent
  // engine enqueues it BEFORE the sync that fetches the counts (they are the caps), see run_decoder.
  std::vector<int> Fs(B), F(B);  // frames per slot / per caller index
  int total = 0;
  auto postnet_all = [&](const int *frames_per_slot) {
    HIP_CHECK(hipEventRecord(ev.e[2], stream));
    for (int j = 0; j < B; ++j) {
      Fs[j] = frames_per_slot[j];
      F[order[j]] = Fs[j];
    }
    total = postnet_groups(d.frames, (size_t)d.max_steps * N_MEL, Fs.data(), order.data(), B, per_chunk);
    HIP_CHECK(hipEventRecord(ev.e[3], stream));
  };
  bool postnet_done = false;
  last_steps = run_decoder(d, lim, [&] { postnet_all(lim.data()); }, &postnet_done);  // (the decoder has finished; the post-net may be running)
  if (host_ctl[HOST_ENC_ERR] != 0) {
    postnet_done = false;
    HIP_CHECK(hipMemsetAsync(enc_err.p, 0, sizeof(int), stream));
    // the 4-CU cooperative BiLSTM needs its workgroups co-resident too: same policy as the decoder --
    // say so, use the single-workgroup recurrence from now on, and run the request again
    enc_gate.demote();
    std::fprintf(stderr, "libxdtts_hip: encoder BiLSTM exchange timed out (grid not co-resident); "
                         "this handle now uses the single-workgroup recurrence\n");
    run_encoder(B, T);
    // batched mode attends over the [B][32][T][4] transpose of processed_memory, written by decoder_bufs() from the
    // timed-out encoder's output: redo it from the fresh one
    if (d.pmem_t) launch_dimgroup_transpose(pmem.p, pmem_t.p, B, T, stream);
    last_steps = run_decoder(d, lim);
  }
  // the durations stage, behind the decode that stands: the final attention_weights_cum of every slot is in HBM, the frame
  // counts and id counts too -- two small launches and one copy, brought down by the entry's final synchronisation
  if (dur.entry && (dur.force || dur_opts.on))
    enqueue_durations(d.awc, d.awc2, d.nframes, d.n_valid, B, T, lens, order.data(), batched_mode, dur.utt_of_chunk, dur_opts);
  if (!postnet_done) postnet_all(host_ctl + HOST_NF);
  *F_total = total;
  return F;
}

static void grow_pinned(unsigned char *&p, size_t &have, size_t need) {
  if (need <= have) return;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  have = 0;
  HIP_CHECK(hipHostMalloc((void **)&p, need, hipHostMallocDefault));
  have = need;
}

void xdtts_tacotron2::enqueue_durations(const float *cum_a, const float *cum_b, const int *nframes_dev, const int *n_valid_dev, int B, int T,
                                        const int *n_valid_host, const int *order, bool batched, const int *utt_of_chunk,
                                        const xdtts::DurationsOpts &o) {
  DurPlan plan;
  const std::string bad = durations_plan(B, T, nullptr, n_valid_host, order, batched ? 1 : 0, cum_b != nullptr, utt_of_chunk, &plan);
  if (!bad.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", bad.c_str());
  const size_t U = plan.utt.size(), N = plan.n_ids;
  const size_t b_chunk = sizeof(DurChunk) * (size_t)B, b_utt = sizeof(DurUtt) * U, b_list = sizeof(int32_t) * (size_t)B;
  grow_pinned(dur_tab_host, dur_tab_host_bytes, b_chunk + b_utt + b_list);
  std::memcpy(dur_tab_host, plan.chunk.data(), b_chunk);
  std::memcpy(dur_tab_host + b_chunk, plan.utt.data(), b_utt);
  std::memcpy(dur_tab_host + b_chunk + b_utt, plan.list.data(), b_list);
  dur_tab_dev.alloc(b_chunk + b_utt + b_list);
  HIP_CHECK(hipMemcpyAsync(dur_tab_dev.p, dur_tab_host, b_chunk + b_utt + b_list, hipMemcpyHostToDevice, stream));
  const size_t b_out = 8 * N + sizeof(AlignmentStats) * U + 8 * N;
  grow_pinned(dur_out_host, dur_out_host_bytes, b_out);
  dur_out_dev.alloc(b_out);
  DurationsJob job{};
  job.cum_a = cum_a;
  job.cum_b = batched ? cum_b : cum_a;
  job.B = B;
  job.T = T;
  job.batched = batched ? 1 : 0;
  job.n_utt = (int)U;
  job.nframes = nframes_dev;
  job.n_valid = n_valid_dev;
  job.tab = reinterpret_cast<const DurChunk *>(dur_tab_dev.p);
  job.utt = reinterpret_cast<const DurUtt *>(dur_tab_dev.p + b_chunk);
  job.list = reinterpret_cast<const int *>(dur_tab_dev.p + b_chunk + b_utt);
  job.lo_q16 = durations_q16(o.min_frames);
  job.hi_q16 = durations_q16(o.max_frames);
  job.start_q16 = reinterpret_cast<uint64_t *>(dur_out_dev.p);
  job.stats = reinterpret_cast<AlignmentStats *>(dur_out_dev.p + 8 * N);
  job.dur = reinterpret_cast<float *>(dur_out_dev.p + 8 * N + sizeof(AlignmentStats) * U);
  job.dur_q16 = reinterpret_cast<uint32_t *>(job.dur + N);
  launch_durations(job, stream);
  HIP_CHECK(hipMemcpyAsync(dur_out_host, dur_out_dev.p, b_out, hipMemcpyDeviceToHost, stream));
  if (!dur_ev) HIP_CHECK(hipEventCreateWithFlags(&dur_ev, hipEventDisableTiming));
  HIP_CHECK(hipEventRecord(dur_ev, stream));
  dur_plan = std::move(plan);
  dur_pending = U;  // (published by the entry, behind its final synchronisation: publish_durations)
}

void xdtts_tacotron2::wait_durations() {
  if (!dur_pending || !dur_ev) fail(XDTTS_ERR_HIP, "durations: nothing was captured");
  HIP_CHECK(hipEventSynchronize(dur_ev));
}

// the cooperative BiLSTM bounds its spins; a timeout there must not pass silently
void xdtts_tacotron2::check_encoder_exchange() {
  if (fetch_and_clear_error_word(enc_err.p, stream)) {
    enc_gate.demote();
    fail(XDTTS_ERR_HIP, "encoder BiLSTM hidden-state exchange timed out (retry uses the single-workgroup recurrence)");
  }
}

void xdtts_tacotron2::finish_timings() {
  HIP_CHECK(hipStreamSynchronize(stream));
  for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&last_ms[i], ev.e[i], ev.e[i + 1]));
  HIP_CHECK(hipEventElapsedTime(&last_ms[3], ev.e[0], ev.e[3]));
}

namespace xdtts {

void chunks_from_splits(const int64_t *ids, size_t n, const size_t *splits, size_t n_splits, int T,
                        std::vector<int64_t> &padded, std::vector<int> &lens) {
  if (!ids || n == 0) fail(XDTTS_ERR_BAD_ARG, "empty id sequence");
  std::vector<size_t> ends;
  if (splits && n_splits) ends.assign(splits, splits + n_splits);
  if (ends.empty() || ends.back() != n) ends.push_back(n);  // mod.rs:412-414
  size_t start = 0;
  for (size_t e : ends) {
    if (e < start || e > n) fail(XDTTS_ERR_BAD_ARG, "splits must be ascending offsets into ids");
    if (e == start) continue;
    const size_t len = e - start;
    if ((int)len > T) fail(XDTTS_ERR_TOO_LONG, "chunk of %zu ids exceeds the %d-id window", len, T);  // mod.rs:363
    lens.push_back((int)len);
    const size_t base = padded.size();
    padded.resize(base + (size_t)T, 0);  // pad id 0 = Unit::Padding, mod.rs:369-371
    std::copy(ids + start, ids + e, padded.begin() + (long)base);
    start = e;
  }
}

std::vector<int64_t> pad_batch_ids(const int64_t *ids, const int32_t *lens, int B, int t_stride, int T) {
  std::vector<int64_t> padded((size_t)B * T, 0);
  for (int b = 0; b < B; ++b) {
    if (lens[b] > T) fail(XDTTS_ERR_TOO_LONG, "chunk %d has %d ids, window is %d", b, lens[b], T);
    if (lens[b] > t_stride || lens[b] <= 0) fail(XDTTS_ERR_BAD_ARG, "chunk %d: bad length %d", b, lens[b]);
    std::copy(ids + (size_t)b * t_stride, ids + (size_t)b * t_stride + lens[b], padded.begin() + (size_t)b * T);
  }
  return padded;
}

xdtts_infer_opts resolve_opts(const xdtts_infer_opts *opts) {
  xdtts_infer_opts o;
  xdtts_infer_opts_default(&o);
  if (opts) o = *opts;
  if (o.max_chunk <= 0) o.max_chunk = 100;
  return o;
}

}  // namespace xdtts
