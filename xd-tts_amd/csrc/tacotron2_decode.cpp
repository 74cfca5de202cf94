// tacotron2_decode.cpp -- run_decoder: the frame loop (mod.rs:302-342) for B chunks in lock-step, served by the first of three
// engines that takes the request.  3..16 chunks: the persistent MFMA engine (decoder_persistent8.hip: 4 / 8 chunk slots,
// decoder_persistent16.hip: 16), one launch for the whole loop.  1..4 chunks: the persistent weight-stationary kernel
// (decoder_persistent.hip) when its 256-workgroup grid can be co-resident.  Everything else, every request after
// XDTTS_DECODER=launch, and every request an engine gave up (a timed-out exchange, a refused launch): the launch-per-stage engine.
#include <algorithm>

#include "tacotron2_handle.h"

using namespace xdtts;

// `after` (may be empty): work that only needs the frame COUNTS of a gate-less decode -- known beforehand: every chunk
// runs to its cap -- enqueued behind the persistent launches and ahead of the sync that fetches error word and counts,
// so the stream does not idle for that round trip (~90 us of the 7.7 ms headline utterance).  `*after_ran` tells the
// caller whether what `after` enqueued stands: not when the engine faulted and the request was decoded again.
struct xdtts_tacotron2::Decode {
  const DecoderBufs &d;
  const std::vector<int> &lim;  // per-chunk step caps (host)
  int max_lim;
  const std::function<void()> *after;  // null unless the decode is gate-less
  bool spec_ran;                       // `after` has been enqueued behind the current attempt
  bool *after_ran;
};

// Returns the number of lock-step iterations executed; host_ctl[HOST_NF + b] = frames of chunk b.
int xdtts_tacotron2::run_decoder(const DecoderBufs &d, const std::vector<int> &lim, const std::function<void()> &after, bool *after_ran) {
  if (after_ran) *after_ran = false;
  if (lim_on_dev != lim || !limits.p) {
    limits.upload(lim.data(), lim.size(), stream);
    lim_on_dev = lim;
  }
  launch_decoder_init(d, limits.p, stream);
  launch_decoder_prologue(d, w, stream);
  Decode dc{d, lim, *std::max_element(lim.begin(), lim.end()), after && !d.use_gate ? &after : nullptr, false, after_ran};
  // an engine answers with the steps it ran, or -1: not its request, or it gave the request up and left the state re-initialised.
  // A cooperative launch the runtime refused: that engine is off for good, the request goes on to the next one.
  auto attempt = [&](int (xdtts_tacotron2::*engine)(Decode &), void (xdtts_tacotron2::*refused)()) {
    try {
      return (this->*engine)(dc);
    } catch (const CoopRefused &) {
      (this->*refused)();
      return decode_again(dc, true);
    }
  };
  int steps = attempt(&xdtts_tacotron2::decode_small_batch, &xdtts_tacotron2::small_batch_refused);
  if (steps < 0) steps = attempt(&xdtts_tacotron2::decode_pairs, &xdtts_tacotron2::pairs_refused);
  if (steps < 0) steps = decode_launches(dc);
  return steps;
}

// step counter, error words and frame counts to the host in one copy; the last fetch of a decode lets `after` enqueue its work
// for a gate-less decode before the host waits (for the copies only)
void xdtts_tacotron2::fetch(Decode &dc, bool last) {
  HIP_CHECK(hipMemcpyAsync(host_ctl, ctlblk.p, sizeof(int) * (size_t)(HOST_NF + dc.d.B), hipMemcpyDeviceToHost, stream));
  if (last && dc.after) {
    HIP_CHECK(hipEventRecord(fetched, stream));
    (*dc.after)();
    dc.spec_ran = true;
    if (while_decoding) while_decoding();
    HIP_CHECK(hipEventSynchronize(fetched));
  } else {
    if (last && while_decoding) while_decoding();
    HIP_CHECK(hipStreamSynchronize(stream));
  }
}

// frame counts are on the host: lock-step iterations; does what `after` enqueued stand?
int xdtts_tacotron2::finish(Decode &dc) {
  int steps = 0;
  bool as_planned = true;
  for (int b = 0; b < dc.d.B; ++b) {
    steps = std::max(steps, host_ctl[HOST_NF + b]);
    as_planned = as_planned && host_ctl[HOST_NF + b] == dc.lim[b];
  }
  if (dc.after_ran) *dc.after_ran = dc.spec_ran && as_planned;
  return steps;
}

// An engine gave the request up (not silent, not fatal: it has said so on stderr): the error word is cleared and the request
// starts again from the initial state.  What `after` enqueued ran on a failed decode: it is enqueued again by the next engine.
// `refused`: the launch never ran -- what the attempt had enqueued before it drains first.
int xdtts_tacotron2::decode_again(Decode &dc, bool refused) {
  dc.spec_ran = false;
  if (refused) HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipMemsetAsync(dec_err.p, 0, sizeof(int), stream));
  launch_decoder_init(dc.d, limits.p, stream);
  return -1;
}

// ---- 3..16 chunks: the persistent MFMA engine ---------------------------------------------------------------------------------
// (its exchange holds one slab per step, 11.3 kB per chunk slot: a request capped at more than 16384 steps -- 190 s of speech --
// takes the other engines rather than gigabytes of ring)
bool xdtts_tacotron2::small_batch_eligible(int B, int T, int max_steps) const {
  if (B < 3 || B > P8_B_MAX || T > PERSIST_T_MAX || max_steps > P8_STEPS_MAX) return false;
  return !env::equals(env::DECODER, "launch");
}
bool xdtts_tacotron2::small_batch_engine(int B, int T, int max_steps) {
  if (!small_batch_eligible(B, T, max_steps)) return false;
  p8_gate.ensure_probed([&] {
    return p8_wanted && decoder_p8_supported(device, 8, PERSIST_T_MAX) && decoder_p8_supported(device, P8_B_MAX, PERSIST_T_MAX);  // (the 8- and the 16-slot kernel)
  });
  return p8_gate.usable() && pair_gate.state != EngineGate::OFF;  // it shares the pair engine's fate
}
// one eligible request: like the pair engine, the cause of a timed-out exchange (another process holding CUs) may be transient
void xdtts_tacotron2::small_batch_tick(int B, int T, int max_steps) {
  if (!small_batch_eligible(B, T, max_steps)) return;
  (void)small_batch_engine(B, T, max_steps);  // (probed before it counts)
  if (p8_gate.tick() && pair_gate.state == EngineGate::OFF && pair_gate.probe_ok) {  // (they were demoted together)
    pair_gate.state = EngineGate::ON;
    pair_gate.demoted_calls = 0;
  }
}

int xdtts_tacotron2::decode_small_batch(Decode &dc) {
  const DecoderBufs &d = dc.d;
  if (d.xf) return -1;
  small_batch_tick(d.B, d.T, dc.max_lim);
  if (!small_batch_engine(d.B, d.T, dc.max_lim)) return -1;
  try {
    dec_exchange.alloc(p8_exchange_words(d.B, dc.max_lim));  // 11.3 kB per chunk slot and step: 90 MB at 8 slots x 1000 steps
  } catch (const Error &e) {
    if (e.code != XDTTS_ERR_OOM) throw;
    (void)hipGetLastError();
    return -1;  // no room for the ring: this request takes the other engines (whose exchange is 63 kB per chunk)
  }
  std::lock_guard<ChipLock> lk(chip_mutex(device));
  P8Bufs g8 = p8_bufs(dec_exchange.p, dec_err.p, d.B, dc.max_lim);
  env::override_int(env::PERSIST_SPINS, &g8.spins);  // test hooks for the lost-workgroup path
  env::override_int(env::PERSIST_FAULT, &g8.fault);
  launch_p8_seed(d, g8, limits.p, stream);
  launch_decoder_p8(d, w, g8, dc.max_lim, stream);
  fetch(dc, true);
  if (!host_ctl[HOST_DEC_ERR]) return finish(dc);
  // the 256-workgroup grid was not co-resident: the pair-persistent engine, which needs the same, would spend a second
  // 2^21-spin time-out finding that out -- both are demoted, both are probed again after PROBE_AFTER requests.  The
  // request runs again on the launch-per-stage engine (row-major state, any B <= 8).
  p8_gate.demote();
  pair_gate.ensure_probed([&] { return decoder_persistent_supported(device, PERSIST_B_MAX, PERSIST_T_MAX); });
  pair_gate.demote();
  std::fprintf(stderr, "libxdtts_hip: persistent MFMA decoder exchange timed out (grid not co-resident); this handle now "
                       "uses the launch-per-stage decoder (probed again after %d calls)\n", EngineGate::PROBE_AFTER);
  return decode_again(dc, false);
}
void xdtts_tacotron2::small_batch_refused() {  // (the pair engine is left alone)
  p8_gate.refuse();
  std::fprintf(stderr, "libxdtts_hip: persistent MFMA decoder launch refused by the runtime; this handle decodes small batches "
                       "with its other engines\n");
}

// ---- 1..4 chunks: the pair-persistent engine ------------------------------------------------------------------------------------
bool xdtts_tacotron2::use_persistent(const DecoderBufs &d) {
  if (d.xf || d.B > 2 * PERSIST_B_MAX || d.T > PERSIST_T_MAX) return false;  // 3..4 chunks: two launches of <= 2
  if (env::equals(env::DECODER, "launch")) return false;
  pair_gate.ensure_probed([&] { return decoder_persistent_supported(device, PERSIST_B_MAX, PERSIST_T_MAX); });
  // a timed-out exchange demotes the handle; the cause (another process holding CUs) may be transient, so
  // the persistent engine gets another try every PROBE_AFTER calls (xdtts_tacotron2_engine_reset: at once)
  pair_gate.tick();
  return pair_gate.usable();
}

int xdtts_tacotron2::decode_pairs(Decode &dc) {
  const DecoderBufs &d = dc.d;
  const std::vector<int> &lim = dc.lim;
  if (!use_persistent(d)) return -1;
  // one launch for the whole loop: the stop rule runs on the device and the kernel ends by itself.
  // Its grid must own the chip, so persistent launches of different handles never overlap.
  std::lock_guard<ChipLock> lk(chip_mutex(device));
  // Chunks are independent, so 3 or 4 of them run as two launches of <= 2 over views of the
  // state arrays (measured: 2 x 15.4 us per step-pair against 37 us per step of the launch path).
  // A 2-chunk launch ends when its first chunk stops and the other is continued by the 1-chunk
  // kernel (~1 us per step faster): the state crosses through the kernel's write-back, x(s)
  // stays in the exchange.
  // The context columns of every LSTM / projection row against the encoder memory, once per request (a GEMM of
  // 0.85 GFLOP per chunk) instead of a 33 us fold loop per chunk in each of the request's launches.
  const float *fold = nullptr;
  if (ctx_fold_table && w.ctx_w.p) {
    ctx_fold.alloc((size_t)d.B * CTXF_ROWS * CTXF_LD);
    GemmArgs fg{};
    fg.A = d.memory;
    fg.lda = EMB;
    fg.strideA = (long)d.T * EMB;
    fg.W = w.ctx_w.p;
    fg.C = ctx_fold.p;
    fg.ldc = CTXF_LD;
    fg.strideC = (long)CTXF_ROWS * CTXF_LD;
    fg.M = d.T;
    fg.N = CTXF_ROWS;
    fg.K = EMB;
    fg.batch = d.B;
    fg.transpose_out = 1;
    launch_gemm_nt(fg, stream);
    fold = ctx_fold.p;
  }
  auto view = [&](int b0, int n) {
    DecoderBufs v = d;
    v.B = n;
    v.ctx_fold = fold ? fold + (size_t)b0 * CTXF_ROWS * CTXF_LD : nullptr;
    v.memory += (size_t)b0 * d.T * EMB;
    v.pmem += (size_t)b0 * d.T * ATT_DIM;
    v.n_valid += b0;
    for (int i = 0; i < 2; ++i) {
      v.att_h[i] = d.att_h[0] + (size_t)b0 * ATT_RNN;  // the persistent kernel keeps h in slot 0 only
      v.dec_h[i] = d.dec_h[0] + (size_t)b0 * DEC_RNN;
    }
    v.att_c += (size_t)b0 * ATT_RNN;
    v.dec_c += (size_t)b0 * DEC_RNN;
    v.aw += (size_t)b0 * d.T;
    v.awc += (size_t)b0 * d.T;
    v.ctx += (size_t)b0 * EMB;
    v.frames += (size_t)b0 * d.max_steps * N_MEL;
    v.gates += (size_t)b0 * d.max_steps;
    v.nframes += b0;
    v.item_base += (uint32_t)b0;
    if (v.drop_masks) v.drop_masks += (size_t)b0 * d.drop_steps * 2 * PRENET;
    return v;
  };
  for (int b0 = 0; b0 < d.B; b0 += PERSIST_B_MAX) {
    const int n = std::min(PERSIST_B_MAX, d.B - b0);
    const DecoderBufs v = view(b0, n);
    int sub_lim = 0;
    for (int b = 0; b < n; ++b) sub_lim = std::max(sub_lim, lim[b0 + b]);
    dec_exchange.alloc(persist_granule_words(n));
    PersistBufs g = persist_bufs(dec_exchange.p, dec_err.p, n);
    if (!pair_skew) g.skew = 0;
    env::override_int(env::PERSIST_SPINS, &g.spins);  // test hooks for the
    env::override_int(env::PERSIST_FAULT, &g.fault);  // lost-workgroup path
    env::override_int(env::PERSIST_SLOW, &g.slow);    // straggler workgroup
    g.shrink = n == 2 ? 1 : 0;
    if (g.shrink && !d.use_gate && lim[b0] == lim[b0 + 1]) {
      // gate-less pair with equal caps: the host knows that neither chunk outlives the other, so no continuation launches
      // (each would do the full weight / LDS set-up and write-back for zero steps)
      g.shrink = 0;
      g.both_run = 1;
    }
#ifdef XDTTS_PERSIST_PROFILE
    static DevBuf<unsigned long long> prof;
    prof.alloc(256 * 24);
    g.prof = prof.p;
#endif
    if (b0 > 0) HIP_CHECK(hipMemsetAsync(d.ctl, 0, sizeof(int), stream));  // step counter of the new launch
    launch_persist_seed(v, g, limits.p + b0, stream);
    if (g.shrink && !d.use_gate && lim[b0] != lim[b0 + 1]) {
      // without the gate the host knows which chunk outlives the other: no round trip in between
      const int first = std::min(lim[b0], lim[b0 + 1]), r = lim[b0] > lim[b0 + 1] ? 0 : 1;
      g.shrink = 0;
      g.both_run = 1;  // (neither chunk stops inside these `first` steps: the skewed loop may run them)
      launch_decoder_persistent(v, w, g, first, stream);
      launch_decoder_persistent(view(b0 + r, 1), w, persist_view(g, r), lim[b0 + r] - first, stream);
    } else {
      launch_decoder_persistent(v, w, g, sub_lim, stream);
      if (g.shrink) {
        // Which chunk, if any, is still running is on the device (ctl[0] = steps executed, nframes[b] = its end): rather than
        // ask (a stream sync and two copies, ~0.1 ms of an 6.7 ms utterance) the continuation of BOTH chunks is enqueued --
        // the 1-chunk kernel returns at once for a chunk that has stopped (at most one survives the other; a survivor that
        // runs first leaves ctl[0] at its own end, which is past the other's), and stops by itself at the chunk's cap.
        for (int r = 0; r < n; ++r) {
          PersistBufs g1 = persist_view(g, r);
          g1.shrink = 0;
          launch_decoder_persistent(view(b0 + r, 1), w, g1, lim[b0 + r], stream);
        }
      }
    }
#ifdef XDTTS_PERSIST_PROFILE
    if (const char *path = env::raw(env::PERSIST_PROFILE)) {
      std::vector<unsigned long long> hp(256 * 24);
      HIP_CHECK(hipMemcpyAsync(hp.data(), prof.p, hp.size() * 8, hipMemcpyDeviceToHost, stream));
      HIP_CHECK(hipStreamSynchronize(stream));
      if (FILE *f = fopen(path, "w")) {
        for (int c = 0; c < 256; ++c) {
          for (int i = 0; i < 24; ++i) fprintf(f, "%llu ", hp[c * 24 + i]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
#endif
  }
  fetch(dc, true);
  if (!host_ctl[HOST_DEC_ERR]) return finish(dc);
  // A bounded spin ran out: the 256-workgroup grid was not co-resident (CUs masked or held by
  // another process).  Not silent, not fatal: say so, switch this handle to the launch-per-stage
  // engine, and decode this request again from the initial state.
  pair_gate.demote();
  std::fprintf(stderr, "libxdtts_hip: persistent decoder exchange timed out (grid not co-resident); "
                       "this handle now uses the launch-per-stage decoder (probed again after %d calls)\n", EngineGate::PROBE_AFTER);
  return decode_again(dc, false);
}
// the runtime refused the cooperative grid: this device cannot host the persistent engine (not a transient, so no
// re-probe); the request is decoded on the launch-per-stage engine
void xdtts_tacotron2::pairs_refused() {
  pair_gate.refuse();
  std::fprintf(stderr, "libxdtts_hip: persistent decoder launch refused by the runtime; this handle uses the "
                       "launch-per-stage decoder\n");
}

// ---- the launch-per-stage engine ------------------------------------------------------------------------------------------------
// Replays a hipGraph holding GRAPH_STEPS decoder steps.  The kernels read the step index from device memory, so one graph
// serves every position of the loop.
void xdtts_tacotron2::replay_steps(const DecoderBufs &d) {
  graph.replay(&d, sizeof d, stream, [&] { launch_decoder_steps(d, w, GRAPH_STEPS, stream); });
}

int xdtts_tacotron2::decode_launches(Decode &dc) {
  const DecoderBufs &d = dc.d;
  const int max_lim = dc.max_lim;
  int launched = 0;
  // the launch that holds the attention LSTM and the attention needs its 256 blocks resident together: like the
  // persistent engine's, such launches of different handles never overlap
  std::unique_lock<ChipLock> chip;
  if (d.hg) chip = std::unique_lock<ChipLock>(chip_mutex(device));
  if (!d.use_gate) {  // deterministic work: every chunk runs to its cap
    while (launched + GRAPH_STEPS <= max_lim) {
      replay_steps(d);
      launched += GRAPH_STEPS;
    }
    if (launched < max_lim) {
      // the last < GRAPH_STEPS steps as plain launches of exactly that many (even) steps: a whole graph would run up to
      // GRAPH_STEPS - 1 steps with no chunk active, three launches of ~3.5 us each (the 647-iteration batch of configs[2]: 13)
      int r = max_lim - launched;
      r += r & 1;
      launch_decoder_steps(d, w, r, stream);
      launched += r;
    }
    launch_decoder_flush(d, w, stream);
    fetch(dc, true);
  } else {
    const int check_every = 3 * GRAPH_STEPS;
    for (;;) {
      for (int i = 0; i < check_every && launched < max_lim; i += GRAPH_STEPS) {
        replay_steps(d);
        launched += GRAPH_STEPS;
      }
      fetch(dc, false);
      int need = 0;
      for (int b = 0; b < d.B; ++b) need = std::max(need, host_ctl[HOST_NF + b]);
      if (host_ctl[0] >= need || launched >= max_lim) break;
    }
    // the projection of step s is completed by the first kernel of step s+1: finish the last one
    launch_decoder_flush(d, w, stream);
    fetch(dc, true);
  }
  if (d.ep_g && host_ctl[HOST_DEC_ERR]) {  // a block of the one-launch attention never saw its neighbours' energies: not silent, not fatal
    HIP_CHECK(hipMemsetAsync(dec_err.p, 0, sizeof(int), stream));
    att_gate.demote();
    std::fprintf(stderr, "libxdtts_hip: batched attention exchange timed out; this handle now uses the "
                         "separate attention kernels (probed again after %d batches)\n", EngineGate::PROBE_AFTER);
    DecoderBufs d2 = d;
    d2.ep_g = nullptr;
    d2.hg = nullptr;
    d2.att_part = nullptr;
    d2.hdg = d2.melg = nullptr;
    d2.dec_part = nullptr;
    return run_decoder(d2, dc.lim);  // (no `after`: the caller enqueues its work behind this decode)
  }
  return finish(dc);
}
