// tacotron2_handle.h -- the mel-generator handle: weights, workspaces and the engines' fallback gates.  The encoder, the
// post-net and the request path are in tacotron2_handle.cpp, the frame loop's three engines in tacotron2_decode.cpp.
#pragma once
#include <functional>

#include "engine_gate.h"
#include "kernels.h"
#include "runtime.h"

namespace xdtts {
// What an entry asks of infer_batch_device about the durations stage: entry = one of the entries the setting covers (the sequence
// and document entries are not: they pass nothing, capture nothing, and the last result is cleared), force = capture whatever the
// setting says (the id-anchored contour entries), utt_of_chunk [B] in the caller's order (nullptr: every chunk an utterance of
// its own).
struct DurAsk {
  bool entry = false, force = false;
  const int *utt_of_chunk = nullptr;
};
}  // namespace xdtts

struct xdtts_tacotron2 {
  using DecoderBufs = xdtts::DecoderBufs;
  using EngineGate = xdtts::EngineGate;
  template <class T>
  using DevBuf = xdtts::DevBuf<T>;
  int device = 0;
  hipStream_t stream = nullptr;
  mutable std::mutex mu;
  std::vector<float> blob;  // canonical weights (host), for save/get_tensor
  xdtts::DeviceWeights w;
  xdtts::Events ev;
  float last_ms[4] = {0, 0, 0, 0};
  int last_steps = 0;

  // workspaces (grown on demand)
  // an input array on the device: either its own allocation (upload) or a view into the request's one staged block (infer_batch_device)
  template <class T>
  struct DevSlot {
    T *p = nullptr;
    DevBuf<T> own;
    void upload(const T *src, size_t count, hipStream_t s) {
      own.upload(src, count, s);
      p = own.p;
    }
  };
  DevSlot<int64_t> ids;
  DevSlot<int> n_valid, limits;
  DevBuf<unsigned char> in_blk;       // ids | lens | step caps | dropout-stream order of one request: ONE host-to-device copy
  unsigned char *in_host = nullptr;   // pinned staging of the same
  size_t in_host_bytes = 0;
  std::vector<int> lim_on_dev;        // the step caps limits.p holds (run_decoder uploads them only when they differ)
  // One control block on the device, mirrored by host_ctl: [0..1] ctl (step counter, spare), [2] encoder error word, [3] decoder
  // error word, [4 ..] frames per chunk -- so that what a decode hands back to the host is ONE copy (it was three of 4-5 us each)
  struct IntRef {
    int *p = nullptr;
  };
  DevBuf<int> ctlblk;
  IntRef ctl, enc_err, dec_err, nframes;
  DevBuf<float> xpadA, xpadB, xproj, memory, pmem;
  const float *xpad_zero[2] = {nullptr, nullptr};  // the allocations and layout whose padding rows are known to be zero
  int xpad_B = 0, xpad_T = 0;
  DevBuf<unsigned long long> enc_exchange;
  DevBuf<unsigned long long> dec_exchange;  // granule buffers of the persistent decoder
  DevBuf<float> ctx_fold;                   // [B][CTXF_ROWS][CTXF_LD] context-fold table of the persistent decoder (kernels.h)
  DevBuf<unsigned long long> att_exchange;
  DevBuf<float> att_part;  // early partial pre-activations of the attention LSTM (DecoderBufs::att_part)
  DevBuf<float> dec_part;  // two-launch form: early partial of the decoder LSTM's h_dec columns (DecoderBufs::dec_part)
  DevBuf<unsigned long long> tail_exchange;  // two-launch form: h_dec and mel granules (DecoderBufs::hdg, melg)
  int n_cu = 0;
  // The fallback gates (engine_gate.h).  What the ABI reports of them: xdtts_tacotron2_engine_state, _small_batch_engine_state.
  EngineGate pair_gate;  // the pair-persistent decoder (decoder_persistent.hip): 1..4 chunks as launches of <= 2
  EngineGate p8_gate;    // the persistent MFMA decoder (decoder_persistent8.hip / 16.hip): 3..16 chunks, one launch for the whole loop
  EngineGate enc_gate;   // the cooperative encoder BiLSTM (nothing to probe: usable until an exchange times out or the launch is refused)
  EngineGate att_gate;   // batched mode: energies, softmax and context in one launch (off: the two-kernel form)
  // XDTTS_ATT_FUSED (read when a handle is created, and again when the gate comes back on): the form of that launch --
  // 2: with the attention LSTM in the same launch, 1: attention alone, 0: two kernels
  int att_form = xdtts::env::int_or(xdtts::env::ATT_FUSED, 2);
  int att_fused() const { return att_gate.state == EngineGate::OFF ? 0 : att_form; }
  // XDTTS_NO_EARLY (read when a handle is created): the attention launch multiplies its whole K instead of adding the early
  // partial of the previous decoder-LSTM launch (second form of the same arithmetic for the agreement test; results agree to 1e-5)
  bool early_partial = !xdtts::env::is_set(xdtts::env::NO_EARLY);
  // XDTTS_NO_CTXFOLD (read when a handle is created): the persistent kernel folds the context columns into the encoder memory
  // itself, in every launch, instead of reading the table one GEMM per request makes (tests compare the two forms)
  bool ctx_fold_table = !xdtts::env::is_set(xdtts::env::NO_CTXFOLD);
  // XDTTS_NO_SKEW (read when a handle is created): pairs of chunks run the persistent kernel's lock-step loop instead of the skewed one
  bool pair_skew = !xdtts::env::is_set(xdtts::env::NO_SKEW);
  // XDTTS_P8=0 (read when a handle is created): 3..8 chunks go to the engines that served them before decoder_persistent8.hip
  bool p8_wanted = [] { const char *p = xdtts::env::raw(xdtts::env::P8); return !(p && p[0] == '0'); }();
  bool two_launch = !xdtts::env::is_set(xdtts::env::NO_TAIL);  // (XDTTS_NO_TAIL: keep the prenet launch; read when a handle is created)
  int coop_group = 16;                      // chunks per cooperative BiLSTM launch: 8 workgroups of 1024 threads per
                                            // chunk must be co-resident, one per CU (set from the CU count in init)
  DevBuf<float> att_h, att_c, dec_h, dec_c, aw, awc, ctx, x, loc, e_part, pmel, frames, gates;
  DevBuf<float> frag;       // batched mode: MFMA-operand copies of x, ctx, att_h[2], dec_h[2]
  DevBuf<float> pmem_t;     // batched mode: processed_memory as [B][32][T][4]
  DevSlot<int> item_perm;    // batched mode: dropout-stream index of the (length-sorted) chunks
  DevBuf<float> dec_in_dev; // parity hook: decoder_input of xdtts_tacotron2_decoder_step
  DevBuf<unsigned char> drop_dev;  // dropout_mode 2: the caller's keep masks
  DevBuf<float> state_stage;       // parity hook: the seven state tensors in the caller's layout
  DevBuf<float> pp0, ppA, ppB, mel_dev;
  std::vector<long> pp_sig;  // layout (items, frames, allocations) whose padding is known to be zero in pp0 / ppA / ppB
  std::function<void()> before_decoder;  // enqueued between the encoder and the frame loop of infer_batch_device (or empty)
  std::function<void()> while_decoding;  // host work for the time the frame loop runs: called once everything of the decode is enqueued, before the host waits for it (or empty)
  int *host_ctl = nullptr;  // pinned mirror of ctlblk: [0..1] ctl, [HOST_ENC_ERR] / [HOST_DEC_ERR] the engines' error words, [HOST_NF ..] nframes
  static constexpr int HOST_ENC_ERR = 2, HOST_DEC_ERR = 3, HOST_NF = 4, CTL_INTS = HOST_NF + 4096;


  // cached hipGraph of GRAPH_STEPS decoder steps for the current (B, T, buffers)
  static constexpr int GRAPH_STEPS = 20;
  xdtts::GraphCache graph;

  // ---- durations (durations.hip, durations_plan.h): per-id timings from attention_weights_cum behind a decode ----
  using DurAsk = xdtts::DurAsk;
  xdtts::DurationsOpts dur_opts = xdtts::durations_default();
  xdtts::DurPlan dur_plan;            // layout of the last capture
  size_t dur_n_utt = 0;               // utterances the last call captured (0: none -- setting off, or an entry outside it)
  size_t dur_pending = 0;             // ... of a capture whose copy is enqueued: published by the entry behind its final synchronisation
  hipEvent_t dur_ev = nullptr;        // behind that copy (the id-anchored contour entries wait for it: they map on the host)
  void publish_durations() { dur_n_utt = dur_pending; dur_pending = 0; }
  void wait_durations();              // until the enqueued capture has landed in the pinned mirror
  DevBuf<unsigned char> dur_tab_dev;  // DurChunk[B] | DurUtt[U] | list[B]
  DevBuf<unsigned char> dur_out_dev;  // start_q16[N] | AlignmentStats[U] | dur[N] | dur_q16[N]
  unsigned char *dur_tab_host = nullptr, *dur_out_host = nullptr;  // pinned: staging of the tables, mirror of the outputs
  size_t dur_tab_host_bytes = 0, dur_out_host_bytes = 0;
  // enqueues the stage and the copy of its outputs on the handle's stream; the entry's final synchronisation brings them down
  void enqueue_durations(const float *cum_a, const float *cum_b, const int *nframes_dev, const int *n_valid_dev, int B, int T,
                         const int *n_valid_host, const int *order, bool batched, const int *utt_of_chunk, const xdtts::DurationsOpts &o);
  const uint64_t *dur_start() const { return reinterpret_cast<const uint64_t *>(dur_out_host); }
  const xdtts::AlignmentStats *dur_stats() const { return reinterpret_cast<const xdtts::AlignmentStats *>(dur_out_host + 8 * dur_plan.n_ids); }
  const float *dur_f32() const { return reinterpret_cast<const float *>(dur_out_host + 8 * dur_plan.n_ids + sizeof(xdtts::AlignmentStats) * dur_plan.utt.size()); }
  const uint32_t *dur_q16() const { return reinterpret_cast<const uint32_t *>(dur_f32() + dur_plan.n_ids); }

  hipEvent_t fetched = nullptr;  // behind the copies that bring error word and frame counts back (run_decoder)
  // every dense contraction of the handle goes through run_gemm: split-K where it pays (gemm.hip: gemm_splitk_plan), the slices'
  // meeting place and the tiles' arrival counters owned by the handle (one stream: launches never overlap)
  DevBuf<float> gemm_ws;
  DevBuf<unsigned> gemm_cnt;

  ~xdtts_tacotron2();
  void init(int dev);
  void run_gemm(xdtts::GemmArgs &g);
  // encoder.onnx (mod.rs:379): ids [B][T] on device -> memory, pmem
  // bilstm: -1 = what the handle's gate says (the request path), 1 / 0 = the parity hook's choice: the cooperative recurrence (a
  // refused launch is an error then) / the single-workgroup one; neither touches the gate
  void run_encoder(int B, int T, int bilstm = -1);
  void upload_dropout_masks(const xdtts_infer_opts &o, int B, const int *lim);
  // force_batched: -1 = by batch size (the MFMA kernels from BATCH_MFMA_MIN chunks), 0 / 1 = the parity hook's choice
  DecoderBufs decoder_bufs(int B, int T, const float *mem, const float *pm, const xdtts_infer_opts &o, int force_batched = -1);
  void run_postnet(const float *frames_dev, size_t frame_stride, const int *F, const long *col_off, int n, float *out, long ldc,
                   bool dense_items = false);
  // the post-net of B chunks in groups of at most GEMM_RAGGED_MAX: slot j has Fs[j] frames at frames_dev + j * frame_stride and is the
  // caller's chunk order[j] (nullptr: j); mel_dev receives the (80 x F_total) matrix in the caller's order, or with per_chunk one dense
  // (80 x F_b) matrix per chunk back to back.  Returns F_total.
  int postnet_groups(const float *frames_dev, size_t frame_stride, const int *Fs, const int *order, int B, bool per_chunk);
  std::vector<int> infer_batch_device(const int64_t *ids_host, const int *lens, int B, int T, const xdtts_infer_opts &o,
                                      const int *fixed_per_item, int *F_total, bool per_chunk = false, const DurAsk &dur = DurAsk());
  void check_encoder_exchange();
  void finish_timings();

  // ---- the frame loop (tacotron2_decode.cpp) ----
  int run_decoder(const DecoderBufs &d, const std::vector<int> &lim, const std::function<void()> &after = {}, bool *after_ran = nullptr);
  bool small_batch_eligible(int B, int T, int max_steps) const;
  void small_batch_tick(int B, int T, int max_steps);
  bool small_batch_engine(int B, int T, int max_steps);
  bool use_persistent(const DecoderBufs &d);

 private:
  struct Decode;  // one request inside run_decoder
  void replay_steps(const DecoderBufs &d);
  void fetch(Decode &dc, bool last);
  int finish(Decode &dc);
  int decode_again(Decode &dc, bool refused);
  int decode_small_batch(Decode &dc);
  int decode_pairs(Decode &dc);
  int decode_launches(Decode &dc);
  void small_batch_refused();
  void pairs_refused();
};

namespace xdtts {
// ids of one utterance cut at `splits` into chunks of at most T ids, each zero-padded to T (mod.rs:361-371, 412-414)
void chunks_from_splits(const int64_t *ids, size_t n, const size_t *splits, size_t n_splits, int T, std::vector<int64_t> &padded,
                        std::vector<int> &lens);
// a caller's [B][t_stride] batch as [B][T], zero-padded
std::vector<int64_t> pad_batch_ids(const int64_t *ids, const int32_t *lens, int B, int t_stride, int T);
xdtts_infer_opts resolve_opts(const xdtts_infer_opts *opts);
}  // namespace xdtts
