/*
 * xdtts.h -- C ABI of libxdtts_hip.so: the MI355X (gfx950) implementation of xd-tts's
 * mel-spectrogram synthesis + vocoding hot path.
 *
 * This is the drop-in boundary.  Every entry point below is what a Rust `extern "C"` block in
 * the reference's src/tacotron2/mod.rs (and a replacement for the `griffin_lim` crate import at
 * src/tacotron2/mod.rs:67-68, src/lib.rs:5) would bind; the reference interface each one
 * replaces is cited as file:line under /root/reference.  INTEGRATION.md shows the Rust shim.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; all floats are IEEE fp32, ids are i64
 *   - every fallible call returns xdtts_status (0 = ok); xdtts_last_error() gives a thread-local
 *     message; no exception or panic crosses this boundary
 *   - handles are opaque, created by *_load / *_new and destroyed by *_free; one handle is bound
 *     to one GPU (device_id) and serialises calls on its own HIP stream
 *   - output buffers returned through `float **` are library-allocated pinned host memory: copy,
 *     then release with xdtts_free()
 *   - mel layout across the boundary is the reference's Array2<f32> (80, F), C order
 *     (src/tacotron2/mod.rs:349-355,430); audio is Vec<f32> (src/lib.rs:141)
 */
#ifndef XDTTS_H
#define XDTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t xdtts_status;
enum {
  XDTTS_OK = 0,
  XDTTS_ERR_BAD_ARG = 1,  /* null pointer, bad shape, id out of range */
  XDTTS_ERR_IO = 2,       /* weight container missing / malformed (anyhow context, mod.rs:249,254,259) */
  XDTTS_ERR_HIP = 3,      /* HIP runtime error */
  XDTTS_ERR_OOM = 4,
  XDTTS_ERR_TOO_LONG = 5, /* a chunk longer than max_chunk: the reference's assert!, mod.rs:363 */
  XDTTS_ERR_NO_DEVICE = 6 /* no gfx950 device: the product path never falls back to the CPU */
};

typedef struct xdtts_tacotron2 xdtts_tacotron2;
typedef struct xdtts_griffinlim xdtts_griffinlim;

/* Decoder options.  Defaults (xdtts_infer_opts_default) are the reference's hard-coded
 * constants: gate_threshold 0.6 and max_steps 1000 (src/tacotron2/mod.rs:279-280), window 100
 * (src/tacotron2/mod.rs:363,369-371,399). */
typedef struct {
  float gate_threshold;
  int32_t max_steps;
  int32_t fixed_steps;   /* 0: stop on the gate (reference behaviour); >0: emit exactly this many
                            frames per chunk (deterministic work for benchmarks/parity) */
  int32_t dropout_mode;  /* 0 off; 1 seeded counter-based masks (the exported decoder graph keeps
                            the prenet's p=0.5 dropout on at inference); 2 explicit: the caller's
                            keep masks (dropout_masks below) */
  uint32_t dropout_seed;
  int32_t max_chunk;     /* encoder window; chunks are zero-padded to exactly this length */
  uint32_t item_base;    /* index of the first chunk in the dropout stream (batch sharding) */
  float fixed_frames_per_id; /* >0 (and fixed_steps == 0): chunk of n ids emits round(n * this)
                            frames -- deterministic work proportional to the chunk length */
  /* dropout_mode 2 (SURVEY.md section 8(b) "explicit(mask ptr)"): keep bytes
   * [chunk][dropout_mask_steps][2 prenet layers][256 units], non-zero = keep (the kept value is
   * doubled, p = 0.5), chunk = index of the chunk within this call, step = frame index.  This is
   * the hook for comparing with ONE recorded run of the real decoder_iter.onnx, whose in-graph
   * RandomUniform draws (src/tacotron2/mod.rs:304) cannot be seeded from outside.  Every chunk's
   * step limit must be <= dropout_mask_steps.  Host memory, read during the call only. */
  const uint8_t *dropout_masks;
  int32_t dropout_mask_steps;
} xdtts_infer_opts;

void xdtts_infer_opts_default(xdtts_infer_opts *opts);

/* ---- Tacotron2 -------------------------------------------------------------------------- */

/* Tacotron2::load(path) -- src/tacotron2/mod.rs:242-267.  `dir` is the reference's model directory:
 * encoder.onnx, decoder_iter.onnx and postnet.onnx (mod.rs:246-259) are read directly (a minimal
 * protobuf reader pulls the weights out of the graphs; nothing of the graphs is executed), or, if
 * present, the flat container `tacotron2.xdtw` written by xdtts_tacotron2_save.  A git-LFS pointer
 * file in place of a graph gives XDTTS_ERR_IO with a message naming `git lfs pull`.
 * What the reader expects of the graphs (torch.onnx.export of the NVIDIA model, csrc/onnx_load.cpp): attention_rnn,
 * decoder_rnn and the encoder BiLSTM as ONNX `LSTM` nodes (the exporter script's LSTMCell -> LSTM form; an LSTMCell
 * decomposed into Gemm/Sigmoid/Tanh is reported as "no LSTM node with input width 768"), convolutions as `Conv` with or
 * without a following `BatchNormalization` (a folded conv is loaded with identity statistics), linear layers as MatMul / Gemm
 * with a constant operand, and the graph input / output names the reference binds (xdtts_model_dir_describe). */
xdtts_status xdtts_tacotron2_load(const char *dir, int32_t device_id, xdtts_tacotron2 **out);

/* device_id of every constructor: a HIP device index, or XDTTS_DEVICE_DEFAULT = the process's default GPU -- environment variable
 * XDTTS_DEVICE (read at every handle creation), 0 without it.  The reference's constructors take no device
 * (`Tacotron2::load(path)`, `GriffinLim::new(..)`, src/lib.rs:40-58): a host that keeps their signatures passes XDTTS_DEVICE_DEFAULT
 * and is spread over the GPUs of a node by one process per GPU with XDTTS_DEVICE = its rank.
 * xdtts_default_device(): what XDTTS_DEVICE_DEFAULT resolves to now, or -1 (XDTTS_DEVICE is not a device index; xdtts_last_error). */
#define XDTTS_DEVICE_DEFAULT (-1)
int32_t xdtts_default_device(void);

/* The host half of Tacotron2::load: reads `dir` (ONNX graphs or tacotron2.xdtw, as above) into a
 * caller-held flat fp32 blob in canonical tensor order (n_floats == xdtts_tensor_total()).  Needs no
 * device; xdtts_tacotron2_load(dir) == this + xdtts_tacotron2_load_blob. */
xdtts_status xdtts_model_dir_read(const char *dir, float *blob, size_t n_floats);

/* The graph inputs / outputs of the three ONNX files of `dir`, one line per file:
 * "decoder_iter.onnx: inputs a,b,.. ; outputs x,y,..\n".  xdtts_tacotron2_load / xdtts_model_dir_read REQUIRE the names the
 * reference binds: the 11 named inputs of src/tacotron2/mod.rs:284-296, the 9 named outputs of :306-307,332-339,
 * `mel_outputs_postnet` (:349), 2 inputs / 3 outputs for the encoder (:379-385) -- XDTTS_ERR_IO otherwise.
 * buf may be NULL with cap 0 to ask for the size (*needed, terminator included). */
xdtts_status xdtts_model_dir_describe(const char *dir, char *buf, size_t cap, size_t *needed);

/* Seeded synthetic weights with the checkpoint's exact shapes. */
xdtts_status xdtts_tacotron2_load_synthetic(uint32_t seed, float rec_scale, int32_t device_id,
                                            xdtts_tacotron2 **out);

/* Weights from a caller-held flat fp32 blob in canonical tensor order (xdtts_tensor_*). */
xdtts_status xdtts_tacotron2_load_blob(const float *blob, size_t n_floats, int32_t device_id,
                                       xdtts_tacotron2 **out);

/* Writes the handle's canonical weights as `dir`/tacotron2.xdtw. */
xdtts_status xdtts_tacotron2_save(const xdtts_tacotron2 *h, const char *dir);

/* Canonical tensor table (names follow the NVIDIA checkpoint the ONNX graphs were exported
 * from, src/tacotron2/mod.rs:137-138). */
int32_t xdtts_tensor_count(void);
const char *xdtts_tensor_name(int32_t i);
int32_t xdtts_tensor_ndim(int32_t i);
int32_t xdtts_tensor_dim(int32_t i, int32_t d);
size_t xdtts_tensor_offset(int32_t i);
size_t xdtts_tensor_total(void);
/* Copies the canonical (un-packed, un-folded) tensor i out of the handle. */
xdtts_status xdtts_tacotron2_get_tensor(const xdtts_tacotron2 *h, int32_t i, float *out);

/* Tacotron2::infer(&[Unit]) -- src/tacotron2/mod.rs:398-437, after the Unit->id mapping
 * (:403-406) and find_splits (:399), which stay on the host side of the FFI (xdtts_host.h).
 * `splits` are the chunk end offsets into ids (ascending, last == n); NULL/0 means one chunk.
 * Each chunk must be <= max_chunk ids (else XDTTS_ERR_TOO_LONG, the reference's assert at :363).
 * Chunks are independent (:422-434): they are decoded together as one batch and concatenated
 * on the time axis (:430).  *mel receives 80 x (*n_frames) floats, C order. */
xdtts_status xdtts_tacotron2_infer_ids(xdtts_tacotron2 *h, const int64_t *ids, size_t n,
                                       const size_t *splits, size_t n_splits,
                                       const xdtts_infer_opts *opts, float **mel,
                                       size_t *n_frames);

/* Batched form of infer_chunk (src/tacotron2/mod.rs:361-393): B independent chunks, ids is
 * B x t_stride with lens[b] valid ids each.  fixed_steps_per_item may be NULL.  mels[b] is
 * 80 x n_frames[b]. */
xdtts_status xdtts_tacotron2_infer_batch(xdtts_tacotron2 *h, const int64_t *ids,
                                         const int32_t *lens, int32_t B, int32_t t_stride,
                                         const xdtts_infer_opts *opts,
                                         const int32_t *fixed_steps_per_item, float **mels,
                                         size_t *n_frames);

/* Parity hooks: the three graphs of the reference one at a time.
 * encoder.onnx (mod.rs:379): ids (T) -> memory (T x 512), processed_memory (T x 128). */
xdtts_status xdtts_tacotron2_encoder(xdtts_tacotron2 *h, const int64_t *ids, int32_t T,
                                     float *memory, float *processed_memory);
/* The same for B chunks of T ids each (ids [B][T], zero-padded by the caller) through the code a batch request runs:
 * memory [B][T][512], processed_memory [B][T][128].  engine: -1 = the BiLSTM engine the handle would use, 1 = the cooperative
 * recurrence (one chunk per group of workgroups up to CUs / 8 chunks, two per group beyond, several launches beyond twice
 * that), 0 = the single-workgroup recurrence.  B in 1..4096, T in 1..512, every id in range, as for xdtts_tacotron2_infer_batch. */
xdtts_status xdtts_tacotron2_encoder_batch(xdtts_tacotron2 *h, int32_t engine, const int64_t *ids, int32_t B, int32_t T,
                                           float *memory, float *processed_memory);
/* run_decoder frame loop (mod.rs:272-342) on caller-supplied encoder outputs: frames are
 * n_frames x 80 (pre-postnet, time-major), gates n_frames. Buffers sized for max_steps. */
xdtts_status xdtts_tacotron2_decoder(xdtts_tacotron2 *h, const float *memory,
                                     const float *processed_memory, int32_t T, int32_t n_valid,
                                     const xdtts_infer_opts *opts, float *frames, float *gates,
                                     size_t *n_frames);
/* ONE call of decoder_iter.onnx (mod.rs:304), teacher-forced: the per-step parity hook of SURVEY.md
 * section 8c(i).  Inputs as the reference feeds them (mod.rs:284-296): memory (T x 512), processed_memory
 * (T x 128), the mask as n_valid (mod.rs:219-220), decoder_input (80) and the seven state tensors; the
 * nine outputs (mod.rs:306-307,332-339): decoder_output (80), gate_prediction (1, the logit) and the
 * seven out_* state tensors, written over the state arguments.  `step` is the frame index (it selects the
 * prenet-dropout masks of the seeded stream; opts->item_base the chunk). */
xdtts_status xdtts_tacotron2_decoder_step(xdtts_tacotron2 *h, const float *memory, const float *processed_memory,
                                          int32_t T, int32_t n_valid, const xdtts_infer_opts *opts, uint32_t step,
                                          const float *decoder_input, float *attention_hidden,
                                          float *attention_cell, float *decoder_hidden, float *decoder_cell,
                                          float *attention_weights, float *attention_weights_cum,
                                          float *attention_context, float *decoder_output,
                                          float *gate_prediction);

/* The same hook through the frame-loop engine the caller names, for B chunks and n_steps >= 1 consecutive calls of
 * decoder_iter.onnx, each fed the previous one's outputs as the reference's loop does (mod.rs:328-341):
 *   engine 0  launch-per-stage GEMV kernels (what xdtts_tacotron2_decoder_step runs)
 *   engine 1  the persistent weight-stationary kernel that serves 1..4-chunk requests -- the BASELINE configs[1]
 *             engine (B <= 2 per launch, T <= 128).  It works from the attention WEIGHTS, so the incoming
 *             attention_context must equal attention_weights . memory, as every state the graph itself produced does
 *             (out_attention_context, mod.rs:332-339); anything else is XDTTS_ERR_BAD_ARG
 *   engine 2  the batched MFMA kernels that serve lock-step batches of >= 5 chunks (configs[2] / [3]); B <= 64
 * All arrays are [B][...] row-major: memory [B][T][512], processed_memory [B][T][128], n_valid [B], decoder_input
 * [B][80], the seven state tensors [B][1024] x4, [B][T] x2, [B][512] (updated in place to the state after the last
 * step); decoder_output [B][n_steps][80] and gate_prediction [B][n_steps] (logits; no stop rule is applied).
 * step0 is the frame index of the first call (it selects the prenet-dropout draws), opts->item_base the first chunk's
 * dropout-stream index.  n_steps > 1 from the zero state gives the engine's written-back state after a free run. */
xdtts_status xdtts_tacotron2_decoder_steps(xdtts_tacotron2 *h, int32_t engine, int32_t B, const float *memory,
                                           const float *processed_memory, int32_t T, const int32_t *n_valid,
                                           const xdtts_infer_opts *opts, uint32_t step0, int32_t n_steps,
                                           const float *decoder_input, float *attention_hidden, float *attention_cell,
                                           float *decoder_hidden, float *decoder_cell, float *attention_weights,
                                           float *attention_weights_cum, float *attention_context, float *decoder_output,
                                           float *gate_prediction);

/* Engine state of a handle: 1 = the persistent decoder / cooperative encoder is in use, 0 = the handle was
 * demoted to the launch-per-stage / single-workgroup engine after a timed-out exchange (it probes the fast
 * engine again by itself every 64 calls), -1 = not probed yet.  batched_attention (lock-step batches of 5 or more
 * chunks): 2 = attention LSTM, energies, softmax and context in one launch whose blocks exchange tagged granules,
 * 1 = the attention alone in one such launch (also: batches beyond 64 chunks), 0 = separate kernels (after a
 * timed-out exchange).  Any of the three pointers may be null.  _reset puts a demoted handle back at once. */
xdtts_status xdtts_tacotron2_engine_state(const xdtts_tacotron2 *h, int32_t *decoder_persistent,
                                          int32_t *encoder_cooperative, int32_t *batched_attention);
xdtts_status xdtts_tacotron2_engine_reset(xdtts_tacotron2 *h);
/* The engine of lock-step batches of 3..8 chunks (one persistent launch for the whole loop, the LSTMs of all chunks on the matrix
 * cores: csrc/decoder_persistent8.hip): 1 = in use, 0 = off (the device cannot host its 256-workgroup grid, an exchange timed
 * out -- such batches then run on the engines either side: pairs of the persistent decoder up to 4 chunks, the batched engine
 * from 5 -- or XDTTS_P8=0 in the environment), -1 = not probed yet.  _engine_reset puts it back to -1 unless a launch was refused. */
xdtts_status xdtts_tacotron2_small_batch_engine_state(const xdtts_tacotron2 *h, int32_t *state);

/* Identity of this build: "src_sha256=<sha256 over the library's sources in name order> arch=gfx950 built_utc=... compiler=...".
 * The .so files are not in the git history (built by `make -C xd-tts_amd`, __graft_entry__.build()); the hash lets a test tell
 * whether the library it loaded was built from the sources next to it. */
const char *xdtts_build_info(void);

/* Measurement aid, not part of the reference's surface: the latency floor of one step of the
 * persistent decoder engine on this device -- its five dependent inter-CU exchanges (x, h_att, 8 x T partial energies,
 * h_dec, mel -> x) with no arithmetic between them, best of five launches of `steps` steps.  tuned != 0: the consumers
 * delay their first polls as the engine does.  bench.py reports it as roofline.latency_floor_us. */
xdtts_status xdtts_edge_floor_us(int32_t device_id, int32_t steps, int32_t T, int32_t tuned, double *us_per_step);

/* postnet.onnx (mod.rs:345-355): frames (F x 80) -> mel_outputs_postnet (80 x F). */
xdtts_status xdtts_tacotron2_postnet(xdtts_tacotron2 *h, const float *frames, int32_t F,
                                     float *mel_out);
/* The same for n >= 1 chunks through the code behind a batch request's decode (groups of at most 64 chunks per launch): chunk i
 * has F[i] >= 1 rows of 80 at frames + i * frame_stride (frame_stride a multiple of 80, in floats; only those rows are read).
 * out receives sum(F) * 80 floats: one (80 x sum F) matrix with the chunks side by side in the caller's order, or with
 * per_chunk != 0 one dense (80 x F[i]) matrix per chunk back to back -- the two layouts of xdtts_tacotron2_infer_ids / _batch. */
xdtts_status xdtts_tacotron2_postnet_batch(xdtts_tacotron2 *h, const float *frames, size_t frame_stride, const int32_t *F,
                                           int32_t n, int32_t per_chunk, float *out);

/* Phase timings of the last infer call on this handle, measured with HIP events on the
 * handle's stream: ms[0] encoder, ms[1] decoder loop, ms[2] postnet, ms[3] total;
 * steps = decoder steps executed. */
xdtts_status xdtts_tacotron2_last_timings(const xdtts_tacotron2 *h, float ms[4], int32_t *steps);

/* ---- Per-id durations and timing marks from the cumulative attention ----------------------
 * Every decoder engine keeps attention_weights_cum ([B][T]) in HBM and leaves it final when it ends: the sum of the chunk's
 * softmax rows over the frames it ran (a stopped chunk is frozen).  Entry t of a chunk's row is therefore the number of frames
 * the decoder spent on id t, and the row sums to the chunk's frame count.  With the setting ON, two small launches behind the
 * decode (never inside it: no per-step capture, no decoder kernel differs) turn these rows into, per utterance and in the
 * caller's order, the chunks' valid ids back to back:
 *   dur[i]        the fp32 cumulative weight of id i as read -- a SOFT duration: the expected number of frames on the id
 *   dur_q16[i]    round-to-nearest-even of dur[i] * 65536 as an unsigned integer (negative or NaN: 0; saturates at 2^32 - 1)
 *   start_q16[i]  65536 * (frames of the utterance's earlier chunks) + the sum of dur_q16 of the chunk's earlier ids; 64-bit
 *                 integer arithmetic only, so the value does not depend on the order of the device's scan.  start is when
 *                 id i is heard for an attention that moves monotonically; it is not a hard (Viterbi) alignment path.
 * and per utterance xdtts_alignment_stats (integer compares and adds on the Q16 values): a cheap check that the attention read
 * the whole sentence -- no id skipped (n_below), none stuck (n_above), the last id reached (last_q16).
 * The setting covers xdtts_tacotron2_infer_ids (one utterance: its chunks) and _infer_batch (every chunk an utterance), and
 * xdtts_synthesize_ids* / xdtts_synthesize_batch* (utterances as utt_chunks says).  The sequence and document entries ignore it
 * and launch nothing; after them, as after any call with the setting off, xdtts_tacotron2_last_durations_count is 0.  With the
 * setting off (the default) nothing is launched, allocated or copied and every entry returns the bits it returned before; with
 * it on the mel and audio bits are unchanged too.
 * Argument rules of the setting: on in {0, 1}; min_frames and max_frames finite, 0 <= min_frames <= max_frames <= 65535. */
typedef struct {
  int32_t on;          /* default 0 */
  float   min_frames;  /* default 0.5: an id under it counts as skipped (n_below) */
  float   max_frames;  /* default 40:  an id over it counts as stuck (n_above) */
} xdtts_durations_opts;
typedef struct {
  uint64_t sum_q16;              /* sum of dur_q16 */
  uint64_t n_frames;             /* frames of the utterance's chunks; sum_q16 / 65536 is close to it */
  uint32_t n_ids;
  uint32_t min_q16, min_index;   /* the shortest id (the first of equals), index in the utterance */
  uint32_t max_q16, max_index;   /* the longest id (the first of equals) */
  uint32_t n_below, n_above;     /* ids with dur_q16 < q16(min_frames) / > q16(max_frames) */
  uint32_t last_q16;             /* the final id's duration */
} xdtts_alignment_stats;         /* 48 bytes */
void xdtts_durations_default(xdtts_durations_opts *o); /* off, 0.5, 40 */
/* o == NULL: the default.  The fields are checked before the handle. */
xdtts_status xdtts_tacotron2_set_durations(xdtts_tacotron2 *h, const xdtts_durations_opts *o);
xdtts_status xdtts_tacotron2_get_durations(const xdtts_tacotron2 *h, xdtts_durations_opts *o);
/* What the last call on the handle captured, shaped like xdtts_griffinlim_last_loudness: the number of utterances (0: none), and
 * per utterance its ids -- *n_ids receives the count, at most cap entries are written to each output, any output may be NULL. */
xdtts_status xdtts_tacotron2_last_durations_count(const xdtts_tacotron2 *h, size_t *n_utterances);
xdtts_status xdtts_tacotron2_last_durations(const xdtts_tacotron2 *h, size_t utterance, float *dur, uint32_t *dur_q16,
                                            uint64_t *start_q16, size_t cap, size_t *n_ids);
xdtts_status xdtts_tacotron2_last_alignment(const xdtts_tacotron2 *h, size_t utterance, xdtts_alignment_stats *out);
/* Parity hook, the stage alone on caller arrays.  cum_a / cum_b: [B][T] cumulative weights by decode SLOT; slot j is the
 * caller's chunk order[j] (NULL: j); nframes[j] in [0, 100000], n_valid[j] in [1, T]; 1 <= B <= 4096, 1 <= T <= 512.
 * batched != 0: the row of slot j is read from cum_b where nframes[j] is odd (the batched kernels ping-pong by step parity),
 * else from cum_a; batched == 0: always cum_a (cum_b may be NULL).  utt_of_chunk[c], c the caller's chunk index, starts at 0
 * and goes up by 0 or 1 (NULL: every chunk an utterance).  opts NULL: the default thresholds.  The outputs hold cap_ids ids /
 * cap_utt utterances; *n_ids / *n_utt receive the counts (sum of n_valid / utterances); too little room, like every other
 * argument error, is XDTTS_ERR_BAD_ARG before a device is touched.  xdtts_durations_reference is the same call on the host,
 * serially; the two agree bit for bit.  The hook leaves xdtts_tacotron2_last_durations_count at 0. */
xdtts_status xdtts_tacotron2_durations_gather(xdtts_tacotron2 *h, const float *cum_a, const float *cum_b, int32_t B, int32_t T,
                                              const int32_t *nframes, const int32_t *n_valid, const int32_t *order,
                                              int32_t batched, const int32_t *utt_of_chunk, const xdtts_durations_opts *opts,
                                              float *dur, uint32_t *dur_q16, uint64_t *start_q16, size_t cap_ids,
                                              xdtts_alignment_stats *stats, size_t cap_utt, size_t *n_ids, size_t *n_utt);
xdtts_status xdtts_durations_reference(const float *cum_a, const float *cum_b, int32_t B, int32_t T, const int32_t *nframes,
                                       const int32_t *n_valid, const int32_t *order, int32_t batched,
                                       const int32_t *utt_of_chunk, const xdtts_durations_opts *opts, float *dur,
                                       uint32_t *dur_q16, uint64_t *start_q16, size_t cap_ids, xdtts_alignment_stats *stats,
                                       size_t cap_utt, size_t *n_ids, size_t *n_utt);
/* A position x in ids, 0 <= x <= n, of an utterance of n ids and n_frames frames -> with k = floor(x) (x == n: k = n - 1) the
 * frame position (start_q16[k] + (x - k) * dur_q16[k]) / 65536 as a fraction of n_frames - 1, clamped to [0, 1]: the pos of an
 * xdtts_prosody_point.  Double arithmetic in this order; NaN for arguments outside the rule; n_frames == 1 gives 0. */
double xdtts_durations_position(const uint64_t *start_q16, const uint32_t *dur_q16, size_t n, size_t n_frames, double x);
/* The delivered sample offset of a Q16 frame position on the PLAIN path: floor(start_q16 * hop * L / (65536 * M)) with L / M
 * the resampler's ratio for rate_out (22050: 1 / 1); -1 for a rate the resampler does not take.  NOT valid behind a rate or a
 * contour (the frames move) or the silence stage (samples are dropped). */
int64_t xdtts_durations_samples(uint64_t start_q16, int32_t hop, int64_t rate_out);

void xdtts_tacotron2_free(xdtts_tacotron2 *h);

/* ---- Griffin-Lim ------------------------------------------------------------------------ */

/* griffin_lim::mel::create_mel_filter_bank(sr, n_fft, n_mels, fmin, fmax: Option<f32>) --
 * src/tacotron2/mod.rs:453.  fmax = NaN means None (sr/2).  out is n_mels x (n_fft/2+1). */
xdtts_status xdtts_mel_filter_bank(float sample_rate, size_t n_fft, size_t n_mels, float fmin,
                                   float fmax_or_nan, float *out);

/* GriffinLim::new(mel_basis, noverlap, power, iter, momentum) -- src/tacotron2/mod.rs:456.
 * n_fft = 2*(n_bins-1); hop = n_fft - noverlap.
 * Accepted, anything else is XDTTS_ERR_BAD_ARG and *out stays null:
 *   n_bins 513 and noverlap 768 (n_fft 1024, hop 256: what the framed-FFT kernels are built for)
 *   mel_basis  n_mels x n_bins of full row rank, n_mels a positive multiple of 16 (a rank-deficient basis is refused by name)
 *   power      finite and > 0          momentum   finite and >= 0 (0: plain Griffin-Lim)
 *   iters      any count, 0 included (0: the inverse STFT of the magnitude under the initial phase)
 * The entries that take a mel (n_mels x F) refuse one whose row count is not the basis's.  Every xdtts_synthesize* entry
 * hands the vocoder the model's 80-row mel where it lies on the device, and so refuses a handle whose n_mels is not 80. */
xdtts_status xdtts_griffinlim_new(const float *mel_basis, size_t n_mels, size_t n_bins,
                                  size_t noverlap, float power, size_t iters, float momentum,
                                  int32_t device_id, xdtts_griffinlim **out);

/* The conventions of GriffinLim::infer's first step that the absent `griffin-lim` crate
 * (Cargo.lock:666-668) leaves open, as switches.  Defaults = the librosa-0.9 reading documented in
 * DESIGN.md section 2 (what every parity test and bench number uses):
 *   nnls_iters      0: S = clip(pinv(basis) . m, 0), the least-squares start of the crate's bounded NNLS
 *                   (lbfgsb 0.1.0, Cargo.lock:888-895); K > 0: K projected-gradient steps of
 *                   min 1/2 |basis x - m|^2, x >= 0 on the device after that start (fixed step
 *                   1/lambda_max(basis basis^T); the iteration's limit is the NNLS solution)
 *   power_mode      0: S = x^(1/power) (librosa mel_to_stft)   1: S = x^power   2: S = x
 *   mel_decompress  0: m = exp(mel) (Tacotron2's ln compression)   1: m = mel   2: m = 10^mel
 *   output_normalise  (G6: the last step of GriffinLim::infer before src/lib.rs:155 scales by i16::MAX)
 *                   0: audio as is   1: audio / max|audio|   2: audio * rms_target / rms(audio)
 *                   3: like 2, the scale limited to 1 / max|audio| so that no sample leaves [-1, 1]   [default 3]
 *                   (2 and 3 differ only for a crest factor above 1 / rms_target = 20 dB -- an utterance that is mostly
 *                   pause -- where 2 would hand src/lib.rs:155's saturating cast samples beyond +-1 to clip)
 *   rms_target      0.1 = -20 dBFS.  Why rms / 0.1: the only outputs of this path the reference holds --
 *                   slides/audio/goodbye.wav and capital_nonsense.wav, both exactly WAV_SPEC (src/lib.rs:25-30) -- sit
 *                   at RMS 0.099994 and 0.099995 of full scale with peaks 0.82 and 0.61: an RMS-0.1 signal after the
 *                   truncating `as i16` cast (tests/golden/reference_audio_facts.json, tools/reference_audio_facts.py)
 * and one switch of xdtts_griffinlim_infer_batch only:
 *   batch_shape     0: a workgroup owns up to 4 or up to 8 frames of an utterance, whichever shape needs less time
 *                   for the batch at hand (the overlap-add then sums in a different order than the single call:
 *                   same audio within the fp32 drift of DESIGN.md section 2, not bit for bit)
 *                   4: always the shape of the single-utterance call: every audio of a batch is bit-identical to
 *                   xdtts_griffinlim_infer on that utterance alone (the same time when its workgroups run two per CU, up to 1.6x
 *                   on a device that admits only one per CU) */
typedef struct {
  int32_t nnls_iters;
  int32_t power_mode;
  int32_t mel_decompress;
  int32_t output_normalise;
  int32_t batch_shape;
  float rms_target;
} xdtts_griffinlim_opts;
void xdtts_griffinlim_opts_default(xdtts_griffinlim_opts *opts);
xdtts_status xdtts_griffinlim_set_opts(xdtts_griffinlim *g, const xdtts_griffinlim_opts *opts);
xdtts_status xdtts_griffinlim_get_opts(const xdtts_griffinlim *g, xdtts_griffinlim_opts *opts);

/* The random initial phase of the crate is un-seeded; here it is a counter-based stream. */
xdtts_status xdtts_griffinlim_set_seed(xdtts_griffinlim *g, uint32_t seed);

/* GriffinLim::infer(&Array2<f32>) -> Vec<f32> -- src/lib.rs:141.  mel is n_mels x F (C order,
 * natural-log compressed as produced by Tacotron2); audio has hop*(F-1) samples. */
xdtts_status xdtts_griffinlim_infer(xdtts_griffinlim *g, const float *mel, size_t n_mels,
                                    size_t n_frames, float **audio, size_t *n_samples);

/* GriffinLim::infer for n_utt utterances in one call (the vocoder half of a batch; the reference calls
 * self.vocoder.infer once per utterance, src/lib.rs:141): mels[u] is n_mels x n_frames[u]; audios[u]
 * receives hop*(n_frames[u]-1) samples: the audio of xdtts_griffinlim_infer on that utterance alone (bit for bit
 * with opts.batch_shape = 4; within fp32 drift with the default, see xdtts_griffinlim_opts), whatever the mix
 * and the order.  Utterances share persistent launches (a workgroup never spans two). */
xdtts_status xdtts_griffinlim_infer_batch(xdtts_griffinlim *g, const float *const *mels, size_t n_mels,
                                          const size_t *n_frames, int32_t n_utt, float **audios,
                                          size_t *n_samples);
/* How a batch of these frame counts would be packed into persistent launches by a call made now (host arithmetic, nothing is
 * launched, no setting changes; the first call on a handle reads the device's attributes).  n_frames[u] >= 2 is what enters the
 * loop (behind a rate change: F').  It reads what the batch entries read at the call: the handle's probed CU count and
 * co-resident 4-frame workgroups per CU, opts.batch_shape, and the developer switches XDTTS_GL (launch: no persistent engine)
 * and XDTTS_GL_BATCH_FORCE.  TF, WG: frames per workgroup (4 or 8) and workgroups per CU (1 or 2) of every launch;
 * launch_of[u]: the launch utterance u rides in, 0 .. n_launches - 1, or -1 where it runs alone on the single call's engine
 * (fewer than 16 frames, or more workgroups than CUs); n_cu: 0 for a handle without a usable persistent engine (every
 * utterance alone).  Any out pointer may be NULL; a NULL handle or n_utt <= 0 is XDTTS_ERR_BAD_ARG. */
xdtts_status xdtts_griffinlim_batch_plan(xdtts_griffinlim *g, const size_t *n_frames, int32_t n_utt, int32_t *TF, int32_t *WG,
                                         int32_t *n_launches, int32_t *launch_of, int32_t *n_cu, int32_t *per_cu4);

/* The loop alone (G2..G5 and the final ISTFT): no mel->linear inversion before it and no output normalisation
 * after it -- the bench / parity entry of SURVEY.md section 8(b).  S is n_bins x F linear magnitude; phase0 is
 * n_bins x F x 2 (cos, sin) or NULL for the seeded stream; iters = 0 uses the handle's count. */
xdtts_status xdtts_griffinlim_infer_linear(xdtts_griffinlim *g, const float *S,
                                           const float *phase0, size_t n_frames, size_t iters,
                                           float **audio, size_t *n_samples);

/* mel -> linear magnitude only (step 1 of GriffinLim::infer): S_out is n_bins x F. */
xdtts_status xdtts_griffinlim_mel_to_linear(xdtts_griffinlim *g, const float *mel,
                                            size_t n_mels, size_t n_frames, float *S_out);

/* Parity hook (teacher-forced): n_iter iterations of the loop inside
 * GriffinLim::infer (src/lib.rs:141) from a caller-held state, no final ISTFT.  S is n_bins x F;
 * angles (unit-modulus phase estimate) and rebuilt (the previous iteration's STFT; zeros before
 * the first) are n_bins x F x 2 (re, im) and are updated in place. */
xdtts_status xdtts_griffinlim_step(xdtts_griffinlim *g, const float *S, float *angles,
                                   float *rebuilt, size_t n_frames, size_t n_iter);

/* ms[0] mel->linear (for the *_prosody and *_contour entries: mel->linear and the prosody stage; with phase_init 1 the SPSI stage as well:
 * everything in front of the loop), ms[1] iterations, ms[2] total of the last call (HIP events).  After
 * xdtts_griffinlim_prosody_linear and xdtts_griffinlim_spsi_phase (and their _batch forms): ms[0] the stage alone, ms[1] the
 * layout change behind it; after xdtts_griffinlim_resample / _resample_batch: ms[0] the stage alone.  With an output rate set
 * (xdtts_griffinlim_set_output_rate) the resampler falls inside ms[1], as the output normalisation does. */
xdtts_status xdtts_griffinlim_last_timings(const xdtts_griffinlim *g, float ms[3]);

/* The inverse direction of GriffinLim::infer's conventions: librosa.stft(y, 1024, hop 256, periodic hann, center, reflect)
 * -> magnitude -> mel basis -> compression, under the handle's power / power_mode / mel_decompress.
 * n_frames = n_samples / hop + 1 (so the audio of an F-frame mel analyses to F frames).  S_out (n_bins x F) and
 * mel_out (n_mels x F) are caller buffers, either may be NULL; mel_floor <= 0 means 1e-5 (Tacotron2's clamp).
 * The exponent is the handle's, inverted: power_mode 0: mel = basis . S^power, 1: S^(1/power), 2: S; the compression inverts
 * mel_decompress: 0: ln(max(m, mel_floor)), 1: m, 2: log10(max(m, mel_floor)).  n_frames may be NULL.
 * _analysis_frames needs no device (g may be NULL: every handle's hop is 256).
 * _analyze_batch: n_utt audios in one magnitude launch and one projection (then one small layout launch per wanted output and
 * utterance); S_outs / mel_outs (either may be NULL, and so may single entries) and n_frames are per utterance; every result
 * equals the single call's bit for bit, whatever the mix and order.  At most 2^20 frames per call. */
size_t       xdtts_griffinlim_analysis_frames(const xdtts_griffinlim *g, size_t n_samples);
xdtts_status xdtts_griffinlim_analyze(xdtts_griffinlim *g, const float *audio, size_t n_samples, float mel_floor,
                                      float *S_out, float *mel_out, size_t *n_frames);
xdtts_status xdtts_griffinlim_analyze_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n_samples,
                                            int32_t n_utt, float mel_floor, float **S_outs, float **mel_outs,
                                            size_t *n_frames);
/* Spectral convergence of `audio` against a target magnitude S (n_bins x F, F == analysis_frames(n_samples)):
 * out[0] = || a |STFT(audio)| - S ||_F / || S ||_F, out[1] = a.  fit_gain 0: a = 1; 1: the least-squares gain
 * a = <|X|,S> / <|X|,|X|> (for audio that went through output_normalise).  S all zero -> XDTTS_ERR_BAD_ARG.
 * The sums are taken in fp64 in a fixed order: the same input gives the same bits on every call. */
xdtts_status xdtts_griffinlim_spectral_convergence(xdtts_griffinlim *g, const float *audio, size_t n_samples,
                                                   const float *S, size_t n_frames, int32_t fit_gain, float out[2]);
/* ms[0] transform + magnitude, ms[1] mel projection / distance, ms[2] total of the last analysis call. */
xdtts_status xdtts_griffinlim_analysis_timings(const xdtts_griffinlim *g, float ms[3]);

/* Prosody: speaking rate and pitch, applied to the linear magnitude between mel -> linear and the Griffin-Lim loop (the
 * reference names prosody among what SSML steers, src/text_normaliser.rs:41-56, and left src/td_psola.rs empty; Tacotron2 has
 * no duration or pitch input).  With S time-major [F][n_bins] and fp32 arithmetic, output frame j of F' is
 *   F' = F if rate == 1, else max(floor((F - 1) / rate + 0.5), 1) + 1                  (xdtts_prosody_frames)
 *   u = min(j * rate, F - 1), i = min(floor(u), F - 2), w = u - i;  St[k] = (1 - w) S[i][k] + w S[i + 1][k]
 *   pitch == 1:  S'[j] = St                                                             (an exact zero stays one)
 *   else  L = ln(max(St, log_floor)); c = real cepstrum of L (1024-point transform of its even extension);
 *         E = the transform of c with c[n] = 0 for lifter < n < 1024 - lifter           (the smooth log envelope: the formants)
 *         R = L - E                                                                     (the log fine structure: the harmonics)
 *         p = k / pitch;  R'[k] = (1 - a) R[floor p] + a R[floor p + 1], a = p - floor p, if p <= 512, else 0
 *         S'[j][k] = exp(E[k] + R'[k])
 * rate > 1 speaks faster (fewer frames), pitch > 1 speaks higher; the envelope stays where it is, so a voice keeps its vowels.
 * The audio has hop * (F' - 1) samples.  On a magnitude that came through the mel basis the pitch change is faithful for
 * modest factors (0.8 .. 1.25) and falls short beyond: the mel bands no longer resolve the upper harmonics.
 * Fields: rate in [0.25, 4], pitch in [0.5, 2], lifter in [1, 255], log_floor > 0, everything finite; F >= 2 unless rate and
 * pitch are both 1 -- anything else is XDTTS_ERR_BAD_ARG, found before a device is touched.  rate == pitch == 1 launches
 * nothing: the results are then the bits of the entries without a prosody argument.
 * The batch and sequence entries take one prosody PER UTTERANCE (the *_batch_prosody / *_sequence_prosody entries below): a
 * batch runs the stage as one ragged launch behind its one mel -> linear GEMM, a sequence runs the single-utterance stage in each
 * utterance's vocoder half.  xdtts_prosody is uniform over its utterance; rate, pitch and gain that vary inside one are
 * xdtts_prosody_contour below. */
typedef struct {
  float rate;
  float pitch;
  int32_t lifter;
  float log_floor;
} xdtts_prosody;
void xdtts_prosody_default(xdtts_prosody *p); /* 1, 1, 30, 1e-5 */
/* F' for F = n_frames; host arithmetic (double), no handle.  0 for a bad argument: rate not in [0.25, 4] or not finite, or
 * n_frames < 2 with rate != 1. */
size_t xdtts_prosody_frames(size_t n_frames, float rate);
/* Parity hook, the prosody stage alone: S (n_bins x F, C order, as xdtts_griffinlim_mel_to_linear returns it) -> S_out
 * (n_bins x F'), a caller buffer sized by xdtts_prosody_frames; n_frames_out may be NULL. */
xdtts_status xdtts_griffinlim_prosody_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_prosody *p,
                                             float *S_out, size_t *n_frames_out);
/* xdtts_griffinlim_infer with the prosody stage between mel -> linear and the loop: audio has hop * (F' - 1) samples.
 * xdtts_griffinlim_last_timings then reports mel -> linear AND the prosody stage as ms[0]. */
xdtts_status xdtts_griffinlim_infer_prosody(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            const xdtts_prosody *p, float **audio, size_t *n_samples);
/* The entries that take an ARRAY of prosodies, p[n_utt], one per utterance (these two, xdtts_synthesize_batch_prosody and
 * xdtts_synthesize_sequence_prosody): n_utt > 0, p not NULL and the fields of every element are checked before the handles are
 * looked at -- XDTTS_ERR_BAD_ARG, the message names the field and the utterance's index; nothing is returned then (the output
 * pointers are NULL, the counts 0).  Utterances whose prosody is the identity pass through unchanged, and a call whose
 * prosodies are all the identity launches nothing new: the bits of the entry without the array.
 * xdtts_griffinlim_infer_batch with the stage behind the batch's one mel -> linear GEMM, as one ragged launch over all utterances:
 * audios[u] has hop * (xdtts_prosody_frames(n_frames[u], p[u].rate) - 1) samples and is what xdtts_griffinlim_infer_prosody returns
 * for that utterance alone (bit for bit with opts.batch_shape = 4, as for the plain pair).  last_timings: ms[0] covers mel ->
 * linear and the stage. */
xdtts_status xdtts_griffinlim_infer_batch_prosody(xdtts_griffinlim *g, const float *const *mels, size_t n_mels,
                                                  const size_t *n_frames, int32_t n_utt, const xdtts_prosody *p /* [n_utt] */,
                                                  float **audios, size_t *n_samples);
/* Parity hook, the ragged stage alone: S[u] (n_bins x F_u) -> S_outs[u] (n_bins x F'_u), caller buffers sized by
 * xdtts_prosody_frames; n_frames_out (per utterance) may be NULL.  F_u >= 1, and >= 2 unless p[u] is the identity.  Every
 * S_outs[u] equals what xdtts_griffinlim_prosody_linear gives for S[u] alone bit for bit, whatever the mix and the order. */
xdtts_status xdtts_griffinlim_prosody_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames,
                                                   int32_t n_utt, const xdtts_prosody *p /* [n_utt] */, float *const *S_outs,
                                                   size_t *n_frames_out);

/* Prosody contours: rate, pitch and gain that VARY inside one utterance -- what nested SSML <prosody> spans and
 * <prosody contour="(0%,+20%) (40%,-10%)"> ask for, without cutting the sentence at every span boundary (which would lose
 * coarticulation and Tacotron2's own phrasing; INTEGRATION.md section 1 maps the SSML to points).  A contour is a list of
 * points (pos, rate, pitch, gain); pos is a FRACTION OF THE UTTERANCE'S OWN DURATION (0 = first frame, 1 = last frame), as in
 * an SSML contour, so no attention alignment is needed.  xdtts_prosody itself is unchanged.
 * Argument rules: n_points in [1, 64]; pos finite, in [0, 1] and non-decreasing over the points (two points at one pos make a
 * step); rate in [0.25, 4]; pitch in [0.5, 2]; gain in [0, 8] (a linear amplitude factor, 0 mutes); every field finite; lifter
 * in [1, 255] and log_floor > 0 as in xdtts_prosody.  The contour is the IDENTITY when every point has rate == pitch == gain
 * == 1.  F >= 2 and F <= 16384 unless the contour is the identity (which takes what xdtts_prosody takes, F = 1 included).
 * Anything else is XDTTS_ERR_BAD_ARG, found before a device is touched; the message names the field and the point's index, in
 * the array entries the utterance's index too.
 * Value of a field v at position x -- host arithmetic in double, in exactly this order of operations:
 *   k = the number of points with pos <= x;  k == 0: v[0];  k == n: v[n-1];  else with a = k - 1, b = k:
 *   v[a] + (v[b] - v[a]) * ((x - pos[a]) / (pos[b] - pos[a]))
 * (a step is right-continuous; values hold constant before the first point and after the last).
 * Frame table, host arithmetic, one entry per input frame m = 0 .. F - 1:
 *   q[m] = (uint32) floor(65536.0 / rate((m + 0.5) / (F - 1)) + 0.5) for m < F - 1: the slowness of interval m in 2^-16 output frames
 *   c[0] = 0, c[m + 1] = c[m] + q[m];  C = c[F - 1]  (F <= 16384 keeps C below 2^32)
 *   pitch_m = (float) pitch(m / (F - 1)),  gain_m = (float) gain(m / (F - 1))
 *   F' = max((C + 32768) >> 16, 1) + 1;  the audio has hop * (F' - 1) samples.
 * Output frame j, device arithmetic in fp32 on integers that are exact:
 *   t = min(j * 65536, C);  i = the interval with c[i] <= t < c[i + 1] (t == C: i = F - 2);  w = (float)(t - c[i]) / (float)q[i]
 *   St[k] = (1 - w) S[i][k] + w S[i + 1][k]                      (the magnitude interpolation of xdtts_prosody)
 *   pj = fmaf(w, pitch_{i+1} - pitch_i, pitch_i),  gj = fmaf(w, gain_{i+1} - gain_i, gain_i)
 *   pj == 1:  S'[j] = gj * St                                     (an exact zero stays one)
 *   else      S'[j][k] = gj * exp(E[k] + R'[k]), with E, R and R' exactly as in xdtts_prosody and p = k / pj.
 * The contours ride the same warp as the frames, so a step becomes a one-frame ramp; the a + w (b - a) form keeps pj at
 * exactly 1 wherever both neighbours are 1, so the cheap branch covers whole unmodified spans.
 * Properties: a one-point contour of rate r is NOT the bits of xdtts_prosody{r} (the slowness is quantised), and F' can differ
 * by one from xdtts_prosody_frames (at most one for F in {2, 3, 5, 37, 48, 800, 16384} and ten rates; e.g. F = 3, r = 0.8).  A
 * rate-1 contour maps frame j to frame j exactly: c[m] = 65536 m.  The identity contour launches nothing and returns the bits
 * of the plain entries; an identity utterance inside a mixed batch is copied.  Batch == single, bit for bit: one kernel serves both.
 * Out of scope: the sequence entries (a caller loops over xdtts_synthesize_ids_contour); semitone targets (the host converts
 * them to factors; absolute-Hz targets and the pitch range are xdtts_pitch_target, below).  Positions in ids (phonemes) are
 * xdtts_synthesize_ids_contour_at_ids / xdtts_synthesize_batch_contour_at_ids, below. */
typedef struct { float pos, rate, pitch, gain; } xdtts_prosody_point;   /* 16 bytes */
typedef struct {
  const xdtts_prosody_point *points;   /* host memory, read during the call only */
  int32_t n_points;                    /* 1 .. 64 */
  int32_t lifter;                      /* as xdtts_prosody: 1 .. 255, default 30 */
  float   log_floor;                   /* > 0, default 1e-5 */
} xdtts_prosody_contour;
void xdtts_prosody_contour_default(xdtts_prosody_contour *c); /* no points (NULL, 0), lifter 30, log_floor 1e-5 */
/* F' for F = n_frames; host arithmetic, no handle.  0 for a bad argument. */
size_t xdtts_prosody_contour_frames(const xdtts_prosody_contour *c, size_t n_frames);
/* The frame table: cum (c), pitch and gain hold n_frames entries each, each pointer may be NULL.  Host arithmetic, no handle.
 * 1 <= n_frames <= 16384 (one frame: the identity alone, as everywhere). */
xdtts_status xdtts_prosody_contour_table(const xdtts_prosody_contour *c, size_t n_frames, uint32_t *cum, float *pitch, float *gain);
/* Parity hooks, the contour stage alone, shaped like xdtts_griffinlim_prosody_linear and _prosody_linear_batch: S_out /
 * S_outs[u] are caller buffers sized by xdtts_prosody_contour_frames.  Every S_outs[u] of the ragged form equals the single
 * hook's bit for bit, whatever the mix and the order.  last_timings: ms[0] = the launch alone, ms[1] = the layout change behind
 * it, ms[2] = both and the upload of the table in front of them. */
xdtts_status xdtts_griffinlim_contour_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_prosody_contour *c,
                                             float *S_out, size_t *n_frames_out);
xdtts_status xdtts_griffinlim_contour_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames,
                                                   int32_t n_utt, const xdtts_prosody_contour *c /* [n_utt] */, float *const *S_outs,
                                                   size_t *n_frames_out);
/* xdtts_griffinlim_infer / _infer_batch with the contour stage between mel -> linear and the loop: audio has hop * (F' - 1)
 * samples; last_timings ms[0] covers mel -> linear and the stage.  The array entry follows the array rules above
 * xdtts_griffinlim_infer_batch_prosody (arguments checked before the handles are looked at, outputs cleared on error); with
 * opts.batch_shape = 4 audios[u] is what xdtts_griffinlim_infer_contour returns for that utterance alone, bit for bit. */
xdtts_status xdtts_griffinlim_infer_contour(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                            const xdtts_prosody_contour *c, float **audio, size_t *n_samples);
xdtts_status xdtts_griffinlim_infer_batch_contour(xdtts_griffinlim *g, const float *const *mels, size_t n_mels,
                                                  const size_t *n_frames, int32_t n_utt, const xdtts_prosody_contour *c /* [n_utt] */,
                                                  float **audios, size_t *n_samples);

/* Pitch tracking on the device, and pitch TARGETS: what SSML <prosody pitch="180Hz"> and <prosody range="..."> ask for.  Both
 * need the utterance's own F0 -- per frame and its median -- which xdtts_prosody and the contours, working with factors, never
 * measure.  The tracker reads the magnitude S [F][513] that mel -> linear leaves (or an analysed one), forms each frame's real
 * cepstrum exactly as xdtts_prosody does, and takes the pitch period from its peak; a second kernel smooths, selects the median
 * and turns a target into one pitch factor per frame, multiplied on the device into the pitch array of a contour table -- no
 * round trip to the host between mel -> linear and the loop.
 * Options xdtts_f0_opts {fmin, fmax, threshold, octave_bias, log_floor}, default {60, 400, 0.2, 0.9, 1e-5}.  Rules: every field
 * finite; 50 <= fmin < fmax <= 1000; threshold >= 0; octave_bias in (0, 1]; log_floor > 0.  Quefrency range, host arithmetic in
 * double: q_lo = ceil(22050 / fmax), q_hi = floor(22050 / fmin); q_lo < q_hi is required (the rules give 22 <= q_lo, q_hi <= 441).
 * Anything else is XDTTS_ERR_BAD_ARG, found before a device is touched; the message names the field.  o == NULL: the default.
 * Per frame (device, fp32), m = S[t][0 .. 512]:
 *   L[k]   = logf(fmaxf(m[k], log_floor))                            (a NaN cell becomes log_floor)
 *   c      = the real cepstrum of L exactly as xdtts_prosody forms it (1024-point transform of the even extension, / 1024)
 *   top    = max c[n], q_lo <= n <= q_hi                             (NaN compares false)
 *   n*     = the LOWEST n in [q_lo, q_hi] with c[n] >= octave_bias * top, c[n] >= c[n-1] and c[n] >= c[n+1]; if top <= 0 or no
 *            n qualifies: the lowest n with c[n] == top; if none (all NaN): q_lo
 *   p      = the parabolic offset of SPSI (below, "offset") on (c[n*-1], c[n*], c[n*+1]), clamped to [-0.5, 0.5]
 *   raw[t] = 22050.0f / ((float)n* + p);  strength[t] = c[n*];  voiced[t] = strength[t] >= threshold   (NaN: unvoiced)
 * The lowest qualifying local maximum, not the plain argmax, keeps a rahmonic (the peak at twice the period) from being taken
 * for the period; octave_bias = 1 is the plain argmax.
 * Per utterance (device; comparisons and selections only, hence exact -- a raw value is a positive float, whose order is the
 * order of its bit pattern):
 *   f0[t] = voiced[t] ? the LOWER median of {raw[u] : |u - t| <= 2, 0 <= u < F, voiced[u]} : 0    (index (n - 1) / 2 of the sorted)
 *   stats : n_frames, n_voiced, median_hz = the lower median of the voiced f0[t] (0 if none), min_hz, max_hz over them (0 if none)
 * Target xdtts_pitch_target {mode, value, range}, default {0, 1, 1}: mode 0 none, 1 `value` in Hz in [50, 1000], 2 `value` a
 * factor in [0.5, 2]; range in [0, 4]: 1 leaves the intonation, 0 flattens it to the median, 2 doubles every excursion in
 * log-frequency.  The IDENTITY is range == 1 with mode 0, or with mode 2 and value == 1: it launches nothing and returns the
 * bits of the entry without a target (xdtts_griffinlim_last_f0 then reports n = 0).
 *   base     = mode 1: value / median_hz;  mode 2: value;  mode 0: 1           (n_voiced == 0: base = 1 and every ratio is 1)
 *   ratio[t] = voiced[t] ? exp2(log2(base) + (range - 1) * (log2(f0[t]) - log2(median_hz))) : base
 *   ratio[t] = fminf(fmaxf(ratio[t], 0.5f), 2.0f);  stats.n_clamped counts the frames the clamp changed;  stats.base_ratio = base
 * Every operation is rounded to fp32 on its own (nothing is fused); log2 and exp2 are the CORRECTLY ROUNDED fp32 functions
 * (taken in double and rounded once, on the device as in xdtts_f0_track_reference), so host and device agree.  The new pitch
 * of frame t is f0[t] ratio[t] = T (f0[t] / median)^range with T = base median.
 * Application: ratio is multiplied, on the device, into the per-frame pitch array of a contour table, the product clamped to
 * [0.5, 2] again, and k_prosody_contour runs as for a contour.  Without a caller's contour the table is the rate-1 one (c[m] =
 * 65536 m, pitch 1, gain 1, F' = F, lifter 30, log_floor 1e-5); with one, rate and gain are the contour's and pitch_m =
 * clamp(contour pitch_m * ratio[m]).  F' depends on the rate alone: the host knows every size before anything is enqueued.
 * An utterance under a target that is not the identity takes what a contour that is not the identity takes, 2 <= F <= 16384;
 * the tracker alone takes 1 <= F <= 16384 per utterance.  Batch == single, bit for bit: a frame needs nothing of its
 * neighbours, and one workgroup owns an utterance's selection.
 * Limits: through mel -> linear (pinv of the 80 mel bands) a 90 Hz voice gives a strength near 0.1 -- the bands no longer
 * resolve its harmonics -- and 70 Hz is lost; on an analysed magnitude (xdtts_griffinlim_f0_audio) the range holds.  Audio
 * that came out of the Griffin-Lim loop carries a weaker peak than its source (about 0.15 against 0.4 for a synthetic voice
 * after 30 iterations, beside 0.14 for white noise): its period is tracked all the same, so give such audio a lower threshold.
 * Out of scope: the sequence and document entries; targets in semitones (the host converts them to a factor, mode 2); voices
 * whose harmonics the mel bands do not resolve. */
typedef struct { float fmin, fmax, threshold, octave_bias, log_floor; } xdtts_f0_opts;      /* 20 bytes */
typedef struct { int32_t mode; float value, range; } xdtts_pitch_target;                    /* 12 bytes */
typedef struct {
  int32_t n_frames, n_voiced, n_clamped;
  float   median_hz, min_hz, max_hz, base_ratio;
} xdtts_f0_stats;                                                                            /* 28 bytes */
void xdtts_f0_opts_default(xdtts_f0_opts *o);
void xdtts_pitch_target_default(xdtts_pitch_target *t);
/* Host arithmetic, no handle, no device.  _plan: the rules and the quefrency range (either pointer may be NULL).
 * _track_reference: the utterance stage from given raw / strength arrays (n_frames >= 1 entries each; a voiced raw value must
 * be positive) -- f0_out, ratio_out (n_frames each) and stats may each be NULL; t == NULL: the default target. */
xdtts_status xdtts_f0_plan(const xdtts_f0_opts *o, int32_t *q_lo, int32_t *q_hi);
xdtts_status xdtts_f0_track_reference(const float *raw, const float *strength, size_t n_frames, const xdtts_f0_opts *o,
                                      const xdtts_pitch_target *t, float *f0_out, float *ratio_out, xdtts_f0_stats *stats);
/* The tracker alone on the caller's magnitude S (n_bins x F, as everywhere at the boundary): raw_out, strength_out, f0_out
 * (F floats each) and stats may each be NULL.  The ragged form runs ONE k_f0_frames launch over all rows and one k_f0_track
 * workgroup per utterance; each output equals the single call's bit for bit.  last_timings: ms[0] = k_f0_frames, ms[1] =
 * k_f0_track, ms[2] = both. */
xdtts_status xdtts_griffinlim_f0_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_f0_opts *o,
                                        float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats);
xdtts_status xdtts_griffinlim_f0_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                              const xdtts_f0_opts *o, float *const *raw_outs, float *const *strength_outs,
                                              float *const *f0_outs, xdtts_f0_stats *stats /* [n_utt] or NULL */);
/* ... from a mel (the handle's mel -> linear, then the stage), and from audio (k_stft_mag of the analysis entries, then the
 * stage; the outputs hold xdtts_griffinlim_analysis_frames(n_samples) entries). */
xdtts_status xdtts_griffinlim_f0(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames, const xdtts_f0_opts *o,
                                 float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats);
xdtts_status xdtts_griffinlim_f0_audio(xdtts_griffinlim *g, const float *audio, size_t n_samples, const xdtts_f0_opts *o,
                                       float *raw_out, float *strength_out, float *f0_out, xdtts_f0_stats *stats);
/* Parity hooks of the application: tracker, ratios, table and k_prosody_contour on the caller's magnitude.  c (c[u]) may be
 * NULL: no contour.  S_out (n_bins x F', F' = xdtts_prosody_contour_frames of the contour, F without one), ratio_out (F floats)
 * and stats may each be NULL.  An utterance whose target and contour are both the identity is copied, its ratios are 1. */
xdtts_status xdtts_griffinlim_pitch_target_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_f0_opts *o,
                                                  const xdtts_pitch_target *t, const xdtts_prosody_contour *c, float *S_out,
                                                  float *ratio_out, xdtts_f0_stats *stats);
xdtts_status xdtts_griffinlim_pitch_target_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames,
                                                        int32_t n_utt, const xdtts_f0_opts *o, const xdtts_pitch_target *t /* [n_utt] */,
                                                        const xdtts_prosody_contour *const *c /* [n_utt] or NULL */,
                                                        float *const *S_outs, float *const *ratio_outs,
                                                        xdtts_f0_stats *stats /* [n_utt] or NULL */);
/* xdtts_griffinlim_infer / _infer_batch with the tracker and the target between mel -> linear and the contour stage: both
 * kernels go onto the handle's stream, the stats travel to a pinned buffer by a copy on the same stream and are collected by
 * the call's final synchronisation (no extra host wait); last_timings ms[0] covers everything in front of the loop.  The batch
 * form takes one target per utterance, one `o` per call and contours that may be NULL per utterance (c == NULL: none at all); it
 * follows the array rules above xdtts_griffinlim_infer_batch_prosody, and with opts.batch_shape = 4 audios[u] is the single
 * call's, bit for bit.  A retry on the fallback engine recomputes from the intact S. */
xdtts_status xdtts_griffinlim_infer_pitch_target(xdtts_griffinlim *g, const float *mel, size_t n_mels, size_t n_frames,
                                                 const xdtts_f0_opts *o, const xdtts_pitch_target *t, const xdtts_prosody_contour *c,
                                                 float **audio, size_t *n_samples);
xdtts_status xdtts_griffinlim_infer_batch_pitch_target(xdtts_griffinlim *g, const float *const *mels, size_t n_mels,
                                                       const size_t *n_frames, int32_t n_utt, const xdtts_f0_opts *o,
                                                       const xdtts_pitch_target *t /* [n_utt] */,
                                                       const xdtts_prosody_contour *const *c /* [n_utt] or NULL */,
                                                       float **audios, size_t *n_samples);
/* The stats of each utterance of the last call that ran the tracker (a target entry, a hook or a tracker entry), in the caller's
 * order, shaped like xdtts_griffinlim_last_loudness; every delivering call clears them first, so *n = 0 after one that ran
 * no tracker (a plain entry, or targets that were all the identity). */
xdtts_status xdtts_griffinlim_last_f0(const xdtts_griffinlim *g, xdtts_f0_stats *out, size_t cap, size_t *n);

/* The initial phase of the loop.  Mode 0 (the default, the crate's behaviour) draws it from the seeded random stream; mode 1
 * computes it from the magnitude by Single Pass Spectrogram Inversion (Beauregard, Harish, Wyse 2015), which lowers the
 * spectral convergence a small iteration budget reaches (about half at 2 and 5 iterations on a voiced signal;
 * not on fast chirps beyond 10 iterations, hence an option).  The definition, on S time-major [F][513] fp32 -- the magnitude
 * that enters the loop: S, or S' behind a prosody stage.  For frame t, m = S[t]:
 *   peaks   k is a peak iff 1 <= k <= 511, m[k] > m[k-1] and m[k] >= m[k+1]           (exact fp32 comparisons; NaN compares false)
 *   offset  a = m[k-1], b = m[k], c = m[k+1];  d = (a - b) + (c - b);  p = d == 0 ? 0 : 0.5f * (a - c) / d, clamped to
 *           [-0.5, 0.5] by fminf(fmaxf(p, -0.5f), 0.5f)                                (all fp32)
 *   phases  are uint32 in units of 2^-32 turn, every sum modulo 2^32.  A peak advances by hop (k + p) / n_fft = (k + p) / 4
 *           turns per frame:  adv(k) = ((k & 3) << 30) + (uint32)(int32) rint(p * 2^30)
 *   owner   o_t(j) = the peak of frame t nearest to bin j by |j - k|, a tie goes to the lower k, a peak owns itself.  A frame
 *           without peaks has o_t(j) = j and delta_t(j) = 0: a silent frame carries the phase through.
 *   sign    the frame starts at sample 0 of its window, so adjacent bins of one sinusoid alternate in sign inside the Hann main
 *           lobe.  With pp = p of the owner o:  shift(j) = 0 for j == o;  pp > 0: 2^31 if j < o or j == o + 1, else 0;
 *           pp <= 0: 2^31 if j > o or j == o - 1, else 0
 *   delta_t(j) = adv(o_t(j)) + shift_t(j)
 *   phi_t[j] = phi_{t-1}[o_t(j)] + delta_t(j),  phi_{-1} = 0; it restarts at 0 for each utterance of a batch or sequence
 *   output  u = (float)(phi >> 8) * 2^-24, angles = (cos 2 pi u, sin 2 pi u) by sincospif(2 u); the previous spectrum is 0.
 * Integers make the recurrence exact in any order of evaluation: the device runs it as a scan over segments of frames, the
 * ragged batch form gives the bits of the single form, and the one place where a device may differ from a host restatement is
 * the rounding of the division in p.
 * The mode is honoured by every entry that draws the initial phase itself: _infer, _infer_prosody, _infer_linear with phase0 ==
 * NULL, _infer_batch, _infer_batch_prosody, xdtts_synthesize_ids / _batch / _sequence and their prosody forms; batch audio ==
 * single audio bit for bit with batch_shape = 4 holds in mode 1 as well.  xdtts_griffinlim_step and _infer_linear with a phase0
 * are unaffected.  With mode 0 every result keeps the bits it had. */
/* 0: the seeded random stream (default; the crate's behaviour)   1: SPSI (definition above) */
xdtts_status xdtts_griffinlim_set_phase_init(xdtts_griffinlim *g, int32_t mode);   /* other values: XDTTS_ERR_BAD_ARG */
xdtts_status xdtts_griffinlim_get_phase_init(const xdtts_griffinlim *g, int32_t *mode);
/* Parity hook, the stage alone, whatever the handle's mode: S (n_bins x F, C order, as xdtts_griffinlim_mel_to_linear
 * returns it), F >= 1 -> turns (n_bins x F, uint32, may be NULL) and angles (n_bins x F x 2 (cos, sin), the layout of
 * infer_linear's phase0, may be NULL). */
xdtts_status xdtts_griffinlim_spsi_phase(xdtts_griffinlim *g, const float *S, size_t n_frames, uint32_t *turns, float *angles);
/* The ragged form the batch entries run: every output equals the single hook's bit for bit, whatever the mix and order. */
xdtts_status xdtts_griffinlim_spsi_phase_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                               uint32_t *const *turns, float *const *angles);

/* Voice timbre: vocal-tract length and breathiness -- the two voice effects TTS services put beside <prosody>.  Prosody changes
 * how a sentence is spoken; timbre changes who seems to speak it: a deeper or lighter voice, a second speaker in a dialogue, a
 * whispered aside, from the one checkpoint.  The cepstral split of xdtts_prosody separates a frame's harmonics from its
 * envelope; prosody moves the harmonics under a fixed envelope, this stage does the reverse.
 *   vtl    in [0.5, 2]: the vocal tract is `vtl` times as long.  The ENVELOPE is resampled on the frequency axis, a formant at
 *          bin b moves to b / vtl; the harmonics are not warped, so F0 stays.
 *   breath in [0, 1]: the harmonics give way to a noise magnitude under the same formants; 1 is a whisper.
 *   seed   of the noise; lifter in [1, 255] and log_floor > 0 as in xdtts_prosody.
 * The setting is the IDENTITY when vtl == 1 && breath == 0 (the default): the stage then launches nothing and allocates
 * nothing, and every entry returns the bits it returns without it.  The definition, exactly, for frame j (the index inside its
 * own utterance) of the magnitude S that would enter the loop, k = 0 .. 512:
 *   L[k]  = ln(max(S[j][k], log_floor))
 *   c     = the real cepstrum of L exactly as xdtts_prosody forms it (1024-point transform of the even extension, / 1024)
 *   E     = the transform of c with c[n] = 0 for lifter < n < 1024 - lifter          (the envelope)
 *   R     = L - E                                                                    (the harmonics)
 *   p     = k * vtl;   E'[k] = p <= 512 ? (1 - a) E[q] + a E[min(q + 1, 512)]  (q = floor p, a = p - q)  :  E[512]
 *   n     = rng_u32(seed, 0x71B8, j * 513 + k) >> 9;   v = (2 n + 1) * 2^-24         (exact in fp32, 0 < v < 1)
 *   N     = 0.5 * ln(-ln v) + 0.28860784          (log of a Rayleigh magnitude, shifted by gamma / 2 to zero mean)
 *   R'[k] = breath == 0 ? R[k] : (1 - breath) * R[k] + breath * N
 *   S'[j][k] = exp(E'[k] + R'[k])
 * The noise depends on (seed, j, k) alone: not on the handle's phase seed, not on where the utterance lies in a batch.
 * Place: behind the prosody / contour / pitch-target stage (the pitch tracker sees the unmodified voice) and in front of the
 * initial phase (with phase_init 1, SPSI runs on S'); out of place, so S and the prosody stage's output stay intact.
 * Timbre is a SETTING OF THE HANDLE -- the voice of that handle -- like the output rate, the loudness target and the initial
 * phase.  Every entry that runs mel -> linear itself honours it: xdtts_griffinlim_infer, _infer_prosody, _infer_contour,
 * _infer_pitch_target and their _batch forms, xdtts_synthesize_ids / _batch / _sequence / _document with all their prosody,
 * contour and pitch-target forms; xdtts_griffinlim_last_timings ms[0] then covers the stage.  xdtts_griffinlim_infer_linear
 * runs the loop on a caller's magnitude and does NOT honour it (such a caller composes with xdtts_griffinlim_timbre_linear);
 * neither do the _prosody_linear, _contour_linear and _pitch_target_linear hooks nor the analysis entries.  One setting holds
 * for every utterance of a batch, sequence or document call; a two-voice dialogue uses two handles and xdtts_griffinlim_join.
 * Argument rules, checked before a handle is looked at (XDTTS_ERR_BAD_ARG, the message names the field): vtl finite and in
 * [0.5, 2], breath finite and in [0, 1], lifter in [1, 255], log_floor finite and > 0; a request of the stage alone holds 1 ..
 * 2^20 frames (no time interpolation: one frame is enough).  A failed set leaves the setting as it was. */
typedef struct { float vtl, breath; uint32_t seed; int32_t lifter; float log_floor; } xdtts_timbre;  /* 20 bytes */
void xdtts_timbre_default(xdtts_timbre *t); /* 1, 0, 1, 30, 1e-5 */
xdtts_status xdtts_griffinlim_set_timbre(xdtts_griffinlim *g, const xdtts_timbre *t);   /* NULL = the default (off) */
xdtts_status xdtts_griffinlim_get_timbre(xdtts_griffinlim *g, xdtts_timbre *t);
/* Parity hook, the stage alone, whatever the handle's setting: S (n_bins x F, C order, as xdtts_griffinlim_mel_to_linear
 * returns it), F >= 1 -> S_out (n_bins x F).  The identity returns S's bits and touches no device. */
xdtts_status xdtts_griffinlim_timbre_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_timbre *t, float *S_out);
/* The ragged form the batch entries run, one setting PER UTTERANCE (the delivering entries pass the handle's to all): every
 * S_outs[u] equals the single hook's for S[u] alone bit for bit, whatever the mix and the order; a bad element's message names
 * the utterance. */
xdtts_status xdtts_griffinlim_timbre_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                  const xdtts_timbre *t /* [n_utt] */, float *const *S_outs);
/* Host arithmetic, no handle, no device: n of cell (frame, bin) above. */
uint32_t xdtts_timbre_noise_bits(uint32_t seed, uint32_t frame, uint32_t bin);

/* Clean-up: spectral noise suppression and a tone curve.  The loop's target is pinv(mel), and Tacotron2's mel is clamped at 1e-5,
 * so every "silent" cell carries a floor that Griffin-Lim turns into broadband hiss under the voice and in every pause (the
 * complaint the `denoiser_strength` knob of NVIDIA's inference script answers).  The remedy is a gain on the magnitude: classical
 * over-subtraction against a per-bin noise estimate with a spectral floor, and beside it a per-device tone profile (handset,
 * small speaker, telephony) as a gain per bin.
 *   strength  in [0, 16]: the over-subtraction factor; 0 = no subtraction
 *   quantile  in [0, 1]: which order statistic over an utterance's frames is "the noise" (0.5: the median of each bin)
 *   floor_db  in [-80, 0]: the most a cell is attenuated
 *   tone      0 .. 8 points (hz, dB), hz strictly ascending in (0, 11025], dB in [-40, 20]; 0 points = flat
 * The setting is the IDENTITY when strength == 0 and every tone_db that is used equals 0 (the default); only these decide it.
 * The stage then launches nothing and allocates nothing, and every entry returns the bits it returns without it.
 * The definition, exactly, for an utterance of F >= 1 frames of the magnitude S as mel -> linear left it (the NNLS refinement
 * included), k = 0 .. 512:
 *   r      = floor((double) quantile * (F - 1))
 *   key(x) = bits(x) & 0x7fffffff       (a total order; the numeric one on the non-negative finite values mel -> linear produces)
 *   N[k]   = without a profile: the float whose bits are the r-th smallest (0-based) of key(S[0 .. F)[k]) -- ties are equal
 *            values and cannot matter; the frames are those of the utterance alone, never a neighbour's in a batch.
 *            With a profile: profile[k].
 *   aN[k]  = fl(strength * N[k])
 *   q      = fl(aN[k] / S[t][k])        (correctly rounded)
 *   d      = fl(1 - q)
 *   gmin   = (float) pow(10, (double) floor_db / 20)         (the single libm call of the gain rule; it runs on the host)
 *   G      = d > gmin ? d : gmin        (a NaN d gives gmin: S == 0 gives gmin, and 0 comes out)
 *   E[k]   = n_tone > 0: (float) pow(10, dB(k) / 20), dB(k) piecewise linear in log2(f_k) between the points and constant
 *            outside them, f_k = k * 22050 / 1024, bin 0 takes the first point's value; in double, on the host.  n_tone == 0: 1.
 *   S'[t][k] = fl(fl(S[t][k] * G) * E[k])
 * Every operation is rounded to fp32 on its own, nothing is fused.  With strength == 0 the selection and G are skipped (G = 1);
 * where every tone_db that is used is 0 the product with E is skipped (E = 1).  Comparisons, selections and single rounded
 * operations only: the device equals xdtts_denoise_reference bit for bit.  Subnormal magnitudes are kept by the kernels;
 * mel -> linear produces none worth the name and nothing relies on them.
 * `profile` is a caller's noise magnitude of n_bins floats (every one finite), or NULL: typically the order statistic of a
 * silent utterance of the same checkpoint, taken once with xdtts_griffinlim_noise_profile.  The handle copies it to the device
 * at set time; the setter drains the stream first, as a growth does.
 * Place: the FIRST stage of the magnitude chain, out of place -- in front of the pitch tracker, prosody, contour, timbre and the
 * initial phase: all of them, and the loop, see the cleaned magnitude; S stays intact for a retry.
 * A SETTING OF THE HANDLE, off by default, honoured by every entry that runs mel -> linear itself: the list in the timbre block
 * above.  xdtts_griffinlim_infer_linear, the _prosody_linear / _contour_linear / _timbre_linear / _f0_linear /
 * _pitch_target_linear hooks, xdtts_griffinlim_f0 and the analysis entries do NOT honour it.  One setting and one profile hold
 * for every utterance of a batch, sequence or document call.
 * Stats, per utterance, all integers (order-free): cells = 513 F; floored = the cells with G == gmin (0 without subtraction);
 * rank = r where the selection ran, else 0; profiled = 1 where the subtraction ran against a profile.  They travel back behind
 * the stage through a pinned buffer, like the tracker's.
 * Argument rules, checked before a handle is looked at (XDTTS_ERR_BAD_ARG; the message names the field, and for the batch hook
 * the utterance): every field finite and in the range above, tone_hz strictly ascending, every profile bin finite; a request of
 * the stage alone holds 1 .. 2^20 frames per utterance.  A failed set leaves the setting as it was.
 * Out of scope: smoothing of the gain over time or frequency (the over-subtraction plus floor rule is the classical stand-alone
 * form; a smoothing rule needs real speech to judge), adaptive minimum-statistics noise tracking, a profile per utterance in the
 * delivering entries, the stage in the analysis direction. */
typedef struct {
  float   strength;    /* 0 .. 16: over-subtraction factor; 0 = no subtraction                      */
  float   quantile;    /* 0 .. 1: which order statistic over an utterance's frames is "the noise"    */
  float   floor_db;    /* -80 .. 0: the most a cell is attenuated (the spectral floor)               */
  int32_t n_tone;      /* 0 .. 8 points of the tone curve; 0 = flat                                  */
  float   tone_hz[8];  /* strictly ascending, 0 < hz <= 11025                                        */
  float   tone_db[8];  /* -40 .. +20                                                                 */
} xdtts_denoise;       /* 80 bytes; default {0, 0.5, -20, 0, {0}, {0}} = the identity */
typedef struct { uint32_t cells, floored, rank, profiled; } xdtts_denoise_stats;
void xdtts_denoise_default(xdtts_denoise *d);
/* d == NULL turns the stage off (the default, and no profile); profile: n_bins floats or NULL. */
xdtts_status xdtts_griffinlim_set_denoise(xdtts_griffinlim *g, const xdtts_denoise *d, const float *profile);
/* profile_out (n_bins floats) may be NULL; *profiled = 1 where a profile is set (it may be NULL too). */
xdtts_status xdtts_griffinlim_get_denoise(xdtts_griffinlim *g, xdtts_denoise *d, float *profile_out, int32_t *profiled);
/* The stats of each utterance of the last delivering call that ran the stage, or of the last hook of the stage alone, in the
 * caller's order, shaped like xdtts_griffinlim_last_f0; *n = 0 after a delivering call with the setting off. */
xdtts_status xdtts_griffinlim_last_denoise(const xdtts_griffinlim *g, xdtts_denoise_stats *out, size_t cap, size_t *n);
/* Parity hook, the stage alone, whatever the handle holds: S (n_bins x F, C order, as xdtts_griffinlim_mel_to_linear returns
 * it), 1 <= F <= 2^20 -> S_out (n_bins x F).  The identity returns S's bits and touches no device.  last_timings: ms[0] = the
 * stage alone, ms[1] = the layout change behind it. */
xdtts_status xdtts_griffinlim_denoise_linear(xdtts_griffinlim *g, const float *S, size_t n_frames, const xdtts_denoise *d,
                                             const float *profile, float *S_out);
/* The ragged form the batch entries run, one setting PER UTTERANCE and one shared profile or NULL: every S_outs[u] equals the
 * single hook's for S[u] alone bit for bit, whatever the mix and the order. */
xdtts_status xdtts_griffinlim_denoise_linear_batch(xdtts_griffinlim *g, const float *const *S, const size_t *n_frames, int32_t n_utt,
                                                   const xdtts_denoise *d /* [n_utt] */, const float *profile, float *const *S_outs);
/* The selection alone: out[k] = N[k] of S under `quantile`. */
xdtts_status xdtts_griffinlim_noise_profile(xdtts_griffinlim *g, const float *S, size_t n_frames, float quantile, float *out /* [n_bins] */);
/* Host arithmetic, no handle, no device: r; gmin; E[513]; and the definition as serial plain C++ (stats may be NULL). */
uint32_t xdtts_denoise_rank(size_t n_frames, float quantile);
float xdtts_denoise_floor(float floor_db);
xdtts_status xdtts_denoise_tone(const xdtts_denoise *d, float *E /* [513] */);
xdtts_status xdtts_denoise_reference(const float *S, size_t n_frames, const xdtts_denoise *d, const float *profile, float *S_out,
                                     xdtts_denoise_stats *stats);

/* The output rate.  The loop produces 22 050 Hz audio (XDTTS_SAMPLE_RATE, the reference's WAV_SPEC); telephony, WebRTC / Opus
 * and audio pipelines want 8 .. 48 kHz and beyond.  With the option set, a polyphase windowed-sinc resampler runs on the
 * device between the final ISTFT and the output normalisation, so the level rules (peak 1, rms target, no sample outside
 * [-1, 1]) hold for the signal the caller receives.  The definition, exactly:
 *   R = 22050, Q = the output rate, g = gcd(Q, R), L = Q / g, M = R / g, W = max(L, M), H = 32 W.
 *   Q is supported iff 8000 <= Q <= 96000 and L <= 640 (8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 88200, 96000
 *   and others); anything else is XDTTS_ERR_BAD_ARG, the message names the rate and the rule.  Q == R is the IDENTITY: it
 *   launches nothing and every result keeps the bits it has without the option (its plan reads L = M = 1, half_len = 0, one tap
 *   of 1).
 *   taps    2 H + 1 of them, k = -H .. H, computed in double and rounded once to fp32:
 *           h[k] = (L / W) rho sinc(rho k / W) I0(beta sqrt(1 - (k / H)^2)) / I0(beta),  rho = 0.9, beta = 10,
 *           sinc(x) = sin(pi x) / (pi x): a Kaiser-windowed low-pass at 0.9 of the lower rate's Nyquist, exactly symmetric.
 *           (fp64 figures for the ten rates above: passband within +-0.0001 dB up to 0.8 of the lower Nyquist, <= -99.7 dB from
 *           that Nyquist upward, every phase's DC gain within 2e-6 of 1; 129 .. 40 961 taps, 65 .. 177 of them per output sample)
 *   output  for N input samples N' = ceil(N L / M) samples,
 *           y[m] = sum over 0 <= n < N with |m M - n L| <= H of x[n] h[m M - n L]
 *           -- zero extension at both ends and zero phase: y[0] sits on x[0].  (scipy.signal.resample_poly(x, L, M, window =
 *           h / L) in fp64.)  All index arithmetic is exact integer arithmetic (m M in 64 bits).
 *   sums    fp32, fused multiply-adds in an order that is a function of (Q, m, N) alone: the ragged batch form returns the
 *           bits of the single form, whatever the mix and order.  |y - y_fp64| <= (c + 2) 2^-24 sum |h| |x| per sample, c = the
 *           number of taps that meet it.
 * Honoured by every entry that delivers a finished utterance: xdtts_griffinlim_infer, _infer_prosody, _infer_contour,
 * _infer_batch and its prosody and contour forms, xdtts_synthesize_ids, _batch and _sequence with their prosody and contour
 * forms; *n_samples is N' = the plan's n_out for hop * (F' - 1) in each.  batch == single bit for bit (batch_shape = 4) holds
 * at every rate.  xdtts_griffinlim_infer_linear (the loop alone), _step and the analysis entries stay at 22 050 Hz.  Not per
 * utterance inside a batch.  (PCM16 / mu-law / A-law on the device and the joined stream: xdtts_synthesize_document below.)
 * xdtts_griffinlim_last_timings: the stage falls inside ms[1] (and ms[2]) exactly as the output normalisation does. */
xdtts_status xdtts_griffinlim_set_output_rate(xdtts_griffinlim *g, int32_t rate);   /* default 22050 */
xdtts_status xdtts_griffinlim_get_output_rate(const xdtts_griffinlim *g, int32_t *rate);
/* Host arithmetic, no handle, no device.  _plan: L, M, half_len = H and n_out = N' for n_in samples; any out pointer may be
 * NULL.  _filter: the library's own fp32 taps, h[-H .. H] (2 H + 1 floats, *n_taps); taps == NULL with cap == 0 asks for the
 * size alone; a buffer that is too small is XDTTS_ERR_BAD_ARG. */
xdtts_status xdtts_resample_plan(int32_t rate_out, size_t n_in, int32_t *L, int32_t *M, int32_t *half_len, size_t *n_out);
xdtts_status xdtts_resample_filter(int32_t rate_out, float *taps, size_t cap, size_t *n_taps);
/* Parity hooks, the stage alone at rate_out whatever the handle's option: audio (n samples at 22 050 Hz, n < 2^28) -> out, a
 * caller buffer sized by xdtts_resample_plan; n_out may be NULL.  The ragged form runs all utterances in one launch and
 * every outs[u] equals the single hook's bit for bit.  Argument errors come back before a device is touched.  Afterwards
 * xdtts_griffinlim_last_timings ms[0] is the stage alone. */
xdtts_status xdtts_griffinlim_resample(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate_out, float *out, size_t *n_out);
xdtts_status xdtts_griffinlim_resample_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt,
                                             int32_t rate_out, float *const *outs, size_t *n_out);

/* Loudness-normalised output.  output_normalise levels an utterance by sample peak or rms; what a product ships is an
 * integrated loudness (ITU-R BS.1770-4 / EBU R128: -16 LUFS for voice assistants, -23 for broadcast) under a true-peak
 * ceiling.  With a target set, that rule runs on the device at the delivered rate, behind the resampler, IN PLACE OF the
 * output normalisation; the scaling is one linear gain, or, with a limiter set (xdtts_griffinlim_set_limiter below), the
 * uncapped gain under a look-ahead true-peak limiter.  The definition, exactly -- Q is the rate of the
 * delivered signal, 8000 <= Q <= 96000, x its N samples (mono):
 *   K-weighting  two biquads in cascade (a0 = 1), from the analogue prototypes by the bilinear transform, K = tan(pi f0 / Q):
 *           high-shelf  f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Qf = 0.7071752369554196,
 *                       Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Qf + K^2,
 *                       b = [Vh + Vb K/Qf + K^2, 2 (K^2 - Vh), Vh - Vb K/Qf + K^2] / a0,  a = [1, 2 (K^2 - 1) / a0, (1 - K/Qf + K^2) / a0]
 *           high-pass   f0 = 38.13547087602444 Hz, Qf = 0.5003270373238773, a0 = 1 + K/Qf + K^2,
 *                       b = [1, -2, 1],  a = [1, 2 (K^2 - 1) / a0, (1 - K/Qf + K^2) / a0]
 *           (Q = 48000 reproduces the coefficient table of BS.1770.)  Both start from the zero state; y = the filtered signal.
 *   blocks  h = (Q + 5) / 10 in integer division; block j covers [j h, j h + 4 h), nb = (N - 4 h) / h + 1 if N >= 4 h, else 0;
 *           z_j = mean of y^2 over block j.
 *   gates   absolute: z_j > 10^((-70 + 0.691) / 10); relative: z_j > 0.1 mean(z over the absolutely gated blocks);
 *           Z = mean of z over the blocks that pass both (0 where none does, or nb = 0): mean_square.
 *           Integrated loudness L = -0.691 + 10 log10 Z, -inf for Z = 0 (the host function below).
 *   true peak  the largest magnitude over x and three interpolated phases p = 1, 2, 3, n = 0 .. N - 1:
 *           y[4 n + p] = sum over j = -12 .. 11 of x[n - j] t[4 j + p]  (|4 j + p| < 48, zero extension),
 *           t[k] = sinc(k / 4) I0(8 sqrt(1 - (k / 48)^2)) / I0(8), in double, rounded once to fp32.
 *   gain    target T (LUFS), ceiling C (dBTP, NaN = none): gain = 10^((T + 0.691) / 20) / sqrt(Z); if a ceiling is set and
 *           gain TP > 10^(C / 20), gain = 10^(C / 20) / TP.  Formed in double, applied as ONE fp32 factor.  Z = 0 (too short,
 *           or silence) leaves the utterance unscaled, as rms 0 does.
 *   arithmetic  filter state, coefficients and every energy sum fp64 (the high-pass has a double pole at 1 - 0.0025 at 96 kHz);
 *           the true peak fp32, fused multiply-adds over j ascending: |TP - TP_fp64| <= 26 2^-24 sum |t| |x|.  No atomics, a
 *           fixed order: the struct is a function of (Q, N, x, T, C) alone, and the ragged batch returns the bits of the
 *           single call, struct and samples.
 * A NaN target means off (the default): nothing new is launched and every result keeps its bits.  The target is finite in
 * [-70, 0], the ceiling in [-20, +6] or NaN; anything else is XDTTS_ERR_BAD_ARG and leaves the setting alone.  Honoured by
 * every entry that delivers a finished utterance (the list of xdtts_griffinlim_set_output_rate); _infer_linear, _step, the
 * analysis entries and the resample hooks stay as they are.  In xdtts_griffinlim_last_timings the stage falls inside ms[1]. */
typedef struct {
  double mean_square;   /* Z */
  double true_peak;     /* linear, of the signal as measured (before the gain) */
  double sample_peak;
  double gain;          /* applied; 1 where nothing was scaled */
  int32_t blocks, gated_blocks;   /* nb, and the blocks that passed both gates */
} xdtts_loudness;
double xdtts_loudness_lufs(const xdtts_loudness *l);   /* host: -0.691 + 10 log10 Z, -inf for Z = 0 */
xdtts_status xdtts_griffinlim_set_loudness(xdtts_griffinlim *g, float target_lufs, float ceiling_dbtp);   /* default NaN, NaN */
xdtts_status xdtts_griffinlim_get_loudness(const xdtts_griffinlim *g, float *target_lufs, float *ceiling_dbtp);
/* The measurement and applied gain of each utterance of the last delivering call, in the caller's order (they travel back
 * behind the audio).  *n = their number, 0 without a target; out == NULL with cap == 0 asks for the number alone. */
xdtts_status xdtts_griffinlim_last_loudness(const xdtts_griffinlim *g, xdtts_loudness *out, size_t cap, size_t *n);
/* Measurement alone on the caller's audio (1 <= n < 2^28 samples) at any rate in range, whatever the handle's setting:
 * gain = 1, nothing is scaled.  The ragged form runs all utterances in one set of launches and every out[u] equals the single
 * call's bit for bit.  Afterwards xdtts_griffinlim_last_timings ms[0] is the stage alone. */
xdtts_status xdtts_griffinlim_loudness(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, xdtts_loudness *out);
xdtts_status xdtts_griffinlim_loudness_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt,
                                             int32_t rate, xdtts_loudness *out);
/* Host arithmetic, no handle, no device.  _plan: h and nb for n samples (either pointer may be NULL).  _filter: coef = the
 * high-shelf's b0 b1 b2 a1 a2, then the high-pass's.  _true_peak_filter: taps[p - 1][j + 12] = t[4 j + p]. */
xdtts_status xdtts_loudness_plan(int32_t rate, size_t n, int32_t *hop, size_t *n_blocks);
xdtts_status xdtts_loudness_filter(int32_t rate, double coef[10]);
xdtts_status xdtts_true_peak_filter(float taps[3][24]);

/* Look-ahead true-peak limiter behind the loudness stage.  The one-gain rule above keeps a ceiling by lowering the WHOLE
 * utterance: where the ceiling binds, the delivered loudness stays below the target.  With a limiter set, the measurement's
 * gain is formed WITHOUT the ceiling (g0 = 10^((T + 0.691) / 20) / sqrt(Z)) and the ceiling is kept by a gain that dips only
 * around the peaks.  The definition, exactly -- x the N fp32 samples at rate Q, g0 a double, c = 10^(C / 20) a double > 0,
 * lookahead_us an integer in [500, 10000]:
 *   half width  H = max(12, (Q lookahead_us + 500000) / 1000000) in 64-bit integer division (960 at 96 kHz and 10 ms).
 *   peak envelope  y[4 n + p] as in the true peak above (the taps of xdtts_true_peak_filter, fp32 fmaf chains over j ascending,
 *           zero extension); Y[n] = max over p of |y[4 n + p]|, Y[-1] = 0; e[n] = max(|x[n]|, Y[n], Y[n - 1]): a peak between
 *           two samples belongs to both of them.
 *   needed gain  G = (float) g0; a[n] = fl(G e[n]); r[n] = 1 unless a[n] > (float) c, then
 *           r[n] = (float)((double)(float) c / (double) a[n]); r = 1 outside [0, N).
 *   hold    m[n] = min r[n - H .. n + H].
 *   smoothing  d[n] = fl(1 - m[n]); w[j] = (0.5 + 0.5 cos(pi j / (H + 1))) / (H + 1), j = -H .. H, in double on the host, rounded
 *           once to fp32 (the exact weights sum to 1); s[n] = fl(1 - sum over j of w[j] d[n + j]), one fmaf chain from 0 over j
 *           ascending.  An all-zero d gives s = 1 exactly.
 *   gain    g[n] = min(s[n], r[n]) (every m[n + j] <= r[n], so s <= r in exact arithmetic; the min covers rounding);
 *           out[n] = fl(x[n] fl(G g[n])).  Symmetric (offline): no latency, attack = release = H samples.  Where g = 1 the
 *           sample has the bits of the one-gain scaling by G.
 *   engaged  if and only if a limiter, a target and a ceiling are set, Z > 0 and g0 TP > c (doubles of the measurement);
 *           otherwise every sample is fl(x G) -- the scaling above by the uncapped gain.
 * With the limiter on, xdtts_loudness.gain is g0, the static gain that was applied; the struct keeps its layout, and the
 * stats below travel back behind it.  Decided on the device, without a host synchronisation; the ragged batch returns the bits
 * of the single call.  At programme level (xdtts_stream_opts.level = 1) the stage runs once over the formed fp32 stream, and
 * the encode reads the limited stream; gaps stay the exact zeros.  0 = off (the default): nothing new is launched and every
 * result keeps its bits.  A value outside 0 and [500, 10000] is XDTTS_ERR_BAD_ARG and leaves the setting alone.
 * Out of scope: make-up gain or iteration toward the target, separate attack and release (the compressor below has both, in
 * front of the level stage); the values delivered
 * for non-finite samples are not specified. */
typedef struct {
  float   min_gain;     /* the smallest g; 1 where nothing was limited */
  int32_t half_width;   /* H */
  int32_t engaged;      /* 1 where the stage ran, 0 where every sample is fl(x G) */
  int64_t limited;      /* samples with g < 1 */
} xdtts_limiter_stats;
xdtts_status xdtts_griffinlim_set_limiter(xdtts_griffinlim *g, int32_t lookahead_us);   /* default 0 */
xdtts_status xdtts_griffinlim_get_limiter(const xdtts_griffinlim *g, int32_t *lookahead_us);
/* The stats of each utterance of the last delivering call, shaped like xdtts_griffinlim_last_loudness; *n = 0 unless a
 * target, a ceiling and a limiter are set (without a ceiling there is nothing to keep: nothing new is launched). */
xdtts_status xdtts_griffinlim_last_limiter(const xdtts_griffinlim *g, xdtts_limiter_stats *out, size_t cap, size_t *n);
/* The stage alone on the caller's audio (1 <= n < 2^28 samples, 8000 <= rate <= 96000, gain0 finite and >= 0, ceiling_lin
 * finite and > 0), whatever the handle's settings: the `engaged` rule is not applied, the stage always runs.  The parity hook:
 * out (n floats) and stats equal xdtts_limiter_reference bit for bit, and every outs[u] of the ragged form equals the single
 * call's.  Argument errors come back before a device is touched.  Afterwards xdtts_griffinlim_last_timings ms[0] is the stage
 * alone. */
xdtts_status xdtts_griffinlim_limit(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin,
                                    int32_t lookahead_us, float *out, xdtts_limiter_stats *stats);
xdtts_status xdtts_griffinlim_limit_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                          double gain0, double ceiling_lin, int32_t lookahead_us, float *const *outs,
                                          xdtts_limiter_stats *stats);
/* Host arithmetic, no handle, no device.  _plan: H and the tile (outputs per workgroup); either pointer may be NULL.  _window:
 * w[0 .. 2 H] = w[-H .. H].  _reference: the definition evaluated sample by sample in plain C++ (stats may be NULL). */
xdtts_status xdtts_limiter_plan(int32_t rate, int32_t lookahead_us, int32_t *half_width, int32_t *tile);
xdtts_status xdtts_limiter_window(int32_t rate, int32_t lookahead_us, float *w);
xdtts_status xdtts_limiter_reference(const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin, int32_t lookahead_us,
                                     float *out, xdtts_limiter_stats *stats);

/* Dynamic range compressor in FRONT of the level stage (<amazon:effect name="drc">).  The stage runs on a finished utterance
 * behind the resampler, at the delivered rate, and in front of whichever level stage is configured -- the output
 * normalisation, the loudness target, the limiter -- so an rms or LUFS target still holds for what the caller receives.
 * Nothing has to be causal: in the place of an attack / release follower (a state-dependent recurrence) the gain is driven by a
 * TENT ENVELOPE in the log domain -- each sample's level spreads backwards with the attack slope and forwards with the release
 * slope, and the envelope is the maximum over all tents: two max-plus scans over integers, associative, order-free, exact.
 * The definition, exactly -- x the n fp32 samples at rate Q, c the settings:
 *   level   a[n] = |x[n]|; l[n] = lvl(a[n]), an int32 in units of 2^-16 octaves: for a normal float 2^e (1 + f), f in [0, 1),
 *           lvl = 65536 e + (int32) fl(65536 p + 0.5) with p = fl(f q(f)), q the degree-8 polynomial of compressor_plan.h
 *           (COMP_LOG2_Q; |f q(f) - log2(1 + f)| <= 4e-8 in exact arithmetic) by Horner's rule in fmaf from the highest
 *           coefficient; zeros and denormals have lvl = L_FLOOR = -127 * 65536.  lvl(1) = 0; no finite float's level exceeds
 *           128 * 65536, so every sum below fits 32 bits inside a tile and 64 bits anywhere.
 *   reference level  P = lvl(max a[n]): thresholds are in dB under the utterance's own sample peak (the level of Griffin-Lim
 *           output in front of the level stage is arbitrary).  A maximum does not depend on the order, so P is exact however
 *           it is reduced.  max a = 0: not engaged, the utterance is delivered unchanged.
 *   slopes  host integers, log10(2) = 0.30102999566398119521, doubles, each step one operation in the order written,
 *           round(v) = floor(v + 0.5):  oct10 = 10 / (20 log10 2);
 *           alpha = clamp(round(65536 oct10 / (attack_ms Q / 1000)), 1, 2^18), rho likewise from release_ms;
 *           T = round(threshold_db (65536 / (20 log10 2))), W = round(knee_db (65536 / (20 log10 2))).
 *           attack_ms: the time in which the gain ramps across 10 dB in front of a loud onset; release_ms: behind it.
 *   envelope  V[n] = max( max over k <= n of (l[k] - (n - k) rho), max over k >= n of (l[k] - (k - n) alpha) ), exact in
 *           integers; serially E[n] = max(l[n], E[n - 1] - rho), its mirror image with alpha, V the larger of the two.
 *   gain    s = (float)(1 / ratio - 1) <= 0, o = V[n] - (P + T) (int32).  In integers: 2 o <= -W: r = 0;  2 |o| < W:
 *           h = fl((float) o + (float)(W / 2)), r = fl(fl(h h) kq) with kq = (float)(s / (2 W)) formed in double;  otherwise
 *           r = fl(s (float) o).  g = min(1, exp2(r / 65536)): r / 65536 = i + f with i = floor, 2^f = fmaf(f, q(f), 1), q of
 *           degree 5 (COMP_EXP2_Q; |1 + f q(f) - 2^f| <= 3e-8), times 2^i through the exponent bits, 0 below -126 octaves.
 *           out[n] = fl(x[n] fl(g mk)), mk = (float) 10^(makeup_db / 20).  Where r = 0, g = 1 exactly: untouched stretches
 *           are fl(x mk), and with makeup_db = 0 they are the input's bits.
 *   stats   peak = max a; max_over = the largest o; compressed = the number of samples with r < 0; engaged.  Integer maxima
 *           and sums: independent of the order of arrival.  Not engaged (or the identity): all four are 0.
 * Settings: threshold_db in [-60, 0] (dB re peak), ratio in [1, 20], knee_db in [0, 24], attack_ms in [0.1, 100], release_ms in
 * [1, 2000], makeup_db in [0, 24], all finite; anything else is XDTTS_ERR_BAD_ARG before a device is touched, the message
 * names the field.  ratio == 1 with makeup_db == 0 is the identity: nothing is launched and every bit is kept.  Decided on the
 * device (P, engaged) without a host synchronisation; the ragged batch returns the bits of the single call, and the device the
 * bits of xdtts_compressor_reference.  Honoured by every entry that delivers an utterance: the single calls, both halves of a
 * sequence, the batch, a demoted engine's retry, and the pieces of xdtts_synthesize_document (each piece on its own, also at
 * programme level).  Off (the default): nothing new is launched and every result keeps its bits.
 * Out of scope: a compressor over the joined document stream, settings per utterance inside a batch, a downward expander or
 * gate, multiband, RMS- or LUFS-relative thresholds; the values delivered for non-finite samples are not specified. */
typedef struct {
  float threshold_db;   /* dB relative to the utterance's sample peak, [-60, 0] */
  float ratio;          /* [1, 20] */
  float knee_db;        /* full width of the soft knee, [0, 24] */
  float attack_ms;      /* [0.1, 100] */
  float release_ms;     /* [1, 2000] */
  float makeup_db;      /* [0, 24] */
} xdtts_compressor;
typedef struct {
  float   peak;         /* max |x| of the utterance in front of the stage; 0 where not engaged */
  int32_t max_over;     /* the largest o = V - (P + T), Q16 octaves */
  int32_t engaged;      /* 1 where the stage ran */
  int64_t compressed;   /* samples with r < 0 */
} xdtts_compressor_stats;
void xdtts_compressor_default(xdtts_compressor *c);   /* the identity: {0, 1, 0, 5, 100, 0} */
/* which = 0: the default; 1: "drc" {-24, 3, 6, 5, 100, 0} -- the level stage behind supplies the make-up.  Else BAD_ARG. */
xdtts_status xdtts_compressor_preset(int32_t which, xdtts_compressor *out);
/* c == NULL switches the stage off (the default).  The fields are looked at before the handle. */
xdtts_status xdtts_griffinlim_set_compressor(xdtts_griffinlim *g, const xdtts_compressor *c);
/* *on = 1 and *c = the setting, or *on = 0 and *c = the default; either pointer may be NULL */
xdtts_status xdtts_griffinlim_get_compressor(const xdtts_griffinlim *g, xdtts_compressor *c, int32_t *on);
/* The stats of each utterance of the last delivering call, shaped like xdtts_griffinlim_last_limiter; *n = 0 unless a
 * compressor other than the identity is set. */
xdtts_status xdtts_griffinlim_last_compressor(const xdtts_griffinlim *g, xdtts_compressor_stats *out, size_t cap, size_t *n);
/* The stage alone on the caller's audio (1 <= n < 2^28 samples, 8000 <= rate <= 96000), whatever the handle's settings.  The
 * parity hook: out (n floats) and stats equal xdtts_compressor_reference bit for bit, and every outs[u] of the ragged form
 * equals the single call's.  Argument errors come back before a device is touched.  Afterwards xdtts_griffinlim_last_timings
 * ms[0] is the stage alone. */
xdtts_status xdtts_griffinlim_compress(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, const xdtts_compressor *c,
                                       float *out, xdtts_compressor_stats *stats);
xdtts_status xdtts_griffinlim_compress_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                             const xdtts_compressor *c, float *const *outs, xdtts_compressor_stats *stats);
/* Host arithmetic, no handle, no device.  _plan: the host integers and the tile (samples per workgroup); any pointer may be
 * NULL.  _level: l[0 .. n) = lvl(|audio|).  _envelope: V[0 .. n).  _reference: the definition evaluated sample by sample in
 * the serial form in plain C++ (stats may be NULL). */
xdtts_status xdtts_compressor_plan(int32_t rate, const xdtts_compressor *c, int32_t *alpha, int32_t *rho, int32_t *T, int32_t *W,
                                   int32_t *tile);
xdtts_status xdtts_compressor_level(const float *audio, size_t n, int32_t *l);
xdtts_status xdtts_compressor_envelope(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, int32_t *V);
xdtts_status xdtts_compressor_reference(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, float *out,
                                        xdtts_compressor_stats *stats);

/* Pause control: the silence stage, the LAST stage of the delivery chain -- behind the level stage, at the delivered rate, out
 * of place.  It trims the near-silence a Tacotron2 utterance starts and ends with down to lead_ms / trail_ms, and caps the
 * pauses inside it at max_pause_ms, so that the gap a listener hears between two pieces of xdtts_synthesize_document is
 * trail + break + lead wherever both pieces have sound and at least that much silence of their own.  The output's length is
 * decided on the device; nothing between the loop and the copy to the host waits for it.  All decisions are integers and
 * comparisons.  The definition, exactly -- x the n fp32 samples at rate Q, s the settings:
 *   plan    in double on the host: W = Q / 200 (integer division: a 5 ms window, 40 .. 480 samples); win(ms) =
 *           (int) floor(ms / 5.0 + 0.5); min_w, lead_w, trail_w, pause_w = win of their fields; fade = min(W / 2,
 *           (int) floor(fade_ms Q / 1000.0 + 0.5)); tfac = (float) pow(10.0, threshold_db / 20.0); the fade gains T[k], k < fade,
 *           are the rising half of the stream stage's table: T[k] = (float)(0.5 - 0.5 cos(pi (k + 0.5) / fade)).
 *   1 peaks   nw = ceil(n / W) windows; window w covers len_w samples from w W (W, but for the last one).  p_w = max |x_i| over
 *             the window, P = max_w p_w: maxima, exact whatever the order.
 *   2 candidates  a0_w = p_w > fl(P tfac): one fp32 product, a strict comparison (P == 0: none).
 *   3 sound   a_w = a0_w and the maximal run of consecutive candidates that contains w has at least max(min_w, 1) windows.
 *   4 no sound anywhere: any_sound = 0, the first min(nw, max(1, lead_w + trail_w)) windows are kept.
 *   5 else, with A the first and Z the last sound window, w is kept when a_w, or w < A and A - w <= lead_w, or w > Z and
 *             w - Z <= trail_w, or -- between its nearest sound windows l < w < r -- pause_w == 0 or w - l <= pause_w -
 *             pause_w / 2 or r - w <= pause_w / 2: a pause of more than pause_w windows shrinks to exactly pause_w.
 *   6 output  the kept windows in order; n_out = the sum of their len_w; lead_cut, trail_cut, pause_cut = the samples dropped in
 *             front of A, behind Z (without sound: all of them) and between; n_cuts = the places where a kept window has a
 *             dropped neighbour.
 *   7 fades   a kept window w > 0 whose window w - 1 is dropped: sample k < fade becomes fl(x T[k]); a kept window w < nw - 1
 *             whose window w + 1 is dropped: sample len_w - 1 - k becomes fl(x T[k]), k < fade.  fade <= W / 2: they never meet.
 *             Every other sample is copied.
 * Settings: threshold_db in [-96, -6] (dB under the utterance's own sample peak), min_sound_ms in [0, 500], lead_ms and trail_ms
 * in [0, 10000], max_pause_ms 0 (pauses untouched) or in [20, 60000], fade_ms in [0, 2.5], all finite; the rate is what
 * xdtts_griffinlim_set_output_rate accepts; 1 <= n < 2^28.  Anything else is XDTTS_ERR_BAD_ARG before a device is touched, the
 * message names the field.  The stage sees what the level stage delivered, and the level stage the untrimmed utterance (the
 * gates of BS.1770 make a loudness target insensitive to the difference).  Honoured by every entry that delivers an utterance:
 * the single calls, both halves of a sequence, the batch, a demoted engine's retry, and the pieces of
 * xdtts_synthesize_document, whose records take n_out (its own edge fade is independent of the stage's fades).  Buffers handed
 * out are sized for the untrimmed utterance; n_samples = n_out.  Off (the default): nothing new is launched or allocated, and
 * every result keeps its bits.
 * Out of scope: trimming in the frame domain in front of the loop, absolute dBFS thresholds, crossfades across a cut; the
 * result for non-finite samples is not specified. */
typedef struct {
  float threshold_db;   /* [-96, -6]   dB under the utterance's own sample peak; default -40 */
  float min_sound_ms;   /* [0, 500]    sound shorter than this counts as silence (clicks); default 20 */
  float lead_ms;        /* [0, 10000]  silence kept in front of the first sound; default 50 */
  float trail_ms;       /* [0, 10000]  silence kept behind the last sound; default 100 */
  float max_pause_ms;   /* 0 = pauses inside the utterance untouched (default), else [20, 60000] */
  float fade_ms;        /* [0, 2.5]    raised-cosine fade either side of every cut; default 2 */
} xdtts_silence;
typedef struct {
  uint32_t n_in, n_out;                     /* samples in front of and behind the stage */
  uint32_t lead_cut, trail_cut, pause_cut;  /* samples dropped: n_out + lead_cut + trail_cut + pause_cut == n_in */
  uint32_t n_cuts;                          /* places where a kept window has a dropped neighbour */
  float    peak;                            /* P */
  uint32_t any_sound;                       /* 0 where no window is sound */
} xdtts_silence_stats;
void xdtts_silence_default(xdtts_silence *s);   /* {-40, 20, 50, 100, 0, 2} */
/* s == NULL switches the stage off (the default).  The fields are looked at before the handle. */
xdtts_status xdtts_griffinlim_set_silence(xdtts_griffinlim *g, const xdtts_silence *s);
/* *on = 1 and *s = the setting, or *on = 0 and *s = the default; either pointer may be NULL */
xdtts_status xdtts_griffinlim_get_silence(const xdtts_griffinlim *g, xdtts_silence *s, int32_t *on);
/* The stats of each utterance of the last delivering call, shaped like xdtts_griffinlim_last_compressor; *n = 0 unless the
 * stage is set. */
xdtts_status xdtts_griffinlim_last_silence(const xdtts_griffinlim *g, xdtts_silence_stats *out, size_t cap, size_t *n);
/* The stage alone on the caller's audio at a given rate, whatever the handle's settings.  The parity hook: out / outs[u] hold n
 * floats, of which the first stats.n_out are written -- they and the stats equal xdtts_silence_reference bit for bit, and every
 * row of the ragged form equals the single call's.  Argument errors come back before a device is touched.  Afterwards
 * xdtts_griffinlim_last_timings ms[0] is the stage alone. */
xdtts_status xdtts_griffinlim_trim(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, const xdtts_silence *s, float *out,
                                   xdtts_silence_stats *stats);
xdtts_status xdtts_griffinlim_trim_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                         const xdtts_silence *s, float *const *outs, xdtts_silence_stats *stats);
/* Host arithmetic, no handle, no device.  _plan: the host integers and the threshold's factor; any pointer may be NULL.
 * _keep: keep[0 .. ceil(n / W)) = 1 where the window is kept.  _reference: the definition as serial plain C++; out holds n
 * floats (not the input's), of which n_out are written; stats may be NULL. */
xdtts_status xdtts_silence_plan(int32_t rate, const xdtts_silence *s, int32_t *W, int32_t *min_w, int32_t *lead_w, int32_t *trail_w,
                                int32_t *pause_w, int32_t *fade, float *tfac);
xdtts_status xdtts_silence_keep(const float *audio, size_t n, int32_t rate, const xdtts_silence *s, uint8_t *keep);
xdtts_status xdtts_silence_reference(const float *audio, size_t n, int32_t rate, const xdtts_silence *s, float *out,
                                     xdtts_silence_stats *stats);

/* Document output: the utterances of a sequence joined with their <break> silences into ONE stream, faded at their edges,
 * levelled by one programme gain and encoded, on the device -- the output stage of XdTts::generate_audio (src/lib.rs:60-108:
 * every piece written as i16, the silences between them, one PCM stream).  The last stage of the delivery chain: rate ->
 * level -> join + sample format.  The definition, exactly:
 *   layout  utterances of n[u] >= 0 samples, u = 0 .. U - 1, 1 <= U <= 4096; gaps gap[0 .. U] in samples at the delivered rate,
 *           gap[0] in front of the first utterance, gap[u + 1] behind utterance u (gaps == NULL: all zero; the host gets the
 *           lengths from xdtts_silence_samples).  offset[u] = gap[0] + sum over v < u of (n[v] + gap[v + 1]);
 *           total = offset[U - 1] + n[U - 1] + gap[U], 1 <= total < 2^28.  Gap samples are exact zeros: fp32 +0.0f, PCM16 0,
 *           mu-law 0xFF, A-law 0xD5.
 *   sample i of utterance u, stream position k = offset[u] + i, in this order; every product is rounded to fp32 on its own
 *   (nothing is fused across the steps):
 *   1 fade    f = min(fade, n[u] / 2) in integer division; T[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade), j < fade, in double on
 *             the host, rounded once to fp32.  i < f: x <- fl(x T[i]); n[u] - 1 - i < f: x <- fl(x T[n[u] - 1 - i]) (the two
 *             exclude each other).  An utterance shorter than 2 fade uses the first f entries only: continuous, the window
 *             just stays below 1.
 *   2 gain    programme level only: x <- fl(x gain), the one fp32 factor below.
 *   3 format 0  x.
 *   4 format 1  v = fl(x 32767.0f).  Without dither q = the Rust cast `v as i16` (truncating toward zero, saturating, NaN -> 0:
 *             the bits of xdtts_audio_to_i16).  With dither d = u(2 k) - u(2 k + 1) (exact in fp32), u(i) = the library's
 *             counter-based uniform of (dither_seed, stream number 0x57AEA401, i): 24 bits in [0, 1); v <- fl(v + d),
 *             q = floor(fl(v + 0.5f)) saturated to [-32768, 32767], NaN -> 0.  The dither is a function of the ABSOLUTE
 *             stream position k: an utterance moved by a gap gets other dither, a stream cut in two does not repeat it.
 *   5 formats 2, 3  from the undithered q of step 4 in sign-magnitude form (the symmetric form of G.711 itself):
 *             a = min(|q|, 32767), neg = q < 0.
 *             mu-law  m = min(a >> 2, 8158) + 33, e = floor(log2 m) - 5 (0 .. 7), mant = (m >> (e + 1)) & 15,
 *                     byte = 0xFF ^ ((neg ? 0x80 : 0) | e << 4 | mant)
 *             A-law   a13 = a >> 3; a13 < 32: e = 0, mant = a13 >> 1; else e = floor(log2 a13) - 4, mant = (a13 >> e) & 15;
 *                     byte = ((neg ? 0 : 0x80) | e << 4 | mant) ^ 0x55
 *             (for q >= 0 the bytes of the common table-driven encoders; for q < 0 the exact mirror, enc(-q) = enc(q) ^ 0x80.)
 *   programme level (level = 1)  BS.1770 is a programme measurement: the utterances enter unlevelled (no output
 *             normalisation, no loudness stage of their own), the stream is formed in fp32 with fades and gaps, measured ONCE as
 *             a single signal of `total` samples at the delivered rate, and the gain rule above (target, ceiling, no gated
 *             block -> 1) gives one factor for every sample.  Needs a target on the handle (xdtts_griffinlim_set_loudness), else
 *             XDTTS_ERR_BAD_ARG; xdtts_griffinlim_last_loudness then returns exactly ONE struct.
 * Out of scope: a document built from xdtts_synthesize_batch; a rate or a format per utterance; noise-shaped dither; dither
 * for G.711; WAV container writing for the 8-bit formats (xdtts_wav_write stays PCM16). */
typedef struct {
  int32_t  format;       /* 0 fp32, 1 PCM16 (little-endian int16), 2 G.711 mu-law, 3 G.711 A-law (one byte a sample) */
  int32_t  dither;       /* 0 none: the reference's cast, 1 TPDF; format 1 only, else XDTTS_ERR_BAD_ARG */
  uint32_t dither_seed;
  int32_t  level;        /* 0 each utterance as the handle delivers it, 1 programme: ONE gain for the whole stream */
  int32_t  fade;         /* samples per utterance edge at the delivered rate, 0 .. 4800; 0 = none */
} xdtts_stream_opts;     /* default {1, 0, 0, 0, 0} */
/* Host arithmetic, no handle, no device.  _sample_bytes: 4, 2, 1, 1; 0 for an unknown format.  _plan: offsets[0 .. n_utt) and
 * *total (either may be NULL) by the layout rule, checked term by term before anything is added.  _fade_table: w[0 .. fade).
 * _encode_sample: steps 3 to 5 for ONE sample x (behind fade and gain) at stream position k, into out[0 .. sample_bytes). */
void xdtts_stream_opts_default(xdtts_stream_opts *o);
size_t xdtts_stream_sample_bytes(int32_t format);
xdtts_status xdtts_stream_plan(const size_t *n, int32_t n_utt, const size_t *gaps, size_t *offsets, size_t *total);
xdtts_status xdtts_stream_fade_table(int32_t fade, float *w);
xdtts_status xdtts_stream_encode_sample(float x, int32_t format, int32_t dither, uint32_t seed, size_t k, void *out);
/* The stage alone on the caller's audio, in one k_stream_join launch (level 1: the fp32 stream is formed and measured first):
 * the parity hook, and an entry for a host that holds batch outputs.  audios[u] may be NULL where n[u] == 0; out takes
 * total * sample_bytes bytes (cap_bytes is checked against it), offsets [n_utt] and total may be NULL.  rate matters to
 * programme level only (the range of xdtts_griffinlim_loudness).  o == NULL: the default.  Argument errors come back before a
 * device is touched, and the message names the field and the index.  Afterwards xdtts_griffinlim_last_timings ms[0] is the
 * stage alone.  (The hook stages utterance u at a device address with the 16-byte phase of audios[u] + offset[u], so a caller
 * reaches the 128-bit and the scalar load route of the kernel from the host.) */
xdtts_status xdtts_griffinlim_join(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt,
                                   const size_t *gaps, int32_t rate, const xdtts_stream_opts *o,
                                   void *out, size_t cap_bytes, size_t *offsets, size_t *total);

void xdtts_griffinlim_free(xdtts_griffinlim *g);

/* ---- XdTts::infer pipeline (src/lib.rs:110-159): mel-gen then vocoder with the mel kept in
 * HBM between the two; both outputs are returned. ------------------------------------------ */
xdtts_status xdtts_synthesize_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                  size_t n, const size_t *splits, size_t n_splits,
                                  const xdtts_infer_opts *opts, float **mel, size_t *n_frames,
                                  float **audio, size_t *n_samples);
/* The same with a prosody (xdtts_prosody above) between mel -> linear and the loop: *mel is Tacotron2's own mel (*n_frames =
 * the unmodified count F), *audio the modified utterance, hop * (xdtts_prosody_frames(F, p->rate) - 1) samples. */
xdtts_status xdtts_synthesize_ids_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                          size_t n, const size_t *splits, size_t n_splits,
                                          const xdtts_infer_opts *opts, const xdtts_prosody *p, float **mel,
                                          size_t *n_frames, float **audio, size_t *n_samples);
/* ... and with a contour (xdtts_prosody_contour above): *mel is Tacotron2's own mel, *audio has hop * (F' - 1) samples, F' =
 * xdtts_prosody_contour_frames(c, *n_frames).  The table is built once the frame count is known. */
xdtts_status xdtts_synthesize_ids_contour(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                          size_t n, const size_t *splits, size_t n_splits,
                                          const xdtts_infer_opts *opts, const xdtts_prosody_contour *c, float **mel,
                                          size_t *n_frames, float **audio, size_t *n_samples);
/* ... and with a contour whose points are anchored at IDS: the arguments of xdtts_synthesize_ids_contour, but a point's pos is
 * a position in the utterance's ids, in [0, n] and non-decreasing (k: in front of id k; n: the end; fractions fall inside an
 * id).  The call captures the durations of its own decode whatever the durations setting says (they come down right behind the
 * frame counts, before anything of the vocoder is enqueued; xdtts_tacotron2_last_durations holds them afterwards), maps every
 * point on the host with xdtts_durations_position(start_q16, dur_q16, n, F, pos), keeps the mapped positions non-decreasing
 * (the running maximum: at a chunk boundary a chunk's Q16 durations can pass the next chunk's base by a rounding), rounds them
 * to float, and runs xdtts_synthesize_ids_contour's machinery on the result: mel and audio equal, bit for bit, those of
 * xdtts_synthesize_ids_contour given the same mapped positions, and an all-identity contour returns the plain call's bits.
 * A bad pos (not finite, outside [0, n], decreasing) is XDTTS_ERR_BAD_ARG naming the point, before a device is touched. */
xdtts_status xdtts_synthesize_ids_contour_at_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                                 size_t n, const size_t *splits, size_t n_splits,
                                                 const xdtts_infer_opts *opts, const xdtts_prosody_contour *c, float **mel,
                                                 size_t *n_frames, float **audio, size_t *n_samples);

/* XdTts::infer (src/lib.rs:110-159) for n_utt utterances in one call -- the "batched / parallel
 * sentences" the author notes at src/phonemes.rs:677-680, BASELINE.json configs[3].  The chunks of
 * all utterances are given as in xdtts_tacotron2_infer_batch (ids [B][t_stride], lens[B], optional
 * per-chunk fixed step counts); utt_chunks[u] = number of CONSECUTIVE chunks that form utterance u
 * (they sum to B; find_splits + the trailing split, src/tacotron2/mod.rs:399,412-414).  All chunks
 * decode in one lock-step batch, each utterance's chunk mels are concatenated on the time axis
 * (mod.rs:430) where the post-net writes them, and the vocoder batch reads that mel in HBM.
 * Results equal xdtts_tacotron2_infer_batch followed by xdtts_griffinlim_infer_batch bit for bit.
 * n_frames[u] / mels[u] (80 x n_frames[u]; mels may be NULL) and n_samples[u] / audios[u] are
 * per utterance; buffers are released with xdtts_free. */
xdtts_status xdtts_synthesize_batch(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                    const int32_t *lens, int32_t B, int32_t t_stride,
                                    const int32_t *utt_chunks, int32_t n_utt,
                                    const xdtts_infer_opts *opts,
                                    const int32_t *fixed_steps_per_item, float **mels,
                                    size_t *n_frames, float **audios, size_t *n_samples);
/* The same with one prosody per utterance (the array rules above xdtts_griffinlim_infer_batch_prosody): mels[u] / n_frames[u] are
 * Tacotron2's own mel and count F_u, audios[u] has hop * (xdtts_prosody_frames(F_u, p[u].rate) - 1) samples.  Results equal
 * xdtts_tacotron2_infer_batch followed by xdtts_griffinlim_infer_batch_prosody bit for bit. */
xdtts_status xdtts_synthesize_batch_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                            const int32_t *lens, int32_t B, int32_t t_stride,
                                            const int32_t *utt_chunks, int32_t n_utt,
                                            const xdtts_infer_opts *opts, const int32_t *fixed_steps_per_item,
                                            const xdtts_prosody *p /* [n_utt] */, float **mels, size_t *n_frames,
                                            float **audios, size_t *n_samples);
/* ... and with one contour per utterance (array rules as above).  Results equal xdtts_tacotron2_infer_batch followed by
 * xdtts_griffinlim_infer_batch_contour bit for bit. */
xdtts_status xdtts_synthesize_batch_contour(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                            const int32_t *lens, int32_t B, int32_t t_stride,
                                            const int32_t *utt_chunks, int32_t n_utt,
                                            const xdtts_infer_opts *opts, const int32_t *fixed_steps_per_item,
                                            const xdtts_prosody_contour *c /* [n_utt] */, float **mels, size_t *n_frames,
                                            float **audios, size_t *n_samples);
/* ... and with one id-anchored contour per utterance (xdtts_synthesize_ids_contour_at_ids above): pos of utterance u's points
 * in [0, the id count of utterance u's chunks]; a bad field names the utterance and the point. */
xdtts_status xdtts_synthesize_batch_contour_at_ids(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                                   const int32_t *lens, int32_t B, int32_t t_stride,
                                                   const int32_t *utt_chunks, int32_t n_utt,
                                                   const xdtts_infer_opts *opts, const int32_t *fixed_steps_per_item,
                                                   const xdtts_prosody_contour *c /* [n_utt] */, float **mels, size_t *n_frames,
                                                   float **audios, size_t *n_samples);
/* xdtts_synthesize_ids and xdtts_synthesize_batch with a pitch target (xdtts_pitch_target, above; o == NULL: the default
 * options; c, or an element of it, may be NULL: no contour): the mel is the plain entry's, bit for bit, the audio goes through
 * the tracker, the target and the contour stage.  The frame count is known only behind the decoder, so the rule on it (2 ..
 * 16384 under a target that is not the identity) is reported then, before anything of the vocoder is enqueued.  Results equal
 * the mel entries followed by xdtts_griffinlim_infer_pitch_target / _infer_batch_pitch_target bit for bit;
 * xdtts_griffinlim_last_f0 returns the stats. */
xdtts_status xdtts_synthesize_ids_pitch_target(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids, size_t n,
                                               const size_t *splits, size_t n_splits, const xdtts_infer_opts *opts,
                                               const xdtts_f0_opts *o, const xdtts_pitch_target *t,
                                               const xdtts_prosody_contour *c, float **mel, size_t *n_frames, float **audio,
                                               size_t *n_samples);
xdtts_status xdtts_synthesize_batch_pitch_target(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *ids,
                                                 const int32_t *lens, int32_t B, int32_t t_stride,
                                                 const int32_t *utt_chunks, int32_t n_utt,
                                                 const xdtts_infer_opts *opts, const int32_t *fixed_steps_per_item,
                                                 const xdtts_f0_opts *o, const xdtts_pitch_target *t /* [n_utt] */,
                                                 const xdtts_prosody_contour *const *c /* [n_utt] or NULL */, float **mels,
                                                 size_t *n_frames, float **audios, size_t *n_samples);

/* XdTts::infer (src/lib.rs:110-159) for a SEQUENCE of n_utt utterances, each decoded alone (batch 1) exactly as
 * xdtts_synthesize_ids does it -- what a loop over src/lib.rs:122-141 does -- with the vocoder of utterance u overlapped with the
 * encoder of utterance u + 1 (the frame loop in between owns the whole GPU; it is ordered behind the previous vocoder).
 * ids[u] / n_ids[u] / splits[u] / n_splits[u] as in xdtts_synthesize_ids (splits may be NULL: one chunk per utterance unless it
 * exceeds the window); mels may be NULL.  Outputs per utterance, released with xdtts_free.  Same bits as n_utt calls of
 * xdtts_synthesize_ids; on an error nothing is returned.  xdtts_tacotron2_last_timings / xdtts_griffinlim_last_timings then
 * report the SUMS over the sequence (HIP events per utterance). */
xdtts_status xdtts_synthesize_sequence(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids,
                                       const size_t *n_ids, const size_t *const *splits, const size_t *n_splits,
                                       int32_t n_utt, const xdtts_infer_opts *opts, float **mels,
                                       size_t *n_frames, float **audios, size_t *n_samples);
/* The same with one prosody per utterance (the array rules above xdtts_griffinlim_infer_batch_prosody) -- a text cut at its
 * <break>s (src/lib.rs:83-104) whose pieces carry their own <prosody>: mels[u] / n_frames[u] are Tacotron2's own, audios[u] has
 * hop * (xdtts_prosody_frames(n_frames[u], p[u].rate) - 1) samples.  Same bits as n_utt calls of xdtts_synthesize_ids_prosody. */
xdtts_status xdtts_synthesize_sequence_prosody(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids,
                                               const size_t *n_ids, const size_t *const *splits, const size_t *n_splits,
                                               int32_t n_utt, const xdtts_infer_opts *opts,
                                               const xdtts_prosody *p /* [n_utt] */, float **mels, size_t *n_frames,
                                               float **audios, size_t *n_samples);
/* XdTts::generate_audio (src/lib.rs:60-108): a text cut at its <break>s, the pieces synthesised one after the other, ONE
 * stream out (the definition above xdtts_stream_opts).  The utterances run exactly as xdtts_synthesize_sequence (p == NULL) or
 * xdtts_synthesize_sequence_prosody runs them, but each utterance's delivered audio STAYS IN HBM: where the sequence copies
 * it to the host, the document copies it device-to-device to its place in a staging buffer.  At level 0 each utterance's
 * level stage runs as in the sequence, at level 1 it is skipped.  Behind the last vocoder: the level-1 measurement if asked
 * for, ONE k_stream_join launch, ONE copy of total * sample_bytes bytes to the host.  gaps [n_utt + 1] (NULL: none) and
 * o->fade are in samples of the handle's output rate, which applies as in every delivering entry.  *stream is released with
 * xdtts_free; mels (may be NULL) / n_frames as in the sequence; offsets [n_utt] may be NULL.  On an error nothing is
 * returned. */
xdtts_status xdtts_synthesize_document(xdtts_tacotron2 *h, xdtts_griffinlim *g, const int64_t *const *ids,
                                       const size_t *n_ids, const size_t *const *splits, const size_t *n_splits,
                                       int32_t n_utt, const xdtts_infer_opts *opts,
                                       const xdtts_prosody *p /* [n_utt] or NULL */,
                                       const size_t *gaps, const xdtts_stream_opts *o,
                                       float **mels, size_t *n_frames,
                                       void **stream, size_t *offsets, size_t *total);

/* ---- host-side front of Tacotron2::infer (stays on the CPU side of the FFI) ---------------- */
/* generate_id_list -- src/tacotron2/mod.rs:90-122: 148 symbols; token text of an id. */
int32_t xdtts_symbol_count(void);
const char *xdtts_symbol_token(int32_t id);
/* Unit::from_str (src/phonemes.rs:450-487) + best_match_for_unit (src/phonemes.rs:627-660):
 * id of a unit token ("IH0", " ", ".", "a"), or -1 where the reference drops the unit
 * (src/tacotron2/mod.rs:403-406).  as_character != 0 looks the token up as Unit::Character. */
int64_t xdtts_unit_id(const char *token, int32_t as_character);
/* split_score -- src/phonemes.rs:663-671. */
int32_t xdtts_split_score(int64_t id);
/* find_splits(units, max_size) -- src/phonemes.rs:681-753, on the id sequence. */
xdtts_status xdtts_find_splits(const int64_t *ids, size_t n, size_t max_size, size_t *out,
                               size_t cap, size_t *n_out);

/* ---- output stage (host) -- src/lib.rs:25-30,125-176 -------------------------------------- */
#define XDTTS_SAMPLE_RATE 22050 /* WAV_SPEC, src/lib.rs:25-30: mono, 22050 Hz, 16-bit signed PCM */
/* `(*sample * i16::MAX as f32) as i16` -- src/lib.rs:153-155.  Rust's float -> int `as` truncates
 * toward zero, saturates at the i16 range and maps NaN to 0. */
xdtts_status xdtts_audio_to_i16(const float *audio, size_t n, int16_t *pcm);
/* write_silence -- src/lib.rs:162-176: number of zero samples of an SSML break,
 * round(sample_rate * seconds). */
size_t xdtts_silence_samples(double seconds, uint32_t sample_rate);
/* The same from the two integer fields of a Rust `Duration` (what write_silence receives): the
 * conversion Duration::as_secs_f32 and the product are evaluated in f32 exactly as src/lib.rs:166
 * does, so the sample count is bit-identical to the reference's at every .5 boundary. */
size_t xdtts_silence_samples_duration(uint64_t secs, uint32_t nanos, uint32_t sample_rate);
/* A complete RIFF/WAVE file with the reference's WAV_SPEC (what hound's WavWriter produces for the
 * i16 writer of src/lib.rs:152-157): 44-byte PCM header + little-endian samples. */
xdtts_status xdtts_wav_write(const char *path, const int16_t *pcm, size_t n, uint32_t sample_rate);
/* ndarray_npy::write_npy(&path, &spectrogram) -- src/lib.rs:128-141: .npy version 1.0, '<f4',
 * C order, shape (rows, cols). */
xdtts_status xdtts_npy_write_f32(const char *path, const float *data, size_t rows, size_t cols);
/* Real time factor as logged at src/lib.rs:145-151: compute seconds / (samples / 22050). */
double xdtts_real_time_factor(double compute_seconds, size_t n_samples);

/* ---- misc ------------------------------------------------------------------------------- */
void xdtts_free(void *p);
const char *xdtts_last_error(void);
int32_t xdtts_device_count(void);
/* Blocks until all work queued on the handle's stream has finished. */
xdtts_status xdtts_tacotron2_sync(xdtts_tacotron2 *h);

#ifdef __cplusplus
}
#endif
#endif /* XDTTS_H */
