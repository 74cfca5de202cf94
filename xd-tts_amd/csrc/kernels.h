// kernels.h -- host-side launch interface of the HIP kernels (gfx950).
#pragma once
#include "common.h"
#include "compressor_plan.h"
#include "delivery_plan.h"
#include "durations_plan.h"
#include "f0_plan.h"
#include "gl_plan.h"
#include "limiter_plan.h"
#include "loudness_plan.h"
#include "magnitude_plan.h"
#include "resample_plan.h"
#include "stream_plan.h"
#include "timbre_plan.h"
#include "weights.h"

namespace xdtts {

// ---- decoder loop (src/tacotron2/mod.rs:272-342) ---------------------------------------------
// Device-side state of B independent chunks decoded in lock-step.  One "step" = one
// decoder_iter.onnx call of the reference (mod.rs:304) for every still-active chunk.
struct DecoderBufs {
  int B, T;
  const float *memory;  // [B][T][512]   encoder output (mod.rs:382)
  const float *pmem;    // [B][T][128]   processed_memory (mod.rs:383)
  const int *n_valid;   // [B]           un-padded length -> mask (mod.rs:219-220)
  float *att_h[2];      // [B][1024]     ping-pong by step parity
  float *att_c;         // [B][1024]
  float *dec_h[2];      // [B][1024]
  float *dec_c;         // [B][1024]
  float *aw, *awc;      // [B][T]        attention_weights, attention_weights_cum
  float *ctx;           // [B][512]      attention_context
  float *x;             // [B][256]      prenet output
  float *loc;           // [B][T][128]   location features of the current step
  float *e_part;        // [B][32][T]    per-block partial energies
  float *pmel;          // [B][264][84]  partial mel/gate sums: 8 context blocks, 256 decoder-LSTM blocks
  float *frames;        // [B][max_steps][80]  decoder_output per step (time-major)
  float *gates;         // [B][max_steps]      gate_prediction logits
  int *nframes;         // [B] in: step limit; out: frames emitted (gate may lower it)
  int *ctl;             // [0] absolute step of the first node of the graph being replayed
  int max_steps;
  int use_gate;
  float gate_threshold;
  float gate_lo, gate_hi;  // logits below / above which sigmoid(gate) > gate_threshold is decided without the sigmoid (device_utils.h: gate_fires)
  int dropout_mode;
  uint32_t dropout_seed, item_base;
  // dropout_mode 2: the caller's keep bytes [chunk][drop_steps][2][256] on the device (chunk = index within the call:
  // item_perm[b] in a sorted batch, b otherwise; views of a batch advance the pointer)
  const unsigned char *drop_masks;
  int drop_steps;
  // Batched mode only (B >= BATCH_MFMA_MIN; null otherwise).  A second copy of the vectors the two
  // LSTM GEMMs consume, in MFMA B-operand order [K/4][Bpad][4] (Bpad = B rounded up to 16, padding
  // zero): lane (chunk, k-quad) of a 16-chunk tile loads one 16-byte vector and the 64 lanes of a wave
  // cover four fully used 256-byte runs.  Written by the producers next to the row-major vectors.
  float *xf, *ctxf, *att_hf[2], *dec_hf[2];
  int Bpad;
  float *awc2;           // [B][T] second cumulative-weights buffer (ping-pong by step parity, batched mode)
  const int *item_perm;  // [B] dropout-stream index of chunk b (the batch is sorted by length), or null = b
  // Persistent engine: the context columns of its LSTM / projection rows folded into the encoder memory,
  // ctx_fold [B][CTXF_ROWS][CTXF_LD]: row n of chunk b holds W_n[ctx cols] . memory_b[t] for t < T (rows: 4096 attention-LSTM
  // rows in packed order, 4096 decoder-LSTM rows, 81 projection rows; DeviceWeights::ctx_w) -- one GEMM per request
  // (tacotron2_decode.cpp) instead of a fold loop in every launch.  null = the kernel folds for itself.
  const float *ctx_fold;
  const float *dec_in;   // parity hook (xdtts_tacotron2_decoder_step): decoder_input [B][80] of this step, or null
  // Batched mode: processed_memory a second time as [B][32 dim groups][T][4] -- the energies kernel reads 4 dims of
  // every time step, 16 bytes out of each 512-byte row of the [T][128] layout; in batched mode `loc` has this layout too
  const float *pmem_t;
  // Batched mode, one-launch attention (k_attention_b): the 8 blocks of a chunk exchange their partial energies as
  // {tag = step + 1, value} granules [B][8][T]; null = the energies / context kernel pair.  att_err: set by a block
  // whose bounded spin ran out.
  unsigned long long *ep_g;
  int *att_err;
  // ... and the attention LSTM in the same launch (k_att_lstm_attention, B <= 64): its output as granules [B][1024]
  // in place of the row-major att_h; null = separate launches
  unsigned long long *hg;
  // ... and, with it, the EARLY partial pre-activations: the columns of an LSTM GEMM whose operand exists one launch ahead
  // are multiplied there, on matrix cores the other launch leaves idle.  att_part [256 blocks][4 tiles][64 lanes][4 gates]
  // (the MFMA D layout of the block's cell-update waves) = W_att[:, 256..1791] . [ctx(s-1) ; h_att(s-1)], written by 256
  // extra blocks of the decoder-LSTM launch of step s-1, added by the attention-LSTM pass of step s, which then only
  // multiplies the 256 prenet columns.  null = the attention launch runs the whole K.
  float *att_part;
  // ... and the TWO-launch form (decoder.hip: dec_tail_chunk): h_dec as granules [B][1024], published by the decoder-LSTM blocks and
  // gathered by the chunk's four projection / prenet blocks of the same launch, which exchange the mel + gate values [B][96];
  // null = the prenet launch sums the partial-mel rows.  One allocation: melg = hdg + B * 1024.
  unsigned long long *hdg, *melg;
  // ... with the decoder LSTM's own-state columns early too: dec_part [256][4][64][4] = W_dec[:, 1536..2559] . h_dec(s-1), written by 256
  // extra blocks of the attention launch of step s, added by the decoder-LSTM pass of step s, which then multiplies [h_att ; ctx] only
  float *dec_part;
  int att_spins, att_fault;  // test hooks: poll limit (0 = default) and a block (index + 1) that never publishes its energies
  int tail_fault;            // test hook, two-launch form: a decoder-LSTM block (index + 1) that never publishes its h_dec granules
  int att_slow;              // test hook: a block (index + 1) of both batched launches that stalls ~7 us at a different point of every step
};
constexpr int ATT_EXCHANGE_BLOCKS = 8;  // granule rows per chunk (CTX_BLOCKS in decoder.hip)
// [B][T][128] -> [B][32][T][4]
void launch_dimgroup_transpose(const float *in, float *out, int B, int T, hipStream_t s);

// Enqueues `nsteps` decoder steps on `s` (5 kernels each) and advances the device step base.
void launch_decoder_steps(const DecoderBufs &d, const DeviceWeights &w, int nsteps, hipStream_t s);
// Parity hook (xdtts_tacotron2_decoder_steps): node i of a sequence alone (state parity i & 1; absolute step ctl[0] + i),
// the advance of the step base, the location features of the current attention weights (launch-per-stage engine; the
// batched engine computes them inside its prenet launch), and the batched engine's state layout conversion.
void launch_decoder_step_at(const DecoderBufs &d, const DeviceWeights &w, int i, hipStream_t s);
void launch_decoder_advance(const DecoderBufs &d, int n, hipStream_t s);
void launch_decoder_early(const DecoderBufs &d, const DeviceWeights &w, int i, hipStream_t s);  // (no-op without d.att_part)
bool decoder_two_launch(const DecoderBufs &d);
void launch_decoder_prologue(const DecoderBufs &d, const DeviceWeights &w, hipStream_t s);  // (no-op in the three-launch form)
void launch_decoder_location(const DecoderBufs &d, const DeviceWeights &w, hipStream_t s);
void launch_decoder_prenet(const DecoderBufs &d, const DeviceWeights &w, hipStream_t s);
void launch_frag_convert(float *rowmajor, float *frag, int B, int Bpad, int n, int dir, hipStream_t s);
// After the last step of a sequence: completes the final frame's projection (frames, gate).
void launch_decoder_flush(const DecoderBufs &d, const DeviceWeights &w, hipStream_t s);
size_t decoder_pmel_floats(int B);
// Zeroes the recurrent state (DecoderState::new, mod.rs:202-233) and sets the step limits.
void launch_decoder_init(const DecoderBufs &d, const int *limits_dev, hipStream_t s);

// ---- persistent weight-stationary decoder (decoder_persistent.hip), small lock-step batches ------
constexpr int CTXF_ROWS = 2 * 4096 + 128, CTXF_LD = 128;  // rows of the context-fold table (81 projection rows, padded), its row stride
// ctx_w [CTXF_ROWS][512]: the context columns of att_w / dec_w (packed row order) and proj_w, zero rows behind
void launch_pack_ctx_rows(const float *att_w, const float *dec_w, const float *proj_w, float *ctx_w, hipStream_t s);
constexpr int PERSIST_B_MAX = 2;    // chunks in lock-step (register file + LDS of a CU hold the slices and two chunks' state)
constexpr int PERSIST_T_MAX = 128;  // encoder steps (the reference's window is 100, mod.rs:363)
// Granule exchange buffers: 8-byte {tag, value} records, [2 step parities][B][n] each.
struct PersistBufs {
  unsigned long long *x, *hatt, *ep, *hdec, *mel;  // (neither the context nor the attention weights cross)
  int *err;  // set by a workgroup whose bounded spin ran out
  int spins, fault;  // developer/test knobs: poll limit (0 = default) and a workgroup (index + 1) that never runs
  int slow;          // test hook: a workgroup (index + 1) that stalls ~7 us at a different point of every step (straggler:
                     // the two-slot exchange must keep every other workgroup from running more than one step ahead of it)
  int skew;    // 2-chunk launch that ends with its first chunk: the chunks run two phases apart (decoder_persistent.hip, "skewed pair")
  int both_run;  // 2-chunk launch without `shrink` whose chunks are both known to run all of its steps (gate-less decode)
  int shrink;  // 2-chunk launch: end as soon as one chunk stops (the host continues with a 1-chunk launch)
  int first;  // delay before a critical consumer's first poll, x 256 clocks (developer knob)
  int efirst;  // the attention role's first poll of the partial energies (it has just published its own slice); lock-step pair only:
               // the one-chunk kernel issues that poll from inside the column block behind the publish (EPOLL_AT, EPOLL_NAP)
  int xfirst;  // the same for the projection role's first poll of x (it has just published its own 16 columns)
  int pfirst;  // the same for the projection role's first poll of h_dec (behind its weight fetch and mask hashing)
  int xlazy, clazy;  // first-poll delay of the x / ctx consumers that are not their producers, x 256 clocks
  int lazy;  // late-poll delay of the off-critical-path consumers, x 256 clocks
  unsigned long long *prof;  // developer profile build only: [256][16] phase clocks, else null
};
size_t persist_granule_words(int B);
PersistBufs persist_bufs(unsigned long long *base, int *err, int B);
// The same exchange seen by a launch over chunks [b0, b0 + n) of the seeded batch.
PersistBufs persist_view(const PersistBufs &g, int b0);
bool decoder_persistent_supported(int device, int B, int T);
// After launch_decoder_init: clears the exchange and publishes x(0) with the chunks' active bits.
void launch_persist_seed(const DecoderBufs &d, const PersistBufs &g, const int *limits_dev, hipStream_t s);
// Parity hook: the same for a sequence that starts at `step` with the prenet output x [B][256] already computed (d.x)
void launch_persist_seed_at(const DecoderBufs &d, const PersistBufs &g, const int *limits_dev, int step, hipStream_t s);
// Runs up to `nsteps` decoder steps in one launch (ends early when every chunk has stopped);
// frames/gates/nframes are complete on return, ctl[0] = steps executed.  No flush needed.
void launch_decoder_persistent(const DecoderBufs &d, const DeviceWeights &w, const PersistBufs &g, int nsteps,
                               hipStream_t s);

// ---- persistent weight-stationary decoder for 3..8 chunks (decoder_persistent8.hip): the LSTMs of all chunks as one MFMA
// stream per wave, the context as a sixth exchange ------------------------------------------------------------------------
constexpr int P8_B_MAX = 16;  // 3..8 chunks: k_decoder_persistent8<4 / 8>; 9..16: k_decoder_persistent16 (same exchange layout, 16 chunk slots)
constexpr int P8_STEPS_MAX = 16384;  // longest request it takes: 190 s of speech, 1.5 GB of ring at 8 chunk slots
struct P8Bufs {
  unsigned *rx, *rhatt, *rctx, *rhdec;  // write-once rings of plain values [step][chunk slots][n], 0xFFFFFFFF = not yet written
  unsigned long long *ep, *mel;         // {tag, value} granules, [2 step parities][chunk slots][n] each (row strides: the serving kernel's slot count)
  int *err;          // set by a workgroup whose bounded spin ran out
  int spins, fault;  // test hooks: poll limit (0 = default) and a workgroup (index + 1) that never runs
  int delay[6];      // naps (64 clocks each) before the first poll of h_att / ctx / h_dec / x / the partial energies / the mel rows (16-slot kernel)
  int ring_steps;    // steps the rings are laid out for
  unsigned long long *prof;  // developer build (-DXDTTS_P8_PROFILE): [workgroup][32] phase clocks
};
size_t p8_exchange_words(int B, int nsteps);
P8Bufs p8_bufs(unsigned long long *base, int *err, int B, int nsteps);
bool decoder_p8_supported(int device, int B, int T);
void launch_p8_seed(const DecoderBufs &d, const P8Bufs &g, const int *limits_dev, hipStream_t s);
void launch_p8_seed_at(const DecoderBufs &d, const P8Bufs &g, const int *limits_dev, int step, hipStream_t s);
// Runs up to `nsteps` decoder steps of d.B <= 8 chunks in one launch (ends early when every chunk has stopped); frames / gates /
// nframes are complete on return, the state is written back, ctl[0] = steps executed.
void launch_decoder_p8(const DecoderBufs &d, const DeviceWeights &w, const P8Bufs &g, int nsteps, hipStream_t s);
// the 16-slot kernel behind the two functions above (decoder_persistent16.hip)
struct P8Weights {
  const float4 *att_w, *dec_w, *q_w, *proj_w;
  const float *att_b, *dec_b, *v_w, *loc_fused, *proj_b, *pre0T, *pre1T;
};
bool decoder_p16_supported(int device, int T);
void launch_decoder_p16(const DecoderBufs &d, const P8Weights &w, const P8Bufs &g, int nsteps, hipStream_t s);

// ---- NT GEMM on the f32 MFMA: C = act(A W^T + bias) (+R) ---------------------------------------
struct GemmArgs {
  const float *A;
  long lda, strideA;  // row m of item z starts at A + z*strideA + m*lda (rows may overlap: conv)
  const float *W;     // [N][K], K contiguous
  const float *bias;  // [N] or null
  float *C;
  long ldc, strideC;
  const float *R;     // residual, indexed like an un-transposed C; or null
  long ldr, strideR;
  int M, N, K, batch;
  // ragged batches (post-net over chunks of different length): per-item row count and extra element
  // offset of C, used when ragged != 0 (batch <= GEMM_RAGGED_MAX); blocks past an item's rows exit
  int ragged;
  int Mz[64];
  long Cz[64];
  int act;            // 0 none, 1 relu, 2 tanh, 3 pow(max(x,0), p)
  int transpose_out;  // store C[n*ldc + m]
  int ldc_rows;       // ragged + transpose_out: item z's row stride is its own Mz[z] -- one dense (N x Mz[z]) matrix per item at C + Cz[z]
  float p;
  // v = alpha * (A W^T) + bias; R is added scaled by beta, before the activation when r_before_act
  // (0 in alpha / beta means 1: zero-initialised args keep the plain form)
  float alpha, beta;
  int r_before_act;
  int xcd_rows;       // set by launch_gemm_nt: block -> tile mapping that keeps a row tile's column tiles on one XCD (gemm.hip)
  // split-K (gemm_splitk_plan): K slices per tile (0 / 1 = none), their meeting place [tiles][slices][1024 floats] and the tiles'
  // arrival counters (zero between launches)
  int splitk;
  float *ws;
  unsigned *cnt;
  int tile;           // 0: launch_gemm_nt's own choice; 32 / 64: the plan's
};
int gemm_splitk_plan(const GemmArgs &g, size_t *ws_floats, size_t *tiles, int *tile);
constexpr int GEMM_RAGGED_MAX = 64;  // (the argument block stays under 1 KB)
void launch_gemm_nt(const GemmArgs &g, hipStream_t s);

// ---- encoder (encoder.onnx, mod.rs:379) ---------------------------------------------------------
// ids [B][T] -> rows [pad, pad+T) of the zero-padded time-major buffer xpad [B][T+2*pad][512]
void launch_embed(const int64_t *ids, const float *emb, float *xpad, int B, int T, int pad, hipStream_t s);
// xproj [2][B][T][1024] (W_ih x + b), WhhT[dir] [256][1024] -> memory [B][T][512]
void launch_bilstm(const float *xproj, const float *whhT_fwd, const float *whhT_bwd, float *memory,
                   int B, int T, hipStream_t s);

// Same recurrence spread over 4 CUs per (direction, chunk) with W_hh resident in registers and a
// tagged-granule exchange of the hidden state (encoder.hip).  Needs all 8*B blocks co-resident.
size_t bilstm_coop_exchange_words(int B);
void launch_bilstm_coop(const float *xproj, const float *whhT_fwd, const float *whhT_bwd, float *memory,
                        unsigned long long *exchange, int *err, int B, int T, int group, hipStream_t s);

// ---- Griffin-Lim -------------------------------------------------------------------------------
struct GlBufs {
  int F, n_fft, hop, nb;   // frames, 1024, 256, 513
  float *S;                // [F][nb]        linear magnitude
  float2 *ang, *ang2;      // [F][nb]        unit-modulus phase estimate (ping-pong for the fused iteration)
  float2 *tprev;           // [F][nb]        previous rebuilt spectrum
  float *frames;           // [F][n_fft]     windowed time frames
  float *wss_inv;          // [hop*(F-1)]    window sum-of-squares divisor per output sample
  const float2 *tw;        // [n_fft]        exp(-2*pi*i*k/n_fft)
  const float *win;        // [n_fft]        periodic hann
};
// Persistent Griffin-Lim (griffinlim.hip: k_gl_persistent): all iterations + the final ISTFT in one
// launch, one workgroup per CU owning 3..TF consecutive frames, state in LDS, 768-sample overlaps
// exchanged with the two neighbours as tagged 8-byte granules.
// (GLP_TF_MAX, GlSeg and the host's planning arithmetic: gl_plan.h)
struct GlPersist {
  const GlSeg *segs;        // [nblk] or null = one utterance of g.F frames split evenly over the workgroups
  unsigned long long *xch;  // [nblk][2 parities][2 sides][768] granules
  int *err;                 // set when a bounded spin ran out
  unsigned epoch;           // tag base of this call (tags = epoch + iteration + 1; never reused within the buffer's life)
  int nblk, TF;
  int per_cu;               // 2: the launch holds up to two 4-frame workgroups per CU (vocoder batch), else 0 / 1
  int spins;                // test hook: poll limit (0 = default)
  int slow;                 // test hook: a workgroup (index + 1) that stalls ~7 us at a different point of every iteration
  int poll_delay;           // first poll of the neighbours' granules: n >= 0: n x 128 clocks after the publish, before the own overlap-add; n < 0: behind it (+ (-1 - n) x 128 clocks)
  int gen_phase;            // 1: the kernel draws the seeded initial phase itself (angles = exp(2 pi i u), previous spectrum 0)
  unsigned seed;            //    instead of reading ang_in / tprev_in (saves the phase-init launch and a round trip through HBM)
  float2 *ang_out, *tprev_out;  // parity hook: final state, or null
  unsigned long long *prof;     // developer profile build only: [nblk][12] phase clocks, else null
};
size_t gl_persistent_xch_words(int nblk);
bool gl_persistent_supported(int device, int *n_cu, int *per_cu4);
void launch_gl_persistent(const GlBufs &g, const GlPersist &p, const float2 *ang_in, const float2 *tprev_in, int n_iter,
                          float alpha, float *audio, hipStream_t s);
// mode 0: exp (natural-log mel), 1: copy (already linear), 2: 10^x
void launch_gl_exp_transpose(const float *mel_80xF, float *out_Fx80, int n_mels, int F, int mode, hipStream_t s);
// out[F][nb] = in[F][ld]^p (p == 1: copy): the exponent of mel->linear after the NNLS refinement
void launch_gl_pow_rows(const float *in, int ld, float *out, int nb, int F, float p, hipStream_t s);
// Output normalisation (mode 1: y / max|y|, 2: y * target / rms(y)) of n_utt utterances in two launches: utterance u is
// the samples [tab_dev[u].x, + tab_dev[u].y) of y (tab_dev == nullptr: one utterance, [first, first + n_max)); n_max = the
// longest of them; parts = GLN_SCRATCH floats of device scratch per utterance.  Deterministic (fixed reduction order).
constexpr int GLN_PARTS = 64;
constexpr int GLN_SCRATCH = 2 * GLN_PARTS;  // floats of scratch per utterance: sums of squares / peaks
void launch_gl_output_normalise(float *y, const int2 *tab_dev, int n_utt, int first, int n_max, int mode, float target,
                                float *parts, hipStream_t s);
void launch_gl_phase_init(const GlBufs &g, uint32_t seed, const float *phase0_dev, hipStream_t s);
// batch form: g.F = total frames of the concatenated utterances; frame_local[f] = index of row f inside its utterance
void launch_gl_phase_init_batch(const GlBufs &g, uint32_t seed, const int *frame_local, hipStream_t s);
void launch_gl_prepare(const GlBufs &g, hipStream_t s);                  // wss_inv for this F
void launch_gl_iterations(const GlBufs &g, int n_iter, float alpha, float *audio, hipStream_t s);  // + final ISTFT
const float2 *launch_gl_iterate(const GlBufs &g, int n_iter, float alpha, hipStream_t s);         // iterations only
void launch_gl_final(const GlBufs &g, const float2 *ang, float *audio, hipStream_t s);            // final ISTFT
// parity hook: iteration state in the crate's (n_bins x F x 2) layout <-> device [F][nb] float2
void launch_gl_state_import(const GlBufs &g, const float *ang_in, const float *reb_in, hipStream_t s);
void launch_gl_state_export(const GlBufs &g, const float2 *ang, const float2 *tprev, float *ang_out, float *reb_out,
                            hipStream_t s);
void launch_transpose(const float *in, float *out, int rows, int cols, hipStream_t s);
// Ragged row copy: item z (< n <= GEMM_RAGGED_MAX) has rows[z] rows of `cols` floats at src + z * src_stride; they go
// to dst + z * dst_stride (one launch instead of a memcpy per chunk: the post-net's padded layer-0 input)
void launch_copy_rows(const float *src, size_t src_stride, float *dst, size_t dst_stride, const int *rows, int n, int cols,
                      hipStream_t s);

// ---- analysis (analysis.hip): audio -> STFT magnitude -> mel, spectral convergence -----------------------------------------
// One workgroup's share of launch_stft_mag: up to four consecutive frames (one wave each) of ONE utterance, so a launch covers
// the frames of several utterances and a frame never reads another utterance's samples.
struct AnSeg {
  long long abase;  // offset of the utterance's first sample in the concatenated audio
  int n;            // samples of the utterance
  int F;            // its frames, n / hop + 1
  int f0;           // the workgroup's first frame, within the utterance
  int row0;         // row of the utterance's first frame in S / P
};
// S [rows][513] = |STFT|; P [rows][ldp] = S^e with zero padding columns (null: not wanted); nblk rows of segs_dev
void launch_stft_mag(const float *audio, const AnSeg *segs_dev, int nblk, const float2 *tw, const float *win, float *S, float *P,
                     int ldp, float e, hipStream_t s);
// melT [F][n_mels] -> (n_mels x F), mode 0: ln(max(m, floor)), 1: m, 2: log10(max(m, floor)) -- launch_gl_exp_transpose inverted
void launch_mel_compress(const float *melT, float *out_melsxF, int n_mels, int F, int mode, float floor, hipStream_t s);
// sums[0..2] = sum x s, sum x x, sum s s over n cells (x = X, s = St) in fp64, in a fixed order: parts = 3 * SPD_PARTS doubles
constexpr int SPD_PARTS = 256;
void launch_spec_distance(const float *X, const float *St, size_t n, double *parts, double *sums, hipStream_t s);

// ---- prosody (prosody.hip): speaking rate and pitch on the magnitude, between mel -> linear and the loop -------------------------
// S [F][513] -> Sout [Fout][513]: frames resampled by `rate` (linear interpolation in time), then, unless pitch == 1, each frame's
// log fine structure (what a cepstral lifter of `lifter` bins leaves of ln max(., log_floor)) resampled by `pitch` on the frequency
// axis under the unchanged envelope.  Fout = prosody_frames(F, rate) (magnitude_plan.h); F >= 2 unless rate == 1.  One launch.
void launch_prosody(const float *S, float *Sout, int F, int Fout, float rate, float pitch, int lifter, float log_floor,
                    const float2 *tw, hipStream_t s);
// The ragged form, one launch for the utterances of a batch: utterance u's F rows start at row src0 of S, its Fout =
// prosody_frames(F, rate) rows at row dst0 of Sout (dst0 ascending, the utterances back to back: dst0[u + 1] = dst0[u] + Fout[u]);
// Fout_all = the sum.  tab is device memory.  Every row equals what launch_prosody gives for the utterance alone, bit for bit;
// an utterance with rate == pitch == 1 is copied.  (struct ProsodyUtt, ContourUtt, TimbreUtt: magnitude_plan.h)
void launch_prosody_batch(const float *S, float *Sout, const ProsodyUtt *tab, int n_utt, int Fout_all, const float2 *tw, hipStream_t s);
// The contour form (xdtts_prosody_contour), single call (n_utt = 1) and ragged batch in one kernel: utterance u's F rows start at
// row src0 of S, its Fout rows at row dst0 of Sout (ascending, back to back), its frame table at entry tab0 of ftab.  ftab
// (device) = the cumulative slownesses c of all utterances, then their pitches, then their gains (float bits), n_tab entries
// each: ContourTable of prosody_contour.h, concatenated.  identity != 0: the rows are copied, no table is read.
void launch_prosody_contour(const float *S, float *Sout, const ContourUtt *utt, int n_utt, const unsigned *ftab, int n_tab, int Fout_all,
                            const float2 *tw, hipStream_t s);

// ---- timbre (timbre.hip): vocal-tract length and breathiness on the magnitude, behind prosody and in front of the initial phase ----
// S -> Sout, out of place, the same frame counts: utterance u's F rows start at row src0 of S and at row dst0 of Sout (dst0
// ascending, back to back; rows_all = the sum of F); per frame the ENVELOPE of the prosody stage's cepstral split is resampled by
// vtl on the frequency axis and the fine structure fades by `breath` into a noise of (seed, frame inside the utterance, bin)
// (include/xdtts.h, timbre_plan.h).  An utterance with vtl == 1 and breath == 0 is copied.  tab (device memory, n_utt records),
// or nullptr: n_utt = 1 and the record is `one`, a kernel argument -- nothing is uploaded.  One launch of one kernel either
// way; a row has the same bits in both forms.
void launch_timbre(const float *S, float *Sout, const TimbreUtt *tab, int n_utt, const TimbreUtt &one, int rows_all, const float2 *tw,
                   hipStream_t s);

// ---- clean-up stage (denoise.hip): spectral subtraction with a floor, and a tone curve, in front of everything else ----------
// (include/xdtts.h, denoise_plan.h).  tab (device memory, n_utt records: struct DenoiseUtt), or nullptr: n_utt = 1 and the
// record is `one`, a kernel argument -- nothing is uploaded.  A cell has the same bits in both forms.
// k_noise_profile: N [n_utt][513] = per bin the rank-th smallest key of the utterance's rows of S; an utterance that selects
// nothing (no subtraction, or a profile) leaves its row of N untouched.
void launch_noise_profile(const float *S, const DenoiseUtt *tab, int n_utt, const DenoiseUtt &one, float *N, hipStream_t s);
// k_denoise: rows_all rows of S -> Sout; Nsel = the table above, profile [513] and tone [.][513] where a record asks for them.
// stats [n_utt]: `floored` is ADDED to (zero it in front of the launch), the other fields are written.
void launch_denoise(const float *S, float *Sout, const DenoiseUtt *tab, int n_utt, const DenoiseUtt &one, int rows_all, const float *Nsel,
                    const float *profile, const float *tone, DenoiseStats *stats, hipStream_t s);

// ---- pitch tracker (f0.hip): F0 per frame from the magnitude's cepstrum, the utterance's median, pitch targets (include/xdtts.h) ----
// raw[t], strength[t] for every row t < rows of S [rows][513] (the utterances of a batch back to back: a frame needs nothing of
// its neighbours); o, q_lo, q_hi: checked options and their quefrency range (f0_plan.h).  One launch.
void launch_f0_frames(const float *S, int rows, const F0Opts &o, int q_lo, int q_hi, const float2 *tw, float *raw, float *strength,
                      hipStream_t s);
// One workgroup per utterance (struct F0Utt: magnitude_plan.h): f0, ratio (rows as raw), stats[u], and for tab0 >= 0 the table's pitches
// ftab[n_tab + tab0 + t] = clamp(ftab[3 n_tab + tab0 + t] * ratio[t]) -- ftab = the table of launch_prosody_contour with a
// FOURTH array behind the three it reads: the pitches before the target.  ftab may be null where no utterance has a table.
void launch_f0_track(const float *raw, const float *strength, const F0Utt *utts_dev, int n_utt, float threshold, float *f0, float *ratio,
                     F0Stats *stats, unsigned *ftab, int n_tab, hipStream_t s);

// ---- initial phase by Single Pass Spectrogram Inversion (phase_spsi.hip; phase_init mode 1, include/xdtts.h) -----------------
// (SPSI_L, the segments of the scan -- SpsiSeg, SpsiUtt, spsi_segments(F) of one utterance: magnitude_plan.h)
struct SpsiBufs {
  uint2 *map;       // [F][513]     (owner, delta) of every cell
  uint2 *comp;      // [nseg][513]  the segments' composites
  unsigned *entry;  // [nseg][513]  the phase in front of each segment
};
// S [F][513] -> ang = (cos, sin) of the SPSI phase, tprev = 0, and with turns != null the phase itself (uint32, 2^-32 turn),
// all [F][513].  segs_dev / utts_dev == null: one utterance of F frames (nseg = spsi_segments(F), n_utt = 1); else the device
// tables of a batch, F = its rows in all.  chained: some utterance has more than one segment (else two launches instead of four).
// An utterance's result does not depend on what else is in the batch, bit for bit.
void launch_spsi(const float *S, int F, const SpsiSeg *segs_dev, const SpsiUtt *utts_dev, int nseg, int n_utt, bool chained,
                 const SpsiBufs &b, float2 *ang, float2 *tprev, unsigned *turns, hipStream_t s);
// parity hook: turns / ang [F][nb] -> the boundary layout (nb x F)
void launch_spsi_export(const unsigned *turns, const float2 *ang, int F, int nb, unsigned *turns_out, float2 *ang_out, hipStream_t s);

// ---- output rate (resample.hip): 22 050 Hz audio -> rate Q behind the loop, polyphase windowed sinc (include/xdtts.h) ---------
// One utterance of a launch: n samples at x + src0 -> n_out = resample_n_out(n) samples at y + dst0; its workgroups are blk0 ..
// blk0 + ceil(n_out / RESAMPLE_BLOCK) of the table's numbering (ascending, the utterances back to back).
// (struct ResampleUtt: delivery_plan.h)
// nblk workgroups, the first being number blk_base of the table's numbering (a launch may cover a run of consecutive utterances:
// tab_dev points at the first of them, n_utt counts them).  tab_dev == nullptr: the one utterance `one` (blk0 = 0), nothing
// is read but the arguments.  rows_dev = ResampleTable::rows on the device.  An output's bits do not depend on what else the
// launch holds.
void launch_resample(const float *x, float *y, const ResampleUtt *tab_dev, int n_utt, int blk_base, int nblk, const ResampleUtt &one,
                     const float *rows_dev, int L, int M, int Jn, int T4, hipStream_t s);

// ---- loudness (loudness.hip): BS.1770 integrated loudness and true peak of the delivered signal, and the gain to a target ----
// One utterance of a launch: n samples at x + src0.  Its workgroups (LOUD_GROUP samples each) are grp0 .. of the table's
// numbering, its segments (LOUD_SEG samples) seg0 .., its 100 ms sub-blocks sb0 .. -- ascending, the utterances back to back;
// those three also index the scratch arrays below.
// (struct LoudUtt: delivery_plan.h)
struct LoudResult {  // == xdtts_loudness (include/xdtts.h)
  double mean_square, true_peak, sample_peak, gain;
  int blocks, gated;
};
struct LoudBufs {
  double *excl;   // [segments][4]  a segment's state on entry, had its group started from zero
  double *agg;    // [groups][4]    a group's final state from zero
  double *gin;    // [groups][4]    a group's true state on entry
  double *part;   // [segments][2]  sum of y^2 inside the first / the second sub-block a segment touches
  double *sub;    // [sub-blocks]   sum of y^2 per 100 ms
  float2 *peaks;  // [groups]       (true peak, sample peak)
};
// The measurement of `count` utterances (records tab_dev[0 .. count), or `one` by value where tab_dev is null: the single call
// uploads nothing) in four launches: local runs + true peak, the carry, the energy runs, the gates.  res[u] receives utterance
// u's struct; tgt = 0 measures only (gain 1), else the gain rule of loudness_plan.h with tgt and ceil.  n_groups = the
// utterances' groups in all, the first being group grp_base.  No atomics, a fixed order everywhere: res[u] is a function of
// (rate, n, the utterance's samples, tgt, ceil) alone.
void launch_loudness_measure(const float *x, const LoudUtt *tab_dev, int count, int grp_base, int n_groups, const LoudUtt &one,
                             const LoudnessTable *table_dev, const LoudBufs &b, LoudResult *res, int rate, double tgt, double ceil,
                             hipStream_t s);
// x[i] *= (float)res[u].gain over the same utterances, one launch
void launch_loudness_scale(float *x, const LoudUtt *tab_dev, int count, int grp_base, int n_groups, const LoudUtt &one,
                           const LoudResult *res, hipStream_t s);

// ---- limiter (limiter.hip): look-ahead true-peak limiter where the loudness stage scaled (include/xdtts.h, limiter_plan.h) ------
// One utterance of a launch: n samples at x + src0 -> n samples at out + dst0 (out of place).  Its workgroups (LIM_TILE outputs
// each) are tile0 .. of the table's numbering, ascending, the utterances back to back.
// (LimUtt = TileUtt: delivery_plan.h)
struct LimJob {
  const float *taps;       // LoudnessTable::taps on the device
  const float *win;        // the 2 H + 1 weights of limiter_window on the device
  const LoudResult *res;   // per utterance: the kernel reads Z, TP and the gain g0 there and decides `engaged`; null: the
  double gain0;            //   stage alone -- always engaged, g0 = gain0
  double ceil;             // the linear ceiling c
  int H;
};
// Two launches: the stats' initial values (min_gain 1, H, engaged, 0), then k_limit over n_tiles workgroups, the first being
// tile tile_base of the table's numbering (tab_dev == nullptr: the one utterance `one`).  stats[u] / job.res[u] belong to
// record u.  Integer and float-bits atomics on the stats only: out and stats are functions of (the utterance, job) alone.
void launch_limit(const float *x, float *out, const LimUtt *tab_dev, int count, int tile_base, int n_tiles, const LimUtt &one,
                  const LimJob &job, LimiterStats *stats, hipStream_t s);

// ---- compressor (compressor.hip): tent-envelope dynamic range compressor in front of the level stage (include/xdtts.h, compressor_plan.h) ----
// One utterance of a launch: n samples at x + src0 -> n samples at out + dst0 (in place where they are the same place).  Its
// workgroups (COMP_TILE samples each) are tile0 .. of the table's numbering, ascending, the utterances back to back.
// (CompUtt = TileUtt: delivery_plan.h)
// Three launches: the stats' initial values, the tiles' aggregates and the peak, then the samples -- n_tiles workgroups each,
// the first being tile tile_base of the table's numbering (tab_dev == nullptr: the one utterance `one`).  agg holds one
// record per tile of the WHOLE table (index = the table's tile number); stats[u] belongs to record u.  Integer atomics on the
// stats only: out and stats are functions of (the utterance, plan) alone.
void launch_compress(const float *x, float *out, const CompUtt *tab_dev, int count, int tile_base, int n_tiles, const CompUtt &one,
                     const CompPlan &plan, CompAgg *agg, CompressorStats *stats, hipStream_t s);

// ---- silence (silence.hip): edge silence trimmed and pauses capped, the last stage of the delivery chain (include/xdtts.h, silence_plan.h) ----
// One utterance of a launch: n samples at x + src0 -> n_out <= n samples at out + dst0, out of place (SilUtt: delivery_plan.h).
// Its workgroups (SIL_TILE samples each) are tile0 .. of the table's numbering and its windows win0 .., ascending, the utterances
// back to back.  Three launches: the windows' peaks (n_tiles workgroups, the first being tile tile_base; tab_dev == nullptr: the
// one utterance `one`), the plan (one workgroup per utterance), the gather (n_tiles workgroups).  The scratch holds one entry
// per window (pw, wl, wr, woff) and per tile (tpk) of the WHOLE table; stats[u] belongs to record u.  fade_tab: plan.fade gains
// on the device (null where fade is 0).  n_out is decided on the device: nothing waits for the host.
struct SilBufs {
  float *pw, *tpk;
  int *wl, *wr, *woff;
};
void launch_silence(const float *x, float *out, const SilUtt *tab_dev, int count, int tile_base, int n_tiles, const SilUtt &one,
                    const SilPlan &plan, const float *fade_tab, const SilBufs &b, SilenceStats *stats, hipStream_t s);

// ---- stream (stream.hip): utterances joined with their gaps into one stream, faded, levelled, encoded (include/xdtts.h) -------
// ONE launch of k_stream_join: job.tab[0 .. n_utt) on the device, ascending off (stream_plan.h: StreamUtt), the utterances'
// samples at job.src + src0; out = total * sample_bytes bytes, 16-byte aligned -- nothing at or behind that is written.
// job.gain (device memory) is read by the kernel: the measurement that writes it is ordered in front on the stream.
void launch_stream_join(const StreamJob &job, void *out, hipStream_t s);

// ---- durations (durations.hip): per-id durations and start marks from attention_weights_cum behind a decode (durations_plan.h) ----
// Everything on the device.  cum_a / cum_b: [B][T] by slot (cum_b is read only where batched != 0); nframes / n_valid: [B] by
// slot, read by the kernel -- nothing waits for the host; tab [B], utt [n_utt], list [B]: DurPlan's tables; dur / dur_q16 /
// start_q16: DurPlan::n_ids entries; stats [n_utt].  Two launches: one wave per slot, then one wave per utterance.
struct DurationsJob {
  const float *cum_a, *cum_b;
  int B, T, batched, n_utt;
  const int *nframes, *n_valid;
  const DurChunk *tab;
  const DurUtt *utt;
  const int *list;
  uint32_t lo_q16, hi_q16;  // durations_q16 of min_frames / max_frames
  float *dur;
  uint32_t *dur_q16;
  uint64_t *start_q16;
  AlignmentStats *stats;
};
void launch_durations(const DurationsJob &job, hipStream_t s);

}  // namespace xdtts
