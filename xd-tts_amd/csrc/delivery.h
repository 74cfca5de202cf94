// delivery.h -- the delivery chain behind the Griffin-Lim loop as one member of the vocoder handle: its settings, the per-rate
// tables, scratch, record tables and pinned stats of the stages (resample.hip, compressor.hip, loudness.hip, limiter.hip, the
// output normalisation of griffinlim.hip, silence.hip), and the ONE runner every request path goes through.  The arithmetic is delivery_plan.h's.
#pragma once
#include "kernels.h"
#include "runtime.h"

namespace xdtts {

// The checks of the *_plan.h headers know no status codes: "" passes, a message fails with XDTTS_ERR_BAD_ARG
inline void bad_arg_if(const std::string &msg) {
  if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s", msg.c_str());
}

// A pinned host array that grows with the request and stays (stats that travel back behind the audio).  Growing frees: the
// caller's stream is idle.
template <class T>
struct PinnedArray {
  T *p = nullptr;
  size_t n = 0;
  PinnedArray() = default;
  PinnedArray(const PinnedArray &) = delete;
  PinnedArray &operator=(const PinnedArray &) = delete;
  ~PinnedArray() {
    if (p) (void)hipHostFree(p);
  }
  void reserve(size_t count) {
    if (count <= n) return;
    if (p) HIP_CHECK(hipHostFree(p));
    p = nullptr;
    n = 0;
    HIP_CHECK(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
    n = count;
  }
};

struct Delivery {
  hipStream_t stream = nullptr;  // the handle's

  // ---- settings (the setters and getters of api_gl_delivery.cpp) ----
  int out_rate = XDTTS_SAMPLE_RATE;  // 22050 = no resampler
  ResamplePlan out_plan;             // of out_rate (the identity by default): set with it
  float loud_target = NAN, loud_ceiling = NAN;  // NaN target = the loudness stage is off (the default)
  int lim_us = 0;                    // the limiter's look-ahead, 0 = off (the default)
  Compressor comp = compressor_default();
  bool comp_set = false;
  bool loudness_on() const { return !std::isnan(loud_target); }
  // with a look-ahead beside a target AND a ceiling, the measurement forms the gain without the ceiling and k_limit takes
  // k_loud_scale's place, out of place into lim_out
  bool limiter_on() const { return lim_us != 0 && loudness_on() && !std::isnan(loud_ceiling); }
  bool compressor_on() const { return comp_set && !compressor_is_identity(comp); }
  Silence sil = silence_default();   // the silence stage: the last one, out of place into sil_out
  bool sil_set = false;
  bool silence_on() const { return sil_set; }
  // What a request path delivers for n samples of the loop: N' at the handle's rate, n at 22050.
  size_t delivered(size_t n) const { return resample_n_out(out_plan, n); }
  // The stages of a request path under these settings; norm_mode: xdtts_griffinlim_opts.output_normalise; unlevelled: a document
  // at programme level takes its utterances without either level stage.
  DeliveryStages stages(int norm_mode, bool unlevelled) const {
    const bool c = compressor_on();
    return delivery_stages(out_rate, out_plan, c, c ? compressor_plan(comp, out_rate) : CompPlan{}, loudness_on(), limiter_on() ? lim_us : 0,
                           norm_mode, unlevelled, silence_on(), silence_on() ? silence_plan(sil, out_rate) : SilPlan{});
  }

  // ---- per-rate tables: functions of the rate (the limiter's: of H) alone, built on the host once per (handle, rate) and kept on
  // the device; the host copies are the uploads' sources and live as long as the handle ----
  ResamplePlan rs_plan;
  ResampleTable rs_table;
  DevBuf<float> rs_rows;
  LoudnessTable loud_table_host{};  // rate 0 = none yet
  DevBuf<LoudnessTable> loud_table;
  int lim_H = 0;                    // the half width whose window is on the device; 0 = none yet
  std::vector<float> lim_win_host;
  DevBuf<float> lim_win;
  void resample_prepare(int rate);  // (checked by the caller, not the identity)
  void loudness_prepare(int rate);
  void limiter_prepare(int rate, int lookahead_us);  // ... and the loudness table's taps
  int sil_fade = 0;                 // the fade whose gains are on the device; 0 = none yet
  std::vector<float> sil_fade_host;
  DevBuf<float> sil_fade_tab;
  void silence_prepare(const SilPlan &p);  // (the gains are a function of plan.fade alone)

  // ---- scratch: grows with the request and stays; growing drains the stream first ----
  DevBuf<float> rs_in, audio_rs;  // the stage hooks' input; the resampled audio
  DevBuf<double> loud_excl, loud_agg, loud_gin, loud_part, loud_sub;  // the scan's scratch (kernels.h: LoudBufs)
  DevBuf<float2> loud_peaks;
  DevBuf<LoudResult> loud_res;       // one per utterance of a request
  DevBuf<float> lim_out;
  DevBuf<LimiterStats> lim_stats;    // one per utterance
  DevBuf<CompAgg> comp_agg;          // one per tile
  DevBuf<CompressorStats> comp_stats;  // one per utterance
  DevBuf<float> norm_parts;          // GLN_SCRATCH per utterance
  DevBuf<float> sil_out, sil_pw, sil_tpk;  // the stage's output rows; one peak per window, one per tile
  DevBuf<int> sil_wl, sil_wr, sil_woff;    // per window: the scans' scratch, the output offset
  DevBuf<SilenceStats> sil_stats;    // one per utterance
  PinnedArray<LoudResult> loud_host;  // the structs travel back behind the audio
  PinnedArray<LimiterStats> lim_host;
  PinnedArray<CompressorStats> comp_host;
  PinnedArray<SilenceStats> sil_host;

  // ---- the request in flight: its plan (whose vectors are the sources of the record tables' uploads; prepare() returns behind
  // them, so the next prepare() may replace the plan at any time) and the tables on the device ----
  DeliveryPlan plan;
  bool tables = false;  // the launches read the device tables; else record 0 travels as a kernel argument and nothing is uploaded
  DevBuf<ResampleUtt> rs_tab;
  DevBuf<CompUtt> comp_tab;
  DevBuf<LoudUtt> loud_tab;
  DevBuf<LimUtt> lim_tab;
  DevBuf<NormUtt> norm_tab;
  DevBuf<SilUtt> sil_tab;
  // Buffers and per-rate tables for p's stages, in front of the launches.
  void size(const DeliveryPlan &p);
  // size(p), p becomes the plan in place and -- with_tables -- its records go up on the stream, which is drained behind them.
  // Without: one row, whose records travel as kernel arguments; nothing is uploaded or waited for.
  void prepare(DeliveryPlan p, bool with_tables);
  // ... for the single request of n samples of the loop at its audio's start, with the single call's own failures (more than
  // 2^31 - 1 resampled samples, 2^28 or more into the loudness stage)
  void prepare_one(const DeliveryStages &s, size_t n);
  // The stages of rows r0 .. r0 + count of the plan in place, in the fixed order, on the stream: loop_audio (the loop's, where the
  // plan's bases point) -> the delivered rows, which lie at dbase of the returned buffer (loop_audio, audio_rs, lim_out or
  // sil_out).  Behind the silence stage a row holds out_samples() samples, known once its stats have travelled back.
  float *run(float *loop_audio, int r0, int count, float rms_target);
  float *level(float *loop_audio, int r0, int count, float rms_target);  // ... everything in front of the silence stage
  // ... the stages one by one, for run(), the level-1 stream and the hooks of a stage alone
  void resample(const float *src, float *dst, int r0, int count);
  void compress(const float *x, float *out, int r0, int count);
  void measure(const float *x, int r0, int count, bool to_target);  // -> loud_res[r0 ..]; to_target: the gain of the settings, else 1
  void limit(const float *x, int r0, int count, const LimJob &job);  // -> lim_out, lim_stats[r0 ..]
  void trim(const float *x, int r0, int count);                      // -> sil_out, sil_stats[r0 ..]
  // the job of the settings reading loud_res + r0 (res_from_loudness), or of the stage alone with (gain0, ceil)
  LimJob limiter_job(bool res_from_loudness, int r0, double gain0, double ceil) const;
  // the stats of rows r0 .. r0 + count of the stages that ran -> the pinned arrays, on s
  void fetch_stats(int r0, int count, hipStream_t s);
  // What utterance u (the caller's order) of the plan in place delivers: n_out of the silence stage where it ran -- behind a
  // drained fetch_stats -- else dn.
  size_t out_samples(size_t u) const { return plan.stages.sil ? (size_t)sil_host.p[plan.tab_pos[u]].n_out : (size_t)plan.dn[u]; }

  // ---- what the last delivering call measured, in the caller's order (xdtts_griffinlim_last_loudness / _limiter / _compressor /
  // _silence) ----
  std::vector<xdtts_loudness> last_loud;
  std::vector<xdtts_limiter_stats> last_lim;
  std::vector<xdtts_compressor_stats> last_comp;
  std::vector<xdtts_silence_stats> last_sil;
  void push_last(size_t r);  // row r of the last fetch_stats
  void clear_last() { last_loud.clear(), last_lim.clear(), last_comp.clear(), last_sil.clear(); }
};

}  // namespace xdtts
