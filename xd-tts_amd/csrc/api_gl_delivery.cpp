// api_gl_delivery.cpp -- the extern "C" boundary, vocoder half: the entries of the delivery chain behind the loop -- output rate,
// loudness, limiter, compressor -- and of the stream stage behind it (join).
#include <algorithm>
#include <cmath>

#include "api_gl.h"

using namespace xdtts;

// A hook of ONE stage alone on checked audios: the plan of the audios back to back in the caller's order (delivery_plan.h; a
// single call passes its record by value, a batch uploads the table -- the two launch forms of the request paths), the
// audios up, ev.e[0], the stage, ev.e[1..2], the rows of the buffer it returns to outs (null: none), the stats, the wait.
template <class Stage>
static void stage_hook(xdtts_griffinlim *g, const DeliveryStages &s, const float *const *audios, const size_t *n, int n_utt, float *const *outs,
                       Stage stage) {  // (the caller holds g->mu)
  const std::vector<size_t> nv(n, n + n_utt);
  const std::vector<long long> base = delivery_bases(nv);
  DeliveryPlan plan = delivery_plan_checked(s, nv, base, delivery_identity(nv.size()));
  HIP_CHECK(hipSetDevice(g->device));
  Delivery &dl = g->dl;
  dl.prepare(std::move(plan), n_utt > 1);
  dl.rs_in.alloc(std::max<size_t>((size_t)base.back() + nv.back(), 1));
  for (int u = 0; u < n_utt; ++u)
    if (n[u]) HIP_CHECK(hipMemcpyAsync(dl.rs_in.p + base[(size_t)u], audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, g->stream));
  HIP_CHECK(hipEventRecord(g->ev.e[0], g->stream));
  const float *result = stage(dl);
  HIP_CHECK(hipEventRecord(g->ev.e[1], g->stream));
  HIP_CHECK(hipEventRecord(g->ev.e[2], g->stream));
  for (int u = 0; outs && u < n_utt; ++u)
    if (dl.plan.dn[(size_t)u])
      HIP_CHECK(hipMemcpyAsync(outs[u], result + dl.plan.dbase[(size_t)u], (size_t)dl.plan.dn[(size_t)u] * sizeof(float), hipMemcpyDeviceToHost, g->stream));
  dl.fetch_stats(0, n_utt, g->stream);
  g->finish_timings();  // (drains the stream: the inputs, the table, the outputs and the stats)
}

extern "C" {

// ---- output rate: 22 050 Hz -> 8 .. 96 kHz behind the loop, in front of the output normalisation (resample_plan.h, resample.hip) ----

// The rate rule of the entries: the plan of a supported rate, else XDTTS_ERR_BAD_ARG with the rate and the rule.
static ResamplePlan resample_plan_checked(int32_t rate) {
  ResamplePlan p;
  const std::string msg = resample_check(rate, &p);
  if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "%s (supported: %d .. %d Hz with rate / gcd(rate, %d) <= %d)", msg.c_str(), RESAMPLE_RATE_MIN,
                         RESAMPLE_RATE_MAX, RESAMPLE_RATE_IN, RESAMPLE_L_MAX);
  return p;
}

xdtts_status xdtts_resample_plan(int32_t rate_out, size_t n_in, int32_t *L, int32_t *M, int32_t *half_len, size_t *n_out) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate_out);
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (half_len) *half_len = p.H;
    if (n_out) *n_out = resample_n_out(p, n_in);
  });
}

xdtts_status xdtts_resample_filter(int32_t rate_out, float *taps, size_t cap, size_t *n_taps) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate_out);
    const size_t n = (size_t)2 * (size_t)p.H + 1;
    if (n_taps) *n_taps = n;
    if (!taps && cap == 0) return;  // the size alone
    if (!taps || cap < n) fail(XDTTS_ERR_BAD_ARG, "rate %d has %zu taps, the buffer holds %zu", rate_out, n, cap);
    std::vector<float> h;
    resample_taps(p, h);
    std::memcpy(taps, h.data(), n * sizeof(float));
  });
}

xdtts_status xdtts_griffinlim_set_output_rate(xdtts_griffinlim *g, int32_t rate) {
  return guard([&] {
    const ResamplePlan p = resample_plan_checked(rate);  // the rate first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->dl.out_rate = rate;
    g->dl.out_plan = p;
  });
}

xdtts_status xdtts_griffinlim_get_output_rate(const xdtts_griffinlim *g, int32_t *rate) {
  return guard([&] {
    if (!g || !rate) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *rate = g->dl.out_rate;
  });
}

// What the stage takes in one call: the analysis entries' sample cap per utterance, and 2^31 - 1 output samples in all.
static constexpr size_t RS_MAX_SAMPLES = (size_t)1 << 28;

// Parity hook of the stage alone, single call and ragged batch: the audios one behind the other on the device, ONE k_resample
// launch (the single call passes its record by value, the batch uploads the table), and back.  last_timings: ms[0] = the
// launch alone.  The identity copies and launches nothing.
xdtts_status xdtts_griffinlim_resample_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate_out,
                                             float *const *outs, size_t *n_out) {
  return guard([&] {
    for (int u = 0; n_out && u < n_utt; ++u) n_out[u] = 0;
    const ResamplePlan p = resample_plan_checked(rate_out);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!g || !audios || !n || !outs) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t out_tot = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (n[u] >= RS_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: at most 2^28 - 1 samples, got %zu", u, n[u]);
      if (n[u] && (!audios[u] || !outs[u])) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio", u);
      out_tot += resample_n_out(p, n[u]);
      if (out_tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples at rate %d", rate_out);
    }
    if (p.identity) {  // nothing to launch, no device
      for (int u = 0; u < n_utt; ++u) {
        if (n[u]) std::memcpy(outs[u], audios[u], n[u] * sizeof(float));
        if (n_out) n_out[u] = n[u];
      }
      return;
    }
    DeliveryStages s;
    s.rate = rate_out;
    s.rs = p;
    s.resampled = true;
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, s, audios, n, n_utt, outs, [&](Delivery &dl) {
      if (n_utt > 1 || n[0]) dl.resample(dl.rs_in.p, dl.audio_rs.p, 0, n_utt);
      return dl.audio_rs.p;
    });
    for (int u = 0; n_out && u < n_utt; ++u) n_out[u] = (size_t)g->dl.plan.dn[(size_t)u];
  });
}

xdtts_status xdtts_griffinlim_resample(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate_out, float *out, size_t *n_out) {
  return xdtts_griffinlim_resample_batch(g, &audio, &n, 1, rate_out, &out, n_out);
}

// ---- loudness: BS.1770 integrated loudness under a true-peak ceiling, behind the resampler (loudness_plan.h, loudness.hip) ----

static void loudness_rate_checked(int32_t rate) {
  bad_arg_if(loudness_check(rate));
}

double xdtts_loudness_lufs(const xdtts_loudness *l) { return l ? loudness_lufs(l->mean_square) : -INFINITY; }

xdtts_status xdtts_loudness_plan(int32_t rate, size_t n, int32_t *hop, size_t *n_blocks) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (hop) *hop = loudness_hop(rate);
    if (n_blocks) *n_blocks = loudness_blocks(rate, n);
  });
}

xdtts_status xdtts_loudness_filter(int32_t rate, double coef[10]) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (!coef) fail(XDTTS_ERR_BAD_ARG, "null argument");
    loudness_coef(rate, coef);
  });
}

xdtts_status xdtts_true_peak_filter(float taps[3][24]) {
  return guard([&] {
    if (!taps) fail(XDTTS_ERR_BAD_ARG, "null argument");
    static_assert(LOUD_TP_PHASES == 3 && LOUD_TP_TAPS == 24, "the header's array type");
    loudness_true_peak_taps(taps);
  });
}

xdtts_status xdtts_griffinlim_set_loudness(xdtts_griffinlim *g, float target_lufs, float ceiling_dbtp) {
  return guard([&] {
    bad_arg_if(loudness_target_check(target_lufs, ceiling_dbtp));  // the values first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->dl.loud_target = target_lufs;
    g->dl.loud_ceiling = ceiling_dbtp;
  });
}

xdtts_status xdtts_griffinlim_get_loudness(const xdtts_griffinlim *g, float *target_lufs, float *ceiling_dbtp) {
  return guard([&] {
    if (!g || !target_lufs || !ceiling_dbtp) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *target_lufs = g->dl.loud_target;
    *ceiling_dbtp = g->dl.loud_ceiling;
  });
}

xdtts_status xdtts_griffinlim_last_loudness(const xdtts_griffinlim *g, xdtts_loudness *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->dl.last_loud : nullptr, false, out, cap, n);
}

// Measurement hook of the stage alone, single call and ragged batch: the audios one behind the other on the device, the four
// launches of launch_loudness_measure (the single call passes its record by value, the batch uploads the table), and the
// structs back.  No target, no scaling: gain = 1.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_loudness_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                             xdtts_loudness *out) {
  return guard([&] {
    loudness_rate_checked(rate);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!g || !audios || !n || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t tot = 0;
    for (int u = 0; u < n_utt; ++u) {
      if (n[u] == 0 || n[u] >= RS_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "utterance %d: need 1 .. 2^28 - 1 samples, got %zu", u, n[u]);
      if (!audios[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio", u);
      tot += n[u];
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    DeliveryStages s;
    s.rate = rate;
    s.loud = true;
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, s, audios, n, n_utt, nullptr, [&](Delivery &dl) {
      dl.measure(dl.rs_in.p, 0, n_utt, false);
      return dl.rs_in.p;
    });
    std::memcpy(out, g->dl.loud_host.p, (size_t)n_utt * sizeof(xdtts_loudness));
  });
}

xdtts_status xdtts_griffinlim_loudness(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, xdtts_loudness *out) {
  return xdtts_griffinlim_loudness_batch(g, &audio, &n, 1, rate, out);
}

// ---- limiter: look-ahead true-peak limiter where the loudness stage scaled (limiter_plan.h, limiter.hip) ------------------------

static_assert(sizeof(xdtts_limiter_stats) == sizeof(LimiterStats) && offsetof(xdtts_limiter_stats, limited) == offsetof(LimiterStats, limited),
              "xdtts_limiter_stats and LimiterStats share one layout");

xdtts_status xdtts_limiter_plan(int32_t rate, int32_t lookahead_us, int32_t *half_width, int32_t *tile) {
  return guard([&] {
    bad_arg_if(limiter_check(rate, lookahead_us));
    if (half_width) *half_width = limiter_half_width(rate, lookahead_us);
    if (tile) *tile = LIM_TILE;
  });
}

xdtts_status xdtts_limiter_window(int32_t rate, int32_t lookahead_us, float *w) {
  return guard([&] {
    bad_arg_if(limiter_check(rate, lookahead_us));
    if (!w) fail(XDTTS_ERR_BAD_ARG, "null argument");
    limiter_window(limiter_half_width(rate, lookahead_us), w);
  });
}

xdtts_status xdtts_limiter_reference(const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin, int32_t lookahead_us,
                                     float *out, xdtts_limiter_stats *stats) {
  return guard([&] {
    bad_arg_if(limiter_args_check(rate, lookahead_us, n, gain0, ceiling_lin));
    if (!audio || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const LimiterStats st = limiter_reference(audio, n, rate, lookahead_us, gain0, ceiling_lin, out);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_limiter(xdtts_griffinlim *g, int32_t lookahead_us) {
  return guard([&] {
    bad_arg_if(limiter_setting_check(lookahead_us));  // the value first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->dl.lim_us = lookahead_us;
  });
}

xdtts_status xdtts_griffinlim_get_limiter(const xdtts_griffinlim *g, int32_t *lookahead_us) {
  return guard([&] {
    if (!g || !lookahead_us) fail(XDTTS_ERR_BAD_ARG, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    *lookahead_us = g->dl.lim_us;
  });
}

xdtts_status xdtts_griffinlim_last_limiter(const xdtts_griffinlim *g, xdtts_limiter_stats *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->dl.last_lim : nullptr, false, out, cap, n);
}

// The stage alone, single call and ragged batch: the audios one behind the other on the device, the two launches of
// launch_limit (the single call passes its record by value, the batch uploads the table), the outputs and the stats back.
// Always engaged, g0 = gain0.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_limit_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                          double gain0, double ceiling_lin, int32_t lookahead_us, float *const *outs,
                                          xdtts_limiter_stats *stats) {
  return guard([&] {
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t tot = 0;
    for (int u = 0; u < n_utt; ++u) {
      const std::string msg = limiter_args_check(rate, lookahead_us, n[u], gain0, ceiling_lin);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      tot += n[u];
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    if (!g || !audios || !outs || !stats) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!audios[u] || !outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio / out", u);
    DeliveryStages s;
    s.rate = rate;
    s.lim_us = lookahead_us;
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, s, audios, n, n_utt, outs, [&](Delivery &dl) {
      dl.limit(dl.rs_in.p, 0, n_utt, dl.limiter_job(false, 0, gain0, ceiling_lin));
      return dl.lim_out.p;
    });
    std::memcpy(stats, g->dl.lim_host.p, (size_t)n_utt * sizeof(xdtts_limiter_stats));
  });
}

xdtts_status xdtts_griffinlim_limit(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, double gain0, double ceiling_lin,
                                    int32_t lookahead_us, float *out, xdtts_limiter_stats *stats) {
  return xdtts_griffinlim_limit_batch(g, &audio, &n, 1, rate, gain0, ceiling_lin, lookahead_us, &out, stats);
}

// ---- compressor: tent-envelope dynamic range compressor in front of the level stage (compressor_plan.h, compressor.hip) --------

static_assert(sizeof(xdtts_compressor) == sizeof(Compressor) && offsetof(xdtts_compressor, makeup_db) == offsetof(Compressor, makeup_db),
              "xdtts_compressor and Compressor share one layout");
static_assert(sizeof(xdtts_compressor_stats) == sizeof(CompressorStats) &&
                  offsetof(xdtts_compressor_stats, compressed) == offsetof(CompressorStats, compressed),
              "xdtts_compressor_stats and CompressorStats share one layout");

// the checked setting (null is an error here: the entries that take "off" look at the pointer first)
static Compressor compressor_checked(const xdtts_compressor *c) {
  if (!c) fail(XDTTS_ERR_BAD_ARG, "compressor: null settings");
  Compressor s;
  std::memcpy(&s, c, sizeof s);
  bad_arg_if(compressor_check(s));
  return s;
}

void xdtts_compressor_default(xdtts_compressor *c) {
  if (!c) return;
  const Compressor d = compressor_default();
  std::memcpy(c, &d, sizeof d);
}

xdtts_status xdtts_compressor_preset(int32_t which, xdtts_compressor *out) {
  return guard([&] {
    if (!out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    Compressor p;
    if (!compressor_preset(which, &p)) fail(XDTTS_ERR_BAD_ARG, "compressor: preset %d is not 0 (default) or 1 (drc)", which);
    std::memcpy(out, &p, sizeof p);
  });
}

xdtts_status xdtts_compressor_plan(int32_t rate, const xdtts_compressor *c, int32_t *alpha, int32_t *rho, int32_t *T, int32_t *W,
                                   int32_t *tile) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    bad_arg_if(compressor_rate_check(rate));
    const CompPlan p = compressor_plan(s, rate);
    if (alpha) *alpha = p.alpha;
    if (rho) *rho = p.rho;
    if (T) *T = p.T;
    if (W) *W = p.W;
    if (tile) *tile = COMP_TILE;
  });
}

xdtts_status xdtts_compressor_level(const float *audio, size_t n, int32_t *l) {
  return guard([&] {
    if (n >= COMP_MAX_SAMPLES) fail(XDTTS_ERR_BAD_ARG, "compressor: need at most 2^28 - 1 samples, got %zu", n);
    if (n && (!audio || !l)) fail(XDTTS_ERR_BAD_ARG, "null argument");
    compressor_level(audio, n, l);
  });
}

xdtts_status xdtts_compressor_envelope(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, int32_t *V) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    bad_arg_if(compressor_args_check(s, rate, n));
    if (!audio || !V) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const CompPlan p = compressor_plan(s, rate);
    std::vector<int32_t> l(n);
    compressor_level(audio, n, l.data());
    compressor_envelope_from_level(l.data(), n, p.alpha, p.rho, V);
  });
}

xdtts_status xdtts_compressor_reference(const float *audio, size_t n, int32_t rate, const xdtts_compressor *c, float *out,
                                        xdtts_compressor_stats *stats) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    bad_arg_if(compressor_args_check(s, rate, n));
    if (!audio || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const CompressorStats st = compressor_reference(audio, n, rate, s, out);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_compressor(xdtts_griffinlim *g, const xdtts_compressor *c) {
  return guard([&] {
    Compressor s = compressor_default();
    if (c) s = compressor_checked(c);  // the fields first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->dl.comp = s;
    g->dl.comp_set = c != nullptr;
  });
}

xdtts_status xdtts_griffinlim_get_compressor(const xdtts_griffinlim *g, xdtts_compressor *c, int32_t *on) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    if (c) std::memcpy(c, &g->dl.comp, sizeof g->dl.comp);
    if (on) *on = g->dl.comp_set ? 1 : 0;
  });
}

xdtts_status xdtts_griffinlim_last_compressor(const xdtts_griffinlim *g, xdtts_compressor_stats *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->dl.last_comp : nullptr, false, out, cap, n);
}

// The stage alone, single call and ragged batch: the audios one behind the other on the device, the three launches of
// launch_compress in place (the single call passes its record by value, the batch uploads the table), the outputs and the
// stats back.  The identity touches no device: the inputs' bits, stats of zeros.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_compress_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                             const xdtts_compressor *c, float *const *outs, xdtts_compressor_stats *stats) {
  return guard([&] {
    const Compressor s = compressor_checked(c);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t tot = 0;
    for (int u = 0; u < n_utt; ++u) {
      const std::string msg = compressor_args_check(s, rate, n[u]);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      tot += n[u];
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    if (!g || !audios || !outs || !stats) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!audios[u] || !outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio / out", u);
    if (compressor_is_identity(s)) {
      for (int u = 0; u < n_utt; ++u) {
        if (outs[u] != audios[u]) std::memmove(outs[u], audios[u], n[u] * sizeof(float));
        stats[u] = xdtts_compressor_stats{0.0f, 0, 0, 0};
      }
      return;
    }
    DeliveryStages ds;
    ds.rate = rate;
    ds.comp = true;
    ds.comp_plan = compressor_plan(s, rate);
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, ds, audios, n, n_utt, outs, [&](Delivery &dl) {
      dl.compress(dl.rs_in.p, dl.rs_in.p, 0, n_utt);  // (in place)
      return dl.rs_in.p;
    });
    std::memcpy(stats, g->dl.comp_host.p, (size_t)n_utt * sizeof(xdtts_compressor_stats));
  });
}

xdtts_status xdtts_griffinlim_compress(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, const xdtts_compressor *c,
                                       float *out, xdtts_compressor_stats *stats) {
  return xdtts_griffinlim_compress_batch(g, &audio, &n, 1, rate, c, &out, stats);
}

// ---- silence: edge silence trimmed, pauses capped, behind the level stage (silence_plan.h, silence.hip) -------------------------

static_assert(sizeof(xdtts_silence) == sizeof(Silence) && offsetof(xdtts_silence, fade_ms) == offsetof(Silence, fade_ms),
              "xdtts_silence and Silence share one layout");
static_assert(sizeof(xdtts_silence_stats) == sizeof(SilenceStats) && offsetof(xdtts_silence_stats, any_sound) == offsetof(SilenceStats, any_sound),
              "xdtts_silence_stats and SilenceStats share one layout");

// the checked setting (null is an error here: the entry that takes "off" looks at the pointer first)
static Silence silence_checked(const xdtts_silence *s) {
  if (!s) fail(XDTTS_ERR_BAD_ARG, "silence: null settings");
  Silence v;
  std::memcpy(&v, s, sizeof v);
  bad_arg_if(silence_check(v));
  return v;
}

void xdtts_silence_default(xdtts_silence *s) {
  if (!s) return;
  const Silence d = silence_default();
  std::memcpy(s, &d, sizeof d);
}

xdtts_status xdtts_silence_plan(int32_t rate, const xdtts_silence *s, int32_t *W, int32_t *min_w, int32_t *lead_w, int32_t *trail_w,
                                int32_t *pause_w, int32_t *fade, float *tfac) {
  return guard([&] {
    const Silence v = silence_checked(s);
    bad_arg_if(silence_rate_check(rate));
    const SilPlan p = silence_plan(v, rate);
    if (W) *W = p.W;
    if (min_w) *min_w = p.min_w;
    if (lead_w) *lead_w = p.lead_w;
    if (trail_w) *trail_w = p.trail_w;
    if (pause_w) *pause_w = p.pause_w;
    if (fade) *fade = p.fade;
    if (tfac) *tfac = p.tfac;
  });
}

xdtts_status xdtts_silence_keep(const float *audio, size_t n, int32_t rate, const xdtts_silence *s, uint8_t *keep) {
  return guard([&] {
    const Silence v = silence_checked(s);
    bad_arg_if(silence_args_check(v, rate, n));
    if (!audio || !keep) fail(XDTTS_ERR_BAD_ARG, "null argument");
    silence_keep(audio, n, silence_plan(v, rate), keep);
  });
}

xdtts_status xdtts_silence_reference(const float *audio, size_t n, int32_t rate, const xdtts_silence *s, float *out, xdtts_silence_stats *stats) {
  return guard([&] {
    const Silence v = silence_checked(s);
    bad_arg_if(silence_args_check(v, rate, n));
    if (!audio || !out || audio == out) fail(XDTTS_ERR_BAD_ARG, "null argument (or out == audio: the stage works out of place)");
    const SilenceStats st = silence_reference(audio, n, rate, v, out);
    if (stats) std::memcpy(stats, &st, sizeof st);
  });
}

xdtts_status xdtts_griffinlim_set_silence(xdtts_griffinlim *g, const xdtts_silence *s) {
  return guard([&] {
    Silence v = silence_default();
    if (s) v = silence_checked(s);  // the fields first: reported without a handle
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    g->dl.sil = v;
    g->dl.sil_set = s != nullptr;
  });
}

xdtts_status xdtts_griffinlim_get_silence(const xdtts_griffinlim *g, xdtts_silence *s, int32_t *on) {
  return guard([&] {
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    if (s) std::memcpy(s, &g->dl.sil, sizeof g->dl.sil);
    if (on) *on = g->dl.sil_set ? 1 : 0;
  });
}

xdtts_status xdtts_griffinlim_last_silence(const xdtts_griffinlim *g, xdtts_silence_stats *out, size_t cap, size_t *n) {
  return last_stats_out(g, g ? &g->dl.last_sil : nullptr, false, out, cap, n);
}

// The stage alone, single call and ragged batch: the audios one behind the other on the device, the three launches of
// launch_silence out of place (the single call passes its record by value, the batch uploads the table), the full-length rows
// and the stats back: outs[u] holds n[u] floats, of which stats[u].n_out are the output.  last_timings: ms[0] = the stage alone.
xdtts_status xdtts_griffinlim_trim_batch(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, int32_t rate,
                                         const xdtts_silence *s, float *const *outs, xdtts_silence_stats *stats) {
  return guard([&] {
    const Silence v = silence_checked(s);
    if (n_utt <= 0) fail(XDTTS_ERR_BAD_ARG, "need at least one utterance, got %d", n_utt);
    if (!n) fail(XDTTS_ERR_BAD_ARG, "null argument");
    size_t tot = 0;
    for (int u = 0; u < n_utt; ++u) {
      const std::string msg = silence_args_check(v, rate, n[u]);
      if (!msg.empty()) fail(XDTTS_ERR_BAD_ARG, "utterance %d: %s", u, msg.c_str());
      tot += n[u];
      if (tot > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "batch too large: more than 2^31 - 1 samples");
    }
    if (!g || !audios || !outs || !stats) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (!audios[u] || !outs[u]) fail(XDTTS_ERR_BAD_ARG, "utterance %d: null audio / out", u);
    DeliveryStages ds;
    ds.rate = rate;
    ds.sil = true;
    ds.sil_plan = silence_plan(v, rate);
    std::lock_guard<std::mutex> lk(g->mu);
    stage_hook(g, ds, audios, n, n_utt, outs, [&](Delivery &dl) {
      dl.trim(dl.rs_in.p, 0, n_utt);
      return dl.sil_out.p;
    });
    std::memcpy(stats, g->dl.sil_host.p, (size_t)n_utt * sizeof(xdtts_silence_stats));
  });
}

xdtts_status xdtts_griffinlim_trim(xdtts_griffinlim *g, const float *audio, size_t n, int32_t rate, const xdtts_silence *s, float *out,
                                   xdtts_silence_stats *stats) {
  return xdtts_griffinlim_trim_batch(g, &audio, &n, 1, rate, s, &out, stats);
}

// ---- stream: the sequence joined with its gaps, faded, levelled, encoded (stream_plan.h, stream.hip) ----------------------------

static_assert(sizeof(xdtts_stream_opts) == sizeof(StreamOpts) && offsetof(xdtts_stream_opts, fade) == offsetof(StreamOpts, fade),
              "xdtts_stream_opts and StreamOpts share one layout");

void xdtts_stream_opts_default(xdtts_stream_opts *o) {
  if (!o) return;
  const StreamOpts d = stream_opts_default();
  std::memcpy(o, &d, sizeof d);
}

size_t xdtts_stream_sample_bytes(int32_t format) { return (size_t)stream_sample_bytes(format); }

xdtts_status xdtts_stream_plan(const size_t *n, int32_t n_utt, const size_t *gaps, size_t *offsets, size_t *total) {
  return guard([&] {
    bad_arg_if(stream_plan(n, n_utt, gaps, offsets, total));
  });
}

xdtts_status xdtts_stream_fade_table(int32_t fade, float *w) {
  return guard([&] {
    if (fade < 0 || fade > STREAM_FADE_MAX) fail(XDTTS_ERR_BAD_ARG, "stream: fade %d is not in [0, %d]", fade, STREAM_FADE_MAX);
    if (fade > 0 && !w) fail(XDTTS_ERR_BAD_ARG, "null argument");
    stream_fade_table(fade, w);
  });
}

xdtts_status xdtts_stream_encode_sample(float x, int32_t format, int32_t dither, uint32_t seed, size_t k, void *out) {
  return guard([&] {
    bad_arg_if(stream_opts_check(StreamOpts{format, dither, seed, 0, 0}));
    if (k >= STREAM_TOTAL_MAX) fail(XDTTS_ERR_BAD_ARG, "stream: position %zu is not below 2^28", k);
    if (!out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    const uint32_t b = stream_encode(x, format, dither, seed, (uint32_t)k);
    std::memcpy(out, &b, (size_t)stream_sample_bytes(format));  // (little endian: the low bytes)
  });
}

xdtts_status xdtts_griffinlim_join(xdtts_griffinlim *g, const float *const *audios, const size_t *n, int32_t n_utt, const size_t *gaps,
                                   int32_t rate, const xdtts_stream_opts *o, void *out, size_t cap_bytes, size_t *offsets, size_t *total) {
  return guard([&] {
    if (total) *total = 0;
    const StreamOpts so = stream_opts_checked(o);
    if (so.level == 1) loudness_rate_checked(rate);
    std::vector<size_t> off((size_t)std::max(0, std::min(n_utt, STREAM_UTT_MAX)));
    size_t tot = 0;
    bad_arg_if(stream_plan(n, n_utt, gaps, off.data(), &tot));
    if (!audios || !out) fail(XDTTS_ERR_BAD_ARG, "null argument");
    for (int u = 0; u < n_utt; ++u)
      if (n[u] && !audios[u]) fail(XDTTS_ERR_BAD_ARG, "audios[%d] is null with n[%d] = %zu", u, u, n[u]);
    const size_t bytes = tot * (size_t)stream_sample_bytes(so.format);
    if (cap_bytes < bytes) fail(XDTTS_ERR_BAD_ARG, "cap_bytes %zu: the stream has %zu samples = %zu bytes", cap_bytes, tot, bytes);
    if (!g) fail(XDTTS_ERR_BAD_ARG, "null handle");
    std::lock_guard<std::mutex> lk(g->mu);
    if (so.level == 1 && !g->dl.loudness_on()) fail(XDTTS_ERR_BAD_ARG, "stream: level 1 (programme) needs a loudness target on the handle");
    HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = g->stream;
    HIP_CHECK(hipStreamSynchronize(st));
    g->clear_last();
    // utterance u at a multiple of four floats plus the 16-byte phase of (its host address + its offset): an interior pack of
    // the kernel then reads at the phase of the caller's buffer
    g->st_tab_host.clear();
    size_t at = 0;
    for (int u = 0; u < n_utt; ++u) {
      const size_t phase = ((reinterpret_cast<uintptr_t>(audios[u]) / sizeof(float)) + off[(size_t)u]) & 3u;
      const size_t src0 = ((at + 3) & ~(size_t)3) + phase;
      g->st_tab_host.push_back(StreamUtt{(long long)src0, (uint32_t)off[(size_t)u], (int32_t)n[u]});
      at = src0 + n[u];
    }
    g->st_used = 0;
    g->stream_reserve(std::max<size_t>(at, 1));
    for (int u = 0; u < n_utt; ++u)
      if (n[u]) HIP_CHECK(hipMemcpyAsync(g->st_src.p + g->st_tab_host[(size_t)u].src0, audios[u], n[u] * sizeof(float), hipMemcpyHostToDevice, st));
    g->stream_join(tot, so, rate, g->ev.e[0]);
    HIP_CHECK(hipEventRecord(g->ev.e[1], st));
    HIP_CHECK(hipEventRecord(g->ev.e[2], st));
    HIP_CHECK(hipMemcpyAsync(out, g->st_out.p, bytes, hipMemcpyDeviceToHost, st));
    g->finish_timings();  // (drains the stream: the inputs, the tables, the stream and the struct)
    if (so.level == 1) g->dl.push_last(0);
    for (int u = 0; offsets && u < n_utt; ++u) offsets[u] = off[(size_t)u];
    if (total) *total = tot;
  });
}

}  // extern "C"
