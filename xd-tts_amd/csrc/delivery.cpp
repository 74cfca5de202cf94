// delivery.cpp -- the delivery chain's state and its one runner (delivery.h): per-rate tables, buffers, the record tables' uploads
// and the launches of resample -> compressor -> output normalisation | loudness (-> limiter) -> silence, for a single request and
// a batch.
#include "delivery.h"

namespace xdtts {

static_assert(sizeof(NormUtt) == sizeof(int2) && sizeof(xdtts_loudness) == sizeof(LoudResult) && sizeof(xdtts_limiter_stats) == sizeof(LimiterStats) &&
                  sizeof(xdtts_compressor_stats) == sizeof(CompressorStats) && sizeof(xdtts_silence_stats) == sizeof(SilenceStats), "the records and stats of the kernels are the boundary's, byte for byte");

void Delivery::resample_prepare(int rate) {
  if (rs_table.rate == rate && rs_rows.p) return;
  HIP_CHECK(hipStreamSynchronize(stream));  // (a launch that reads the table of another rate may be in flight)
  const std::string msg = resample_check(rate, &rs_plan);
  if (!msg.empty() || rs_plan.identity) fail(XDTTS_ERR_BAD_ARG, "resample: no table for rate %d", rate);
  std::vector<float> h;
  resample_taps(rs_plan, h);
  rs_table.rate = 0;
  resample_table(rs_plan, h, rs_table);
  if (resample_window(rs_table) > RESAMPLE_WINDOW) {  // (never: the rate rule bounds M / L and the entries per phase)
    rs_table.rate = 0;
    fail(XDTTS_ERR_BAD_ARG, "resample: rate %d needs a window of %d samples", rate, resample_window(rs_table));
  }
  rs_rows.upload(rs_table.rows.data(), rs_table.rows.size(), stream);
}

void Delivery::loudness_prepare(int rate) {
  if (loud_table_host.rate == rate && loud_table.p) return;
  HIP_CHECK(hipStreamSynchronize(stream));  // (a launch that reads the table of another rate may be in flight)
  bad_arg_if(loudness_check(rate));
  loud_table_host.rate = 0;
  loudness_table(rate, loud_table_host);
  loud_table.upload(&loud_table_host, 1, stream);
}

void Delivery::limiter_prepare(int rate, int lookahead_us) {
  bad_arg_if(limiter_check(rate, lookahead_us));
  loudness_prepare(rate);  // (the taps)
  const int H = limiter_half_width(rate, lookahead_us);
  if (H == lim_H && lim_win.p) return;
  HIP_CHECK(hipStreamSynchronize(stream));  // (a launch that reads another window may be in flight)
  lim_H = 0;
  lim_win_host.resize((size_t)(2 * H + 1));
  limiter_window(H, lim_win_host.data());
  lim_win.upload(lim_win_host.data(), lim_win_host.size(), stream);
  lim_H = H;
}

void Delivery::silence_prepare(const SilPlan &p) {
  if (p.fade == 0 || (p.fade == sil_fade && sil_fade_tab.p)) return;
  HIP_CHECK(hipStreamSynchronize(stream));  // (a launch that reads the gains of another fade may be in flight)
  sil_fade = 0;
  sil_fade_host.resize((size_t)p.fade);
  silence_fade_table(p, sil_fade_host.data());
  sil_fade_tab.upload(sil_fade_host.data(), sil_fade_host.size(), stream);
  sil_fade = p.fade;
}

void Delivery::size(const DeliveryPlan &p) {
  const DeliveryStages &s = p.stages;
  const size_t n_utt = std::max<size_t>(p.dn.size(), 1);
  if (s.resampled) {
    audio_rs.alloc(std::max<size_t>(p.rs_total, 1));
    resample_prepare(s.rate);
  }
  if (s.loud) {
    loudness_prepare(s.rate);
    const size_t groups = std::max<size_t>(p.groups, 1), segs = groups * LOUD_LANES;
    if (segs > loud_excl.n / 4 || n_utt > loud_res.n) HIP_CHECK(hipStreamSynchronize(stream));  // (growing frees what a launch may read)
    loud_excl.alloc(segs * 4);
    loud_agg.alloc(groups * 4);
    loud_gin.alloc(groups * 4);
    loud_part.alloc(segs * 2);
    loud_sub.alloc(groups * 3 + n_utt);  // (h >= 800: at most three sub-blocks begin inside a group of 2048, one more per utterance)
    loud_peaks.alloc(groups);
    loud_res.alloc(n_utt);
    loud_host.reserve(n_utt);
  }
  if (s.lim_us) {
    limiter_prepare(s.rate, s.lim_us);
    const size_t floats = std::max<size_t>(p.lim_extent, 1);
    if (floats > lim_out.n || n_utt > lim_stats.n) HIP_CHECK(hipStreamSynchronize(stream));  // (growing frees what a launch may touch)
    lim_out.alloc(floats);
    lim_stats.alloc(n_utt);
    lim_host.reserve(n_utt);
  }
  if (s.comp) {
    const size_t tiles = std::max<size_t>(p.comp_tiles, 1);
    if (tiles > comp_agg.n || n_utt > comp_stats.n) HIP_CHECK(hipStreamSynchronize(stream));  // (growing frees what a launch may touch)
    comp_agg.alloc(tiles);
    comp_stats.alloc(n_utt);
    comp_host.reserve(n_utt);
  }
  if (s.norm_mode) norm_parts.alloc((size_t)GLN_SCRATCH * n_utt);
  if (s.sil) {
    silence_prepare(s.sil_plan);
    const size_t floats = std::max<size_t>(p.lim_extent, 1), wins = std::max<size_t>(p.sil_wins, 1), tiles = std::max<size_t>(p.sil_tiles, 1);
    if (floats > sil_out.n || wins > sil_pw.n || tiles > sil_tpk.n || n_utt > sil_stats.n)
      HIP_CHECK(hipStreamSynchronize(stream));  // (growing frees what a launch may touch)
    sil_out.alloc(floats);
    sil_pw.alloc(wins);
    sil_wl.alloc(wins);
    sil_wr.alloc(wins);
    sil_woff.alloc(wins);
    sil_tpk.alloc(tiles);
    sil_stats.alloc(n_utt);
    sil_host.reserve(n_utt);
  }
}

void Delivery::prepare_one(const DeliveryStages &s, size_t n) {
  const size_t dn = s.resampled ? resample_n_out(s.rs, n) : n;
  if (s.resampled && dn > (size_t)0x7fffffff) fail(XDTTS_ERR_BAD_ARG, "resample: %zu output samples are more than 2^31 - 1", dn);
  if (s.loud && (dn == 0 || dn >= ((size_t)1 << 28))) fail(XDTTS_ERR_BAD_ARG, "loudness: need 1 .. 2^28 - 1 samples, got %zu", dn);
  prepare(delivery_plan(s, {n}, {0}, {0}), false);
}

void Delivery::prepare(DeliveryPlan p, bool with_tables) {
  size(p);
  plan = std::move(p);
  tables = with_tables;
  const DeliveryStages &t = plan.stages;
  if (!tables) return;
  if (t.norm_mode) norm_tab.upload(plan.norm.data(), plan.norm.size(), stream);
  if (t.resampled) rs_tab.upload(plan.rs.data(), plan.rs.size(), stream);
  if (t.loud) loud_tab.upload(plan.loud.data(), plan.loud.size(), stream);
  if (t.lim_us) lim_tab.upload(plan.lim.data(), plan.lim.size(), stream);
  if (t.comp) comp_tab.upload(plan.comp.data(), plan.comp.size(), stream);
  if (t.sil) sil_tab.upload(plan.sil.data(), plan.sil.size(), stream);
  if (t.any()) HIP_CHECK(hipStreamSynchronize(stream));  // the tables are up: the plan's vectors are no upload's source any more
}

// Both launch forms of every stage: the device table from row r0, or -- a single request -- record 0 by value.  count >= 1.
void Delivery::resample(const float *src, float *dst, int r0, int count) {
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  launch_resample(src, dst, tables ? rs_tab.p + r0 : nullptr, count, e.blk0, e.blocks, tables ? ResampleUtt{} : plan.rs[(size_t)r0], rs_rows.p,
                  rs_table.L, rs_table.M, rs_table.Jn, rs_table.T4, stream);
}

void Delivery::compress(const float *x, float *out, int r0, int count) {
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  launch_compress(x, out, tables ? comp_tab.p + r0 : nullptr, count, e.ctile0, e.ctiles, tables ? CompUtt{} : plan.comp[(size_t)r0],
                  plan.stages.comp_plan, comp_agg.p, comp_stats.p + r0, stream);
}

void Delivery::measure(const float *x, int r0, int count, bool to_target) {
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  const LoudBufs b{loud_excl.p, loud_agg.p, loud_gin.p, loud_part.p, loud_sub.p, loud_peaks.p};
  launch_loudness_measure(x, tables ? loud_tab.p + r0 : nullptr, count, e.grp0, e.groups, tables ? LoudUtt{} : plan.loud[(size_t)r0], loud_table.p, b,
                          loud_res.p + r0, plan.stages.rate, to_target ? loudness_target_lin(loud_target) : 0.0,
                          to_target && !plan.stages.lim_us ? loudness_ceiling_lin(loud_ceiling) : 0.0, stream);
}

LimJob Delivery::limiter_job(bool res_from_loudness, int r0, double gain0, double ceil) const {
  return LimJob{&loud_table.p->taps[0][0], lim_win.p, res_from_loudness ? loud_res.p + r0 : nullptr, gain0, ceil, lim_H};
}

void Delivery::limit(const float *x, int r0, int count, const LimJob &job) {
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  launch_limit(x, lim_out.p, tables ? lim_tab.p + r0 : nullptr, count, e.tile0, e.tiles, tables ? LimUtt{} : plan.lim[(size_t)r0], job,
               lim_stats.p + r0, stream);
}

void Delivery::trim(const float *x, int r0, int count) {
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  const SilPlan &sp = plan.stages.sil_plan;
  launch_silence(x, sil_out.p, tables ? sil_tab.p + r0 : nullptr, count, e.stile0, e.stiles, tables ? SilUtt{} : plan.sil[(size_t)r0], sp,
                 sp.fade > 0 ? sil_fade_tab.p : nullptr, SilBufs{sil_pw.p, sil_tpk.p, sil_wl.p, sil_wr.p, sil_woff.p}, sil_stats.p + r0, stream);
}

// THE delivery order: the output rate, then the compressor in place on what is delivered, then the level stage -- the output
// normalisation, or with a target the loudness rule in its place, whose gain the limiter applies out of place where it is on --
// and behind them all the silence stage, out of place, on what the level stage delivered.
float *Delivery::run(float *loop_audio, int r0, int count, float rms_target) {
  float *x = level(loop_audio, r0, count, rms_target);
  if (count <= 0 || !plan.stages.sil) return x;
  trim(x, r0, count);
  return sil_out.p;
}

float *Delivery::level(float *loop_audio, int r0, int count, float rms_target) {
  const DeliveryStages &s = plan.stages;
  float *x = s.resampled ? audio_rs.p : loop_audio;
  if (count <= 0) return x;
  if (s.resampled) resample(loop_audio, x, r0, count);
  if (s.comp) compress(x, x, r0, count);
  const DeliveryExtents e = delivery_extents(plan, r0, count);
  if (s.norm_mode)
    launch_gl_output_normalise(x, tables ? reinterpret_cast<const int2 *>(norm_tab.p + r0) : nullptr, count, tables ? 0 : plan.norm[(size_t)r0].first,
                               e.n_max, s.norm_mode, rms_target, norm_parts.p + (size_t)r0 * GLN_SCRATCH, stream);
  if (!s.loud) return x;
  measure(x, r0, count, true);
  if (s.lim_us) {
    limit(x, r0, count, limiter_job(true, r0, 0.0, loudness_ceiling_lin(loud_ceiling)));
    return lim_out.p;
  }
  launch_loudness_scale(x, tables ? loud_tab.p + r0 : nullptr, count, e.grp0, e.groups, tables ? LoudUtt{} : plan.loud[(size_t)r0], loud_res.p + r0, stream);
  return x;
}

void Delivery::fetch_stats(int r0, int count, hipStream_t s) {
  if (count <= 0) return;
  const DeliveryStages &st = plan.stages;
  if (st.loud) HIP_CHECK(hipMemcpyAsync(loud_host.p + r0, loud_res.p + r0, (size_t)count * sizeof(LoudResult), hipMemcpyDeviceToHost, s));
  if (st.lim_us) HIP_CHECK(hipMemcpyAsync(lim_host.p + r0, lim_stats.p + r0, (size_t)count * sizeof(LimiterStats), hipMemcpyDeviceToHost, s));
  if (st.comp) HIP_CHECK(hipMemcpyAsync(comp_host.p + r0, comp_stats.p + r0, (size_t)count * sizeof(CompressorStats), hipMemcpyDeviceToHost, s));
  if (st.sil) HIP_CHECK(hipMemcpyAsync(sil_host.p + r0, sil_stats.p + r0, (size_t)count * sizeof(SilenceStats), hipMemcpyDeviceToHost, s));
}

void Delivery::push_last(size_t r) {
  const DeliveryStages &st = plan.stages;
  auto push = [](auto &last, const auto *from) {
    last.emplace_back();
    std::memcpy(&last.back(), from, sizeof last.back());
  };
  if (st.loud) push(last_loud, loud_host.p + r);
  if (st.lim_us) push(last_lim, lim_host.p + r);
  if (st.comp) push(last_comp, comp_host.p + r);
  if (st.sil) push(last_sil, sil_host.p + r);
}

}  // namespace xdtts
