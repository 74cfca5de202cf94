// delivery_plan.h -- the host arithmetic of the delivery chain behind the Griffin-Lim loop: which stages run (resample, then
// compressor, then output normalisation or loudness with or without the limiter, then the silence stage), where every utterance's delivered samples
// lie, the per-utterance records of the stages' launches with their running workgroup numbers, the totals every buffer is
// sized from, and the launch extents of a run of consecutive rows.  Plain host C++, no HIP: tests/delivery_plan_test.cpp drives
// it on a machine without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "compressor_plan.h"
#include "limiter_plan.h"
#include "loudness_plan.h"
#include "resample_plan.h"
#include "silence_plan.h"

namespace xdtts {

// ---- the records: one utterance of a stage's launch (kernels.h: launch_resample, launch_loudness_measure, launch_limit,
// launch_compress, launch_gl_output_normalise).  A stage's workgroups are numbered over the whole table, ascending, the
// utterances back to back in the table's order.
// n samples at x + src0 -> n_out = resample_n_out(n) samples at y + dst0; workgroups blk0 .. blk0 + ceil(n_out / RESAMPLE_BLOCK)
struct ResampleUtt {
  long long src0, dst0;
  int n, n_out, blk0, pad;
};
// n samples at x + src0; workgroups (LOUD_GROUP samples each) grp0 .., segments (LOUD_SEG samples) seg0 .., 100 ms sub-blocks
// sb0 .. -- those three also index the stage's scratch arrays
struct LoudUtt {
  long long src0;
  int n, grp0, seg0, sb0;
};
// n samples at x + src0 -> n samples at out + dst0; workgroups (tiles) tile0 ..  The limiter's (LIM_TILE outputs each, out of
// place) and the compressor's (COMP_TILE samples, in place where the two are the same place)
struct TileUtt {
  long long src0, dst0;
  int n, tile0;
};
using LimUtt = TileUtt;
using CompUtt = TileUtt;
// the silence stage's: n samples at x + src0 -> at most n samples at out + dst0; workgroups (SIL_TILE samples) tile0 .. index the
// tile peaks, windows win0 .. the per-window scratch
struct SilUtt {
  long long src0, dst0;
  int n, tile0, win0, pad;
};
// the output normaliser's: n samples from `first` (an int2 on the device)
struct NormUtt {
  int first, n;
};

// Which stages a request runs, decided once.  A request path asks delivery_stages(); a hook of one stage alone sets its field.
struct DeliveryStages {
  int rate = RESAMPLE_RATE_IN;  // of the delivered signal
  ResamplePlan rs;              // of `rate` (resampled only)
  bool resampled = false, comp = false, loud = false;
  int lim_us = 0;     // the limiter's look-ahead, 0 = off
  int norm_mode = 0;  // the output normalisation's mode, 0 = off
  CompPlan comp_plan{};
  bool sil = false;   // the silence stage, behind everything else
  SilPlan sil_plan{};
  bool any() const { return resampled || comp || loud || lim_us || norm_mode || sil; }
};
// lim_on needs loud_on (the limiter takes the place of the loudness stage's gain); the loudness rule takes the output
// normalisation's place; unlevelled (a document at programme level takes its utterances so) switches both level stages off.
// The silence stage depends on none of them.
inline DeliveryStages delivery_stages(int rate, const ResamplePlan &rs, bool comp_on, const CompPlan &comp_plan, bool loud_on, int lim_us,
                                      int norm_mode, bool unlevelled, bool sil_on = false, const SilPlan &sil_plan = SilPlan{}) {
  DeliveryStages s;
  s.rate = rate;
  s.rs = rs;
  s.resampled = rate != RESAMPLE_RATE_IN;
  s.comp = comp_on;
  s.comp_plan = comp_plan;
  s.loud = loud_on && !unlevelled;
  s.lim_us = s.loud ? lim_us : 0;
  s.norm_mode = s.loud || unlevelled ? 0 : norm_mode;
  s.sil = sil_on;
  s.sil_plan = sil_plan;
  return s;
}

struct DeliveryPlan {
  DeliveryStages stages;
  // per utterance, in the caller's order: the delivered samples dbase .. dbase + dn (at 22050 the loop's audio where it lies, at
  // another rate the resampled utterances back to back), and its row in every table
  std::vector<int> dn, tab_pos;
  std::vector<long long> dbase;
  // per row, in the layout order; a stage that is off has no records (norm: always)
  std::vector<ResampleUtt> rs;
  std::vector<CompUtt> comp;
  std::vector<LoudUtt> loud;
  std::vector<LimUtt> lim;
  std::vector<NormUtt> norm;
  std::vector<SilUtt> sil;
  // what the buffers are sized from: resampled samples, loudness groups, limiter tiles, compressor tiles, the floats the limiter's
  // output spans (its rows lie where the delivered ones do, and so do the silence stage's), the silence stage's tiles and windows
  size_t rs_total = 0, groups = 0, lim_tiles = 0, comp_tiles = 0, lim_extent = 0, sil_tiles = 0, sil_wins = 0;
};

// base[u] for utterances back to back
inline std::vector<long long> delivery_bases(const std::vector<size_t> &n) {
  std::vector<long long> base(n.size());
  long long at = 0;
  for (size_t u = 0; u < n.size(); ++u) base[u] = at, at += (long long)n[u];
  return base;
}

// n[u] samples of the loop at base[u] of its audio; order: every utterance once, as the rows are laid out (the batch: the order
// its launches finish in, GlBatchPlan::order; a single call or a hook: the identity).  Throws std::length_error where a rate
// other than 22050 takes the delivered samples past 2^31 - 1.
inline DeliveryPlan delivery_plan(const DeliveryStages &s, const std::vector<size_t> &n, const std::vector<long long> &base,
                                  const std::vector<int> &order) {
  DeliveryPlan p;
  p.stages = s;
  const size_t U = n.size();
  p.dn.resize(U);
  p.dbase.resize(U);
  p.tab_pos.assign(U, 0);
  size_t rtot = 0;
  for (size_t u = 0; u < U; ++u) {
    if (s.resampled) {
      p.dbase[u] = (long long)rtot;
      rtot += resample_n_out(s.rs, n[u]);
      if (rtot > (size_t)0x7fffffff) throw std::length_error("batch too large: more than 2^31 - 1 samples at rate " + std::to_string(s.rate));
      p.dn[u] = (int)(rtot - (size_t)p.dbase[u]);
    } else {
      p.dbase[u] = base[u];
      p.dn[u] = (int)n[u];
    }
    p.lim_extent = std::max(p.lim_extent, (size_t)p.dbase[u] + (size_t)p.dn[u]);
  }
  p.rs_total = rtot;
  int blk = 0, grp = 0, seg = 0, sb = 0, tile = 0, ctile = 0, stile = 0, swin = 0;
  for (int u : order) {
    const long long d0 = p.dbase[(size_t)u];
    const int dn = p.dn[(size_t)u];
    p.tab_pos[(size_t)u] = (int)p.norm.size();
    p.norm.push_back({(int)d0, dn});
    if (s.comp) {
      p.comp.push_back({d0, d0, dn, ctile});
      ctile += (int)compressor_tiles((size_t)dn);
    }
    if (s.loud) {
      p.loud.push_back({d0, dn, grp, seg, sb});
      grp += (int)loudness_groups((size_t)dn);
      seg += (int)loudness_segments((size_t)dn);
      sb += (int)loudness_sub_blocks(s.rate, (size_t)dn);
    }
    if (s.lim_us) {
      p.lim.push_back({d0, d0, dn, tile});
      tile += (int)limiter_tiles((size_t)dn);
    }
    if (s.sil) {
      p.sil.push_back({d0, d0, dn, stile, swin, 0});
      stile += (int)silence_tiles((size_t)dn);
      swin += (int)silence_windows((size_t)dn, s.sil_plan.W);
    }
    if (s.resampled) {
      p.rs.push_back({base[(size_t)u], d0, (int)n[(size_t)u], dn, blk, 0});
      blk += (dn + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    }
  }
  p.groups = (size_t)grp, p.lim_tiles = (size_t)tile, p.comp_tiles = (size_t)ctile, p.sil_tiles = (size_t)stile, p.sil_wins = (size_t)swin;
  return p;
}
inline std::vector<int> delivery_identity(size_t n) {
  std::vector<int> o(n);
  std::iota(o.begin(), o.end(), 0);
  return o;
}

// One launch per stage over rows r0 .. r0 + count: each stage's first workgroup and its workgroups in all, and the longest row
struct DeliveryExtents {
  int blk0 = 0, blocks = 0, grp0 = 0, groups = 0, tile0 = 0, tiles = 0, ctile0 = 0, ctiles = 0, n_max = 0, stile0 = 0, stiles = 0;
};
inline DeliveryExtents delivery_extents(const DeliveryPlan &p, int r0, int count) {
  DeliveryExtents e;
  if (count <= 0) return e;
  const size_t a = (size_t)r0, b = (size_t)(r0 + count - 1);
  if (!p.rs.empty()) e.blk0 = p.rs[a].blk0, e.blocks = p.rs[b].blk0 + (p.rs[b].n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK - e.blk0;
  if (!p.loud.empty()) e.grp0 = p.loud[a].grp0, e.groups = p.loud[b].grp0 + (int)loudness_groups((size_t)p.loud[b].n) - e.grp0;
  if (!p.lim.empty()) e.tile0 = p.lim[a].tile0, e.tiles = p.lim[b].tile0 + (int)limiter_tiles((size_t)p.lim[b].n) - e.tile0;
  if (!p.comp.empty()) e.ctile0 = p.comp[a].tile0, e.ctiles = p.comp[b].tile0 + (int)compressor_tiles((size_t)p.comp[b].n) - e.ctile0;
  if (!p.sil.empty()) e.stile0 = p.sil[a].tile0, e.stiles = p.sil[b].tile0 + (int)silence_tiles((size_t)p.sil[b].n) - e.stile0;
  for (size_t r = a; r <= b; ++r) e.n_max = std::max(e.n_max, p.norm[r].n);
  return e;
}

}  // namespace xdtts
