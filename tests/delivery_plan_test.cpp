// delivery_plan_test.cpp -- the delivery chain's host arithmetic (xd-tts_amd/csrc/delivery_plan.h) on the host alone (no HIP, no
// GPU): delivered counts and places against values worked out by hand, the running workgroup numbers of every record table
// under a permuted layout order, the launch extents of runs of rows, the row orders of two multi-launch batches with the runs of
// rows the request path takes launch by launch, and the 2^31 - 1 failure.
// Built and run by tests/test_delivery_plan_cpu.py (plain, and with the address and undefined-behaviour sanitizers); prints "ok".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "delivery_plan.h"
#include "gl_plan.h"

using namespace xdtts;

static std::string g_case;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK(%s)  [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// the loop's samples of up to five utterances: below one compressor tile, exactly one, one sample over, odd, several
static const size_t N_LOOP[5] = {256, 4096, 4097, 12293, 9984};
static const long long BASE[5] = {0, 256, 4352, 8449, 20742};
// ceil(n * 160 / 441) and ceil(n * 320 / 147), by hand
static const int DN_8000[5] = {93, 1487, 1487, 4461, 3623};
static const long long DBASE_8000[5] = {0, 93, 1580, 3067, 7528};
static const int DN_48000[5] = {558, 8917, 8919, 26761, 21734};
static const long long DBASE_48000[5] = {0, 558, 9475, 18394, 45155};

static DeliveryStages all_on(int rate) {
  ResamplePlan rs;
  CHECK(resample_check(rate, &rs).empty());
  Compressor c = compressor_default();
  CHECK(compressor_preset(1, &c));
  return delivery_stages(rate, rs, true, compressor_plan(c, rate), true, 5000, 3, false);
}

static void check_plan(int rate, int n_utt, const std::vector<int> &order, const int *dn_want, const long long *dbase_want) {
  g_case = "rate " + std::to_string(rate) + " n_utt " + std::to_string(n_utt) + " first row " + std::to_string(order[0]);
  const std::vector<size_t> n(N_LOOP, N_LOOP + n_utt);
  const std::vector<long long> base = delivery_bases(n);
  const DeliveryStages s = all_on(rate);
  CHECK(s.resampled == (rate != 22050) && s.comp && s.loud && s.lim_us == 5000 && s.norm_mode == 0);  // loudness takes the normaliser's place
  const DeliveryPlan p = delivery_plan(s, n, base, order);
  CHECK((int)p.dn.size() == n_utt && (int)p.norm.size() == n_utt && (int)p.comp.size() == n_utt && (int)p.loud.size() == n_utt &&
        (int)p.lim.size() == n_utt && p.rs.size() == (s.resampled ? (size_t)n_utt : 0));
  size_t extent = 0;
  for (int u = 0; u < n_utt; ++u) {
    CHECK(base[(size_t)u] == BASE[u]);
    CHECK(p.dn[(size_t)u] == dn_want[u] && p.dbase[(size_t)u] == dbase_want[u]);
    extent = std::max(extent, (size_t)(dbase_want[u] + dn_want[u]));
  }
  CHECK(p.lim_extent == extent && p.rs_total == (s.resampled ? extent : 0));
  // every record's running numbers = the sum of its predecessors' extents in layout order; row r is utterance order[r]
  int blk = 0, grp = 0, seg = 0, sb = 0, tile = 0, ctile = 0;
  for (int r = 0; r < n_utt; ++r) {
    const int u = order[(size_t)r], dn = dn_want[u];
    const long long d0 = dbase_want[u];
    CHECK(p.tab_pos[(size_t)u] == r);
    CHECK(p.norm[(size_t)r].first == (int)d0 && p.norm[(size_t)r].n == dn);
    const CompUtt &c = p.comp[(size_t)r];
    CHECK(c.src0 == d0 && c.dst0 == d0 && c.n == dn && c.tile0 == ctile);
    const LoudUtt &l = p.loud[(size_t)r];
    CHECK(l.src0 == d0 && l.n == dn && l.grp0 == grp && l.seg0 == seg && l.sb0 == sb);
    const LimUtt &m = p.lim[(size_t)r];
    CHECK(m.src0 == d0 && m.dst0 == d0 && m.n == dn && m.tile0 == tile);
    if (s.resampled) {
      const ResampleUtt &q = p.rs[(size_t)r];
      CHECK(q.src0 == BASE[u] && q.dst0 == d0 && q.n == (int)N_LOOP[u] && q.n_out == dn && q.blk0 == blk && q.pad == 0);
    }
    blk += (dn + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
    grp += (int)loudness_groups((size_t)dn);
    seg += (int)loudness_segments((size_t)dn);
    sb += (int)loudness_sub_blocks(rate, (size_t)dn);
    tile += (int)limiter_tiles((size_t)dn);
    ctile += (int)compressor_tiles((size_t)dn);
  }
  CHECK(p.groups == (size_t)grp && p.lim_tiles == (size_t)tile && p.comp_tiles == (size_t)ctile);
  // any consecutive run of `order` is a run of consecutive rows, and its launch extents are the sums over those rows
  for (int r0 = 0; r0 < n_utt; ++r0)
    for (int count = 1; r0 + count <= n_utt; ++count) {
      int blocks = 0, groups = 0, tiles = 0, ctiles = 0, n_max = 0;
      for (int r = r0; r < r0 + count; ++r) {
        const int dn = dn_want[order[(size_t)r]];
        CHECK(p.tab_pos[(size_t)order[(size_t)r]] == r0 + (r - r0));
        blocks += (dn + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK;
        groups += (int)loudness_groups((size_t)dn);
        tiles += (int)limiter_tiles((size_t)dn);
        ctiles += (int)compressor_tiles((size_t)dn);
        n_max = std::max(n_max, dn);
      }
      const DeliveryExtents e = delivery_extents(p, r0, count);
      CHECK(e.groups == groups && e.grp0 == p.loud[(size_t)r0].grp0 && e.tiles == tiles && e.tile0 == p.lim[(size_t)r0].tile0);
      CHECK(e.ctiles == ctiles && e.ctile0 == p.comp[(size_t)r0].tile0 && e.n_max == n_max);
      if (s.resampled) CHECK(e.blocks == blocks && e.blk0 == p.rs[(size_t)r0].blk0);
      else CHECK(e.blocks == 0 && e.blk0 == 0);
    }
  const DeliveryExtents none = delivery_extents(p, 0, 0);
  CHECK(none.blocks == 0 && none.groups == 0 && none.tiles == 0 && none.ctiles == 0 && none.n_max == 0);
}

static void check_stages() {
  g_case = "stages";
  ResamplePlan id;
  const CompPlan cp{};
  DeliveryStages s = delivery_stages(22050, id, false, cp, false, 0, 3, false);  // the default handle: the normaliser alone
  CHECK(!s.resampled && !s.comp && !s.loud && s.lim_us == 0 && s.norm_mode == 3 && s.any());
  s = delivery_stages(22050, id, false, cp, false, 0, 0, false);
  CHECK(!s.any());
  s = delivery_stages(22050, id, true, cp, true, 5000, 3, true);  // a document at programme level: neither level stage
  CHECK(s.comp && !s.loud && s.lim_us == 0 && s.norm_mode == 0);
  s = delivery_stages(22050, id, false, cp, false, 5000, 2, false);  // a look-ahead without a target: no limiter
  CHECK(!s.loud && s.lim_us == 0 && s.norm_mode == 2);
  // a stage that is off has no records; the normaliser's rows are the delivered ones
  const std::vector<size_t> n(N_LOOP, N_LOOP + 2);
  const DeliveryPlan p = delivery_plan(s, n, delivery_bases(n), delivery_identity(2));
  CHECK(p.rs.empty() && p.comp.empty() && p.loud.empty() && p.lim.empty() && p.norm.size() == 2 && p.norm[1].first == 256 && p.norm[1].n == 4096);
  CHECK(p.rs_total == 0 && p.groups == 0 && p.lim_tiles == 0 && p.comp_tiles == 0 && p.lim_extent == 4352);
}

// 11025 Hz halves the count (L = 1, M = 2): sixteen utterances of 268435454 samples deliver 134217727 each, 2147483632 in all
static bool too_large(size_t last) {
  ResamplePlan rs;
  CHECK(resample_check(11025, &rs).empty() && rs.L == 1 && rs.M == 2);
  DeliveryStages s;
  s.rate = 11025;
  s.rs = rs;
  s.resampled = true;
  std::vector<size_t> n(16, 268435454);
  n.push_back(last);
  try {
    const DeliveryPlan p = delivery_plan(s, n, delivery_bases(n), delivery_identity(n.size()));
    CHECK(p.rs_total == (size_t)2147483632 + (last + 1) / 2 && p.dbase[16] == 2147483632LL);
    return false;
  } catch (const std::length_error &e) {
    CHECK(std::string(e.what()) == "batch too large: more than 2^31 - 1 samples at rate 11025");
    return true;
  }
}

// The row orders of real multi-launch batches (gl_plan.h: GlBatchPlan::order at 256 CUs; the batches A and C of
// tests/vocoder_batches.py): the request path runs every stage once per launch over the rows of that launch's riders, then once
// per alone utterance.  Those runs of rows are consecutive, start where the previous one ended, and their extents tile every
// stage's workgroup range exactly once.
static void check_batch_orders() {
  std::vector<int> A = {1000, 1001, 999, 5, 17}, C;
  for (int i = 0; i < 70; ++i) C.push_back(16 + (7 * i) % 23);
  const int forces[3] = {41, 42, 8};
  const int rates[3] = {22050, 8000, 48000};
  for (const std::vector<int> *Fu : {&A, &C})
    for (int force : forces)
      for (int rate : rates) {
        g_case = "batch of " + std::to_string(Fu->size()) + " force " + std::to_string(force) + " rate " + std::to_string(rate);
        const GlBatchPlan gp = gl_batch_plan(*Fu, 256, 256, 2, 0, force);
        const int n_utt = (int)Fu->size();
        CHECK((int)gp.order.size() == n_utt);
        if (Fu == &A) CHECK(gp.launches.size() == (force == 41 ? 3u : 2u) && gp.order != delivery_identity(5));
        else CHECK(gp.launches.size() == (force == 42 ? 1u : 2u) && gp.order != delivery_identity(70));
        std::vector<size_t> n;
        for (int F : *Fu) n.push_back((size_t)256 * (size_t)(F - 1));
        DeliveryStages s = all_on(rate);
        s.sil = true;
        s.sil_plan = silence_plan(silence_default(), rate);
        const DeliveryPlan p = delivery_plan(s, n, delivery_bases(n), gp.order);
        std::vector<std::vector<int>> fetches;
        for (const GlBatchPlan::Launch &L : gp.launches) fetches.push_back(L.utts);
        for (int u = 0; u < n_utt; ++u)
          if (!gp.batched[(size_t)u]) fetches.push_back(std::vector<int>(1, u));
        int row = 0, blk = 0, grp = 0, tile = 0, ctile = 0, stile = 0;
        std::vector<int> seen((size_t)n_utt, 0);
        for (const std::vector<int> &utts : fetches) {
          const int r0 = p.tab_pos[(size_t)utts[0]], count = (int)utts.size();
          CHECK(r0 == row);
          int n_max = 0;
          for (int i = 0; i < count; ++i) {
            CHECK(p.tab_pos[(size_t)utts[(size_t)i]] == r0 + i && gp.order[(size_t)(r0 + i)] == utts[(size_t)i]);
            CHECK(p.norm[(size_t)(r0 + i)].first == (int)p.dbase[(size_t)utts[(size_t)i]] && p.norm[(size_t)(r0 + i)].n == p.dn[(size_t)utts[(size_t)i]]);
            n_max = std::max(n_max, p.dn[(size_t)utts[(size_t)i]]);
            ++seen[(size_t)utts[(size_t)i]];
          }
          const DeliveryExtents e = delivery_extents(p, r0, count);
          CHECK(e.grp0 == grp && e.tile0 == tile && e.ctile0 == ctile && e.stile0 == stile && e.n_max == n_max);
          CHECK(e.groups > 0 && e.tiles > 0 && e.ctiles > 0 && e.stiles > 0);
          if (s.resampled) CHECK(e.blk0 == blk && e.blocks > 0);
          else CHECK(e.blk0 == 0 && e.blocks == 0);
          row += count, blk += e.blocks, grp += e.groups, tile += e.tiles, ctile += e.ctiles, stile += e.stiles;
        }
        for (int u = 0; u < n_utt; ++u) CHECK(seen[(size_t)u] == 1);
        CHECK(row == n_utt && (size_t)grp == p.groups && (size_t)tile == p.lim_tiles && (size_t)ctile == p.comp_tiles && (size_t)stile == p.sil_tiles);
        if (s.resampled) CHECK(blk == p.rs.back().blk0 + (p.rs.back().n_out + RESAMPLE_BLOCK - 1) / RESAMPLE_BLOCK);
      }
}

int main() {
  check_stages();
  check_batch_orders();
  const std::vector<std::vector<int>> orders[3] = {{{0}}, {{0, 1}, {1, 0}}, {{0, 1, 2, 3, 4}, {3, 0, 4, 1, 2}, {4, 3, 2, 1, 0}}};
  const int counts[3] = {1, 2, 5};
  for (int k = 0; k < 3; ++k)
    for (const std::vector<int> &order : orders[k]) {
      int dn22[5];
      for (int u = 0; u < 5; ++u) dn22[u] = (int)N_LOOP[u];
      check_plan(22050, counts[k], order, dn22, BASE);
      check_plan(8000, counts[k], order, DN_8000, DBASE_8000);
      check_plan(48000, counts[k], order, DN_48000, DBASE_48000);
    }
  g_case = "2^31 - 1";
  CHECK(!too_large(29) && !too_large(30));  // 15 more: 2^31 - 1 delivered samples, at the limit
  CHECK(too_large(31) && too_large(32));    // 16 more: one sample beyond
  std::puts("ok");
  return 0;
}
