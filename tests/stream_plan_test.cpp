// Stand-alone driver of csrc/stream_plan.h (plain g++, built with -fsanitize=address,undefined by tests/test_stream_cpu.py):
// the plan against its definition, the argument rules, and the walk of k_stream_join -- tiles, the record cache of a tile, the
// owner search, the three routes of a pack, the last partial pack -- run on the host exactly as the kernel runs it, into buffers
// of the exact size (the sanitizer sees every index), and compared byte for byte with the sample-by-sample definition.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stream_plan.h"

using namespace xdtts;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);          \
      ++failures;                                                  \
    }                                                              \
  } while (0)

struct Case {
  std::vector<size_t> n, gaps;
  int fade, phase;  // phase: floats by which every utterance's source is moved off a 16-byte boundary
};

static float sample(size_t u, size_t i) { return 0.9f * std::sin(0.37f * (float)i + (float)u) + ((i % 7 == 3) ? 0.05f : -0.01f); }

// the definition, sample by sample: the owner by a linear scan
static void definition(const Case &c, const std::vector<size_t> &off, size_t total, const std::vector<std::vector<float>> &x,
                       const std::vector<float> &T, const StreamOpts &o, const float *gain, std::vector<unsigned char> &out) {
  const int sb = stream_sample_bytes(o.format);
  out.assign(total * (size_t)sb, 0);
  for (size_t k = 0; k < total; ++k) {
    uint32_t b = stream_silence(o.format);
    for (size_t u = 0; u < c.n.size(); ++u)
      if (k >= off[u] && k < off[u] + c.n[u]) {
        const float y = stream_shape(x[u][k - off[u]], (int)(k - off[u]), (int)c.n[u], o.fade, T.empty() ? nullptr : T.data(), gain != nullptr, gain ? *gain : 1.0f);
        b = stream_encode(y, o.format, o.dither, o.dither_seed, (uint32_t)k);
      }
    std::memcpy(&out[k * (size_t)sb], &b, (size_t)sb);
  }
}

template <int FORMAT>
static void walk(const StreamJob &J, std::vector<unsigned char> &out) {
  const int sb = stream_sample_bytes(FORMAT), P = STREAM_PACK_BYTES / sb;
  const uint32_t n_packs = stream_packs(J.total, FORMAT), tiles = stream_tiles(J.total, FORMAT);
  CHECK((size_t)tiles * STREAM_TILE_PACKS >= n_packs && (size_t)(tiles - 1) * STREAM_TILE_PACKS < n_packs);
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    const uint32_t pack0 = tile * (uint32_t)STREAM_TILE_PACKS;
    const StreamCache c = stream_cache_plan(J.tab, J.n_utt, pack0 * (uint32_t)P);
    CHECK(c.u0 >= 0 && c.cnt >= 1 && c.cnt <= STREAM_CACHE && c.u0 + c.cnt <= J.n_utt);
    std::vector<StreamUtt> cache(J.tab + c.u0, J.tab + c.u0 + c.cnt);  // exactly the records a workgroup loads
    for (int s = 0; s < STREAM_STEPS; ++s)
      for (int lane = 0; lane < STREAM_WG; ++lane) {
        const uint32_t pack = pack0 + (uint32_t)(s * STREAM_WG + lane);
        if (pack >= n_packs) continue;
        uint32_t w[4];
        stream_pack<FORMAT>(J, cache.data(), c, pack, w);
        const size_t k0 = (size_t)pack * P, valid = k0 + P <= J.total ? (size_t)P : J.total - k0;
        CHECK(valid >= 1 && (k0 + valid) * sb <= out.size());
        std::memcpy(&out[k0 * sb], w, valid * sb);
      }
  }
}

static void run_case(const Case &c, const char *name) {
  const int U = (int)c.n.size();
  std::vector<size_t> off(U);
  size_t total = 0;
  CHECK(stream_plan(c.n.data(), U, c.gaps.empty() ? nullptr : c.gaps.data(), off.data(), &total).empty());
  size_t at = c.gaps.empty() ? 0 : c.gaps[0];
  for (int u = 0; u < U; ++u) {  // the plan against its definition
    CHECK(off[u] == at);
    at += c.n[u] + (c.gaps.empty() ? 0 : c.gaps[u + 1]);
  }
  CHECK(total == at);
  // the sources back to back as the entries stage them, in a buffer of the exact size
  std::vector<std::vector<float>> x(U);
  std::vector<StreamUtt> tab;
  size_t cur = 0;
  for (int u = 0; u < U; ++u) {
    x[u].resize(c.n[u]);
    for (size_t i = 0; i < c.n[u]; ++i) x[u][i] = sample((size_t)u, i);
    const size_t src0 = ((cur + 3) & ~(size_t)3) + ((off[u] + (size_t)c.phase) & 3u);
    tab.push_back(StreamUtt{(long long)src0, (uint32_t)off[u], (int32_t)c.n[u]});
    cur = src0 + c.n[u];
  }
  float *src = (float *)std::aligned_alloc(16, std::max<size_t>((cur * sizeof(float) + 15) / 16, 1) * 16);
  float *src_exact = src;  // (the size is a multiple of the alignment: at most 12 bytes behind the last sample)
  for (int u = 0; u < U; ++u)
    if (c.n[u]) std::memcpy(src_exact + tab[u].src0, x[u].data(), c.n[u] * sizeof(float));
  std::vector<float> T((size_t)c.fade);
  if (c.fade) stream_fade_table(c.fade, T.data());
  const double gain64 = 0.7312345;
  const float gain32 = (float)gain64;
  for (int fmt = 0; fmt < 4; ++fmt)
    for (int variant = 0; variant < 3; ++variant) {  // plain; programme gain; dither (PCM16 only)
      if (variant == 2 && fmt != STREAM_PCM16) continue;
      StreamOpts o{fmt, variant == 2, 12345u, variant == 1, c.fade};
      CHECK(stream_opts_check(o).empty());
      StreamJob J{};
      J.src = src_exact;
      J.tab = tab.data();
      J.fade_tab = c.fade ? T.data() : nullptr;
      J.gain = variant == 1 ? &gain64 : nullptr;
      J.n_utt = U;
      J.total = (uint32_t)total;
      J.format = fmt;
      J.dither = o.dither;
      J.seed = o.dither_seed;
      J.fade = c.fade;
      std::vector<unsigned char> want, got(total * (size_t)stream_sample_bytes(fmt), 0x5A);
      definition(c, off, total, x, T, o, variant == 1 ? &gain32 : nullptr, want);
      switch (fmt) {
        case STREAM_F32: walk<STREAM_F32>(J, got); break;
        case STREAM_PCM16: walk<STREAM_PCM16>(J, got); break;
        case STREAM_ULAW: walk<STREAM_ULAW>(J, got); break;
        default: walk<STREAM_ALAW>(J, got); break;
      }
      if (got != want) {
        size_t i = 0;
        while (got[i] == want[i]) ++i;
        std::printf("FAILED %s: format %d variant %d differs at byte %zu of %zu\n", name, fmt, variant, i, want.size());
        ++failures;
      }
    }
  std::free(src);
}

int main() {
  // ---- one sample: known answers ----
  CHECK(stream_cast_i16(1.0f * 32767.0f) == 32767 && stream_cast_i16(-40000.f) == -32768 && stream_cast_i16(NAN) == 0 && stream_cast_i16(-0.99f) == 0);
  CHECK(stream_ulaw(0) == 0xFF && stream_alaw(0) == 0xD5 && stream_ulaw(-1) == 0x7F && stream_alaw(-1) == 0x55);
  CHECK(stream_ulaw(32767) == 0x80 && stream_ulaw(-32768) == 0x00 && stream_alaw(32767) == 0xAA && stream_alaw(-32768) == 0x2A);
  for (int q = 1; q <= 32767; ++q) {
    if (stream_ulaw(-q) != (stream_ulaw(q) ^ 0x80u) || stream_alaw(-q) != (stream_alaw(q) ^ 0x80u)) {
      CHECK(!"mirror");
      break;
    }
  }
  for (uint32_t k = 0; k < 4096; ++k) {
    const float d = stream_dither(7u, k);
    if (!(d > -1.0f && d < 1.0f)) CHECK(!"dither range");
  }
  CHECK(stream_sample_bytes(0) == 4 && stream_sample_bytes(1) == 2 && stream_sample_bytes(2) == 1 && stream_sample_bytes(3) == 1 && stream_sample_bytes(4) == 0);
  // ---- the argument rules ----
  {
    size_t n1[1] = {0}, big[2] = {((size_t)1 << 28) - 1, 1}, tot = 7, huge[1] = {~(size_t)0};
    std::vector<size_t> many(4097, 1);
    CHECK(!stream_plan(n1, 0, nullptr, nullptr, &tot).empty() && tot == 0);
    CHECK(!stream_plan(many.data(), 4097, nullptr, nullptr, nullptr).empty());
    CHECK(stream_plan(many.data(), 4096, nullptr, nullptr, &tot).empty() && tot == 4096);
    CHECK(!stream_plan(n1, 1, nullptr, nullptr, nullptr).empty());                      // total 0
    CHECK(stream_plan(big, 1, nullptr, nullptr, &tot).empty() && tot == ((size_t)1 << 28) - 1);
    CHECK(stream_plan(big, 2, nullptr, nullptr, &tot).find("n[1]") != std::string::npos);  // total 2^28
    CHECK(stream_plan(n1, 1, big, nullptr, &tot).find("gaps[1]") != std::string::npos);
    CHECK(stream_plan(huge, 1, nullptr, nullptr, &tot).find("n[0]") != std::string::npos);  // (no overflow on the way)
    CHECK(!stream_opts_check(StreamOpts{4, 0, 0, 0, 0}).empty() && !stream_opts_check(StreamOpts{-1, 0, 0, 0, 0}).empty());
    CHECK(!stream_opts_check(StreamOpts{2, 1, 0, 0, 0}).empty() && !stream_opts_check(StreamOpts{0, 1, 0, 0, 0}).empty());
    CHECK(!stream_opts_check(StreamOpts{1, 0, 0, 0, 4801}).empty() && stream_opts_check(StreamOpts{1, 1, 0, 1, 4800}).empty());
    CHECK(!stream_opts_check(StreamOpts{1, 0, 0, 2, 0}).empty() && !stream_opts_check(StreamOpts{1, 2, 0, 0, 0}).empty());
  }
  // ---- the walk ----
  run_case(Case{{1}, {}, 0, 0}, "one sample");
  run_case(Case{{1, 2, 7, 15, 16, 17, 33}, {0, 1, 3, 0, 16, 5, 0, 2}, 5, 0}, "small mix");
  {
    Case c{{}, {}, 1, 0};  // 300 utterances of 1 .. 3 samples, gaps 0 .. 2: packs that span several, more records than the cache holds
    uint32_t s = 1;
    c.gaps.push_back(2);
    for (int u = 0; u < 300; ++u) {
      s = mix32(s + 17u);
      c.n.push_back(1 + s % 3);
      c.gaps.push_back((s >> 8) % 3);
    }
    run_case(c, "many tiny");
  }
  for (int phase = 0; phase < 4; ++phase) {
    // one utterance across three tiles of every format (a G.711 tile is 16384 samples), a leading and a trailing gap; then a
    // zero-length utterance in the middle and last packs of 1, 3 and 15 samples
    run_case(Case{{2 * 16384 + 999}, {37, 41}, 64, phase}, "three tiles");
    run_case(Case{{40, 0, 0, 23, 50}, {3, 0, 5, 0, 0, 0}, 64, phase}, "zero length");
    run_case(Case{{4097}, {}, 4800, phase}, "4097");
    run_case(Case{{8195}, {}, 0, phase}, "8195");
    run_case(Case{{16399}, {}, 0, phase}, "16399");
  }
  run_case(Case{{9600, 9601, 3}, {0, 7, 0, 0}, 4800, 0}, "fade 4800");
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
