// durations_plan.h -- the host arithmetic of the durations stage (xdtts_durations_opts; the definition: include/xdtts.h): the
// argument rules, the layout of the output -- per utterance its chunks' valid ids back to back, in the caller's order -- the
// chunk table the kernel reads, the serial reference, and the two maps from ids to frames and from frames to samples.
// Plain C++, no HIP and none of the library's headers but resample_plan.h: tests/durations_plan_test.cpp drives it with plain
// g++.  What the device shares carries DUR_HD: durations.hip's kernels convert with durations_q16.
//
// What the stage reads: after a decode, attention_weights_cum of chunk slot j (the sum of that chunk's softmax rows over the
// frames it ran; a stopped chunk is frozen) -- awc[j][t] is the number of frames the decoder spent on id t, a SOFT duration.
//   row     slot j (decode order) is the caller's chunk order[j].  The batched kernels ping-pong the cumulative weights by step
//           parity: step s reads buffer (s & 1) and writes the other, so after nframes[j] steps the final row of slot j is in
//           cum_b where nframes[j] is odd and in cum_a where it is even.  Every other engine: cum_a.
//   mask    positions t >= n_valid[j] are padding: nothing is emitted for them
//   dur     the fp32 cumulative weight as read;  dur_q16 = durations_q16(dur): ONE exactly scaled float, ONE rounding
//   start   65536 * (frames of the utterance's earlier chunks) + the exclusive prefix sum of dur_q16 inside the chunk; integers
//           only, 64 bits: the result does not depend on the order of the scan
//   stats   integer compares and adds on the Q16 values, per utterance
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "resample_plan.h"

#ifdef __HIPCC__
#define DUR_HD __host__ __device__ __attribute__((always_inline))
#else
#define DUR_HD
#endif

namespace xdtts {

constexpr int DUR_T_MAX = 512;          // ids of a chunk: T_MAX of the decoder
constexpr int DUR_B_MAX = 4096;         // chunks of a request
constexpr int DUR_FRAMES_MAX = 100000;  // frames of a chunk: the bound of max_steps
constexpr int DUR_HOP = 256;            // samples per frame of the vocoder's loop

struct DurationsOpts {  // == xdtts_durations_opts
  int32_t on;
  float min_frames, max_frames;
};

struct AlignmentStats {  // == xdtts_alignment_stats
  uint64_t sum_q16;   // sum of dur_q16 over the utterance's ids
  uint64_t n_frames;  // frames of the utterance's chunks
  uint32_t n_ids;
  uint32_t min_q16, min_index;  // the shortest id (the first of equals) and its index in the utterance
  uint32_t max_q16, max_index;  // the longest id (the first of equals)
  uint32_t n_below, n_above;    // ids with dur_q16 < q16(min_frames) / > q16(max_frames)
  uint32_t last_q16;            // the final id's duration: did the attention reach the end?
};

inline DurationsOpts durations_default() { return DurationsOpts{0, 0.5f, 40.0f}; }

// round-to-nearest-even of x * 65536 as an unsigned integer; NaN and negatives give 0, 65536 frames and more saturate (the
// rule of __float2uint_rn, which the device uses).  x * 65536 is exact in fp32: a power of two.
DUR_HD inline uint32_t durations_q16(float x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __float2uint_rn(x * 65536.0f);
#else
  const float s = x * 65536.0f;
  if (!(s > 0.0f)) return 0u;
  if (s >= 4294967296.0f) return 0xFFFFFFFFu;
  const double d = (double)s;
  uint64_t f = (uint64_t)d;  // floor: d > 0
  const double r = d - (double)f;
  if (r > 0.5 || (r == 0.5 && (f & 1u))) ++f;  // (from 2^24 on s is an integer: f stays below 2^32)
  return (uint32_t)f;
#endif
}

// "" if the fields are a setting, else the message: it names the field
inline std::string durations_check(const DurationsOpts &o) {
  char msg[160];
  if (o.on != 0 && o.on != 1) {
    std::snprintf(msg, sizeof msg, "durations on %d is not 0 or 1", (int)o.on);
    return msg;
  }
  if (!std::isfinite(o.min_frames) || o.min_frames < 0.0f || o.min_frames > 65535.0f) {
    std::snprintf(msg, sizeof msg, "durations min_frames %g is not in [0, 65535]", (double)o.min_frames);
    return msg;
  }
  if (!std::isfinite(o.max_frames) || o.max_frames < o.min_frames || o.max_frames > 65535.0f) {
    std::snprintf(msg, sizeof msg, "durations max_frames %g is not in [min_frames, 65535]", (double)o.max_frames);
    return msg;
  }
  return "";
}

// One chunk slot of the kernel's table / one utterance.  list[] holds, utterance by utterance, the slots of the utterance's
// chunks in the caller's order: the earlier chunks of the chunk at position k are list[list0 .. list0 + k).
struct DurChunk {
  int32_t caller;   // order[j]
  int32_t utt;
  int32_t out_off;  // index of the chunk's first id in the output
  int32_t n;        // its ids (the host's count: the device never writes past it)
  int32_t list0, k;
};
struct DurUtt {
  int32_t id_off, n_ids;
  int32_t list0, n_chunks;
};
struct DurPlan {
  std::vector<DurChunk> chunk;  // [B], by slot
  std::vector<DurUtt> utt;
  std::vector<int32_t> list;    // [B]
  size_t n_ids = 0;
};

// The argument rules of the stage on caller arrays, and the plan.  order == nullptr: slot j is chunk j.  utt_of_chunk ==
// nullptr: every chunk is an utterance of its own; else utt_of_chunk[c] (c: the caller's chunk index) starts at 0 and goes up
// by 0 or 1.  nframes == nullptr is allowed where only the layout is wanted (the request path: the counts are on the device).
inline std::string durations_plan(int B, int T, const int *nframes, const int *n_valid, const int *order, int batched, bool have_cum_b,
                                  const int *utt_of_chunk, DurPlan *plan) {
  char msg[200];
  if (B < 1 || B > DUR_B_MAX) {
    std::snprintf(msg, sizeof msg, "durations: batch %d is not in [1, %d]", B, DUR_B_MAX);
    return msg;
  }
  if (T < 1 || T > DUR_T_MAX) {
    std::snprintf(msg, sizeof msg, "durations: window %d is not in [1, %d]", T, DUR_T_MAX);
    return msg;
  }
  if (batched != 0 && batched != 1) {
    std::snprintf(msg, sizeof msg, "durations: batched %d is not 0 or 1", batched);
    return msg;
  }
  if (batched && !have_cum_b) return "durations: batched mode needs the second cumulative buffer (cum_b)";
  if (!n_valid) return "durations: n_valid is null";
  std::vector<int> slot_of(B, -1);
  for (int j = 0; j < B; ++j) {
    const int c = order ? order[j] : j;
    if (c < 0 || c >= B || slot_of[c] >= 0) {
      std::snprintf(msg, sizeof msg, "durations: order is not a permutation of 0..%d (slot %d)", B - 1, j);
      return msg;
    }
    slot_of[c] = j;
    if (n_valid[j] < 1 || n_valid[j] > T) {
      std::snprintf(msg, sizeof msg, "durations: slot %d: n_valid %d is not in [1, %d]", j, n_valid[j], T);
      return msg;
    }
    if (nframes && (nframes[j] < 0 || nframes[j] > DUR_FRAMES_MAX)) {
      std::snprintf(msg, sizeof msg, "durations: slot %d: nframes %d is not in [0, %d]", j, nframes[j], DUR_FRAMES_MAX);
      return msg;
    }
  }
  if (utt_of_chunk)
    for (int c = 0; c < B; ++c) {
      const int prev = c ? utt_of_chunk[c - 1] : 0;
      if (utt_of_chunk[c] < prev || utt_of_chunk[c] > prev + (c ? 1 : 0)) {
        std::snprintf(msg, sizeof msg, "durations: utt_of_chunk[%d] = %d: utterances start at 0 and go up by 0 or 1", c, utt_of_chunk[c]);
        return msg;
      }
    }
  if (!plan) return "";
  DurPlan p;
  p.chunk.resize(B);
  p.list.resize(B);
  int off = 0;
  for (int c = 0; c < B; ++c) {
    const int u = utt_of_chunk ? utt_of_chunk[c] : c, j = slot_of[c];
    if (u == (int)p.utt.size()) p.utt.push_back(DurUtt{off, 0, c, 0});
    DurUtt &U = p.utt[u];
    p.list[c] = j;  // (the utterances' chunks are consecutive in the caller's order: list index == c)
    p.chunk[j] = DurChunk{c, u, off, n_valid[j], U.list0, U.n_chunks};
    U.n_ids += n_valid[j];
    U.n_chunks += 1;
    off += n_valid[j];
  }
  p.n_ids = (size_t)off;
  *plan = std::move(p);
  return "";
}

// The stage, serially: dur / dur_q16 / start_q16 hold plan.n_ids entries, stats plan.utt.size(); any of them may be null.
inline void durations_reference(const DurPlan &p, const float *cum_a, const float *cum_b, int T, const int *nframes, int batched,
                                const DurationsOpts &o, float *dur, uint32_t *dur_q16, uint64_t *start_q16, AlignmentStats *stats) {
  const uint32_t lo = durations_q16(o.min_frames), hi = durations_q16(o.max_frames);
  for (size_t u = 0; u < p.utt.size(); ++u) {
    const DurUtt &U = p.utt[u];
    AlignmentStats s{};
    s.n_ids = (uint32_t)U.n_ids;
    s.min_q16 = 0xFFFFFFFFu;
    uint64_t base = 0;  // frames of the earlier chunks
    uint32_t i = 0;     // index in the utterance
    for (int k = 0; k < U.n_chunks; ++k) {
      const int j = p.list[U.list0 + k];
      const DurChunk &c = p.chunk[j];
      const float *row = (batched && (nframes[j] & 1) ? cum_b : cum_a) + (size_t)j * T;
      uint64_t run = 0;
      for (int t = 0; t < c.n; ++t, ++i) {
        const uint32_t q = durations_q16(row[t]);
        const size_t at = (size_t)c.out_off + t;
        if (dur) dur[at] = row[t];
        if (dur_q16) dur_q16[at] = q;
        if (start_q16) start_q16[at] = base * 65536u + run;
        run += q;
        s.sum_q16 += q;
        if (q < s.min_q16 || i == 0) s.min_q16 = q, s.min_index = i;
        if (q > s.max_q16 || i == 0) s.max_q16 = q, s.max_index = i;
        s.n_below += q < lo;
        s.n_above += q > hi;
        s.last_q16 = q;
      }
      base += (uint64_t)nframes[j];
    }
    s.n_frames = base;
    if (stats) stats[u] = s;
  }
}

// A position x in ids, 0 <= x <= n, of an utterance of F frames -> the frame position start[k] + (x - k) dur[k], k = floor(x)
// (x == n: the end of the last id), as a fraction of F - 1 clamped to [0, 1]: a contour point's pos.  Double throughout.  NaN
// for arguments outside the rule (the callers name the point).
inline double durations_position(const uint64_t *start_q16, const uint32_t *dur_q16, size_t n, size_t F, double x) {
  if (!start_q16 || !dur_q16 || n == 0 || F == 0 || !(x >= 0.0) || !(x <= (double)n)) return std::nan("");
  size_t k = (size_t)std::floor(x);
  if (k >= n) k = n - 1;  // x == n: frac = 1
  const double frame = ((double)start_q16[k] + (x - (double)k) * (double)dur_q16[k]) / 65536.0;
  if (F == 1) return 0.0;
  const double pos = frame / (double)(F - 1);
  return pos < 0.0 ? 0.0 : (pos > 1.0 ? 1.0 : pos);
}

// The delivered sample offset of a Q16 frame position on the PLAIN path: frame f starts at sample f * hop of the vocoder's
// loop, and the resampler delivers sample floor(s L / M) for input position s (resample_plan.h; the identity has L = M = 1).
// NOT valid behind a rate or contour change (the frames move) or the silence stage (samples are dropped).  -1: the rate is not
// one the resampler takes.
inline int64_t durations_samples(uint64_t start_q16, int hop, long long rate_out) {
  ResamplePlan rp;
  if (hop < 1 || !resample_check(rate_out, &rp).empty()) return -1;
  // floor(start hop L / (65536 M)), exact: 128-bit integers
  const unsigned __int128 num = (unsigned __int128)start_q16 * (unsigned)hop * (unsigned)rp.L;
  return (int64_t)(num / ((unsigned __int128)65536u * (unsigned)rp.M));
}

}  // namespace xdtts
