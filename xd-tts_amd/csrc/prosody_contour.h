// prosody_contour.h -- the host arithmetic of a prosody contour (xdtts_prosody_contour, include/xdtts.h): the argument rules, the
// value of a field at a position, the frame table {c, pitch, gain} and F'.  The device (prosody.hip: k_prosody_contour) reads
// nothing but this table, and every caller -- the two host entries, the parity hooks, the request paths -- builds it here.
// Plain host C++, no HIP and none of the library's headers: tests/contour_table_test.cpp drives it with plain g++.
// The arithmetic is double, in the order of operations the definition writes down, and is kept from being contracted into
// fused multiply-adds: tests/test_contour_cpu.py compares the table with a numpy restatement bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#if defined(__clang__)
#define XDTTS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define XDTTS_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace xdtts {

struct ContourPoint {  // the layout of xdtts_prosody_point
  float pos, rate, pitch, gain;
};
constexpr int CONTOUR_MAX_POINTS = 64;
constexpr size_t CONTOUR_MAX_FRAMES = 16384;          // keeps C = c[F - 1] below 2^32 at rate 0.25
constexpr size_t CONTOUR_MAX_IDENTITY_FRAMES = (size_t)1 << 20;  // what the uniform prosody takes (prosody_check)

inline bool contour_is_identity(const ContourPoint *pts, int n) {
  for (int k = 0; k < n; ++k)
    if (pts[k].rate != 1.0f || pts[k].pitch != 1.0f || pts[k].gain != 1.0f) return false;
  return true;
}

// The argument rules.  "" if the contour may run on n_frames frames, else the message: it names the field and the point.
inline std::string contour_check(const ContourPoint *pts, int n, int lifter, float log_floor, size_t n_frames) {
  char msg[160];
  auto say = [&](const char *field, int k, double v, const char *rule) {
    std::snprintf(msg, sizeof msg, "contour point %d: %s %g %s", k, field, v, rule);
    return std::string(msg);
  };
  if (n < 1 || n > CONTOUR_MAX_POINTS) {
    std::snprintf(msg, sizeof msg, "contour n_points %d is not in [1, %d]", n, CONTOUR_MAX_POINTS);
    return msg;
  }
  if (!pts) return "null contour points";
  for (int k = 0; k < n; ++k) {
    const ContourPoint &p = pts[k];
    if (!std::isfinite(p.pos) || p.pos < 0.0f || p.pos > 1.0f) return say("pos", k, p.pos, "is not in [0, 1]");
    if (k > 0 && p.pos < pts[k - 1].pos) return say("pos", k, p.pos, "is below the point before it");
    if (!std::isfinite(p.rate) || p.rate < 0.25f || p.rate > 4.0f) return say("rate", k, p.rate, "is not in [0.25, 4]");
    if (!std::isfinite(p.pitch) || p.pitch < 0.5f || p.pitch > 2.0f) return say("pitch", k, p.pitch, "is not in [0.5, 2]");
    if (!std::isfinite(p.gain) || p.gain < 0.0f || p.gain > 8.0f) return say("gain", k, p.gain, "is not in [0, 8]");
  }
  if (lifter < 1 || lifter > 255) {
    std::snprintf(msg, sizeof msg, "contour lifter %d is not in [1, 255]", lifter);
    return msg;
  }
  if (!std::isfinite(log_floor) || !(log_floor > 0.0f)) {
    std::snprintf(msg, sizeof msg, "contour log_floor %g is not a positive number", (double)log_floor);
    return msg;
  }
  if (contour_is_identity(pts, n)) {
    if (n_frames > CONTOUR_MAX_IDENTITY_FRAMES) {
      std::snprintf(msg, sizeof msg, "contour n_frames: at most 2^20 frames, got %zu", n_frames);
      return msg;
    }
  } else if (n_frames < 2 || n_frames > CONTOUR_MAX_FRAMES) {
    std::snprintf(msg, sizeof msg, "contour n_frames: a contour that is not the identity takes 2 .. %zu frames, got %zu", CONTOUR_MAX_FRAMES, n_frames);
    return msg;
  }
  return "";
}

enum ContourField { CONTOUR_RATE = 1, CONTOUR_PITCH = 2, CONTOUR_GAIN = 3 };

// The value of a field at position x: constant before the first point and behind the last, linear in between, and
// right-continuous at a step (two points at one pos).
inline double contour_value(const ContourPoint *pts, int n, ContourField f, double x) {
  XDTTS_NO_CONTRACT
  auto v = [&](int k) { return (double)(f == CONTOUR_RATE ? pts[k].rate : (f == CONTOUR_PITCH ? pts[k].pitch : pts[k].gain)); };
  int k = 0;  // the number of points with pos <= x
  while (k < n && (double)pts[k].pos <= x) ++k;
  if (k == 0) return v(0);
  if (k == n) return v(n - 1);
  const int a = k - 1, b = k;  // pos[a] <= x < pos[b]
  const double frac = (x - (double)pts[a].pos) / ((double)pts[b].pos - (double)pts[a].pos);
  const double rise = (v(b) - v(a)) * frac;
  return v(a) + rise;
}

// The frame table of one utterance, one entry per INPUT frame m < F:
//   c[0] = 0, c[m + 1] = c[m] + q[m], q[m] = floor(65536 / rate((m + 0.5) / (F - 1)) + 0.5): the slowness of interval m in
//   2^-16 output frames (16384 .. 262144);  pitch[m], gain[m] = the fields at m / (F - 1), rounded to float.
//   Fout = max((c[F - 1] + 32768) >> 16, 1) + 1.
// The identity needs no table: Fout = F and the vectors stay empty.
struct ContourTable {
  bool identity = true;
  int F = 0, Fout = 0;
  int lifter = 30;
  float log_floor = 1e-5f;
  std::vector<uint32_t> c;
  std::vector<float> pitch, gain;
};

inline size_t contour_frames_of(uint64_t C) {
  const uint64_t n = (C + 32768u) >> 16;
  return (size_t)(n > 1 ? n : 1) + 1;
}

// (the arguments have passed contour_check; cum / pitch / gain: F entries each, any may be null)
inline size_t contour_fill(const ContourPoint *pts, int n, size_t F, uint32_t *cum, float *pitch, float *gain) {
  XDTTS_NO_CONTRACT
  if (F < 2) {  // one frame (the identity alone comes here)
    if (F == 1) {
      if (cum) cum[0] = 0;
      if (pitch) pitch[0] = (float)contour_value(pts, n, CONTOUR_PITCH, 0.0);
      if (gain) gain[0] = (float)contour_value(pts, n, CONTOUR_GAIN, 0.0);
    }
    return F;
  }
  const double span = (double)(F - 1);
  uint64_t c = 0;
  for (size_t m = 0; m < F; ++m) {
    if (cum) cum[m] = (uint32_t)c;
    const double x = (double)m / span;
    if (pitch) pitch[m] = (float)contour_value(pts, n, CONTOUR_PITCH, x);
    if (gain) gain[m] = (float)contour_value(pts, n, CONTOUR_GAIN, x);
    if (m + 1 < F) {
      const double xr = ((double)m + 0.5) / span;
      const double slow = 65536.0 / contour_value(pts, n, CONTOUR_RATE, xr);
      c += (uint64_t)std::floor(slow + 0.5);
    }
  }
  return contour_frames_of(c);
}

// Frames behind the stage, 0 for a bad argument.
inline size_t contour_frames(const ContourPoint *pts, int n, int lifter, float log_floor, size_t F) {
  if (!contour_check(pts, n, lifter, log_floor, F).empty()) return 0;
  if (contour_is_identity(pts, n)) return F;
  return contour_fill(pts, n, F, nullptr, nullptr, nullptr);
}

// The table a request runs on (arguments checked by the caller).
inline void contour_build(const ContourPoint *pts, int n, int lifter, float log_floor, size_t F, ContourTable &t) {
  t = ContourTable();
  t.F = (int)F;
  t.lifter = lifter;
  t.log_floor = log_floor;
  t.identity = contour_is_identity(pts, n);
  if (t.identity) {
    t.Fout = (int)F;
    return;
  }
  t.c.resize(F);
  t.pitch.resize(F);
  t.gain.resize(F);
  t.Fout = (int)contour_fill(pts, n, F, t.c.data(), t.pitch.data(), t.gain.data());
}

}  // namespace xdtts

#if !defined(__clang__)
#pragma GCC pop_options
#endif
