// gl_plan.h -- the integer arithmetic that feeds the persistent Griffin-Lim kernel (griffinlim.hip: k_gl_persistent): how one
// utterance is split over workgroups, where the utterances of a ragged batch lie, and which of them share a launch.  Its
// results are the rows and offsets that co-resident workgroups poll on.  Plain host C++, no HIP: tests/gl_plan_test.cpp drives
// it on a machine without a GPU, at CU counts and workgroup shapes the GPU tests never see.
#pragma once
#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <utility>
#include <vector>

namespace xdtts {

constexpr int GLP_TF_MAX = 8;  // frames per workgroup (LDS: 10.3 KB of state + 4 KB of frame each; 8 waves = 2 per SIMD)
// One workgroup's share when a launch covers SEVERAL utterances (vocoder batch): the utterances' frames
// are concatenated in S / angles / previous spectrum, workgroups never span two utterances and exchange
// overlaps only inside their own.
struct GlSeg {
  int fbase;   // row of the utterance's first frame in the concatenated arrays
  int F;       // frames of the utterance
  int f0;      // first own frame, within the utterance
  int n_own;   // own frames (3..TF)
  int first;   // no left neighbour
  int last;    // no right neighbour
  int abase;   // offset of the utterance's samples in the audio output
  int pad;
};

// One utterance in a launch of its own: TF frames per workgroup, nblk workgroups; false = the launch-per-iteration engine.
inline bool gl_persistent_plan(int F, int n_cu, int *TF, int *nblk) {
  if (F < 16) return false;  // reflect padding folds more than once: two-kernel path
  int tf = std::max(4, (F + n_cu - 1) / n_cu);
  if (tf > GLP_TF_MAX) return false;
  const int nb = (F + tf - 1) / tf;
  if (nb > n_cu || F / nb < 3) return false;  // one workgroup per CU; every block needs >= 3 frames
  *TF = tf;
  *nblk = nb;
  return true;
}
// ... and the even split of its frames: workgroup b owns [gl_fstart(b), gl_fstart(b + 1)) (the kernel's glp_fstart)
inline int gl_fstart(int b, int F, int nblk) { return (int)(((long long)b * F) / nblk); }

// Utterances back to back: utterance u is the rows row0[u] .. row0[u] + F[u] of `total`.
struct Rows {
  std::vector<int> row0, F;
  size_t total = 0;
  int n() const { return (int)F.size(); }
  // the next utterance; throws std::length_error(too_large) when the total passes cap (<= 2^24: the rows are ints)
  void add(size_t rows, size_t cap, const char *too_large) {
    if (rows > cap || total + rows > cap) throw std::length_error(too_large);
    row0.push_back((int)total);
    F.push_back((int)rows);
    total += rows;
  }
};

// The persistent launches of a vocoder batch.  A workgroup owns up to 4 frames (one wave each) or up to 8 (two waves per
// SIMD): an iteration of the 8-frame shape takes 6.8 us against 5.35 us (tools/gl_tf_sweep.py), so it wins as soon as it saves
// launches.  Two 4-frame workgroups per CU (k_gl_persistent<4, 2>: the state in LDS, 256 registers) take 7.1 us for the same
// eight frames (tools/vocoder_batch.py) and keep the 4-frame split, i.e. the single call's audio bit for bit.
struct GlBatchPlan {
  int TF = 4, WG = 1;       // frames per workgroup, workgroups per CU
  std::vector<GlSeg> segs;  // the workgroups of all launches
  struct Launch {
    int seg0, nblk;         // its rows of segs
    std::vector<int> utts;  // its utterances, in the order their workgroups ride
  };
  std::vector<Launch> launches;
  std::vector<char> batched;  // [n_utt] 1: rides in a launch; 0: runs alone, on the engine its own call would use
  std::vector<int> order;     // every utterance once, as the audio is normalised and fetched: launch by launch, then the alone ones
};

// One shape's packing: first-fit decreasing over launches of n_cu * wg workgroups (which launch an utterance rides in does not
// change its audio: its own split into workgroups depends on its frame count alone).  Returns the relative cost, launches x
// time per iteration of the shape; riders (if wanted) receives each launch's utterances.
inline double gl_batch_pack(const std::vector<int> &Fu, int n_cu, int tf, int wg, std::vector<std::vector<int>> *riders = nullptr) {
  std::vector<std::pair<int, int>> items;  // (workgroups, utterance)
  int n_alone = 0;
  for (int u = 0; u < (int)Fu.size(); ++u) {
    const int nb = (Fu[u] + tf - 1) / tf;
    if (Fu[u] < 16 || nb > n_cu || Fu[u] / nb < 3) {  // on its own
      n_alone += Fu[u] >= 16;  // (a launch of the 5..8-frame shape; the tiny ones cost next to nothing)
      continue;
    }
    items.emplace_back(nb, u);
  }
  std::stable_sort(items.begin(), items.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first > b.first; });
  std::vector<int> room;  // free workgroups of each launch
  std::vector<std::vector<int>> local;
  std::vector<std::vector<int>> &rd = riders ? *riders : local;
  rd.clear();
  for (const auto &it : items) {
    size_t k = 0;
    while (k < room.size() && room[k] < it.first) ++k;
    if (k == room.size()) {
      room.push_back(n_cu * wg);
      rd.emplace_back();
    }
    room[k] -= it.first;
    rd[k].push_back(it.second);
  }
  // us per iteration of one launch of each shape (tools/vocoder_shapes.py, round 4 with the 16-byte exchange granules:
  // 4.5-5.2 / 5.8-6.3 / 5.9-6.3; round 3: 5.35 / 7.1 / 6.8) -- at equal cost the 4-frame shape, whose audio is the single call's
  return (tf <= 4 ? (wg > 1 ? 6.0 : 4.85) : 6.1) * (double)rd.size() + 6.1 * n_alone;
}

// Fu: frames per utterance; per_cu4: co-resident 4-frame workgroups per CU; batch_shape: the option (0 = cheapest shape,
// 4 = the 4-frame shape, which splits an utterance the way its own call does); force: the developer switch, 8 = 8-frame
// workgroups, 41 / 42 = 4-frame, one / two per CU, anything else = none.  n_cu = 0 (no usable persistent engine): the empty
// plan, every utterance alone.
inline GlBatchPlan gl_batch_plan(const std::vector<int> &Fu, int hop, int n_cu, int per_cu4, int batch_shape, int force) {
  const int n_utt = (int)Fu.size();
  GlBatchPlan P;
  P.batched.assign((size_t)n_utt, 0);
  if (n_cu > 0) {
    if (per_cu4 >= 2 && gl_batch_pack(Fu, n_cu, 4, 2) < gl_batch_pack(Fu, n_cu, 4, 1)) P.WG = 2;
    if (batch_shape == 0 && gl_batch_pack(Fu, n_cu, GLP_TF_MAX, 1) < gl_batch_pack(Fu, n_cu, 4, P.WG)) P.TF = GLP_TF_MAX, P.WG = 1;
    if (force == 8) P.TF = GLP_TF_MAX, P.WG = 1;
    if (force == 41) P.TF = 4, P.WG = 1;
    if (force == 42 && per_cu4 >= 2) P.TF = 4, P.WG = 2;
    std::vector<int> fbase((size_t)n_utt), abase((size_t)n_utt);
    for (int u = 0, f = 0, a = 0; u < n_utt; f += Fu[u], a += hop * (Fu[u] - 1), ++u) fbase[(size_t)u] = f, abase[(size_t)u] = a;
    std::vector<std::vector<int>> riders;
    gl_batch_pack(Fu, n_cu, P.TF, P.WG, &riders);
    for (std::vector<int> &utts : riders) {
      const int seg0 = (int)P.segs.size();
      for (int u : utts) {
        const int nb = (Fu[u] + P.TF - 1) / P.TF;
        for (int b = 0; b < nb; ++b) {
          GlSeg sg{};
          sg.fbase = fbase[(size_t)u];
          sg.F = Fu[u];
          sg.f0 = gl_fstart(b, Fu[u], nb);
          sg.n_own = gl_fstart(b + 1, Fu[u], nb) - sg.f0;
          sg.first = b == 0;
          sg.last = b + 1 == nb;
          sg.abase = abase[(size_t)u];
          P.segs.push_back(sg);
        }
        P.batched[(size_t)u] = 1;
        P.order.push_back(u);
      }
      P.launches.push_back({seg0, (int)P.segs.size() - seg0, std::move(utts)});
    }
  }
  for (int u = 0; u < n_utt; ++u)
    if (!P.batched[(size_t)u]) P.order.push_back(u);
  return P;
}

}  // namespace xdtts
