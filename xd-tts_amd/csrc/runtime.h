// runtime.h -- what both handles and every extern "C" entry point share: the error boundary, device selection, the pool of
// pinned host buffers handed to the caller, timing events, the per-GPU lock of the co-resident grids, and the small helpers
// (drain guard, error-word fetch, cached hipGraph) that used to be written out at each place of use.
#pragma once
#include <sys/types.h>

#include <mutex>
#include <new>
#include <vector>

#include "common.h"

namespace xdtts {

const char *last_error();

template <class F>
xdtts_status guard(F &&f) {
  try {
    f();
    return XDTTS_OK;
  } catch (const Error &e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::bad_alloc &) {
    set_last_error("host allocation failed");
    return XDTTS_ERR_OOM;
  } catch (const std::exception &e) {
    set_last_error(e.what());
    return XDTTS_ERR_HIP;
  } catch (const CoopRefused &) {  // (not a std::exception; the engines catch it where they can fall back)
    set_last_error("cooperative launch refused by the runtime: the grid does not fit this device");
    return XDTTS_ERR_HIP;
  } catch (...) {  // nothing unwinds through the C ABI
    set_last_error("unexpected exception");
    return XDTTS_ERR_HIP;
  }
}

int default_device();              // XDTTS_DEVICE, 0 without it
int select_device(int device_id);  // returns the device actually selected

// Pinned host buffers handed to the caller (runtime.cpp: PinnedPool).
float *pinned_alloc(size_t n_floats);
void pinned_release(void *p);  // xdtts_free: a buffer, or a piece of a slab
void pinned_add_pieces(void *slab, const std::vector<float *> &cut);

// Owns a pinned output buffer until the call has succeeded: an exception on the way (a failed
// copy, a later stage that throws) returns it to the pool instead of leaving it live forever.
struct PinnedGuard {
  float *p = nullptr;
  PinnedGuard() = default;
  explicit PinnedGuard(size_t n_floats) : p(pinned_alloc(n_floats)) {}
  PinnedGuard(PinnedGuard &&o) noexcept : p(o.p) { o.p = nullptr; }
  PinnedGuard(const PinnedGuard &) = delete;
  PinnedGuard &operator=(const PinnedGuard &) = delete;
  PinnedGuard &operator=(PinnedGuard &&o) noexcept {
    if (this != &o) {
      if (p) pinned_release(p);
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~PinnedGuard() {
    if (p) pinned_release(p);
  }
  float *release() {
    float *r = p;
    p = nullptr;
    return r;
  }
};

// A pinned slab whose pieces go to the caller one by one (PinnedPool::add_pieces).  Until hand_over() the slab is the
// guard's: an exception on the way returns it whole.
struct PinnedSlab {
  float *base = nullptr;
  std::vector<float *> cut;
  explicit PinnedSlab(size_t n_floats) : base(pinned_alloc(n_floats)) {}
  PinnedSlab(const PinnedSlab &) = delete;
  PinnedSlab &operator=(const PinnedSlab &) = delete;
  ~PinnedSlab() {
    if (base) pinned_release(base);
  }
  float *piece(size_t offset_floats) {  // (distinct offsets: a piece is identified by its address)
    cut.push_back(base + offset_floats);
    return cut.back();
  }
  void hand_over() {  // from here on every piece is the caller's; the slab follows the last one
    if (cut.empty()) return;
    pinned_add_pieces(base, cut);
    base = nullptr;
  }
};

struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  void create() {
    for (auto &x : e) HIP_CHECK(hipEventCreate(&x));
  }
  ~Events() {
    for (auto &x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// Declared behind the pinned buffers a copy is in flight into, i.e. destroyed before them: whatever throws, the streams
// drain first and only then do the buffers go back to the shared pool.  (By reference: a stream created later counts.)
struct Drain {
  hipStream_t &a;
  hipStream_t &b;
  explicit Drain(hipStream_t &s) : a(s), b(s) {}
  Drain(hipStream_t &s, hipStream_t &t) : a(s), b(t) {}
  ~Drain() {
    if (a) (void)hipStreamSynchronize(a);
    if (b && &b != &a) (void)hipStreamSynchronize(b);
  }
};

// The cooperative encoder BiLSTM and the persistent decoder need their whole grid co-resident, so
// two of them from different handles must never be in flight together (each could hold CUs the
// other waits for).  Every call that launches one holds this lock from enqueue to completion.
// Between PROCESSES that share a GPU the same rule holds; XDTTS_CHIP_LOCK_DIR=<dir> (read once) adds an flock on
// <dir>/xdtts_chip_<pci bus id>.lock to the lock, so that co-resident launches of different processes take turns instead of
// timing out into the fallback engines (bench.py's two-ranks-on-one-GPU test mode uses it; so can a multi-worker server).
class ChipLock {
  std::recursive_mutex m;
  int depth = 0, fd = -2;  // fd -2: not looked at yet (in this process), -1: no file lock
  const int device;
  pid_t owner = 0;         // the process that opened fd: a forked child inherits the open file DESCRIPTION, on which parent and
                           // child would both "hold" the flock -- it opens its own
  void open_file();

 public:
  explicit ChipLock(int d) : device(d) {}
  void lock();
  void unlock();
};
ChipLock &chip_mutex(int device);

// An engine's error word (set by a workgroup whose bounded spin ran out): fetched behind everything enqueued on `s`, and
// cleared when set.  Returns whether it was set.
bool fetch_and_clear_error_word(int *dev_word, hipStream_t s);

// One cached hipGraph: replay() captures what `enqueue` puts on the stream unless the cached graph was captured for the
// same key bytes, then launches it.
struct GraphCache {
  hipGraphExec_t exec = nullptr;
  std::vector<unsigned char> key;
  GraphCache() = default;
  GraphCache(const GraphCache &) = delete;
  GraphCache &operator=(const GraphCache &) = delete;
  ~GraphCache() {
    if (exec) (void)hipGraphExecDestroy(exec);
  }
  template <class F>
  void replay(const void *key_bytes, size_t n, hipStream_t s, F &&enqueue) {
    if (!exec || key.size() != n || std::memcmp(key.data(), key_bytes, n) != 0) {
      if (exec) {
        (void)hipGraphExecDestroy(exec);
        exec = nullptr;
      }
      hipGraph_t g = nullptr;
      HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      try {
        enqueue();
      } catch (...) {
        (void)hipStreamEndCapture(s, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
      }
      HIP_CHECK(hipStreamEndCapture(s, &g));
      hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIP_CHECK(e);
      key.assign((const unsigned char *)key_bytes, (const unsigned char *)key_bytes + n);
    }
    HIP_CHECK(hipGraphLaunch(exec, s));
  }
};

}  // namespace xdtts
