// runtime.cpp -- error plumbing, device selection, the pinned-buffer pool and the per-GPU lock (runtime.h).
#include "runtime.h"

#include <algorithm>
#include <map>
#include <memory>

#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#include <cerrno>

namespace xdtts {

static thread_local std::string g_last_error;
void set_last_error(const char *msg) { g_last_error = msg ? msg : ""; }
void fail(xdtts_status code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  throw Error(code, buf);
}
const char *last_error() { return g_last_error.c_str(); }

// XDTTS_DEVICE_DEFAULT (-1) as a device_id = "the process's default GPU": the value of the environment variable XDTTS_DEVICE (read at
// every handle creation), 0 without it.  It is how a host that keeps the reference's constructor signatures -- Tacotron2::load(path),
// GriffinLim::new(..) take no device (src/lib.rs:40-58) -- is spread over the 8 GPUs of a node: one process per GPU, XDTTS_DEVICE = its
// rank; the shim's load_on / new_on pass an explicit id instead.
int default_device() {
  const char *e = env::raw(env::DEVICE);
  if (!e || !*e) return 0;
  char *end = nullptr;
  const long v = std::strtol(e, &end, 10);
  if (end == e || *end != 0 || v < 0 || v > 1023) fail(XDTTS_ERR_BAD_ARG, "XDTTS_DEVICE=\"%s\" is not a device index", e);
  return (int)v;
}
int select_device(int device_id) {  // returns the device actually selected
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    fail(XDTTS_ERR_NO_DEVICE, "no HIP device visible: libxdtts_hip has no CPU fallback");
  if (device_id == XDTTS_DEVICE_DEFAULT) device_id = default_device();
  if (device_id < 0 || device_id >= n) fail(XDTTS_ERR_BAD_ARG, "device_id %d out of range (0..%d)", device_id, n - 1);
  HIP_CHECK(hipSetDevice(device_id));
  return device_id;
}

// Pinned host buffers handed to the caller.  hipHostMalloc/hipHostFree cost hundreds of
// microseconds (page pinning), comparable to a whole vocoder run, so released buffers are kept in
// a small size-classed pool and reused by later calls.
namespace {
struct PinnedPool {
  std::mutex mu;
  std::map<void *, size_t> live;                     // buffer -> capacity (bytes)
  std::multimap<size_t, void *> spare;               // capacity -> buffer
  size_t spare_bytes = 0;
  static constexpr size_t MAX_SPARE = 256u << 20;
  static size_t size_class(size_t bytes) {
    size_t c = 4096;
    while (c < bytes) c <<= 1;
    return c;
  }
  float *get(size_t bytes) {
    const size_t cap = size_class(bytes);
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = spare.find(cap);
      if (it != spare.end()) {
        void *p = it->second;
        spare.erase(it);
        spare_bytes -= cap;
        live[p] = cap;
        return (float *)p;
      }
    }
    void *p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, cap, hipHostMallocDefault));
    std::lock_guard<std::mutex> lk(mu);
    live[p] = cap;
    return (float *)p;
  }
  // A slab handed out in pieces (the mels of a batch: one copy from the device, no repacking on the host): every piece
  // is released on its own (xdtts_free), the slab goes back to the pool with the last one.
  std::map<void *, void *> part_of;  // piece -> slab
  std::map<void *, int> pieces;      // slab -> pieces outstanding
  void add_pieces(void *slab, const std::vector<float *> &cut) {  // all or nothing, under one lock
    std::lock_guard<std::mutex> lk(mu);
    size_t done = 0;
    try {
      for (; done < cut.size(); ++done) part_of[cut[done]] = slab;
      pieces[slab] = (int)cut.size();
    } catch (...) {
      for (size_t i = 0; i < done; ++i) part_of.erase(cut[i]);
      throw;
    }
  }
  void put(void *p) {
    std::unique_lock<std::mutex> lk(mu);
    auto pt = part_of.find(p);
    if (pt != part_of.end()) {
      void *slab = pt->second;
      part_of.erase(pt);
      if (--pieces[slab] > 0) return;
      pieces.erase(slab);
      p = slab;
    }
    if (pieces.count(p)) return;  // a second xdtts_free of a slab's first piece while others are still out: not the slab's turn
    auto it = live.find(p);
    if (it == live.end()) return;  // not ours, or already released (a double xdtts_free): nothing to do --
                                   // freeing it here could hand a buffer in `spare` back to the runtime
    const size_t cap = it->second;
    live.erase(it);
    if (spare_bytes + cap <= MAX_SPARE) {
      spare.emplace(cap, p);
      spare_bytes += cap;
      return;
    }
    lk.unlock();
    (void)hipHostFree(p);
  }
};
PinnedPool &pinned_pool() {
  static PinnedPool *pool = new PinnedPool();  // intentionally leaked: outlives static destruction order
  return *pool;
}
}  // namespace

float *pinned_alloc(size_t n_floats) { return pinned_pool().get(std::max<size_t>(n_floats, 1) * sizeof(float)); }
void pinned_release(void *p) { pinned_pool().put(p); }
void pinned_add_pieces(void *slab, const std::vector<float *> &cut) { pinned_pool().add_pieces(slab, cut); }

void ChipLock::open_file() {
  if (fd >= 0 && owner != getpid()) ::close(fd);   // (the inherited descriptor; the parent's stays open in the parent)
  fd = -1;
  owner = getpid();
  const char *dir = env::raw(env::CHIP_LOCK_DIR);
  if (!dir || !*dir) return;
  char bus[64] = "unknown";
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) std::snprintf(bus, sizeof bus, "dev%d", device);
  for (char *c = bus; *c; ++c)
    if (*c == ':' || *c == '/') *c = '_';
  const std::string path = std::string(dir) + "/xdtts_chip_" + bus + ".lock";
  fd = ::open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC, 0666);
  if (fd >= 0) (void)::fchmod(fd, 0666);  // (the creator's umask must not lock a second user out; fails harmlessly for a non-owner)
  if (fd < 0) fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);  // another user's 0644 file, or fs.protected_regular in a sticky directory: flock needs no write access
  if (fd < 0) {
    // the caller asked for cross-process serialisation and cannot have it: an error, not a warning (without the lock two
    // processes time each other's co-resident launches out into the fallback engines)
    fd = -2;
    fail(XDTTS_ERR_IO, "XDTTS_CHIP_LOCK_DIR: cannot open %s (%s)", path.c_str(), std::strerror(errno));
  }
}
void ChipLock::lock() {
  m.lock();
  if (depth == 0) {
    try {
      if (fd == -2 || owner != getpid()) open_file();
    } catch (...) {
      m.unlock();
      throw;
    }
    if (fd >= 0)
      while (::flock(fd, LOCK_EX) != 0 && errno == EINTR) {
      }
  }
  ++depth;
}
void ChipLock::unlock() {
  if (--depth == 0 && fd >= 0) (void)::flock(fd, LOCK_UN);
  m.unlock();
}
ChipLock &chip_mutex(int device) {
  static std::mutex g;
  static std::map<int, std::unique_ptr<ChipLock>> locks;  // one per GPU of this process, keyed by the device id itself
  std::lock_guard<std::mutex> l(g);
  std::unique_ptr<ChipLock> &p = locks[device];
  if (!p) p.reset(new ChipLock(device));
  return *p;
}

bool fetch_and_clear_error_word(int *dev_word, hipStream_t s) {
  int e = 0;
  HIP_CHECK(hipMemcpyAsync(&e, dev_word, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (e) HIP_CHECK(hipMemsetAsync(dev_word, 0, sizeof(int), s));
  return e != 0;
}

}  // namespace xdtts
