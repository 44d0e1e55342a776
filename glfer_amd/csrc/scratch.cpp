// scratch.cpp -- the per-call scratch allocator behind scratch.hpp: pools, kept blocks, the cap.
#include "plan.h"

#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace glfer {
// ---- scratch.  Three sources, by size:
//   * under 1 MiB (statistics, tables, level states): a stream-ordered pool of their own, so that
//     they never carve a piece out of a large free block of the default pool;
//   * 1 MiB .. 16 MiB: the device's default stream-ordered pool, release threshold raised (by default
//     it hands everything back at the next synchronisation);
//   * 16 MiB and more (averaged rows, a mean-corrected copy of a stream, the big-block scratch,
//     LMP / F-test spectra: hundreds of MB to GB): blocks this library keeps (plain hipMalloc, size
//     classes a sixteenth of a power of two apart, at most kBigBlocks per device, never returned
//     before the process ends).  The stream-ordered pool is not made for these: tools/pooltail on this
//     stack -- 2.2 GiB malloc + touch + free + sync per call, sizes alternating by 64 KB: median 2.0 ms
//     a call and ONE CALL IN THREE over 10 ms, up to 4 s (a waterfall call with 2 GiB of averaged
//     rows: 2.3 ms, one in ~100 taking 4.4 s); the same through one kept block: 17 us, never more than
//     24.  A kept block is handed out under a mutex; giving it back records an event on the stream
//     that used it, and the next taker on ANOTHER stream waits for that event first (stream order
//     preserved, nothing synchronised on the host).  When all kept blocks are out (concurrent calls)
//     or would not fit, the request falls through to the pool.  GLFER_SCRATCH_CACHE=0 turns it off.
namespace {
constexpr int kBigBlocks = 6;
constexpr size_t kBigMin = (size_t)16 << 20;
struct BigBlock {
  void *p = nullptr;
  size_t cap = 0;
  bool out = false;
  hipEvent_t freed = nullptr;
  hipStream_t last = nullptr;
  bool used = false;                                 // an event has been recorded on it
  int dev = -1;                                      // the device it was allocated on
};
struct DeviceScratch {
  bool init = false;
  hipMemPool_t small_pool = nullptr;
  BigBlock big[kBigBlocks];
};
std::mutex g_scratch_mu;
DeviceScratch g_scratch[64];
// Bytes of kept blocks per device above which IDLE blocks are given back before a new one is made
// (GLFER_SCRATCH_CAP_MB; default 16 GiB of a 288 GB card; glfer_hip_scratch_limit sets it at run time).
// A single request larger than the cap is still served -- by a kept block that is the only one.
size_t g_scratch_cap = [] {
  const char *e = getenv("GLFER_SCRATCH_CAP_MB");
  return e && *e ? (size_t)strtoull(e, nullptr, 10) << 20 : (size_t)16 << 30;
}();
// Frees one idle kept block (after the work recorded on it has completed).  Caller holds the mutex
// and has the block's device current.
void drop_block(BigBlock &b) {
  if (b.used) (void)hipEventSynchronize(b.freed);
  (void)hipFree(b.p);
  (void)hipEventDestroy(b.freed);
  b = BigBlock();
}
// Idle kept blocks of a device, smallest first, until at most `keep_bytes` stay (blocks that are out
// with a call stay and count).  Returns the bytes freed.
size_t trim_locked(DeviceScratch &ds, size_t keep_bytes) {
  size_t held = 0, freed = 0;
  for (BigBlock &b : ds.big)
    if (b.p) held += b.cap;
  while (held > keep_bytes) {
    BigBlock *victim = nullptr;
    for (BigBlock &b : ds.big)
      if (b.p && !b.out && (!victim || b.cap < victim->cap)) victim = &b;
    if (!victim) break;
    held -= victim->cap;
    freed += victim->cap;
    drop_block(*victim);
  }
  return freed;
}
bool scratch_cache_on() {
  static const bool on = [] {
    const char *e = getenv("GLFER_SCRATCH_CACHE");
    return !(e && atoi(e) == 0 && *e);
  }();
  return on;
}
}  // namespace

bool scratch_keeping() { return scratch_cache_on(); }
size_t scratch_cap() {
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  return g_scratch_cap;
}

hipError_t scratch_malloc(void **p, size_t bytes, hipStream_t st) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipMallocAsync(p, bytes, st);
  std::unique_lock<std::mutex> lock(g_scratch_mu);
  DeviceScratch &ds = g_scratch[dev];
  if (!ds.init) {
    ds.init = true;
    hipMemPool_t pool = nullptr;
    uint64_t keep = (uint64_t)8 << 30;
    if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess ||
        hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess)
      (void)hipGetLastError();                   // the pool keeps its default: slower, not wrong
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    uint64_t keep_small = (uint64_t)64 << 20;
    if (hipMemPoolCreate(&ds.small_pool, &props) != hipSuccess ||
        hipMemPoolSetAttribute(ds.small_pool, hipMemPoolAttrReleaseThreshold, &keep_small) != hipSuccess) {
      (void)hipGetLastError();                   // no second pool: everything from the default one
      ds.small_pool = nullptr;
    }
  }
  if (bytes < ((size_t)1 << 20) && ds.small_pool) {
    hipMemPool_t from = ds.small_pool;
    lock.unlock();
    return hipMallocFromPoolAsync(p, bytes, from, st);
  }
  if (bytes >= kBigMin && scratch_cache_on()) {
    size_t cls = (size_t)1 << 20;                    // size classes: a batch one row longer finds the block of the last call
    while (cls * 32 <= bytes) cls <<= 1;
    const size_t want = (bytes + cls - 1) / cls * cls;
    BigBlock *best = nullptr, *empty = nullptr;
    for (BigBlock &b : ds.big) {
      if (!b.p) {
        if (!empty) empty = &b;
      } else if (!b.out && b.cap >= want && (!best || b.cap < best->cap)) {
        best = &b;
      }
    }
    if (!best && !empty) {                           // every slot taken by smaller blocks: the smallest idle one makes room
      BigBlock *victim = nullptr;
      for (BigBlock &b : ds.big)
        if (!b.out && b.cap < want && (!victim || b.cap < victim->cap)) victim = &b;
      if (victim) {
        drop_block(*victim);
        empty = victim;
      }
    }
    if (!best && empty) {                            // a new kept block (synchronous hipMalloc: once per size class)
      // the byte cap: idle blocks go first (none of them fits -- `best` would have been one)
      size_t held = 0;
      for (BigBlock &b : ds.big)
        if (b.p) held += b.cap;
      if (held + want > g_scratch_cap) trim_locked(ds, g_scratch_cap > want ? g_scratch_cap - want : 0);
      void *q = nullptr;
      hipEvent_t ev = nullptr;
      hipError_t me = hipMalloc(&q, want);
      if (me != hipSuccess) {                        // out of memory: every idle kept block goes back, then once more
        (void)hipGetLastError();
        q = nullptr;
        if (trim_locked(ds, 0) > 0) me = hipMalloc(&q, want);
        for (BigBlock &b : ds.big)                   // the slot may have moved: any empty one will do
          if (!b.p) { empty = &b; break; }
      }
      if (me == hipSuccess && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
        empty->p = q;
        empty->cap = want;
        empty->freed = ev;
        empty->used = false;
        empty->dev = dev;
        best = empty;
      } else {
        (void)hipGetLastError();
        if (q) (void)hipFree(q);
      }
    }
    if (best) {
      best->out = true;
      hipError_t e = hipSuccess;
      if (best->used && best->last != st) e = hipStreamWaitEvent(st, best->freed, 0);
      if (e != hipSuccess) {
        best->out = false;
        return e;
      }
      *p = best->p;
      return hipSuccess;
    }
  }
  lock.unlock();
  return hipMallocAsync(p, bytes, st);
}

// gives back what scratch_malloc handed out (stream-ordered either way)
void scratch_free(void *q, hipStream_t st) {
  if (!q) return;
  {
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    for (DeviceScratch &ds : g_scratch)
      for (BigBlock &b : ds.big)
        if (b.p == q) {
          // the event is recorded on the stream that used the block -- a stream of the block's own
          // device, which need not be the caller's current one
          int cur = -1;
          const bool moved = hipGetDevice(&cur) == hipSuccess && cur != b.dev && b.dev >= 0 && hipSetDevice(b.dev) == hipSuccess;
          if (hipEventRecord(b.freed, st) == hipSuccess) {
            b.used = true;
            b.last = st;
          } else {
            // no event to order the next taker behind: wait here for the work on `st`, after which
            // the block is free for any stream (used = false: nothing to wait for)
            (void)hipGetLastError();
            if (hipStreamSynchronize(st) != hipSuccess) {
              (void)hipGetLastError();               // not even that: the block leaves the cache for good
              (void)hipDeviceSynchronize();
              (void)hipFree(b.p);
              (void)hipEventDestroy(b.freed);
              b = BigBlock();
              if (moved) (void)hipSetDevice(cur);
              return;
            }
            b.used = false;
            b.last = nullptr;
          }
          b.out = false;
          // the cap bounds what is KEPT, not only what is newly made: a block handed back while the
          // device holds more than the cap -- a reused block larger than a cap set since, glfer_hip_scratch_limit(0)
          // -- goes back now (drop_block waits for the event just recorded, then hipFree)
          if (b.dev >= 0 && b.dev < 64) trim_locked(g_scratch[b.dev], g_scratch_cap);
          if (moved) (void)hipSetDevice(cur);
          return;
        }
  }
  (void)hipFreeAsync(q, st);
}

// glfer_hip_scratch_trim / glfer_hip_scratch_limit (include/glfer_hip.h)
size_t scratch_trim(int dev, size_t keep_bytes) {
  if (dev < 0 || dev >= 64) return 0;
  DeviceGuard guard(dev);
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  return trim_locked(g_scratch[dev], keep_bytes);
}
size_t scratch_held(int dev) {
  if (dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  size_t held = 0;
  for (BigBlock &b : g_scratch[dev].big)
    if (b.p) held += b.cap;
  return held;
}
void scratch_set_cap(size_t bytes) {
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  g_scratch_cap = bytes;
  // idle blocks above the new cap go back at once, on every device that holds any
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  for (int dev = 0; dev < 64; dev++) {
    size_t held = 0;
    for (BigBlock &b : g_scratch[dev].big)
      if (b.p) held += b.cap;
    if (held <= bytes) continue;
    if (dev != cur && hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); continue; }
    trim_locked(g_scratch[dev], bytes);
    if (dev != cur && cur >= 0) (void)hipSetDevice(cur);
  }
}

}  // namespace glfer
