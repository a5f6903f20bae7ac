// stage.hpp -- the staging of one chunked call and its whole protocol: HIP host
// code only (no kernel, no ipls_dev, no engine lock).  engine.hip drives every
// chunked entry point through these steps and maps a step's Status to its error.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/ipls_agg.h"

namespace ipls {
struct PinnedSlot {
  void* host = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
};
}  // namespace ipls

// The staging of one chunked call, owned by that call alone from acquire to
// release, so the caller's source or sink -- a socket recv/send, a JNI array
// copy -- runs with no engine lock held.  A pinned host
// ring, a device buffer for the whole bucket (or snapshot) and two copy
// streams of its own.  Stages are pooled per shard and freed only at close.
//   inbound  (host -> `d` -> fold): acquire, begin_in, per chunk slot + push,
//     landed; under the engine lock join, the fold, mark_read; release.
//   outbound (snapshot -> `d` -> sink): acquire; under the engine lock the
//     snapshot kernel, publish; then ring, once or several times; release.
//   any failure after acquire: release(ok = false), the give-up path.
// Invariants of a stage in the pool: every pinned slot whose copy may still be
// in flight is `pending` (its event recorded after that copy); `free_pending`
// says a kernel on the shard stream may still read `d` (`free_ev` recorded
// after it); `ready_pending` -- `ready` was recorded for this use (publish)
// and nothing has waited for it yet (the ring's wait and the give-up path
// clear it) -- is false, so no snapshot kernel still writes `d`.
struct ipls_stage {
  // chunk k crosses PCIe on copy[k % n_copy]: with two streams the DMA setup
  // of chunk k + 1 overlaps the transfer of chunk k (IPLS_STAGE_STREAMS=1
  // gives one stream, the A/B of profiles/r06)
  hipStream_t copy[2] = {};
  int n_copy = 0;
  // the pinned host ring: chunk k in slot k % n_slot, so the copy engine can
  // run up to n_slot - 1 chunks ahead of a caller's slow source or sink
  // (IPLS_STAGE_SLOTS, 2..4; 3 by default)
  static constexpr int kMaxSlots = 4;
  ipls::PinnedSlot slot[kMaxSlots];
  int n_slot = 0;
  void* d = nullptr;
  size_t d_cap = 0;
  hipEvent_t landed[2] = {};      // copy streams -> shard stream: every chunk is in `d`
  hipEvent_t ready = nullptr;     // shard stream -> copy streams: the snapshot is in `d`
  bool ready_pending = false;
  hipEvent_t free_ev = nullptr;   // shard stream: the fold that read `d` has run
  bool free_pending = false;
};

namespace ipls {
namespace stage {

// What a step reports: IPLS_OK, a failed HIP call (the text is "<what> failed:
// <hipGetErrorString(hip)>") or, with hip == hipSuccess, a refusal whose text is `what`.
struct Status {
  int code = IPLS_OK;
  const char* what = "";
  hipError_t hip = hipSuccess;
  explicit operator bool() const { return code != IPLS_OK; }
};

// A failed call also leaves HIP's per-thread last error set; it is cleared here.
inline Status hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return {};
  (void)hipGetLastError();
  return {e == hipErrorOutOfMemory ? IPLS_E_NOMEM : IPLS_E_DEVICE, what, e};
}

// One per engine: a stage per concurrent chunked call, made lazily.  `mu` guards the vectors only.
struct Pool {
  std::mutex mu;
  std::vector<ipls_stage*> all, idle;
};

// Back to the pool.  ok: the success path, no HIP call.  Otherwise (and for a
// published snapshot nothing has waited for) the one give-up path: every copy
// of this use is done and a recorded snapshot is complete before any reuse.
inline void release(Pool& pool, ipls_stage* st, bool ok) {
  if (!ok || st->ready_pending) {
    for (int i = 0; i < st->n_copy; ++i) (void)hipStreamSynchronize(st->copy[i]);
    if (st->ready_pending) (void)hipEventSynchronize(st->ready);
    (void)hipGetLastError();
    st->ready_pending = false;
    for (auto& sl : st->slot) sl.pending = false;
  }
  std::lock_guard<std::mutex> lk(pool.mu);
  pool.idle.push_back(st);
}

// Take an idle stage of the pool (or make one) and size it, on its device: `dev_bytes` of device buffer, pinned
// slots of `slot_bytes`.  Regrowing frees only memory this call owns, after the copies and the kernel that last
// used it are done.
inline Status acquire(Pool& pool, size_t dev_bytes, size_t slot_bytes, ipls_stage** out) {
  *out = nullptr;
  ipls_stage* st = nullptr;
  {
    std::lock_guard<std::mutex> lk(pool.mu);
    if (pool.idle.empty()) {
      pool.all.push_back(st = new ipls_stage());
    } else {
      st = pool.idle.back();
      pool.idle.pop_back();
    }
  }
  if (!st->n_copy) {
    const char* e = std::getenv("IPLS_STAGE_STREAMS");
    st->n_copy = (e && std::atoi(e) == 1) ? 1 : 2;
    const char* sl = std::getenv("IPLS_STAGE_SLOTS");
    st->n_slot = sl ? std::max(2, std::min(ipls_stage::kMaxSlots, std::atoi(sl))) : 3;
  }
  Status rc;
  for (int i = 0; i < st->n_copy && !rc; ++i)
    if (!st->copy[i]) rc = hip(hipStreamCreateWithFlags(&st->copy[i], hipStreamNonBlocking), "hipStreamCreate");
  for (hipEvent_t* e : {&st->landed[0], &st->landed[1], &st->ready, &st->free_ev})
    if (!rc && !*e) rc = hip(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate");
  if (!rc && st->d_cap < dev_bytes) {
    if (st->d) {
      // the fold that last read `d` and every copy of the stage are done before it is freed
      if (st->free_pending) rc = hip(hipEventSynchronize(st->free_ev), "hipEventSynchronize");
      for (int i = 0; i < st->n_copy && !rc; ++i) rc = hip(hipStreamSynchronize(st->copy[i]), "hipStreamSynchronize");
      if (!rc) rc = hip(hipFree(st->d), "hipFree");
      if (!rc) {
        st->d = nullptr;
        st->d_cap = 0;
        st->free_pending = false;
      }
    }
    const size_t cap = (dev_bytes + (1 << 20) - 1) >> 20 << 20;
    if (!rc) rc = hip(hipMalloc(&st->d, cap), "hipMalloc");
    if (!rc) st->d_cap = cap;
  }
  for (int i = 0; i < st->n_slot && !rc; ++i) {
    PinnedSlot& s = st->slot[i];
    if (s.cap < slot_bytes) {
      if (s.pending) rc = hip(hipEventSynchronize(s.ev), "hipEventSynchronize");
      if (!rc) s.pending = false;
      // never free a slot a copy may still read or write (the r05/h fault
      // analysis): its last copy's event must have completed
      if (!rc && s.host && s.ev && hipEventQuery(s.ev) != hipSuccess) {
        (void)hipGetLastError();
        rc = {IPLS_E_DEVICE, "internal: pinned slot regrown with a copy in flight"};
      }
      if (!rc && s.host) rc = hip(hipHostFree(s.host), "hipHostFree");
      if (!rc) {
        s.host = nullptr;
        s.cap = 0;
        const size_t cap = std::max<size_t>(slot_bytes, 64 << 10);
        rc = hip(hipHostMalloc(&s.host, cap, hipHostMallocDefault), "hipHostMalloc");
        if (!rc) s.cap = cap;
      }
    }
    if (!rc && !s.ev) rc = hip(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming), "hipEventCreate");
  }
  if (rc) release(pool, st, true);   // nothing of this use was queued
  else *out = st;
  return rc;
}

// At close, once no call uses the engine: every stage ever made is freed.
inline void destroy(Pool& pool) {
  for (ipls_stage* st : pool.all) {
    for (hipStream_t cs : st->copy)
      if (cs) {
        hipStreamSynchronize(cs);
        hipStreamDestroy(cs);
      }
    for (auto& s : st->slot) {
      if (s.host) hipHostFree(s.host);
      if (s.ev) hipEventDestroy(s.ev);
    }
    if (st->d) hipFree(st->d);
    for (hipEvent_t e : {st->landed[0], st->landed[1], st->ready, st->free_ev})
      if (e) hipEventDestroy(e);
    delete st;
  }
}

// ---- inbound ----
// The fold that last read `d` runs before this use's copies overwrite it.
inline Status begin_in(ipls_stage* st) {
  Status rc;
  for (int i = 0; i < st->n_copy && st->free_pending && !rc; ++i)
    rc = hip(hipStreamWaitEvent(st->copy[i], st->free_ev, 0), "hipStreamWaitEvent");
  return rc;
}

// The pinned slot of chunk k, free for the host to write: the copy that last used it is done.
inline Status slot(ipls_stage* st, int64_t k, void** host) {
  PinnedSlot& sl = st->slot[k % st->n_slot];
  if (sl.pending) {
    if (Status rc = hip(hipEventSynchronize(sl.ev), "hipEventSynchronize")) return rc;
    sl.pending = false;
  }
  *host = sl.host;
  return {};
}

// Chunk k's H2D copies, n_ranges of them, in elements of esz bytes: n[i] from
// src[i] of the slot to dst[i] of `d` + pad, every range inside the slot and
// ending at least `pad` bytes before the end of `d`.
inline Status push(ipls_stage* st, int64_t k, const int64_t* src, const int64_t* dst, const int64_t* n, int n_ranges,
                   size_t esz, size_t pad = 0) {
  PinnedSlot& sl = st->slot[k % st->n_slot];
  hipStream_t cs = st->copy[k % st->n_copy];
  for (int i = 0; i < n_ranges; ++i) {
    if (src[i] < 0 || dst[i] < 0 || n[i] < 0 || (size_t)(src[i] + n[i]) * esz > sl.cap ||
        (size_t)(dst[i] + n[i]) * esz + 2 * pad > st->d_cap)
      return {IPLS_E_INVAL, "internal: a staged range outside its buffers"};
    char* to = (char*)st->d + pad + (size_t)dst[i] * esz;
    const char* from = (const char*)sl.host + (size_t)src[i] * esz;
    if (Status rc = hip(hipMemcpyAsync(to, from, (size_t)n[i] * esz, hipMemcpyHostToDevice, cs), "hipMemcpyAsync"))
      return rc;
    sl.pending = true;   // from the first queued copy on: the event below, or the give-up drain, covers it
  }
  return hip(hipEventRecord(sl.ev, cs), "hipEventRecord");
}

// After the last chunk: the events the shard stream will wait for.
inline Status landed(ipls_stage* st) {
  Status rc;
  for (int i = 0; i < st->n_copy && !rc; ++i) rc = hip(hipEventRecord(st->landed[i], st->copy[i]), "hipEventRecord");
  return rc;
}

// With the engine lock held: the shard stream waits for every chunk (no host wait).
inline Status join(ipls_stage* st, hipStream_t shard) {
  Status rc;
  for (int i = 0; i < st->n_copy && !rc; ++i)
    rc = hip(hipStreamWaitEvent(shard, st->landed[i], 0), "hipStreamWaitEvent");
  return rc;
}

// With the engine lock held, after the fold or its failure: whatever ran,
// nothing queued on the shard stream after this point reads `d`.
inline void mark_read(ipls_stage* st, hipStream_t shard) {
  st->free_pending = hipEventRecord(st->free_ev, shard) == hipSuccess;
  if (st->free_pending) return;
  (void)hipGetLastError();
  (void)hipStreamSynchronize(shard);
}

// ---- outbound ----
// With the engine lock held, after the snapshot kernel was queued on the shard stream.
inline Status publish(ipls_stage* st, hipStream_t shard) {
  const Status rc = hip(hipEventRecord(st->ready, shard), "hipEventRecord");
  st->ready_pending = !rc;
  return rc;
}

// The published snapshot handed out in pieces, with no engine lock held: piece k + 1 crosses PCIe into one pinned
// slot on a copy stream while the consumer has piece k from another.  In bytes: [0, n) at `d` (inside the stage's
// buffer) go to call(host, off, len) in pieces of c; a non-zero return stops the ring and is returned.  A HIP
// failure sets *err and returns its code.  The stage stays the caller's: release(ok) after IPLS_OK only (copies
// may still be in flight otherwise).
template <class Call>
int ring(ipls_stage* st, const char* d, int64_t n, int64_t c, Status* err, Call call) {
  Status rc;
  void* host = nullptr;
  // a previous call's H2D may still read a slot (an inbound call does not
  // wait for its copies on the host): the D2H into it waits for that copy
  for (int i = 0; i < st->n_slot && !rc; ++i) rc = slot(st, i, &host);
  auto also = [&](Status s) { rc = rc ? rc : s; };   // every call is made, the first failure kept
  for (int i = 0; i < st->n_copy; ++i) also(hip(hipStreamWaitEvent(st->copy[i], st->ready, 0), "hipStreamWaitEvent"));
  // the copy streams now run behind `ready`: waiting for them waits for the snapshot too
  if (!rc) st->ready_pending = false;
  const int64_t K = n > 0 ? (n + c - 1) / c : 0;
  int64_t issued = 0;
  auto issue = [&]() {   // the next chunk, into slot issued % n_slot (its previous chunk's sink has returned)
    const int64_t k = issued++, off = k * c, len = std::min(c, n - off);
    PinnedSlot& sl = st->slot[k % st->n_slot];
    hipStream_t cs = st->copy[k % st->n_copy];
    also(hip(hipMemcpyAsync(sl.host, d + off, (size_t)len, hipMemcpyDeviceToHost, cs), "hipMemcpyAsync"));
    also(hip(hipEventRecord(sl.ev, cs), "hipEventRecord"));
    sl.pending = true;
  };
  while (issued < K && issued < st->n_slot && !rc) issue();   // the ring's first fill
  int stopped = 0;
  for (int64_t k = 0; k < K && !rc && !stopped; ++k) {
    if ((rc = slot(st, k, &host))) break;   // chunk k is in its slot
    stopped = call(host, k * c, std::min(c, n - k * c));
    if (!stopped && issued < K) issue();   // into the slot just consumed
  }
  if (rc) *err = rc;
  return rc ? rc.code : stopped;
}

}  // namespace stage
}  // namespace ipls
