// engine.hip -- the single-device aggregation engine behind the C-ABI
// (include/ipls_agg.h; the exported entry points are in ipls_agg.cpp, which
// shards a handle's partitions over one engine per device).  One engine =
// the PeerData accumulator state of a contiguous block of partitions on one
// GPU, one HIP stream, one mutex.
//
// Device layout: one arena of doubles per handle holding, for
// every partition p, four arrays of L_p doubles -- AGG (Aggregated_Gradients,
// PeerData.java:144), REP (Replicas_Gradients, :137), FUT (Aggregated_
// Gradients_from_future) and W (Weights, :149, which IPLS.java:1141 aliases
// with Weight_Address, :189) -- each starting on a 256-byte boundary.
// Device-side tables (partition descriptors + bucket pointers) are uploaded
// through a small pinned ring and cached, so a repeated reduce over resident
// buckets is one kernel launch and nothing else.  The chunked calls stage
// through a stage each (struct ipls_stage, pooled per engine) and take the
// engine lock only for their fold or snapshot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/ipls_agg.h"
#include "ipls_kernels.hpp"
#include "seg_kernels.hpp"
#include "seg_diff_kernels.hpp"
#include "seg_peers_kernels.hpp"
#include "seg_copies_kernels.hpp"
#include "seg_round_kernels.hpp"
#include "javaser.hpp"
#include "engine.hpp"
#include "operand.hpp"
#include "pubsub_host.hpp"
#include "reduce_plan.hpp"
#include "seg_plan.hpp"
#include "stage.hpp"

using namespace ipls;
using namespace ipls::reduceplan;
namespace op = ipls::operand;
namespace stg = ipls::stage;

namespace {

thread_local std::string g_tls_err;

constexpr int64_t kAlignElems = 32;  // 256 B
constexpr int kRingSlots = 4;

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

}  // namespace

struct ipls_dev {
  std::mutex mu;
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;

  // geometry
  int64_t model_size = 0;  // 0 => synthetic geometry
  int P = 0;
  int64_t chunk = 0;  // flat stride between partitions
  int secure = 0;
  std::vector<int64_t> len, flat_off;
  int64_t max_len = 0, flat_total = 0;   // flat_total: end of this engine's flat segment
  int p_lo = 0;                           // first partition of the handle held here
  int64_t flat_base = 0;                  // flat offset of partition p_lo

  // arena
  double* arena = nullptr;
  int64_t arena_elems = 0;
  std::vector<int64_t> agg_off, rep_off, w_off, fut_off;
  std::vector<uint8_t> agg_zero, rep_zero, fut_zero;  // "logically +0.0" flags

  // table upload ring (pinned host slots -> device slots)
  PinnedSlot ring[kRingSlots];
  void* d_table[kRingSlots] = {};
  size_t d_table_cap[kRingSlots] = {};
  int ring_next = 0;
  std::vector<unsigned char> last_table;  // cache of the last uploaded table
  int last_slot = -1;

  // staging of the chunked calls (stage.hpp): one stage per concurrent call,
  // pooled (lazily, freed at close); the pool's mutex is never taken with mu
  // held for longer than a push
  stg::Pool stages;
  // staging
  void* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  hipEvent_t copy_ev = nullptr;
  // pubsub ingest pipeline: text copies on their own stream, the decodes on
  // `stream` behind an event per message (created on first use)
  static constexpr int kCopyThreads = 4;
  hipStream_t copy_stream[kCopyThreads] = {};
  hipEvent_t ingest_ev = nullptr;
  std::vector<hipEvent_t> msg_ev;
  // Per-arrival staging of pageable buckets, double-buffered: bucket k+1 is
  // copied into one slot while the fold of bucket k still reads the other.
  struct StageSlot {
    void* d = nullptr;
    size_t cap = 0;
    hipEvent_t free_ev = nullptr;   // recorded after the fold that reads the slot
    bool pending = false;
  };
  StageSlot stage[2];
  int stage_next = 0;
  // Asynchronous folds (ipls_agg_accumulate_async).  Device buckets are not
  // folded on arrival: per (target, partition) their pointers queue up and the
  // next flush folds each queue in one launch, in call order -- the same
  // expression (((acc + b0) + b1) + ...) the per-arrival folds evaluate, at
  // (k+2)/k x 8 B per element instead of 24.  Every other entry point flushes
  // first (IPLS_LOCK).  Pinned host buckets fold at once (zero copy).
  struct Pending {
    std::vector<const void*> bufs;
    Fmt fmt = kFmtF64;   // the queue's bucket format (one per queue)
  };
  // queue of (target, p) at pend[target * P + p]; pend_keys lists the
  // non-empty ones (a flat table: the per-arrival call is a few loads and a
  // push, no map walk)
  std::vector<Pending> pend;
  std::vector<int> pend_keys;
  int pending_n = 0;
  int coalesce = 32;                                // queue length that triggers a flush (ipls_agg_set_coalesce)
  // Tickets complete in issue order: a launch happens only after every earlier
  // ticket was launched, and batch b completes tickets (prev.max, b.max_ticket].
  struct Batch {
    uint64_t max_ticket;
    hipEvent_t ev;
  };
  static constexpr int kMaxBatches = 64;
  std::deque<Batch> batches;
  std::vector<hipEvent_t> ev_free;
  uint64_t ticket_next = 1, ticket_done = 0, launched_upto = 0;

  // checksum result
  unsigned long long* d_sum = nullptr;
  double* d_cnt = nullptr;   // per-partition count slots of a fused round (P doubles)
  unsigned long long* d_gbuf = nullptr;   // Updater.run's Gradient_Buff (Updater.java:162), lazily
  unsigned long long* d_merge = nullptr;  // storage-merge accumulator, grown on demand
  int64_t merge_cap = 0;
  // PeerData.Other_Replica_Gradients / _Received, keyed (partition, aggregator);
  // Collect_Replicas folds them in the order the front's HashMap model gives
  struct OtherRep {
    unsigned long long* d = nullptr;
    int64_t n = 0;
    int32_t received = 0;
  };
  std::map<std::pair<int, int32_t>, OtherRep> other;
  int64_t gbuf_len = 0;
  ipls_launch_info last_launch{};   // the last fold launch (ipls_agg_last_launch)
};

namespace {

int fail(ipls_dev* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  g_tls_err = buf;
  return code;
}

// What a call returns when op::resolve did not say kTake: IPLS_OK for a no-op,
// else the refusal's code with its text as the handle's error.
int not_taken(ipls_dev* h, const op::Refusal& why) { return why.code ? fail(h, why.code, "%s", why.text) : IPLS_OK; }

int flush_pending(ipls_dev* h);

// Take the handle's lock and fold any queued asynchronous device arrivals
// first, so every entry point sees the accumulators in call order.
#define IPLS_LOCK(h)                            \
  std::lock_guard<std::mutex> lk_(h->mu);       \
  if (int rc_ = flush_pending(h)) return rc_

// A failed call also leaves HIP's per-thread last error set; it is cleared
// here so that the next launch check (hipGetLastError) does not report it.
#define HIP_TRY(h, expr)                                                                \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (void)hipGetLastError();                                                          \
      return fail((h), e_ == hipErrorOutOfMemory ? IPLS_E_NOMEM : IPLS_E_DEVICE,        \
                  "%s failed: %s", #expr, hipGetErrorString(e_));                       \
    }                                                                                   \
  } while (0)

int64_t ref_chunk(int64_t m, int p) { return (int64_t)(int32_t)(m / p) + 1; }  // IPLS.java:1019


int check_part(ipls_dev* h, int p) {
  if (p < 0 || p >= h->P) return fail(h, IPLS_E_RANGE, "partition %d out of range [0,%d)", p, h->P);
  return IPLS_OK;
}

int64_t target_off(ipls_dev* h, int p, int target) {
  switch (target) {
    case IPLS_TGT_AGG: return h->agg_off[p];
    case IPLS_TGT_REP: return h->rep_off[p];
    case IPLS_TGT_WEIGHTS:
    case IPLS_TGT_WADDR: return h->w_off[p];
    case IPLS_TGT_FUTURE: return h->fut_off[p];
    default: return -1;
  }
}

uint8_t* zero_flag(ipls_dev* h, int p, int target) {
  if (target == IPLS_TGT_AGG) return &h->agg_zero[p];
  if (target == IPLS_TGT_REP) return &h->rep_zero[p];
  if (target == IPLS_TGT_FUTURE) return &h->fut_zero[p];
  return nullptr;
}

// Make a logically-zero accumulator physically zero (before anything reads it
// with ACCUM semantics or hands its address out).
int materialize(ipls_dev* h, int p, int target) {
  uint8_t* f = zero_flag(h, p, target);
  if (f && *f) {
    HIP_TRY(h, hipMemsetAsync(h->arena + target_off(h, p, target), 0, (size_t)h->len[p] * 8, h->stream));
    *f = 0;
  }
  return IPLS_OK;
}

int ensure_pinned(ipls_dev* h, PinnedSlot& s, size_t bytes) {
  if (s.pending) {
    HIP_TRY(h, hipEventSynchronize(s.ev));
    s.pending = false;
  }
  if (s.cap < bytes) {
    if (s.host) HIP_TRY(h, hipHostFree(s.host));
    s.host = nullptr;
    s.cap = 0;
    size_t cap = std::max<size_t>(bytes, 64 << 10);
    HIP_TRY(h, hipHostMalloc(&s.host, cap, hipHostMallocDefault));
    s.cap = cap;
  }
  if (!s.ev) HIP_TRY(h, hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  return IPLS_OK;
}

// ---- chunked-call staging (ipls_stage) ----
// A failure outside the engine lock: the calling thread's message, and the
// handle's under its lock (h->err is shared with the locked paths).
int fail_nl(ipls_dev* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_tls_err = buf;
  if (h) {
    std::lock_guard<std::mutex> lk(h->mu);
    h->err = buf;
  }
  return code;
}

// A stage step's Status (stage.hpp) as this engine's error: with the engine lock held (`locked`) or not.
int stage_rc(ipls_dev* h, const stg::Status& s, bool locked = false) {
  if (!s) return IPLS_OK;
  const auto f = locked ? fail : fail_nl;
  return s.hip == hipSuccess ? f(h, s.code, "%s", s.what) : f(h, s.code, "%s failed: %s", s.what, hipGetErrorString(s.hip));
}

// The shard's device made current on the calling thread, outside the engine lock.
int use_nl(ipls_dev* h) { return stage_rc(h, stg::hip(dev_use(h->device), "dev_use(h->device)")); }

}  // namespace

// The end of a chunked call's use of its stage (engine.hpp): stage.hpp's release, its give-up path after a failure.
void dev_stage_release(ipls_dev* h, ipls_stage* st, int rc) {
  if (!h || !st) return;
  if (rc) (void)dev_use(h->device);
  stg::release(h->stages, st, rc == IPLS_OK);
}

namespace {

// The outbound half every chunked read starts with: a stage of the call's own (every buffer first: a failure
// there leaves the accumulators as they were), then under the engine lock the queued arrivals, fill(st) -- which
// queues the snapshot into st->d on the shard stream -- and the publish.
template <class Fill>
int stage_snapshot(ipls_dev* h, size_t dev_bytes, size_t slot_bytes, ipls_stage** out, Fill fill) {
  if (int rc = use_nl(h)) return rc;
  ipls_stage* st = nullptr;
  if (int rc = stage_rc(h, stg::acquire(h->stages, dev_bytes, slot_bytes, &st))) return rc;
  int rc = IPLS_OK;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    rc = flush_pending(h);
    if (!rc) rc = fill(st);
    if (!rc) rc = stage_rc(h, stg::publish(st, h->stream), true);
  }
  if (rc) {   // a kernel of this call may have been queued before the failure
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
    dev_stage_release(h, st, rc);
    return rc;
  }
  *out = st;
  return IPLS_OK;
}

// The geometry checks of the chunked entries, fixed at open and so made without the lock (a target's offset is
// not read: promote_future swaps AGG/FUT storage under it).
int check_chunk(ipls_dev* h, int64_t chunk, const char* unit) {
  const bool ok = chunk >= 2 && !(chunk & 1);
  return ok ? IPLS_OK : fail_nl(h, IPLS_E_INVAL, "chunk of %lld %s: even and >= 2", (long long)chunk, unit);
}
int check_part_nl(ipls_dev* h, int p) {
  return p >= 0 && p < h->P ? IPLS_OK : fail_nl(h, IPLS_E_RANGE, "partition %d out of range [0,%d)", p, h->P);
}
int check_target_nl(ipls_dev* h, int target) {
  const bool ok = target >= IPLS_TGT_AGG && target <= IPLS_TGT_FUTURE;
  return ok ? IPLS_OK : fail_nl(h, IPLS_E_INVAL, "bad target %d", target);
}

int ensure_scratch(ipls_dev* h, size_t bytes) {
  if (h->scratch_bytes >= bytes) return IPLS_OK;
  if (h->d_scratch) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipFree(h->d_scratch));
    h->d_scratch = nullptr;
    h->scratch_bytes = 0;
  }
  size_t cap = (size_t)align_up((int64_t)bytes, 1 << 20);
  HIP_TRY(h, hipMalloc(&h->d_scratch, cap));
  h->scratch_bytes = cap;
  return IPLS_OK;
}

// Upload a table through the pinned ring; returns its device address.  An
// identical table to the previous upload is not re-sent.
int upload_table(ipls_dev* h, const void* data, size_t bytes, void** dev) {
  if (h->last_slot >= 0 && h->last_table.size() == bytes &&
      std::memcmp(h->last_table.data(), data, bytes) == 0) {
    *dev = h->d_table[h->last_slot];
    return IPLS_OK;
  }
  const int s = h->ring_next;
  h->ring_next = (s + 1) % kRingSlots;
  int rc = ensure_pinned(h, h->ring[s], bytes);
  if (rc) return rc;
  if (h->d_table_cap[s] < bytes) {
    if (h->d_table[s]) {
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      HIP_TRY(h, hipFree(h->d_table[s]));
    }
    h->d_table[s] = nullptr;
    h->d_table_cap[s] = 0;
    size_t cap = std::max<size_t>(bytes, 64 << 10);
    HIP_TRY(h, hipMalloc(&h->d_table[s], cap));
    h->d_table_cap[s] = cap;
  }
  std::memcpy(h->ring[s].host, data, bytes);
  HIP_TRY(h, hipMemcpyAsync(h->d_table[s], h->ring[s].host, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->ring[s].ev, h->stream));
  h->ring[s].pending = true;
  h->last_table.assign((const unsigned char*)data, (const unsigned char*)data + bytes);
  h->last_slot = s;
  *dev = h->d_table[s];
  return IPLS_OK;
}

// Copy `bytes` of host memory to device `dst` through the pinned double buffer.
// The caller's buffer is no longer referenced when this returns.
bool is_pinned_host(const void* p, void** dev_alias = nullptr) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: clear the sticky error
    return false;
  }
  if (a.type != hipMemoryTypeHost) return false;
  if (dev_alias) {
    // device address of the same bytes (== p for hipHostMalloc; may differ
    // for hipHostRegister'ed memory)
    const char* base_h = (const char*)a.hostPointer;
    const char* base_d = (const char*)a.devicePointer;
    *dev_alias = (base_h && base_d) ? (void*)(base_d + ((const char*)p - base_h)) : nullptr;
  }
  return true;
}

// Memory a kernel of this process may write at the address p itself: device
// memory, or pinned host memory mapped at the same address (hipHostMalloc).
// Pageable memory is rejected before any launch (a kernel store there faults).
bool kernel_writable(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) return true;
  void* alias = nullptr;
  return a.type == hipMemoryTypeHost && is_pinned_host(p, &alias) && alias == p;
}

// Copy `bytes` of host memory (pinned or pageable) to device `dst` on the
// handle's stream and wait for that copy only: the caller may reuse its buffer
// on return, kernels queued behind the copy keep running.  HIP's own path for
// pageable sources runs at the PCIe rate (56 GB/s measured, tools/h2d_bench.hip),
// where a memcpy into pinned staging was capped at ~31 GB/s by one CPU thread.
int stage_h2d(ipls_dev* h, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return IPLS_OK;
  if (!h->copy_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->copy_ev, hipEventDisableTiming));
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(h->copy_ev, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->copy_ev));
  return IPLS_OK;
}

// Host-synchronous H2D copy of a pageable buffer on a copy stream: no
// ordering against `stream` (the caller owns `dst`), so it overlaps the fold
// of the previous arrival.  (Splitting it over two threads measured within
// noise at 32 MiB and +1.6 % at 64 MiB, profiles/r01/host_e2e_pageable_split.txt.)
int copy_pageable(ipls_dev* h, void* dst, const void* src, size_t bytes) {
  if (!h->copy_stream[0]) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream[0], hipStreamNonBlocking));
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->copy_stream[0]));
  HIP_TRY(h, hipStreamSynchronize(h->copy_stream[0]));
  return IPLS_OK;
}

// Stage one pageable per-arrival bucket into the next of the two staging
// slots; bucket_slot_busy() marks the slot busy until the fold queued after it.
int stage_bucket(ipls_dev* h, const void* src, size_t bytes, const void** dptr) {
  ipls_dev::StageSlot& sl = h->stage[h->stage_next];
  if (sl.pending) {   // the fold that read this slot two arrivals ago
    HIP_TRY(h, hipEventSynchronize(sl.free_ev));
    sl.pending = false;
  }
  if (sl.cap < bytes) {
    if (sl.d) HIP_TRY(h, hipFree(sl.d));
    sl.d = nullptr;
    sl.cap = 0;
    const size_t cap = (size_t)align_up((int64_t)bytes, 1 << 20);
    HIP_TRY(h, hipMalloc(&sl.d, cap));
    sl.cap = cap;
  }
  if (!sl.free_ev) HIP_TRY(h, hipEventCreateWithFlags(&sl.free_ev, hipEventDisableTiming));
  if (int rc = copy_pageable(h, sl.d, src, bytes)) return rc;
  *dptr = sl.d;
  return IPLS_OK;
}

int bucket_slot_busy(ipls_dev* h) {
  ipls_dev::StageSlot& sl = h->stage[h->stage_next];
  HIP_TRY(h, hipEventRecord(sl.free_ev, h->stream));
  sl.pending = true;
  h->stage_next ^= 1;
  return IPLS_OK;
}

int d2h(ipls_dev* h, void* dst, const void* src, size_t bytes) {
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

unsigned blocks_for(int64_t n, int64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// The elementwise kernels (k_fold_n, k_blend, k_scale, k_encode_secure) take
// their 16-B tile shape when every operand is 16-B aligned: one block per
// kEwTile elements; otherwise the 8-B grid-stride loop on a capped grid.
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static dim3 ew_grid(int64_t n, bool vec, unsigned cap) {
  return dim3(std::max(1u, vec ? blocks_for(n, kEwTile) : std::min<unsigned>(blocks_for(n, kBlock), cap)));
}

// ---- runtime flags -> template arguments ----
// Each helper calls f with a value whose type carries the flag as a constant
// (decltype(x)::value; a format is the type itself), so a launch site names
// the combinations it instantiates.  The lambdas only launch.
template <class F> auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

static void launch_bswap(hipStream_t st, const unsigned long long* in, unsigned long long* out, int64_t n) {
  with_bool(al16(in) && al16(out), [&](auto v) {
    hipLaunchKernelGGL(k_bswap64<decltype(v)::value>, ew_grid(n, decltype(v)::value, 4096), dim3(kBlock), 0, st, in, out, n);
  });
}
// Host bytes into the scratch buffer (grown to hold `cap` bytes if that is more) on the handle's stream.
int to_scratch(ipls_dev* h, const void* src, size_t bytes, size_t cap = 0) {
  if (int rc = ensure_scratch(h, std::max<size_t>({bytes, cap, 1}))) return rc;
  return stage_h2d(h, h->d_scratch, src, bytes);
}
// Its mirror: the big-endian bytes of n device doubles, byte-swapped into the scratch buffer, then copied out.
int be_to_host(ipls_dev* h, void* dst, const void* src, int64_t n) {
  if (int rc = ensure_scratch(h, (size_t)n * 8)) return rc;
  launch_bswap(h->stream, (const unsigned long long*)src, (unsigned long long*)h->d_scratch, n);
  HIP_TRY(h, hipGetLastError());
  return d2h(h, dst, h->d_scratch, (size_t)n * 8);
}

template <int V> using Int = std::integral_constant<int, V>;
template <class F> auto with_start(int start, F&& f) {
  return start == kZero ? f(Int<kZero>{}) : start == kFirst ? f(Int<kFirst>{}) : f(Int<kAccum>{});
}
// ZERO or ACCUM only: the fused rounds (AGG is never FIRST-started) and k_fold1_narrow
template <class F> auto with_start_za(int start, F&& f) { return start == kZero ? f(Int<kZero>{}) : f(Int<kAccum>{}); }
// be_in x be_out x start: the flags of a fold over doubles
template <class F> auto with_fold(bool be_in, bool be_out, int start, F&& f) {
  return with_bool(be_in, [&](auto bi) {
    return with_bool(be_out, [&](auto bo) { return with_start(start, [&](auto s) { return f(bi, bo, s); }); });
  });
}
// Calls f with a value of the kernels' format type for a trainer format.
template <class F> auto with_narrow(Fmt fmt, F&& f) {
  switch (fmt) {
    case kFmtF32: return f(FmtF32{});
    case kFmtF16: return f(FmtF16{});
    case kFmtBF16: return f(FmtBF16{});
    default: break;
  }
  // a caller without its fmt_trainer guard: never run a narrow kernel on doubles
  fprintf(stderr, "ipls_agg: with_narrow called with format %d\n", (int)fmt);
  abort();
}

// The plan header is host-only: it takes the C-ABI's start modes, which are the
// kernels' template starts, and states the map-2 grid and the default block again.
static_assert(kZero == IPLS_START_ZERO && kFirst == IPLS_START_FIRST && kAccum == IPLS_START_ACCUM, "one start code");
static_assert(kSmallBS == kBlock && kScalarBS == kBlock, "one default block");
static_assert(plan_grid(2, 1) == grid_blocks(2, 1) && plan_grid(2, 8) == grid_blocks(2, 8) &&
              plan_grid(2, 4097) == grid_blocks(2, 4097) && plan_grid(3, 4097) == grid_blocks(3, 4097), "one grid");

// What a fold launch ran (ipls_agg_last_launch): tests assert that a case
// reaches the kernel shape it was written for.
ipls_launch_info launch_info(int kernel, int shape, int block, int r, int seqf, int map, int64_t grid, bool be_in,
                             bool be_out, int start) {
  return ipls_launch_info{kernel, shape, block, r, seqf, map, grid, be_in, be_out, start, 0};
}
ipls_launch_info launch_info(const ReducePlan& p, bool be_in, bool be_out, int start) {
  return launch_info(p.kernel, p.shape, p.block, p.r, p.seqf, p.map, p.grid, be_in, be_out, start);
}

// ---- kernel dispatch: k_reduce / k_round, from plan_reduce (reduce_plan.hpp) ----
// the template arguments of one wide fold, named as k_reduce and k_round name them
template <int G_, int R_, int MAP_, int BS_, int SEQF_>
struct Tiles {
  static constexpr int G = G_, R = R_, MAP = MAP_, BS = BS_, SEQF = SEQF_;
};
template <bool BE_IN, bool BE_OUT, int START, bool FIN = false>
ipls_launch_info launch_reduce_v(int64_t maxL, int n_parts, hipStream_t st, const unsigned long long* const* bufs,
                                 const PartDesc* parts, int k, int secure = 0, const double* cnts = nullptr) {
  constexpr int R = big_r(BE_IN, START), SEQF = big_seqf(BE_IN, START);
  constexpr int RM = mid_r(BE_IN, START), SEQFM = mid_seqf(BE_IN, START);
  const ReducePlan p = plan_reduce(BE_IN, START, FIN, maxL, n_parts);
  const dim3 grid((unsigned)p.grid);
  auto run = [&](auto t) {
    typedef decltype(t) T;
    if constexpr (FIN)
      hipLaunchKernelGGL((k_round<BE_IN, START, T::G, T::R, T::MAP, T::BS, T::SEQF>), grid, dim3(T::BS), 0, st, bufs,
                         parts, k, (int)p.tpp, n_parts, secure, cnts);
    else
      hipLaunchKernelGGL((k_reduce<BE_IN, BE_OUT, START, T::G, T::R, true, T::MAP, T::BS, T::SEQF>), grid,
                         dim3(T::BS), 0, st, bufs, parts, k, (int)p.tpp, n_parts);
  };
  // exactly the (shape, map) pairs plan_reduce gives
  switch (p.shape) {
    case IPLS_SHAPE_HALF:
      if constexpr (half_allowed(START, FIN)) {
        if (p.map == 3) run(Tiles<kBigG, kHalfR, 3, kHalfBS, 0>{});
        else run(Tiles<kBigG, kHalfR, kBigMap, kHalfBS, 0>{});
      }
      break;
    case IPLS_SHAPE_BIG:
      if (p.map == 3) run(Tiles<kBigG, R, 3, kBigBS, SEQF>{});
      else if (p.map == 2) run(Tiles<kBigG, R, 2, kBigBS, SEQF>{});
      else run(Tiles<kBigG, R, kBigMap, kBigBS, SEQF>{});
      break;
    case IPLS_SHAPE_MID:
      if (p.map == 3) run(Tiles<kBigG, RM, 3, kMidBS, SEQFM>{});
      else run(Tiles<kBigG, RM, kBigMap, kMidBS, SEQFM>{});
      break;
    default: run(Tiles<kSmallG, kSmallR, kSmallMap, kSmallBS, 0>{});
  }
  return launch_info(p, BE_IN, BE_OUT, START);
}

ipls_launch_info launch_reduce(bool be_in, bool be_out, int start, int64_t maxL, int n_parts, hipStream_t st,
                               const unsigned long long* const* bufs, const PartDesc* parts, int k) {
  return with_fold(be_in, be_out, start, [&](auto i, auto o, auto s) {
    return launch_reduce_v<decltype(i)::value, decltype(o)::value, decltype(s)::value>(maxL, n_parts, st, bufs, parts, k);
  });
}

// fused round: native-double Weights out, ZERO or ACCUM start (AGG is never
// FIRST-started).  A one-block pre-pass folds each partition's count slot
// (k + 2 scalar loads per partition) so that the wide kernel reads one value
// per block instead of a k-long chain of dependent loads.
ipls_launch_info launch_reduce_fin(bool be_in, int start, int secure, int64_t maxL, int n_parts, hipStream_t st,
                                   const unsigned long long* const* bufs, const PartDesc* parts, int k,
                                   double* cnts) {
  return with_bool(be_in, [&](auto bi) {
    return with_start_za(start, [&](auto s) {
      constexpr bool BI = decltype(bi)::value;
      constexpr int ST = decltype(s)::value;
      hipLaunchKernelGGL((k_round_counts<BI, ST>), dim3(n_parts), dim3(64), 0, st, bufs, parts, k, n_parts, cnts);
      return launch_reduce_v<BI, false, ST, true>(maxL, n_parts, st, bufs, parts, k, secure, cnts);
    });
  });
}

// k_reduce_scalar on plan_reduce_scalar's grid
void launch_reduce_scalar(bool be_in, bool be_out, int start, const ReducePlan& p, hipStream_t st,
                          const unsigned long long* const* bufs, const PartDesc* parts, int k) {
  with_fold(be_in, be_out, start, [&](auto bi, auto bo, auto s) {
    hipLaunchKernelGGL((k_reduce_scalar<decltype(bi)::value, decltype(bo)::value, decltype(s)::value>),
                       dim3((unsigned)p.grid), dim3(kBlock), 0, st, bufs, parts, k, (int)p.tpp, p.tile);
  });
}

// ---- kernel dispatch: k_reduce_narrow, from plan_reduce_narrow (reduce_plan.hpp) ----
// Element by element (!vec) the kernel has no map 3 and no prefetch.
template <class S>
ipls_launch_info launch_reduce_narrow(bool be_out, int start, bool vec, int64_t maxL, int n_parts, hipStream_t st,
                                      const typename S::elem* const* bufs, const PartDesc* parts, int k) {
  constexpr NarrowShape K = narrow_shape(sizeof(typename S::elem));
  const ReducePlan p = plan_reduce_narrow(sizeof(typename S::elem), false, vec, maxL, n_parts);
  const dim3 grid((unsigned)p.grid);
  with_bool(be_out, [&](auto bo) {
    with_start(start, [&](auto s) {
      auto run = [&](auto map, auto v) {
        constexpr bool V = decltype(v)::value;
        hipLaunchKernelGGL((k_reduce_narrow<S, decltype(bo)::value, decltype(s)::value, K.r, K.bs, decltype(map)::value,
                                            V, (V ? K.pf : 0), K.e>),
                           grid, dim3(K.bs), 0, st, bufs, parts, k, (int)p.tpp, n_parts);
      };
      if (!vec) run(Int<0>{}, std::false_type{});
      else if (p.map == 3) run(Int<3>{}, std::true_type{});
      else run(Int<0>{}, std::true_type{});
    });
  });
  return launch_info(p, false, be_out, start);
}

// ---- kernel dispatch: k_round_narrow (the fused round over DEV_F32 / DEV_F16 / DEV_BF16 buckets) ----
// The fold's shape (narrow_shape: 1024 lanes x 2 vectors of floats, x 4 of
// 16-bit elements, the next peer prefetched), every operand 16-B aligned; the
// count pre-pass first, as for k_round.  A: the averages' format (S when the
// round writes none).  ZERO or ACCUM start; partial last tiles first (map 3).
template <class S, class A>
ipls_launch_info launch_round_narrow(int start, int secure, int64_t maxL, int n_parts, hipStream_t st,
                                     const typename S::elem* const* bufs, const PartDesc* parts, int k,
                                     double* cnts) {
  constexpr NarrowShape K = narrow_shape(sizeof(typename S::elem));
  const ReducePlan p = plan_reduce_narrow(sizeof(typename S::elem), true, true, maxL, n_parts);
  with_start_za(start, [&](auto s) {
    constexpr int ST = decltype(s)::value;
    hipLaunchKernelGGL((k_round_counts_narrow<S, ST>), dim3(n_parts), dim3(64), 0, st, bufs, parts, k, n_parts, cnts);
    hipLaunchKernelGGL((k_round_narrow<S, A, ST, K.r, K.bs, K.pf>), dim3((unsigned)p.grid), dim3(K.bs), 0, st, bufs,
                       parts, k, (int)p.tpp, n_parts, p.map, secure, (const double*)cnts);
  });
  return launch_info(p, false, false, start);
}

// Core of accumulate / reduce_batch: all pointers device-resident.  The
// destination is the handle's `target` accumulators, or -- when ext_dst is
// given -- one caller buffer per partition (doubles or, be_out, BE bytes).
// fused round (fin != nullptr): fold into AGG's values and write
// W = fold + REP to Weights, plus the averages at fin->avg (if set); AGG and
// REP end logically zero.  Callers guarantee 16-B aligned buckets.
struct FinOut {
  unsigned long long* avg;   // averages of p_first.. at flat_off[p] - flat_off[p_first], or null
  Fmt fmt = kFmtF64;         // their format: doubles, or with trainer-format buckets a trainer format
};

// k_fold1_narrow's launch: 4 groups of 4 elements per lane in flight (k_fold1's
// R), and a grid of at most 2048 workgroups of 256 lanes, what 256 CUs hold at
// once at this kernel's register count; longer buckets take further trips.
constexpr int kFold1NarrowR = 4;
constexpr unsigned kFold1NarrowGrid = 2048;

// host_src: the bucket is pinned host memory read over PCIe (zero copy); the
// single-bucket fold then runs on 128 workgroups, which measured 1-2.5 GB/s
// above 256..4096 (tools/h2d_bench.hip, profiles/r01/h2d_bench_fold1.txt).
int reduce_dev(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, Fmt fmt_in,
               int start_mode, int target, void* const* ext_dst = nullptr, bool be_out = false,
               const FinOut* fin = nullptr, bool host_src = false, const int64_t* lens = nullptr,
               bool arrival = false) {
  // arrival: one trainer-format bucket of a per-arrival caller (accumulate, the
  // chunked fold) takes k_fold1_narrow; reduce_batch never sets it and keeps
  // k_reduce_narrow at one partition and one bucket.
  // fmt_in: what the buckets hold.  The trainer formats (floats, halves,
  // bfloat16s) are aligned to their element size; with fin they take
  // k_round_narrow, the averages (if any) in a trainer format too.
  const bool be_in = fmt_in == kFmtBE, tr_in = fmt_trainer(fmt_in);
  // lens: lengths of caller destinations that are not this engine's
  // partitions (ext_dst only, e.g. a replica slot's partial sums)
  auto len_of = [&](int q) -> int64_t { return lens ? lens[q] : h->len[p_first + q]; };
  auto dst_of = [&](int q) -> unsigned long long* {
    if (fin) return (unsigned long long*)(h->arena + h->w_off[p_first + q]);
    return ext_dst ? (unsigned long long*)ext_dst[q]
                   : (unsigned long long*)(h->arena + target_off(h, p_first + q, target));
  };
  if (k <= 0 && !fin) {
    if (start_mode == IPLS_START_ZERO) {
      for (int q = 0; q < n_parts; ++q) {
        uint8_t* f = ext_dst ? nullptr : zero_flag(h, p_first + q, target);
        if (f) *f = 1;
        else HIP_TRY(h, hipMemsetAsync(dst_of(q), 0, (size_t)len_of(q) * 8, h->stream));
      }
    }
    return IPLS_OK;  // ACCUM / FIRST with no bucket: nothing to fold
  }
  // Resolve start mode per the logically-zero flags: an ACCUM into a +0.0
  // accumulator is exactly a ZERO-start fold.
  int start = start_mode;
  if (start_mode == IPLS_START_ACCUM && !ext_dst) {
    int nz = 0;
    for (int q = 0; q < n_parts; ++q) {
      uint8_t* f = zero_flag(h, p_first + q, target);
      nz += (f && *f) ? 1 : 0;
    }
    if (nz == n_parts) start = IPLS_START_ZERO;
    else if (nz) {
      for (int q = 0; q < n_parts; ++q) {
        int rc = materialize(h, p_first + q, target);
        if (rc) return rc;
      }
    }
  }
  // one bucket into one partition (every per-arrival fold): pointers go as
  // kernel arguments, no table upload
  if (!fin && !tr_in && n_parts == 1 && k == 1 && bufs[0]) {
    unsigned long long* d0 = dst_of(0);
    const int64_t L = len_of(0);
    if (d0 && !((uintptr_t)bufs[0] & 15) && !((uintptr_t)d0 & 15) && L > 0) {
      const auto* s0 = (const unsigned long long*)bufs[0];
      const unsigned blocks =
          std::max(1u, std::min<unsigned>(blocks_for((L >> 1), kBlock * 4), host_src ? 128u : 4096u));
      with_fold(be_in, be_out, start, [&](auto bi, auto bo, auto s) {
        hipLaunchKernelGGL((k_fold1<decltype(bi)::value, decltype(bo)::value, decltype(s)::value>), dim3(blocks),
                           dim3(kBlock), 0, h->stream, d0, s0, L);
      });
      HIP_TRY(h, hipGetLastError());
      h->last_launch = launch_info(IPLS_KERNEL_FOLD1, 0, kBlock, 4, 0, 0, blocks, be_in, be_out, start);
      if (!ext_dst)
        if (uint8_t* f = zero_flag(h, p_first, target)) *f = 0;
      return IPLS_OK;
    }
  }
  // the same for one arrival of a trainer format (k_fold1_narrow): the source
  // aligned to the lane's load (16 B of floats, 8 B of 16-bit elements), the
  // target to 16 B; any other alignment keeps the table route below
  if (!fin && tr_in && arrival && !be_out && start != IPLS_START_FIRST && n_parts == 1 && k == 1 && bufs[0]) {
    unsigned long long* d0 = dst_of(0);
    const int64_t L = len_of(0);
    if (d0 && !((uintptr_t)bufs[0] & (uintptr_t)(4 * fmt_size(fmt_in) - 1)) && !((uintptr_t)d0 & 15) && L > 0) {
      const unsigned blocks = std::max(1u, std::min<unsigned>(blocks_for(L >> 2, kBlock * kFold1NarrowR), kFold1NarrowGrid));
      with_narrow(fmt_in, [&](auto s) {
        typedef decltype(s) S;
        const auto* s0 = (const typename S::elem*)bufs[0];
        with_start_za(start, [&](auto st) {   // never FIRST (the guard above), never BE out
          hipLaunchKernelGGL((k_fold1_narrow<S, decltype(st)::value, kFold1NarrowR>), dim3(blocks), dim3(kBlock), 0,
                             h->stream, d0, s0, L);
        });
      });
      HIP_TRY(h, hipGetLastError());
      h->last_launch = launch_info(fmt_size(fmt_in) == 4 ? IPLS_KERNEL_FOLD1_F32 : IPLS_KERNEL_FOLD1_H16, 0, kBlock,
                                   kFold1NarrowR, 1, 0, blocks, false, false, start);
      if (!ext_dst)
        if (uint8_t* f = zero_flag(h, p_first, target)) *f = 0;
      return IPLS_OK;
    }
  }
  bool aligned16 = true;
  int64_t maxL = 0;
  for (int q = 0; q < n_parts; ++q) maxL = std::max(maxL, len_of(q));
  for (int64_t i = 0; i < (int64_t)n_parts * k; ++i) {
    if (!bufs[i]) return fail(h, IPLS_E_INVAL, "bucket pointer %lld is NULL", (long long)i);
    uintptr_t a = (uintptr_t)bufs[i];
    if (a & (uintptr_t)(fmt_size(fmt_in) - 1))
      return fail(h, IPLS_E_INVAL, "bucket %lld not %d-byte aligned", (long long)i, fmt_size(fmt_in));
    if (a & 15) aligned16 = false;
  }
  // table = [PartDesc x n_parts][ptr x n_parts*k]
  const size_t desc_bytes = sizeof(PartDesc) * n_parts;
  const size_t bytes = desc_bytes + sizeof(void*) * (size_t)n_parts * k;
  std::vector<unsigned char> tbl(bytes);
  PartDesc* pd = (PartDesc*)tbl.data();
  for (int q = 0; q < n_parts; ++q) {
    const int p = p_first + q;
    pd[q].len = len_of(q);
    pd[q].dst = dst_of(q);
    pd[q].init = pd[q].dst;
    pd[q].rep = nullptr;
    pd[q].avg = nullptr;
    if (fin) {
      pd[q].init = (const unsigned long long*)(h->arena + h->agg_off[p]);
      if (!h->rep_zero[p]) pd[q].rep = (const unsigned long long*)(h->arena + h->rep_off[p]);
      if (fin->avg)   // a byte pointer: the averages' elements are doubles or of a trainer format
        pd[q].avg = (unsigned long long*)((char*)fin->avg +
                                          (h->flat_off[p] - h->flat_off[p_first]) * (int64_t)fmt_size(fin->fmt));
    }
    if (!pd[q].dst) return fail(h, IPLS_E_INVAL, "destination %d is NULL", q);
    if ((uintptr_t)pd[q].dst & 7) return fail(h, IPLS_E_INVAL, "destination %d not 8-byte aligned", q);
    if ((uintptr_t)pd[q].dst & 15) aligned16 = false;
  }
  if (k > 0) std::memcpy(tbl.data() + desc_bytes, bufs, sizeof(void*) * (size_t)n_parts * k);
  void* dtab = nullptr;
  int rc = upload_table(h, tbl.data(), bytes, &dtab);
  if (rc) return rc;
  const PartDesc* dparts = (const PartDesc*)dtab;
  auto dbufs = (const unsigned long long* const*)((char*)dtab + desc_bytes);
  if (fin) {
    if (!aligned16 || (fin->avg && tr_in != fmt_trainer(fin->fmt)))
      return fail(h, IPLS_E_INVAL, "fused round needs 16-B aligned buckets and averages of the buckets' family");
    if (tr_in) {
      h->last_launch = with_narrow(fmt_in, [&](auto s) {
        typedef decltype(s) S;
        return with_narrow(fin->avg ? fin->fmt : fmt_in, [&](auto a) {
          return launch_round_narrow<S, decltype(a)>(start, h->secure, maxL, n_parts, h->stream,
                                                     (const typename S::elem* const*)dbufs, dparts, k, h->d_cnt);
        });
      });
    } else {
      h->last_launch = launch_reduce_fin(be_in, start, h->secure, maxL, n_parts, h->stream, dbufs, dparts, k, h->d_cnt);
    }
    HIP_TRY(h, hipGetLastError());
    for (int q = p_first; q < p_first + n_parts; ++q) h->agg_zero[q] = h->rep_zero[q] = 1;
    return IPLS_OK;
  }
  if (tr_in) {
    h->last_launch = with_narrow(fmt_in, [&](auto s) {
      typedef decltype(s) S;
      return launch_reduce_narrow<S>(be_out, start, aligned16, maxL, n_parts, h->stream,
                                     (const typename S::elem* const*)dbufs, dparts, k);
    });
  } else if (aligned16) {
    h->last_launch = launch_reduce(be_in, be_out, start, maxL, n_parts, h->stream, dbufs, dparts, k);
  } else {
    const ReducePlan p = plan_reduce_scalar(maxL, n_parts);
    launch_reduce_scalar(be_in, be_out, start, p, h->stream, dbufs, dparts, k);
    h->last_launch = launch_info(p, be_in, be_out, start);
  }
  HIP_TRY(h, hipGetLastError());
  if (!ext_dst)
    for (int q = 0; q < n_parts; ++q) {
      uint8_t* f = zero_flag(h, p_first + q, target);
      if (f) *f = 0;
    }
  return IPLS_OK;
}

int partition_geometry(const ipls_agg_cfg* c, std::vector<int64_t>& len, std::vector<int64_t>& off,
                       int64_t& chunk, std::string& why) {
  const int P = c->n_partitions;
  len.resize(P);
  off.resize(P);
  if (c->model_size > 0) {
    chunk = ref_chunk(c->model_size, P);
    for (int i = 0; i < P; ++i) {
      // IPLS.java:1023-1028 / 1862-1872
      int64_t L = ((int64_t)(i + 1) * chunk > c->model_size) ? c->model_size - (int64_t)i * chunk + 1
                                                             : chunk + 1;
      if (L < 1) {
        // L < 0: new double[L] throws NegativeArraySizeException (IPLS.java:1863);
        // L == 0: the count-slot store overruns the array (IPLS.java:1894, 1033).
        char b[160];
        snprintf(b, sizeof b, "partition %d length %lld < 1 (%s)", i, (long long)L,
                 L < 0 ? "NegativeArraySizeException, IPLS.java:1863"
                       : "ArrayIndexOutOfBoundsException, IPLS.java:1894");
        why = b;
        return L < 0 ? IPLS_E_NEGSIZE : IPLS_E_RANGE;
      }
      len[i] = L;
      off[i] = (int64_t)i * chunk;
    }
  } else {
    if (c->bucket_len < 1) {
      why = "bucket_len must be >= 1 when model_size == 0";
      return IPLS_E_INVAL;
    }
    chunk = c->bucket_len - 1;
    for (int i = 0; i < P; ++i) {
      len[i] = c->bucket_len;
      off[i] = (int64_t)i * chunk;
    }
  }
  return IPLS_OK;
}

}  // namespace

// ===========================================================================
// Engine entry points (engine.hpp).  The handle-free ipls_* utilities further
// down keep the C linkage of their declarations in include/ipls_agg.h.
// ===========================================================================
const char* dev_last_error(const ipls_dev* h) {
  if (h) return h->err.c_str();
  return g_tls_err.c_str();
}

// The front's own failures land in the same per-thread message that
// ipls_agg_last_error(NULL) reads.
void dev_set_thread_error(const char* msg) { g_tls_err = msg ? msg : ""; }

namespace {
thread_local int t_dev = -1;   // this thread's current device inside a C-ABI call, -1 = unknown
}
hipError_t dev_use(int device) {
  if (t_dev == device) return hipSuccess;
  const hipError_t e = hipSetDevice(device);
  t_dev = e == hipSuccess ? device : -1;
  return e;
}
void dev_track(int device) { t_dev = device; }
int dev_tracked() { return t_dev; }

int dev_geometry(const ipls_agg_cfg* cfg, std::vector<int64_t>& len, std::vector<int64_t>& off, int64_t& chunk,
                 std::string& why) {
  return partition_geometry(cfg, len, off, chunk, why);
}

// One engine for the partitions [p_lo, p_hi) of the handle's geometry on
// `device` (the front has validated cfg and the device ordinal).  Partition
// q of the engine is partition p_lo + q of the handle; flat offsets stay the
// handle's (flat model coordinates), flat_base is the first one.
int dev_open(const ipls_agg_cfg* cfg, int device, int p_lo, int p_hi, ipls_dev** out) {
  if (!cfg || !out || p_lo < 0 || p_hi < p_lo || p_hi > cfg->n_partitions)
    return fail(nullptr, IPLS_E_INVAL, "bad engine range");
  *out = nullptr;
  ipls_dev* h = new (std::nothrow) ipls_dev();
  if (!h) return fail(nullptr, IPLS_E_NOMEM, "host allocation failed");
  std::string why;
  std::vector<int64_t> glen, goff;
  int rc = partition_geometry(cfg, glen, goff, h->chunk, why);
  if (rc) {
    delete h;
    return fail(nullptr, rc, "%s", why.c_str());
  }
  h->len.assign(glen.begin() + p_lo, glen.begin() + p_hi);
  h->flat_off.assign(goff.begin() + p_lo, goff.begin() + p_hi);
  h->p_lo = p_lo;
  // an empty engine (p_hi == p_lo) owns no partition: a replica slot only
  h->flat_base = p_hi > p_lo ? h->flat_off[0] : 0;
  h->P = p_hi - p_lo;
  h->device = device;
  h->model_size = cfg->model_size;
  h->secure = cfg->secure;
  h->agg_off.resize(h->P);
  h->rep_off.resize(h->P);
  h->w_off.resize(h->P);
  h->fut_off.resize(h->P);
  h->agg_zero.assign(h->P, 1);
  h->rep_zero.assign(h->P, 1);
  h->fut_zero.assign(h->P, 1);
  int64_t cur = 0;
  for (int p = 0; p < h->P; ++p) {
    h->max_len = std::max(h->max_len, h->len[p]);
    h->flat_total = std::max(h->flat_total, h->flat_off[p] + h->len[p] - 1);
    h->agg_off[p] = cur; cur = align_up(cur + h->len[p], kAlignElems);
    h->rep_off[p] = cur; cur = align_up(cur + h->len[p], kAlignElems);
    h->w_off[p] = cur;   cur = align_up(cur + h->len[p], kAlignElems);
    h->fut_off[p] = cur; cur = align_up(cur + h->len[p], kAlignElems);
  }
  h->arena_elems = cur;
  // new double[(int)_MODEL_SIZE/_PARTITIONS + 2] (Updater.java:162)
  h->gbuf_len = h->model_size > 0 ? (int64_t)((int32_t)h->model_size / cfg->n_partitions) + 2 : cfg->bucket_len;
  auto cleanup = [&](int code) {
    (void)hipGetLastError();   // the failed call's error must not reach a later launch check
    dev_close(h);
    return code;
  };
  if (dev_use(h->device) != hipSuccess) return cleanup(fail(nullptr, IPLS_E_DEVICE, "dev_use(%d) failed", h->device));
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(nullptr, IPLS_E_DEVICE, "hipStreamCreate failed"));
  if (h->arena_elems > 0 && hipMalloc(&h->arena, (size_t)h->arena_elems * 8) != hipSuccess) {
    (void)hipGetLastError();   // not sticky: the next launch check must not see it
    h->arena = nullptr;
    return cleanup(fail(nullptr, IPLS_E_NOMEM, "hipMalloc of %lld-byte arena failed", (long long)h->arena_elems * 8));
  }
  if (hipMalloc(&h->d_sum, 64) != hipSuccess) return cleanup(fail(nullptr, IPLS_E_NOMEM, "hipMalloc failed"));
  if (hipMalloc(&h->d_cnt, sizeof(double) * std::max(1, h->P)) != hipSuccess)
    return cleanup(fail(nullptr, IPLS_E_NOMEM, "hipMalloc failed"));
  // InitializeWeights(): new double[] -> all zero (IPLS.java:1860-1878).
  if ((h->arena && hipMemsetAsync(h->arena, 0, (size_t)h->arena_elems * 8, h->stream) != hipSuccess) ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return cleanup(fail(nullptr, IPLS_E_DEVICE, "arena clear failed"));
  *out = h;
  return IPLS_OK;
}

int dev_close(ipls_dev* h) {
  if (!h) return IPLS_OK;
  dev_use(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (auto& s : h->ring) {
    if (s.host) hipHostFree(s.host);
    if (s.ev) hipEventDestroy(s.ev);
  }
  stg::destroy(h->stages);
  if (h->copy_ev) hipEventDestroy(h->copy_ev);
  for (hipStream_t cs : h->copy_stream)
    if (cs) {
      hipStreamSynchronize(cs);
      hipStreamDestroy(cs);
    }
  for (auto& sl : h->stage) {
    if (sl.d) hipFree(sl.d);
    if (sl.free_ev) hipEventDestroy(sl.free_ev);
  }
  if (h->ingest_ev) hipEventDestroy(h->ingest_ev);
  for (hipEvent_t e : h->msg_ev) hipEventDestroy(e);
  for (auto& b : h->batches) hipEventDestroy(b.ev);
  for (hipEvent_t e : h->ev_free) hipEventDestroy(e);
  for (void* d : h->d_table)
    if (d) hipFree(d);
  if (h->d_scratch) hipFree(h->d_scratch);
  if (h->d_sum) hipFree(h->d_sum);
  if (h->d_cnt) hipFree(h->d_cnt);
  if (h->d_gbuf) hipFree(h->d_gbuf);
  if (h->d_merge) hipFree(h->d_merge);
  for (auto& kv : h->other)
    if (kv.second.d) hipFree(kv.second.d);
  if (h->arena) hipFree(h->arena);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
  return IPLS_OK;
}

void* dev_stream(ipls_dev* h) { return h ? (void*)h->stream : nullptr; }

// sync and wait hold the handle's lock only to flush and to book-keep: the
// host waits with it released, so the Updater and daemon threads (or any
// other caller) keep queueing folds meanwhile.
int dev_sync(ipls_dev* h) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  std::unique_lock<std::mutex> lk(h->mu);
  if (int rc = flush_pending(h)) return rc;
  lk.unlock();
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    lk.lock();
    return fail(h, IPLS_E_DEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  }
  return IPLS_OK;
}

int dev_wait(ipls_dev* h, uint64_t ticket) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  std::unique_lock<std::mutex> lk(h->mu);
  if (ticket >= h->ticket_next) return fail(h, IPLS_E_INVAL, "ticket %llu was never issued", (unsigned long long)ticket);
  if (ticket <= h->ticket_done) return IPLS_OK;
  if (ticket > h->launched_upto)
    if (int rc = flush_pending(h)) return rc;
  // the first launch group that covers `ticket` (groups complete in order)
  hipEvent_t ev = nullptr;
  uint64_t covered = 0;
  for (const auto& b : h->batches)
    if (b.max_ticket >= ticket) {
      ev = b.ev;
      covered = b.max_ticket;
      break;
    }
  if (!ev) return IPLS_OK;   // already retired by another waiter
  lk.unlock();
  // If another thread retires and re-records this event meanwhile, the wait
  // only gets longer: the re-recorded work was queued after ours.
  const hipError_t e = hipEventSynchronize(ev);
  lk.lock();
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, IPLS_E_DEVICE, "hipEventSynchronize failed: %s", hipGetErrorString(e));
  }
  while (!h->batches.empty() && h->batches.front().max_ticket <= covered) {
    h->ev_free.push_back(h->batches.front().ev);
    h->batches.pop_front();
  }
  h->ticket_done = std::max(h->ticket_done, covered);
  return IPLS_OK;
}

int dev_flush(ipls_dev* h) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);   // launches the queued folds; does not wait for them
  return IPLS_OK;
}

int dev_set_coalesce(ipls_dev* h, int max_group) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  h->coalesce = std::max(1, max_group);
  return IPLS_OK;
}

namespace {

// Close the launches queued since the last batch: tickets up to ticket_next-1
// complete at the event recorded now.
int end_batch(ipls_dev* h) {
  hipEvent_t ev;
  if (!h->ev_free.empty()) {
    ev = h->ev_free.back();
    h->ev_free.pop_back();
  } else {
    HIP_TRY(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  HIP_TRY(h, hipEventRecord(ev, h->stream));
  h->batches.push_back({h->ticket_next - 1, ev});
  h->launched_upto = h->ticket_next - 1;
  while ((int)h->batches.size() > ipls_dev::kMaxBatches) {   // bound the events in flight
    const ipls_dev::Batch b = h->batches.front();
    HIP_TRY(h, hipEventSynchronize(b.ev));
    h->batches.pop_front();
    h->ev_free.push_back(b.ev);
    h->ticket_done = std::max(h->ticket_done, b.max_ticket);
  }
  return IPLS_OK;
}

// Fold every queued device arrival: runs of consecutive partitions of one
// target with the same queue length and byte order go as one launch (the
// batch kernel's table is [partition][peer]).
int flush_pending(ipls_dev* h) {
  if (h->pend_keys.empty()) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  int rc = IPLS_OK;
  std::vector<int>& keys = h->pend_keys;
  std::sort(keys.begin(), keys.end());   // (target, p) ascending
  std::vector<const void*> tab;
  for (size_t i = 0; i < keys.size() && !rc;) {
    const int key = keys[i], target = key / h->P, p0 = key % h->P;
    const ipls_dev::Pending& q0 = h->pend[key];
    const size_t k = q0.bufs.size();
    size_t j = i + 1;
    int n = 1;
    while (j < keys.size() && keys[j] == key + n && keys[j] / h->P == target && h->pend[keys[j]].bufs.size() == k &&
           h->pend[keys[j]].fmt == q0.fmt) {
      ++n;
      ++j;
    }
    tab.clear();
    for (size_t t = i; t < j; ++t) tab.insert(tab.end(), h->pend[keys[t]].bufs.begin(), h->pend[keys[t]].bufs.end());
    rc = reduce_dev(h, p0, n, tab.data(), (int)k, q0.fmt, IPLS_START_ACCUM, target);
    i = j;
  }
  for (int key : keys) h->pend[key].bufs.clear();   // keeps the capacity
  keys.clear();
  h->pending_n = 0;
  if (rc) return rc;
  return end_batch(h);
}

}  // namespace

int dev_reduce_batch(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k,
                          int src_kind, int start_mode, int target) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_parts <= 0 || p_first < 0 || p_first + n_parts > h->P)
    return fail(h, IPLS_E_RANGE, "partitions [%d,%d) out of range [0,%d)", p_first, p_first + n_parts, h->P);
  if (src_kind != IPLS_DEV_F64 && src_kind != IPLS_DEV_BE && !kind_trainer_dev(src_kind))
    return fail(h, IPLS_E_INVAL, "reduce_batch takes device buckets (DEV_F64/DEV_BE/DEV_F32/DEV_F16/DEV_BF16)");
  if (start_mode < IPLS_START_ACCUM || start_mode > IPLS_START_FIRST) return fail(h, IPLS_E_INVAL, "bad start mode");
  if (target_off(h, 0, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  if (k < 0 || (k > 0 && !bufs)) return fail(h, IPLS_E_INVAL, "bad bucket list");
  HIP_TRY(h, dev_use(h->device));
  return reduce_dev(h, p_first, n_parts, bufs, k, kind_fmt(src_kind), start_mode, target);
}

int dev_accumulate(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  // a null source is Gradient == null: the Updater loops do nothing (Updater.java:115)
  const int64_t L = h->len[p];
  op::Resolved v;
  if (op::resolve(op::kAccumulate, src, n, src_kind, L, &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  // a co-located trainer's float / half / bfloat16 bucket is widened in the fold (Model.java:423); from the
  // host 4 or 2 B per element cross PCIe
  const size_t bytes = (size_t)L * fmt_size(v.fmt);
  const void* dptr = v.ptr;
  if (v.host) {
    void* alias = nullptr;
    if (v.from == op::kRaw && !fmt_trainer(v.fmt) && op::zero_copy_arrival(v.ptr, bytes) && is_pinned_host(v.ptr, &alias) &&
        alias) {
      // Zero copy: the fold kernel reads the pinned bucket over PCIe (no
      // staging copy, no second pass).  The call returns once the kernel
      // is done with the caller's bytes.
      const void* bl[1] = {alias};
      if (int rc = reduce_dev(h, p, 1, bl, 1, v.fmt, IPLS_START_ACCUM, target, nullptr, false, nullptr, true)) return rc;
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      return IPLS_OK;
    }
    // (a container's payload is unaligned, a frame's starts at byte 14: staging realigns it)
    if (int rc = stage_bucket(h, v.ptr, bytes, &dptr)) return rc;
  }
  const void* bl[1] = {dptr};
  if (int rc = reduce_dev(h, p, 1, bl, 1, v.fmt, IPLS_START_ACCUM, target, nullptr, false, nullptr, false, nullptr,
                          /*arrival=*/true))
    return rc;
  return v.host ? bucket_slot_busy(h) : IPLS_OK;
}

int dev_accumulate_async(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind,
                              uint64_t* ticket) {
  if (!h || !ticket) return fail(h, IPLS_E_INVAL, "null argument");
  op::Resolved v;
  if (src && (op::kDev & op::bit(src_kind))) {
    // device bucket: queued, folded with the partition's other queued buckets
    // (a queue holds one format: a bucket of another one flushes first, so
    // call order is kept across F64, BE, F32, F16 and BF16 arrivals)
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_part(h, p)) return rc;
    if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
    if (op::resolve(op::kAccumulateAsync, src, n, src_kind, h->len[p], &v) != op::kTake) return not_taken(h, v.why);
    const Fmt fmt = v.fmt;
    // Weights and Weight_Address are one array (IPLS.java:1141): one queue
    const int qt = target == IPLS_TGT_WADDR ? IPLS_TGT_WEIGHTS : target;
    if (h->pend.empty()) h->pend.resize((size_t)5 * h->P);   // 5 targets (include/ipls_agg.h)
    ipls_dev::Pending& q = h->pend[(size_t)qt * h->P + p];
    if (!q.bufs.empty() && q.fmt != fmt)
      if (int rc = flush_pending(h)) return rc;
    if (q.bufs.empty()) h->pend_keys.push_back(qt * h->P + p);
    q.fmt = fmt;
    q.bufs.push_back(src);
    ++h->pending_n;
    *ticket = h->ticket_next++;
    // flush when the queues average `coalesce` buckets (arrivals spread over
    // partitions flush as one rectangular launch), or one queue holds twice that
    if ((int)q.bufs.size() >= 2 * h->coalesce || h->pending_n >= h->coalesce * (int)h->pend_keys.size())
      return flush_pending(h);
    return IPLS_OK;
  }
  void* alias = nullptr;
  const bool host = op::kHostD & op::bit(src_kind);
  if (!src || !host || !op::zero_copy_queued(src) || !is_pinned_host(src, &alias) || !alias) {
    // not a pinned host bucket: the synchronous path, already complete on return
    int rc = dev_accumulate(h, p, target, src, n, src_kind);
    std::lock_guard<std::mutex> lk(h->mu);
    *ticket = h->ticket_done;
    return rc;
  }
  IPLS_LOCK(h);   // earlier queued device buckets fold first
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  if (op::resolve(op::kAccumulateAsync, src, n, src_kind, h->len[p], &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  const void* bl[1] = {alias};   // zero copy: the kernel reads the pinned bucket over PCIe
  if (int rc = reduce_dev(h, p, 1, bl, 1, v.fmt, IPLS_START_ACCUM, target, nullptr, false, nullptr, true)) return rc;
  *ticket = h->ticket_next++;
  return end_batch(h);
}

// One range of one arrival: src[0..n) folded into target[off..off+n) of
// partition p, zero copy from pinned host memory, asynchronous.  The JNI
// shim's heap-array natives copy a Java double[] into pinned staging chunk by
// chunk and fold each chunk as soon as it has landed, so the copy of the next
// chunk overlaps the fold of this one.  Whatever the split, every element of
// the bucket is added exactly once, in call order: the bits of the
// whole-bucket fold (Updater.java:115-117).
int dev_accumulate_range(ipls_dev* h, int p, int target, const void* src, int64_t off, int64_t n, int src_kind,
                         uint64_t* ticket) {
  if (!h || !ticket || !src) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);   // earlier queued device buckets fold first
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  const int64_t L = h->len[p];
  op::Resolved v;
  if (op::resolve(op::kAccumulateRange, src, n, src_kind, L, &v) != op::kTake) return not_taken(h, v.why);
  if (off < 0 || n < 0 || off > L || n > L - off)
    return fail(h, IPLS_E_RANGE, "range [%lld, %lld) outside partition %d of length %lld", (long long)off,
                (long long)(off + n), p, (long long)L);
  if ((off & 1) || !op::zero_copy_queued(src))
    return fail(h, IPLS_E_INVAL, "a ranged fold needs an even start and 16-B aligned bytes");
  void* alias = nullptr;
  if (!is_pinned_host(src, &alias) || !alias)
    return fail(h, IPLS_E_INVAL, "a ranged fold reads pinned host memory (ipls_host_alloc)");
  if (n == 0) {
    *ticket = h->ticket_done;
    return IPLS_OK;
  }
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, target)) return rc;   // a logically-zero target becomes real zeros first
  unsigned long long* d0 = (unsigned long long*)(h->arena + target_off(h, p, target)) + off;
  const auto* s0 = (const unsigned long long*)alias;
  const unsigned blocks = std::max(1u, std::min<unsigned>(blocks_for(n >> 1, kBlock * 4), 128u));
  const bool be = v.fmt == kFmtBE;
  with_bool(be, [&](auto b) {
    hipLaunchKernelGGL((k_fold1<decltype(b)::value, false, kAccum>), dim3(blocks), dim3(kBlock), 0, h->stream, d0, s0, n);
  });
  HIP_TRY(h, hipGetLastError());
  h->last_launch = launch_info(IPLS_KERNEL_FOLD1, 0, kBlock, 4, 0, 0, blocks, be, false, IPLS_START_ACCUM);
  *ticket = h->ticket_next++;
  return end_batch(h);
}

// One arrival produced by the caller chunk by chunk, as one call (Updater's
// whole-bucket fold under PeerData.mtx, Updater.java:72-149, 115-117).
// Chunk k is filled by source() into a pinned slot of a stage of this call's
// own (stage.hpp) and sent to its device buffer while the source fills chunk
// k + 1 -- all with NO engine lock held, so a source that blocks (a socket
// recv) stalls only this call.  Once every chunk has landed, the lock is
// taken for the fold alone: one launch over the whole bucket (24 B per
// element).  So the arrival takes effect, as one unit, when its last chunk
// has landed -- the reference's order: Middleware's Deserialize reads the
// whole stream before UpdateModel takes PeerData.mtx (Middleware.java:224,
// 246).  A source that stops leaves the target untouched.
// The element format is a parameter: kFmtF64 / kFmtBE (the source
// writes 8 B per value) or a trainer format (4 or 2 B per value, the fold is
// k_fold1_narrow from the stage, 20 or 18 B per element); n, chunk and the
// source's offsets count elements in every format.
static int accumulate_chunked_fmt(ipls_dev* h, int p, int target, int64_t n, int src_kind, bool narrow, int64_t chunk,
                                  ipls_chunk_source source, void* ctx) {
  if (!h || !source) return fail_nl(h, IPLS_E_INVAL, "null argument");
  if (int rc = check_chunk(h, chunk, "values")) return rc;
  if (int rc = check_part_nl(h, p)) return rc;
  if (int rc = check_target_nl(h, target)) return rc;
  const int64_t L = h->len[p];
  op::Resolved v;   // the kind, and a short bucket before any source call (Updater.java:115)
  if (op::resolve(narrow ? op::kChunkedNarrow : op::kChunked, nullptr, n, src_kind, L, &v) != op::kTake)
    return fail_nl(h, v.why.code, "%s", v.why.text);
  const Fmt fmt = v.fmt;
  if (int rc = use_nl(h)) return rc;
  const int64_t c = std::min(chunk, L);
  const int64_t esz = fmt_size(fmt);
  ipls_stage* st = nullptr;
  if (int rc = stage_rc(h, stg::acquire(h->stages, (size_t)(L * esz), (size_t)(c * esz), &st))) return rc;
  int rc = stage_rc(h, stg::begin_in(st));
  for (int64_t k = 0, off = 0; off < L && !rc; ++k, off += c) {
    void* host = nullptr;
    if ((rc = stage_rc(h, stg::slot(st, k, &host)))) break;
    const int64_t len = std::min(c, L - off);
    if (source(ctx, host, off, len) != 0) {
      rc = fail_nl(h, IPLS_E_INVAL, "the chunk source stopped at offset %lld: nothing folded", (long long)off);
      break;
    }
    const int64_t slot_off = 0;
    rc = stage_rc(h, stg::push(st, k, &slot_off, &off, &len, 1, (size_t)esz));
  }
  if (!rc) rc = stage_rc(h, stg::landed(st));
  if (!rc) {
    std::lock_guard<std::mutex> lk(h->mu);
    rc = flush_pending(h);   // earlier queued device buckets fold first
    if (!rc) rc = stage_rc(h, stg::join(st, h->stream), true);
    const void* bl[1] = {st->d};
    if (!rc)
      rc = reduce_dev(h, p, 1, bl, 1, fmt, IPLS_START_ACCUM, target, nullptr, false, nullptr, false, nullptr,
                      /*arrival=*/true);
    stg::mark_read(st, h->stream);
  }
  dev_stage_release(h, st, rc);   // after a failure nothing, or not all, was folded: the copies are drained
  return rc;
}

int dev_accumulate_chunked(ipls_dev* h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                           ipls_chunk_source source, void* ctx) {
  return accumulate_chunked_fmt(h, p, target, n, src_kind, false, chunk, source, ctx);
}

// The same call for a trainer's float, half or bfloat16 bucket: 4 or 2 B per
// value through the source, the ring and PCIe, widened in the fold.
int dev_accumulate_chunked_narrow(ipls_dev* h, int p, int target, int64_t n, int src_kind, int64_t chunk,
                                  ipls_chunk_source source, void* ctx) {
  return accumulate_chunked_fmt(h, p, target, n, src_kind, true, chunk, source, ctx);
}

// ---- the whole-gradient streamed update (ipls_agg_update_gradient_chunked) ----
// The front (ipls_agg.cpp) plans the call (flat_plan.hpp) and drives one stage per involved shard through these
// (engine.hpp has the order).  Nothing here but the commit takes an engine lock.
constexpr size_t kFlatPad = 16;   // bytes before and after the staged segment (k_update_flat's shifted loads)

int dev_flat_begin(ipls_dev* h, Fmt fmt, int64_t seg, int64_t slot_elems, ipls_stage** st_out) {
  if (!h || !st_out || seg < 0 || slot_elems < 1) return fail_nl(h, IPLS_E_INVAL, "bad argument");
  *st_out = nullptr;
  if (int rc = use_nl(h)) return rc;
  const size_t esz = (size_t)fmt_size(fmt);
  ipls_stage* st = nullptr;
  if (int rc = stage_rc(h, stg::acquire(h->stages, (size_t)seg * esz + 2 * kFlatPad, (size_t)slot_elems * esz, &st)))
    return rc;
  const int rc = stage_rc(h, stg::begin_in(st));
  if (rc) dev_stage_release(h, st, rc);
  else *st_out = st;
  return rc;
}

int dev_flat_slot(ipls_dev* h, ipls_stage* st, int64_t k, void** host) {
  if (int rc = use_nl(h)) return rc;
  return stage_rc(h, stg::slot(st, k, host));
}

int dev_flat_copy(ipls_dev* h, ipls_stage* st, int64_t k, Fmt fmt, const int64_t* src, const int64_t* dst,
                  const int64_t* n, int n_copies) {
  if (n_copies <= 0) return IPLS_OK;
  if (int rc = use_nl(h)) return rc;
  return stage_rc(h, stg::push(st, k, src, dst, n, n_copies, (size_t)fmt_size(fmt), kFlatPad));
}

int dev_flat_landed(ipls_dev* h, ipls_stage* st) {
  if (int rc = use_nl(h)) return rc;
  return stage_rc(h, stg::landed(st));
}

template <class S, bool BE>
static void launch_update_flat(hipStream_t st, dim3 grid, const FlatJob* jobs, const void* src) {
  hipLaunchKernelGGL((k_update_flat<S, BE>), grid, dim3(kBlock), 0, st, jobs, (const typename S::elem*)src);
}

// The commit of one call: the engines' locks in the order given (the front
// passes ascending shard index), ALL held at once; under them every shard
// first folds its queued arrivals and makes its stream wait for the stage's
// copies, then every shard gets its launch(es); then the locks go.  So the
// gradient is one unit against every other call on those shards.  A failure
// before the first launch leaves every accumulator and flag as it was.  The
// stages are released (after a drain of their copy streams on failure).
int dev_flat_commit(const flat_commit* c, int n, Fmt fmt) {
  int rc = IPLS_OK;
  for (int s = 0; s < n; ++s) c[s].h->mu.lock();
  for (int s = 0; s < n && !rc; ++s) {
    ipls_dev* h = c[s].h;
    rc = stage_rc(h, stg::hip(dev_use(h->device), "dev_use"), true);
    if (!rc) rc = flush_pending(h);   // earlier queued device buckets fold first
    if (!rc) rc = stage_rc(h, stg::join(c[s].st, h->stream), true);
  }
  const int64_t tile = fmt_trainer(fmt) ? flat_tile<FmtF32>() : flat_tile<FmtD64>();
  for (int s = 0; s < n && !rc; ++s) {
    ipls_dev* h = c[s].h;
    rc = [&]() -> int {
      HIP_TRY(h, dev_use(h->device));
      const char* d_in = (const char*)c[s].st->d + kFlatPad;
      const flat_job* fj = c[s].jobs;
      for (int l = 0; l < c[s].n_launches; fj += c[s].launch_len[l], ++l) {
        for (int j0 = 0; j0 < c[s].launch_len[l]; j0 += 65535) {   // gridDim.y
          const int nj = std::min(65535, c[s].launch_len[l] - j0);
          std::vector<FlatJob> jobs((size_t)nj);
          int64_t maxL = 1;
          bool all_vec = true, all_zero = true;
          for (int j = 0; j < nj; ++j) {
            const flat_job& f = fj[j0 + j];
            if (f.q < 0 || f.q >= h->P || f.ncopy < 0 || f.ncopy > h->len[f.q] - 1 || f.lo < 0)
              return fail(h, IPLS_E_INVAL, "internal: bad whole-gradient job");
            FlatJob& o = jobs[(size_t)j];
            o.lo = f.lo;
            o.ncopy = f.ncopy;
            o.L = h->len[f.q];
            o.dst = (unsigned long long*)(h->arena + h->agg_off[f.q]);
            o.zero = h->agg_zero[f.q];
            maxL = std::max(maxL, o.L);
            all_vec = all_vec && f.ncopy >= tile;
            all_zero = all_zero && o.zero;
          }
          void* djobs = nullptr;
          if (int r = upload_table(h, jobs.data(), jobs.size() * sizeof(FlatJob), &djobs)) return r;
          const dim3 grid(blocks_for(maxL, tile), (unsigned)nj);
          if (fmt == kFmtF64) launch_update_flat<FmtD64, false>(h->stream, grid, (const FlatJob*)djobs, d_in);
          else if (fmt == kFmtBE) launch_update_flat<FmtD64, true>(h->stream, grid, (const FlatJob*)djobs, d_in);
          else
            with_narrow(fmt, [&](auto sfmt) {
              launch_update_flat<decltype(sfmt), false>(h->stream, grid, (const FlatJob*)djobs, d_in);
            });
          HIP_TRY(h, hipGetLastError());
          for (int j = 0; j < nj; ++j) h->agg_zero[fj[j0 + j].q] = 0;
          h->last_launch = launch_info(IPLS_KERNEL_UPDATE_FLAT, 0, kBlock, kFlatR, all_vec ? 1 : 0, 0,
                                       (int64_t)grid.x * grid.y, fmt == kFmtBE, false, all_zero ? kZero : kAccum);
        }
      }
      return IPLS_OK;
    }();
  }
  for (int s = 0; s < n; ++s) {
    if (dev_use(c[s].h->device) != hipSuccess) (void)hipGetLastError();   // (the record then fails: a synchronise)
    stg::mark_read(c[s].st, c[s].h->stream);
  }
  for (int s = n - 1; s >= 0; --s) c[s].h->mu.unlock();
  // after a failure a shard stream may not have waited for the copies: they are drained
  for (int s = 0; s < n; ++s) dev_stage_release(c[s].h, c[s].st, rc);
  return rc;
}

// A stage's published snapshot handed out through its ring (stg::ring), no engine lock held.
template <class Call>
static int stage_ring(ipls_dev* h, ipls_stage* st, const char* d, int64_t n, int64_t c, Call call) {
  stg::Status err;
  const int rc = stg::ring(st, d, n, c, &err, call);
  return err ? stage_rc(h, err) : rc;
}

// n values of the snapshot to the sink in chunks of c; `base` is added to the
// offsets the sink sees.
static int stage_deliver(ipls_dev* h, ipls_stage* st, int64_t n, int64_t c, int64_t base, ipls_chunk_sink sink, void* ctx,
                  const char* stopped_note) {
  return stage_ring(h, st, (const char*)st->d, 8 * n, 8 * c, [&](const void* host, int64_t off, int64_t len) {
    if (sink(ctx, (const double*)host, base + off / 8, len / 8) == 0) return IPLS_OK;
    return fail_nl(h, IPLS_E_INVAL, "the chunk sink stopped the transfer at offset %lld%s", (long long)(base + off / 8),
                   stopped_note);
  });
}

// The same for a byte sink: bytes [0, n) at d, seen by the sink at offsets base, base + 1, ...
static int stage_deliver_bytes(ipls_dev* h, ipls_stage* st, const char* d, int64_t n, int64_t c, int64_t base,
                               ipls_byte_sink sink, void* ctx) {
  return stage_ring(h, st, d, n, c, [&](const void* host, int64_t off, int64_t len) {
    if (sink(ctx, (const uint8_t*)host, base + off, len) == 0) return IPLS_OK;
    return fail_nl(h, IPLS_E_INVAL, "the byte sink stopped the transfer at offset %lld", (long long)(base + off));
  });
}

// The reverse: target[off..off+n) of partition p into pinned host memory,
// native or big-endian (putDouble order, as update_file writes it,
// MyIPFSClass.java:105-116), asynchronous.  The JNI shim's byte[] outputs
// copy chunk k into the Java array while chunk k+1 is still in flight.
int dev_read_range(ipls_dev* h, int p, int target, void* dst, int64_t off, int64_t n, int dst_kind, uint64_t* ticket) {
  if (!h || !ticket || !dst) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  if (dst_kind != IPLS_HOST_F64 && dst_kind != IPLS_HOST_BE)
    return fail(h, IPLS_E_INVAL, "a ranged read writes pinned host memory (HOST_F64 / HOST_BE), not kind %d", dst_kind);
  const int64_t L = h->len[p];
  if (off < 0 || n < 0 || off > L || n > L - off)
    return fail(h, IPLS_E_RANGE, "range [%lld, %lld) outside partition %d of length %lld", (long long)off,
                (long long)(off + n), p, (long long)L);
  void* alias = nullptr;
  if (!is_pinned_host(dst, &alias) || !alias)
    return fail(h, IPLS_E_INVAL, "a ranged read writes pinned host memory (ipls_host_alloc)");
  if (n == 0) {
    *ticket = h->ticket_done;
    return IPLS_OK;
  }
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, target)) return rc;
  const unsigned long long* src = (const unsigned long long*)(h->arena + target_off(h, p, target)) + off;
  if (dst_kind == IPLS_HOST_BE) {
    // byte-swapped into the same offsets of the device scratch, then copied
    if (int rc = ensure_scratch(h, (size_t)L * 8)) return rc;
    unsigned long long* sc = (unsigned long long*)h->d_scratch + off;
    launch_bswap(h->stream, src, sc, n);
    HIP_TRY(h, hipGetLastError());
    src = sc;
  }
  HIP_TRY(h, hipMemcpyAsync(dst, src, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  *ticket = h->ticket_next++;
  return end_batch(h);
}

// GetParameters(hash, Gradient_Buff) (MyIPFSClass.java:444-455) into the
// engine's Gradient_Buff (Updater.java:162, zeroed once, Updater.java:165-167):
// arr[i] = getDouble() for i < data.length/8; past arr.length it throws after
// the in-range stores (IPLS_E_RANGE, buffer already overwritten).  Entries
// beyond the file keep the previous request's values.  *zero_copy: the kernel
// reads the caller's pinned bytes (wait before returning to the caller).
static int gbuf_load(ipls_dev* h, const void* bytes, int64_t n_bytes, bool* zero_copy) {
  const int64_t G = h->gbuf_len;
  *zero_copy = false;
  op::Resolved v;   // "bad byte buffer"
  if (op::resolve(op::kUpdateIndirect, bytes, n_bytes, IPLS_HOST_BE, G, &v) != op::kTake) return not_taken(h, v.why);
  if (!h->d_gbuf) {
    HIP_TRY(h, hipMalloc(&h->d_gbuf, (size_t)std::max<int64_t>(G, 1) * 8));
    HIP_TRY(h, hipMemsetAsync(h->d_gbuf, 0, (size_t)std::max<int64_t>(G, 1) * 8, h->stream));
  }
  const int64_t nd = v.n, nw = std::min(nd, G);
  if (nw > 0) {
    const void* dsrc = nullptr;
    void* alias = nullptr;
    if (op::zero_copy_arrival(bytes, (size_t)nw * 8) && is_pinned_host(bytes, &alias) && alias) {
      dsrc = alias;
      *zero_copy = true;
    } else {
      // double-buffered like the per-arrival buckets (stage_bucket)
      if (int rc = stage_bucket(h, bytes, (size_t)nw * 8, &dsrc)) return rc;
    }
    launch_bswap(h->stream, (const unsigned long long*)dsrc, h->d_gbuf, nw);
    HIP_TRY(h, hipGetLastError());
    if (!*zero_copy)
      if (int rc = bucket_slot_busy(h)) return rc;
  }
  if (nd > G) {
    if (*zero_copy) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return fail(h, IPLS_E_RANGE, "GetParameters: %lld doubles > Gradient_Buff length %lld "
                "(ArrayIndexOutOfBoundsException, MyIPFSClass.java:451)", (long long)nd, (long long)G);
  }
  return IPLS_OK;
}

int dev_update_indirect(ipls_dev* h, int p, int target, const void* bytes, int64_t n_bytes) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  HIP_TRY(h, dev_use(h->device));
  const int64_t G = h->gbuf_len;
  bool zero_copy = false;
  if (int rc = gbuf_load(h, bytes, n_bytes, &zero_copy)) return rc;
  // _Update(Gradient_Buff, ...): target[p][i] += Gradient_Buff[i], i < L_p
  if (h->len[p] > G)
    return fail(h, IPLS_E_RANGE, "partition length %lld > Gradient_Buff length %lld", (long long)h->len[p],
                (long long)G);
  const void* bl[1] = {h->d_gbuf};
  if (int rc = reduce_dev(h, p, 1, bl, 1, kFmtF64, IPLS_START_ACCUM, target)) return rc;
  if (zero_copy) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

// The Gradient_Buff load alone, for a request whose partition lives in
// another engine (the handle keeps ONE Gradient_Buff, as the reference has
// one Updater thread): *gbuf / *glen describe the device buffer afterwards;
// the caller orders the fold after this engine's stream.
int dev_gbuf_load(ipls_dev* h, const void* bytes, int64_t n_bytes, const void** gbuf, int64_t* glen) {
  if (!h || !gbuf || !glen) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  HIP_TRY(h, dev_use(h->device));
  bool zero_copy = false;
  if (int rc = gbuf_load(h, bytes, n_bytes, &zero_copy)) return rc;
  if (zero_copy) HIP_TRY(h, hipStreamSynchronize(h->stream));
  *gbuf = h->d_gbuf;
  *glen = h->gbuf_len;
  return IPLS_OK;
}

int dev_reset(ipls_dev* h, int p) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (p == IPLS_ALL_PARTITIONS) {
    for (int q = 0; q < h->P; ++q) h->agg_zero[q] = h->rep_zero[q] = 1;
    return IPLS_OK;
  }
  if (int rc = check_part(h, p)) return rc;
  h->agg_zero[p] = h->rep_zero[p] = 1;
  return IPLS_OK;
}

int dev_promote_future(ipls_dev* h, const int32_t* parts, int n_parts) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_parts < 0 || (n_parts > 0 && !parts)) return fail(h, IPLS_E_INVAL, "bad partition list");
  for (int i = 0; i < n_parts; ++i)
    if (int rc = check_part(h, parts[i])) return rc;
  for (int i = 0; i < n_parts; ++i) {
    const int p = parts[i];
    // AGG[p][j] = FUTURE[p].get(j); FUTURE[p].set(j, 0.0)   (IPLS.java:1558-1561)
    std::swap(h->agg_off[p], h->fut_off[p]);
    h->agg_zero[p] = h->fut_zero[p];
    h->fut_zero[p] = 1;
  }
  return IPLS_OK;
}

int dev_device_ptr(ipls_dev* h, int p, int target, void** ptr) {
  if (!h || !ptr) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, target)) return rc;
  *ptr = h->arena + target_off(h, p, target);
  return IPLS_OK;
}

int dev_read(ipls_dev* h, int p, int target, void* dst, int64_t n, int dst_kind) {
  if (!h || !dst) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  const int64_t L = h->len[p];
  if (n < L) return fail(h, IPLS_E_RANGE, "output of %lld < partition length %lld", (long long)n, (long long)L);
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, target)) return rc;
  const double* srcd = h->arena + target_off(h, p, target);
  switch (dst_kind) {
    case IPLS_HOST_F64:
      return d2h(h, dst, srcd, (size_t)L * 8);
    case IPLS_DEV_F64:
      HIP_TRY(h, hipMemcpyAsync(dst, srcd, (size_t)L * 8, hipMemcpyDeviceToDevice, h->stream));
      return IPLS_OK;
    case IPLS_DEV_BE:
      launch_bswap(h->stream, (const unsigned long long*)srcd, (unsigned long long*)dst, L);
      HIP_TRY(h, hipGetLastError());
      return IPLS_OK;
    case IPLS_HOST_BE:
      return be_to_host(h, dst, srcd, L);
    default:
      return fail(h, IPLS_E_INVAL, "bad dst_kind %d", dst_kind);
  }
}

int dev_checksum(ipls_dev* h, int p, int target, uint64_t* out) {
  if (!h || !out) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, target)) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_sum, 0, 8, h->stream));
  const int64_t L = h->len[p];
  hipLaunchKernelGGL(k_checksum<false>, dim3(std::max(1u, std::min<unsigned>(blocks_for(L, kBlock * 8), 2048))),
                     dim3(kBlock), 0, h->stream,
                     (const unsigned long long*)(h->arena + target_off(h, p, target)), L, h->d_sum);
  HIP_TRY(h, hipGetLastError());
  unsigned long long v = 0;
  if (int rc = d2h(h, &v, h->d_sum, 8)) return rc;
  *out = v;
  return IPLS_OK;
}

// AggregatePartition's W = AGG + REP for partitions [p0, p0+np) (IPLS.java:1256-1269).
static int finalize_range(ipls_dev* h, int p0, int np) {
  // AGG logically zero but present as an operand -> make it physical.
  bool rep_zero_all = true;
  for (int q = p0; q < p0 + np; ++q) {
    if (int rc = materialize(h, q, IPLS_TGT_AGG)) return rc;
    rep_zero_all = rep_zero_all && h->rep_zero[q];
  }
  if (!rep_zero_all)
    for (int q = p0; q < p0 + np; ++q)
      if (int rc = materialize(h, q, IPLS_TGT_REP)) return rc;
  std::vector<FinDesc> fd(np);
  int64_t maxL = 0;
  for (int q = 0; q < np; ++q) {
    fd[q] = FinDesc{h->len[p0 + q], h->agg_off[p0 + q], h->rep_off[p0 + q], h->w_off[p0 + q]};
    maxL = std::max(maxL, fd[q].len);
  }
  void* dtab = nullptr;
  if (int rc = upload_table(h, fd.data(), fd.size() * sizeof(FinDesc), &dtab)) return rc;
  const int64_t tile = kFinTile;
  const int tpp = (int)((maxL + tile - 1) / tile);
  // AGG/REP are left in place and flagged logically zero (IPLS.java:1268-1269
  // zeroes them; the next fold starts from +0.0 without reading them).
  if (rep_zero_all)
    hipLaunchKernelGGL((k_finalize<true, false>), dim3((unsigned)tpp * np), dim3(kBlock), 0, h->stream,
                       (const FinDesc*)dtab, h->arena, tpp);
  else
    hipLaunchKernelGGL((k_finalize<false, false>), dim3((unsigned)tpp * np), dim3(kBlock), 0, h->stream,
                       (const FinDesc*)dtab, h->arena, tpp);
  HIP_TRY(h, hipGetLastError());
  for (int q = p0; q < p0 + np; ++q) h->agg_zero[q] = h->rep_zero[q] = 1;
  return IPLS_OK;
}

// GetPartitions' divide (IPLS.java:1159-1174) of Weights[p0..p0+np) into d_out,
// partition p at flat_off[p] - flat_off[p0].
// The divide's descriptor table for Weights[p0..p0+np), uploaded, and its tiles per partition (0: none).
static int divide_table(ipls_dev* h, int p0, int np, const DivDesc** dtab, int* tpp) {
  std::vector<DivDesc> dd(np);
  int64_t maxn = 0;
  for (int q = 0; q < np; ++q) {
    const int p = p0 + q;
    dd[q] = DivDesc{h->len[p], h->w_off[p], h->flat_off[p] - h->flat_off[p0]};
    maxn = std::max(maxn, h->len[p] - 1);
  }
  *tpp = (int)((std::max<int64_t>(maxn, 0) + kDivTile - 1) / kDivTile);
  if (*tpp == 0) return IPLS_OK;
  void* d = nullptr;
  if (int rc = upload_table(h, dd.data(), dd.size() * sizeof(DivDesc), &d)) return rc;
  *dtab = (const DivDesc*)d;
  return IPLS_OK;
}

static int divide_range(ipls_dev* h, int p0, int np, unsigned long long* d_out, bool be) {
  const DivDesc* dtab = nullptr;
  int tpp = 0;
  if (int rc = divide_table(h, p0, np, &dtab, &tpp)) return rc;
  if (tpp == 0) return IPLS_OK;
  with_bool(be, [&](auto b) {
    with_bool(h->secure != 0, [&](auto sec) {
      hipLaunchKernelGGL((k_divide<decltype(b)::value, decltype(sec)::value>), dim3((unsigned)tpp * np), dim3(kBlock),
                         0, h->stream, dtab, (const double*)h->arena, d_out, tpp);
    });
  });
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

// The same divide narrowed to a trainer format (k_divide_narrow): d_out holds
// floats, halves or bfloat16s.
static int divide_range_narrow(ipls_dev* h, int p0, int np, void* d_out, Fmt fmt) {
  const DivDesc* dtab = nullptr;
  int tpp = 0;
  if (int rc = divide_table(h, p0, np, &dtab, &tpp)) return rc;
  if (tpp == 0) return IPLS_OK;
  with_narrow(fmt, [&](auto s) {
    typedef decltype(s) S;
    with_bool(h->secure != 0, [&](auto sec) {
      hipLaunchKernelGGL((k_divide_narrow<S, decltype(sec)::value>), dim3((unsigned)tpp * np), dim3(kBlock), 0,
                         h->stream, dtab, (const double*)h->arena, (typename S::elem*)d_out, tpp);
    });
  });
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

int dev_finalize(ipls_dev* h, int p, void* sum_out, int sum_kind, double* avg_out) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  int p0 = p, np = 1;
  if (p == IPLS_ALL_PARTITIONS) {
    p0 = 0;
    np = h->P;
    if (sum_out || avg_out) return fail(h, IPLS_E_INVAL, "host outputs need a single partition");
  } else if (int rc = check_part(h, p)) {
    return rc;
  }
  // validate the outputs before anything is consumed: finalize_range flags
  // AGG/REP logically zero, so a rejected call must not get that far
  if (sum_out && sum_kind != IPLS_HOST_F64 && sum_kind != IPLS_HOST_BE)
    return fail(h, IPLS_E_INVAL, "sum_kind must be HOST_F64 or HOST_BE");
  HIP_TRY(h, dev_use(h->device));
  if (int rc = finalize_range(h, p0, np)) return rc;

  if (np == 1 && (sum_out || avg_out)) {
    const int64_t L = h->len[p0];
    const double* w = h->arena + h->w_off[p0];
    if (sum_out) {
      if (sum_kind == IPLS_HOST_F64) {
        if (int rc = d2h(h, sum_out, w, (size_t)L * 8)) return rc;
      } else if (sum_kind == IPLS_HOST_BE) {
        if (int rc = be_to_host(h, sum_out, w, L)) return rc;
      } else {
        return fail(h, IPLS_E_INVAL, "sum_kind must be HOST_F64 or HOST_BE");
      }
    }
    if (avg_out && L > 1) {
      if (int rc = ensure_scratch(h, (size_t)L * 8)) return rc;
      if (int rc = divide_range(h, p0, 1, (unsigned long long*)h->d_scratch, false)) return rc;
      if (int rc = d2h(h, avg_out, h->d_scratch, (size_t)(L - 1) * 8)) return rc;
    }
  }
  return IPLS_OK;
}

// AggregatePartition of one partition with the commit_update bytes (or the
// sum as doubles) handed to a sink chunk by chunk, as one call.  Under the
// engine lock: W = AGG + REP and a snapshot of W (or of its big-endian bytes)
// into this call's own staging -- one kernel or copy on the shard stream.
// The lock is then released and the snapshot goes to the sink through the
// pinned ring, chunks k + 1 .. k + 2 in flight while sink() copies chunk k.
// The bytes are the W of this call's AggregatePartition whatever another
// caller's set_weights / fold / finalize does meanwhile (the per-range reads
// of dev_read_range cannot promise that), and a slow sink (a socket send)
// holds nothing: the reference writes after Get_Partitions has returned
// (Middleware.java:254).
int dev_finalize_chunked(ipls_dev* h, int p, int sum_kind, int64_t chunk, ipls_chunk_sink sink, void* ctx) {
  if (!h || !sink) return fail_nl(h, IPLS_E_INVAL, "null argument");
  if (int rc = check_chunk(h, chunk, "values")) return rc;
  if (int rc = check_part_nl(h, p)) return rc;
  if (sum_kind != IPLS_HOST_F64 && sum_kind != IPLS_HOST_BE)
    return fail_nl(h, IPLS_E_INVAL, "sum_kind must be HOST_F64 or HOST_BE");
  const int64_t L = h->len[p], c = std::min(chunk, L);
  ipls_stage* st = nullptr;
  int rc = stage_snapshot(h, (size_t)L * 8, (size_t)c * 8, &st, [&](ipls_stage* s) {
    if (int r = finalize_range(h, p, 1)) return r;
    const unsigned long long* w = (const unsigned long long*)(h->arena + h->w_off[p]);
    hipError_t e;
    if (sum_kind == IPLS_HOST_BE) {
      launch_bswap(h->stream, w, (unsigned long long*)s->d, L);
      e = hipGetLastError();
    } else {
      e = hipMemcpyAsync(s->d, w, (size_t)L * 8, hipMemcpyDeviceToDevice, h->stream);
    }
    if (e == hipSuccess) return IPLS_OK;
    (void)hipGetLastError();
    return fail(h, IPLS_E_DEVICE, "W snapshot: %s", hipGetErrorString(e));
  });
  if (rc) return rc;
  rc = stage_deliver(h, st, L, c, 0, sink, ctx, " (the round is consumed)");
  dev_stage_release(h, st, rc);
  return rc;
}

int dev_set_weights(ipls_dev* h, int p, const void* src, int64_t n, int src_kind) {
  if (!h || !src) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  const int64_t L = h->len[p];
  op::Resolved v;
  if (op::resolve(op::kSetWeights, src, n, src_kind, L, &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  // ThreadReceiver pid 4 (IPLS.java:491-498): Weight_Address[p][i] = GET_GRADIENTS(frame) payload[i] for
  // i < L_p.  GetParameters(hash, arr) writes all its data.length / 8 values (MyIPFSClass.java:449-452).
  const int64_t m = v.from == op::kFrame ? L : v.n;
  double* w = h->arena + h->w_off[p];
  const void* d = v.ptr;
  if (v.host) {
    if (v.fmt == kFmtF64) return stage_h2d(h, w, v.ptr, (size_t)m * 8);
    if (int rc = to_scratch(h, v.ptr, (size_t)m * 8)) return rc;
    d = h->d_scratch;
  } else if (v.fmt == kFmtF64) {
    HIP_TRY(h, hipMemcpyAsync(w, v.ptr, (size_t)m * 8, hipMemcpyDeviceToDevice, h->stream));
    return IPLS_OK;
  }
  launch_bswap(h->stream, (const unsigned long long*)d, (unsigned long long*)w, m);
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

// A resolved flat vector (doubles, or a trainer format at 4 or 2 B per element
// on the device and over PCIe) as device memory: one of host memory goes
// through the scratch buffer, one of device memory is used in place.
static int flat_to_device(ipls_dev* h, const op::SrcView& v, const unsigned long long** d) {
  *d = (const unsigned long long*)v.ptr;
  if (!v.host) return IPLS_OK;
  if (int rc = to_scratch(h, v.ptr, (size_t)v.n * fmt_size(v.fmt))) return rc;
  *d = (const unsigned long long*)h->d_scratch;
  return IPLS_OK;
}

int dev_other_replica(ipls_dev* h, int p, int32_t aggregator, const void* src, int64_t n, int src_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  auto key = std::make_pair(p, aggregator);
  auto it = h->other.find(key);
  const bool first = it == h->other.end();
  // Download_Scheduler.java:254-260: `for j < gradients.length: Other[j] += g[j]`
  // -- a longer download overruns the stored array (rejected before folding).
  op::Resolved v;
  if (op::resolve(op::kOtherReplica, src, n, src_kind, first ? -1 : it->second.n, &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  const unsigned long long* d;
  const bool be = v.fmt == kFmtBE;
  if (int rc = flat_to_device(h, v, &d)) return rc;
  unsigned long long* dst = first ? nullptr : it->second.d;
  // Other.put(key, GetParameters(Hash)): a new array of the file's length (:263)
  if (first) HIP_TRY(h, hipMalloc(&dst, (size_t)std::max<int64_t>(n, 1) * 8));
  hipError_t e = hipSuccess;
  if (n > 0) {
    const bool vec = al16(dst) && al16(d);
    const dim3 g = ew_grid(n, vec, 4096);
    with_bool(be, [&](auto b) {
      with_bool(first, [&](auto f) {
        with_bool(vec, [&](auto v) {
          hipLaunchKernelGGL((k_fold_n<decltype(b)::value, decltype(f)::value, decltype(v)::value>), g, dim3(kBlock),
                             0, h->stream, dst, d, n);
        });
      });
    });
    e = hipGetLastError();
  }
  if (e == hipSuccess && v.host) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {   // the store is left as it was (the front's key model relies on it)
    (void)hipGetLastError();
    if (first) hipFree(dst);
    return fail(h, IPLS_E_DEVICE, "replica fold failed: %s", hipGetErrorString(e));
  }
  if (first) h->other[key] = ipls_dev::OtherRep{dst, n, 1};
  else it->second.received += 1;   // Other_Replica_Gradients_Received + 1 (:260)
  return IPLS_OK;
}

int dev_other_replica_drop(ipls_dev* h, int p, int32_t aggregator) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  auto it = h->other.find(std::make_pair(p, aggregator));
  if (it == h->other.end()) return 0;   // containsKey false: nothing to remove
  // Other_Replica_Gradients.remove(key) + Other_Replica_Gradients_Received.remove(key)
  // (Download_Scheduler.java:215-217, 329-332, 438-440).  Folds into the array
  // may still be queued on the stream: free it only after them.
  HIP_TRY(h, dev_use(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  hipFree(it->second.d);
  h->other.erase(it);
  return 1;
}

int dev_collect_replicas(ipls_dev* h, int32_t* participants, const int32_t* order, int n_order) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  HIP_TRY(h, dev_use(h->device));
  // the fold order: `new ArrayList<>(Other_Replica_Gradients.keySet())`
  // (IPLS.java:1218), given by the front's model of the JDK HashMap
  // (java_hashmap.hpp) as engine-local (p, aggregator) pairs -- every stored
  // key exactly once
  if (n_order != (int)h->other.size() || (n_order > 0 && !order))
    return fail(h, IPLS_E_INVAL, "collect order lists %d keys, the store holds %zu", n_order, h->other.size());
  std::vector<std::map<std::pair<int, int32_t>, ipls_dev::OtherRep>::iterator> seq;
  seq.reserve(n_order);
  std::set<std::pair<int, int32_t>> seen;   // each key once (O(n log n) for large stores)
  for (int i = 0; i < n_order; ++i) {
    const std::pair<int, int32_t> key((int)order[2 * i], order[2 * i + 1]);
    auto it = h->other.find(key);
    if (it == h->other.end() || !seen.insert(key).second)
      return fail(h, IPLS_E_INVAL, "collect order key (%d, %d) is not a stored key", order[2 * i] + h->p_lo,
                  order[2 * i + 1]);
    seq.push_back(it);
  }
  // REP[p] is a double[L_p]: a longer stored array overruns it (IPLS.java:1225).
  for (auto& kv : h->other)
    if (kv.second.n > h->len[kv.first.first])
      return fail(h, IPLS_E_RANGE, "stored replica of %lld doubles > partition %d length %lld "
                  "(ArrayIndexOutOfBoundsException, IPLS.java:1225)", (long long)kv.second.n, kv.first.first,
                  (long long)h->len[kv.first.first]);
  if (participants)
    for (int q = 0; q < h->P; ++q) participants[q] = 0;
  int folded = 0;
  for (auto& it : seq) {   // IPLS.java:1222-1234: REP[p][j] = REP[p][j] + Other[j], j < Other.length
    const int p = it->first.first;
    const int64_t n = it->second.n;
    // PeerData.Participants (IPLS.java:1229-1234): the put / replace sits INSIDE
    // the j loop, so the reference adds the key's download count once per
    // element -- received * n in all, in wrapping int arithmetic
    if (participants)
      participants[p] = (int32_t)((uint32_t)participants[p] + (uint32_t)it->second.received * (uint32_t)n);
    if (n > 0) {
      if (int rc = materialize(h, p, IPLS_TGT_REP)) return rc;
      auto rdst = (unsigned long long*)(h->arena + h->rep_off[p]);
      const bool vec = al16(rdst) && al16(it->second.d);
      with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((k_fold_n<false, false, decltype(v)::value>), ew_grid(n, vec, 4096), dim3(kBlock), 0, h->stream,
                           rdst, it->second.d, n);
      });
      HIP_TRY(h, hipGetLastError());
    }
    ++folded;
  }
  // Other_Replica_Gradients = new HashMap<>() (:1237-1238)
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (auto& kv : h->other) hipFree(kv.second.d);
  h->other.clear();
  return folded;
}

int dev_load_model(ipls_dev* h, const void* src, int64_t n, int src_kind) {
  if (!h || !src) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  op::Resolved v;
  if (op::resolve(op::kLoadModel, src, n, src_kind, h->flat_total, &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  const unsigned long long* d;
  const Fmt fmt = v.fmt;
  // only this engine's segment [flat_base, flat_total) of the model
  v.ptr = (const char*)v.ptr + fmt_size(fmt) * h->flat_base;
  v.n = h->flat_total - h->flat_base;
  if (int rc = flat_to_device(h, v, &d)) return rc;
  for (int p = 0; p < h->P; ++p) {
    const int64_t L = h->len[p];
    // IPLS.java:1883-1895: values for j < min((i+1)c, M), count slot 0.0
    if (fmt_trainer(fmt))
      with_narrow(fmt, [&](auto s) {
        typedef decltype(s) S;
        hipLaunchKernelGGL(k_load_model_narrow<S>, dim3(blocks_for(L, kBlock)), dim3(kBlock), 0, h->stream,
                           (const typename S::elem*)d, h->flat_off[p] - h->flat_base, L - 1, L,
                           h->arena + h->w_off[p]);
      });
    else
      with_bool(fmt == kFmtBE, [&](auto be) {
        hipLaunchKernelGGL(k_load_model<decltype(be)::value>, dim3(blocks_for(L, kBlock)), dim3(kBlock), 0, h->stream, d,
                           h->flat_off[p] - h->flat_base, L - 1, L, h->arena + h->w_off[p]);
      });
    HIP_TRY(h, hipGetLastError());
    h->agg_zero[p] = h->rep_zero[p] = h->fut_zero[p] = 1;   // IPLS.java:1886-1898
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

// OrganizeGradients bounds for partition p of a flat vector of n values.
static int split_bounds(ipls_dev* h, int p, int64_t n, int64_t* ncopy) {
  const int64_t lo = h->flat_off[p];
  const int64_t hi = std::min(lo + h->chunk, n);
  const int64_t nc = std::max<int64_t>(0, hi - lo);
  if (nc > h->len[p] - 1)
    return fail(h, IPLS_E_RANGE, "gradient vector of %lld values overruns partition %d (ArrayIndexOutOfBounds, IPLS.java:1030)",
                (long long)n, p);
  *ncopy = nc;
  return IPLS_OK;
}

int dev_split(ipls_dev* h, const void* flat, int64_t n, int src_kind, int p, void* dst, int dst_kind) {
  if (!h || !flat || !dst) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  int64_t ncopy;
  if (int rc = split_bounds(h, p, n, &ncopy)) return rc;
  HIP_TRY(h, dev_use(h->device));
  const int64_t L = h->len[p];
  op::Resolved sv;
  if (op::resolve(op::kSplit, flat, n, src_kind, L, &sv) != op::kTake) return not_taken(h, sv.why);
  // only the partition's own slice is needed on the device (doubles, or
  // floats, halves or bfloat16s at 4 or 2 B per element): a host slice is
  // staged into the first L + 1 doubles' worth of scratch, the output after it
  const Fmt fmt = fmt_trainer(sv.fmt) ? sv.fmt : kFmtF64;
  const bool be_in = sv.fmt == kFmtBE;
  const int esz = fmt_size(fmt);
  const char* slice = (const char*)flat + h->flat_off[p] * esz;
  if (int rc = sv.host ? to_scratch(h, slice, (size_t)ncopy * esz, (size_t)(2 * L + 2) * 8)
                      : ensure_scratch(h, (size_t)(fmt_trainer(fmt) ? 2 * L + 2 : L + 1) * 8))
    return rc;
  const auto* d = (const unsigned long long*)(sv.host ? (const char*)h->d_scratch : slice);
  const bool host_out = dst_kind == IPLS_HOST_F64 || dst_kind == IPLS_HOST_BE;
  const bool be_out = dst_kind == IPLS_HOST_BE || dst_kind == IPLS_DEV_BE;
  if (!host_out && dst_kind != IPLS_DEV_F64 && dst_kind != IPLS_DEV_BE)
    return fail(h, IPLS_E_INVAL, "bad dst_kind %d", dst_kind);
  unsigned long long* out = host_out ? (unsigned long long*)((char*)h->d_scratch + (size_t)(L + 1) * 8)
                                     : (unsigned long long*)dst;
  if (host_out && !sv.host) out = (unsigned long long*)h->d_scratch;
  const bool vec = al16(d) && al16(out);
  const dim3 g = vec ? dim3(std::max(1u, blocks_for(L, kEwTile))) : dim3(blocks_for(L, kBlock));
  auto flags = [&](auto&& f) {   // f(be_out, vec)
    with_bool(be_out, [&](auto bo) { with_bool(vec, [&](auto v) { f(bo, v); }); });
  };
  if (fmt_trainer(fmt))
    with_narrow(fmt, [&](auto s) {
      typedef decltype(s) S;
      flags([&](auto bo, auto v) {
        hipLaunchKernelGGL((k_split_narrow<S, decltype(bo)::value, 0, decltype(v)::value>), g, dim3(kBlock), 0,
                           h->stream, (const typename S::elem*)d, (int64_t)0, ncopy, L, out);
      });
    });
  else
    with_bool(be_in, [&](auto bi) {
      flags([&](auto bo, auto v) {
        hipLaunchKernelGGL((k_split<decltype(bi)::value, decltype(bo)::value, 0, decltype(v)::value>), g, dim3(kBlock),
                           0, h->stream, d, (int64_t)0, ncopy, L, out);
      });
    });
  HIP_TRY(h, hipGetLastError());
  if (host_out) return d2h(h, dst, out, (size_t)L * 8);
  return IPLS_OK;
}

int dev_update_gradient(ipls_dev* h, const void* flat, int64_t n, int src_kind, const int32_t* owned,
                             int n_owned) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  if (!flat) return IPLS_OK;  // Gradients == null (IPLS.java:1708-1713, 1738 `&& Gradients != null`)
  IPLS_LOCK(h);
  if (n_owned < 0 || (n_owned > 0 && !owned)) return fail(h, IPLS_E_INVAL, "bad owned list");
  // OrganizeGradients splits every partition before anything is accumulated
  // (IPLS.java:1709), so a length error leaves the accumulators untouched.
  std::vector<int64_t> nc(h->P);
  for (int p = 0; p < h->P; ++p)
    if (int rc = split_bounds(h, p, n, &nc[p])) return rc;
  for (int i = 0; i < n_owned; ++i)
    if (int rc = check_part(h, owned[i])) return rc;
  if (n_owned == 0) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  op::Resolved sv;
  if (op::resolve(op::kUpdateGradient, flat, n, src_kind, 0, &sv) != op::kTake) return not_taken(h, sv.why);
  // only this engine's segment of the gradient vector (flat_base on)
  const int64_t seg = std::max<int64_t>(0, std::min(n, h->flat_total) - h->flat_base);
  const Fmt fmt = fmt_trainer(sv.fmt) ? sv.fmt : kFmtF64;
  const bool be = sv.fmt == kFmtBE;
  const int64_t esz = fmt_size(fmt);
  const char* base = (const char*)flat + esz * h->flat_base;
  auto d = (const unsigned long long*)base;   // device memory is read in place
  if (sv.host) {
    // from host memory only the owned partitions' values cross PCIe, at 8, 4
    // or 2 B per element: the others are split by OrganizeGradients too, but
    // never accumulated (IPLS.java:1737-1743), so their bytes are never read here
    if (int rc = ensure_scratch(h, (size_t)std::max<int64_t>(seg, 1) * esz)) return rc;
    for (int i = 0; i < n_owned; ++i) {
      const int64_t lo = h->flat_off[owned[i]] - h->flat_base;
      if (int rc = stage_h2d(h, (char*)h->d_scratch + esz * lo, base + esz * lo, (size_t)nc[owned[i]] * esz)) return rc;
    }
    d = (const unsigned long long*)h->d_scratch;
  }
  for (int i = 0; i < n_owned; ++i) {
    const int p = owned[i];
    const int64_t L = h->len[p];
    unsigned long long* acc = (unsigned long long*)(h->arena + h->agg_off[p]);
    const bool zero = h->agg_zero[p];
    const int64_t lo = h->flat_off[p] - h->flat_base;
    // the segment's start decides: partitions whose flat offset is odd read
    // their values at 8 mod 16 and keep the element-per-lane shape
    // (trainer formats: per partition too -- flat + p*chunk elements is only
    // element-aligned in general)
    const bool vec = al16((const char*)d + esz * lo) && al16(acc);
    const dim3 g = vec ? dim3(std::max(1u, blocks_for(L, kEwTile))) : dim3(blocks_for(L, kBlock));
    // Logically-zero accumulator: MODE 2 writes +0.0 + v without reading it
    // (the bits of a fold into zeros)
    auto flags = [&](auto&& f) {   // f(zero, vec)
      with_bool(zero, [&](auto z) { with_bool(vec, [&](auto v) { f(z, v); }); });
    };
    if (fmt_trainer(fmt))
      with_narrow(fmt, [&](auto s) {
        typedef decltype(s) S;
        flags([&](auto z, auto v) {
          hipLaunchKernelGGL((k_split_narrow<S, false, decltype(z)::value ? 2 : 1, decltype(v)::value>), g,
                             dim3(kBlock), 0, h->stream, (const typename S::elem*)d, lo, nc[p], L, acc);
        });
      });
    else
      with_bool(be, [&](auto bi) {
        flags([&](auto z, auto v) {
          hipLaunchKernelGGL((k_split<decltype(bi)::value, false, decltype(z)::value ? 2 : 1, decltype(v)::value>), g,
                             dim3(kBlock), 0, h->stream, d, lo, nc[p], L, acc);
        });
      });
    HIP_TRY(h, hipGetLastError());
    h->agg_zero[p] = 0;
  }
  return IPLS_OK;
}

int dev_get_partitions(ipls_dev* h, void* out, int64_t n, int out_kind) {
  if (!h || !out) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  // out holds this engine's segment: flat offsets [flat_base, flat_total)
  const int64_t M = h->flat_total - h->flat_base;
  if (n < M) return fail(h, IPLS_E_RANGE, "output of %lld < model size %lld", (long long)n, (long long)M);
  if (out_kind != IPLS_HOST_F64 && out_kind != IPLS_HOST_BE_CANON && out_kind != IPLS_DEV_F64 &&
      !kind_trainer(out_kind))
    return fail(h, IPLS_E_INVAL, "bad out_kind %d", out_kind);
  HIP_TRY(h, dev_use(h->device));
  if (kind_trainer(out_kind)) {
    // Model.java:388-390: the model narrowed to float, half or bfloat16, on the
    // device; a host output comes back as 4 or 2 B per value
    const Fmt fmt = kind_fmt(out_kind);
    const int esz = fmt_size(fmt);
    if ((uintptr_t)out & (uintptr_t)(esz - 1)) return fail(h, IPLS_E_INVAL, "output not %d-byte aligned", esz);
    void* d_n = out;
    if (kind_trainer_host(out_kind)) {
      if (int rc = ensure_scratch(h, (size_t)std::max<int64_t>(M, 1) * esz)) return rc;
      d_n = h->d_scratch;
    }
    if (int rc = divide_range_narrow(h, 0, h->P, d_n, fmt)) return rc;
    if (kind_trainer_dev(out_kind)) return IPLS_OK;
    return d2h(h, out, d_n, (size_t)M * esz);
  }
  unsigned long long* d_out;
  if (out_kind == IPLS_DEV_F64) {
    if ((uintptr_t)out & 7) return fail(h, IPLS_E_INVAL, "device output not 8-byte aligned");
    d_out = (unsigned long long*)out;
  } else {
    if (int rc = ensure_scratch(h, (size_t)std::max<int64_t>(M, 1) * 8)) return rc;
    d_out = (unsigned long long*)h->d_scratch;
  }
  if (int rc = divide_range(h, 0, h->P, d_out, out_kind == IPLS_HOST_BE_CANON)) return rc;
  if (out_kind == IPLS_DEV_F64) return IPLS_OK;
  return d2h(h, out, d_out, (size_t)M * 8);
}

// GetPartitions (IPLS.java:1159-1174) handed to the caller chunk by chunk,
// in two phases so that a multi-shard handle snapshots every shard before it
// delivers any byte (ipls_agg.cpp):
//  * snapshot, under the engine lock: the divide runs once into this call's
//    own staging (wire: the same values as Middleware's task-3 writeDouble
//    stream -- big-endian, NaN canonical: k_divide's OUT_BE form);
//  * deliver, with no lock held: chunk k + 1 is copied into one slot of the
//    stage's pinned ring while sink() consumes chunk k from another slot,
//    on the calling thread (the JNI shim's sink is SetDoubleArrayRegion, the
//    Middleware's a socket send).  sink gets flat model offsets (this engine's
//    segment starts at flat_base); a non-zero return stops the transfer
//    (IPLS_E_INVAL, nothing further is delivered).
// *st is null when the engine's segment is empty.
// fmt: kFmtF64 (doubles, or with `wire` the big-endian stream), or a trainer
// format -- the snapshot is then k_divide_narrow's, M elements of 4 or 2 B.
int dev_get_partitions_snapshot(ipls_dev* h, int64_t chunk, bool wire, ipls_stage** st_out, Fmt fmt) {
  *st_out = nullptr;
  if (!h) return fail_nl(h, IPLS_E_INVAL, "null argument");
  if (int rc = check_chunk(h, chunk, fmt_trainer(fmt) ? "values" : "doubles")) return rc;
  if (wire && fmt_trainer(fmt)) return fail_nl(h, IPLS_E_INVAL, "the wire stream holds doubles");
  const int64_t M = h->flat_total - h->flat_base;
  if (M <= 0) return IPLS_OK;
  const size_t esz = (size_t)fmt_size(fmt);
  return stage_snapshot(h, (size_t)M * esz, (size_t)std::min(chunk, M) * esz, st_out, [&](ipls_stage* st) {
    return fmt_trainer(fmt) ? divide_range_narrow(h, 0, h->P, st->d, fmt)
                            : divide_range(h, 0, h->P, (unsigned long long*)st->d, wire);
  });
}

int dev_get_partitions_deliver(ipls_dev* h, ipls_stage* st, int64_t chunk, ipls_chunk_sink sink, void* ctx) {
  if (!st) return IPLS_OK;
  const int64_t M = h->flat_total - h->flat_base;
  if (int rc = use_nl(h)) return rc;
  return stage_deliver(h, st, M, std::min(chunk, M), h->flat_base, sink, ctx, "");
}

// Delivery of a trainer-format snapshot: bytes, at byte offsets of the flat
// narrowed model, every piece a whole number of elements (chunk in elements).
int dev_get_partitions_deliver_narrow(ipls_dev* h, ipls_stage* st, int64_t chunk, Fmt fmt, ipls_byte_sink sink,
                                      void* ctx) {
  if (!st) return IPLS_OK;
  const int64_t M = h->flat_total - h->flat_base, esz = fmt_size(fmt);
  if (int rc = use_nl(h)) return rc;
  return stage_deliver_bytes(h, st, (const char*)st->d, M * esz, std::min(chunk, M) * esz, h->flat_base * esz, sink, ctx);
}

// ---- device utilities ----
int ipls_synth_fill(void* dst, int64_t len, uint64_t seed, int p, int k, int dst_kind, void* stream) {
  if (!dst || len < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (len == 0) return IPLS_OK;
  const unsigned long long key = seed ^ ((unsigned long long)(uint32_t)p << 40) ^ ((unsigned long long)(uint32_t)k << 32);
  const dim3 g(std::min<unsigned>(blocks_for(len, kBlock * 4), 8192));
  if (dst_kind == IPLS_DEV_BE)
    hipLaunchKernelGGL(k_synth<true>, g, dim3(kBlock), 0, (hipStream_t)stream, (unsigned long long*)dst, len, key);
  else if (dst_kind == IPLS_DEV_F64)
    hipLaunchKernelGGL(k_synth<false>, g, dim3(kBlock), 0, (hipStream_t)stream, (unsigned long long*)dst, len, key);
  else
    return fail(nullptr, IPLS_E_INVAL, "dst_kind must be DEV_F64 or DEV_BE");
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, IPLS_E_DEVICE, "k_synth launch: %s", hipGetErrorString(e));
  return IPLS_OK;
}

int ipls_checksum_dev(const void* src, int64_t n, int src_kind, uint64_t* out, void* stream) {
  if (!out || n < 0 || (n > 0 && !src)) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (n == 0) {
    *out = 0;
    return IPLS_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* d = nullptr;
  if (hipMallocAsync((void**)&d, 8, st) != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, IPLS_E_NOMEM, "hipMallocAsync failed");
  }
  hipMemsetAsync(d, 0, 8, st);
  const dim3 g(std::max(1u, std::min<unsigned>(blocks_for(n, kBlock * 8), 2048)));
  if (src_kind == IPLS_DEV_BE)
    hipLaunchKernelGGL(k_checksum<true>, g, dim3(kBlock), 0, st, (const unsigned long long*)src, n, d);
  else
    hipLaunchKernelGGL(k_checksum<false>, g, dim3(kBlock), 0, st, (const unsigned long long*)src, n, d);
  unsigned long long v = 0;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&v, d, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFreeAsync(d, st);
  if (e != hipSuccess) return fail(nullptr, IPLS_E_DEVICE, "checksum: %s", hipGetErrorString(e));
  *out = v;
  return IPLS_OK;
}

int dev_reduce_batch_out(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, int src_kind,
                              int start_mode, void* const* dst, int dst_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_parts <= 0 || p_first < 0 || p_first + n_parts > h->P)
    return fail(h, IPLS_E_RANGE, "partitions [%d,%d) out of range [0,%d)", p_first, p_first + n_parts, h->P);
  if (src_kind != IPLS_DEV_F64 && src_kind != IPLS_DEV_BE && !kind_trainer_dev(src_kind))
    return fail(h, IPLS_E_INVAL, "reduce_batch_out takes device buckets (DEV_F64/DEV_BE/DEV_F32/DEV_F16/DEV_BF16)");
  if (dst_kind != IPLS_DEV_F64 && dst_kind != IPLS_DEV_BE)
    return fail(h, IPLS_E_INVAL, "reduce_batch_out writes device buffers (DEV_F64/DEV_BE)");
  if (start_mode < IPLS_START_ACCUM || start_mode > IPLS_START_FIRST) return fail(h, IPLS_E_INVAL, "bad start mode");
  if (!dst || k < 0 || (k > 0 && !bufs)) return fail(h, IPLS_E_INVAL, "bad bucket/destination list");
  HIP_TRY(h, dev_use(h->device));
  return reduce_dev(h, p_first, n_parts, bufs, k, kind_fmt(src_kind), start_mode, IPLS_TGT_AGG, dst,
                    dst_kind == IPLS_DEV_BE);
}

int dev_aggregate_round(ipls_dev* h, int p_first, int n_parts, const void* const* bufs, int k, int src_kind,
                             void* avg_out, int avg_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_parts <= 0 || p_first < 0 || p_first + n_parts > h->P)
    return fail(h, IPLS_E_RANGE, "partitions [%d,%d) out of range [0,%d)", p_first, p_first + n_parts, h->P);
  if (src_kind != IPLS_DEV_F64 && src_kind != IPLS_DEV_BE && !kind_trainer_dev(src_kind))
    return fail(h, IPLS_E_INVAL, "aggregate_round takes device buckets (DEV_F64/DEV_BE/DEV_F32/DEV_F16/DEV_BF16)");
  const Fmt fmt_in = kind_fmt(src_kind);
  const bool tr_in = fmt_trainer(fmt_in);
  // averages narrowed to a trainer format (floats, halves, bfloat16s)
  const bool tr_avg = avg_out && kind_trainer(avg_kind);
  const Fmt fmt_avg = tr_avg ? kind_fmt(avg_kind) : kFmtF64;
  if (avg_out && !tr_avg && avg_kind != IPLS_DEV_F64 && avg_kind != IPLS_HOST_F64)
    return fail(h, IPLS_E_INVAL, "avg_kind must be DEV_F64, HOST_F64 or a DEV/HOST F32, F16 or BF16 kind");
  if (k < 0 || (k > 0 && !bufs)) return fail(h, IPLS_E_INVAL, "bad bucket list");
  if (tr_in)
    for (int64_t i = 0; i < (int64_t)n_parts * k; ++i)   // before anything is consumed
      if (!bufs[i] || ((uintptr_t)bufs[i] & (uintptr_t)(fmt_size(fmt_in) - 1)))
        return fail(h, IPLS_E_INVAL, "bucket %lld NULL or not %d-byte aligned", (long long)i, fmt_size(fmt_in));
  HIP_TRY(h, dev_use(h->device));
  const int p_last = p_first + n_parts - 1;
  const int64_t n_avg = h->flat_off[p_last] + h->len[p_last] - 1 - h->flat_off[p_first];
  unsigned long long* d_avg = nullptr;
  if (tr_avg && n_avg > 0) {
    if ((uintptr_t)avg_out & (uintptr_t)(fmt_size(fmt_avg) - 1))
      return fail(h, IPLS_E_INVAL, "output not %d-byte aligned", fmt_size(fmt_avg));
    if (kind_trainer_dev(avg_kind)) {
      d_avg = (unsigned long long*)avg_out;
    } else {
      if (int rc = ensure_scratch(h, (size_t)n_avg * fmt_size(fmt_avg))) return rc;
      d_avg = (unsigned long long*)h->d_scratch;
    }
  } else if (avg_out && n_avg > 0) {
    if (avg_kind == IPLS_DEV_F64) {
      if ((uintptr_t)avg_out & 7) return fail(h, IPLS_E_INVAL, "device output not 8-byte aligned");
      d_avg = (unsigned long long*)avg_out;
    } else {
      if (int rc = ensure_scratch(h, (size_t)n_avg * 8)) return rc;
      d_avg = (unsigned long long*)h->d_scratch;
    }
  }
  bool aligned16 = true;
  for (int64_t i = 0; i < (int64_t)n_parts * k; ++i) aligned16 = aligned16 && !((uintptr_t)bufs[i] & 15);
  // fused: doubles in, doubles out (k_round); a trainer format in, none or a trainer format out (k_round_narrow)
  if (aligned16 && (tr_in ? (!avg_out || tr_avg) : !tr_avg)) {
    FinOut fo{d_avg, fmt_avg};
    if (int rc = reduce_dev(h, p_first, n_parts, bufs, k, fmt_in, IPLS_START_ACCUM, IPLS_TGT_AGG,
                            nullptr, false, &fo))
      return rc;
  } else {
    // 8-B aligned buckets (frames at odd offsets): the same three steps unfused
    // trainer-format buckets off a 16-B boundary or with F64 averages, F64 / BE
    // buckets with trainer-format averages: the widening fold / the narrowing
    // divide take the place of the fused kernel's halves (bit-identical by definition)
    if (int rc = reduce_dev(h, p_first, n_parts, bufs, k, fmt_in, IPLS_START_ACCUM, IPLS_TGT_AGG)) return rc;
    if (int rc = finalize_range(h, p_first, n_parts)) return rc;
    if (d_avg) {
      if (tr_avg) {
        if (int rc = divide_range_narrow(h, p_first, n_parts, d_avg, fmt_avg)) return rc;
      } else if (int rc = divide_range(h, p_first, n_parts, d_avg, false)) {
        return rc;
      }
    }
  }
  if (d_avg && kind_trainer_host(avg_kind)) return d2h(h, avg_out, d_avg, (size_t)n_avg * fmt_size(fmt_avg));
  if (d_avg && avg_kind == IPLS_HOST_F64) return d2h(h, avg_out, d_avg, (size_t)n_avg * 8);
  return IPLS_OK;
}

// ---- pubsub ingest: base64url (x layers) -> frame -> fold, on the device ----
namespace {

// Copy-issuing threads of the pubsub ingest (IPLS_INGEST_COPY_THREADS, 1..4).
int ingest_copy_threads() {
  static const int n = [] {
    const char* e = std::getenv("IPLS_INGEST_COPY_THREADS");
    const int v = e ? std::atoi(e) : 2;
    return std::max(1, std::min(v, (int)ipls_dev::kCopyThreads));
  }();
  return n;
}

}  // namespace

// Pipeline: the host reads each text's ends (the '=' rules of both layers and
// the 14-byte frame header need only the first 28 and last 8 chars), so no
// device round trip sits between the copies and the decodes.  Texts go up on
// copy_stream while `stream` decodes the previous ones behind a per-message
// event; one sync reads the invalid-char flags, then each partition's frames
// are folded in message order.
int dev_ingest_pubsub(ipls_dev* h, int target, const uint8_t* const* msgs, const int64_t* lens, int n_msgs,
                           int layers, const int32_t* parts, int32_t* status) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_msgs < 0 || (n_msgs > 0 && (!msgs || !lens))) return fail(h, IPLS_E_INVAL, "bad message list");
  if (layers < 1 || layers > 2) return fail(h, IPLS_E_INVAL, "layers must be 1 or 2");
  if (target_off(h, 0, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  if (n_msgs == 0) return 0;
  HIP_TRY(h, dev_use(h->device));

  // 1. host: tail rules, frame header, routing (GET_GRADIENTS, MyIPFSClass.java:1437-1459).
  //    post[i] = the status if the device finds no invalid char; decode[i] = needs the device.
  std::vector<int32_t> st(n_msgs, 0), post(n_msgs, 0), route(n_msgs, -1);
  std::vector<int64_t> dc(n_msgs, 0), dc2(n_msgs, 0);
  std::vector<uint8_t> decode(n_msgs, 0);
  for (int i = 0; i < n_msgs; ++i) {
    const pubsub::Pre pre = pubsub::precheck(msgs[i], lens[i], layers);   // pubsub_host.cpp
    if (pre.status) { st[i] = pre.status; continue; }
    dc[i] = pre.dc;
    dc2[i] = pre.dc2;
    decode[i] = 1;
    if (pre.n == 0) { post[i] = 1; continue; }      // arr_len == 0 -> null gradient: no fold
    const int p = parts ? parts[i] : pre.a;
    if (p < 0 || p >= h->P || pre.n < h->len[p]) { post[i] = IPLS_E_RANGE; continue; }
    route[i] = p;
  }

  // 2. device: scratch [texts][layer-1 output][frames], 256-B aligned per message;
  //    frames start 2 bytes in so the payload (frame byte 14) is 16-B aligned.
  std::vector<int64_t> text_off(n_msgs, 0), mid_off(n_msgs, 0), frame_off(n_msgs, 0);
  int64_t off = 0;
  for (int i = 0; i < n_msgs; ++i)
    if (decode[i]) { text_off[i] = off; off = align_up(off + lens[i] + 16, 256); }
  if (layers == 2)
    for (int i = 0; i < n_msgs; ++i)
      if (decode[i]) { mid_off[i] = off; off = align_up(off + lens[i] + 16, 256); }
  for (int i = 0; i < n_msgs; ++i)
    if (decode[i]) { frame_off[i] = off + 2; off = align_up(off + 2 + lens[i] + 16, 256); }
  int n_dec = 0;
  for (int i = 0; i < n_msgs; ++i) n_dec += decode[i];
  if (n_dec) {
    if (int rc = ensure_scratch(h, (size_t)off + 64 * (size_t)n_msgs + 4096)) return rc;
    unsigned char* base = (unsigned char*)h->d_scratch;
    int* d_err = (int*)(base + off);
    std::vector<B64Desc> desc(2 * (size_t)n_msgs);
    for (int i = 0; i < n_msgs; ++i) {
      if (!decode[i]) continue;
      desc[i] = B64Desc{text_off[i], dc[i] / 4, layers == 2 ? mid_off[i] : frame_off[i], (int32_t)(dc[i] % 4), 0};
      desc[n_msgs + i] = B64Desc{mid_off[i], dc2[i] / 4, frame_off[i], (int32_t)(dc2[i] % 4), 0};
    }
    void* dtab = nullptr;
    if (int rc = upload_table(h, desc.data(), sizeof(B64Desc) * desc.size(), &dtab)) return rc;
    const B64Desc* d1 = (const B64Desc*)dtab;
    HIP_TRY(h, hipMemsetAsync(d_err, 0, sizeof(int) * n_msgs, h->stream));
    // Texts are pageable: each hipMemcpyAsync blocks its calling thread and
    // pays ~45 us of setup between transfers, so T threads issue the copies
    // (message j of the batch on thread j % T, its own stream) and this thread
    // queues each message's decodes behind that copy's event as it lands.
    const int T = std::max(1, std::min(ingest_copy_threads(), n_dec));
    for (int t = 0; t < T; ++t)
      if (!h->copy_stream[t]) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream[t], hipStreamNonBlocking));
    if (!h->ingest_ev) HIP_TRY(h, hipEventCreateWithFlags(&h->ingest_ev, hipEventDisableTiming));
    while ((int)h->msg_ev.size() < n_msgs) {
      hipEvent_t e;
      HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      h->msg_ev.push_back(e);
    }
    // the scratch may still be read by earlier work on `stream`
    HIP_TRY(h, hipEventRecord(h->ingest_ev, h->stream));
    for (int t = 0; t < T; ++t) HIP_TRY(h, hipStreamWaitEvent(h->copy_stream[t], h->ingest_ev, 0));
    std::vector<int> order;
    for (int i = 0; i < n_msgs; ++i)
      if (decode[i]) order.push_back(i);
    std::unique_ptr<std::atomic<int>[]> ready(new std::atomic<int>[n_dec]);   // 0 pending, 1 recorded, <0 error
    for (int j = 0; j < n_dec; ++j) ready[j].store(0);
    auto copier = [&](int t) {
      dev_use(h->device);
      for (int j = t; j < n_dec; j += T) {
        const int i = order[j];
        hipError_t e = hipMemcpyAsync(base + text_off[i], msgs[i], lens[i], hipMemcpyHostToDevice, h->copy_stream[t]);
        if (e == hipSuccess) e = hipEventRecord(h->msg_ev[i], h->copy_stream[t]);
        ready[j].store(e == hipSuccess ? 1 : -(int)e, std::memory_order_release);
        if (e != hipSuccess) {
          for (int r = j + T; r < n_dec; r += T) ready[r].store(-(int)e, std::memory_order_release);
          return;
        }
      }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(copier, t);
    if (T == 1) copier(0);
    else pool.emplace_back(copier, 0);
    int copy_err = 0;
    for (int j = 0; j < n_dec && !copy_err; ++j) {
      int r;
      while ((r = ready[j].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
      if (r < 0) { copy_err = -r; break; }
      const int i = order[j];
      hipStreamWaitEvent(h->stream, h->msg_ev[i], 0);
      hipLaunchKernelGGL(k_b64url_decode, dim3(blocks_for(dc[i] / 16 + 1, kBlock)), dim3(kBlock), 0, h->stream,
                         (const unsigned char*)base, d1 + i, base, d_err + i);
      if (layers == 2)
        hipLaunchKernelGGL(k_b64url_decode, dim3(blocks_for(dc2[i] / 16 + 1, kBlock)), dim3(kBlock), 0, h->stream,
                           (const unsigned char*)base, d1 + n_msgs + i, base, d_err + i);
    }
    for (auto& th : pool) th.join();
    if (copy_err) return fail(h, IPLS_E_DEVICE, "pubsub text copy failed: %s", hipGetErrorString((hipError_t)copy_err));
    HIP_TRY(h, hipGetLastError());
    std::vector<int> herr(n_msgs, 0);
    HIP_TRY(h, hipMemcpyAsync(herr.data(), d_err, sizeof(int) * n_msgs, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_msgs; ++i)
      if (decode[i]) st[i] = herr[i] ? IPLS_E_FORMAT : post[i];
    // 3. fold each partition's frames in message order
    std::vector<std::vector<const void*>> per_part(h->P);
    for (int i = 0; i < n_msgs; ++i)
      if (decode[i] && st[i] == 0) per_part[route[i]].push_back(base + frame_off[i] + 14);
    int folded = 0;
    for (int p = 0; p < h->P; ++p) {
      if (per_part[p].empty()) continue;
      if (int rc = reduce_dev(h, p, 1, per_part[p].data(), (int)per_part[p].size(), kFmtBE, IPLS_START_ACCUM, target))
        return rc;
      folded += (int)per_part[p].size();
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n_msgs);
    return folded;
  }
  if (status) std::memcpy(status, st.data(), sizeof(int32_t) * n_msgs);
  return 0;
}

int dev_blend(ipls_dev* h, int p, int target, const void* src, int64_t n, int src_kind, double a, double b) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  const int64_t L = h->len[p];
  op::Resolved v;   // HOST_DARR: the array's big-endian payload, then as HOST_BE
  if (op::resolve(op::kBlend, src, n, src_kind, L, &v) != op::kTake) return not_taken(h, v.why);
  HIP_TRY(h, dev_use(h->device));
  if (v.host)
    if (int rc = to_scratch(h, v.ptr, (size_t)L * 8)) return rc;
  auto gs = (const unsigned long long*)(v.host ? h->d_scratch : v.ptr);
  if (int rc = materialize(h, p, target)) return rc;
  double* t = h->arena + target_off(h, p, target);
  const bool vec = al16(t) && al16(gs);
  const dim3 g = ew_grid(L, vec, 8192);
  with_bool(v.fmt == kFmtBE, [&](auto be) {
    with_bool(vec, [&](auto vc) {
      hipLaunchKernelGGL((k_blend<decltype(be)::value, decltype(vc)::value>), g, dim3(kBlock), 0, h->stream, t, gs, L, a, b);
    });
  });
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

int dev_scale(ipls_dev* h, int p, int dst_target, int src_target, double c) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, dst_target) < 0 || target_off(h, p, src_target) < 0) return fail(h, IPLS_E_INVAL, "bad target");
  HIP_TRY(h, dev_use(h->device));
  if (int rc = materialize(h, p, src_target)) return rc;
  if (uint8_t* f = zero_flag(h, p, dst_target)) *f = 0;
  const int64_t L = h->len[p];
  double* sd = h->arena + target_off(h, p, dst_target);
  auto ss = (const double*)(h->arena + target_off(h, p, src_target));
  with_bool(al16(sd) && al16(ss), [&](auto v) {
    hipLaunchKernelGGL(k_scale<decltype(v)::value>, ew_grid(L, decltype(v)::value, 8192), dim3(kBlock), 0, h->stream, sd, ss,
                       L, c);
  });
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

int ipls_encode_secure(const void* src, void* dst, int64_t n, int src_kind, int dst_kind, void* stream) {
  if (!src || !dst || n < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if ((src_kind != IPLS_DEV_F64 && src_kind != IPLS_DEV_BE) || (dst_kind != IPLS_DEV_F64 && dst_kind != IPLS_DEV_BE))
    return fail(nullptr, IPLS_E_INVAL, "device operands only (DEV_F64 / DEV_BE)");
  if (n == 0) return IPLS_OK;
  hipStream_t st = (hipStream_t)stream;
  auto s = (const unsigned long long*)src;
  auto d = (unsigned long long*)dst;
  const bool bi = src_kind == IPLS_DEV_BE, bo = dst_kind == IPLS_DEV_BE;
  const bool vec = al16(s) && al16(d);
  const dim3 g = ew_grid(n, vec, 8192);
  with_bool(bi, [&](auto i) {
    with_bool(bo, [&](auto o) {
      with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((k_encode_secure<decltype(i)::value, decltype(o)::value, decltype(v)::value>), g,
                           dim3(kBlock), 0, st, s, d, n);
      });
    });
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, IPLS_E_DEVICE, "k_encode_secure: %s", hipGetErrorString(e));
  return IPLS_OK;
}

int ipls_host_alloc(size_t bytes, void** ptr) {
  if (!ptr) return fail(nullptr, IPLS_E_INVAL, "null ptr");
  *ptr = nullptr;
  if (bytes == 0) return IPLS_OK;
  hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *ptr = nullptr;
    (void)hipGetLastError();
    return fail(nullptr, e == hipErrorNoDevice ? IPLS_E_NODEV : IPLS_E_NOMEM, "hipHostMalloc(%zu): %s", bytes,
                hipGetErrorString(e));
  }
  return IPLS_OK;
}

int ipls_host_free(void* ptr) {
  if (!ptr) return IPLS_OK;
  hipError_t e = hipHostFree(ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, IPLS_E_INVAL, "hipHostFree: %s", hipGetErrorString(e));
  }
  return IPLS_OK;
}

static uint32_t rd_be32(const uint8_t* b) {
  return ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
}

int64_t ipls_frame_parse(const uint8_t* frame, int64_t len, int16_t* pid, int32_t* a, int32_t* b,
                         int64_t* payload_off, int64_t* origin_off) {
  if (!frame || len < 14) return fail(nullptr, IPLS_E_FORMAT, "frame shorter than its 14-byte header");
  const int16_t pd = (int16_t)(((uint16_t)frame[0] << 8) | frame[1]);
  const int32_t n = (int32_t)rd_be32(frame + 2);
  if (n < 0 || 14 + 8 * (int64_t)n > len)
    return fail(nullptr, IPLS_E_FORMAT, "frame declares %d doubles but holds %lld bytes", n, (long long)len);
  if (pid) *pid = pd;
  if (a) *a = (int32_t)rd_be32(frame + 6);
  if (b) *b = (int32_t)rd_be32(frame + 10);
  if (payload_off) *payload_off = 14;
  if (origin_off) *origin_off = 14 + 8 * (int64_t)n;
  return n;
}

int64_t ipls_pair_parse(const uint8_t* buf, int64_t len, int32_t* workers, int64_t* payload_off) {
  if (!buf || len < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  const char* why = nullptr;
  const int64_t nd = javaser::parse_pair(buf, len, workers, payload_off, &why);
  if (nd < 0) return fail(nullptr, IPLS_E_FORMAT, "partial update: %s", why ? why : "malformed");
  return nd;
}

int64_t ipls_pair_encode(int32_t workers, const void* g, int64_t n, int g_kind, uint8_t* out, int64_t out_cap) {
  if (n < 0 || n > INT32_MAX || (n > 0 && out && !g)) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (g_kind != IPLS_HOST_F64 && g_kind != IPLS_HOST_BE) return fail(nullptr, IPLS_E_INVAL, "g_kind must be HOST_F64/BE");
  const int64_t hl = javaser::pair_header_len(), total = hl + 8 * n + javaser::pair_trailer_len();
  if (!out) return total;
  if (out_cap < total) return fail(nullptr, IPLS_E_RANGE, "partial update needs %lld bytes", (long long)total);
  javaser::write_pair_header(out, workers, (int32_t)n);
  if (g_kind == IPLS_HOST_BE) {
    std::memcpy(out + hl, g, (size_t)n * 8);
  } else {
    for (int64_t i = 0; i < n; ++i) {   // ObjectOutputStream: writeDouble = BE doubleToLongBits
      uint64_t v;
      std::memcpy(&v, (const char*)g + 8 * i, 8);
      v = __builtin_bswap64(v);
      std::memcpy(out + hl + 8 * i, &v, 8);
    }
  }
  javaser::write_pair_trailer(out + hl + 8 * n);
  return total;
}

// ---- saved-model files: host codecs (javaser.hpp) ----
namespace {

// n doubles (HOST_F64 or HOST_BE) as the big-endian payload of a double[]
void put_payload(uint8_t* out, const void* g, int64_t n, int g_kind) {
  if (g_kind == IPLS_HOST_BE) {
    if (n) std::memcpy(out, g, (size_t)n * 8);
    return;
  }
  for (int64_t i = 0; i < n; ++i) {
    uint64_t v;
    std::memcpy(&v, (const char*)g + 8 * i, 8);
    v = __builtin_bswap64(v);
    std::memcpy(out + 8 * i, &v, 8);
  }
}

// Double.doubleToLongBits: every NaN is the canonical one
uint64_t canon_bits(uint64_t v) {
  return ((v & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (v & 0x000FFFFFFFFFFFFFull)) ? 0x7FF8000000000000ull
                                                                                                : v;
}

const uint8_t kDlistLead[6] = {0x73, 0x71, 0x00, 0x7E, 0x00, 0x02};   // TC_OBJECT TC_REFERENCE <Double's descriptor>

}  // namespace

int64_t ipls_saved_parse(const uint8_t* bytes, int64_t len, int32_t* keys, int64_t* lens, int64_t* payload_offs,
                         int64_t max_entries) {
  if (!bytes || len < 0 || max_entries < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  const char* why = nullptr;
  const int64_t n = javaser::parse_saved(bytes, len, keys, lens, payload_offs, max_entries, &why);
  if (n < 0) return fail(nullptr, IPLS_E_FORMAT, "saved model: %s", why ? why : "malformed");
  return n;
}

int64_t ipls_saved_encode(const int32_t* parts, int n_parts, const void* const* arrays, const int64_t* lens, int g_kind,
                          uint8_t* out, int64_t out_cap) {
  if (n_parts < 0 || (n_parts > 0 && (!parts || !lens))) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (g_kind != IPLS_HOST_F64 && g_kind != IPLS_HOST_BE) return fail(nullptr, IPLS_E_INVAL, "g_kind must be HOST_F64/BE");
  std::vector<int32_t> order;
  int32_t buckets, threshold;
  javaser::saved_shape(parts, n_parts, order, &buckets, &threshold);
  // key -> its first listing
  std::vector<int> at(order.size());
  for (size_t e = 0; e < order.size(); ++e) at[e] = int(std::find(parts, parts + n_parts, order[e]) - parts);
  int64_t total = order.empty() ? 82 : 1;
  for (size_t e = 0; e < order.size(); ++e) {
    const int64_t L = lens[at[e]];
    if (L < 0 || L > INT32_MAX || (L > 0 && out && (!arrays || !arrays[at[e]])))
      return fail(nullptr, IPLS_E_INVAL, "bad array %d", at[e]);
    total += (e == 0 ? 181 : 20) + 8 * L;
  }
  if (!out) return total;
  if (out_cap < total) return fail(nullptr, IPLS_E_RANGE, "saved model needs %lld bytes", (long long)total);
  if (order.empty()) return javaser::saved_empty(out);
  int64_t o = 0;
  for (size_t e = 0; e < order.size(); ++e) {
    uint8_t pre[javaser::kSavedPrefixMax];
    const int64_t L = lens[at[e]];
    const int64_t pl = javaser::saved_entry_prefix(pre, e == 0, threshold, buckets, (int32_t)order.size(), order[e], (int32_t)L);
    std::memcpy(out + o, pre, (size_t)pl);
    put_payload(out + o + pl, arrays ? arrays[at[e]] : nullptr, L, g_kind);
    o += pl + 8 * L;
  }
  out[o++] = 0x78;
  return o;
}

int64_t ipls_darr_parse(const uint8_t* bytes, int64_t len, int64_t* payload_off) {
  if (!bytes || len < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  const char* why = nullptr;
  const int64_t n = javaser::parse_darr(bytes, len, payload_off, &why);
  if (n < 0) return fail(nullptr, IPLS_E_FORMAT, "serialised double[]: %s", why ? why : "malformed");
  return n;
}

int64_t ipls_darr_encode(const void* g, int64_t n, int g_kind, uint8_t* out, int64_t out_cap) {
  if (n < 0 || n > INT32_MAX || (n > 0 && out && !g)) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (g_kind != IPLS_HOST_F64 && g_kind != IPLS_HOST_BE) return fail(nullptr, IPLS_E_INVAL, "g_kind must be HOST_F64/BE");
  const int64_t total = javaser::kDarrHeader + 8 * n;
  if (!out) return total;
  if (out_cap < total) return fail(nullptr, IPLS_E_RANGE, "serialised double[] needs %lld bytes", (long long)total);
  javaser::darr_header(out, (int32_t)n);
  put_payload(out + javaser::kDarrHeader, g, n, g_kind);
  return total;
}

int64_t ipls_dlist_parse(const uint8_t* bytes, int64_t len, double* values, int64_t max_values) {
  if (!bytes || len < 0 || max_values < 0) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  const char* why = nullptr;
  const int64_t n = javaser::parse_dlist(bytes, len, &why);
  if (n < 0) return fail(nullptr, IPLS_E_FORMAT, "serialised ArrayList<Double>: %s", why ? why : "malformed");
  for (int64_t i = 0; i < n; ++i) {
    const uint8_t* r = bytes + javaser::kDlistFirst + javaser::kDlistRecord * i;
    if (i > 0 && std::memcmp(r - 6, kDlistLead, 6) != 0)
      return fail(nullptr, IPLS_E_FORMAT, "serialised ArrayList<Double>: element %lld is not a Double", (long long)i);
    if (values && i < max_values) {
      uint64_t v;
      std::memcpy(&v, r, 8);
      v = __builtin_bswap64(v);
      std::memcpy(values + i, &v, 8);
    }
  }
  return n;
}

int64_t ipls_dlist_encode(const void* g, int64_t n, int g_kind, uint8_t* out, int64_t out_cap) {
  if (n < 0 || n > INT32_MAX || (n > 0 && out && !g)) return fail(nullptr, IPLS_E_INVAL, "bad argument");
  if (g_kind != IPLS_HOST_F64 && g_kind != IPLS_HOST_BE) return fail(nullptr, IPLS_E_INVAL, "g_kind must be HOST_F64/BE");
  const int64_t total = javaser::dlist_total(n);
  if (!out) return total;
  if (out_cap < total) return fail(nullptr, IPLS_E_RANGE, "serialised list needs %lld bytes", (long long)total);
  int64_t o = javaser::dlist_header(out, (int32_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (i > 0) {
      std::memcpy(out + o, kDlistLead, 6);
      o += 6;
    }
    uint64_t v;
    std::memcpy(&v, (const char*)g + 8 * i, 8);
    if (g_kind == IPLS_HOST_BE) v = __builtin_bswap64(v);
    v = __builtin_bswap64(canon_bits(v));
    std::memcpy(out + o, &v, 8);
    o += 8;
  }
  out[o++] = 0x78;
  return o;
}

int64_t dev_commit_partial(ipls_dev* h, int p, int32_t workers, uint8_t* out, int64_t out_cap) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  const int64_t L = h->len[p];
  const int64_t hl = javaser::pair_header_len(), total = hl + 8 * L + javaser::pair_trailer_len();
  if (!out) return total;
  if (out_cap < total) return fail(h, IPLS_E_RANGE, "partial update needs %lld bytes", (long long)total);
  HIP_TRY(h, dev_use(h->device));
  javaser::write_pair_header(out, workers, (int32_t)L);
  if (h->agg_zero[p]) {
    std::memset(out + hl, 0, (size_t)L * 8);   // +0.0 in any byte order
  } else {
    if (int rc = be_to_host(h, out + hl, h->arena + h->agg_off[p], L)) return rc;
  }
  javaser::write_pair_trailer(out + hl + 8 * L);
  return total;
}

int64_t dev_merge_files(ipls_dev* h, const uint8_t* const* files, const int64_t* lens, int k, int file_kind,
                             uint8_t* out, int64_t out_cap) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (k < 1 || !files || !lens) return fail(h, IPLS_E_INVAL, "need at least one file");
  if (file_kind != IPLS_HOST_BE && file_kind != IPLS_HOST_PAIR) return fail(h, IPLS_E_INVAL, "file_kind BE or PAIR");
  // decode every file's payload position first (GetParameters / Download_Partial_Updates)
  std::vector<int64_t> nd(k), off(k);
  for (int i = 0; i < k; ++i) {
    if (!files[i] && lens[i] > 0) return fail(h, IPLS_E_INVAL, "file %d is NULL", i);
    if (file_kind == IPLS_HOST_BE) {
      nd[i] = lens[i] / 8;
      off[i] = 0;
    } else {
      int32_t w;
      const char* why = nullptr;
      nd[i] = javaser::parse_pair(files[i], lens[i], &w, &off[i], &why);
      if (nd[i] < 0) return fail(h, IPLS_E_FORMAT, "file %d: %s (ObjectInputStream)", i, why ? why : "malformed");
    }
    if (i > 0 && nd[i] > nd[0])   // Aggregation[j] += Gradient[j] for j < Gradient.length (:244-246)
      return fail(h, IPLS_E_RANGE, "file %d has %lld doubles > %lld of the first "
                  "(ArrayIndexOutOfBoundsException, Decentralized_Storage_Receiver.java:245)", i,
                  (long long)nd[i], (long long)nd[0]);
  }
  const int64_t n0 = nd[0];
  if (out_cap < 8 * n0 || (!out && n0 > 0)) return fail(h, IPLS_E_RANGE, "merge output needs %lld bytes", (long long)(8 * n0));
  if (n0 == 0) return 0;
  HIP_TRY(h, dev_use(h->device));
  if (h->merge_cap < n0) {
    if (h->d_merge) {
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      HIP_TRY(h, hipFree(h->d_merge));
      h->d_merge = nullptr;
      h->merge_cap = 0;
    }
    HIP_TRY(h, hipMalloc(&h->d_merge, (size_t)n0 * 8));
    h->merge_cap = n0;
  }
  for (int i = 0; i < k; ++i) {
    if (nd[i] == 0) continue;
    if (int rc = to_scratch(h, files[i] + off[i], (size_t)nd[i] * 8)) return rc;
    // (both device buffers come from hipMalloc: the tile shape)
    const bool vec = al16(h->d_merge) && al16(h->d_scratch);
    const dim3 g = ew_grid(nd[i], vec, 4096);
    auto msrc = (const unsigned long long*)h->d_scratch;
    with_bool(i == 0, [&](auto first) {   // Aggregation = GetParameters(Hashes.get(0)): the first file as is
      with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((k_fold_n<true, decltype(first)::value, decltype(v)::value>), g, dim3(kBlock), 0, h->stream,
                           h->d_merge, msrc, nd[i]);
      });
    });
    HIP_TRY(h, hipGetLastError());
  }
  // update_file(..., Aggregation): putDouble per element (MyIPFSClass.java:105-116)
  if (int rc = be_to_host(h, out, h->d_merge, n0)) return rc;
  return 8 * n0;
}

int64_t ipls_frame_encode(const double* g, int64_t n, int g_kind, int32_t a, int32_t b, int16_t pid,
                          const uint8_t* origin, int32_t origin_len, uint8_t* out, int64_t out_cap) {
  if (n < 0 || n > INT32_MAX || origin_len < 0 || !out || (n > 0 && !g) || (origin_len > 0 && !origin))
    return fail(nullptr, IPLS_E_INVAL, "bad argument");
  const int64_t total = 14 + 8 * n + origin_len;
  if (out_cap < total) return fail(nullptr, IPLS_E_RANGE, "frame needs %lld bytes", (long long)total);
  out[0] = (uint8_t)((uint16_t)pid >> 8);
  out[1] = (uint8_t)pid;
  const uint32_t hv[3] = {(uint32_t)n, (uint32_t)a, (uint32_t)b};
  for (int f = 0; f < 3; ++f)
    for (int i = 0; i < 4; ++i) out[2 + 4 * f + i] = (uint8_t)(hv[f] >> (24 - 8 * i));
  if (n > 0) {
    std::vector<double> tmp;
    const double* src = g;
    if (g_kind == IPLS_DEV_F64) {
      tmp.resize(n);
      if (hipMemcpy(tmp.data(), g, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(nullptr, IPLS_E_DEVICE, "frame encode D2H failed");
      src = tmp.data();
    } else if (g_kind != IPLS_HOST_F64) {
      return fail(nullptr, IPLS_E_INVAL, "g_kind must be HOST_F64 or DEV_F64");
    }
    for (int64_t i = 0; i < n; ++i) {  // putDouble(14 + 8i, g[i]) -- raw bits, BE
      uint64_t v;
      std::memcpy(&v, &src[i], 8);
      v = __builtin_bswap64(v);
      std::memcpy(out + 14 + 8 * i, &v, 8);
    }
  }
  if (origin_len) std::memcpy(out + 14 + 8 * n, origin, (size_t)origin_len);
  return total;
}

// ---- Marshall_Packet of an accumulator, encoded on the device (a9) ----
// IPLS.java:1429-1430 publishes the aggregator's partial sum as
// Marshall_Packet(Aggregated_Gradients[p], id, iteration, workers + 1, 3):
// the frame (MyIPFSClass.java:990-1013) base64url-encoded with padding
// (:1016).  The text is produced by k_b64url_encode_frame straight from the
// accumulator: no host pass over the doubles, no blocking copy of them.
int64_t dev_publish(ipls_dev* h, int p, int target, int32_t a, int32_t b, int16_t pid, const uint8_t* origin,
                    int32_t origin_len, void* out, int64_t out_cap, int out_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (int rc = check_part(h, p)) return rc;
  if (target_off(h, p, target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  if (origin_len < 0 || (origin_len > 0 && !origin)) return fail(h, IPLS_E_INVAL, "bad origin");
  if (out_kind != IPLS_HOST_TEXT && out_kind != IPLS_DEV_TEXT) return fail(h, IPLS_E_INVAL, "out_kind HOST_TEXT/DEV_TEXT");
  const int64_t n = h->len[p];
  const int64_t F = 14 + 8 * n + origin_len;
  const int64_t T = pubsub::b64_enc_len(F);
  if (!out) return T;
  if (out_cap < T) return fail(h, IPLS_E_RANGE, "publish text needs %lld bytes", (long long)T);
  HIP_TRY(h, dev_use(h->device));
  FrameEnc fe{};
  const uint32_t hv[3] = {(uint32_t)n, (uint32_t)a, (uint32_t)b};
  fe.hdr[0] = (unsigned char)((uint16_t)pid >> 8);   // putShort(0, pid)
  fe.hdr[1] = (unsigned char)pid;
  for (int f = 0; f < 3; ++f)                        // putInt(2 | 6 | 10, ...)
    for (int i = 0; i < 4; ++i) fe.hdr[2 + 4 * f + i] = (unsigned char)(hv[f] >> (24 - 8 * i));
  fe.n = n;
  fe.origin_len = origin_len;
  fe.origin = nullptr;
  if (origin_len > 0) {
    void* d = nullptr;
    if (int rc = upload_table(h, origin, (size_t)origin_len, &d)) return rc;
    fe.origin = (const unsigned char*)d;
  }
  uint8_t* zf = zero_flag(h, p, target);
  const unsigned long long* src =
      (zf && *zf) ? nullptr : (const unsigned long long*)(h->arena + target_off(h, p, target));
  unsigned char* dst = (unsigned char*)out;
  if (out_kind == IPLS_DEV_TEXT && !kernel_writable(out))
    return fail(h, IPLS_E_INVAL, "DEV_TEXT output is neither device memory nor pinned host memory");
  const bool dev_direct = out_kind == IPLS_DEV_TEXT && !((uintptr_t)out & 15);
  if (!dev_direct) {
    if (int rc = ensure_scratch(h, (size_t)T + 64)) return rc;
    dst = (unsigned char*)h->d_scratch;
  }
  const int64_t groups = (F + 23) / 24;
  hipLaunchKernelGGL(k_b64url_encode_frame, dim3(std::max(1u, std::min<unsigned>(blocks_for(groups, kBlock), 16384))),
                     dim3(kBlock), 0, h->stream, fe, src, dst, groups, T);
  HIP_TRY(h, hipGetLastError());
  if (out_kind == IPLS_DEV_TEXT) {
    // stream-ordered like every device-only call (the origin bytes were
    // already copied into the pinned upload ring)
    if (!dev_direct) HIP_TRY(h, hipMemcpyAsync(out, dst, (size_t)T, hipMemcpyDeviceToDevice, h->stream));
    return T;
  }
  if (int rc = d2h(h, out, dst, (size_t)T)) return rc;
  return T;
}

// Several partitions' publish texts in one launch (the loop over Auth_List,
// IPLS.java:1423-1431): text i of local partition parts[i] (field b = b[i])
// lands at out + offs[i], lens[i] bytes; offs are 64-byte multiples (the
// front lays them out).  HOST_TEXT: one D2H per text after the launch.
int64_t dev_publish_many(ipls_dev* h, int n, const int* parts, int target, int32_t a, const int32_t* b, int16_t pid,
                         const uint8_t* origin, int32_t origin_len, void* out, const int64_t* offs,
                         const int64_t* lens, int out_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n <= 0) return IPLS_OK;
  if (origin_len < 0 || (origin_len > 0 && !origin)) return fail(h, IPLS_E_INVAL, "bad origin");
  if (out_kind != IPLS_HOST_TEXT && out_kind != IPLS_DEV_TEXT) return fail(h, IPLS_E_INVAL, "out_kind HOST_TEXT/DEV_TEXT");
  for (int i = 0; i < n; ++i) {
    if (int rc = check_part(h, parts[i])) return rc;
    if (target_off(h, parts[i], target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
  }
  HIP_TRY(h, dev_use(h->device));
  if (out_kind == IPLS_DEV_TEXT && !kernel_writable(out))
    return fail(h, IPLS_E_INVAL, "DEV_TEXT output is neither device memory nor pinned host memory");
  const unsigned char* dorig = nullptr;
  if (origin_len > 0) {
    void* d = nullptr;
    if (int rc = upload_table(h, origin, (size_t)origin_len, &d)) return rc;
    dorig = (const unsigned char*)d;
  }
  // texts land straight in a 16-B aligned device buffer; else in the scratch
  // buffer at the same offsets, then copied out
  const bool direct = out_kind == IPLS_DEV_TEXT && !((uintptr_t)out & 15);
  int64_t span = 0;
  for (int i = 0; i < n; ++i) span = std::max(span, offs[i] + lens[i]);
  int64_t lo = span;
  for (int i = 0; i < n; ++i) lo = std::min(lo, offs[i]);
  unsigned char* base = (unsigned char*)out;
  if (!direct) {
    if (int rc = ensure_scratch(h, (size_t)(span - lo) + 64)) return rc;
    base = (unsigned char*)h->d_scratch - lo;
  }
  std::vector<FrameJob> jobs(n);
  int64_t max_groups = 1;
  for (int i = 0; i < n; ++i) {
    const int p = parts[i];
    FrameJob& j = jobs[i];
    j = FrameJob{};
    const int64_t L = h->len[p];
    const uint32_t hv[3] = {(uint32_t)L, (uint32_t)a, (uint32_t)b[i]};
    j.f.hdr[0] = (unsigned char)((uint16_t)pid >> 8);   // putShort(0, pid)
    j.f.hdr[1] = (unsigned char)pid;
    for (int f = 0; f < 3; ++f)                         // putInt(2 | 6 | 10, ...)
      for (int k = 0; k < 4; ++k) j.f.hdr[2 + 4 * f + k] = (unsigned char)(hv[f] >> (24 - 8 * k));
    j.f.n = L;
    j.f.origin_len = origin_len;
    j.f.origin = dorig;
    uint8_t* zf = zero_flag(h, p, target);
    j.src = (zf && *zf) ? nullptr : (const unsigned long long*)(h->arena + target_off(h, p, target));
    j.out = base + offs[i];
    j.groups = (14 + 8 * L + origin_len + 23) / 24;
    j.text_len = lens[i];
    max_groups = std::max(max_groups, j.groups);
  }
  void* djobs = nullptr;
  if (int rc = upload_table(h, jobs.data(), jobs.size() * sizeof(FrameJob), &djobs)) return rc;
  const unsigned gx = std::max(1u, std::min<unsigned>(blocks_for(max_groups, kBlock), 16384));
  hipLaunchKernelGGL(k_b64url_encode_frames, dim3(gx, (unsigned)n), dim3(kBlock), 0, h->stream,
                     (const FrameJob*)djobs);
  HIP_TRY(h, hipGetLastError());
  if (direct) return IPLS_OK;                           // stream-ordered
  const hipMemcpyKind kind = out_kind == IPLS_DEV_TEXT ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (int i = 0; i < n; ++i)
    HIP_TRY(h, hipMemcpyAsync((unsigned char*)out + offs[i], base + offs[i], (size_t)lens[i], kind, h->stream));
  if (out_kind == IPLS_HOST_TEXT) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

// ---- SendGradients: a flat gradient's partitions as pubsub texts (k_b64url_encode_flat) ----
// IPLS.java:1350-1400 -> Send_Gradient_Partition (:1290-1322, direct mode): for every partition the peer does not
// own, Marshall_Packet(OrganizeGradients(g)[p], id, p, middleware_iteration, 3) under Base64.getUrlEncoder.  One
// launch reads the listed partitions' values where they lie in the flat vector (doubles, big-endian doubles or a
// trainer format, at any element offset), generates the count slot and the zero tail, and writes the texts: no
// split to host doubles, no host frame, no host base64 pass.
namespace {
void frame_header(unsigned char* hdr, int16_t pid, int64_t n, int32_t a, int32_t b) {
  const uint32_t hv[3] = {(uint32_t)n, (uint32_t)a, (uint32_t)b};
  hdr[0] = (unsigned char)((uint16_t)pid >> 8);        // putShort(0, pid)
  hdr[1] = (unsigned char)pid;
  for (int f = 0; f < 3; ++f)                          // putInt(2 | 6 | 10, ...)
    for (int k = 0; k < 4; ++k) hdr[2 + 4 * f + k] = (unsigned char)(hv[f] >> (24 - 8 * k));
}
// Base64.getUrlEncoder ('=' padding) of n bytes on the host: the 14-byte frames of a null gradient
void b64url_host(const unsigned char* in, int64_t n, unsigned char* out) {
  static const char tab[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
  for (int64_t i = 0; i < n; i += 3, out += 4) {
    const int nb = n - i >= 3 ? 3 : (int)(n - i);
    const unsigned v = (unsigned)in[i] << 16 | (nb > 1 ? (unsigned)in[i + 1] << 8 : 0u) | (nb > 2 ? (unsigned)in[i + 2] : 0u);
    out[0] = (unsigned char)tab[v >> 18];
    out[1] = (unsigned char)tab[(v >> 12) & 63];
    out[2] = nb > 1 ? (unsigned char)tab[(v >> 6) & 63] : (unsigned char)'=';
    out[3] = nb > 2 ? (unsigned char)tab[v & 63] : (unsigned char)'=';
  }
}
}  // namespace

int64_t dev_send_many(ipls_dev* h, const void* flat, int64_t n, int src_kind, int n_parts, const int* parts,
                      int32_t iteration, int16_t pid, const uint8_t* origin, int32_t origin_len, void* out,
                      const int64_t* offs, const int64_t* lens, int out_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  // the shard's scratch buffer and stream; no accumulator, zero flag or queue is read or written, so queued
  // arrivals stay queued (no IPLS_LOCK flush)
  std::lock_guard<std::mutex> lk_(h->mu);
  if (n_parts <= 0) return IPLS_OK;
  if (origin_len < 0 || (origin_len > 0 && !origin)) return fail(h, IPLS_E_INVAL, "bad origin");
  if (out_kind != IPLS_HOST_TEXT && out_kind != IPLS_DEV_TEXT) return fail(h, IPLS_E_INVAL, "out_kind HOST_TEXT/DEV_TEXT");
  for (int i = 0; i < n_parts; ++i)
    if (int rc = check_part(h, parts[i])) return rc;
  // OrganizeGradients splits every partition before anything is sent (IPLS.java:1030)
  std::vector<int64_t> nc(h->P, 0);
  if (flat)
    for (int p = 0; p < h->P; ++p)
      if (int rc = split_bounds(h, p, n, &nc[p])) return rc;
  HIP_TRY(h, dev_use(h->device));
  if (out_kind == IPLS_DEV_TEXT && !kernel_writable(out))
    return fail(h, IPLS_E_INVAL, "DEV_TEXT output is neither device memory nor pinned host memory");
  if (!flat) {
    // "did not train in time" (IPLS.java:1306-1312): Marshall_Packet(null, ...), n = 0, the header and the origin
    std::vector<unsigned char> frame((size_t)(14 + origin_len)), text;
    if (origin_len) std::memcpy(frame.data() + 14, origin, (size_t)origin_len);
    for (int i = 0; i < n_parts; ++i) {
      frame_header(frame.data(), pid, 0, h->p_lo + parts[i], iteration);
      text.resize((size_t)lens[i]);
      b64url_host(frame.data(), (int64_t)frame.size(), text.data());
      if (out_kind == IPLS_HOST_TEXT) std::memcpy((unsigned char*)out + offs[i], text.data(), text.size());
      else if (int rc = stage_h2d(h, (unsigned char*)out + offs[i], text.data(), text.size())) return rc;
    }
    return IPLS_OK;
  }
  op::Resolved sv;
  if (op::resolve(op::kSplit, flat, n, src_kind, 0, &sv) != op::kTake) return not_taken(h, sv.why);
  const Fmt fmt = fmt_trainer(sv.fmt) ? sv.fmt : kFmtF64;
  const bool be_in = sv.fmt == kFmtBE;
  const int64_t esz = fmt_size(fmt);
  const unsigned char* dorig = nullptr;
  if (origin_len > 0) {
    void* d = nullptr;
    if (int rc = upload_table(h, origin, (size_t)origin_len, &d)) return rc;
    dorig = (const unsigned char*)d;
  }
  // texts land straight in a 16-B aligned device buffer; else in the scratch buffer at the same offsets, then
  // copied out.  A host source is staged behind them: only the bytes from the first listed partition's first
  // value to the last one's last value cross PCIe.
  const bool direct = out_kind == IPLS_DEV_TEXT && !((uintptr_t)out & 15);
  int64_t span = 0;
  for (int i = 0; i < n_parts; ++i) span = std::max(span, offs[i] + lens[i]);
  int64_t lo = span;
  for (int i = 0; i < n_parts; ++i) lo = std::min(lo, offs[i]);
  const int64_t text_bytes = direct ? 0 : align_up(span - lo + 64, 256);
  int64_t s_lo = INT64_MAX, s_hi = 0;   // the listed values' range in the flat vector, in elements
  for (int i = 0; i < n_parts; ++i) {
    const int p = parts[i];
    if (nc[p] == 0) continue;
    s_lo = std::min(s_lo, h->flat_off[p]);
    s_hi = std::max(s_hi, h->flat_off[p] + nc[p]);
  }
  if (s_hi == 0) s_lo = 0;
  const int64_t src_bytes = sv.host ? (s_hi - s_lo) * esz : 0;
  if (text_bytes + src_bytes > 0)
    if (int rc = ensure_scratch(h, (size_t)(text_bytes + src_bytes))) return rc;
  unsigned char* base = direct ? (unsigned char*)out : (unsigned char*)h->d_scratch - lo;
  const char* d = (const char*)flat;   // device memory is read in place
  int64_t d_first = 0;                 // the flat offset of d's first element
  if (sv.host) {
    d = (const char*)h->d_scratch + text_bytes;
    d_first = s_lo;
    if (int rc = stage_h2d(h, (void*)d, (const char*)flat + esz * s_lo, (size_t)src_bytes)) return rc;
  }
  std::vector<FlatEncJob> jobs((size_t)n_parts);
  int64_t max_groups = 1;
  bool any_fast = false;
  for (int i = 0; i < n_parts; ++i) {
    const int p = parts[i];
    FlatEncJob& j = jobs[(size_t)i];
    j = FlatEncJob{};
    const int64_t L = h->len[p];
    frame_header(j.hdr, pid, L, h->p_lo + p, iteration);
    j.L = L;
    j.ncopy = nc[p];
    j.lo = nc[p] ? h->flat_off[p] - d_first : 0;
    j.origin_len = origin_len;
    j.origin = dorig;
    j.out = base + offs[i];
    j.groups = (14 + 8 * L + origin_len + 23) / 24;
    j.text_len = lens[i];
    max_groups = std::max(max_groups, j.groups);
    any_fast = any_fast || nc[p] >= 5;   // lane 1's values 1 .. 4 lie below ncopy
  }
  void* djobs = nullptr;
  if (int rc = upload_table(h, jobs.data(), jobs.size() * sizeof(FlatEncJob), &djobs)) return rc;
  const unsigned gx = std::max(1u, std::min<unsigned>(blocks_for(max_groups, kBlock), 16384));
  const dim3 grid(gx, (unsigned)n_parts);
  if (fmt_trainer(fmt))
    with_narrow(fmt, [&](auto s) {
      typedef decltype(s) S;
      hipLaunchKernelGGL((k_b64url_encode_flat<S, false>), grid, dim3(kBlock), 0, h->stream, (const FlatEncJob*)djobs,
                         (const typename S::elem*)d);
    });
  else
    with_bool(be_in, [&](auto bi) {
      hipLaunchKernelGGL((k_b64url_encode_flat<FmtD64, decltype(bi)::value>), grid, dim3(kBlock), 0, h->stream,
                         (const FlatEncJob*)djobs, (const unsigned long long*)d);
    });
  HIP_TRY(h, hipGetLastError());
  h->last_launch = launch_info(IPLS_KERNEL_ENCODE_FLAT, 0, kBlock, 4, any_fast ? 1 : 0, 0, (int64_t)gx * n_parts, be_in,
                               false, 0);
  if (direct) return IPLS_OK;                           // stream-ordered
  const hipMemcpyKind kind = out_kind == IPLS_DEV_TEXT ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (int i = 0; i < n_parts; ++i)
    HIP_TRY(h, hipMemcpyAsync((unsigned char*)out + offs[i], base + offs[i], (size_t)lens[i], kind, h->stream));
  if (out_kind == IPLS_HOST_TEXT) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

// ---- the segment-list calls (engine.hpp; seg_plan.hpp plans, seg_kernels.hpp runs) ----
namespace {
// Several tables of one launch in one upload: each starts 16-B aligned.
struct TablePack {
  std::vector<unsigned char> bytes;
  template <class T>
  size_t add(const T* v, size_t n) {
    const size_t at = (bytes.size() + 15) / 16 * 16;
    bytes.resize(at + std::max<size_t>(n * sizeof(T), 16));
    if (n) std::memcpy(bytes.data() + at, v, n * sizeof(T));
    return at;
  }
};

segplan::Geometry seg_geometry(const ipls_dev* h) {
  segplan::Geometry g;
  g.P = h->P;
  g.chunk = h->chunk;
  g.off = h->flat_off.data();
  g.len = h->len.data();
  g.flat_base = h->flat_base;
  g.flat_total = h->flat_total;
  return g;
}
std::vector<segplan::Seg> seg_table(const seg_ref* segs, int n_segs) {
  std::vector<segplan::Seg> v((size_t)std::max(n_segs, 0));
  for (int s = 0; s < n_segs; ++s) {
    v[(size_t)s].n = segs[s].n;
    v[(size_t)s].fmt = segs[s].fmt;
    v[(size_t)s].mod = (int)((uintptr_t)segs[s].ptr & 127);
  }
  return v;
}
std::vector<SegPiece> seg_pieces(const segplan::Plan& pl, const seg_ref* segs) {
  std::vector<SegPiece> v(pl.pieces.size());
  for (size_t k = 0; k < v.size(); ++k) {
    const segplan::Piece& p = pl.pieces[k];
    const seg_ref& sg = segs[p.seg];
    v[k] = SegPiece{p.dst, p.n, (const char*)sg.ptr + p.src * segplan::fmt_esz(sg.fmt), sg.fmt};
  }
  return v;
}
// The difference calls: per piece, its first SUBTRAHEND element (the plan is the minuend list's).
std::vector<const void*> seg_pieces_b(const segplan::Plan& pl, const seg_ref* segs, const void* const* b_ptrs) {
  std::vector<const void*> v(pl.pieces.size());
  for (size_t k = 0; k < v.size(); ++k) {
    const segplan::Piece& p = pl.pieces[k];
    v[k] = (const char*)b_ptrs[p.seg] + p.src * segplan::fmt_esz(segs[p.seg].fmt);
  }
  return v;
}
// a plan's refusal as the call's (the front has refused a bad table before)
int seg_plan_rc(ipls_dev* h, const segplan::Plan& pl) {
  switch (pl.status) {
    case segplan::kOk: return IPLS_OK;
    case segplan::kOverrun:
      return fail(h, IPLS_E_RANGE, "gradient list of %lld values overruns partition %d (ArrayIndexOutOfBounds, IPLS.java:1030)",
                  (long long)pl.n, h->p_lo + pl.bad);
    case segplan::kBadPartition: return fail(h, IPLS_E_RANGE, "partition %d out of range [0,%d)", pl.bad, h->P);
    case segplan::kShort:
      return fail(h, IPLS_E_RANGE, "output list of %lld < model size %lld", (long long)pl.n, (long long)h->flat_total);
    default: return fail(h, IPLS_E_INVAL, "bad segment list");
  }
}
}  // namespace

// b_ptrs: null, or the subtrahend list of a difference call (one pointer per segment, lengths and formats segs')
static int update_segs(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs, const int32_t* owned,
                       int n_owned) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  const segplan::Plan pl = segplan::plan_update(seg_geometry(h), tab.data(), n_segs, owned, n_owned, kSegTile);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  if (n_owned == 0) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  const std::vector<SegPiece> pieces = seg_pieces(pl, segs);
  std::vector<const void*> bsrc;
  if (b_ptrs) bsrc = seg_pieces_b(pl, segs, b_ptrs);
  for (const segplan::Launch& l : pl.launches) {
    std::vector<SegJob> jobs(l.jobs.size());
    bool all_zero = true;
    for (size_t j = 0; j < jobs.size(); ++j) {
      const int q = l.jobs[j].q;
      jobs[j] = SegJob{(unsigned long long*)(h->arena + h->agg_off[q]), l.jobs[j].ncopy, l.jobs[j].L, h->agg_zero[q]};
      all_zero = all_zero && h->agg_zero[q];
    }
    TablePack pack;
    const size_t at_items = pack.add(l.items.data(), l.items.size());
    const size_t at_jobs = pack.add(jobs.data(), jobs.size());
    const size_t at_pieces = pack.add(pieces.data(), pieces.size());
    const size_t at_bsrc = b_ptrs ? pack.add(bsrc.data(), bsrc.size()) : 0;
    void* d = nullptr;
    if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &d)) return rc;
    const char* dt = (const char*)d;
    if (b_ptrs)
      hipLaunchKernelGGL(k_update_segs_diff, dim3((unsigned)l.items.size()), dim3(kBlock), 0, h->stream,
                         (const segplan::Item*)(dt + at_items), (const SegJob*)(dt + at_jobs),
                         (const SegPiece*)(dt + at_pieces), (const void* const*)(dt + at_bsrc));
    else
      hipLaunchKernelGGL(k_update_segs, dim3((unsigned)l.items.size()), dim3(kBlock), 0, h->stream,
                         (const segplan::Item*)(dt + at_items), (const SegJob*)(dt + at_jobs),
                         (const SegPiece*)(dt + at_pieces));
    HIP_TRY(h, hipGetLastError());
    for (const segplan::Job& j : l.jobs) h->agg_zero[j.q] = 0;
    h->last_launch = launch_info(b_ptrs ? IPLS_KERNEL_UPDATE_SEGS_DIFF : IPLS_KERNEL_UPDATE_SEGS, 0, kBlock, kSegV,
                                 l.any_whole ? 1 : 0, 0, (int64_t)l.items.size(), false, false,
                                 all_zero ? kZero : kAccum);
  }
  return IPLS_OK;
}

int dev_update_gradient_segs(ipls_dev* h, const seg_ref* segs, int n_segs, const int32_t* owned, int n_owned) {
  return update_segs(h, segs, nullptr, n_segs, owned, n_owned);
}
int dev_update_gradient_segs_diff(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs,
                                  const int32_t* owned, int n_owned) {
  if (n_segs > 0 && !b_ptrs) return fail(h, IPLS_E_INVAL, "null subtrahend list");
  static const void* const none[1] = {nullptr};
  return update_segs(h, segs, b_ptrs ? b_ptrs : none, n_segs, owned, n_owned);
}

// The peer-list call: K lists in one launch.  The plan is made over `owned` without its repeats (so it has one
// launch); how often a partition stood in `owned` goes into its job, and the kernel adds every peer's value that
// often in a row -- the bits of K twin calls whose repeat levels run inside each call.
int dev_update_gradient_segs_peers(ipls_dev* h, const seg_ref* segs, bool diff, const void* const* t_ptrs, int n_peers,
                                   int n_segs, const int32_t* owned, int n_owned) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_peers < 1 || !t_ptrs) return fail(h, IPLS_E_INVAL, "bad peer list");
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  std::vector<int32_t> uniq;                          // owned without repeats, in order of first appearance
  std::vector<int32_t> mult((size_t)h->P, 0);
  bool listed = n_owned >= 0 && (n_owned == 0 || owned);
  for (int i = 0; listed && i < n_owned; ++i) {
    listed = owned[i] >= 0 && owned[i] < h->P;
    if (listed && mult[(size_t)owned[i]]++ == 0) uniq.push_back(owned[i]);
  }
  // a list the plan refuses goes to it as it came
  const segplan::Plan pl = listed ? segplan::plan_update(seg_geometry(h), tab.data(), n_segs, uniq.data(),
                                                         (int)uniq.size(), kSegTile)
                                  : segplan::plan_update(seg_geometry(h), tab.data(), n_segs, owned, n_owned, kSegTile);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  if (n_owned == 0) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  const segplan::Launch& l = pl.launches[0];          // no repeats: one launch
  const std::vector<SegPiece> pieces = seg_pieces(pl, segs);
  std::vector<const void*> psrc(pieces.size() * (size_t)n_peers);
  for (size_t k = 0; k < pieces.size(); ++k) {
    const segplan::Piece& p = pl.pieces[k];
    const int64_t at = p.src * segplan::fmt_esz(segs[p.seg].fmt);
    for (int q = 0; q < n_peers; ++q)
      psrc[k * (size_t)n_peers + (size_t)q] = (const char*)t_ptrs[(size_t)q * (size_t)n_segs + (size_t)p.seg] + at;
  }
  std::vector<SegPeersJob> jobs(l.jobs.size());
  bool all_zero = true;
  for (size_t j = 0; j < jobs.size(); ++j) {
    const int q = l.jobs[j].q;
    jobs[j] = SegPeersJob{(unsigned long long*)(h->arena + h->agg_off[q]), l.jobs[j].ncopy, l.jobs[j].L,
                          h->agg_zero[q] ? 1 : 0, mult[(size_t)q]};
    all_zero = all_zero && h->agg_zero[q];
  }
  TablePack pack;
  const size_t at_items = pack.add(l.items.data(), l.items.size());
  const size_t at_jobs = pack.add(jobs.data(), jobs.size());
  const size_t at_pieces = pack.add(pieces.data(), pieces.size());
  const size_t at_psrc = pack.add(psrc.data(), psrc.size());
  void* d = nullptr;
  if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &d)) return rc;
  const char* dt = (const char*)d;
  with_bool(diff, [&](auto df) {
    hipLaunchKernelGGL((k_update_segs_peers<decltype(df)::value>), dim3((unsigned)l.items.size()), dim3(kBlock), 0,
                       h->stream, (const segplan::Item*)(dt + at_items), (const SegPeersJob*)(dt + at_jobs),
                       (const SegPiece*)(dt + at_pieces), (const void* const*)(dt + at_psrc), n_peers);
  });
  HIP_TRY(h, hipGetLastError());
  for (const segplan::Job& j : l.jobs) h->agg_zero[j.q] = 0;
  h->last_launch = launch_info(IPLS_KERNEL_UPDATE_SEGS_PEERS, 0, kBlock, kSegV, l.any_whole ? 1 : 0, 0,
                               (int64_t)l.items.size(), false, false, all_zero ? kZero : kAccum);
  return IPLS_OK;
}

int dev_get_partitions_segs(ipls_dev* h, const seg_ref* segs, int n_segs) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  const segplan::Plan pl = segplan::plan_divide(seg_geometry(h), tab.data(), n_segs, kSegTile);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  const segplan::Launch& l = pl.launches[0];
  if (l.items.empty()) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  std::vector<void*> outs((size_t)n_segs);
  for (int s = 0; s < n_segs; ++s) outs[(size_t)s] = const_cast<void*>(segs[s].ptr);
  std::vector<SegDivPart> parts((size_t)h->P);
  for (int q = 0; q < h->P; ++q) parts[(size_t)q] = SegDivPart{h->arena + h->w_off[q], h->len[q]};
  TablePack pack;
  const size_t at_items = pack.add(l.items.data(), l.items.size());
  const size_t at_outs = pack.add(outs.data(), outs.size());
  const size_t at_parts = pack.add(parts.data(), parts.size());
  void* d = nullptr;
  if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &d)) return rc;
  const char* dt = (const char*)d;
  with_bool(h->secure != 0, [&](auto sec) {
    hipLaunchKernelGGL((k_divide_segs<decltype(sec)::value>), dim3((unsigned)l.items.size()), dim3(kBlock), 0,
                       h->stream, (const segplan::Item*)(dt + at_items), (void* const*)(dt + at_outs),
                       (const SegDivPart*)(dt + at_parts), h->chunk, (int64_t)h->p_lo);
  });
  HIP_TRY(h, hipGetLastError());
  h->last_launch = launch_info(IPLS_KERNEL_DIVIDE_SEGS, 0, kBlock, kSegV, l.any_whole ? 1 : 0, 0,
                               (int64_t)l.items.size(), false, false, 0);
  return IPLS_OK;
}

// The output-copy-list call: n_lists lists written by one launch.  The plan is the twin's, made from list 0's
// addresses (segs); the pointer tables of all the lists travel as one [n_lists][n_segs] array in the same upload.
int dev_get_partitions_segs_copies(ipls_dev* h, const seg_ref* segs, void* const* o_ptrs, int n_lists, int n_segs) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_lists < 1 || (n_segs > 0 && !o_ptrs)) return fail(h, IPLS_E_INVAL, "bad output copy list");
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  const segplan::Plan pl = segplan::plan_divide(seg_geometry(h), tab.data(), n_segs, kSegTile);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  const segplan::Launch& l = pl.launches[0];
  if (l.items.empty()) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  std::vector<SegDivPart> parts((size_t)h->P);
  for (int q = 0; q < h->P; ++q) parts[(size_t)q] = SegDivPart{h->arena + h->w_off[q], h->len[q]};
  TablePack pack;
  const size_t at_items = pack.add(l.items.data(), l.items.size());
  const size_t at_outs = pack.add(o_ptrs, (size_t)n_lists * (size_t)n_segs);
  const size_t at_parts = pack.add(parts.data(), parts.size());
  void* d = nullptr;
  if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &d)) return rc;
  const char* dt = (const char*)d;
  with_bool(h->secure != 0, [&](auto sec) {
    hipLaunchKernelGGL((k_divide_segs_copies<decltype(sec)::value>), dim3((unsigned)l.items.size()), dim3(kBlock), 0,
                       h->stream, (const segplan::Item*)(dt + at_items), (void* const*)(dt + at_outs), n_lists, n_segs,
                       (const SegDivPart*)(dt + at_parts), h->chunk, (int64_t)h->p_lo);
  });
  HIP_TRY(h, hipGetLastError());
  h->last_launch = launch_info(IPLS_KERNEL_DIVIDE_SEGS_COPIES, 0, kBlock, kSegV, l.any_whole ? 1 : 0, 0,
                               (int64_t)l.items.size(), false, false, 0);
  return IPLS_OK;
}

// The many-trainers round: the fold of the peer-list call, W = AGG + REP and the divide of the output-copy-list call
// in one launch over ALL the shard's partitions (the plan is the update's, over 0 .. P-1 in ascending order, so no
// destination tile belongs to two items).  A partition's multiplicity in `owned` goes into its job; 0 means not
// owned: W is read and divided only.  The logically-zero flags go to the kernel as they are -- nothing is
// materialized, AGG is never stored -- and every owned partition leaves with both set.
int dev_round_segs_peers(ipls_dev* h, const seg_ref* segs, bool diff, const void* const* t_ptrs, int n_peers,
                         void* const* o_ptrs, int n_lists, int n_segs, const int32_t* owned, int n_owned) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  if (n_peers < 1 || !t_ptrs) return fail(h, IPLS_E_INVAL, "bad peer list");
  if (n_lists < 1 || (n_segs > 0 && !o_ptrs)) return fail(h, IPLS_E_INVAL, "bad output copy list");
  if (n_owned < 0 || (n_owned > 0 && !owned)) return fail(h, IPLS_E_INVAL, "bad owned list");
  std::vector<int32_t> mult((size_t)h->P, 0), all((size_t)h->P);
  for (int i = 0; i < n_owned; ++i) {
    if (int rc = check_part(h, owned[i])) return rc;
    ++mult[(size_t)owned[i]];
  }
  for (int q = 0; q < h->P; ++q) all[(size_t)q] = q;
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  const segplan::Plan pl = segplan::plan_update(seg_geometry(h), tab.data(), n_segs, all.data(), h->P, kSegTile);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  if (pl.n < h->flat_total)
    return fail(h, IPLS_E_RANGE, "output list of %lld < model size %lld", (long long)pl.n, (long long)h->flat_total);
  if (h->P == 0) return IPLS_OK;
  const segplan::Launch& l = pl.launches[0];          // no repeats: one launch
  // both twins' bounds together: every partition's values are its whole body, and the pieces are the shard's model
  int64_t covered = 0;
  for (const segplan::Job& j : l.jobs) {
    if (j.ncopy != j.L - 1)
      return fail(h, IPLS_E_RANGE, "partition %d holds %lld values, the lists give it %lld", h->p_lo + j.q,
                  (long long)(j.L - 1), (long long)j.ncopy);
    covered += j.ncopy;
  }
  int64_t in_pieces = 0;
  for (const segplan::Piece& p : pl.pieces) in_pieces += p.n;
  if (covered != in_pieces || covered != h->flat_total - h->flat_base)
    return fail(h, IPLS_E_RANGE, "the lists' %lld values on this shard are not its %lld model values",
                (long long)in_pieces, (long long)(h->flat_total - h->flat_base));
  if (l.items.empty()) return IPLS_OK;
  HIP_TRY(h, dev_use(h->device));
  const std::vector<SegPiece> pieces = seg_pieces(pl, segs);
  std::vector<const void*> psrc(pieces.size() * (size_t)n_peers);
  std::vector<void*> pdst(pieces.size() * (size_t)n_lists);
  for (size_t k = 0; k < pieces.size(); ++k) {
    const segplan::Piece& p = pl.pieces[k];
    const int64_t at = p.src * segplan::fmt_esz(segs[p.seg].fmt);
    for (int q = 0; q < n_peers; ++q)
      psrc[k * (size_t)n_peers + (size_t)q] = (const char*)t_ptrs[(size_t)q * (size_t)n_segs + (size_t)p.seg] + at;
    for (int q = 0; q < n_lists; ++q)
      pdst[k * (size_t)n_lists + (size_t)q] = (char*)o_ptrs[(size_t)q * (size_t)n_segs + (size_t)p.seg] + at;
  }
  std::vector<SegRoundJob> jobs(l.jobs.size());
  bool all_zero = n_owned > 0;   // the divide alone starts nothing: 0, as the divide twins report
  for (size_t j = 0; j < jobs.size(); ++j) {
    const int q = l.jobs[j].q;
    jobs[j] = SegRoundJob{(const unsigned long long*)(h->arena + h->agg_off[q]),
                          (const unsigned long long*)(h->arena + h->rep_off[q]),
                          (unsigned long long*)(h->arena + h->w_off[q]), l.jobs[j].ncopy, l.jobs[j].L,
                          h->agg_zero[q] ? 1 : 0, h->rep_zero[q] ? 1 : 0, mult[(size_t)q], 0};
    if (mult[(size_t)q]) all_zero = all_zero && h->agg_zero[q];
  }
  TablePack pack;
  const size_t at_items = pack.add(l.items.data(), l.items.size());
  const size_t at_jobs = pack.add(jobs.data(), jobs.size());
  const size_t at_pieces = pack.add(pieces.data(), pieces.size());
  const size_t at_psrc = pack.add(psrc.data(), psrc.size());
  const size_t at_pdst = pack.add(pdst.data(), pdst.size());
  void* d = nullptr;
  if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &d)) return rc;
  const char* dt = (const char*)d;
  with_bool(diff, [&](auto df) {
    with_bool(h->secure != 0, [&](auto sec) {
      hipLaunchKernelGGL((k_round_segs_peers<decltype(df)::value, decltype(sec)::value>),
                         dim3((unsigned)l.items.size()), dim3(kBlock), 0, h->stream,
                         (const segplan::Item*)(dt + at_items), (const SegRoundJob*)(dt + at_jobs),
                         (const SegPiece*)(dt + at_pieces), (const void* const*)(dt + at_psrc), n_peers,
                         (void* const*)(dt + at_pdst), n_lists);
    });
  });
  HIP_TRY(h, hipGetLastError());
  for (int q = 0; q < h->P; ++q)
    if (mult[(size_t)q]) h->agg_zero[q] = h->rep_zero[q] = 1;
  h->last_launch = launch_info(IPLS_KERNEL_ROUND_SEGS_PEERS, 0, kBlock, kSegV, l.any_whole ? 1 : 0, 0,
                               (int64_t)l.items.size(), false, false, all_zero ? kZero : kAccum);
  return IPLS_OK;
}

// dev_send_many over a segment list: device sources only, read where they lie.
// b_ptrs: null, or the subtrahend list of a difference call.
static int64_t send_many_segs(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs, int n_parts,
                              const int* parts, int32_t iteration, int16_t pid, const uint8_t* origin,
                              int32_t origin_len, void* out, const int64_t* offs, const int64_t* lens, int out_kind) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  // as dev_send_many: no accumulator, zero flag or queue is read or written, so queued arrivals stay queued
  std::lock_guard<std::mutex> lk_(h->mu);
  if (n_parts <= 0) return IPLS_OK;
  if (origin_len < 0 || (origin_len > 0 && !origin)) return fail(h, IPLS_E_INVAL, "bad origin");
  if (out_kind != IPLS_HOST_TEXT && out_kind != IPLS_DEV_TEXT) return fail(h, IPLS_E_INVAL, "out_kind HOST_TEXT/DEV_TEXT");
  for (int i = 0; i < n_parts; ++i)
    if (int rc = check_part(h, parts[i])) return rc;
  const std::vector<segplan::Seg> tab = seg_table(segs, n_segs);
  const segplan::Plan pl = segplan::plan_send(seg_geometry(h), tab.data(), n_segs, parts, n_parts);
  if (int rc = seg_plan_rc(h, pl)) return rc;
  HIP_TRY(h, dev_use(h->device));
  if (out_kind == IPLS_DEV_TEXT && !kernel_writable(out))
    return fail(h, IPLS_E_INVAL, "DEV_TEXT output is neither device memory nor pinned host memory");
  const unsigned char* dorig = nullptr;
  if (origin_len > 0) {
    void* d = nullptr;
    if (int rc = upload_table(h, origin, (size_t)origin_len, &d)) return rc;
    dorig = (const unsigned char*)d;
  }
  // texts land straight in a 16-B aligned device buffer; else in the scratch buffer at the same offsets, then copied out
  const bool direct = out_kind == IPLS_DEV_TEXT && !((uintptr_t)out & 15);
  int64_t span = 0;
  for (int i = 0; i < n_parts; ++i) span = std::max(span, offs[i] + lens[i]);
  int64_t lo = span;
  for (int i = 0; i < n_parts; ++i) lo = std::min(lo, offs[i]);
  if (!direct)
    if (int rc = ensure_scratch(h, (size_t)align_up(span - lo + 64, 256))) return rc;
  unsigned char* base = direct ? (unsigned char*)out : (unsigned char*)h->d_scratch - lo;
  const std::vector<SegPiece> pieces = seg_pieces(pl, segs);
  const segplan::Launch& l = pl.launches[0];
  std::vector<SegEncJob> jobs((size_t)n_parts);
  int64_t max_groups = 1;
  bool any_fast = false;
  for (int i = 0; i < n_parts; ++i) {
    const segplan::Job& pj = l.jobs[(size_t)i];
    SegEncJob& j = jobs[(size_t)i];
    j = SegEncJob{};
    frame_header(j.hdr, pid, pj.L, h->p_lo + pj.q, iteration);
    j.L = pj.L;
    j.ncopy = pj.ncopy;
    j.piece_lo = pj.piece_lo;
    j.piece_hi = pj.piece_hi;
    j.origin_len = origin_len;
    j.origin = dorig;
    j.out = base + offs[i];
    j.groups = (14 + 8 * pj.L + origin_len + 23) / 24;
    j.text_len = lens[i];
    max_groups = std::max(max_groups, j.groups);
    // a lane g >= 1 is fast when its values 3g - 2 .. 3g + 1 lie in one piece
    for (int k = pj.piece_lo; k < pj.piece_hi && !any_fast; ++k) {
      const segplan::Piece& p = pl.pieces[(size_t)k];
      const int64_t g = std::max<int64_t>(1, (p.dst + 2 + 2) / 3);
      any_fast = 3 * g + 2 <= p.dst + p.n;
    }
  }
  TablePack pack;
  const size_t at_jobs = pack.add(jobs.data(), jobs.size());
  const size_t at_pieces = pack.add(pieces.data(), pieces.size());
  std::vector<const void*> bsrc;
  if (b_ptrs) bsrc = seg_pieces_b(pl, segs, b_ptrs);
  const size_t at_bsrc = b_ptrs ? pack.add(bsrc.data(), bsrc.size()) : 0;
  void* djobs = nullptr;
  if (int rc = upload_table(h, pack.bytes.data(), pack.bytes.size(), &djobs)) return rc;
  const unsigned gx = std::max(1u, std::min<unsigned>(blocks_for(max_groups, kBlock), 16384));
  const dim3 grid(gx, (unsigned)n_parts);
  if (b_ptrs)
    hipLaunchKernelGGL(k_b64url_encode_segs_diff, grid, dim3(kBlock), 0, h->stream,
                       (const SegEncJob*)((const char*)djobs + at_jobs), (const SegPiece*)((const char*)djobs + at_pieces),
                       (const void* const*)((const char*)djobs + at_bsrc));
  else
    hipLaunchKernelGGL(k_b64url_encode_segs, grid, dim3(kBlock), 0, h->stream,
                       (const SegEncJob*)((const char*)djobs + at_jobs), (const SegPiece*)((const char*)djobs + at_pieces));
  HIP_TRY(h, hipGetLastError());
  h->last_launch = launch_info(b_ptrs ? IPLS_KERNEL_ENCODE_SEGS_DIFF : IPLS_KERNEL_ENCODE_SEGS, 0, kBlock, 3,
                               any_fast ? 1 : 0, 0, (int64_t)gx * n_parts, false, false, 0);
  if (direct) return IPLS_OK;                           // stream-ordered
  const hipMemcpyKind kind = out_kind == IPLS_DEV_TEXT ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (int i = 0; i < n_parts; ++i)
    HIP_TRY(h, hipMemcpyAsync((unsigned char*)out + offs[i], base + offs[i], (size_t)lens[i], kind, h->stream));
  if (out_kind == IPLS_HOST_TEXT) HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

int64_t dev_send_many_segs(ipls_dev* h, const seg_ref* segs, int n_segs, int n_parts, const int* parts,
                           int32_t iteration, int16_t pid, const uint8_t* origin, int32_t origin_len, void* out,
                           const int64_t* offs, const int64_t* lens, int out_kind) {
  return send_many_segs(h, segs, nullptr, n_segs, n_parts, parts, iteration, pid, origin, origin_len, out, offs, lens,
                        out_kind);
}
int64_t dev_send_many_segs_diff(ipls_dev* h, const seg_ref* segs, const void* const* b_ptrs, int n_segs, int n_parts,
                                const int* parts, int32_t iteration, int16_t pid, const uint8_t* origin,
                                int32_t origin_len, void* out, const int64_t* offs, const int64_t* lens, int out_kind) {
  if (n_segs > 0 && !b_ptrs) return fail(h, IPLS_E_INVAL, "null subtrahend list");
  static const void* const none[1] = {nullptr};
  return send_many_segs(h, segs, b_ptrs ? b_ptrs : none, n_segs, n_parts, parts, iteration, pid, origin, origin_len,
                        out, offs, lens, out_kind);
}

// ---- saved-model files on the device (engine.hpp) ----
static_assert(sizeof(ser_entry::prefix) == kSerPrefixMax && kSerPrefixMax == javaser::kSavedPrefixMax, "one prefix size");

int dev_ser_pack(ipls_dev* h, const ser_entry* entries, int n, int target, bool boxed, int64_t slot_bytes,
                 ipls_stage** st_out, int64_t* nbytes) {
  if (!h || !entries || !st_out || !nbytes || n <= 0 || n > 65535) return fail_nl(h, IPLS_E_INVAL, "bad argument");
  *st_out = nullptr;
  std::vector<SerPackJob> jobs((size_t)n);
  int64_t total = 0, max_words = 1;
  for (int i = 0; i < n; ++i) {
    const ser_entry& e = entries[i];
    if (int rc = check_part_nl(h, e.q)) return rc;
    if (int rc = check_target_nl(h, target)) return rc;
    if (e.prefix_len < (boxed ? 6 : 0) || e.prefix_len > kSerPrefixMax) return fail_nl(h, IPLS_E_INVAL, "bad prefix");
    SerPackJob& j = jobs[(size_t)i];
    j = SerPackJob{};
    j.n = h->len[e.q];
    j.pos = total;
    j.prefix_len = e.prefix_len;
    j.suffix = e.suffix;
    std::memcpy(j.prefix, e.prefix, (size_t)e.prefix_len);
    const int64_t body = boxed ? 14 * j.n - 6 : 8 * j.n;
    total += e.prefix_len + body + (e.suffix >= 0 ? 1 : 0);
    max_words = std::max(max_words, body / 16 + 1);
  }
  *nbytes = total;
  const size_t slot = (size_t)std::max<int64_t>(16, std::min(slot_bytes, total));
  return stage_snapshot(h, (size_t)total + 32, slot, st_out, [&](ipls_stage* st) {
    for (int i = 0; i < n; ++i) {
      const uint8_t* zf = zero_flag(h, entries[i].q, target);
      jobs[(size_t)i].src =
          (zf && *zf) ? nullptr : (const unsigned long long*)(h->arena + target_off(h, entries[i].q, target));
    }
    void* djobs = nullptr;
    if (int r = upload_table(h, jobs.data(), jobs.size() * sizeof(SerPackJob), &djobs)) return r;
    const dim3 grid(std::max(1u, std::min<unsigned>(blocks_for(max_words, kSerTileWords), 16384)), (unsigned)n);
    if (boxed) hipLaunchKernelGGL(k_ser_pack_boxed, grid, dim3(kBlock), 0, h->stream, (const SerPackJob*)djobs, (unsigned char*)st->d);
    else hipLaunchKernelGGL(k_ser_pack, grid, dim3(kBlock), 0, h->stream, (const SerPackJob*)djobs, (unsigned char*)st->d);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? IPLS_OK : fail(h, IPLS_E_DEVICE, "saved-model pack: %s", hipGetErrorString(e));
  });
}

int dev_ser_deliver(ipls_dev* h, ipls_stage* st, int64_t off, int64_t n, int64_t chunk, int64_t base, ipls_byte_sink sink,
                    void* ctx) {
  if (!h || !st || !sink || chunk < 16) return fail_nl(h, IPLS_E_INVAL, "bad argument");
  if (int rc = use_nl(h)) return rc;
  const int64_t c = std::min<int64_t>(chunk, (int64_t)st->slot[0].cap);
  return stage_deliver_bytes(h, st, (const char*)st->d + off, n, c, base, sink, ctx);
}

int dev_ser_apply(ipls_dev* h, const uint8_t* bytes, int64_t lo, int64_t hi, const int* q, const int64_t* offs, int n,
                  int mode, int target, double a, double b) {
  if (!h || !bytes || !q || !offs || n <= 0 || n > 65535 || lo < 0 || hi < lo) return fail(h, IPLS_E_INVAL, "bad argument");
  IPLS_LOCK(h);
  std::vector<SerApplyJob> jobs((size_t)n);
  int64_t max_pairs = 1;
  for (int i = 0; i < n; ++i) {
    if (int rc = check_part(h, q[i])) return rc;
    if (target_off(h, q[i], target) < 0) return fail(h, IPLS_E_INVAL, "bad target %d", target);
    const int64_t L = h->len[q[i]];
    if (offs[i] < lo || offs[i] + 8 * L > hi) return fail(h, IPLS_E_RANGE, "payload of partition %d outside the file", q[i]);
    jobs[(size_t)i] = SerApplyJob{h->arena + target_off(h, q[i], target), L, offs[i] - lo};
    max_pairs = std::max(max_pairs, L / 2 + 1);
  }
  HIP_TRY(h, dev_use(h->device));
  if (int rc = to_scratch(h, bytes + lo, (size_t)(hi - lo), (size_t)(hi - lo) + 32)) return rc;
  for (int i = 0; i < n; ++i) {
    if (mode == IPLS_SAVED_BLEND) {
      if (int rc = materialize(h, q[i], target)) return rc;
    } else if (uint8_t* zf = zero_flag(h, q[i], target)) {
      *zf = 0;   // every value is written
    }
  }
  void* djobs = nullptr;
  if (int rc = upload_table(h, jobs.data(), jobs.size() * sizeof(SerApplyJob), &djobs)) return rc;
  const dim3 grid(std::max(1u, std::min<unsigned>(blocks_for(max_pairs, kSerTileWords), 16384)), (unsigned)n);
  if (mode == IPLS_SAVED_BLEND)
    hipLaunchKernelGGL(k_ser_apply<true>, grid, dim3(kBlock), 0, h->stream, (const SerApplyJob*)djobs,
                       (const unsigned char*)h->d_scratch, a, b);
  else
    hipLaunchKernelGGL(k_ser_apply<false>, grid, dim3(kBlock), 0, h->stream, (const SerApplyJob*)djobs,
                       (const unsigned char*)h->d_scratch, a, b);
  HIP_TRY(h, hipGetLastError());
  return IPLS_OK;
}

int dev_load_dlist(ipls_dev* h, const uint8_t* bytes, int64_t nvals, int64_t hi, bool apply) {
  if (!h || !bytes) return fail(h, IPLS_E_INVAL, "null argument");
  IPLS_LOCK(h);
  const int64_t g0 = h->flat_base;
  if (hi < 0) hi = h->flat_total;
  if (hi > nvals || hi < h->flat_total || g0 > hi)
    return fail(h, IPLS_E_RANGE, "model of %lld values < model size %lld", (long long)nvals, (long long)h->flat_total);
  HIP_TRY(h, dev_use(h->device));
  // scratch: [records g0..hi, 14 bytes each, + slack][their values][flag]
  const int64_t img = 14 * (hi - g0), val_off = align_up(img + 32, 16), flag_off = val_off + 8 * (hi - g0);
  if (int rc = ensure_scratch(h, (size_t)flag_off + 16)) return rc;
  unsigned char* base = (unsigned char*)h->d_scratch;
  unsigned long long* vals = (unsigned long long*)(base + val_off);
  unsigned* dflag = (unsigned*)(base + flag_off);
  if (int rc = stage_h2d(h, base, bytes + javaser::kDlistFirst - 6 + 14 * g0, (size_t)img)) return rc;
  HIP_TRY(h, hipMemsetAsync(dflag, 0, 4, h->stream));
  hipLaunchKernelGGL(k_ser_unbox, dim3(std::max(1u, std::min<unsigned>(blocks_for(hi - g0, kBlock), 8192))), dim3(kBlock), 0,
                     h->stream, (const unsigned char*)base, (int64_t)0, g0, hi, vals, dflag);
  HIP_TRY(h, hipGetLastError());
  unsigned flag = 0;
  if (int rc = d2h(h, &flag, dflag, 4)) return rc;
  if (flag) return fail(h, IPLS_E_FORMAT, "serialised ArrayList<Double>: an element is not a Double");
  if (!apply) return IPLS_OK;
  for (int p = 0; p < h->P; ++p) {
    const int64_t L = h->len[p];
    // IPLS.java:1883-1895: values for j < min((i+1)c, M), count slot 0.0
    hipLaunchKernelGGL(k_load_model<false>, dim3(blocks_for(L, kBlock)), dim3(kBlock), 0, h->stream, vals,
                       h->flat_off[p] - h->flat_base, L - 1, L, h->arena + h->w_off[p]);
    HIP_TRY(h, hipGetLastError());
    h->agg_zero[p] = h->rep_zero[p] = h->fut_zero[p] = 1;   // IPLS.java:1886-1898
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return IPLS_OK;
}

// ---- engine plumbing used by the multi-device front (ipls_agg.cpp) ----
int dev_device(const ipls_dev* h) { return h ? h->device : -1; }

int dev_last_launch(const ipls_dev* h, ipls_launch_info* out) {
  if (!h || !out) return IPLS_E_INVAL;
  *out = h->last_launch;
  return IPLS_OK;
}

// Fixed-order fold of k device buckets per destination into caller device
// buffers that are NOT this engine's partitions (a replica slot's partial
// sums): lens[q] doubles each, dst[q] native doubles.  Same kernels, same
// order as reduce_batch_out.
int dev_reduce_ext(ipls_dev* h, int n, const int64_t* lens, const void* const* bufs, int k, bool be_in,
                   int start_mode, void* const* dst) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  IPLS_LOCK(h);
  HIP_TRY(h, dev_use(h->device));
  return reduce_dev(h, 0, n, bufs, k, be_fmt(be_in), start_mode, IPLS_TGT_AGG, dst, false, nullptr, false, lens);
}

// Collect_Replicas' length rule (IPLS.java:1225) over this engine's stored
// Other_Replica_Gradients, without folding anything.
int dev_other_check(ipls_dev* h) {
  if (!h) return fail(nullptr, IPLS_E_INVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  for (auto& kv : h->other)
    if (kv.second.n > h->len[kv.first.first])
      return fail(h, IPLS_E_RANGE, "stored replica of %lld doubles > partition %d length %lld "
                  "(ArrayIndexOutOfBoundsException, IPLS.java:1225)", (long long)kv.second.n,
                  kv.first.first + h->p_lo, (long long)h->len[kv.first.first]);
  return IPLS_OK;
}
