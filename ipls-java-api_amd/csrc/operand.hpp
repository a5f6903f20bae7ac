// operand.hpp -- what a source operand (src, n, src_kind) of a C-ABI call is:
// where its values are, how many, in what format, in host or device memory,
// and whether the call takes it.  Host-only like reduce_plan.hpp (no HIP type;
// tests/cpp/test_operand.cpp runs it on the CPU).  kRows is the single
// statement of which call takes which kind; engine.hip resolves every source
// through resolve() and then does its own staging and launch.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../include/ipls_agg.h"
#include "fmt.hpp"
#include "javaser.hpp"

namespace ipls {
namespace operand {

enum Container : int { kRaw, kFrame, kPair, kDarr };
struct SrcView {
  const void* ptr;   // the first value, after any container header
  int64_t n;         // values
  Fmt fmt;
  bool host;         // host memory (pageable or pinned), else device memory
  Container from;
};
struct Refusal {
  int code;          // IPLS_E_*; IPLS_OK when nothing was refused
  char text[200];    // for fail(), unchanged
};
struct Resolved : SrcView {   // what resolve() fills: the view when it says kTake, else `why`
  Refusal why;
};

// kind sets: bit k is operand kind k; bit 31 stands for every kind outside 0..30
constexpr uint32_t bit(int kind) { return kind >= 0 && kind < 31 ? 1u << kind : 1u << 31; }
constexpr uint32_t kHostD = bit(IPLS_HOST_F64) | bit(IPLS_HOST_BE), kDevD = bit(IPLS_DEV_F64) | bit(IPLS_DEV_BE);
constexpr uint32_t kHostT = bit(IPLS_HOST_F32) | bit(IPLS_HOST_F16) | bit(IPLS_HOST_BF16);
constexpr uint32_t kDevT = bit(IPLS_DEV_F32) | bit(IPLS_DEV_F16) | bit(IPLS_DEV_BF16);
constexpr uint32_t kDev = kDevD | kDevT, kFlat = kHostD | kDevD | kHostT | kDevT, kAll = ~0u;
constexpr uint32_t kBoxed = bit(IPLS_HOST_FRAME) | bit(IPLS_HOST_PAIR) | bit(IPLS_HOST_DARR);

// The three length rules, against L: the partition, the model, or the stored array.
enum Len : int {
  kAtLeast,        // accumulate, blend: `Agg[i] + g[i]` for i < L_p overruns a shorter bucket (Updater.java:115)
  kAtMost,         // set_weights: GetParameters writes data.length / 8 values into arr (MyIPFSClass.java:449-452);
                   // more than L overrun arr, n <= 0 writes nothing
  kAtMostStored,   // other_replica: `Other[j] += g[j]` for j < g.length (Download_Scheduler.java:254-260) against
                   // the array in the engine's store (L < 0: none yet)
  kByEngine        // the engine's own bounds: a range, OrganizeGradients' split_bounds, Gradient_Buff
};
enum Null : int { kNullNoop, kNullRefused, kNullIfEmpty, kNoSource };   // kNullIfEmpty: null only with n == 0
enum EmptyFrame : int { kEmptyNoop, kEmptyRefused, kNoFrame };          // a frame whose array length is 0
enum ZeroCopy : int { kStaged, kArrival, kQueued };                     // the predicate below that the host path asks

enum Call : int {
  kAccumulate, kAccumulateAsync, kAccumulateRange, kSetWeights, kBlend, kOtherReplica, kLoadModel, kSplit,
  kUpdateGradient, kUpdateIndirect, kChunked, kChunkedNarrow, kCalls
};
struct Row {
  const char* name;
  uint32_t kinds;            // taken
  uint32_t early;            // of the others, refused before the length rule (the rest after it)
  Null null;
  const char* null_text;
  Len len;
  const char* len_text;      // (n, L); null: kShortBucket with `unit`
  const char* unit;
  EmptyFrame empty;
  const char* frame_short;   // a frame is held to "at least L" with this text (n, L) whatever `len` says
  const char* bad_kind;      // (kind)
  const char* dev_noun;      // misaligned trainer-format sources: "<noun> not <size>-byte aligned"
  const char* host_noun;
  bool dev_d_aligned;        // DEV_F64 / DEV_BE are held to 8 bytes too (elsewhere nobody checks them) ...
  bool align_first;          // ... and before the length rule
  bool n_bytes;              // n counts bytes of big-endian doubles, n / 8 values (MyIPFSClass.java:449)
  ZeroCopy zero_copy;
};

constexpr char kShortBucket[] = "bucket of %lld %s shorter than partition length %lld";
constexpr char kMisaligned[] = "%s not %d-byte aligned";
constexpr char kBadFrame[] = "malformed frame (BufferUnderflowException)";
constexpr char kNoGradients[] = "frame without gradients (NullPointerException, IPLS.java:498)";
constexpr char kBadPair[] = "partial update: %s (ObjectInputStream)";
constexpr char kBadDarr[] = "serialised double[]: %s (ObjectInputStream)";
constexpr char kBadSrc[] = "bad src_kind %d", kBadFlat[] = "bad flat kind %d", kNullArg[] = "null argument";

// Today's behaviour of every entry point, its wording included (three nouns
// for a misaligned source, two texts for an unknown kind, kinds refused before
// the length rule here and after it there): kept, and named here so that a
// later change can settle them on purpose.
constexpr Row kRows[kCalls] = {
    {"accumulate", kFlat | kBoxed, kAll, kNullNoop, nullptr, kAtLeast, nullptr, "doubles", kEmptyNoop, nullptr, kBadSrc,
     "device bucket", "host bucket", false, false, false, kArrival},
    // device kinds queue, pinned HOST_F64 / HOST_BE fold at once, everything else is an accumulate
    {"accumulate_async", kFlat | kBoxed, kAll, kNullNoop, nullptr, kAtLeast, nullptr, "doubles", kEmptyNoop, nullptr,
     kBadSrc, "device bucket", "host bucket", true, false, false, kQueued},
    {"accumulate_range", kHostD, kAll, kNullRefused, kNullArg, kByEngine, nullptr, nullptr, kNoFrame, nullptr,
     "a ranged fold reads a pinned host bucket (HOST_F64 / HOST_BE), not kind %d", nullptr, nullptr, false, false, false,
     kQueued},
    // ThreadReceiver pid 4 (IPLS.java:491-498) for a frame, GetParameters for the rest
    {"set_weights", kHostD | kDevD | bit(IPLS_HOST_FRAME) | bit(IPLS_HOST_DARR), 0, kNullRefused, kNullArg, kAtMost,
     "downloaded partition of %lld doubles > length %lld", nullptr, kEmptyRefused,
     "frame payload of %lld doubles < length %lld (IPLS.java:498)", kBadSrc, nullptr, nullptr, false, false, false, kStaged},
    {"blend", kHostD | kDevD | bit(IPLS_HOST_DARR), 0, kNullNoop, nullptr, kAtLeast, nullptr, "doubles", kNoFrame, nullptr,
     kBadSrc, nullptr, nullptr, false, false, false, kStaged},
    {"other_replica", kHostD | kDevD, kHostT | kDevT, kNullIfEmpty, "bad bucket", kAtMostStored,
     "replica download of %lld doubles > stored %lld (ArrayIndexOutOfBoundsException, Download_Scheduler.java:257)",
     nullptr, kNoFrame, nullptr, kBadFlat, "device bucket", nullptr, true, true, false, kStaged},
    // L: the model size (HOST_DLIST never reaches an engine: the front decodes its header)
    {"load_model", kFlat, 0, kNullRefused, kNullArg, kAtLeast, "model of %lld values < model size %lld", nullptr, kNoFrame,
     nullptr, kBadFlat, "device vector", "host vector", false, false, false, kStaged},
    {"split", kFlat, kAll, kNullRefused, kNullArg, kByEngine, nullptr, nullptr, kNoFrame, nullptr, kBadSrc, "vector",
     "vector", false, false, false, kStaged},
    {"update_gradient", kFlat, kAll, kNullNoop, nullptr, kByEngine, nullptr, nullptr, kNoFrame, nullptr, kBadFlat,
     "device vector", "host vector", false, false, false, kStaged},
    // no kind argument: the bytes of a GetParameters file, which the engine names HOST_BE
    {"update_indirect", bit(IPLS_HOST_BE), kAll, kNullIfEmpty, "bad byte buffer", kByEngine, nullptr, nullptr, kNoFrame,
     nullptr, kBadSrc, nullptr, nullptr, false, false, true, kArrival},
    // the chunked calls have a source function instead of a pointer
    {"accumulate_chunked", kHostD, kAll, kNoSource, nullptr, kAtLeast, nullptr, "doubles", kNoFrame, nullptr,
     "a chunked fold takes HOST_F64 or HOST_BE values, not kind %d", nullptr, nullptr, false, false, false, kStaged},
    {"accumulate_chunked_narrow", kHostT, kAll, kNoSource, nullptr, kAtLeast, nullptr, "values", kNoFrame, nullptr,
     "a narrow chunked fold takes HOST_F32, HOST_F16 or HOST_BF16 values, not kind %d", nullptr, nullptr, false, false,
     false, kStaged},
};

// Zero copy: may a kernel read a pinned host source in place?  The pure part;
// whether the memory is pinned is the engine's hipPointerGetAttributes.
// kArrival (accumulate, the Gradient_Buff load): 8-byte aligned and at least
// 64 KiB, below which the staged copy is quicker.
inline bool zero_copy_arrival(const void* p, size_t bytes) { return ((uintptr_t)p & 7) == 0 && bytes >= (1u << 16); }
// kQueued (accumulate_async, accumulate_range): 16-byte aligned, any size.
inline bool zero_copy_queued(const void* p) { return ((uintptr_t)p & 15) == 0; }

enum : int { kNoop = 0, kTake = 1 };

// (src, n, kind) of call c, against L as the row's length rule reads it.
// kTake: *r describes the source.  kNoop: the call returns IPLS_OK and does
// nothing.  Otherwise the refusal's code, with r->why filled.
inline int resolve(Call c, const void* src, int64_t n, int kind, int64_t L, Resolved* r) {
  const Row& row = kRows[c];
  SrcView& v = *r;
  r->why.code = IPLS_OK;
  auto refuse = [&](int code, const char* fmt, auto... a) {
    snprintf(r->why.text, sizeof r->why.text, fmt, a...);
    return r->why.code = code;
  };
  if (row.null == kNullIfEmpty ? n < 0 || (n > 0 && !src) : !src && row.null != kNoSource)
    return row.null == kNullNoop ? kNoop : refuse(IPLS_E_INVAL, "%s", row.null_text);
  const uint32_t kb = bit(kind);
  const bool taken = row.kinds & kb;
  if (!taken && (row.early & kb)) return refuse(IPLS_E_INVAL, row.bad_kind, kind);
  v = SrcView{src, row.n_bytes ? n / 8 : n, taken ? kind_fmt(kind) : kFmtF64, !(kDev & kb), kRaw};
  if (taken && (kBoxed & kb)) {
    // The payload is big-endian and in general unaligned (a frame's starts at byte 14): every site stages it.
    int64_t poff = 0;
    const char* what = nullptr;
    if (kind == IPLS_HOST_FRAME) {
      v.n = ipls_frame_parse((const uint8_t*)src, n, nullptr, nullptr, nullptr, &poff, nullptr);
      if (v.n < 0) return refuse(IPLS_E_FORMAT, "%s", kBadFrame);
      // arr_len == 0 -> Gradients = null (MyIPFSClass.java:1449-1451)
      if (v.n == 0) return row.empty == kEmptyNoop ? kNoop : refuse(IPLS_E_INVAL, "%s", kNoGradients);
    } else if (kind == IPLS_HOST_PAIR) {
      // Download_Partial_Updates(hash).getValue1() -> queue -> _Update (Download_Scheduler.java:324)
      int32_t workers;
      v.n = javaser::parse_pair((const uint8_t*)src, n, &workers, &poff, &what);
      if (v.n < 0) return refuse(IPLS_E_FORMAT, kBadPair, what ? what : "malformed");
    } else {
      // the single-partition hand-over file (MyIPFSClass.java:261-270): the Pair's double[] alone
      v.n = javaser::parse_darr((const uint8_t*)src, n, &poff, &what);
      if (v.n < 0) return refuse(IPLS_E_FORMAT, kBadDarr, what ? what : "malformed");
    }
    v.ptr = (const char*)src + poff;
    v.fmt = kFmtBE;
    v.from = kind == IPLS_HOST_FRAME ? kFrame : kind == IPLS_HOST_PAIR ? kPair : kDarr;
  }
  const char* noun = v.host ? row.host_noun : row.dev_noun;
  const bool misaligned = taken && noun && (fmt_trainer(v.fmt) || (row.dev_d_aligned && !v.host)) &&
                          ((uintptr_t)v.ptr & (uintptr_t)(fmt_size(v.fmt) - 1));
  if (misaligned && row.align_first) return refuse(IPLS_E_INVAL, kMisaligned, noun, fmt_size(v.fmt));
  if (v.from == kFrame && row.frame_short) {
    if (v.n < L) return refuse(IPLS_E_RANGE, row.frame_short, (long long)v.n, (long long)L);
  } else if (row.len == kAtLeast ? v.n < L : row.len == kAtMost ? v.n > L : row.len == kAtMostStored && L >= 0 && v.n > L) {
    if (row.len_text) return refuse(IPLS_E_RANGE, row.len_text, (long long)v.n, (long long)L);
    return refuse(IPLS_E_RANGE, kShortBucket, (long long)v.n, row.unit, (long long)L);
  } else if (row.len == kAtMost && v.n <= 0) {
    return kNoop;
  }
  if (!taken) return refuse(IPLS_E_INVAL, row.bad_kind, kind);
  if (misaligned) return refuse(IPLS_E_INVAL, kMisaligned, noun, fmt_size(v.fmt));
  return kTake;
}

}  // namespace operand
}  // namespace ipls
