// The source-operand resolver (csrc/operand.hpp) on the CPU, alone: every
// entry-point row x every operand kind 0..16 and an unknown one (17), with
//   n in {0, L-1, L, L+1} for L in {1, 2, 9} (other_replica also with nothing stored),
//   the source 0, 1, 2, 4 and 8 bytes off a 16-byte boundary,
//   a null source,
//   and for the container kinds a well-formed frame, pair and double[] of L
//   values (from ipls_frame_encode and javaser's writers), each cut by one
//   byte, a frame of array length 0 and a frame one double short of L.
// What must come out is stated a second time below, call by call, the way the
// entry points used to spell it: the kinds a call takes (kTakes, the lists of
// include/ipls_agg.h), the code and text of every refusal, and for a taken
// source the payload pointer (input + header length), count, format and memory.
// Every buffer ends where its allocation ends, so a read past a truncated
// container is an AddressSanitizer report.  Built with
// -fsanitize=address,undefined (make operand_test); prints one line and exits
// 0, or the first mismatch and exits 1.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "operand.hpp"

using namespace ipls::operand;
namespace js = ipls::javaser;

static const std::set<int> kD = {0, 1, 3, 4}, kT = {11, 12, 13, 14, 15, 16};
static std::set<int> plus(std::set<int> a, const std::set<int>& b) {
  a.insert(b.begin(), b.end());
  return a;
}
// which kinds each call takes (include/ipls_agg.h; DESIGN.md §1 "Operand kinds")
static const std::set<int> kTakes[kCalls] = {
    plus(plus(kD, kT), {2, 6, 9}),   // accumulate: doubles, trainer formats, FRAME, PAIR, DARR
    plus(plus(kD, kT), {2, 6, 9}),   // accumulate_async: as accumulate
    {0, 1},                          // accumulate_range: HOST_F64, HOST_BE
    plus(kD, {2, 9}),                // set_weights: doubles, FRAME, DARR
    plus(kD, {9}),                   // blend: doubles, DARR
    kD,                              // other_replica: doubles
    plus(kD, kT),                    // load_model: doubles and trainer formats (HOST_DLIST is the front's)
    plus(kD, kT),                    // split
    plus(kD, kT),                    // update_gradient
    {1},                             // update_indirect: big-endian bytes
    {0, 1},                          // accumulate_chunked
    {12, 14, 16},                    // accumulate_chunked_narrow
};

struct Want {
  int out;            // kTake, kNoop or IPLS_E_*
  std::string text;   // of a refusal
  int64_t hdr, n;     // of a taken source: payload = input + hdr, n values
};
static Want take(int64_t hdr, int64_t n) { return Want{kTake, "", hdr, n}; }
static Want noop() { return Want{kNoop, "", 0, 0}; }
static Want refuse(int code, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return Want{code, buf, 0, 0};
}
static bool dev_kind(int k) { return k == 3 || k == 4 || k == 11 || k == 13 || k == 15; }
static int esz(int k) { return k == 11 || k == 12 ? 4 : k >= 13 && k <= 16 ? 2 : 8; }
static bool off_by(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) != 0; }
static Want short_bucket(int64_t n, const char* unit, int64_t L) {
  return refuse(IPLS_E_RANGE, "bucket of %lld %s shorter than partition length %lld", (long long)n, unit, (long long)L);
}

// what the container at src holds, as this program built it (nd < 0: cut short; why: the parser's own word)
struct Box {
  int64_t nd, hdr;
  std::string why;
};
static Want bad_box(int kind, const Box& b) {
  if (kind == 2) return refuse(IPLS_E_FORMAT, "malformed frame (BufferUnderflowException)");
  return refuse(IPLS_E_FORMAT, kind == 6 ? "partial update: %s (ObjectInputStream)" : "serialised double[]: %s (ObjectInputStream)",
                b.why.c_str());
}

static Want want(Call c, int k, const void* src, int64_t n, int64_t L, const Box& b) {
  const bool doubles = kD.count(k), trainer = kT.count(k);
  switch (c) {
    case kAccumulate:
    case kAccumulateAsync:
      if (!src) return noop();
      if (k == 2 || k == 6 || k == 9) {
        if (b.nd < 0) return bad_box(k, b);
        if (k == 2 && b.nd == 0) return noop();
        if (b.nd < L) return short_bucket(b.nd, "doubles", L);
        return take(b.hdr, b.nd);
      }
      if (!doubles && !trainer) return refuse(IPLS_E_INVAL, "bad src_kind %d", k);
      if (n < L) return short_bucket(n, "doubles", L);
      if ((trainer || (c == kAccumulateAsync && dev_kind(k))) && off_by(src, esz(k)))
        return refuse(IPLS_E_INVAL, "%s bucket not %d-byte aligned", dev_kind(k) ? "device" : "host", esz(k));
      return take(0, n);
    case kAccumulateRange:
      if (!src) return refuse(IPLS_E_INVAL, "null argument");
      if (k != 0 && k != 1)
        return refuse(IPLS_E_INVAL, "a ranged fold reads a pinned host bucket (HOST_F64 / HOST_BE), not kind %d", k);
      return take(0, n);
    case kSetWeights: {
      if (!src) return refuse(IPLS_E_INVAL, "null argument");
      int64_t hdr = 0;
      if (k == 2) {
        if (b.nd < 0) return bad_box(k, b);
        if (b.nd == 0) return refuse(IPLS_E_INVAL, "frame without gradients (NullPointerException, IPLS.java:498)");
        if (b.nd < L)
          return refuse(IPLS_E_RANGE, "frame payload of %lld doubles < length %lld (IPLS.java:498)", (long long)b.nd, (long long)L);
        return take(b.hdr, b.nd);
      }
      if (k == 9) {
        if (b.nd < 0) return bad_box(k, b);
        n = b.nd;
        hdr = b.hdr;
      }
      if (n > L) return refuse(IPLS_E_RANGE, "downloaded partition of %lld doubles > length %lld", (long long)n, (long long)L);
      if (n <= 0) return noop();
      if (!doubles && k != 9) return refuse(IPLS_E_INVAL, "bad src_kind %d", k);
      return take(hdr, n);
    }
    case kBlend: {
      if (!src) return noop();
      int64_t hdr = 0;
      if (k == 9) {
        if (b.nd < 0) return bad_box(k, b);
        n = b.nd;
        hdr = b.hdr;
      }
      if (n < L) return short_bucket(n, "doubles", L);
      if (!doubles && k != 9) return refuse(IPLS_E_INVAL, "bad src_kind %d", k);
      return take(hdr, n);
    }
    case kOtherReplica:   // L: the stored array's length, < 0 for none
      if (n < 0 || (n > 0 && !src)) return refuse(IPLS_E_INVAL, "bad bucket");
      if (trainer) return refuse(IPLS_E_INVAL, "bad flat kind %d", k);
      if ((k == 3 || k == 4) && off_by(src, 8)) return refuse(IPLS_E_INVAL, "device bucket not 8-byte aligned");
      if (L >= 0 && n > L)
        return refuse(IPLS_E_RANGE, "replica download of %lld doubles > stored %lld "
                      "(ArrayIndexOutOfBoundsException, Download_Scheduler.java:257)", (long long)n, (long long)L);
      if (!doubles) return refuse(IPLS_E_INVAL, "bad flat kind %d", k);
      return take(0, n);
    case kLoadModel:   // L: the model size
      if (!src) return refuse(IPLS_E_INVAL, "null argument");
      if (n < L) return refuse(IPLS_E_RANGE, "model of %lld values < model size %lld", (long long)n, (long long)L);
      if (!doubles && !trainer) return refuse(IPLS_E_INVAL, "bad flat kind %d", k);
      if (trainer && off_by(src, esz(k)))
        return refuse(IPLS_E_INVAL, "%s vector not %d-byte aligned", dev_kind(k) ? "device" : "host", esz(k));
      return take(0, n);
    case kSplit:
      if (!src) return refuse(IPLS_E_INVAL, "null argument");
      if (trainer && off_by(src, esz(k))) return refuse(IPLS_E_INVAL, "vector not %d-byte aligned", esz(k));
      if (!doubles && !trainer) return refuse(IPLS_E_INVAL, "bad src_kind %d", k);
      return take(0, n);
    case kUpdateGradient:
      if (!src) return noop();
      if (trainer && off_by(src, esz(k)))
        return refuse(IPLS_E_INVAL, "%s vector not %d-byte aligned", dev_kind(k) ? "device" : "host", esz(k));
      if (!doubles && !trainer) return refuse(IPLS_E_INVAL, "bad flat kind %d", k);
      return take(0, n);
    case kUpdateIndirect:   // n: bytes
      if (n < 0 || (n > 0 && !src)) return refuse(IPLS_E_INVAL, "bad byte buffer");
      if (k != 1) return refuse(IPLS_E_INVAL, "bad src_kind %d", k);   // the engine passes HOST_BE only
      return take(0, n / 8);
    case kChunked:
      if (k != 0 && k != 1) return refuse(IPLS_E_INVAL, "a chunked fold takes HOST_F64 or HOST_BE values, not kind %d", k);
      if (n < L) return short_bucket(n, "doubles", L);
      return take(0, n);
    case kChunkedNarrow:
      if (k != 12 && k != 14 && k != 16)
        return refuse(IPLS_E_INVAL, "a narrow chunked fold takes HOST_F32, HOST_F16 or HOST_BF16 values, not kind %d", k);
      if (n < L) return short_bucket(n, "values", L);
      return take(0, n);
    default:
      break;
  }
  std::abort();
}

static long g_cases;
[[noreturn]] static void die(const char* what, Call c, int k, int64_t n, int64_t L, int off, const Want& w, int got,
                             const Resolved& r) {
  std::fprintf(stderr, "operand: %s: %s kind %d n %lld L %lld offset %d\n  want %d \"%s\" hdr %lld n %lld\n  got  %d \"%s\" n %lld\n",
               what, kRows[c].name, k, (long long)n, (long long)L, off, w.out, w.text.c_str(), (long long)w.hdr, (long long)w.n,
               got, got < 0 ? r.why.text : "", got == kTake ? (long long)r.n : 0LL);
  std::exit(1);
}

static void check(Call c, int k, const void* src, int64_t n, int64_t L, int off, const Box& b) {
  const Want w = want(c, k, src, n, L, b);
  Resolved r;
  std::memset(&r, 0x5a, sizeof r);
  const int got = resolve(c, src, n, k, L, &r);
  ++g_cases;
  if (got != w.out) die("outcome", c, k, n, L, off, w, got, r);
  if (got == kTake && !kTakes[c].count(k)) die("a kind outside the list was taken", c, k, n, L, off, w, got, r);
  if (got < 0 && (r.why.code != got || w.text != r.why.text)) die("refusal", c, k, n, L, off, w, got, r);
  if (got >= 0 && r.why.code != IPLS_OK) die("code of a source that was not refused", c, k, n, L, off, w, got, r);
  if (got != kTake) return;
  const bool box = w.hdr != 0;
  const Container from = !box ? kRaw : k == 2 ? kFrame : k == 6 ? kPair : kDarr;
  if (r.ptr != (src ? (const char*)src + w.hdr : nullptr) || r.n != w.n || r.fmt != (box ? kFmtBE : kind_fmt(k)) ||
      r.host != !dev_kind(k) || r.from != from)
    die("view", c, k, n, L, off, w, got, r);
}

// `bytes` copied so that they start `off` bytes past a 16-byte boundary and end with their allocation
struct Placed {
  void* block = nullptr;
  uint8_t* at = nullptr;
  Placed(const std::vector<uint8_t>& bytes, int off) {
    if (posix_memalign(&block, 16, off + bytes.size() + (bytes.empty() && !off ? 1 : 0))) std::abort();
    at = (uint8_t*)block + off;
    if (!bytes.empty()) std::memcpy(at, bytes.data(), bytes.size());
  }
  ~Placed() { std::free(block); }
  Placed(const Placed&) = delete;
};

static std::vector<double> values(int64_t n) {
  std::vector<double> g((size_t)n);
  for (int64_t i = 0; i < n; ++i) g[(size_t)i] = 1.5 * (double)(i + 1);
  return g;
}
static std::vector<uint8_t> be_bytes(int64_t n) {
  std::vector<uint8_t> out((size_t)n * 8);
  const std::vector<double> g = values(n);
  for (int64_t i = 0; i < n; ++i) {
    uint64_t v;
    std::memcpy(&v, &g[(size_t)i], 8);
    v = __builtin_bswap64(v);
    std::memcpy(&out[(size_t)i * 8], &v, 8);
  }
  return out;
}
static std::vector<uint8_t> frame(int64_t n) {
  std::vector<uint8_t> out(14 + (size_t)n * 8);
  const std::vector<double> g = values(n);
  if (ipls_frame_encode(g.data(), n, IPLS_HOST_F64, 3, 7, 3, nullptr, 0, out.data(), (int64_t)out.size()) != (int64_t)out.size())
    std::abort();
  return out;
}
static std::vector<uint8_t> boxed(int kind, int64_t n) {
  if (kind == 2) return frame(n);
  std::vector<uint8_t> out, pay = be_bytes(n);
  if (kind == 6) {
    out.resize((size_t)js::pair_header_len());
    js::write_pair_header(out.data(), 5, (int32_t)n);
    out.insert(out.end(), pay.begin(), pay.end());
    out.resize(out.size() + (size_t)js::pair_trailer_len());
    js::write_pair_trailer(out.data() + out.size() - js::pair_trailer_len());
  } else {
    out.resize((size_t)js::kSavedPrefixMax);
    out.resize((size_t)js::darr_header(out.data(), (int32_t)n));
    out.insert(out.end(), pay.begin(), pay.end());
  }
  return out;
}
// what the bytes hold, by the parser's own account of a cut stream (its word goes into the refusal's text)
static Box box_of(int kind, const uint8_t* bytes, int64_t len, int64_t nd) {
  Box b{nd, kind == 2 ? 14 : kind == 6 ? js::pair_header_len() : js::kDarrHeader, ""};
  if (nd >= 0 || kind == 2) return b;
  const char* why = nullptr;
  int64_t poff;
  int32_t workers;
  const int64_t got = kind == 6 ? js::parse_pair(bytes, len, &workers, &poff, &why) : js::parse_darr(bytes, len, &poff, &why);
  if (got >= 0) std::abort();
  b.why = why ? why : "malformed";
  return b;
}

int main() {
  static const int kOffs[] = {0, 1, 2, 4, 8};
  static const int64_t kLens[] = {1, 2, 9, -1};   // -1: other_replica with nothing stored
  const Box none{0, 0, ""};
  for (int c = 0; c < kCalls; ++c) {
    // the table against the lists above
    for (int k = 0; k <= 17; ++k)
      if (((kRows[c].kinds & bit(k)) != 0) != (kTakes[c].count(k) != 0)) {
        std::fprintf(stderr, "operand: row %s and the header's list disagree on kind %d\n", kRows[c].name, k);
        return 1;
      }
    for (int k = 0; k <= 17; ++k)
      for (int64_t L : kLens) {
        if (L < 0 && c != kOtherReplica) continue;
        const bool bytes_in = c == kUpdateIndirect;   // n counts bytes there: the same counts, and one odd byte more
        for (int64_t n : {(int64_t)0, L - 1, L, L + 1}) {
          for (int off : kOffs) {
            const Placed p(std::vector<uint8_t>((size_t)std::max<int64_t>(n, 0) * 8), off);
            // a raw source: nothing reads it, a container kind the row takes excepted -- those bytes are zeros,
            // a cut frame / stream (array length 0 for a frame of 14 bytes or more)
            Box b = none;
            if (kTakes[c].count(k) && (k == 2 || k == 6 || k == 9)) {
              const std::vector<uint8_t> z((size_t)std::max<int64_t>(n, 0), 0);
              const Placed q(z, off);
              b = box_of(k, q.at, (int64_t)z.size(), k == 2 && n >= 14 ? 0 : -1);
              check((Call)c, k, q.at, std::max<int64_t>(n, 0), L, off, b);
              continue;
            }
            check((Call)c, k, p.at, bytes_in ? 8 * n + (n > 0) : n, L, off, b);
          }
          check((Call)c, k, nullptr, n, L, -1, none);   // a null source
        }
        if (L < 0 || (k != 2 && k != 6 && k != 9)) continue;
        // containers: L values, the same cut by one byte, an empty frame, a frame one double short
        for (int off : kOffs) {
          const std::vector<uint8_t> whole = boxed(k, L);
          std::vector<uint8_t> cut(whole.begin(), whole.end() - 1);
          const Placed pw(whole, off), pc(cut, off);
          // rows that do not take the kind read n as a count and never look at the bytes
          check((Call)c, k, pw.at, (int64_t)whole.size(), L, off, box_of(k, pw.at, (int64_t)whole.size(), L));
          check((Call)c, k, pc.at, (int64_t)cut.size(), L, off, box_of(k, pc.at, (int64_t)cut.size(), -1));
          if (k != 2) continue;
          const std::vector<uint8_t> empty = frame(0), less = frame(L - 1);
          const Placed pe(empty, off), pl(less, off);
          check((Call)c, k, pe.at, (int64_t)empty.size(), L, off, box_of(k, pe.at, (int64_t)empty.size(), 0));
          check((Call)c, k, pl.at, (int64_t)less.size(), L, off, box_of(k, pl.at, (int64_t)less.size(), L - 1));
        }
      }
  }
  // the two zero-copy predicates at their seams
  alignas(16) static char buf[32];
  if (!zero_copy_arrival(buf + 8, 65536) || zero_copy_arrival(buf + 8, 65535) || zero_copy_arrival(buf + 4, 65536) ||
      !zero_copy_queued(buf) || zero_copy_queued(buf + 8)) {
    std::fprintf(stderr, "operand: zero-copy predicates\n");
    return 1;
  }
  std::printf("operand ok: %ld cases over %d rows\n", g_cases, (int)kCalls);
  return 0;
}
