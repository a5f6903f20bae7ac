// fmt.hpp -- the element formats of sources and outputs, and the operand kinds
// (include/ipls_agg.h) that carry them.  Host-only; shared by the front, the
// engine and operand.hpp.
#pragma once

#include "../../include/ipls_agg.h"

// Element format of a source or an output: native doubles, big-endian double
// bytes, or one of the trainer formats of include/ipls_agg.h (floats, IEEE
// binary16, bfloat16), which the kernels widen / narrow in registers.  The
// values are also the format codes of the accumulate_async queues.
enum Fmt : int { kFmtF64 = 0, kFmtBE = 1, kFmtF32 = 2, kFmtF16 = 3, kFmtBF16 = 4 };
constexpr Fmt be_fmt(bool be) { return be ? kFmtBE : kFmtF64; }
constexpr bool fmt_trainer(Fmt f) { return f >= kFmtF32; }                    // widened on the device
constexpr bool fmt_h16(Fmt f) { return f == kFmtF16 || f == kFmtBF16; }
constexpr int fmt_size(Fmt f) { return f == kFmtF32 ? 4 : fmt_h16(f) ? 2 : 8; }   // bytes per element (= alignment)
// format of an operand kind where the trainer kinds are accepted; every other kind counts as doubles
constexpr Fmt kind_fmt(int kind) {
  return kind == IPLS_DEV_BE || kind == IPLS_HOST_BE                ? kFmtBE
         : kind == IPLS_DEV_F32 || kind == IPLS_HOST_F32            ? kFmtF32
         : kind == IPLS_DEV_F16 || kind == IPLS_HOST_F16            ? kFmtF16
         : kind == IPLS_DEV_BF16 || kind == IPLS_HOST_BF16          ? kFmtBF16
                                                                    : kFmtF64;
}
constexpr bool kind_trainer_dev(int kind) { return kind == IPLS_DEV_F32 || kind == IPLS_DEV_F16 || kind == IPLS_DEV_BF16; }
constexpr bool kind_trainer_host(int kind) { return kind == IPLS_HOST_F32 || kind == IPLS_HOST_F16 || kind == IPLS_HOST_BF16; }
constexpr bool kind_trainer(int kind) { return kind_trainer_dev(kind) || kind_trainer_host(kind); }
