// seg_kernels.hpp -- the kernels of the segment-list calls
// (ipls_agg_update_gradient_segs, ipls_agg_get_partitions_segs,
// ipls_agg_send_gradients_segs; include/ipls_agg.h): the flat vector is the
// concatenation of a list of device arrays, each of its own element format,
// and is read or written where those arrays lie.  The host plan
// (seg_plan.hpp) turns the list into pieces (runs of one segment inside one
// partition) and items (one destination tile each); blockIdx.x is the item.
// Included by engine.hip after ipls_kernels.hpp, whose helpers it uses.
#pragma once

#include "ipls_kernels.hpp"
#include "seg_plan.hpp"

namespace ipls {

// The tile of k_update_segs and k_divide_segs, in elements, for every format:
// kBlock lanes x kSegV elements (k_divide's and k_divide_narrow's tile).
constexpr int kSegV = 8;
constexpr int64_t kSegTile = (int64_t)kBlock * kSegV;
static_assert(kSegTile == kDivTile, "the segment calls use the divide's tile");

// A piece on the device: destination elements [dst, dst + n) of its partition
// are the n elements of format fmt at src (the piece's first element).
struct SegPiece {
  int64_t dst, n;
  const void* src;
  int64_t fmt;     // segplan::kF64 ..
};
struct SegJob {
  unsigned long long* dst;    // the accumulator (256-B aligned)
  int64_t ncopy, L;
  int64_t zero;               // logically +0.0: written without being read
};

// Element e of an array of format fmt (a run-time value), widened.
__device__ __forceinline__ double seg_load(const void* p, int64_t e, int fmt) {
  switch (fmt) {
    case segplan::kF64: return __builtin_bit_cast(double, ld8((const unsigned long long*)p + e));
    case segplan::kF32: return FmtF32::widen(FmtF32::ldraw((const float*)p + e));
    case segplan::kF16: return FmtF16::widen(FmtF16::ldraw((const unsigned short*)p + e));
    default: return FmtBF16::widen(FmtBF16::ldraw((const unsigned short*)p + e));
  }
}

// The piece of [lo, hi) (sorted by dst, non-empty, covering i) that holds
// destination element i: a bounded binary search.
__device__ __forceinline__ int seg_piece_of(const SegPiece* __restrict__ pieces, int lo, int hi, int64_t i) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pieces[mid].dst <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------
// k_update_segs: k_update_flat's accumulate over a shard's owned partitions in
// one launch, from a segment list:
//   dst[i] = (zero ? +0.0 : dst[i]) + v,   v = (double)(flat value off + i)
//   for i < ncopy, 1.0 at i == ncopy (the count slot), 0.0 above (the add is
//   still made: a -0.0 accumulator element becomes +0.0).
// A `whole` item (a full tile inside one piece, so below ncopy) takes the
// vector body of its format, block-uniform and dispatched outside the loops:
// all loads first, then the adds, then 16-B stores of which one instruction of
// a wave writes whole 128-B lines (trainer formats through k_fold1_narrow's
// lane ^ 4 exchange).  The residue of the tile's first source element against
// a 16-B load (8 B of 16-bit elements) decides the loads: 0 = aligned vector
// loads, anything else = naturally aligned element loads.  No load ever
// touches a byte outside its piece, so a segment needs no padding and its
// first and last tile are tiles like any other.
// Every other item goes element by element: the value of element i comes from
// a binary search of the item's pieces and a load of that piece's format.
// ---------------------------------------------------------------------------
template <class S>
__device__ __forceinline__ void update_segs_whole(const typename S::elem* __restrict__ src, unsigned long long* dst,
                                                  int64_t base, bool zero, bool aligned) {
  typedef typename S::elem T;
  const int tid = threadIdx.x;
  if constexpr (sizeof(T) == 8) {
    constexpr int R = kSegV / 2;
    auto body = [&](auto al) {
      constexpr bool AL = decltype(al)::value;
      u2 sv[R], dv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 2 * ((int64_t)r * kBlock + tid);
        if constexpr (AL) {
          sv[r] = __builtin_nontemporal_load((gcu2)(src + i));
        } else {
          sv[r].x = ld8(src + i);
          sv[r].y = ld8(src + i + 1);
        }
        if (!zero) dv[r] = *(gcu2)(dst + base + i);
        else dv[r] = u2{0, 0};
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 2 * ((int64_t)r * kBlock + tid);
        const d2 x = decode2<false>(sv[r]);
        const d2 a = __builtin_bit_cast(d2, dv[r]);   // +0.0 when the accumulator is logically zero
        *(gu2)(dst + base + i) = encode2<false>(d2{a.x + x.x, a.y + x.y});
      }
    };
    if (aligned) body(std::true_type{});
    else body(std::false_type{});
  } else {
    constexpr int R = kSegV / 4;
    typedef typename S::template Vec<4> V;
    auto body = [&](auto al) {
      constexpr bool AL = decltype(al)::value;
      V sv[R];
      typename S::raw el[R][4];
      u2 t[R][2];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 4 * ((int64_t)r * kBlock + tid);
        if constexpr (AL) {
          sv[r] = S::template ldv<4>(src + i);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) el[r][c] = S::ldraw(src + i + c);
        }
        if (!zero) {
          t[r][0] = ld16<false>(dst + base + i);
          t[r][1] = ld16<false>(dst + base + i + 2);
        } else {
          t[r][0] = t[r][1] = u2{0, 0};
        }
      }
      const bool hi = tid & 4;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if constexpr (AL) v[c] = S::template get<4>(sv[r], c);
          else v[c] = S::widen(el[r][c]);
        }
        const d2 x = __builtin_bit_cast(d2, t[r][0]), y = __builtin_bit_cast(d2, t[r][1]);
        const double a0 = x.x + v[0], a1 = x.y + v[1], a2 = y.x + v[2], a3 = y.y + v[3];
        // k_fold1_narrow's stores: lanes 8k..8k+3 own one 128-B line of sums, 8k+4..8k+7 the next
        const int64_t o = base + 4 * ((int64_t)r * kBlock + tid);
        const d2 own = d2{a0, a1};
        const d2 got = d2{__shfl_xor(a2, 4), __shfl_xor(a3, 4)};
        __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
        __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
      }
    };
    if (aligned) body(std::true_type{});
    else body(std::false_type{});
  }
}

__global__ __launch_bounds__(kBlock) void k_update_segs(const segplan::Item* __restrict__ items,
                                                        const SegJob* __restrict__ jobs,
                                                        const SegPiece* __restrict__ pieces) {
  const segplan::Item it = items[blockIdx.x];
  const SegJob j = jobs[it.job];
  const bool zero = j.zero != 0;
  if (it.whole) {
    const SegPiece pc = pieces[it.piece_lo];
    const int64_t e = it.lo - pc.dst;   // the tile's first element in the piece
    switch (it.fmt) {
      case segplan::kF64:
        update_segs_whole<FmtD64>((const unsigned long long*)pc.src + e, j.dst, it.lo, zero, it.res == 0);
        break;
      case segplan::kF32:
        update_segs_whole<FmtF32>((const float*)pc.src + e, j.dst, it.lo, zero, it.res == 0);
        break;
      case segplan::kF16:
        update_segs_whole<FmtF16>((const unsigned short*)pc.src + e, j.dst, it.lo, zero, (it.res & 3) == 0);
        break;
      default:
        update_segs_whole<FmtBF16>((const unsigned short*)pc.src + e, j.dst, it.lo, zero, (it.res & 3) == 0);
        break;
    }
    return;
  }
  for (int64_t i = it.lo + threadIdx.x; i < it.hi; i += kBlock) {
    double v;
    if (i < j.ncopy) {
      const SegPiece pc = pieces[seg_piece_of(pieces, it.piece_lo, it.piece_hi, i)];
      v = seg_load(pc.src, i - pc.dst, (int)pc.fmt);
    } else {
      v = i == j.ncopy ? 1.0 : 0.0;
    }
    const double a = zero ? 0.0 : __builtin_bit_cast(double, ld8(j.dst + i));
    st8(j.dst + i, __builtin_bit_cast(unsigned long long, a + v));
  }
}

// ---------------------------------------------------------------------------
// k_divide_segs: the GetPartitions divide (k_divide / k_divide_narrow) written
// into a list of output arrays:
//   out_s[e] = narrow_s(cnt_p == 0.0 ? W[p][j] : W[p][j] / den_p),
//   f = start_s + e, p = f / chunk, j = f - p * chunk,
// the IEEE double division, rounded once to float for F32 and from that float
// to the format for F16 / BF16; doubles are stored as they are.  Never a
// reciprocal, never a division in the narrow format.  An item is a tile of one
// output segment: the head up to the first 128-B line, then whole-line tiles.
// A `whole` item (a full tile inside one partition) is k_divide_narrow's body
// (k_divide's for doubles): W read with 8-B loads, 16 B stored per lane
// non-temporally, a wave's store whole lines.  Every other item goes element
// by element and reads the count slot of each element's own partition, so a
// partition seam inside a tile uses each side's own count.
// ---------------------------------------------------------------------------
struct SegDivPart {
  const double* w;   // Weights[q]
  int64_t len;       // L_q (the count slot is w[len - 1])
};

template <class S>
__device__ __forceinline__ void divide_segs_whole(const double* __restrict__ w, typename S::elem* o, double cnt,
                                                  double den) {
  typedef typename S::elem T;
  constexpr int EV = 16 / sizeof(T);                   // values per store
  constexpr int V = kSegTile / ((int64_t)kBlock * EV); // stores per lane
  static_assert((int64_t)kBlock * EV * V == kSegTile, "one tile size for every element size");
  // wave (threadIdx.x / 64) owns [wave * 64 * EV * V, + 64 * EV * V)
  const int64_t wave_base = (int64_t)(threadIdx.x >> 6) * 64 * EV * V + EV * (threadIdx.x & 63);
  double x[V][EV];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int64_t i = wave_base + (int64_t)v * 64 * EV;
#pragma unroll
    for (int c = 0; c < EV; ++c) x[v][c] = __builtin_nontemporal_load((const IPLS_GLOBAL double*)(w + i + c));
  }
  auto q = [&](double a) -> double { return (cnt == 0.0) ? a : a / den; };
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int64_t i = wave_base + (int64_t)v * 64 * EV;
    const double* xv = x[v];
    if constexpr (sizeof(T) == 8) {
      u2 y;
      y.x = __builtin_bit_cast(unsigned long long, q(xv[0]));
      y.y = __builtin_bit_cast(unsigned long long, q(xv[1]));
      __builtin_nontemporal_store(y, (gu2)(o + i));
    } else {
      auto f = [&](double a) -> unsigned { return S::narrow((float)q(a)); };
      // the words are spelled out, as in k_divide_narrow (a loop over them loses the non-temporal hint)
      u4w y;
      if constexpr (sizeof(T) == 2)
        y = u4w{f(xv[0]) | (f(xv[1]) << 16), f(xv[2]) | (f(xv[3]) << 16), f(xv[4]) | (f(xv[5]) << 16),
                f(xv[6]) | (f(xv[7]) << 16)};
      else
        y = u4w{f(xv[0]), f(xv[1]), f(xv[2]), f(xv[3])};
      __builtin_nontemporal_store(y, (IPLS_GLOBAL u4w*)(o + i));
    }
  }
}

template <bool SECURE>
__global__ __launch_bounds__(kBlock) void k_divide_segs(const segplan::Item* __restrict__ items,
                                                        void* const* __restrict__ outs,
                                                        const SegDivPart* __restrict__ parts, int64_t chunk,
                                                        int64_t p_lo) {
  const segplan::Item it = items[blockIdx.x];
  void* out = outs[it.job];
  if (it.whole) {
    const int64_t p = it.flat / chunk;
    const SegDivPart d = parts[p - p_lo];
    const double cnt = d.w[d.len - 1];
    const double den = SECURE ? 1e12 * cnt : cnt;   // IPLS.java:1167
    const double* w = d.w + (it.flat - p * chunk);
    switch (it.fmt) {
      case segplan::kF64: divide_segs_whole<FmtD64>(w, (unsigned long long*)out + it.lo, cnt, den); break;
      case segplan::kF32: divide_segs_whole<FmtF32>(w, (float*)out + it.lo, cnt, den); break;
      case segplan::kF16: divide_segs_whole<FmtF16>(w, (unsigned short*)out + it.lo, cnt, den); break;
      default: divide_segs_whole<FmtBF16>(w, (unsigned short*)out + it.lo, cnt, den); break;
    }
    return;
  }
  for (int64_t e = it.lo + threadIdx.x; e < it.hi; e += kBlock) {
    const int64_t f = it.flat + (e - it.lo);
    const int64_t p = f / chunk;
    const SegDivPart d = parts[p - p_lo];
    const double cnt = d.w[d.len - 1];
    const double den = SECURE ? 1e12 * cnt : cnt;
    const double x = d.w[f - p * chunk];
    const double y = (cnt == 0.0) ? x : x / den;
    switch (it.fmt) {
      case segplan::kF64: st8((unsigned long long*)out + e, __builtin_bit_cast(unsigned long long, y)); break;
      case segplan::kF32: FmtF32::put((float*)out + e, FmtF32::narrow((float)y)); break;
      case segplan::kF16: FmtF16::put((unsigned short*)out + e, FmtF16::narrow((float)y)); break;
      default: FmtBF16::put((unsigned short*)out + e, FmtBF16::narrow((float)y)); break;
    }
  }
}

// ---------------------------------------------------------------------------
// k_b64url_encode_segs: k_b64url_encode_flat over a segment list -- the pubsub
// texts of the listed partitions (blockIdx.y = job), the same decomposition:
// lane g owns frame bytes [24g, 24g + 24).  It is fast when g >= 1, its four
// values 3g-2 .. 3g+1 lie below ncopy AND in one piece, and then loads them by
// that piece's format; every other lane (the header, a window across a segment
// seam, the window that holds ncopy, the zero tail, the origin) goes byte by
// byte through the "flat value i" accessor over the job's pieces.  Nothing is
// added to anything: a -0.0 value is -0.0 in the text.
// ---------------------------------------------------------------------------
struct SegEncJob {
  unsigned char hdr[16];          // 14 header bytes
  int64_t L;                      // doubles in the payload
  int64_t ncopy;                  // of which copied from the segments
  int64_t piece_lo, piece_hi;     // the partition's pieces
  int64_t origin_len;
  const unsigned char* origin;    // device copy of the origin bytes
  unsigned char* out;
  int64_t groups;
  int64_t text_len;
};

__global__ __launch_bounds__(kBlock) void k_b64url_encode_segs(const SegEncJob* __restrict__ jobs,
                                                               const SegPiece* __restrict__ pieces) {
  __shared__ u4w stage[2 * kBlock];
  __shared__ unsigned char tab[64];
  init_b64url_table(tab);
  const SegEncJob& j = jobs[blockIdx.y];
  const int64_t L = j.L, ncopy = j.ncopy, groups = j.groups;
  const int plo = (int)j.piece_lo, phi = (int)j.piece_hi;
  const int64_t F = 14 + 8 * L + j.origin_len;   // frame bytes
  auto value_bits = [&](int64_t i) -> unsigned long long {   // payload value i < ncopy
    const SegPiece pc = pieces[seg_piece_of(pieces, plo, phi, i)];
    return __builtin_bit_cast(unsigned long long, seg_load(pc.src, i - pc.dst, (int)pc.fmt));
  };
  auto frame_byte_at = [&](int64_t b) -> unsigned {
    if (b < 14) return j.hdr[b];
    const int64_t q = b - 14;
    if (q >= 8 * L) return j.origin[q - 8 * L];
    const int64_t i = q >> 3;
    const unsigned long long v = i < ncopy ? value_bits(i) : i == ncopy ? 0x3FF0000000000000ull : 0ull;
    return (unsigned)(v >> (8 * (7 - (q & 7)))) & 0xFF;   // putDouble: big-endian
  };
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u4w* ws = stage + 128 * wv;
  for (int64_t g0 = (int64_t)blockIdx.x * kBlock; g0 < groups; g0 += (int64_t)gridDim.x * kBlock) {
    const int64_t gw = g0 + 64 * wv;                // this wave's first group
    const int64_t g = gw + lane;
    u4w c0 = {0u, 0u, 0u, 0u}, c1 = {0u, 0u, 0u, 0u};
    bool done = g >= groups;
    if (!done && g >= 1 && 3 * g + 2 <= ncopy) {
      const int64_t i = 3 * g - 2;
      const SegPiece pc = pieces[seg_piece_of(pieces, plo, phi, i)];
      if (i + 4 <= pc.dst + pc.n) {
        const int64_t e = i - pc.dst;
        const int fmt = (int)pc.fmt;
        const unsigned long long v0 = __builtin_bit_cast(unsigned long long, seg_load(pc.src, e, fmt));
        const unsigned long long v1 = __builtin_bit_cast(unsigned long long, seg_load(pc.src, e + 1, fmt));
        const unsigned long long v2 = __builtin_bit_cast(unsigned long long, seg_load(pc.src, e + 2, fmt));
        const unsigned long long v3 = __builtin_bit_cast(unsigned long long, seg_load(pc.src, e + 3, fmt));
        window_chars(v0, v1, v2, v3, tab, c0, c1);
        done = true;
      }
    }
    if (!done) {
      unsigned q8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      for (int u = 0; u < 8; ++u) {
        const int64_t b = 24 * g + 3 * u;
        if (b >= F) break;
        const int nb = F - b >= 3 ? 3 : (int)(F - b);
        unsigned v = frame_byte_at(b) << 16;
        if (nb > 1) v |= frame_byte_at(b + 1) << 8;
        if (nb > 2) v |= frame_byte_at(b + 2);
        q8[u] = padded_quad(v, nb);
      }
      c0 = u4w{q8[0], q8[1], q8[2], q8[3]};
      c1 = u4w{q8[4], q8[5], q8[6], q8[7]};
    }
    store_wave_text(ws, lane, c0, c1, j.out, gw, j.text_len);
  }
}

}  // namespace ipls
