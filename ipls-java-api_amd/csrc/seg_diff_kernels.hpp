// seg_diff_kernels.hpp -- the kernels of the difference-list calls
// (ipls_agg_update_gradient_segs_diff, ipls_agg_send_gradients_segs_diff;
// include/ipls_agg.h): a segment list with two pointer tables over one table
// of lengths and formats.  Flat value f = start_s + e is
//   (double) sub_k(a[s][e], b[s][e]),
// the subtraction made in the segment's own format (Model.java:126-128,
// Dumm.sub(params) in the INDArray's data type; only the result is widened):
// doubles and floats subtract natively (one rounding, subnormals kept), the
// 16-bit formats as (float)a - (float)b rounded to nearest-even into the
// format by the narrowing the divide kernels use (overflow to +-inf,
// subnormals kept), then widened by the format's rule.  Built without
// contraction and without fast-math, like everything else here.
// The plan, the pieces and the jobs are seg_kernels.hpp's, made from the
// minuend list; the subtrahend travels as one pointer per piece (the piece's
// first subtrahend element), a parallel array in the same upload.  Its
// alignment is not in the plan: a whole tile takes it from the address.
// Included by engine.hip after seg_kernels.hpp.
#pragma once

#include "seg_kernels.hpp"

namespace ipls {

// a - b in format S, widened.
template <class S>
__device__ __forceinline__ double seg_sub(typename S::raw a, typename S::raw b) {
  if constexpr (sizeof(typename S::raw) == 4) {
    return (double)(a - b);
  } else {
    const float d = (float)S::widen(a) - (float)S::widen(b);   // the widenings are exact, so are these casts
    return S::widen((typename S::raw)S::narrow(d));
  }
}

// Element e of the difference of two arrays of format fmt (a run-time value), widened.
__device__ __forceinline__ double seg_diff_load(const void* a, const void* b, int64_t e, int fmt) {
  switch (fmt) {
    case segplan::kF64:
      return __builtin_bit_cast(double, ld8((const unsigned long long*)a + e)) -
             __builtin_bit_cast(double, ld8((const unsigned long long*)b + e));
    case segplan::kF32: return seg_sub<FmtF32>(FmtF32::ldraw((const float*)a + e), FmtF32::ldraw((const float*)b + e));
    case segplan::kF16:
      return seg_sub<FmtF16>(FmtF16::ldraw((const unsigned short*)a + e), FmtF16::ldraw((const unsigned short*)b + e));
    default:
      return seg_sub<FmtBF16>(FmtBF16::ldraw((const unsigned short*)a + e), FmtBF16::ldraw((const unsigned short*)b + e));
  }
}

// Four consecutive trainer-format elements of one source as a lane holds them
// between the loads and the subtract: one aligned non-temporal vector load
// (AL), or four naturally aligned element loads.
template <class S, bool AL>
struct SegQuad {
  typename S::template Vec<4> v;
  typename S::raw el[4];
  __device__ __forceinline__ void load(const typename S::elem* p) {
    if constexpr (AL) {
      v = S::template ldv<4>(p);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = S::ldraw(p + c);
    }
  }
  __device__ __forceinline__ typename S::raw get(int c) const {
    if constexpr (!AL) return el[c];
    else if constexpr (sizeof(typename S::raw) == 4) return v[c];
    else return (typename S::raw)(v.w[c >> 1] >> (16 * (c & 1)));
  }
};

// ---------------------------------------------------------------------------
// k_update_segs_diff: k_update_segs with the value of element i the difference
// of the two lists,
//   dst[i] = (zero ? +0.0 : dst[i]) + (double)sub(a_i, b_i)   for i < ncopy,
// 1.0 at ncopy, 0.0 above, the add always made.  The decomposition is
// k_update_segs's: a `whole` item is block-uniform, dispatched by format
// outside the loops; each source on its own takes aligned non-temporal vector
// loads when its residue against a 16-B load (8 B of 16-bit elements) is 0 and
// naturally aligned element loads otherwise -- four combinations per format,
// block-uniform.  All loads of both lists and of the accumulator first, then
// subtract, round to the format, widen and add, then the 16-B stores of which
// one instruction of a wave writes whole 128-B lines.  No load touches a byte
// outside its piece in either list.  Every other item goes element by element.
// ---------------------------------------------------------------------------
template <class S>
__device__ __forceinline__ void update_segs_diff_whole(const typename S::elem* a, const typename S::elem* b,
                                                       unsigned long long* dst, int64_t base, bool zero, bool a_al,
                                                       bool b_al) {
  typedef typename S::elem T;
  const int tid = threadIdx.x;
  if constexpr (sizeof(T) == 8) {
    constexpr int R = kSegV / 2;
    auto body = [&](auto aal, auto bal) {
      constexpr bool AA = decltype(aal)::value, BA = decltype(bal)::value;
      u2 av[R], bv[R], dv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 2 * ((int64_t)r * kBlock + tid);
        if constexpr (AA) {
          av[r] = __builtin_nontemporal_load((gcu2)(a + i));
        } else {
          av[r].x = ld8(a + i);
          av[r].y = ld8(a + i + 1);
        }
        if constexpr (BA) {
          bv[r] = __builtin_nontemporal_load((gcu2)(b + i));
        } else {
          bv[r].x = ld8(b + i);
          bv[r].y = ld8(b + i + 1);
        }
        if (!zero) dv[r] = *(gcu2)(dst + base + i);
        else dv[r] = u2{0, 0};
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 2 * ((int64_t)r * kBlock + tid);
        const d2 x = decode2<false>(av[r]), y = decode2<false>(bv[r]);
        const d2 acc = __builtin_bit_cast(d2, dv[r]);   // +0.0 when the accumulator is logically zero
        *(gu2)(dst + base + i) = encode2<false>(d2{acc.x + (x.x - y.x), acc.y + (x.y - y.y)});
      }
    };
    if (a_al && b_al) body(std::true_type{}, std::true_type{});
    else if (a_al) body(std::true_type{}, std::false_type{});
    else if (b_al) body(std::false_type{}, std::true_type{});
    else body(std::false_type{}, std::false_type{});
  } else {
    constexpr int R = kSegV / 4;
    auto body = [&](auto aal, auto bal) {
      SegQuad<S, decltype(aal)::value> qa[R];
      SegQuad<S, decltype(bal)::value> qb[R];
      u2 t[R][2];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t i = 4 * ((int64_t)r * kBlock + tid);
        qa[r].load(a + i);
        qb[r].load(b + i);
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
        for (int c = 0; c < 4; ++c) v[c] = seg_sub<S>(qa[r].get(c), qb[r].get(c));
        const d2 x = __builtin_bit_cast(d2, t[r][0]), y = __builtin_bit_cast(d2, t[r][1]);
        const double a0 = x.x + v[0], a1 = x.y + v[1], a2 = y.x + v[2], a3 = y.y + v[3];
        // k_update_segs's stores: lanes 8k..8k+3 own one 128-B line of sums, 8k+4..8k+7 the next
        const int64_t o = base + 4 * ((int64_t)r * kBlock + tid);
        const d2 own = d2{a0, a1};
        const d2 got = d2{__shfl_xor(a2, 4), __shfl_xor(a3, 4)};
        __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
        __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
      }
    };
    if (a_al && b_al) body(std::true_type{}, std::true_type{});
    else if (a_al) body(std::true_type{}, std::false_type{});
    else if (b_al) body(std::false_type{}, std::true_type{});
    else body(std::false_type{}, std::false_type{});
  }
}

// bsrc[k]: the first subtrahend element of piece k (pieces[k].src is the minuend's)
__global__ __launch_bounds__(kBlock) void k_update_segs_diff(const segplan::Item* __restrict__ items,
                                                             const SegJob* __restrict__ jobs,
                                                             const SegPiece* __restrict__ pieces,
                                                             const void* const* __restrict__ bsrc) {
  const segplan::Item it = items[blockIdx.x];
  const SegJob j = jobs[it.job];
  const bool zero = j.zero != 0;
  if (it.whole) {
    const SegPiece pc = pieces[it.piece_lo];
    const void* pb = bsrc[it.piece_lo];
    const int64_t e = it.lo - pc.dst;   // the tile's first element in the piece
    switch (it.fmt) {
      case segplan::kF64: {
        const unsigned long long* b = (const unsigned long long*)pb + e;
        update_segs_diff_whole<FmtD64>((const unsigned long long*)pc.src + e, b, j.dst, it.lo, zero, it.res == 0,
                                       ((uintptr_t)b & 15) == 0);
        break;
      }
      case segplan::kF32: {
        const float* b = (const float*)pb + e;
        update_segs_diff_whole<FmtF32>((const float*)pc.src + e, b, j.dst, it.lo, zero, it.res == 0,
                                       ((uintptr_t)b & 15) == 0);
        break;
      }
      case segplan::kF16: {
        const unsigned short* b = (const unsigned short*)pb + e;
        update_segs_diff_whole<FmtF16>((const unsigned short*)pc.src + e, b, j.dst, it.lo, zero, (it.res & 3) == 0,
                                       ((uintptr_t)b & 7) == 0);
        break;
      }
      default: {
        const unsigned short* b = (const unsigned short*)pb + e;
        update_segs_diff_whole<FmtBF16>((const unsigned short*)pc.src + e, b, j.dst, it.lo, zero, (it.res & 3) == 0,
                                        ((uintptr_t)b & 7) == 0);
        break;
      }
    }
    return;
  }
  for (int64_t i = it.lo + threadIdx.x; i < it.hi; i += kBlock) {
    double v;
    if (i < j.ncopy) {
      const int k = seg_piece_of(pieces, it.piece_lo, it.piece_hi, i);
      const SegPiece pc = pieces[k];
      v = seg_diff_load(pc.src, bsrc[k], i - pc.dst, (int)pc.fmt);
    } else {
      v = i == j.ncopy ? 1.0 : 0.0;
    }
    const double acc = zero ? 0.0 : __builtin_bit_cast(double, ld8(j.dst + i));
    st8(j.dst + i, __builtin_bit_cast(unsigned long long, acc + v));
  }
}

// ---------------------------------------------------------------------------
// k_b64url_encode_segs_diff: k_b64url_encode_segs with the "flat value i"
// accessor the difference of the two lists.  Same decomposition: a lane is
// fast when its four values lie below ncopy and in one piece; every other lane
// goes byte by byte.  Nothing is added to anything: a -0.0 difference is -0.0
// in the text.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_b64url_encode_segs_diff(const SegEncJob* __restrict__ jobs,
                                                                    const SegPiece* __restrict__ pieces,
                                                                    const void* const* __restrict__ bsrc) {
  __shared__ u4w stage[2 * kBlock];
  __shared__ unsigned char tab[64];
  init_b64url_table(tab);
  const SegEncJob& j = jobs[blockIdx.y];
  const int64_t L = j.L, ncopy = j.ncopy, groups = j.groups;
  const int plo = (int)j.piece_lo, phi = (int)j.piece_hi;
  const int64_t F = 14 + 8 * L + j.origin_len;   // frame bytes
  auto value_bits = [&](int64_t i) -> unsigned long long {   // payload value i < ncopy
    const int k = seg_piece_of(pieces, plo, phi, i);
    const SegPiece pc = pieces[k];
    return __builtin_bit_cast(unsigned long long, seg_diff_load(pc.src, bsrc[k], i - pc.dst, (int)pc.fmt));
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
      const int k = seg_piece_of(pieces, plo, phi, i);
      const SegPiece pc = pieces[k];
      if (i + 4 <= pc.dst + pc.n) {
        const void* pb = bsrc[k];
        const int64_t e = i - pc.dst;
        const int fmt = (int)pc.fmt;
        const unsigned long long v0 = __builtin_bit_cast(unsigned long long, seg_diff_load(pc.src, pb, e, fmt));
        const unsigned long long v1 = __builtin_bit_cast(unsigned long long, seg_diff_load(pc.src, pb, e + 1, fmt));
        const unsigned long long v2 = __builtin_bit_cast(unsigned long long, seg_diff_load(pc.src, pb, e + 2, fmt));
        const unsigned long long v3 = __builtin_bit_cast(unsigned long long, seg_diff_load(pc.src, pb, e + 3, fmt));
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
