// seg_peers_kernels.hpp -- the kernel of the peer-list call
// (ipls_agg_update_gradient_segs_peers; include/ipls_agg.h): K segment lists
// over one table of lengths and formats, the trained parameters of K trainers
// that share one architecture, folded into the accumulators in one launch.
// Peer k's flat value f = start_s + e is (double) t_k[s][e] (DIFF false), or
// (double) sub_kind(m[s][e], t_k[s][e]) with one shared minuend list m (DIFF
// true), the subtraction seg_diff_kernels.hpp's seg_sub: made in the segment's
// own format, rounded by the format's narrow, only the result widened.
//   dst[i] = (((start + v_0) + .. + v_0) + v_1 + ..) + v_{K-1},
// every peer's value added `mult` times in a row (the job's multiplicity: how
// often its partition stands in `owned`) before the next peer's, start = +0.0
// when the accumulator is logically zero; at the count slot v_k = 1.0, above
// it 0.0, the adds always made.  Nothing on the peer axis is reassociated, so
// the bits are those of K calls of the single-peer twin in peer order.
// The plan, the items and the pieces are seg_kernels.hpp's, made from the
// shared table (with the addresses of the minuend list, or of peer 0); the
// peers travel as psrc[piece * K + k], the piece's first element in peer k's
// list, a parallel array in the same upload.  No list's alignment is read from
// the plan: a whole tile takes each one's from its address, block-uniform.
// Built without contraction and without fast-math, no LDS, vector stores only.
// Included by engine.hip after seg_diff_kernels.hpp.
#pragma once

#include "seg_diff_kernels.hpp"

namespace ipls {

// Peers whose loads a whole tile issues before the group's arithmetic
// (DESIGN.md §3.9 has the sweep over 2, 4 and 8: 2 is the fastest, at occupancy 7 to 8).
#ifndef IPLS_SEG_PEERS_G
#define IPLS_SEG_PEERS_G 2
#endif
constexpr int kSegPeersG = IPLS_SEG_PEERS_G;

// SegJob with the multiplicity of the job's partition in `owned`.
struct SegPeersJob {
  unsigned long long* dst;    // the accumulator (256-B aligned)
  int64_t ncopy, L;
  int32_t zero;               // logically +0.0: written without being read
  int32_t mult;               // every peer's value is added this often in a row (>= 1)
};

// Four consecutive trainer-format elements of one list as a lane holds them
// between the loads and the arithmetic.  Whether the list takes one aligned
// non-temporal vector load or four naturally aligned element loads is a
// run-time fact of its address, uniform over the block.
template <class S, int ESZ = sizeof(typename S::raw)>
struct PeerQuad {   // 4-byte elements: the same registers either way
  typename S::raw el[4];
  __device__ __forceinline__ void load(const typename S::elem* p, bool al) {
    if (al) {
      const typename S::template Vec<4> v = S::template ldv<4>(p);
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = S::ldraw(p + c);
    }
  }
  __device__ __forceinline__ typename S::raw get(int c, bool) const { return el[c]; }
};
template <class S>
struct PeerQuad<S, 2> {   // 16-bit elements: two words of a vector load, or one element per word
  unsigned w[4];
  __device__ __forceinline__ void load(const typename S::elem* p, bool al) {
    if (al) {
      const typename S::template Vec<4> v = S::template ldv<4>(p);
      w[0] = v.w[0], w[1] = v.w[1], w[2] = 0u, w[3] = 0u;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) w[c] = S::ldraw(p + c);
    }
  }
  __device__ __forceinline__ typename S::raw get(int c, bool al) const {
    return (typename S::raw)(al ? w[c >> 1] >> (16 * (c & 1)) : w[c]);
  }
};

// ---------------------------------------------------------------------------
// A `whole` item of format S: the accumulator tile and the minuend tile are
// loaded once, the peers are walked in order in groups of kSegPeersG whose
// loads are all issued before the group's arithmetic, and the sums are stored
// once after the last peer with the twins' 16-B stores (lane ^ 4 exchange for
// the trainer formats).  m: the tile's first minuend element (DIFF);
// psrc: the piece's K peer pointers; e: the tile's first element in the piece.
// Every load reads elements [e, e + kSegTile) of its piece and nothing else.
// ---------------------------------------------------------------------------
template <class S, bool DIFF>
__device__ __forceinline__ void update_segs_peers_whole(const typename S::elem* m,
                                                        const void* const* __restrict__ psrc, int64_t e, int K,
                                                        int mult, unsigned long long* dst, int64_t base, bool zero) {
  typedef typename S::elem T;
  constexpr int G = kSegPeersG;
  const int tid = threadIdx.x;
  if constexpr (sizeof(T) == 8) {
    constexpr int R = kSegV / 2;
    auto load2 = [](const T* p, bool al) -> u2 {
      if (al) return __builtin_nontemporal_load((gcu2)p);
      u2 v;
      v.x = ld8(p);
      v.y = ld8(p + 1);
      return v;
    };
    u2 mv[R];
    d2 acc[R];
    const bool m_al = DIFF && ((uintptr_t)m & 15) == 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = 2 * ((int64_t)r * kBlock + tid);
      if constexpr (DIFF) mv[r] = load2(m + i, m_al);
      acc[r] = zero ? d2{0.0, 0.0} : __builtin_bit_cast(d2, *(gcu2)(dst + base + i));   // +0.0 when logically zero
    }
    for (int k0 = 0; k0 < K; k0 += G) {
      u2 pv[G][R];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (k0 + g < K) {
          const T* p = (const T*)psrc[k0 + g] + e;
          const bool al = ((uintptr_t)p & 15) == 0;
#pragma unroll
          for (int r = 0; r < R; ++r) pv[g][r] = load2(p + 2 * ((int64_t)r * kBlock + tid), al);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (k0 + g < K) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            d2 v = decode2<false>(pv[g][r]);
            if constexpr (DIFF) {
              const d2 a = decode2<false>(mv[r]);
              v = d2{a.x - v.x, a.y - v.y};
            }
            for (int t = 0; t < mult; ++t) acc[r] = d2{acc[r].x + v.x, acc[r].y + v.y};
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = 2 * ((int64_t)r * kBlock + tid);
      *(gu2)(dst + base + i) = encode2<false>(acc[r]);
    }
  } else {
    constexpr int R = kSegV / 4;
    constexpr uintptr_t kMask = sizeof(T) == 4 ? 15 : 7;   // a 16-B load, 8 B of 16-bit elements
    PeerQuad<S> qm[R];
    double acc[R][4];
    const bool m_al = DIFF && ((uintptr_t)m & kMask) == 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = 4 * ((int64_t)r * kBlock + tid);
      if constexpr (DIFF) qm[r].load(m + i, m_al);
      u2 t0 = u2{0, 0}, t1 = u2{0, 0};   // +0.0 when the accumulator is logically zero
      if (!zero) {
        t0 = ld16<false>(dst + base + i);
        t1 = ld16<false>(dst + base + i + 2);
      }
      const d2 x = __builtin_bit_cast(d2, t0), y = __builtin_bit_cast(d2, t1);
      acc[r][0] = x.x, acc[r][1] = x.y, acc[r][2] = y.x, acc[r][3] = y.y;
    }
    for (int k0 = 0; k0 < K; k0 += G) {
      PeerQuad<S> q[G][R];
      bool al[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        al[g] = false;
        if (k0 + g < K) {
          const T* p = (const T*)psrc[k0 + g] + e;
          al[g] = ((uintptr_t)p & kMask) == 0;
#pragma unroll
          for (int r = 0; r < R; ++r) q[g][r].load(p + 4 * ((int64_t)r * kBlock + tid), al[g]);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (k0 + g < K) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            double v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if constexpr (DIFF) v[c] = seg_sub<S>(qm[r].get(c, m_al), q[g][r].get(c, al[g]));
              else v[c] = S::widen(q[g][r].get(c, al[g]));
            }
            for (int t = 0; t < mult; ++t) {
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[r][c] = acc[r][c] + v[c];
            }
          }
        }
      }
    }
    const bool hi = tid & 4;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // k_update_segs's stores: lanes 8k..8k+3 own one 128-B line of sums, 8k+4..8k+7 the next
      const int64_t o = base + 4 * ((int64_t)r * kBlock + tid);
      const d2 own = d2{acc[r][0], acc[r][1]};
      const d2 got = d2{__shfl_xor(acc[r][2], 4), __shfl_xor(acc[r][3], 4)};
      __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
      __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
    }
  }
}

// pieces[k].src: the piece's first minuend element (DIFF; not read otherwise);
// psrc[k * K + p]: its first element in peer p's list.
template <bool DIFF>
__global__ __launch_bounds__(kBlock) void k_update_segs_peers(const segplan::Item* __restrict__ items,
                                                              const SegPeersJob* __restrict__ jobs,
                                                              const SegPiece* __restrict__ pieces,
                                                              const void* const* __restrict__ psrc, int K) {
  const segplan::Item it = items[blockIdx.x];
  const SegPeersJob j = jobs[it.job];
  const bool zero = j.zero != 0;
  const int mult = j.mult;
  if (it.whole) {
    const SegPiece pc = pieces[it.piece_lo];
    const void* const* pp = psrc + (int64_t)it.piece_lo * K;
    const int64_t e = it.lo - pc.dst;   // the tile's first element in the piece
    switch (it.fmt) {
      case segplan::kF64:
        update_segs_peers_whole<FmtD64, DIFF>((const unsigned long long*)pc.src + e, pp, e, K, mult, j.dst, it.lo, zero);
        break;
      case segplan::kF32:
        update_segs_peers_whole<FmtF32, DIFF>((const float*)pc.src + e, pp, e, K, mult, j.dst, it.lo, zero);
        break;
      case segplan::kF16:
        update_segs_peers_whole<FmtF16, DIFF>((const unsigned short*)pc.src + e, pp, e, K, mult, j.dst, it.lo, zero);
        break;
      default:
        update_segs_peers_whole<FmtBF16, DIFF>((const unsigned short*)pc.src + e, pp, e, K, mult, j.dst, it.lo, zero);
        break;
    }
    return;
  }
  for (int64_t i = it.lo + threadIdx.x; i < it.hi; i += kBlock) {
    double acc = zero ? 0.0 : __builtin_bit_cast(double, ld8(j.dst + i));
    if (i < j.ncopy) {
      const int k = seg_piece_of(pieces, it.piece_lo, it.piece_hi, i);
      const SegPiece pc = pieces[k];
      const void* const* pp = psrc + (int64_t)k * K;
      for (int p = 0; p < K; ++p) {
        const double v = DIFF ? seg_diff_load(pc.src, pp[p], i - pc.dst, (int)pc.fmt)
                              : seg_load(pp[p], i - pc.dst, (int)pc.fmt);
        for (int t = 0; t < mult; ++t) acc = acc + v;
      }
    } else {
      const double v = i == j.ncopy ? 1.0 : 0.0;
      for (int64_t t = 0; t < (int64_t)K * mult; ++t) acc = acc + v;
    }
    st8(j.dst + i, __builtin_bit_cast(unsigned long long, acc));
  }
}

}  // namespace ipls
