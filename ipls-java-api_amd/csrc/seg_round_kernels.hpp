// seg_round_kernels.hpp -- the kernel of the many-trainers round
// (ipls_agg_round_segs_peers; include/ipls_agg.h): K trainers' segment lists
// folded over the accumulators, W = that + REP, and W divided by its count into
// n_lists output lists, in one pass over one shard's partitions -- the end
// state of k_update_segs_peers, k_finalize and k_divide_segs_copies run one
// after another, with AGG never stored and W never read back.
// Per element i of an OWNED partition (the job's mult >= 1):
//   s    = (((start + v_0) .. mult times) + v_1 ..) + v_{K-1}   seg_peers_kernels.hpp's value rule: start = +0.0
//          when AGG is logically zero, v_k = 1.0 at the count slot, 0.0 above it, the adds always made;
//   W[i] = s + (REP logically zero ? +0.0 : REP[i])             k_finalize's two forms: a -0.0 sum becomes +0.0;
//   cnt  = W's count slot, computed by every block from AGG[L-1] (or +0.0), the K * mult additions of 1.0 made one
//          after another and REP[L-1] (or +0.0): W[L-1] of an owned partition is never read, another block of the
//          same launch writes it;
// of a partition that is NOT owned (mult == 0) W is only read, cnt = W[L-1].  Then, for i < ncopy, every list k gets
//   out_k = narrow(cnt == 0.0 ? W[i] : W[i] / den),  den = cnt (secure: 1e12 * cnt),
// k_divide_segs's value: the IEEE double division, rounded once to float for F32 and from that float to the format
// for F16 / BF16, doubles stored as they are.  The count slot and the tail go to W only.
// The plan is k_update_segs's over ALL partitions of the shard (one item per destination tile, no tile in two
// items); the peers travel as psrc[piece * K + k] and the outputs as pdst[piece * n_lists + k], the piece's first
// element in peer k's / list k's array.  No list's alignment is read from the plan.
//
// IN PLACE.  An output list may be the very arrays of the minuend list or of a peer list (same pointer, same
// segment, same table).  The invariant that makes that safe: AN ELEMENT OF THE OUTPUT LISTS IS STORED BY THE BLOCK
// THAT LOADED THAT ELEMENT OF THE INPUT LISTS, AND BY NO OTHER, AFTER EVERY LOAD OF THE BLOCK.  A whole tile's lane
// tid HOLDS elements [4 (r kBlock + tid), + 4) (two for doubles) of every input.  From an aligned list it loads
// exactly those and into an aligned list it stores exactly those; at a misaligned list the loads and the stores are
// aligned vectors shifted by one lane inside the wave (RoundQuad below; the store loop), so a lane reads and writes
// list elements another lane of its wave holds: hence the __syncthreads() between the last load and the first list
// store of a whole tile.  (The values stored also depend
// on every one of those loads, and the exchange never leaves the wave.)  Every other item handles element i in one
// lane from its loads to its stores.  (The lane ^ 4 exchange moves W's values only: W is no input.)  No store
// layout may ever write an element of a list that another BLOCK reads.
// Built without contraction and without fast-math, no LDS, vector stores only.
// Included by engine.hip after seg_copies_kernels.hpp.
#pragma once

#include "seg_copies_kernels.hpp"
#include "seg_peers_kernels.hpp"

namespace ipls {

struct SegRoundJob {
  const unsigned long long* agg;   // the accumulators (256-B aligned); not read when logically zero
  const unsigned long long* rep;
  unsigned long long* w;           // Weights: written when owned, read when not
  int64_t ncopy, L;
  int32_t agg_zero, rep_zero;      // logically +0.0
  int32_t mult;                    // how often the partition stands in `owned`; 0: not owned, the divide alone
  int32_t pad_;
};

// At a list whose tile is misaligned: 0 -- naturally aligned element loads and stores for every format; 1 -- aligned
// vectors shifted by one lane inside each wave, for the peers' loads and the lists' stores alike, where the
// elements are 4 or 8 bytes wide, element loads and stores for the 16-bit formats; 2 -- shifted vectors for every
// format.  1 is what measured fastest (f32 is faster shifted, bf16 faster element by element: DESIGN.md §3.11);
// 0 and 2 are build variants (lib/ab/libipls_agg_roundshift0.so, ..2.so; tools/seg_round_probe.py).
#ifndef IPLS_SEG_ROUND_SHIFT
#define IPLS_SEG_ROUND_SHIFT 1
#endif
template <class T>
constexpr bool seg_round_shift() { return IPLS_SEG_ROUND_SHIFT >= (sizeof(T) == 2 ? 2 : 1); }

// Four consecutive trainer-format elements of one peer list as a lane holds them between the loads and the
// arithmetic.  `chunk` is the first of the 256 elements the lane's WAVE holds in this step (lane t holds elements
// [4t, 4t + 4) of them), a the residue of that address against an aligned vector of four elements, in elements,
// uniform over the block.  a == 0: one aligned non-temporal vector load per lane.  Otherwise the 63 aligned vectors
// that lie wholly inside the chunk -- elements [4 - a + 4t, 8 - a + 4t) -- go to lanes 0 .. 62, and lane 63 loads
// the four elements they leave, the chunk's first 4 - a and last a, one by one into the places a 64th vector would
// have them; finish() then takes the places a .. 3 of the previous lane's vector (lane 63's for lane 0) and the
// places 0 .. a-1 of the lane's own.  No load touches a byte outside the chunk.
template <class S, int ESZ = sizeof(typename S::raw)>
struct RoundQuad {   // 4-byte elements
  typename S::raw el[4];
  __device__ __forceinline__ void load(const typename S::elem* chunk, int lane, int a) {
    if (a == 0) {
      const typename S::template Vec<4> v = S::template ldv<4>(chunk + 4 * lane);
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = v[c];
    } else if (!seg_round_shift<typename S::elem>()) {
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = S::ldraw(chunk + 4 * lane + c);
    } else if (lane < 63) {
      const typename S::template Vec<4> v = S::template ldv<4>(chunk + (4 - a) + 4 * lane);
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) el[c] = S::ldraw(c < a ? chunk + 256 - a + c : chunk + c - a);
    }
  }
  __device__ __forceinline__ void finish(int lane, int a) {
    if (a == 0 || !seg_round_shift<typename S::elem>()) return;
    const int src = (lane + 63) & 63;
    const typename S::raw p1 = __shfl(el[1], src), p2 = __shfl(el[2], src), p3 = __shfl(el[3], src);
    const typename S::raw v0 = el[0], v1 = el[1], v2 = el[2];
    if (a == 1) el[0] = p1, el[1] = p2, el[2] = p3, el[3] = v0;
    else if (a == 2) el[0] = p2, el[1] = p3, el[2] = v0, el[3] = v1;
    else el[0] = p3, el[1] = v0, el[2] = v1, el[3] = v2;
  }
  __device__ __forceinline__ typename S::raw get(int c) const { return el[c]; }
};
template <class S>
struct RoundQuad<S, 2> {   // 16-bit elements: two packed words
  unsigned w[2];
  __device__ __forceinline__ void load(const typename S::elem* chunk, int lane, int a) {
    if (a == 0 || (seg_round_shift<typename S::elem>() && lane < 63)) {
      const typename S::template Vec<4> v = S::template ldv<4>(chunk + (a == 0 ? 0 : 4 - a) + 4 * lane);
      w[0] = v.w[0], w[1] = v.w[1];
    } else {
      unsigned x[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        x[c] = S::ldraw(!seg_round_shift<typename S::elem>() ? chunk + 4 * lane + c : c < a ? chunk + 256 - a + c : chunk + c - a);
      w[0] = x[0] | (x[1] << 16), w[1] = x[2] | (x[3] << 16);
    }
  }
  __device__ __forceinline__ void finish(int lane, int a) {
    if (a == 0 || !seg_round_shift<typename S::elem>()) return;
    const int src = (lane + 63) & 63;
    const unsigned long long prev = (unsigned long long)__shfl(w[0], src) | ((unsigned long long)__shfl(w[1], src) << 32);
    const unsigned long long own = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    const unsigned long long y = (prev >> (16 * a)) | (own << (64 - 16 * a));   // a is 1, 2 or 3
    w[0] = (unsigned)y, w[1] = (unsigned)(y >> 32);
  }
  __device__ __forceinline__ typename S::raw get(int c) const {
    return (typename S::raw)(w[c >> 1] >> (16 * (c & 1)));
  }
};

// The count an OWNED partition ends with: k_update_segs_peers's count slot, then k_finalize's add.
__device__ __forceinline__ double round_count(const SegRoundJob& j, int K) {
  double cnt = j.agg_zero ? 0.0 : __builtin_bit_cast(double, ld8(j.agg + j.L - 1));
  for (int64_t t = 0; t < (int64_t)K * j.mult; ++t) cnt = cnt + 1.0;
  return cnt + (j.rep_zero ? 0.0 : __builtin_bit_cast(double, ld8(j.rep + j.L - 1)));
}

// ---------------------------------------------------------------------------
// A `whole` item of format S (a full tile inside one piece, so below ncopy).
// Owned: update_segs_peers_whole's structure -- the AGG tile (or +0.0) and the
// minuend tile are loaded once, the peers are walked in order in groups of
// kSegPeersG whose loads are all issued before the group's arithmetic, the
// count chain runs beside the lane's eight; then the REP tile (or +0.0) is
// loaded and added, W stored with the twins' 16-B stores, and the quotients
// stored to every list in order.  Not owned: the W tile is loaded in the same
// lane layout.
// A list whose tile starts 16-B aligned (8 B of 16-bit elements) takes one
// non-temporal vector store per lane and group of elements.  At any other
// address, where the elements are 4 or 8 bytes wide, the vectors are shifted
// by one lane inside each wave so that they are aligned again, and only the
// first and the last lane of a wave store single naturally aligned elements;
// the peers' loads do the same (RoundQuad).  The 16-bit formats take naturally
// aligned element loads and stores there, which measured faster for them
// (DESIGN.md §3.11).  The choice is block-uniform
// per list.  No load or store leaves elements [e, e + kSegTile) of its piece.
// ---------------------------------------------------------------------------
template <class S, bool DIFF, bool SECURE>
__device__ __forceinline__ void round_segs_peers_whole(const typename S::elem* m, const void* const* __restrict__ psrc,
                                                       int K, void* const* __restrict__ pdst, int n_lists, int64_t e,
                                                       const SegRoundJob& j, int64_t base) {
  typedef typename S::elem T;
  constexpr int G = kSegPeersG;
  constexpr int EL = sizeof(T) == 8 ? 2 : 4;   // consecutive elements a lane owns per step
  constexpr int R = kSegV / EL;
  const int tid = threadIdx.x;
  const int mult = j.mult;
  double wv[R][EL];
  double cnt;
  if (mult == 0) {   // block-uniform: the divide alone
    cnt = __builtin_bit_cast(double, ld8(j.w + j.L - 1));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = base + EL * ((int64_t)r * kBlock + tid);
#pragma unroll
      for (int c = 0; c < EL; c += 2) {
        const d2 x = __builtin_bit_cast(d2, ld16<true>(j.w + i + c));
        wv[r][c] = x.x, wv[r][c + 1] = x.y;
      }
    }
  } else {
    const bool zero = j.agg_zero != 0, rzero = j.rep_zero != 0;
    cnt = zero ? 0.0 : __builtin_bit_cast(double, ld8(j.agg + j.L - 1));
    const double rcnt = rzero ? 0.0 : __builtin_bit_cast(double, ld8(j.rep + j.L - 1));
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = base + EL * ((int64_t)r * kBlock + tid);
#pragma unroll
      for (int c = 0; c < EL; c += 2) {
        u2 a = u2{0, 0};   // +0.0 when the accumulator is logically zero
        if (!zero) a = ld16<false>(j.agg + i + c);
        const d2 x = __builtin_bit_cast(d2, a);
        wv[r][c] = x.x, wv[r][c + 1] = x.y;
      }
    }
    if constexpr (sizeof(T) == 8) {
      auto load2 = [](const T* p, bool al) -> u2 {
        if (al) return __builtin_nontemporal_load((gcu2)p);
        u2 v;
        v.x = ld8(p);
        v.y = ld8(p + 1);
        return v;
      };
      u2 mv[R];
      const bool m_al = DIFF && ((uintptr_t)m & 15) == 0;
      if constexpr (DIFF) {
#pragma unroll
        for (int r = 0; r < R; ++r) mv[r] = load2(m + 2 * ((int64_t)r * kBlock + tid), m_al);
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
              for (int t = 0; t < mult; ++t) wv[r][0] = wv[r][0] + v.x, wv[r][1] = wv[r][1] + v.y;
            }
            for (int t = 0; t < mult; ++t) cnt = cnt + 1.0;
          }
        }
      }
    } else {
      constexpr uintptr_t kMask = sizeof(T) == 4 ? 15 : 7;   // a 16-B load, 8 B of 16-bit elements
      PeerQuad<S> qm[R];
      const bool m_al = DIFF && ((uintptr_t)m & kMask) == 0;
      if constexpr (DIFF) {
#pragma unroll
        for (int r = 0; r < R; ++r) qm[r].load(m + 4 * ((int64_t)r * kBlock + tid), m_al);
      }
      for (int k0 = 0; k0 < K; k0 += G) {
        RoundQuad<S> q[G][R];
        int ra[G];   // each peer's residue at the tile, in elements (0: aligned)
        const int lane = tid & 63;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          ra[g] = 0;
          if (k0 + g < K) {
            const T* p = (const T*)psrc[k0 + g] + e;
            ra[g] = (int)(((uintptr_t)p & kMask) / sizeof(T));
#pragma unroll
            for (int r = 0; r < R; ++r) q[g][r].load(p + 4 * ((int64_t)r * kBlock + (tid & ~63)), lane, ra[g]);
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (k0 + g < K) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
              double v[4];
              q[g][r].finish(lane, ra[g]);
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                if constexpr (DIFF) v[c] = seg_sub<S>(qm[r].get(c, m_al), q[g][r].get(c));
                else v[c] = S::widen(q[g][r].get(c));
              }
              for (int t = 0; t < mult; ++t) {
#pragma unroll
                for (int c = 0; c < 4; ++c) wv[r][c] = wv[r][c] + v[c];
              }
            }
            for (int t = 0; t < mult; ++t) cnt = cnt + 1.0;
          }
        }
      }
    }
    // k_finalize: W = AGG + REP, REP logically zero an addition of +0.0.  REP is loaded here, after the peers, so
    // that its registers are not held across the peer loop
    cnt = cnt + rcnt;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t i = base + EL * ((int64_t)r * kBlock + tid);
#pragma unroll
      for (int c = 0; c < EL; c += 2) {
        u2 rv = u2{0, 0};
        if (!rzero) rv = ld16<true>(j.rep + i + c);
        const d2 y = __builtin_bit_cast(d2, rv);
        wv[r][c] = wv[r][c] + y.x, wv[r][c + 1] = wv[r][c + 1] + y.y;
      }
    }
    if constexpr (sizeof(T) == 8) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        *(gu2)(j.w + base + 2 * ((int64_t)r * kBlock + tid)) = encode2<false>(d2{wv[r][0], wv[r][1]});
    } else {
      const bool hi = tid & 4;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        // k_update_segs's stores: lanes 8k..8k+3 own one 128-B line of sums, 8k+4..8k+7 the next
        const int64_t o = base + 4 * ((int64_t)r * kBlock + tid);
        const d2 own = d2{wv[r][0], wv[r][1]};
        const d2 got = d2{__shfl_xor(wv[r][2], 4), __shfl_xor(wv[r][3], 4)};
        __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(j.w + (hi ? o - 14 : o)));
        __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(j.w + (hi ? o : o + 18)));
      }
    }
  }
  // the divide, made once per element; then every list in order
  const double den = SECURE ? 1e12 * cnt : cnt;   // IPLS.java:1167
  auto q = [&](double a) -> double { return (cnt == 0.0) ? a : a / den; };
  typedef typename std::conditional<sizeof(T) == 8, unsigned long long, unsigned>::type B;   // an element's bits
  typedef unsigned u2w __attribute__((ext_vector_type(2)));
  B y[R][EL];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int c = 0; c < EL; ++c) {
      if constexpr (sizeof(T) == 8) y[r][c] = __builtin_bit_cast(unsigned long long, q(wv[r][c]));
      else y[r][c] = S::narrow((float)q(wv[r][c]));
    }
  }
  auto st_el = [](T* p, B b) {
    if constexpr (sizeof(T) == 8) st8(p, b);
    else S::put(p, b);
  };
  // EL elements at an address aligned to their EL * sizeof(T) bytes: one non-temporal store
  auto st_vec = [](T* p, B b0, B b1, B b2, B b3) {
    if constexpr (sizeof(T) == 8) __builtin_nontemporal_store(u2{b0, b1}, (gu2)p);
    else if constexpr (sizeof(T) == 4) __builtin_nontemporal_store(u4w{b0, b1, b2, b3}, (IPLS_GLOBAL u4w*)p);
    else __builtin_nontemporal_store(u2w{b0 | (b1 << 16), b2 | (b3 << 16)}, (IPLS_GLOBAL u2w*)p);
  };
  // The stores below write, from one lane, elements that its neighbour in the WAVE loaded: every load of the block
  // is behind this barrier (see IN PLACE at the top of the file).
  __syncthreads();
  const int lane = tid & 63;
  for (int k = 0; k < n_lists; ++k) {
    T* o = (T*)pdst[k] + e;   // uniform over the block
    const int a = (int)(((uintptr_t)o & (EL * sizeof(T) - 1)) / sizeof(T));   // the tile's residue, in elements
    if (a == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        st_vec(o + EL * ((int64_t)r * kBlock + tid), y[r][0], y[r][1], y[r][EL - 2], y[r][EL - 1]);
      continue;
    }
    // Misaligned: element s = EL - a of the tile is the first aligned one.  A lane stores the aligned vector that
    // starts at its element s -- its own elements s .. EL-1 and elements 0 .. s-1 of the next lane of its wave; the
    // wave's first lane adds its own elements 0 .. s-1 and its last lane stores only its own s .. EL-1, element by
    // element.  A wave so writes exactly the 64 * EL elements its lanes hold, and nothing else.
    const int s = EL - a;
    if (!seg_round_shift<T>()) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int c = 0; c < EL; ++c) st_el(o + EL * ((int64_t)r * kBlock + tid) + c, y[r][c]);
      }
      continue;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      T* ov = o + EL * ((int64_t)r * kBlock + tid);
      B n[EL - 1];
#pragma unroll
      for (int c = 0; c < EL - 1; ++c) n[c] = __shfl_down(y[r][c], 1);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < EL - 1; ++c)
          if (c < s) st_el(ov + c, y[r][c]);
      }
      if (lane == 63) {
#pragma unroll
        for (int c = 1; c < EL; ++c)
          if (c >= s) st_el(ov + c, y[r][c]);
      } else if constexpr (EL == 2) {
        st_vec(ov + 1, y[r][1], n[0], 0, 0);
      } else if (s == 1) {
        st_vec(ov + 1, y[r][1], y[r][2], y[r][3], n[0]);
      } else if (s == 2) {
        st_vec(ov + 2, y[r][2], y[r][3], n[0], n[1]);
      } else {
        st_vec(ov + 3, y[r][3], n[0], n[1], n[2]);
      }
    }
  }
}

// Element e of list array p of format fmt (a run-time value) = narrow(y).
__device__ __forceinline__ void seg_store(void* p, int64_t e, int fmt, double y) {
  switch (fmt) {
    case segplan::kF64: st8((unsigned long long*)p + e, __builtin_bit_cast(unsigned long long, y)); break;
    case segplan::kF32: FmtF32::put((float*)p + e, FmtF32::narrow((float)y)); break;
    case segplan::kF16: FmtF16::put((unsigned short*)p + e, FmtF16::narrow((float)y)); break;
    default: FmtBF16::put((unsigned short*)p + e, FmtBF16::narrow((float)y)); break;
  }
}

// pieces[k].src: the piece's first minuend element (DIFF; not read otherwise);
// psrc[k * K + p]: its first element in peer p's list; pdst[k * n_lists + l]: in output list l.
template <bool DIFF, bool SECURE>
__global__ __launch_bounds__(kBlock) void k_round_segs_peers(const segplan::Item* __restrict__ items,
                                                             const SegRoundJob* __restrict__ jobs,
                                                             const SegPiece* __restrict__ pieces,
                                                             const void* const* __restrict__ psrc, int K,
                                                             void* const* __restrict__ pdst, int n_lists) {
  const segplan::Item it = items[blockIdx.x];
  const SegRoundJob j = jobs[it.job];
  if (it.whole) {
    const SegPiece pc = pieces[it.piece_lo];
    const void* const* pp = psrc + (int64_t)it.piece_lo * K;
    void* const* po = pdst + (int64_t)it.piece_lo * n_lists;
    const int64_t e = it.lo - pc.dst;   // the tile's first element in the piece
    switch (it.fmt) {
      case segplan::kF64:
        round_segs_peers_whole<FmtD64, DIFF, SECURE>((const unsigned long long*)pc.src + e, pp, K, po, n_lists, e, j, it.lo);
        break;
      case segplan::kF32:
        round_segs_peers_whole<FmtF32, DIFF, SECURE>((const float*)pc.src + e, pp, K, po, n_lists, e, j, it.lo);
        break;
      case segplan::kF16:
        round_segs_peers_whole<FmtF16, DIFF, SECURE>((const unsigned short*)pc.src + e, pp, K, po, n_lists, e, j, it.lo);
        break;
      default:
        round_segs_peers_whole<FmtBF16, DIFF, SECURE>((const unsigned short*)pc.src + e, pp, K, po, n_lists, e, j, it.lo);
        break;
    }
    return;
  }
  const int mult = j.mult;
  const bool zero = j.agg_zero != 0, rzero = j.rep_zero != 0;
  const double cnt = mult == 0 ? __builtin_bit_cast(double, ld8(j.w + j.L - 1)) : round_count(j, K);
  const double den = SECURE ? 1e12 * cnt : cnt;
  for (int64_t i = it.lo + threadIdx.x; i < it.hi; i += kBlock) {
    int k = 0;
    if (i < j.ncopy) k = seg_piece_of(pieces, it.piece_lo, it.piece_hi, i);
    double w;
    if (mult == 0) {
      if (i >= j.ncopy) continue;   // W is read only, and the count slot and the tail go to no list
      w = __builtin_bit_cast(double, ld8(j.w + i));
    } else {
      double acc = zero ? 0.0 : __builtin_bit_cast(double, ld8(j.agg + i));
      if (i < j.ncopy) {
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
      w = acc + (rzero ? 0.0 : __builtin_bit_cast(double, ld8(j.rep + i)));
      st8(j.w + i, __builtin_bit_cast(unsigned long long, w));
      if (i >= j.ncopy) continue;
    }
    const SegPiece pc = pieces[k];
    void* const* po = pdst + (int64_t)k * n_lists;
    const double y = (cnt == 0.0) ? w : w / den;
    for (int l = 0; l < n_lists; ++l) seg_store(po[l], i - pc.dst, (int)pc.fmt, y);
  }
}

}  // namespace ipls
