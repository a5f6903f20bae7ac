// seg_copies_kernels.hpp -- the kernel of the output-copy-list call
// (ipls_agg_get_partitions_segs_copies; include/ipls_agg.h): n_lists segment
// lists over one table of lengths and formats -- the parameter tensors of K
// trainers that share one architecture and the received model they all start
// the next round from -- every one written with the GetPartitions divide in
// one launch:
//   out_k[s][e] = narrow_s(cnt_p == 0.0 ? W[p][j] : W[p][j] / den_p)  for every k,
//   f = start_s + e, p = f / chunk, j = f - p * chunk,
// k_divide_segs's value (seg_kernels.hpp): the IEEE double division, rounded
// once to float for F32 and from that float to the format for F16 / BF16,
// doubles stored as they are.  W and the count slot are read once, the division
// and the narrowing are made once, and the result is stored to list 0, list 1,
// .. in that order, so every list ends with the bits of the single-list twin.
// The plan and the items are k_divide_segs's, made from the shared table with
// list 0's addresses; the lists travel as outs[k * n_segs + s], list-major, in
// the same upload.  No list's alignment is read from the plan: a whole tile
// takes each one's from its address, block-uniform.
// Built without contraction and without fast-math, no LDS, vector stores only.
// Included by engine.hip after seg_peers_kernels.hpp.
#pragma once

#include <type_traits>

#include "seg_kernels.hpp"

namespace ipls {

// ---------------------------------------------------------------------------
// One item of format S.  outs: &outs[job], list k's array of the segment is
// outs[k * n_segs].
// A `whole` item (a full tile inside one partition) is divide_segs_whole's
// body up to the stores: the 16-B vectors of a lane stay in registers and the
// lists are walked in order.  A list whose tile starts 16-B aligned takes the
// twin's non-temporal 16-B stores (a wave's store covers whole lines when the
// list is line-aligned as list 0 is); any other residue takes naturally
// aligned element stores of the same values at the same elements.  Either way
// a lane writes elements [lo + i, lo + i + EV) of its vectors and nothing else.
// Every other item goes element by element, the count slot read per element's
// own partition, the value made once and stored to every list.
// ---------------------------------------------------------------------------
template <class S, bool SECURE>
__device__ __forceinline__ void divide_segs_copies_item(const segplan::Item& it, void* const* __restrict__ outs,
                                                        int n_lists, int64_t n_segs,
                                                        const SegDivPart* __restrict__ parts, int64_t chunk,
                                                        int64_t p_lo) {
  typedef typename S::elem T;
  if (it.whole) {
    constexpr int EV = 16 / sizeof(T);                   // values per store
    constexpr int V = kSegTile / ((int64_t)kBlock * EV); // stores per lane
    static_assert((int64_t)kBlock * EV * V == kSegTile, "one tile size for every element size");
    typedef typename std::conditional<sizeof(T) == 8, u2, u4w>::type Q;
    const int64_t p = it.flat / chunk;
    const SegDivPart d = parts[p - p_lo];
    const double cnt = d.w[d.len - 1];
    const double den = SECURE ? 1e12 * cnt : cnt;   // IPLS.java:1167
    const double* w = d.w + (it.flat - p * chunk);
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
    Q y[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const double* xv = x[v];
      if constexpr (sizeof(T) == 8) {
        y[v].x = __builtin_bit_cast(unsigned long long, q(xv[0]));
        y[v].y = __builtin_bit_cast(unsigned long long, q(xv[1]));
      } else {
        auto f = [&](double a) -> unsigned { return S::narrow((float)q(a)); };
        // the words are spelled out, as in divide_segs_whole
        if constexpr (sizeof(T) == 2)
          y[v] = u4w{f(xv[0]) | (f(xv[1]) << 16), f(xv[2]) | (f(xv[3]) << 16), f(xv[4]) | (f(xv[5]) << 16),
                     f(xv[6]) | (f(xv[7]) << 16)};
        else
          y[v] = u4w{f(xv[0]), f(xv[1]), f(xv[2]), f(xv[3])};
      }
    }
    for (int k = 0; k < n_lists; ++k) {
      T* o = (T*)outs[(int64_t)k * n_segs] + it.lo;   // uniform over the block
      if (((uintptr_t)o & 15) == 0) {
#pragma unroll
        for (int v = 0; v < V; ++v)
          __builtin_nontemporal_store(y[v], (IPLS_GLOBAL Q*)(o + wave_base + (int64_t)v * 64 * EV));
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          T* ov = o + wave_base + (int64_t)v * 64 * EV;
          if constexpr (sizeof(T) == 8) {
            st8(ov, y[v].x);
            st8(ov + 1, y[v].y);
          } else if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int c = 0; c < EV; ++c) S::put(ov + c, y[v][c]);
          } else {
#pragma unroll
            for (int c = 0; c < EV; ++c) S::put(ov + c, y[v][c >> 1] >> (16 * (c & 1)));
          }
        }
      }
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
    if constexpr (sizeof(T) == 8) {
      const unsigned long long b = __builtin_bit_cast(unsigned long long, y);
      for (int k = 0; k < n_lists; ++k) st8((T*)outs[(int64_t)k * n_segs] + e, b);
    } else {
      const unsigned b = S::narrow((float)y);
      for (int k = 0; k < n_lists; ++k) S::put((T*)outs[(int64_t)k * n_segs] + e, b);
    }
  }
}

// outs[k * n_segs + s]: list k's array of segment s (not looked at when the segment is empty: it has no item).
template <bool SECURE>
__global__ __launch_bounds__(kBlock) void k_divide_segs_copies(const segplan::Item* __restrict__ items,
                                                               void* const* __restrict__ outs, int n_lists,
                                                               int n_segs, const SegDivPart* __restrict__ parts,
                                                               int64_t chunk, int64_t p_lo) {
  const segplan::Item it = items[blockIdx.x];
  void* const* o = outs + it.job;
  switch (it.fmt) {
    case segplan::kF64: divide_segs_copies_item<FmtD64, SECURE>(it, o, n_lists, n_segs, parts, chunk, p_lo); break;
    case segplan::kF32: divide_segs_copies_item<FmtF32, SECURE>(it, o, n_lists, n_segs, parts, chunk, p_lo); break;
    case segplan::kF16: divide_segs_copies_item<FmtF16, SECURE>(it, o, n_lists, n_segs, parts, chunk, p_lo); break;
    default: divide_segs_copies_item<FmtBF16, SECURE>(it, o, n_lists, n_segs, parts, chunk, p_lo); break;
  }
}

}  // namespace ipls
