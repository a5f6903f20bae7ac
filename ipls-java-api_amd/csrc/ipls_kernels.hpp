// ipls_kernels.hpp -- gfx950 (CDNA4) HIP kernels of the IPLS aggregation path.
//
// Design:
//  * The hot kernel is a fixed-order elementwise fold over K peer buckets.
//    Each lane owns 16 contiguous bytes (2 doubles) per step and walks the
//    peers in order, so every element is ((+0.0 + b0) + b1) + ... exactly as
//    Updater.java:115-117 / IPLS.java:1740 compute it.  No shuffle or tree
//    reduction touches the peer axis: that would reassociate the sum and
//    break bit parity (SURVEY.md §7 "Order vs. shuffles").
//  * Memory-level parallelism comes from issuing the loads of G peers
//    (G x 16 B per lane) before folding them; bucket base pointers are
//    wave-uniform (scalar loads from a device table).
//  * Wavefront DPP reductions + LDS staging are used where the reduction is
//    order-free: the integer checksum kernel (exact, any association).
//  * Compiled with -ffp-contract=off; double division is the IEEE-correct
//    v_div_scale/v_div_fmas/v_div_fixup sequence (no fast-math).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef IPLS_ROT
#define IPLS_ROT 0
#endif
// IPLS_ROUND_PAIRS=1: the fused round's wave-pair tile layout (reduce_tiles);
// the =0 build (the round-2 layout) is the A/B variant
#ifndef IPLS_ROUND_PAIRS
#define IPLS_ROUND_PAIRS 1
#endif

namespace ipls {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
typedef unsigned u4w __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;

enum Start : int { kAccum = 0, kZero = 1, kFirst = 2 };

struct PartDesc {
  int64_t len;                      // L_p incl. count slot
  unsigned long long* dst;          // target: an arena accumulator or a caller buffer
  // fused-round fields (k_round only):
  const unsigned long long* init;   // START_ACCUM source (the AGG accumulator)
  const unsigned long long* rep;    // REP accumulator, or null = logically +0.0
  unsigned long long* avg;          // averaged values out (L-1 doubles), or null
};

// Global-address-space views.  Bucket pointers come from a device table, so
// the compiler cannot infer their address space and would emit flat_load with
// a vmcnt(0)+lgkmcnt(0) wait after EVERY load (fully serialised).  Casting to
// addrspace(1) gives global_load and counted vmcnt waits.
#define IPLS_GLOBAL __attribute__((address_space(1)))
typedef const IPLS_GLOBAL u2* gcu2;
typedef IPLS_GLOBAL u2* gu2;
typedef const IPLS_GLOBAL unsigned long long* gcu64;
typedef IPLS_GLOBAL unsigned long long* gu64;

// NOTE: never __builtin_bit_cast(double, v.y) on an ext_vector element: hipcc
// (ROCm 7.2) lowers it to element 0 (measured in the ISA).  Copy the element
// to a scalar first, or bit_cast the whole vector.
__device__ __forceinline__ double be_to_f64(unsigned long long v) {
  return __builtin_bit_cast(double, __builtin_bswap64(v));
}
__device__ __forceinline__ unsigned long long f64_to_be(double v) {
  return __builtin_bswap64(__builtin_bit_cast(unsigned long long, v));
}

template <bool NT>
__device__ __forceinline__ u2 ld16(const unsigned long long* p) {
  if constexpr (NT) return __builtin_nontemporal_load((gcu2)p);
  else return *(gcu2)p;
}
__device__ __forceinline__ unsigned long long ld8(const unsigned long long* p) { return *(gcu64)p; }
__device__ __forceinline__ void st8(unsigned long long* p, unsigned long long v) { *(gu64)p = v; }

template <bool BE>
__device__ __forceinline__ d2 decode2(u2 raw) {
  if constexpr (BE) {
    const unsigned long long a = raw.x, b = raw.y;
    u2 s;
    s.x = __builtin_bswap64(a);
    s.y = __builtin_bswap64(b);
    return __builtin_bit_cast(d2, s);
  } else {
    return __builtin_bit_cast(d2, raw);
  }
}
template <bool BE>
__device__ __forceinline__ u2 encode2(d2 v) {
  u2 raw = __builtin_bit_cast(u2, v);
  if constexpr (BE) {
    const unsigned long long a = raw.x, b = raw.y;
    raw.x = __builtin_bswap64(a);
    raw.y = __builtin_bswap64(b);
  }
  return raw;
}
template <bool BE>
__device__ __forceinline__ double decode1(unsigned long long raw) {
  if constexpr (BE) return be_to_f64(raw);
  else return __builtin_bit_cast(double, raw);
}

// ---------------------------------------------------------------------------
// k_reduce: target[q] = fold(start; bufs[q*k + 0..k-1]) for the partitions of
// one batch.  Grid = n_parts * tiles_per_part blocks of 256 lanes; a tile is
// 256 * 2 * R doubles.  Full tiles take the vector path; the one partial tile
// per partition takes a scalar path (odd lengths, e.g. ETHModel's 147,869).
//   BE_IN  : buckets hold big-endian doubles (IPFS file bytes) -> bswap fused
//   BE_OUT : write the sum as big-endian bytes (update_file), else doubles
//   G      : peers whose loads are in flight together per lane
//   R      : 16-byte vectors per lane per tile
//   NT     : non-temporal loads (each byte is read exactly once)
//   MAP    : block -> (partition, tile) order.  0 = partition-major;
//            1 = tile-major (consecutive blocks in different partitions);
//            2 = XCD-chunked: blocks b, b+8, b+16.. (one XCD under the observed
//                round-robin dispatch) walk one contiguous 1/8 of the work, so
//                the 8 XCDs stream 8 distant regions (speed only, never
//                correctness: any placement computes the same result).
// ---------------------------------------------------------------------------
//            MAP 2 needs gridDim.x padded to a multiple of 8 (grid_blocks());
//            the padding blocks map past the last tile and exit.
__host__ __device__ constexpr int64_t grid_blocks(int map, int64_t tiles) {
  return map == 2 ? (tiles + 7) / 8 * 8 : tiles;
}

//            3 = partial tiles first: blocks [0, n_parts) take the last tile of
//                each partition (partial when L is not a multiple of the tile),
//                the rest the full tiles partition-major.  With 1 workgroup per
//                CU the short partial blocks then run beside the first round of
//                full tiles instead of pushing full tiles into an extra round
//                (L = 4194305: 2064 blocks = 8 rounds + 15 full tiles alone).
__device__ __forceinline__ void map_block(int map, int nblocks, int tiles_per_part, int n_parts, int& q, int& t) {
  int b = blockIdx.x;
  if (map == 3) {
    if (b < n_parts) {
      q = b;
      t = tiles_per_part - 1;
    } else {
      b -= n_parts;
      q = b / (tiles_per_part - 1);
      t = b - q * (tiles_per_part - 1);
    }
    return;
  }
  if (map == 2) {
    const int per = nblocks >> 3;  // nblocks % 8 == 0 (grid_blocks)
    b = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (b >= tiles_per_part * n_parts) { q = n_parts; t = 0; return; }
  }
  if (map == 1) {
    q = b % n_parts;
    t = b / n_parts;
  } else {
    q = b / tiles_per_part;
    t = b - q * tiles_per_part;
  }
}

//   BS     : lanes per workgroup
//   FIN    : fused round -- dst is Weights[p] and receives fold + REP
//            (AggregatePartition, IPLS.java:1256), and parts[q].avg (if set)
//            the GetPartitions divide (IPLS.java:1159-1174), in the same pass
template <bool BE_IN, bool BE_OUT, int START, int G, int R, bool NT, int MAP, int BS, bool FIN, int SEQF>
__device__ __forceinline__ void reduce_tiles(
    const unsigned long long* const* __restrict__ bufs, const PartDesc* __restrict__ parts,
    int k, int tiles_per_part, int n_parts, int secure, const double* __restrict__ cnts) {
  constexpr int kBlock = BS;   // lanes per workgroup (shadows the namespace default)
  constexpr int64_t kTile = (int64_t)kBlock * 2 * R;
  int q, t;
  map_block(MAP, gridDim.x, tiles_per_part, n_parts, q, t);
  if (q >= n_parts) return;
  const int64_t L = parts[q].len;
  const int64_t base = (int64_t)t * kTile;
  if (base >= L) return;
  unsigned long long* __restrict__ dst = parts[q].dst;
  const unsigned long long* const* __restrict__ pb = bufs + (size_t)q * k;
  const int tid = threadIdx.x;
  const int j0 = (START == kFirst) ? 1 : 0;
  static_assert(!(FIN && BE_OUT), "the fused round writes native Weights");
  // ACCUM source: the target itself, or AGG when the round is fused
  const unsigned long long* __restrict__ init = FIN ? parts[q].init : dst;
  const unsigned long long* __restrict__ rep = FIN ? parts[q].rep : nullptr;
  unsigned long long* __restrict__ avg = FIN ? parts[q].avg : nullptr;
  // count slot W[L-1] (k_round_counts folded it exactly as element L-1 is)
  double den = 0.0, cnt = 0.0;
  if constexpr (FIN) {
    if (avg) {
      cnt = cnts[q];
      den = secure ? 1e12 * cnt : cnt;   // Math.pow(10,12) * W[last] (IPLS.java:1167)
    }
  }
  const bool avg_aligned = FIN && !((uintptr_t)avg & 15);
  // fused epilogue for element e holding fold value a: W = a + REP; avg = W / count
  auto fin1 = [&](int64_t e, double a) {
    const double w = a + (rep ? __builtin_bit_cast(double, ld8(rep + e)) : 0.0);
    st8(dst + e, __builtin_bit_cast(unsigned long long, w));
    if (avg && e < L - 1) st8(avg + e, __builtin_bit_cast(unsigned long long, cnt == 0.0 ? w : w / den));
  };

  if (base + kTile <= L) {
    // ---------------- vector path: R x 16 B per lane ----------------
    // (hipcc, held to 128 VGPRs by the 1024-lane bound, issues a peer's R
    // loads one or two at a time per wave (checked in the ISA); the 16 waves
    // of a CU then sweep one 16 KiB window of the bucket at a time, which is
    // the DRAM pattern that measured best -- forcing all R loads in flight
    // with scheduling barriers was slower.)
    int64_t off[R];
    // IPLS_ROT=1 (A/B builds only): tile t visits its R sub-windows starting
    // at sub-window t mod R, so neighbouring tiles in flight at the same loop
    // step touch different offsets of their chunks (accumulator r always
    // pairs with the same sub-window, so every element's fold is unchanged)
#if IPLS_ROT
    const int rot = t & (R - 1);
#else
    constexpr int rot = 0;
#endif
    // PAIRS (the fused round): a wave's vectors 2m and 2m+1 are adjacent 1 KiB
    // pieces, so a wave owns 2 KiB contiguous per pair (the CU still sweeps one
    // window of each bucket per two vectors), and an averages run at 8 mod 16
    // needs single 8-B stores every 2 KiB instead of every 1 KiB (epilogue).
    // Same elements, same fold: bit-identical; +0.3 to +0.8 points on config
    // C's round in three processes (profiles/r03/an/pairs2_probe.jsonl).
    constexpr bool PAIRS = FIN && IPLS_ROUND_PAIRS && (R % 2 == 0);
    if constexpr (PAIRS) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        off[r] = base + 2 * ((int64_t)(r >> 1) * 2 * kBlock + (tid >> 6) * 128 + (r & 1) * 64 + (tid & 63));
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) off[r] = base + 2 * ((int64_t)((r + rot) & (R - 1)) * kBlock + tid);
    }

    // SEQ: one peer per step, each of its R vectors loaded, decoded and added
    // before the next is issued (a scheduling fence between them).  This is
    // the schedule hipcc picks by itself for native doubles; with the bswap
    // (or the ACCUM read of the target) in between it would hoist the loads
    // instead and spill at R = 16.
    constexpr bool SEQ = SEQF > 0 && G == 1;
    d2 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (START == kZero) {
        acc[r] = d2{0.0, 0.0};
      } else if constexpr (START == kFirst) {
        acc[r] = decode2<BE_IN>(ld16<NT>(pb[0] + off[r]));
      } else {  // kAccum: the target holds native doubles (or BE if BE_OUT)
        acc[r] = decode2<BE_OUT>(ld16<false>(init + off[r]));
      }
      if constexpr (SEQ && START != kZero) __builtin_amdgcn_sched_barrier(0);
    }
    int j = j0;
    if constexpr (SEQ) {
      for (; j < k; ++j) {
        const unsigned long long* __restrict__ src = pb[j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const d2 x = decode2<BE_IN>(ld16<NT>(src + off[r]));
          acc[r].x = acc[r].x + x.x;
          acc[r].y = acc[r].y + x.y;
          // SEQF = F + 10*T: a fence after every F vectors, none among the last T
          if constexpr (SEQF > 0)
            if ((r + 1) % (SEQF % 10) == 0 && r + 1 < R - SEQF / 10) __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
    for (; j + G <= k; j += G) {
      u2 v[G][R];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const unsigned long long* __restrict__ src = pb[j + g];
#pragma unroll
        for (int r = 0; r < R; ++r) v[g][r] = ld16<NT>(src + off[r]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          d2 x = decode2<BE_IN>(v[g][r]);
          acc[r].x = acc[r].x + x.x;
          acc[r].y = acc[r].y + x.y;
        }
      }
    }
    for (; j < k; ++j) {
      const unsigned long long* __restrict__ src = pb[j];
      u2 v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = ld16<NT>(src + off[r]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        d2 x = decode2<BE_IN>(v[r]);
        acc[r].x = acc[r].x + x.x;
        acc[r].y = acc[r].y + x.y;
      }
    }
    }  // !SEQ
    if constexpr (FIN) {
      // W = fold + REP (AggregatePartition, IPLS.java:1256), and the averages'
      // R stores before W's: two runs of stores per wave instead of
      // alternating between the two streams every vector
      // (tools/round_epilogue_sweep.hip, profiles/r02/s4/round_epilogue.txt)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (rep) {
          const d2 y = decode2<false>(ld16<true>(rep + off[r]));
          acc[r].x = acc[r].x + y.x;
          acc[r].y = acc[r].y + y.y;
        } else {
          acc[r].x = acc[r].x + 0.0;   // AGG + REP with REP == +0.0, as AggregatePartition computes it
          acc[r].y = acc[r].y + 0.0;
        }
        if (avg) {
          // averages of elements e, e+1 (e + 1 may be the count slot L-1, which is not output)
          const int64_t e = off[r];
          const double ax = cnt == 0.0 ? acc[r].x : acc[r].x / den;
          const double ay = cnt == 0.0 ? acc[r].y : acc[r].y / den;
          if (avg_aligned) {
            if (e + 1 < L - 1) __builtin_nontemporal_store(encode2<false>(d2{ax, ay}), (gu2)(avg + e));
            else st8(avg + e, __builtin_bit_cast(unsigned long long, ax));
          } else if constexpr (PAIRS) {
            // piece r pairs its lane-63 y with piece r+1's lane-0 x (r even);
            // piece r+1 directly follows piece r, so singles fall every 2 KiB
            const int lane = tid & 63;
            const double nx = __shfl_down(ax, 1);
            if ((r & 1) == 0) {
              const double nb = acc[r + 1].x + (rep && lane == 0 ? __builtin_bit_cast(double, ld8(rep + off[r + 1])) : 0.0);
              const double b0 = __shfl(cnt == 0.0 ? nb : nb / den, 0);
              if (lane == 0) st8(avg + e, __builtin_bit_cast(unsigned long long, ax));
              __builtin_nontemporal_store(encode2<false>(d2{ay, lane < 63 ? nx : b0}), (gu2)(avg + e + 1));
            } else {
              if (lane < 63) __builtin_nontemporal_store(encode2<false>(d2{ay, nx}), (gu2)(avg + e + 1));
              else if (e + 1 < L - 1) st8(avg + e + 1, __builtin_bit_cast(unsigned long long, ay));
            }
          } else {
            // avg + e is 8 mod 16: lane t writes the aligned pair (e+1, e+2) =
            // (its y, lane t+1's x); the wave's first x and last y go alone.
            const double nx = __shfl_down(ax, 1);
            const int lane = tid & 63;
            if (lane == 0) st8(avg + e, __builtin_bit_cast(unsigned long long, ax));
            if (lane < 63) __builtin_nontemporal_store(encode2<false>(d2{ay, nx}), (gu2)(avg + e + 1));
            else if (e + 1 < L - 1) st8(avg + e + 1, __builtin_bit_cast(unsigned long long, ay));
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) __builtin_nontemporal_store(encode2<false>(acc[r]), (gu2)(dst + off[r]));
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) __builtin_nontemporal_store(encode2<BE_OUT>(acc[r]), (gu2)(dst + off[r]));
    }
  } else {
    // ------- partial last tile: 2*BS-element vector steps, scalar remainder -------
    constexpr int kPB = 8;
    for (int64_t sb = base; sb < L; sb += 2 * kBlock) {
      const int64_t i = sb + 2 * tid;
      if (sb + 2 * kBlock <= L) {
        d2 acc;
        if constexpr (START == kZero) acc = d2{0.0, 0.0};
        else if constexpr (START == kFirst) acc = decode2<BE_IN>(ld16<NT>(pb[0] + i));
        else acc = decode2<BE_OUT>(ld16<false>(init + i));
        // peers in groups of kPB loads in flight (the fold order is unchanged):
        // a one-at-a-time chain of k dependent loads made this block take longer
        // than a full tile
        int jj = j0;
        for (; jj + kPB <= k; jj += kPB) {
          u2 v[kPB];
#pragma unroll
          for (int g = 0; g < kPB; ++g) v[g] = ld16<NT>(pb[jj + g] + i);
#pragma unroll
          for (int g = 0; g < kPB; ++g) {
            const d2 x = decode2<BE_IN>(v[g]);
            acc.x = acc.x + x.x;
            acc.y = acc.y + x.y;
          }
        }
        for (; jj < k; ++jj) {
          const d2 x = decode2<BE_IN>(ld16<NT>(pb[jj] + i));
          acc.x = acc.x + x.x;
          acc.y = acc.y + x.y;
        }
        if constexpr (FIN) {
          fin1(i, acc.x);
          fin1(i + 1, acc.y);
        } else {
          __builtin_nontemporal_store(encode2<BE_OUT>(acc), (gu2)(dst + i));
        }
      } else {
        for (int64_t e = sb + tid; e < L; e += kBlock) {
          double acc;
          if constexpr (START == kZero) acc = 0.0;
          else if constexpr (START == kFirst) acc = decode1<BE_IN>(ld8(pb[0] + e));
          else acc = decode1<BE_OUT>(ld8(init + e));
          int jj = j0;
          for (; jj + kPB <= k; jj += kPB) {
            unsigned long long v[kPB];
#pragma unroll
            for (int g = 0; g < kPB; ++g) v[g] = ld8(pb[jj + g] + e);
#pragma unroll
            for (int g = 0; g < kPB; ++g) acc = acc + decode1<BE_IN>(v[g]);
          }
          for (; jj < k; ++jj) acc = acc + decode1<BE_IN>(ld8(pb[jj] + e));
          if constexpr (FIN) fin1(e, acc);
          else st8(dst + e, BE_OUT ? f64_to_be(acc) : __builtin_bit_cast(unsigned long long, acc));
        }
      }
    }
  }
}

// The batched fold (the benchmarked kernel) and the fused round are two
// kernels over the same tile code, so profiles name them apart.
template <bool BE_IN, bool BE_OUT, int START, int G, int R, bool NT, int MAP = 0, int BS = kBlock, int SEQF = 0>
__global__ __launch_bounds__(BS) void k_reduce(const unsigned long long* const* __restrict__ bufs,
                                               const PartDesc* __restrict__ parts, int k, int tiles_per_part,
                                               int n_parts) {
  reduce_tiles<BE_IN, BE_OUT, START, G, R, NT, MAP, BS, false, SEQF>(bufs, parts, k, tiles_per_part, n_parts, 0,
                                                                     nullptr);
}

template <bool BE_IN, int START, int G, int R, int MAP = 0, int BS = kBlock, int SEQF = 0>
__global__ __launch_bounds__(BS) void k_round(const unsigned long long* const* __restrict__ bufs,
                                              const PartDesc* __restrict__ parts, int k, int tiles_per_part,
                                              int n_parts, int secure, const double* __restrict__ cnts) {
  reduce_tiles<BE_IN, false, START, G, R, true, MAP, BS, true, SEQF>(bufs, parts, k, tiles_per_part, n_parts, secure,
                                                               cnts);
}

// Shape of the elementwise kernels below (k_fold_n, k_blend, k_scale,
// k_encode_secure) when every operand is 16-B aligned (VEC, decided by the
// host): a block of kBlock lanes owns kEwTile consecutive elements, each lane
// kEwV 16-B vectors, loads first, then the arithmetic and stores; the one
// partial tile goes element by element.  Otherwise (a bucket at an 8 mod 16
// address, e.g. a payload inside a Java-serialised file) the 8-B grid-stride
// loop.  Same per-element expressions, so the same bits either way.  From
// cold caches at 64 Mi elements the tiles take k_blend from 56 to 75 %,
// k_scale from 62 to 79 % and k_fold_n from 59 to 75 % of 8 TB/s
// (tools/elementwise_sweep.hip, profiles/r04/zl/).
constexpr int kEwV = 4;
constexpr int64_t kEwTile = (int64_t)kBlock * 2 * kEwV;

// Elementwise fold of one bucket of n doubles into dst (off the hot path:
// Download_Scheduler's Other_Replica_Gradients and their Collect_Replicas fold).
//   FIRST: dst[i] = decode(src[i])          (GetParameters(Hash): a new array)
//   else : dst[i] = dst[i] + decode(src[i])
template <bool BE_IN, bool FIRST, bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_fold_n(unsigned long long* __restrict__ dst,
                                                   const unsigned long long* __restrict__ src, int64_t n) {
  auto one = [&](int64_t i) {
    const double x = decode1<BE_IN>(ld8(src + i));
    const double y = FIRST ? x : __builtin_bit_cast(double, ld8(dst + i)) + x;
    st8(dst + i, __builtin_bit_cast(unsigned long long, y));
  };
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= n) {
      u2 sv[kEwV], dv[kEwV];
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
        sv[v] = __builtin_nontemporal_load((gcu2)(src + i));
        if constexpr (!FIRST) dv[v] = *(gcu2)(dst + i);
      }
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
        d2 o = decode2<BE_IN>(sv[v]);
        if constexpr (!FIRST) {
          const d2 y = __builtin_bit_cast(d2, dv[v]);
          o.x = y.x + o.x;
          o.y = y.y + o.y;
        }
        *(gu2)(dst + i) = __builtin_bit_cast(u2, o);
      }
      return;
    }
    for (int64_t i = base + threadIdx.x; i < n; i += kBlock) one(i);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) one(i);
  }
}

// Count slot of a fused round, one wave per partition: the same fold k_round
// applies to element L-1, i.e. W[L-1] =
// (init[L-1] | +0.0) + b_0[L-1] + ... + b_{k-1}[L-1] + (REP[L-1] | +0.0).
// Lane j loads b_j[L-1] (64 independent loads in flight instead of a chain of
// k pointer + value loads), then every lane adds the broadcast values in peer
// order -- the identical expression, so the identical bits.
template <bool BE_IN, int START>
__global__ __launch_bounds__(64) void k_round_counts(const unsigned long long* const* __restrict__ bufs,
                                                     const PartDesc* __restrict__ parts, int k, int n_parts,
                                                     double* __restrict__ cnts) {
  const int q = blockIdx.x;
  if (q >= n_parts) return;
  const int lane = threadIdx.x;
  const PartDesc d = parts[q];
  const int64_t e = d.len - 1;
  const unsigned long long* const* pb = bufs + (size_t)q * k;
  double c = (START == kZero) ? 0.0 : __builtin_bit_cast(double, ld8(d.init + e));
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int j = j0 + lane;
    const double v = j < k ? decode1<BE_IN>(ld8(pb[j] + e)) : 0.0;
    const int m = k - j0 < 64 ? k - j0 : 64;
    for (int t = 0; t < m; ++t) c = c + __shfl(v, t);
  }
  if (lane == 0) cnts[q] = c + (d.rep ? __builtin_bit_cast(double, ld8(d.rep + e)) : 0.0);
}

// Same fold for buckets that are only 8-byte aligned (e.g. a device view into
// a frame payload): one double per lane per step.
template <bool BE_IN, bool BE_OUT, int START>
__global__ __launch_bounds__(kBlock) void k_reduce_scalar(
    const unsigned long long* const* __restrict__ bufs, const PartDesc* __restrict__ parts,
    int k, int tiles_per_part, int64_t tile) {
  const int q = blockIdx.x / tiles_per_part;
  const int t = blockIdx.x - q * tiles_per_part;
  const int64_t L = parts[q].len;
  const int64_t base = (int64_t)t * tile;
  if (base >= L) return;
  unsigned long long* __restrict__ dst = parts[q].dst;
  const unsigned long long* const* __restrict__ pb = bufs + (size_t)q * k;
  const int64_t end = (base + tile < L) ? base + tile : L;
  const int j0 = (START == kFirst) ? 1 : 0;
  for (int64_t i = base + threadIdx.x; i < end; i += kBlock) {
    double acc;
    if constexpr (START == kZero) acc = 0.0;
    else if constexpr (START == kFirst) acc = decode1<BE_IN>(ld8(pb[0] + i));
    else acc = decode1<BE_OUT>(ld8(dst + i));
    for (int j = j0; j < k; ++j) acc = acc + decode1<BE_IN>(ld8(pb[j] + i));
    st8(dst + i, BE_OUT ? f64_to_be(acc) : __builtin_bit_cast(unsigned long long, acc));
  }
}

// ---------------------------------------------------------------------------
// k_fold1: the single-bucket fold of one arrival (Updater._Update,
// Updater.java:115-117), pointers passed as kernel arguments -- no table
// upload, so a per-arrival fold is one launch and nothing else on the stream.
//   dst[i] = start(dst[i]) + decode(src[i]),  start: ZERO +0.0 | ACCUM dst | FIRST none
// 16-B aligned src/dst; R pairs per lane in flight (zero-copy sources are
// read over PCIe, where more outstanding requests per lane pay).
// ---------------------------------------------------------------------------
template <bool BE_IN, bool BE_OUT, int START, int R = 4>
__global__ __launch_bounds__(kBlock) void k_fold1(unsigned long long* __restrict__ dst,
                                                  const unsigned long long* __restrict__ src, int64_t L) {
  const int64_t n2 = L >> 1;   // whole pairs
  const int64_t stride = (int64_t)gridDim.x * kBlock * R;
  auto fold = [&](const u2& v, const u2& t) -> u2 {
    const d2 x = decode2<BE_IN>(v);
    if constexpr (START == kFirst) return encode2<BE_OUT>(x);
    d2 a = (START == kZero) ? d2{0.0, 0.0} : decode2<BE_OUT>(t);
    a.x = a.x + x.x;
    a.y = a.y + x.y;
    return encode2<BE_OUT>(a);
  };
  int64_t b = (int64_t)blockIdx.x * kBlock * R + threadIdx.x;
  for (; b + (int64_t)(R - 1) * kBlock < n2; b += stride) {   // all R pairs in range: loads first
    u2 v[R], t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = ld16<true>(src + 2 * (b + r * kBlock));
    if constexpr (START == kAccum) {
#pragma unroll
      for (int r = 0; r < R; ++r) t[r] = ld16<false>(dst + 2 * (b + r * kBlock));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) __builtin_nontemporal_store(fold(v[r], t[r]), (gu2)(dst + 2 * (b + r * kBlock)));
  }
  for (int r = 0; r < R; ++r) {   // this lane's last, partial group
    const int64_t i2 = b + r * kBlock;
    if (i2 < n2) {
      const u2 t = (START == kAccum) ? ld16<false>(dst + 2 * i2) : u2{0, 0};
      __builtin_nontemporal_store(fold(ld16<true>(src + 2 * i2), t), (gu2)(dst + 2 * i2));
    }
  }
  if ((L & 1) && blockIdx.x == 0 && threadIdx.x == 0) {   // odd length: the last element
    const int64_t e = L - 1;
    const double x = decode1<BE_IN>(ld8(src + e));
    double a;
    if constexpr (START == kFirst) a = x;
    else a = ((START == kZero) ? 0.0 : decode1<BE_OUT>(ld8(dst + e))) + x;
    st8(dst + e, BE_OUT ? f64_to_be(a) : __builtin_bit_cast(unsigned long long, a));
  }
}

// ---------------------------------------------------------------------------
// k_finalize: AggregatePartition (IPLS.java:1255-1270) over a batch.
//   W[i] = AGG[i] + REP[i]  (REP_ZERO: AGG[i] + 0.0 without reading REP)
//   Weight_Address is the same array as Weights (IPLS.java:1141 aliases them).
//   AGG/REP are zeroed unless the host marks them "logically zero" instead.
// ---------------------------------------------------------------------------
struct FinDesc {
  int64_t len;
  int64_t agg_off, rep_off, w_off;
};

// 16-B vectors per lane of k_finalize / k_divide (tile = kBlock * 2 * kV doubles)
constexpr int kFinV = 8, kDivV = 4;   // tools/copy_sweep.hip, profiles/r02/s3/copy_sweep.txt
constexpr int64_t kFinTile = (int64_t)kBlock * 2 * kFinV, kDivTile = (int64_t)kBlock * 2 * kDivV;

//   BS, V: lanes per workgroup and 16-B vectors per lane (tile = BS * 2 * V
//   doubles); the host launches the defaults (tools/copy_sweep.hip sweeps them)
template <bool REP_ZERO, bool ZERO_ACC, int BS = kBlock, int V = kFinV>
__global__ __launch_bounds__(BS) void k_finalize(const FinDesc* __restrict__ parts,
                                                 double* __restrict__ arena,
                                                 int tiles_per_part) {
  // 16 B per lane per step (arena arrays are 256-B aligned), V steps per lane.
  constexpr int kBlock = BS;
  constexpr int kV = V;
  constexpr int64_t kTile = (int64_t)kBlock * 2 * kV;
  const int q = blockIdx.x / tiles_per_part;
  const int t = blockIdx.x - q * tiles_per_part;
  const FinDesc d = parts[q];
  const int64_t base = (int64_t)t * kTile;
  if (base >= d.len) return;
  const int64_t end = (base + kTile < d.len) ? base + kTile : d.len;
  double* agg = arena + d.agg_off;
  double* rep = arena + d.rep_off;
  double* w = arena + d.w_off;
  if (end - base == kTile) {
    u2 a[kV], r[kV];
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
      a[v] = __builtin_nontemporal_load((gcu2)(agg + i));
      if constexpr (!REP_ZERO) r[v] = __builtin_nontemporal_load((gcu2)(rep + i));
    }
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
      const d2 x = __builtin_bit_cast(d2, a[v]);
      const d2 y = REP_ZERO ? d2{0.0, 0.0} : __builtin_bit_cast(d2, r[v]);
      d2 o;
      o.x = x.x + y.x;
      o.y = x.y + y.y;
      // nt stores: plain ones run this kernel ~5 % faster but leave W dirty in
      // the caches, and the next kernel (the GetPartitions divide reading W)
      // pays the write-back: nt in both is the fastest round
      __builtin_nontemporal_store(__builtin_bit_cast(u2, o), (gu2)(w + i));
      if constexpr (ZERO_ACC) {
        __builtin_nontemporal_store(u2{0, 0}, (gu2)(agg + i));
        if constexpr (!REP_ZERO) __builtin_nontemporal_store(u2{0, 0}, (gu2)(rep + i));
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < end; i += kBlock) {
    const double a = agg[i];
    const double r = REP_ZERO ? 0.0 : rep[i];
    w[i] = a + r;
    if constexpr (ZERO_ACC) {
      agg[i] = 0.0;
      if constexpr (!REP_ZERO) rep[i] = 0.0;
    }
  }
}

// ---------------------------------------------------------------------------
// k_divide: GetPartitions (IPLS.java:1159-1174) -> flat model.
//   out[m] = cnt == 0.0 ? W[p][j] : W[p][j] / cnt      (secure: / (1e12*cnt))
//   m = p*chunk + j.  OUT_BE writes DataOutputStream.writeDouble bytes
//   (big-endian, NaN canonicalised, Middleware.java:164-170).
// ---------------------------------------------------------------------------
struct DivDesc {
  int64_t len;    // L_p
  int64_t w_off;  // arena offset of Weights[p]
  int64_t out_off;
};

template <bool OUT_BE, bool SECURE, int BS = kBlock, int V = kDivV>
__global__ __launch_bounds__(BS) void k_divide(const DivDesc* __restrict__ parts,
                                               const double* __restrict__ arena,
                                               unsigned long long* __restrict__ out,
                                               int tiles_per_part) {
  // The flat output offset p*chunk is arbitrary, so the tiles are laid over
  // the OUTPUT: block 0 first writes the `head` elements up to the first 128-B
  // line boundary of this partition's output, then every wave stores whole
  // lines (64 lanes x 16 B = 8 lines), and each lane reads its two W values
  // with 8-B loads (W's alignment relative to the output is arbitrary; reads
  // of partial lines cost little, partial-line writes do).  A wave's V steps
  // cover V adjacent KiB of the output (wave-contiguous), so the W line one
  // step's window shares with the next is read by the same wave back to back:
  // 2-2.5 % faster than every wave of the block taking one KiB per step, with
  // 1.025x read PMC against 1.029x (tools/copy_sweep.hip "8B wc",
  // profiles/r05/m/).
  constexpr int kBlock = BS;
  constexpr int kV = V;
  constexpr int64_t kTile = (int64_t)kBlock * 2 * kV;
  static_assert(BS % 64 == 0, "whole waves");
  const int q = blockIdx.x / tiles_per_part;
  const int t = blockIdx.x - q * tiles_per_part;
  const DivDesc d = parts[q];
  const int64_t n = d.len - 1;
  const double* w = arena + d.w_off;
  const double cnt = w[d.len - 1];
  // Math.pow(10,12) * W[last] (IPLS.java:1167): 1e12 is exact, product rounded once.
  const double den = SECURE ? 1e12 * cnt : cnt;
  auto f = [&](double x) -> unsigned long long {
    const double y = (cnt == 0.0) ? x : x / den;
    unsigned long long bits = __builtin_bit_cast(unsigned long long, y);
    if constexpr (OUT_BE) {
      if (y != y) bits = 0x7ff8000000000000ULL;
      bits = __builtin_bswap64(bits);
    }
    return bits;
  };
  unsigned long long* o = out + d.out_off;
  const int64_t to_line = (16 - (int64_t)(((uintptr_t)o >> 3) & 15)) & 15;   // elements to a 128-B boundary
  const int64_t head = to_line < n ? to_line : n;
  if (t == 0 && threadIdx.x < head) o[threadIdx.x] = f(w[threadIdx.x]);
  const int64_t base = (int64_t)t * kTile + head;
  if (base >= n) return;
  if (base + kTile <= n) {
    // element index of this lane's pair at step v: wave (threadIdx.x / 64) owns
    // [base + wave * 128 * V, + 128 * V)
    const int64_t wave_base = base + (int64_t)(threadIdx.x >> 6) * 128 * kV + 2 * (threadIdx.x & 63);
    double x[kV][2];
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      const int64_t i = wave_base + (int64_t)v * 128;
      x[v][0] = __builtin_nontemporal_load((const __attribute__((address_space(1))) double*)(w + i));
      x[v][1] = __builtin_nontemporal_load((const __attribute__((address_space(1))) double*)(w + i + 1));
    }
#pragma unroll
    for (int v = 0; v < kV; ++v) {
      const int64_t i = wave_base + (int64_t)v * 128;
      u2 v2;
      v2.x = f(x[v][0]);
      v2.y = f(x[v][1]);
      __builtin_nontemporal_store(v2, (gu2)(o + i));
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < n; i += kBlock) o[i] = f(w[i]);
}

// ---------------------------------------------------------------------------
// k_split: OrganizeGradients (IPLS.java:1018-1040) for one partition:
//   dst[j] = flat[p*chunk + j] for j < min(chunk, n - p*chunk) (guarded),
//   dst[stop] = 1.0, rest 0.0.  Optional fused fold into an accumulator
//   (UpdateGradient own-accumulate, IPLS.java:1737-1743).
// ---------------------------------------------------------------------------
//   MODE 0: dst = v (OrganizeGradients' split; BE_OUT packs big-endian)
//   MODE 1: dst = dst + v (own accumulate into AGG, IPLS.java:1737-1743)
//   MODE 2: dst = +0.0 + v (the same into a logically-zero AGG: the zeros are
//           not read, and the bits equal a fold into a zeroed array)
//   VEC: the elementwise tile shape (see k_fold_n) when flat + lo and dst are
//   16-B aligned; tiles wholly inside [0, ncopy) go 16 B at a time, the tile
//   that holds the count slot element by element.
template <bool BE_IN, bool BE_OUT, int MODE, bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_split(const unsigned long long* __restrict__ flat,
                                                  int64_t lo, int64_t ncopy, int64_t L,
                                                  unsigned long long* __restrict__ dst) {
  static_assert(MODE == 0 || !BE_OUT, "the folds write native doubles");
  auto one = [&](int64_t i) {
    double v;
    if (i < ncopy) v = decode1<BE_IN>(flat[lo + i]);
    else if (i == ncopy) v = 1.0;
    else v = 0.0;
    if constexpr (MODE == 1) {
      const double a = __builtin_bit_cast(double, dst[i]);
      dst[i] = __builtin_bit_cast(unsigned long long, a + v);
    } else if constexpr (MODE == 2) {
      dst[i] = __builtin_bit_cast(unsigned long long, 0.0 + v);
    } else {
      dst[i] = BE_OUT ? f64_to_be(v) : __builtin_bit_cast(unsigned long long, v);
    }
  };
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= ncopy) {
      const unsigned long long* src = flat + lo;
      u2 sv[kEwV], dv[kEwV];
#pragma unroll
      for (int k = 0; k < kEwV; ++k) {
        const int64_t i = base + 2 * ((int64_t)k * kBlock + threadIdx.x);
        sv[k] = __builtin_nontemporal_load((gcu2)(src + i));
        if constexpr (MODE == 1) dv[k] = *(gcu2)(dst + i);
      }
#pragma unroll
      for (int k = 0; k < kEwV; ++k) {
        const int64_t i = base + 2 * ((int64_t)k * kBlock + threadIdx.x);
        const d2 x = decode2<BE_IN>(sv[k]);
        d2 o;
        if constexpr (MODE == 1) {
          const d2 a = __builtin_bit_cast(d2, dv[k]);
          o = d2{a.x + x.x, a.y + x.y};
        } else if constexpr (MODE == 2) {
          o = d2{0.0 + x.x, 0.0 + x.y};
        } else {
          o = x;
        }
        *(gu2)(dst + i) = encode2<BE_OUT>(o);
      }
      return;
    }
    const int64_t end = base + kEwTile < L ? base + kEwTile : L;
    for (int64_t i = base + threadIdx.x; i < end; i += kBlock) one(i);
  } else {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < L) one(i);
  }
}

// Layout conversion between native and big-endian doubles (pack / unpack).
//   VEC: the 16-B tile shape of the elementwise kernels (kEwTile elements per
//   block, see k_fold_n) when both operands are 16-B aligned
template <bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_bswap64(const unsigned long long* __restrict__ in,
                                                    unsigned long long* __restrict__ out, int64_t n) {
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= n) {
      u2 v[kEwV];
#pragma unroll
      for (int k = 0; k < kEwV; ++k) v[k] = __builtin_nontemporal_load((gcu2)(in + base + 2 * ((int64_t)k * kBlock + threadIdx.x)));
#pragma unroll
      for (int k = 0; k < kEwV; ++k) {
        const unsigned long long a = v[k].x, b = v[k].y;
        __builtin_nontemporal_store(u2{__builtin_bswap64(a), __builtin_bswap64(b)},
                                    (gu2)(out + base + 2 * ((int64_t)k * kBlock + threadIdx.x)));
      }
      return;
    }
    for (int64_t i = base + threadIdx.x; i < n; i += kBlock) out[i] = __builtin_bswap64(in[i]);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
      out[i] = __builtin_bswap64(in[i]);
  }
}

// Strided model load (InitializeWeights(List<Double>), IPLS.java:1880-1901):
// dst[j] = flat[lo + j] for j < ncopy, dst[L-1] = 0.0.
template <bool BE_IN>
__global__ __launch_bounds__(kBlock) void k_load_model(const unsigned long long* __restrict__ flat,
                                                       int64_t lo, int64_t ncopy, int64_t L,
                                                       double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= L) return;
  dst[i] = (i < ncopy) ? decode1<BE_IN>(flat[lo + i]) : 0.0;
}

// ---------------------------------------------------------------------------
// Synthetic workload and checksum.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long v) {
  unsigned long long z = v + 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

template <bool BE_OUT>
__global__ __launch_bounds__(kBlock) void k_synth(unsigned long long* __restrict__ dst, int64_t L,
                                                  unsigned long long key) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < L;
       i += (int64_t)gridDim.x * kBlock) {
    double x;
    if (i == L - 1) {
      x = 1.0;
    } else {
      const double u = (double)(splitmix64(key ^ (unsigned long long)i) >> 11) * 0x1.0p-53;
      double tt = 2.0 * u;
      tt = tt - 1.0;
      x = tt * 1e-2;
    }
    dst[i] = BE_OUT ? f64_to_be(x) : __builtin_bit_cast(unsigned long long, x);
  }
}

// 64-bit wave sum with DPP row shifts + row broadcasts (gfx9 DPP controls):
// inclusive scan inside each 16-lane row, then row_bcast:15 / row_bcast:31
// carry the row totals up; lane 63 ends with the wave total.  The sum is an
// exact integer (mod 2^64), so association does not matter here.
__device__ __forceinline__ unsigned long long dpp_shift(unsigned long long v, int ctrl_id) {
  const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
  int rl, rh;
  switch (ctrl_id) {
    case 0: rl = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xF, 0xF, true);
            rh = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xF, 0xF, true); break;  // row_shr:1
    case 1: rl = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xF, 0xF, true);
            rh = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xF, 0xF, true); break;  // row_shr:2
    case 2: rl = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xF, 0xF, true);
            rh = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xF, 0xF, true); break;  // row_shr:4
    case 3: rl = __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xF, 0xF, true);
            rh = __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xF, 0xF, true); break;  // row_shr:8
    case 4: rl = __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xA, 0xF, false);
            rh = __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xA, 0xF, false); break; // row_bcast:15
    default: rl = __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xC, 0xF, false);
             rh = __builtin_amdgcn_update_dpp(0, hi, 0x143, 0xC, 0xF, false); break; // row_bcast:31
  }
  return ((unsigned long long)(unsigned)rh << 32) | (unsigned)rl;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int c = 0; c < 6; ++c) v += dpp_shift(v, c);
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

template <bool BE_IN>
__global__ __launch_bounds__(kBlock) void k_checksum(const unsigned long long* __restrict__ x,
                                                     int64_t n, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long lds[kBlock / 64];
  unsigned long long s = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    unsigned long long b = BE_IN ? __builtin_bswap64(x[i]) : x[i];
    s += splitmix64(b + (unsigned long long)i * 0x9E3779B97F4A7C15ULL);
  }
  s = wave_sum_u64(s);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) lds[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += lds[w];
    atomicAdd(out, t);
  }
}

// ---------------------------------------------------------------------------
// k_b64url_decode: java.util.Base64 URL decoding of a batch of messages
// (ThreadReceiver.run / process, IPLS.java:855-859, 399; Utils.java:14-15).
// The host strips and validates the '=' tail; the kernel decodes every full
// 4-char unit (16 chars per lane: one dwordx4 load -> 12 bytes) plus the
// partial last unit, and flags any byte outside A-Z a-z 0-9 - _ (Java's
// IllegalArgumentException) in err[msg].  blockIdx.y = message.
// ---------------------------------------------------------------------------
struct B64Desc {
  int64_t src_off;  // byte offset of the text in src (16-B aligned)
  int64_t units;    // full 4-char units
  int64_t dst_off;  // byte offset of the decoded bytes in dst
  int32_t tail;     // data chars in the partial last unit: 0, 2 or 3
  int32_t pad;
};

__device__ __forceinline__ unsigned b64url_val(unsigned c) {
  // A-Z 0-25, a-z 26-51, 0-9 52-61, '-' 62, '_' 63, else 0x100 (invalid)
  if (c - 'A' < 26u) return c - 'A';
  if (c - 'a' < 26u) return c - 'a' + 26;
  if (c - '0' < 10u) return c - '0' + 52;
  if (c == '-') return 62;
  if (c == '_') return 63;
  return 0x100;
}

// 4 chars (little-endian packed in a dword) -> 24 bits; bit 24+ set if invalid.
__device__ __forceinline__ unsigned b64url_unit(unsigned w) {
  const unsigned a = b64url_val(w & 0xFF), b = b64url_val((w >> 8) & 0xFF);
  const unsigned c = b64url_val((w >> 16) & 0xFF), d = b64url_val(w >> 24);
  return (a << 18) | (b << 12) | (c << 6) | d | ((a | b | c | d) & 0x100 ? 0x1000000u : 0u);
}

__global__ __launch_bounds__(kBlock) void k_b64url_decode(const unsigned char* __restrict__ src,
                                                          const B64Desc* __restrict__ descs,
                                                          unsigned char* __restrict__ dst,
                                                          int* __restrict__ err) {
  const int m = blockIdx.y;
  const B64Desc d = descs[m];
  const unsigned char* s = src + d.src_off;
  unsigned char* o = dst + d.dst_off;
  const int64_t u0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 4;   // first unit of this lane
  if (u0 > d.units) return;
  unsigned bad = 0;
  if (u0 + 4 <= d.units) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const u4 w = *(const IPLS_GLOBAL u4*)(s + 4 * u0);
    const unsigned v[4] = {b64url_unit(w.x), b64url_unit(w.y), b64url_unit(w.z), b64url_unit(w.w)};
    bad = (v[0] | v[1] | v[2] | v[3]) & 0x1000000u;
    unsigned char* q = o + 3 * u0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      q[3 * i] = (unsigned char)(v[i] >> 16);
      q[3 * i + 1] = (unsigned char)(v[i] >> 8);
      q[3 * i + 2] = (unsigned char)v[i];
    }
  } else {
    for (int64_t u = u0; u < d.units; ++u) {
      const unsigned char* c = s + 4 * u;
      const unsigned w = c[0] | (c[1] << 8) | (c[2] << 16) | ((unsigned)c[3] << 24);
      const unsigned v = b64url_unit(w);
      bad |= v & 0x1000000u;
      o[3 * u] = (unsigned char)(v >> 16);
      o[3 * u + 1] = (unsigned char)(v >> 8);
      o[3 * u + 2] = (unsigned char)v;
    }
    if (d.tail && u0 + 4 > d.units) {   // the lane that ends the full units does the tail
      const unsigned char* c = s + 4 * d.units;
      unsigned v = 0, inval = 0;
      for (int i = 0; i < d.tail; ++i) {
        const unsigned x = b64url_val(c[i]);
        inval |= x;
        v |= (x & 63u) << (18 - 6 * i);
      }
      bad |= inval & 0x100;
      o[3 * d.units] = (unsigned char)(v >> 16);
      if (d.tail == 3) o[3 * d.units + 1] = (unsigned char)(v >> 8);
    }
  }
  if (bad) atomicOr(err + m, 1);
}

// ---------------------------------------------------------------------------
// k_b64url_encode_frame: Marshall_Packet (MyIPFSClass.java:990-1017) of an
// accumulator, straight from HBM -- the frame
//   [i16 pid][i32 n][i32 a][i32 b][n x f64 big-endian][origin bytes]
// encoded by Base64.getUrlEncoder (with '=' padding, :1016).  Lane g writes
// the 32 chars of frame bytes [24g, 24g+24).  Lanes whose window lies inside
// the payload (all but the first and the last few) load the 4 doubles it
// spans (it starts 2 bytes into one: 24g - 14 = 8(3g-2) + 2), take the
// window's 6 big-endian words by funnel shifts and emit 8 units = 2 x 16 B;
// the others assemble their bytes one at a time.  src == null: the
// accumulator is logically +0.0 (all payload bytes zero).
// ---------------------------------------------------------------------------
struct FrameEnc {
  unsigned char hdr[16];          // 14 header bytes
  int64_t n;                      // doubles in the payload
  int64_t origin_len;
  const unsigned char* origin;    // device copy of the origin bytes
};

__device__ __forceinline__ unsigned b64url_char(unsigned v) {
  return v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '-' : '_';
}
// 24 bits -> 4 chars packed little-endian (first char in the low byte)
__device__ __forceinline__ unsigned b64url_quad(unsigned v) {
  return b64url_char((v >> 18) & 63) | (b64url_char((v >> 12) & 63) << 8) | (b64url_char((v >> 6) & 63) << 16) |
         (b64url_char(v & 63) << 24);
}

__device__ __forceinline__ unsigned frame_byte(const FrameEnc& f, const unsigned long long* __restrict__ src,
                                               int64_t j) {
  if (j < 14) return f.hdr[j];
  const int64_t q = j - 14;
  if (q < 8 * f.n) {
    if (!src) return 0;
    const unsigned long long v = ld8(src + (q >> 3));
    return (unsigned)(v >> (8 * (7 - (q & 7)))) & 0xFF;   // putDouble: big-endian
  }
  return f.origin[q - 8 * f.n];
}

// Interior chars come from a 64-byte LDS table, one ds_read_u8 per char: the
// branchy b64url_char mapping made the kernel VALU-bound (~400 integer ops
// per lane for 24 bytes; 30.4 us for a 4M-double partition against 15.8 us
// for a copy of the same bytes).  With the table: 18-20 us.  A 4-chars-per-
// dword SWAR map (v_perm offsets) and staging the wave's input window through
// LDS with coalesced 16-B loads were both slower (tools/publish_sweep.hip,
// profiles/r02/publish_sweep.txt).
__device__ __forceinline__ unsigned b64url_quad_lut(const unsigned char* tab, unsigned v) {
  return (unsigned)tab[(v >> 18) & 63] | ((unsigned)tab[(v >> 12) & 63] << 8) | ((unsigned)tab[(v >> 6) & 63] << 16) |
         ((unsigned)tab[v & 63] << 24);
}

// The three pieces below are shared with k_b64url_encode_flat, whose payload
// is not an accumulator.
// A fast lane's 32 chars from the 4 payload doubles its window spans, as the
// numbers their big-endian bytes spell (v0 first): the window starts 2 bytes
// into v0.
__device__ __forceinline__ void window_chars(unsigned long long v0, unsigned long long v1, unsigned long long v2,
                                             unsigned long long v3, const unsigned char* tab, u4w& c0, u4w& c1) {
  // big-endian words of the 32 payload bytes, then the window's 6 (2 bytes in)
  const unsigned W[8] = {(unsigned)(v0 >> 32), (unsigned)v0, (unsigned)(v1 >> 32), (unsigned)v1,
                         (unsigned)(v2 >> 32), (unsigned)v2, (unsigned)(v3 >> 32), (unsigned)v3};
  unsigned O[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) O[k] = (W[k] << 16) | (W[k + 1] >> 16);
  const unsigned long long X0 = ((unsigned long long)O[0] << 32) | O[1];
  const unsigned long long X1 = ((unsigned long long)O[2] << 32) | O[3];
  const unsigned long long X2 = ((unsigned long long)O[4] << 32) | O[5];
  c0.x = b64url_quad_lut(tab, (unsigned)(X0 >> 40) & 0xFFFFFF);
  c0.y = b64url_quad_lut(tab, (unsigned)(X0 >> 16) & 0xFFFFFF);
  c0.z = b64url_quad_lut(tab, (unsigned)((X0 << 8) | (X1 >> 56)) & 0xFFFFFF);
  c0.w = b64url_quad_lut(tab, (unsigned)(X1 >> 32) & 0xFFFFFF);
  c1.x = b64url_quad_lut(tab, (unsigned)(X1 >> 8) & 0xFFFFFF);
  c1.y = b64url_quad_lut(tab, (unsigned)((X1 << 16) | (X2 >> 48)) & 0xFFFFFF);
  c1.z = b64url_quad_lut(tab, (unsigned)(X2 >> 24) & 0xFFFFFF);
  c1.w = b64url_quad_lut(tab, (unsigned)X2 & 0xFFFFFF);
}

// A slow lane's unit of nb = 1 .. 3 frame bytes (v = the bytes, first in bits 23:16): '=' padding on the last unit
__device__ __forceinline__ unsigned padded_quad(unsigned v, int nb) {
  unsigned q = b64url_quad(v);
  if (nb < 3) q = (q & 0x00FFFFFFu) | ((unsigned)'=' << 24);
  if (nb < 2) q = (q & 0xFF00FFFFu) | ((unsigned)'=' << 16);
  return q;
}

// Each lane's 32 chars go through a wave-private LDS row so that every wave
// then stores its 2 KiB of text as two contiguous 1 KiB rows (lane-strided
// 16-B stores would leave every 128-B line half written per instruction).
// LDS ops of one wave complete in order: a compiler barrier suffices.
// ws = the wave's row, gw = the wave's first group.
__device__ __forceinline__ void store_wave_text(u4w* ws, int lane, const u4w& c0, const u4w& c1,
                                                unsigned char* __restrict__ out, int64_t gw, int64_t text_len) {
  ws[2 * lane] = c0;
  ws[2 * lane + 1] = c1;
  __builtin_amdgcn_wave_barrier();
  const int64_t wbase = 32 * gw;                  // this wave's 2 KiB of text
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u4w v = ws[64 * h + lane];
    const int64_t o = wbase + 1024 * h + 16 * lane;
    if (o + 16 <= text_len) {
      __builtin_nontemporal_store(v, (IPLS_GLOBAL u4w*)(out + o));
    } else if (o < text_len) {   // the text's last partial 16 B
      const unsigned w4[4] = {v.x, v.y, v.z, v.w};
      for (int64_t c = 0; o + c < text_len; ++c) out[o + c] = (unsigned char)(w4[c >> 2] >> (8 * (c & 3)));
    }
  }
  __builtin_amdgcn_wave_barrier();   // the row is rewritten by the next iteration
}

// One text: blocks [0, gridDim.x) of this job walk its groups grid-stride.
// tab = the 64-char table in LDS, stage = 2 * kBlock 16-B rows of LDS.
__device__ __forceinline__ void encode_frame_job(const FrameEnc& f, const unsigned long long* __restrict__ src,
                                                 unsigned char* __restrict__ out, int64_t groups, int64_t text_len,
                                                 const unsigned char* tab, u4w* stage) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u4w* ws = stage + 128 * wv;
  const int64_t F = 14 + 8 * f.n + f.origin_len;   // frame bytes
  for (int64_t g0 = (int64_t)blockIdx.x * kBlock; g0 < groups; g0 += (int64_t)gridDim.x * kBlock) {
    const int64_t gw = g0 + 64 * wv;                // this wave's first group
    const int64_t g = gw + lane;
    const int64_t b0 = 24 * g;
    u4w c0 = {0u, 0u, 0u, 0u}, c1 = {0u, 0u, 0u, 0u};
    if (g < groups && g >= 1 && b0 + 24 <= 14 + 8 * f.n && src) {
      const unsigned long long* s = src + (3 * g - 2);
      const unsigned long long v0 = ld8(s), v1 = ld8(s + 1), v2 = ld8(s + 2), v3 = ld8(s + 3);
      window_chars(v0, v1, v2, v3, tab, c0, c1);
    } else if (g < groups) {
      // header / tail lanes: byte by byte, '=' padding on the last unit
      unsigned q8[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      for (int u = 0; u < 8; ++u) {
        const int64_t j = b0 + 3 * u;
        if (j >= F) break;
        const int nb = F - j >= 3 ? 3 : (int)(F - j);
        unsigned v = frame_byte(f, src, j) << 16;
        if (nb > 1) v |= frame_byte(f, src, j + 1) << 8;
        if (nb > 2) v |= frame_byte(f, src, j + 2);
        q8[u] = padded_quad(v, nb);
      }
      c0 = u4w{q8[0], q8[1], q8[2], q8[3]};
      c1 = u4w{q8[4], q8[5], q8[6], q8[7]};
    }
    store_wave_text(ws, lane, c0, c1, out, gw, text_len);
  }
}

__device__ __forceinline__ void init_b64url_table(unsigned char* tab) {
  if (threadIdx.x < 64) tab[threadIdx.x] = (unsigned char)b64url_char(threadIdx.x);
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void k_b64url_encode_frame(FrameEnc f, const unsigned long long* __restrict__ src,
                                                               unsigned char* __restrict__ out, int64_t groups,
                                                               int64_t text_len) {
  __shared__ u4w stage[2 * kBlock];
  __shared__ unsigned char tab[64];
  init_b64url_table(tab);
  encode_frame_job(f, src, out, groups, text_len, tab, stage);
}

// Several partitions' texts in one launch (the publish loop over Auth_List,
// IPLS.java:1423-1431): blockIdx.y = job.  Every text starts 16-B aligned.
struct FrameJob {
  FrameEnc f;
  const unsigned long long* src;   // accumulator, or null = logically +0.0
  unsigned char* out;
  int64_t groups;
  int64_t text_len;
};

__global__ __launch_bounds__(kBlock) void k_b64url_encode_frames(const FrameJob* __restrict__ jobs) {
  __shared__ u4w stage[2 * kBlock];
  __shared__ unsigned char tab[64];
  init_b64url_table(tab);
  const FrameJob& j = jobs[blockIdx.y];
  encode_frame_job(j.f, j.src, j.out, j.groups, j.text_len, tab, stage);
}

// ---------------------------------------------------------------------------
// Variants, each product rounded, then the sum rounded
// (Java evaluates a*W + b*g left to right, no FMA; -ffp-contract=off here):
//   k_blend : t[i] = a*t[i] + b*g[i]
//             async replica fold  a=0.75, b=1      (Updater.java:57-59)
//             leaving-peer blend  a=0.6,  b=1-0.6  (Updater.java:65-69)
//   k_scale : d[i] = c*s[i]        async publish 0.25*W (Updater.java:197-199)
//   k_encode_secure : Middleware.Encode (Middleware.java:196-210):
//             x > 10 -> 10*1e12, x < -10 -> -10*1e12, else x*1e12
// ---------------------------------------------------------------------------
//   VEC: the tile shape of kEwV 16-B vectors per lane (see k_fold_n).
template <bool BE_IN, bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_blend(double* __restrict__ t, const unsigned long long* __restrict__ g,
                                                  int64_t L, double a, double b) {
  auto one = [&](int64_t i) {
    const double x = decode1<BE_IN>(ld8(g + i));
    const double aw = a * t[i];
    const double bg = b * x;
    t[i] = aw + bg;
  };
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= L) {
      u2 gv[kEwV], tv[kEwV];
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
        gv[v] = __builtin_nontemporal_load((gcu2)(g + i));
        tv[v] = *(gcu2)(t + i);
      }
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const int64_t i = base + 2 * ((int64_t)v * kBlock + threadIdx.x);
        const d2 x = decode2<BE_IN>(gv[v]);
        const d2 w = __builtin_bit_cast(d2, tv[v]);
        const double awx = a * w.x, bgx = b * x.x, awy = a * w.y, bgy = b * x.y;
        *(gu2)(t + i) = __builtin_bit_cast(u2, d2{awx + bgx, awy + bgy});
      }
      return;
    }
    for (int64_t i = base + threadIdx.x; i < L; i += kBlock) one(i);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < L; i += (int64_t)gridDim.x * kBlock) one(i);
  }
}

template <bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_scale(double* __restrict__ d, const double* __restrict__ s, int64_t L,
                                                  double c) {
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= L) {
      u2 sv[kEwV];
#pragma unroll
      for (int v = 0; v < kEwV; ++v)
        sv[v] = __builtin_nontemporal_load((gcu2)(s + base + 2 * ((int64_t)v * kBlock + threadIdx.x)));
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const d2 x = __builtin_bit_cast(d2, sv[v]);
        __builtin_nontemporal_store(__builtin_bit_cast(u2, d2{c * x.x, c * x.y}),
                                    (gu2)(d + base + 2 * ((int64_t)v * kBlock + threadIdx.x)));
      }
      return;
    }
    for (int64_t i = base + threadIdx.x; i < L; i += kBlock) d[i] = c * s[i];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < L; i += (int64_t)gridDim.x * kBlock)
      d[i] = c * s[i];
  }
}

__device__ __forceinline__ double encode_secure1(double x) {
  if (x > 10.0) return 10 * 1e12;
  if (x < -10.0) return -10 * 1e12;
  return x * 1e12;
}

template <bool BE_IN, bool BE_OUT, bool VEC = false>
__global__ __launch_bounds__(kBlock) void k_encode_secure(const unsigned long long* __restrict__ src,
                                                          unsigned long long* __restrict__ dst, int64_t n) {
  auto one = [&](int64_t i) {
    const double y = encode_secure1(decode1<BE_IN>(ld8(src + i)));
    st8(dst + i, BE_OUT ? f64_to_be(y) : __builtin_bit_cast(unsigned long long, y));
  };
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= n) {
      u2 sv[kEwV];
#pragma unroll
      for (int v = 0; v < kEwV; ++v)
        sv[v] = __builtin_nontemporal_load((gcu2)(src + base + 2 * ((int64_t)v * kBlock + threadIdx.x)));
#pragma unroll
      for (int v = 0; v < kEwV; ++v) {
        const d2 x = decode2<BE_IN>(sv[v]);
        __builtin_nontemporal_store(encode2<BE_OUT>(d2{encode_secure1(x.x), encode_secure1(x.y)}),
                                    (gu2)(dst + base + 2 * ((int64_t)v * kBlock + threadIdx.x)));
      }
      return;
    }
    for (int64_t i = base + threadIdx.x; i < n; i += kBlock) one(i);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) one(i);
  }
}

// ---------------------------------------------------------------------------
// Saved-model files (javaser.hpp): Java object streams whose double payloads
// sit at byte offsets that are never 8-B aligned (MAP 5 or 1 mod 8, DARR 27,
// DLIST odd offsets in a 14-byte stride).  An image is the file's bytes (or a
// contiguous piece of them) in a 16-B aligned device buffer; a job is one run
// of framing + payload inside it.  blockIdx.y = job.
//
// Pack: the image's aligned 16-B words that lie wholly inside a payload are
// each written once, by one non-temporal 16-B store composed in registers
// from the neighbouring values (a funnel shift by the job's byte residue);
// the bytes before the first and after the last such word of a job -- its
// framing, under 16 payload bytes each side, the suffix -- are written one
// byte at a time by the job's first block.  No byte has two writers, and a
// 16-B word that two jobs share is byte-written by both (disjoint bytes).
// ---------------------------------------------------------------------------
constexpr int kSerV = 4;                                       // 16-B words per lane per tile
constexpr int64_t kSerTileWords = (int64_t)kBlock * kSerV;     // 16 KiB of image per block
constexpr int kSerPrefixMax = 192;

struct SerPackJob {
  const unsigned long long* src;   // n native doubles, or null = logically +0.0
  int64_t n;
  int64_t pos;                     // image byte offset of the job's first byte
  int32_t prefix_len;
  int32_t suffix;                  // one byte after the payload, or -1
  unsigned char prefix[kSerPrefixMax];
};

// X = the 8 stream bytes that start s bytes (0..7) into the big-endian
// sequence hi, lo -- as a big-endian integer
__device__ __forceinline__ unsigned long long ser_funnel(unsigned long long hi, unsigned long long lo, int s) {
  return s ? (hi << (8 * s)) | (lo >> (64 - 8 * s)) : hi;
}

__device__ __forceinline__ unsigned ser_pack_byte(const SerPackJob& j, int64_t B, int64_t E, int64_t a) {
  if (a < B) return j.prefix[a - j.pos];
  if (a >= E) return (unsigned)j.suffix;
  if (!j.src) return 0;
  const int64_t q = a - B;
  return (unsigned)(ld8(j.src + (q >> 3)) >> (8 * (7 - (q & 7)))) & 0xFF;
}

__global__ __launch_bounds__(kBlock) void k_ser_pack(const SerPackJob* __restrict__ jobs, unsigned char* __restrict__ img) {
  const SerPackJob& j = jobs[blockIdx.y];
  const int64_t B = j.pos + j.prefix_len, E = B + 8 * j.n;     // the payload's bytes
  const int64_t end = E + (j.suffix >= 0 ? 1 : 0);
  int64_t w0 = (B + 15) >> 4, w1 = E >> 4;                      // whole words [w0, w1)
  if (w1 < w0) w1 = w0;
  const int s = (int)((16 * w0 - B) & 7);                       // bytes into value k where a word starts
  const unsigned long long* src = j.src;
  // word w starts in value k = (16 w - B) >> 3 and needs values k, k + 1 and (s > 0) k + 2 < n
  auto compose = [&](unsigned long long a, unsigned long long b, unsigned long long c) {
    return u2{__builtin_bswap64(ser_funnel(a, b, s)), __builtin_bswap64(ser_funnel(b, c, s))};
  };
  for (int64_t t0 = w0 + (int64_t)blockIdx.x * kSerTileWords; t0 < w1; t0 += (int64_t)gridDim.x * kSerTileWords) {
    if (!src) {
#pragma unroll
      for (int v = 0; v < kSerV; ++v) {
        const int64_t w = t0 + (int64_t)v * kBlock + threadIdx.x;
        if (w < w1) __builtin_nontemporal_store(u2{0, 0}, (gu2)(img + 16 * w));
      }
      continue;
    }
    unsigned long long a[kSerV], b[kSerV], c[kSerV];
#pragma unroll
    for (int v = 0; v < kSerV; ++v) {
      const int64_t w = t0 + (int64_t)v * kBlock + threadIdx.x;
      a[v] = b[v] = c[v] = 0;
      if (w < w1) {
        const int64_t k = (16 * w - B) >> 3;
        a[v] = ld8(src + k);
        b[v] = ld8(src + k + 1);
        if (s) c[v] = ld8(src + k + 2);
      }
    }
#pragma unroll
    for (int v = 0; v < kSerV; ++v) {
      const int64_t w = t0 + (int64_t)v * kBlock + threadIdx.x;
      if (w < w1) __builtin_nontemporal_store(compose(a[v], b[v], c[v]), (gu2)(img + 16 * w));
    }
  }
  if (blockIdx.x == 0) {
    const int64_t head_end = w1 > w0 ? 16 * w0 : end;           // no whole word: everything byte-wise
    for (int64_t a = j.pos + threadIdx.x; a < head_end; a += kBlock) img[a] = (unsigned char)ser_pack_byte(j, B, E, a);
    if (w1 > w0)
      for (int64_t a = 16 * w1 + threadIdx.x; a < end; a += kBlock) img[a] = (unsigned char)ser_pack_byte(j, B, E, a);
  }
}

// Boxed pack (DLIST): after the job's prefix come n records of 14 bytes whose
// first six are constant, except that the first record's six are the last six
// bytes of the prefix -- so the record region starts at B = pos + prefix_len
// - 6 and value g sits at B + 14 g + 6.  A 16-B word touches at most two
// values and the first lead byte of a third record.  Values are
// doubleToLongBits: NaN canonicalised.
constexpr unsigned long long kBoxLead = 0x7371007E0002ull;      // TC_OBJECT TC_REFERENCE 0x7e0002, 48 bits

__device__ __forceinline__ unsigned long long canon_nan_bits(unsigned long long v) {
  return ((v & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (v & 0x000FFFFFFFFFFFFFull)) ? 0x7FF8000000000000ull : v;
}

__device__ __forceinline__ unsigned ser_box_byte(const SerPackJob& j, int64_t B, int64_t E, int64_t a) {
  if (a < B + 6) return j.prefix[a - j.pos];
  if (a >= E) return (unsigned)j.suffix;
  const int64_t t = a - B, g = t / 14;
  const int o = (int)(t - 14 * g);
  if (o < 6) return (unsigned)(kBoxLead >> (8 * (5 - o))) & 0xFF;
  const unsigned long long v = j.src ? canon_nan_bits(ld8(j.src + g)) : 0;
  return (unsigned)(v >> (8 * (13 - o))) & 0xFF;
}

__global__ __launch_bounds__(kBlock) void k_ser_pack_boxed(const SerPackJob* __restrict__ jobs,
                                                           unsigned char* __restrict__ img) {
  const SerPackJob& j = jobs[blockIdx.y];
  const int64_t B = j.pos + j.prefix_len - 6, E = B + 14 * j.n;   // records [B, E)
  const int64_t end = E + (j.suffix >= 0 ? 1 : 0);
  int64_t w0 = (B + 6 + 15) >> 4, w1 = E >> 4;                    // whole words past the prefix
  if (w1 < w0) w1 = w0;
  const unsigned long long* src = j.src;
  for (int64_t t0 = w0 + (int64_t)blockIdx.x * kSerTileWords; t0 < w1; t0 += (int64_t)gridDim.x * kSerTileWords) {
#pragma unroll
    for (int v = 0; v < kSerV; ++v) {
      const int64_t w = t0 + (int64_t)v * kBlock + threadIdx.x;
      if (w >= w1) continue;
      const int64_t t = 16 * w - B, g = t / 14;
      const int o = (int)(t - 14 * g);                              // 0..13: where the word starts in record g
      // record g + 1 exists whenever the word reaches its value (o > 4)
      unsigned long long x = 0, y = 0;
      if (src) {
        x = canon_nan_bits(ld8(src + g));
        if (o > 4) y = canon_nan_bits(ld8(src + g + 1));
      }
      // the 32 stream bytes from record g's start, as big-endian words
      const unsigned long long q0 = (kBoxLead << 16) | (x >> 48), q1 = (x << 16) | (kBoxLead >> 32),
                               q2 = (kBoxLead << 32) | (y >> 32), q3 = (y << 32) | (kBoxLead >> 16);
      const int sh = o & 7;
      const unsigned long long lo = o < 8 ? q0 : q1, mid = o < 8 ? q1 : q2, hi = o < 8 ? q2 : q3;
      __builtin_nontemporal_store(u2{__builtin_bswap64(ser_funnel(lo, mid, sh)), __builtin_bswap64(ser_funnel(mid, hi, sh))},
                                  (gu2)(img + 16 * w));
    }
  }
  if (blockIdx.x == 0) {
    const int64_t head_end = w1 > w0 ? 16 * w0 : end;
    for (int64_t a = j.pos + threadIdx.x; a < head_end; a += kBlock) img[a] = (unsigned char)ser_box_byte(j, B, E, a);
    if (w1 > w0)
      for (int64_t a = 16 * w1 + threadIdx.x; a < end; a += kBlock) img[a] = (unsigned char)ser_box_byte(j, B, E, a);
  }
}

// Unpack and apply: target[i] = v[i] (SET) or a*target[i] + b*v[i] (BLEND:
// k_blend's arithmetic, both products rounded, then the sum), v[i] the
// big-endian double at image byte off + 8 i, any residue.  The image buffer is
// readable for 32 bytes past its last payload byte.
struct SerApplyJob {
  double* dst;
  int64_t n;
  int64_t off;                     // image byte offset of the payload
};

// the 8 image bytes at byte a, as the value they encode (two aligned 8-B loads)
__device__ __forceinline__ unsigned long long ser_load_be(const unsigned char* img, int64_t a) {
  const unsigned long long* w = (const unsigned long long*)(img + (a & ~(int64_t)7));
  const int r = (int)(a & 7);
  const unsigned long long m0 = ld8(w);
  if (!r) return __builtin_bswap64(m0);
  return __builtin_bswap64((m0 >> (8 * r)) | (ld8(w + 1) << (64 - 8 * r)));
}

template <bool BLEND>
__global__ __launch_bounds__(kBlock) void k_ser_apply(const SerApplyJob* __restrict__ jobs,
                                                      const unsigned char* __restrict__ img, double a, double b) {
  const SerApplyJob& j = jobs[blockIdx.y];
  double* dst = j.dst;
  auto put = [&](double t, unsigned long long bits) {
    const double x = __builtin_bit_cast(double, bits);
    if constexpr (BLEND) {
      const double aw = a * t, bg = b * x;
      return aw + bg;
    } else {
      return x;
    }
  };
  const bool vec = (((uintptr_t)dst) & 15) == 0;
  const int64_t pairs = vec ? j.n >> 1 : 0;
  const int r = (int)(j.off & 15), rr = r & 7;                    // the same for every pair of the job
  for (int64_t t0 = (int64_t)blockIdx.x * kSerTileWords; t0 < pairs; t0 += (int64_t)gridDim.x * kSerTileWords) {
    u2 m0[kSerV], m1[kSerV], tv[kSerV];
#pragma unroll
    for (int v = 0; v < kSerV; ++v) {
      const int64_t i = t0 + (int64_t)v * kBlock + threadIdx.x;
      if (i < pairs) {
        const unsigned long long* w = (const unsigned long long*)(img + ((j.off + 16 * i) & ~(int64_t)15));
        m0[v] = __builtin_nontemporal_load((gcu2)w);
        m1[v] = r ? *(gcu2)(w + 2) : u2{0, 0};
        if constexpr (BLEND) tv[v] = *(gcu2)(dst + 2 * i);
      }
    }
#pragma unroll
    for (int v = 0; v < kSerV; ++v) {
      const int64_t i = t0 + (int64_t)v * kBlock + threadIdx.x;
      if (i < pairs) {
        // the 32 image bytes from the aligned word, as little-endian words
        const unsigned long long a0 = m0[v].x, a1 = m0[v].y, a2 = m1[v].x, a3 = m1[v].y;
        const unsigned long long l0 = r < 8 ? a0 : a1, l1 = r < 8 ? a1 : a2, l2 = r < 8 ? a2 : a3;
        const unsigned long long e0 = rr ? (l0 >> (8 * rr)) | (l1 << (64 - 8 * rr)) : l0;
        const unsigned long long e1 = rr ? (l1 >> (8 * rr)) | (l2 << (64 - 8 * rr)) : l1;
        d2 t = d2{0.0, 0.0};
        if constexpr (BLEND) t = __builtin_bit_cast(d2, tv[v]);
        const double ox = put(t.x, __builtin_bswap64(e0)), oy = put(t.y, __builtin_bswap64(e1));
        *(gu2)(dst + 2 * i) = __builtin_bit_cast(u2, d2{ox, oy});
      }
    }
  }
  // the odd last value, or every value of a target that is not 16-B aligned
  for (int64_t i = 2 * pairs + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < j.n; i += (int64_t)gridDim.x * kBlock)
    dst[i] = put(BLEND ? dst[i] : 0.0, ser_load_be(img, j.off + 8 * i));
}

// Unpack, boxed (DLIST): out[g - g0] = value g for g in [g0, g1) of the
// records at image byte rec0 + 14 g (six lead bytes, eight value bytes); a
// record g >= 1 whose lead is not the constant sets *flag.  The host checks
// the flag before anything is applied.
__global__ __launch_bounds__(kBlock) void k_ser_unbox(const unsigned char* __restrict__ img, int64_t rec0, int64_t g0,
                                                      int64_t g1, unsigned long long* __restrict__ out,
                                                      unsigned* __restrict__ flag) {
  for (int64_t g = g0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; g < g1; g += (int64_t)gridDim.x * kBlock) {
    const int64_t a = rec0 + 14 * (g - g0);
    if (g >= 1 && (ser_load_be(img, a) >> 16) != kBoxLead) *flag = 1u;
    out[g - g0] = ser_load_be(img, a + 6);
  }
}

// ===========================================================================
// Trainer boundary: sources and outputs narrower than a double.  float32
// (Model.java:423 widens a float INDArray to the doubles it hands to
// UpdateGradient; Model.java:388-390 narrows GetPartitions' doubles back into
// one) and the two 16-bit formats a trainer under autocast (or a DL4J network
// built with DataType.HALF / BFLOAT16) holds.  One kernel per job, with the
// format as a template parameter S (FmtF32, FmtF16, FmtBF16).
// Sources: v = (double)src[i] in registers -- a float directly, binary16 by
// f16 -> f32 -> f64, bfloat16 by (bits << 16) taken as an f32 -> f64; every
// step is exact, subnormals included (no flush flag anywhere: a bf16 subnormal
// is an f32 subnormal) -- then every expression is the f64 kernel's, so the
// bits are those of the f64 path fed the widened values.
// Outputs: the f64 quotient rounded once to float (v_cvt_f32_f64, ties to
// even), and for a 16-bit format that float rounded to the format (ties to
// even, overflow to +-inf, subnormals kept, -0.0 kept, NaN stays NaN): two
// roundings, what a trainer gets when it narrows the f32 output itself.
//
// A format supplies:
//   elem, raw        the element type of a buffer; one loaded element
//   Vec<E>, ldv<E>   E consecutive elements as loaded by one non-temporal load
//   get<E>(v, c)     element c of such a vector, widened
//   unpack(v)        such a vector as a lane of the fold keeps it until the adds
//   ldraw, widen     the scalar load and its widening
//   narrow(float)    the element's bit pattern for a float; put stores one
//   kPeersVec<E>     peers in flight on the fold's partial-tile vector steps
// ===========================================================================
typedef float f4 __attribute__((ext_vector_type(4)));

// 4 floats of one load as the fold keeps them between the load and the adds: unpacked, like
// HWords.  Kept as one float4 value, hipcc carries the fold's prefetched peer as 64-bit pairs and
// the fold at config C measured 0.3-0.5 % slower (profiles/narrow_unify/float4_fold/).  The split
// keeps the float4: unpacked there, its accumulate form measured 0.3 % slower
// (profiles/narrow_unify/unpacked_split/).
struct FQuad {
  float f[4];
};
struct FmtF32 {
  typedef float elem;
  typedef float raw;
  template <int E>
  using Vec = f4;
  template <int E>
  static constexpr int kPeersVec = 8;
  template <int E>
  static __device__ __forceinline__ f4 ldv(const float* p) {
    static_assert(E == 4, "floats come 4 to a 16-B load");
    return __builtin_nontemporal_load((const IPLS_GLOBAL f4*)p);
  }
  static __device__ __forceinline__ FQuad unpack(const f4& t) { return FQuad{{t.x, t.y, t.z, t.w}}; }
  template <int E>
  static __device__ __forceinline__ double get(const f4& v, int c) { return (double)v[c]; }
  template <int E>
  static __device__ __forceinline__ double get(const FQuad& v, int c) { return (double)v.f[c]; }
  static __device__ __forceinline__ float ldraw(const float* p) { return *(const IPLS_GLOBAL float*)p; }
  static __device__ __forceinline__ double widen(float f) { return (double)f; }
  // the caller's (float)d is the output: nothing more to round
  static __device__ __forceinline__ unsigned narrow(float f) { return __builtin_bit_cast(unsigned, f); }
  static __device__ __forceinline__ void put(float* p, unsigned b) { *p = __builtin_bit_cast(float, b); }
};

// E consecutive 16-bit elements as E / 2 words: one 8-B (E = 4) or 16-B (E = 8) non-temporal load
template <int E>
struct HWords {
  unsigned w[E / 2];
};
// what the two 16-bit formats share; D supplies widen, lo / hi (the two elements of a word) and narrow
template <class D>
struct Fmt16 {
  typedef unsigned short elem;
  typedef unsigned short raw;
  template <int E>
  using Vec = HWords<E>;
  // 64 B per lane in flight (8 peers of 16 B next to 8 f64 accumulators spill at 1024 lanes)
  template <int E>
  static constexpr int kPeersVec = 32 / E;
  template <int E>
  static __device__ __forceinline__ HWords<E> ldv(const unsigned short* p) {
    HWords<E> r;
    if constexpr (E == 8) {
      const u4w t = __builtin_nontemporal_load((const IPLS_GLOBAL u4w*)p);
      r.w[0] = t.x, r.w[1] = t.y, r.w[2] = t.z, r.w[3] = t.w;
    } else {
      static_assert(E == 4, "4 or 8 elements per load");
      typedef unsigned u2w __attribute__((ext_vector_type(2)));
      const u2w t = __builtin_nontemporal_load((const IPLS_GLOBAL u2w*)p);
      r.w[0] = t.x, r.w[1] = t.y;
    }
    return r;
  }
  template <int E>
  static __device__ __forceinline__ const HWords<E>& unpack(const HWords<E>& v) { return v; }
  template <int E>
  static __device__ __forceinline__ double get(const HWords<E>& v, int c) {
    return (c & 1) ? D::hi(v.w[c >> 1]) : D::lo(v.w[c >> 1]);
  }
  static __device__ __forceinline__ unsigned short ldraw(const unsigned short* p) {
    return *(const IPLS_GLOBAL unsigned short*)p;
  }
  static __device__ __forceinline__ void put(unsigned short* p, unsigned b) {
    *(IPLS_GLOBAL unsigned short*)p = (unsigned short)b;
  }
};
struct FmtF16 : Fmt16<FmtF16> {     // IEEE binary16
  static __device__ __forceinline__ double widen(unsigned short b) {
    return (double)(float)__builtin_bit_cast(_Float16, b);
  }
  static __device__ __forceinline__ double lo(unsigned w) { return widen((unsigned short)(w & 0xffffu)); }
  static __device__ __forceinline__ double hi(unsigned w) { return widen((unsigned short)(w >> 16)); }
  // v_cvt_f16_f32.  The caller's (float)d must stay a rounding of its own (v_cvt_f32_f64): the library is built
  // with -ffp-contract=off -fno-fast-math, under which hipcc keeps both; without them it folds the pair into one
  // f64 -> f16 sequence, a single rounding (test_get_partitions_h16's 0x3c00 quotient fails then).
  static __device__ __forceinline__ unsigned narrow(float f) {
    return __builtin_bit_cast(unsigned short, (_Float16)f);
  }
};
struct FmtBF16 : Fmt16<FmtBF16> {   // bfloat16: the upper half of an f32
  static __device__ __forceinline__ double widen(unsigned short b) {
    return (double)__builtin_bit_cast(float, (unsigned)b << 16);
  }
  static __device__ __forceinline__ double lo(unsigned w) { return (double)__builtin_bit_cast(float, w << 16); }
  static __device__ __forceinline__ double hi(unsigned w) { return (double)__builtin_bit_cast(float, w & 0xffff0000u); }
  static __device__ __forceinline__ unsigned narrow(float f) {   // v_cvt_pk_bf16_f32 on gfx950
    return __builtin_bit_cast(unsigned short, (__bf16)f);
  }
};

// ---------------------------------------------------------------------------
// k_reduce_narrow: the batched fixed-order fold (k_reduce) over buckets of a
// narrow format.  Grid = n_parts * tiles_per_part blocks of BS lanes; a tile
// is BS * E * R elements.  A lane owns E consecutive elements per vector: one
// non-temporal load per peer per vector, E widenings, E chained f64 adds into
// E accumulators, E / 2 16-B stores (native doubles, or BE_OUT bytes).  The
// peer axis is walked in order per element, as in reduce_tiles.
//   E   : 4 is what the library instantiates (with XP = 1): 16-B loads of
//         floats, 8-B loads of 16-bit elements, and the lane ^ 4 swap below
//         before the stores.  Floats have no other layout.  E = 8 and XP = 0
//         exist for 16-bit sources and tools/reduce_h16_sweep.hip only: the
//         layout that lost the sweep and the no-exchange baselines, kept so
//         that the sweep recorded in DESIGN.md 3.5.1 can be re-run on the same
//         kernel body.  8 = 16-B loads; the lane's 8 sums are 64 B, so the 8
//         lanes that own four adjacent 128-B lines transpose their 16-B pairs
//         among themselves (two butterfly steps, lane ^ 4 then lane ^ 2) and
//         every store instruction writes whole lines.
//   VEC : every bucket and every destination of the launch is 16-B aligned
//         (decided by the host); full tiles then take the vector path and the
//         partial last tile E*BS-element vector steps with a scalar remainder.
//         !VEC: everything element by element (buckets at 4 mod 16 etc.;
//         element-sized loads, 8 peers in flight).
//   MAP : 0 partition-major, 3 partial tiles first (map_block).
//   PF  : 1 = peer j+1's R loads are issued before peer j's values are added
//         (two peers' loads in flight per lane, the fold order unchanged).
//   XP  : 0 = no exchange between lanes, every lane stores its own sums as
//         they lie (quarter or half lines per store instruction): the sweep's
//         baseline for the two layouts, not used by the library.
// ACCUM reads the target in BE_OUT's byte order, like k_reduce.
// ---------------------------------------------------------------------------
template <class S, bool BE_OUT, int START, int R, int BS, int MAP, bool VEC, int PF = 0, int E = 4, int XP = 1>
__global__ __launch_bounds__(BS) void k_reduce_narrow(const typename S::elem* const* __restrict__ bufs,
                                                      const PartDesc* __restrict__ parts, int k, int tiles_per_part,
                                                      int n_parts) {
  typedef typename S::elem T;
  auto ldu = [](const T* p) { return S::unpack(S::template ldv<E>(p)); };   // what a lane keeps of a load
  typedef decltype(ldu((const T*)nullptr)) V;
  static_assert(E == 4 || (E == 8 && sizeof(T) == 2), "8 elements per lane: 16-bit sources only");
  static_assert(XP == 1 || sizeof(T) == 2, "the no-exchange baseline: 16-bit sources only");
  constexpr int64_t kTile = (int64_t)BS * E * R;
  constexpr int kPB = 8;                               // peers in flight on the element-by-element path
  constexpr int kPBV = S::template kPeersVec<E>;       // ... and on the partial tile's vector steps
  int q, t;
  map_block(MAP, gridDim.x, tiles_per_part, n_parts, q, t);
  if (q >= n_parts) return;
  const int64_t L = parts[q].len;
  const int64_t base = (int64_t)t * kTile;
  if (base >= L) return;
  unsigned long long* __restrict__ dst = parts[q].dst;
  const T* const* __restrict__ pb = bufs + (size_t)q * k;
  const int tid = threadIdx.x;
  const int j0 = (START == kFirst) ? 1 : 0;

  auto add = [](double (&a)[E], const V& v) {
#pragma unroll
    for (int c = 0; c < E; ++c) a[c] = a[c] + S::template get<E>(v, c);
  };
  auto init = [&](double (&a)[E], int64_t o) {
    if constexpr (START == kZero) {
#pragma unroll
      for (int c = 0; c < E; ++c) a[c] = 0.0;
    } else if constexpr (START == kFirst) {
      const V x = ldu(pb[0] + o);
#pragma unroll
      for (int c = 0; c < E; ++c) a[c] = S::template get<E>(x, c);
    } else {
#pragma unroll
      for (int c = 0; c < E / 2; ++c) {
        const d2 x = decode2<BE_OUT>(ld16<false>(dst + o + 2 * c));
        a[2 * c] = x.x, a[2 * c + 1] = x.y;
      }
    }
  };

  if (VEC && base + kTile <= L) {
    // lane's first element of the tile; vector r is r * BS * E elements on
    const int64_t o0 = base + E * (int64_t)tid;
    double acc[R][E];
#pragma unroll
    for (int r = 0; r < R; ++r) init(acc[r], o0 + (int64_t)r * BS * E);
    if constexpr (PF) {
      V v[R];
      if (j0 < k) {
        const T* __restrict__ src = pb[j0] + o0;
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = ldu(src + (int64_t)r * BS * E);
      }
      for (int j = j0; j < k; ++j) {
        V nx[R];
        if (j + 1 < k) {
          const T* __restrict__ src = pb[j + 1] + o0;
#pragma unroll
          for (int r = 0; r < R; ++r) nx[r] = ldu(src + (int64_t)r * BS * E);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) add(acc[r], v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = nx[r];
      }
    } else {
      for (int j = j0; j < k; ++j) {
        const T* __restrict__ src = pb[j] + o0;
        V v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = ldu(src + (int64_t)r * BS * E);
#pragma unroll
        for (int r = 0; r < R; ++r) add(acc[r], v[r]);
      }
    }
    if constexpr (!XP) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < E / 2; ++c)
          __builtin_nontemporal_store(encode2<BE_OUT>(d2{acc[r][2 * c], acc[r][2 * c + 1]}),
                                      (gu2)(dst + o0 + (int64_t)r * BS * E + 2 * c));
    } else if constexpr (E == 4) {
      // A lane's 4 sums are 32 B, so its own two 16-B stores would each cover
      // half of every 128-B line the wave writes (measured: WRITE_SIZE 1.12x the
      // algorithmic 8 L).  Instead the 8 lanes that own two adjacent lines
      // (lanes 0-3 the first, 4-7 the second) swap their upper pair of sums
      // with lane ^ 4: the first store instruction then writes the first line
      // whole -- lanes 0-3 their own lower pairs, lanes 4-7 the upper pairs of
      // lanes 0-3 -- and the second one the second line.  Values only move
      // between lanes; every sum is unchanged.
      const bool hi = tid & 4;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t o = o0 + (int64_t)r * BS * 4;
        const d2 own = d2{acc[r][0], acc[r][1]};
        const d2 got = d2{__shfl_xor(acc[r][2], 4), __shfl_xor(acc[r][3], 4)};   // elements o ^ 16 .. + 2, + 3
        __builtin_nontemporal_store(encode2<BE_OUT>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
        __builtin_nontemporal_store(encode2<BE_OUT>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
      }
    } else {
      // A lane's 8 sums are 64 B = pairs 0..3; lanes 8g..8g+7 own four adjacent
      // lines (32 pairs).  Pair i of lane (a2 a1 a0) sits at pair address
      // 4 * lane + i.  Two exchanges move the line number (the lane's upper two
      // bits) into the pair index: with lane ^ 4 the pairs whose bit 1 differs
      // from a2, with lane ^ 2 those whose bit 0 differs from a1.  Afterwards
      // pair slot i of every lane of the group belongs to line i, at 16-B slot
      // 4 a0 + 2 a2 + a1 of it, and store instruction i writes line i whole.
      // Values only move between lanes; every sum is unchanged.
      const bool a2 = tid & 4, a1 = tid & 2;
      const int64_t slot = 8 * (tid & 1) + 4 * ((tid >> 2) & 1) + 2 * ((tid >> 1) & 1);   // in doubles
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t g = o0 + (int64_t)r * BS * 8 - 8 * (tid & 7);   // the group's first element
        double p[4][2], s[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i][0] = acc[r][2 * i], p[i][1] = acc[r][2 * i + 1];
#pragma unroll
        for (int i = 0; i < 2; ++i)     // step 1: send pairs with bit 1 != a2
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const double got = __shfl_xor(a2 ? p[i][c] : p[2 + i][c], 4);
            s[i][c] = a2 ? got : p[i][c];
            s[2 + i][c] = a2 ? p[2 + i][c] : got;
          }
#pragma unroll
        for (int i = 0; i < 2; ++i)     // step 2: send pairs with bit 0 != a1
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const double got = __shfl_xor(a1 ? s[2 * i][c] : s[2 * i + 1][c], 2);
            p[2 * i][c] = a1 ? got : s[2 * i][c];
            p[2 * i + 1][c] = a1 ? s[2 * i + 1][c] : got;
          }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          __builtin_nontemporal_store(encode2<BE_OUT>(d2{p[i][0], p[i][1]}), (gu2)(dst + g + 16 * i + slot));
      }
    }
    return;
  }
  // ------- partial last tile, or a launch with a misaligned operand -------
  const int64_t end = base + kTile < L ? base + kTile : L;
  int64_t sb = base;
  if constexpr (VEC) {
    for (; sb + E * BS <= end; sb += E * BS) {
      const int64_t o = sb + E * (int64_t)tid;
      double a[E];
      init(a, o);
      int jj = j0;
      for (; jj + kPBV <= k; jj += kPBV) {
        V v[kPBV];
#pragma unroll
        for (int g = 0; g < kPBV; ++g) v[g] = ldu(pb[jj + g] + o);
#pragma unroll
        for (int g = 0; g < kPBV; ++g) add(a, v[g]);
      }
      for (; jj < k; ++jj) add(a, ldu(pb[jj] + o));
#pragma unroll
      for (int c = 0; c < E / 2; ++c)
        __builtin_nontemporal_store(encode2<BE_OUT>(d2{a[2 * c], a[2 * c + 1]}), (gu2)(dst + o + 2 * c));
    }
  }
  for (int64_t e = sb + tid; e < end; e += BS) {
    double acc;
    if constexpr (START == kZero) acc = 0.0;
    else if constexpr (START == kFirst) acc = S::widen(S::ldraw(pb[0] + e));
    else acc = decode1<BE_OUT>(ld8(dst + e));
    int jj = j0;
    for (; jj + kPB <= k; jj += kPB) {
      typename S::raw v[kPB];
#pragma unroll
      for (int g = 0; g < kPB; ++g) v[g] = S::ldraw(pb[jj + g] + e);
#pragma unroll
      for (int g = 0; g < kPB; ++g) acc = acc + S::widen(v[g]);
    }
    for (; jj < k; ++jj) acc = acc + S::widen(S::ldraw(pb[jj] + e));
    st8(dst + e, BE_OUT ? f64_to_be(acc) : __builtin_bit_cast(unsigned long long, acc));
  }
}

// ---------------------------------------------------------------------------
// k_fold1_narrow: the single-bucket fold of one arrival (k_fold1) over a
// bucket of a narrow format, pointers passed as kernel arguments -- no table.
//   dst[i] = start + S::widen(src[i]),  start: ZERO +0.0 | ACCUM dst[i]
// The targets are native doubles in the arena: no BE_OUT, no FIRST.
// A lane owns 4 consecutive elements per group: one non-temporal load through
// ldv<4> (16 B of floats, 8 B of 16-bit elements), for ACCUM two 16-B target
// loads, four widenings, four f64 adds.  A block's trip is kBlock * R groups
// (4 * kBlock * R elements), a lane's R groups kBlock groups apart, all loads
// before the adds; the blocks walk the bucket in a grid-stride loop.  A trip
// that lies wholly inside the bucket stores through k_reduce_narrow's lane ^ 4
// exchange, so each store instruction writes whole 128-B lines and nothing
// outside the trip; a block's one partial trip stores every lane's own two
// pairs.  The last L mod 4 elements go element by element from one lane.
// src is aligned to the lane's load and dst to 16 B (decided by the host).
// ---------------------------------------------------------------------------
template <class S, int START, int R = 4>
__global__ __launch_bounds__(kBlock) void k_fold1_narrow(unsigned long long* __restrict__ dst,
                                                         const typename S::elem* __restrict__ src, int64_t L) {
  static_assert(START == kZero || START == kAccum, "an arrival adds to +0.0 or to the target");
  typedef typename S::elem T;
  auto ldu = [](const T* p) { return S::unpack(S::template ldv<4>(p)); };
  typedef decltype(ldu((const T*)nullptr)) V;
  const int64_t n4 = L >> 2;   // whole groups
  const int64_t trip = (int64_t)kBlock * R, stride = (int64_t)gridDim.x * trip;
  const int tid = threadIdx.x;
  auto sums = [](double (&a)[4], const V& v, const u2& t0, const u2& t1) {
    if constexpr (START == kZero) {
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = 0.0;
    } else {
      const d2 x = __builtin_bit_cast(d2, t0), y = __builtin_bit_cast(d2, t1);
      a[0] = x.x, a[1] = x.y, a[2] = y.x, a[3] = y.y;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = a[c] + S::template get<4>(v, c);
  };
  int64_t B = (int64_t)blockIdx.x * trip;
  for (; B + trip <= n4; B += stride) {   // the whole trip in range: loads first, whole-line stores
    const int64_t g0 = B + tid;
    V v[R];
    u2 t[R][2];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = ldu(src + 4 * (g0 + (int64_t)r * kBlock));
    if constexpr (START == kAccum) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        t[r][0] = ld16<false>(dst + 4 * (g0 + (int64_t)r * kBlock));
        t[r][1] = ld16<false>(dst + 4 * (g0 + (int64_t)r * kBlock) + 2);
      }
    }
    const bool hi = tid & 4;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double a[4];
      sums(a, v[r], t[r][0], t[r][1]);
      // lanes 8m..8m+3 own one 128-B line of sums, 8m+4..8m+7 the next: the
      // upper pairs change hands with lane ^ 4 (k_reduce_narrow's E == 4 stores)
      const int64_t o = 4 * (g0 + (int64_t)r * kBlock);
      const d2 own = d2{a[0], a[1]};
      const d2 got = d2{__shfl_xor(a[2], 4), __shfl_xor(a[3], 4)};   // elements (o ^ 16) + 2, + 3
      __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
      __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
    }
  }
  if (B < n4) {   // this block's partial trip: every lane stores its own pairs
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t g = B + tid + (int64_t)r * kBlock;
      if (g < n4) {
        const int64_t o = 4 * g;
        const V v = ldu(src + o);
        u2 t0 = u2{0, 0}, t1 = u2{0, 0};
        if constexpr (START == kAccum) t0 = ld16<false>(dst + o), t1 = ld16<false>(dst + o + 2);
        double a[4];
        sums(a, v, t0, t1);
        __builtin_nontemporal_store(encode2<false>(d2{a[0], a[1]}), (gu2)(dst + o));
        __builtin_nontemporal_store(encode2<false>(d2{a[2], a[3]}), (gu2)(dst + o + 2));
      }
    }
  }
  if ((L & 3) && blockIdx.x == 0 && tid == 0) {   // the last L mod 4 elements
    for (int64_t e = 4 * n4; e < L; ++e) {
      const double x = S::widen(S::ldraw(src + e));
      const double a = ((START == kZero) ? 0.0 : __builtin_bit_cast(double, ld8(dst + e))) + x;
      st8(dst + e, __builtin_bit_cast(unsigned long long, a));
    }
  }
}

// k_split over a flat vector of a narrow format: OrganizeGradients (MODE 0)
// and UpdateGradient's own accumulate (MODE 1, 2), the expressions of k_split
// on v = (double)flat[lo + i].  VEC (decided by the host per partition: flat +
// p*chunk is only element-aligned in general): the partition's slice of the
// flat vector and its destination are both 16-B aligned; a block then owns
// kEwTile consecutive elements and a lane kEwTile / kBlock = 8 of them, as
// 16-B loads of 16 / sizeof(elem) elements (2 vectors of 4 floats, vector k at
// base + 4 * (k * kBlock + lane), or 1 vector of 8 16-bit elements).  The tile
// that holds the count slot (1.0, what a widened count slot of 1 is) goes
// element by element.
template <class S, bool BE_OUT, int MODE, bool VEC>
__global__ __launch_bounds__(kBlock) void k_split_narrow(const typename S::elem* __restrict__ flat, int64_t lo,
                                                         int64_t ncopy, int64_t L,
                                                         unsigned long long* __restrict__ dst) {
  static_assert(MODE == 0 || !BE_OUT, "the folds write native doubles");
  constexpr int EV = 16 / sizeof(typename S::elem);   // elements per load
  constexpr int NV = kEwTile / kBlock / EV;           // loads per lane
  static_assert((int64_t)kBlock * EV * NV == kEwTile, "one elementwise tile size");
  auto one = [&](int64_t i) {
    double v;
    if (i < ncopy) v = S::widen(S::ldraw(flat + lo + i));
    else if (i == ncopy) v = 1.0;
    else v = 0.0;
    if constexpr (MODE == 1) {
      const double a = __builtin_bit_cast(double, dst[i]);
      dst[i] = __builtin_bit_cast(unsigned long long, a + v);
    } else if constexpr (MODE == 2) {
      dst[i] = __builtin_bit_cast(unsigned long long, 0.0 + v);
    } else {
      dst[i] = BE_OUT ? f64_to_be(v) : __builtin_bit_cast(unsigned long long, v);
    }
  };
  if constexpr (VEC) {
    const int64_t base = (int64_t)blockIdx.x * kEwTile;
    if (base + kEwTile <= ncopy) {
      const typename S::elem* src = flat + lo;
      typename S::template Vec<EV> sv[NV];
      u2 dv[NV][EV / 2];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t i = base + EV * ((int64_t)k * kBlock + threadIdx.x);
        sv[k] = S::template ldv<EV>(src + i);
        if constexpr (MODE == 1) {
#pragma unroll
          for (int c = 0; c < EV / 2; ++c) dv[k][c] = *(gcu2)(dst + i + 2 * c);
        }
      }
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int64_t i = base + EV * ((int64_t)k * kBlock + threadIdx.x);
#pragma unroll
        for (int c = 0; c < EV / 2; ++c) {
          const d2 x = d2{S::template get<EV>(sv[k], 2 * c), S::template get<EV>(sv[k], 2 * c + 1)};
          d2 o;
          if constexpr (MODE == 1) {
            const d2 a = __builtin_bit_cast(d2, dv[k][c]);
            o = d2{a.x + x.x, a.y + x.y};
          } else if constexpr (MODE == 2) {
            o = d2{0.0 + x.x, 0.0 + x.y};
          } else {
            o = x;
          }
          *(gu2)(dst + i + 2 * c) = encode2<BE_OUT>(o);
        }
      }
      return;
    }
    const int64_t end = base + kEwTile < L ? base + kEwTile : L;
    for (int64_t i = base + threadIdx.x; i < end; i += kBlock) one(i);
  } else {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < L) one(i);
  }
}

// k_load_model over a model of a narrow format (InitializeWeights from model.params()).
template <class S>
__global__ __launch_bounds__(kBlock) void k_load_model_narrow(const typename S::elem* __restrict__ flat, int64_t lo,
                                                              int64_t ncopy, int64_t L, double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= L) return;
  dst[i] = (i < ncopy) ? S::widen(S::ldraw(flat + lo + i)) : 0.0;
}

// ---------------------------------------------------------------------------
// k_divide_narrow: the GetPartitions divide (k_divide) narrowed to a format:
//   out[m] = narrow((float)(cnt == 0.0 ? W[p][j] : W[p][j] / den))
// The quotient is k_divide's IEEE double division; it is rounded once to
// float (ties to even; overflow to +-inf, subnormals kept, -0.0 stays -0.0),
// and for a 16-bit format that float is rounded to the format (the two-step
// rule above).  Never a division in the narrow format, never a reciprocal.
// Tiles of kDivTile values are laid over the OUTPUT as in k_divide: block 0
// writes the `head` values up to the first 128-B line of this partition's
// output (p*chunk elements is arbitrary mod a line), then every lane stores
// 16 B = 16 / sizeof(elem) values and a wave whole lines (64 x 16 B = 8
// lines); W is read with 8-B loads (its alignment against the output is
// arbitrary).
// ---------------------------------------------------------------------------
template <class S, bool SECURE>
__global__ __launch_bounds__(kBlock) void k_divide_narrow(const DivDesc* __restrict__ parts,
                                                          const double* __restrict__ arena,
                                                          typename S::elem* __restrict__ out, int tiles_per_part) {
  typedef typename S::elem T;
  constexpr int EV = 16 / sizeof(T);                   // values per store
  constexpr int PW = 4 / sizeof(T);                    // values per 32-bit word
  constexpr int V = kDivTile / ((int64_t)kBlock * EV); // stores per lane
  constexpr int LINE = 128 / sizeof(T);                // values per 128-B line
  // kDivTile is the f64 divide's tile, tuned for k_divide (kDivV).  The shape below (V stores per lane) was
  // measured at 2048 values: a retuned kDivV must not change it unnoticed.
  static_assert(kDivTile == 2048, "the narrow divide's tile is 2048 values");
  static_assert((int64_t)kBlock * EV * V == kDivTile, "one divide tile size for every element size");
  static_assert(kBlock % 64 == 0, "whole waves");
  const int q = blockIdx.x / tiles_per_part;
  const int t = blockIdx.x - q * tiles_per_part;
  const DivDesc d = parts[q];
  const int64_t n = d.len - 1;
  const double* w = arena + d.w_off;
  const double cnt = w[d.len - 1];
  const double den = SECURE ? 1e12 * cnt : cnt;   // IPLS.java:1167
  auto f = [&](double x) -> unsigned { return S::narrow((float)((cnt == 0.0) ? x : x / den)); };
  T* o = out + d.out_off;
  const int64_t to_line = (LINE - (int64_t)(((uintptr_t)o / sizeof(T)) & (LINE - 1))) & (LINE - 1);
  const int64_t head = to_line < n ? to_line : n;
  if (t == 0 && threadIdx.x < head) S::put(o + threadIdx.x, f(w[threadIdx.x]));
  const int64_t base = (int64_t)t * kDivTile + head;
  if (base >= n) return;
  if (base + kDivTile <= n) {
    // wave (threadIdx.x / 64) owns [base + wave * 64 * EV * V, + 64 * EV * V)
    const int64_t wave_base = base + (int64_t)(threadIdx.x >> 6) * 64 * EV * V + EV * (threadIdx.x & 63);
    double x[V][EV];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int64_t i = wave_base + (int64_t)v * 64 * EV;
#pragma unroll
      for (int c = 0; c < EV; ++c)
        x[v][c] = __builtin_nontemporal_load((const IPLS_GLOBAL double*)(w + i + c));
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int64_t i = wave_base + (int64_t)v * 64 * EV;
      // The four words are spelled out: with a loop over them inside this one, which has a single
      // trip for 16-bit elements, hipcc hoists the store out of it and drops its non-temporal hint
      // (seen in the assembly; GetPartitions to bfloat16 then ran a few per cent slower, runs not kept).
      const double* xv = x[v];
      u4w y;
      if constexpr (PW == 2)
        y = u4w{f(xv[0]) | (f(xv[1]) << 16), f(xv[2]) | (f(xv[3]) << 16), f(xv[4]) | (f(xv[5]) << 16),
                f(xv[6]) | (f(xv[7]) << 16)};
      else
        y = u4w{f(xv[0]), f(xv[1]), f(xv[2]), f(xv[3])};
      __builtin_nontemporal_store(y, (IPLS_GLOBAL u4w*)(o + i));
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < n; i += kBlock) S::put(o + i, f(w[i]));
}

// ---------------------------------------------------------------------------
// k_round_narrow: the fused round (k_round) for the trainer formats -- buckets
// of format S in, W as native doubles and the averages in format A out, in one
// pass: AGG is never stored.  The body is k_reduce_narrow's VEC path (E = 4
// elements per lane per vector, one non-temporal load per peer per vector, PF:
// the next peer's loads issued before this peer's adds), followed by
// reduce_tiles<FIN>'s epilogue restated for four f64 accumulators per vector.
// Per element e holding the fold value a:
//   w      = a + (rep ? REP[e] : 0.0)          AggregatePartition (IPLS.java:1256); the + 0.0 is kept
//   W[e]   = w                                 native doubles, the lane ^ 4 swap of k_reduce_narrow
//   avg[e] = A::narrow((float)(cnt == 0.0 ? w : w / den))   for e < L - 1: k_divide_narrow's expression
// (an IEEE double division, one rounding to float, then the format's own).
// The host guarantees 16-B aligned buckets; AGG, REP and W are arena slots.
// Averages: partition p's start at an arbitrary element of the output.  With
// m = (address of parts[q].avg / sizeof(A::elem)) mod 4, uniform per block:
//   m == 0: a lane stores its own four values (16 B of floats, 8 B of 16-bit);
//   m != 0: a lane stores the aligned group made of its own last m values and
//           lane t+1's first 4 - m (__shfl_down, as k_round does at 8 mod 16);
//           the wave's first 4 - m and last m values go element by element.
// Either way one store instruction of a wave writes one contiguous run (1 KiB
// of floats, 512 B of 16-bit values) of which only the two ends share a line.
// The last element of a full tile may be the count slot L - 1 (L a multiple of
// the tile): it gets W but no average.  The partial last tile goes through
// k_reduce_narrow's 4*BS-element vector steps and scalar remainder, every
// element finishing through fin1.
//   map : 0 partition-major, 3 partial tiles first (map_block); a runtime
//         argument: 3 x 3 x 2 instantiations instead of 36.
// ---------------------------------------------------------------------------
template <class A>
__device__ __forceinline__ void st_avg1(typename A::elem* p, unsigned b) {   // one average, as a global store
  if constexpr (sizeof(typename A::elem) == 4) *(IPLS_GLOBAL unsigned*)p = b;
  else *(IPLS_GLOBAL unsigned short*)p = (unsigned short)b;
}
template <class A>
__device__ __forceinline__ void st_avg4(typename A::elem* p, unsigned g0, unsigned g1, unsigned g2, unsigned g3) {
  if constexpr (sizeof(typename A::elem) == 4) {
    __builtin_nontemporal_store(u4w{g0, g1, g2, g3}, (IPLS_GLOBAL u4w*)p);
  } else {
    typedef unsigned u2w __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(u2w{g0 | (g1 << 16), g2 | (g3 << 16)}, (IPLS_GLOBAL u2w*)p);
  }
}

template <class S, class A, int START, int R, int BS, int PF>
__global__ __launch_bounds__(BS) void k_round_narrow(const typename S::elem* const* __restrict__ bufs,
                                                     const PartDesc* __restrict__ parts, int k, int tiles_per_part,
                                                     int n_parts, int map, int secure,
                                                     const double* __restrict__ cnts) {
  typedef typename S::elem T;
  typedef typename A::elem O;
  constexpr int E = 4;
  static_assert(START == kZero || START == kAccum, "AGG is never FIRST-started");
  auto ldu = [](const T* p) { return S::unpack(S::template ldv<E>(p)); };
  typedef decltype(ldu((const T*)nullptr)) V;
  constexpr int64_t kTile = (int64_t)BS * E * R;
  constexpr int kPB = 8;
  constexpr int kPBV = S::template kPeersVec<E>;
  int q, t;
  map_block(map, gridDim.x, tiles_per_part, n_parts, q, t);
  if (q >= n_parts) return;
  const int64_t L = parts[q].len;
  const int64_t base = (int64_t)t * kTile;
  if (base >= L) return;
  unsigned long long* __restrict__ dst = parts[q].dst;           // W
  const unsigned long long* __restrict__ agg = parts[q].init;    // ACCUM source
  const unsigned long long* __restrict__ rep = parts[q].rep;
  O* __restrict__ avg = (O*)parts[q].avg;
  const T* const* __restrict__ pb = bufs + (size_t)q * k;
  const int tid = threadIdx.x;
  // count slot W[L-1] (k_round_counts_narrow folded it exactly as element L-1 is)
  double den = 0.0, cnt = 0.0;
  if (avg) {
    cnt = cnts[q];
    den = secure ? 1e12 * cnt : cnt;   // Math.pow(10,12) * W[last] (IPLS.java:1167)
  }
  auto add = [](double (&a)[E], const V& v) {
#pragma unroll
    for (int c = 0; c < E; ++c) a[c] = a[c] + S::template get<E>(v, c);
  };
  auto init = [&](double (&a)[E], int64_t o) {
    if constexpr (START == kZero) {
#pragma unroll
      for (int c = 0; c < E; ++c) a[c] = 0.0;
    } else {
#pragma unroll
      for (int c = 0; c < E / 2; ++c) {
        const d2 x = decode2<false>(ld16<false>(agg + o + 2 * c));
        a[2 * c] = x.x, a[2 * c + 1] = x.y;
      }
    }
  };
  auto quot = [&](double w) -> unsigned { return A::narrow((float)(cnt == 0.0 ? w : w / den)); };
  // fused epilogue for element e holding fold value a, element by element
  auto fin1 = [&](int64_t e, double a) {
    const double w = a + (rep ? __builtin_bit_cast(double, ld8(rep + e)) : 0.0);
    st8(dst + e, __builtin_bit_cast(unsigned long long, w));
    if (avg && e < L - 1) st_avg1<A>(avg + e, quot(w));
  };

  if (base + kTile <= L) {
    const int64_t o0 = base + E * (int64_t)tid;
    double acc[R][E];
#pragma unroll
    for (int r = 0; r < R; ++r) init(acc[r], o0 + (int64_t)r * BS * E);
    if constexpr (PF) {
      V v[R];
      if (0 < k) {
        const T* __restrict__ src = pb[0] + o0;
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = ldu(src + (int64_t)r * BS * E);
      }
      for (int j = 0; j < k; ++j) {
        V nx[R];
        if (j + 1 < k) {
          const T* __restrict__ src = pb[j + 1] + o0;
#pragma unroll
          for (int r = 0; r < R; ++r) nx[r] = ldu(src + (int64_t)r * BS * E);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) add(acc[r], v[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = nx[r];
      }
    } else {
      for (int j = 0; j < k; ++j) {
        const T* __restrict__ src = pb[j] + o0;
        V v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = ldu(src + (int64_t)r * BS * E);
#pragma unroll
        for (int r = 0; r < R; ++r) add(acc[r], v[r]);
      }
    }
    // W = fold + REP, and the averages' R stores before W's (as in k_round)
    const int m = (int)(((uintptr_t)avg / sizeof(O)) & 3);
    const int lane = tid & 63;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t o = o0 + (int64_t)r * BS * E;
      if (rep) {
#pragma unroll
        for (int c = 0; c < E / 2; ++c) {
          const d2 y = decode2<false>(ld16<true>(rep + o + 2 * c));
          acc[r][2 * c] = acc[r][2 * c] + y.x;
          acc[r][2 * c + 1] = acc[r][2 * c + 1] + y.y;
        }
      } else {
#pragma unroll
        for (int c = 0; c < E; ++c) acc[r][c] = acc[r][c] + 0.0;   // AGG + REP with REP == +0.0
      }
      if (avg) {
        const unsigned y0 = quot(acc[r][0]), y1 = quot(acc[r][1]), y2 = quot(acc[r][2]), y3 = quot(acc[r][3]);
        if (m == 0) {
          // element o + 3 may be the count slot L-1, which is not output
          if (o + 3 < L - 1) {
            st_avg4<A>(avg + o, y0, y1, y2, y3);
          } else {
            st_avg1<A>(avg + o, y0);
            st_avg1<A>(avg + o + 1, y1);
            st_avg1<A>(avg + o + 2, y2);
          }
        } else {
          // avg + o is m elements past a 16-B (floats) / 8-B (16-bit) boundary: lane t writes the aligned
          // group (o + 4 - m .. o + 7 - m) = its own last m values and lane t+1's first 4 - m
          const unsigned n0 = __shfl_down(y0, 1), n1 = __shfl_down(y1, 1), n2 = __shfl_down(y2, 1);
          unsigned g0, g1, g2, g3;
          if (m == 1) g0 = y3, g1 = n0, g2 = n1, g3 = n2;
          else if (m == 2) g0 = y2, g1 = y3, g2 = n0, g3 = n1;
          else g0 = y1, g1 = y2, g2 = y3, g3 = n0;
          if (lane < 63) {
            st_avg4<A>(avg + o + 4 - m, g0, g1, g2, g3);
          } else {
            // the wave's last m values (the very last may be the count slot L-1)
            if (m >= 3) st_avg1<A>(avg + o + 1, y1);
            if (m >= 2) st_avg1<A>(avg + o + 2, y2);
            if (o + 3 < L - 1) st_avg1<A>(avg + o + 3, y3);
          }
          if (lane == 0) {   // the wave's first 4 - m values
            st_avg1<A>(avg + o, y0);
            if (m <= 2) st_avg1<A>(avg + o + 1, y1);
            if (m <= 1) st_avg1<A>(avg + o + 2, y2);
          }
        }
      }
    }
    // W: the 8 lanes that own two adjacent 128-B lines swap their upper pair
    // of sums with lane ^ 4, so each store instruction writes whole lines
    // (k_reduce_narrow's E == 4 stores)
    const bool hi = tid & 4;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t o = o0 + (int64_t)r * BS * 4;
      const d2 own = d2{acc[r][0], acc[r][1]};
      const d2 got = d2{__shfl_xor(acc[r][2], 4), __shfl_xor(acc[r][3], 4)};   // elements o ^ 16 .. + 2, + 3
      __builtin_nontemporal_store(encode2<false>(hi ? got : own), (gu2)(dst + (hi ? o - 14 : o)));
      __builtin_nontemporal_store(encode2<false>(hi ? own : got), (gu2)(dst + (hi ? o : o + 18)));
    }
    return;
  }
  // ------- partial last tile: 4*BS-element vector steps, scalar remainder -------
  const int64_t end = base + kTile < L ? base + kTile : L;
  int64_t sb = base;
  for (; sb + E * BS <= end; sb += E * BS) {
    const int64_t o = sb + E * (int64_t)tid;
    double a[E];
    init(a, o);
    int jj = 0;
    for (; jj + kPBV <= k; jj += kPBV) {
      V v[kPBV];
#pragma unroll
      for (int g = 0; g < kPBV; ++g) v[g] = ldu(pb[jj + g] + o);
#pragma unroll
      for (int g = 0; g < kPBV; ++g) add(a, v[g]);
    }
    for (; jj < k; ++jj) add(a, ldu(pb[jj] + o));
#pragma unroll
    for (int c = 0; c < E; ++c) fin1(o + c, a[c]);
  }
  for (int64_t e = sb + tid; e < end; e += BS) {
    double acc;
    if constexpr (START == kZero) acc = 0.0;
    else acc = decode1<false>(ld8(agg + e));
    int jj = 0;
    for (; jj + kPB <= k; jj += kPB) {
      typename S::raw v[kPB];
#pragma unroll
      for (int g = 0; g < kPB; ++g) v[g] = S::ldraw(pb[jj + g] + e);
#pragma unroll
      for (int g = 0; g < kPB; ++g) acc = acc + S::widen(v[g]);
    }
    for (; jj < k; ++jj) acc = acc + S::widen(S::ldraw(pb[jj] + e));
    fin1(e, acc);
  }
}

// Count slot of a fused narrow round, one wave per partition: k_round_counts
// with the format's widening load --
// cnt = ((init[L-1] | +0.0) + b_0[L-1] + ... + b_{k-1}[L-1]) + (REP[L-1] | +0.0),
// the identical expression in the identical order, so the bits element L-1 of
// the round gets.
template <class S, int START>
__global__ __launch_bounds__(64) void k_round_counts_narrow(const typename S::elem* const* __restrict__ bufs,
                                                            const PartDesc* __restrict__ parts, int k, int n_parts,
                                                            double* __restrict__ cnts) {
  const int q = blockIdx.x;
  if (q >= n_parts) return;
  const int lane = threadIdx.x;
  const PartDesc d = parts[q];
  const int64_t e = d.len - 1;
  const typename S::elem* const* pb = bufs + (size_t)q * k;
  double c = (START == kZero) ? 0.0 : __builtin_bit_cast(double, ld8(d.init + e));
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int j = j0 + lane;
    const double v = j < k ? S::widen(S::ldraw(pb[j] + e)) : 0.0;
    const int m = k - j0 < 64 ? k - j0 : 64;
    for (int t = 0; t < m; ++t) c = c + __shfl(v, t);
  }
  if (lane == 0) cnts[q] = c + (d.rep ? __builtin_bit_cast(double, ld8(d.rep + e)) : 0.0);
}

// ---------------------------------------------------------------------------
// k_update_flat: UpdateGradient's own accumulate (IPLS.java:1737-1743, k_split
// MODE 1 / 2) over ALL owned partitions of a shard in one launch, from one
// staged flat vector (ipls_agg_update_gradient_chunked).  blockIdx.y is the
// job, blockIdx.x the tile of its partition:
//   dst[i] = (zero ? +0.0 : dst[i]) + v,   v = (double)src[lo + i] for
//   i < ncopy, 1.0 at i == ncopy (the count slot, generated here), 0.0 above
//   (the add is still made: a -0.0 accumulator element becomes +0.0).
// Tiling is aligned to the DESTINATION (accumulators are 256-B aligned): a
// lane owns G consecutive elements at an aligned dst index -- 2 doubles (S =
// FmtD64) or 4 elements (trainer formats) -- R = kFlatR groups kBlock groups
// apart, so a tile is kBlock * G * R elements; all loads first, then the adds,
// then 16-B stores (trainer formats through k_fold1_narrow's lane ^ 4
// exchange, so a store instruction writes whole 128-B lines).
// The source is only element-aligned: `src` (a kernel argument, 16-B aligned)
// plus lo elements, and m = lo mod G is the job's residue against the lane's
// load (16 B of doubles or floats, 8 B of 16-bit elements), uniform per job.
//   m == 0: aligned vector loads, as k_split<VEC> / k_fold1_narrow.
//   m != 0, SHIFT: the aligned vector load that holds the group's first
//     element (it starts m elements early), completed with the first m
//     elements of lane t + 1's load by __shfl_down; the wave's last lane loads
//     its next vector itself.  The loads of a tile touch up to G - 1 elements
//     before lo and after lo + ncopy: the stage is padded by 16 B at both
//     ends, and between partitions those are the neighbour's bytes; they are
//     loaded and never used.
//   m != 0, !SHIFT: G naturally aligned element loads per group.
// SHIFT defaults to the form that measured faster for the element width.
// Tiles wholly inside [0, ncopy) take that body; the tile that holds ncopy and
// everything after it go element by element.  The zero flag is a per-job
// uniform branch.  BE_IN (doubles only): big-endian bytes, bswap in registers.
// ---------------------------------------------------------------------------
struct FlatJob {
  int64_t lo;                 // first source element of the partition, from `src`
  int64_t ncopy, L;
  unsigned long long* dst;    // the accumulator (256-B aligned)
  int64_t zero;               // logically +0.0: written without being read
};
struct FmtD64 {               // doubles as 64-bit words (native or big-endian)
  typedef unsigned long long elem;
};
// Which form a non-zero residue takes, per element width, as measured
// (tools/update_flat_sweep.hip): doubles are faster shifted,
// the trainer formats with element loads.  Both forms are instantiated by the
// sweep tool, which also compares their bits.
#ifndef IPLS_FLAT_SHIFT
#define IPLS_FLAT_SHIFT 1          // doubles: 1 shifted aligned loads, 0 element loads
#endif
#ifndef IPLS_FLAT_SHIFT_NARROW
#define IPLS_FLAT_SHIFT_NARROW 0   // f32 / f16 / bf16: the same choice
#endif
constexpr int kFlatR = 4;
template <class S>
constexpr int64_t flat_tile() { return (int64_t)kBlock * (sizeof(typename S::elem) == 8 ? 2 : 4) * kFlatR; }
template <class S>
constexpr bool flat_shift() { return sizeof(typename S::elem) == 8 ? IPLS_FLAT_SHIFT != 0 : IPLS_FLAT_SHIFT_NARROW != 0; }

template <class S, bool BE_IN, bool SHIFT = flat_shift<S>()>
__global__ __launch_bounds__(kBlock) void k_update_flat(const FlatJob* __restrict__ jobs,
                                                        const typename S::elem* __restrict__ src0) {
  typedef typename S::elem T;
  constexpr bool kWide = sizeof(T) == 8;
  static_assert(kWide || !BE_IN, "only doubles come big-endian");
  constexpr int R = kFlatR;
  constexpr int64_t tile = flat_tile<S>();
  const FlatJob j = jobs[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.x * tile;
  if (base >= j.L) return;
  const T* src = src0 + j.lo;
  unsigned long long* dst = j.dst;
  const bool zero = j.zero != 0;
  const int tid = threadIdx.x;
  const bool last = (tid & 63) == 63;   // no lane t + 1 in the wave
  if (base + tile <= j.ncopy) {
    // MODE 0: aligned loads; 1: shifted aligned loads; 2: element loads.  One body per mode, chosen by the
    // job-uniform residue outside the loops, so each holds only its own registers.
    if constexpr (kWide) {
      auto body = [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        u2 sv[R], dv[R];
        unsigned long long ex[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t i = base + 2 * ((int64_t)r * kBlock + tid);
          ex[r] = 0;
          if constexpr (MODE == 0) {
            sv[r] = __builtin_nontemporal_load((gcu2)(src + i));
          } else if constexpr (MODE == 1) {
            sv[r] = __builtin_nontemporal_load((gcu2)(src + i - 1));   // elements i - 1, i
            if (last) ex[r] = ld8(src + i + 1);
          } else {
            sv[r].x = ld8(src + i);
            sv[r].y = ld8(src + i + 1);
          }
          if (!zero) dv[r] = *(gcu2)(dst + i);
          else dv[r] = u2{0, 0};
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t i = base + 2 * ((int64_t)r * kBlock + tid);
          u2 raw = sv[r];
          if constexpr (MODE == 1) {
            const unsigned long long own = sv[r].x, up = sv[r].y;
            const unsigned long long nx = __shfl_down(own, 1);   // lane t + 1's element i + 1
            raw.x = up;
            raw.y = last ? ex[r] : nx;
          }
          const d2 x = decode2<BE_IN>(raw);
          const d2 a = __builtin_bit_cast(d2, dv[r]);   // +0.0 when the accumulator is logically zero
          *(gu2)(dst + i) = encode2<false>(d2{a.x + x.x, a.y + x.y});
        }
      };
      if ((j.lo & 1) == 0) body(std::integral_constant<int, 0>{});
      else body(std::integral_constant<int, SHIFT ? 1 : 2>{});
    } else {
      const int m = (int)(j.lo & 3);
      typedef typename S::template Vec<4> V;
      constexpr bool kF32 = sizeof(T) == 4;
      auto body = [&](auto mode) {
        constexpr int MODE = decltype(mode)::value;
        V sv[R], nv[R];
        typename S::raw el[R][4];
        u2 t[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t i = base + 4 * ((int64_t)r * kBlock + tid);
          if constexpr (MODE == 0) {
            sv[r] = S::template ldv<4>(src + i);
          } else if constexpr (MODE == 1) {
            sv[r] = S::template ldv<4>(src + i - m);                  // elements i - m .. i - m + 3
            nv[r] = sv[r];
            if (last) nv[r] = S::template ldv<4>(src + i - m + 4);
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) el[r][c] = S::ldraw(src + i + c);
          }
          if (!zero) {
            t[r][0] = ld16<false>(dst + i);
            t[r][1] = ld16<false>(dst + i + 2);
          } else {
            t[r][0] = t[r][1] = u2{0, 0};
          }
        }
        const bool hi = tid & 4;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          double v[4];
          if constexpr (MODE == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = S::template get<4>(sv[r], c);
          } else if constexpr (MODE == 1) {
            if constexpr (kF32) {
              const float o0 = sv[r].x, o1 = sv[r].y, o2 = sv[r].z, o3 = sv[r].w;
              float n0 = __shfl_down(o0, 1), n1 = __shfl_down(o1, 1), n2 = __shfl_down(o2, 1);
              if (last) n0 = nv[r].x, n1 = nv[r].y, n2 = nv[r].z;
              const float s0 = m == 1 ? o1 : m == 2 ? o2 : o3;
              const float s1 = m == 1 ? o2 : m == 2 ? o3 : n0;
              const float s2 = m == 1 ? o3 : m == 2 ? n0 : n1;
              const float s3 = m == 1 ? n0 : m == 2 ? n1 : n2;
              v[0] = (double)s0, v[1] = (double)s1, v[2] = (double)s2, v[3] = (double)s3;
            } else {
              const unsigned long long own = ((unsigned long long)sv[r].w[1] << 32) | sv[r].w[0];
              unsigned long long nx = __shfl_down(own, 1);
              if (last) nx = ((unsigned long long)nv[r].w[1] << 32) | nv[r].w[0];
              const unsigned long long sh = (own >> (16 * m)) | (nx << (64 - 16 * m));   // m in 1..3
              V s;
              s.w[0] = (unsigned)sh, s.w[1] = (unsigned)(sh >> 32);
#pragma unroll
              for (int c = 0; c < 4; ++c) v[c] = S::template get<4>(s, c);
            }
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = S::widen(el[r][c]);
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
      if (m == 0) body(std::integral_constant<int, 0>{});
      else body(std::integral_constant<int, SHIFT ? 1 : 2>{});
    }
    return;
  }
  const int64_t end = base + tile < j.L ? base + tile : j.L;
  for (int64_t i = base + tid; i < end; i += kBlock) {
    double v;
    if (i < j.ncopy) {
      if constexpr (kWide) v = decode1<BE_IN>(ld8(src + i));
      else v = S::widen(S::ldraw(src + i));
    } else {
      v = i == j.ncopy ? 1.0 : 0.0;
    }
    const double a = zero ? 0.0 : __builtin_bit_cast(double, ld8(dst + i));
    st8(dst + i, __builtin_bit_cast(unsigned long long, a + v));
  }
}

// ---------------------------------------------------------------------------
// k_b64url_encode_flat: SendGradients (IPLS.java:1350-1400) -- the pubsub
// texts of a flat gradient's partitions, one launch over a shard's listed
// partitions (blockIdx.y = job, as in k_b64url_encode_frames).  Text =
// Base64.getUrlEncoder(Marshall_Packet(OrganizeGradients(flat)[p], ...)), the
// frame [14 header bytes][L x f64 BE][origin], whose payload value i is
//   (double)src[lo + i]  i < ncopy   widened as the F32 / F16 / BF16 kinds
//                                    are (doubles pass bit for bit; BE_IN
//                                    byte-swaps in registers)
//   1.0                  i == ncopy  the count slot, generated here
//                                    (IPLS.java:1033)
//   +0.0                 ncopy < i < L   a gradient shorter than the model
// Nothing is added to anything: putDouble writes raw bits, so a -0.0 value is
// -0.0 in the text.  The decomposition is k_b64url_encode_frame's: lane g owns
// frame bytes [24g, 24g + 24); it is fast when g >= 1 and its four values
// 3g-2 .. 3g+1 all lie below ncopy, and then loads its four source elements
// at lo + 3g - 2 one by one (the source is only element-aligned: lo has any
// residue) and goes through window_chars; every other lane (the header, the
// window that holds ncopy, the zero tail, the origin) goes byte by byte.
// ---------------------------------------------------------------------------
struct FlatEncJob {
  unsigned char hdr[16];          // 14 header bytes
  int64_t L;                      // doubles in the payload
  int64_t ncopy;                  // of which copied from the source
  int64_t lo;                     // the partition's first element, from `src`
  int64_t origin_len;
  const unsigned char* origin;    // device copy of the origin bytes
  unsigned char* out;
  int64_t groups;
  int64_t text_len;
};

// Payload value `p[0]` as the number its big-endian bytes spell.
template <class S, bool BE_IN>
__device__ __forceinline__ unsigned long long flat_value_bits(const typename S::elem* p) {
  if constexpr (sizeof(typename S::elem) == 8) {
    const unsigned long long v = ld8(p);
    return BE_IN ? __builtin_bswap64(v) : v;
  } else {
    return __builtin_bit_cast(unsigned long long, S::widen(S::ldraw(p)));
  }
}

template <class S, bool BE_IN>
__global__ __launch_bounds__(kBlock) void k_b64url_encode_flat(const FlatEncJob* __restrict__ jobs,
                                                               const typename S::elem* __restrict__ src0) {
  typedef typename S::elem T;
  static_assert(sizeof(T) == 8 || !BE_IN, "only doubles come big-endian");
  __shared__ u4w stage[2 * kBlock];
  __shared__ unsigned char tab[64];
  init_b64url_table(tab);
  const FlatEncJob& j = jobs[blockIdx.y];
  const T* src = src0 + j.lo;
  const int64_t L = j.L, ncopy = j.ncopy, groups = j.groups;
  const int64_t F = 14 + 8 * L + j.origin_len;   // frame bytes
  auto frame_byte_at = [&](int64_t b) -> unsigned {
    if (b < 14) return j.hdr[b];
    const int64_t q = b - 14;
    if (q >= 8 * L) return j.origin[q - 8 * L];
    const int64_t i = q >> 3;
    const unsigned long long v = i < ncopy ? flat_value_bits<S, BE_IN>(src + i) : i == ncopy ? 0x3FF0000000000000ull : 0ull;
    return (unsigned)(v >> (8 * (7 - (q & 7)))) & 0xFF;   // putDouble: big-endian
  };
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u4w* ws = stage + 128 * wv;
  for (int64_t g0 = (int64_t)blockIdx.x * kBlock; g0 < groups; g0 += (int64_t)gridDim.x * kBlock) {
    const int64_t gw = g0 + 64 * wv;                // this wave's first group
    const int64_t g = gw + lane;
    u4w c0 = {0u, 0u, 0u, 0u}, c1 = {0u, 0u, 0u, 0u};
    if (g < groups && g >= 1 && 3 * g + 2 <= ncopy) {
      const T* s = src + (3 * g - 2);
      const unsigned long long v0 = flat_value_bits<S, BE_IN>(s), v1 = flat_value_bits<S, BE_IN>(s + 1);
      const unsigned long long v2 = flat_value_bits<S, BE_IN>(s + 2), v3 = flat_value_bits<S, BE_IN>(s + 3);
      window_chars(v0, v1, v2, v3, tab, c0, c1);
    } else if (g < groups) {
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
