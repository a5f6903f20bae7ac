// reduce_plan.hpp -- the host-side plan of a fold launch: the shape, tile, block
// order and grid of a batch of n_parts partitions of at most maxL elements.
// engine.hip launches from it and fills the launch record from it; a launch's
// template arguments and the plan's numbers come from the same constexpr
// functions.  Plain C++ with no HIP type in it, so the stand-alone program
// tests/cpp/test_reduce_plan.cpp checks it on the CPU.
#pragma once

#include <stdint.h>

#include "../../include/ipls_agg.h"

namespace ipls::reduceplan {

// The fields of ipls_launch_info (r is its `vectors`; the narrow plans report
// `vec` in seqf and no shape), the tile in elements, tiles per partition, blocks.
struct ReducePlan {
  int kernel, shape, block, r, seqf, map;
  int64_t tile, tpp, grid;
};

// ---- kernel dispatch: k_reduce ----
// Three shapes (tools/reduce_sweep.hip, profiles/r01/sweep*.txt), the first
// whose tiles fill the 256 CUs (fill()):
//  * big: 1024-lane workgroups, 1 peer in flight x 16 x 16 B per lane, i.e.
//    each CU streams one 256 KiB contiguous chunk of one bucket at a time
//    (fewer, longer DRAM streams): 85-89 % of 8 TB/s on config C over every
//    bucket layout tried, vs 80-86 % for 256-lane / 64 KiB blocks;
//  * mid: the same per-lane work on 256-lane workgroups (64 KiB chunks), for
//    batches of one or a few partitions: 1 x 4M x 32 at 86.2 % vs 72.7 % for
//    the small shape and 55.8 % for the big one on 128 CUs
//    (profiles/r01/sweep_few_partitions.txt);
//  * small: 256 lanes, 8 peers in flight x 16 B per lane, partition-major --
//    enough blocks for short partitions (ETHModel's 3 x 147,872).
constexpr int kBigG = 1, kBigMap = 0, kBigBS = 1024, kMidBS = 256;
constexpr int kSmallG = 8, kSmallR = 1, kSmallMap = 0, kSmallBS = 256;
// A tile count fills the chip when it is at least two waves of 256 CUs, or
// one or more waves with at most a fifth of the last one idle.
inline bool fill(int64_t tiles) {
  if (tiles >= 512) return true;
  if (tiles < 256) return false;
  const int64_t waves = (tiles + 255) / 256;
  return tiles * 5 >= waves * 256 * 4;
}
// 16 x 16 B per lane in the 128-VGPR budget of a 1024-lane workgroup:
// native doubles 126 VGPRs; big-endian input 110 with the SEQ schedule of
// reduce_tiles (hipcc's own schedule hoisted the loads around the bswap and
// spilled 184 B).  The ACCUM start keeps 8 (at 16 it still spills around
// the loop -- checked with -Rpass-analysis=kernel-resource-usage).
// IPLS_BE_BIG_R / IPLS_BE_SEQF rebuild the big-endian big shape with another
// schedule for same-process A/B runs (make -C ipls-java-api_amd variants,
// bench.py --be-schedule-ab); the shipped library uses the defaults.
#ifndef IPLS_BE_BIG_R
#define IPLS_BE_BIG_R 16
#endif
#ifndef IPLS_BE_SEQF
#define IPLS_BE_SEQF 3
#endif
constexpr int big_r(bool be_in, int start) { return start != IPLS_START_ACCUM ? (be_in ? IPLS_BE_BIG_R : 16) : 8; }
// SEQ schedule of the big shape (0 = hipcc's own): big-endian input at R = 16
// loads, decodes and adds a peer's vectors three at a time with a fence after
// each group (SEQF = 3; 118 VGPRs, no spills).  Round 2 swept fence periods
// 1-8 with and without a free tail in one process (profiles/r02/s3/
// sweep_be_tail{1,2}*.txt): 3 beats round 1's every-2-with-the-last-4-free
// (SEQF = 42) by 0.7-1.6 points on C's and D's shapes, BE in and in + out;
// periods >= 5, a free tail on period 3, and period 1 are all slower.
constexpr int big_seqf(bool be_in, int start) { return (be_in && big_r(be_in, start) > 8) ? IPLS_BE_SEQF : 0; }
// Block order of the big shape over whole tiles: partition-major (map 0),
// except big-endian input on grids of at most 4096 tiles, which runs
// XCD-chunked (map 2: each XCD walks one contiguous eighth of the work).  With
// SEQF = 3, map 2 measured +2 to +3.6 points at 2-4 partitions of 4M x 32,
// +0.2 to +0.6 at 16, and -3.6 at 64 (config D, 8192 tiles); native doubles
// gain nothing from it at 16 (profiles/r02/s3/sweep_be_map.txt,
// sweep_map_fewp.txt) and run the half shape below on short grids.
inline int big_map(bool be_in, int64_t tiles) { return (be_in && tiles <= 4096) ? 2 : kBigMap; }
// The half shape (round 3): ZERO/FIRST start, batches of fewer than 4
// rounds of big tiles on 256 CUs (fewer than 1024 whole big tiles: one to
// seven partitions of 4M, config B), and larger grids that the big tiles
// would leave partly idle in their last round (below).  512-lane workgroups at R = 16 -- 128
// KiB of a bucket per block, one workgroup per CU, no spills, every load of a
// peer's chunk in flight: native doubles at 164 VGPRs, big-endian input on
// hipcc's own schedule at 172 (the 256-VGPR budget of 512 lanes needs no SEQ
// fences).  Same process, same buckets (profiles/r03/e/sweep_fewp.txt,
// r03/f/sweep_512_*.txt, r03/h/sweep_fewp_be.txt): native 1/2/3/5/7
// partitions of 4M x 32 at 87.1/83.2/89.8/89.5/89.1 % against 56.2/80.5/
// 74.9/80.7/82.7 % for the big shape (whose 128 tiles per partition leave
// half a round idle at odd counts) and 87.4/70.1/85.2/78.5/81.0 % for mid;
// big-endian in + out 88.2/87.8/87.0/86.0/85.0 % against 84.3 (mid)/82.7/
// 84.5 (mid)/79.6/82.9 % for what shipped; config B 80.2-82.3 % against
// 78.7-81.8 %.  At config C (2048 big tiles) the big shape stays ahead
// (87.1-87.8 vs 85.0-87.1 %), at F they tie, at D (BE) big SEQF = 3 wins.
// Both counts are of WHOLE tiles: a partial last tile (map 3) is scheduled
// first and runs beside the first round, so 4M + 3 doubles is one round of
// 256 half tiles, not 257.
constexpr int kHalfBS = 512, kHalfR = 16;
// The fused round (k_round, 166 VGPRs native / 174 big-endian at 512 lanes,
// no spills) takes the half shape on the same rule: same process, same
// buckets against its big/mid shapes (tools/half_round_probe.py,
// profiles/r03/i/half_round_probe.jsonl): 1/2/3/5 partitions of 4M x 32 at
// 85.4/81.2/80.8/81.0 % vs 84.5/79.0/78.1/74.2 %, 3 x 4M big-endian 80.2 vs
// 74.3 %, config B's shape 71.9 vs 72.8 %.  IPLS_HALF_ROUND=0 builds the
// fused round without it (the A/B variant, make variants).
#ifndef IPLS_HALF_ROUND
#define IPLS_HALF_ROUND 1
#endif
// ACCUM (the fold reads its target too) on fewer than 1024 big R = 16
// tiles: the half shape at R = 16 (202 VGPRs native, 204 big-endian, no
// spills) instead of the big R = 8 tiles of the same size.  Same process
// (profiles/r03/k/sweep_accum.txt, r03/l/sweep_accum2*.txt): 1/2/3/5
// partitions of 4M x 32 at 83.9/82.7/85.3/84.9 % vs 81.0/80.9/82.3/82.5 %,
// big-endian 1/3 at 81.8/82.9 vs 79.2/81.4 %; at 16/32/64 partitions the two
// tie (82.3/79.9/81.6 vs 81.8/80.2/81.2 %), which the big R = 8 tiles keep.
// The fused round's ACCUM start (AGG already holds arrivals) keeps big/mid.
#ifndef IPLS_HALF_ACCUM
#define IPLS_HALF_ACCUM 1
#endif
// Which folds may take the half shape at all; for the others its kernels are
// not instantiated (engine.hip asks this in an if constexpr).
constexpr bool half_allowed(int start, bool fin) {
  return (!fin || IPLS_HALF_ROUND) && (start != IPLS_START_ACCUM || (IPLS_HALF_ACCUM && !fin));
}
// Past 4 rounds the half shape also takes grids whose big tiles leave part
// of the last round idle while its own tiles do not (with L = 4M: 9, 11, 13,
// 15 partitions; profiles/r03/k/sweep_midp.txt: 9 x 4M 87.3-87.5 vs 82.8-83.0 %,
// 13 x 4M 84.3-84.4 vs 83.4-83.5 %), and leaves whole rounds to the big shape
// (8, 10, 12 x 4M: big ahead by 0-0.8 points).
inline double round_eff(int64_t tiles) {   // busy fraction of the rounds of 256 one-workgroup CUs
  const int64_t r = (tiles + 255) / 256;
  return r > 0 ? (double)tiles / (double)(r * 256) : 0.0;
}
// The big tiles counted are the R = 16 ones (32768 doubles) for every start
// mode: ACCUM's big shape runs R = 8 tiles the size of a half tile.
// IPLS_HALF_ALWAYS=1 (A/B builds only) sends every grid that fills to it.
#ifndef IPLS_HALF_ALWAYS
#define IPLS_HALF_ALWAYS 0
#endif
inline bool use_half(int64_t maxL, int n_parts, int64_t half_tile) {
  const int64_t tb = (maxL / ((int64_t)kBigBS * 2 * 16)) * n_parts, th = (maxL / half_tile) * n_parts;
  return fill(th) && (IPLS_HALF_ALWAYS || tb < 1024 || round_eff(th) > round_eff(tb) + 0.06);
}
// The mid shape (256 lanes, one or two partitions: per-partition flushes, the
// storage merge of one partition's files) with big-endian input runs 8
// vectors per lane on hipcc's own schedule (100 VGPRs, no spills): one
// partition of 4M x 32 peers at 83-86 % against 55-64 % for the big shape's
// R = 16 SEQ schedules at 256 lanes (profiles/r02/s3/sweep_be_p1.txt, BE in
// and BE in + out, two processes each).  Native doubles keep R = 16 (86-88 %).
constexpr int mid_r(bool be_in, int start) { return be_in ? 8 : big_r(be_in, start); }
constexpr int mid_seqf(bool be_in, int start) { return mid_r(be_in, start) > 8 ? big_seqf(be_in, start) : 0; }

// partial last tiles are scheduled first (map 3, ipls_kernels.hpp map_block)
inline bool partial_last(int64_t maxL, int64_t tile) { return maxL > tile && maxL % tile != 0; }
// map 2 pads the grid to the 8 XCDs (ipls_kernels.hpp grid_blocks; engine.hip asserts that the two agree)
constexpr int64_t plan_grid(int map, int64_t tiles) { return map == 2 ? (tiles + 7) / 8 * 8 : tiles; }

// The plan of k_reduce (fin: of the fused round, k_round); start is IPLS_START_*.
inline ReducePlan plan_reduce(bool be_in, int start, bool fin, int64_t maxL, int n_parts) {
  ReducePlan p{};
  p.kernel = fin ? IPLS_KERNEL_ROUND : IPLS_KERNEL_REDUCE;
  auto tiles = [&](int shape, int block, int r, int seqf) {   // try a shape: its tiles over the whole batch
    p.shape = shape, p.block = block, p.r = r, p.seqf = seqf;
    p.tile = (int64_t)block * 2 * r;
    p.tpp = (maxL + p.tile - 1) / p.tile;
    return p.tpp * n_parts;
  };
  if (half_allowed(start, fin) && use_half(maxL, n_parts, (int64_t)kHalfBS * 2 * kHalfR)) {
    tiles(IPLS_SHAPE_HALF, kHalfBS, kHalfR, 0);
    p.map = partial_last(maxL, p.tile) ? 3 : kBigMap;
  } else if (const int64_t tb = tiles(IPLS_SHAPE_BIG, kBigBS, big_r(be_in, start), big_seqf(be_in, start)); fill(tb)) {
    p.map = partial_last(maxL, p.tile) ? 3 : big_map(be_in, tb);
  } else if (fill(tiles(IPLS_SHAPE_MID, kMidBS, mid_r(be_in, start), mid_seqf(be_in, start)))) {
    p.map = partial_last(maxL, p.tile) ? 3 : kBigMap;
  } else {
    tiles(IPLS_SHAPE_SMALL, kSmallBS, kSmallR, 0);
    p.map = kSmallMap;
  }
  p.grid = plan_grid(p.map, p.tpp * n_parts);
  return p;
}

// The scalar fallback (k_reduce_scalar: a bucket or a destination off 16 B):
// tiles of 8 elements per lane, partition-major.
constexpr int kScalarBS = 256, kScalarPerLane = 8;
inline ReducePlan plan_reduce_scalar(int64_t maxL, int n_parts) {
  const int64_t tile = (int64_t)kScalarBS * kScalarPerLane, tpp = (maxL + tile - 1) / tile;
  return ReducePlan{IPLS_KERNEL_REDUCE_SCALAR, 0, kScalarBS, 1, 0, 0, tile, tpp, tpp * n_parts};
}

// ---- kernel dispatch: k_reduce_narrow (DEV_F32 / DEV_F16 / DEV_BF16 buckets) ----
// One shape per element size (narrow_shape), for every grid; the two blocks
// below say why floats and 16-bit elements differ in vectors per lane.
// Floats: 1024-lane workgroups, 2 vectors of 4 floats per
// lane (32 KiB of a bucket per block, 16 accumulator VGPRs), the next peer's 2
// loads issued before this peer's values are added (PF = 1; 70 VGPRs, no
// spills).  Same process, same buckets, single launches
// (tools/reduce_f32_sweep.hip, profiles/f32_boundary/sweep_*.txt): config C's
// 16 x 4M x 32 at 79.8 % of 8 TB/s against 70.3-77.0 % for the other
// prefetching shapes of 256..1024 lanes x 2..8 vectors and 70.6-79.8 % without
// the prefetch; 1 x 4M x 32 at 82.4 %, the best of the sweep; ETHModel's
// 3 x 147,870 x 3 within 5 % of the best.
// 16-bit formats: layout A of the sweep -- 8-B loads, 4 elements per lane per
// vector, the same lane ^ 4 swap before the stores as for floats -- on
// 1024-lane workgroups with 4 vectors per lane (32 KiB of a bucket per
// block, 32 accumulator VGPRs), the next peer's 4 loads issued before this
// peer's values are added (68-90 VGPRs over the start modes, no scratch).
// Same process, same buckets, single launches, sums 128-B aligned as in the
// arena (tools/reduce_h16_sweep.hip, profiles/h16_boundary/sweep_*.txt).  At
// config C's 16 x 4M x 32 three shapes are level: this one 0.781-0.796 ms
// (75.9-77.4 % of 8 TB/s), layout A's 512 x 2 0.791-0.792 ms, and layout B
// (16-B loads, 8 elements per lane, pairs transposed across 8 lanes) at
// 512 x 2 without the prefetch 0.771-0.799 ms, the fastest row for halves.
// 1 x 4M x 32 decides: this shape 77.2 % (level with the column's best, B's
// 1024 x 2 with the prefetch, 77.4 %, which has 73.3-73.7 % at config C)
// against 69.2 % for B's 512 x 2 and 64.5 % for A's 512 x 2.  ETHModel's
// 3 x 147,870 x 3 takes 7.5 us against 6.6 us for the tiles of 8,192 elements
// and below (30 blocks instead of 57 or more).  Both layouts write 1.0000x the algorithmic bytes; without
// the exchange A writes 1.114x and B 1.56-1.59x (pmc_sweep_WRITE_SIZE.csv).
// Partial last tiles are scheduled first (map 3) as for k_reduce.  vec: every
// bucket and destination is 16-B aligned; otherwise the same grid runs element
// by element.
struct NarrowShape {
  int bs, r, pf, e;   // lanes, vectors per lane, next-peer prefetch, elements per lane per vector
  int kernel;         // what the launch record names
};
constexpr NarrowShape narrow_shape(int elem_size) {
  return elem_size == 4 ? NarrowShape{1024, 2, 1, 4, IPLS_KERNEL_REDUCE_F32}
                        : NarrowShape{1024, 4, 1, 4, IPLS_KERNEL_REDUCE_H16};
}
// The plan of k_reduce_narrow (fin: of the fused round, k_round_narrow, which
// runs only with every operand 16-B aligned) over elements of 4 or 2 bytes.
inline ReducePlan plan_reduce_narrow(int elem_size, bool fin, bool vec, int64_t maxL, int n_parts) {
  const NarrowShape K = narrow_shape(elem_size);
  const int kernel = !fin ? K.kernel : elem_size == 4 ? IPLS_KERNEL_ROUND_F32 : IPLS_KERNEL_ROUND_H16;
  const int64_t tile = (int64_t)K.bs * K.e * K.r, tpp = (maxL + tile - 1) / tile;
  const int v = (vec || fin) ? 1 : 0;
  return ReducePlan{kernel, 0, K.bs, K.r, v, (v && partial_last(maxL, tile)) ? 3 : 0, tile, tpp, tpp * n_parts};
}

}  // namespace ipls::reduceplan
