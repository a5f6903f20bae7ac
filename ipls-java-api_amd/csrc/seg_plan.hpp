// seg_plan.hpp -- the host-side plan of the segment-list calls
// (ipls_agg_update_gradient_segs, ipls_agg_send_gradients_segs,
// ipls_agg_get_partitions_segs; include/ipls_agg.h): how a flat vector that is
// given as a LIST of arrays -- the concatenation of n_segs segments in list
// order, each of its own element format -- meets the partitions of one shard.
// Plain C++ with no HIP type in it, so the stand-alone program
// tests/cpp/test_seg_plan.cpp checks it under the sanitizers against a
// brute-force element map.
//
// Geometry is the shard's (engine.hip): engine partition q holds len[q]
// doubles (count slot included) and takes flat[off[q] .. off[q] + ncopy_q),
// ncopy_q = clamp(min(off[q] + chunk, n) - off[q], 0 ..), n = sum of the
// segment lengths; off[] is in the handle's flat coordinates and ascends in
// steps of `chunk`; the shard's flat segment is [flat_base, flat_total).
//
// Two products:
//   pieces  for a partition, the sorted runs (first destination index, count,
//           segment, first element in the segment) that cover [0, ncopy);
//           empty segments hold nothing and make no piece;
//   items   one per destination tile of `tile` elements, the unit one block of
//           k_update_segs / k_divide_segs works on.  No destination tile is
//           ever given to two items of one launch.
// Cost: O(n_segs) for the segment starts, O(log n_segs) per partition to find
// its first segment, O(1) per piece and per item.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ipls {
namespace segplan {

enum Status : int { kOk = 0, kBadArg = 1, kOverrun = 2, kBadPartition = 3, kShort = 4 };

// element formats of a segment, in the order the kernels dispatch on
enum : int { kF64 = 0, kF32 = 1, kF16 = 2, kBF16 = 3 };
inline int fmt_esz(int fmt) { return fmt == kF64 ? 8 : fmt == kF32 ? 4 : 2; }

struct Geometry {
  int P = 0;                       // partitions of the shard
  int64_t chunk = 0;               // flat stride between partitions
  const int64_t* off = nullptr;    // per partition, handle flat coordinates
  const int64_t* len = nullptr;
  int64_t flat_base = 0, flat_total = 0;
};

struct Seg {
  int64_t n = 0;     // elements
  int fmt = kF64;
  int mod = 0;       // address mod 128 (a multiple of the element size)
};

// A run of one segment inside one partition: destination elements
// [dst, dst + n) of the partition are elements [src, src + n) of segment seg.
struct Piece {
  int64_t dst = 0, n = 0;
  int seg = 0;
  int64_t src = 0;
};

// One destination tile.  Update: job indexes the launch's jobs, [lo, hi) are
// accumulator elements, [piece_lo, piece_hi) the pieces (of Plan::pieces) that
// meet the tile (none above ncopy).  Divide: job is the OUTPUT segment,
// [lo, hi) its elements, flat the flat index of element lo.
// fmt: the format of the tile's only piece / of the output segment; -1 when
// the tile's pieces have several formats or it has none.
// res: the residue, in elements, of the tile's first source element against a
// 16-byte load (0 when the tile has no piece).
// whole: a full tile inside one piece (so below ncopy) / inside one partition.
struct Item {
  int32_t job = 0, fmt = -1;
  int32_t piece_lo = 0, piece_hi = 0;
  int64_t lo = 0, hi = 0;
  int64_t flat = 0;
  int32_t res = 0, whole = 0;
};

struct Job {
  int q = 0;                         // engine partition
  int64_t ncopy = 0, L = 0;
  int piece_lo = 0, piece_hi = 0;    // its pieces, sorted by dst
};

struct Launch {
  std::vector<Job> jobs;
  std::vector<Item> items;
  bool any_whole = false;
};

struct Plan {
  Status status = kOk;
  int bad = -1;                      // the partition that overruns / the bad list entry
  int64_t n = 0;                     // values in the list
  std::vector<Piece> pieces;
  // update: launch j holds the j-th occurrence of every partition in `owned`
  // (two jobs of one launch never write the same accumulator), in owned order;
  // send: one launch, job i is parts[i]; divide: one launch, no jobs
  std::vector<Launch> launches;
};

inline int64_t ncopy_of(const Geometry& g, int q, int64_t n) {
  return std::max<int64_t>(0, std::min(g.off[q] + g.chunk, n) - g.off[q]);
}

// start[s] = flat index of segment s's first element; start[n_segs] = n
inline bool seg_starts(const Seg* segs, int n_segs, std::vector<int64_t>& start) {
  start.assign((size_t)n_segs + 1, 0);
  for (int s = 0; s < n_segs; ++s) {
    if (segs[s].n < 0 || segs[s].n > INT64_MAX - start[(size_t)s]) return false;
    start[(size_t)s + 1] = start[(size_t)s] + segs[s].n;
  }
  return true;
}

// The pieces of flat [a, b), destination index f - a, appended to out.
inline void pieces_of(const std::vector<int64_t>& start, int n_segs, int64_t a, int64_t b, std::vector<Piece>& out) {
  if (b <= a) return;
  // the last segment that starts at or before a (empty ones at a are stepped over below)
  int s = (int)(std::upper_bound(start.begin(), start.begin() + n_segs, a) - start.begin()) - 1;
  for (int64_t f = a; f < b && s < n_segs; ++s) {
    const int64_t e = std::min(start[(size_t)s + 1], b);
    if (e <= f) continue;            // empty, or wholly before a
    Piece p;
    p.dst = f - a;
    p.n = e - f;
    p.seg = s;
    p.src = f - start[(size_t)s];
    out.push_back(p);
    f = e;
  }
}

// The tiles of one job over [0, L), appended to l.items.
inline void job_items(const Plan& pl, Launch& l, int job, const Seg* segs, int64_t tile) {
  const Job& j = l.jobs[(size_t)job];
  int k = j.piece_lo;
  for (int64_t lo = 0; lo < j.L; lo += tile) {
    Item it;
    it.job = job;
    it.lo = lo;
    it.hi = std::min(lo + tile, j.L);
    while (k < j.piece_hi && pl.pieces[(size_t)k].dst + pl.pieces[(size_t)k].n <= lo) ++k;
    it.piece_lo = k;
    int e = k;
    while (e < j.piece_hi && pl.pieces[(size_t)e].dst < it.hi) ++e;
    it.piece_hi = e;
    if (e > k) {
      const Piece& p = pl.pieces[(size_t)k];
      const Seg& sg = segs[p.seg];
      const int esz = fmt_esz(sg.fmt);
      it.fmt = sg.fmt;
      for (int m = k + 1; m < e; ++m)
        if (segs[pl.pieces[(size_t)m].seg].fmt != sg.fmt) it.fmt = -1;
      const int64_t first = p.src + std::max<int64_t>(lo - p.dst, 0);   // the tile's first source element
      it.res = (int)(((int64_t)sg.mod + (first % 16) * esz) % 16) / esz;
      it.whole = e == k + 1 && it.hi - lo == tile && p.dst <= lo && it.hi <= p.dst + p.n;
    }
    l.any_whole = l.any_whole || it.whole;
    l.items.push_back(it);
  }
}

inline bool args_ok(const Geometry& g, const Seg* segs, int n_segs, int64_t tile) {
  if (g.P < 0 || n_segs < 0 || (n_segs > 0 && !segs) || tile < 1 || (g.P > 0 && (!g.off || !g.len))) return false;
  for (int s = 0; s < n_segs; ++s)
    if (segs[s].fmt < kF64 || segs[s].fmt > kBF16 || segs[s].mod < 0 || segs[s].mod >= 128 ||
        segs[s].mod % fmt_esz(segs[s].fmt))
      return false;
  return true;
}

// UpdateGradient (with_items) and SendGradients (!with_items: `list` is the
// partition list, one launch, job i is list[i]).
inline Plan plan_source(const Geometry& g, const Seg* segs, int n_segs, const int32_t* list, int n_list, int64_t tile,
                        bool with_items) {
  Plan pl;
  std::vector<int64_t> start;
  if (!args_ok(g, segs, n_segs, tile) || n_list < 0 || (n_list > 0 && !list) || !seg_starts(segs, n_segs, start)) {
    pl.status = kBadArg;
    return pl;
  }
  pl.n = start[(size_t)n_segs];
  // OrganizeGradients splits every partition before anything is accumulated or sent
  for (int q = 0; q < g.P; ++q)
    if (ncopy_of(g, q, pl.n) > g.len[q] - 1) {
      pl.status = kOverrun;
      pl.bad = q;
      return pl;
    }
  for (int i = 0; i < n_list; ++i)
    if (list[i] < 0 || list[i] >= g.P) {
      pl.status = kBadPartition;
      pl.bad = list[i];
      return pl;
    }
  if (n_list == 0) return pl;
  std::vector<int> times((size_t)g.P, 0), first((size_t)g.P, -1), last((size_t)g.P, -1);
  for (int i = 0; i < n_list; ++i) {
    const int q = list[i];
    if (first[(size_t)q] < 0) {      // a repeated partition shares its pieces
      first[(size_t)q] = (int)pl.pieces.size();
      pieces_of(start, n_segs, g.off[q], g.off[q] + ncopy_of(g, q, pl.n), pl.pieces);
      last[(size_t)q] = (int)pl.pieces.size();
    }
    const int j = with_items ? times[(size_t)q]++ : 0;
    if ((int)pl.launches.size() <= j) pl.launches.resize((size_t)j + 1);
    Job job;
    job.q = q;
    job.ncopy = ncopy_of(g, q, pl.n);
    job.L = g.len[q];
    job.piece_lo = first[(size_t)q];
    job.piece_hi = last[(size_t)q];
    pl.launches[(size_t)j].jobs.push_back(job);
  }
  if (with_items)
    for (Launch& l : pl.launches)
      for (int j = 0; j < (int)l.jobs.size(); ++j) job_items(pl, l, j, segs, tile);
  return pl;
}

inline Plan plan_update(const Geometry& g, const Seg* segs, int n_segs, const int32_t* owned, int n_owned,
                        int64_t tile) {
  return plan_source(g, segs, n_segs, owned, n_owned, tile, true);
}
inline Plan plan_send(const Geometry& g, const Seg* segs, int n_segs, const int32_t* parts, int n_parts) {
  return plan_source(g, segs, n_segs, parts, n_parts, 1, false);
}

// GetPartitions: the tiles are laid over each OUTPUT segment's part of the
// shard's [flat_base, flat_total): first the head up to the first 128-byte
// line of the output (an item of its own, never whole), then whole-line tiles.
inline Plan plan_divide(const Geometry& g, const Seg* segs, int n_segs, int64_t tile) {
  Plan pl;
  std::vector<int64_t> start;
  if (!args_ok(g, segs, n_segs, tile) || !seg_starts(segs, n_segs, start)) {
    pl.status = kBadArg;
    return pl;
  }
  pl.n = start[(size_t)n_segs];
  if (pl.n < g.flat_total) {
    pl.status = kShort;
    return pl;
  }
  pl.launches.resize(1);
  Launch& l = pl.launches[0];
  if (g.flat_total <= g.flat_base || g.chunk < 1) return pl;
  int s = (int)(std::upper_bound(start.begin(), start.begin() + n_segs, g.flat_base) - start.begin()) - 1;
  for (; s < n_segs && start[(size_t)s] < g.flat_total; ++s) {
    const int64_t a = std::max(start[(size_t)s], g.flat_base), b = std::min(start[(size_t)s + 1], g.flat_total);
    if (b <= a) continue;
    const int esz = fmt_esz(segs[s].fmt);
    const int64_t e0 = a - start[(size_t)s], e1 = b - start[(size_t)s];
    const int64_t at = ((int64_t)segs[s].mod + (e0 % 128) * esz) % 128;   // address of element e0, mod 128
    const int64_t head = std::min<int64_t>(((128 - at) % 128) / esz, e1 - e0);
    for (int64_t lo = e0; lo < e1;) {
      Item it;
      it.job = s;
      it.fmt = segs[s].fmt;
      it.lo = lo;
      const bool is_head = lo == e0 && head > 0;
      it.hi = is_head ? lo + head : std::min(lo + tile, e1);
      it.flat = start[(size_t)s] + lo;
      it.whole = !is_head && it.hi - it.lo == tile && it.flat / g.chunk == (it.flat + tile - 1) / g.chunk;
      l.any_whole = l.any_whole || it.whole;
      l.items.push_back(it);
      lo = it.hi;
    }
  }
  return pl;
}

}  // namespace segplan
}  // namespace ipls
