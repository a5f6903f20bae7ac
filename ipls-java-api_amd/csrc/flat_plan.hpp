// flat_plan.hpp -- the host-side plan of ipls_agg_update_gradient_chunked
// (include/ipls_agg.h): which source calls a whole flat gradient of n values is
// received in, which byte ranges of each chunk cross PCIe, and which jobs
// k_update_flat runs on each shard.  Plain C++ with no HIP type in it, so the
// stand-alone program tests/cpp/test_flat_plan.cpp checks it under the
// sanitizers against a brute-force element map.
//
// Geometry is the handle's (IPLS.java:1019-1028): partition p holds len[p]
// doubles (count slot included) and takes flat[off[p] .. off[p] + ncopy_p),
// ncopy_p = clamp(min(off[p] + chunk, n) - off[p], 0 ..); off[] ascends in
// steps of `chunk`.  Shard s owns partitions [shard_lo[s], shard_lo[s + 1]);
// its flat segment starts at off[shard_lo[s]] and its stage holds element
// flat index f at stage element f - base.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ipls {
namespace flatplan {

enum Status : int { kOk = 0, kBadArg = 1, kOverrun = 2, kBadPartition = 3 };

struct Geometry {
  int P = 0;
  int64_t chunk = 0;                 // flat stride between partitions
  std::vector<int64_t> off, len;     // per partition
  std::vector<int> shard_lo;         // S + 1 ascending partition bounds, shard_lo[0] = 0, shard_lo[S] = P
  int S() const { return (int)shard_lo.size() - 1; }
  int64_t flat_total() const {
    int64_t t = 0;
    for (int p = 0; p < P; ++p) t = std::max(t, off[p] + len[p] - 1);
    return t;
  }
};

// One call of the source: elements [off, off + n) of the flat vector, received
// into the ring of involved shard `stage` (an index into Plan::shards; the
// nearest involved shard when the chunk's own shard owns nothing of `owned`).
struct Chunk {
  int64_t off = 0, n = 0;
  int shard = 0;       // the shard whose flat segment holds the chunk
  int stage = 0;       // index into Plan::shards of the ring it is received into
  int copy_lo = 0, copy_hi = 0;   // its H2D ranges: Plan::copies[copy_lo .. copy_hi)
};

// One H2D: n elements from element `src` of the chunk's slot to element `dst`
// of the stage of the chunk's shard.
struct Copy {
  int64_t src = 0, dst = 0, n = 0;
};

// One job of a launch: AGG[p][i] += flat value at stage element lo + i for
// i < ncopy, 1.0 at ncopy, 0.0 above, for i < L.
struct Job {
  int p = 0;           // handle partition
  int64_t lo = 0, ncopy = 0, L = 0;
};

struct ShardPlan {
  int shard = 0;
  int64_t base = 0;    // flat index of stage element 0
  int64_t seg = 0;     // stage elements: up to the end of the last value any owned partition copies
  // launch j holds the j-th occurrence of every partition in `owned` (two jobs
  // of one launch never write the same accumulator), in owned order
  std::vector<std::vector<Job>> launches;
};

struct Plan {
  Status status = kOk;
  int bad = -1;        // the partition that overruns / the bad owned entry
  std::vector<Chunk> chunks;
  std::vector<Copy> copies;
  std::vector<ShardPlan> shards;   // the involved shards, ascending
};

inline int64_t ncopy_of(const Geometry& g, int p, int64_t n) {
  return std::max<int64_t>(0, std::min(g.off[p] + g.chunk, n) - g.off[p]);
}

inline Plan make_plan(const Geometry& g, int64_t n, const int32_t* owned, int n_owned, int64_t chunk) {
  Plan pl;
  if (n < 0 || n_owned < 0 || (n_owned > 0 && !owned) || chunk < 2 || (chunk & 1) || g.P < 0 || g.S() < 1) {
    pl.status = kBadArg;
    return pl;
  }
  // OrganizeGradients splits every partition before anything is accumulated
  for (int p = 0; p < g.P; ++p)
    if (ncopy_of(g, p, n) > g.len[p] - 1) {
      pl.status = kOverrun;
      pl.bad = p;
      return pl;
    }
  for (int i = 0; i < n_owned; ++i)
    if (owned[i] < 0 || owned[i] >= g.P) {
      pl.status = kBadPartition;
      pl.bad = owned[i];
      return pl;
    }
  if (n_owned == 0) return pl;

  const int S = g.S();
  std::vector<int> owner((size_t)g.P);
  for (int s = 0; s < S; ++s)
    for (int p = g.shard_lo[s]; p < g.shard_lo[s + 1]; ++p) owner[(size_t)p] = s;
  std::vector<int> times((size_t)g.P, 0);       // occurrences of p seen so far
  std::vector<int> stage_of((size_t)S, -1);     // shard -> index into pl.shards
  for (int i = 0; i < n_owned; ++i) {
    const int s = owner[(size_t)owned[i]];
    if (stage_of[(size_t)s] < 0) stage_of[(size_t)s] = 0;
  }
  for (int s = 0; s < S; ++s)
    if (stage_of[(size_t)s] == 0) {
      stage_of[(size_t)s] = (int)pl.shards.size();
      ShardPlan sp;
      sp.shard = s;
      sp.base = g.off[(size_t)g.shard_lo[s]];
      pl.shards.push_back(sp);
    }
  for (int i = 0; i < n_owned; ++i) {
    const int p = owned[i];
    ShardPlan& sp = pl.shards[(size_t)stage_of[(size_t)owner[(size_t)p]]];
    const int j = times[(size_t)p]++;
    if ((int)sp.launches.size() <= j) sp.launches.resize((size_t)j + 1);
    Job job;
    job.p = p;
    job.lo = g.off[(size_t)p] - sp.base;
    job.ncopy = ncopy_of(g, p, n);
    job.L = g.len[(size_t)p];
    sp.launches[(size_t)j].push_back(job);
    sp.seg = std::max(sp.seg, job.lo + job.ncopy);
  }

  // the source calls: consecutive, at most `chunk` elements, cut at the flat
  // start of every non-empty shard
  const int64_t end = std::min(n, g.flat_total());
  std::vector<int> ne;   // non-empty shards
  for (int s = 0; s < S; ++s)
    if (g.shard_lo[s + 1] > g.shard_lo[s]) ne.push_back(s);
  size_t cur = 0;        // ne[cur] holds `pos`
  for (int64_t pos = 0; pos < end;) {
    while (cur + 1 < ne.size() && g.off[(size_t)g.shard_lo[ne[cur + 1]]] <= pos) ++cur;
    int64_t len = std::min(chunk, end - pos);
    if (cur + 1 < ne.size()) len = std::min(len, g.off[(size_t)g.shard_lo[ne[cur + 1]]] - pos);
    Chunk c;
    c.off = pos;
    c.n = len;
    c.shard = ne[cur];
    c.copy_lo = (int)pl.copies.size();
    const int st = stage_of[(size_t)c.shard];
    if (st >= 0) {
      c.stage = st;
      const ShardPlan& sp = pl.shards[(size_t)st];
      // the owned partitions this chunk intersects, each once
      const int p0 = std::max(g.shard_lo[c.shard], (int)(pos / std::max<int64_t>(g.chunk, 1)) - 1);
      for (int p = std::max(p0, 0); p < g.shard_lo[c.shard + 1] && g.off[(size_t)p] < pos + len; ++p) {
        if (!times[(size_t)p]) continue;
        const int64_t a = std::max(pos, g.off[(size_t)p]);
        const int64_t b = std::min(pos + len, g.off[(size_t)p] + ncopy_of(g, p, n));
        if (b <= a) continue;
        Copy cp;
        cp.src = a - pos;
        cp.dst = a - sp.base;
        cp.n = b - a;
        pl.copies.push_back(cp);
      }
    } else {
      // no partition of this shard is owned: the chunk is received (a socket
      // source must consume it) into the ring of the next involved shard, or
      // of the last one, and nothing of it crosses PCIe
      int pick = (int)pl.shards.size() - 1;
      for (int k = 0; k < (int)pl.shards.size(); ++k)
        if (pl.shards[(size_t)k].shard > c.shard) {
          pick = k;
          break;
        }
      c.stage = pick;
    }
    c.copy_hi = (int)pl.copies.size();
    pl.chunks.push_back(c);
    pos += len;
  }
  return pl;
}

}  // namespace flatplan
}  // namespace ipls
