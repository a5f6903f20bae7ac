// The plan of ipls_agg_update_gradient_chunked (csrc/flat_plan.hpp) against a
// brute-force element map, for every small geometry: P <= 6 partitions by the
// reference chunk rule (chunk = M / P + 1 <= 9), every n in [0, M + 2], every
// owned subset (and lists with repeats), every split of the partitions into 1
// to 3 contiguous shards (empty ones included), call chunks 2 .. 12.
//   * every owned element is copied exactly once, to the right stage offset
//   * nothing that is not owned is copied
//   * the source calls tile [0, min(n, flat size)) in order, none longer than
//     the chunk, none across a shard's flat start
//   * a chunk makes at most one copy per owned partition
//   * the jobs: every occurrence of a partition once, none twice in a launch
// Built with -fsanitize=address,undefined (make flat_plan_test); prints one
// line and exits 0, or the first mismatch and exits 1.  The whole sweep is 28
// million plans: the checker keeps its own maps in fixed arrays (the plan's
// vectors are the code under test and stay), and the (P, M, shard split) cases
// are handed out to worker threads (`--threads N`, by default one per CPU, at
// most 16).
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "flat_plan.hpp"

using namespace ipls::flatplan;

static std::atomic<long> g_plans{0};
static constexpr int kMaxP = 6, kMaxS = 3, kMaxFlat = 64;   // the sweep's bounds; main() keeps to them

#define FAIL(...)                                                                          \
  do {                                                                                     \
    std::fprintf(stderr, "flat_plan: M=%lld P=%d n=%lld chunk=%lld shards=[", (long long)M, g.P, (long long)n, \
                 (long long)chunk);                                                        \
    for (int v : g.shard_lo) std::fprintf(stderr, "%d ", v);                               \
    std::fprintf(stderr, "] owned=[");                                                     \
    for (int32_t v : owned) std::fprintf(stderr, "%d ", v);                                \
    std::fprintf(stderr, "]: ");                                                           \
    std::fprintf(stderr, __VA_ARGS__);                                                     \
    std::fprintf(stderr, "\n");                                                            \
    std::fflush(stderr);                                                                   \
    _exit(1);                                                                              \
  } while (0)

static void check(const Geometry& g, int64_t M, int64_t n, const std::vector<int32_t>& owned, int64_t chunk) {
  const Plan pl = make_plan(g, n, owned.data(), (int)owned.size(), chunk);
  // brute force: does any partition overrun?
  int over = -1;
  for (int p = 0; p < g.P && over < 0; ++p) {
    int64_t c = 0;
    for (int64_t j = 0; j < g.chunk; ++j)
      if (g.off[p] + j < n) ++c;
    if (c > g.len[p] - 1) over = p;
  }
  if (over >= 0) {
    if (pl.status != kOverrun || pl.bad != over) FAIL("expected an overrun of partition %d, got status %d", over, pl.status);
    if (!pl.chunks.empty() || !pl.copies.empty()) FAIL("an overrun plan has source calls");
    return;
  }
  if (pl.status != kOk) FAIL("status %d", pl.status);
  if (owned.empty()) {
    if (!pl.chunks.empty() || !pl.shards.empty()) FAIL("an empty owned list has source calls");
    return;
  }
  const int S = g.S();
  int owner[kMaxP] = {}, times[kMaxP] = {};
  for (int s = 0; s < S; ++s)
    for (int p = g.shard_lo[s]; p < g.shard_lo[s + 1]; ++p) owner[p] = s;
  for (int32_t p : owned) ++times[p];
  const int64_t end = std::min(n, g.flat_total());
  // the element map: flat index -> (partition, owned?)
  int part_of[kMaxFlat], copied[kMaxFlat] = {};
  if (end > kMaxFlat) FAIL("the sweep outgrew the checker's maps");
  for (int64_t f = 0; f < end; ++f) part_of[f] = -1;
  for (int p = 0; p < g.P; ++p)
    for (int64_t j = 0; j < g.chunk && j < g.len[p] - 1; ++j)
      if (g.off[p] + j < end) part_of[g.off[p] + j] = p;
  // the involved shards
  int stage_of[kMaxS] = {-1, -1, -1};
  for (size_t k = 0; k < pl.shards.size(); ++k) {
    if (k && pl.shards[k].shard <= pl.shards[k - 1].shard) FAIL("shards not ascending");
    stage_of[pl.shards[k].shard] = (int)k;
    if (pl.shards[k].base != g.off[g.shard_lo[pl.shards[k].shard]]) FAIL("shard base");
  }
  for (int s = 0; s < S; ++s) {
    bool inv = false;
    for (int32_t p : owned) inv |= owner[p] == s;
    if (inv != (stage_of[s] >= 0)) FAIL("shard %d involved=%d but planned=%d", s, inv, stage_of[s] >= 0);
  }
  // the chunks
  int64_t pos = 0;
  for (const Chunk& c : pl.chunks) {
    if (c.off != pos) FAIL("chunk at %lld, expected %lld", (long long)c.off, (long long)pos);
    if (c.n < 1 || c.n > chunk) FAIL("chunk of %lld", (long long)c.n);
    if (c.stage < 0 || c.stage >= (int)pl.shards.size()) FAIL("chunk stage %d", c.stage);
    for (int64_t f = c.off; f < c.off + c.n; ++f) {
      // the shard that holds flat index f: the one owning partition min(f / chunk, P - 1)
      const int p = (int)std::min<int64_t>(g.chunk ? f / g.chunk : 0, g.P - 1);
      if (owner[p] != c.shard) FAIL("chunk [%lld,+%lld) crosses into shard %d at %lld", (long long)c.off, (long long)c.n, owner[p], (long long)f);
    }
    if (stage_of[c.shard] >= 0 && c.stage != stage_of[c.shard]) FAIL("chunk received into another shard's ring");
    if (stage_of[c.shard] < 0 && c.copy_hi != c.copy_lo) FAIL("copies on a shard that owns nothing");
    int per_part[kMaxP] = {};
    for (int k = c.copy_lo; k < c.copy_hi; ++k) {
      const Copy& cp = pl.copies[k];
      if (cp.n < 1 || cp.src < 0 || cp.src + cp.n > c.n) FAIL("copy outside its chunk");
      const ShardPlan& sp = pl.shards[c.stage];
      if (cp.dst < 0 || cp.dst + cp.n > sp.seg) FAIL("copy outside the stage");
      int first_p = -1;
      for (int64_t e = 0; e < cp.n; ++e) {
        const int64_t f = c.off + cp.src + e;
        if (cp.dst + e != f - sp.base) FAIL("element %lld lands at stage offset %lld", (long long)f, (long long)(cp.dst + e));
        if (part_of[f] < 0 || !times[part_of[f]]) FAIL("element %lld is not owned and was copied", (long long)f);
        if (first_p < 0) first_p = part_of[f];
        if (part_of[f] != first_p) FAIL("a copy spans two partitions");
        ++copied[f];
      }
      if (++per_part[first_p] > 1) FAIL("two copies of partition %d in one chunk", first_p);
    }
    pos += c.n;
  }
  if (pos != end) FAIL("chunks end at %lld, expected %lld", (long long)pos, (long long)end);
  for (int64_t f = 0; f < end; ++f) {
    const bool want = part_of[f] >= 0 && times[part_of[f]];
    if (copied[f] != (want ? 1 : 0)) FAIL("element %lld copied %d times, expected %d", (long long)f, copied[f], want ? 1 : 0);
  }
  // the jobs
  int seen[kMaxP] = {};
  for (const ShardPlan& sp : pl.shards)
    for (const auto& launch : sp.launches) {
      if (launch.empty()) FAIL("an empty launch");
      int in_launch[kMaxP] = {};
      for (const Job& j : launch) {
        if (owner[j.p] != sp.shard) FAIL("job of partition %d on shard %d", j.p, sp.shard);
        if (++in_launch[j.p] > 1) FAIL("partition %d twice in one launch", j.p);
        ++seen[j.p];
        int64_t nc = 0;
        for (int64_t f = g.off[j.p]; f < g.off[j.p] + g.chunk; ++f)
          if (f < n) ++nc;
        if (j.lo != g.off[j.p] - sp.base || j.ncopy != nc || j.L != g.len[j.p]) FAIL("job of partition %d", j.p);
      }
    }
  for (int p = 0; p < g.P; ++p)
    if (seen[p] != times[p]) FAIL("partition %d in %d jobs, owned %d times", p, seen[p], times[p]);
}

struct Case {
  int P;
  int64_t M;
  std::vector<int> split;
};

static void sweep(const Case& c) {
  const int P = c.P;
  const int64_t M = c.M;
  Geometry g;
  g.P = P;
  g.chunk = M / P + 1;
  for (int i = 0; i < P; ++i) {
    g.len.push_back(((int64_t)(i + 1) * g.chunk > M) ? M - (int64_t)i * g.chunk + 1 : g.chunk + 1);
    g.off.push_back((int64_t)i * g.chunk);
  }
  g.shard_lo = c.split;
  std::vector<int32_t> owned;
  owned.reserve(8);
  long plans = 0;
  for (int64_t n = 0; n <= M + 2; ++n)
    for (int64_t chunk = 2; chunk <= 12; chunk += 2) {
      for (unsigned mask = 0; mask < (1u << P); ++mask) {
        owned.clear();
        for (int p = P - 1; p >= 0; --p)   // descending: the list's order is the caller's
          if (mask >> p & 1) owned.push_back(p);
        check(g, M, n, owned, chunk);
      }
      // repeats: a partition twice, and three times around another
      owned.assign({P - 1, P - 1});
      check(g, M, n, owned, chunk);
      owned.assign({0, P / 2, 0, 0});
      check(g, M, n, owned, chunk);
      plans += (1l << P) + 2;
    }
  g_plans += plans;
}

int main(int argc, char** argv) {
  unsigned threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  if (argc > 2 && !std::strcmp(argv[1], "--threads")) threads = (unsigned)std::max(1, std::atoi(argv[2]));
  std::vector<Case> cases;
  static_assert(kMaxP == 6 && kMaxS == 3, "the loops below");
  for (int P = kMaxP; P >= 1; --P)   // the long cases first
    for (int64_t M = 1; M / P + 1 <= 9; ++M) {
      bool ok = true;
      for (int i = 0; i < P; ++i) ok &= (((int64_t)(i + 1) * (M / P + 1) > M) ? M - (int64_t)i * (M / P + 1) + 1 : M / P + 2) >= 1;
      if (!ok) continue;   // the handle refuses this geometry at open
      cases.push_back({P, M, {0, P}});
      for (int a = 0; a <= P; ++a) cases.push_back({P, M, {0, a, P}});
      for (int a = 0; a <= P; ++a)
        for (int b = a; b <= P; ++b) cases.push_back({P, M, {0, a, b, P}});
    }
  std::atomic<size_t> next{0};
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < threads; ++t)
    pool.emplace_back([&] {
      for (size_t i; (i = next++) < cases.size();) sweep(cases[i]);
    });
  for (auto& th : pool) th.join();
  // refusals
  {
    Geometry g;
    g.P = 2, g.chunk = 3, g.off = {0, 3}, g.len = {4, 3}, g.shard_lo = {0, 2};
    const int32_t bad[] = {0, 2}, neg[] = {-1}, ok[] = {0};
    if (make_plan(g, 5, bad, 2, 4).status != kBadPartition || make_plan(g, 5, neg, 1, 4).status != kBadPartition ||
        make_plan(g, 5, ok, 1, 3).status != kBadArg || make_plan(g, 5, ok, 1, 0).status != kBadArg ||
        make_plan(g, 5, nullptr, 1, 4).status != kBadArg || make_plan(g, -1, ok, 1, 4).status != kBadArg) {
      std::fprintf(stderr, "flat_plan: a bad argument was accepted\n");
      return 1;
    }
  }
  std::printf("flat_plan ok: %ld plans\n", g_plans.load());
  return 0;
}
