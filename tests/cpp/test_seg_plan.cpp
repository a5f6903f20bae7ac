// The plan of the segment-list calls (csrc/seg_plan.hpp) against a brute-force
// element map: the flat vector is spelled out element by element as (segment,
// element in the segment), and every piece and item of a plan is checked
// against that map.
//   * geometry by the reference chunk rule (chunk = M / P + 1) and synthetic
//     (every partition chunk + 1 long), chunk down to 1, tile 1 .. 8
//   * segment tables: random, with empty segments and 1-element runs; seams
//     planted on every tile seam and partition boundary; every format and
//     every address residue the format allows
//   * n from 0 to past the model (an overrun), owned lists with repeats
//   * one shard, and the partitions split into two shards
// Checked: the pieces of a job cover [0, ncopy) in order without a gap, each
// names the element the map names; every accumulator tile is one item of its
// launch and no tile is in two; piece ranges, format, residue and `whole` of
// an item are what the map gives; the j-th repeat goes to launch j; the
// divide's items cover every output element of the shard below the model size
// once, start on 128-byte lines after the head, and are `whole` only inside
// one partition.
// Built with -fsanitize=address,undefined (make seg_plan_test); prints one line
// and exits 0, or the first mismatch and exits 1.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "seg_plan.hpp"

using namespace ipls::segplan;

static long g_plans = 0;

struct Case {
  std::vector<int64_t> off, len;   // the whole handle
  int64_t chunk = 0;
  std::vector<Seg> segs;
  int64_t tile = 1;
  int lo = 0, hi = 0;              // the shard's partitions
};

#define FAIL(...)                                                                                          \
  do {                                                                                                     \
    std::fprintf(stderr, "seg_plan: P=%d chunk=%lld tile=%lld shard=[%d,%d) segs=[", (int)c.off.size(),    \
                 (long long)c.chunk, (long long)c.tile, c.lo, c.hi);                                       \
    for (const Seg& s_ : c.segs) std::fprintf(stderr, "%lld/f%d/m%d ", (long long)s_.n, s_.fmt, s_.mod);   \
    std::fprintf(stderr, "]: ");                                                                           \
    std::fprintf(stderr, __VA_ARGS__);                                                                     \
    std::fprintf(stderr, "\n");                                                                            \
    std::fflush(stderr);                                                                                   \
    _exit(1);                                                                                              \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
static int rnd_below(int n) { return (int)(rnd() % (uint64_t)n); }

static Geometry shard_geometry(const Case& c) {
  Geometry g;
  g.P = c.hi - c.lo;
  g.chunk = c.chunk;
  g.off = c.off.data() + c.lo;
  g.len = c.len.data() + c.lo;
  g.flat_base = g.P ? c.off[(size_t)c.lo] : 0;
  g.flat_total = 0;
  for (int p = c.lo; p < c.hi; ++p) g.flat_total = std::max(g.flat_total, c.off[(size_t)p] + c.len[(size_t)p] - 1);
  return g;
}

// the brute-force map: flat element f is element el[f] of segment sg[f]
struct Map {
  std::vector<int> sg;
  std::vector<int64_t> el;
};
static Map element_map(const Case& c) {
  Map m;
  for (int s = 0; s < (int)c.segs.size(); ++s)
    for (int64_t e = 0; e < c.segs[(size_t)s].n; ++e) {
      m.sg.push_back(s);
      m.el.push_back(e);
    }
  return m;
}
static int residue(const Seg& s, int64_t e) {
  const int esz = fmt_esz(s.fmt);
  return (int)((s.mod + e * esz) % 16) / esz;
}

static void check_source(const Case& c, const std::vector<int32_t>& list, bool update) {
  const Geometry g = shard_geometry(c);
  const Map m = element_map(c);
  const int64_t n = (int64_t)m.sg.size();
  const Plan pl = update ? plan_update(g, c.segs.data(), (int)c.segs.size(), list.data(), (int)list.size(), c.tile)
                         : plan_send(g, c.segs.data(), (int)c.segs.size(), list.data(), (int)list.size());
  ++g_plans;
  int over = -1;
  for (int q = 0; q < g.P && over < 0; ++q) {
    int64_t cnt = 0;
    for (int64_t j = 0; j < g.chunk; ++j)
      if (g.off[q] + j < n) ++cnt;
    if (cnt > g.len[q] - 1) over = q;
  }
  if (over >= 0) {
    if (pl.status != kOverrun || pl.bad != over) FAIL("expected an overrun of partition %d, got status %d", over, pl.status);
    if (!pl.launches.empty()) FAIL("an overrun plan has launches");
    return;
  }
  if (pl.status != kOk) FAIL("status %d", pl.status);
  if (pl.n != n) FAIL("n %lld, expected %lld", (long long)pl.n, (long long)n);
  // the j-th repeat of a partition is in launch j (update) / job i is list[i] (send)
  std::vector<int> times((size_t)g.P, 0);
  std::vector<size_t> at(pl.launches.size(), 0);
  for (size_t i = 0; i < list.size(); ++i) {
    const size_t j = update ? (size_t)times[(size_t)list[i]]++ : 0;
    if (j >= pl.launches.size() || at[j] >= pl.launches[j].jobs.size() || pl.launches[j].jobs[at[j]].q != list[i])
      FAIL("list entry %zu (partition %d) is not job %zu of launch %zu", i, list[i], j < at.size() ? at[j] : 0, j);
    ++at[j];
  }
  for (size_t j = 0; j < pl.launches.size(); ++j)
    if (at[j] != pl.launches[j].jobs.size()) FAIL("launch %zu has %zu jobs, expected %zu", j, pl.launches[j].jobs.size(), at[j]);
  for (const Launch& l : pl.launches) {
    std::vector<char> seen((size_t)g.P, 0);
    bool any_whole = false;
    size_t item = 0;
    for (int ji = 0; ji < (int)l.jobs.size(); ++ji) {
      const Job& j = l.jobs[(size_t)ji];
      if (update && seen[(size_t)j.q]++) FAIL("partition %d twice in one launch", j.q);
      int64_t ncopy = 0;
      for (int64_t k = 0; k < g.chunk; ++k)
        if (g.off[j.q] + k < n) ++ncopy;
      if (j.ncopy != ncopy || j.L != g.len[j.q]) FAIL("job of partition %d: ncopy %lld L %lld", j.q, (long long)j.ncopy, (long long)j.L);
      if (j.piece_lo < 0 || j.piece_hi < j.piece_lo || j.piece_hi > (int)pl.pieces.size()) FAIL("piece range of partition %d", j.q);
      // the pieces against the map, element by element
      int64_t d = 0;
      for (int k = j.piece_lo; k < j.piece_hi; ++k) {
        const Piece& p = pl.pieces[(size_t)k];
        if (p.n < 1 || p.dst != d) FAIL("partition %d piece %d: dst %lld n %lld, expected dst %lld", j.q, k, (long long)p.dst, (long long)p.n, (long long)d);
        for (int64_t e = 0; e < p.n; ++e, ++d) {
          const int64_t f = g.off[j.q] + d;
          if (d >= ncopy || m.sg[(size_t)f] != p.seg || m.el[(size_t)f] != p.src + e)
            FAIL("partition %d element %lld: piece says (%d, %lld)", j.q, (long long)d, p.seg, (long long)(p.src + e));
        }
        if (k + 1 < j.piece_hi && pl.pieces[(size_t)k + 1].seg == p.seg) FAIL("two pieces of one segment in a row");
      }
      if (d != ncopy) FAIL("partition %d: pieces cover %lld of %lld", j.q, (long long)d, (long long)ncopy);
      if (!update) continue;
      // the items: the tiles of [0, L) in order, each once
      for (int64_t lo = 0; lo < j.L; lo += c.tile, ++item) {
        if (item >= l.items.size()) FAIL("partition %d: tile at %lld has no item", j.q, (long long)lo);
        const Item& it = l.items[item];
        const int64_t hi = std::min(lo + c.tile, j.L);
        if (it.job != ji || it.lo != lo || it.hi != hi) FAIL("item %zu: job %d [%lld, %lld)", item, it.job, (long long)it.lo, (long long)it.hi);
        // what the map says about the tile
        int k_lo = -1, k_hi = -1, fmt = -2, seg0 = -1;
        bool one_seg = true;
        for (int64_t i = lo; i < hi && i < ncopy; ++i) {
          const int64_t f = g.off[j.q] + i;
          int k = j.piece_lo;
          while (!(pl.pieces[(size_t)k].dst <= i && i < pl.pieces[(size_t)k].dst + pl.pieces[(size_t)k].n)) ++k;
          if (k_lo < 0) k_lo = k;
          k_hi = k + 1;
          const int sf = c.segs[(size_t)m.sg[(size_t)f]].fmt;
          fmt = fmt == -2 || fmt == sf ? sf : -1;
          if (seg0 < 0) seg0 = m.sg[(size_t)f];
          one_seg = one_seg && seg0 == m.sg[(size_t)f];
        }
        if (k_lo < 0) {
          if (it.piece_lo != it.piece_hi || it.whole || it.fmt != -1 || it.res != 0) FAIL("item %zu above ncopy has pieces", item);
          continue;
        }
        if (it.piece_lo != k_lo || it.piece_hi != k_hi) FAIL("item %zu: pieces [%d, %d), expected [%d, %d)", item, it.piece_lo, it.piece_hi, k_lo, k_hi);
        if (it.fmt != fmt) FAIL("item %zu: fmt %d, expected %d", item, it.fmt, fmt);
        const int64_t f0 = g.off[j.q] + lo;
        const int res = residue(c.segs[(size_t)m.sg[(size_t)f0]], m.el[(size_t)f0]);
        if (it.res != res) FAIL("item %zu: residue %d, expected %d", item, it.res, res);
        const bool whole = hi - lo == c.tile && hi <= ncopy && one_seg;
        if ((it.whole != 0) != whole) FAIL("item %zu: whole %d, expected %d", item, it.whole, (int)whole);
        any_whole = any_whole || whole;
      }
    }
    if (update && item != l.items.size()) FAIL("%zu items, expected %zu", l.items.size(), item);
    if (update && l.any_whole != any_whole) FAIL("any_whole %d", (int)l.any_whole);
  }
}

static void check_divide(const Case& c) {
  const Geometry g = shard_geometry(c);
  const Map m = element_map(c);
  const int64_t n = (int64_t)m.sg.size();
  const Plan pl = plan_divide(g, c.segs.data(), (int)c.segs.size(), c.tile);
  ++g_plans;
  if (n < g.flat_total) {
    if (pl.status != kShort || !pl.launches.empty()) FAIL("a short list: status %d", pl.status);
    return;
  }
  if (pl.status != kOk || pl.launches.size() != 1) FAIL("divide status %d", pl.status);
  std::vector<int> hits((size_t)n, 0);
  std::vector<int64_t> start(c.segs.size() + 1, 0);
  for (size_t s = 0; s < c.segs.size(); ++s) start[s + 1] = start[s] + c.segs[s].n;
  for (const Item& it : pl.launches[0].items) {
    if (it.job < 0 || it.job >= (int)c.segs.size() || it.lo < 0 || it.hi <= it.lo || it.hi > c.segs[(size_t)it.job].n)
      FAIL("divide item out of its segment");
    const Seg& sg = c.segs[(size_t)it.job];
    if (it.flat != start[(size_t)it.job] + it.lo || it.fmt != sg.fmt) FAIL("divide item: flat %lld fmt %d", (long long)it.flat, it.fmt);
    for (int64_t e = it.lo; e < it.hi; ++e) ++hits[(size_t)(it.flat + e - it.lo)];
    const int esz = fmt_esz(sg.fmt);
    const int64_t addr = sg.mod + it.lo * esz;
    // the segment's first item here ends at the first 128-byte line (walked byte address by byte address),
    // every later one starts a whole number of tiles after that
    const int64_t e0 = std::max(start[(size_t)it.job], g.flat_base) - start[(size_t)it.job];
    const int64_t e1 = std::min(start[(size_t)it.job + 1], g.flat_total) - start[(size_t)it.job];
    int64_t body = e0;
    while (body < e1 && (sg.mod + body * esz) % 128) ++body;
    const bool head = it.lo < body;
    if (head && (it.lo != e0 || it.hi != body)) FAIL("the head is [%lld, %lld), expected [%lld, %lld)", (long long)it.lo, (long long)it.hi, (long long)e0, (long long)body);
    if (!head && ((it.lo - body) % c.tile || it.hi != std::min(it.lo + c.tile, e1)))
      FAIL("divide item [%lld, %lld) is not a tile after the head at %lld", (long long)it.lo, (long long)it.hi, (long long)body);
    if (c.tile * esz % 128 == 0 && !head && addr % 128) FAIL("divide item at element %lld does not start on a line", (long long)it.lo);
    const bool whole = !head && it.hi - it.lo == c.tile && it.flat / g.chunk == (it.flat + c.tile - 1) / g.chunk;
    if ((it.whole != 0) != whole) FAIL("divide item at %lld: whole %d, expected %d", (long long)it.flat, it.whole, (int)whole);
  }
  for (int64_t f = 0; f < n; ++f) {
    const int want = f >= g.flat_base && f < g.flat_total;
    if (hits[(size_t)f] != want) FAIL("output element %lld written %d times, expected %d", (long long)f, hits[(size_t)f], want);
  }
}

static int mod_for(int fmt) { return rnd_below(128 / fmt_esz(fmt)) * fmt_esz(fmt); }

// segment tables that sum to n values
static std::vector<Seg> random_segs(int64_t n) {
  std::vector<Seg> v;
  int64_t left = n;
  while (left > 0 || rnd_below(4) == 0) {
    Seg s;
    const int kind = rnd_below(6);
    s.n = kind == 0 ? 0 : kind == 1 ? 1 : 1 + rnd_below(9);
    s.n = std::min(s.n, left);
    s.fmt = rnd_below(4);
    s.mod = mod_for(s.fmt);
    v.push_back(s);
    left -= s.n;
    if (v.size() > 64) break;
  }
  if (left > 0) {
    Seg s;
    s.n = left;
    s.fmt = rnd_below(4);
    s.mod = mod_for(s.fmt);
    v.push_back(s);
  }
  return v;
}
// seams exactly at the given flat indices (sorted), an empty segment at every other one
static std::vector<Seg> seam_segs(int64_t n, const std::vector<int64_t>& seams) {
  std::vector<Seg> v;
  int64_t at = 0;
  int k = 0;
  auto push = [&](int64_t len) {
    Seg s;
    s.n = len;
    s.fmt = k++ % 4;
    s.mod = mod_for(s.fmt);
    v.push_back(s);
  };
  for (int64_t b : seams) {
    if (b <= at || b >= n) continue;
    push(b - at);
    if (k % 2) push(0);
    at = b;
  }
  if (n > at) push(n - at);
  return v;
}

int main() {
  for (int P = 1; P <= 5; ++P)
    for (int64_t M = P; M <= 40; M += (M < 12 ? 1 : 7)) {
      for (int synthetic = 0; synthetic < 2; ++synthetic) {
        Case c;
        c.chunk = synthetic ? std::max<int64_t>(M / P, 1) : M / P + 1;
        bool ok = true;
        for (int p = 0; p < P; ++p) {
          const int64_t L = synthetic ? c.chunk + 1 : ((int64_t)(p + 1) * c.chunk > M ? M - (int64_t)p * c.chunk + 1 : c.chunk + 1);
          if (L < 1) ok = false;
          c.len.push_back(L);
          c.off.push_back((int64_t)p * c.chunk);
        }
        if (!ok) continue;
        int64_t total = 0;
        for (int p = 0; p < P; ++p) total = std::max(total, c.off[(size_t)p] + c.len[(size_t)p] - 1);
        for (c.tile = 1; c.tile <= 8; c.tile += (c.tile < 4 ? 1 : 4)) {
          // seams on every tile seam of every partition and on every partition boundary
          std::vector<int64_t> seams;
          for (int p = 0; p < P; ++p)
            for (int64_t t = 0; t < c.chunk; t += c.tile) seams.push_back(c.off[(size_t)p] + t);
          std::sort(seams.begin(), seams.end());
          seams.erase(std::unique(seams.begin(), seams.end()), seams.end());
          for (int64_t n : {(int64_t)0, (int64_t)1, total / 2, total - 1, total, total + 1, total + 3}) {
            if (n < 0) continue;
            for (int rep = 0; rep < 6; ++rep) {
              c.segs = rep == 0 ? seam_segs(n, seams) : random_segs(n);
              if (rep == 1 && n > 0) {   // one segment
                Seg s;
                s.n = n;
                s.fmt = rnd_below(4);
                s.mod = mod_for(s.fmt);
                c.segs.assign(1, s);
              }
              for (int split = 0; split <= P; split += std::max(1, P / 2)) {   // one shard, then two
                const int cuts[2][2] = {{0, split ? split : P}, {split ? split : P, P}};
                for (int sh = 0; sh < 2; ++sh) {
                  c.lo = cuts[sh][0];
                  c.hi = cuts[sh][1];
                  const int Ps = c.hi - c.lo;
                  std::vector<int32_t> list;
                  check_source(c, list, true);
                  for (int q = 0; q < Ps; ++q) list.push_back(q);
                  check_source(c, list, true);
                  check_source(c, list, false);
                  if (Ps) {
                    list.clear();
                    for (int i = 0; i < 1 + rnd_below(6); ++i) list.push_back(rnd_below(Ps));   // repeats
                    check_source(c, list, true);
                    check_source(c, list, false);
                  }
                  check_divide(c);
                }
              }
            }
          }
        }
      }
    }
  // a tile of whole 128-byte lines for every format: the divide's tiles then start on lines
  for (int rep = 0; rep < 40; ++rep) {
    Case c;
    c.chunk = 150 + rnd_below(200);
    c.tile = 64;
    const int P = 1 + rnd_below(4);
    for (int p = 0; p < P; ++p) {
      c.len.push_back(c.chunk + 1);
      c.off.push_back((int64_t)p * c.chunk);
    }
    const int64_t total = (int64_t)P * c.chunk;
    std::vector<Seg> v = random_segs(rnd_below(200));   // short segments first, then long ones
    int64_t have = 0;
    for (const Seg& s : v) have += s.n;
    while (have < total + rep % 3) {
      Seg s;
      s.n = std::min<int64_t>(1 + rnd_below(400), total + rep % 3 - have);
      s.fmt = rnd_below(4);
      s.mod = mod_for(s.fmt);
      v.push_back(s);
      have += s.n;
    }
    c.segs = v;
    const int split = rnd_below(P + 1);
    const int cuts[2][2] = {{0, split}, {split, P}};
    for (int sh = 0; sh < 2; ++sh) {
      c.lo = cuts[sh][0];
      c.hi = cuts[sh][1];
      check_divide(c);
      std::vector<int32_t> list;
      for (int q = 0; q < c.hi - c.lo; ++q) list.push_back(q);
      if (have <= total) check_source(c, list, true);
    }
  }
  // bad arguments are refused, not planned
  {
    Case c;
    c.chunk = 4;
    c.off = {0, 4};
    c.len = {5, 5};
    c.hi = 2;
    const Geometry g = shard_geometry(c);
    Seg s;
    s.n = -1;
    if (plan_update(g, &s, 1, nullptr, 0, 4).status != kBadArg) FAIL("a negative length was planned");
    s.n = 3;
    s.fmt = 7;
    if (plan_divide(g, &s, 1, 4).status != kBadArg) FAIL("an unknown format was planned");
    s.fmt = kF32;
    s.mod = 2;
    if (plan_update(g, &s, 1, nullptr, 0, 4).status != kBadArg) FAIL("a misaligned segment was planned");
    s.mod = 4;
    const int32_t bad[1] = {2};
    const Plan pl = plan_update(g, &s, 1, bad, 1, 4);
    if (pl.status != kBadPartition || pl.bad != 2) FAIL("a bad owned entry was planned");
  }
  std::printf("seg_plan: %ld plans ok\n", g_plans);
  return 0;
}
