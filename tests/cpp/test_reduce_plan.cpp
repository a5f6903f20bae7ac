// The plan of a fold launch (csrc/reduce_plan.hpp) on the CPU:
//   a. parity: over the grid below the plans are, line for line, those of
//      tests/golden/reduce_plan_cases.txt, recorded from the launch functions
//      as they stood before the plan became a header of its own.  A line is
//        f64 <fin> <be_in> <start> <maxL> <n_parts> <kernel> <shape> <block> <r> <seqf> <map> <tpp> <grid>
//        nar <elem size> <fin> <vec> <maxL> <n_parts> <kernel> <shape> <block> <r> <seqf> <map> <tpp> <grid>
//      (start as IPLS_START_*; k_reduce from ZERO, FIRST, ACCUM, k_round from
//      ZERO, ACCUM; be_out does not enter the decision);
//   b. the production shapes that the GPU tests and DESIGN.md state;
//   c. the set of (kernel, shape, block, r, seqf, map, be_in, start) over the
//      grid is exactly what expected_combinations() of
//      tests/test_gpu_wide_small.py lists for the wide shapes (without be_out)
//      plus the small shape.
// Built with -fsanitize=address,undefined (make reduce_plan_test); prints one
// line and exits 0, or the first mismatch and exits 1.
//   test_reduce_plan <fixture>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "reduce_plan.hpp"

using namespace ipls::reduceplan;

static const int64_t kLens[] = {1,     2,     511,   512,    513,     4096,    4097,    8191,    8192,   8193,
                                16384, 16385, 32768, 32769,  147872,  1048576, 4194304, 4194307, 8388608};
static const int kParts[] = {1, 2, 3, 5, 7, 8, 9, 11, 13, 15, 16, 17, 31, 32, 64, 128, 300, 500};
static const int Z = IPLS_START_ZERO, F = IPLS_START_FIRST, A = IPLS_START_ACCUM;

typedef std::array<int, 8> Combo;   // kernel, shape, block, r, seqf, map, be_in, start
static std::set<Combo> g_seen;
static FILE* g_fix;
static long g_plans, g_line;

[[noreturn]] static void die(const std::string& what) {
  std::fprintf(stderr, "reduce_plan: %s\n", what.c_str());
  std::exit(1);
}

static void row(const char* tag, int a, int b, int c, int64_t maxL, int np, const ReducePlan& p) {
  char got[160], want[160];
  std::snprintf(got, sizeof got, "%s %d %d %d %lld %d %d %d %d %d %d %d %lld %lld\n", tag, a, b, c, (long long)maxL, np,
                p.kernel, p.shape, p.block, p.r, p.seqf, p.map, (long long)p.tpp, (long long)p.grid);
  ++g_line;
  if (!std::fgets(want, sizeof want, g_fix)) die("the fixture ends before line " + std::to_string(g_line));
  if (std::strcmp(got, want)) die("line " + std::to_string(g_line) + ": plan\n  " + got + "fixture\n  " + want);
  // the tile is what the kernels compute from their template arguments
  const int64_t tile = (int64_t)p.block * (tag[0] == 'f' ? 2 : 4) * p.r;
  if (p.tile != tile || p.tpp != (maxL + tile - 1) / tile) die(std::string("tile of ") + got);
  ++g_plans;
}

static void sweep() {
  for (int64_t L : kLens)
    for (int np : kParts) {
      for (int be_in = 0; be_in < 2; ++be_in)
        for (int fin = 0; fin < 2; ++fin)
          for (int start : {Z, F, A}) {
            if (fin && start == F) continue;
            const ReducePlan p = plan_reduce(be_in, start, fin, L, np);
            row("f64", fin, be_in, start, L, np, p);
            g_seen.insert(Combo{p.kernel, p.shape, p.block, p.r, p.seqf, p.map, be_in, start});
          }
      for (int esz : {4, 2})
        for (int fin = 0; fin < 2; ++fin)
          for (int vec = 0; vec < 2; ++vec) row("nar", esz, fin, vec, L, np, plan_reduce_narrow(esz, fin, vec, L, np));
    }
  char rest[8];
  if (std::fgets(rest, sizeof rest, g_fix)) die("the fixture goes on after line " + std::to_string(g_line));
}

// b. -1: not stated
struct Pin {
  const char* what;
  int be_in, start, fin;
  int64_t maxL;
  int n_parts;
  int shape, block, r, seqf, map;
  int64_t grid;
};
static const int64_t M4 = 4194304;
static const Pin kPins[] = {
    {"config C: 16 x 4M native", 0, Z, 0, M4, 16, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 2048},
    {"config D: 64 x 4M big-endian", 1, Z, 0, M4, 64, IPLS_SHAPE_BIG, 1024, 16, 3, 0, 8192},
    {"8 x 4M big-endian", 1, Z, 0, M4, 8, IPLS_SHAPE_BIG, 1024, 16, 3, 2, 1024},
    {"ACCUM on D", 1, A, 0, M4, 64, IPLS_SHAPE_BIG, 1024, 8, 0, 0, 16384},
    {"1 x 4M native", 0, Z, 0, M4, 1, IPLS_SHAPE_HALF, 512, 16, 0, 0, 256},
    {"2 x 4M native", 0, Z, 0, M4, 2, IPLS_SHAPE_HALF, 512, 16, 0, 0, 512},
    {"3 x 4M native", 0, Z, 0, M4, 3, IPLS_SHAPE_HALF, 512, 16, 0, 0, 768},
    {"5 x 4M native", 0, Z, 0, M4, 5, IPLS_SHAPE_HALF, 512, 16, 0, 0, 1280},
    {"7 x 4M native", 0, Z, 0, M4, 7, IPLS_SHAPE_HALF, 512, 16, 0, 0, 1792},
    {"9 x 4M native", 0, Z, 0, M4, 9, IPLS_SHAPE_HALF, 512, 16, 0, 0, 2304},
    {"11 x 4M native", 0, Z, 0, M4, 11, IPLS_SHAPE_HALF, 512, 16, 0, 0, 2816},
    {"13 x 4M native", 0, Z, 0, M4, 13, IPLS_SHAPE_HALF, 512, 16, 0, 0, 3328},
    {"15 x 4M native", 0, Z, 0, M4, 15, IPLS_SHAPE_HALF, 512, 16, 0, 0, 3840},
    {"8 x 4M native", 0, Z, 0, M4, 8, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 1024},
    {"10 x 4M native", 0, Z, 0, M4, 10, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 1280},
    {"12 x 4M native", 0, Z, 0, M4, 12, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 1536},
    {"16 x 4M native, FIRST", 0, F, 0, M4, 16, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 2048},
    // the partial tile is not counted: 256 whole half tiles fill, and 257 blocks run
    {"1 x (4M + 3) native", 0, Z, 0, M4 + 3, 1, IPLS_SHAPE_HALF, 512, 16, 0, 3, 257},
    {"ETHModel: 3 x 147,872", 0, Z, 0, 147872, 3, IPLS_SHAPE_SMALL, 256, 1, 0, 0, 867},
    {"300 tiny partitions", 0, Z, 0, 5, 300, IPLS_SHAPE_SMALL, 256, 1, 0, 0, 300},
    {"300 tiny partitions, big-endian", 1, Z, 0, 5, 300, IPLS_SHAPE_SMALL, 256, 1, 0, 0, 300},
    {"500 tiny partitions", 0, Z, 0, 5, 500, IPLS_SHAPE_BIG, 1024, 16, 0, 0, 500},
    {"500 tiny partitions, big-endian", 1, Z, 0, 5, 500, IPLS_SHAPE_BIG, 1024, 16, 3, 2, 504},
};

static void pins() {
  for (const Pin& w : kPins) {
    const ReducePlan p = plan_reduce(w.be_in, w.start, w.fin, w.maxL, w.n_parts);
    if (p.kernel != (w.fin ? IPLS_KERNEL_ROUND : IPLS_KERNEL_REDUCE) || p.shape != w.shape || p.block != w.block ||
        p.r != w.r || p.seqf != w.seqf || p.map != w.map || p.grid != w.grid) {
      char b[200];
      std::snprintf(b, sizeof b, "%s: shape %d block %d r %d seqf %d map %d grid %lld", w.what, p.shape, p.block, p.r,
                    p.seqf, p.map, (long long)p.grid);
      die(b);
    }
    ++g_plans;
  }
}

// c. expected_combinations() of tests/test_gpu_wide_small.py, without be_out, plus small
static std::set<Combo> expected() {
  std::set<Combo> out;
  for (int fin = 0; fin < 2; ++fin)
    for (int be_in = 0; be_in < 2; ++be_in)
      for (int start : {Z, A, F}) {
        if (fin && start == F) continue;
        const int kernel = fin ? IPLS_KERNEL_ROUND : IPLS_KERNEL_REDUCE;
        out.insert(Combo{kernel, IPLS_SHAPE_SMALL, 256, 1, 0, 0, be_in, start});
        for (int shape : {IPLS_SHAPE_HALF, IPLS_SHAPE_BIG, IPLS_SHAPE_MID}) {
          if (fin && shape == IPLS_SHAPE_HALF && start == A) continue;
          int block, r, seqf = 0;   // variant()
          if (shape == IPLS_SHAPE_HALF) block = 512, r = 16;
          else if (shape == IPLS_SHAPE_BIG) block = 1024, r = start == A ? 8 : 16, seqf = (start != A && be_in) ? 3 : 0;
          else block = 256, r = (be_in || start == A) ? 8 : 16;
          for (int map : {0, 3, 2}) {
            if (map == 2 && !(shape == IPLS_SHAPE_BIG && be_in)) continue;
            out.insert(Combo{kernel, shape, block, r, seqf, map, be_in, start});
          }
        }
      }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: test_reduce_plan <tests/golden/reduce_plan_cases.txt>");
  g_fix = std::fopen(argv[1], "r");
  if (!g_fix) die(std::string("cannot open ") + argv[1]);
  sweep();
  std::fclose(g_fix);
  const long swept = g_plans;
  pins();
  const std::set<Combo> want = expected();
  for (const Combo& c : want)
    if (!g_seen.count(c))
      die("the grid never reaches kernel " + std::to_string(c[0]) + " shape " + std::to_string(c[1]) + " r " +
          std::to_string(c[3]) + " map " + std::to_string(c[5]) + " be_in " + std::to_string(c[6]) + " start " +
          std::to_string(c[7]));
  for (const Combo& c : g_seen)
    if (!want.count(c))
      die("unexpected: kernel " + std::to_string(c[0]) + " shape " + std::to_string(c[1]) + " block " +
          std::to_string(c[2]) + " r " + std::to_string(c[3]) + " seqf " + std::to_string(c[4]) + " map " +
          std::to_string(c[5]) + " be_in " + std::to_string(c[6]) + " start " + std::to_string(c[7]));
  std::printf("reduce_plan ok: %ld plans\n", swept);
  return 0;
}
