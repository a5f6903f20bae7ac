// fuzz_saved_model.cpp -- the saved-model parsers (ipls-java-api_amd/csrc/
// javaser.cpp: HashMap<Integer,double[]>, double[], ArrayList<Double>) under
// AddressSanitizer + UBSan on the host.  The corpus of tests/test_saved_model.py:
// every truncation and every single-byte mutation (all 255 other values) of a
// small stream of each shape, each in a heap copy of exactly its length; an
// accepted parse has its whole table walked and every payload byte read.
// Built and run by tests/test_saved_model.py (g++ -fsanitize=address,undefined).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "javaser.hpp"

using namespace ipls::javaser;

namespace {

std::vector<uint8_t> make_map(const std::vector<int32_t>& parts, const std::vector<int32_t>& lens) {
  std::vector<int32_t> order;
  int32_t buckets, threshold;
  saved_shape(parts.data(), (int)parts.size(), order, &buckets, &threshold);
  std::vector<uint8_t> out;
  if (order.empty()) {
    out.resize(kSavedPrefixMax);
    out.resize((size_t)saved_empty(out.data()));
    return out;
  }
  for (size_t e = 0; e < order.size(); ++e) {
    size_t at = 0;
    while (parts[at] != order[e]) ++at;
    uint8_t pre[kSavedPrefixMax];
    const int64_t pl = saved_entry_prefix(pre, e == 0, threshold, buckets, (int32_t)order.size(), order[e], lens[at]);
    out.insert(out.end(), pre, pre + pl);
    for (int i = 0; i < 8 * lens[at]; ++i) out.push_back(uint8_t(i * 29 + 7 * (int)e));
  }
  out.push_back(0x78);
  return out;
}

std::vector<uint8_t> make_darr(int32_t n) {
  std::vector<uint8_t> out((size_t)kDarrHeader);
  darr_header(out.data(), n);
  for (int i = 0; i < 8 * n; ++i) out.push_back(uint8_t(i * 31));
  return out;
}

std::vector<uint8_t> make_dlist(int32_t n) {
  static const uint8_t lead[6] = {0x73, 0x71, 0x00, 0x7E, 0x00, 0x02};
  std::vector<uint8_t> out((size_t)kSavedPrefixMax);
  out.resize((size_t)dlist_header(out.data(), n));
  for (int32_t i = 0; i < n; ++i) {
    if (i) out.insert(out.end(), lead, lead + 6);
    for (int k = 0; k < 8; ++k) out.push_back(uint8_t(i * 8 + k));
  }
  out.push_back(0x78);
  return out;
}

long accepted = 0, rejected = 0;
volatile unsigned sink;

// One input through all three parsers, from a heap block of exactly its size.
void feed(const std::vector<uint8_t>& b) {
  std::vector<uint8_t> heap(b);   // ASan: a read past heap.size() is reported
  const uint8_t* p = heap.data();
  const int64_t n = (int64_t)heap.size();
  const char* why = nullptr;
  int32_t keys[8];
  int64_t lens[8], offs[8];
  const int64_t m = parse_saved(p, n, keys, lens, offs, 8, &why);
  if (m >= 0) {
    for (int64_t e = 0; e < m && e < 8; ++e)
      for (int64_t k = 0; k < 8 * lens[e]; ++k) sink += p[offs[e] + k];
    ++accepted;
  } else {
    ++rejected;
  }
  int64_t off = 0;
  const int64_t d = parse_darr(p, n, &off, &why);
  if (d >= 0)
    for (int64_t k = 0; k < 8 * d; ++k) sink += p[off + k];
  (d >= 0 ? accepted : rejected)++;
  const int64_t l = parse_dlist(p, n, &why);
  if (l > 0)
    for (int64_t k = 0; k < 8; ++k) sink += p[kDlistFirst + kDlistRecord * (l - 1) + k];
  (l >= 0 ? accepted : rejected)++;
}

}  // namespace

int main() {
  const std::vector<std::vector<uint8_t>> seeds = {
      make_map({3, 19}, {2, 3}), make_map({16, 0, 5}, {0, 1, 2}), make_map({}, {}), make_map({7}, {0}),
      make_darr(0), make_darr(3), make_dlist(0), make_dlist(1), make_dlist(3)};
  // the seeds themselves parse, as what they are
  {
    const char* why = nullptr;
    int32_t keys[8];
    int64_t lens[8], offs[8], off;
    if (parse_saved(seeds[0].data(), (int64_t)seeds[0].size(), keys, lens, offs, 8, &why) != 2 || keys[0] != 3 ||
        keys[1] != 19 || lens[0] != 2 || lens[1] != 3 || offs[0] != 181 || offs[1] != 181 + 16 + 20 ||
        parse_saved(seeds[2].data(), (int64_t)seeds[2].size(), keys, lens, offs, 8, &why) != 0 || seeds[2].size() != 82 ||
        parse_darr(seeds[5].data(), (int64_t)seeds[5].size(), &off, &why) != 3 || off != 27 ||
        parse_dlist(seeds[8].data(), (int64_t)seeds[8].size(), &why) != 3 || seeds[8].size() != 129 + 8 + 28 + 1) {
      std::printf("FAIL valid stream: %s\n", why ? why : "?");
      return 1;
    }
  }
  for (const auto& good : seeds) {
    for (size_t cut = 0; cut < good.size(); ++cut) feed(std::vector<uint8_t>(good.begin(), good.begin() + cut));
    for (size_t i = 0; i < good.size(); ++i)
      for (int v = 0; v < 256; ++v) {
        if (v == good[i]) continue;
        std::vector<uint8_t> b(good);
        b[i] = uint8_t(v);
        feed(b);
      }
  }
  std::mt19937_64 rng(4242);
  for (int it = 0; it < 20000; ++it) {   // several flips, sometimes cut short
    std::vector<uint8_t> b(seeds[rng() % seeds.size()]);
    const int flips = 1 + int(rng() % 6);
    for (int k = 0; k < flips; ++k) b[rng() % b.size()] = uint8_t(rng());
    if (rng() % 4 == 0) b.resize(rng() % (b.size() + 1));
    feed(b);
  }
  std::printf("fuzz ok: %ld accepted, %ld rejected\n", accepted, rejected);
  return 0;
}
