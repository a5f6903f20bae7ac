// saved_model_sweep.hip -- dev tool: device rates of the saved-model kernels
// (ipls_kernels.hpp: k_ser_pack, k_ser_pack_boxed, k_ser_apply) against the
// aligned copy-shaped yardstick k_bswap64<VEC> over the same partitions, in one
// process.  Each figure is K back-to-back launches between two HIP events;
// every measurement is repeated REPS times round-robin and the minimum and
// maximum rates are printed, as one JSON line.
//
// Usage: saved_model_sweep P L K REPS      (default: config C, 16 x 4194304, 10, 5)
// Algorithmic bytes per value: pack 8 read + 8 written (+ framing), boxed
// pack 8 + 14, apply SET 8 + 8, apply BLEND 8 + 8 + 8, bswap 8 + 8.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../ipls-java-api_amd/csrc/ipls_kernels.hpp"

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e = (x);                                                                \
    if (e != hipSuccess) {                                                             \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

using namespace ipls;

int main(int argc, char** argv) {
  const int P = argc > 1 ? atoi(argv[1]) : 16;
  const int64_t L = argc > 2 ? atoll(argv[2]) : 4194304;
  const int K = argc > 3 ? atoi(argv[3]) : 10;
  const int REPS = argc > 4 ? atoi(argv[4]) : 5;
  if (P < 1 || P > 65535 || L < 2 || K < 1 || REPS < 1) return 2;
  const int64_t stride = (L + 31) / 32 * 32;   // accumulators 256-B aligned, as in the arena

  // the MAP image: entry 0 after 181 framing bytes, later entries after 20; one end byte
  std::vector<SerPackJob> pack((size_t)P), box((size_t)P);
  std::vector<SerApplyJob> apply((size_t)P);
  double *arena = nullptr, *dst = nullptr;
  CK(hipMalloc(&arena, (size_t)P * stride * 8));
  CK(hipMalloc(&dst, (size_t)P * stride * 8));
  CK(hipMemset(arena, 0x3c, (size_t)P * stride * 8));
  CK(hipMemset(dst, 0x3c, (size_t)P * stride * 8));
  int64_t map_bytes = 0, box_bytes = 0;
  for (int p = 0; p < P; ++p) {
    SerPackJob& j = pack[(size_t)p];
    j = SerPackJob{};
    j.src = (const unsigned long long*)(arena + p * stride);
    j.n = L;
    j.pos = map_bytes;
    j.prefix_len = p == 0 ? 181 : 20;
    j.suffix = p + 1 == P ? 0x78 : -1;
    apply[(size_t)p] = SerApplyJob{dst + p * stride, L, j.pos + j.prefix_len};
    map_bytes += j.prefix_len + 8 * L + (j.suffix >= 0 ? 1 : 0);
    SerPackJob& b = box[(size_t)p];
    b = j;
    b.pos = box_bytes;
    b.prefix_len = p == 0 ? 129 : 6;
    box_bytes += b.prefix_len + 14 * L - 6 + (b.suffix >= 0 ? 1 : 0);
  }
  unsigned char *img = nullptr, *bimg = nullptr;
  SerPackJob *dpack = nullptr, *dbox = nullptr;
  SerApplyJob* dapply = nullptr;
  CK(hipMalloc(&img, (size_t)map_bytes + 32));
  CK(hipMalloc(&bimg, (size_t)box_bytes + 32));
  CK(hipMalloc(&dpack, pack.size() * sizeof(SerPackJob)));
  CK(hipMalloc(&dbox, box.size() * sizeof(SerPackJob)));
  CK(hipMalloc(&dapply, apply.size() * sizeof(SerApplyJob)));
  CK(hipMemcpy(dpack, pack.data(), pack.size() * sizeof(SerPackJob), hipMemcpyHostToDevice));
  CK(hipMemcpy(dbox, box.data(), box.size() * sizeof(SerPackJob), hipMemcpyHostToDevice));
  CK(hipMemcpy(dapply, apply.data(), apply.size() * sizeof(SerApplyJob), hipMemcpyHostToDevice));

  auto blocks = [](int64_t n, int64_t per) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 16384)); };
  const dim3 gp(blocks(8 * L / 16 + 1, kSerTileWords), (unsigned)P), gb(blocks((14 * L - 6) / 16 + 1, kSerTileWords), (unsigned)P),
      ga(blocks(L / 2 + 1, kSerTileWords), (unsigned)P);
  struct Var {
    std::string name;
    double bytes;
    std::function<void()> launch;
    double lo = 1e30, hi = 0;
  };
  std::vector<Var> vars;
  vars.push_back({"pack", 8.0 * P * L + (double)map_bytes,
                  [&]() { hipLaunchKernelGGL(k_ser_pack, gp, dim3(kBlock), 0, 0, dpack, img); }});
  vars.push_back({"pack_boxed", 8.0 * P * L + (double)box_bytes,
                  [&]() { hipLaunchKernelGGL(k_ser_pack_boxed, gb, dim3(kBlock), 0, 0, dbox, bimg); }});
  vars.push_back({"apply_set", 16.0 * P * L,
                  [&]() { hipLaunchKernelGGL(k_ser_apply<false>, ga, dim3(kBlock), 0, 0, dapply, img, 0.6, 0.4); }});
  vars.push_back({"apply_blend", 24.0 * P * L,
                  [&]() { hipLaunchKernelGGL(k_ser_apply<true>, ga, dim3(kBlock), 0, 0, dapply, img, 0.6, 0.4); }});
  vars.push_back({"bswap_yardstick", 16.0 * P * L, [&]() {
                    for (int p = 0; p < P; ++p)
                      hipLaunchKernelGGL(k_bswap64<true>, dim3((unsigned)((L + kEwTile - 1) / kEwTile)), dim3(kBlock), 0, 0,
                                         (const unsigned long long*)(arena + p * stride),
                                         (unsigned long long*)(dst + p * stride), L);
                  }});
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (auto& v : vars) v.launch();   // warm-up: code objects, pages
  CK(hipDeviceSynchronize());
  for (int r = 0; r < REPS; ++r)
    for (auto& v : vars) {
      CK(hipEventRecord(e0, 0));
      for (int k = 0; k < K; ++k) v.launch();
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double gbs = v.bytes * K / (ms * 1e-3) / 1e9;
      v.lo = std::min(v.lo, gbs);
      v.hi = std::max(v.hi, gbs);
    }
  printf("{\"P\": %d, \"L\": %lld, \"K\": %d, \"reps\": %d", P, (long long)L, K, REPS);
  for (auto& v : vars) printf(", \"%s_gbs\": [%.1f, %.1f]", v.name.c_str(), v.lo, v.hi);
  printf("}\n");
  return 0;
}
