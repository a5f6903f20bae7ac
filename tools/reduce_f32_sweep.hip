// reduce_f32_sweep.hip -- dev tool: time k_reduce_narrow shapes over float buckets on one MI355X.
//
// Usage: reduce_f32_sweep P L K REPS
// Allocates P*K float buckets of L elements (16-B aligned), fills them with
// (2u-1)*1e-2 from splitmix64 and 1.0f in the count slot, then times every
// (lanes, vectors per lane, next-peer prefetch) variant of k_reduce_narrow<FmtF32> REPS times,
// interleaved round-robin in one process, START_ZERO into native doubles.
// Reports the median and minimum kernel time (hipEvents, one launch per
// sample after a warm-up launch) and the fraction of 8 TB/s over the
// algorithmic bytes (4K + 8) * L * P.  Every variant's sums are compared
// with the first one's (exact 64-bit compare of partition 0 and P-1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../ipls-java-api_amd/csrc/ipls_kernels.hpp"

using namespace ipls;

#define CK(x)                                                                     \
  do {                                                                            \
    hipError_t e = (x);                                                           \
    if (e != hipSuccess) {                                                        \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e)); \
      exit(1);                                                                    \
    }                                                                             \
  } while (0)

__global__ __launch_bounds__(256) void k_fill32(float* dst, int64_t L, unsigned long long seed) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const double u = (double)(splitmix64(seed ^ (unsigned long long)i) >> 11) * 0x1.0p-53;
    dst[i] = i == L - 1 ? 1.0f : (float)((2.0 * u - 1.0) * 1e-2);
  }
}

struct Variant {
  std::string name;
  int64_t tile;
  std::function<void(int64_t tpp, bool partial)> launch;
  std::vector<float> ms;
};

int main(int argc, char** argv) {
  const int P = argc > 1 ? atoi(argv[1]) : 16;
  const int64_t L = argc > 2 ? atoll(argv[2]) : 4194305;
  const int K = argc > 3 ? atoi(argv[3]) : 32;
  const int reps = argc > 4 ? atoi(argv[4]) : 7;
  const int64_t s32 = (L + 3) / 4 * 4 + 64, s64 = (L + 1) / 2 * 2 + 32;
  float* src;
  unsigned long long* dst;
  CK(hipMalloc(&src, (size_t)P * K * s32 * 4));
  CK(hipMalloc(&dst, (size_t)P * s64 * 8));
  std::vector<const float*> hb((size_t)P * K);
  std::vector<PartDesc> hp(P);
  for (int q = 0; q < P; ++q) {
    hp[q] = PartDesc{L, dst + (size_t)q * s64, nullptr, nullptr, nullptr};
    for (int j = 0; j < K; ++j) {
      hb[(size_t)q * K + j] = src + ((size_t)q * K + j) * s32;
      hipLaunchKernelGGL(k_fill32, dim3(2048), dim3(256), 0, 0, src + ((size_t)q * K + j) * s32, L,
                         0x1B52026ULL ^ ((unsigned long long)q << 40) ^ ((unsigned long long)j << 32));
    }
  }
  CK(hipGetLastError());
  const float** dbufs;
  PartDesc* dparts;
  CK(hipMalloc(&dbufs, hb.size() * sizeof(float*)));
  CK(hipMalloc(&dparts, hp.size() * sizeof(PartDesc)));
  CK(hipMemcpy(dbufs, hb.data(), hb.size() * sizeof(float*), hipMemcpyHostToDevice));
  CK(hipMemcpy(dparts, hp.data(), hp.size() * sizeof(PartDesc), hipMemcpyHostToDevice));
  CK(hipDeviceSynchronize());

  std::vector<Variant> vs;
#define VAR(BS, R, PF)                                                                                        \
  vs.push_back(Variant{"bs" #BS "_r" #R "_pf" #PF, (int64_t)BS * 4 * R, [=](int64_t tpp, bool partial) {             \
                         const dim3 g((unsigned)(tpp * P));                                                 \
                         if (partial)                                                                       \
                           hipLaunchKernelGGL((k_reduce_narrow<FmtF32, false, kZero, R, BS, 3, true, PF>), g, dim3(BS), 0, 0, \
                                              (const float* const*)dbufs, dparts, K, (int)tpp, P);          \
                         else                                                                               \
                           hipLaunchKernelGGL((k_reduce_narrow<FmtF32, false, kZero, R, BS, 0, true, PF>), g, dim3(BS), 0, 0, \
                                              (const float* const*)dbufs, dparts, K, (int)tpp, P);          \
                       }, {}})
  VAR(256, 2, 0);
  VAR(256, 4, 0);
  VAR(256, 8, 0);
  VAR(512, 4, 0);
  VAR(512, 8, 0);
  VAR(512, 16, 0);
  VAR(1024, 4, 0);
  VAR(1024, 8, 0);
  VAR(256, 2, 1);
  VAR(256, 4, 1);
  VAR(256, 8, 1);
  VAR(512, 2, 1);
  VAR(512, 4, 1);
  VAR(512, 8, 1);
  VAR(1024, 2, 1);
  VAR(1024, 4, 1);
#undef VAR
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<unsigned long long> ref(2 * L), got(2 * L);
  for (int r = -1; r < reps; ++r) {
    for (size_t i = 0; i < vs.size(); ++i) {
      Variant& v = vs[i];
      const int64_t tpp = (L + v.tile - 1) / v.tile;
      const bool partial = tpp > 1 && L % v.tile != 0;
      if (r < 0) CK(hipMemset(dst, 0xff, (size_t)P * s64 * 8));
      CK(hipEventRecord(e0, 0));
      v.launch(tpp, partial);
      CK(hipEventRecord(e1, 0));
      CK(hipGetLastError());
      CK(hipEventSynchronize(e1));
      if (r < 0) {   // warm-up pass: also the exactness check
        std::vector<unsigned long long>& o = i == 0 ? ref : got;
        CK(hipMemcpy(o.data(), dst, (size_t)L * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(o.data() + L, dst + (size_t)(P - 1) * s64, (size_t)L * 8, hipMemcpyDeviceToHost));
        if (i > 0 && memcmp(ref.data(), got.data(), (size_t)2 * L * 8) != 0) {
          fprintf(stderr, "%s differs from %s\n", v.name.c_str(), vs[0].name.c_str());
          return 1;
        }
        continue;
      }
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      v.ms.push_back(ms);
    }
  }
  const double bytes = (4.0 * K + 8.0) * (double)L * P;
  printf("P=%d L=%lld K=%d reps=%d algorithmic bytes=%.0f\n", P, (long long)L, K, reps, bytes);
  for (Variant& v : vs) {
    std::sort(v.ms.begin(), v.ms.end());
    const float med = v.ms[v.ms.size() / 2], mn = v.ms[0];
    printf("%-12s tile %7lld  median %.4f ms (%.1f %% of 8 TB/s)  min %.4f ms (%.1f %%)\n", v.name.c_str(),
           (long long)v.tile, med, bytes / (med * 1e-3) / 8e12 * 100, mn, bytes / (mn * 1e-3) / 8e12 * 100);
  }
  return 0;
}
