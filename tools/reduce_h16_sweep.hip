// reduce_h16_sweep.hip -- dev tool: time k_reduce_narrow shapes over 16-bit buckets on one MI355X.
//
// Usage: reduce_h16_sweep P L K REPS [half|bf16]
// Allocates P*K 16-bit buckets of L elements (16-B aligned), fills them with
// (2u-1)*1e-2 from splitmix64 narrowed to the format and 1.0 in the count
// slot, then times every (layout, lanes, vectors per lane, next-peer prefetch)
// variant of k_reduce_narrow REPS times, interleaved round-robin in one process,
// START_ZERO into native doubles.  Layout A: 8-B loads, 4 elements per lane,
// the lane^4 swap of the float fold; layout B: 16-B loads, 8 elements per lane, the
// pair transpose across 8 lanes; Aplain / Bplain: the same without any exchange
// between lanes (half- and quarter-line stores).  Sum slots are 128-B aligned
// like the library's arena.  Reports the median and minimum kernel time
// (hipEvents, one launch per sample after a warm-up launch) and the fraction
// of 8 TB/s over the algorithmic bytes (2K + 8) * L * P.  Every variant's sums
// are compared with the first one's (exact 64-bit compare of partition 0 and
// P-1).
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

template <class H>
__global__ __launch_bounds__(256) void k_fill16(unsigned short* dst, int64_t L, unsigned long long seed) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const double u = (double)(splitmix64(seed ^ (unsigned long long)i) >> 11) * 0x1.0p-53;
    dst[i] = (unsigned short)H::narrow(i == L - 1 ? 1.0f : (float)((2.0 * u - 1.0) * 1e-2));
  }
}

struct Variant {
  std::string name;
  int64_t tile;
  std::function<void(int64_t tpp, bool partial)> launch;
  std::vector<float> ms;
};

template <class H>
int run(int P, int64_t L, int K, int reps, const char* fmt) {
  // bucket slots 16-B aligned (what the kernel needs), sum slots 128-B aligned like the library's arena, so that
  // whole-line stores are whole lines here too
  const int64_t s16 = (L + 7) / 8 * 8 + 64, s64 = (L + 15) / 16 * 16 + 32;
  unsigned short* src;
  unsigned long long* dst;
  CK(hipMalloc(&src, (size_t)P * K * s16 * 2));
  CK(hipMalloc(&dst, (size_t)P * s64 * 8));
  std::vector<const unsigned short*> hb((size_t)P * K);
  std::vector<PartDesc> hp(P);
  for (int q = 0; q < P; ++q) {
    hp[q] = PartDesc{L, dst + (size_t)q * s64, nullptr, nullptr, nullptr};
    for (int j = 0; j < K; ++j) {
      hb[(size_t)q * K + j] = src + ((size_t)q * K + j) * s16;
      hipLaunchKernelGGL(k_fill16<H>, dim3(2048), dim3(256), 0, 0, src + ((size_t)q * K + j) * s16, L,
                         0x1B52026ULL ^ ((unsigned long long)q << 40) ^ ((unsigned long long)j << 32));
    }
  }
  CK(hipGetLastError());
  const unsigned short** dbufs;
  PartDesc* dparts;
  CK(hipMalloc(&dbufs, hb.size() * sizeof(void*)));
  CK(hipMalloc(&dparts, hp.size() * sizeof(PartDesc)));
  CK(hipMemcpy(dbufs, hb.data(), hb.size() * sizeof(void*), hipMemcpyHostToDevice));
  CK(hipMemcpy(dparts, hp.data(), hp.size() * sizeof(PartDesc), hipMemcpyHostToDevice));
  CK(hipDeviceSynchronize());

  std::vector<Variant> vs;
#define VAR(LAY, E, BS, R, PF) VARX(LAY, E, BS, R, PF, 1)
#define VARX(LAY, E, BS, R, PF, XP)                                                                                     \
  vs.push_back(Variant{#LAY "_bs" #BS "_r" #R "_pf" #PF, (int64_t)BS * E * R, [=](int64_t tpp, bool partial) {     \
                         const dim3 g((unsigned)(tpp * P));                                                        \
                         if (partial)                                                                              \
                           hipLaunchKernelGGL((k_reduce_narrow<H, false, kZero, R, BS, 3, true, PF, E, XP>), g, dim3(BS), \
                                              0, 0, (const unsigned short* const*)dbufs, dparts, K, (int)tpp, P);  \
                         else                                                                                      \
                           hipLaunchKernelGGL((k_reduce_narrow<H, false, kZero, R, BS, 0, true, PF, E, XP>), g, dim3(BS), \
                                              0, 0, (const unsigned short* const*)dbufs, dparts, K, (int)tpp, P);  \
                       }, {}})
  VAR(A, 4, 256, 4, 1);
  VAR(A, 4, 512, 2, 1);
  VAR(A, 4, 512, 4, 1);
  VAR(A, 4, 1024, 2, 1);
  VAR(A, 4, 1024, 4, 1);
  VAR(A, 4, 1024, 2, 0);
  VAR(A, 4, 1024, 4, 0);
  VAR(B, 8, 256, 1, 1);
  VAR(B, 8, 256, 2, 1);
  VAR(B, 8, 512, 1, 1);
  VAR(B, 8, 512, 2, 1);
  VAR(B, 8, 1024, 1, 1);
  VAR(B, 8, 1024, 2, 1);
  VAR(B, 8, 512, 2, 0);
  VAR(B, 8, 1024, 1, 0);
  VAR(B, 8, 1024, 2, 0);
  VARX(Aplain, 4, 512, 2, 1, 0);      // the two best shapes without the exchange between lanes
  VARX(Bplain, 8, 1024, 2, 1, 0);
#undef VARX
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
  const double bytes = (2.0 * K + 8.0) * (double)L * P;
  printf("%s P=%d L=%lld K=%d reps=%d algorithmic bytes=%.0f\n", fmt, P, (long long)L, K, reps, bytes);
  for (Variant& v : vs) {
    std::sort(v.ms.begin(), v.ms.end());
    const float med = v.ms[v.ms.size() / 2], mn = v.ms[0];
    printf("%-16s tile %7lld  median %.4f ms (%.1f %% of 8 TB/s)  min %.4f ms (%.1f %%)\n", v.name.c_str(),
           (long long)v.tile, med, bytes / (med * 1e-3) / 8e12 * 100, mn, bytes / (mn * 1e-3) / 8e12 * 100);
  }
  return 0;
}

int main(int argc, char** argv) {
  const int P = argc > 1 ? atoi(argv[1]) : 16;
  const int64_t L = argc > 2 ? atoll(argv[2]) : 4194305;
  const int K = argc > 3 ? atoi(argv[3]) : 32;
  const int reps = argc > 4 ? atoi(argv[4]) : 7;
  const char* fmt = argc > 5 ? argv[5] : "bf16";
  if (!strcmp(fmt, "half")) return run<FmtF16>(P, L, K, reps, fmt);
  return run<FmtBF16>(P, L, K, reps, fmt);
}
