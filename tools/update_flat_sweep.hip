// update_flat_sweep.hip -- dev tool: k_update_flat (one launch over all
// partitions of a staged flat vector, ipls_agg_update_gradient_chunked) alone
// on the device, against the P per-partition k_split / k_split_narrow launches
// dev_update_gradient makes over the same DEV-resident vector, and its
// shifted-load form against the element-load form (the SHIFT template
// parameter) at the residues where they differ.  Outputs of the three are
// compared bit for bit before anything is timed.
// Shapes: ETHModel (443,610 values over 3 partitions, chunk 147,871: odd), 16
// partitions with an odd chunk (4,194,305) and with an even one (4,194,304).
// Formats: f64, big-endian f64, f32, f16, bf16.  Modes: ACCUM and into zero.
// Each figure is the median of 7 spans of REPS back-to-back launches between
// two events, with min and max; GB/s over the algorithmic bytes ((s + 16) per
// element ACCUM, (s + 8) into zero) and that as a fraction of 8 TB/s.
// tools/update_flat_probe.py runs it and keeps the output.
// Usage: update_flat_sweep [REPS]   (default 20)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ipls-java-api_amd/csrc/ipls_kernels.hpp"

using namespace ipls;

static unsigned blocks_for(int64_t n, int64_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

#define CK(x)                                                                          \
  do {                                                                                 \
    hipError_t e = (x);                                                                \
    if (e != hipSuccess) {                                                             \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e)); \
      exit(1);                                                                         \
    }                                                                                  \
  } while (0)

struct Shape {
  const char* name;
  int P;
  int64_t M;
};

struct Geo {
  int64_t chunk;
  std::vector<int64_t> len, off, acc_off;   // acc_off: 256-B aligned accumulator offsets (doubles)
  int64_t acc_total = 0, maxL = 0;
};

static Geo geometry(const Shape& s) {
  Geo g;
  g.chunk = s.M / s.P + 1;
  for (int i = 0; i < s.P; ++i) {
    const int64_t L = ((int64_t)(i + 1) * g.chunk > s.M) ? s.M - (int64_t)i * g.chunk + 1 : g.chunk + 1;
    g.len.push_back(L);
    g.off.push_back((int64_t)i * g.chunk);
    g.acc_off.push_back(g.acc_total);
    g.acc_total = (g.acc_total + L + 31) / 32 * 32;
    g.maxL = std::max(g.maxL, L);
  }
  return g;
}

template <class F>
static void timed(const char* shape, const char* fmt, const char* mode, const char* what, int reps, double bytes, F&& launch) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  launch();
  CK(hipDeviceSynchronize());
  std::vector<float> ms;
  for (int span = 0; span < 7; ++span) {
    CK(hipEventRecord(a));
    for (int r = 0; r < reps; ++r) launch();
    CK(hipEventRecord(b));
    CK(hipEventSynchronize(b));
    float t;
    CK(hipEventElapsedTime(&t, a, b));
    ms.push_back(t / reps);
  }
  CK(hipGetLastError());
  std::sort(ms.begin(), ms.end());
  const double gbs = bytes / (ms[3] * 1e-3) / 1e9;
  printf("%-10s %-5s %-6s %-22s median %8.4f ms  min %8.4f  max %8.4f  %8.1f GB/s  %5.1f %% of 8 TB/s\n", shape, fmt,
         mode, what, ms[3], ms[0], ms[6], gbs, gbs / 80.0);
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
}

// S: FmtD64 (BE: big-endian) or a trainer format
template <class S, bool BE>
static void run(const Shape& sh, const char* fmt, int reps) {
  typedef typename S::elem T;
  constexpr bool kWide = sizeof(T) == 8;
  const Geo g = geometry(sh);
  const size_t esz = sizeof(T);
  // the staged vector: 16 B of padding, then M elements
  char* d_raw;
  CK(hipMalloc(&d_raw, (size_t)sh.M * esz + 32));
  std::vector<T> hsrc((size_t)sh.M);
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (auto& v : hsrc) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    if constexpr (kWide) {
      double dv = (double)(int64_t)(x >> 20) * 1e-9;
      unsigned long long b;
      memcpy(&b, &dv, 8);
      v = BE ? __builtin_bswap64(b) : b;
    } else if constexpr (sizeof(T) == 4) {
      v = (float)(int)(x >> 44) * 1e-3f;
    } else {
      v = (T)(0x3c00 ^ (x >> 56));   // a normal number in either 16-bit format
    }
  }
  T* d_src = (T*)(d_raw + 16);
  CK(hipMemcpy(d_src, hsrc.data(), (size_t)sh.M * esz, hipMemcpyHostToDevice));
  unsigned long long* acc[3];
  std::vector<double> hinit((size_t)g.acc_total, 0.25);
  for (auto& a : acc) {
    CK(hipMalloc(&a, (size_t)g.acc_total * 8));
    CK(hipMemcpy(a, hinit.data(), (size_t)g.acc_total * 8, hipMemcpyHostToDevice));
  }
  const int64_t tile = flat_tile<S>();
  const dim3 grid(blocks_for(g.maxL, tile), (unsigned)sh.P);
  for (int zero = 0; zero < 2; ++zero) {
    FlatJob* d_jobs[3];
    for (int k = 0; k < 3; ++k) {
      std::vector<FlatJob> jobs((size_t)sh.P);
      for (int p = 0; p < sh.P; ++p)
        jobs[(size_t)p] = FlatJob{g.off[p], g.len[p] - 1, g.len[p], acc[k] + g.acc_off[p], zero};
      CK(hipMalloc(&d_jobs[k], jobs.size() * sizeof(FlatJob)));
      CK(hipMemcpy(d_jobs[k], jobs.data(), jobs.size() * sizeof(FlatJob), hipMemcpyHostToDevice));
    }
    auto flat_shift = [&] { hipLaunchKernelGGL((k_update_flat<S, BE, true>), grid, dim3(kBlock), 0, 0, d_jobs[0], d_src); };
    auto flat_plain = [&] { hipLaunchKernelGGL((k_update_flat<S, BE, false>), grid, dim3(kBlock), 0, 0, d_jobs[1], d_src); };
    auto splits = [&] {   // dev_update_gradient's launches
      for (int p = 0; p < sh.P; ++p) {
        const int64_t L = g.len[p], nc = L - 1;
        unsigned long long* a = acc[2] + g.acc_off[p];
        const bool vec = (((uintptr_t)(d_src + g.off[p])) & 15) == 0;
        const dim3 gg = vec ? dim3(std::max(1u, blocks_for(L, kEwTile))) : dim3(blocks_for(L, kBlock));
        if constexpr (kWide) {
          if (vec) {
            if (zero) hipLaunchKernelGGL((k_split<BE, false, 2, true>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
            else hipLaunchKernelGGL((k_split<BE, false, 1, true>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
          } else {
            if (zero) hipLaunchKernelGGL((k_split<BE, false, 2, false>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
            else hipLaunchKernelGGL((k_split<BE, false, 1, false>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
          }
        } else {
          if (vec) {
            if (zero) hipLaunchKernelGGL((k_split_narrow<S, false, 2, true>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
            else hipLaunchKernelGGL((k_split_narrow<S, false, 1, true>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
          } else {
            if (zero) hipLaunchKernelGGL((k_split_narrow<S, false, 2, false>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
            else hipLaunchKernelGGL((k_split_narrow<S, false, 1, false>), gg, dim3(kBlock), 0, 0, d_src, g.off[p], nc, L, a);
          }
        }
      }
    };
    // one launch of each from the same start: the three results must be the same bits
    for (auto& a : acc) CK(hipMemcpy(a, hinit.data(), (size_t)g.acc_total * 8, hipMemcpyHostToDevice));
    flat_shift(), flat_plain(), splits();
    CK(hipDeviceSynchronize());
    CK(hipGetLastError());
    std::vector<unsigned long long> h0((size_t)g.acc_total), h1(h0.size());
    CK(hipMemcpy(h0.data(), acc[0], h0.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 1; k < 3; ++k) {
      CK(hipMemcpy(h1.data(), acc[k], h1.size() * 8, hipMemcpyDeviceToHost));
      for (int p = 0; p < sh.P; ++p)
        if (memcmp(h0.data() + g.acc_off[p], h1.data() + g.acc_off[p], (size_t)g.len[p] * 8) != 0) {
          fprintf(stderr, "%s %s zero=%d: %s differs from the shifted form in partition %d\n", sh.name, fmt, zero,
                  k == 1 ? "the element-load form" : "k_split", p);
          exit(1);
        }
    }
    int64_t elems = 0;
    for (int p = 0; p < sh.P; ++p) elems += g.len[p];
    const double bytes = (double)elems * (esz + (zero ? 8 : 16));
    const char* mode = zero ? "zero" : "accum";
    timed(sh.name, fmt, mode, "k_update_flat shifted", reps, bytes, flat_shift);
    timed(sh.name, fmt, mode, "k_update_flat plain", reps, bytes, flat_plain);
    timed(sh.name, fmt, mode, "P k_split launches", reps, bytes, splits);
    for (auto& j : d_jobs) CK(hipFree(j));
  }
  for (auto& a : acc) CK(hipFree(a));
  CK(hipFree(d_raw));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 20;
  const Shape shapes[] = {{"ethmodel", 3, 443610}, {"16x4M-odd", 16, 16 * 4194304ll}, {"16x4M-even", 16, 16 * 4194303ll}};
  for (const Shape& s : shapes) {
    printf("# %s: P %d, M %lld, chunk %lld\n", s.name, s.P, (long long)s.M, (long long)(s.M / s.P + 1));
    run<FmtD64, false>(s, "f64", reps);
    run<FmtD64, true>(s, "be", reps);
    run<FmtF32, false>(s, "f32", reps);
    run<FmtF16, false>(s, "f16", reps);
    run<FmtBF16, false>(s, "bf16", reps);
    fflush(stdout);
  }
  return 0;
}
