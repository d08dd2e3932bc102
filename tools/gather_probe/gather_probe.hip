// gather_probe.hip — calibration of rocprofv3 FETCH_SIZE / WRITE_SIZE for the access widths of the
// check kernels (MI355X_MICROARCH.md §HBM: "Other access widths are uncalibrated: calibrate on a
// known byte count in your own access pattern"). Each kernel reads N random, aligned chunks of one
// width from a table far larger than the 256 MiB Infinity Cache (so nearly every chunk is a distinct
// HBM line) and writes one u32 per lane. Known bytes: N x width read, N x 4 written.
//   build: hipcc -O3 --offload-arch=gfx950 -o gather_probe gather_probe.hip
//   run:   rocprofv3 --pmc FETCH_SIZE -- ./gather_probe   (then WRITE_SIZE in a separate pass)
//
// ./gather_probe --two-table [out.json] — the closure join's access shape against two tables, to
// price the layout of the second one (resource fronts). A "check" is one random 64-B
// line of a 12.8 GB table (four lanes x 16 B, nontemporal: the user slot) and, in the same round,
// one random record of a 30 M-record table (the resource side) laid out as
//   a  64-B stride, first 32 B read (two lanes x 16 B): the join today, 1.92 GB
//   b  32-B stride, 32 B read: 0.96 GB
//   c  16-B stride, one lane x 16 B: 0.48 GB
//   at, bt, ct  the same three with a plain (temporal) load of the record, the user line still nontemporal
//   n  no random read at all: the ceiling of the launch path, to show the others are memory-bound
// Both ids come from the wave's streamed 640-B item block (32 checks x 20 B, staged through LDS as
// the join stages it), and 40 lanes store 4 B each (160 B per 32 checks). A launch is 65,536 checks
// (eight 32-check waves per CU); four streams keep four launches in flight; every launch reads its
// own item block out of a ring of 256, so no id pair repeats inside the Infinity Cache's window.
// Five repeats per case, the cases alternated. One JSON object with checks/s per case and repeat.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned long long mix(unsigned long long x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

template <int W>  // bytes per chunk: 4, 16, 32, 64
__global__ void __launch_bounds__(256) k_gather(const unsigned char* __restrict__ tab, unsigned long long n_chunks,
                                                unsigned seed, unsigned* __restrict__ out) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long c = mix((unsigned long long)i * 0x9E3779B97F4A7C15ull + seed) % n_chunks;
  const unsigned char* p = tab + c * W;
  unsigned acc = 0;
  if constexpr (W == 4) {
    acc = *reinterpret_cast<const unsigned*>(p);
  } else {
    const u64x2* q = reinterpret_cast<const u64x2*>(p);
#pragma unroll
    for (int k = 0; k < W / 16; ++k) {
      const u64x2 v = q[k];
      acc ^= (unsigned)v.x ^ (unsigned)(v.y >> 7);
    }
  }
  out[i] = acc;
}

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

// ---- two-table mode ------------------------------------------------------------------------------
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define GP_GLOBAL __attribute__((address_space(1)))  // global_load, not flat_load: as the join's slot loads
constexpr unsigned kChecks = 65536;          // per launch: 256 CUs x 8 waves x 32 checks
constexpr unsigned kRing = 256;              // item blocks (launches with ids of their own)
constexpr unsigned long long kUsers = 200000000ull, kDocs = 30000000ull;

// items[i] = {doc id, user id, 3 words of filler}: 20 B per check, as gck_item
__global__ void __launch_bounds__(256) k_items(unsigned* __restrict__ items, unsigned long long n) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long h = mix(i * 0x9E3779B97F4A7C15ull + 99u), g = mix(h + 0x632BE59BD9B4E019ull);
  unsigned* it = items + i * 5;
  it[0] = (unsigned)(g % kDocs);
  it[1] = (unsigned)(h % kUsers);
  it[2] = (unsigned)i, it[3] = 1u, it[4] = 2u;
}

__device__ __forceinline__ void lds_wave_fence() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

// MODE 0..2 = layouts a..c, 3 = n; NT: the record's load is nontemporal. One wave per 32 checks, 4 waves per block; n is a multiple of 128.
template <int MODE, bool NT>
__global__ void __launch_bounds__(256) k_two(const unsigned char* __restrict__ U, const unsigned char* __restrict__ D,
                                             const unsigned* __restrict__ items, unsigned* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned s_item[4][40 * 4];
  __shared__ unsigned long long s_ua[4][32], s_da[4][32];
  const unsigned wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned w0 = (blockIdx.x * 4 + wib) * 32;  // < kChecks (grid = kChecks / 128)
  if (lane < 40) *reinterpret_cast<u32x4*>(&s_item[wib][lane * 4]) = *reinterpret_cast<const u32x4*>(items + (size_t)w0 * 5 + lane * 4);
  lds_wave_fence();
  constexpr unsigned kStride = MODE == 0 ? 64 : MODE == 1 ? 32 : 16;
  if (lane < 32) {
    const unsigned doc = s_item[wib][lane * 5], usr = s_item[wib][lane * 5 + 1];  // < kDocs, < kUsers (k_items)
    s_ua[wib][lane] = (unsigned long long)(uintptr_t)(U + (size_t)usr * 64);
    s_da[wib][lane] = (unsigned long long)(uintptr_t)(D + (size_t)doc * kStride);
  }
  lds_wave_fence();
  u32x4 y[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  if constexpr (MODE != 3) {
#pragma unroll
    for (unsigned r = 0; r < 2; ++r)  // user line of check 16 r + lane / 4, chunk lane % 4
      y[r] = __builtin_nontemporal_load((const GP_GLOBAL u32x4*)(s_ua[wib][16 * r + (lane >> 2)] + (lane & 3) * 16));
    // 32 B of check lane / 2, chunk lane % 2; or the check's own 16-B record
    const GP_GLOBAL u32x4* p = MODE <= 1 ? (const GP_GLOBAL u32x4*)(s_da[wib][lane >> 1] + (lane & 1) * 16)
                                         : (const GP_GLOBAL u32x4*)s_da[wib][lane & 31];
    if (MODE <= 1 || lane < 32) {
      if constexpr (NT) y[2] = __builtin_nontemporal_load(p); else y[2] = *p;
    }
  } else {
    y[0].x = (unsigned)s_ua[wib][lane & 31] ^ (unsigned)s_da[wib][lane & 31];
  }
  unsigned acc = 0;
#pragma unroll
  for (unsigned r = 0; r < 3; ++r) acc ^= y[r].x + y[r].y * 3 + y[r].z * 5 + y[r].w * 7;
  acc ^= (unsigned)__shfl_xor((int)acc, 32, 64);
  if (lane < 40) out[(size_t)(w0 / 32) * 40 + lane] = acc;  // 160 B per wave
}

static int two_table(const char* json_path) {
  const size_t u_bytes = kUsers * 64, d_bytes = kDocs * 64;
  const size_t item_words = (size_t)kRing * kChecks * 5;
  unsigned char *U = nullptr, *D = nullptr;
  unsigned *items = nullptr, *out = nullptr;
  constexpr int kStreams = 4, kCases = 7, kReps = 5, kPerStream = 2048;  // 8,192 launches per repeat
  CK(hipMalloc(&U, u_bytes));
  CK(hipMalloc(&D, d_bytes));
  CK(hipMalloc(&items, item_words * 4));
  CK(hipMalloc(&out, (size_t)kStreams * (kChecks / 32) * 40 * 4));
  CK(hipMemset(U, 0x3C, u_bytes));
  CK(hipMemset(D, 0x5A, d_bytes));
  const unsigned long long n_items = (unsigned long long)kRing * kChecks;
  hipLaunchKernelGGL(k_items, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, 0, items, n_items);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  hipStream_t st[kStreams];
  for (auto& s : st) CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  static const char* names[kCases] = {"a_stride64_read32", "b_stride32_read32", "c_stride16_read16", "at_stride64_read32_temporal",
                                      "bt_stride32_read32_temporal", "ct_stride16_read16_temporal", "n_no_random_read"};
  auto launch = [&](int c, int s, unsigned blk) {
    const unsigned* it = items + (size_t)(blk % kRing) * kChecks * 5;
    unsigned* o = out + (size_t)s * (kChecks / 32) * 40;
    const dim3 g(kChecks / 128), b(256);
    switch (c) {
      case 0: hipLaunchKernelGGL((k_two<0, true>), g, b, 0, st[s], U, D, it, o); break;
      case 1: hipLaunchKernelGGL((k_two<1, true>), g, b, 0, st[s], U, D, it, o); break;
      case 2: hipLaunchKernelGGL((k_two<2, true>), g, b, 0, st[s], U, D, it, o); break;
      case 3: hipLaunchKernelGGL((k_two<0, false>), g, b, 0, st[s], U, D, it, o); break;
      case 4: hipLaunchKernelGGL((k_two<1, false>), g, b, 0, st[s], U, D, it, o); break;
      case 5: hipLaunchKernelGGL((k_two<2, false>), g, b, 0, st[s], U, D, it, o); break;
      default: hipLaunchKernelGGL((k_two<3, true>), g, b, 0, st[s], U, D, it, o); break;
    }
  };
  // one repeat: every stream's launches from a host thread of its own; wall time to the last one's end
  std::atomic<bool> failed{false};
  auto repeat = [&](int c, int per_stream) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int s = 0; s < kStreams; ++s)
      th.emplace_back([&, s] {
        for (int k = 0; k < per_stream; ++k) launch(c, s, (unsigned)(k * kStreams + s));
        if (hipStreamSynchronize(st[s]) != hipSuccess) failed = true;
      });
    for (auto& t : th) t.join();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  double rate[kCases][kReps], lo[kCases], hi[kCases], med[kCases];
  for (int c = 0; c < kCases && !failed; ++c) repeat(c, 64);  // warm-up (code objects, clocks)
  for (int r = 0; r < kReps && !failed; ++r)
    for (int c = 0; c < kCases && !failed; ++c) {
      const double sec = repeat(c, kPerStream);
      rate[c][r] = (double)kStreams * kPerStream * kChecks / sec;
    }
  CK(hipGetLastError());
  if (failed) {
    fprintf(stderr, "a launch failed\n");
    return 1;
  }
  FILE* f = json_path ? fopen(json_path, "w") : stdout;
  if (!f) {
    perror(json_path);
    return 1;
  }
  fprintf(f, "{\"checks_per_launch\": %u, \"launches_in_flight\": %d, \"launches_per_repeat\": %d, \"users\": %llu, \"docs\": %llu,\n \"cases\": {\n",
          kChecks, kStreams, kStreams * kPerStream, kUsers, kDocs);
  for (int c = 0; c < kCases; ++c) {
    double v[kReps];
    std::copy(rate[c], rate[c] + kReps, v);
    std::sort(v, v + kReps);
    lo[c] = v[0], hi[c] = v[kReps - 1], med[c] = v[kReps / 2];
    fprintf(f, "  \"%s\": {\"Gchecks_s\": [", names[c]);
    for (int r = 0; r < kReps; ++r) fprintf(f, "%s%.3f", r ? ", " : "", rate[c][r] * 1e-9);
    fprintf(f, "], \"median\": %.3f, \"min\": %.3f, \"max\": %.3f}%s\n", v[kReps / 2] * 1e-9, v[0] * 1e-9, v[kReps - 1] * 1e-9,
            c + 1 < kCases ? "," : "");
  }
  // the layout's go / no-go: c beats a by more than the larger of the two spreads — as the join
  // loads today (nontemporal), and with the record's load temporal in both
  auto verdict = [&](const char* key, int a, int c, const char* end) {
    const double spread = std::max(hi[a] - lo[a], hi[c] - lo[c]), gain = med[c] - med[a];
    fprintf(f, " \"%s\": {\"c_minus_a_median\": %.3f, \"larger_spread\": %.3f, \"c_over_a\": %.4f, \"c_beats_a\": %s}%s\n", key, gain * 1e-9,
            spread * 1e-9, med[c] / med[a], gain > spread ? "true" : "false", end);
  };
  fprintf(f, " },\n");
  verdict("nontemporal", 0, 2, ",");
  verdict("temporal", 3, 5, ",");
  verdict("temporal_c_vs_today_a", 0, 5, "");
  fprintf(f, "}\n");
  if (f != stdout) fclose(f);
  for (auto& s : st) CK(hipStreamDestroy(s));
  CK(hipFree(U));
  CK(hipFree(D));
  CK(hipFree(items));
  CK(hipFree(out));
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--two-table")) return two_table(argc > 2 ? argv[2] : nullptr);
  const size_t tab_bytes = (size_t)4 << 30;  // 4 GiB: 16x the Infinity Cache
  const unsigned n = 1u << 24;               // lanes per kernel
  unsigned char* tab = nullptr;
  unsigned* out = nullptr;
  CK(hipMalloc(&tab, tab_bytes));
  CK(hipMalloc(&out, (size_t)n * 4));
  CK(hipMemset(tab, 0x5A, tab_bytes));
  CK(hipDeviceSynchronize());
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  auto run = [&](auto kern, int width) {
    for (int rep = 0; rep < 3; ++rep) {
      CK(hipEventRecord(a, 0));
      hipLaunchKernelGGL(kern, dim3(n / 256), dim3(256), 0, 0, tab, tab_bytes / width, 1234u + rep, out);
      CK(hipEventRecord(b, 0));
      CK(hipEventSynchronize(b));
      float ms = 0.f;
      CK(hipEventElapsedTime(&ms, a, b));
      printf("{\"width\": %d, \"lanes\": %u, \"read_bytes\": %llu, \"write_bytes\": %llu, \"ms\": %.4f, \"GBps\": %.1f}\n",
             width, n, (unsigned long long)n * width, (unsigned long long)n * 4, ms, (double)n * width / (ms * 1e6));
    }
    return 0;
  };
  if (run(k_gather<4>, 4) || run(k_gather<16>, 16) || run(k_gather<32>, 32) || run(k_gather<64>, 64)) return 1;
  CK(hipFree(tab));
  CK(hipFree(out));
  return 0;
}
