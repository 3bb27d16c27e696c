// Device time per launch of the headline confusion-matrix update over a 406 MB input ring (26 x 8192 x 1000 bf16,
// larger than the 256 MB MALL, as bench.py streams it), back-to-back launches timed with HIP events.
// Variants isolate the costs: empty launch, pure streaming read, the ordinal argmax with the int64 atomic / a label
// store / an int32 atomic, the raw-bit reductions (vlean), and launch shapes (one row per wave vs two; 256 / 512 / 1024
// threads).  Two rings: randn-like rows and all-negative (log-softmax-like) rows.  Every variant is timed five times
// (median, min, max); the raw-bit variants' labels are first checked against the ordinal reduction's.
// Build: hipcc -O3 --offload-arch=gfx950 confmat_ring_mb.hip -o confmat_ring_mb
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <chrono>

#define CK(x)                                                               \
  do {                                                                      \
    hipError_t e = (x);                                                     \
    if (e != hipSuccess) {                                                  \
      std::printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

__global__ void empty_kernel(int* p) {
  if (p == nullptr && threadIdx.x == 1234) *p = 0;
}

// pure read floor: each wave reads rows (kPer x 16 B per lane), xor-folds them, writes nothing
template <int kPer, int kRowsPerWave>
__global__ void __launch_bounds__(1024) vread(const uint16_t* __restrict__ preds, int N, int C, int* __restrict__ sink) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int nchunks = C / 8;
  uint32_t x = 0;
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wave * kRowsPerWave + r;
    if (row >= N) break;
    const u32x4* rp = reinterpret_cast<const u32x4*>(preds + (long long)row * C);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int ci = lane + j * 64;
      if (ci < nchunks) {
        const u32x4 v = __builtin_nontemporal_load(rp + ci);
        x ^= v[0] ^ v[1] ^ v[2] ^ v[3];
      }
    }
  }
  if (x == 0x12345678u) sink[0] = x;
}

// as in stat_scores.hip: the device library's DPP reduction, without __reduce_max_sync's xors and mask check
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return __ockl_wfred_max_u32(v); }
// the form the ordinal kernel was measured with before (kept for ord_row, the baseline of every comparison here)
__device__ __forceinline__ uint32_t wave_max_u32_sync(uint32_t v) {
  return static_cast<uint32_t>(__reduce_max_sync(~0ull, static_cast<int>(v ^ 0x80000000u))) ^ 0x80000000u;
}

// the ordinal row reduction of mc_argmax_ord16_kernel (csrc/classification/stat_scores.hip) without its NaN / +-0 test
template <int kPer>
__device__ __forceinline__ int ord_row(const u32x4 (&buf)[kPer], int lane, int nchunks) {
  u16x2 mx = {0, 0};
  uint32_t ordw[kPer][4];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int ci = lane + j * 64;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = buf[j][k];
      const s16x2 sw = __builtin_bit_cast(s16x2, w);
      const uint32_t sgn = __builtin_bit_cast(uint32_t, static_cast<s16x2>(sw >> (s16x2){15, 15}));
      const uint32_t o = w ^ (sgn | 0x80008000u);
      ordw[j][k] = o;
      if (ci < nchunks) mx = __builtin_elementwise_max(mx, __builtin_bit_cast(u16x2, o));
    }
  }
  const uint32_t lmax = mx.x > mx.y ? mx.x : mx.y;
  uint32_t first = 0xffffu;
#pragma unroll
  for (int j = kPer - 1; j >= 0; --j) {
    const int ci = lane + j * 64;
    if (ci < nchunks) {
#pragma unroll
      for (int k = 3; k >= 0; --k) {
        const uint32_t o = ordw[j][k];
        if ((o >> 16) == lmax) first = ci * 8 + 2 * k + 1;
        if ((o & 0xffffu) == lmax) first = ci * 8 + 2 * k;
      }
    }
  }
  const uint32_t key = wave_max_u32_sync((lmax << 16) | (0xffffu - first));
  return 0xffff - static_cast<int>(key & 0xffffu);
}

// kMode 0: int64 atomic into confmat, 1: label store only, 2: int32 atomic
template <int kMode>
__device__ __forceinline__ void emit(long long t, int bidx, int row, int C, unsigned long long* __restrict__ out,
                                     int* __restrict__ lab) {
  if (kMode == 0) atomicAdd(out + t * C + bidx, 1ull);
  else if (kMode == 1) lab[row] = bidx;
  else atomicAdd(reinterpret_cast<unsigned int*>(out) + t * C + bidx, 1u);
}

// production-style ordinal argmax, all rows of a wave's share loaded up front
template <int kPer, int kRowsPerWave, int kMode>
__global__ void __launch_bounds__(1024) vord(const uint16_t* __restrict__ preds, const int64_t* __restrict__ target,
                                            int N, int C, unsigned long long* __restrict__ out,
                                            int* __restrict__ lab) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int nchunks = C / 8;
  u32x4 buf[kRowsPerWave][kPer];
  long long t[kRowsPerWave];
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wave * kRowsPerWave + r;
    const u32x4* rp = reinterpret_cast<const u32x4*>(preds + (long long)(row < N ? row : 0) * C);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int ci = lane + j * 64;
      if (ci < nchunks) buf[r][j] = __builtin_nontemporal_load(rp + ci);
    }
    t[r] = lane == 0 && row < N ? target[row] : 0;
  }
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    const int row = wave * kRowsPerWave + r;
    if (row >= N) break;
    const int bidx = ord_row<kPer>(buf[r], lane, nchunks);
    if (lane == 0) emit<kMode>(t[r], bidx, row, C, out, lab);
  }
}

__device__ __forceinline__ uint32_t pk_nonzero_u16(uint32_t x) {  // 1 in each half that is not 0
  uint32_t t;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(t) : "v"(x), "s"(0x00010001u));
  return t;
}

// The lean reduction on raw bf16 bit patterns (wave_argmax_raw16 in stat_scores.hip), one row per wave, no loop:
// packed signed max + packed unsigned max per word (+ packed unsigned min with kNegMin, which serves all-negative rows
// here; without it they go to ord_row).  kScan 0: wave max first, then a per-lane no-match mask written as min(x, 1)
// (which the compiler turns into compares and selects, 7 ops a word) and a wave min of the first column; kScan 1:
// per-lane compare scan against the lane max and ONE wave max over (max << 16 | 0xffff - column), all-negative rows
// to ord_row; kScan 2 (needs kNegMin): the shipped form.  Lanes past the row's end hold the last chunk again.
template <int kPer, int kScan, bool kNegMin, int kMode>
__global__ void __launch_bounds__(1024) vlean(const uint16_t* __restrict__ preds, const int64_t* __restrict__ target,
                                             int N, int C, unsigned long long* __restrict__ out,
                                             int* __restrict__ lab) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) / 64;
  const int nchunks = C / 8;
  if (row >= N) return;
  u32x4 cur[kPer];
  const u32x4* rp = reinterpret_cast<const u32x4*>(preds + (long long)row * C);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int ci = lane + j * 64;
    cur[j] = __builtin_nontemporal_load(rp + (ci < nchunks ? ci : nchunks - 1));
  }
  const long long t = lane == 0 ? target[row] : 0;
  s16x2 smx = {-32768, -32768};
  u16x2 umx = {0, 0}, umn = {0xffff, 0xffff};
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = cur[j][k];
      smx = __builtin_elementwise_max(smx, __builtin_bit_cast(s16x2, w));
      umx = __builtin_elementwise_max(umx, __builtin_bit_cast(u16x2, w));
      if (kNegMin) umn = __builtin_elementwise_min(umn, __builtin_bit_cast(u16x2, w));
    }
  }
  const int ls = smx.x > smx.y ? smx.x : smx.y;
  const uint32_t lu = umx.x > umx.y ? umx.x : umx.y;
  const bool neg_nan = __any(lu > 0xff80u);
  int bidx = -1;
  if (kScan == 0) {
    const int s = __reduce_max_sync(~0ull, ls);
    uint32_t v = 0;
    bool exact = false;
    if (!neg_nan && s > 0 && s <= 0x7f80) {
      v = static_cast<uint32_t>(s);
      exact = true;
    } else if (kNegMin && !neg_nan && s < 0) {
      const uint32_t ln = umn.x < umn.y ? umn.x : umn.y;
      v = static_cast<uint32_t>(__reduce_min_sync(~0ull, static_cast<int>(ln)));
      exact = true;
    }
    if (exact) {
      const uint32_t vv = v * 0x10001u;
      uint32_t miss = 0;
#pragma unroll
      for (int j = kPer - 1; j >= 0; --j) {
#pragma unroll
        for (int k = 3; k >= 0; --k) {
          const u16x2 x = __builtin_bit_cast(u16x2, cur[j][k] ^ vv);
          const u16x2 one = {1, 1};
          miss = (miss << 1) | __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, one));
        }
      }
      constexpr uint32_t kWords = (1u << (4 * kPer)) - 1u;
      const uint32_t hit = ~miss;
      const int plo = 2 * __builtin_ctz((hit & kWords) | 0x10000u);
      const int phi = 2 * __builtin_ctz(((hit >> 16) & kWords) | 0x10000u) + 1;
      const int pos = plo < phi ? plo : phi;
      const int col = pos >= 32 ? 0x7fffffff : lane * 8 + (pos >> 3) * 512 + (pos & 7);
      bidx = __reduce_min_sync(~0ull, col);
    }
  } else if (kScan == 2) {  // the shipped form: the lane's own maximum mapped to its ordinal, mask scan, ONE wave max
    const uint32_t ln = umn.x < umn.y ? umn.x : umn.y;
    const bool lneg = ls < 0;
    const uint32_t c = lneg ? ln : static_cast<uint32_t>(ls);
    const uint32_t ord = c ^ (lneg ? 0xffffu : 0x8000u);
    const uint32_t cc = c | (c << 16);
    uint32_t miss = 0;
#pragma unroll
    for (int j = kPer - 1; j >= 0; --j) {
#pragma unroll
      for (int k = 3; k >= 0; --k) miss = (miss << 1) | pk_nonzero_u16(cur[j][k] ^ cc);
    }
    constexpr uint32_t kWords = (1u << (4 * kPer)) - 1u;
    const uint32_t hit = ~miss;
    const int plo = 2 * __builtin_ctz((hit & kWords) | 0x10000u);
    const int phi = 2 * __builtin_ctz(((hit >> 16) & kWords) | 0x10000u) + 1;
    const int pos = plo < phi ? plo : phi;
    const uint32_t col = lane * 8 + (pos >> 3) * 512 + (pos & 7);
    const uint32_t key = wave_max_u32((ord << 16) | (0xffffu - col));
    const uint32_t kmax = key >> 16;
    if (!neg_nan && kmax <= 0xff80u && kmax != 0x8000u && kmax != 0x7fffu) bidx = 0xffff - static_cast<int>(key & 0xffffu);
  } else {
    const uint32_t l16 = static_cast<uint32_t>(ls) & 0xffffu;
    uint32_t first = 0xffffu;
#pragma unroll
    for (int j = kPer - 1; j >= 0; --j) {
      const int ci = lane + j * 64;
#pragma unroll
      for (int k = 3; k >= 0; --k) {
        const uint32_t w = cur[j][k];
        if ((w >> 16) == l16) first = ci * 8 + 2 * k + 1;
        if ((w & 0xffffu) == l16) first = ci * 8 + 2 * k;
      }
    }
    const int key = __reduce_max_sync(~0ull, static_cast<int>((static_cast<uint32_t>(ls) << 16) | (0xffffu - first)));
    const int s = key >> 16;
    if (!neg_nan && s > 0 && s <= 0x7f80) bidx = 0xffff - (key & 0xffff);
  }
  if (bidx < 0) bidx = ord_row<kPer>(cur, lane, nchunks);  // wave-uniform
  if (lane == 0) emit<kMode>(t, bidx, row, C, out, lab);
}

int main() {
  const int N = 8192, C = 1000, NB = 26, kRings = 2;
  const char* ring_name[kRings] = {"randn", "allneg"};
  std::vector<uint16_t> h(static_cast<size_t>(N) * C);
  std::vector<int64_t> ht(N);
  uint32_t s = 12345;
  auto rnd = [&] {
    s = s * 1664525u + 1013904223u;
    return s;
  };
  // ring 0: uniform in [-3, 3) (randn-like: a positive maximum in every row); ring 1: log-softmax-like, all in
  // [-12, -0.001]
  uint16_t* dp[kRings][NB];
  int64_t* dt[NB];
  for (int r = 0; r < kRings; ++r) {
    for (int b = 0; b < NB; ++b) {
      for (auto& x : h) {
        const float u01 = (rnd() >> 8) / 16777216.0f;
        const float f = r == 0 ? (u01 - 0.5f) * 6.f : -(u01 * 12.f + 0.001f);
        uint32_t u;
        std::memcpy(&u, &f, 4);
        x = (uint16_t)(u >> 16);
      }
      CK(hipMalloc(&dp[r][b], h.size() * 2));
      CK(hipMemcpy(dp[r][b], h.data(), h.size() * 2, hipMemcpyHostToDevice));
    }
  }
  for (int b = 0; b < NB; ++b) {
    for (auto& t : ht) t = rnd() % C;
    CK(hipMalloc(&dt[b], N * 8));
    CK(hipMemcpy(dt[b], ht.data(), N * 8, hipMemcpyHostToDevice));
  }
  unsigned long long* out;
  int *lab, *lab_ref;
  CK(hipMalloc(&out, (size_t)C * C * 8));
  CK(hipMalloc(&lab, N * 4));
  CK(hipMalloc(&lab_ref, N * 4));
  CK(hipMemset(out, 0, (size_t)C * C * 8));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int reps = 520, kRepeat = 5;
  // every variant is timed kRepeat times; "us" is the median, us_min / us_max the run's own spread
  auto timeit = [&](const char* ring, const char* name, auto launch) {
    float us[kRepeat];
    for (int r = 0; r < kRepeat; ++r) {
      for (int i = 0; i < 52; ++i) launch(i % NB);
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0));
      for (int i = 0; i < reps; ++i) launch(i % NB);
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      us[r] = ms * 1e3f / reps;
    }
    CK(hipGetLastError());
    for (int i = 1; i < kRepeat; ++i)
      for (int j = i; j > 0 && us[j] < us[j - 1]; --j) std::swap(us[j], us[j - 1]);
    const float med = us[kRepeat / 2];
    std::printf("{\"ring\": \"%s\", \"variant\": \"%s\", \"us\": %.3f, \"us_min\": %.3f, \"us_max\": %.3f, \"TBps\": %.2f}\n",
                ring, name, med, us[0], us[kRepeat - 1], (double)N * C * 2 / (med * 1e-6) / 1e12);
    std::fflush(stdout);
  };
  timeit("-", "empty_2048x256", [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(2048), dim3(256), 0, 0, lab); });
  timeit("-", "empty_1x64", [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, 0, lab); });
  timeit("-", "empty_512x1024", [&](int) { hipLaunchKernelGGL(empty_kernel, dim3(512), dim3(1024), 0, 0, lab); });
  for (int r = 0; r < kRings; ++r) {
    uint16_t** p = dp[r];
    const char* rn = ring_name[r];
    // the lean variants' labels against the ordinal reduction's on one batch
    {
      std::vector<int> a(N), b(N);
      hipLaunchKernelGGL((vord<2, 1, 1>), dim3(N / 8), dim3(512), 0, 0, p[0], dt[0], N, C, out, lab_ref);
      CK(hipMemcpy(a.data(), lab_ref, N * 4, hipMemcpyDeviceToHost));
      auto check = [&](const char* name, auto launch) {
        CK(hipMemset(lab, 0xff, N * 4));
        launch();
        CK(hipMemcpy(b.data(), lab, N * 4, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int i = 0; i < N; ++i) bad += a[i] != b[i];
        std::printf("{\"ring\": \"%s\", \"check\": \"%s\", \"label_mismatches\": %d}\n", rn, name, bad);
        if (bad) std::exit(2);  // a wrong column must not reach the atomics of the timed variants
      };
      check("lean_mask3", [&] { hipLaunchKernelGGL((vlean<2, 0, true, 1>), dim3(N / 8), dim3(512), 0, 0, p[0], dt[0], N, C, out, lab); });
      check("lean_mask2", [&] { hipLaunchKernelGGL((vlean<2, 0, false, 1>), dim3(N / 8), dim3(512), 0, 0, p[0], dt[0], N, C, out, lab); });
      check("lean_key2", [&] { hipLaunchKernelGGL((vlean<2, 1, false, 1>), dim3(N / 8), dim3(512), 0, 0, p[0], dt[0], N, C, out, lab); });
      check("lean_key3", [&] { hipLaunchKernelGGL((vlean<2, 2, true, 1>), dim3(N / 8), dim3(512), 0, 0, p[0], dt[0], N, C, out, lab); });
    }
    for (int bs : {256, 512, 1024}) {
      const dim3 g1(N / (bs / 64)), g2(N / (bs / 32)), blk(bs);
      char name[64];
      std::snprintf(name, sizeof(name), "read_1row_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vread<2, 1>), g1, blk, 0, 0, p[b], N, C, lab); });
      if (r == 0) {
        std::snprintf(name, sizeof(name), "read_2row_b%d", bs);
        timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vread<2, 2>), g2, blk, 0, 0, p[b], N, C, lab); });
        std::snprintf(name, sizeof(name), "ord_2row_i64atomic_b%d", bs);
        timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vord<2, 2, 0>), g2, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      }
      std::snprintf(name, sizeof(name), "ord_1row_i64atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vord<2, 1, 0>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      if (bs == 256) continue;
      std::snprintf(name, sizeof(name), "ord_1row_labelstore_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vord<2, 1, 1>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "ord_1row_i32atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vord<2, 1, 2>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_mask3_i64atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 0, true, 0>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_mask3_labelstore_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 0, true, 1>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_mask2_i64atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 0, false, 0>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_key2_i64atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 1, false, 0>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_key3_i64atomic_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 2, true, 0>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
      std::snprintf(name, sizeof(name), "lean_key3_labelstore_b%d", bs);
      timeit(rn, name, [&](int b) { hipLaunchKernelGGL((vlean<2, 2, true, 1>), g1, blk, 0, 0, p[b], dt[b], N, C, out, lab); });
    }
  }
  // host-side launch cost alone: launches into a stream blocked behind a long kernel are queued, not run
  {
    const int L = 400;
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < L; ++i) hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, 0, lab);
    auto t1 = std::chrono::steady_clock::now();
    CK(hipDeviceSynchronize());
    std::printf("{\"variant\": \"host_launch_cost\", \"us\": %.3f}\n",
                std::chrono::duration<double, std::micro>(t1 - t0).count() / L);
  }
  return 0;
}
