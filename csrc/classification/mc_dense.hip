// Dense-prediction multiclass updates: float scores [N, C, X] with X > 1 (segmentation logits [N, C, H, W] against
// [N, H, W] targets), where the class axis has stride X and the pixels are the contiguous axis.  Fills the outputs of
// mc_update (stat_scores.hip): the [C, C] int64 confusion matrix or the [G, 3C + 1] stats workspace (global or
// samplewise), for f32 / f16 / bf16 scores; f64 and label inputs stay on mc_update's kernels.
//
// mc_dense_kernel (top_k = 1):
//   * work split: a tile is blockDim * P consecutive pixels of ONE sample (P = 16 B of scores: 8 pixels of 16-bit, 4 of
//     f32); a thread owns P adjacent pixels.  The grid is persistent (a few blocks per CU) and block b walks the
//     contiguous tile range [b T / G, (b + 1) T / G), so a block meets each sample change once.
//   * loads: per class one 16-byte load per thread at preds + (n C + c) X + x0, kClassUnroll classes issued before the
//     first compare; the running (best, index) of the P pixels stays in registers.  Rows start at byte (n C + c) X
//     sizeof: the load width is the largest of 16 / 8 / 4 / 2 bytes dividing X * sizeof and the base pointer (a
//     template parameter), a thread then covers its 16 bytes with 1 / 2 / 4 / 8 loads.  Since the width divides the
//     row length, a load is wholly inside the row or wholly past it: the pixel tail needs no partial load.
//   * compare: classes ascend and a class replaces the best only if !(v <= best) && best == best in fp32 -- NaN wins,
//     then the larger value, then the smaller index, which is argmax_better for an ascending scan.  (16-bit scores
//     widen exactly; the order-preserving ordinals of the row kernels would cost a NaN and a -0 fix-up per element
//     here, where there is no cross-lane reduction for an integer key to speed up.)
//   * counting: a thread merges runs of equal (target, prediction) among its P pixels and adds the run length with one
//     atomic per run -- label maps are large uniform regions, and one atomic per pixel on one address is what
//     serialises.  The histogram (C x C or 3C + 1 int32) is private to the block in LDS up to kLdsHistMaxKb (dynamic
//     LDS above 64 KB: one 1024-thread block per CU from 80 KB on), flushed non-zero bins only with int64 atomics: at
//     the end, at a sample change in samplewise mode, and before 2^30 pixels.  Larger histograms (C > 202 confusion
//     matrix) take the same run-merged adds as global int64 atomics.
//
// mc_dense_topk_kernel (stats, 2 <= top_k <= 16): one pixel per lane (adjacent lanes, adjacent pixels), kTopkUnroll
// class loads in flight, the k best kept sorted in registers by insertion as topk.hip's 64-bit keys (ordered fp32
// bits << 32 | ~class: NaN highest, ties to the smaller class), slots a compile-time 2 / 4 / 8 / 16.  Counted by
// mc_accumulate's rule: tp[t] if t is among the k else fn[t]; fp[p] for each of the k labels p != t.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, over the int64 / int32 / uint8 target
// types; scratch is 0 bytes per lane in every variant, LDS is dynamic only -- the histogram, 4 nbins bytes):
//   mc_dense_kernel, load width 16 / 8 / 4 / 2 B      VGPRs                 SGPRs   waves per SIMD
//     f32                                             45-46 / 47-48 / 44    <= 101  8 / 8 / 7
//     f16                                             62-63 / 63-64 / 61 / 65  <= 106  8 / 7 / 7 / 7
//     bf16                                            61-62 / 63-64 / 61 / 65  <= 106  8 / 7 / 7 / 7
//   mc_dense_topk_kernel, 2 / 4 / 8 / 16 slots        38 / 42 / 55 / 88     <= 106  8 / 8 / 8 / 5   (every score type)
// The launch asks for 16 waves per CU (4 per SIMD), which all of them hold resident.
//
// Measured on MI355X (benchmarks/bench_mc_dense.py, profiles/mc_dense_bench.jsonl: update() call, median of 30, three
// alternated processes per setting; old = TM_AMD_MC_DENSE=0 in the same run, whose round-to-round spread was <= 1.2 %):
//   8 x 19 x 512 x 1024 bf16   confusion matrix 52.1 us (old 110.6), macro accuracy 57.6 (393.0)
//   8 x 19 x 512 x 1024 f32    75.2 (136.5), 80.8 (468.4)
//   8 x 150 x 512 x 512 bf16   121.1 (460.2), 127.6 (394.8)
//   16 x 21 x 512 x 512 f16    52.5 (118.7), 60.5 (434.8)
//   256 x 19 x 24 x 24 bf16    15.7 (110.1), 22.9 (33.7)     -- X = 576, just above kDenseMinX
//   8 x 19 x 512 x 1024 bf16, top_k = 5 accuracy: 307.5 us (torch.topk + label histogram: 11178)
// i.e. 0.86-1.37 x the time a device copy's bandwidth needs to read the large inputs once.  The C = 150 confusion
// matrix with its 90 KB histogram in LDS (one 1024-thread block per CU) takes 121.1 us, with the run-merged global
// atomics instead (TM_AMD_MC_DENSE_LDS_KB=64) 223.5 us: the LDS histogram is kept up to the 160 KB limit.  No shape
// class lost to the old dispatch, so the condition was not narrowed further.
//
// mc_update sends argmax inputs with X >= kDenseMinX here (TM_AMD_MC_DENSE=0: the old dispatch, for A/B runs); below
// that most lanes of a tile would idle, so those inputs keep mc_fewbins_kernel / mc_items_kernel (not measured).  The
// direct entry ops.mc_dense_update takes any X >= 2.
#include "../common/tm_common.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace tm_amd {
namespace {

constexpr int kDenseMaxBlock = 1024;
constexpr int kDenseBlocksPerCu = 4;  // of 256 threads
constexpr int kClassUnroll = 4;  // classes whose 16-byte loads are issued before the first compare
constexpr int kTopkBlock = 256;
constexpr int kTopkUnroll = 8;
constexpr int kTopkMax = 16;
constexpr long long kFlushPixels = 1LL << 30;  // int32 bins: a block flushes before it has counted this many pixels
enum DenseMode : int { kDenseConfmat = 0, kDenseStats = 1 };
using u64 = unsigned long long;

// a thread's 16 bytes of one class row: `nvalid` of them (a multiple of LB) lie inside the row, the rest read as 0
template <int LB>
__device__ __forceinline__ void load_slot(const unsigned char* __restrict__ p, int nvalid, uint32_t (&w)[4]) {
  if constexpr (LB == 16) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (nvalid == 16) v = *reinterpret_cast<const u32x4*>(p);
    w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
  } else if constexpr (LB == 8) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      uint2 v = make_uint2(0u, 0u);
      if (u * 8 < nvalid) v = *reinterpret_cast<const uint2*>(p + u * 8);
      w[2 * u] = v.x, w[2 * u + 1] = v.y;
    }
  } else if constexpr (LB == 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = u * 4 < nvalid ? *reinterpret_cast<const uint32_t*>(p + u * 4) : 0u;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t lo = u * 4 < nvalid ? *reinterpret_cast<const unsigned short*>(p + u * 4) : 0u;
      const uint32_t hi = u * 4 + 2 < nvalid ? *reinterpret_cast<const unsigned short*>(p + u * 4 + 2) : 0u;
      w[u] = lo | (hi << 16);
    }
  }
}

// pixel j of a loaded slot as fp32 (exact for every input type)
template <typename scalar_t, int J>
__device__ __forceinline__ float slot_elem(const uint32_t (&w)[4]) {
  if constexpr (sizeof(scalar_t) == 4) {
    return __uint_as_float(w[J]);
  } else {
    const uint32_t word = w[J >> 1];
    if constexpr (std::is_same<scalar_t, c10::BFloat16>::value) {
      return __uint_as_float((J & 1) ? (word & 0xffff0000u) : (word << 16));
    } else {
      const unsigned short h = static_cast<unsigned short>((J & 1) ? (word >> 16) : (word & 0xffffu));
      return static_cast<float>(__builtin_bit_cast(_Float16, h));
    }
  }
}

template <typename scalar_t, int P, int J = 0>
__device__ __forceinline__ void slot_argmax(const uint32_t (&w)[4], int c, float (&best)[P], int (&bidx)[P]) {
  if constexpr (J < P) {
    const float v = slot_elem<scalar_t, J>(w);
    // ascending classes: NaN wins, then the larger value, then the smaller (earlier) index
    const bool better = !(v <= best[J]) && best[J] == best[J];
    best[J] = better ? v : best[J];
    bidx[J] = better ? c : bidx[J];
    slot_argmax<scalar_t, P, J + 1>(w, c, best, bidx);
  }
}

// add `v` observations to a bin of the block's LDS histogram, or of the group's global one
__device__ __forceinline__ void bin_add(int* lds, int64_t* __restrict__ gout, bool use_lds, long long bin, int v) {
  if (use_lds) atomicAdd(&lds[bin], v);
  else atomic_add_i64(gout + bin, v);
}

// non-zero bins to the group's global histogram; the LDS copy is left zeroed for the next group
__device__ __forceinline__ void hist_flush(int* lds, int nbins, int64_t* __restrict__ gout) {
  __syncthreads();
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
    const int v = lds[b];
    if (v) {
      atomic_add_i64(gout + b, v);
      lds[b] = 0;
    }
  }
  __syncthreads();
}

// The walk over a block's tiles, shared by both kernels.  enter() is block-uniform and flushes the LDS histogram when
// the sample changes (samplewise) or the int32 bins could overflow.
struct TileWalk {
  long long tile, end, n, ts;  // current tile, one past the block's last, its sample, its index within the sample
  long long prev_n, since;
  __device__ __forceinline__ void init(long long tiles, long long tiles_per_sample) {
    tile = tiles * blockIdx.x / gridDim.x;
    end = tiles * (blockIdx.x + 1) / gridDim.x;
    n = tile / tiles_per_sample;
    ts = tile - n * tiles_per_sample;
    prev_n = -1;
    since = 0;
  }
  __device__ __forceinline__ void enter(long long tile_px, bool use_lds, bool samplewise, int* lds, int nbins,
                                        int64_t* __restrict__ out) {
    if (use_lds && prev_n >= 0 && ((samplewise && n != prev_n) || since + tile_px > kFlushPixels)) {
      hist_flush(lds, nbins, out + (samplewise ? prev_n : 0) * nbins);
      since = 0;
    }
    prev_n = n;
    since += tile_px;
  }
  __device__ __forceinline__ void advance(long long tiles_per_sample) {
    ++tile;
    if (++ts == tiles_per_sample) ts = 0, ++n;
  }
};

template <typename scalar_t, typename target_t, int LB>
__global__ void __launch_bounds__(kDenseMaxBlock) mc_dense_kernel(const scalar_t* __restrict__ preds,
                                                                  const target_t* __restrict__ target, long long N,
                                                                  long long X, int C, long long ignore,
                                                                  bool has_ignore, int mode, bool samplewise,
                                                                  bool use_lds, long long tiles_per_sample,
                                                                  int64_t* __restrict__ out, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  constexpr int P = 16 / sizeof(scalar_t);
  const int nbins = mode == kDenseConfmat ? C * C : 3 * C + 1;
  const long long tile_px = static_cast<long long>(blockDim.x) * P;
  const long long row_bytes = X * static_cast<long long>(sizeof(scalar_t));
  if (use_lds) {
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) lds[b] = 0;
    __syncthreads();
  }
  TileWalk tw;
  tw.init(N * tiles_per_sample, tiles_per_sample);
  for (; tw.tile < tw.end; tw.advance(tiles_per_sample)) {
    tw.enter(tile_px, use_lds, samplewise, lds, nbins, out);
    const long long n = tw.n;
    const long long x0 = tw.ts * tile_px + static_cast<long long>(threadIdx.x) * P;
    const long long rem = X - x0;  // pixels of the row from x0 on (<= 0: this thread is past the row)
    const int npx = rem >= P ? P : (rem > 0 ? static_cast<int>(rem) : 0);
    const int nvalid = npx * static_cast<int>(sizeof(scalar_t));

    long long tv[P];
#pragma unroll
    for (int j = 0; j < P; ++j) tv[j] = j < npx ? static_cast<long long>(target[n * X + x0 + j]) : -1;

    float best[P];
    int bidx[P];
#pragma unroll
    for (int j = 0; j < P; ++j) best[j] = -INFINITY, bidx[j] = 0;  // all -inf: nothing beats class 0
    const unsigned char* base = reinterpret_cast<const unsigned char*>(preds + n * C * X + x0);
    for (int c = 0; c < C; c += kClassUnroll) {  // the last group is cut short by block-uniform branches
      uint32_t w[kClassUnroll][4];
#pragma unroll
      for (int u = 0; u < kClassUnroll; ++u)
        if (c + u < C) load_slot<LB>(base + (c + u) * row_bytes, nvalid, w[u]);
#pragma unroll
      for (int u = 0; u < kClassUnroll; ++u)
        if (c + u < C) slot_argmax<scalar_t, P>(w[u], c + u, best, bidx);
    }

    int64_t* gout = out + (samplewise ? n : 0) * nbins;
    auto emit = [&](int t, int p, int len) {
      if (mode == kDenseConfmat) {
        bin_add(lds, gout, use_lds, static_cast<long long>(t) * C + p, len);
      } else if (t == p) {
        bin_add(lds, gout, use_lds, t, len);
      } else {
        bin_add(lds, gout, use_lds, C + p, len);
        bin_add(lds, gout, use_lds, 2LL * C + t, len);
      }
    };
    int rt = -1, rp = 0, rl = 0;  // the open run: target, prediction, length
#pragma unroll
    for (int j = 0; j < P; ++j) {
      int t = -1;  // mc_target's contract: ignored and out-of-range targets are skipped, the latter flagged
      if (j < npx && !(has_ignore && tv[j] == ignore)) {
        if (tv[j] < 0 || tv[j] >= C) raise_flag(flag, kErrTargetOutOfRange);
        else t = static_cast<int>(tv[j]);
      }
      if (t >= 0 && t == rt && bidx[j] == rp) {
        ++rl;
      } else {
        if (rl) emit(rt, rp, rl);
        rt = t, rp = bidx[j], rl = t >= 0 ? 1 : 0;
      }
    }
    if (rl) emit(rt, rp, rl);
  }
  if (use_lds && tw.prev_n >= 0) hist_flush(lds, nbins, out + (samplewise ? tw.prev_n : 0) * nbins);
}

// ------------------------------------------------------------------------------------------------------ top_k
// topk.hip's key: larger key = torch.topk's order (NaN highest, -0 == +0), ties to the smaller class; never 0
__device__ __forceinline__ u64 topk_key(float f, int col) {
  unsigned u = __float_as_uint(f == 0.f ? 0.f : f);
  u = (f != f) ? 0xffffffffu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
  return (static_cast<u64>(u) << 32) | static_cast<unsigned>(~col);
}

template <int KP>
__device__ __forceinline__ void topk_offer(u64 (&s)[KP], u64& thr, u64 key, int K) {
  if (key <= thr) return;
#pragma unroll
  for (int q = KP - 1; q >= 1; --q) {
    if (q < K) {
      const u64 up = s[q - 1];
      s[q] = key > up ? up : (key > s[q] ? key : s[q]);
    }
  }
  s[0] = key > s[0] ? key : s[0];
#pragma unroll
  for (int q = 0; q < KP; ++q)
    if (q == K - 1) thr = s[q];
}

template <typename scalar_t, typename target_t, int KP>
__global__ void __launch_bounds__(kTopkBlock) mc_dense_topk_kernel(const scalar_t* __restrict__ preds,
                                                                   const target_t* __restrict__ target, long long N,
                                                                   long long X, int C, int K, long long ignore,
                                                                   bool has_ignore, bool samplewise, bool use_lds,
                                                                   long long tiles_per_sample,
                                                                   int64_t* __restrict__ out, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) int lds[];
  const int nbins = 3 * C + 1;
  const long long tile_px = blockDim.x;
  if (use_lds) {
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) lds[b] = 0;
    __syncthreads();
  }
  TileWalk tw;
  tw.init(N * tiles_per_sample, tiles_per_sample);
  for (; tw.tile < tw.end; tw.advance(tiles_per_sample)) {
    tw.enter(tile_px, use_lds, samplewise, lds, nbins, out);
    const long long n = tw.n;
    const long long x = tw.ts * tile_px + threadIdx.x;
    if (x >= X) continue;  // no barrier below: the walk's flushes are ahead of this
    const long long tv = static_cast<long long>(target[n * X + x]);
    if (has_ignore && tv == ignore) continue;
    if (tv < 0 || tv >= C) {
      raise_flag(flag, kErrTargetOutOfRange);
      continue;
    }
    const int t = static_cast<int>(tv);
    u64 s[KP];
    u64 thr = 0;
#pragma unroll
    for (int q = 0; q < KP; ++q) s[q] = 0;
    const scalar_t* p = preds + n * C * X + x;
    int c = 0;
    for (; c + kTopkUnroll <= C; c += kTopkUnroll) {
      float v[kTopkUnroll];
#pragma unroll
      for (int u = 0; u < kTopkUnroll; ++u) v[u] = to_f32(p[(c + u) * X]);
#pragma unroll
      for (int u = 0; u < kTopkUnroll; ++u) topk_offer<KP>(s, thr, topk_key(v[u], c + u), K);
    }
    for (; c < C; ++c) topk_offer<KP>(s, thr, topk_key(to_f32(p[c * X]), c), K);

    int64_t* gout = out + (samplewise ? n : 0) * nbins;
    bool hit = false;
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      if (q < K) {
        const int col = static_cast<int>(~static_cast<unsigned>(s[q]));
        if (col == t) hit = true;
        else bin_add(lds, gout, use_lds, C + col, 1);
      }
    }
    bin_add(lds, gout, use_lds, hit ? t : 2LL * C + t, 1);
  }
  if (use_lds && tw.prev_n >= 0) hist_flush(lds, nbins, out + (samplewise ? tw.prev_n : 0) * nbins);
}

// ---------------------------------------------------------------------------------------------------- launchers
constexpr int kLdsHistMaxKb = 160;  // gfx950: 160 KB of LDS per CU

// largest LDS histogram a block may hold, in bytes (TM_AMD_MC_DENSE_LDS_KB: measurement knob, e.g. 64 sends
// 111 <= C <= 202 confusion matrices to the global run-merged adds)
long long lds_hist_limit(int device) {
  static const long long knob = [] {
    const char* e = std::getenv("TM_AMD_MC_DENSE_LDS_KB");
    return 1024LL * (e ? std::max(0, std::atoi(e)) : kLdsHistMaxKb);
  }();
  static const long long dev_max = [device] {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || v <= 0) v = 65536;
    return static_cast<long long>(v);
  }();
  return std::min(knob, dev_max);
}

template <typename K>
void allow_lds(K kernel, size_t lds_bytes) {
  if (lds_bytes > 48 * 1024)
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds_bytes)) == hipSuccess,
                "mc_dense_update: cannot reserve ", lds_bytes, " bytes of LDS");
}

#define TM_DISPATCH_DENSE_SCORES(dtype, ...)                                        \
  [&] {                                                                             \
    switch (dtype) {                                                                \
      case at::kFloat: { using scalar_t = float; return __VA_ARGS__(); }            \
      case at::kHalf: { using scalar_t = c10::Half; return __VA_ARGS__(); }         \
      default: { using scalar_t = c10::BFloat16; return __VA_ARGS__(); }            \
    }                                                                               \
  }()

template <typename F>
void with_load_bytes(int lb, F&& f) {
  switch (lb) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 2>{}); break;
  }
}

template <typename F>
void with_topk_slots(int k, F&& f) {
  if (k <= 2) f(std::integral_constant<int, 2>{});
  else if (k <= 4) f(std::integral_constant<int, 4>{});
  else if (k <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace

// Dense multiclass update (see the header).  preds: f32 / f16 / bf16 [N, C, X], X >= 2; target: int [N, X];
// mode 0: out = confmat [C, C] int64; mode 1: out = workspace [G, 3C + 1] int64 (G = N if samplewise else 1);
// top_k > 1: stats mode only.  Returns false, having done nothing, where the kernels do not apply (CPU tensors,
// X == 1, f64 / integer preds, top_k outside [1, min(16, C)] or top_k > 1 for the confusion matrix).
bool mc_dense_update(const at::Tensor& preds, const at::Tensor& target, at::Tensor out, at::Tensor flag,
                     int64_t num_classes, int64_t ignore_index, bool has_ignore, int64_t mode, bool samplewise,
                     int64_t top_k) {
  const auto dt = preds.scalar_type();
  if (!preds.is_cuda() || !(dt == at::kFloat || dt == at::kHalf || dt == at::kBFloat16)) return false;
  if (target.numel() == 0 || target.dim() < 1 || target.is_floating_point() || num_classes < 1 || num_classes >= (1LL << 30)) return false;
  const long long N = target.size(0);
  const long long X = target.numel() / N;
  const int C = static_cast<int>(num_classes);
  if (X < 2 || top_k < 1 || top_k > kTopkMax || top_k > C || (top_k > 1 && mode != kDenseStats)) return false;
  TM_CHECK_CUDA(preds);
  TM_SAME_DEVICE(preds, target);
  TM_SAME_DEVICE(preds, out);
  TM_SAME_DEVICE(preds, flag);
  TM_CHECK_CONTIG(preds);
  TM_CHECK_CONTIG(target);
  TM_CHECK_CONTIG(out);
  TORCH_CHECK(mode == kDenseConfmat || mode == kDenseStats, "mc_dense_update: bad mode");
  TORCH_CHECK(out.scalar_type() == at::kLong, "mc_dense_update: out must be int64");
  TORCH_CHECK(flag.scalar_type() == at::kInt && flag.numel() >= 1, "mc_dense_update: flag must be int32[1]");
  TORCH_CHECK(preds.numel() == N * C * X, "mc_dense_update: preds must be [N, C, ...] matching target");
  const long long nbins = mode == kDenseConfmat ? static_cast<long long>(C) * C : 3LL * C + 1;
  TORCH_CHECK(out.numel() == (mode == kDenseStats && samplewise ? N : 1) * nbins, "mc_dense_update: out has wrong size");
  TORCH_CHECK(nbins < (1LL << 31), "mc_dense_update: too many classes");
  if (mode == kDenseConfmat) samplewise = false;

  const int device = preds.get_device();
  const int cus = cu_count(device);
  const long long hist_bytes = nbins * static_cast<long long>(sizeof(int));
  const bool use_lds = hist_bytes <= lds_hist_limit(device);
  const size_t lds_bytes = use_lds ? static_cast<size_t>(hist_bytes) : 0;
  // 16 waves per CU, which every variant's registers allow resident at once (the grid is persistent: a block that
  // had to wait for a slot would run after the others): 4 x 256 threads, or 2 x 512 / 1 x 1024 where the LDS of a
  // CU holds only so many histograms
  const long long fit = use_lds ? kLdsHistMaxKb * 1024LL / hist_bytes : kDenseBlocksPerCu;  // histograms per CU
  const int per_cu = fit >= kDenseBlocksPerCu ? kDenseBlocksPerCu : (fit >= 2 ? 2 : 1);
  const int threads = 256 * kDenseBlocksPerCu / per_cu;
  auto s = stream();
  int64_t* outp = out.data_ptr<int64_t>();
  int* flagp = flag.data_ptr<int>();
  TM_DISPATCH_TARGET(target.scalar_type(), "mc_dense_update", [&] {
    const target_t* tp = reinterpret_cast<const target_t*>(target.data_ptr());
    TM_DISPATCH_DENSE_SCORES(dt, [&] {
      const scalar_t* pp = reinterpret_cast<const scalar_t*>(preds.data_ptr());
      if (top_k > 1) {
        const long long tps = (X + kTopkBlock - 1) / kTopkBlock;
        const int grid = static_cast<int>(std::min<long long>(N * tps, static_cast<long long>(kDenseBlocksPerCu) * cus));
        with_topk_slots(static_cast<int>(top_k), [&](auto kp) {
          auto kernel = mc_dense_topk_kernel<scalar_t, target_t, decltype(kp)::value>;
          allow_lds(kernel, lds_bytes);
          hipLaunchKernelGGL(kernel, dim3(grid), dim3(kTopkBlock), lds_bytes, s, pp, tp, N, X, C,
                             static_cast<int>(top_k), ignore_index, has_ignore, samplewise, use_lds, tps, outp, flagp);
        });
        return;
      }
      const long long tile_px = static_cast<long long>(threads) * (16 / sizeof(scalar_t));
      const long long tps = (X + tile_px - 1) / tile_px;
      const int grid = static_cast<int>(std::min<long long>(N * tps, static_cast<long long>(per_cu) * cus));
      // the widest load that every class row's first byte and length allow
      const uintptr_t align = reinterpret_cast<uintptr_t>(pp) | static_cast<uintptr_t>(X * sizeof(scalar_t));
      const int lb = align % 16 == 0 ? 16 : (align % 8 == 0 ? 8 : (align % 4 == 0 ? 4 : 2));
      with_load_bytes(lb, [&](auto lb_tag) {
        constexpr int LB = decltype(lb_tag)::value;
        if constexpr (LB >= static_cast<int>(sizeof(scalar_t))) {
          auto kernel = mc_dense_kernel<scalar_t, target_t, LB>;
          allow_lds(kernel, lds_bytes);
          hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds_bytes, s, pp, tp, N, X, C, ignore_index,
                             has_ignore, static_cast<int>(mode), samplewise, use_lds, tps, outp, flagp);
        }
      });
    });
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return true;
}

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def("mc_dense_update(Tensor preds, Tensor target, Tensor(a!) out, Tensor(b!) flag, int num_classes, "
        "int ignore_index, bool has_ignore, int mode, bool samplewise, int top_k) -> bool");
}
TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) { m.impl("mc_dense_update", &mc_dense_update); }

}  // namespace tm_amd
