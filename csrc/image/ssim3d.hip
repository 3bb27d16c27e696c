// Fused SSIM / contrast-sensitivity kernel for 3-D volumes (separable Gaussian or uniform window).
//
// Same contract as ssim.hip one dimension up: the reference's reflect-pad + crop keeps exactly the windows that lie
// fully inside the volume, so only those are evaluated, straight from the unpadded [P, D, H, W] volumes.  A 3-D LDS
// tile with a halo on every axis would re-read each voxel ~6x; instead a block marches along the depth axis:
//
//   block = (4*PX) x 64 in-plane output tile of one plane x a contiguous chunk of output depth, 256 threads
//           (4 wave64, one wave across W; every thread owns PX vertically adjacent pixels of its column)
//   per input slice z of the chunk (chunk + kd - 1 of them):
//   1. stage the (TH+kh-1) x (64+kw-1) tile of x and y in LDS in the accumulation type (16-byte global loads where
//      the row start allows them, scalar edges)
//   2. pass along W: 5 running moments per (row, out-col) -> LDS
//   3. pass along H per owned pixel -> 5 in-plane filtered moments in registers
//   4. depth ring in registers: KD pending output slices x 5 moments per owned pixel, ring[q] += wd[tap] * m.  KD is a
//      template parameter and the march is unrolled in groups of KD, so every slot and tap index is a constant.
//   5. the slot that took its last tap is a finished output voxel: SSIM and CS are added to the thread's sums and
//      the slot is cleared.  The end of a chunk flushes nothing; later outputs belong to the next chunk's block.
//   block reduction -> one (sum SSIM, sum CS) slot per block, written in a fixed order (no atomics, deterministic).
#include "../common/tm_common.h"

#include <type_traits>

namespace tm_amd {
namespace {

constexpr int kTW = 64;      // output cols per block (one wave across)
constexpr int kMaxK = 33;    // largest in-plane window edge
constexpr int kMaxKD = 11;   // largest depth window (ring slots held in registers)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

template <typename T>
struct Acc {
  using type = float;
  static constexpr int kPX = 2;  // owned pixels per thread
};
template <>
struct Acc<double> {
  using type = double;
  static constexpr int kPX = 1;  // the fp64 ring is twice as wide: own one pixel to stay in registers
};

template <typename scalar_t>
__device__ __forceinline__ typename Acc<scalar_t>::type load_acc(scalar_t v) {
  if constexpr (std::is_same<scalar_t, double>::value) {
    return v;
  } else {
    return to_f32(v);
  }
}

// One (in_h x in_w) tile of slice `g` ([H, W], row-major) -> LDS `s`, zero outside the slice.  Work items are
// (row, 16-byte chunk) pairs; the chunks are aligned in global memory, so a row starts `mis` elements into its first.
template <typename scalar_t>
__device__ __forceinline__ void stage_tile(const scalar_t* __restrict__ g, typename Acc<scalar_t>::type* __restrict__ s,
                                           int H, int W, int r0, int c0, int in_h, int in_w, int tid) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kVec = 16 / sizeof(scalar_t);
  const int nv = (in_w + 2 * kVec - 2) / kVec;  // chunks that cover in_w elements at any misalignment
  const int row_len = min(in_w, W - c0);
  for (int i = tid; i < in_h * nv; i += kThreads) {
    const int r = i / nv, k = i - r * nv;
    const int gr = r0 + r;
    acc_t* srow = s + r * in_w;
    if (gr >= H) {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = k * kVec + e;
        if (col < in_w) srow[col] = acc_t(0);
      }
      continue;
    }
    const scalar_t* grow = g + static_cast<long long>(gr) * W + c0;
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(grow) / sizeof(scalar_t)) & (kVec - 1));
    const int cb = k * kVec - mis;
    if (cb >= 0 && cb + kVec <= row_len) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(grow + cb);
      scalar_t v[kVec];
      __builtin_memcpy(v, &raw, sizeof(raw));
#pragma unroll
      for (int e = 0; e < kVec; ++e) srow[cb + e] = load_acc(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = cb + e;
        if (col >= 0 && col < in_w) srow[col] = col < row_len ? load_acc(grow[col]) : acc_t(0);
      }
    }
  }
}

template <typename scalar_t, int KD>
__global__ void __launch_bounds__(kThreads)
    ssim3d_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y, int D, int H, int W, int kh, int kw,
                  const typename Acc<scalar_t>::type* __restrict__ wd, const typename Acc<scalar_t>::type* __restrict__ wh,
                  const typename Acc<scalar_t>::type* __restrict__ ww, const typename Acc<scalar_t>::type* __restrict__ c12,
                  int tiles_w, int chunk, typename Acc<scalar_t>::type* __restrict__ part) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kPX = Acc<scalar_t>::kPX;
  constexpr int kTH = kWaves * kPX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int in_h = kTH + kh - 1, in_w = kTW + kw - 1;
  acc_t* sx = reinterpret_cast<acc_t*>(smem);
  acc_t* sy = sx + in_h * in_w;
  acc_t* hm = sy + in_h * in_w;  // 5 x [in_h][kTW]
  __shared__ acc_t swh[kMaxK], sww[kMaxK];
  __shared__ acc_t red[2][kWaves];

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kTH, c0 = (tile % tiles_w) * kTW;
  const int out_d = D - KD + 1, out_h = H - kh + 1, out_w = W - kw + 1;
  const int z0 = blockIdx.z * chunk;               // first output slice == first input slice of this block
  const int n_in = min(chunk, out_d - z0) + KD - 1;  // input slices to march over; z0 + n_in <= D
  const long long slice = static_cast<long long>(H) * W;
  const scalar_t* px = x + (plane * D + z0) * slice;
  const scalar_t* py = y + (plane * D + z0) * slice;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  if (tid < kh) swh[tid] = wh[tid];
  if (tid < kw) sww[tid] = ww[tid];
  acc_t wdr[KD];
#pragma unroll
  for (int j = 0; j < KD; ++j) wdr[j] = wd[j];
  const acc_t c1 = c12[0], c2 = c12[1];

  const int row_a = wave * kPX;  // first owned row of the tile; the owned column is `lane`
  bool ok[kPX];
#pragma unroll
  for (int p = 0; p < kPX; ++p) ok[p] = r0 + row_a + p < out_h && c0 + lane < out_w;
  acc_t ring[KD][kPX][5];
#pragma unroll
  for (int q = 0; q < KD; ++q)
#pragma unroll
    for (int p = 0; p < kPX; ++p)
#pragma unroll
      for (int m = 0; m < 5; ++m) ring[q][p][m] = acc_t(0);
  acc_t s_ssim = 0, s_cs = 0;
  const int plane_sz = in_h * kTW;

  for (int s0 = 0; s0 < n_in; s0 += KD) {
#pragma unroll
    for (int r = 0; r < KD; ++r) {
      const int s = s0 + r;  // block-uniform
      if (s < n_in) {
        // the previous slice's W pass (reader of sx / sy) ended before its second barrier
        stage_tile(px + s * slice, sx, H, W, r0, c0, in_h, in_w, tid);
        stage_tile(py + s * slice, sy, H, W, r0, c0, in_h, in_w, tid);
        __syncthreads();  // also: the previous slice's H pass (reader of hm) is done
        for (int i = tid; i < plane_sz; i += kThreads) {
          const int rr = i / kTW, c = i % kTW;
          const acc_t* rx = sx + rr * in_w + c;
          const acc_t* ry = sy + rr * in_w + c;
          acc_t m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;
          for (int j = 0; j < kw; ++j) {
            const acc_t w = sww[j], a = rx[j], b = ry[j];
            m1 += w * a;
            m2 += w * b;
            m3 += w * a * a;
            m4 += w * b * b;
            m5 += w * a * b;
          }
          hm[i] = m1;
          hm[plane_sz + i] = m2;
          hm[2 * plane_sz + i] = m3;
          hm[3 * plane_sz + i] = m4;
          hm[4 * plane_sz + i] = m5;
        }
        __syncthreads();
        // H pass: the kPX owned pixels are vertically adjacent, so each loaded row feeds all of them
        acc_t mom[kPX][5];
#pragma unroll
        for (int p = 0; p < kPX; ++p)
#pragma unroll
          for (int m = 0; m < 5; ++m) mom[p][m] = acc_t(0);
        for (int k = 0; k < kh + kPX - 1; ++k) {
          const int o = (row_a + k) * kTW + lane;
          acc_t v[5];
#pragma unroll
          for (int m = 0; m < 5; ++m) v[m] = hm[m * plane_sz + o];
#pragma unroll
          for (int p = 0; p < kPX; ++p) {
            const int t = k - p;
            const acc_t w = (t >= 0 && t < kh) ? swh[t] : acc_t(0);
#pragma unroll
            for (int m = 0; m < 5; ++m) mom[p][m] += w * v[m];
          }
        }
        // depth ring: input slice s is tap (r - q) mod KD of the output slice pending in slot q
#pragma unroll
        for (int q = 0; q < KD; ++q) {
          const acc_t w = wdr[(r - q + KD) % KD];
#pragma unroll
          for (int p = 0; p < kPX; ++p)
#pragma unroll
            for (int m = 0; m < 5; ++m) ring[q][p][m] += w * mom[p][m];
        }
        const int qd = (r + 1) % KD;  // the slot that just took tap KD - 1: output slice z0 + s - (KD - 1)
        if (s >= KD - 1) {
#pragma unroll
          for (int p = 0; p < kPX; ++p) {
            if (!ok[p]) continue;
            const acc_t mx = ring[qd][p][0], my = ring[qd][p][1];
            const acc_t exx = ring[qd][p][2], eyy = ring[qd][p][3], exy = ring[qd][p][4];
            const acc_t mxx = mx * mx, myy = my * my, mxy = mx * my;
            const acc_t sxx = exx - mxx > 0 ? exx - mxx : acc_t(0);
            const acc_t syy = eyy - myy > 0 ? eyy - myy : acc_t(0);
            const acc_t sxy = exy - mxy;
            const acc_t upper = 2 * sxy + c2;
            const acc_t lower = sxx + syy + c2;
            s_ssim += ((2 * mxy + c1) * upper) / ((mxx + myy + c1) * lower);
            s_cs += upper / lower;
          }
        }
#pragma unroll
        for (int p = 0; p < kPX; ++p)
#pragma unroll
          for (int m = 0; m < 5; ++m) ring[qd][p][m] = acc_t(0);
      }
    }
  }
  s_ssim = wave_sum(s_ssim);
  s_cs = wave_sum(s_cs);
  if (lane == 0) {
    red[0][wave] = s_ssim;
    red[1][wave] = s_cs;
  }
  __syncthreads();
  if (tid == 0) {
    acc_t a = 0, b = 0;
    for (int w = 0; w < kWaves; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    const long long slot = (plane * gridDim.z + blockIdx.z) * gridDim.x + tile;
    part[slot * 2] = a;
    part[slot * 2 + 1] = b;
  }
}

}  // namespace

// x, y: [P, D, H, W] volumes (contiguous, same dtype); wd [kd], wh [kh], ww [kw] separable window taps and c12 [3]
// (c1, c2, eps) in the accumulation dtype (f32, or f64 for f64 inputs).  depth_chunk > 0 forces the number of output
// slices per block, 0 lets the launcher pick.  Returns part [P, chunks * tiles, 2] of per-block (sum SSIM, sum CS)
// over the valid windows.
at::Tensor ssim3d_partials(const at::Tensor& x, const at::Tensor& y, const at::Tensor& wd, const at::Tensor& wh,
                           const at::Tensor& ww, const at::Tensor& c12, int64_t depth_chunk) {
  TM_CHECK_CUDA(x);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type(), "ssim3d: x / y mismatch");
  TORCH_CHECK(x.dim() == 4, "ssim3d: expects [planes, D, H, W]");
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, wd);
  TM_SAME_DEVICE(x, wh);
  TM_SAME_DEVICE(x, ww);
  TM_SAME_DEVICE(x, c12);
  const int kd = static_cast<int>(wd.numel()), kh = static_cast<int>(wh.numel()), kw = static_cast<int>(ww.numel());
  TORCH_CHECK(kd >= 1 && kd <= kMaxKD && kd % 2 == 1, "ssim3d: depth window must be odd and 1..", kMaxKD);
  TORCH_CHECK(kh >= 1 && kw >= 1 && kh <= kMaxK && kw <= kMaxK, "ssim3d: in-plane window must be 1..", kMaxK);
  const long long planes = x.size(0);
  TORCH_CHECK(x.size(1) < (1 << 30) && x.size(2) < (1 << 30) && x.size(3) < (1 << 30), "ssim3d: extent too large");
  const int D = static_cast<int>(x.size(1)), H = static_cast<int>(x.size(2)), W = static_cast<int>(x.size(3));
  TORCH_CHECK(D >= kd && H >= kh && W >= kw, "ssim3d: volume smaller than the window");
  TORCH_CHECK(planes <= 65535, "ssim3d: too many planes for one launch");
  TORCH_CHECK(depth_chunk >= 0, "ssim3d: depth_chunk must be >= 0");
  const bool dbl = x.scalar_type() == at::kDouble;
  const auto acc_type = dbl ? at::kDouble : at::kFloat;
  TORCH_CHECK(c12.numel() >= 3, "ssim3d: c12 must hold (c1, c2, eps)");
  TORCH_CHECK(wd.scalar_type() == acc_type && wh.scalar_type() == acc_type && ww.scalar_type() == acc_type &&
                  c12.scalar_type() == acc_type,
              "ssim3d: window / constants must be in the accumulation dtype");
  TM_CHECK_CONTIG(wd);
  TM_CHECK_CONTIG(wh);
  TM_CHECK_CONTIG(ww);
  TM_CHECK_CONTIG(c12);
  const int th = kWaves * (dbl ? Acc<double>::kPX : Acc<float>::kPX);
  const int out_d = D - kd + 1, out_h = H - kh + 1, out_w = W - kw + 1;
  const int tiles_w = (out_w + kTW - 1) / kTW, tiles_h = (out_h + th - 1) / th;
  const long long tiles = static_cast<long long>(tiles_w) * tiles_h;
  TORCH_CHECK(tiles < (1LL << 31), "ssim3d: too many in-plane tiles for one launch");
  long long chunk = depth_chunk;
  if (chunk == 0) {
    // the longest chunk that still leaves ~2 blocks per CU (every chunk re-reads kd - 1 halo slices), not below kd
    const long long want = 2LL * cu_count(x.get_device());
    const long long in_plane = std::max<long long>(1, tiles * planes);
    const long long n_chunks = (want + in_plane - 1) / in_plane;
    chunk = std::max<long long>(out_d / n_chunks, kd);
  }
  chunk = std::min<long long>(chunk, out_d);
  const int chunks = static_cast<int>((out_d + chunk - 1) / chunk);
  TORCH_CHECK(chunks <= 65535, "ssim3d: too many depth chunks for one launch");
  at::Tensor part = at::empty({planes, chunks * tiles, 2}, x.options().dtype(acc_type));
  if (planes == 0) return part;
  const int in_h = th + kh - 1, in_w = kTW + kw - 1;
  const size_t esz = dbl ? sizeof(double) : sizeof(float);
  const size_t lds = esz * (2 * static_cast<size_t>(in_h) * in_w + 5 * static_cast<size_t>(in_h) * kTW);
  TORCH_CHECK(lds <= 150 * 1024, "ssim3d: window too large for the LDS tile (use a smaller kernel / fp32 inputs)");
  auto s = stream();
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(planes), static_cast<unsigned>(chunks));
  TM_DISPATCH_FLOAT(x.scalar_type(), "ssim3d", [&] {
    using acc_t = typename Acc<scalar_t>::type;
    auto launch = [&](auto kd_c) {
      constexpr int KD = decltype(kd_c)::value;
      if (lds > 64 * 1024) {
        TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ssim3d_kernel<scalar_t, KD>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        static_cast<int>(lds)) == hipSuccess,
                    "ssim3d: could not raise the dynamic LDS limit");
      }
      hipLaunchKernelGGL((ssim3d_kernel<scalar_t, KD>), grid, dim3(kThreads), lds, s,
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),
                         reinterpret_cast<const scalar_t*>(y.data_ptr()), D, H, W, kh, kw, wd.data_ptr<acc_t>(),
                         wh.data_ptr<acc_t>(), ww.data_ptr<acc_t>(), c12.data_ptr<acc_t>(), tiles_w,
                         static_cast<int>(chunk), part.data_ptr<acc_t>());
    };
    switch (kd) {
      case 1: launch(std::integral_constant<int, 1>{}); break;
      case 3: launch(std::integral_constant<int, 3>{}); break;
      case 5: launch(std::integral_constant<int, 5>{}); break;
      case 7: launch(std::integral_constant<int, 7>{}); break;
      case 9: launch(std::integral_constant<int, 9>{}); break;
      default: launch(std::integral_constant<int, 11>{}); break;
    }
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return part;
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def(
      "ssim3d_partials(Tensor x, Tensor y, Tensor wd, Tensor wh, Tensor ww, Tensor c12, int depth_chunk) -> Tensor");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) { m.impl("ssim3d_partials", &tm_amd::ssim3d_partials); }
