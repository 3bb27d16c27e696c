// Fused backward of the 2-D SSIM / contrast-sensitivity window sums (the gradient of ssim.hip's mode 0).
//
// The forward convolves five moment maps (x, y, x^2, y^2, xy) with the separable window and sums SSIM and CS over
// the valid windows of a plane.  With g = (gs, gc) the upstream gradient of those two sums, every valid window j
// has five coefficients -- d/d(mu_x), d/d(E[x^2]), d/d(E[xy]), d/d(mu_y), d/d(E[y^2]) -- and
//
//   grad_x[i] = sum_j w[i-j] (g_a[j] + 2 x[i] g_exx[j] + y[i] g_exy[j])        (grad_y likewise with g_b, g_eyy)
//
// i.e. the transposed convolution of the coefficient maps with the same window.  Nothing is kept from the forward:
// a block recomputes the window statistics it needs from x and y, so autograd saves the two inputs only.
//
//   block = 16 x 32 tile of INPUT-GRADIENT pixels of one plane, 256 threads (4 wave64), every thread owns 2 pixels
//   with nh = 16 + kh - 1, nw = 32 + kw - 1 (windows touching the tile), ih = 16 + 2(kh-1), iw = 32 + 2(kw-1):
//   1. stage the ih x iw tile of x and y (halo of k-1 on every side, zero outside the image) in LDS as acc_t;
//      the owned centre pixels go to registers, after which the staged tile is only needed by step 2
//   2. row pass: 5 moments per (input row, window col) -> hm [5][ih][nw].  The second one is of x - y, not of y:
//      mu_y = mu_x - mu_d costs nothing, and d/dc1 = sum gA mu_d^2 / B1 (= sum gA + gB, where mu_x ~ mu_y cancels
//      all but a few bits of an fp32 1 - A1 / B1) then comes from an accurately known mu_d
//   3. column pass per window -> mu, E[..] -> the coefficient maps coef [NC][nh][nw], written OVER the dead x / y
//      tile; windows outside [0, out_h) x [0, out_w) get zeros.  NC = 5, or 3 (g_a, g_exx, g_exy) when grad_y is
//      not wanted: that variant is a separate instantiation that never forms or filters the y maps.
//      The window (r, c) is owned by the tile that holds pixel (r, c): owned windows add (gA + gB, gU + gL) to the
//      block's d/dc1, d/dc2 partial (every window counted once across the grid; fixed order, no atomics).
//   4. transposed column pass: t [NC][16][nw] over the dead hm
//   5. transposed row pass per owned pixel, combined with the centre x / y from registers, rounded once on store.
//
// LDS = sizeof(acc_t) * (max(NC nh nw, 2 ih iw) + 5 ih nw) + taps:
//   11 x 11, fp32: max(5*26*42, 2*36*52) + 5*36*42 = 5460 + 7560 = 13020 words = 50.9 KB -> 3 blocks / CU
//   11 x 11, fp64: 101.7 KB -> 1 block / CU (same tile; the fp64 path is for checking, not for speed)
//   15 x 15, fp64: (max(6900, 5280) + 10120) * 8 = 133 KB, the largest request; 17 x 17 fp64 would need 150 KB.
// Windows up to kMaxK = 15 on either edge are served for every dtype; larger ones stay on the convolution path
// (torchmetrics_amd/functional/image/ssim.py checks the same limit before it calls this op).
#include "../common/tm_common.h"

#include <algorithm>
#include <tuple>
#include <type_traits>

namespace tm_amd {
namespace {

constexpr int kGH = 16;     // gradient rows per block
constexpr int kGW = 32;     // gradient cols per block
constexpr int kMaxK = 15;   // largest window edge of the fused backward
constexpr int kThreads = 256;
constexpr int kOwn = kGH * kGW / kThreads;  // pixels per thread in the last pass

template <typename T>
struct Acc {
  using type = float;
};
template <>
struct Acc<double> {
  using type = double;
};

template <typename scalar_t>
__device__ __forceinline__ typename Acc<scalar_t>::type load_acc(scalar_t v) {
  if constexpr (std::is_same<scalar_t, double>::value) {
    return v;
  } else {
    return to_f32(v);
  }
}

template <typename scalar_t, bool kNeedY>
__global__ void __launch_bounds__(kThreads)
    ssim2d_backward_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y, int H, int W, int kh, int kw,
                           const typename Acc<scalar_t>::type* __restrict__ wh,
                           const typename Acc<scalar_t>::type* __restrict__ ww,
                           const typename Acc<scalar_t>::type* __restrict__ c12,
                           const typename Acc<scalar_t>::type* __restrict__ g, int tiles_w, scalar_t* __restrict__ gx,
                           scalar_t* __restrict__ gy, typename Acc<scalar_t>::type* __restrict__ gc_part) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int NC = kNeedY ? 5 : 3;  // coefficient maps: g_a, g_exx, g_exy (, g_b, g_eyy)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ih = kGH + 2 * (kh - 1), iw = kGW + 2 * (kw - 1);
  const int nh = kGH + kh - 1, nw = kGW + kw - 1;
  const int in_sz = ih * iw, hm_sz = ih * nw, co_sz = nh * nw, t_sz = kGH * nw;
  acc_t* sx = reinterpret_cast<acc_t*>(smem);
  acc_t* sy = sx + in_sz;
  acc_t* coef = sx;  // steps 3-4, over the staged tile
  acc_t* hm = sx + max(NC * co_sz, 2 * in_sz);
  acc_t* tm = hm;  // steps 4-5, over the row-pass moments
  __shared__ acc_t swh[kMaxK], sww[kMaxK];
  __shared__ acc_t red[2][kThreads / kWave];

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kGH, c0 = (tile % tiles_w) * kGW;
  const int rs = r0 - (kh - 1), cs = c0 - (kw - 1);  // image coordinates of local (0, 0): staged tile and windows
  const scalar_t* px = x + plane * H * W;
  const scalar_t* py = y + plane * H * W;
  const int tid = threadIdx.x;
  if (tid < kh) swh[tid] = wh[tid];
  if (tid < kw) sww[tid] = ww[tid];
  // 1. stage
  for (int i = tid; i < in_sz; i += kThreads) {
    const int r = i / iw, c = i - r * iw;
    const int gr = rs + r, gc = cs + c;
    const bool ok = gr >= 0 && gr < H && gc >= 0 && gc < W;
    const long long o = static_cast<long long>(gr) * W + gc;
    sx[i] = ok ? load_acc(px[o]) : acc_t(0);
    sy[i] = ok ? load_acc(py[o]) : acc_t(0);
  }
  __syncthreads();
  acc_t cx[kOwn], cy[kOwn];
#pragma unroll
  for (int n = 0; n < kOwn; ++n) {
    const int p = tid + n * kThreads;
    const int o = (p / kGW + kh - 1) * iw + (p % kGW) + kw - 1;
    cx[n] = sx[o];
    cy[n] = sy[o];
  }
  // 2. row pass: window col c of the tile covers staged cols c .. c + kw - 1
  for (int i = tid; i < hm_sz; i += kThreads) {
    const int r = i / nw, c = i - r * nw;
    const acc_t* rx = sx + r * iw + c;
    const acc_t* ry = sy + r * iw + c;
    acc_t m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;
    for (int j = 0; j < kw; ++j) {
      const acc_t w = sww[j], a = rx[j], b = ry[j];
      m1 += w * a;
      m2 += w * (a - b);
      m3 += w * a * a;
      m4 += w * b * b;
      m5 += w * a * b;
    }
    hm[i] = m1;
    hm[hm_sz + i] = m2;
    hm[2 * hm_sz + i] = m3;
    hm[3 * hm_sz + i] = m4;
    hm[4 * hm_sz + i] = m5;
  }
  __syncthreads();
  // 3. column pass -> window statistics -> coefficient maps (over sx / sy, dead since the barrier above)
  const acc_t c1 = c12[0], c2 = c12[1];
  const acc_t gs = g[plane * 2], gcs = g[plane * 2 + 1];
  const int out_h = H - kh + 1, out_w = W - kw + 1;
  acc_t dc1 = 0, dc2 = 0;
  for (int i = tid; i < co_sz; i += kThreads) {
    const int r = i / nw, c = i - r * nw;
    const int wr = rs + r, wc = cs + c;
    acc_t g_a = 0, g_exx = 0, g_exy = 0, g_b = 0, g_eyy = 0;
    if (wr >= 0 && wr < out_h && wc >= 0 && wc < out_w) {
      acc_t a = 0, d = 0, exx = 0, eyy = 0, exy = 0;
      for (int k = 0; k < kh; ++k) {
        const int o = (r + k) * nw + c;
        const acc_t w = swh[k];
        a += w * hm[o];
        d += w * hm[hm_sz + o];
        exx += w * hm[2 * hm_sz + o];
        eyy += w * hm[3 * hm_sz + o];
        exy += w * hm[4 * hm_sz + o];
      }
      const acc_t b = a - d;
      const acc_t vx = exx - a * a, vy = eyy - b * b;
      const acc_t kx = vx >= 0 ? acc_t(1) : acc_t(0), ky = vy >= 0 ? acc_t(1) : acc_t(0);  // clamp(min=0) gradient
      const acc_t sxx = vx > 0 ? vx : acc_t(0), syy = vy > 0 ? vy : acc_t(0), sxy = exy - a * b;
      const acc_t A1 = 2 * a * b + c1, B1 = a * a + b * b + c1;
      const acc_t U = 2 * sxy + c2, L = sxx + syy + c2;
      const acc_t S = (A1 * U) / (B1 * L), CS = U / L;
      const acc_t gU = gs * A1 / (B1 * L) + gcs / L;
      const acc_t gL = -(gs * S + gcs * CS) / L;
      const acc_t gA = gs * U / (B1 * L);
      const acc_t gB = -gs * S / B1;
      g_a = 2 * b * gA + 2 * a * gB - 2 * b * gU - 2 * a * kx * gL;
      g_exx = kx * gL;
      g_exy = 2 * gU;
      if constexpr (kNeedY) {
        g_b = 2 * a * gA + 2 * b * gB - 2 * a * gU - 2 * b * ky * gL;
        g_eyy = ky * gL;
      }
      if (wr >= r0 && wc >= c0) {  // this tile's own windows (wr < r0 + kGH and wc < c0 + kGW always hold)
        // gA + gB and gU + gL with the c1 / c2 that cancel in them taken out: B1 - A1 = d^2, L - U = sxx + syy - 2 sxy
        dc1 += gA * d * d / B1;
        dc2 += (gs * A1 / B1 + gcs) * (sxx + syy - 2 * sxy) / (L * L);
      }
    }
    coef[i] = g_a;
    coef[co_sz + i] = g_exx;
    coef[2 * co_sz + i] = g_exy;
    if constexpr (kNeedY) {
      coef[3 * co_sz + i] = g_b;
      coef[4 * co_sz + i] = g_eyy;
    }
  }
  __syncthreads();
  // 4. transposed column pass (over hm): pixel row r takes window rows r + kh - 1 - k with weight wh[k]
  for (int i = tid; i < t_sz; i += kThreads) {
    const int r = i / nw, c = i - r * nw;
    acc_t t[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) t[m] = 0;
    for (int k = 0; k < kh; ++k) {
      const int o = (r + kh - 1 - k) * nw + c;
      const acc_t w = swh[k];
#pragma unroll
      for (int m = 0; m < NC; ++m) t[m] += w * coef[m * co_sz + o];
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) tm[m * t_sz + i] = t[m];
  }
  __syncthreads();
  // 5. transposed row pass per owned pixel: pixel col c takes window cols c + kw - 1 - k with weight ww[k]
#pragma unroll
  for (int n = 0; n < kOwn; ++n) {
    const int p = tid + n * kThreads;
    const int r = p / kGW, c = p % kGW;
    if (r0 + r >= H || c0 + c >= W) continue;
    acc_t t[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) t[m] = 0;
    for (int k = 0; k < kw; ++k) {
      const int o = r * nw + c + kw - 1 - k;
      const acc_t w = sww[k];
#pragma unroll
      for (int m = 0; m < NC; ++m) t[m] += w * tm[m * t_sz + o];
    }
    const long long o = plane * H * W + static_cast<long long>(r0 + r) * W + c0 + c;
    gx[o] = static_cast<scalar_t>(t[0] + 2 * cx[n] * t[1] + cy[n] * t[2]);
    if constexpr (kNeedY) gy[o] = static_cast<scalar_t>(t[NC - 2] + 2 * cy[n] * t[NC - 1] + cx[n] * t[2]);
  }
  // d/dc1, d/dc2 of this tile's own windows
  if (gc_part == nullptr) return;  // uniform over the grid
  dc1 = wave_sum(dc1);
  dc2 = wave_sum(dc2);
  const int wave = tid / kWave;
  if ((tid & (kWave - 1)) == 0) {
    red[0][wave] = dc1;
    red[1][wave] = dc2;
  }
  __syncthreads();
  if (tid == 0) {
    acc_t a = 0, b = 0;
    for (int w = 0; w < kThreads / kWave; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    const long long slot = plane * gridDim.x + tile;
    gc_part[slot * 2] = a;
    gc_part[slot * 2 + 1] = b;
  }
}

template <typename scalar_t, bool kNeedY>
void launch(const at::Tensor& x, const at::Tensor& y, const at::Tensor& wh, const at::Tensor& ww,
            const at::Tensor& c12, const at::Tensor& g, int tiles, int tiles_w, size_t lds, at::Tensor& gx,
            at::Tensor& gy, at::Tensor& gc_part, bool need_c) {
  using acc_t = typename Acc<scalar_t>::type;
  auto* kern = &ssim2d_backward_kernel<scalar_t, kNeedY>;
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)) == hipSuccess,
                "ssim2d_backward: could not raise the dynamic LDS limit");
  }
  hipLaunchKernelGGL(kern, dim3(tiles, static_cast<unsigned>(x.size(0))), dim3(kThreads), lds, stream(),
                     reinterpret_cast<const scalar_t*>(x.data_ptr()), reinterpret_cast<const scalar_t*>(y.data_ptr()),
                     static_cast<int>(x.size(1)), static_cast<int>(x.size(2)), static_cast<int>(wh.numel()),
                     static_cast<int>(ww.numel()), wh.data_ptr<acc_t>(), ww.data_ptr<acc_t>(), c12.data_ptr<acc_t>(),
                     g.data_ptr<acc_t>(), tiles_w, reinterpret_cast<scalar_t*>(gx.data_ptr()),
                     kNeedY ? reinterpret_cast<scalar_t*>(gy.data_ptr()) : nullptr,
                     need_c ? gc_part.data_ptr<acc_t>() : nullptr);
}

}  // namespace

// x, y: [P, H, W] planes (contiguous, same dtype); wh [kh], ww [kw], c12 [>= 2] as for ssim2d_partials; g [P, 2]:
// upstream gradient of each plane's (sum SSIM, sum CS) over its valid windows, in the accumulation dtype.
// Returns (gx, gy or an empty tensor, gc_part [P, tiles, 2] of per-tile (d/dc1, d/dc2) or an empty tensor).
std::tuple<at::Tensor, at::Tensor, at::Tensor> ssim2d_backward(const at::Tensor& x, const at::Tensor& y,
                                                               const at::Tensor& wh, const at::Tensor& ww,
                                                               const at::Tensor& c12, const at::Tensor& g,
                                                               bool need_y, bool need_c) {
  TM_CHECK_CUDA(x);
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, wh);
  TM_SAME_DEVICE(x, ww);
  TM_SAME_DEVICE(x, c12);
  TM_SAME_DEVICE(x, g);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TM_CHECK_CONTIG(wh);
  TM_CHECK_CONTIG(ww);
  TM_CHECK_CONTIG(c12);
  TM_CHECK_CONTIG(g);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type(), "ssim2d_backward: x / y mismatch");
  TORCH_CHECK(x.dim() == 3, "ssim2d_backward: expects [planes, H, W]");
  const int kh = static_cast<int>(wh.numel()), kw = static_cast<int>(ww.numel());
  TORCH_CHECK(kh >= 1 && kw >= 1 && kh <= kMaxK && kw <= kMaxK, "ssim2d_backward: window must be 1..", kMaxK);
  const long long planes = x.size(0);
  TORCH_CHECK(x.size(1) < (1 << 30) && x.size(2) < (1 << 30), "ssim2d_backward: image too large");
  const int H = static_cast<int>(x.size(1)), W = static_cast<int>(x.size(2));
  TORCH_CHECK(H >= kh && W >= kw, "ssim2d_backward: image smaller than the window");
  TORCH_CHECK(planes <= 65535, "ssim2d_backward: too many planes for one launch");
  const bool dbl = x.scalar_type() == at::kDouble;
  const auto acc_type = dbl ? at::kDouble : at::kFloat;
  TORCH_CHECK(c12.numel() >= 2, "ssim2d_backward: c12 must hold (c1, c2)");
  TORCH_CHECK(wh.scalar_type() == acc_type && ww.scalar_type() == acc_type && c12.scalar_type() == acc_type &&
                  g.scalar_type() == acc_type,
              "ssim2d_backward: window / constants / upstream gradient must be in the accumulation dtype");
  TORCH_CHECK(g.dim() == 2 && g.size(0) == planes && g.size(1) == 2, "ssim2d_backward: g must be [planes, 2]");
  const int tiles_w = (W + kGW - 1) / kGW, tiles_h = (H + kGH - 1) / kGH;
  const long long tiles_ll = static_cast<long long>(tiles_w) * tiles_h;
  TORCH_CHECK(tiles_ll < (1LL << 31), "ssim2d_backward: too many tiles for one launch");
  const int tiles = static_cast<int>(tiles_ll);
  at::Tensor gx = at::empty_like(x);
  at::Tensor gy = need_y ? at::empty_like(y) : at::empty({0}, x.options());
  const int64_t gc_p = need_c ? planes : 0, gc_t = need_c ? tiles : 0;
  at::Tensor gc_part = at::empty({gc_p, gc_t, 2}, x.options().dtype(acc_type));
  if (planes == 0) return {gx, gy, gc_part};
  const size_t ih = kGH + 2 * (kh - 1), iw = kGW + 2 * (kw - 1), nh = kGH + kh - 1, nw = kGW + kw - 1;
  const size_t nc = need_y ? 5 : 3;
  const size_t esz = dbl ? sizeof(double) : sizeof(float);
  const size_t lds = esz * (std::max(nc * nh * nw, 2 * ih * iw) + 5 * ih * nw);
  TORCH_CHECK(lds <= 150 * 1024, "ssim2d_backward: window too large for the LDS tile");
  TM_DISPATCH_FLOAT(x.scalar_type(), "ssim2d_backward", [&] {
    if (need_y) {
      launch<scalar_t, true>(x, y, wh, ww, c12, g, tiles, tiles_w, lds, gx, gy, gc_part, need_c);
    } else {
      launch<scalar_t, false>(x, y, wh, ww, c12, g, tiles, tiles_w, lds, gx, gy, gc_part, need_c);
    }
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {gx, gy, gc_part};
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def(
      "ssim2d_backward(Tensor x, Tensor y, Tensor wh, Tensor ww, Tensor c12, Tensor g, bool need_y, bool need_c) -> "
      "(Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) { m.impl("ssim2d_backward", &tm_amd::ssim2d_backward); }
