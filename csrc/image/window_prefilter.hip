// Windowed image statistics with the prefilter fused into the window kernel's LDS tile: one VIF pyramid scale (Gaussian
// blur + 2x decimation, then the VIF window terms) and SCC (symmetric-padded high-pass convolution, then the zero-padded
// uniform-window correlation).
//
// Both metrics are "small prefilter -> five windowed second moments of the filtered planes -> per-window formula -> sum".
// csrc/image/ssim.hip runs everything after the prefilter in one launch; the prefilter used to be a vendor convolution
// with padded / strided / re-packed temporaries around it.  Here the filtered tile is built in LDS by the block that
// consumes it, with the same 16 x 64 window tile, 256 threads, fixed-order block reduction and one partial per block.
//
// vif_scale_kernel, taps n, block = 16 x TW windows of the decimated plane (TW = 64; 32 for fp64):
//   1. stage the (2*(16+n-1)+n-2) x (2*(TW+n-1)+n-2) source tile of x and y in LDS, widened to the accumulation type
//      (4-element vector loads when the rows are aligned)                                  [55 x 151 at n = 9]
//   2. vertical taps at the even rows only -> (16+n-1) x src_w, then horizontal taps at the even columns only ->
//      the decimated (16+n-1) x (TW+n-1) tile: no pixel the decimation drops is ever computed.  The vertical pass
//      comes first because it shrinks the larger extent of the intermediate (96 KB of LDS at n = 9 in fp32; the
//      other order needs 98 KB and does not fit 17 taps).
//   3. the block writes the decimated pixels it owns (its 16 x TW origin region; the last tile row / column also the
//      trailing n-1 halo) for the next scale to read: every pixel is written by exactly one block
//   4. horizontal then vertical windowed moments of the decimated tile, the VIF terms of ssim2d_kernel's mode 2,
//      block reduction -> (numerator, denominator) partial
//   The source tile is dead after 2, the vertical intermediate after the decimated tile exists: the decimated tile and
//   the horizontal moments reuse their LDS.
//
// scc_kernel, filter kh x kw, window ws, block = 16 x 64 outputs of the H x W correlation map:
//   1. stage the (16+ws-1+kh-1) x (64+ws-1+kw-1) input tile with the symmetric (edge-repeating) border folded into the
//      index arithmetic
//   2. true convolution (flipped taps) x 2 -> the (16+ws-1) x (64+ws-1) high-pass tile, zero outside the image (the
//      zero padding of the window stage)
//   3. uniform separable window moments (the horizontal moments reuse the input tile's LDS), cov / (sd_x sd_y) with 0
//      where undefined, block reduction -> one partial
#include "../common/tm_common.h"

namespace tm_amd {
namespace {

constexpr int kTH = 16;         // window rows per block
constexpr int kThreads = 256;
constexpr int kMaxTaps = 17;    // VIF blur / window taps
constexpr int kMaxFilt = 9;     // SCC high-pass filter edge
constexpr int kMaxWin = 33;     // SCC window edge
constexpr size_t kLdsLimit = 160 * 1024 - 512;  // gfx950 workgroup LDS less the static arrays below

template <typename T>
struct Acc {
  using type = float;
};
template <>
struct Acc<double> {
  using type = double;
};

// window columns per block of the VIF kernel: fp64 takes half the tile so that the 9-tap scale fits the LDS
template <typename T>
constexpr int kVifTW = 64;
template <>
constexpr int kVifTW<double> = 32;

template <typename T>
struct alignas(sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16) Vec4 {
  T v[4];
};

// an input element in the accumulation type (fp64 stays fp64: to_f32 would round it)
template <typename acc_t, typename T>
__device__ __forceinline__ acc_t widen(T v) {
  if constexpr (std::is_same<T, acc_t>::value) {
    return v;
  } else {
    return static_cast<acc_t>(to_f32(v));
  }
}

// fixed-order sum of (a, b) over the block; valid in thread 0
template <typename acc_t>
__device__ __forceinline__ void block_sum2(acc_t& a, acc_t& b, acc_t (*red)[kThreads / kWave]) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int tid = threadIdx.x, wave = tid / kWave;
  if ((tid & (kWave - 1)) == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (tid == 0) {
    a = 0;
    b = 0;
    for (int w = 0; w < kThreads / kWave; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
  }
}

// horizontal pass of the five windowed moments: t [rows][tw_in] of x and y -> hm 5 x [rows][TW]
template <typename acc_t, int TW, bool UNIFORM>
__device__ __forceinline__ void moments_rows(const acc_t* tx, const acc_t* ty, int rows, int tw_in, int k,
                                             const acc_t* wk, acc_t* hm) {
  const int plane_sz = rows * TW;
  for (int i = threadIdx.x; i < plane_sz; i += kThreads) {
    const int r = i / TW, c = i % TW;
    const acc_t* rx = tx + r * tw_in + c;
    const acc_t* ry = ty + r * tw_in + c;
    acc_t m1 = 0, m2 = 0, m3 = 0, m4 = 0, m5 = 0;
    for (int j = 0; j < k; ++j) {
      const acc_t w = UNIFORM ? acc_t(1) : wk[j], a = rx[j], b = ry[j];
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
}

template <typename scalar_t, int TW>
__global__ void __launch_bounds__(kThreads) vif_scale_kernel(const scalar_t* __restrict__ x,
                                                             const scalar_t* __restrict__ y, int H, int W, int n,
                                                             const typename Acc<scalar_t>::type* __restrict__ taps,
                                                             const typename Acc<scalar_t>::type* __restrict__ c12,
                                                             int Hd, int Wd, int tiles_h, int tiles_w, int vec,
                                                             typename Acc<scalar_t>::type* __restrict__ xd,
                                                             typename Acc<scalar_t>::type* __restrict__ yd,
                                                             typename Acc<scalar_t>::type* __restrict__ part) {
  using acc_t = typename Acc<scalar_t>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ acc_t sk[kMaxTaps];
  __shared__ acc_t red[2][kThreads / kWave];
  const int dh = kTH + n - 1, dw = TW + n - 1;          // decimated tile
  const int sh = 2 * dh + n - 2, sw = 2 * dw + n - 2;   // source tile
  acc_t* sx = reinterpret_cast<acc_t*>(smem);           // [sh][sw]
  acc_t* sy = sx + sh * sw;
  acc_t* vx = sy + sh * sw;                             // [dh][sw], even rows after the vertical taps
  acc_t* vy = vx + dh * sw;
  acc_t* dx = sx;                                       // [dh][dw], over the dead source tile
  acc_t* dy = dx + dh * dw;
  acc_t* hm = dy + dh * dw;                             // 5 x [dh][TW], over the dead source tile and intermediate

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x, tr = tile / tiles_w, tc = tile % tiles_w;
  const int r0 = tr * kTH, c0 = tc * TW;  // origin in the decimated plane; 2 r0, 2 c0 in the source
  const scalar_t* px = x + plane * H * W;
  const scalar_t* py = y + plane * H * W;
  const int tid = threadIdx.x;
  if (tid < n) sk[tid] = taps[tid];

  // 1. source tile (zero outside the image: such pixels only reach decimated pixels that nothing uses)
  const int sw4 = (sw + 3) / 4;
  for (int i = tid; i < sh * sw4; i += kThreads) {
    const int r = i / sw4, c = (i % sw4) * 4;
    const int gr = 2 * r0 + r, gc = 2 * c0 + c;
    const long long g = static_cast<long long>(gr) * W + gc;
    acc_t ax[4], ay[4];
    if (vec && gr < H && gc + 3 < W) {
      const Vec4<scalar_t> qx = *reinterpret_cast<const Vec4<scalar_t>*>(px + g);
      const Vec4<scalar_t> qy = *reinterpret_cast<const Vec4<scalar_t>*>(py + g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ax[e] = widen<acc_t>(qx.v[e]);
        ay[e] = widen<acc_t>(qy.v[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = gr < H && gc + e < W;
        ax[e] = ok ? widen<acc_t>(px[g + e]) : acc_t(0);
        ay[e] = ok ? widen<acc_t>(py[g + e]) : acc_t(0);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e < sw) {
        sx[r * sw + c + e] = ax[e];
        sy[r * sw + c + e] = ay[e];
      }
    }
  }
  __syncthreads();
  // 2a. vertical taps at the even rows
  for (int i = tid; i < dh * sw; i += kThreads) {
    const int r = i / sw, c = i % sw;
    const acc_t* qx = sx + 2 * r * sw + c;
    const acc_t* qy = sy + 2 * r * sw + c;
    acc_t a = 0, b = 0;
    for (int k = 0; k < n; ++k) {
      a += sk[k] * qx[k * sw];
      b += sk[k] * qy[k * sw];
    }
    vx[i] = a;
    vy[i] = b;
  }
  __syncthreads();
  // 2b. horizontal taps at the even columns -> decimated tile; 3. the pixels this block owns go to global memory
  const int own_h = tr == tiles_h - 1 ? dh : kTH, own_w = tc == tiles_w - 1 ? dw : TW;
  for (int i = tid; i < dh * dw; i += kThreads) {
    const int r = i / dw, c = i % dw;
    const acc_t* qx = vx + r * sw + 2 * c;
    const acc_t* qy = vy + r * sw + 2 * c;
    acc_t a = 0, b = 0;
    for (int k = 0; k < n; ++k) {
      a += sk[k] * qx[k];
      b += sk[k] * qy[k];
    }
    dx[i] = a;
    dy[i] = b;
    if (r < own_h && c < own_w && r0 + r < Hd && c0 + c < Wd) {
      const long long o = (plane * Hd + r0 + r) * Wd + c0 + c;
      xd[o] = a;
      yd[o] = b;
    }
  }
  __syncthreads();
  // 4. windowed moments of the decimated tile and the VIF terms (x = reference, y = distorted)
  moments_rows<acc_t, TW, false>(dx, dy, dh, dw, n, sk, hm);
  __syncthreads();
  const acc_t sn = c12[0], eps = c12[2];
  const int out_h = Hd - n + 1, out_w = Wd - n + 1;
  const int plane_sz = dh * TW;
  acc_t s_num = 0, s_den = 0;
  for (int i = tid; i < kTH * TW; i += kThreads) {
    const int r = i / TW, c = i % TW;
    if (r0 + r >= out_h || c0 + c >= out_w) continue;
    acc_t mx = 0, my = 0, exx = 0, eyy = 0, exy = 0;
    for (int k = 0; k < n; ++k) {
      const int o = (r + k) * TW + c;
      const acc_t w = sk[k];
      mx += w * hm[o];
      my += w * hm[plane_sz + o];
      exx += w * hm[2 * plane_sz + o];
      eyy += w * hm[3 * plane_sz + o];
      exy += w * hm[4 * plane_sz + o];
    }
    const acc_t sxx = exx - mx * mx > 0 ? exx - mx * mx : acc_t(0);
    const acc_t syy = eyy - my * my > 0 ? eyy - my * my : acc_t(0);
    const acc_t sxy = exy - mx * my;
    acc_t stt = sxx, g = sxy / (sxx + eps), sv = syy - g * sxy;
    if (stt < eps) {
      g = 0;
      sv = syy;
      stt = 0;
    }
    if (syy < eps) {
      g = 0;
      sv = 0;
    }
    if (g < 0) {
      sv = syy;
      g = 0;
    }
    sv = sv > eps ? sv : eps;
    s_num += log10(acc_t(1) + g * g * stt / (sv + sn));
    s_den += log10(acc_t(1) + stt / sn);
  }
  block_sum2(s_num, s_den, red);
  if (tid == 0) {
    const long long slot = plane * gridDim.x + tile;
    part[slot * 2] = s_num;
    part[slot * 2 + 1] = s_den;
  }
}

// mirror an index of the symmetric-padded axis back into [0, n); clamped where even the mirror lies outside (such
// inputs only reach high-pass positions outside the image, which are zeroed)
__device__ __forceinline__ int sym_index(int g, int n) {
  if (g < 0) g = -g - 1;
  if (g >= n) g = 2 * n - 1 - g;
  return g < 0 ? 0 : (g >= n ? n - 1 : g);
}

constexpr int kSccTW = 64;

__global__ void __launch_bounds__(kThreads) scc_kernel(const float* __restrict__ x, const float* __restrict__ y, int H,
                                                       int W, int kh, int kw, int ws,
                                                       const float* __restrict__ filt, int tiles_w,
                                                       float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sf[kMaxFilt * kMaxFilt];  // flipped taps x 2
  __shared__ float red[2][kThreads / kWave];
  const int hh = kTH + ws - 1, hw = kSccTW + ws - 1;  // high-pass tile
  const int ih = hh + kh - 1, iw = hw + kw - 1;       // input tile
  float* hx = reinterpret_cast<float*>(smem);         // [hh][hw]
  float* hy = hx + hh * hw;
  float* ix = hy + hh * hw;                           // [ih][iw]
  float* iy = ix + ih * iw;
  float* hm = ix;                                     // 5 x [hh][64], over the dead input tile

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kTH, c0 = (tile % tiles_w) * kSccTW;
  const float* px = x + plane * H * W;
  const float* py = y + plane * H * W;
  const int tid = threadIdx.x;
  if (tid < kh * kw) sf[tid] = 2.0f * filt[kh * kw - 1 - tid];
  const int lo = ws / 2;  // ceil((ws-1)/2) zero rows / columns before the image; (ws-1)/2 after
  // the high-pass tile starts at image position (r0 - lo, c0 - lo); the input tile (kh-1)/2, (kw-1)/2 before that
  const int gr0 = r0 - lo - (kh - 1) / 2, gc0 = c0 - lo - (kw - 1) / 2;
  for (int i = tid; i < ih * iw; i += kThreads) {
    const int r = i / iw, c = i % iw;
    const long long g = static_cast<long long>(sym_index(gr0 + r, H)) * W + sym_index(gc0 + c, W);
    ix[i] = px[g];
    iy[i] = py[g];
  }
  __syncthreads();
  for (int i = tid; i < hh * hw; i += kThreads) {
    const int r = i / hw, c = i % hw;
    const int gr = r0 - lo + r, gc = c0 - lo + c;
    float a = 0, b = 0;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
      for (int u = 0; u < kh; ++u) {
        const float* qx = ix + (r + u) * iw + c;
        const float* qy = iy + (r + u) * iw + c;
        for (int v = 0; v < kw; ++v) {
          const float f = sf[u * kw + v];
          a += f * qx[v];
          b += f * qy[v];
        }
      }
    }
    hx[i] = a;
    hy[i] = b;
  }
  __syncthreads();
  moments_rows<float, kSccTW, true>(hx, hy, hh, hw, ws, nullptr, hm);
  __syncthreads();
  const int plane_sz = hh * kSccTW;
  const float inv = 1.0f / static_cast<float>(ws * ws);
  float s = 0, unused = 0;
  for (int i = tid; i < kTH * kSccTW; i += kThreads) {
    const int r = i / kSccTW, c = i % kSccTW;
    if (r0 + r >= H || c0 + c >= W) continue;
    float mx = 0, my = 0, exx = 0, eyy = 0, exy = 0;
    for (int k = 0; k < ws; ++k) {
      const int o = (r + k) * kSccTW + c;
      mx += hm[o];
      my += hm[plane_sz + o];
      exx += hm[2 * plane_sz + o];
      eyy += hm[3 * plane_sz + o];
      exy += hm[4 * plane_sz + o];
    }
    mx *= inv, my *= inv, exx *= inv, eyy *= inv, exy *= inv;
    const float sxx = exx - mx * mx > 0 ? exx - mx * mx : 0.0f;
    const float syy = eyy - my * my > 0 ? eyy - my * my : 0.0f;
    const float den = sqrtf(sxx) * sqrtf(syy);
    s += den == 0.0f ? 0.0f : (exy - mx * my) / den;
  }
  block_sum2(s, unused, red);
  if (tid == 0) part[plane * gridDim.x + tile] = s;
}

template <typename scalar_t, int TW>
void launch_vif_scale(const at::Tensor& x, const at::Tensor& y, const at::Tensor& taps, const at::Tensor& c12, int n,
                      int Hd, int Wd, at::Tensor& xd, at::Tensor& yd, at::Tensor& part, int tiles_h, int tiles_w) {
  using acc_t = typename Acc<scalar_t>::type;
  const int H = static_cast<int>(x.size(1)), W = static_cast<int>(x.size(2));
  const size_t dh = kTH + n - 1, dw = TW + n - 1, sh = 2 * dh + n - 2, sw = 2 * dw + n - 2;
  const size_t stage12 = 2 * sh * sw + 2 * dh * sw, stage34 = 2 * dh * dw + 5 * dh * TW;
  const size_t lds = sizeof(acc_t) * (stage12 > stage34 ? stage12 : stage34);
  TORCH_CHECK(lds <= kLdsLimit, "vif_scale: ", n, " taps need ", lds, " bytes of LDS, more than a workgroup has");
  const auto kernel = &vif_scale_kernel<scalar_t, TW>;
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)) == hipSuccess,
                "vif_scale: could not raise the dynamic LDS limit");
  }
  const size_t align = sizeof(Vec4<scalar_t>) < 16 ? sizeof(Vec4<scalar_t>) : 16;
  const int vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % align == 0 &&
                  reinterpret_cast<uintptr_t>(y.data_ptr()) % align == 0;
  hipLaunchKernelGGL(kernel, dim3(tiles_h * tiles_w, static_cast<unsigned>(x.size(0))), dim3(kThreads), lds, stream(),
                     reinterpret_cast<const scalar_t*>(x.data_ptr()), reinterpret_cast<const scalar_t*>(y.data_ptr()),
                     H, W, n, taps.data_ptr<acc_t>(), c12.data_ptr<acc_t>(), Hd, Wd, tiles_h, tiles_w, vec,
                     xd.data_ptr<acc_t>(), yd.data_ptr<acc_t>(), part.data_ptr<acc_t>());
}

}  // namespace

// One VIF pyramid step: blur x (reference) and y (distorted) [P, H, W] with the separable Gaussian `taps` (odd n <= 17,
// accumulation dtype: f64 for f64 inputs, else f32), keep every second valid pixel, and sum the VIF terms over the n x n
// windows of the result.  c12 = (sigma_n^2, -, eps).  Returns the decimated planes xd, yd [P, ceil((H-n+1)/2),
// ceil((W-n+1)/2)] in the accumulation dtype and part [P, tiles, 2] of per-tile (numerator, denominator) sums.
std::tuple<at::Tensor, at::Tensor, at::Tensor> vif_scale(const at::Tensor& x, const at::Tensor& y,
                                                         const at::Tensor& taps, const at::Tensor& c12) {
  TM_CHECK_CUDA(x);
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, taps);
  TM_SAME_DEVICE(x, c12);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TM_CHECK_CONTIG(taps);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type(), "vif_scale: x / y mismatch");
  TORCH_CHECK(x.dim() == 3, "vif_scale: expects [planes, H, W]");
  const int n = static_cast<int>(taps.numel());
  TORCH_CHECK(n >= 1 && n <= kMaxTaps && n % 2 == 1, "vif_scale: taps must be odd, 1..", kMaxTaps);
  const bool dbl = x.scalar_type() == at::kDouble;
  const auto acc_type = dbl ? at::kDouble : at::kFloat;
  TORCH_CHECK(c12.numel() >= 3 && c12.is_contiguous(), "vif_scale: c12 must hold (sigma_n^2, -, eps)");
  TORCH_CHECK(taps.scalar_type() == acc_type && c12.scalar_type() == acc_type,
              "vif_scale: taps / constants must be in the accumulation dtype");
  const long long planes = x.size(0);
  TORCH_CHECK(planes <= 65535, "vif_scale: too many planes for one launch");
  TORCH_CHECK(x.size(1) < (1 << 30) && x.size(2) < (1 << 30), "vif_scale: plane too large");
  const int H = static_cast<int>(x.size(1)), W = static_cast<int>(x.size(2));
  const int Hd = (H - n + 2) / 2, Wd = (W - n + 2) / 2;  // ceil((H - n + 1) / 2)
  TORCH_CHECK(H >= n && W >= n && Hd >= n && Wd >= n, "vif_scale: the decimated plane must hold one ", n, " x ", n,
              " window");
  const int tw = dbl ? kVifTW<double> : kVifTW<float>;
  const int tiles_h = (Hd - n + 1 + kTH - 1) / kTH, tiles_w = (Wd - n + 1 + tw - 1) / tw;
  const auto opts = x.options().dtype(acc_type);
  at::Tensor xd = at::empty({planes, Hd, Wd}, opts), yd = at::empty({planes, Hd, Wd}, opts);
  at::Tensor part = at::empty({planes, static_cast<long long>(tiles_h) * tiles_w, 2}, opts);
  if (planes == 0) return {xd, yd, part};
  TM_DISPATCH_FLOAT(x.scalar_type(), "vif_scale", [&] {
    launch_vif_scale<scalar_t, kVifTW<scalar_t>>(x, y, taps, c12, n, Hd, Wd, xd, yd, part, tiles_h, tiles_w);
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {xd, yd, part};
}

// SCC of x, y [P, H, W] (f32): high-pass both with filt [kh, kw] (kh, kw <= 9 and no larger than the plane; true
// convolution over the symmetric-padded plane, times 2), then the correlation of the two over every window x window
// neighbourhood of the zero-padded result (window <= 33).  Returns part [P, tiles] of per-tile sums over the H x W map.
at::Tensor scc_partials(const at::Tensor& x, const at::Tensor& y, const at::Tensor& filt, int64_t window) {
  TM_CHECK_CUDA(x);
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, filt);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TM_CHECK_CONTIG(filt);
  TORCH_CHECK(x.sizes() == y.sizes() && x.dim() == 3, "scc_partials: expects two [planes, H, W] tensors");
  TORCH_CHECK(x.scalar_type() == at::kFloat && y.scalar_type() == at::kFloat && filt.scalar_type() == at::kFloat,
              "scc_partials: f32 only");
  TORCH_CHECK(filt.dim() == 2, "scc_partials: filt must be [kh, kw]");
  const long long planes = x.size(0);
  TORCH_CHECK(planes <= 65535, "scc_partials: too many planes for one launch");
  TORCH_CHECK(x.size(1) < (1 << 30) && x.size(2) < (1 << 30), "scc_partials: plane too large");
  const int H = static_cast<int>(x.size(1)), W = static_cast<int>(x.size(2));
  const int kh = static_cast<int>(filt.size(0)), kw = static_cast<int>(filt.size(1));
  TORCH_CHECK(kh >= 1 && kw >= 1 && kh <= kMaxFilt && kw <= kMaxFilt && kh <= H && kw <= W,
              "scc_partials: filter edges must be 1..", kMaxFilt, " and no larger than the plane");
  TORCH_CHECK(window >= 1 && window <= kMaxWin, "scc_partials: window must be 1..", kMaxWin);
  const int ws = static_cast<int>(window);
  const int tiles_w = (W + kSccTW - 1) / kSccTW, tiles_h = (H + kTH - 1) / kTH;
  at::Tensor part = at::empty({planes, static_cast<long long>(tiles_h) * tiles_w}, x.options());
  if (planes == 0 || H == 0 || W == 0) return part;
  const size_t hh = kTH + ws - 1, hw = kSccTW + ws - 1, ih = hh + kh - 1, iw = hw + kw - 1;
  const size_t in_sz = 2 * ih * iw, hm_sz = 5 * hh * kSccTW;
  const size_t lds = sizeof(float) * (2 * hh * hw + (in_sz > hm_sz ? in_sz : hm_sz));
  TORCH_CHECK(lds <= kLdsLimit, "scc_partials: tile does not fit the LDS");
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&scc_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) == hipSuccess,
                "scc_partials: could not raise the dynamic LDS limit");
  }
  hipLaunchKernelGGL(scc_kernel, dim3(tiles_h * tiles_w, static_cast<unsigned>(planes)), dim3(kThreads), lds, stream(),
                     x.data_ptr<float>(), y.data_ptr<float>(), H, W, kh, kw, ws, filt.data_ptr<float>(), tiles_w,
                     part.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return part;
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def("vif_scale(Tensor x, Tensor y, Tensor taps, Tensor c12) -> (Tensor, Tensor, Tensor)");
  m.def("scc_partials(Tensor x, Tensor y, Tensor filt, int window) -> Tensor");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) {
  m.impl("vif_scale", &tm_amd::vif_scale);
  m.impl("scc_partials", &tm_amd::scc_partials);
}
