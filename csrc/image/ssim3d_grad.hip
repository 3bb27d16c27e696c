// Fused backward of the 3-D SSIM / contrast-sensitivity window sums (the gradient of ssim3d.hip).
//
// The math is ssim_grad.hip's one axis up.  With g = (gs, gc) the upstream gradient of a volume's (sum SSIM, sum CS),
// every valid window j has five coefficients -- d/d(mu_x), d/d(E[x^2]), d/d(E[xy]), d/d(mu_y), d/d(E[y^2]) -- and
//
//   grad_x[i] = sum_j wd wh ww[i-j] (g_a[j] + 2 x[i] g_exx[j] + y[i] g_exy[j])     (grad_y likewise with g_b, g_eyy)
//
// i.e. the transposed separable 3-D convolution of the coefficient volumes.  A one-launch recompute as in 2-D would
// need a ring of KD pending window slices over (16+10) x (32+10) positions x 5 moments = 240 KB at 11^3, more than
// the 160 KB of LDS, so the work is two launches with the coefficient volumes coef [P][NC][out_d][out_h][out_w]
// (accumulation dtype; NC = 5, or 3 without grad_y) in global memory.  Nothing is kept from the forward.
//
// Launch 1, ssim3d_coef_kernel: the forward's depth march (same tile, same register ring) with another epilogue.
//   block = (4*PX) x 64 window tile of one volume x a chunk of window depth, 256 threads, one wave across W
//   per input slice: stage x / y -> W pass of 5 moments to LDS -> H pass to registers -> depth ring of KD pending
//   window slices.  The second moment is of x - y, not of y (mu_y = mu_x - mu_d): d/dc1 = sum gA mu_d^2 / B1 then comes
//   from an accurately known mu_d, where an fp32 1 - A1 / B1 has almost no correct bits when mu_x ~ mu_y.
//   The slot that took its last tap is a finished window: its coefficients are stored (lane across W: coalesced rows)
//   and its d/dc1, d/dc2 terms added to the thread's sums; one (dc1, dc2) slot per block, fixed order, no atomics.
//
// Launch 2, ssim3d_grad_kernel: the transposed march.
//   block = (4*PX) x 64 tile of GRADIENT voxels of one volume x a chunk of gradient depth z0 .. z1
//   visits window slices j = z0 - KD + 1 .. z1 (those outside [0, out_d) are skipped, block-uniform); per slice:
//   stage the NC coefficient tiles with a halo of k - 1 rows / cols before the tile (zero outside the valid windows)
//   -> transposed W pass to LDS -> transposed H pass to NC registers per owned voxel -> ring[q] += wd[z - j] * t over
//   the KD pending gradient slices.  Window slice j is the last one of gradient slice z = j: that slot is finished,
//   x and y of its voxels are read from global memory (one coalesced row per wave), combined, rounded once, stored.
//   With step s = j - (z0 - KD + 1) this is the forward's ring with the depth taps reversed, so every slot and tap
//   index is a compile-time constant here too.
//
// LDS (words of acc_t; TH = 8 for fp32 / 16-bit, 4 for fp64; ih = TH + kh - 1, iw = 64 + kw - 1):
//   launch 1: 2 ih iw + 5 ih 64     11 x 11 fp32: 2*18*74 + 5*18*64 = 8424 = 33.7 KB;  15 x 15 fp64: 8568 = 68.5 KB
//   launch 2: NC ih iw + NC ih 64   11 x 11 fp32: 5*18*74 + 5*18*64 = 12420 = 49.7 KB -> 3 blocks / CU
//                                   15 x 15 fp32: 5*22*78 + 5*22*64 = 15620 = 62.5 KB; 15 x 15 fp64: 12780 = 102 KB
// VGPRs: the ring is KD * PX * 5 accumulators = 110 registers at KD = 11 in either precision (fp64: PX = 1), plus
//   PX * 5 H-pass results and the taps; every instantiation is built for 256 threads (512 VGPRs) and has no scratch.
// In-plane windows up to kMaxK = 15 (the 2-D backward's limit) and depth windows up to 11 are served; the rest stays on
// the convolution path (torchmetrics_amd/functional/image/ssim.py checks the same limits before it calls this op).
#include "../common/tm_common.h"

#include <algorithm>
#include <tuple>
#include <utility>
#include <type_traits>

namespace tm_amd {
namespace {

constexpr int kTW = 64;      // tile cols per block (one wave across)
constexpr int kMaxK = 15;    // largest in-plane window edge of the fused backward
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

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the march's inner loop over ring slots, expanded at
// compile time.  A `#pragma unroll` over these long bodies is declined by the optimizer at KD = 11, which leaves the
// ring dynamically indexed and so in scratch memory.
template <int... Rs, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Rs...>, F&& f) {
  (f(std::integral_constant<int, Rs>{}), ...);
}

// One (in_h x in_w) tile at (r0, c0) of slice `g` ([H, W], row-major) -> LDS `s`, zero outside the slice; r0 and c0
// may be negative (launch 2 stages a halo before its tile).  Work items are (row, 16-byte chunk) pairs; the chunks
// are aligned in global memory, so a row starts `mis` elements into its first.
template <typename src_t>
__device__ __forceinline__ void stage_tile(const src_t* __restrict__ g, typename Acc<src_t>::type* __restrict__ s, int H,
                                           int W, int r0, int c0, int in_h, int in_w, int tid) {
  using acc_t = typename Acc<src_t>::type;
  constexpr int kVec = 16 / sizeof(src_t);
  const int nv = (in_w + 2 * kVec - 2) / kVec;  // chunks that cover in_w elements at any misalignment
  for (int i = tid; i < in_h * nv; i += kThreads) {
    const int r = i / nv, k = i - r * nv;
    const int gr = r0 + r;
    acc_t* srow = s + r * in_w;
    if (gr < 0 || gr >= H) {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = k * kVec + e;
        if (col < in_w) srow[col] = acc_t(0);
      }
      continue;
    }
    const long long e0 = static_cast<long long>(gr) * W + c0;  // element of tile col 0 (before the row if c0 < 0)
    const long long a0 = static_cast<long long>(reinterpret_cast<uintptr_t>(g) / sizeof(src_t)) + e0;
    const int mis = static_cast<int>(a0 & (kVec - 1));
    const int cb = k * kVec - mis;
    if (cb >= 0 && cb + kVec <= in_w && c0 + cb >= 0 && c0 + cb + kVec <= W) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(g + (e0 + cb));
      src_t v[kVec];
      __builtin_memcpy(v, &raw, sizeof(raw));
#pragma unroll
      for (int e = 0; e < kVec; ++e) srow[cb + e] = load_acc(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = cb + e;
        if (col >= 0 && col < in_w) {
          const int gc = c0 + col;
          srow[col] = (gc >= 0 && gc < W) ? load_acc(g[e0 + col]) : acc_t(0);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ launch 1: coefficients
template <typename scalar_t, int KD>
__global__ void __launch_bounds__(kThreads)
    ssim3d_coef_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y, int D, int H, int W, int kh, int kw,
                       const typename Acc<scalar_t>::type* __restrict__ wd, const typename Acc<scalar_t>::type* __restrict__ wh,
                       const typename Acc<scalar_t>::type* __restrict__ ww, const typename Acc<scalar_t>::type* __restrict__ c12,
                       const typename Acc<scalar_t>::type* __restrict__ g, int tiles_w, int chunk, int nc,
                       typename Acc<scalar_t>::type* __restrict__ coef, typename Acc<scalar_t>::type* __restrict__ gc_part) {
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
  const int z0 = blockIdx.z * chunk;               // first window slice == first input slice of this block
  const int n_in = min(chunk, out_d - z0) + KD - 1;  // input slices to march over; z0 + n_in <= D
  const long long slice = static_cast<long long>(H) * W;
  const long long vol = static_cast<long long>(out_d) * out_h * out_w;
  const scalar_t* px = x + (plane * D + z0) * slice;
  const scalar_t* py = y + (plane * D + z0) * slice;
  acc_t* pc = coef + plane * nc * vol;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  if (tid < kh) swh[tid] = wh[tid];
  if (tid < kw) sww[tid] = ww[tid];
  acc_t wdr[KD];
#pragma unroll
  for (int j = 0; j < KD; ++j) wdr[j] = wd[j];
  const acc_t c1 = c12[0], c2 = c12[1];
  const acc_t gs = g[plane * 2], gcs = g[plane * 2 + 1];

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
  acc_t dc1 = 0, dc2 = 0;
  const int plane_sz = in_h * kTW;

  for (int s0 = 0; s0 < n_in; s0 += KD) {
    static_for(std::make_integer_sequence<int, KD>{}, [&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
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
            m2 += w * (a - b);
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
        // depth ring: input slice s is tap (r - q) mod KD of the window slice pending in slot q
#pragma unroll
        for (int q = 0; q < KD; ++q) {
          const acc_t w = wdr[(r - q + KD) % KD];
#pragma unroll
          for (int p = 0; p < kPX; ++p)
#pragma unroll
            for (int m = 0; m < 5; ++m) ring[q][p][m] += w * mom[p][m];
        }
        const int qd = (r + 1) % KD;  // the slot that just took tap KD - 1: window slice z0 + s - (KD - 1)
        if (s >= KD - 1) {
          const long long zo = z0 + s - (KD - 1);
#pragma unroll
          for (int p = 0; p < kPX; ++p) {
            if (!ok[p]) continue;
            const acc_t a = ring[qd][p][0], d = ring[qd][p][1];
            const acc_t exx = ring[qd][p][2], eyy = ring[qd][p][3], exy = ring[qd][p][4];
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
            acc_t* o = pc + (zo * out_h + (r0 + row_a + p)) * out_w + c0 + lane;
            o[0] = 2 * b * gA + 2 * a * gB - 2 * b * gU - 2 * a * kx * gL;
            o[vol] = kx * gL;
            o[2 * vol] = 2 * gU;
            if (nc == 5) {
              o[3 * vol] = 2 * a * gA + 2 * b * gB - 2 * a * gU - 2 * b * ky * gL;
              o[4 * vol] = ky * gL;
            }
            // gA + gB and gU + gL with the c1 / c2 that cancel in them taken out: B1 - A1 = d^2, L - U = sxx + syy - 2 sxy
            dc1 += gA * d * d / B1;
            dc2 += (gs * A1 / B1 + gcs) * (sxx + syy - 2 * sxy) / (L * L);
          }
        }
#pragma unroll
        for (int p = 0; p < kPX; ++p)
#pragma unroll
          for (int m = 0; m < 5; ++m) ring[qd][p][m] = acc_t(0);
      }
    });
  }
  if (gc_part == nullptr) return;  // uniform over the grid
  dc1 = wave_sum(dc1);
  dc2 = wave_sum(dc2);
  if (lane == 0) {
    red[0][wave] = dc1;
    red[1][wave] = dc2;
  }
  __syncthreads();
  if (tid == 0) {
    acc_t a = 0, b = 0;
    for (int w = 0; w < kWaves; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
    const long long slot = (plane * gridDim.z + blockIdx.z) * gridDim.x + tile;
    gc_part[slot * 2] = a;
    gc_part[slot * 2 + 1] = b;
  }
}

// ------------------------------------------------------------------------------------- launch 2: transposed march
template <typename scalar_t, int KD, int NC>
__global__ void __launch_bounds__(kThreads)
    ssim3d_grad_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y,
                       const typename Acc<scalar_t>::type* __restrict__ coef, int D, int H, int W, int kh, int kw,
                       const typename Acc<scalar_t>::type* __restrict__ wd, const typename Acc<scalar_t>::type* __restrict__ wh,
                       const typename Acc<scalar_t>::type* __restrict__ ww, int tiles_w, int chunk,
                       scalar_t* __restrict__ gx, scalar_t* __restrict__ gy) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kPX = Acc<scalar_t>::kPX;
  constexpr int kTH = kWaves * kPX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int in_h = kTH + kh - 1, in_w = kTW + kw - 1;
  const int tile_sz = in_h * in_w, plane_sz = in_h * kTW;
  acc_t* sc = reinterpret_cast<acc_t*>(smem);  // NC x [in_h][in_w] coefficient tiles
  acc_t* tw = sc + NC * tile_sz;               // NC x [in_h][kTW] after the transposed W pass
  __shared__ acc_t swh[kMaxK], sww[kMaxK];

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kTH, c0 = (tile % tiles_w) * kTW;  // first gradient pixel of the tile
  const int out_d = D - KD + 1, out_h = H - kh + 1, out_w = W - kw + 1;
  const int z0 = blockIdx.z * chunk;              // first gradient slice of this block
  const int n_vis = min(chunk, D - z0) + KD - 1;  // window slices j0 .. j0 + n_vis - 1, some outside [0, out_d)
  const int j0 = z0 - (KD - 1);
  const long long wslice = static_cast<long long>(out_h) * out_w;
  const acc_t* pc = coef + plane * NC * out_d * wslice;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  if (tid < kh) swh[tid] = wh[tid];
  if (tid < kw) sww[tid] = ww[tid];
  acc_t wdr[KD];  // reversed: step s is depth tap KD - 1 - ((s - o) mod KD) of the gradient slice o pending in a slot
#pragma unroll
  for (int j = 0; j < KD; ++j) wdr[j] = wd[KD - 1 - j];

  const int row_a = wave * kPX;  // first owned row of the tile; the owned column is `lane`
  bool ok[kPX];
#pragma unroll
  for (int p = 0; p < kPX; ++p) ok[p] = r0 + row_a + p < H && c0 + lane < W;
  acc_t ring[KD][kPX][NC];
#pragma unroll
  for (int q = 0; q < KD; ++q)
#pragma unroll
    for (int p = 0; p < kPX; ++p)
#pragma unroll
      for (int m = 0; m < NC; ++m) ring[q][p][m] = acc_t(0);

  for (int s0 = 0; s0 < n_vis; s0 += KD) {
    static_for(std::make_integer_sequence<int, KD>{}, [&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      const int s = s0 + r;  // block-uniform
      if (s < n_vis) {
        const int j = j0 + s;
        if (j >= 0 && j < out_d) {
          // the previous slice's W pass (reader of sc) ended before its second barrier
#pragma nounroll  // one copy of the stager per step keeps the expanded march within the instruction cache
          for (int m = 0; m < NC; ++m)
            stage_tile(pc + (static_cast<long long>(m) * out_d + j) * wslice, sc + m * tile_sz, out_h, out_w,
                       r0 - (kh - 1), c0 - (kw - 1), in_h, in_w, tid);
          __syncthreads();  // also: the previous slice's H pass (reader of tw) is done
          // transposed W pass: pixel col c takes window cols c - k, i.e. tile cols c + kw - 1 - k, with weight ww[k]
          for (int i = tid; i < plane_sz; i += kThreads) {
            const int rr = i / kTW, c = i % kTW;
            const acc_t* row = sc + rr * in_w + c + kw - 1;
            acc_t t[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) t[m] = acc_t(0);
            for (int k = 0; k < kw; ++k) {
              const acc_t w = sww[k];
#pragma unroll
              for (int m = 0; m < NC; ++m) t[m] += w * row[m * tile_sz - k];
            }
#pragma unroll
            for (int m = 0; m < NC; ++m) tw[m * plane_sz + i] = t[m];
          }
          __syncthreads();
          // transposed H pass: pixel row a + p takes tile rows a + p + kh - 1 - k with weight wh[k]; each loaded row
          // feeds all kPX vertically adjacent owned pixels
          acc_t t[kPX][NC];
#pragma unroll
          for (int p = 0; p < kPX; ++p)
#pragma unroll
            for (int m = 0; m < NC; ++m) t[p][m] = acc_t(0);
          for (int k = 0; k < kh + kPX - 1; ++k) {
            const int o = (row_a + k) * kTW + lane;
            acc_t v[NC];
#pragma unroll
            for (int m = 0; m < NC; ++m) v[m] = tw[m * plane_sz + o];
#pragma unroll
            for (int p = 0; p < kPX; ++p) {
              const int tp = kh - 1 - (k - p);
              const acc_t w = (tp >= 0 && tp < kh) ? swh[tp] : acc_t(0);
#pragma unroll
              for (int m = 0; m < NC; ++m) t[p][m] += w * v[m];
            }
          }
#pragma unroll
          for (int q = 0; q < KD; ++q) {
            const acc_t w = wdr[(r - q + KD) % KD];
#pragma unroll
            for (int p = 0; p < kPX; ++p)
#pragma unroll
              for (int m = 0; m < NC; ++m) ring[q][p][m] += w * t[p][m];
          }
        }
        const int qd = (r + 1) % KD;  // window slice j was the last of gradient slice z = j = z0 + s - (KD - 1)
        if (s >= KD - 1) {
#pragma unroll
          for (int p = 0; p < kPX; ++p) {
            if (!ok[p]) continue;
            const long long o = ((plane * D + j) * H + (r0 + row_a + p)) * W + c0 + lane;
            const acc_t xv = load_acc(x[o]), yv = load_acc(y[o]);
            gx[o] = static_cast<scalar_t>(ring[qd][p][0] + 2 * xv * ring[qd][p][1] + yv * ring[qd][p][2]);
            if constexpr (NC == 5)
              gy[o] = static_cast<scalar_t>(ring[qd][p][3] + 2 * yv * ring[qd][p][4] + xv * ring[qd][p][2]);
          }
        }
#pragma unroll
        for (int p = 0; p < kPX; ++p)
#pragma unroll
          for (int m = 0; m < NC; ++m) ring[qd][p][m] = acc_t(0);
      }
    });
  }
}

template <typename K>
void raise_lds(K* kern, size_t lds) {
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)) == hipSuccess,
                "ssim3d_backward: could not raise the dynamic LDS limit");
  }
}

// the longest chunk that still leaves ~2 blocks per CU (every chunk re-reads kd - 1 halo slices), not below kd
int pick_chunk(long long forced, int extent, long long blocks_in_plane, int kd, int device) {
  long long chunk = forced;
  if (chunk == 0) {
    const long long want = 2LL * cu_count(device);
    const long long in_plane = std::max<long long>(1, blocks_in_plane);
    const long long n_chunks = (want + in_plane - 1) / in_plane;
    chunk = std::max<long long>(extent / n_chunks, kd);
  }
  return static_cast<int>(std::min<long long>(chunk, extent));
}

}  // namespace

// x, y: [P, D, H, W] volumes (contiguous, same dtype); wd [kd], wh [kh], ww [kw], c12 [>= 2] as for ssim3d_partials;
// g [P, 2]: upstream gradient of each volume's (sum SSIM, sum CS) over its valid windows, in the accumulation dtype.
// depth_chunk > 0 forces the slices per block of both launches, 0 lets the launcher pick.
// Returns (gx, gy or an empty tensor, gc_part [P, blocks, 2] of per-block (d/dc1, d/dc2) or an empty tensor).
// Scratch: the coefficient volumes, NC x (number of windows) accumulation-dtype words (NC = 5, or 3 without gy):
// about 33 MB at 2 x 1 x 128^3 and 82 MB at 1 x 1 x 160 x 192 x 160 in fp32, freed when the op returns.
std::tuple<at::Tensor, at::Tensor, at::Tensor> ssim3d_backward(const at::Tensor& x, const at::Tensor& y,
                                                               const at::Tensor& wd, const at::Tensor& wh,
                                                               const at::Tensor& ww, const at::Tensor& c12,
                                                               const at::Tensor& g, bool need_y, bool need_c,
                                                               int64_t depth_chunk) {
  TM_CHECK_CUDA(x);
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, wd);
  TM_SAME_DEVICE(x, wh);
  TM_SAME_DEVICE(x, ww);
  TM_SAME_DEVICE(x, c12);
  TM_SAME_DEVICE(x, g);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TM_CHECK_CONTIG(wd);
  TM_CHECK_CONTIG(wh);
  TM_CHECK_CONTIG(ww);
  TM_CHECK_CONTIG(c12);
  TM_CHECK_CONTIG(g);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type(), "ssim3d_backward: x / y mismatch");
  TORCH_CHECK(x.dim() == 4, "ssim3d_backward: expects [planes, D, H, W]");
  const int kd = static_cast<int>(wd.numel()), kh = static_cast<int>(wh.numel()), kw = static_cast<int>(ww.numel());
  TORCH_CHECK(kd >= 1 && kd <= kMaxKD && kd % 2 == 1, "ssim3d_backward: depth window must be odd and 1..", kMaxKD);
  TORCH_CHECK(kh >= 1 && kw >= 1 && kh <= kMaxK && kw <= kMaxK, "ssim3d_backward: in-plane window must be 1..", kMaxK);
  const long long planes = x.size(0);
  TORCH_CHECK(x.size(1) < (1 << 30) && x.size(2) < (1 << 30) && x.size(3) < (1 << 30),
              "ssim3d_backward: extent too large");
  const int D = static_cast<int>(x.size(1)), H = static_cast<int>(x.size(2)), W = static_cast<int>(x.size(3));
  TORCH_CHECK(D >= kd && H >= kh && W >= kw, "ssim3d_backward: volume smaller than the window");
  TORCH_CHECK(planes <= 65535, "ssim3d_backward: too many planes for one launch");
  TORCH_CHECK(depth_chunk >= 0, "ssim3d_backward: depth_chunk must be >= 0");
  const bool dbl = x.scalar_type() == at::kDouble;
  const auto acc_type = dbl ? at::kDouble : at::kFloat;
  TORCH_CHECK(c12.numel() >= 2, "ssim3d_backward: c12 must hold (c1, c2)");
  TORCH_CHECK(wd.scalar_type() == acc_type && wh.scalar_type() == acc_type && ww.scalar_type() == acc_type &&
                  c12.scalar_type() == acc_type && g.scalar_type() == acc_type,
              "ssim3d_backward: window / constants / upstream gradient must be in the accumulation dtype");
  TORCH_CHECK(g.dim() == 2 && g.size(0) == planes && g.size(1) == 2, "ssim3d_backward: g must be [planes, 2]");
  const int th = kWaves * (dbl ? Acc<double>::kPX : Acc<float>::kPX);
  const int out_d = D - kd + 1, out_h = H - kh + 1, out_w = W - kw + 1;
  // launch 1 tiles the windows, launch 2 the voxels
  const int wt_w = (out_w + kTW - 1) / kTW, wt_h = (out_h + th - 1) / th;
  const int gt_w = (W + kTW - 1) / kTW, gt_h = (H + th - 1) / th;
  const long long wtiles = static_cast<long long>(wt_w) * wt_h, gtiles = static_cast<long long>(gt_w) * gt_h;
  TORCH_CHECK(gtiles < (1LL << 31), "ssim3d_backward: too many in-plane tiles for one launch");
  const int wchunk = pick_chunk(depth_chunk, out_d, wtiles * planes, kd, x.get_device());
  const int gchunk = pick_chunk(depth_chunk, D, gtiles * planes, kd, x.get_device());
  const int wchunks = (out_d + wchunk - 1) / wchunk, gchunks = (D + gchunk - 1) / gchunk;
  TORCH_CHECK(wchunks <= 65535 && gchunks <= 65535, "ssim3d_backward: too many depth chunks for one launch");
  const int nc = need_y ? 5 : 3;
  at::Tensor gx = at::empty_like(x);
  at::Tensor gy = need_y ? at::empty_like(y) : at::empty({0}, x.options());
  const int64_t gc_p = need_c ? planes : 0, gc_t = need_c ? wchunks * wtiles : 0;
  at::Tensor gc_part = at::empty({gc_p, gc_t, 2}, x.options().dtype(acc_type));
  if (planes == 0) return {gx, gy, gc_part};
  at::Tensor coef = at::empty({planes, nc, out_d, out_h, out_w}, x.options().dtype(acc_type));
  const size_t in_h = th + kh - 1, in_w = kTW + kw - 1;
  const size_t esz = dbl ? sizeof(double) : sizeof(float);
  const size_t lds1 = esz * (2 * in_h * in_w + 5 * in_h * kTW);
  const size_t lds2 = esz * nc * (in_h * in_w + in_h * kTW);
  TORCH_CHECK(lds1 <= 150 * 1024 && lds2 <= 150 * 1024, "ssim3d_backward: window too large for the LDS tile");
  auto s = stream();
  const dim3 grid1(static_cast<unsigned>(wtiles), static_cast<unsigned>(planes), static_cast<unsigned>(wchunks));
  const dim3 grid2(static_cast<unsigned>(gtiles), static_cast<unsigned>(planes), static_cast<unsigned>(gchunks));
  TM_DISPATCH_FLOAT(x.scalar_type(), "ssim3d_backward", [&] {
    using acc_t = typename Acc<scalar_t>::type;
    const auto* xp = reinterpret_cast<const scalar_t*>(x.data_ptr());
    const auto* yp = reinterpret_cast<const scalar_t*>(y.data_ptr());
    auto launch = [&](auto kd_c) {
      constexpr int KD = decltype(kd_c)::value;
      auto* k1 = &ssim3d_coef_kernel<scalar_t, KD>;
      raise_lds(k1, lds1);
      hipLaunchKernelGGL(k1, grid1, dim3(kThreads), lds1, s, xp, yp, D, H, W, kh, kw, wd.data_ptr<acc_t>(),
                         wh.data_ptr<acc_t>(), ww.data_ptr<acc_t>(), c12.data_ptr<acc_t>(), g.data_ptr<acc_t>(), wt_w,
                         wchunk, nc, coef.data_ptr<acc_t>(), need_c ? gc_part.data_ptr<acc_t>() : nullptr);
      auto launch2 = [&](auto nc_c) {
        constexpr int NC = decltype(nc_c)::value;
        auto* k2 = &ssim3d_grad_kernel<scalar_t, KD, NC>;
        raise_lds(k2, lds2);
        hipLaunchKernelGGL(k2, grid2, dim3(kThreads), lds2, s, xp, yp, coef.data_ptr<acc_t>(), D, H, W, kh, kw,
                           wd.data_ptr<acc_t>(), wh.data_ptr<acc_t>(), ww.data_ptr<acc_t>(), gt_w, gchunk,
                           reinterpret_cast<scalar_t*>(gx.data_ptr()),
                           need_y ? reinterpret_cast<scalar_t*>(gy.data_ptr()) : nullptr);
      };
      if (need_y) {
        launch2(std::integral_constant<int, 5>{});
      } else {
        launch2(std::integral_constant<int, 3>{});
      }
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
  return {gx, gy, gc_part};
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def(
      "ssim3d_backward(Tensor x, Tensor y, Tensor wd, Tensor wh, Tensor ww, Tensor c12, Tensor g, bool need_y, "
      "bool need_c, int depth_chunk) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) { m.impl("ssim3d_backward", &tm_amd::ssim3d_backward); }
