// Pansharpening metrics (D_lambda, D_s, QNR): the UQI of every band pair of one tensor in one launch, and the
// degradation of the panchromatic image (box filter + bilinear decimation) in one pass.
//
// band_uqi_kernel: x [B, C, H, W] -> per-block partial sums of the UQI map of every pair (i < j) over the valid windows.
//   The pair set is split like a SYRK: bands are cut into groups of G = 4 and the grid is (pixel tile, sample, group
//   pair gi <= gj).  A block owns an (8 PX) x 32 tile of windows (PX = 4: 32 x 32; fp64 PX = 2: 16 x 32), 256 threads,
//   thread = (column, PX vertically adjacent windows).
//   1. stage the (8 PX + k - 1) x (32 + k - 1) tile of the block's 4 (gi == gj) or 4 + n (gi < gj) bands in LDS in the
//      accumulation type (row pitch 28 + 4 ceil((k + 3) / 4), zero outside the plane and in the pitch columns;
//      4-element global loads where the rows are aligned).  42 x 44 x 4 B per band at k = 11: 58 KB for 8 bands.
//   2. statistics, two bands at a time: row pass of x and x^2 into four scratch planes (a work item is one row x 4
//      adjacent outputs: it walks the row in 16-byte LDS reads and slides the taps through 4 registers), column pass
//      for the PX windows a thread owns (every scratch row read once for PX outputs).  mu and the clamped variance of
//      every staged band stay in registers: 2 x 8 x PX values.
//   3. for every band i of group gi: row pass of the products x_i x_j, formed on the fly from the two staged tiles,
//      for all partner bands j at once (up to four scratch planes, reused from 2), then per partner the column pass,
//      q = (2 mu_i mu_j)(2 (E[x_i x_j] - mu_i mu_j)) / ((mu_i^2 + mu_j^2)(s_ii + s_jj) + eps), the arithmetic of
//      ssim2d_kernel's UQI mode, and the per-pair register accumulator.  Nothing product-shaped reaches global memory.
//   4. wave reduction + fixed-order sum over the 4 waves; one partial per (block, pair), plain stores, every slot of
//      part [B, tiles, pairs] written by exactly one block: no atomics, identical bits between calls.
//   Filtered maps per tile: 2 per staged band + 1 per pair (C = 8: 44 + 20 recomputed statistics, against 140) and
//   every band tile is read from global memory once per group pair instead of C - 1 times after two gathers.
//   No matrix instructions: the work is a separable k-tap fp32 filter per product map, not a GEMM.
//   G = 4 is chosen by reasoning, not by a sweep: 8 staged bands + 4 scratch planes are 80.6 KB at k = 11, so two
//   blocks share a CU's 160 KB; G = 8 would leave one.
//
// pan_degrade_kernel: pan [P, H, W] -> [P, h, w], the box filter of `window` over the mirror-padded plane followed by
//   the bilinear resize, for integer ratios rh = H / h, rw = W / w.  The bilinear source coordinate (d + 0.5) r - 0.5
//   has fraction 0 (odd r: one box output) or 0.5 (even r: the mean of two neighbours), so an output is one separable
//   window of nt = window + (r even) taps (1/2 at both ends for even r) starting at source index
//   d r + (r - 1) / 2 - window / 2; only the h x w outputs are computed.  A block stages the source tile of its
//   th x tw outputs (mirroring in the index arithmetic), runs the column pass at the th output rows, then the row pass
//   at the tw output columns, scales by 1 / window^2 and rounds once to the input type.  The host halves the tile
//   until the source tile fits 64 KB of LDS (a 1 x 1 tile needs at most 34 x 34 elements).
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch in any instantiation:
//   kernel                          VGPRs  SGPRs  scratch  static LDS  dynamic LDS at k = 11 (4 / 8 staged bands)
//   band_uqi f32 / f16 / bf16, PX 4   182     75     0        352 B      51 072 / 80 640 B   (2 blocks per CU)
//   band_uqi f64, PX 2                149     76     0        672 B      63 232 / 99 840 B   (2 / 1 blocks per CU)
//   pan_degrade f32 / f16 / bf16       20     63     0          0        23 232 B at window 7, ratio 4
//   pan_degrade f64                    28     48     0          0        46 464 B
//
// Timings (MI355X, benchmarks/bench_qnr.py -> profiles/qnr_bench.jsonl; median call, preds 4 x 8 x 1024^2 with ms
// 4 x 8 x 256^2 / 16 x 4 x 512^2 with 16 x 4 x 128^2; in brackets the gathered pairs in front of ssim2d_kernel and the
// torch box filter + resize, same tensors, same process):
//   D_lambda  fp32 1.00 / 0.29 ms (3.02 / 0.82 ms)   bf16 1.09 / 0.31 ms (2.96 / 0.79 ms)
//   D_s       fp32 0.83 / 0.49 ms (4.53 / 2.40 ms)   bf16 0.81 / 0.52 ms (4.63 / 2.29 ms)
//   QNR       fp32 1.87 / 0.81 ms (7.60 / 3.25 ms)   bf16 1.94 / 0.85 ms (7.63 / 3.11 ms)
//   D_lambda at 2 / 3 bands, 16 x C x 512^2 fp32: 0.14 / 0.21 ms (0.42 / 0.51 ms): the dispatch needs no floor on C.
#include "../common/tm_common.h"

#include <type_traits>

namespace tm_amd {
namespace {

constexpr int kG = 4;         // bands per group
constexpr int kTW = 32;       // window columns per block
constexpr int kGW = 4;        // adjacent outputs of one row-pass work item
constexpr int kRG = 8;        // row groups: kThreads / kTW
constexpr int kMaxK = 15;     // largest window; keep BAND_UQI_MAX_WINDOW (ops/__init__.py) equal
constexpr int kTapPad = 20;   // zero-padded taps: 4 ceil((kMaxK + 3) / 4) (row pass) >= kMaxK + 3 (column pass, PX = 4)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxBox = 33;   // largest pan_degrade window; keep PAN_DEGRADE_MAX_WINDOW equal
constexpr size_t kPanLds = 64 * 1024;

template <typename T>
struct Acc {
  using type = float;
  static constexpr int kPX = 4;
};
template <>
struct Acc<double> {
  using type = double;
  static constexpr int kPX = 2;  // 8 staged fp64 bands + scratch of the 32-row tile would need 161 KB
};

template <typename T>
using vec4 = T __attribute__((ext_vector_type(4)));

template <typename T>
struct alignas(sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16) Vec4 {
  T v[4];
};

template <typename acc_t, typename T>
__device__ __forceinline__ acc_t widen(T v) {
  if constexpr (std::is_same<T, acc_t>::value) {
    return v;
  } else {
    return static_cast<acc_t>(to_f32(v));
  }
}

struct Geo {
  int H, W, C, k;
  int in_h;     // staged rows: 8 PX + k - 1
  int pitch;    // staged row pitch, a multiple of 4
  int nj4;      // row-pass steps in vectors of 4: ceil((k + 3) / 4)
  int tiles_w;
  int vec;      // rows of the planes start 4-element aligned
};

// One band's tile -> LDS; zero where the source lies outside the plane and in the pitch columns past the tile.
template <typename scalar_t>
__device__ __forceinline__ void stage_band(const scalar_t* __restrict__ g, typename Acc<scalar_t>::type* __restrict__ s,
                                           const Geo& q, int r0, int c0, int tid) {
  using acc_t = typename Acc<scalar_t>::type;
  const int in_w = kTW + q.k - 1, p4 = q.pitch / 4;
  for (int i = tid; i < q.in_h * p4; i += kThreads) {
    const int r = i / p4, c = (i - r * p4) * 4;
    const int gr = r0 + r, gc = c0 + c;
    const long long o = static_cast<long long>(gr) * q.W + gc;
    vec4<acc_t> out;
    if (q.vec && gr < q.H && gc + 3 < q.W && c + 3 < in_w) {
      const Vec4<scalar_t> v = *reinterpret_cast<const Vec4<scalar_t>*>(g + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = widen<acc_t>(v.v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = gr < q.H && gc + e < q.W && c + e < in_w;
        out[e] = ok ? widen<acc_t>(g[o + e]) : acc_t(0);
      }
    }
    *reinterpret_cast<vec4<acc_t>*>(s + r * q.pitch + c) = out;
  }
}

// Row pass of nb bands' statistics: tiles t0 + b * tile_sz -> scratch planes 2b (x) and 2b + 1 (x^2), [in_h][kTW].
template <typename acc_t>
__device__ __forceinline__ void row_pass_stats(const acc_t* __restrict__ t0, int nb, int tile_sz,
                                               const acc_t* __restrict__ wq, acc_t* __restrict__ scr, const Geo& q,
                                               int tid) {
  using v4 = vec4<acc_t>;
  const int per = q.in_h * (kTW / kGW), plane_sz = q.in_h * kTW;
  for (int i = tid; i < nb * per; i += kThreads) {
    const int b = i / per, rem = i - b * per;
    const int r = rem / (kTW / kGW), c = (rem % (kTW / kGW)) * kGW;
    const v4* ra = reinterpret_cast<const v4*>(t0 + b * tile_sz + r * q.pitch + c);
    acc_t m1[kGW] = {0, 0, 0, 0}, m2[kGW] = {0, 0, 0, 0};
    acc_t w[kGW] = {0, 0, 0, 0};  // at input col c + j: the taps j, j - 1, j - 2, j - 3 of outputs c .. c + 3
    for (int j4 = 0; j4 < q.nj4; ++j4) {
      const v4 a4 = ra[j4], wn = reinterpret_cast<const v4*>(wq)[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[3] = w[2];
        w[2] = w[1];
        w[1] = w[0];
        w[0] = wn[e];
        const acc_t a = a4[e], aa = a * a;
#pragma unroll
        for (int o = 0; o < kGW; ++o) {
          m1[o] += w[o] * a;
          m2[o] += w[o] * aa;
        }
      }
    }
    acc_t* dst = scr + 2 * b * plane_sz + r * kTW + c;
    *reinterpret_cast<v4*>(dst) = v4{m1[0], m1[1], m1[2], m1[3]};
    *reinterpret_cast<v4*>(dst + plane_sz) = v4{m2[0], m2[1], m2[2], m2[3]};
  }
}

// Row pass of the products of tile ta with nb partner tiles tb0 + b * tile_sz -> scratch plane b.
template <typename acc_t>
__device__ __forceinline__ void row_pass_prod(const acc_t* __restrict__ ta, const acc_t* __restrict__ tb0, int nb,
                                              int tile_sz, const acc_t* __restrict__ wq, acc_t* __restrict__ scr,
                                              const Geo& q, int tid) {
  using v4 = vec4<acc_t>;
  const int per = q.in_h * (kTW / kGW), plane_sz = q.in_h * kTW;
  for (int i = tid; i < nb * per; i += kThreads) {
    const int b = i / per, rem = i - b * per;
    const int r = rem / (kTW / kGW), c = (rem % (kTW / kGW)) * kGW;
    const v4* ra = reinterpret_cast<const v4*>(ta + r * q.pitch + c);
    const v4* rb = reinterpret_cast<const v4*>(tb0 + b * tile_sz + r * q.pitch + c);
    acc_t m[kGW] = {0, 0, 0, 0}, w[kGW] = {0, 0, 0, 0};
    for (int j4 = 0; j4 < q.nj4; ++j4) {
      const v4 a4 = ra[j4], b4 = rb[j4], wn = reinterpret_cast<const v4*>(wq)[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[3] = w[2];
        w[2] = w[1];
        w[1] = w[0];
        w[0] = wn[e];
        const acc_t p = a4[e] * b4[e];
#pragma unroll
        for (int o = 0; o < kGW; ++o) m[o] += w[o] * p;
      }
    }
    *reinterpret_cast<v4*>(scr + b * plane_sz + r * kTW + c) = v4{m[0], m[1], m[2], m[3]};
  }
}

// Column pass of one scratch plane for the PX windows (rows row_a .. row_a + PX - 1, column col) of a thread.
template <typename acc_t, int PX>
__device__ __forceinline__ void col_pass(const acc_t* __restrict__ plane, const acc_t* __restrict__ wp, int k,
                                         int row_a, int col, acc_t (&m)[PX]) {
  acc_t w[PX];
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    w[p] = acc_t(0);
    m[p] = acc_t(0);
  }
  for (int j = 0; j < k + PX - 1; ++j) {
#pragma unroll
    for (int p = PX - 1; p > 0; --p) w[p] = w[p - 1];  // window p sees tap j - p
    w[0] = wp[j];
    const acc_t v = plane[(row_a + j) * kTW + col];
#pragma unroll
    for (int p = 0; p < PX; ++p) m[p] += w[p] * v;
  }
}

// The work of one block; DIAG: gi == gj (slots 0 .. na - 1, pairs i < j), else slots 0 .. 3 = group gi (always full)
// and 4 .. 4 + nb - 1 = group gj.  Every loop over slots is unrolled so that the register arrays are indexed statically.
template <typename scalar_t, int PX, bool DIAG>
__device__ __forceinline__ void band_block(const scalar_t* __restrict__ x, const Geo& q, int gi, int gj, int na, int nb,
                                           const typename Acc<scalar_t>::type* __restrict__ wq,
                                           typename Acc<scalar_t>::type eps, typename Acc<scalar_t>::type* smem,
                                           typename Acc<scalar_t>::type (*red)[kWaves],
                                           typename Acc<scalar_t>::type* __restrict__ part, int pairs) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int NS = DIAG ? kG : 2 * kG;
  const int tid = threadIdx.x, col = tid % kTW, row_a = (tid / kTW) * PX;
  const int tile = blockIdx.x, r0 = (tile / q.tiles_w) * (kRG * PX), c0 = (tile % q.tiles_w) * kTW;
  const long long sample = blockIdx.y;
  const int ns = DIAG ? na : kG + nb;
  const int tile_sz = q.in_h * q.pitch, plane_sz = q.in_h * kTW;
  acc_t* scr = smem + NS * tile_sz;  // 4 planes [in_h][kTW]

  for (int s = 0; s < ns; ++s) {
    const int band = s < kG ? gi * kG + s : gj * kG + s - kG;
    stage_band<scalar_t>(x + (sample * q.C + band) * q.H * q.W, smem + s * tile_sz, q, r0, c0, tid);
  }
  __syncthreads();

  acc_t mu[NS][PX], var[NS][PX];
#pragma unroll
  for (int sp = 0; sp < NS / 2; ++sp) {
    if (2 * sp < ns) {  // block-uniform
      row_pass_stats(smem + 2 * sp * tile_sz, ns - 2 * sp < 2 ? 1 : 2, tile_sz, wq, scr, q, tid);
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (2 * sp + b < ns) {
          acc_t e2[PX];
          col_pass<acc_t, PX>(scr + 2 * b * plane_sz, wq, q.k, row_a, col, mu[2 * sp + b]);
          col_pass<acc_t, PX>(scr + (2 * b + 1) * plane_sz, wq, q.k, row_a, col, e2);
#pragma unroll
          for (int p = 0; p < PX; ++p) {
            const acc_t d = e2[p] - mu[2 * sp + b][p] * mu[2 * sp + b][p];
            var[2 * sp + b][p] = d > 0 ? d : acc_t(0);
          }
        }
      }
      __syncthreads();
    }
  }

  const int out_h = q.H - q.k + 1, out_w = q.W - q.k + 1;
  bool ok[PX];
#pragma unroll
  for (int p = 0; p < PX; ++p) ok[p] = r0 + row_a + p < out_h && c0 + col < out_w;
  acc_t acc[kG][kG];
#pragma unroll
  for (int i = 0; i < kG; ++i)
#pragma unroll
    for (int jj = 0; jj < kG; ++jj) acc[i][jj] = acc_t(0);

#pragma unroll
  for (int i = 0; i < kG; ++i) {
    const int first = DIAG ? i + 1 : kG;            // slot of the first partner of band i
    const int np = DIAG ? na - 1 - i : nb;          // partners
    if (i < na && np > 0) {                         // block-uniform
      row_pass_prod(smem + i * tile_sz, smem + first * tile_sz, np, tile_sz, wq, scr, q, tid);
      __syncthreads();
#pragma unroll
      for (int jj = 0; jj < kG; ++jj) {
        constexpr int kLast = NS - 1;
        const int sb = first + jj < kLast ? first + jj : kLast;  // clamped: slots past NS - 1 have jj >= np
        if (jj < np) {
          acc_t e[PX];
          col_pass<acc_t, PX>(scr + jj * plane_sz, wq, q.k, row_a, col, e);
#pragma unroll
          for (int p = 0; p < PX; ++p) {
            const acc_t mx = mu[i][p], my = mu[sb][p];
            const acc_t mxy = mx * my;
            const acc_t upper = 2 * (e[p] - mxy);
            const acc_t lower = var[i][p] + var[sb][p];
            const acc_t v = ((2 * mxy) * upper) / ((mx * mx + my * my) * lower + eps);
            acc[i][jj] += ok[p] ? v : acc_t(0);
          }
        }
      }
      __syncthreads();
    }
  }

  // one partial per (block, pair): wave sums, then a fixed-order sum over the waves by thread i * kG + jj
#pragma unroll
  for (int i = 0; i < kG; ++i)
#pragma unroll
    for (int jj = 0; jj < kG; ++jj) {
      const acc_t v = wave_sum(acc[i][jj]);
      if ((tid & (kWave - 1)) == 0) red[i * kG + jj][tid / kWave] = v;
    }
  __syncthreads();
  if (tid < kG * kG) {
    const int i = tid / kG, jj = tid % kG;
    const int a = gi * kG + i, b = DIAG ? a + 1 + jj : gj * kG + jj;
    if (a < q.C && b < q.C && (DIAG ? i + 1 + jj < kG : true)) {
      acc_t s = 0;
      for (int w = 0; w < kWaves; ++w) s += red[tid][w];
      const long long pidx = static_cast<long long>(a) * q.C - static_cast<long long>(a) * (a + 1) / 2 + (b - a - 1);
      part[(sample * gridDim.x + tile) * pairs + pidx] = s;
    }
  }
}

template <typename scalar_t, int PX>
__global__ void __launch_bounds__(kThreads)
    band_uqi_kernel(const scalar_t* __restrict__ x, Geo q, const typename Acc<scalar_t>::type* __restrict__ taps,
                    const typename Acc<scalar_t>::type* __restrict__ consts,
                    typename Acc<scalar_t>::type* __restrict__ part, int pairs) {
  using acc_t = typename Acc<scalar_t>::type;
  extern __shared__ __attribute__((aligned(32))) char smem_raw[];
  __shared__ __attribute__((aligned(32))) acc_t wq[kTapPad];
  __shared__ acc_t red[kG * kG][kWaves];
  // group pair of this block: blockIdx.z enumerates gi <= gj row by row
  const int ng = (q.C + kG - 1) / kG;
  int gi = 0, z = blockIdx.z;
  while (z >= ng - gi) {
    z -= ng - gi;
    ++gi;
  }
  const int gj = gi + z;
  const int na = q.C - gi * kG < kG ? q.C - gi * kG : kG;
  const int nb = q.C - gj * kG < kG ? q.C - gj * kG : kG;
  if (gi == gj && na < 2) return;  // a last group of one band has no pair of its own (block-uniform)
  if (threadIdx.x < kTapPad) wq[threadIdx.x] = static_cast<int>(threadIdx.x) < q.k ? taps[threadIdx.x] : acc_t(0);
  const acc_t eps = consts[2];
  acc_t* smem = reinterpret_cast<acc_t*>(smem_raw);
  if (gi == gj) {
    band_block<scalar_t, PX, true>(x, q, gi, gj, na, nb, wq, eps, smem, red, part, pairs);
  } else {
    band_block<scalar_t, PX, false>(x, q, gi, gj, na, nb, wq, eps, smem, red, part, pairs);
  }
}

// ------------------------------------------------------------------------------------------------- pan_degrade
struct PanGeo {
  int H, W, h, w;
  int rh, rw;        // integer ratios
  int ws;            // box window
  int nth, ntw;      // taps per axis: ws + (ratio even)
  int offh, offw;    // source index of tap 0 of output 0: (r - 1) / 2 - ws / 2
  int th, tw;        // outputs per block
  int sh, sw;        // staged source tile: (th - 1) rh + nth, (tw - 1) rw + ntw
  int tiles_w;
};

// mirror an index of the edge-inclusive ("symmetric") padded axis back into [0, n); clamped where a partial tile
// reaches past the padding (such values only feed outputs that are not stored)
__device__ __forceinline__ int sym_index(int g, int n) {
  if (g < 0) g = -g - 1;
  if (g >= n) g = 2 * n - 1 - g;
  return g < 0 ? 0 : (g >= n ? n - 1 : g);
}

template <typename scalar_t>
__global__ void __launch_bounds__(kThreads)
    pan_degrade_kernel(const scalar_t* __restrict__ pan, PanGeo q, scalar_t* __restrict__ out) {
  using acc_t = typename Acc<scalar_t>::type;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  acc_t* src = reinterpret_cast<acc_t*>(smem_raw);  // [sh][sw]
  acc_t* mid = src + q.sh * q.sw;                   // [th][sw], after the column pass
  const int tid = threadIdx.x, tile = blockIdx.x;
  const long long plane = blockIdx.y;
  const int oy0 = (tile / q.tiles_w) * q.th, ox0 = (tile % q.tiles_w) * q.tw;
  const int gy0 = oy0 * q.rh + q.offh, gx0 = ox0 * q.rw + q.offw;
  const scalar_t* p = pan + plane * q.H * q.W;
  for (int i = tid; i < q.sh * q.sw; i += kThreads) {
    const int r = i / q.sw, c = i - r * q.sw;
    src[i] = widen<acc_t>(p[static_cast<long long>(sym_index(gy0 + r, q.H)) * q.W + sym_index(gx0 + c, q.W)]);
  }
  __syncthreads();
  const bool half_h = q.nth > q.ws, half_w = q.ntw > q.ws;  // even ratio: 1/2 at both end taps
  for (int i = tid; i < q.th * q.sw; i += kThreads) {
    const int r = i / q.sw, c = i - r * q.sw;
    const acc_t* col = src + r * q.rh * q.sw + c;
    acc_t s = 0;
    for (int k = 0; k < q.nth; ++k) s += col[k * q.sw];
    if (half_h) s -= acc_t(0.5) * (col[0] + col[(q.nth - 1) * q.sw]);
    mid[i] = s;
  }
  __syncthreads();
  const acc_t inv = acc_t(1) / static_cast<acc_t>(q.ws * q.ws);
  for (int i = tid; i < q.th * q.tw; i += kThreads) {
    const int r = i / q.tw, c = i - r * q.tw;
    if (oy0 + r >= q.h || ox0 + c >= q.w) continue;
    const acc_t* row = mid + r * q.sw + c * q.rw;
    acc_t s = 0;
    for (int k = 0; k < q.ntw; ++k) s += row[k];
    if (half_w) s -= acc_t(0.5) * (row[0] + row[q.ntw - 1]);
    out[(plane * q.h + oy0 + r) * q.w + ox0 + c] = static_cast<scalar_t>(s * inv);
  }
}

template <typename scalar_t>
void launch_band_uqi(const at::Tensor& x, const at::Tensor& taps, const at::Tensor& consts, at::Tensor& part, int k,
                     int pairs) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int PX = Acc<scalar_t>::kPX;
  Geo q;
  q.C = static_cast<int>(x.size(1));
  q.H = static_cast<int>(x.size(2));
  q.W = static_cast<int>(x.size(3));
  q.k = k;
  q.in_h = kRG * PX + k - 1;
  q.nj4 = (k + 3 + 3) / 4;
  q.pitch = kTW - kGW + 4 * q.nj4;
  q.tiles_w = (q.W - k + 1 + kTW - 1) / kTW;
  const size_t align = sizeof(Vec4<scalar_t>) < 16 ? sizeof(Vec4<scalar_t>) : 16;
  q.vec = q.W % 4 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % align == 0;
  const int ng = (q.C + kG - 1) / kG;
  const int slots = ng == 1 ? kG : 2 * kG;  // staged tiles the largest block of this launch holds
  const size_t lds = sizeof(acc_t) * (static_cast<size_t>(slots) * q.in_h * q.pitch + 4 * q.in_h * kTW);
  const auto kernel = &band_uqi_kernel<scalar_t, PX>;
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)) == hipSuccess,
                "band_uqi_partials: could not raise the dynamic LDS limit");
  }
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(part.size(1)), static_cast<unsigned>(x.size(0)), ng * (ng + 1) / 2),
                     dim3(kThreads), lds, stream(), reinterpret_cast<const scalar_t*>(x.data_ptr()), q,
                     taps.data_ptr<acc_t>(), consts.data_ptr<acc_t>(), part.data_ptr<acc_t>(), pairs);
}

}  // namespace

// x [B, C, H, W] (f32 / f16 / bf16 / f64, C >= 2); taps: the 1-D window (odd, <= 15, H and W at least that) and
// consts (-, -, eps), both in the accumulation dtype (f64 for f64 inputs, else f32).  Returns part [B, tiles, pairs]:
// per-tile sums over the valid windows of the UQI map of every band pair i < j, in triu_indices(C, C, 1) order.
at::Tensor band_uqi_partials(const at::Tensor& x, const at::Tensor& taps, const at::Tensor& consts) {
  TM_CHECK_CUDA(x);
  TM_SAME_DEVICE(x, taps);
  TM_SAME_DEVICE(x, consts);
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(taps);
  TM_CHECK_CONTIG(consts);
  TORCH_CHECK(x.dim() == 4 && x.size(1) >= 2, "band_uqi_partials: expects [B, C, H, W] with at least two bands");
  const int k = static_cast<int>(taps.numel());
  TORCH_CHECK(taps.dim() == 1 && k >= 1 && k <= kMaxK && k % 2 == 1, "band_uqi_partials: taps must be odd, 1..", kMaxK);
  const auto acc_type = x.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  TORCH_CHECK(consts.numel() >= 3, "band_uqi_partials: consts must hold (-, -, eps)");
  TORCH_CHECK(taps.scalar_type() == acc_type && consts.scalar_type() == acc_type,
              "band_uqi_partials: taps / constants must be in the accumulation dtype");
  TORCH_CHECK(x.size(2) < (1 << 30) && x.size(3) < (1 << 30), "band_uqi_partials: plane too large");
  TORCH_CHECK(x.size(2) >= k && x.size(3) >= k, "band_uqi_partials: the plane must hold one ", k, " x ", k, " window");
  const long long B = x.size(0), C = x.size(1);
  TORCH_CHECK(B <= 65535 && C <= 1024, "band_uqi_partials: too many samples or bands for one launch");
  const int th = kRG * (acc_type == at::kDouble ? Acc<double>::kPX : Acc<float>::kPX);
  const long long tiles = ((x.size(2) - k + 1 + th - 1) / th) * ((x.size(3) - k + 1 + kTW - 1) / kTW);
  const long long pairs = C * (C - 1) / 2;
  at::Tensor part = at::empty({B, tiles, pairs}, x.options().dtype(acc_type));
  if (B == 0) return part;
  TM_DISPATCH_FLOAT(x.scalar_type(), "band_uqi_partials", [&] {
    launch_band_uqi<scalar_t>(x, taps, consts, part, k, static_cast<int>(pairs));
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return part;
}

// pan [B, C, H, W] -> [B, C, h, w] in the same dtype: the window x window box filter over the mirror-padded planes
// (window / 2 before, window / 2 + window % 2 - 1 after) followed by the bilinear resize (align_corners = False, no
// antialias) to (h, w); h must divide H and w must divide W, window <= 33 and no larger than the plane.
at::Tensor pan_degrade(const at::Tensor& pan, int64_t window, int64_t h, int64_t w) {
  TM_CHECK_CUDA(pan);
  TM_CHECK_CONTIG(pan);
  TORCH_CHECK(pan.dim() == 4, "pan_degrade: expects [B, C, H, W]");
  TORCH_CHECK(pan.size(2) < (1 << 30) && pan.size(3) < (1 << 30), "pan_degrade: plane too large");
  const long long planes = pan.size(0) * pan.size(1);
  TORCH_CHECK(planes <= 65535, "pan_degrade: too many planes for one launch");
  PanGeo q;
  q.H = static_cast<int>(pan.size(2));
  q.W = static_cast<int>(pan.size(3));
  TORCH_CHECK(h >= 1 && w >= 1 && q.H % h == 0 && q.W % w == 0, "pan_degrade: (h, w) must divide the plane");
  TORCH_CHECK(window >= 1 && window <= kMaxBox && window <= q.H && window <= q.W,
              "pan_degrade: window must be 1..", kMaxBox, " and no larger than the plane");
  q.h = static_cast<int>(h);
  q.w = static_cast<int>(w);
  q.rh = q.H / q.h;
  q.rw = q.W / q.w;
  q.ws = static_cast<int>(window);
  q.nth = q.ws + (q.rh % 2 == 0);
  q.ntw = q.ws + (q.rw % 2 == 0);
  q.offh = (q.rh - 1) / 2 - q.ws / 2;
  q.offw = (q.rw - 1) / 2 - q.ws / 2;
  at::Tensor out = at::empty({pan.size(0), pan.size(1), h, w}, pan.options());
  if (planes == 0) return out;
  const size_t esz = pan.scalar_type() == at::kDouble ? 8 : 4;
  q.th = 8;
  q.tw = 32;
  for (;;) {  // halve the tile, the wider extent first, until its source tile fits; 1 x 1 always does
    q.sh = (q.th - 1) * q.rh + q.nth;
    q.sw = (q.tw - 1) * q.rw + q.ntw;
    if (esz * (static_cast<size_t>(q.sh) + q.th) * q.sw <= kPanLds) break;
    TORCH_CHECK(q.th > 1 || q.tw > 1, "pan_degrade: one window does not fit the LDS");
    if (static_cast<long long>(q.tw) * q.rw >= static_cast<long long>(q.th) * q.rh && q.tw > 1) {
      q.tw /= 2;
    } else if (q.th > 1) {
      q.th /= 2;
    } else {
      q.tw /= 2;
    }
  }
  const size_t lds = esz * (static_cast<size_t>(q.sh) + q.th) * q.sw;
  q.tiles_w = (q.w + q.tw - 1) / q.tw;
  const long long tiles = static_cast<long long>((q.h + q.th - 1) / q.th) * q.tiles_w;
  TORCH_CHECK(tiles < (1LL << 31), "pan_degrade: too many tiles");
  TM_DISPATCH_FLOAT(pan.scalar_type(), "pan_degrade", [&] {
    hipLaunchKernelGGL(pan_degrade_kernel<scalar_t>, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(planes)),
                       dim3(kThreads), lds, stream(), reinterpret_cast<const scalar_t*>(pan.data_ptr()), q,
                       reinterpret_cast<scalar_t*>(out.data_ptr()));
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def("band_uqi_partials(Tensor x, Tensor taps, Tensor consts) -> Tensor");
  m.def("pan_degrade(Tensor pan, int window, int h, int w) -> Tensor");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) {
  m.impl("band_uqi_partials", &tm_amd::band_uqi_partials);
  m.impl("pan_degrade", &tm_amd::pan_degrade);
}
