// Full SSIM / UQI maps of 2-D images and 3-D volumes, with the per-image score from the same launch.
//
// The score kernels (ssim.hip, ssim3d.hip) evaluate only the windows that lie fully inside the input and keep no
// per-pixel value.  The map has a value at every input pixel (the window centred on it, the input reflected at its
// edges without repeating the edge pixel) or, border = valid, at every fully inside window.  No padded copy exists:
// the reflection is an index mapping applied while a tile is staged into LDS.
//
//   block = 256 threads (4 wave64) on a (4*PX) x 64 output tile; lane = output column, every thread owns PX
//           vertically adjacent pixels of it (2-D: PX = 8, fp64 4 or 1 by LDS budget; volumes: PX = 2, fp64 1)
//   1. stage the (TH+kh-1) x (64+kw-1) tile of x and y in LDS in the accumulation type: aligned 16-byte global loads
//      wherever a chunk maps to contiguous in-range source pixels, scalar loads at reflected / ragged edges
//   2. W pass, register blocked: a work item is one row x 4 adjacent output columns.  It walks the row in LDS vectors
//      of 4 (ds_read_b128; the row pitch is a multiple of 4) and slides the window taps through 4 registers, so an
//      input value and a tap are read once for 4 outputs: ~3 (kw+3)/4 LDS reads per output instead of 3 kw.  The
//      taps are zero padded in LDS, which makes the pitch columns past the tile harmless (they are staged as zeros).
//   3. H pass: the PX owned pixels share every row they read (5 (kh+PX-1)/PX LDS reads per pixel), taps slide through
//      PX registers the same way.
//   4. 2-D: SSIM / UQI per pixel; the tile of results goes through the (now free) staging LDS and leaves as aligned
//      16-byte stores, scalar at ragged edges.  Interior pixels are added to the block's (sum, sum CS) partial.
//      Volumes: the march of ssim3d.hip over the padded depth index 0 .. D+2pd-1, staging source slice
//      reflect(s - pd) (halo slices are re-read); the register ring of KD pending output slices is statically indexed
//      (only the ring update is instantiated per slot, the staging and the passes exist once in the code).
//      A completed slot stores its row segments of the map slice (one 64-pixel run per wave and row) and adds to the
//      partial only where the voxel is interior.
//   One partial per block, written in a fixed order: no atomics, bit-identical between calls.
#include "../common/tm_common.h"

#include <tuple>
#include <type_traits>
#include <utility>

namespace tm_amd {
namespace {

constexpr int kTW = 64;     // output cols per block (one wave across)
constexpr int kGW = 4;      // adjacent outputs of one W-pass work item
constexpr int kMaxK = 33;   // largest in-plane window edge; keep SSIM_MAP_MAX_WINDOW (ops/__init__.py) equal
constexpr int kMaxKD = 11;  // largest depth window (ring slots held in registers)
constexpr int kTapPad = 40;  // zero-padded tap arrays: kMaxK + 7 (H pass, PX = 8), 4 * ceil((kMaxK + 3) / 4) (W pass)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr size_t kLdsBudget = 150 * 1024;

template <typename T>
struct Acc {
  using type = float;
  static constexpr int kImgPX = 8;       // owned pixels per thread in the image kernel ...
  static constexpr int kImgPXSmall = 8;  // ... and where that tile's LDS does not fit
  static constexpr int kVolPX = 2;       // owned pixels per thread in the volume kernel
};
template <>
struct Acc<double> {
  using type = double;
  static constexpr int kImgPX = 4;
  static constexpr int kImgPXSmall = 1;  // fp64 windows over 23
  static constexpr int kVolPX = 1;       // the fp64 ring is twice as wide
};

template <typename T>
using vec4 = T __attribute__((ext_vector_type(4)));

template <typename scalar_t>
__device__ __forceinline__ typename Acc<scalar_t>::type load_acc(scalar_t v) {
  if constexpr (std::is_same<scalar_t, double>::value) {
    return v;
  } else {
    return to_f32(v);
  }
}

// In-plane geometry shared by both kernels.  Output pixel (r, c) reads staged rows r - r0 .. + kh - 1 and staged cols
// c - c0 .. + kw - 1 of its tile; the tile's first staged row / col is source (r0 - ph, c0 - pw).
struct Geo {
  int H, W;      // source plane
  int kh, kw;    // window
  int oh, ow;    // stored map plane: H x W (reflect) or the valid windows
  int ph, pw;    // half windows (reflect) or 0 (valid)
  int reflect;   // source indices outside the plane are mirrored (else such pixels are never needed)
  int pitch;     // LDS row pitch of the staged tile, a multiple of 4: 60 + 4 * nj4
  int nj4;       // W-pass steps in vectors of 4: ceil((kw + 3) / 4)
};

__host__ __device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One (in_h x pitch) tile of plane `g` ([H, W], row-major) -> LDS `s`; zero where the source index (after the
// reflection) falls outside the plane and in the pitch columns past the tile.  Work items are (row, 16-byte chunk)
// pairs; the chunks are aligned in global memory, so a row starts `mis` elements into its first.
template <typename scalar_t>
__device__ __forceinline__ void stage_tile(const scalar_t* __restrict__ g, typename Acc<scalar_t>::type* __restrict__ s,
                                           const Geo& q, int r0, int c0, int in_h, int tid) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kVec = 16 / sizeof(scalar_t);
  const int in_w = kTW + q.kw - 1;
  const int nv = (q.pitch + 2 * kVec - 2) / kVec;  // chunks that cover pitch elements at any misalignment
  const int cs = c0 - q.pw;                        // source col of tile col 0, before any reflection
  for (int i = tid; i < in_h * nv; i += kThreads) {
    const int r = i / nv, k = i - r * nv;
    acc_t* srow = s + r * q.pitch;
    int gr = r0 - q.ph + r;
    if (q.reflect) gr = mirror(gr, q.H);
    const bool row_ok = gr >= 0 && gr < q.H;
    const long long row_off = static_cast<long long>(row_ok ? gr : 0) * q.W;
    const long long e0 = row_off + cs;  // element of tile col 0 (may lie before the row)
    const int mis = static_cast<int>(
        (static_cast<long long>(reinterpret_cast<uintptr_t>(g) / sizeof(scalar_t)) + e0) & (kVec - 1));
    const int cb = k * kVec - mis;  // first tile col of this chunk
    if (row_ok && cb >= 0 && cb + kVec <= in_w && cs + cb >= 0 && cs + cb + kVec <= q.W) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(g + (e0 + cb));
      scalar_t v[kVec];
      __builtin_memcpy(v, &raw, sizeof(raw));
#pragma unroll
      for (int e = 0; e < kVec; ++e) srow[cb + e] = load_acc(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = cb + e;
        if (col < 0 || col >= q.pitch) continue;
        int c = cs + col;
        if (q.reflect) c = mirror(c, q.W);
        const bool ok = row_ok && col < in_w && c >= 0 && c < q.W;
        srow[col] = ok ? load_acc(g[row_off + c]) : acc_t(0);
      }
    }
  }
}

// W pass over the staged tile: hm[m][row][col] = sum_j ww[j] * v_m[row][col + j] for the 5 moments
// v = (x, y, x*x, y*y, x*y).  `wq`: ww zero padded to 4 * nj4 entries.
template <typename acc_t>
__device__ __forceinline__ void w_pass(const acc_t* __restrict__ sx, const acc_t* __restrict__ sy,
                                       const acc_t* __restrict__ wq, acc_t* __restrict__ hm, const Geo& q, int in_h,
                                       int tid) {
  using v4 = vec4<acc_t>;
  const int plane_sz = in_h * kTW;
  for (int i = tid; i < in_h * (kTW / kGW); i += kThreads) {
    const int r = i / (kTW / kGW), c = (i % (kTW / kGW)) * kGW;
    const v4* rx = reinterpret_cast<const v4*>(sx + r * q.pitch + c);
    const v4* ry = reinterpret_cast<const v4*>(sy + r * q.pitch + c);
    acc_t m[kGW][5];
#pragma unroll
    for (int o = 0; o < kGW; ++o)
#pragma unroll
      for (int k = 0; k < 5; ++k) m[o][k] = acc_t(0);
    acc_t w[kGW] = {0, 0, 0, 0};  // at input col c + j: the taps j, j - 1, j - 2, j - 3 of outputs c .. c + 3
    for (int j4 = 0; j4 < q.nj4; ++j4) {
      const v4 a4 = rx[j4], b4 = ry[j4], wn = reinterpret_cast<const v4*>(wq)[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w[3] = w[2];
        w[2] = w[1];
        w[1] = w[0];
        w[0] = wn[e];
        const acc_t a = a4[e], b = b4[e];
        const acc_t v[5] = {a, b, a * a, b * b, a * b};
#pragma unroll
        for (int o = 0; o < kGW; ++o)
#pragma unroll
          for (int k = 0; k < 5; ++k) m[o][k] += w[o] * v[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      v4 out;
#pragma unroll
      for (int o = 0; o < kGW; ++o) out[o] = m[o][k];
      *reinterpret_cast<v4*>(hm + k * plane_sz + r * kTW + c) = out;
    }
  }
}

// H pass for the PX vertically adjacent pixels (rows row_a .. row_a + PX - 1, column `lane`) of one thread.
// `wp`: wh zero padded to kh + PX - 1 entries.
template <typename acc_t, int PX>
__device__ __forceinline__ void h_pass(const acc_t* __restrict__ hm, const acc_t* __restrict__ wp, int in_h, int kh,
                                       int row_a, int lane, acc_t (&mom)[PX][5]) {
  const int plane_sz = in_h * kTW;
  acc_t w[PX];
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    w[p] = acc_t(0);
#pragma unroll
    for (int k = 0; k < 5; ++k) mom[p][k] = acc_t(0);
  }
  for (int j = 0; j < kh + PX - 1; ++j) {
#pragma unroll
    for (int p = PX - 1; p > 0; --p) w[p] = w[p - 1];  // pixel p sees tap j - p
    w[0] = wp[j];
    const int o = (row_a + j) * kTW + lane;
    acc_t v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = hm[k * plane_sz + o];
#pragma unroll
    for (int p = 0; p < PX; ++p)
#pragma unroll
      for (int k = 0; k < 5; ++k) mom[p][k] += w[p] * v[k];
  }
}

// SSIM (mode 0; cs = contrast sensitivity) or UQI (mode 1) of one window from its 5 filtered moments: the arithmetic
// of ssim2d_kernel, variance clamps included.
template <typename acc_t>
__device__ __forceinline__ void window_value(const acc_t (&m)[5], acc_t c1, acc_t c2, acc_t eps, int mode, acc_t& val,
                                             acc_t& cs) {
  const acc_t mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
  const acc_t sxx = m[2] - mxx > 0 ? m[2] - mxx : acc_t(0);
  const acc_t syy = m[3] - myy > 0 ? m[3] - myy : acc_t(0);
  const acc_t sxy = m[4] - mxy;
  if (mode == 0) {
    const acc_t upper = 2 * sxy + c2;
    const acc_t lower = sxx + syy + c2;
    val = ((2 * mxy + c1) * upper) / ((mxx + myy + c1) * lower);
    cs = upper / lower;
  } else {
    val = ((2 * mxy) * (2 * sxy)) / ((mxx + myy) * (sxx + syy) + eps);
    cs = acc_t(0);
  }
}

// Sum (a, b) over the block into part[slot]; ends with a block barrier passed by every thread.
template <typename acc_t>
__device__ __forceinline__ void block_partial(acc_t a, acc_t b, acc_t (&red)[2][kWaves], acc_t* __restrict__ part,
                                              long long slot, int tid) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((tid & (kWave - 1)) == 0) {
    red[0][tid / kWave] = a;
    red[1][tid / kWave] = b;
  }
  __syncthreads();
  if (tid == 0) {
    acc_t sa = 0, sb = 0;
    for (int w = 0; w < kWaves; ++w) {
      sa += red[0][w];
      sb += red[1][w];
    }
    part[slot * 2] = sa;
    part[slot * 2 + 1] = sb;
  }
}

// f(integral_constant<int, R>) for the R in 0 .. N-1 that equals r (a chain of wave-uniform compares)
template <typename F, int... R>
__device__ __forceinline__ void static_switch(int r, std::integer_sequence<int, R...>, F&& f) {
  ((r == R ? (f(std::integral_constant<int, R>{}), 0) : 0), ...);
}

template <typename scalar_t, int PX>
__global__ void __launch_bounds__(kThreads)
    ssim2d_map_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y, Geo q,
                      const typename Acc<scalar_t>::type* __restrict__ wh,
                      const typename Acc<scalar_t>::type* __restrict__ ww,
                      const typename Acc<scalar_t>::type* __restrict__ c12, int tiles_w, int mode,
                      scalar_t* __restrict__ map, typename Acc<scalar_t>::type* __restrict__ part) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kTH = kWaves * PX;
  constexpr int kVec = 16 / sizeof(scalar_t);
  extern __shared__ __attribute__((aligned(32))) char smem[];
  const int in_h = kTH + q.kh - 1;
  acc_t* sx = reinterpret_cast<acc_t*>(smem);
  acc_t* sy = sx + in_h * q.pitch;
  acc_t* hm = sy + in_h * q.pitch;  // 5 x [in_h][kTW]
  __shared__ __attribute__((aligned(32))) acc_t swh[kTapPad], sww[kTapPad];
  __shared__ acc_t red[2][kWaves];

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kTH, c0 = (tile % tiles_w) * kTW;
  const scalar_t* px = x + plane * q.H * q.W;
  const scalar_t* py = y + plane * q.H * q.W;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  if (tid < kTapPad) {
    swh[tid] = tid < q.kh ? wh[tid] : acc_t(0);
    sww[tid] = tid < q.kw ? ww[tid] : acc_t(0);
  }
  stage_tile(px, sx, q, r0, c0, in_h, tid);
  stage_tile(py, sy, q, r0, c0, in_h, tid);
  __syncthreads();
  w_pass(sx, sy, sww, hm, q, in_h, tid);
  __syncthreads();
  const int row_a = wave * PX;
  acc_t mom[PX][5];
  h_pass<acc_t, PX>(hm, swh, in_h, q.kh, row_a, lane, mom);

  // sx / sy are dead since the barrier after the W pass: the tile of results passes through them
  scalar_t* so = reinterpret_cast<scalar_t*>(smem);
  const acc_t c1 = c12[0], c2 = c12[1], eps = c12[2];
  acc_t s_val = 0, s_cs = 0;
  const int c = c0 + lane;
  const bool col_in = c >= q.pw && c < q.ow - q.pw;
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const int r = r0 + row_a + p;
    if (r >= q.oh || c >= q.ow) continue;
    acc_t val, cs;
    window_value(mom[p], c1, c2, eps, mode, val, cs);
    so[(row_a + p) * kTW + lane] = static_cast<scalar_t>(val);
    if (col_in && r >= q.ph && r < q.oh - q.ph) {  // with border = valid, ph = pw = 0: every stored pixel
      s_val += val;
      s_cs += cs;
    }
  }
  block_partial(s_val, s_cs, red, part, plane * gridDim.x + tile, tid);  // barrier: `so` is complete

  scalar_t* mp = map + plane * q.oh * q.ow;
  const int rows = min(kTH, q.oh - r0), row_len = min(kTW, q.ow - c0);
  constexpr int nv = (kTW + 2 * kVec - 2) / kVec;
  for (int i = tid; i < rows * nv; i += kThreads) {
    const int r = i / nv, k = i - r * nv;
    scalar_t* grow = mp + static_cast<long long>(r0 + r) * q.ow + c0;
    const scalar_t* srow = so + r * kTW;
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(grow) / sizeof(scalar_t)) & (kVec - 1));
    const int cb = k * kVec - mis;
    if (cb >= 0 && cb + kVec <= row_len) {
      scalar_t v[kVec];
#pragma unroll
      for (int e = 0; e < kVec; ++e) v[e] = srow[cb + e];
      u32x4 raw;
      __builtin_memcpy(&raw, v, sizeof(raw));
      *reinterpret_cast<u32x4*>(grow + cb) = raw;
    } else {
#pragma unroll
      for (int e = 0; e < kVec; ++e) {
        const int col = cb + e;
        if (col >= 0 && col < row_len) grow[col] = srow[col];
      }
    }
  }
}

template <typename scalar_t, int KD>
__global__ void __launch_bounds__(kThreads)
    ssim3d_map_kernel(const scalar_t* __restrict__ x, const scalar_t* __restrict__ y, int D, Geo q,
                      const typename Acc<scalar_t>::type* __restrict__ wd,
                      const typename Acc<scalar_t>::type* __restrict__ wh,
                      const typename Acc<scalar_t>::type* __restrict__ ww,
                      const typename Acc<scalar_t>::type* __restrict__ c12, int tiles_w, int chunk,
                      scalar_t* __restrict__ map, typename Acc<scalar_t>::type* __restrict__ part) {
  using acc_t = typename Acc<scalar_t>::type;
  constexpr int kPX = Acc<scalar_t>::kVolPX;
  constexpr int kTH = kWaves * kPX;
  constexpr int kPD = KD / 2;
  extern __shared__ __attribute__((aligned(32))) char smem[];
  const int in_h = kTH + q.kh - 1;
  acc_t* sx = reinterpret_cast<acc_t*>(smem);
  acc_t* sy = sx + in_h * q.pitch;
  acc_t* hm = sy + in_h * q.pitch;  // 5 x [in_h][kTW]
  __shared__ __attribute__((aligned(32))) acc_t swh[kTapPad], sww[kTapPad];
  __shared__ acc_t red[2][kWaves];

  const long long plane = blockIdx.y;
  const int tile = blockIdx.x;
  const int r0 = (tile / tiles_w) * kTH, c0 = (tile % tiles_w) * kTW;
  const int z0 = blockIdx.z * chunk;              // first output slice == first padded input slice of this block
  const int n_in = min(chunk, D - z0) + KD - 1;   // padded slices to march over; z0 + n_in <= D + 2 * kPD
  const long long slice = static_cast<long long>(q.H) * q.W;
  const scalar_t* px = x + plane * D * slice;
  const scalar_t* py = y + plane * D * slice;
  scalar_t* mp = map + plane * D * slice;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  if (tid < kTapPad) {
    swh[tid] = tid < q.kh ? wh[tid] : acc_t(0);
    sww[tid] = tid < q.kw ? ww[tid] : acc_t(0);
  }
  acc_t wdr[KD];
#pragma unroll
  for (int j = 0; j < KD; ++j) wdr[j] = wd[j];
  const acc_t c1 = c12[0], c2 = c12[1];

  const int row_a = wave * kPX;  // first owned row of the tile; the owned column is `lane`
  const int c = c0 + lane;
  bool ok[kPX], inner[kPX];
#pragma unroll
  for (int p = 0; p < kPX; ++p) {
    const int r = r0 + row_a + p;
    ok[p] = r < q.H && c < q.W;
    inner[p] = r >= q.ph && r < q.H - q.ph && c >= q.pw && c < q.W - q.pw;
  }
  acc_t ring[KD][kPX][5];
#pragma unroll
  for (int s = 0; s < KD; ++s)
#pragma unroll
    for (int p = 0; p < kPX; ++p)
#pragma unroll
      for (int k = 0; k < 5; ++k) ring[s][p][k] = acc_t(0);
  acc_t s_val = 0, s_cs = 0;

  int r = 0;  // s mod KD, block-uniform
  for (int s = 0; s < n_in; ++s) {
    // the previous slice's W pass (reader of sx / sy) ended before its second barrier
    const long long src = mirror(z0 + s - kPD, D) * slice;
    stage_tile(px + src, sx, q, r0, c0, in_h, tid);
    stage_tile(py + src, sy, q, r0, c0, in_h, tid);
    __syncthreads();  // also: the previous slice's H pass (reader of hm) is done
    w_pass(sx, sy, sww, hm, q, in_h, tid);
    __syncthreads();
    acc_t mom[kPX][5];
    h_pass<acc_t, kPX>(hm, swh, in_h, q.kh, row_a, lane, mom);
    // Only the ring update depends on r; it alone is instantiated per value of r, so every slot and tap index in
    // it is a constant and the staging and the two passes above exist once in the code.
    static_switch(r, std::make_integer_sequence<int, KD>{}, [&](auto rc) __attribute__((always_inline)) {
      constexpr int R = decltype(rc)::value;
      // depth ring: padded slice s is tap (R - slot) mod KD of the output slice pending in that slot
#pragma unroll
      for (int t = 0; t < KD; ++t) {
        const acc_t w = wdr[(R - t + KD) % KD];
#pragma unroll
        for (int p = 0; p < kPX; ++p)
#pragma unroll
          for (int k = 0; k < 5; ++k) ring[t][p][k] += w * mom[p][k];
      }
      constexpr int qd = (R + 1) % KD;  // the slot that just took tap KD - 1: output slice z0 + s - (KD - 1) < D
      if (s >= KD - 1) {
        const int z = z0 + s - (KD - 1);
        const bool z_in = z >= kPD && z < D - kPD;
#pragma unroll
        for (int p = 0; p < kPX; ++p) {
          if (!ok[p]) continue;
          acc_t val, cs;
          window_value(ring[qd][p], c1, c2, acc_t(0), 0, val, cs);
          mp[z * slice + static_cast<long long>(r0 + row_a + p) * q.W + c] = static_cast<scalar_t>(val);
          if (z_in && inner[p]) {
            s_val += val;
            s_cs += cs;
          }
        }
      }
#pragma unroll
      for (int p = 0; p < kPX; ++p)
#pragma unroll
        for (int k = 0; k < 5; ++k) ring[qd][p][k] = acc_t(0);
    });
    r = r + 1 == KD ? 0 : r + 1;
  }
  block_partial(s_val, s_cs, red, part, (plane * gridDim.z + blockIdx.z) * gridDim.x + tile, tid);
}

struct MapArgs {
  Geo q;
  bool dbl;
  at::ScalarType acc_type;
};

// shared argument checks of both launchers; x is [P, (D,) H, W]
MapArgs check_args(const char* name, const at::Tensor& x, const at::Tensor& y, const at::Tensor& wh,
                   const at::Tensor& ww, const at::Tensor& c12, bool reflect) {
  TM_CHECK_CONTIG(x);
  TM_CHECK_CONTIG(y);
  TORCH_CHECK(x.sizes() == y.sizes() && x.scalar_type() == y.scalar_type(), name, ": x / y mismatch");
  TM_SAME_DEVICE(x, y);
  TM_SAME_DEVICE(x, wh);
  TM_SAME_DEVICE(x, ww);
  TM_SAME_DEVICE(x, c12);
  TM_CHECK_CONTIG(wh);
  TM_CHECK_CONTIG(ww);
  TM_CHECK_CONTIG(c12);
  MapArgs a;
  Geo& q = a.q;
  q.kh = static_cast<int>(wh.numel());
  q.kw = static_cast<int>(ww.numel());
  TORCH_CHECK(q.kh >= 1 && q.kw >= 1 && q.kh <= kMaxK && q.kw <= kMaxK, name, ": in-plane window must be 1..", kMaxK);
  TORCH_CHECK(!reflect || (q.kh % 2 == 1 && q.kw % 2 == 1), name, ": a reflected border needs an odd window");
  TORCH_CHECK(x.size(-2) < (1 << 30) && x.size(-1) < (1 << 30), name, ": extent too large");
  q.H = static_cast<int>(x.size(-2));
  q.W = static_cast<int>(x.size(-1));
  TORCH_CHECK(q.H >= q.kh && q.W >= q.kw, name, ": input smaller than the window");
  TORCH_CHECK(x.size(0) <= 65535, name, ": too many planes for one launch");
  q.reflect = reflect ? 1 : 0;
  q.ph = reflect ? q.kh / 2 : 0;
  q.pw = reflect ? q.kw / 2 : 0;
  q.oh = reflect ? q.H : q.H - q.kh + 1;
  q.ow = reflect ? q.W : q.W - q.kw + 1;
  q.nj4 = (q.kw + kGW - 1 + 3) / 4;
  q.pitch = kTW - kGW + 4 * q.nj4;
  a.dbl = x.scalar_type() == at::kDouble;
  a.acc_type = a.dbl ? at::kDouble : at::kFloat;
  TORCH_CHECK(c12.numel() >= 3, name, ": c12 must hold (c1, c2, eps)");
  TORCH_CHECK(wh.scalar_type() == a.acc_type && ww.scalar_type() == a.acc_type && c12.scalar_type() == a.acc_type,
              name, ": window / constants must be in the accumulation dtype");
  return a;
}

size_t lds_bytes(const Geo& q, int th, bool dbl) {
  const size_t in_h = th + q.kh - 1;
  return (dbl ? sizeof(double) : sizeof(float)) * (2 * in_h * q.pitch + 5 * in_h * kTW);
}

template <typename K>
void raise_lds_limit(K kernel, size_t lds, const char* name) {
  if (lds > 64 * 1024) {
    TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds)) == hipSuccess,
                name, ": could not raise the dynamic LDS limit");
  }
}

}  // namespace

// x, y: [P, H, W] planes (contiguous, same dtype); wh [kh], ww [kw] window taps and c12 [3] (c1, c2, eps) in the
// accumulation dtype (f32, or f64 for f64 inputs); mode 0 = SSIM, 1 = UQI.  reflect: map [P, H, W], the window
// centred on every pixel with mirrored borders (odd windows); else map [P, H-kh+1, W-kw+1], the valid windows.
// Returns (map in the input dtype, part [P, tiles, 2] of per-tile (sum SSIM|UQI, sum CS) over the valid windows).
std::tuple<at::Tensor, at::Tensor> ssim2d_map(const at::Tensor& x, const at::Tensor& y, const at::Tensor& wh,
                                              const at::Tensor& ww, const at::Tensor& c12, int64_t mode,
                                              bool reflect) {
  TM_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 3, "ssim2d_map: expects [planes, H, W]");
  TORCH_CHECK(mode == 0 || mode == 1, "ssim2d_map: mode must be 0 (SSIM) or 1 (UQI)");
  const MapArgs a = check_args("ssim2d_map", x, y, wh, ww, c12, reflect);
  const Geo& q = a.q;
  // the tallest tile whose LDS fits: 32 rows; fp64 16 rows up to window 23, 4 rows above
  const bool tall = !a.dbl || lds_bytes(q, kWaves * Acc<double>::kImgPX, true) <= kLdsBudget;
  const int th = kWaves * (!a.dbl ? Acc<float>::kImgPX : tall ? Acc<double>::kImgPX : Acc<double>::kImgPXSmall);
  const size_t lds = lds_bytes(q, th, a.dbl);
  TORCH_CHECK(lds <= kLdsBudget, "ssim2d_map: window too large for the LDS tile");
  const long long planes = x.size(0);
  const int tiles_w = (q.ow + kTW - 1) / kTW, tiles_h = (q.oh + th - 1) / th;
  const long long tiles = static_cast<long long>(tiles_w) * tiles_h;
  TORCH_CHECK(tiles < (1LL << 31), "ssim2d_map: too many tiles for one launch");
  at::Tensor map = at::empty({planes, q.oh, q.ow}, x.options());
  at::Tensor part = at::empty({planes, tiles, 2}, x.options().dtype(a.acc_type));
  if (planes == 0) return {map, part};
  auto s = stream();
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(planes));
  TM_DISPATCH_FLOAT(x.scalar_type(), "ssim2d_map", [&] {
    using acc_t = typename Acc<scalar_t>::type;
    auto launch = [&](auto px_c) {
      constexpr int PX = decltype(px_c)::value;
      raise_lds_limit(&ssim2d_map_kernel<scalar_t, PX>, lds, "ssim2d_map");
      hipLaunchKernelGGL((ssim2d_map_kernel<scalar_t, PX>), grid, dim3(kThreads), lds, s,
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),
                         reinterpret_cast<const scalar_t*>(y.data_ptr()), q, wh.data_ptr<acc_t>(),
                         ww.data_ptr<acc_t>(), c12.data_ptr<acc_t>(), tiles_w, static_cast<int>(mode),
                         reinterpret_cast<scalar_t*>(map.data_ptr()), part.data_ptr<acc_t>());
    };
    if (tall) {
      launch(std::integral_constant<int, Acc<scalar_t>::kImgPX>{});
    } else {
      launch(std::integral_constant<int, Acc<scalar_t>::kImgPXSmall>{});
    }
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {map, part};
}

// x, y: [P, D, H, W] volumes; wd [kd] (odd, at most 11), wh, ww and c12 as above.  depth_chunk > 0 forces the number
// of output slices per block, 0 lets the launcher pick.  Returns (map [P, D, H, W] in the input dtype with mirrored
// borders, part [P, chunks * tiles, 2] of per-block (sum SSIM, sum CS) over the valid windows).
std::tuple<at::Tensor, at::Tensor> ssim3d_map(const at::Tensor& x, const at::Tensor& y, const at::Tensor& wd,
                                              const at::Tensor& wh, const at::Tensor& ww, const at::Tensor& c12,
                                              int64_t depth_chunk) {
  TM_CHECK_CUDA(x);
  TORCH_CHECK(x.dim() == 4, "ssim3d_map: expects [planes, D, H, W]");
  const MapArgs a = check_args("ssim3d_map", x, y, wh, ww, c12, true);
  const Geo& q = a.q;
  TM_SAME_DEVICE(x, wd);
  TM_CHECK_CONTIG(wd);
  TORCH_CHECK(wd.scalar_type() == a.acc_type, "ssim3d_map: window must be in the accumulation dtype");
  const int kd = static_cast<int>(wd.numel());
  TORCH_CHECK(kd >= 1 && kd <= kMaxKD && kd % 2 == 1, "ssim3d_map: depth window must be odd and 1..", kMaxKD);
  TORCH_CHECK(x.size(1) < (1 << 30), "ssim3d_map: extent too large");
  const int D = static_cast<int>(x.size(1));
  TORCH_CHECK(D >= kd, "ssim3d_map: volume smaller than the window");
  TORCH_CHECK(depth_chunk >= 0, "ssim3d_map: depth_chunk must be >= 0");
  const int th = kWaves * (a.dbl ? Acc<double>::kVolPX : Acc<float>::kVolPX);
  const size_t lds = lds_bytes(q, th, a.dbl);
  TORCH_CHECK(lds <= kLdsBudget, "ssim3d_map: window too large for the LDS tile");
  const long long planes = x.size(0);
  const int tiles_w = (q.W + kTW - 1) / kTW, tiles_h = (q.H + th - 1) / th;
  const long long tiles = static_cast<long long>(tiles_w) * tiles_h;
  TORCH_CHECK(tiles < (1LL << 31), "ssim3d_map: too many in-plane tiles for one launch");
  long long chunk = depth_chunk;
  if (chunk == 0) {
    // the longest chunk that still leaves ~2 blocks per CU (every chunk re-reads kd - 1 halo slices), not below kd
    const long long want = 2LL * cu_count(x.get_device());
    const long long in_plane = std::max<long long>(1, tiles * planes);
    const long long n_chunks = (want + in_plane - 1) / in_plane;
    chunk = std::max<long long>(D / n_chunks, kd);
  }
  chunk = std::min<long long>(chunk, D);
  const int chunks = static_cast<int>((D + chunk - 1) / chunk);
  TORCH_CHECK(chunks <= 65535, "ssim3d_map: too many depth chunks for one launch");
  at::Tensor map = at::empty_like(x);
  at::Tensor part = at::empty({planes, chunks * tiles, 2}, x.options().dtype(a.acc_type));
  if (planes == 0) return {map, part};
  auto s = stream();
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(planes), static_cast<unsigned>(chunks));
  TM_DISPATCH_FLOAT(x.scalar_type(), "ssim3d_map", [&] {
    using acc_t = typename Acc<scalar_t>::type;
    auto launch = [&](auto kd_c) {
      constexpr int KD = decltype(kd_c)::value;
      raise_lds_limit(&ssim3d_map_kernel<scalar_t, KD>, lds, "ssim3d_map");
      hipLaunchKernelGGL((ssim3d_map_kernel<scalar_t, KD>), grid, dim3(kThreads), lds, s,
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),
                         reinterpret_cast<const scalar_t*>(y.data_ptr()), D, q, wd.data_ptr<acc_t>(),
                         wh.data_ptr<acc_t>(), ww.data_ptr<acc_t>(), c12.data_ptr<acc_t>(), tiles_w,
                         static_cast<int>(chunk), reinterpret_cast<scalar_t*>(map.data_ptr()),
                         part.data_ptr<acc_t>());
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
  return {map, part};
}

}  // namespace tm_amd

TORCH_LIBRARY_FRAGMENT(tm_amd, m) {
  m.def("ssim2d_map(Tensor x, Tensor y, Tensor wh, Tensor ww, Tensor c12, int mode, bool reflect) -> (Tensor, Tensor)");
  m.def(
      "ssim3d_map(Tensor x, Tensor y, Tensor wd, Tensor wh, Tensor ww, Tensor c12, int depth_chunk) -> "
      "(Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(tm_amd, CUDA, m) {
  m.impl("ssim2d_map", &tm_amd::ssim2d_map);
  m.impl("ssim3d_map", &tm_amd::ssim3d_map);
}
