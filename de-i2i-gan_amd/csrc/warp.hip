// The geometric DiffAugment policies (utils/diffaug.py: scale -> rotate -> aniso) on fp32 NCHW images: per sample ONE bilinear
// resampling with a 2x2 matrix about the image centre (include/dei2i_hip.h gives the map op for op), and its adjoint -- the exact
// transpose with the forward's own weights, so the op is differentiable to any order (ops._Warp / _WarpAdjoint).
//
// Forward: one thread per output pixel.  Coordinates, the four weights and the four tap offsets are computed once and reused over
// the channels.  A workgroup is a 32 x 8 pixel tile: with M near the identity a wave reads two 32-pixel row pieces per tap row, and
// under a rotation the tile's footprint in the source stays compact (about 32 x 8 rotated) instead of one 256-pixel line.
//
// Adjoint: the transpose of a bilinear warp is a scatter; here it is a GATHER in a fixed order, without atomics.  One thread owns
// one INPUT pixel (y, x) and sums, over the output pixels (i, j) in ascending row-major order, weight(i, j -> y, x) * g[i][j], the
// weight recomputed from (i, j) by warp_taps -- the function the forward uses -- so what the adjoint adds is bit for bit what the
// forward multiplied by.  Output pixel (i, j) touches (y, x) iff its computed u0 is x - 1 or x and its v0 is y - 1 or y.  The
// thread finds its candidates in a box and keeps those that pass this exact test; the box only has to CONTAIN them.
//
// The box and its margin.  Let T = (cx + tu, cy + tv) as the forward rounds it (the thread forms the same fp32 sums) and
// d = (j - cx, i - cy), exact for W, H <= 2^16.  The forward computes u = fl(fl(fl(m00 dx) + fl(m01 dy)) + Tu).  For a pixel that
// touches (y, x), u is in [x - 1, x + 1) and v in [y - 1, y + 1), so with eps = 2^-24 and S = max(H, W), |m| <= 4, |dx|, |dy| <= S / 2:
//   M d = (u, v) - T + E,   |E| <= eps (|u| + |m00 dx| + |m01 dy| + |m00 dx + m01 dy|) <= eps (S + 2 S + 2 S + 4 S) = 9 S eps
// per component, hence d = Minv ((x, y) - T + (a, b)) + Minv E with |a|, |b| <= 1: d lies within
//   (|i00| + |i01|, |i10| + |i11|)  of  Minv ((x, y) - T),   up to  |Minv E| <= 8 * 9 S eps = 72 S eps <= 0.29  at S = 2^16
// (the usable gate bounds every inverse entry by 4).  The thread computes Minv and the centre in DOUBLE: the products of det are
// exact, |det| >= 1/32 under the gate (some |m| >= 1/8 since M Minv = I, and |det| = |m| / |inverse entry| >= |m| / 4), so the
// centre is off by less than 1e-9 -- the result does not depend on the inverse's precision.  A margin of 1 covers 0.29 + 1e-9
// with room to spare; the box is then at most 2 (8 + 1) + 1 = 19 pixels a side, which the loops also enforce as a hard cap.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace dei2i {
namespace {

// one record of the table (include/dei2i_hip.h: DEI2I_WARP_REC_WORDS words)
struct WarpRec {
  float m00, m01, m10, m11, tu, tv;
  int pad0, pad1;
};
static_assert(sizeof(WarpRec) == 4 * DEI2I_WARP_REC_WORDS && alignof(WarpRec) == 4, "a record is 8 words of a float table");

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;
constexpr double kMargin = 1.0;
constexpr int kBox = 19;                   // 2 * (4 + 4 + kMargin) + 1
constexpr int kMaxSide = 1 << 16;          // the margin argument above holds up to this H and W
constexpr int kChunk = 4;                  // channels per pass of the adjoint's candidate loop

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }          // false for NaN and +-inf

// the gate of include/dei2i_hip.h: a record that fails it is applied as the identity
__device__ __forceinline__ bool usable(const WarpRec& r) {
  if (!(finite_f(r.m00) && finite_f(r.m01) && finite_f(r.m10) && finite_f(r.m11) && finite_f(r.tu) && finite_f(r.tv))) return false;
  const float big = fmaxf(fmaxf(fabsf(r.m00), fabsf(r.m01)), fmaxf(fabsf(r.m10), fabsf(r.m11)));
  const double det = (double)r.m00 * (double)r.m11 - (double)r.m01 * (double)r.m10;
  return big <= 4.f && det != 0.0 && (double)big <= 4.0 * fabs(det);
}

__device__ __forceinline__ WarpRec effective(const WarpRec* __restrict__ tab, long long n) {
  WarpRec r = tab[n];
  if (!usable(r)) r = WarpRec{1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0, 0};
  return r;
}

struct Taps {
  int u0, v0;
  float w00, w01, w10, w11;          // of (v0, u0), (v0, u0 + 1), (v0 + 1, u0), (v0 + 1, u0 + 1)
};

// Where output pixel (i, j) samples and with what weights; false: the pixel is 0 (u or v not finite or outside [-1, W) x [-1, H),
// decided in floating point -- only then are u0 in [-1, W - 1] and v0 in [-1, H - 1] converted).  Both directions call this.
__device__ __forceinline__ bool warp_taps(const WarpRec& r, int i, int j, float cx, float cy, float Wf, float Hf, Taps& t) {
  const float dx = (float)j - cx, dy = (float)i - cy;
  const float u = (r.m00 * dx + r.m01 * dy) + (cx + r.tu);
  const float v = (r.m10 * dx + r.m11 * dy) + (cy + r.tv);
  if (!(u >= -1.f && u < Wf && v >= -1.f && v < Hf)) return false;          // (NaN fails every comparison)
  const float u0 = floorf(u), v0 = floorf(v);
  const float fu = u - u0, fv = v - v0;
  t.u0 = (int)u0;
  t.v0 = (int)v0;
  t.w00 = (1.f - fv) * (1.f - fu);
  t.w01 = (1.f - fv) * fu;
  t.w10 = fv * (1.f - fu);
  t.w11 = fv * fu;
  return true;
}

// item = one 32 x 8 pixel tile of one sample; the pixel of this thread, or false when it is off the image
__device__ __forceinline__ bool tile_pixel(long long item, int tiles_x, int tiles, int H, int W, long long& n, int& i, int& j) {
  n = item / tiles;
  const int tile = (int)(item - n * tiles);
  i = (tile / tiles_x) * kTileH + (int)(threadIdx.x >> 5);
  j = (tile % tiles_x) * kTileW + (int)(threadIdx.x & 31);
  return i < H && j < W;
}

__global__ __launch_bounds__(kThreads) void warp_forward_kernel(const float* __restrict__ src, const WarpRec* __restrict__ tab,
                                                                int C, int H, int W, int tiles_x, int tiles, long long items,
                                                                float* __restrict__ dst) {
  const size_t plane = (size_t)H * W;
  const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    long long n;
    int i, j;
    if (!tile_pixel(item, tiles_x, tiles, H, W, n, i, j)) continue;
    const WarpRec r = effective(tab, n);
    float* out = dst + (size_t)n * C * plane + (size_t)i * W + j;
    Taps t;
    if (!warp_taps(r, i, j, cx, cy, (float)W, (float)H, t)) {
      for (int c = 0; c < C; ++c) out[c * plane] = 0.f;
      continue;
    }
    const bool r0 = t.v0 >= 0, r1 = t.v0 + 1 < H, c0 = t.u0 >= 0, c1 = t.u0 + 1 < W;          // (v0 <= H - 1 and u0 <= W - 1 already)
    // the address of tap (v0, u0), formed only from indices clamped into the image
    const float* p = src + (size_t)n * C * plane + (size_t)(r0 ? t.v0 : 0) * W + (c0 ? t.u0 : 0);
    const int right = (c0 && c1) ? 1 : 0, down = (r0 && r1) ? W : 0;          // a clamped tap is its neighbour: offset 0
    for (int c = 0; c < C; ++c) {
      const float* q = p + c * plane;
      const float t0 = (r0 && c0) ? t.w00 * q[0] : 0.f;
      const float t1 = (r0 && c1) ? t.w01 * q[right] : 0.f;
      const float t2 = (r1 && c0) ? t.w10 * q[down] : 0.f;
      const float t3 = (r1 && c1) ? t.w11 * q[down + right] : 0.f;
      out[c * plane] = ((t0 + t1) + t2) + t3;
    }
  }
}

__global__ __launch_bounds__(kThreads) void warp_adjoint_kernel(const float* __restrict__ src, const WarpRec* __restrict__ tab,
                                                                int C, int H, int W, int tiles_x, int tiles, long long items,
                                                                float* __restrict__ dst) {
  const size_t plane = (size_t)H * W;
  const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    long long n;
    int y, x;
    if (!tile_pixel(item, tiles_x, tiles, H, W, n, y, x)) continue;
    const WarpRec r = effective(tab, n);
    // the candidate box (derivation at the top of the file), in double, clamped to the image BEFORE any conversion to integer
    const double det = (double)r.m00 * (double)r.m11 - (double)r.m01 * (double)r.m10;
    const double i00 = (double)r.m11 / det, i01 = -(double)r.m01 / det, i10 = -(double)r.m10 / det, i11 = (double)r.m00 / det;
    const double a = (double)x - (double)(cx + r.tu), b = (double)y - (double)(cy + r.tv);
    const double jc = (i00 * a + i01 * b) + (double)cx, ic = (i10 * a + i11 * b) + (double)cy;
    const double ex = fabs(i00) + fabs(i01) + kMargin, ey = fabs(i10) + fabs(i11) + kMargin;
    const double jlo = fmax(ceil(jc - ex), 0.0), jhi = fmin(floor(jc + ex), (double)(W - 1));
    const double ilo = fmax(ceil(ic - ey), 0.0), ihi = fmin(floor(ic + ey), (double)(H - 1));
    const bool any = jc == jc && ic == ic && jlo <= jhi && ilo <= ihi;          // (a NaN centre: tu or tv overflowed T, no pixel is valid)
    const int j0 = any ? (int)jlo : 0, i0 = any ? (int)ilo : 0;
    const int j1 = any ? min((int)jhi, j0 + kBox - 1) : -1, i1 = any ? min((int)ihi, i0 + kBox - 1) : -1;
    const float* img = src + (size_t)n * C * plane;
    float* out = dst + (size_t)n * C * plane + (size_t)y * W + x;
    for (int cb = 0; cb < C; cb += kChunk) {
      float acc[kChunk] = {0.f, 0.f, 0.f, 0.f};
      for (int i = i0; i <= i1; ++i) {
        for (int j = j0; j <= j1; ++j) {
          Taps t;
          if (!warp_taps(r, i, j, cx, cy, (float)W, (float)H, t)) continue;
          const unsigned dv = (unsigned)(y - t.v0), du = (unsigned)(x - t.u0);
          if (dv > 1u || du > 1u) continue;                     // (y, x) is none of this pixel's four taps
          const float w = dv ? (du ? t.w11 : t.w10) : (du ? t.w01 : t.w00);
          const float* g = img + (size_t)cb * plane + (size_t)i * W + j;
#pragma unroll
          for (int k = 0; k < kChunk; ++k)
            if (cb + k < C) acc[k] = acc[k] + w * g[k * plane];
        }
      }
#pragma unroll
      for (int k = 0; k < kChunk; ++k)
        if (cb + k < C) out[(size_t)(cb + k) * plane] = acc[k];
    }
  }
}

// One workgroup strides over the warp runs x N records; flags: 3 bits per run of the WHOLE run list (DEI2I_WARP_SCALE / _ROTATE /
// _ANISO; 0: not a warp run, no row in the table).  The call count is read by every thread and stored + 1 by thread 0 behind the
// barrier, as in diffaug_draw_kernel.  GATED: block 5 gates the three policies, block 4 is drawn as without gates, so a row's
// parameters do not depend on its gates and p = 1 is the ungated table.  exp2f, sinf, cosf are the accurate library functions.
template <bool GATED>
__global__ __launch_bounds__(kThreads) void warp_draw_kernel(unsigned long long seed, unsigned long long* __restrict__ counter, int runs,
                                                             unsigned long long flags, int warp_runs, int N, unsigned row0,
                                                             const float* __restrict__ p_dev, WarpRec* __restrict__ tab) {
  const unsigned long long call = *counter;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)call, c1 = (uint32_t)(call >> 32);
  float p = 1.f;
  if (GATED) p = *p_dev;
  for (int i = threadIdx.x; i < warp_runs * N; i += kThreads) {
    const int b = i / N, n = i - b * N;
    int run = 0, fl = 0;
    for (int r = 0, seen = 0; r < runs; ++r) {            // the b-th warp run of the list
      const int g = (int)(flags >> (3 * r)) & 7;
      if (g && seen++ == b) {
        run = r;
        fl = g;
        break;
      }
    }
    const uint32_t row = row0 + (uint32_t)n;
    const Philox4 x = philox4x32_10(c0, c1, (uint32_t)run | (4u << 16), row, k0, k1);
    if (GATED) {
      const Philox4 g = philox4x32_10(c0, c1, (uint32_t)run | (5u << 16), row, k0, k1);
      if (!(unit_float(g.x0) < p)) fl &= ~DEI2I_WARP_SCALE;
      if (!(unit_float(g.x1) < p)) fl &= ~DEI2I_WARP_ROTATE;
      if (!(unit_float(g.x2) < p)) fl &= ~DEI2I_WARP_ANISO;
    }
    float s = 1.f, c = 1.f, sn = 0.f, l = 1.f;
    if (fl & DEI2I_WARP_SCALE) s = exp2f(unit_float(x.x0) - 0.5f);
    if (fl & DEI2I_WARP_ROTATE) {
      const float theta = (2.f * unit_float(x.x1) - 1.f) * 3.14159265358979323846f;
      c = cosf(theta);
      sn = sinf(theta);
    }
    if (fl & DEI2I_WARP_ANISO) l = exp2f(unit_float(x.x2) - 0.5f);
    const float cs = c * s, ss = sn * s;
    tab[i] = WarpRec{l * cs, l * (-ss), ss / l, cs / l, 0.f, 0.f, 0, 0};
  }
  __syncthreads();
  if (threadIdx.x == 0) *counter = call + 1;
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int dei2i_warp(int N, int C, int H, int W, const float* tab_dev, int adjoint, const float* src, float* dst,
                          dei2i_stream s) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || !tab_dev || !src || !dst) return DEI2I_ERR_BAD_ARG;
  const WarpRec* tab = reinterpret_cast<const WarpRec*>(tab_dev);
  if ((long long)N * C * H * W >= (1ll << 40) || (long long)C * H * W >= (1ll << 31)) return DEI2I_ERR_BAD_ARG;
  if (H > kMaxSide || W > kMaxSide) return DEI2I_ERR_BAD_ARG;
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t bytes = (uintptr_t)N * C * H * W * sizeof(float);
  if (a < b + bytes && b < a + bytes) return DEI2I_ERR_BAD_ARG;          // in place (or overlapping): every pixel reads its neighbours
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles = tiles_x * ((H + kTileH - 1) / kTileH);
  const long long items = (long long)N * tiles;
  const unsigned grid = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
  if (adjoint)
    hipLaunchKernelGGL(warp_adjoint_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, src, tab, C, H, W, tiles_x, tiles, items,
                       dst);
  else
    hipLaunchKernelGGL(warp_forward_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, src, tab, C, H, W, tiles_x, tiles, items,
                       dst);
  return (int)hipGetLastError();
}

// both draws: p_dev null = dei2i_warp_draw, else dei2i_warp_draw_p
static int warp_draw_launch(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                            float* tab, dei2i_stream s) {
  if (!counter_dev || !tab || runs <= 0 || runs > DEI2I_DIFFAUG_MAX_RUNS || N <= 0 || row0 < 0) return DEI2I_ERR_BAD_ARG;
  if ((long long)row0 + N > (1ll << 31) || (long long)runs * N >= (1ll << 24)) return DEI2I_ERR_BAD_ARG;
  if ((run_flags >> (3 * runs)) != 0) return DEI2I_ERR_BAD_ARG;
  int warp_runs = 0;
  for (int r = 0; r < runs; ++r) warp_runs += ((run_flags >> (3 * r)) & 7u) != 0;
  if (warp_runs == 0) return DEI2I_ERR_BAD_ARG;                             // (nothing to draw: the launch would only count)
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(counter_dev);
  if (p_dev)
    hipLaunchKernelGGL(warp_draw_kernel<true>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, warp_runs, N, (unsigned)row0, p_dev, reinterpret_cast<WarpRec*>(tab));
  else
    hipLaunchKernelGGL(warp_draw_kernel<false>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, warp_runs, N, (unsigned)row0, p_dev, reinterpret_cast<WarpRec*>(tab));
  return (int)hipGetLastError();
}

extern "C" int dei2i_warp_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, float* tab, dei2i_stream s) {
  return warp_draw_launch(seed, counter_dev, runs, run_flags, N, row0, nullptr, tab, s);
}

extern "C" int dei2i_warp_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                                 float* tab, dei2i_stream s) {
  if (!p_dev) return DEI2I_ERR_BAD_ARG;
  return warp_draw_launch(seed, counter_dev, runs, run_flags, N, row0, p_dev, tab, s);
}
