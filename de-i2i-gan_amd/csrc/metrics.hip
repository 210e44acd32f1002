// Validation metrics on fp32 NCHW images (trainer.validate(); ops.image_metrics / ops.clf_counts): per image the sums PSNR, L1
// and SSIM are made of, and the confusion counts of the discriminator's classifier -- accumulated on the device, no host read.
//
// dei2i_image_metrics.  SSIM of Wang et al. 2004: 11-tap Gaussian window (sigma 1.5, normalised), "valid" positions only, so an
// H x W plane has (H - 10) x (W - 10) of them.  One workgroup owns one 32 x 32 tile of window positions of one plane:
//   1. it stages the 42 x 42 input halo of x and of y in LDS (pitch 44: whole quads), read from memory once -- 16-byte loads when
//      VEC holds (blit.hip's rule: W % 4 == 0 and 16-byte aligned pointers, so a quad is wholly inside or outside the plane),
//      scalar loads otherwise; what lies off the plane is 0;
//   2. the pixel-error sums (squared, absolute; with a mask also over the pixels whose mask is not 0, and their count) come from
//      the staged tile over the tile's OWNER region, rows [i0, i0 + 32) and columns [j0, j0 + 32) of the plane -- the last tile
//      row / column owns up to the plane's edge, H - i0 <= 42 rows -- so overlapping halos count every pixel exactly once;
//   3. the horizontal pass writes the five maps (x, y, x^2, y^2, xy) of 42 rows x 32 columns to LDS, the vertical pass and the
//      SSIM formula stay in registers, four positions per thread.
// Both passes accumulate in float64 and the maps are rounded to fp32 once when stored: sigma^2 = E[x^2] - mu^2 is a small difference
// of numbers near 1 that stands next to C2 = (0.03 L)^2 = 3.6e-3, and eleven fp32 roundings per tap line would show in the fifth digit of SSIM.
// LDS: 2 * 42 * 44 * 4 + 5 * 42 * 32 * 4 + 64 = 41 728 bytes; 170 VGPRs, no scratch, 2 waves per SIMD.  Every workgroup stores six float64 partials (no atomics); a second
// launch sums a plane's tiles and an image's planes in a fixed order: the result is bit-reproducible.
//
// dei2i_clf_counts: one workgroup over (N, K) logits and targets, rows in chunks of 256; thread k < K owns class k's four counts,
// so no atomics either; it adds into the caller's int64 words.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kTaps = 11;
constexpr int kHalo = kTile + kTaps - 1;      // 42
constexpr int kPitch = 44;                    // whole quads per staged row
constexpr int kQuads = kPitch / 4;
constexpr int kSums = 6;                      // sse, sae, masked sse, masked sae, masked count, ssim

struct Window {
  double w[kTaps];
};

// the halo of one plane at (i0, j0) -> L[kHalo][kPitch]; off the plane: 0
template <bool VEC>
__device__ __forceinline__ void stage(const float* __restrict__ plane, int H, int W, int i0, int j0, float* __restrict__ L) {
  if (VEC) {
    for (int q = threadIdx.x; q < kHalo * kQuads; q += kThreads) {
      const int r = q / kQuads, c = (q - r * kQuads) * 4;
      const int i = i0 + r, j = j0 + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < H && j < W) v = *reinterpret_cast<const float4*>(plane + (size_t)i * W + j);      // (W % 4 == 0: j + 3 < W)
      *reinterpret_cast<float4*>(L + r * kPitch + c) = v;
    }
  } else {
    for (int e = threadIdx.x; e < kHalo * kPitch; e += kThreads) {
      const int r = e / kPitch, c = e - r * kPitch;
      const int i = i0 + r, j = j0 + c;
      L[e] = (i < H && j < W) ? plane[(size_t)i * W + j] : 0.f;
    }
  }
}

// the sum of v over the workgroup in a fixed order, valid in thread 0; red: one double per wave
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int wave = threadIdx.x / warpSize, waves = kThreads / warpSize;
  __syncthreads();                                        // (the previous sum's reads of red)
  if (threadIdx.x % warpSize == 0) red[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < waves; ++w) total += red[w];
  return total;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void image_metrics_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ mask, int C, int H, int W, int tiles_x,
                                                                 int tiles, long long items, Window win, double c1, double c2,
                                                                 double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float LX[kHalo * kPitch];
  __shared__ __attribute__((aligned(16))) float LY[kHalo * kPitch];
  __shared__ float HM[5][kHalo * kTile];
  __shared__ double red[kThreads / 32];
  const size_t plane = (size_t)H * W;
  const int Ho = H - (kTaps - 1), Wo = W - (kTaps - 1);
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long p = item / tiles;                     // plane n * C + c
    const int tile = (int)(item - p * tiles);
    const int ti = tile / tiles_x, tj = tile - ti * tiles_x;
    const int i0 = ti * kTile, j0 = tj * kTile;
    __syncthreads();                                      // (the previous item's reads of LX / LY / HM)
    stage<VEC>(x + (size_t)p * plane, H, W, i0, j0, LX);
    stage<VEC>(y + (size_t)p * plane, H, W, i0, j0, LY);
    __syncthreads();

    // ---- pixel errors over the owner region ----
    const int own_r = (i0 + kTile >= Ho) ? H - i0 : kTile;              // (the last tile row: to the plane's edge, <= kHalo)
    const int own_c = (j0 + kTile >= Wo) ? W - j0 : kTile;
    const float* mrow = mask ? mask + (size_t)(p / C) * plane : nullptr;
    double sse = 0.0, sae = 0.0, msse = 0.0, msae = 0.0, mcnt = 0.0;
    for (int e = threadIdx.x; e < kHalo * kHalo; e += kThreads) {
      const int r = e / kHalo, c = e - r * kHalo;
      if (r < own_r && c < own_c) {
        const double d = (double)LX[r * kPitch + c] - (double)LY[r * kPitch + c];
        const double sq = d * d, ab = fabs(d);
        sse += sq;
        sae += ab;
        if (mrow && mrow[(size_t)(i0 + r) * W + (j0 + c)] != 0.f) {
          msse += sq;
          msae += ab;
          mcnt += 1.0;
        }
      }
    }

    // ---- horizontal pass: five maps, kHalo rows x kTile columns ----
    for (int e = threadIdx.x; e < kHalo * kTile; e += kThreads) {
      const int r = e / kTile, c = e - r * kTile;
      const float* lx = LX + r * kPitch + c;
      const float* ly = LY + r * kPitch + c;
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const double a = (double)lx[k], b = (double)ly[k], w = win.w[k];
        const double wa = w * a, wb = w * b;
        ax += wa;
        ay += wb;
        axx = fma(wa, a, axx);
        ayy = fma(wb, b, ayy);
        axy = fma(wa, b, axy);
      }
      HM[0][e] = (float)ax;
      HM[1][e] = (float)ay;
      HM[2][e] = (float)axx;
      HM[3][e] = (float)ayy;
      HM[4][e] = (float)axy;
    }
    __syncthreads();

    // ---- vertical pass and the formula: rows r0 .. r0 + 3 of column col ----
    const int col = (int)(threadIdx.x & (kTile - 1)), r0 = (int)(threadIdx.x / kTile) * 4;
    double acc[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
    for (int t = 0; t < kTaps + 3; ++t) {
      double v[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) v[m] = (double)HM[m][(r0 + t) * kTile + col];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = t - o;
        if (k >= 0 && k < kTaps) {
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[o][m] = fma(win.w[k], v[m], acc[o][m]);
        }
      }
    }
    double ssim = 0.0;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (i0 + r0 + o < Ho && j0 + col < Wo) {
        const double mx = acc[o][0], my = acc[o][1];
        const double vx = acc[o][2] - mx * mx, vy = acc[o][3] - my * my, cxy = acc[o][4] - mx * my;
        ssim += ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
      }
    }

    const double sums[kSums] = {sse, sae, msse, msae, mcnt, ssim};
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      const double total = block_sum(sums[k], red);
      if (threadIdx.x == 0) partial[item * kSums + k] = total;
    }
  }
}

// out[n][k] = sum over the image's C * tiles partials, thread-strided in ascending order and then over the threads in a fixed tree
__global__ __launch_bounds__(kThreads) void image_metrics_sum_kernel(const double* __restrict__ partial, long long per_image,
                                                                     double* __restrict__ out) {
  __shared__ double red[kThreads / 32];
  const double* base = partial + (size_t)blockIdx.x * per_image * kSums;
  for (int k = 0; k < kSums; ++k) {
    double v = 0.0;
    for (long long i = threadIdx.x; i < per_image; i += kThreads) v += base[i * kSums + k];
    const double total = block_sum(v, red);
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * kSums + k] = total;
  }
}

// counts: TP[K] | FP[K] | FN[K] | TN[K] | rows that match in every class.  MULTI: per class logit > 0 against target > 0.5;
// else the row's first argmax of the logits against that of the targets.
template <bool MULTI>
__global__ __launch_bounds__(kThreads) void clf_counts_kernel(const float* __restrict__ logits, const float* __restrict__ targets, int N,
                                                              int K, long long* __restrict__ counts) {
  __shared__ int s_pred[kThreads], s_tgt[kThreads];
  __shared__ int s_match[kThreads];
  int match = 0;
  for (int n0 = 0; n0 < N; n0 += kThreads) {
    const int n = n0 + (int)threadIdx.x;
    if (n < N) {
      const float* lg = logits + (size_t)n * K;
      const float* tg = targets + (size_t)n * K;
      if (MULTI) {
        bool same = true;
        for (int k = 0; k < K; ++k) same = same && ((lg[k] > 0.f) == (tg[k] > 0.5f));
        match += same;
      } else {
        int pi = 0, qi = 0;
        for (int k = 1; k < K; ++k) {
          if (lg[k] > lg[pi]) pi = k;
          if (tg[k] > tg[qi]) qi = k;
        }
        s_pred[threadIdx.x] = pi;
        s_tgt[threadIdx.x] = qi;
        match += pi == qi;
      }
    }
    __syncthreads();
    const int rows = N - n0 < kThreads ? N - n0 : kThreads;
    for (int k = threadIdx.x; k < K; k += kThreads) {
      long long tp = 0, fp = 0, fn = 0, tn = 0;
      for (int r = 0; r < rows; ++r) {
        bool pos, want;
        if (MULTI) {
          pos = logits[(size_t)(n0 + r) * K + k] > 0.f;
          want = targets[(size_t)(n0 + r) * K + k] > 0.5f;
        } else {
          pos = s_pred[r] == k;
          want = s_tgt[r] == k;
        }
        tp += pos && want;
        fp += pos && !want;
        fn += !pos && want;
        tn += !pos && !want;
      }
      counts[k] += tp;                                    // (class k's words belong to this thread alone)
      counts[K + k] += fp;
      counts[2 * K + k] += fn;
      counts[3 * K + k] += tn;
    }
    __syncthreads();
  }
  s_match[threadIdx.x] = match;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int t = 0; t < kThreads; ++t) total += s_match[t];
    counts[4 * (size_t)K] += total;
  }
}

inline int tiles_of(int extent) { return (extent - (kTaps - 1) + kTile - 1) / kTile; }

bool image_shape_ok(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H < kTaps || W < kTaps) return false;
  return (long long)N * C * H * W < (1ll << 40) && (long long)C * H * W < (1ll << 31);
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int64_t dei2i_image_metrics_ws_doubles(int N, int C, int H, int W) {
  if (!image_shape_ok(N, C, H, W)) return 0;
  return (int64_t)N * C * tiles_of(H) * tiles_of(W) * kSums;
}

extern "C" int dei2i_image_metrics(int N, int C, int H, int W, const float* x, const float* y, const float* mask, double data_range,
                                   double* ws, double* out, dei2i_stream s) {
  if (!image_shape_ok(N, C, H, W) || !x || !y || !ws || !out || !(data_range > 0.0)) return DEI2I_ERR_BAD_ARG;
  const int tiles_x = tiles_of(W), tiles = tiles_x * tiles_of(H);
  const long long items = (long long)N * C * tiles;
  const unsigned grid = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
  Window win;
  double total = 0.0;
  for (int k = 0; k < kTaps; ++k) {
    const double d = (double)(k - kTaps / 2);
    total += win.w[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
  }
  for (int k = 0; k < kTaps; ++k) win.w[k] /= total;
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
  if ((W % 4 == 0) && ((a | b) & 15) == 0)
    hipLaunchKernelGGL(image_metrics_kernel<true>, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, x, y, mask, C, H, W, tiles_x, tiles,
                       items, win, c1, c2, ws);
  else
    hipLaunchKernelGGL(image_metrics_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, x, y, mask, C, H, W, tiles_x, tiles,
                       items, win, c1, c2, ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(image_metrics_sum_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)s, ws, (long long)C * tiles, out);
  return (int)hipGetLastError();
}

extern "C" int dei2i_clf_counts(int N, int K, const float* logits, const float* targets, int kind, int64_t* counts, dei2i_stream s) {
  if (N <= 0 || K <= 0 || !logits || !targets || !counts || (long long)N * K >= (1ll << 31)) return DEI2I_ERR_BAD_ARG;
  if (kind != DEI2I_CLF_MULTI && kind != DEI2I_CLF_ARGMAX) return DEI2I_ERR_BAD_ARG;
  long long* out = reinterpret_cast<long long*>(counts);
  if (kind == DEI2I_CLF_MULTI)
    hipLaunchKernelGGL(clf_counts_kernel<true>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, logits, targets, N, K, out);
  else
    hipLaunchKernelGGL(clf_counts_kernel<false>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, logits, targets, N, K, out);
  return (int)hipGetLastError();
}
