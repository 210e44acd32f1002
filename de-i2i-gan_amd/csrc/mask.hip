// Device-drawn shifted patch masks of the MAE pre-training stage (utils/masks.py) and the mask-token fill (networks/architecture.py
// MaskToken) on fp32 NCHW images.
//
//   mask[n, i, j]      = keep[n, (i + rs) / patch, (j + cs) / patch]          (1 = pixel kept; keep: one byte per patch of the grid
//                                                                              GH x GW = (H / patch + 1) x (W / patch + 1))
//   filled[n, c, i, j] = mask ? imgs[n, c, i, j] : token[broadcast]
//
// dei2i_mask_draw fills (rs, cs) and keep on the device: Philox4x32-10 keyed by a seed, counted by (call, patch quad, global row),
// the call count one word of device memory that the launch itself advances (the pattern of dei2i_diffaug_draw) -- an eager step and
// a replay of a captured step draw the same mask, and every replay draws a new one.  The fill and its token gradient read the
// shifts from device memory for the same reason.  The token gradient sums over the batch in ascending order, one thread per element:
// no atomics, bit-reproducible.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"
#include "philox.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kShiftStream = 0xC0000000u;      // counter word c2 of the shifts
constexpr uint32_t kKeepStream = 0x80000000u;       // ... of patch quad q: kKeepStream | q  (q < 2^24; bit 31 is never set by diffaug.hip)

// One workgroup strides over the N x ceil(GH GW / 4) patch quads.  Every thread reads the call count, then thread 0 stores
// count + 1 behind the barrier: one launch, no atomics.  The only float arithmetic is unit_float's exact product and a compare.
__global__ __launch_bounds__(kThreads) void mask_draw_kernel(unsigned long long seed, unsigned long long* __restrict__ counter, int N,
                                                             unsigned row0, int P, int patch, float keep_prob, int* __restrict__ shift,
                                                             unsigned char* __restrict__ keep) {
  const unsigned long long call = *counter;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)call, c1 = (uint32_t)(call >> 32);
  if (threadIdx.x == 0) {
    const Philox4 x = philox4x32_10(c0, c1, kShiftStream, 0u, k0, k1);
    shift[0] = (int)__umulhi(x.x0, (uint32_t)patch);
    shift[1] = (int)__umulhi(x.x1, (uint32_t)patch);
  }
  const int Q = (P + 3) >> 2;
  const long long items = (long long)N * Q;
  for (long long k = threadIdx.x; k < items; k += kThreads) {
    const int n = (int)(k / Q), q = (int)(k - (long long)n * Q);
    const Philox4 x = philox4x32_10(c0, c1, kKeepStream | (uint32_t)q, row0 + (uint32_t)n, k0, k1);
    const uint32_t w[4] = {x.x0, x.x1, x.x2, x.x3};
    unsigned char* dst = keep + (size_t)n * P;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = 4 * q + e;
      if (t < P) dst[t] = unit_float(w[e]) < keep_prob ? 1 : 0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) *counter = call + 1;
}

struct TokenStrides {
  long long n, c, i, j;      // in elements; 0 on a broadcast dim
};

// the patch row / column of a pixel row / column: the shifts come from device memory, so the index is clamped to the grid
__device__ __forceinline__ int patch_of(int pos, int shift, int patch, int G) {
  const int g = (pos + shift) / patch;
  return g < 0 ? 0 : (g >= G ? G - 1 : g);
}

// each thread one quad of pixels along W (VEC) or one pixel, all channels; k runs over N x H x per_row
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mask_fill_kernel(int N, int C, int H, int W, int patch, int GH, int GW,
                                                             const int* __restrict__ shift, const unsigned char* __restrict__ keep,
                                                             const float* __restrict__ imgs, const float* __restrict__ token,
                                                             TokenStrides ts, float* __restrict__ filled, float* __restrict__ mask_out) {
  constexpr int L = VEC ? 4 : 1;
  const int per_row = VEC ? (W >> 2) : W;
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= (long long)N * H * per_row) return;
  const int j = (int)(k % per_row) * L;
  const long long rest = k / per_row;
  const int i = (int)(rest % H), n = (int)(rest / H);
  const int rs = shift[0], cs = shift[1];
  const unsigned char* krow = keep + ((size_t)n * GH + patch_of(i, rs, patch, GH)) * GW;
  bool kept[L];
#pragma unroll
  for (int e = 0; e < L; ++e) kept[e] = krow[patch_of(j + e, cs, patch, GW)] != 0;
  const size_t plane = (size_t)H * W, pix = (size_t)i * W + j;
  if (mask_out) {
    float* m = mask_out + (size_t)n * plane + pix;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(m) = make_float4(kept[0] ? 1.f : 0.f, kept[1] ? 1.f : 0.f, kept[2] ? 1.f : 0.f, kept[3] ? 1.f : 0.f);
    } else {
      m[0] = kept[0] ? 1.f : 0.f;
    }
  }
  for (int c = 0; c < C; ++c) {
    const size_t at = ((size_t)n * C + c) * plane + pix;
    float v[L];
    if constexpr (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(imgs + at);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = imgs[at];
    }
#pragma unroll
    for (int e = 0; e < L; ++e)
      if (!kept[e]) v[e] = token ? token[n * ts.n + c * ts.c + i * ts.i + (j + e) * ts.j] : 0.f;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(filled + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      filled[at] = v[0];
    }
  }
}

// grad_full[c, i, j] = sum over n (ascending) of the masked pixels' grad_out; k runs over C x H x per_row
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mask_fill_bwd_kernel(int N, int C, int H, int W, int patch, int GH, int GW,
                                                                 const int* __restrict__ shift, const unsigned char* __restrict__ keep,
                                                                 const float* __restrict__ grad_out, float* __restrict__ grad_full) {
  constexpr int L = VEC ? 4 : 1;
  const int per_row = VEC ? (W >> 2) : W;
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= (long long)C * H * per_row) return;
  const int j = (int)(k % per_row) * L;
  const long long rest = k / per_row;
  const int i = (int)(rest % H), c = (int)(rest / H);
  const int gi = patch_of(i, shift[0], patch, GH), cs = shift[1];
  int gj[L];
#pragma unroll
  for (int e = 0; e < L; ++e) gj[e] = patch_of(j + e, cs, patch, GW);
  const size_t plane = (size_t)H * W, pix = (size_t)i * W + j;
  float acc[L];
#pragma unroll
  for (int e = 0; e < L; ++e) acc[e] = 0.f;
  for (int n = 0; n < N; ++n) {
    const unsigned char* krow = keep + ((size_t)n * GH + gi) * GW;
    const size_t at = ((size_t)n * C + c) * plane + pix;
    float g[L];
    if constexpr (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(grad_out + at);
      g[0] = q.x; g[1] = q.y; g[2] = q.z; g[3] = q.w;
    } else {
      g[0] = grad_out[at];
    }
#pragma unroll
    for (int e = 0; e < L; ++e)
      if (krow[gj[e]] == 0) acc[e] += g[e];
  }
  float* dst = grad_full + (size_t)c * plane + pix;
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
    dst[0] = acc[0];
  }
}

// the shape gate of the two image kernels: sizes, a whole number of patches, the indices the kernels form in 64 bits
bool image_shape_ok(int N, int C, int H, int W, int patch) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || patch <= 0 || H % patch != 0 || W % patch != 0) return false;
  return (long long)N * C * H * W < (1ll << 40) && (long long)C * H * W < (1ll << 31) && (long long)N * H * W < (1ll << 38);
}

bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int dei2i_mask_draw(uint64_t seed, uint64_t* counter_dev, int N, int row0, int GH, int GW, int patch, float keep_prob,
                               int* shift_dev, unsigned char* keep_dev, dei2i_stream s) {
  if (!counter_dev || !shift_dev || !keep_dev || N <= 0 || row0 < 0 || GH <= 0 || GW <= 0 || patch <= 0) return DEI2I_ERR_BAD_ARG;
  if ((long long)row0 + N > (1ll << 31) || (long long)GH * GW >= (1ll << 26)) return DEI2I_ERR_BAD_ARG;
  if (!(keep_prob >= 0.f && keep_prob <= 1.f)) return DEI2I_ERR_BAD_ARG;          // (a NaN fails both)
  hipLaunchKernelGGL(mask_draw_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed,
                     reinterpret_cast<unsigned long long*>(counter_dev), N, (unsigned)row0, GH * GW, patch, keep_prob, shift_dev, keep_dev);
  return (int)hipGetLastError();
}

extern "C" int dei2i_mask_fill(int N, int C, int H, int W, int patch, const int* shift_dev, const unsigned char* keep_dev,
                               const float* imgs, const float* token, const int64_t* token_strides, float* filled, float* mask_out,
                               dei2i_stream s) {
  if (!shift_dev || !keep_dev || !imgs || !filled || (token && !token_strides) || !image_shape_ok(N, C, H, W, patch))
    return DEI2I_ERR_BAD_ARG;
  TokenStrides ts = {0, 0, 0, 0};
  if (token) {
    for (int d = 0; d < 4; ++d)
      if (token_strides[d] < 0) return DEI2I_ERR_BAD_ARG;
    ts = TokenStrides{token_strides[0], token_strides[1], token_strides[2], token_strides[3]};
  }
  const int GH = H / patch + 1, GW = W / patch + 1;
  const bool vec = W % 4 == 0 && aligned16(imgs, filled, mask_out);
  const long long items = (long long)N * H * (vec ? W / 4 : W);
  const dim3 grid((unsigned)((items + kThreads - 1) / kThreads));
  if (vec)
    hipLaunchKernelGGL(mask_fill_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)s, N, C, H, W, patch, GH, GW, shift_dev, keep_dev,
                       imgs, token, ts, filled, mask_out);
  else
    hipLaunchKernelGGL(mask_fill_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)s, N, C, H, W, patch, GH, GW, shift_dev, keep_dev,
                       imgs, token, ts, filled, mask_out);
  return (int)hipGetLastError();
}

extern "C" int dei2i_mask_fill_bwd(int N, int C, int H, int W, int patch, const int* shift_dev, const unsigned char* keep_dev,
                                   const float* grad_out, float* grad_full, dei2i_stream s) {
  if (!shift_dev || !keep_dev || !grad_out || !grad_full || !image_shape_ok(N, C, H, W, patch)) return DEI2I_ERR_BAD_ARG;
  const int GH = H / patch + 1, GW = W / patch + 1;
  const bool vec = W % 4 == 0 && aligned16(grad_out, grad_full);
  const long long items = (long long)C * H * (vec ? W / 4 : W);
  const dim3 grid((unsigned)((items + kThreads - 1) / kThreads));
  if (vec)
    hipLaunchKernelGGL(mask_fill_bwd_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)s, N, C, H, W, patch, GH, GW, shift_dev,
                       keep_dev, grad_out, grad_full);
  else
    hipLaunchKernelGGL(mask_fill_bwd_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)s, N, C, H, W, patch, GH, GW, shift_dev,
                       keep_dev, grad_out, grad_full);
  return (int)hipGetLastError();
}
