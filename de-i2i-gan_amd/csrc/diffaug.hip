// DiffAugment (utils/diffaug.py: color -> translation -> cutout) on fp32 NCHW images as ONE affine operator per sample and policy
// run, with its adjoint -- the op is differentiable to any order (ops._DiffAug / _DiffAugAdjoint).
//
//   y = Cut . Trans . (L x + beta),   L(x)[c] = a x[c] + b mean_c(x) + k mean_chw(x)
//   (a = kc ks, b = kc (1 - ks), k = 1 - kc; brightness beta, saturation ks, contrast kc: the contrast mean of the saturated image is
//   mean_chw(x) + beta).  L is self-adjoint, so the input gradient is L(h) with h = Trans^T (Cut g), and h is never written:
//   h[q] = g[q - t] where q - t is inside and not cut out.
//
// mode 0: forward with beta; mode 1: the forward's linear part (beta = 0: the adjoint's own gradient); mode 2: adjoint.
// One launch reduces each sample to <= 64 fixed-order partial sums (only when the run has color: mean_chw), a second applies the
// operator; the apply kernel sums the partials in a fixed order itself -- no atomics, bit-reproducible.
//
// dei2i_diffaug_draw fills the record table on the device: Philox4x32-10 keyed by a seed, counted by (call, run, global row), the
// call count one word of device memory that the launch itself advances -- an eager step and a replay of a captured step draw the
// same parameters, and every replay draws new ones.  dei2i_diffaug_draw_p is the same draw with a gate per row and policy: each
// policy applies with a probability read from device memory (adaptive discriminator augmentation; its controller: ada.hip).
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"
#include "philox.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunks = 64;

__device__ __forceinline__ bool in_hole(const dei2i_diffaug_rec& r, int i, int j, int ch, int cw) {
  return i >= r.top && i < r.top + ch && j >= r.left && j < r.left + cw;
}

// output pixel (i, j) of the forward takes a value: its source (i + ty, j + tx) is inside and (i, j) is not cut out
__device__ __forceinline__ bool fwd_valid(const dei2i_diffaug_rec& r, int i, int j, int H, int W, int ch, int cw) {
  const int si = i + r.ty, sj = j + r.tx;
  return si >= 0 && si < H && sj >= 0 && sj < W && !in_hole(r, i, j, ch, cw);
}

// grid (chunks, N): partial[n][chunk] = sum over rows [chunk*rpc, +rpc) of src (masked: times fwd_valid -- the sum of h = Trans^T Cut g)
__global__ __launch_bounds__(kThreads) void diffaug_reduce_kernel(const float* __restrict__ src, const dei2i_diffaug_rec* __restrict__ tab,
                                                                  int C, int H, int W, int ch, int cw, int rpc, int masked, int vec,
                                                                  float* __restrict__ partial) {
  __shared__ float lds[kThreads / 64];
  const int n = blockIdx.y, chunk = blockIdx.x;
  const dei2i_diffaug_rec r = tab[n];
  const int r0 = chunk * rpc, R = min(H, r0 + rpc) - r0;
  const float* img = src + (size_t)n * C * H * W;
  float acc = 0.f;
  if (vec) {
    const int W4 = W >> 2, items = C * R * W4;
    for (int k = threadIdx.x; k < items; k += kThreads) {
      const int j = (k % W4) * 4, rest = k / W4, i = r0 + rest % R, c = rest / R;
      const float4 v = *reinterpret_cast<const float4*>(img + ((size_t)c * H + i) * W + j);
      if (!masked) {
        acc += (v.x + v.y) + (v.z + v.w);
      } else {
        acc += ((fwd_valid(r, i, j, H, W, ch, cw) ? v.x : 0.f) + (fwd_valid(r, i, j + 1, H, W, ch, cw) ? v.y : 0.f)) +
               ((fwd_valid(r, i, j + 2, H, W, ch, cw) ? v.z : 0.f) + (fwd_valid(r, i, j + 3, H, W, ch, cw) ? v.w : 0.f));
      }
    }
  } else {
    const int items = C * R * W;
    for (int k = threadIdx.x; k < items; k += kThreads) {
      const int j = k % W, rest = k / W, i = r0 + rest % R, c = rest / R;
      const float v = img[((size_t)c * H + i) * W + j];
      acc += (!masked || fwd_valid(r, i, j, H, W, ch, cw)) ? v : 0.f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[n * gridDim.x + chunk] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// the masked source quad of a row: float4 when all four are taken and the address is 16-byte aligned, else per element
__device__ __forceinline__ float4 load_quad(const float* row, int sj, int mask, bool fast) {
  if (fast) return *reinterpret_cast<const float4*>(row + sj);
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (mask & 1) q.x = row[sj];
  if (mask & 2) q.y = row[sj + 1];
  if (mask & 4) q.z = row[sj + 2];
  if (mask & 8) q.w = row[sj + 3];
  return q;
}

// grid (ceil(H * W/4 or H * W, 256), N): each thread one quad of output pixels along W (vec) or one pixel, all channels
__global__ __launch_bounds__(kThreads) void diffaug_apply_kernel(const float* __restrict__ src, const dei2i_diffaug_rec* __restrict__ tab,
                                                                 const float* __restrict__ partial, int chunks, int C, int H, int W,
                                                                 int ch, int cw, int mode, int color, int vec, float* __restrict__ dst) {
  __shared__ float s_mean;
  const int n = blockIdx.y;
  const dei2i_diffaug_rec r = tab[n];
  const bool adj = mode == 2;
  float M = 0.f;
  if (color) {
    if (threadIdx.x < 64) {
      float v = (int)threadIdx.x < chunks ? partial[n * chunks + threadIdx.x] : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
      if (threadIdx.x == 0) s_mean = v / (float)(C * H * W);
    }
    __syncthreads();
    M = s_mean;
  }
  const float base = r.k * M + (mode == 0 ? r.beta : 0.f);
  const float off = adj ? base : 0.f;          // value of a pixel whose source is masked: L(0) + mean term (adjoint), 0 (forward)
  const float invC = 1.f / (float)C;
  const int sy = adj ? -r.ty : r.ty, sx = adj ? -r.tx : r.tx;
  const size_t plane = (size_t)H * W;
  const float* img = src + (size_t)n * C * plane;
  float* out = dst + (size_t)n * C * plane;
  const int per_row = vec ? (W >> 2) : W;
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= H * per_row) return;
  const int i = k / per_row, j = (k % per_row) * (vec ? 4 : 1);
  const int si = i + sy;
  const bool row_in = si >= 0 && si < H;
  const int lanes = vec ? 4 : 1;
  int mask = 0;
  for (int e = 0; e < lanes; ++e) {
    const int sj = j + e + sx;
    if (row_in && sj >= 0 && sj < W && !(adj ? in_hole(r, si, sj, ch, cw) : in_hole(r, i, j + e, ch, cw))) mask |= 1 << e;
  }
  if (vec) {
    const bool fast = mask == 15 && (sx & 3) == 0;
    float4 mc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mask) {
      for (int c = 0; c < C; ++c) {
        const float4 q = load_quad(img + c * plane + (size_t)si * W, j + sx, mask, fast);
        mc.x += q.x; mc.y += q.y; mc.z += q.z; mc.w += q.w;
      }
      mc.x *= invC; mc.y *= invC; mc.z *= invC; mc.w *= invC;
    }
    for (int c = 0; c < C; ++c) {
      float4 o = make_float4(off, off, off, off);
      if (mask) {
        const float4 q = load_quad(img + c * plane + (size_t)si * W, j + sx, mask, fast);
        if (mask & 1) o.x = r.a * q.x + r.b * mc.x + base;
        if (mask & 2) o.y = r.a * q.y + r.b * mc.y + base;
        if (mask & 4) o.z = r.a * q.z + r.b * mc.z + base;
        if (mask & 8) o.w = r.a * q.w + r.b * mc.w + base;
      }
      *reinterpret_cast<float4*>(out + c * plane + (size_t)i * W + j) = o;
    }
  } else {
    const size_t s_off = mask ? (size_t)si * W + (j + sx) : 0;
    float mc = 0.f;
    if (mask) {
      for (int c = 0; c < C; ++c) mc += img[c * plane + s_off];
      mc *= invC;
    }
    for (int c = 0; c < C; ++c)
      out[c * plane + (size_t)i * W + j] = mask ? r.a * img[c * plane + s_off] + r.b * mc + base : off;
  }
}

// ---- device-drawn records (Philox4x32-10 and unit_float: philox.h) ----------------------------------------------------
// what the host works out once per call: the integer ranges of utils.diffaug.draw_params
struct DrawGeom {
  int max_y, max_x;          // translation: ty in [-max_y, max_y], tx in [-max_x, max_x]
  int range_cy, range_cx;    // cutout centre: cy in [0, range_cy), cx in [0, range_cx)
  int half_ch, half_cw;      // top = cy - half_ch, left = cx - half_cw
  int H, W;                  // (GATED) the cut window of a row whose cutout gate is off starts at (H, W): off the image
};

// One workgroup strides over the runs x N records.  flags: 3 bits per run (DEI2I_DIFFAUG_COLOR / _TRANSLATION / _CUTOUT).  Every
// thread reads the call count, then thread 0 stores count + 1 behind the barrier: one launch, no atomics.  Contraction is off:
// the arithmetic has no multiply-add, so a numpy reference reproduces the table bit for bit.
// GATED (dei2i_diffaug_draw_p): a third Philox block, run | 2 << 16, gives one gate per policy (x0 color, x1 translation, x2
// cutout); a policy of the run applies to the row iff unit_float(x) < *p_dev, else its fields go back to the identity.  The
// parameter blocks are drawn as without gates, so a row's parameters do not depend on its gates and p = 1 is the ungated table.
template <bool GATED>
__global__ __launch_bounds__(kThreads) void diffaug_draw_kernel(unsigned long long seed, unsigned long long* __restrict__ counter,
                                                                int runs, unsigned long long flags, int N, unsigned row0,
                                                                DrawGeom g, const float* __restrict__ p_dev,
                                                                dei2i_diffaug_rec* __restrict__ tab) {
#pragma clang fp contract(off)
  const unsigned long long call = *counter;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)call, c1 = (uint32_t)(call >> 32);
  float p = 1.f;
  if (GATED) p = *p_dev;
  for (int i = threadIdx.x; i < runs * N; i += kThreads) {
    const int run = i / N, n = i - run * N;
    const unsigned f = (unsigned)(flags >> (3 * run)) & 7u;
    const uint32_t row = row0 + (uint32_t)n;
    dei2i_diffaug_rec r = {1.f, 0.f, 0.f, 0.f, 0, 0, 0, 0};
    if (f & DEI2I_DIFFAUG_COLOR) {
      const Philox4 x = philox4x32_10(c0, c1, (uint32_t)run, row, k0, k1);
      const float rb = unit_float(x.x0), rs = unit_float(x.x1), rc = unit_float(x.x2);
      const float ks = 2.f * rs, kc = rc + 0.5f;
      r.a = kc * ks;
      r.b = kc * (1.f - ks);
      r.k = 1.f - kc;
      r.beta = rb - 0.5f;
    }
    if (f & (DEI2I_DIFFAUG_TRANSLATION | DEI2I_DIFFAUG_CUTOUT)) {
      const Philox4 x = philox4x32_10(c0, c1, (uint32_t)run | (1u << 16), row, k0, k1);
      if (f & DEI2I_DIFFAUG_TRANSLATION) {
        r.ty = -g.max_y + (int)__umulhi(x.x0, (uint32_t)(2 * g.max_y + 1));
        r.tx = -g.max_x + (int)__umulhi(x.x1, (uint32_t)(2 * g.max_x + 1));
      }
      if (f & DEI2I_DIFFAUG_CUTOUT) {
        r.top = (int)__umulhi(x.x2, (uint32_t)g.range_cy) - g.half_ch;
        r.left = (int)__umulhi(x.x3, (uint32_t)g.range_cx) - g.half_cw;
      }
    }
    if (GATED) {
      const Philox4 x = philox4x32_10(c0, c1, (uint32_t)run | (2u << 16), row, k0, k1);
      if ((f & DEI2I_DIFFAUG_COLOR) && !(unit_float(x.x0) < p)) {
        r.a = 1.f;
        r.b = r.k = r.beta = 0.f;
      }
      if ((f & DEI2I_DIFFAUG_TRANSLATION) && !(unit_float(x.x1) < p)) r.ty = r.tx = 0;
      if ((f & DEI2I_DIFFAUG_CUTOUT) && !(unit_float(x.x2) < p)) {
        r.top = g.H;          // rows [H, H + ch) x cols [W, W + cw): no pixel of the image (in_hole is false in every mode)
        r.left = g.W;
      }
    }
    tab[i] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) *counter = call + 1;
}

void chunking(int N, int H, int* rpc, int* chunks) {
  int want = (1024 + N - 1) / N;               // ~4 blocks per CU over the batch
  want = want < 1 ? 1 : (want > kMaxChunks ? kMaxChunks : want);
  if (want > H) want = H;
  *rpc = (H + want - 1) / want;
  *chunks = (H + *rpc - 1) / *rpc;
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" size_t dei2i_diffaug_partial_floats(int N) { return (size_t)(N > 0 ? N : 0) * kMaxChunks; }

extern "C" int dei2i_diffaug(int mode, int N, int C, int H, int W, int ch, int cw, int color, const float* src,
                             const dei2i_diffaug_rec* tab, float* partial, float* dst, dei2i_stream s) {
  if (mode < 0 || mode > 2 || N <= 0 || C <= 0 || H <= 0 || W <= 0 || ch < 0 || cw < 0 || !src || !tab || !dst || (color && !partial))
    return DEI2I_ERR_BAD_ARG;
  if ((long long)N * C * H * W >= (1ll << 40) || (long long)C * H * W >= (1ll << 31)) return DEI2I_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)s;
  const int vec = (W % 4 == 0) && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  int rpc = H, chunks = 1;
  if (color) {
    chunking(N, H, &rpc, &chunks);
    hipLaunchKernelGGL(diffaug_reduce_kernel, dim3((unsigned)chunks, (unsigned)N), dim3(kThreads), 0, st, src, tab, C, H, W, ch, cw, rpc,
                       mode == 2 ? 1 : 0, vec, partial);
  }
  const long long items = (long long)H * (vec ? W / 4 : W);
  hipLaunchKernelGGL(diffaug_apply_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads), (unsigned)N), dim3(kThreads), 0, st, src,
                     tab, partial, chunks, C, H, W, ch, cw, mode, color, vec, dst);
  return (int)hipGetLastError();
}

// both draws: p_dev null = dei2i_diffaug_draw (no gate block), else dei2i_diffaug_draw_p
static int draw_launch(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int H, int W,
                       const float* p_dev, dei2i_diffaug_rec* tab, dei2i_stream s) {
  if (!counter_dev || !tab || runs <= 0 || runs > DEI2I_DIFFAUG_MAX_RUNS || N <= 0 || row0 < 0 || H <= 0 || W <= 0) return DEI2I_ERR_BAD_ARG;
  if ((long long)row0 + N > (1ll << 31) || (long long)runs * N >= (1ll << 24) || H > (1 << 24) || W > (1 << 24)) return DEI2I_ERR_BAD_ARG;
  if ((run_flags >> (3 * runs)) != 0) return DEI2I_ERR_BAD_ARG;
  for (int r = 0; r < runs; ++r)
    if (((run_flags >> (3 * r)) & 7u) == 0) return DEI2I_ERR_BAD_ARG;          // (a run holds at least one policy)
  const int ch = (int)(H * 0.5 + 0.5), cw = (int)(W * 0.5 + 0.5);
  DrawGeom g;
  g.max_y = (int)(H * 0.125 + 0.5);
  g.max_x = (int)(W * 0.125 + 0.5);
  g.range_cy = H + (1 - ch % 2);
  g.range_cx = W + (1 - cw % 2);
  g.half_ch = ch / 2;
  g.half_cw = cw / 2;
  g.H = H;
  g.W = W;
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(counter_dev);
  if (p_dev)
    hipLaunchKernelGGL(diffaug_draw_kernel<true>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, N, (unsigned)row0, g, p_dev, tab);
  else
    hipLaunchKernelGGL(diffaug_draw_kernel<false>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, N, (unsigned)row0, g, p_dev, tab);
  return (int)hipGetLastError();
}

extern "C" int dei2i_diffaug_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int H, int W,
                                  dei2i_diffaug_rec* tab, dei2i_stream s) {
  return draw_launch(seed, counter_dev, runs, run_flags, N, row0, H, W, nullptr, tab, s);
}

extern "C" int dei2i_diffaug_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int H, int W,
                                    const float* p_dev, dei2i_diffaug_rec* tab, dei2i_stream s) {
  if (!p_dev) return DEI2I_ERR_BAD_ARG;
  return draw_launch(seed, counter_dev, runs, run_flags, N, row0, H, W, p_dev, tab, s);
}
