// Fused multi-tensor Adam / AdamW: one launch updates every parameter tensor of a network.
// torch.optim.Adam single-tensor semantics (no amsgrad), reference call site trainers/base_trainer.py:75-89
// (Adam betas (0.5, 0.999); AdamW betas (0.9, 0.95) with torch's default decoupled weight decay 1e-2 for the MAE stage):
//   p *= 1 - lr*wd  (AdamW only: keep = 1 - lr*wd, 1 for Adam)
//   g = g*grad_scale + wd*p  (COUPLED: torch.optim.Adam's weight_decay, stargan-v2 core/solver.py:52-56; p.grad is not written)
//   m += (1-b1)(g-m); v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// Global-norm clipping (torch.nn.utils.clip_grad_norm_, L2) rides on grad_scale: grad_sumsq_kernel + grad_clip_finalize_kernel leave
// grad_scale * min(1, max_norm / (|g * grad_scale| + 1e-6)) in device memory, where the CLIP form of adam_kernel reads it.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"

namespace dei2i {

// One element's update, shared by the float4 loop and the scalar loop of adam_kernel so that an element gets the same bits
// whichever loop reaches it (the tail of a tensor, a tensor that is not 16-byte aligned).  Left to the compiler, the two loops
// were contracted into different fused multiply-adds; here every rounding is written out and contraction is off.
template <bool COUPLED>
DEI2I_D void adam_update(float& p, const float g, float& m, float& v, const float one_minus_b1, const float beta2,
                         const float one_minus_b2, const float eps, const float inv_c2, const float step_size,
                         const float grad_scale, const float keep, const float wd) {
#pragma clang fp contract(off)
  const float gv = COUPLED ? fmaf(g, grad_scale, wd * p) : g * grad_scale;
  m = fmaf(one_minus_b1, COUPLED ? gv - m : fmaf(g, grad_scale, -m), m);
  v = COUPLED ? fmaf(beta2, v, gv * (one_minus_b2 * gv)) : fmaf(gv, one_minus_b2 * gv, beta2 * v);
  const float denom = fmaf(sqrtf(v), inv_c2, eps);
  p = fmaf(p, keep, -(step_size * (m / denom)));
}

// DEV: (lr, bias_c1, bias_c2_sqrt, keep) are row `*index` of the device array `hyper` (`rows` rows of 4 floats) instead of the
// kernel arguments of the same names -- what a captured graph replays with per-step values; the rest of the math is shared.
// CLIP: grad_scale is `*scale` (what grad_clip_finalize_kernel left) instead of the kernel argument.
template <bool COUPLED, bool DEV, bool CLIP>
__global__ __launch_bounds__(256) void adam_kernel(const dei2i_adam_rec* __restrict__ table, float lr, float beta1,
                                                   float beta2, float eps, float bias_c1, float bias_c2_sqrt,
                                                   float grad_scale, float keep, float wd, const float* __restrict__ hyper,
                                                   const int* __restrict__ index, int rows, const float* __restrict__ scale) {
  const dei2i_adam_rec rec = table[blockIdx.y];
  if (CLIP) grad_scale = *scale;
  if (DEV) {
    const int r = *index;
    if (r < 0 || r >= rows) return;          // (the host refreshes the rows before the index can reach their end)
    lr = hyper[4 * r];
    bias_c1 = hyper[4 * r + 1];
    bias_c2_sqrt = hyper[4 * r + 2];
    if (!COUPLED) keep = hyper[4 * r + 3];
  }
  const float step_size = lr / bias_c1;
  const float inv_c2 = 1.f / bias_c2_sqrt;
  const float a1 = 1.f - beta1, a2 = 1.f - beta2;
  const int64_t n = rec.n;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(rec.p) | reinterpret_cast<uintptr_t>(rec.g) |
                       reinterpret_cast<uintptr_t>(rec.m) | reinterpret_cast<uintptr_t>(rec.v)) & 15) == 0 ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 p = reinterpret_cast<float4*>(rec.p)[i];
    const float4 g = reinterpret_cast<const float4*>(rec.g)[i];
    float4 m = reinterpret_cast<float4*>(rec.m)[i];
    float4 v = reinterpret_cast<float4*>(rec.v)[i];
    float* pp = &p.x; const float* gp = &g.x; float* mp = &m.x; float* vp = &v.x;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      adam_update<COUPLED>(pp[e], gp[e], mp[e], vp[e], a1, beta2, a2, eps, inv_c2, step_size, grad_scale, keep, wd);
    reinterpret_cast<float4*>(rec.p)[i] = p;
    reinterpret_cast<float4*>(rec.m)[i] = m;
    reinterpret_cast<float4*>(rec.v)[i] = v;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float p = rec.p[i], m = rec.m[i], v = rec.v[i];
    adam_update<COUPLED>(p, rec.g[i], m, v, a1, beta2, a2, eps, inv_c2, step_size, grad_scale, keep, wd);
    rec.m[i] = m;
    rec.v[i] = v;
    rec.p[i] = p;
  }
}

// Sum of g^2 over every tensor of the table, the first half of the global gradient norm: workgroup (x, y) sums its grid-stride
// share of row y in fp32 -- one fmaf per element in either loop, so an element contributes the same bits whichever loop reaches
// it -- then the 64 lanes by shuffle and the four waves through LDS, in a fixed order.  Every workgroup stores its partial (0
// when it had no element): nothing is cleared beforehand, nothing is atomic, the same inputs give the same bits.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const dei2i_adam_rec* __restrict__ table, float* __restrict__ partial) {
  const dei2i_adam_rec rec = table[blockIdx.y];
  const int64_t n = rec.n;
  const int64_t n4 = (reinterpret_cast<uintptr_t>(rec.g) & 15) == 0 ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 g = reinterpret_cast<const float4*>(rec.g)[i];
    acc = fmaf(g.x, g.x, acc);
    acc = fmaf(g.y, g.y, acc);
    acc = fmaf(g.z, g.z, acc);
    acc = fmaf(g.w, g.w, acc);
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float g = rec.g[i];
    acc = fmaf(g, g, acc);
  }
  acc = wave_sum(acc);
  __shared__ float waves[4];
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

// The second half, one workgroup: S = the sum of the partials in double (thread t adds t, t + 256, ..., then a fixed LDS tree);
// out[0] = sqrt(S) * grad_scale, the norm of the gradients the optimizer applies; out[1] = grad_scale * min(1, max_norm /
// (out[0] + 1e-6)) in float, clip_grad_norm_'s arithmetic (a NaN stays NaN, as torch.clamp(max=1) leaves it).
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const float* __restrict__ partial, int n, float grad_scale,
                                                                 float max_norm, float* __restrict__ out) {
  __shared__ double tree[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
  tree[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) tree[threadIdx.x] += tree[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)(sqrt(tree[0]) * (double)grad_scale);
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
    out[0] = norm;
    out[1] = grad_scale * coef;
  }
}

// ---- state digest: every 32-bit word of a list of tensors reduced to one 64-bit word, in integers mod 2^64 ----
//   digest = sum_k sum_i splitmix64(splitmix64((k << 32) | i) + w[k][i])      (k: the tensor's place in the list, i: the word's in it)
// A sum of integers: any order of the additions gives the same bits, so the grid, the two loops and the tree below are free.
DEI2I_D uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The sum of 256 threads' words through LDS; the result is valid in thread 0.
DEI2I_D uint64_t block_sum_u64(uint64_t v, uint64_t* tree) {
  tree[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) tree[threadIdx.x] += tree[threadIdx.x + o];
    __syncthreads();
  }
  return tree[0];
}

// Workgroup (x, y) hashes its grid-stride share of row y's rec.n words at rec.p (only these two fields are read): 16 bytes a lane
// where the row is 16-byte aligned, word by word otherwise and for the tail.  Like grad_sumsq_kernel every workgroup stores its
// partial (0 when it had no word): nothing is cleared beforehand, nothing is atomic.
__global__ __launch_bounds__(256) void state_digest_kernel(const dei2i_adam_rec* __restrict__ table, uint32_t row0,
                                                           uint64_t* __restrict__ partial) {
  __shared__ uint64_t tree[256];
  const dei2i_adam_rec rec = table[blockIdx.y];
  const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(rec.p);
  const uint64_t hi = (uint64_t)(row0 + blockIdx.y) << 32;
  const int64_t n = rec.n;
  const int64_t n4 = (reinterpret_cast<uintptr_t>(w) & 15) == 0 ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(w)[i];
    const uint64_t at = hi | (uint64_t)(4 * i);
    acc += splitmix64(splitmix64(at) + v.x);
    acc += splitmix64(splitmix64(at + 1) + v.y);
    acc += splitmix64(splitmix64(at + 2) + v.z);
    acc += splitmix64(splitmix64(at + 3) + v.w);
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    acc += splitmix64(splitmix64(hi | (uint64_t)i) + w[i]);
  acc = block_sum_u64(acc, tree);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

// One workgroup: out[0] = (accumulate ? out[0] : 0) + the sum of the n partials.
__global__ __launch_bounds__(256) void state_digest_finalize_kernel(const uint64_t* __restrict__ partial, int n, int accumulate,
                                                                    uint64_t* __restrict__ out) {
  __shared__ uint64_t tree[256];
  uint64_t s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = block_sum_u64(s, tree);
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0) + s;
}

// torch.optim.SGD / torch.optim.RMSprop with the defaults the reference constructs them with (trainers/base_trainer.py:71-74: only
// lr is passed -- no momentum, no weight decay, RMSprop alpha 0.99, eps 1e-8, not centered), same pointer table (RMSprop's
// square average lives in rec.m; rec.v is not touched):
//   kind 0  p -= lr * g                       kind 1  sq = alpha sq + (1 - alpha) g^2;  p -= lr * g / (sqrt(sq) + eps)
__global__ __launch_bounds__(256) void sgd_rmsprop_kernel(const dei2i_adam_rec* __restrict__ table, int kind, float lr, float alpha,
                                                          float eps, float grad_scale) {
  const dei2i_adam_rec rec = table[blockIdx.y];
  const int64_t n = rec.n, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gv = rec.g[i] * grad_scale;
    if (kind == 0) {
      rec.p[i] -= lr * gv;
    } else {
      const float sq = alpha * rec.m[i] + (1.f - alpha) * gv * gv;
      rec.m[i] = sq;
      rec.p[i] -= lr * (gv / (sqrtf(sq) + eps));
    }
  }
}

// stargan-v2's EMA (core/solver.py:549-551: param_test = torch.lerp(param, param_test, beta)) over every tensor of a network in
// place: rec.p = param_test (lerp end), rec.g = param (lerp start).  torch.lerp's formula: start + w (end - start) for |w| < 0.5,
// end - (end - start)(1 - w) otherwise.  One element, shared by both forms of the kernel so that they give the same bits.
DEI2I_D float ema_update(const float start, const float end, const float w, const bool hi) {
  const float diff = end - start;
  return hi ? end - diff * (1.f - w) : start + w * diff;
}

// DEV: w is row `*index` of the device array `weights` (`rows` floats) instead of the kernel argument -- what a captured graph
// replays with a weight that changes from one update to the next (the delayed start of the defectGAN / MAE trainers' EMA).
template <bool DEV>
__global__ __launch_bounds__(256) void ema_lerp_kernel(const dei2i_adam_rec* __restrict__ table, float w,
                                                       const float* __restrict__ weights, const int* __restrict__ index, int rows) {
  const dei2i_adam_rec rec = table[blockIdx.y];
  if (DEV) {
    const int r = *index;
    if (r < 0 || r >= rows) return;          // (the host refreshes the rows before the index can reach their end)
    w = weights[r];
  }
  const int64_t n = rec.n, stride = (int64_t)gridDim.x * blockDim.x;
  const bool hi = fabsf(w) >= 0.5f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    rec.p[i] = ema_update(rec.g[i], rec.p[i], w, hi);
}

}  // namespace dei2i

using namespace dei2i;

// The grid of a multi-tensor launch: y = the table's rows; x = 256-thread workgroups for the longest tensor at `per_thread`
// elements a thread, between 1 and `cap` (the kernels stride over what is left).
static dim3 table_grid(int64_t max_n, int per_thread, int64_t cap, int count) {
  int64_t bx = (max_n / per_thread + 255) / 256;
  if (bx < 1) bx = 1;
  if (bx > cap) bx = cap;
  return dim3((unsigned)bx, (unsigned)count);
}

// The one launch of adam_kernel: the runtime triple (coupled, dev, clip) picks the instance.  A DEV launch needs the rows and their
// index, a CLIP launch the scale; what a form does not read is whatever its entry point passes for it.
static int adam_dispatch(bool coupled, bool dev, bool clip, const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr,
                         float beta1, float beta2, float eps, float bias_c1, float bias_c2_sqrt, float grad_scale, float keep, float wd,
                         const float* hyper_dev, const int* index_dev, int rows, const float* scale_dev, dei2i_stream s) {
  if (!table_dev || count <= 0 || max_n <= 0 || (dev && (!hyper_dev || !index_dev || rows <= 0)) || (clip && !scale_dev))
    return DEI2I_ERR_BAD_ARG;
  static constexpr decltype(&adam_kernel<false, false, false>) kernels[8] = {
      adam_kernel<false, false, false>, adam_kernel<false, false, true>, adam_kernel<false, true, false>, adam_kernel<false, true, true>,
      adam_kernel<true, false, false>,  adam_kernel<true, false, true>,  adam_kernel<true, true, false>,  adam_kernel<true, true, true>};
  hipLaunchKernelGGL(kernels[4 * coupled + 2 * dev + clip], table_grid(max_n, 4, 512, count), dim3(256), 0, (hipStream_t)s, table_dev,
                     lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt, grad_scale, keep, wd, hyper_dev, index_dev, rows, scale_dev);
  return (int)hipGetLastError();
}

extern "C" int dei2i_sgd_rmsprop_step(const dei2i_adam_rec* table_dev, int count, int64_t max_n, int kind, float lr, float alpha,
                                      float eps, float grad_scale, dei2i_stream s) {
  if (!table_dev || count <= 0 || max_n <= 0 || (kind != 0 && kind != 1)) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(sgd_rmsprop_kernel, table_grid(max_n, 1, 2048, count), dim3(256), 0, (hipStream_t)s, table_dev, kind, lr, alpha,
                     eps, grad_scale);
  return (int)hipGetLastError();
}

// (lr, the bias corrections and `keep` as arguments; decoupled: p *= 1 - lr * decoupled_decay, _l2: g += weight_decay * p)
extern "C" int dei2i_adam_step(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2,
                               float eps, float bias_c1, float bias_c2_sqrt, float grad_scale, float decoupled_decay,
                               dei2i_stream s) {
  return adam_dispatch(false, false, false, table_dev, count, max_n, lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt, grad_scale,
                       1.f - lr * decoupled_decay, 0.f, nullptr, nullptr, 0, nullptr, s);
}

extern "C" int dei2i_adam_step_l2(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2,
                                  float eps, float bias_c1, float bias_c2_sqrt, float grad_scale, float weight_decay, dei2i_stream s) {
  return adam_dispatch(true, false, false, table_dev, count, max_n, lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt, grad_scale, 1.f,
                       weight_decay, nullptr, nullptr, 0, nullptr, s);
}

// (the _dev forms: lr, the bias corrections and `keep` come from `hyper_dev`; the kernel arguments of those names are not read)
extern "C" int dei2i_adam_step_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev,
                                   const int* index_dev, int rows, float beta1, float beta2, float eps, float grad_scale,
                                   dei2i_stream s) {
  return adam_dispatch(false, true, false, table_dev, count, max_n, 0.f, beta1, beta2, eps, 1.f, 1.f, grad_scale, 1.f, 0.f, hyper_dev,
                       index_dev, rows, nullptr, s);
}

extern "C" int dei2i_adam_step_l2_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev,
                                      const int* index_dev, int rows, float beta1, float beta2, float eps, float grad_scale,
                                      float weight_decay, dei2i_stream s) {
  return adam_dispatch(true, true, false, table_dev, count, max_n, 0.f, beta1, beta2, eps, 1.f, 1.f, grad_scale, 1.f, weight_decay,
                       hyper_dev, index_dev, rows, nullptr, s);
}

// (the _clip forms: grad_scale comes from *scale_dev, where dei2i_grad_clip_finalize left it; `coupled` selects the _l2 update)
extern "C" int dei2i_adam_step_clip(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float lr, float beta1, float beta2,
                                    float eps, float bias_c1, float bias_c2_sqrt, const float* scale_dev, int coupled,
                                    float weight_decay, dei2i_stream s) {
  return adam_dispatch(coupled != 0, false, true, table_dev, count, max_n, lr, beta1, beta2, eps, bias_c1, bias_c2_sqrt, 1.f,
                       coupled ? 1.f : 1.f - lr * weight_decay, coupled ? weight_decay : 0.f, nullptr, nullptr, 0, scale_dev, s);
}

extern "C" int dei2i_adam_step_clip_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* hyper_dev,
                                        const int* index_dev, int rows, float beta1, float beta2, float eps,
                                        const float* scale_dev, int coupled, float weight_decay, dei2i_stream s) {
  return adam_dispatch(coupled != 0, true, true, table_dev, count, max_n, 0.f, beta1, beta2, eps, 1.f, 1.f, 1.f, 1.f,
                       coupled ? weight_decay : 0.f, hyper_dev, index_dev, rows, scale_dev, s);
}

extern "C" int dei2i_grad_sumsq_blocks(int64_t max_n) { return (int)table_grid(max_n, 4, 512, 1).x; }

extern "C" int dei2i_grad_sumsq(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float* partial_dev, dei2i_stream s) {
  if (!table_dev || count <= 0 || max_n <= 0 || !partial_dev) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_sumsq_kernel, table_grid(max_n, 4, 512, count), dim3(256), 0, (hipStream_t)s, table_dev, partial_dev);
  return (int)hipGetLastError();
}

extern "C" int dei2i_grad_clip_finalize(const float* partial_dev, int n_partials, float grad_scale, float max_norm, float* out_dev,
                                        dei2i_stream s) {
  if (!partial_dev || n_partials <= 0 || !(max_norm > 0.f) || !out_dev) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial_dev, n_partials, grad_scale, max_norm,
                     out_dev);
  return (int)hipGetLastError();
}

extern "C" int dei2i_state_digest_blocks(int64_t max_n) { return (int)table_grid(max_n, 4, 512, 1).x; }

extern "C" int dei2i_state_digest(const dei2i_adam_rec* table_dev, int count, int64_t max_n, int64_t row0, uint64_t* partial_dev,
                                  int accumulate, uint64_t* out_dev, dei2i_stream s) {
  // (a word's index and a row's place share one 64-bit key: 32 bits each)
  if (!table_dev || count <= 0 || count > DEI2I_DIGEST_MAX_ROWS || max_n <= 0 || max_n > ((int64_t)1 << 32) || row0 < 0 || row0 + count > ((int64_t)1 << 32) ||
      !partial_dev || !out_dev)
    return DEI2I_ERR_BAD_ARG;
  const dim3 grid = table_grid(max_n, 4, 512, count);
  hipLaunchKernelGGL(state_digest_kernel, grid, dim3(256), 0, (hipStream_t)s, table_dev, (uint32_t)row0, partial_dev);
  hipLaunchKernelGGL(state_digest_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, partial_dev, (int)(grid.x * grid.y),
                     accumulate, out_dev);
  return (int)hipGetLastError();
}

__global__ void index_advance_kernel(int* index) { *index += 1; }

extern "C" int dei2i_index_advance(int* index_dev, dei2i_stream s) {
  if (!index_dev) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(index_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, index_dev);
  return (int)hipGetLastError();
}

extern "C" int dei2i_ema_lerp(const dei2i_adam_rec* table_dev, int count, int64_t max_n, float weight, dei2i_stream s) {
  if (!table_dev || count <= 0 || max_n <= 0) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(ema_lerp_kernel<false>, table_grid(max_n, 1, 1024, count), dim3(256), 0, (hipStream_t)s, table_dev, weight,
                     nullptr, nullptr, 0);
  return (int)hipGetLastError();
}

extern "C" int dei2i_ema_lerp_dev(const dei2i_adam_rec* table_dev, int count, int64_t max_n, const float* weights_dev,
                                  const int* index_dev, int rows, dei2i_stream s) {
  if (!table_dev || count <= 0 || max_n <= 0 || !weights_dev || !index_dev || rows <= 0) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(ema_lerp_kernel<true>, table_grid(max_n, 1, 1024, count), dim3(256), 0, (hipStream_t)s, table_dev, 0.f,
                     weights_dev, index_dev, rows);
  return (int)hipGetLastError();
}
