// The controller of adaptive discriminator augmentation (Karras et al. 2020, "Training Generative Adversarial Networks with Limited
// Data", section 3.1): the probability p of dei2i_diffaug_draw_p follows the overfitting heuristic r_t = E[sign(D(real))].
//
//   dei2i_ada_measure: pair = (sum of sign(logit), number of logits) of one tensor of D's real logits, as two int64 words
//   dei2i_ada_apply:   adds the pair and the number of real images into the accumulators; every `interval` calls
//                      r_t = sum / count, p = clamp(p + sign(r_t - target) * rows * inv_images, 0, p_max), accumulators = 0
//
// Everything lives in device memory and each launch is one workgroup, so a D update needs no host read and a captured step replays
// the controller exactly as the eager step runs it.  The sums are integers: exact, independent of order, and the SUM of the pairs
// of N ranks (parallel.GradReducer.ada_exchange, between the two launches) is the pair of one process on the whole batch.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;

// One workgroup strides over the logits.  A thread's count is at most n / 256 + 1 < 2^23 and a wave's 64 times that, so int holds
// them; the four wave sums meet in 64 bits.  NaN and +-0 compare false both ways: 0 towards the sum, 1 towards the count.
__global__ __launch_bounds__(kThreads) void ada_measure_kernel(const float* __restrict__ x, int n, long long* __restrict__ pair,
                                                               int accumulate) {
  __shared__ int lds[kThreads / 64];
  int acc = 0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float v = x[i];
    acc += (v > 0.f ? 1 : 0) - (v < 0.f ? 1 : 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long sum = ((long long)lds[0] + lds[1]) + ((long long)lds[2] + lds[3]);
    pair[0] = (accumulate ? pair[0] : 0ll) + sum;
    pair[1] = (accumulate ? pair[1] : 0ll) + (long long)n;
  }
}

// One thread.  Contraction is off: p + step is an add of a rounded product, as a numpy float32 model computes it.
__global__ void ada_apply_kernel(const long long* __restrict__ pair, long long rows, float* __restrict__ p_rt, long long* __restrict__ acc,
                                 int interval, float target, float inv_images, float p_max) {
#pragma clang fp contract(off)
  const long long sum = acc[0] + pair[0], count = acc[1] + pair[1], seen = acc[2] + rows, calls = acc[3] + 1;
  if (calls < interval) {
    acc[0] = sum;
    acc[1] = count;
    acc[2] = seen;
    acc[3] = calls;
    return;
  }
  const float rt = (float)sum / (float)count;
  const float step = (float)seen * inv_images;
  float p = p_rt[0] + (rt > target ? step : (rt < target ? -step : 0.f));
  p = p < 0.f ? 0.f : p;
  p = p > p_max ? p_max : p;
  p_rt[0] = p;
  p_rt[1] = rt;
  acc[0] = acc[1] = acc[2] = acc[3] = 0;
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int dei2i_ada_measure(const float* logits, int64_t n, int64_t* pair_dev, int accumulate, dei2i_stream s) {
  if (!logits || !pair_dev || n <= 0 || n >= (1ll << 31)) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(ada_measure_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)s, logits, (int)n,
                     reinterpret_cast<long long*>(pair_dev), accumulate);
  return (int)hipGetLastError();
}

extern "C" int dei2i_ada_apply(const int64_t* pair_dev, int64_t rows, float* p_rt_dev, int64_t* acc_dev, int interval, float target,
                               float inv_images, float p_max, dei2i_stream s) {
  if (!pair_dev || !p_rt_dev || !acc_dev || interval <= 0 || rows <= 0) return DEI2I_ERR_BAD_ARG;
  if (!(p_max >= 0.f && p_max <= 1.f) || !(target > -1.f && target < 1.f) || !(inv_images >= 0.f)) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(ada_apply_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, reinterpret_cast<const long long*>(pair_dev),
                     (long long)rows, p_rt_dev, reinterpret_cast<long long*>(acc_dev), interval, target, inv_images, p_max);
  return (int)hipGetLastError();
}
