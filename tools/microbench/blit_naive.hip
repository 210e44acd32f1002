// The yardstick of tools/bench_blit.py: dei2i_blit's map (csrc/blit.hip) as a plain gather, one thread per output pixel -- coalesced
// writes, and for the transposing codes (odd k) reads that stride by a row per lane.  Not part of the library.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libblit_naive.so blit_naive.hip
#include <hip/hip_runtime.h>

__global__ __launch_bounds__(256) void blit_naive_kernel(const float* __restrict__ src, const int* __restrict__ codes, int C, int H, int W,
                                                         long long total, int inverse, float* __restrict__ dst) {
  const long long plane = (long long)H * W;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long p = t / plane;
    const int q = (int)(t - p * plane), i = q / W, j = q - i * W;
    int code = codes[p / C] & 7;
    if (H != W) code &= 1;
    if (inverse && !(code & 1)) code = ((4 - (code >> 1)) & 3) << 1;
    const int f = code & 1, k = code >> 1;
    const int u = (k & 1) ? j : i, v = (k & 1) ? i : j;
    const int si = (k >> 1) ? H - 1 - u : u, sj = ((f ^ k ^ (k >> 1)) & 1) ? W - 1 - v : v;
    dst[t] = src[p * plane + (long long)si * W + sj];
  }
}

extern "C" int blit_naive(int N, int C, int H, int W, const int* codes, int inverse, const float* src, float* dst, void* stream) {
  const long long total = (long long)N * C * H * W;
  if (total <= 0 || !codes || !src || !dst) return -2;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(blit_naive_kernel, dim3((unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20))), dim3(256), 0, (hipStream_t)stream, src,
                     codes, C, H, W, total, inverse, dst);
  return (int)hipGetLastError();
}
