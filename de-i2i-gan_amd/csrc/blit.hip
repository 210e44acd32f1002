// The pixel-blitting DiffAugment policies (utils/diffaug.py: flip -> rot90) on fp32 NCHW images: one element of the dihedral group
// per sample, code = f | k << 1 -- mirror left-right when f, then k quarter turns (torch.rot90) -- applied as a permutation of the
// pixels.  Its adjoint is the inverse permutation (ops._Blit / _BlitInverse), so the op is differentiable to any order and exact.
//
// Every code is one of two access patterns.  With (u, v) = (i, j) for even k and (j, i) for odd k, output pixel (i, j) takes source
// pixel (ra ? H-1-u : u, rb ? W-1-v : v):
//   code  0 id   1 f    2 r1     3 f,r1   4 r2    5 f,r2   6 r3     7 f,r3
//   src   i,j    i,~j   j,~i     j,i      ~i,~j   ~i,j     ~j,i     ~j,~i          (~x = S-1-x)
// so ra = k >> 1 and rb = f ^ (k & 1) ^ (k >> 1).  Even k moves rows (reversed or not); odd k is a transpose and goes through LDS.
//
// One workgroup serves one 32 x 32 output tile of one plane at a time (the code is uniform within it); 256 threads, each one quad
// along W.  Transposes stage the source tile in LDS already in output order, L[out row][out col] with a row stride of 33 dwords:
// the lanes of a 32-lane group hold 4 source rows x 8 quads, whose element e lands on bank (+-c +-r + const) mod 32 with c = 4m + e
// (m < 8) and r < 4 -- 32 distinct banks, and the read of 4 output rows x 8 quads is (i + 4m + e) mod 32 alike: ds_write_b32 and
// ds_read_b32 both bank modulo 32 within a 32-lane half, so neither side conflicts.  (Stride 32 would put the 8 quads of a row on
// one bank.)  Global reads and writes are both rows of the tile: 128 contiguous bytes per 8 lanes.
//
// dei2i_blit_draw fills the code table on the device under the rules of dei2i_diffaug_draw (one workgroup, no atomics, the call
// count advanced by the launch); dei2i_blit_draw_p gates each policy with a probability read from device memory.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"
#include "philox.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;
constexpr int kPitch = kTile + 1;

// the element a launch applies: code & 7, the quarter turns dropped on a non-square image, inverted when asked
__device__ __forceinline__ int effective_code(int word, bool square, int inverse) {
  int code = word & 7;
  if (!square) code &= 1;
  if (inverse && !(code & 1)) code = ((4 - (code >> 1)) & 3) << 1;          // (a reflection is its own inverse)
  return code;
}

// VEC: W % 4 == 0 and both pointers 16-byte aligned -- every quad of a row is wholly inside or outside the image
template <bool VEC>
__global__ __launch_bounds__(kThreads) void blit_kernel(const float* __restrict__ src, const int* __restrict__ codes, int C, int H, int W,
                                                        int tiles_x, int tiles, long long items, int inverse,
                                                        float* __restrict__ dst) {
  __shared__ float L[kTile * kPitch];
  const size_t plane = (size_t)H * W;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long p = item / tiles;                     // plane n * C + c
    const int tile = (int)(item - p * tiles);
    const int code = effective_code(codes[p / C], H == W, inverse);
    const int f = code & 1, k = code >> 1;
    const bool ra = (k >> 1) != 0, rb = ((f ^ k ^ (k >> 1)) & 1) != 0;
    const int i0 = (tile / tiles_x) * kTile, j0 = (tile % tiles_x) * kTile;
    const float* img = src + (size_t)p * plane;
    float* out = dst + (size_t)p * plane;
    if (!(k & 1)) {
      // rows: out[i][j] = img[ra ? H-1-i : i][rb ? W-1-j : j]
      if (VEC) {
        const int i = i0 + (int)(threadIdx.x >> 3), j = j0 + (int)(threadIdx.x & 7) * 4;
        if (i < H && j < W) {
          const float* row = img + (size_t)(ra ? H - 1 - i : i) * W;
          float4 v;
          if (rb) {
            const float4 q = *reinterpret_cast<const float4*>(row + (W - 4 - j));
            v = make_float4(q.w, q.z, q.y, q.x);
          } else {
            v = *reinterpret_cast<const float4*>(row + j);
          }
          *reinterpret_cast<float4*>(out + (size_t)i * W + j) = v;
        }
      } else {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int i = i0 + (int)(threadIdx.x >> 5) + 8 * it, j = j0 + (int)(threadIdx.x & 31);
          if (i < H && j < W) out[(size_t)i * W + j] = img[(size_t)(ra ? H - 1 - i : i) * W + (rb ? W - 1 - j : j)];
        }
      }
      continue;
    }
    // transpose (H == W == S): out[i][j] = img[ra ? S-1-j : j][rb ? S-1-i : i].  The source tile of this output tile starts at
    // (sr0, sc0), possibly off the image at the edges; source (sr0 + r, sc0 + c) is output (i0 + (rb ? 31-c : c), j0 + (ra ? 31-r : r)).
    const int S = H;
    const int sr0 = ra ? S - kTile - j0 : j0, sc0 = rb ? S - kTile - i0 : i0;
    __syncthreads();                                      // (the previous item's reads of L)
    if (VEC) {
      const int r = (int)(threadIdx.x >> 3), c = (int)(threadIdx.x & 7) * 4;
      const int si = sr0 + r, sj = sc0 + c;               // (S % 4 == 0: sc0 and sj are multiples of 4)
      if (si >= 0 && si < S && sj >= 0 && sj < S) {
        const float4 v = *reinterpret_cast<const float4*>(img + (size_t)si * S + sj);
        const int col = ra ? kTile - 1 - r : r;
        L[(rb ? kTile - 1 - c : c) * kPitch + col] = v.x;
        L[(rb ? kTile - 2 - c : c + 1) * kPitch + col] = v.y;
        L[(rb ? kTile - 3 - c : c + 2) * kPitch + col] = v.z;
        L[(rb ? kTile - 4 - c : c + 3) * kPitch + col] = v.w;
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int r = (int)(threadIdx.x >> 5) + 8 * it, c = (int)(threadIdx.x & 31);
        const int si = sr0 + r, sj = sc0 + c;
        if (si >= 0 && si < S && sj >= 0 && sj < S)
          L[(rb ? kTile - 1 - c : c) * kPitch + (ra ? kTile - 1 - r : r)] = img[(size_t)si * S + sj];
      }
    }
    __syncthreads();
    if (VEC) {
      const int il = (int)(threadIdx.x >> 3), jl = (int)(threadIdx.x & 7) * 4;
      const int i = i0 + il, j = j0 + jl;
      if (i < S && j < S) {
        const float* l = L + il * kPitch + jl;
        *reinterpret_cast<float4*>(out + (size_t)i * S + j) = make_float4(l[0], l[1], l[2], l[3]);
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int il = (int)(threadIdx.x >> 5) + 8 * it, jl = (int)(threadIdx.x & 31);
        const int i = i0 + il, j = j0 + jl;
        if (i < S && j < S) out[(size_t)i * S + j] = L[il * kPitch + jl];
      }
    }
  }
}

// One workgroup strides over the blit runs x N codes; run_flags: 2 bits per run of the WHOLE run list (DEI2I_BLIT_FLIP / _ROT90;
// 0: not a blit run, no row in the table).  The call count is read by every thread and stored + 1 by thread 0 behind the barrier,
// as in diffaug_draw_kernel.  GATED: x2 gates flip and x3 gates rot90 of the same Philox block, so a row's f and k do not depend on
// its gates and p = 1 is the ungated table.
template <bool GATED>
__global__ __launch_bounds__(kThreads) void blit_draw_kernel(unsigned long long seed, unsigned long long* __restrict__ counter, int runs,
                                                             unsigned long long flags, int blit_runs, int N, unsigned row0,
                                                             const float* __restrict__ p_dev, int* __restrict__ codes) {
  const unsigned long long call = *counter;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)call, c1 = (uint32_t)(call >> 32);
  float p = 1.f;
  if (GATED) p = *p_dev;
  for (int i = threadIdx.x; i < blit_runs * N; i += kThreads) {
    const int b = i / N, n = i - b * N;
    int run = 0, fl = 0;
    for (int r = 0, seen = 0; r < runs; ++r) {            // the b-th blit run of the list
      const int g = (int)(flags >> (2 * r)) & 3;
      if (g && seen++ == b) {
        run = r;
        fl = g;
        break;
      }
    }
    const Philox4 x = philox4x32_10(c0, c1, (uint32_t)run | (3u << 16), row0 + (uint32_t)n, k0, k1);
    int f = (fl & DEI2I_BLIT_FLIP) ? (int)(x.x0 >> 31) : 0;
    int k = (fl & DEI2I_BLIT_ROT90) ? (int)__umulhi(x.x1, 4u) : 0;
    if (GATED) {
      if (!(unit_float(x.x2) < p)) f = 0;
      if (!(unit_float(x.x3) < p)) k = 0;
    }
    codes[i] = f | k << 1;
  }
  __syncthreads();
  if (threadIdx.x == 0) *counter = call + 1;
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int dei2i_blit(int N, int C, int H, int W, const int* codes_dev, int inverse, const float* src, float* dst, dei2i_stream s) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || !codes_dev || !src || !dst) return DEI2I_ERR_BAD_ARG;
  if ((long long)N * C * H * W >= (1ll << 40) || (long long)C * H * W >= (1ll << 31)) return DEI2I_ERR_BAD_ARG;
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t bytes = (uintptr_t)N * C * H * W * sizeof(float);
  if (a < b + bytes && b < a + bytes) return DEI2I_ERR_BAD_ARG;          // in place (or overlapping): a permutation cannot be
  const int tiles_x = (W + kTile - 1) / kTile, tiles = tiles_x * ((H + kTile - 1) / kTile);
  const long long items = (long long)N * C * tiles;
  const unsigned grid = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
  if ((W % 4 == 0) && ((a | b) & 15) == 0)
    hipLaunchKernelGGL(blit_kernel<true>, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, src, codes_dev, C, H, W, tiles_x, tiles, items,
                       inverse, dst);
  else
    hipLaunchKernelGGL(blit_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)s, src, codes_dev, C, H, W, tiles_x, tiles, items,
                       inverse, dst);
  return (int)hipGetLastError();
}

// both draws: p_dev null = dei2i_blit_draw, else dei2i_blit_draw_p
static int blit_draw_launch(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                            int* codes, dei2i_stream s) {
  if (!counter_dev || !codes || runs <= 0 || runs > DEI2I_DIFFAUG_MAX_RUNS || N <= 0 || row0 < 0) return DEI2I_ERR_BAD_ARG;
  if ((long long)row0 + N > (1ll << 31) || (long long)runs * N >= (1ll << 24)) return DEI2I_ERR_BAD_ARG;
  if ((run_flags >> (2 * runs)) != 0) return DEI2I_ERR_BAD_ARG;
  int blit_runs = 0;
  for (int r = 0; r < runs; ++r) blit_runs += ((run_flags >> (2 * r)) & 3u) != 0;
  if (blit_runs == 0) return DEI2I_ERR_BAD_ARG;                             // (nothing to draw: the launch would only count)
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(counter_dev);
  if (p_dev)
    hipLaunchKernelGGL(blit_draw_kernel<true>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, blit_runs, N, (unsigned)row0, p_dev, codes);
  else
    hipLaunchKernelGGL(blit_draw_kernel<false>, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed, counter, runs,
                       (unsigned long long)run_flags, blit_runs, N, (unsigned)row0, p_dev, codes);
  return (int)hipGetLastError();
}

extern "C" int dei2i_blit_draw(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, int* codes,
                               dei2i_stream s) {
  return blit_draw_launch(seed, counter_dev, runs, run_flags, N, row0, nullptr, codes, s);
}

extern "C" int dei2i_blit_draw_p(uint64_t seed, uint64_t* counter_dev, int runs, uint64_t run_flags, int N, int row0, const float* p_dev,
                                 int* codes, dei2i_stream s) {
  if (!p_dev) return DEI2I_ERR_BAD_ARG;
  return blit_draw_launch(seed, counter_dev, runs, run_flags, N, row0, p_dev, codes, s);
}
