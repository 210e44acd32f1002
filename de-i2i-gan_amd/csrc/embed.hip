// Device-drawn style embeddings of the SEAN generator (models/defectgan_model.py _get_style_embeds): per sample num_embeds rows of
// an embedding bank, drawn uniformly from the rows stored for the sample's label combination.
//
//   index[n, e] = offset[combo(n)] + mulhi(word(call, n, e), count[combo(n)])        (-1: an empty combination, or an invalid row)
//   feat[n, e, :] = index >= 0 ? bank[index[n, e], :] : 0
//
// dei2i_embed_draw fills the indices on the device: Philox4x32-10 keyed by a seed, counted by (call, slot quad, global row), the
// call count one word of device memory that the launch itself advances (the pattern of dei2i_mask_draw) -- an eager step and a
// replay of a captured step draw the same rows, and every replay draws new ones.  dei2i_embed_gather copies the rows; the index
// comes from device memory, so every index is checked against the bank before an address is formed from it.  Integer arithmetic and
// copies only: bit-exact, no atomics on global memory.
#include <hip/hip_runtime.h>

#include "../../include/dei2i_hip.h"
#include "launch.h"
#include "philox.h"

namespace dei2i {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kEmbedStream = 0xA0000000u;      // counter word c2 of slot quad q: kEmbedStream | q  (q < 2^26)

// One workgroup strides over the N x ceil(num_embeds / 4) slot quads.  Every thread reads the call count, then thread 0 stores
// count + 1 behind the barrier: one launch, no global atomics.  The rows whose labels are not all 0 or 1 are counted in LDS (by the
// thread that holds the row's quad 0) and thread 0 adds the sum to *invalid next to the counter store.
__global__ __launch_bounds__(kThreads) void embed_draw_kernel(unsigned long long seed, unsigned long long* __restrict__ counter, int N,
                                                              unsigned row0, int label_nc, int num_embeds,
                                                              const float* __restrict__ labels, const int* __restrict__ table,
                                                              long long table_total, int* __restrict__ index_out,
                                                              unsigned long long* __restrict__ invalid) {
  __shared__ unsigned bad_rows;
  const unsigned long long call = *counter;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)call, c1 = (uint32_t)(call >> 32);
  if (threadIdx.x == 0) bad_rows = 0u;
  __syncthreads();
  const int Q = (num_embeds + 3) >> 2;
  const long long items = (long long)N * Q;
  for (long long k = threadIdx.x; k < items; k += kThreads) {
    const int n = (int)(k / Q), q = (int)(k - (long long)n * Q);
    const float* lab = labels + (size_t)n * label_nc;
    int combo = 0;
    bool valid = true;
    for (int i = 0; i < label_nc; ++i) {
      const float v = lab[i];
      if (v > -1.f && v < 2.f) combo = (combo << 1) | (int)v;      // (int)v is 0 or 1 exactly on this interval; a NaN fails it
      else valid = false;
    }
    if (!valid && q == 0) atomicAdd(&bad_rows, 1u);      // (LDS)
    long long offset = 0;
    uint32_t count = 0u;
    if (valid) {
      const int off = table[2 * combo], cnt = table[2 * combo + 1];
      if (off >= 0 && cnt > 0 && (long long)off + cnt <= table_total) {      // (a table entry that leaves the bank draws nothing)
        offset = off;
        count = (uint32_t)cnt;
      }
    }
    const Philox4 x = philox4x32_10(c0, c1, kEmbedStream | (uint32_t)q, row0 + (uint32_t)n, k0, k1);
    const uint32_t w[4] = {x.x0, x.x1, x.x2, x.x3};
    int* dst = index_out + (size_t)n * num_embeds;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int t = 4 * q + e;
      if (t < num_embeds) dst[t] = count ? (int)(offset + __umulhi(w[e], count)) : -1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *counter = call + 1;
    *invalid = *invalid + bad_rows;
  }
}

// out[r, :] = bank[index[r], :], zeros for an index outside [0, bank_rows): each thread one quad of floats (VEC) or one float,
// grid-stride over rows x per_row
template <bool VEC>
__global__ __launch_bounds__(kThreads) void embed_gather_kernel(long long rows, int embed_nc, const int* __restrict__ index,
                                                                const float* __restrict__ bank, long long bank_rows,
                                                                float* __restrict__ out) {
  constexpr int L = VEC ? 4 : 1;
  const int per_row = VEC ? (embed_nc >> 2) : embed_nc;
  const long long total = rows * per_row, stride = (long long)gridDim.x * kThreads;
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < total; k += stride) {
    const long long r = k / per_row;
    const int c = (int)(k - r * per_row) * L;
    const long long idx = index[r];
    const bool hit = idx >= 0 && idx < bank_rows;
    float* dst = out + (size_t)r * embed_nc + c;
    if constexpr (VEC) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (hit) v = *reinterpret_cast<const float4*>(bank + (size_t)idx * embed_nc + c);
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = hit ? bank[(size_t)idx * embed_nc + c] : 0.f;
    }
  }
}

}  // namespace
}  // namespace dei2i

using namespace dei2i;

extern "C" int dei2i_embed_draw(uint64_t seed, uint64_t* counter_dev, int N, int row0, int label_nc, int num_embeds,
                                const float* labels, const int* table, int64_t table_total, int* index_out, uint64_t* invalid_dev,
                                dei2i_stream s) {
  if (!counter_dev || !labels || !table || !index_out || !invalid_dev || N <= 0 || row0 < 0 || num_embeds <= 0 || table_total < 0)
    return DEI2I_ERR_BAD_ARG;
  if ((long long)row0 + N > (1ll << 31) || label_nc < 1 || label_nc > DEI2I_EMBED_MAX_LABEL_NC || num_embeds > (1 << 28)) return DEI2I_ERR_BAD_ARG;
  hipLaunchKernelGGL(embed_draw_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)s, (unsigned long long)seed,
                     reinterpret_cast<unsigned long long*>(counter_dev), N, (unsigned)row0, label_nc, num_embeds, labels, table,
                     (long long)table_total, index_out, reinterpret_cast<unsigned long long*>(invalid_dev));
  return (int)hipGetLastError();
}

extern "C" int dei2i_embed_gather(int64_t rows, int embed_nc, const int* index, const float* bank, int64_t bank_rows, float* out,
                                  dei2i_stream s) {
  if (!index || !bank || !out || rows <= 0 || embed_nc <= 0 || bank_rows <= 0) return DEI2I_ERR_BAD_ARG;
  constexpr long long kMax = 1ll << 40;
  if (rows > (kMax - 1) / embed_nc || bank_rows > (kMax - 1) / embed_nc) return DEI2I_ERR_BAD_ARG;      // (elements: 40 bits)
  const bool vec = embed_nc % 4 == 0 && ((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const long long items = rows * (vec ? embed_nc / 4 : embed_nc);
  const dim3 grid(grid_for((size_t)items, kThreads));
  if (vec)
    hipLaunchKernelGGL(embed_gather_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)s, (long long)rows, embed_nc, index, bank,
                       (long long)bank_rows, out);
  else
    hipLaunchKernelGGL(embed_gather_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)s, (long long)rows, embed_nc, index, bank,
                       (long long)bank_rows, out);
  return (int)hipGetLastError();
}
