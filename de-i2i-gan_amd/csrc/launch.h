// Internal declarations shared by the .hip translation units of libdei2i_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "common.h"
#include "geom.h"

namespace dei2i {

enum ProfFamily : int { PROF_GATHER_GEMM = 0, PROF_WGRAD = 1, PROF_HALO_CONV = 2, PROF_HALO_FOLD = 3, PROF_FAMILIES = 4 };
// host-side launch counters, one per MFMA kernel family (dei2i_launch_counts: the tests assert WHICH kernel served a shape,
// so that a silent fall-through to the generic GEMM cannot pass a parity test meant for a tuned kernel)
enum KernelId : int { K_GATHER_V1 = 0, K_GATHER_V2, K_HALO_CONV, K_HALO_CONV_FP8, K_THIN_CIN, K_THIN_COUT, K_WGRAD_V1, K_WGRAD_V2,
                      K_WGRAD_HALO, K_WGRAD_THIN, K_HALO16_CONV, K_SPLITK_FINALIZE, K_HALO16_S2, K_COUNT };
void count_launch(int kid);
void prof_begin(int family, double flops, hipStream_t st);
void prof_end(int family, hipStream_t st);

// The A-B switches of dei2i_set_option (names, values and defaults: include/dei2i_hip.h) and the device's CU count
// (dei2i_init; 256 until then): the library's one copy.
struct Options {
  int gather_gemm_v2 = 1;
  int wgrad_v2 = 1;
  int halo_conv = 1;
  int thin_conv = 1;
  int halo16 = 1;           // 0 = always the 8 x 32 tile kernel (conv_halo.hip)
  int halo16_fold = 1;      // 0 = ring GEMM + finalize + border fold as separate launches
  int halo16_s2 = 1;        // 0 = the 4x4 stride-2 convs stay on the gather GEMM
  int wgrad_halo = 1;
  int wgrad_thin = 1;
  int dgrad_s2_ring = 1;    // stride-2 reflect dgrads decomposed (interior into dx + ring rectangles)
  int num_cu = 256;
};
extern Options g_opt;
inline int num_cu() { return g_opt.num_cu; }

inline double conv_flops(const GatherDesc& g, int rows) {
  return 2.0 * (double)g.M * (double)(g.th * g.tw) * (double)g.Clog * (double)rows;
}

// Raises the kernel's dynamic-LDS limit to at least `bytes` (runtime.hip remembers, per kernel address, the largest value set:
// a size already covered costs no runtime call).
hipError_t ensure_dyn_lds(const void* kernel, size_t bytes);

// The launch protocol of the counted kernels, written once: LDS limit, launch counter, profiling bracket, launch, error.
// A failed attribute call returns before anything is counted or profiled.
template <typename... KArgs, typename... Args>
static inline hipError_t launch_counted(int kid, int family, double flops, void (*kern)(KArgs...), dim3 grid, dim3 block,
                                        size_t lds, hipStream_t st, Args&&... args) {
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds);
  if (e != hipSuccess) return e;
  count_launch(kid);
  prof_begin(family, flops, st);
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  prof_end(family, st);
  return hipGetLastError();
}

struct DescPack {
  GatherDesc d[4];
  long long woff[4];      // element offset of each class's packed weights
  FastDiv fd_taps[4];     // divide by th*tw (v2 k-step order)
  int n;
  int ws_compact;         // split-K partials indexed by (m_base[class] + m) instead of the output pixel
  int skip_dead_taps;     // v1: skip the k-steps of a tap that contributes zero to every row of the tile (reflect ring)
  int m_base[4];
};

// Every launcher below returns hipErrorNotSupported when the shape does not qualify; each *_shape_ok is the whole shape gate of
// its kernel, called by the launcher and by the C ABI's *_supported predicates.
hipError_t gather_gemm_v2(const DescPack& pack, const void* src, const void* wgt, int wrows, const float* bias, void* out,
                          float* ws, size_t ws_bytes, int ldc, int act, hipStream_t st);
hipError_t thin_cout_conv(const GatherDesc& g, const void* src, const void* wgt, int wrows, const float* bias, void* out, int ldc,
                          int act, hipStream_t st);
hipError_t thin_cin_conv(const GatherDesc& g, const void* src, const void* wgt, int wrows, const float* bias, void* out, int ldc,
                         int act, hipStream_t st);
bool halo_conv_shape_ok(const GatherDesc& g, int ldc, bool pro, bool pro_ring);
hipError_t halo_conv(const GatherDesc& g, const void* src, const void* wgt, int wrows, const float* bias, void* out, int ldc,
                     int act, hipStream_t st, const float* dequant = nullptr, const ConvPro* pro = nullptr,
                     float* stats = nullptr);

// 16 x 32 pixel tiles, 32-channel slices (conv_halo16.hip): the large-grid 3x3 stride-1 layers
hipError_t halo16_conv(const GatherDesc& g, const void* src, const void* wgt, int wrows, const float* bias, void* out, int ldc,
                       int act, hipStream_t st, float* stats = nullptr, const void* ring = nullptr, bool fold = false,
                       const EpiNorm* en = nullptr);
bool halo16_shape_ok(const GatherDesc& g, int ldc, bool fold, bool epin, bool ring);     // the 3x3 forms (options apart)
bool halo16_s2_shape_ok(const GatherDesc& g, int ldc);     // the 4x4 stride-2 form of the 16 x 32 tile kernel takes this conv
hipError_t gather_gemm(int dtype, const GatherDesc& g, const void* src, const void* wgt, int wrows, const float* bias,
                       void* out, float* ws, size_t ws_bytes, int ldc, int act, hipStream_t st);
hipError_t gather_gemm_multi(int dtype, const GatherDesc* descs, const long long* woffs, int n, const void* src,
                             const void* wgt, int wrows, const float* bias, void* out, float* ws, size_t ws_bytes, int ldc,
                             int act, hipStream_t st, bool compact_ws = false);
// One wgrad slab: the packed [Cout][K] gradient with the row count rounded up to 8, so the kernels' 8-row store
// groups need no per-row guard (the rows beyond Cout are never read).
static inline long long wgrad_slab_elems(int co_rows, int K) { return (long long)((co_rows + 7) & ~7) * K; }
// The split plan of the slab-writing wgrad launchers (wgrad_v2, wgrad_halo, wgrad_thin): `want` splits of `units` work units
// (pixel chunks / half-tiles), clamped to the slabs that fit in capacity_elems; every split takes `per` units, which leaves
// `zs` non-empty splits (the grid's split extent and *nsplit_out).  false: not even one slab fits.  How many splits a kernel
// wants is its launcher's own policy.
struct WgradSplitPlan {
  long long slab_elems;
  int splits;             // `want` after the clamp
  int per, zs;
};
static inline bool wgrad_split_plan(int co_rows, int K, size_t capacity_elems, int want, int units, WgradSplitPlan& p) {
  p.slab_elems = wgrad_slab_elems(co_rows, K);
  p.splits = want;
  if ((size_t)p.slab_elems * p.splits > capacity_elems) p.splits = (int)(capacity_elems / (size_t)p.slab_elems);
  if (p.splits < 1) return false;
  p.per = (units + p.splits - 1) / p.splits;
  p.zs = (units + p.per - 1) / p.per;
  return true;
}
// dw holds up to capacity_elems floats; split z writes slab z, *nsplit_out slabs to be summed by wgrad_reduce_unpack
// (deterministic).
hipError_t wgrad_gemm(int dtype, const GatherDesc& g, const void* src, const void* dy, int co_rows, int ldy, float* dw,
                      size_t capacity_elems, int* nsplit_out, hipStream_t st);

hipError_t wgrad_v2(const GatherDesc& g, const void* src, const void* dy, int co_rows, int ldy, float* slabs,
                    size_t slab_capacity_elems, int* nsplit_out, hipStream_t st);
// 0: not taken; else the tile it takes -- 1: 64 co x 128 ci, 2: 64 co x 64 ci with the taps over two wave groups, 3: 128 co x 64 ci
int wgrad_halo_shape_ok(const GatherDesc& g, int co_rows, bool pro_ring);
hipError_t wgrad_halo(const GatherDesc& g, const void* src, const void* dy, int co_rows, int ldy, float* slabs,
                      size_t slab_capacity_elems, int* nsplit_out, bool force, hipStream_t st,
                      const ConvPro* pro = nullptr);
hipError_t wgrad_thin(const GatherDesc& g, const void* src, const void* dy, int co_rows, int ldy, float* slabs,
                      size_t slab_capacity_elems, int* nsplit_out, hipStream_t st);
hipError_t wgrad_reduce_unpack(float* slabs, int nsplit, long long slab_elems, float* dw, int Cout, int Cin, int CinS,
                               int taps, int accumulate, hipStream_t st);

// A typed launch written once: f gets a value of the element type (bf16_t for DT_BF16, float for every other code) --
//   by_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(k<T>, ..., (const T*)x, ...); });
template <typename F>
static inline void by_dtype(int dtype, F&& f) {
  if (dtype == DT_BF16) f(bf16_t{});
  else f(float{});
}

inline unsigned grid_for(size_t work_items, int threads, unsigned cap = 256u * 8u) {
  size_t b = (work_items + threads - 1) / threads;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

}  // namespace dei2i
