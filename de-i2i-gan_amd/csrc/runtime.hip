// Library bookkeeping: device query, error strings, in-library HIP-event timing of one kernel family.
#include <hip/hip_runtime.h>
#include <mutex>
#include <string.h>
#include <vector>

#include "../../include/dei2i_hip.h"
#include "launch.h"

namespace dei2i {

Options g_opt;

// Dynamic-LDS limits raised so far, keyed by kernel address.  Launches come from the forward thread and from autograd's
// backward thread, hence the lock; a full table only means that further kernels ask the runtime on every launch.
struct LdsLimit { const void* kernel; size_t bytes; };
static LdsLimit g_lds_limits[64];
static int g_lds_kernels = 0;
static std::mutex g_lds_mutex;

hipError_t ensure_dyn_lds(const void* kernel, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_lds_mutex);
  int i = 0;
  while (i < g_lds_kernels && g_lds_limits[i].kernel != kernel) ++i;
  if (i < g_lds_kernels && bytes <= g_lds_limits[i].bytes) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  if (i == g_lds_kernels && g_lds_kernels < 64) g_lds_limits[g_lds_kernels++] = LdsLimit{kernel, 0};
  if (i < g_lds_kernels) g_lds_limits[i].bytes = bytes;
  return hipSuccess;
}

struct ProfState {
  bool on = false;
  bool events = true;          // false: count launches and FLOPs only (no HIP events: nothing is added to the stream)
  int every = 1;               // events around every `every`-th launch only (a sample: two event records break back-to-back dispatch)
  bool armed = false;          // the current launch is bracketed
  double flops_timed = 0.0;    // FLOPs of the bracketed launches
  size_t counted = 0;
  std::vector<hipEvent_t> starts, stops;
  size_t used = 0;
  double flops = 0.0;
};
static ProfState g_prof[PROF_FAMILIES];

static long long g_launches[K_COUNT];
void count_launch(int kid) { g_launches[kid]++; }
static const char* const g_kernel_names[] = {"gather_v1", "gather_v2", "halo_conv", "halo_conv_fp8", "thin_cin", "thin_cout",
                                             "wgrad_v1", "wgrad_v2", "wgrad_halo", "wgrad_thin", "halo16_conv", "splitk_finalize", "halo16_s2"};
static_assert(sizeof(g_kernel_names) / sizeof(g_kernel_names[0]) == K_COUNT, "one name per KernelId, in its order");

static const struct { const char* name; int Options::*member; } g_option_table[] = {
    {"gather_gemm_v2", &Options::gather_gemm_v2}, {"wgrad_v2", &Options::wgrad_v2},     {"halo_conv", &Options::halo_conv},
    {"thin_conv", &Options::thin_conv},           {"halo16", &Options::halo16},         {"halo16_fold", &Options::halo16_fold},
    {"halo16_s2", &Options::halo16_s2},           {"wgrad_halo", &Options::wgrad_halo}, {"wgrad_thin", &Options::wgrad_thin},
    {"dgrad_s2_ring", &Options::dgrad_s2_ring}};

void prof_begin(int family, double flops, hipStream_t st) {
  ProfState& p = g_prof[family];
  if (!p.on) return;
  p.counted++;
  p.flops += flops;
  p.armed = p.events && (p.counted - 1) % (size_t)p.every == 0;
  if (!p.armed) return;
  p.flops_timed += flops;
  if (p.used == p.starts.size()) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    p.starts.push_back(a);
    p.stops.push_back(b);
  }
  hipEventRecord(p.starts[p.used], st);
}

void prof_end(int family, hipStream_t st) {
  ProfState& p = g_prof[family];
  if (!p.on || !p.armed) return;
  hipEventRecord(p.stops[p.used], st);
  p.used++;
}

}  // namespace dei2i

using namespace dei2i;

extern "C" {

int dei2i_version(void) { return 100; }

int dei2i_init(int device) {
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return (int)e;
  g_opt.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  return 0;
}

const char* dei2i_error_string(int code) {
  if (code == DEI2I_ERR_BAD_ARG) return "dei2i: bad argument";
  if (code == DEI2I_ERR_WORKSPACE) return "dei2i: workspace too small";
  if (code >= 0) return hipGetErrorString((hipError_t)code);
  return "dei2i: unknown error";
}

int dei2i_set_option(const char* name, int value) {
  if (name == nullptr) return DEI2I_ERR_BAD_ARG;
  for (const auto& o : g_option_table)
    if (strcmp(name, o.name) == 0) { g_opt.*o.member = value; return 0; }
  return DEI2I_ERR_BAD_ARG;
}

int dei2i_launch_counts(int64_t* out, int n) {
  for (int i = 0; i < n && i < K_COUNT; ++i) out[i] = (int64_t)g_launches[i];
  return K_COUNT;
}
void dei2i_launch_counts_reset(void) { for (int i = 0; i < K_COUNT; ++i) g_launches[i] = 0; }
const char* dei2i_kernel_name(int kid) { return kid >= 0 && kid < K_COUNT ? g_kernel_names[kid] : nullptr; }

int dei2i_prof_enable(int family, int on) {
  if (family < 0 || family >= PROF_FAMILIES) return DEI2I_ERR_BAD_ARG;
  ProfState& p = g_prof[family];
  p.on = on != 0;
  p.events = on != 2;
  p.every = on >= 3 ? on : 1;
  p.used = 0;
  p.counted = 0;
  p.flops = 0.0;
  p.flops_timed = 0.0;
  return 0;
}

int dei2i_prof_collect_timed(int family, int64_t* timed_launches, double* timed_flops) {
  if (family < 0 || family >= PROF_FAMILIES) return DEI2I_ERR_BAD_ARG;
  if (timed_launches) *timed_launches = (int64_t)g_prof[family].used;
  if (timed_flops) *timed_flops = g_prof[family].flops_timed;
  return 0;
}

int dei2i_prof_collect(int family, int64_t* launches, double* total_ms, double* total_flops) {
  if (family < 0 || family >= PROF_FAMILIES) return DEI2I_ERR_BAD_ARG;
  ProfState& p = g_prof[family];
  double ms = 0.0;
  for (size_t i = 0; i < p.used; ++i) {
    hipError_t e = hipEventSynchronize(p.stops[i]);
    if (e != hipSuccess) return (int)e;
    float t = 0.f;
    e = hipEventElapsedTime(&t, p.starts[i], p.stops[i]);
    if (e != hipSuccess) return (int)e;
    ms += t;
  }
  if (launches) *launches = (int64_t)p.counted;
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = p.flops;
  p.used = 0;
  p.counted = 0;
  p.flops = 0.0;
  p.flops_timed = 0.0;
  return 0;
}

}  // extern "C"
