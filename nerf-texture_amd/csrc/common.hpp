// Shared host/device helpers of libnerftex_hip.so (gfx950 only; no CUDA / portability shims).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/nerftex_hip.h"

namespace nerftex {

// ---- error reporting: int status + thread-local text (include/nerftex_hip.h) -------------------
void set_error(const char* fmt, ...);
void clear_error();

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
        return NERFTEX_ERR_HIP;
    }
    return NERFTEX_OK;
}

#define NERFTEX_HIP_TRY(expr, what)                                                   \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            ::nerftex::set_error("%s: %s", what, hipGetErrorString(_e));              \
            return NERFTEX_ERR_HIP;                                                   \
        }                                                                             \
    } while (0)

template <typename T>
constexpr T div_up(T a, T b) { return (a + b - 1) / b; }

// compute units of the current device (256 on an MI355X)
inline int device_cus() {
    static int cus[16] = {0};  // per device: a process may drive GPUs of different sizes
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    if (cus[dev] == 0) {
        hipDeviceProp_t prop;
        cus[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return cus[dev];
}

// ---- tuning knobs (runtime.hip) ----------------------------------------------------------------------------------------
// A/B switches and tuning parameters of the kernels.  Read ONCE when the library is loaded (NERFTEX_TUNE="name=value,..." plus
// the older one-variable-per-switch names), changed afterwards only through nerftex_tune_set(); a launch reads a plain array.
// ONE list: X(enumerator, "name of nerftex_tune_set / NERFTEX_TUNE") -- the enum below and the name table of runtime.hip are both generated from it.
#define NERFTEX_KNOBS(X)                                                                                                                           \
    X(kKnobGridFwd, "grid_fwd")                   /* 0 auto, 1 thread-per-sample kernel, 2 level-per-XCD kernel */                                 \
    X(kKnobGridBwd, "grid_bwd")                   /* 0 auto, 1 per-sample atomics, 2 tile owners (binned / sweep) */                               \
    X(kKnobGridBwdSweep, "grid_bwd_sweep")        /* 1: the tile-owner sweep instead of binning */                                                 \
    X(kKnobGridBwdItems, "grid_bwd_items")        /* sweep: work items per level (0 = auto) */                                                     \
    X(kKnobGridBwdSlice, "grid_bwd_slice")        /* binning: records per K4 work item (0 = default) */                                            \
    X(kKnobGridBwdNoMerge, "grid_bwd_nomerge")    /* binning: 1 = do not merge runs of samples that share a cell */                                \
    X(kKnobGridBwdProbe, "grid_bwd_probe")        /* phase ablation of K3 / K4 for profiling (0 = off; results are garbage when set) */            \
    X(kKnobMarch, "march")                        /* 0 auto, 1 replay, 2 log */                                                                    \
    X(kKnobMarchSerial, "march_serial")           /* 1: one-ray-per-lane DDA for the counting pass */                                              \
    X(kKnobFfmlpWgPerCu, "ffmlp_wg_per_cu")       /* forward: workgroups per CU (0 = default) */                                                   \
    X(kKnobFfmlpBwdSplit, "ffmlp_bwd_split")      /* 1: dgrad kernel + wgrad kernel through backward_buffer instead of the fused backward */       \
    X(kKnobMarchLean, "march_lean")               /* 1: the training march's count pass compiled for 64 registers (spills; slower alone, a better neighbour on a shared CU) */ \
    X(kKnobGridBwdStage, "grid_bwd_stage")        /* binning: LDS record slots per fill workgroup (0 = default; the rest of a workgroup's block goes straight to memory) */ \
    X(kKnobCompositeKeep, "composite_keep")       /* composite_step_kernel: 64-sample chunks a wave keeps in registers between its forward and backward walk (1..4; 0 = default 2) */ \
    X(kKnobMarchCountProbe, "march_count_probe")  /* phase ablation of march_count_parallel_kernel for profiling: 1..3 = every segment stops after that phase (0 = off; results are garbage when set) */
enum Knob {
#define NERFTEX_KNOB_ENUM(id, name) id,
    NERFTEX_KNOBS(NERFTEX_KNOB_ENUM)
#undef NERFTEX_KNOB_ENUM
    kKnobCount
};
extern long g_knobs[kKnobCount];
inline long knob(Knob k) { return g_knobs[k]; }

// ---- optional per-kernel timing (runtime.hip): { KernelTimer t("name", stream); hipLaunchKernelGGL(...); } --------------
extern int g_profile_mode;                   // 0 off, 1 every kernel, 2 hash-grid kernels only
constexpr int kTimeAny = 1, kTimeGrid = 2;  // timer groups
void profile_begin(const char* name, hipStream_t st, int* slot);
void profile_end(hipStream_t st, int slot);
struct KernelTimer {
    hipStream_t st;
    int slot = -1;
    KernelTimer(const char* name, hipStream_t s, int group = kTimeAny) : st(s) {
        if (g_profile_mode == 1 || (g_profile_mode == 2 && group == kTimeGrid)) profile_begin(name, s, &slot);
    }
    ~KernelTimer() { if (slot >= 0) profile_end(st, slot); }
};

// ---- device-side types --------------------------------------------------------------------------
using half_t = _Float16;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float16_t __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;  // gfx950 wavefront

// "rows per unit" of a launch sized by a device-side count (the inference loop: units = alive rays, rows per unit = n_step): a plain number,
// or -- bit 31 set, NERFTEX_ROWS_AUTO(N, F) of include/nerftex_hip.h -- "derive it from the count": n_step = clamp(F N / count, F, 8 F), the
// rule of nerf/renderer.py:470 with F N slots per iteration, evaluated by every kernel of the iteration from the same device word, so that
// an iteration can be recorded into a HIP graph without the host knowing how many rays are alive
__host__ __device__ __forceinline__ uint32_t unit_rows(uint32_t code, uint32_t count) {
    if (!(code >> 31)) return code;
    const uint32_t F = (code >> 24) & 127u, N = code & 0xffffffu;
    const uint32_t q = F * N / (count ? count : 1u);
    return q < F ? F : (q > 8u * F ? 8u * F : q);
}
// the rows of a B-row launch that carry anything: min(B, units_dev[0] * rows per unit); units_dev == NULL = all of them
__device__ __forceinline__ uint32_t live_rows(uint32_t B, const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    if (!units_dev) return B;
    const uint32_t n = (uint32_t)units_dev[0];
    return min(B, n * unit_rows(rows_per_unit, n));
}
// the mark nerftex_march_rays_dev leaves in the sample slots a ray does not use (1e30 as the direction's first component)
__device__ __forceinline__ bool slot_unused(const float* __restrict__ dirs, size_t row) { return dirs[row * 3] > 1e29f; }

}  // namespace nerftex
