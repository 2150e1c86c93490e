// The loss of a training step from the rays' errors (squared, or the step's criterion summed over the channels) -- err[N] -> loss, scaled loss -- in render_tail_forward_kernel's summation order
// (trainstep.hip): 64 consecutive rays by a shuffle tree, four such sums one after the other (its 256-ray workgroup), the workgroups' sums strided
// over 256 accumulators, those by the same tree.  ONE workgroup does it: nerftex_composite_step's second launch, or -- when the step's field
// backward follows (nerftex_field_backward_live_consume) -- an extra workgroup of its weight-gradient reduction launch, where it costs nothing.
#pragma once
#include "common.hpp"

namespace nerftex {

struct StepLossJob {
    const float* err;  // [n] squared error per ray
    uint32_t n;
    float loss_mul;
    const float* scale;  // device float or nullptr
    float *loss, *scaled_loss;  // scaled_loss may be nullptr
};
constexpr uint32_t kStepLossMaxRays = 256u * 1024u;
struct StepLossLds {
    float group[kStepLossMaxRays / 64];  // 16 KB
    float part[kStepLossMaxRays / 256];
    float last[4];
};

// The criterion of a step that is not the plain MSE one (nerftex_step_loss_desc): what the general instantiations of the tail kernels carry as
// wave-uniform fields.  err[n] is, for every kind, the sum over the ray's three channels of the elementwise criterion -- step_loss_sum below is
// the same sum for all of them.  torch's semantics: mse_loss, l1_loss (abs backward: sign, 0 at 0), huber_loss (quadratic where |d| <= delta).
struct StepCriterion {
    uint32_t kind = NERFTEX_LOSS_MSE;
    float param = 0.0f;                   // Huber's delta
    float* ray_loss = nullptr;            // optional [N]: err / 3, the reference's criterion(pred, gt).mean(-1)
    float* error_map = nullptr;           // optional [error_cells]
    const int64_t* error_inds = nullptr;  // [N] flat cell per ray; outside [0, error_cells): the ray updates nothing
    uint64_t error_cells = 0;
    float keep = 0.1f, take = 0.9f;
};
struct NoCriterion {};  // what the MSE instantiations take in its place

__device__ __forceinline__ float criterion_element(uint32_t kind, float delta, float d) {
#pragma clang fp contract(off)
    if (kind == NERFTEX_LOSS_L1) return fabsf(d);
    if (kind == NERFTEX_LOSS_HUBER) {
        const float a = fabsf(d);
        return a <= delta ? 0.5f * a * a : delta * (a - 0.5f * delta);
    }
    return d * d;
}
// de/dd of the L1 and Huber elements (the MSE gradient keeps its own expression: ray_loss_gradient / render_tail_backward_kernel)
__device__ __forceinline__ float criterion_slope(uint32_t kind, float delta, float d) {
#pragma clang fp contract(off)
    const float sign = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    if (kind == NERFTEX_LOSS_HUBER) return fabsf(d) <= delta ? d : delta * sign;
    return sign;
}
// one channel of grad_image for L1 / Huber: (de/dd) * g / (3N)
__device__ __forceinline__ float criterion_grad(uint32_t kind, float delta, float d, float g, float count) {
#pragma clang fp contract(off)
    return criterion_slope(kind, delta, d) * g / count;
}
// ONE thread per ray calls this with the ray's err: the per-ray loss and the error map's moving average (nerf/utils.py:617-632:
// 0.1 * old + 0.9 * error).  A plain read-modify-write: the rays' cells are distinct (multinomial without replacement); with duplicates one
// of the candidates lands, as in torch's scatter_.
__device__ __forceinline__ void record_ray_loss(const StepCriterion& k, uint32_t index, float err) {
#pragma clang fp contract(off)
    const float mean = err / 3.0f;
    if (k.ray_loss != nullptr) k.ray_loss[index] = mean;
    if (k.error_map != nullptr) {
        const int64_t cell = k.error_inds[index];
        if (cell >= 0 && (uint64_t)cell < k.error_cells) {
            const float old = k.error_map[cell];
            k.error_map[cell] = k.keep * old + k.take * mean;
        }
    }
}

// the criterion of a nerftex_step_loss_desc (all a backward reads); false (error set): unusable.  NULL: the MSE.
inline bool take_step_loss_kind(const nerftex_step_loss_desc* d, StepCriterion& out, const char* who) {
    out = StepCriterion{};
    if (d == nullptr) return true;
    if (d->kind != NERFTEX_LOSS_MSE && d->kind != NERFTEX_LOSS_L1 && d->kind != NERFTEX_LOSS_HUBER) {
        set_error("%s: unknown criterion kind %u (NERFTEX_LOSS_MSE, _L1 or _HUBER)", who, d->kind);
        return false;
    }
    if (d->kind == NERFTEX_LOSS_HUBER && !(d->param > 0.0f && d->param <= 3.4028234e38f)) {
        set_error("%s: the Huber criterion needs a finite delta > 0, got %g", who, (double)d->param);
        return false;
    }
    out.kind = d->kind;
    out.param = d->param;
    return true;
}
// ... with its outputs: the per-ray loss and the error map
inline bool take_step_loss_desc(const nerftex_step_loss_desc* d, StepCriterion& out, const char* who) {
    if (!take_step_loss_kind(d, out, who)) return false;
    if (d == nullptr) return true;
    if ((d->error_map != nullptr) != (d->error_inds != nullptr)) {
        set_error("%s: error_map and error_inds go together (a map needs the rays' cells, the cells need a map)", who);
        return false;
    }
    out.ray_loss = d->ray_loss;
    out.error_map = d->error_map;
    out.error_inds = d->error_inds;
    out.error_cells = d->error_cells;
    out.keep = d->keep;
    out.take = d->take;
    return true;
}

// Per-ray backgrounds and RGBA pixels (nerftex_step_pixels_desc): what the pixel instantiations of the tail kernels carry beside the criterion.
// nerf/utils.py:602-615 draws bg_color = torch.rand_like(images[..., :3]) and blends gt_rgb = rgb * a + bg_color * (1 - a); renderer.py:424
// blends image + (1 - weights_sum)[:, None] * bg_color.  Every operation below is rounded on its own (contraction off), in torch's order.
struct StepPixels {
    const float* bg_rays = nullptr;  // [N,3]
    const float* rgba = nullptr;     // [N,4] or nullptr: the target is then the caller's [N,3]
    float* target_out = nullptr;     // [N,3] with rgba: the blended target, written by a forward, read by a backward
};
struct StepCriterionPx : StepCriterion {
    StepPixels px;
};
struct RayPixels { float bg[3], gt[3]; };
// ONE ray's seven new values (three of the background, four of the pixel) and its target; `target` is read when there is no rgba
__device__ __forceinline__ RayPixels load_ray_pixels(const StepPixels& px, const float* __restrict__ target, size_t n) {
#pragma clang fp contract(off)
    RayPixels p;
#pragma unroll
    for (int c = 0; c < 3; c++) p.bg[c] = px.bg_rays[3 * n + c];
    if (px.rgba != nullptr) {
        const float a = px.rgba[4 * n + 3];
        const float rest = 1.0f - a;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float fore = px.rgba[4 * n + c] * a;
            const float back = p.bg[c] * rest;
            p.gt[c] = fore + back;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) p.gt[c] = target[3 * n + c];
    }
    return p;
}
// grad_weights_sum of image_out[c] = image[c] + (1 - weights_sum) * bg[c]; with bg == 1 the bits of the scalar form's -(sum * 1)
__device__ __forceinline__ float opacity_gradient(float gi0, float gi1, float gi2, const float* bg) {
#pragma clang fp contract(off)
    float sum = 0.0f;
    sum += gi0 * bg[0];
    sum += gi1 * bg[1];
    sum += gi2 * bg[2];
    return -sum;
}
// one channel of grad_image for any criterion: the MSE's own expression (render_tail_backward_kernel), else criterion_grad
__device__ __forceinline__ float pixel_grad(uint32_t kind, float delta, float norm, float count, float d, float g) {
#pragma clang fp contract(off)
    if (kind == NERFTEX_LOSS_MSE) return norm * d * g;
    return criterion_grad(kind, delta, d, g, count);
}

// a nerftex_step_pixels_desc beside the entry's `target`; false (error set): unusable
inline bool take_step_pixels_desc(const nerftex_step_pixels_desc* d, const float* target, StepPixels& out, const char* who) {
    out = StepPixels{};
    if (d->bg_rays == nullptr) {
        set_error("%s: the pixels descriptor needs bg_rays, the [N,3] per-ray background", who);
        return false;
    }
    if ((d->rgba != nullptr) == (target != nullptr)) {
        set_error("%s: exactly one of the pixels descriptor's rgba [N,4] and the entry's target [N,3] (got %s)", who, target ? "both" : "neither");
        return false;
    }
    if (d->rgba != nullptr && d->target_out == nullptr) {
        set_error("%s: rgba needs target_out, the [N,3] buffer of the blended target", who);
        return false;
    }
    out.bg_rays = d->bg_rays;
    out.rgba = d->rgba;
    out.target_out = d->rgba != nullptr ? d->target_out : nullptr;
    return true;
}
// ... of a backward entry: its target is the [N,3] the forward wrote
inline bool take_step_pixels_backward(const nerftex_step_pixels_desc* d, const float*& target, StepPixels& out, const char* who) {
    if (!take_step_pixels_desc(d, target, out, who)) return false;
    if (out.rgba != nullptr) target = out.target_out;
    out.rgba = nullptr;
    out.target_out = nullptr;
    return true;
}

template <uint32_t THREADS>
__device__ __forceinline__ void step_loss_sum(const StepLossJob& job, StepLossLds& lds) {
    static_assert(THREADS >= 256 && THREADS % 64 == 0, "");
    constexpr uint32_t kWaves = THREADS / 64, kAhead = 8192 / THREADS;  // (8192 rays: every value is requested before the first is used -- one memory round trip)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x / 64u;
    const uint32_t N = job.n, groups = (N + 63u) / 64u, parts = (N + 255u) / 256u;
    const float scale = (threadIdx.x == 0 && job.scaled_loss && job.scale) ? *job.scale : 1.0f;  // (requested with the errors, not behind the last barrier)
    for (uint32_t q0 = wave; q0 < parts * 4; q0 += kWaves * kAhead) {
        float v[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; j++) {
            const uint32_t q = q0 + j * kWaves, m = q * 64u + lane;
            v[j] = q < groups && m < N ? job.err[m] : 0.0f;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)  // (level by level over all the trees: kAhead independent shuffles in flight, not one chain after the other)
#pragma unroll
            for (uint32_t j = 0; j < kAhead; j++) v[j] += __shfl_down(v[j], o, 64);
#pragma unroll
        for (uint32_t j = 0; j < kAhead; j++)
            if (lane == 0 && q0 + j * kWaves < parts * 4) lds.group[q0 + j * kWaves] = v[j];
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < parts; p += THREADS) {
        float sacc = 0.0f;
        for (uint32_t i = 0; i < 4; i++) sacc += lds.group[4 * p + i];
        lds.part[p] = sacc;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        float acc = 0.0f;
        for (uint32_t i = threadIdx.x; i < parts; i += 256) acc += lds.part[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if (lane == 0) lds.last[wave] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.0f;
        for (uint32_t i = 0; i < 4; i++) total += lds.last[i];
        const float l = total / (float)((size_t)N * 3) * job.loss_mul;
        *job.loss = l;
        if (job.scaled_loss) *job.scaled_loss = job.scale ? l * scale : l;
    }
}

}  // namespace nerftex
