// Fitting SH lighting to an equirectangular environment map (nerf/sh_light_model.py:730-766, EnvMap2SH): the reference runs up to 5000 Adam
// iterations, each a forward over the whole map (SH2Envmap, :712-727), a backward, an optimizer step and a loss.item().  Its objective
//     loss(c) = mean over pixels and colours of (Y(dir) . c - y)^2
// is a fixed linear least-squares problem in the 27 numbers c[0..8][0..2], so the map is read ONCE: a moments kernel sums, in fp64,
//     G = sum Y Y^T (45 distinct entries),  b = sum Y y^T (27),  s = sum y^2 (3)
// and one wave then runs the whole loop on them: gradient 2 / (3 H W) (G c - b), torch's single-tensor Adam in fp32, the loss
// (c^T G c - 2 c^T b + s) / (3 H W) in fp64 and the reference's stopping rule.  Two launches, no host synchronisation.
// Included at the end of fieldglue.hip behind shlight.inc: svox2_basis9, kThreads and contraction off (file scope) come from there.
#include "adam_math.hpp"

namespace nerftex {
namespace {

constexpr int kMomG = 45, kMomB = 27, kMomS = 3, kMoments = kMomG + kMomB + kMomS;
constexpr uint32_t kEnvMaxBlocks = 1024;  // workgroups of the moments kernel: a function of H W alone, and so is the summation order

inline uint32_t envmap_blocks(uint64_t pixels) {
    const uint64_t n = div_up(pixels, (uint64_t)kThreads);
    return (uint32_t)(n < kEnvMaxBlocks ? n : kEnvMaxBlocks);
}

// G's upper triangle, row by row: (i, j), i <= j
__host__ __device__ __forceinline__ constexpr int gram_index(int i, int j) { return i <= j ? i * 9 - i * (i - 1) / 2 + (j - i) : j * 9 - j * (j - 1) / 2 + (i - j); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

// partial[blockIdx.x][0..74]: this workgroup's share of G, b, s.  The pixels of a thread, their order, the wave's butterfly and the four waves'
// order are fixed by H W.
__global__ __launch_bounds__(kThreads) void envmap_moments_kernel(const float* __restrict__ envmap, const float* __restrict__ phi,
                                                                  const float* __restrict__ theta, const uint32_t W, const uint64_t pixels,
                                                                  double* __restrict__ partial) {
    __shared__ double wave_sums[kThreads / kWave][kMoments];
    double acc[kMoments];
#pragma unroll
    for (int i = 0; i < kMoments; i++) acc[i] = 0.0;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < pixels; p += (uint64_t)gridDim.x * kThreads) {
        const float ph = phi[p / W], th = theta[p % W];
        // SH2Envmap's direction (cos theta sin phi, cos phi, sin theta sin phi), every product rounded to fp32 as the framework's
        const float sp = sinf(ph);
        float y9[9];
        svox2_basis9(cosf(th) * sp, cosf(ph), sinf(th) * sp, y9);
        double yd[9], px[3];
#pragma unroll
        for (int k = 0; k < 9; k++) yd[k] = (double)y9[k];
#pragma unroll
        for (int c = 0; c < 3; c++) px[c] = (double)envmap[p * 3 + c];
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = i; j < 9; j++) acc[gram_index(i, j)] = acc[gram_index(i, j)] + yd[i] * yd[j];
#pragma unroll
        for (int k = 0; k < 9; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) acc[kMomG + k * 3 + c] = acc[kMomG + k * 3 + c] + yd[k] * px[c];
#pragma unroll
        for (int c = 0; c < 3; c++) acc[kMomG + kMomB + c] = acc[kMomG + kMomB + c] + px[c] * px[c];
    }
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < kMoments; i++) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) wave_sums[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < kMoments) {
        double v = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; w++) v = v + wave_sums[w][threadIdx.x];
        partial[(size_t)blockIdx.x * kMoments + threadIdx.x] = v;
    }
}

// One wave: closes the partials (in workgroup order), then EnvMap2SH's loop (:744-760).  Lane l < 27 owns coefficient (k, c) = (l / 3, l % 3) of
// rows 0..8; rows 9.. receive no gradient in the reference (SH2Envmap reads envSHs[:9]) and stay 0.  torch.optim.Adam's single-tensor update on
// fp32 tensors with its host-side double scalars:
//     m.lerp_(g, 1 - b1);  v.mul_(b2).addcmul_(g, g, value = 1 - b2);  denom = (sqrt(v) / sqrt(1 - b2^t)).add_(eps);  p.addcdiv_(m, denom, value = -lr / (1 - b1^t))
__global__ __launch_bounds__(kWave) void envmap_iterate_kernel(const double* __restrict__ partial, const uint32_t n_partials, const double pixels3,
                                                               const uint32_t n_sh, const AdamConsts k, const uint32_t max_steps, const double min_loss,
                                                               const uint32_t min_steps, float* __restrict__ env_shs, int32_t* __restrict__ steps_run,
                                                               double* __restrict__ final_loss) {
    __shared__ double mom[kMoments];
    const int lane = threadIdx.x;
    for (int e = lane; e < kMoments; e += kWave) {
        double s = 0.0;
        for (uint32_t i = 0; i < n_partials; i++) s = s + partial[(size_t)i * kMoments + e];
        mom[e] = s;
    }
    __syncthreads();
    const bool owner = lane < 27;
    const int row = owner ? lane / 3 : 0, col = owner ? lane % 3 : 0;
    double g_row[9];
#pragma unroll
    for (int j = 0; j < 9; j++) g_row[j] = mom[gram_index(row, j)];
    const double b_own = mom[kMomG + row * 3 + col];
    const double sum_y2 = (mom[kMomG + kMomB] + mom[kMomG + kMomB + 1]) + mom[kMomG + kMomB + 2];
    const double grad_scale = 2.0 / pixels3;
    const float w1 = (float)(1 - k.beta1), b2 = (float)k.beta2, w2 = (float)(1 - k.beta2), eps = (float)k.eps;
    float p = 0.0f, m = 0.0f, v = 0.0f;
    double loss = 0.0;
    uint32_t step = 0;
    while (step < max_steps) {
        double gc = 0.0;  // (G c)[row, col]
#pragma unroll
        for (int j = 0; j < 9; j++) gc = gc + g_row[j] * (double)__shfl(p, j * 3 + col, kWave);
        // the loss of the parameters before this step's update: c^T G c - 2 c^T b + sum y^2, the 27 terms through the wave's butterfly
        loss = (wave_sum(owner ? (double)p * (gc - 2.0 * b_own) : 0.0) + sum_y2) / pixels3;
        const float g = (float)(grad_scale * (gc - b_own));
        step++;
        const float step_size = (float)(k.lr / (1 - pow(k.beta1, (double)step)));
        const float bc2_sqrt = (float)sqrt(1 - pow(k.beta2, (double)step));
        m = m + w1 * (g - m);
        v = v * b2;
        v = v + (w2 * g) * g;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = p + (-step_size * m) / denom;
        if (loss < min_loss && step - 1 > min_steps) break;  // (the reference's 0-based `step > 2000`, after the update)
    }
    if (owner) env_shs[lane] = p;
    for (uint32_t i = 27 + lane; i < n_sh * 3; i += kWave) env_shs[i] = 0.0f;
    if (lane == 0) {
        *steps_run = (int32_t)step;
        *final_loss = loss;
    }
}

int check_envmap_desc(const nerftex_envmap_fit_desc* d) {
    if (!d) {
        set_error("envmap_fit: NULL descriptor");
        return NERFTEX_ERR_INVALID;
    }
    if (d->H == 0 || d->W == 0) {
        set_error("envmap_fit: the map holds at least one pixel, but got [%u, %u]", d->H, d->W);
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_sh < 9) {
        set_error("envmap_fit: the lighting holds at least 9 SH rows, but got %u", d->n_sh);
        return NERFTEX_ERR_INVALID;
    }
    if (!(d->lr > 0.0) || !std::isfinite(d->lr) || std::isnan(d->min_loss) || d->max_steps == 0) {
        set_error("envmap_fit: lr is positive and finite, min_loss is a number and max_steps is positive");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->envmap || !d->phi || !d->theta || !d->env_shs || !d->steps_run || !d->final_loss) {
        set_error("envmap_fit: envmap, phi, theta, env_shs, steps_run and final_loss must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 7) || (reinterpret_cast<uintptr_t>(d->final_loss) & 7) ||
        d->scratch_bytes < nerftex_envmap_fit_scratch_bytes(d->H, d->W)) {
        set_error("envmap_fit: scratch must be 8-byte aligned and hold %zu bytes, and final_loss must be 8-byte aligned",
                  nerftex_envmap_fit_scratch_bytes(d->H, d->W));
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_envmap_fit_scratch_bytes(uint32_t H, uint32_t W) {
    const uint32_t blocks = envmap_blocks((uint64_t)H * W);
    return (size_t)(blocks ? blocks : 1u) * kMoments * sizeof(double);
}

extern "C" int nerftex_envmap_fit(const nerftex_envmap_fit_desc* d, void* stream) {
    clear_error();
    int rc = check_envmap_desc(d);
    if (rc != NERFTEX_OK) return rc;
    hipStream_t st = as_stream(stream);
    const uint64_t pixels = (uint64_t)d->H * d->W;
    const uint32_t blocks = envmap_blocks(pixels);
    double* partial = static_cast<double*>(d->scratch);
    {
        KernelTimer kt("envmap_moments_kernel", st);
        hipLaunchKernelGGL(envmap_moments_kernel, dim3(blocks), dim3(kThreads), 0, st, d->envmap, d->phi, d->theta, d->W, pixels, partial);
    }
    if ((rc = check_launch("envmap_fit(moments)")) != NERFTEX_OK) return rc;
    {
        const AdamConsts k{d->lr, 0.9, 0.999, 1e-8};
        KernelTimer kt("envmap_iterate_kernel", st);
        hipLaunchKernelGGL(envmap_iterate_kernel, dim3(1), dim3(kWave), 0, st, partial, blocks, 3.0 * (double)pixels, d->n_sh, k, d->max_steps, d->min_loss,
                           d->min_steps, d->env_shs, d->steps_run, d->final_loss);
    }
    return check_launch("envmap_fit(iterate)");
}
