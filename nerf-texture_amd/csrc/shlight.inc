// The SH light head of the curved field (nerf/sh_light_model.py:554-616, SH_EnvmapMaterialNet.forward behind its BRDF MLP).
//
// The reference shades every sample with ~40 small framework ops: two sigmoids on the half BRDF outputs, the irradiance sum of the first nine
// svox2 SH bases at the shading normal (cosine lobe applied, clamped at 0), the same sum at the view direction reflected about the normal (the
// glossiness attenuation is exp(0) = 1 as the reference executes it: its order_coeff is arange(0, 1)), a clamp, and the 1 / gamma tone map through
// safe_pow -- and the mirror image in the backward pass.  Here it is one streaming kernel per direction (+ a 9 C block closing sum for the
// lighting gradient), the framework's arithmetic step by step: the sigmoids in fp32 narrowed to half, everything behind them fp32 with every
// operation rounded on its own (no contraction across the framework's op boundaries).  The backward pass recomputes the forward from its inputs.
// Included at the end of fieldglue.hip (the field's other glue kernels; common.hpp, <cmath> and narrow() come from there).

#pragma clang fp contract(off)  // every framework op rounds on its own (file scope: holds for everything below)

namespace nerftex {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMaxBlocks = 1024;  // backward: workgroups (a function of B alone: the summation order must not depend on the machine)
constexpr int kPartial = 27;           // floats per workgroup partial: 9 bases x (at most) 3 colours

// svox2's constants (sh_light_model.py:22-30) as the fp32 values the framework multiplies with
constexpr float kC0 = 0.28209479177387814f, kC1 = 0.4886025119029199f;
constexpr float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float kPi = 3.14159265358979323846f;

// render_irrandiance_sh_sum's cosine lobe: FloatTensor([3.14, 2.09 x 3, 0.79 x 5]) / pi
__host__ __device__ __forceinline__ float lobe(int k) { return (k == 0 ? 3.14f : k < 4 ? 2.09f : 0.79f) / kPi; }

// svox2_eval_sh_bases(9, dirs) (:52-76): NOT sh_common.hpp's tcnn ordering
__device__ __forceinline__ void svox2_basis9(const float x, const float y, const float z, float (&r)[9]) {
    r[0] = kC0;
    r[1] = -kC1 * y;
    r[2] = kC1 * z;
    r[3] = -kC1 * x;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, yz = y * z, xz = x * z;
    r[4] = kC2[0] * xy;
    r[5] = kC2[1] * yz;
    r[6] = kC2[2] * ((2.0f * zz - xx) - yy);
    r[7] = kC2[3] * xz;
    r[8] = kC2[4] * (xx - yy);
}

// torch.clamp keeps a NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float clamp0(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
// safe_pow(x, p) = pow(relu(where(|x| <= 1e-6, 1e-6, x)), p)  (:314-325)
__device__ __forceinline__ float safe_base(float v) {
    const float s = fabsf(v) <= 1e-6f ? 1e-6f : v;
    return s < 0.0f ? 0.0f : s;
}

template <int C>
struct Row {
    half_t a[3], sw;       // albedo, specular weight: the half sigmoids
    float yn[9], yw[9];    // bases at the normal and at the reflected direction
    float irr[C], srgb[C]; // irradiance at the normal before its clamp; at the reflected direction
    float sum[3];          // diffuse + specular before the clamp
    float diffuse[3], spec[C];
};

// envSHs[:9] x lobe through uniform loads: every lane reads the same words
template <int C>
__device__ __forceinline__ void load_env(const float* __restrict__ env, float (&el)[9][C]) {
#pragma unroll
    for (int k = 0; k < 9; k++)
#pragma unroll
        for (int c = 0; c < C; c++) el[k][c] = env[k * C + c] * lobe(k);
}

__device__ __forceinline__ void load_brdf(const half_t* __restrict__ brdf, uint32_t stride, bool wide, size_t b, half_t (&v)[4]) {
    if (wide) {  // rows of whole 8-byte words
        const half4_t w = *reinterpret_cast<const half4_t*>(brdf + b * stride);
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = brdf[b * stride + i];
    }
}

// the head's arithmetic of one row: n the shading normal, view the view direction (not normalised), both in registers
template <int C>
__device__ __forceinline__ void shade_vectors(const half_t (&x)[4], const float (&n)[3], const float (&view)[3], const float (&el)[9][C],
                                              const bool use_specular, Row<C>& r) {
#pragma unroll
    for (int c = 0; c < 3; c++) r.a[c] = narrow(1.0f / (1.0f + expf(-(float)x[c])));
    r.sw = narrow(1.0f / (1.0f + expf(-(float)x[3])));
    svox2_basis9(n[0], n[1], n[2], r.yn);
    float drgb[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        float acc = el[0][c] * r.yn[0];
#pragma unroll
        for (int k = 1; k < 9; k++) acc = acc + el[k][c] * r.yn[k];
        r.irr[c] = acc;
        drgb[c] = clamp0(acc);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) r.diffuse[c] = (float)r.a[c] * drgb[C == 3 ? c : 0];
    if (use_specular) {
        float d[3] = {view[0], view[1], view[2]};
        auto unit = [](float (&v)[3]) {  // v / (|v| + 1e-9)
            const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-9f;
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = v[c] / len;
        };
        unit(d);
        const float cos_theta = -((d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]);
        float w[3];
#pragma unroll
        for (int c = 0; c < 3; c++) w[c] = (2.0f * cos_theta) * n[c] + d[c];
        unit(w);
        svox2_basis9(w[0], w[1], w[2], r.yw);
#pragma unroll
        for (int c = 0; c < C; c++) {
            float acc = el[0][c] * r.yw[0];
#pragma unroll
            for (int k = 1; k < 9; k++) acc = acc + el[k][c] * r.yw[k];
            r.srgb[c] = acc;
            r.spec[c] = (float)r.sw * acc;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) r.yw[k] = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) r.srgb[c] = 0.0f, r.spec[c] = 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) r.sum[c] = r.diffuse[c] + r.spec[C == 3 ? c : 0];
}

// shade_vectors with row b's normal and direction loaded from global memory (the direction only where the specular term reads it)
template <int C>
__device__ __forceinline__ void shade_row(const half_t (&x)[4], const float* __restrict__ normals, const float* __restrict__ dirs, const size_t b,
                                          const float (&el)[9][C], const bool use_specular, Row<C>& r) {
    const float n[3] = {normals[b * 3], normals[b * 3 + 1], normals[b * 3 + 2]};
    float view[3] = {0.0f, 0.0f, 0.0f};
    if (use_specular) view[0] = dirs[b * 3], view[1] = dirs[b * 3 + 1], view[2] = dirs[b * 3 + 2];
    shade_vectors<C>(x, n, view, el, use_specular, r);
}

// the head's four outputs of a shaded row, component c: 0 colour, 1 specular, 2 diffuse, 3 albedo (NERFTEX_LIGHT_VISUAL_*)
template <int C>
__device__ __forceinline__ float row_output(const Row<C>& r, const int c, const int which, const float inv_gamma) {
    switch (which) {
        case 0: return powf(safe_base(clamp0(r.sum[c])), inv_gamma);
        case 1: return powf(safe_base(clamp01(r.spec[C == 3 ? c : 0])), inv_gamma);
        case 2: return powf(safe_base(clamp01(r.diffuse[c])), inv_gamma);
        default: return clamp01((float)r.a[c]);
    }
}

template <int C>
__global__ __launch_bounds__(kThreads) void sh_light_forward_kernel(const half_t* __restrict__ brdf, const uint32_t stride, const bool wide,
                                                                    const float* __restrict__ normals, const float* __restrict__ dirs,
                                                                    const float* __restrict__ env, const uint8_t* __restrict__ mask, const uint32_t B,
                                                                    const float inv_gamma, const bool use_specular, float* __restrict__ color,
                                                                    float* __restrict__ specular, float* __restrict__ diffuse, float* __restrict__ albedo) {
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            color[(size_t)b * 3 + c] = 0.0f;
            if (specular) specular[(size_t)b * 3 + c] = 0.0f;
            if (diffuse) diffuse[(size_t)b * 3 + c] = 0.0f;
            if (albedo) albedo[(size_t)b * 3 + c] = 0.0f;
        }
        return;
    }
    float el[9][C];
    load_env<C>(env, el);
    half_t x[4];
    load_brdf(brdf, stride, wide, b, x);
    Row<C> r;
    shade_row<C>(x, normals, dirs, b, el, use_specular, r);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        color[(size_t)b * 3 + c] = row_output<C>(r, c, 0, inv_gamma);
        if (specular) specular[(size_t)b * 3 + c] = row_output<C>(r, c, 1, inv_gamma);
        if (diffuse) diffuse[(size_t)b * 3 + c] = row_output<C>(r, c, 2, inv_gamma);
        if (albedo) albedo[(size_t)b * 3 + c] = row_output<C>(r, c, 3, inv_gamma);
    }
}

// the framework's sigmoid backward on fp16 tensors, in fp16 ARITHMETIC: (g (1 - y)) y, every operation rounded to half (fieldglue.hip)
__device__ __forceinline__ half_t sigmoid_backward_half(const half_t g, const half_t y) {
    half_t t = (half_t)1.0f - y;
    asm volatile("" : "+v"(t));
    half_t u = g * t;
    asm volatile("" : "+v"(u));
    return u * y;
}

// grad_color [B,3] -> grad_brdf [B,stride] half (columns 0..3; the rest 0) and this workgroup's partial of the lighting gradient
//   partial[blockIdx.x][k * C + c] = sum over the workgroup's samples of  d loss / d (envSHs[k, c] x lobe[k])
// The samples of a workgroup, the order in which a thread adds its samples, the wave's butterfly and the four waves' order are all fixed by B.
template <int C>
__global__ __launch_bounds__(kThreads) void sh_light_backward_kernel(const half_t* __restrict__ brdf, const uint32_t stride, const bool wide,
                                                                     const float* __restrict__ normals, const float* __restrict__ dirs,
                                                                     const float* __restrict__ env, const uint8_t* __restrict__ mask, const uint32_t B,
                                                                     const float inv_gamma, const float inv_gamma_m1, const bool use_specular,
                                                                     const float* __restrict__ grad_color, half_t* __restrict__ grad_brdf,
                                                                     float* __restrict__ partial) {
    __shared__ float wave_sums[kThreads / kWave][kPartial];
    float el[9][C];
    load_env<C>(env, el);
    float acc[9 * C];
#pragma unroll
    for (int i = 0; i < 9 * C; i++) acc[i] = 0.0f;
    for (uint32_t b = blockIdx.x * kThreads + threadIdx.x; b < B; b += gridDim.x * kThreads) {
        half_t gx[4] = {0, 0, 0, 0};
        if (!mask || mask[b]) {
            half_t x[4];
            load_brdf(brdf, stride, wide, b, x);
            Row<C> r;
            shade_row<C>(x, normals, dirs, b, el, use_specular, r);
            float g_irr[C], g_srgb[C], g_sw = 0.0f;
#pragma unroll
            for (int c = 0; c < C; c++) g_irr[c] = 0.0f, g_srgb[c] = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int cc = C == 3 ? c : 0;
                // pow backward  g (p x^(p-1));  the where passes it on outside |x| <= 1e-6, the clamp where its input is >= 0
                const float base = safe_base(clamp0(r.sum[c]));
                float gs = grad_color[(size_t)b * 3 + c] * (inv_gamma * powf(base, inv_gamma_m1));
                if (!(r.sum[c] >= 0.0f) || fabsf(clamp0(r.sum[c])) <= 1e-6f) gs = 0.0f;
                // diffuse = float(albedo) drgb: the gradient to the half albedo is narrowed where autograd casts it back
                const float drgb = clamp0(r.irr[cc]);
                gx[c] = sigmoid_backward_half(narrow(gs * drgb), r.a[c]);
                g_irr[cc] = g_irr[cc] + gs * (float)r.a[c];
                g_srgb[cc] = g_srgb[cc] + gs;  // (the specular term's share: times the weight below)
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
                if (!(r.irr[c] >= 0.0f)) g_irr[c] = 0.0f;
                if (use_specular) {
                    g_sw = g_sw + g_srgb[c] * r.srgb[c];
                    g_srgb[c] = g_srgb[c] * (float)r.sw;
                } else {
                    g_srgb[c] = 0.0f;
                }
            }
            if (use_specular) gx[3] = sigmoid_backward_half(narrow(g_sw), r.sw);
#pragma unroll
            for (int k = 0; k < 9; k++)
#pragma unroll
                for (int c = 0; c < C; c++) acc[k * C + c] = acc[k * C + c] + (g_irr[c] * r.yn[k] + g_srgb[c] * r.yw[k]);
        }
        half_t* row = grad_brdf + (size_t)b * stride;
        if (wide) {
            const half4_t lo = {gx[0], gx[1], gx[2], gx[3]};
            const half4_t zero = {0, 0, 0, 0};
            *reinterpret_cast<half4_t*>(row) = lo;
            for (uint32_t i = 4; i < stride; i += 4) *reinterpret_cast<half4_t*>(row + i) = zero;
        } else {
            for (uint32_t i = 0; i < stride; i++) row[i] = i < 4 ? gx[i] : (half_t)0.0f;
        }
    }
    // wave butterfly (every lane takes part: the loop above has ended for all of them), then the four waves in order
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < 9 * C; i++) {
        float v = acc[i];
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off, kWave);
        if (lane == 0) wave_sums[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 9 * C) {
        float v = wave_sums[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; w++) v = v + wave_sums[w][threadIdx.x];
        partial[(size_t)blockIdx.x * kPartial + threadIdx.x] = v;
    }
}

// grad_env_shs[k, c] = lobe[k] x (the workgroup partials summed in a fixed order), rows 9.. = 0; overwritten.  One wave per value.
__global__ __launch_bounds__(kWave) void sh_light_env_sum_kernel(const float* __restrict__ partial, const uint32_t n_partials, const uint32_t C,
                                                                 const uint32_t n_sh, float* __restrict__ grad_env) {
    const uint32_t v = blockIdx.x, lane = threadIdx.x;
    float s = 0.0f;
    for (uint32_t i = lane; i < n_partials; i += kWave) s = s + partial[(size_t)i * kPartial + v];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s = s + __shfl_xor(s, off, kWave);
    if (lane == 0) grad_env[v] = s * lobe((int)(v / C));
    if (v == 0)
        for (uint32_t i = 9 * C + lane; i < n_sh * C; i += kWave) grad_env[i] = 0.0f;
}

inline uint32_t backward_blocks(uint32_t B) { return B == 0 ? 0u : (div_up(B, (uint32_t)kThreads) < kMaxBlocks ? div_up(B, (uint32_t)kThreads) : kMaxBlocks); }

int check_desc(const nerftex_sh_light_desc* d, const char* what, bool backward) {
    if (!d) {
        set_error("%s: NULL descriptor", what);
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_sh < 9 || (d->n_color != 1 && d->n_color != 3)) {
        set_error("%s: the lighting holds at least 9 SH rows of 1 or 3 colours, but got [%u, %u]", what, d->n_sh, d->n_color);
        return NERFTEX_ERR_INVALID;
    }
    if (d->brdf_stride < 5 || !(d->gamma > 0.0f) || !std::isfinite(d->gamma)) {
        set_error("%s: the BRDF rows hold at least 5 values (got %u) and gamma is positive and finite", what, d->brdf_stride);
        return NERFTEX_ERR_INVALID;
    }
    if (d->flags & ~(uint32_t)NERFTEX_SH_LIGHT_SPECULAR) {
        set_error("%s: unknown flags 0x%x", what, d->flags);
        return NERFTEX_ERR_INVALID;
    }
    if (backward && !d->grad_env_shs) {
        set_error("%s: grad_env_shs must not be NULL", what);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    if (!d->brdf || !d->normals || !d->dirs || !d->env_shs || (!backward && !d->color)) {
        set_error("%s: brdf, normals, dirs, env_shs%s must not be NULL", what, backward ? "" : " and color");
        return NERFTEX_ERR_INVALID;
    }
    if (backward && (!d->grad_color || !d->grad_brdf || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 3) ||
                     d->scratch_bytes < nerftex_sh_light_scratch_bytes(d->B))) {
        set_error("%s: grad_color and grad_brdf must not be NULL, and scratch must be 4-byte aligned and hold %zu bytes", what,
                  nerftex_sh_light_scratch_bytes(d->B));
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

// rows of whole, aligned 8-byte words: the four used columns travel as one load / store
inline bool wide_rows(const void* p, const void* q, uint32_t stride) {
    return stride % 4 == 0 && !((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 7);
}

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_sh_light_scratch_bytes(uint32_t B) { return (size_t)(backward_blocks(B) ? backward_blocks(B) : 1u) * kPartial * sizeof(float); }

extern "C" int nerftex_sh_light_forward(const nerftex_sh_light_desc* d, void* stream) {
    clear_error();
    const int rc = check_desc(d, "sh_light_forward", false);
    if (rc != NERFTEX_OK || d->B == 0) return rc;
    hipStream_t st = as_stream(stream);
    const half_t* brdf = static_cast<const half_t*>(d->brdf);
    const bool wide = wide_rows(d->brdf, nullptr, d->brdf_stride), spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
    const float inv_gamma = (float)(1.0 / (double)d->gamma);
    const dim3 grid(div_up(d->B, (uint32_t)kThreads)), block(kThreads);
    {
        KernelTimer kt("sh_light_forward_kernel", st);
        if (d->n_color == 3)
            hipLaunchKernelGGL(sh_light_forward_kernel<3>, grid, block, 0, st, brdf, d->brdf_stride, wide, d->normals, d->dirs, d->env_shs, d->mask, d->B, inv_gamma,
                               spec, d->color, d->specular, d->diffuse, d->albedo);
        else
            hipLaunchKernelGGL(sh_light_forward_kernel<1>, grid, block, 0, st, brdf, d->brdf_stride, wide, d->normals, d->dirs, d->env_shs, d->mask, d->B, inv_gamma,
                               spec, d->color, d->specular, d->diffuse, d->albedo);
    }
    return check_launch("sh_light_forward");
}

extern "C" int nerftex_sh_light_backward(const nerftex_sh_light_desc* d, void* stream) {
    clear_error();
    int rc = check_desc(d, "sh_light_backward", true);
    if (rc != NERFTEX_OK) return rc;
    hipStream_t st = as_stream(stream);
    const uint32_t blocks = backward_blocks(d->B);
    float* partial = static_cast<float*>(d->scratch);
    if (blocks) {
        const half_t* brdf = static_cast<const half_t*>(d->brdf);
        half_t* grad_brdf = static_cast<half_t*>(d->grad_brdf);
        const bool wide = wide_rows(d->brdf, d->grad_brdf, d->brdf_stride), spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
        const double p = 1.0 / (double)d->gamma;
        KernelTimer kt("sh_light_backward_kernel", st);
        if (d->n_color == 3)
            hipLaunchKernelGGL(sh_light_backward_kernel<3>, dim3(blocks), dim3(kThreads), 0, st, brdf, d->brdf_stride, wide, d->normals, d->dirs, d->env_shs, d->mask,
                               d->B, (float)p, (float)(p - 1.0), spec, d->grad_color, grad_brdf, partial);
        else
            hipLaunchKernelGGL(sh_light_backward_kernel<1>, dim3(blocks), dim3(kThreads), 0, st, brdf, d->brdf_stride, wide, d->normals, d->dirs, d->env_shs, d->mask,
                               d->B, (float)p, (float)(p - 1.0), spec, d->grad_color, grad_brdf, partial);
    }
    if ((rc = check_launch("sh_light_backward")) != NERFTEX_OK) return rc;
    {
        // (B == 0: no partials; the sum writes the zeros)
        KernelTimer kt("sh_light_env_sum_kernel", st);
        hipLaunchKernelGGL(sh_light_env_sum_kernel, dim3(9 * d->n_color), dim3(kWave), 0, st, partial, blocks, d->n_color, d->n_sh, d->grad_env_shs);
    }
    return check_launch("sh_light_backward(sum)");
}

// ---- per-sample probe lighting (sh_light_model.py:561-571 with shade_visibility): imported lighting in eval, one of K coefficient sets per row ----
// The reference picks, per sample, the probe whose direction is closest to the sample's coarse normal -- argmax over a [B, K] product -- and
// gathers a [B, 9, 3] table for the head.  Here a workgroup stages the K directions and the K tables (x lobe) in LDS once; a row walks the
// directions (every lane reads the same word), keeps the first best and shades itself with shade_row<3> / row_output<3> from its table.

namespace nerftex {
namespace {

constexpr uint32_t kMaxProbes = 256;

__global__ __launch_bounds__(kThreads) void sh_light_probe_forward_kernel(const half_t* __restrict__ brdf, const uint32_t stride, const bool wide,
                                                                          const float* __restrict__ normals, const float* __restrict__ dirs,
                                                                          const float* __restrict__ normals2, const float* __restrict__ probes,
                                                                          const float* __restrict__ probe_shs, const uint32_t K,
                                                                          const uint8_t* __restrict__ mask, const uint32_t B, const float inv_gamma,
                                                                          const bool use_specular, float* __restrict__ color, float* __restrict__ specular,
                                                                          float* __restrict__ diffuse, float* __restrict__ albedo) {
    extern __shared__ float probe_lds[];  // [K][3] directions, then [K][9][3] tables x lobe
    float* dir_lds = probe_lds;
    float* el_lds = probe_lds + (size_t)K * 3;
    for (uint32_t i = threadIdx.x; i < K * 3; i += kThreads) dir_lds[i] = probes[i];
    for (uint32_t i = threadIdx.x; i < K * 27; i += kThreads) el_lds[i] = probe_shs[i] * lobe((int)((i % 27) / 3));
    __syncthreads();
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            color[(size_t)b * 3 + c] = 0.0f;
            if (specular) specular[(size_t)b * 3 + c] = 0.0f;
            if (diffuse) diffuse[(size_t)b * 3 + c] = 0.0f;
            if (albedo) albedo[(size_t)b * 3 + c] = 0.0f;
        }
        return;
    }
    const float n2[3] = {normals2[(size_t)b * 3], normals2[(size_t)b * 3 + 1], normals2[(size_t)b * 3 + 2]};
    uint32_t best = 0;
    float best_dot = (n2[0] * dir_lds[0] + n2[1] * dir_lds[1]) + n2[2] * dir_lds[2];
    for (uint32_t k = 1; k < K; k++) {
        const float dot = (n2[0] * dir_lds[k * 3] + n2[1] * dir_lds[k * 3 + 1]) + n2[2] * dir_lds[k * 3 + 2];
        if (dot > best_dot) best_dot = dot, best = k;  // (strictly: the lowest index among equal maxima)
    }
    float el[9][3];
#pragma unroll
    for (int k = 0; k < 9; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) el[k][c] = el_lds[best * 27 + k * 3 + c];
    half_t x[4];
    load_brdf(brdf, stride, wide, b, x);
    Row<3> r;
    shade_row<3>(x, normals, dirs, b, el, use_specular, r);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        color[(size_t)b * 3 + c] = row_output<3>(r, c, 0, inv_gamma);
        if (specular) specular[(size_t)b * 3 + c] = row_output<3>(r, c, 1, inv_gamma);
        if (diffuse) diffuse[(size_t)b * 3 + c] = row_output<3>(r, c, 2, inv_gamma);
        if (albedo) albedo[(size_t)b * 3 + c] = row_output<3>(r, c, 3, inv_gamma);
    }
}

int check_probe_desc(const nerftex_sh_light_probe_desc* d) {
    const char* what = "sh_light_probe_forward";
    if (!d) {
        set_error("%s: NULL descriptor", what);
        return NERFTEX_ERR_INVALID;
    }
    if (d->K == 0 || d->K > kMaxProbes) {
        set_error("%s: between 1 and %u probes, but got %u", what, kMaxProbes, d->K);
        return NERFTEX_ERR_INVALID;
    }
    if (d->brdf_stride < 5 || !(d->gamma > 0.0f) || !std::isfinite(d->gamma)) {
        set_error("%s: the BRDF rows hold at least 5 values (got %u) and gamma is positive and finite", what, d->brdf_stride);
        return NERFTEX_ERR_INVALID;
    }
    if (d->flags & ~(uint32_t)NERFTEX_SH_LIGHT_SPECULAR) {
        set_error("%s: unknown flags 0x%x", what, d->flags);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    if (!d->brdf || !d->normals || !d->dirs || !d->normals_secondary || !d->probes || !d->probe_shs || !d->color) {
        set_error("%s: brdf, normals, dirs, normals_secondary, probes, probe_shs and color must not be NULL", what);
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

}  // namespace
}  // namespace nerftex

extern "C" int nerftex_sh_light_probe_forward(const nerftex_sh_light_probe_desc* d, void* stream) {
    clear_error();
    const int rc = check_probe_desc(d);
    if (rc != NERFTEX_OK || d->B == 0) return rc;
    hipStream_t st = as_stream(stream);
    const bool wide = wide_rows(d->brdf, nullptr, d->brdf_stride), spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
    const float inv_gamma = (float)(1.0 / (double)d->gamma);
    {
        KernelTimer kt("sh_light_probe_forward_kernel", st);
        hipLaunchKernelGGL(sh_light_probe_forward_kernel, dim3(div_up(d->B, (uint32_t)kThreads)), dim3(kThreads), (size_t)d->K * 30 * sizeof(float), st,
                           static_cast<const half_t*>(d->brdf), d->brdf_stride, wide, d->normals, d->dirs, d->normals_secondary, d->probes, d->probe_shs, d->K,
                           d->mask, d->B, inv_gamma, spec, d->color, d->specular, d->diffuse, d->albedo);
    }
    return check_launch("sh_light_probe_forward");
}
