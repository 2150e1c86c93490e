// The per-probe visibility lighting of an imported map (nerf/sh_light_model.py:647-670 load_envmap_with_visibility without a file, :692-709
// fit_product_of_SHs): for each of K probes, `rounds` Adam steps that pull 9 x 3 SH coefficients, started at the imported lighting, towards the
// product of that lighting and the probe's rotated visibility lobe on `batch` fresh sphere points per step.  The reference never clears the
// gradient, so Adam sees the SUM of all gradients so far; the result is defined by that trajectory and is followed as executed.
// Op by op that is K x rounds x ~60 launches; here ONE launch: a workgroup per probe walks all rounds.  A round is a latency chain
//     points -> 27 partial sums per thread -> wave reduction on the DPP paths -> LDS across the four waves -> Adam -> the next round's parameters
// with one barrier: the per-wave sums are double-buffered in LDS, every wave closes them and runs the 27 updates redundantly (lane l < 27 owns
// coefficient (k, c) = (l / 3, l % 3)), and hands the parameters to all its lanes by v_readlane -- they live in scalar registers.
// Included at the end of fieldglue.hip behind envmap.inc: svox2_basis9, kThreads, AdamConsts and contraction off (file scope) come from there.

namespace nerftex {
namespace {

constexpr int kVisWaves = kThreads / kWave;
constexpr int kVisAhead = 4;  // points of the next round a thread loads ahead of this round's barrier: batch <= 1024 is covered entirely

// wave64 sums on the DPP cross-lane paths of the VALU, the six steps of raymarching.hip's wave_scan_add: the totals arrive in lane 63.  All 27
// sums take a step together, so that no DPP operation waits on the VALU result just before it.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void vis_dpp_step(float (&v)[28]) {
#pragma unroll
    for (int i = 0; i < 27; i++)
        v[i] = v[i] + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[i]), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ void vis_wave_totals_in_lane63(float (&v)[28]) {
    vis_dpp_step<0x111, 0xf>(v);  // row_shr 1, 2, 4, 8: a lane without a source adds 0
    vis_dpp_step<0x112, 0xf>(v);
    vis_dpp_step<0x114, 0xf>(v);
    vis_dpp_step<0x118, 0xf>(v);
    vis_dpp_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    vis_dpp_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
}
__device__ __forceinline__ float vis_lane(float v, int lane) {  // lane's value in a scalar register (lane is a constant after unrolling)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// two uniforms in [0, 1) with 24 bits for (seed, probe, round, sample): the counter hash of occupancy.hip's uniform01, keyed so that the
// point does not depend on the launch shape.  This library's own stream, not torch's.
__device__ __forceinline__ void vis_uniforms(uint64_t seed, uint32_t probe, uint32_t round, uint32_t sample, float& u1, float& u2) {
    uint64_t s = (seed ^ 0x9E3779B97F4A7C15ull) + ((uint64_t)probe << 32 | round) * 0xD1342543DE82EF95ull;
    s ^= s >> 32; s *= 0xD6E8FEB86659FD93ull; s ^= s >> 32;
    s += (uint64_t)sample * 0x9E3779B97F4A7C15ull;
    s ^= s >> 32; s *= 0xD6E8FEB86659FD93ull; s ^= s >> 32; s *= 0xD6E8FEB86659FD93ull; s ^= s >> 32;
    u1 = (float)(uint32_t)(s >> 40) * (1.0f / 16777216.0f);
    u2 = (float)((uint32_t)(s >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
}

// the reference's point (:701-703): phi = 2 pi u1, theta = acos(1 - 2 u2), (cos phi sin theta, sin phi sin theta, cos theta)
__device__ __forceinline__ void vis_point(float u1, float u2, float (&p)[3]) {
    const float phi = (2.0f * kPi) * u1, theta = acosf(1.0f - 2.0f * u2);
    float sp, cp, st, ct;
    sincosf(phi, &sp, &cp);  // (one range reduction for the pair)
    sincosf(theta, &st, &ct);
    p[0] = cp * st;
    p[1] = sp * st;
    p[2] = ct;
}

__global__ __launch_bounds__(kThreads) void envmap_vis_fit_kernel(const float* __restrict__ env_shs, const float* __restrict__ lobes, const uint32_t rounds,
                                                                  const uint32_t batch, const AdamConsts k, const uint64_t seed,
                                                                  const float* __restrict__ points, float* __restrict__ points_out,
                                                                  float* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) float wave_sums[2][kVisWaves][28];
    __shared__ float fixed_lds[36];  // sh1 and the lobe for the per-point arithmetic: read from LDS they live in vector registers (in scalar registers beside the 27 parameters they spill)
    const uint32_t probe = blockIdx.x, tid = threadIdx.x;
    const int lane = tid % kWave, wave = tid / kWave;
    const bool owner = lane < 27;
        float sh[27];
#pragma unroll
    for (int i = 0; i < 27; i++) sh[i] = env_shs[i];
    if (tid < 36) fixed_lds[tid] = tid < 27 ? env_shs[tid] : lobes[(size_t)probe * 9 + (tid - 27)];
    float p_own = owner ? env_shs[lane] : 0.0f, g_run = 0.0f, m = 0.0f, v = 0.0f;
    const float inv_batch2 = 2.0f / (float)batch;
    const float w1 = (float)(1 - k.beta1), b2 = (float)k.beta2, w2 = (float)(1 - k.beta2), eps = (float)k.eps;
    double b1t = 1.0, b2t = 1.0;  // beta^t by running products in double (torch: beta ** t; the two agree to ~1e-13 at t = 800, below fp32's rounding of the results)
    const size_t probe_base = (size_t)probe * rounds * batch;

    float ahead[kVisAhead][3];
    auto load_ahead = [&](uint32_t r) {
#pragma unroll
        for (int j = 0; j < kVisAhead; j++) {
            const uint32_t i = tid + (uint32_t)j * kThreads;
            if (i < batch) {
                const float* src = points + (probe_base + (size_t)r * batch + i) * 3;
                ahead[j][0] = src[0]; ahead[j][1] = src[1]; ahead[j][2] = src[2];
            }
        }
    };
    if (points) load_ahead(0);

    __syncthreads();
    for (uint32_t r = 0; r < rounds; r++) {
        float acc[28], sh1[27], lob[9];
#pragma unroll
        for (int i = 0; i < 28; i++) acc[i] = 0.0f;
#pragma unroll
        for (int i = 0; i < 27; i++) sh1[i] = fixed_lds[i];
#pragma unroll
        for (int i = 0; i < 9; i++) lob[i] = fixed_lds[27 + i];
        auto one_point = [&](const float (&p)[3], uint32_t i) {
            if (points_out) {
                float* dst = points_out + (probe_base + (size_t)r * batch + i) * 3;
                dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
            }
            float b[9];
            svox2_basis9(p[0], p[1], p[2], b);
            float vis = b[0] * lob[0];
#pragma unroll
            for (int q = 1; q < 9; q++) vis = vis + b[q] * lob[q];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float light = b[0] * sh1[c], pred = b[0] * sh[c];
#pragma unroll
                for (int q = 1; q < 9; q++) {
                    light = light + b[q] * sh1[q * 3 + c];
                    pred = pred + b[q] * sh[q * 3 + c];
                }
                const float res = (pred - light * vis) * inv_batch2;  // d loss / d pred: 2 (pred - gt) / batch
#pragma unroll
                for (int q = 0; q < 9; q++) acc[q * 3 + c] = acc[q * 3 + c] + res * b[q];
            }
        };
        if (points) {
#pragma unroll
            for (int j = 0; j < kVisAhead; j++) {
                const uint32_t i = tid + (uint32_t)j * kThreads;
                if (i < batch) one_point(ahead[j], i);
            }
            for (uint64_t i = tid + kVisAhead * kThreads; i < batch; i += kThreads) {  // (64 bits: no wrap however large the batch)
                const float* src = points + (probe_base + (size_t)r * batch + i) * 3;
                const float p[3] = {src[0], src[1], src[2]};
                one_point(p, (uint32_t)i);
            }
            if (r + 1 < rounds) load_ahead(r + 1);  // in flight across the reduction and the barrier
        } else {
            for (uint64_t i = tid; i < batch; i += kThreads) {
                float u1, u2, p[3];
                vis_uniforms(seed, probe, r, (uint32_t)i, u1, u2);
                vis_point(u1, u2, p);
                one_point(p, (uint32_t)i);
            }
        }
        // the wave's 27 sums (lane 63), the four waves through LDS in wave order: one barrier per round, the buffers alternate
        vis_wave_totals_in_lane63(acc);
        if (lane == kWave - 1) {
            float4* mine = reinterpret_cast<float4*>(wave_sums[r & 1][wave]);  // (slot 27 carries acc[27] = 0: what the lanes that own nothing read)
#pragma unroll
            for (int q = 0; q < 7; q++) mine[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        }
        __syncthreads();
        const int slot = owner ? lane : 27;
        float g = wave_sums[r & 1][0][slot];
#pragma unroll
        for (int w = 1; w < kVisWaves; w++) g = g + wave_sums[r & 1][w][slot];
        g_run = g_run + g;  // never cleared: the reference calls no zero_grad()
        // torch.optim.Adam's single-tensor update on fp32 state with its host-side double scalars (envmap.inc states the ops)
        b1t *= k.beta1;
        b2t *= k.beta2;
        const float step_size = (float)(k.lr / (1 - b1t));
        const float bc2_sqrt = (float)sqrt(1 - b2t);
        m = m + w1 * (g_run - m);
        v = v * b2;
        v = v + (w2 * g_run) * g_run;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p_own = p_own + (-step_size * m) / denom;
#pragma unroll
        for (int i = 0; i < 27; i++) sh[i] = vis_lane(p_own, i);
    }
    if (wave == 0 && owner) tables[(size_t)probe * 27 + lane] = p_own;
}

int check_envmap_vis_desc(const nerftex_envmap_vis_fit_desc* d) {
    if (!d) {
        set_error("envmap_vis_fit: NULL descriptor");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->env_shs || !d->lobes || !d->tables) {
        set_error("envmap_vis_fit: env_shs, lobes and tables must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_sh < 9) {
        set_error("envmap_vis_fit: the lighting holds at least 9 SH rows, but got %u", d->n_sh);
        return NERFTEX_ERR_INVALID;
    }
    if (d->K == 0 || d->K > 256) {
        set_error("envmap_vis_fit: 1 to 256 probes, but got %u", d->K);
        return NERFTEX_ERR_INVALID;
    }
    if (d->rounds == 0 || d->batch == 0) {
        set_error("envmap_vis_fit: rounds and batch are positive, but got %u and %u", d->rounds, d->batch);
        return NERFTEX_ERR_INVALID;
    }
    if (!(d->lr > 0.0) || !std::isfinite(d->lr)) {
        set_error("envmap_vis_fit: lr is positive and finite");
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

}  // namespace
}  // namespace nerftex

extern "C" int nerftex_envmap_vis_fit(const nerftex_envmap_vis_fit_desc* d, void* stream) {
    clear_error();
    const int rc = check_envmap_vis_desc(d);
    if (rc != NERFTEX_OK) return rc;
    hipStream_t st = as_stream(stream);
    {
        const AdamConsts k{d->lr, 0.9, 0.999, 1e-8};
        KernelTimer kt("envmap_vis_fit_kernel", st);
        hipLaunchKernelGGL(envmap_vis_fit_kernel, dim3(d->K), dim3(kThreads), 0, st, d->env_shs, d->lobes, d->rounds, d->batch, k, d->seed, d->points,
                           d->points_out, d->tables);
    }
    return check_launch("envmap_vis_fit");
}
