// nerftex_curved_light_infer: the curved field with the SH light model as ONE device-count call (include/nerftex_hip.h), the rows contract of
// nerftex_curved_field_infer.  Included at the end of fieldglue.hip behind shlight.inc: the closing kernel below shades a row with the head's own
// row functions (shade_row, row_output) under that file's fp contract(off), restated here; the light mid kernel, the packed normal-net
// block's constants and the back half's buffers (LightBack) live in fieldglue.hip in front of both.  curved_light_back_half below is the closing
// sequence of all three lit entries (this one, planar_light.inc, shape_light.inc): light mid -> BRDF net -> closing kernel.

#pragma clang fp contract(off)  // every framework op rounds on its own (file scope, as shlight.inc)

namespace nerftex {
namespace {

// brdf [B,16] half (the BRDF net's output rows), normals [B,3] the light mid's shading normals, sigma_raw [B] fp32, mask [B] bytes
//   -> sigma [B] = mask ? sigma_raw : 0,  rgbs [B,3] = mask ? the head's output `which` (NERFTEX_LIGHT_VISUAL_*) : 0;  a marked slot: exactly 0
template <int C>
__global__ __launch_bounds__(kThreads) void curved_light_out_rows_kernel(const half_t* __restrict__ brdf, const float* __restrict__ normals,
                                                                         const float* __restrict__ dirs, const float* __restrict__ env,
                                                                         const uint8_t* __restrict__ mask, const float* __restrict__ sigma_raw, const uint32_t B,
                                                                         const float inv_gamma, const bool use_specular, const int which,
                                                                         float* __restrict__ sigma, float* __restrict__ rgbs,
                                                                         const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit) {
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= live_rows(B, units_dev, rows_per_unit)) return;
    if (slot_unused(dirs, b) || !mask[b]) {
        sigma[b] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) rgbs[(size_t)b * 3 + c] = 0.0f;
        return;
    }
    float el[9][C];
    load_env<C>(env, el);
    half_t x[4];
    load_brdf(brdf, 16, true, b, x);
    Row<C> r;
    shade_row<C>(x, normals, dirs, b, el, use_specular, r);
    sigma[b] = sigma_raw[b];
#pragma unroll
    for (int c = 0; c < 3; c++) rgbs[(size_t)b * 3 + c] = row_output<C>(r, c, which, inv_gamma);
}

// The closing kernel under relighting (nerftex_relight_desc, include/nerftex_hip.h), the same rows contract: coarse [B,3] is the RAW coarse normal
// the back half holds, normalised here as forward() does (twice: tools/map.py:720, network_curvedfield.py:295 -- the light mid's own `cn`), so no
// scratch buffer is added.  ROTATE: rotation [9] (device, row-major; uniform over the wave: scalar loads) turns the view direction, the shading normal
// and the coarse normal as einsum('ab,nb->na') does under fp16 autocast -- both operands rounded to half, the products (exact in fp32) added in
// ascending b, the sum rounded to half: the convention of lip_dot and of the light mid's frame rotations.  PROBES: K directions and K tables x lobe are
// staged once per workgroup in LDS (120 K bytes); a row walks the directions (every lane reads the same word: a broadcast) with
// sh_light_probe_forward_kernel's arithmetic, (x px + y py) + z pz, the lowest index among equal maxima, and shades with that table.  PROBES
// implies three colours.  `normals` (the caller's shading_normal or the scratch's) is only read: shading_normal stays the UNROTATED normal.
// A workgroup wholly past the live rows leaves before it stages anything.
template <int C, bool PROBES, bool ROTATE>
__global__ __launch_bounds__(kThreads) void curved_relight_out_rows_kernel(const half_t* __restrict__ brdf, const float* __restrict__ normals,
                                                                           const float* __restrict__ dirs, const float* __restrict__ coarse,
                                                                           const float* __restrict__ env, const float* __restrict__ probes,
                                                                           const float* __restrict__ probe_shs, const uint32_t K,
                                                                           const float* __restrict__ rotation, const uint8_t* __restrict__ mask,
                                                                           const float* __restrict__ sigma_raw, const uint32_t B, const float inv_gamma,
                                                                           const bool use_specular, const int which, float* __restrict__ sigma,
                                                                           float* __restrict__ rgbs, const int32_t* __restrict__ units_dev,
                                                                           const uint32_t rows_per_unit) {
    static_assert(!PROBES || C == 3, "the probe tables hold three colours");
    extern __shared__ float relight_lds[];  // PROBES: [K][3] directions, then [K][9][3] tables x lobe
    const uint32_t live = live_rows(B, units_dev, rows_per_unit);
    if (blockIdx.x * kThreads >= live) return;  // (the whole workgroup: nobody is left waiting at the barrier)
    if constexpr (PROBES) {
        for (uint32_t i = threadIdx.x; i < K * 3; i += kThreads) relight_lds[i] = probes[i];
        for (uint32_t i = threadIdx.x; i < K * 27; i += kThreads) relight_lds[K * 3 + i] = probe_shs[i] * lobe((int)((i % 27) / 3));
        __syncthreads();
    }
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= live) return;
    if (slot_unused(dirs, b) || !mask[b]) {
        sigma[b] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) rgbs[(size_t)b * 3 + c] = 0.0f;
        return;
    }
    float n[3], view[3], cn[3];
#pragma unroll
    for (int c = 0; c < 3; c++) n[c] = normals[(size_t)b * 3 + c], view[c] = dirs[(size_t)b * 3 + c];
    if constexpr (PROBES) {
        auto unit = [](float (&v)[3]) {  // v / (|v| + 1e-5)
            const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-5f;
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = v[c] / len;
        };
#pragma unroll
        for (int c = 0; c < 3; c++) cn[c] = coarse[(size_t)b * 3 + c];
        unit(cn);
        unit(cn);
    }
    if constexpr (ROTATE) {
        float rh[9];
#pragma unroll
        for (int k = 0; k < 9; k++) rh[k] = (float)narrow(rotation[k]);
        auto rotate = [&rh](float (&v)[3]) {
            const float vh[3] = {(float)narrow(v[0]), (float)narrow(v[1]), (float)narrow(v[2])};
#pragma unroll
            for (int a = 0; a < 3; a++) v[a] = (float)narrow((rh[a * 3] * vh[0] + rh[a * 3 + 1] * vh[1]) + rh[a * 3 + 2] * vh[2]);
        };
        rotate(view);
        rotate(n);
        if constexpr (PROBES) rotate(cn);
    }
    float el[9][C];
    if constexpr (PROBES) {
        const float* dir_lds = relight_lds;
        const float* el_lds = relight_lds + (size_t)K * 3;
        uint32_t best = 0;
        float best_dot = (cn[0] * dir_lds[0] + cn[1] * dir_lds[1]) + cn[2] * dir_lds[2];
        for (uint32_t k = 1; k < K; k++) {
            const float dot = (cn[0] * dir_lds[k * 3] + cn[1] * dir_lds[k * 3 + 1]) + cn[2] * dir_lds[k * 3 + 2];
            if (dot > best_dot) best_dot = dot, best = k;  // (strictly: the lowest index among equal maxima)
        }
#pragma unroll
        for (int k = 0; k < 9; k++)
#pragma unroll
            for (int c = 0; c < C; c++) el[k][c] = el_lds[best * 27 + k * 3 + c];
    } else {
        load_env<C>(env, el);
    }
    half_t x[4];
    load_brdf(brdf, 16, true, b, x);
    Row<C> r;
    shade_vectors<C>(x, n, view, el, use_specular, r);
    sigma[b] = sigma_raw[b];
#pragma unroll
    for (int c = 0; c < 3; c++) rgbs[(size_t)b * 3 + c] = row_output<C>(r, c, which, inv_gamma);
}

// whether a relight descriptor changes the closing launch at all: NULL, or no probes and no rotation, is the chain as it is
inline bool relight_active(const nerftex_relight_desc* r) { return r && (r->K != 0 || r->rotation); }

// The refusals of a nerftex_relight_desc, behind light_head_ok's (n_color and eval are valid by then); `who`: the entry's name in the messages.
template <typename Desc>
bool relight_ok(const Desc* d, const nerftex_relight_desc* r, const char* who) {
    if (!r) return true;
    if (r->K > kMaxProbes) {
        set_error("%s: at most %u probes, but got %u", who, kMaxProbes, r->K);
        return false;
    }
    if (r->K > 0 && (!r->probes || !r->probe_shs)) {
        set_error("%s: %u probes, but probes [K,3] or probe_shs [K,9,3] is NULL", who, r->K);
        return false;
    }
    if (r->K > 0 && d->n_color != 3) {
        set_error("%s: per-probe lighting holds three colours, but n_color is %u", who, d->n_color);
        return false;
    }
    if (d->eval == 0) {
        set_error("%s: a relight descriptor with eval == 0: imported lighting and the lighting rotation are eval-only", who);
        return false;
    }
    if (reinterpret_cast<uintptr_t>(r->rotation) & 3) {
        set_error("%s: rotation must be 4-byte aligned", who);
        return false;
    }
    return true;
}

// the scratch of one nerftex_curved_light_infer call: the front half's buffers (fieldglue.hip), then its own
struct CurvedLightScratch {
    ScratchCarver carve;
    CurvedFront f;
    float* tbn;
    half_t* n_lbc;
    LightBack back;
    CurvedLightScratch(void* scratch, size_t B)
        : carve{reinterpret_cast<uintptr_t>(scratch), B}, f(carve), tbn(carve.take<float>(9)), n_lbc(carve.take<half_t>(8)), back(carve) {}
};

// The refusals over the light head's members (n_sh .. eval), which the two lit chains' descriptors share; `who`: the entry's name in the messages.
template <typename Desc>
bool light_head_ok(const Desc* d, const char* who) {
    if (d->n_sh < 9 || (d->n_color != 1 && d->n_color != 3)) {
        set_error("%s: the lighting holds at least 9 SH rows of 1 or 3 colours, but got [%u, %u]", who, d->n_sh, d->n_color);
        return false;
    }
    if (!(d->gamma > 0.0f) || !std::isfinite(d->gamma) || (d->flags & ~(uint32_t)NERFTEX_SH_LIGHT_SPECULAR) || d->visual_mode > NERFTEX_LIGHT_VISUAL_ALBEDO ||
        (d->eval != 0 && d->eval != 1)) {
        set_error("%s: gamma is positive and finite, flags holds NERFTEX_SH_LIGHT_SPECULAR or nothing (got 0x%x), visual_mode is one of "
                  "NERFTEX_LIGHT_VISUAL_* (got %u) and eval is 0 or 1 (got %d)", who, d->flags, d->visual_mode, d->eval);
        return false;
    }
    return true;
}

// the closing launch of the lit chains
template <typename Desc>
void launch_light_out(const Desc* d, const nerftex_relight_desc* r, const half_t* brdf, const float* shading, const float* coarse, const uint8_t* mask,
                      const float* sigma_raw, hipStream_t st) {
    const dim3 grid(div_up(d->B, 256u)), block(256);
    const float inv_gamma = (float)(1.0 / (double)d->gamma);
    const bool spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
    if (relight_active(r)) {  // (relight_ok has passed: probes come with three colours)
        KernelTimer kt("curved_relight_out_rows_kernel", st);
        const size_t lds = (size_t)r->K * 30 * sizeof(float);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, lds, st, brdf, shading, d->dirs, coarse, d->env_shs, r->probes, r->probe_shs, r->K, r->rotation, mask, sigma_raw,
                               d->B, inv_gamma, spec, (int)d->visual_mode, d->sigma, d->rgbs, d->units_dev, d->rows_per_unit);
        };
        if (r->K && r->rotation) go(curved_relight_out_rows_kernel<3, true, true>);
        else if (r->K) go(curved_relight_out_rows_kernel<3, true, false>);
        else if (d->n_color == 3) go(curved_relight_out_rows_kernel<3, false, true>);
        else go(curved_relight_out_rows_kernel<1, false, true>);
        return;
    }
    KernelTimer kt("curved_light_out_rows_kernel", st);
    if (d->n_color == 3)
        hipLaunchKernelGGL(curved_light_out_rows_kernel<3>, grid, block, 0, st, brdf, shading, d->dirs, d->env_shs, mask, sigma_raw, d->B, inv_gamma, spec,
                           (int)d->visual_mode, d->sigma, d->rgbs, d->units_dev, d->rows_per_unit);
    else
        hipLaunchKernelGGL(curved_light_out_rows_kernel<1>, grid, block, 0, st, brdf, shading, d->dirs, d->env_shs, mask, sigma_raw, d->B, inv_gamma, spec,
                           (int)d->visual_mode, d->sigma, d->rgbs, d->units_dev, d->rows_per_unit);
}

// The launches of the lit chains' back half: light mid (the normal nets, FRAMES rotations by tbn, tbn2, tbn3 -- curved_light_mid_row -- into the caller's
// shading_normal or the scratch's) -> BRDF net 16 -> 64 x 3 -> 5 -> the head + mask as fp32.  h [B,16]: the sigma net's output, xin [B,48] its input,
// n_lbc [4,B,2]: the normal table's features, normal [B,3]: the raw coarse normal, mask [B]; labels: the entry's check_launch labels of the two kernels.
// r: the entry's relight descriptor or NULL (relight_ok has passed); it changes the closing launch only.
template <int FRAMES, typename Desc>
int curved_light_back_half(const Desc* d, const nerftex_relight_desc* r, const half_t* h, const half_t* xin, const half_t* n_lbc, const float* normal, const float* tbn, const float* tbn2,
                           const float* tbn3, const uint8_t* mask, const LightBack& k, const char* const (&labels)[2], void* stream) {
    hipStream_t st = as_stream(stream);
    float* shading = d->shading_normal ? d->shading_normal : k.shading;
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    {
        KernelTimer kt("curved_light_mid_rows_kernel", st);
        hipLaunchKernelGGL(curved_light_mid_rows_kernel<FRAMES>, dim3(div_up(B, 256u)), dim3(256), 0, st, h, xin, n_lbc, normal, tbn, tbn2, tbn3, d->dirs,
                           static_cast<const half_t*>(d->normal_weights), d->normal_biases, B, d->fc_weight, d->eval, k.sigma_raw, k.brdf_in, shading, units, rpu);
    }
    int rc = check_launch(labels[0]);
    if (rc != NERFTEX_OK) return rc;
    rc = ffmlp_inference_rows(k.brdf_in, d->brdf_weights, B, 16, 64, 3, k.brdf, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    launch_light_out(d, r, k.brdf, shading, normal, mask, k.sigma_raw, st);
    return check_launch(labels[1]);
}

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_light_infer_scratch_bytes(uint32_t B) { return CurvedLightScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_light_infer(const nerftex_curved_light_infer_desc* d, void* stream) { return nerftex_curved_light_infer_relit(d, nullptr, stream); }

extern "C" int nerftex_curved_light_infer_relit(const nerftex_curved_light_infer_desc* d, const nerftex_relight_desc* r, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_light_infer")) return NERFTEX_ERR_INVALID;
    if (!front_shapes_ok(d) || d->normal_C != 2 || d->normal_L != 4 || d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 ||
        d->brdf_hidden != 64 || d->brdf_layers != 3 || d->brdf_out != 5) {
        set_error("curved_light_infer: the kernels serve the default SH-lit curved field only (12 height bands, a 3-D table of 8 levels x 2 features, a normal "
                  "table of 4 levels x 2 features, sigma net 48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (!light_head_ok(d, "curved_light_infer") || !relight_ok(d, r, "curved_light_infer")) return NERFTEX_ERR_INVALID;
    if (d->B == 0) return NERFTEX_OK;
    const CurvedLightScratch sc(d->scratch, d->B);
    if (!front_pointers_ok(d, sc.carve.at) || !d->tbn || !d->normal_table || !d->normal_offsets || !d->normal_weights || !d->normal_biases || !d->brdf_weights ||
        !d->env_shs) {
        set_error("curved_light_infer: handles, inputs, frames, tables, weights, lighting and outputs must not be NULL, and scratch must be 256-byte aligned "
                  "and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!front_scales_ok(d) || !aligned16(d->brdf_weights) ||
        ((reinterpret_cast<uintptr_t>(d->normal_weights) | reinterpret_cast<uintptr_t>(d->normal_biases)) & 3) || !(d->normal_in_mul > 0.0f) ||
        !std::isfinite(d->normal_in_mul)) {
        set_error("curved_light_infer: the MLP weight vectors must be 16-byte aligned, the normal net's block 4-byte aligned, and the gathers' input scales "
                  "positive and finite");
        return NERFTEX_ERR_INVALID;
    }
    int rc = curved_front_gather(d, sc.f, sc.tbn, stream);
    if (rc != NERFTEX_OK) return rc;
    // (the normal table's gather, in front of the pack kernel: an exported entry, as the texture table's)
    rc = nerftex_grid_encode_forward_rows(sc.f.p_sur, d->normal_table, d->normal_offsets, sc.n_lbc, d->B, d->D, d->normal_C, d->normal_L, d->normal_S, d->normal_H,
                                          d->normal_gridtype, d->normal_align_corners, NERFTEX_F16, NERFTEX_LAYOUT_LBC, d->normal_in_add, d->normal_in_mul,
                                          d->units_dev, d->rows_per_unit, stream);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = curved_front_sigma(d, sc.f, "curved_light_infer(pack)", stream)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_light_infer(mid)", "curved_light_infer(out)"};
    return curved_light_back_half<1>(d, r, sc.f.h, sc.f.xin, sc.n_lbc, sc.f.normal, sc.tbn, nullptr, nullptr, sc.f.mask, sc.back, labels, stream);
}
