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
void launch_light_out(const Desc* d, const half_t* brdf, const float* shading, const uint8_t* mask, const float* sigma_raw, hipStream_t st) {
    const dim3 grid(div_up(d->B, 256u)), block(256);
    const float inv_gamma = (float)(1.0 / (double)d->gamma);
    const bool spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
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
template <int FRAMES, typename Desc>
int curved_light_back_half(const Desc* d, const half_t* h, const half_t* xin, const half_t* n_lbc, const float* normal, const float* tbn, const float* tbn2,
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
    launch_light_out(d, k.brdf, shading, mask, k.sigma_raw, st);
    return check_launch(labels[1]);
}

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_light_infer_scratch_bytes(uint32_t B) { return CurvedLightScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_light_infer(const nerftex_curved_light_infer_desc* d, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_light_infer")) return NERFTEX_ERR_INVALID;
    if (!front_shapes_ok(d) || d->normal_C != 2 || d->normal_L != 4 || d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 ||
        d->brdf_hidden != 64 || d->brdf_layers != 3 || d->brdf_out != 5) {
        set_error("curved_light_infer: the kernels serve the default SH-lit curved field only (12 height bands, a 3-D table of 8 levels x 2 features, a normal "
                  "table of 4 levels x 2 features, sigma net 48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (!light_head_ok(d, "curved_light_infer")) return NERFTEX_ERR_INVALID;
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
    return curved_light_back_half<1>(d, sc.f.h, sc.f.xin, sc.n_lbc, sc.f.normal, sc.tbn, nullptr, nullptr, sc.f.mask, sc.back, labels, stream);
}
