// nerftex_curved_light_infer: the curved field with the SH light model as ONE device-count call (include/nerftex_hip.h), the rows contract of
// nerftex_curved_field_infer.  Included at the end of fieldglue.hip behind shlight.inc: the closing kernel below shades a row with the head's own
// row functions (shade_row, row_output) under that file's fp contract(off), restated here; the light mid kernel and the packed normal-net
// block's constants live in fieldglue.hip in front of both.

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

// the scratch of one nerftex_curved_light_infer call: every buffer starts on a 256-byte boundary
struct CurvedLightScratch {
    size_t idx, dist, p_sur, normal, tbn, mask, x_lbc, n_lbc, xin, h, sigma_raw, brdf_in, brdf, shading, total;
    explicit CurvedLightScratch(size_t B) {
        size_t at = 0;
        auto take = [&](size_t bytes_per_row) {
            const size_t here = at;
            at += (B * bytes_per_row + 255) / 256 * 256;
            return here;
        };
        idx = take(16 * sizeof(int32_t));  // (sized for the largest K)
        dist = take(16 * sizeof(float));
        p_sur = take(3 * sizeof(float));
        normal = take(3 * sizeof(float));
        tbn = take(9 * sizeof(float));
        mask = take(1);
        x_lbc = take(16 * sizeof(half_t));
        n_lbc = take(8 * sizeof(half_t));
        xin = take(48 * sizeof(half_t));
        h = take(16 * sizeof(half_t));
        sigma_raw = take(sizeof(float));
        brdf_in = take(16 * sizeof(half_t));
        brdf = take(16 * sizeof(half_t));
        shading = take(3 * sizeof(float));  // (used when the caller does not ask for the shading normal)
        total = at;
    }
};

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_light_infer_scratch_bytes(uint32_t B) { return CurvedLightScratch(B).total; }

extern "C" int nerftex_curved_light_infer(const nerftex_curved_light_infer_desc* d, void* stream) {
    clear_error();
    if (!d) {
        set_error("curved_light_infer: NULL descriptor");
        return NERFTEX_ERR_INVALID;
    }
    if (d->B % 128 != 0) {
        set_error("curved_light_infer: the batch must be a multiple of 128 rows, but got %u", d->B);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B != 0 && (d->n_verts == 0 || d->n_verts > 0x7fffffffu)) {
        set_error("curved_light_infer: the mesh needs between 1 and 2^31 - 1 vertices, but got %u", d->n_verts);
        return NERFTEX_ERR_INVALID;
    }
    if (d->K == 0 || d->K > 16) {
        set_error("curved_light_infer: 1 <= K <= 16 neighbours per point, but got %u", d->K);
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_freqs != 12 || d->D != 3 || d->C != 2 || d->L != 8 || d->normal_C != 2 || d->normal_L != 4 || d->sigma_in != 48 || d->sigma_hidden != 32 ||
        d->sigma_layers != 2 || d->sigma_out != 16 || d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 || d->brdf_hidden != 64 ||
        d->brdf_layers != 3 || d->brdf_out != 5) {
        set_error("curved_light_infer: the kernels serve the default SH-lit curved field only (12 height bands, a 3-D table of 8 levels x 2 features, a normal "
                  "table of 4 levels x 2 features, sigma net 48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_sh < 9 || (d->n_color != 1 && d->n_color != 3)) {
        set_error("curved_light_infer: the lighting holds at least 9 SH rows of 1 or 3 colours, but got [%u, %u]", d->n_sh, d->n_color);
        return NERFTEX_ERR_INVALID;
    }
    if (!(d->gamma > 0.0f) || !std::isfinite(d->gamma) || (d->flags & ~(uint32_t)NERFTEX_SH_LIGHT_SPECULAR) || d->visual_mode > NERFTEX_LIGHT_VISUAL_ALBEDO ||
        (d->eval != 0 && d->eval != 1)) {
        set_error("curved_light_infer: gamma is positive and finite, flags holds NERFTEX_SH_LIGHT_SPECULAR or nothing (got 0x%x), visual_mode is one of "
                  "NERFTEX_LIGHT_VISUAL_* (got %u) and eval is 0 or 1 (got %d)", d->flags, d->visual_mode, d->eval);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    const CurvedLightScratch at(d->B);
    if (!d->knn || !d->tracer || !d->xyz || !d->dirs || !d->mesh_vertices || !d->vertex_normals || !d->tbn || !d->table || !d->offsets || !d->normal_table ||
        !d->normal_offsets || !d->sigma_weights || !d->normal_weights || !d->normal_biases || !d->brdf_weights || !d->env_shs || !d->sigma || !d->rgbs ||
        !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < at.total) {
        set_error("curved_light_infer: handles, inputs, frames, tables, weights, lighting and outputs must not be NULL, and scratch must be 256-byte aligned "
                  "and hold %zu bytes", at.total);
        return NERFTEX_ERR_INVALID;
    }
    if (((reinterpret_cast<uintptr_t>(d->sigma_weights) | reinterpret_cast<uintptr_t>(d->brdf_weights)) & 15) ||
        ((reinterpret_cast<uintptr_t>(d->normal_weights) | reinterpret_cast<uintptr_t>(d->normal_biases)) & 3) || !(d->in_mul > 0.0f) || !std::isfinite(d->in_mul) ||
        !(d->normal_in_mul > 0.0f) || !std::isfinite(d->normal_in_mul)) {
        set_error("curved_light_infer: the MLP weight vectors must be 16-byte aligned, the normal net's block 4-byte aligned, and the gathers' input scales "
                  "positive and finite");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    char* sc = static_cast<char*>(d->scratch);
    int32_t* idx = reinterpret_cast<int32_t*>(sc + at.idx);
    float* dist = reinterpret_cast<float*>(sc + at.dist);
    float* p_sur = reinterpret_cast<float*>(sc + at.p_sur);
    float* normal = reinterpret_cast<float*>(sc + at.normal);
    float* tbn = reinterpret_cast<float*>(sc + at.tbn);
    uint8_t* mask = reinterpret_cast<uint8_t*>(sc + at.mask);
    half_t* x_lbc = reinterpret_cast<half_t*>(sc + at.x_lbc);
    half_t* n_lbc = reinterpret_cast<half_t*>(sc + at.n_lbc);
    half_t* xin = reinterpret_cast<half_t*>(sc + at.xin);
    half_t* h = reinterpret_cast<half_t*>(sc + at.h);
    float* sigma_raw = reinterpret_cast<float*>(sc + at.sigma_raw);
    half_t* brdf_in = reinterpret_cast<half_t*>(sc + at.brdf_in);
    half_t* brdf = reinterpret_cast<half_t*>(sc + at.brdf);
    float* shading = d->shading_normal ? d->shading_normal : reinterpret_cast<float*>(sc + at.shading);
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    const dim3 grid(div_up(B, 256u)), block(256);

    int rc = knn_query_rows(d->knn, d->xyz, d->dirs, B, d->K, idx, dist, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    rc = curved_project_rows(d->tracer, d->xyz, d->dirs, idx, dist, B, d->K, d->mesh_vertices, d->vertex_normals, d->n_verts, d->dir_vec_wdist, d->h_threshold,
                             p_sur, mask, normal, xin, units, rpu, st, d->tbn, tbn);
    if (rc != NERFTEX_OK) return rc;
    // (exported entries of this library: they clear the error text, which holds nothing at this point, and check the gathers' own arguments)
    rc = nerftex_grid_encode_forward_rows(p_sur, d->table, d->offsets, x_lbc, B, d->D, d->C, d->L, d->S, d->H, d->gridtype, d->align_corners, NERFTEX_F16,
                                          NERFTEX_LAYOUT_LBC, d->in_add, d->in_mul, units, rpu, stream);
    if (rc != NERFTEX_OK) return rc;
    rc = nerftex_grid_encode_forward_rows(p_sur, d->normal_table, d->normal_offsets, n_lbc, B, d->D, d->normal_C, d->normal_L, d->normal_S, d->normal_H,
                                          d->normal_gridtype, d->normal_align_corners, NERFTEX_F16, NERFTEX_LAYOUT_LBC, d->normal_in_add, d->normal_in_mul, units,
                                          rpu, stream);
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt("curved_pack_features_rows_kernel", st);
        hipLaunchKernelGGL(curved_pack_features_rows_kernel, grid, block, 0, st, x_lbc, B, xin, units, rpu);
    }
    if ((rc = check_launch("curved_light_infer(pack)")) != NERFTEX_OK) return rc;
    rc = ffmlp_inference_rows(xin, d->sigma_weights, B, 48, 32, 2, h, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt("curved_light_mid_rows_kernel", st);
        hipLaunchKernelGGL(curved_light_mid_rows_kernel, grid, block, 0, st, h, xin, n_lbc, normal, tbn, d->dirs, static_cast<const half_t*>(d->normal_weights),
                           d->normal_biases, B, d->fc_weight, d->eval, sigma_raw, brdf_in, shading, units, rpu);
    }
    if ((rc = check_launch("curved_light_infer(mid)")) != NERFTEX_OK) return rc;
    rc = ffmlp_inference_rows(brdf_in, d->brdf_weights, B, 16, 64, 3, brdf, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    {
        const float inv_gamma = (float)(1.0 / (double)d->gamma);
        const bool spec = (d->flags & NERFTEX_SH_LIGHT_SPECULAR) != 0;
        KernelTimer kt("curved_light_out_rows_kernel", st);
        if (d->n_color == 3)
            hipLaunchKernelGGL(curved_light_out_rows_kernel<3>, grid, block, 0, st, brdf, shading, d->dirs, d->env_shs, mask, sigma_raw, B, inv_gamma, spec,
                               (int)d->visual_mode, d->sigma, d->rgbs, units, rpu);
        else
            hipLaunchKernelGGL(curved_light_out_rows_kernel<1>, grid, block, 0, st, brdf, shading, d->dirs, d->env_shs, mask, sigma_raw, B, inv_gamma, spec,
                               (int)d->visual_mode, d->sigma, d->rgbs, units, rpu);
    }
    return check_launch("curved_light_infer(out)");
}
