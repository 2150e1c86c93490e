// The imported planar map under the SH light model: the `pred_normal` part of the 'field' branch of MeshFeatureField.forward (tools/map.py:670-675,
// :722-730) -- beside the feature read of planar.inc, a bilinear read of the [H, W, 8] phi map (the normal net's own table features), a nearest read
// of the per-texel frame and patch id, and the patch's inverted frame -- as one launch (nerftex_planar_light_lookup), and the lit field's no-grad
// forward over it as one device-count call (nerftex_curved_light_import_infer).  Included at the end of fieldglue.hip behind curved_light.inc: the
// row function of the lookup is planar.inc's, the lit reads lit_reads.hpp's, the closing sequence (the mid kernel with its second frame, the BRDF net, the closing
// kernel) curved_light.inc's curved_light_back_half.
//
// Lane mapping: one thread per row, as planar.inc's (DESIGN.md 4.15, 4.17).

namespace nerftex {
namespace {

// ROWS: the rows contract; phi goes out as half, level-major [4, B, 2] (what curved_light_mid_row reads as n_lbc); id_out is not written.
// Otherwise the plain form: every row, phi as fp32 [B, 8] (the values the half ones are the narrowing of), the sampled id [B].
// Both: local_tbn [B, 9] the texel's frame, sample_tbn [B, 9] row `id` of the inverted patch frames; an id outside [0, P) (the caller's to
// rule out) reads nothing and gives zeros.  A marked slot reads no texel of any map and writes planar_lookup_row's zeros only.
template <bool ROWS>
__global__ __launch_bounds__(256) void planar_light_lookup_rows_kernel(const float* __restrict__ xyz, const float* __restrict__ dirs, const uint32_t B,
                                                                       const PlanarArgs a, const PlanarLightArgs l, float* __restrict__ p_uv,
                                                                       float* __restrict__ sdf_out, uint8_t* __restrict__ mask, float* __restrict__ normal,
                                                                       half_t* __restrict__ xin, void* __restrict__ phi_out, int32_t* __restrict__ id_out,
                                                                       float* __restrict__ local_tbn, float* __restrict__ sample_tbn,
                                                                       const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit) {
    uint32_t b;
    float u, v;
    if (!planar_lookup_row<ROWS>(xyz, dirs, B, a, p_uv, sdf_out, mask, normal, xin, units_dev, rows_per_unit, b, u, v)) return;
    lit_reads_row<ROWS>(l, a.H, a.W, u, v, b, B, phi_out, id_out, local_tbn, sample_tbn);  // (lit_reads.hpp: the reads the lit shape lookup shares)
}

template <bool ROWS>
void launch_planar_light_lookup(hipStream_t st, const float* xyz, const float* dirs, uint32_t B, const PlanarArgs& a, const PlanarLightArgs& l, float* p_uv,
                                float* sdf, uint8_t* mask, float* normal, half_t* xin, void* phi, int32_t* id, float* local_tbn, float* sample_tbn,
                                const int32_t* units_dev, uint32_t rows_per_unit) {
    KernelTimer kt("planar_light_lookup_rows_kernel", st);
    hipLaunchKernelGGL(planar_light_lookup_rows_kernel<ROWS>, dim3(div_up(B, 256u)), dim3(256), 0, st, xyz, dirs, B, a, l, p_uv, sdf, mask, normal, xin, phi, id,
                       local_tbn, sample_tbn, units_dev, rows_per_unit);
}

// the scratch of one nerftex_curved_light_import_infer call
struct LightImportScratch {
    ScratchCarver carve;
    uint8_t* mask;
    float* normal;
    half_t *xin, *h, *n_lbc;
    float *local_tbn, *sample_tbn;
    LightBack back;
    LightImportScratch(void* scratch, size_t B)
        : carve{reinterpret_cast<uintptr_t>(scratch), B}, mask(carve.take<uint8_t>(1)), normal(carve.take<float>(3)), xin(carve.take<half_t>(48)),
          h(carve.take<half_t>(16)), n_lbc(carve.take<half_t>(8)), local_tbn(carve.take<float>(9)), sample_tbn(carve.take<float>(9)), back(carve) {}
};

}  // namespace
}  // namespace nerftex

extern "C" int nerftex_planar_light_lookup(const float* xyz, const float* map, const float* phi_map, const float* frame_map, const float* sample_tbn_inv,
                                           uint32_t map_h, uint32_t map_w, uint32_t n_patches, uint32_t mode, float plane_scale0, float plane_scale1,
                                           float height_scale0, float height_scale1, float sdf_offset, float h_threshold, uint32_t n_freqs, uint32_t B, float* p_uv,
                                           float* sdf, uint8_t* mask, void* xin, float* phi, int32_t* patch_id, float* local_tbn, float* sample_tbn,
                                           void* stream) {
    clear_error();
    if (n_freqs != kInferFreqs) {
        set_error("planar_light_lookup: the kernel writes the curved field's 12 height bands, but got n_freqs = %u", n_freqs);
        return NERFTEX_ERR_INVALID;
    }
    if (!map_extent_ok("planar_light_lookup", true, map_h, map_w)) return NERFTEX_ERR_INVALID;
    if (n_patches == 0 || n_patches > (1u << 24)) {
        set_error("planar_light_lookup: between 1 and 2^24 patch frames (an id is read from an fp32 texel), but got %u", n_patches);
        return NERFTEX_ERR_INVALID;
    }
    if (B == 0) return NERFTEX_OK;
    if (!xyz || !map || !phi_map || !frame_map || !sample_tbn_inv || !p_uv || !sdf || !mask || !xin || !phi || !patch_id || !local_tbn || !sample_tbn ||
        !aligned16(map) || !aligned16(phi_map) || !aligned16(frame_map) || !aligned16(sample_tbn_inv) || !aligned16(xin) || !aligned16(phi)) {
        set_error("planar_light_lookup: inputs, maps and outputs must not be NULL, and the maps, the patch frames, xin and phi must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    if (!planar_scales_ok(mode, plane_scale0, plane_scale1, height_scale0, height_scale1, sdf_offset, h_threshold)) {
        set_error("planar_light_lookup: mode is NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE, the scales and h_threshold positive and finite, sdf_offset "
                  "finite");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const PlanarArgs a{map, map_h, map_w, (int)mode, plane_scale0, plane_scale1, height_scale0, height_scale1, sdf_offset, h_threshold};
    const PlanarLightArgs l{phi_map, frame_map, sample_tbn_inv, n_patches};
    launch_planar_light_lookup<false>(st, xyz, nullptr, B, a, l, p_uv, sdf, mask, nullptr, static_cast<half_t*>(xin), phi, patch_id, local_tbn, sample_tbn, nullptr,
                                      0u);
    return check_launch("planar_light_lookup");
}

extern "C" size_t nerftex_curved_light_import_infer_scratch_bytes(uint32_t B) { return LightImportScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_light_import_infer(const nerftex_curved_light_import_infer_desc* d, void* stream) { return nerftex_curved_light_import_infer_relit(d, nullptr, stream); }

extern "C" int nerftex_curved_light_import_infer_relit(const nerftex_curved_light_import_infer_desc* d, const nerftex_relight_desc* r, void* stream) {
    clear_error();
    if (!batch_ok(d, "curved_light_import_infer")) return NERFTEX_ERR_INVALID;
    if (d->n_features != 16 || d->n_phi != 8 || d->n_freqs != kInferFreqs || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 ||
        d->sigma_out != 16 || d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 || d->brdf_hidden != 64 || d->brdf_layers != 3 ||
        d->brdf_out != 5) {
        set_error("curved_light_import_infer: the kernels serve the default SH-lit curved field only (a map of 16 features, a phi map of 8, 12 height bands, "
                  "sigma net 48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (!light_head_ok(d, "curved_light_import_infer") || !relight_ok(d, r, "curved_light_import_infer")) return NERFTEX_ERR_INVALID;
    if (!map_extent_ok("curved_light_import_infer", true, d->map_h, d->map_w)) return NERFTEX_ERR_INVALID;
    if (d->n_patches == 0 || d->n_patches > (1u << 24)) {
        set_error("curved_light_import_infer: between 1 and 2^24 patch frames (an id is read from an fp32 texel), but got %u", d->n_patches);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    const LightImportScratch sc(d->scratch, d->B);
    if (!d->xyz || !d->dirs || !d->map || !d->phi_map || !d->frame_map || !d->sample_tbn_inv || !d->sigma_weights || !d->normal_weights || !d->normal_biases ||
        !d->brdf_weights || !d->env_shs || !d->sigma || !d->rgbs || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) ||
        d->scratch_bytes < sc.carve.at) {
        set_error("curved_light_import_infer: inputs, maps, patch frames, weights, lighting and outputs must not be NULL, and scratch must be 256-byte aligned "
                  "and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->map) || !aligned16(d->phi_map) || !aligned16(d->frame_map) || !aligned16(d->sample_tbn_inv) || !aligned16(d->sigma_weights) ||
        !aligned16(d->brdf_weights) || ((reinterpret_cast<uintptr_t>(d->normal_weights) | reinterpret_cast<uintptr_t>(d->normal_biases)) & 3)) {
        set_error("curved_light_import_infer: the maps, the patch frames and the MLP weight vectors must be 16-byte aligned, the normal net's block 4-byte "
                  "aligned");
        return NERFTEX_ERR_INVALID;
    }
    if (!planar_scales_ok(d->mode, d->plane_scale0, d->plane_scale1, d->height_scale0, d->height_scale1, d->sdf_offset, d->h_threshold)) {
        set_error("curved_light_import_infer: mode is NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE, the scales and h_threshold positive and finite, "
                  "sdf_offset finite");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    const PlanarArgs a{d->map, d->map_h, d->map_w, (int)d->mode, d->plane_scale0, d->plane_scale1, d->height_scale0, d->height_scale1, d->sdf_offset, d->h_threshold};
    const PlanarLightArgs l{d->phi_map, d->frame_map, d->sample_tbn_inv, d->n_patches};
    launch_planar_light_lookup<true>(st, d->xyz, d->dirs, B, a, l, nullptr, nullptr, sc.mask, sc.normal, sc.xin, sc.n_lbc, nullptr, sc.local_tbn, sc.sample_tbn, units,
                                     rpu);
    int rc = check_launch("curved_light_import_infer(lookup)");
    if (rc != NERFTEX_OK) return rc;
    if ((rc = ffmlp_inference_rows(sc.xin, d->sigma_weights, B, 48, 32, 2, sc.h, units, rpu, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_light_import_infer(mid)", "curved_light_import_infer(out)"};
    return curved_light_back_half<2>(d, r, sc.h, sc.xin, sc.n_lbc, sc.normal, sc.local_tbn, sc.sample_tbn, nullptr, sc.mask, sc.back, labels, stream);
}
