// The imported maps on a NEW UV-mapped mesh under the SH light model: the `pred_normal` part of the 'shape' branch of MeshFeatureField.forward
// (tools/map.py:693-707, :722-730) as one device-count call (nerftex_curved_light_shape_infer).  Included at the end of fieldglue.hip behind
// planar_light.inc: the neighbour search is knn.hip's, the lit shape lookup raytracer.hip's (shape_lookup_kernel<ROWS, LIT>, the lit reads of
// lit_reads.hpp), the head's refusals and the closing sequence (the mid kernel with all three frames, the BRDF net, the closing kernel:
// curved_light_back_half) curved_light.inc's.
// DESIGN.md 4.18.

namespace nerftex {
namespace {

// the scratch of one nerftex_curved_light_shape_infer call
struct LightShapeScratch {
    ScratchCarver carve;
    ShapeFront f;  // (fieldglue.hip: what nerftex_curved_shape_infer's scratch leads with, too)
    half_t* n_lbc;
    float *local_tbn, *sample_tbn, *new_tbn;
    LightBack back;
    LightShapeScratch(void* scratch, size_t B)
        : carve{reinterpret_cast<uintptr_t>(scratch), B}, f(carve), n_lbc(carve.take<half_t>(8)), local_tbn(carve.take<float>(9)),
          sample_tbn(carve.take<float>(9)), new_tbn(carve.take<float>(9)), back(carve) {}
};

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_light_shape_infer_scratch_bytes(uint32_t B) { return LightShapeScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_light_shape_infer(const nerftex_curved_light_shape_infer_desc* d, void* stream) { return nerftex_curved_light_shape_infer_relit(d, nullptr, stream); }

extern "C" int nerftex_curved_light_shape_infer_relit(const nerftex_curved_light_shape_infer_desc* d, const nerftex_relight_desc* r, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_light_shape_infer")) return NERFTEX_ERR_INVALID;  // NULL descriptor, B % 128, n_verts, K
    if (d->n_features != 16 || d->n_phi != 8 || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 || d->sigma_out != 16 ||
        d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 || d->brdf_hidden != 64 || d->brdf_layers != 3 || d->brdf_out != 5) {
        set_error("curved_light_shape_infer: the kernels serve the default SH-lit curved field only (a map of 16 features, a phi map of 8, sigma net "
                  "48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (!light_head_ok(d, "curved_light_shape_infer") || !relight_ok(d, r, "curved_light_shape_infer")) return NERFTEX_ERR_INVALID;
    if (!d->tracer || d->n_faces != raytracer_triangles(d->tracer)) {
        set_error("curved_light_shape_infer: a raytracer is required and face_uv must hold its %u faces, but got %u", raytracer_triangles(d->tracer), d->n_faces);
        return NERFTEX_ERR_INVALID;
    }
    const LightShapeScratch sc(d->scratch, d->B);
    const ShapeLookup s{d->face_uv, d->map, d->map_h, d->map_w, d->sdf_scale, d->sdf_offset, d->uv_rate, d->h_threshold, d->n_freqs, sc.f.xin};
    if (const char* why = shape_lookup_refusal(s)) {
        set_error("curved_light_shape_infer: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_patches == 0 || d->n_patches > (1u << 24)) {
        set_error("curved_light_shape_infer: between 1 and 2^24 patch frames (an id is read from an fp32 texel), but got %u", d->n_patches);
        return NERFTEX_ERR_INVALID;
    }
    if (d->n_tbn_faces != d->n_faces) {
        set_error("curved_light_shape_infer: face_tbn must hold the raytracer's %u faces, but got %u", d->n_faces, d->n_tbn_faces);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    if (!d->knn || !d->xyz || !d->dirs || !d->mesh_vertices || !d->vertex_normals || !d->face_uv || !d->face_tbn || !d->map || !d->phi_map || !d->frame_map ||
        !d->sample_tbn_inv || !d->sigma_weights || !d->normal_weights || !d->normal_biases || !d->brdf_weights || !d->env_shs || !d->sigma || !d->rgbs ||
        !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < sc.carve.at) {
        set_error("curved_light_shape_infer: handles, inputs, mesh arrays, face_uv, face_tbn, maps, patch frames, weights, lighting and outputs must not be "
                  "NULL, and scratch must be 256-byte aligned and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->phi_map) || !aligned16(d->frame_map) || !aligned16(d->sample_tbn_inv) || !aligned16(d->face_tbn) || !aligned16(d->sigma_weights) ||
        !aligned16(d->brdf_weights) || ((reinterpret_cast<uintptr_t>(d->normal_weights) | reinterpret_cast<uintptr_t>(d->normal_biases)) & 3)) {
        set_error("curved_light_shape_infer: the lit maps, the patch frames, the face frames and the MLP weight vectors must be 16-byte aligned, the normal "
                  "net's block 4-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    const ShapeLight t{d->phi_map, d->frame_map, d->sample_tbn_inv, d->n_patches, d->face_tbn, d->n_tbn_faces, sc.n_lbc, sc.local_tbn, sc.sample_tbn, sc.new_tbn};
    int rc = knn_query_rows(d->knn, d->xyz, d->dirs, B, d->K, sc.f.idx, sc.f.dist, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = curved_shape_light_rows(d->tracer, d->xyz, d->dirs, sc.f.idx, sc.f.dist, B, d->K, d->mesh_vertices, d->vertex_normals, d->n_verts, s, t, sc.f.mask,
                                      sc.f.normal, units, rpu, st)) != NERFTEX_OK)
        return rc;
    if ((rc = ffmlp_inference_rows(sc.f.xin, d->sigma_weights, B, 48, 32, 2, sc.f.h, units, rpu, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_light_shape_infer(mid)", "curved_light_shape_infer(out)"};
    return curved_light_back_half<3>(d, r, sc.f.h, sc.f.xin, sc.n_lbc, sc.f.normal, sc.local_tbn, sc.sample_tbn, sc.new_tbn, sc.f.mask, sc.back, labels, stream);
}
