// The curved field's no-grad forward over features baked onto the vertices of a fine mesh as one device-count call (nerftex_curved_unhash_infer):
// MeshFeatureField.forward's `imported_type == 'unhash'` branch (tools/map.py:708-714) -- neighbour search over the field's OWN mesh -> vertex lookup
// over the FINE mesh's BVH (raytracer.hip) -> the shared back half.  Host code only; included by fieldglue.hip behind planar.inc.

namespace nerftex {
namespace {

// the scratch of one nerftex_curved_unhash_infer call: the shape chain's buffers (neighbour list, mask, normal, xin, h) and the back half's
struct UnhashScratch {
    ScratchCarver carve;
    ShapeFront f;
    CurvedBack back;
    UnhashScratch(void* scratch, size_t B) : carve{reinterpret_cast<uintptr_t>(scratch), B}, f(carve), back(carve) {}
};

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_unhash_infer_scratch_bytes(uint32_t B) { return UnhashScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_unhash_infer(const nerftex_curved_unhash_infer_desc* d, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_unhash_infer")) return NERFTEX_ERR_INVALID;  // NULL descriptor, B % 128, n_verts, K
    if (d->n_features != 16 || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 || d->sigma_out != 16 || !back_shapes_ok(d)) {
        set_error("curved_unhash_infer: the kernels serve the default curved field only (16 features per vertex, sigma net 48 -> 32 x 2 -> 16, "
                  "colour net 32 -> 64 x 3 -> 3)");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->tracer || d->n_faces != raytracer_triangles(d->tracer)) {
        set_error("curved_unhash_infer: a raytracer over the fine mesh is required and face_vertices must hold its %u faces, but got %u",
                  raytracer_triangles(d->tracer), d->n_faces);
        return NERFTEX_ERR_INVALID;
    }
    const UnhashScratch sc(d->scratch, d->B);
    const VertexLookup s{d->face_vertices, d->vertex_features, d->n_fine_verts, d->dir_vec_wdist, d->sdf_scale, d->sdf_offset, d->h_threshold, d->n_freqs, sc.f.xin};
    if (const char* why = vertex_lookup_refusal(s)) {
        set_error("curved_unhash_infer: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    if (!d->knn || !d->xyz || !d->dirs || !d->mesh_vertices || !d->vertex_normals || !d->fine_vertices || !d->face_vertices || !d->vertex_features ||
        !d->sigma_weights || !d->color_weights || !d->sigma || !d->rgbs || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) ||
        d->scratch_bytes < sc.carve.at) {
        set_error("curved_unhash_infer: handles, inputs, both meshes' arrays, face_vertices, vertex_features, weights and outputs must not be NULL, and scratch "
                  "must be 256-byte aligned and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->sigma_weights) || !aligned16(d->color_weights)) {
        set_error("curved_unhash_infer: the weight vectors must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    int rc = knn_query_rows(d->knn, d->xyz, d->dirs, d->B, d->K, sc.f.idx, sc.f.dist, d->units_dev, d->rows_per_unit, st);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = curved_vertex_rows(d->tracer, d->xyz, d->dirs, sc.f.idx, sc.f.dist, d->B, d->K, d->mesh_vertices, d->vertex_normals, d->n_verts, s, sc.f.mask,
                                 sc.f.normal, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK)
        return rc;
    if ((rc = ffmlp_inference_rows(sc.f.xin, d->sigma_weights, d->B, 48, 32, 2, sc.f.h, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_unhash_infer(mid)", "curved_unhash_infer(out)"};
    return curved_back_half(d, sc.f.h, sc.f.normal, sc.f.mask, sc.back, labels, stream);
}
