// The curved field's no-grad forward over an imported feature PATCH as one device-count call: nerftex_curved_patch_infer (the static light model) and
// nerftex_curved_light_patch_infer (the SH light model) -- the `imported_type == 'patch'` branch of MeshFeatureField.forward (tools/map.py:676-692,
// :719-730).  Included at the end of fieldglue.hip behind shape_light.inc.  Five launches each: the patch lookup (knn.hip / patch_import.inc: the K = 8
// search and the dual-distance resampling in ONE kernel), then the four launches the import chains already have -- sigma net, then curved_back_half
// or curved_light_back_half<1>.  The lit mid kernel with ONE rotation reads its frame per row from scratch already (the mesh chain's hit-face frame);
// here that buffer holds the lookup's weighted frame, and the half rounding points of DESIGN.md 4.14 are its own: one product, rounded to half.
// DESIGN.md 4.20.

namespace nerftex {
namespace {

// the scratch of one nerftex_curved_light_patch_infer call (the static entry's is planar.inc's ImportScratch: the same buffers)
struct LightPatchScratch {
    ScratchCarver carve;
    uint8_t* mask;
    float* normal;
    half_t *xin, *h, *n_lbc;
    float* tbn;
    LightBack back;
    LightPatchScratch(void* scratch, size_t B)
        : carve{reinterpret_cast<uintptr_t>(scratch), B}, mask(carve.take<uint8_t>(1)), normal(carve.take<float>(3)), xin(carve.take<half_t>(48)),
          h(carve.take<half_t>(16)), n_lbc(carve.take<half_t>(8)), tbn(carve.take<float>(9)), back(carve) {}
};

// the refusal over the patch's point count, which both entries ask right behind the batch (the lookup's own refusals follow the shapes)
template <typename Desc>
bool patch_points_ok(const Desc* d, const char* who) {
    if (!d->knn || d->n_points != knn_points(d->knn) || d->n_points < 8u || d->n_points > 0x7fffffffu) {
        set_error("%s: a neighbour grid over the patch's points is required, n_points must be its point count (%u), and a patch holds between 8 and "
                  "2^31 - 1 points, but got %u", who, knn_points(d->knn), d->n_points);
        return false;
    }
    return true;
}

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_patch_infer_scratch_bytes(uint32_t B) { return ImportScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_patch_infer(const nerftex_curved_patch_infer_desc* d, void* stream) {
    clear_error();
    if (!batch_ok(d, "curved_patch_infer")) return NERFTEX_ERR_INVALID;  // NULL descriptor, B % 128
    if (!patch_points_ok(d, "curved_patch_infer")) return NERFTEX_ERR_INVALID;
    if (d->n_features != 16 || d->n_freqs != kInferFreqs || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 || d->sigma_out != 16 ||
        !back_shapes_ok(d)) {
        set_error("curved_patch_infer: the kernels serve the default curved field only (a patch of 16 features, 12 height bands, "
                  "sigma net 48 -> 32 x 2 -> 16, colour net 32 -> 64 x 3 -> 3)");
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    const ImportScratch sc(d->scratch, d->B);
    if (!d->xyz || !d->dirs || !d->geom || !d->features || !d->sigma_weights || !d->color_weights || !d->sigma || !d->rgbs || !d->scratch ||
        (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < sc.carve.at) {
        set_error("curved_patch_infer: inputs, the patch's records, weights and outputs must not be NULL, and scratch must be 256-byte aligned and hold %zu bytes",
                  sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->sigma_weights) || !aligned16(d->color_weights)) {
        set_error("curved_patch_infer: the weight vectors must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    const PatchLookup s{d->knn, d->geom, d->features, nullptr, d->n_points, d->h_threshold, d->n_freqs, sc.xin};
    if (const char* why = patch_lookup_refusal(s, false)) {  // (what is left of it: alignment of the records, h_threshold)
        set_error("curved_patch_infer: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    int rc = patch_lookup_rows(s, d->xyz, d->dirs, d->B, sc.mask, sc.normal, nullptr, nullptr, d->units_dev, d->rows_per_unit, st);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = ffmlp_inference_rows(sc.xin, d->sigma_weights, d->B, 48, 32, 2, sc.h, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_patch_infer(mid)", "curved_patch_infer(out)"};
    return curved_back_half(d, sc.h, sc.normal, sc.mask, sc.back, labels, stream);
}

extern "C" size_t nerftex_curved_light_patch_infer_scratch_bytes(uint32_t B) { return LightPatchScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_light_patch_infer(const nerftex_curved_light_patch_infer_desc* d, void* stream) { return nerftex_curved_light_patch_infer_relit(d, nullptr, stream); }

extern "C" int nerftex_curved_light_patch_infer_relit(const nerftex_curved_light_patch_infer_desc* d, const nerftex_relight_desc* r, void* stream) {
    clear_error();
    if (!batch_ok(d, "curved_light_patch_infer")) return NERFTEX_ERR_INVALID;
    if (!patch_points_ok(d, "curved_light_patch_infer")) return NERFTEX_ERR_INVALID;
    if (d->n_features != 16 || d->n_phi != 8 || d->n_freqs != kInferFreqs || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 ||
        d->sigma_out != 16 || d->normal_hidden != 16 || d->normal_layers != 2 || d->brdf_in != 16 || d->brdf_hidden != 64 || d->brdf_layers != 3 ||
        d->brdf_out != 5) {
        set_error("curved_light_patch_infer: the kernels serve the default SH-lit curved field only (a patch of 16 features and 8 phi features, 12 height "
                  "bands, sigma net 48 -> 32 x 2 -> 16, normal nets 16 wide with 2 hidden layers, BRDF net 16 -> 64 x 3 -> 5)");
        return NERFTEX_ERR_INVALID;
    }
    if (!light_head_ok(d, "curved_light_patch_infer") || !relight_ok(d, r, "curved_light_patch_infer")) return NERFTEX_ERR_INVALID;
    if (d->B == 0) return NERFTEX_OK;
    const LightPatchScratch sc(d->scratch, d->B);
    if (!d->xyz || !d->dirs || !d->geom || !d->features || !d->lit || !d->sigma_weights || !d->normal_weights || !d->normal_biases || !d->brdf_weights ||
        !d->env_shs || !d->sigma || !d->rgbs || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < sc.carve.at) {
        set_error("curved_light_patch_infer: inputs, the patch's records, weights, lighting and outputs must not be NULL, and scratch must be 256-byte aligned "
                  "and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->sigma_weights) || !aligned16(d->brdf_weights) ||
        ((reinterpret_cast<uintptr_t>(d->normal_weights) | reinterpret_cast<uintptr_t>(d->normal_biases)) & 3)) {
        set_error("curved_light_patch_infer: the MLP weight vectors must be 16-byte aligned, the normal net's block 4-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    const PatchLookup s{d->knn, d->geom, d->features, d->lit, d->n_points, d->h_threshold, d->n_freqs, sc.xin};
    if (const char* why = patch_lookup_refusal(s, true)) {
        set_error("curved_light_patch_infer: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    int rc = patch_lookup_rows(s, d->xyz, d->dirs, B, sc.mask, sc.normal, sc.n_lbc, sc.tbn, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = ffmlp_inference_rows(sc.xin, d->sigma_weights, B, 48, 32, 2, sc.h, units, rpu, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_light_patch_infer(mid)", "curved_light_patch_infer(out)"};
    return curved_light_back_half<1>(d, r, sc.h, sc.xin, sc.n_lbc, sc.normal, sc.tbn, nullptr, nullptr, sc.mask, sc.back, labels, stream);
}
