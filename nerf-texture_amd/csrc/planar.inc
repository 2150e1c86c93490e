// The planar lookup of an imported feature map (nerftex_planar_lookup) and the curved field's no-grad forward over it as one device-count call
// (nerftex_curved_import_infer): MeshFeatureField.forward's `imported_type == 'field'` branch (tools/map.py:646-668) -- an O(1) bilinear read of a
// [H, W, 16] fp32 image on the xy plane where the mesh chain searches neighbours, traces twice and gathers a hash table.  Included by fieldglue.hip
// in FRONT of shlight.inc (whose file-scope pragma holds for everything behind it); the kernel switches contraction off itself.

namespace nerftex {
namespace {

struct PlanarArgs {
    const float* map;  // [H, W, 16] fp32, channel-last, 16-byte aligned
    uint32_t H, W;
    int divide;          // 0: u = x0 * plane0, v = x1 * plane1;  1: u = x0 / plane0, v = x1 / plane1 (true divisions)
    float plane0, plane1;
    float height0, height1;  // sdf = (x2 * height0) * height1 - offset
    float offset, h_threshold;
};

// One thread per row: the four corners' 64 bytes each as four 16-byte loads, 16 independent loads in flight, two 16-byte stores of features.  (Four
// adjacent lanes per row, one quarter of each corner per lane, measured no faster -- DESIGN.md 4.15 -- and was removed.)
// ROWS: the rows contract of nerftex_curved_field_infer's kernels (writes the raw normal (0, 0, 1) for the mid kernel); otherwise the plain form
// (every row, writes p_uv and sdf).  Both write mask [B] and the sigma net's input row xin [B,48] = [half(features) | half(ladder) | ones].
// One row of the lookup: everything the two kernels below and the lit lookup (planar_light.inc) write alike -- one expression tree, so the same
// bits wherever it is called.  -> false: this thread is done (past the live rows, or a marked slot whose zeros are written); true: b, u, v are
// the row and the map coordinates of a row that reads its texels.
template <bool ROWS>
__device__ __forceinline__ bool planar_lookup_row(const float* __restrict__ xyz, const float* __restrict__ dirs, const uint32_t B, const PlanarArgs& a,
                                                  float* __restrict__ p_uv, float* __restrict__ sdf_out, uint8_t* __restrict__ mask, float* __restrict__ normal,
                                                  half_t* __restrict__ xin, const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit, uint32_t& b,
                                                  float& u, float& v) {
#pragma clang fp contract(off)  // every framework op rounds on its own
    b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (ROWS ? live_rows(B, units_dev, rows_per_unit) : B)) return false;
    half_t* row = xin + (size_t)b * 48;
    if (ROWS && slot_unused(dirs, b)) {  // no texel is read
        mask[b] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) normal[(size_t)b * 3 + c] = 0.0f;
        const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        reinterpret_cast<half8_t*>(row)[0] = zero;
        reinterpret_cast<half8_t*>(row)[1] = zero;
        write_unused_ladder(row);
        return false;
    }
    const float x0 = xyz[(size_t)b * 3], x1 = xyz[(size_t)b * 3 + 1], x2 = xyz[(size_t)b * 3 + 2];
    u = a.divide ? x0 / a.plane0 : x0 * a.plane0;
    v = a.divide ? x1 / a.plane1 : x1 * a.plane1;
    const float sdf = (x2 * a.height0) * a.height1 - a.offset;
    mask[b] = (fabsf(sdf) < a.h_threshold && u >= -1.0f && u <= 1.0f && v >= -1.0f && v <= 1.0f) ? 1 : 0;
    if (ROWS) {
        normal[(size_t)b * 3] = 0.0f; normal[(size_t)b * 3 + 1] = 0.0f; normal[(size_t)b * 3 + 2] = 1.0f;
    } else {
        p_uv[(size_t)b * 2] = u; p_uv[(size_t)b * 2 + 1] = v;
        sdf_out[b] = sdf;
    }
    // grid_sample(bilinear, align_corners=True, padding zeros); u runs along the map's first axis (bilinear_read.hpp: the shape lookup's read, too)
    half4_t o[4];
    bilinear_read(a.map, a.H, a.W, u, v, o);
    store_features(o, row);
    write_height_ladder(sdf, row);
    return true;
}

template <bool ROWS>
__global__ __launch_bounds__(256) void planar_lookup_rows_kernel(const float* __restrict__ xyz, const float* __restrict__ dirs, const uint32_t B, const PlanarArgs a,
                                                                 float* __restrict__ p_uv, float* __restrict__ sdf_out, uint8_t* __restrict__ mask,
                                                                 float* __restrict__ normal, half_t* __restrict__ xin, const int32_t* __restrict__ units_dev,
                                                                 const uint32_t rows_per_unit) {
    uint32_t b;
    float u, v;
    planar_lookup_row<ROWS>(xyz, dirs, B, a, p_uv, sdf_out, mask, normal, xin, units_dev, rows_per_unit, b, u, v);
}

template <bool ROWS>
void launch_planar_lookup(hipStream_t st, const float* xyz, const float* dirs, uint32_t B, const PlanarArgs& a, float* p_uv, float* sdf, uint8_t* mask,
                          float* normal, half_t* xin, const int32_t* units_dev, uint32_t rows_per_unit) {
    KernelTimer kt("planar_lookup_rows_kernel", st);
    hipLaunchKernelGGL(planar_lookup_rows_kernel<ROWS>, dim3(div_up(B, 256u)), dim3(256), 0, st, xyz, dirs, B, a, p_uv, sdf, mask, normal, xin, units_dev, rows_per_unit);
}

// (no message: each entry names what it refuses)
inline bool planar_scales_ok(uint32_t mode, float p0, float p1, float h0, float h1, float offset, float h_threshold) {
    auto pos = [](float v) { return v > 0.0f && std::isfinite(v); };
    return mode <= 1u && pos(p0) && pos(p1) && pos(h0) && pos(h1) && pos(h_threshold) && std::isfinite(offset);
}

// The refusal of a map's extent, for the two planar lookups and the two import entries (planar_light.inc: `maps` = the lit ones, which read several).
inline bool map_extent_ok(const char* who, bool maps, uint32_t map_h, uint32_t map_w) {
    if (map_h == 0 || map_h > 16384u || map_w == 0 || map_w > 16384u) {
        set_error("%s: the %s between 1 and 16384 texels along each axis, but got %u x %u", who, maps ? "maps need" : "map needs", map_h, map_w);
        return false;
    }
    return true;
}

// the scratch of one nerftex_curved_import_infer call
struct ImportScratch {
    ScratchCarver carve;
    uint8_t* mask;
    float* normal;
    half_t *xin, *h;
    CurvedBack back;
    ImportScratch(void* scratch, size_t B)
        : carve{reinterpret_cast<uintptr_t>(scratch), B}, mask(carve.take<uint8_t>(1)), normal(carve.take<float>(3)), xin(carve.take<half_t>(48)),
          h(carve.take<half_t>(16)), back(carve) {}
};

}  // namespace
}  // namespace nerftex

extern "C" int nerftex_planar_lookup(const float* xyz, const float* map, uint32_t map_h, uint32_t map_w, uint32_t mode, float plane_scale0, float plane_scale1,
                                     float height_scale0, float height_scale1, float sdf_offset, float h_threshold, uint32_t n_freqs, uint32_t B, float* p_uv,
                                     float* sdf, uint8_t* mask, void* xin, void* stream) {
    clear_error();
    if (n_freqs != kInferFreqs) {
        set_error("planar_lookup: the kernel writes the curved field's 12 height bands, but got n_freqs = %u", n_freqs);
        return NERFTEX_ERR_INVALID;
    }
    if (!map_extent_ok("planar_lookup", false, map_h, map_w)) return NERFTEX_ERR_INVALID;
    if (B == 0) return NERFTEX_OK;
    if (!xyz || !map || !p_uv || !sdf || !mask || !xin || !aligned16(map) || !aligned16(xin)) {
        set_error("planar_lookup: inputs, map and outputs must not be NULL, and the map and xin must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    if (!planar_scales_ok(mode, plane_scale0, plane_scale1, height_scale0, height_scale1, sdf_offset, h_threshold)) {
        set_error("planar_lookup: mode is NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE, the scales and h_threshold positive and finite, sdf_offset finite");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const PlanarArgs a{map, map_h, map_w, (int)mode, plane_scale0, plane_scale1, height_scale0, height_scale1, sdf_offset, h_threshold};
    launch_planar_lookup<false>(st, xyz, nullptr, B, a, p_uv, sdf, mask, nullptr, static_cast<half_t*>(xin), nullptr, 0u);
    return check_launch("planar_lookup");
}

extern "C" size_t nerftex_curved_import_infer_scratch_bytes(uint32_t B) { return ImportScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_import_infer(const nerftex_curved_import_infer_desc* d, void* stream) {
    clear_error();
    if (!batch_ok(d, "curved_import_infer")) return NERFTEX_ERR_INVALID;
    if (d->n_features != 16 || d->n_freqs != kInferFreqs || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 || d->sigma_out != 16 ||
        !back_shapes_ok(d)) {
        set_error("curved_import_infer: the kernels serve the default curved field only (a map of 16 features, 12 height bands, "
                  "sigma net 48 -> 32 x 2 -> 16, colour net 32 -> 64 x 3 -> 3)");
        return NERFTEX_ERR_INVALID;
    }
    if (!map_extent_ok("curved_import_infer", false, d->map_h, d->map_w)) return NERFTEX_ERR_INVALID;
    if (d->B == 0) return NERFTEX_OK;
    const ImportScratch sc(d->scratch, d->B);
    if (!d->xyz || !d->dirs || !d->map || !d->sigma_weights || !d->color_weights || !d->sigma || !d->rgbs || !d->scratch ||
        (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < sc.carve.at) {
        set_error("curved_import_infer: inputs, map, weights and outputs must not be NULL, and scratch must be 256-byte aligned and hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->map) || !aligned16(d->sigma_weights) || !aligned16(d->color_weights)) {
        set_error("curved_import_infer: the map and the weight vectors must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    if (!planar_scales_ok(d->mode, d->plane_scale0, d->plane_scale1, d->height_scale0, d->height_scale1, d->sdf_offset, d->h_threshold)) {
        set_error("curved_import_infer: mode is NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE, the scales and h_threshold positive and finite, sdf_offset finite");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const PlanarArgs a{d->map, d->map_h, d->map_w, (int)d->mode, d->plane_scale0, d->plane_scale1, d->height_scale0, d->height_scale1, d->sdf_offset, d->h_threshold};
    launch_planar_lookup<true>(st, d->xyz, d->dirs, d->B, a, nullptr, nullptr, sc.mask, sc.normal, sc.xin, d->units_dev, d->rows_per_unit);
    int rc = check_launch("curved_import_infer(lookup)");
    if (rc != NERFTEX_OK) return rc;
    if ((rc = ffmlp_inference_rows(sc.xin, d->sigma_weights, d->B, 48, 32, 2, sc.h, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_import_infer(mid)", "curved_import_infer(out)"};
    return curved_back_half(d, sc.h, sc.normal, sc.mask, sc.back, labels, stream);
}


// ---- the same map on a new UV-mapped mesh (nerftex_curved_shape_infer): neighbour search -> shape lookup (raytracer.hip) -> the shared back half --------
namespace nerftex {
namespace {

// the scratch of one nerftex_curved_shape_infer call
struct ShapeScratch {
    ScratchCarver carve;
    ShapeFront f;
    CurvedBack back;
    ShapeScratch(void* scratch, size_t B) : carve{reinterpret_cast<uintptr_t>(scratch), B}, f(carve), back(carve) {}
};

}  // namespace
}  // namespace nerftex

extern "C" size_t nerftex_curved_shape_infer_scratch_bytes(uint32_t B) { return ShapeScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_shape_infer(const nerftex_curved_shape_infer_desc* d, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_shape_infer")) return NERFTEX_ERR_INVALID;  // NULL descriptor, B % 128, n_verts, K
    if (d->n_features != 16 || d->sigma_in != 48 || d->sigma_hidden != 32 || d->sigma_layers != 2 || d->sigma_out != 16 || !back_shapes_ok(d)) {
        set_error("curved_shape_infer: the kernels serve the default curved field only (a map of 16 features, sigma net 48 -> 32 x 2 -> 16, "
                  "colour net 32 -> 64 x 3 -> 3)");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->tracer || d->n_faces != raytracer_triangles(d->tracer)) {
        set_error("curved_shape_infer: a raytracer is required and face_uv must hold its %u faces, but got %u", raytracer_triangles(d->tracer), d->n_faces);
        return NERFTEX_ERR_INVALID;
    }
    const ShapeScratch sc(d->scratch, d->B);
    const ShapeLookup s{d->face_uv, d->map, d->map_h, d->map_w, d->sdf_scale, d->sdf_offset, d->uv_rate, d->h_threshold, d->n_freqs, sc.f.xin};
    if (const char* why = shape_lookup_refusal(s)) {
        set_error("curved_shape_infer: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    if (!d->knn || !d->xyz || !d->dirs || !d->mesh_vertices || !d->vertex_normals || !d->face_uv || !d->map || !d->sigma_weights || !d->color_weights || !d->sigma ||
        !d->rgbs || !d->scratch || (reinterpret_cast<uintptr_t>(d->scratch) & 255) || d->scratch_bytes < sc.carve.at) {
        set_error("curved_shape_infer: handles, inputs, mesh arrays, face_uv, map, weights and outputs must not be NULL, and scratch must be 256-byte aligned and "
                  "hold %zu bytes", sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!aligned16(d->sigma_weights) || !aligned16(d->color_weights)) {
        set_error("curved_shape_infer: the weight vectors must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    int rc = knn_query_rows(d->knn, d->xyz, d->dirs, d->B, d->K, sc.f.idx, sc.f.dist, d->units_dev, d->rows_per_unit, st);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = curved_shape_rows(d->tracer, d->xyz, d->dirs, sc.f.idx, sc.f.dist, d->B, d->K, d->mesh_vertices, d->vertex_normals, d->n_verts, s, sc.f.mask,
                                sc.f.normal, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK)
        return rc;
    if ((rc = ffmlp_inference_rows(sc.f.xin, d->sigma_weights, d->B, 48, 32, 2, sc.f.h, d->units_dev, d->rows_per_unit, st)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_shape_infer(mid)", "curved_shape_infer(out)"};
    return curved_back_half(d, sc.f.h, sc.f.normal, sc.f.mask, sc.back, labels, stream);
}
