// The launches of nerftex_curved_field_infer (fieldglue.hip) that live beside the kernels they share their arithmetic with: the
// device-count ("rows") forms of the neighbour search (knn.hip), the projector (raytracer.hip) and the FFMLP inference kernel (ffmlp.hip).
// Every one of them evaluates live = min(B, units_dev[0] * unit_rows(rows_per_unit, units_dev[0])) from the same device word, does nothing
// for rows >= live and -- search and projector -- nothing but a few constant stores for the slots nerftex_march_rays_dev marked unused.
// Not part of the C ABI: they enqueue on `st`, allocate nothing and clear no error text (the entry point did).
#pragma once

#include "common.hpp"

namespace nerftex {

// idx [N,K] int32, dist [N,K]: the rows of nerftex_knn_query for unmarked live rows, nothing written for the others
int knn_query_rows(const nerftex_knn* kn, const float* xyz, const float* dirs, uint32_t N, uint32_t K, int32_t* idx, float* dist,
                   const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

// nerftex_curved_project with n_freqs = 12 for unmarked live rows: p_sur [N,3], h_mask [N], normal [N,3], and half(z_embed) followed by the
// seven padding ones straight into columns 16..47 of the sigma net's input xin [N,48] (what nerftex_curved_pack_inputs builds from z_embed;
// height_ladder.hpp: the one ladder the planar lookup of an imported map, planar.inc, writes too).
// A marked live row: p_sur = 1e30 (the gather answers zeros without a table read), h_mask = 0, normal = 0, z = 0 | ones.
// tbn_out [N,9] (optional, with the per-face frames tbn [F,9]): the hit face's frame as nerftex_curved_project writes it, zeros for a marked
// row; NULL: no frame is read or written (the static light model's chain).
int curved_project_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                        uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, float dir_vec_wdist, float h_threshold,
                        float* p_sur, uint8_t* h_mask, float* normal, void* xin, const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st,
                        const float* tbn = nullptr, float* tbn_out = nullptr);

// The shape lookup (raytracer.hip: an imported map on a new UV-mapped mesh) -- what nerftex_shape_lookup and nerftex_curved_shape_infer hand it alike.
struct ShapeLookup {
    const float* face_uv;  // [F,6]
    const float* map;      // [map_h, map_w, 16] fp32
    uint32_t map_h, map_w;
    float sdf_scale, sdf_offset, uv_rate, h_threshold;
    uint32_t n_freqs;
    void* xin;             // [N,48] half
};
uint32_t raytracer_triangles(const nerftex_raytracer* rt);
// NULL, or why the two entries refuse these values -- in the order include/nerftex_hip.h documents: map extents, n_freqs, alignment of the map and
// of xin, scales and threshold, offset
const char* shape_lookup_refusal(const ShapeLookup& s);
// nerftex_shape_lookup's rows for unmarked live rows: mask [N], the raw coarse normal [N,3], and the whole sigma-net input row xin [N,48] =
// [half(features) | half(ladder) | ones].  A marked live row, or one whose normal is not finite: mask = 0, normal = 0, features 0, z = 0 | ones;
// nothing is traced and no texel read.  The caller has validated (front_batch_ok's K and n_verts, n_faces, shape_lookup_refusal).
int curved_shape_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                      const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const ShapeLookup& s, uint8_t* mask, float* normal,
                      const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

// The lit shape lookup (raytracer.hip: the same lookup under the SH light model) -- what nerftex_shape_light_lookup and
// nerftex_curved_light_shape_infer hand it beside a ShapeLookup.
struct ShapeLight {
    const float* phi_map;         // [map_h, map_w, 8] fp32
    const float* frame_map;       // [map_h, map_w, 12] fp32
    const float* sample_tbn_inv;  // [n_patches, 12] fp32
    uint32_t n_patches;
    const float* face_tbn;        // [n_tbn_faces, 12] fp32, by original face id
    uint32_t n_tbn_faces;
    void* phi;                    // rows form: half [4,N,2]; plain form: fp32 [N,8]
    float *local_tbn, *sample_tbn, *new_tbn;  // [N,9] each
};
// NULL, or why the two entries refuse these values -- in the order include/nerftex_hip.h documents: n_patches, a NULL pointer, alignment of the
// maps, the frames and phi, then a face_tbn that does not hold the tracer's n_triangles faces
const char* shape_light_refusal(const ShapeLight& t, uint32_t n_triangles);
// curved_shape_rows plus the lit reads for unmarked live rows: phi (half, level-major), local_tbn, sample_tbn and new_tbn.  A marked live row,
// or one whose normal is not finite, reads no face, UV, frame or texel and writes zeros for all four on top of curved_shape_rows' constants.
int curved_shape_light_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                            uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const ShapeLookup& s, const ShapeLight& t,
                            uint8_t* mask, float* normal, const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

// The vertex lookup (raytracer.hip: the field baked onto the vertices of a fine mesh) -- what nerftex_vertex_lookup and
// nerftex_curved_unhash_infer hand it alike.
struct VertexLookup {
    const int32_t* face_vertices;  // [n_faces,3] corner vertex ids by original face id
    const float* features;         // [n_fine_verts,16] fp32
    uint32_t n_fine_verts;
    float dir_vec_wdist, sdf_scale, sdf_offset, h_threshold;
    uint32_t n_freqs;
    void* xin;                     // [N,48] half
};
// NULL, or why the two entries refuse these values -- in the order include/nerftex_hip.h documents: the fine vertex count, n_freqs, alignment of the
// features and of xin, scale and threshold, offset
const char* vertex_lookup_refusal(const VertexLookup& s);
// nerftex_vertex_lookup's rows for unmarked live rows: mask [N], the raw coarse normal [N,3], and the whole sigma-net input row xin [N,48] =
// [half(features) | half(ladder) | ones].  A marked live row: mask = 0, normal = 0, features 0, z = 0 | ones; nothing is traced and no row read.
// The caller has validated (front_batch_ok's K and n_verts, n_faces, vertex_lookup_refusal).
int curved_vertex_rows(const nerftex_raytracer* rt_fine, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                       const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const VertexLookup& s, uint8_t* mask, float* normal,
                       const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

// The patch lookup (knn.hip / patch_import.inc: an imported feature patch resampled from its 8 nearest points) -- what the two plain entries and
// nerftex_curved_patch_infer / nerftex_curved_light_patch_infer (patch_chain.inc) hand it alike.
struct PatchLookup {
    const nerftex_knn* knn;  // the neighbour grid over the patch's points
    const float* geom;       // [n_points, 8] fp32
    const float* features;   // [n_points, 16] fp32
    const float* lit;        // [n_points, 20] fp32 (the lit forms)
    uint32_t n_points;
    float h_threshold;
    uint32_t n_freqs;
    void* xin;               // [N,48] half
};
uint32_t knn_points(const nerftex_knn* kn);
// NULL, or why the entries refuse these values -- in the order include/nerftex_hip.h documents: the grid and the point count, n_freqs, a NULL record
// array, alignment of the records and of xin, h_threshold
const char* patch_lookup_refusal(const PatchLookup& s, bool lit);
// the lookup's rows for unmarked live rows: mask [N], the raw coarse normal [N,3], the whole sigma-net input row xin [N,48] and -- n_lbc not NULL: the
// lit form -- phi as half, level-major [4,N,2], and the weighted frame tbn [N,9].  A marked live row: mask = 0, normal = 0, features 0, z = 0 | ones;
// nothing is searched or gathered, phi and tbn are not written.  The caller has validated (patch_lookup_refusal).
int patch_lookup_rows(const PatchLookup& s, const float* xyz, const float* dirs, uint32_t N, uint8_t* mask, float* normal, void* n_lbc, float* tbn,
                      const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

// The scan launch of nerftex_patch_front (raytracer.hip / patch_export.inc; the kernel sits beside the neighbour search in knn.hip): for the
// chunk's pre-lift origins [B, S2, 3], stats[4 b + 2] = max(stats[4 b + 2], bits of the patch's largest nearest-scan-point distance).
int patch_scan(const nerftex_knn* scan, const float* origins, uint32_t B, uint32_t S2, uint32_t* stats, hipStream_t st);

// nerftex_ffmlp_inference (fp16, ReLU, no output activation) of the curved field's networks -- (IN, H, NL) = (48, 32, 2), (32, 64, 3) or the SH
// light head's BRDF net (16, 64, 3) -- over the 128-row workgroups that hold a live row; a workgroup wholly past the live rows exits before it
// stages its weights.
int ffmlp_inference_rows(const void* inputs, const void* weights, uint32_t B, uint32_t IN, uint32_t H, uint32_t NL, void* outputs,
                         const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st);

}  // namespace nerftex
