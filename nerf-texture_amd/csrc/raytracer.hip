// Closest-hit ray / triangle-mesh queries for gfx950 (MI355X): host-built BVH-4 + stack traversal kernel.
//
// Replaces the reference's external/RayTracer (src/bvh.cu:527-610 build, :259-302 traversal, :695-721 kernel;
// include/raytracing/triangle.cuh:27-39 triangle test, bounding_box.cuh:151-198 slab test;
// src/raytracer.cu:21-58 the RayTracer object) behind include/nerftex_hip.h.  No Eigen, no pybind:
//   * build (host, C++): triangles {a,b,c,id}; a node with more than 8 triangles gets FOUR children by two
//     rounds of median split (nth_element) on the axis of largest centroid variance; the 4 children of a node
//     are contiguous, so an inner node is (first_child, first_child+4) and a leaf is (-begin-1, -end-1) over
//     the reordered triangle array, 32 B per node -- the layout the reference uses.
//   * trace (device): one thread per ray, 32-entry stack, children visited nearest-first (4-element sorting
//     network) and pruned against the current closest hit.  In the curved-field lookup the rays are
//     incoherent (origin = sample point, direction = +-local normal), so the kernel is latency-bound on the
//     ~1 MiB of L2-resident nodes + triangles; one-wave workgroups spread small batches over the CUs.
// Arithmetic follows oracle/src/orc_raytracer.c expression by expression (explicit fmaf, no other contraction).
#include "bilinear_read.hpp"
#include "common.hpp"
#include "curved_infer.hpp"
#include "height_ladder.hpp"
#include "lit_reads.hpp"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

struct nerftex_raytracer {
    void* nodes = nullptr;      // device, Node[n_nodes]
    void* triangles = nullptr;  // device, Tri[n_triangles] (reordered; .id = original face)
    uint32_t n_nodes = 0, n_triangles = 0;
    uint32_t face0 = 0;  // where original face 0 sits in the reordered array (the shape lookup reads it for a point both traces miss)
    int device = 0;
};

namespace nerftex {
namespace {

constexpr float kMaxDist = 10.0f;  // bvh.cu:36
constexpr uint32_t kLeafSize = 8;  // raytracer.cu:36
constexpr int kStack = 32;

struct Tri {
    float a[3], b[3], c[3];
    int64_t id;
};
static_assert(sizeof(Tri) == 48, "48-byte triangles like the reference");
struct Node {
    float lo[3], hi[3];
    int left, right;
};
static_assert(sizeof(Node) == 32, "32-byte nodes like the reference");

// ---------------------------------------------------------------- host build
inline float centroid(const Tri& t, int axis) { return (t.a[axis] + t.b[axis] + t.c[axis]) / 3.0f; }

void bounds(const Tri* begin, const Tri* end, Node& n) {
    for (int k = 0; k < 3; k++) {
        n.lo[k] = std::numeric_limits<float>::infinity();
        n.hi[k] = -std::numeric_limits<float>::infinity();
    }
    for (const Tri* t = begin; t != end; ++t)
        for (int k = 0; k < 3; k++) {
            n.lo[k] = std::min({n.lo[k], t->a[k], t->b[k], t->c[k]});
            n.hi[k] = std::max({n.hi[k], t->a[k], t->b[k], t->c[k]});
        }
}

// median split of [begin, end) on the axis of largest centroid variance; returns the middle
Tri* split(Tri* begin, Tri* end) {
    const size_t n = (size_t)(end - begin);
    double mean[3] = {0, 0, 0}, var[3] = {0, 0, 0};
    for (Tri* t = begin; t != end; ++t)
        for (int k = 0; k < 3; k++) mean[k] += centroid(*t, k);
    for (int k = 0; k < 3; k++) mean[k] /= (double)n;
    for (Tri* t = begin; t != end; ++t)
        for (int k = 0; k < 3; k++) {
            const double d = centroid(*t, k) - mean[k];
            var[k] += d * d;
        }
    int axis = 0;
    if (var[1] > var[axis]) axis = 1;
    if (var[2] > var[axis]) axis = 2;
    Tri* mid = begin + n / 2;
    std::nth_element(begin, mid, end, [axis](const Tri& x, const Tri& y) { return centroid(x, axis) < centroid(y, axis); });
    return mid;
}

void build_bvh(std::vector<Tri>& tris, std::vector<Node>& nodes) {
    struct Work { int node; Tri* begin; Tri* end; };
    nodes.clear();
    nodes.emplace_back();
    bounds(tris.data(), tris.data() + tris.size(), nodes[0]);
    if (tris.size() <= kLeafSize) {  // degenerate mesh: the root is the only leaf
        nodes[0].left = -1;
        nodes[0].right = -(int)tris.size() - 1;
        return;
    }
    std::vector<Work> stack{{0, tris.data(), tris.data() + tris.size()}};
    while (!stack.empty()) {
        const Work w = stack.back();
        stack.pop_back();
        Tri* m1 = split(w.begin, w.end);
        Tri* m0 = split(w.begin, m1);
        Tri* m2 = split(m1, w.end);
        Tri* cuts[5] = {w.begin, m0, m1, m2, w.end};
        const int first = (int)nodes.size();
        nodes[w.node].left = first;
        nodes[w.node].right = first + 4;
        nodes.resize(nodes.size() + 4);
        for (int c = 0; c < 4; c++) {
            Node& child = nodes[first + c];
            bounds(cuts[c], cuts[c + 1], child);
            const size_t cnt = (size_t)(cuts[c + 1] - cuts[c]);
            if (cnt <= kLeafSize) {
                child.left = -(int)(cuts[c] - tris.data()) - 1;
                child.right = -(int)(cuts[c + 1] - tris.data()) - 1;
            } else {
                stack.push_back({first + c, cuts[c], cuts[c + 1]});
            }
        }
    }
}

// ---------------------------------------------------------------- device traversal
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
    return {fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x))};
}
__device__ __forceinline__ float dot(const V3& a, const V3& b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 load3(const float* p) { return {p[0], p[1], p[2]}; }

// triangle.cuh:27-39: t on hit, 1e6 otherwise
__device__ __forceinline__ float tri_hit(const Tri& tr, const V3& ro, const V3& rd) {
    const V3 a = load3(tr.a);
    const V3 v1v0 = sub(load3(tr.b), a), v2v0 = sub(load3(tr.c), a), rov0 = sub(ro, a);
    const V3 n = cross(v1v0, v2v0);
    const V3 q = cross(rov0, rd);
    const float d = 1.0f / dot(rd, n);
    const float u = d * -dot(q, v2v0);
    const float v = d * dot(q, v1v0);
    float t = d * -dot(n, rov0);
    if (u < 0.0f || u > 1.0f || v < 0.0f || (u + v) > 1.0f || t < 0.0f) t = 1e6f;
    return t;
}

// bounding_box.cuh:151-198: entry distance of the slab test, FLT_MAX on a miss.  The reference divides by the direction six times per
// box; a box test only STEERS the traversal (which nodes are visited, in which order) -- the hit distance comes from the triangle test
// -- so here the three reciprocals are taken once per ray (IEEE divisions: the inf / nan cases of an axis-parallel ray stay what they
// are) and every slab interval is widened by 2^-21 of its ends: whatever the exact-division test accepts or orders in front of the
// current hit, this one does too (a superset of the reference's visits, the same closest hit), at a dozen multiplies and selects per box
// instead of 6 divisions of ~10 instructions each.  (Widening by a FACTOR keeps an infinite end infinite; a subtraction would make it nan.)
__device__ __forceinline__ float box_entry(const Node& n, const V3& o, const V3& rinv) {
    constexpr float kMiss = 3.402823466e+38f, kDown = 1.0f - 4.76837158e-7f, kUp = 1.0f + 4.76837158e-7f;
    auto lower = [](float t) { return t * (t >= 0.0f ? kDown : kUp); };  // towards -inf
    auto upper = [](float t) { return t * (t >= 0.0f ? kUp : kDown); };   // towards +inf
    float tmin = (n.lo[0] - o.x) * rinv.x, tmax = (n.hi[0] - o.x) * rinv.x, s;
    if (tmin > tmax) { s = tmin; tmin = tmax; tmax = s; }
    tmin = lower(tmin); tmax = upper(tmax);
    float tymin = (n.lo[1] - o.y) * rinv.y, tymax = (n.hi[1] - o.y) * rinv.y;
    if (tymin > tymax) { s = tymin; tymin = tymax; tymax = s; }
    tymin = lower(tymin); tymax = upper(tymax);
    if (tmin > tymax || tymin > tmax) return kMiss;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (n.lo[2] - o.z) * rinv.z, tzmax = (n.hi[2] - o.z) * rinv.z;
    if (tzmin > tzmax) { s = tzmin; tzmin = tzmax; tzmax = s; }
    tzmin = lower(tzmin); tzmax = upper(tzmax);
    if (tmin > tzmax || tzmin > tmax) return kMiss;
    if (tzmin > tmin) tmin = tzmin;
    return tmin;
}

// closest hit of one ray: returns the distance (kMaxDist on a miss) and the index of the hit triangle in the reordered array (-1)
__device__ __forceinline__ float closest_hit(const V3& ro, const V3& rd, const Node* __restrict__ nodes, const Tri* __restrict__ tris, int& best) {
    int stack[kStack];
    int sp = 0;
    stack[sp++] = 0;
    float mint = kMaxDist;
    best = -1;
    const V3 rinv{1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z};
    while (sp > 0) {
        const Node node = nodes[stack[--sp]];
        if (node.left < 0) {
            const int end = -node.right - 1;
            for (int k = -node.left - 1; k < end; ++k) {
                const float t = tri_hit(tris[k], ro, rd);
                if (t < mint) { mint = t; best = k; }
            }
        } else {
            float dist[4];
            int idx[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                idx[c] = node.left + c;
                dist[c] = box_entry(nodes[idx[c]], ro, rinv);
            }
            // sort descending so that the nearest child is pushed last and popped first (bvh.cu:169-174)
#define NERFTEX_CAS(a, b)                                                                       \
    if (dist[a] < dist[b]) { float td = dist[a]; dist[a] = dist[b]; dist[b] = td; int ti = idx[a]; idx[a] = idx[b]; idx[b] = ti; }
            NERFTEX_CAS(0, 2) NERFTEX_CAS(1, 3) NERFTEX_CAS(0, 1) NERFTEX_CAS(2, 3) NERFTEX_CAS(1, 2)
#undef NERFTEX_CAS
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (dist[c] < mint) stack[sp++] = idx[c];  // cannot overflow: create_raytracer rejects trees deeper than the stack allows
        }
    }
    return mint;
}

__global__ __launch_bounds__(64) void raytrace_kernel(uint32_t N, const float* rays_o, const float* rays_d,
                                                      float* positions, float* normals, float* __restrict__ depth,  // positions/normals may alias rays_o/rays_d (inplace)
                                                      int64_t* __restrict__ face_idx, const Node* __restrict__ nodes,
                                                      const Tri* __restrict__ tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const V3 ro = load3(rays_o + 3 * (size_t)i), rd = load3(rays_d + 3 * (size_t)i);
    int best;
    const float mint = closest_hit(ro, rd, nodes, tris, best);
    depth[i] = mint;
    positions[3 * (size_t)i] = fmaf(mint, rd.x, ro.x);
    positions[3 * (size_t)i + 1] = fmaf(mint, rd.y, ro.y);
    positions[3 * (size_t)i + 2] = fmaf(mint, rd.z, ro.z);
    if (best >= 0) {
        const Tri tr = tris[best];
        const V3 a = load3(tr.a);
        const V3 n = cross(sub(load3(tr.b), a), sub(load3(tr.c), a));
        const float len = sqrtf(dot(n, n));
        normals[3 * (size_t)i] = n.x / len;
        normals[3 * (size_t)i + 1] = n.y / len;
        normals[3 * (size_t)i + 2] = n.z / len;
        face_idx[i] = tr.id;
    } else {
        normals[3 * (size_t)i] = 0.0f;
        normals[3 * (size_t)i + 1] = 0.0f;
        normals[3 * (size_t)i + 2] = 0.0f;
    }
}

// ---------------------------------------------------------------- curved-field projector
// MeshProjector.project of the reference (tools/map.py:414-433) for one sample point per thread, in one kernel:
//   coarse normal from the K nearest mesh vertices (knn(), :454-501, use_dir_vec=True, Shepard weights: the vertex normals and the
//   mean direction to the neighbours, inverse-distance weighted) -> closest hit along +normal and along -normal -> the nearer one is the
//   surface point, its signed distance the height (inside negative) -> |height| < min(9.5, h_threshold) mask, face id, the face's
//   tangent frame, and the frequency encoding of the height that MeshFeatureField.forward feeds its networks (tools/map.py:635,
//   tools/encoding.py:5-43).  The reference runs this as ~35 framework launches + two trace launches and materialises every
//   intermediate ([N,K,3] gathers, two full hit records); the neighbour search itself (frnn, un-vendored) stays outside.
constexpr int kMaxK = 16;
// knn() of tools/map.py:454-501 with its defaults (use_dir_vec=True, Shepard weights): the coarse normal of the point x from its K nearest mesh
// vertices -- their normals and the mean direction to them, inverse-distance weighted.  The one normal of the projector (curved_project_point) and
// of the vertex lookup (vertex_lookup_kernel), whose branch calls the same knn() over the field's own mesh: one expression tree, the same bits.
__device__ __forceinline__ V3 shepard_normal(const V3& x, const uint32_t i, const int32_t* __restrict__ knn_idx, const float* __restrict__ knn_dist, const uint32_t K,
                                             const float* __restrict__ verts, const float* __restrict__ vnormals, const int n_verts, const float dir_vec_wdist) {
    V3 mean_dir{0, 0, 0}, nsum{0, 0, 0}, acc{0, 0, 0};
    float wsum = 0;
    for (uint32_t k = 0; k < K; k++) {
        // a neighbour list from elsewhere may pad with -1 (frnn): the framework's vertex_normals[-1] is the LAST row, so is it here; anything
        // still outside the mesh is clamped -- the loads below must stay inside the two vertex arrays whatever the list holds
        int v = knn_idx[(size_t)i * K + k];
        v = v < 0 ? v + n_verts : v;
        v = min(max(v, 0), n_verts - 1);
        const float dis = knn_dist[(size_t)i * K + k];
        const V3 n = load3(vnormals + 3 * (size_t)v);
        const V3 d = sub(x, load3(verts + 3 * (size_t)v));
        const float dl = sqrtf(dot(d, d)) + 1e-5f;
        const float w = 1.0f / (dis + 1e-7f);
        mean_dir = {fmaf(w, d.x / dl, mean_dir.x), fmaf(w, d.y / dl, mean_dir.y), fmaf(w, d.z / dl, mean_dir.z)};
        nsum = {nsum.x + n.x, nsum.y + n.y, nsum.z + n.z};
        const float nl = sqrtf(dot(n, n)) + 1e-5f;
        acc = {fmaf(w, n.x / nl, acc.x), fmaf(w, n.y / nl, acc.y), fmaf(w, n.z / nl, acc.z)};
        wsum += w;
    }
    if (dot(mean_dir, nsum) < 0) mean_dir = {-mean_dir.x, -mean_dir.y, -mean_dir.z};  // the sign test against mean(normals) = against their sum
    {
        const float ml = sqrtf(dot(mean_dir, mean_dir)) + 1e-5f;
        mean_dir = {mean_dir.x / ml, mean_dir.y / ml, mean_dir.z / ml};
        const float w = 1.0f / (fmaxf(dir_vec_wdist, 1e-5f) + 1e-7f);
        const float nl = sqrtf(dot(mean_dir, mean_dir)) + 1e-5f;
        acc = {fmaf(w, mean_dir.x / nl, acc.x), fmaf(w, mean_dir.y / nl, acc.y), fmaf(w, mean_dir.z / nl, acc.z)};
        wsum += w;
    }
    V3 nrm{acc.x / wsum, acc.y / wsum, acc.z / wsum};
    const float l = sqrtf(dot(nrm, nrm)) + 1e-5f;
    return {nrm.x / l, nrm.y / l, nrm.z / l};
}

// One point of the projector, run by the TWO lanes of a pair (side 0: the trace along +normal, which also writes; side 1: along -normal) -- both
// lanes must arrive here together: the traces meet in an __shfl_xor.
// INFER (nerftex_curved_field_infer): no height, face or frame output, and FreqEncoder(height) leaves as the 16-bit values the sigma net reads --
// z_embed is then the point's row of that net's [N,48] half input, columns 16..40 = half(z), 41..47 = the padding ones.
template <bool INFER>
__device__ __forceinline__ void curved_project_point(const uint32_t i, const uint32_t side, const float* __restrict__ xyz, const int32_t* __restrict__ knn_idx,
                                                     const float* __restrict__ knn_dist, uint32_t K, const float* __restrict__ verts,
                                                     const float* __restrict__ vnormals, int n_verts, float dir_vec_wdist, float h_limit,
                                                     const Node* __restrict__ nodes, const Tri* __restrict__ tris, const float* __restrict__ tbn,
                                                     uint32_t n_freqs, float* __restrict__ p_sur, float* __restrict__ sdf_out, uint8_t* __restrict__ h_mask,
                                                     float* __restrict__ normal_out, int64_t* __restrict__ face_idx, float* __restrict__ tbn_out,
                                                     void* __restrict__ z_embed) {
    const V3 x = load3(xyz + 3 * (size_t)i);
    // ---- knn(): weighted normal (both lanes of a pair: the same loads, served once)
    const V3 nrm = shepard_normal(x, i, knn_idx, knn_dist, K, verts, vnormals, n_verts, dir_vec_wdist);
    // ---- project(): two closest hits, the nearer wins
    const V3 neg{-nrm.x, -nrm.y, -nrm.z};
    int b_mine;
    const float d_mine = closest_hit(x, side ? neg : nrm, nodes, tris, b_mine);
    const float d_other = __shfl_xor(d_mine, 1, kWave);
    const int b_other = __shfl_xor(b_mine, 1, kWave);
    if (side) return;  // lane 0 of the pair (the +normal trace) writes the point's outputs
    const float d1 = d_mine, d2 = d_other;
    const int b1 = b_mine, b2 = b_other;
    const bool inner = d1 < d2;
    const float d = inner ? d1 : d2;
    const V3 dir = inner ? nrm : neg;
    const int best = inner ? b1 : b2;
    const float sdf = inner ? -d1 : d2;
    p_sur[3 * (size_t)i] = fmaf(d, dir.x, x.x);
    p_sur[3 * (size_t)i + 1] = fmaf(d, dir.y, x.y);
    p_sur[3 * (size_t)i + 2] = fmaf(d, dir.z, x.z);
    h_mask[i] = fabsf(sdf) < h_limit ? 1 : 0;
    normal_out[3 * (size_t)i] = nrm.x; normal_out[3 * (size_t)i + 1] = nrm.y; normal_out[3 * (size_t)i + 2] = nrm.z;
    if constexpr (INFER) {
        write_height_ladder(sdf, static_cast<half_t*>(z_embed) + (size_t)i * 48);  // (height_ladder.hpp: the planar lookup's ladder, too)
        if (tbn_out) {  // (the light-model chain: the hit face's frame, as the plain form below)
            const int64_t hit = best >= 0 ? tris[best].id : (int64_t)0;
#pragma unroll
            for (int k = 0; k < 9; k++) tbn_out[9 * (size_t)i + k] = tbn[9 * (size_t)hit + k];
        }
        return;
    }
    sdf_out[i] = sdf;
    const int64_t face = best >= 0 ? tris[best].id : -1;
    face_idx[i] = face;
    if (tbn_out) {
#pragma unroll
        for (int k = 0; k < 9; k++) tbn_out[9 * (size_t)i + k] = tbn[9 * (size_t)(face >= 0 ? face : (int64_t)0) + k];  // face -1 indexes the last row in torch; the mask covers it
    }
    if (z_embed) {  // FreqEncoder(input_dim=1, log sampling): [h, sin(h 2^0), cos(h 2^0), sin(h 2^1), ...]
        float* z = static_cast<float*>(z_embed) + (size_t)i * (1 + 2 * n_freqs);
        z[0] = sdf;
        float f = 1.0f;
        for (uint32_t k = 0; k < n_freqs; k++, f *= 2.0f) {
            z[1 + 2 * k] = sinf(sdf * f);
            z[2 + 2 * k] = cosf(sdf * f);
        }
    }
}

__global__ __launch_bounds__(64) void curved_project_kernel(uint32_t N, const float* __restrict__ xyz, const int32_t* __restrict__ knn_idx,
                                                            const float* __restrict__ knn_dist, uint32_t K, const float* __restrict__ verts,
                                                            const float* __restrict__ vnormals, int n_verts, float dir_vec_wdist, float h_limit,
                                                            const Node* __restrict__ nodes, const Tri* __restrict__ tris,
                                                            const float* __restrict__ tbn, uint32_t n_freqs, float* __restrict__ p_sur,
                                                            float* __restrict__ sdf_out, uint8_t* __restrict__ h_mask, float* __restrict__ normal_out,
                                                            int64_t* __restrict__ face_idx, float* __restrict__ tbn_out, float* __restrict__ z_embed) {
    // TWO lanes per point, one per trace direction: the kernel is bound by the latency of its dependent node loads, and a batch of a few
    // hundred thousand points with two traversals back to back per thread does not even fill the chip's wave slots once
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = tid >> 1, side = tid & 1u;
    if (i >= N) return;  // N odd: the partner of the last point's lane 0 exists (same i), nobody is left alone in a pair
    curved_project_point<false>(i, side, xyz, knn_idx, knn_dist, K, verts, vnormals, n_verts, dir_vec_wdist, h_limit, nodes, tris, tbn, n_freqs, p_sur, sdf_out,
                                h_mask, normal_out, face_idx, tbn_out, z_embed);
}

// the rows form (nerftex_curved_field_infer).  Both tests are on the point index i, which the two lanes of a pair share: a pair leaves, or answers a
// marked slot, or walks the tree TOGETHER -- no lane reaches the __shfl_xor of the traces without its partner.
__global__ __launch_bounds__(64) void curved_project_rows_kernel(uint32_t N, const float* __restrict__ xyz, const float* __restrict__ dirs,
                                                                 const int32_t* __restrict__ knn_idx, const float* __restrict__ knn_dist, uint32_t K,
                                                                 const float* __restrict__ verts, const float* __restrict__ vnormals, int n_verts,
                                                                 float dir_vec_wdist, float h_limit, const Node* __restrict__ nodes, const Tri* __restrict__ tris,
                                                                 float* __restrict__ p_sur, uint8_t* __restrict__ h_mask, float* __restrict__ normal_out,
                                                                 half_t* __restrict__ xin, const int32_t* __restrict__ units_dev, uint32_t rows_per_unit,
                                                                 const float* __restrict__ tbn, float* __restrict__ tbn_out) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = tid >> 1, side = tid & 1u;
    if (i >= live_rows(N, units_dev, rows_per_unit)) return;
    if (slot_unused(dirs, i)) {  // no neighbour list to read, no tree to walk: the constants that make the rest of the chain answer zeros cheaply
        if (side) return;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            p_sur[3 * (size_t)i + c] = 1e30f;  // far outside the box: the gather writes zeros without touching the table
            normal_out[3 * (size_t)i + c] = 0.0f;
        }
        h_mask[i] = 0;
        write_unused_ladder(xin + (size_t)i * 48);
        if (tbn_out) {
#pragma unroll
            for (int k = 0; k < 9; k++) tbn_out[9 * (size_t)i + k] = 0.0f;
        }
        return;
    }
    curved_project_point<true>(i, side, xyz, knn_idx, knn_dist, K, verts, vnormals, n_verts, dir_vec_wdist, h_limit, nodes, tris, tbn, kInferFreqs, p_sur,
                               nullptr, h_mask, normal_out, nullptr, tbn_out, xin);
}

// ---------------------------------------------------------------- shape lookup: an imported map on a new UV-mapped mesh
// The `imported_type == 'shape'` branch of MeshFeatureField.forward (tools/map.py:693-700) for one sample point per PAIR of lanes, in one kernel
// behind the neighbour search: MeshProjector.uvh (:536-543) = knn(use_dir_vec=False, weighting='DualD', nn_consis_check=True) (:454-501) ->
// barycentric_mapping (:503-528: the two traces, the scaled and offset height, the mask that also wants a hit, the hit's barycentric coordinates,
// :85-93) -> per-vertex UVs interpolated, times uv_rate -> the bilinear read of the imported map (bilinear_read.hpp) and FreqEncoder(height).
// Every operation rounds on its own, as a framework op does: plain products and sums, no fused multiply-add -- except the surface point, which
// is the tracer's own o + t d (raytrace_kernel's fmaf).
struct ShapeArgs {
    const float* map;      // [H, W, 16] fp32, 16-byte aligned
    uint32_t H, W;
    const float* face_uv;  // [F, 6]: the three corners' (u, v) of every face
    float sdf_scale, sdf_offset, uv_rate, h_limit;
    uint32_t face0;        // nerftex_raytracer::face0
};

__device__ __forceinline__ float dot_plain(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float norm_plain(const V3& a) { return sqrtf(dot_plain(a, a)); }
__device__ __forceinline__ V3 cross_plain(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// What the LIT form reads and writes beside that (nerftex_shape_light_lookup, nerftex_curved_light_shape_infer: the `pred_normal` part of the
// branch, tools/map.py:702-707, and the hit face's frame, :542): the three maps of lit_reads.hpp at the row's own (u, v), and per-face frames.
struct ShapeLitArgs {
    PlanarLightArgs l;
    const float* face_tbn;  // [F, 12] fp32, 16-byte aligned, indexed by the ORIGINAL face id: the 9 floats of the face's frame, three zeros
    void* phi;              // ROWS: half [4, N, 2], otherwise fp32 [N, 8]
    int32_t* patch_id;      // [N] (plain form only)
    float *local_tbn, *sample_tbn, *new_tbn;  // [N, 9] each
};

// ROWS: the rows contract of nerftex_curved_field_infer's kernels (no p_uv, sdf or face output); otherwise the plain form (every row).
// LIT: the lit reads too (t is not read without it).  Their placement: everything that depends on (u, v) -- the nearest frame read, the patch
// frame that hangs on its id, the phi read -- sits on lane 0 beside the feature read, issued in that order in front of it; the face frame,
// which depends on `best` only and both lanes hold, sits on lane 1 beside the ladder.  No second shuffle: the other placement (u, v handed to
// lane 1 through one more __shfl_xor, the lit reads there) was not measured.
// Lane mapping: the projector's -- lanes 2 i and 2 i + 1 compute the point's normal alike (the same loads, served once), trace along +normal and
// -normal and meet in an __shfl_xor; every exit in front of it is decided by the point, so a pair leaves or stays TOGETHER.  Behind it both lanes
// hold d1, d2 and the tail is split: lane 0 does barycentrics, UV, the four texels and every per-point store, lane 1 the height ladder.
template <bool ROWS, bool LIT = false>
__global__ __launch_bounds__(64) void shape_lookup_kernel(const uint32_t N, const float* __restrict__ xyz, const float* __restrict__ dirs,
                                                          const int32_t* __restrict__ knn_idx, const float* __restrict__ knn_dist, const uint32_t K,
                                                          const float* __restrict__ verts, const float* __restrict__ vnormals, const int n_verts,
                                                          const Node* __restrict__ nodes, const Tri* __restrict__ tris, const ShapeArgs a,
                                                          float* __restrict__ p_uv, float* __restrict__ sdf_out, uint8_t* __restrict__ mask,
                                                          float* __restrict__ normal_out, int64_t* __restrict__ face_idx, half_t* __restrict__ xin,
                                                          const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit, const ShapeLitArgs t) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = tid >> 1, side = tid & 1u;
    if (i >= (ROWS ? live_rows(N, units_dev, rows_per_unit) : N)) return;
    half_t* row = xin + (size_t)i * 48;
    // a marked slot, or a point whose normal is not finite: mask 0 and the constants that make the rest of the chain answer zeros
    auto answer_nothing = [&]() {
        mask[i] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) normal_out[3 * (size_t)i + c] = 0.0f;
        const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        reinterpret_cast<half8_t*>(row)[0] = zero;
        reinterpret_cast<half8_t*>(row)[1] = zero;
        write_unused_ladder(row);
        if constexpr (!ROWS) {
            p_uv[2 * (size_t)i] = 0.0f; p_uv[2 * (size_t)i + 1] = 0.0f;
            sdf_out[i] = 0.0f;
            face_idx[i] = -1;
        }
        if constexpr (LIT) {  // zeros for phi and all three frames (the mid kernel reads them for every unmarked row), patch_id -1 in the plain form
            lit_reads_nothing<ROWS>(i, N, t.phi, t.patch_id, t.local_tbn, t.sample_tbn);
#pragma unroll
            for (int k = 0; k < 9; k++) t.new_tbn[9 * (size_t)i + k] = 0.0f;
        }
    };
    if (ROWS && slot_unused(dirs, i)) {  // no neighbour list to read, no tree to walk, no texel
        if (!side) answer_nothing();
        return;
    }
    const V3 x = load3(xyz + 3 * (size_t)i);
    // ---- knn(use_dir_vec=False, weighting='DualD', nn_consis_check=True): a neighbour on the other side of the point than the nearest one
    // (cos <= 0 between the two directions) is pushed out to 1e5; the index rules are curved_project_point's
    auto vertex_of = [&](uint32_t k) {
        int v = knn_idx[(size_t)i * K + k];
        v = v < 0 ? v + n_verts : v;
        return min(max(v, 0), n_verts - 1);
    };
    float dis[kMaxK];
    V3 dir0{0, 0, 0};
    float dk = -3.402823466e+38f, d1n = 3.402823466e+38f;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxK; k++) {
        dis[k] = 0.0f;
        if (k < K) {
            const V3 d = sub(x, load3(verts + 3 * (size_t)vertex_of(k)));
            const float dl = norm_plain(d) + 1e-5f;
            const V3 dir{d.x / dl, d.y / dl, d.z / dl};
            if (k == 0) dir0 = dir;
            dis[k] = dot_plain(dir, dir0) > 0.0f ? knn_dist[(size_t)i * K + k] : 1e5f;
            dk = fmaxf(dk, dis[k]);
            d1n = fminf(d1n, dis[k]);
        }
    }
    float w[kMaxK];
    float wsum = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxK; k++) {
        w[k] = 0.0f;
        if (k < K) {
            w[k] = (dk - dis[k]) / (dk - d1n + 1e-5f) * (dk + d1n) / (dk + dis[k]);
            wsum = k == 0 ? w[k] : wsum + w[k];
        }
    }
    V3 nrm{0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxK; k++) {
        if (k < K) {
            const V3 n = load3(vnormals + 3 * (size_t)vertex_of(k));
            const float nl = norm_plain(n) + 1e-5f;
            const float wk = w[k] / wsum;  // (no epsilon: 0 / 0 when every kept distance ties, K == 1, or the point sits on its nearest vertex)
            const V3 t{(n.x / nl) * wk, (n.y / nl) * wk, (n.z / nl) * wk};
            nrm = k == 0 ? t : V3{nrm.x + t.x, nrm.y + t.y, nrm.z + t.z};
        }
    }
    {
        const float l = norm_plain(nrm) + 1e-5f;
        nrm = {nrm.x / l, nrm.y / l, nrm.z / l};
    }
    if (!(isfinite(nrm.x) && isfinite(nrm.y) && isfinite(nrm.z))) {  // (the reference carries the NaN into its traces, which miss: here a defined answer)
        if (!side) answer_nothing();
        return;
    }
    // ---- barycentric_mapping(): two closest hits, the nearer wins
    const V3 neg{-nrm.x, -nrm.y, -nrm.z};
    int b_mine;
    const float d_mine = closest_hit(x, side ? neg : nrm, nodes, tris, b_mine);
    const float d_other = __shfl_xor(d_mine, 1, kWave);
    const int b_other = __shfl_xor(b_mine, 1, kWave);
    const float d1 = side ? d_other : d_mine, d2 = side ? d_mine : d_other;
    const bool inner = d1 < d2;
    const float sdf = (inner ? -d1 : d2) / a.sdf_scale - a.sdf_offset;  // (a true division)
    if (side) {  // lane 1: the ladder, columns 16..47
        if constexpr (LIT) {  // ... and new_tbn = tbn[face], face -1 overwritten by 0 (tools/map.py:521, :542): three 16-byte loads, issued in front of the ladder
            const int best1 = inner ? b_other : b_mine;  // (this lane traced -normal: the partner's face is d1's)
            const int64_t id = best1 >= 0 ? tris[(uint32_t)best1].id : (int64_t)0;
            const float4_t* src = reinterpret_cast<const float4_t*>(t.face_tbn + 12 * (size_t)id);
            const float4_t f0 = src[0], f1 = src[1], f2 = src[2];
            float* dst = t.new_tbn + 9 * (size_t)i;
            dst[0] = f0[0]; dst[1] = f0[1]; dst[2] = f0[2]; dst[3] = f0[3];
            dst[4] = f1[0]; dst[5] = f1[1]; dst[6] = f1[2]; dst[7] = f1[3];
            dst[8] = f2[0];
        }
        write_height_ladder(sdf, row);
        return;
    }
    const int best = inner ? b_mine : b_other;
    const Tri tr = tris[best >= 0 ? (uint32_t)best : a.face0];  // face -1 reads face 0, as the reference does; the mask covers it
    const int64_t face = best >= 0 ? tr.id : (int64_t)-1;
    const float2_t* fuv = reinterpret_cast<const float2_t*>(a.face_uv + 6 * (size_t)(best >= 0 ? tr.id : (int64_t)0));
    const float2_t uv0 = fuv[0], uv1 = fuv[1], uv2 = fuv[2];
    const float d = inner ? d1 : d2;
    const V3 dir = inner ? nrm : neg;
    const V3 p_sur{fmaf(d, dir.x, x.x), fmaf(d, dir.y, x.y), fmaf(d, dir.z, x.z)};
    // points_to_barycentric (tools/map.py:85-93)
    const V3 p0 = sub(load3(tr.a), p_sur), p1 = sub(load3(tr.b), p_sur), p2 = sub(load3(tr.c), p_sur);
    const float s0 = norm_plain(cross_plain(p1, p2)), s1 = norm_plain(cross_plain(p2, p0)), s2 = norm_plain(cross_plain(p0, p1));
    const float den = ((s0 + s1) + s2) + 1e-5f;
    const float b0 = s0 / den, b1 = s1 / den, b2 = s2 / den;
    const float u = ((uv0.x * b0 + uv1.x * b1) + uv2.x * b2) * a.uv_rate;
    const float v = ((uv0.y * b0 + uv1.y * b1) + uv2.y * b2) * a.uv_rate;
    if constexpr (LIT) lit_reads_row<ROWS>(t.l, a.H, a.W, u, v, i, N, t.phi, t.patch_id, t.local_tbn, t.sample_tbn);
    half4_t o[4];
    bilinear_read(a.map, a.H, a.W, u, v, o);
    store_features(o, row);
    mask[i] = (fabsf(sdf) < a.h_limit && best >= 0) ? 1 : 0;
    normal_out[3 * (size_t)i] = nrm.x; normal_out[3 * (size_t)i + 1] = nrm.y; normal_out[3 * (size_t)i + 2] = nrm.z;
    if constexpr (!ROWS) {
        p_uv[2 * (size_t)i] = u; p_uv[2 * (size_t)i + 1] = v;
        sdf_out[i] = sdf;
        face_idx[i] = face;
    }
}

// ---------------------------------------------------------------- vertex lookup: the field baked onto the vertices of a fine mesh
// The `imported_type == 'unhash'` branch of MeshFeatureField.forward (tools/map.py:708-714) for one sample point per PAIR of lanes, in one kernel
// behind the neighbour search over the field's OWN mesh: knn() with its defaults (:454-501, shepard_normal above: the projector's normal) ->
// barycentric_mapping over the FINE mesh (:503-528: the two traces, the scaled and offset height, the mask that also wants a hit, the hit's
// barycentric coordinates, :85-93) -> the three corners' feature rows interpolated -> FreqEncoder(height).  The reference's query_tbn(x) of :711 is
// dead work there (nothing reads its tuple) and is not done.
// Behind the normal every operation rounds on its own, as the shape lookup's do: plain products and sums, no fused multiply-add -- except the
// surface point, which is the tracer's own o + t d.
// Lane mapping: the shape lookup's.  Lanes 2 i and 2 i + 1 compute the normal alike, trace along +normal and -normal and meet in an __shfl_xor; every
// exit in front of it is decided by the point.  Behind it lane 0 does the barycentrics, the three 64-byte row reads (twelve independent 16-byte
// loads, issued as soon as the hit's face is known, in front of the barycentric arithmetic) and every per-point store, lane 1 the height ladder.
// The corners come from the tracer's own triangle record (the fp32 values of fine_vertices[face_vertices[face]], which it was built from): one
// 48-byte read the face id needs anyway, where three more dependent gathers into a [V',3] array would stand.
struct VertexArgs {
    const int32_t* face_vertices;  // [F,3]: the three corners' vertex ids by ORIGINAL face id, each in [0, V') (the caller's promise)
    const float* features;         // [V',16] fp32, 16-byte aligned
    float dir_vec_wdist, sdf_scale, sdf_offset, h_limit;
    uint32_t face0;                // nerftex_raytracer::face0
};

// ROWS: the rows contract of nerftex_curved_field_infer's kernels (no sdf, face or barycentric output); otherwise the plain form (every row).
template <bool ROWS>
__global__ __launch_bounds__(64) void vertex_lookup_kernel(const uint32_t N, const float* __restrict__ xyz, const float* __restrict__ dirs,
                                                           const int32_t* __restrict__ knn_idx, const float* __restrict__ knn_dist, const uint32_t K,
                                                           const float* __restrict__ verts, const float* __restrict__ vnormals, const int n_verts,
                                                           const Node* __restrict__ nodes, const Tri* __restrict__ tris, const VertexArgs a,
                                                           float* __restrict__ sdf_out, uint8_t* __restrict__ mask, float* __restrict__ normal_out,
                                                           int64_t* __restrict__ face_idx, float* __restrict__ bary_out, half_t* __restrict__ xin,
                                                           const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = tid >> 1, side = tid & 1u;
    if (i >= (ROWS ? live_rows(N, units_dev, rows_per_unit) : N)) return;
    half_t* row = xin + (size_t)i * 48;
    if (ROWS && slot_unused(dirs, i)) {  // no neighbour list to read, no tree to walk, no row: the constants that make the rest of the chain answer zeros
        if (side) return;
        mask[i] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) normal_out[3 * (size_t)i + c] = 0.0f;
        const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        reinterpret_cast<half8_t*>(row)[0] = zero;
        reinterpret_cast<half8_t*>(row)[1] = zero;
        write_unused_ladder(row);
        return;
    }
    const V3 x = load3(xyz + 3 * (size_t)i);
    const V3 nrm = shepard_normal(x, i, knn_idx, knn_dist, K, verts, vnormals, n_verts, a.dir_vec_wdist);
    // ---- barycentric_mapping(): two closest hits on the fine mesh, the nearer wins
    const V3 neg{-nrm.x, -nrm.y, -nrm.z};
    int b_mine;
    const float d_mine = closest_hit(x, side ? neg : nrm, nodes, tris, b_mine);
    const float d_other = __shfl_xor(d_mine, 1, kWave);
    const int b_other = __shfl_xor(b_mine, 1, kWave);
    const float d1 = side ? d_other : d_mine, d2 = side ? d_mine : d_other;
    const bool inner = d1 < d2;
    const float sdf = (inner ? -d1 : d2) / a.sdf_scale - a.sdf_offset;  // (a true division)
    if (side) {  // lane 1: the ladder, columns 16..47
        write_height_ladder(sdf, row);
        return;
    }
    const int best = inner ? b_mine : b_other;
    const Tri tr = tris[best >= 0 ? (uint32_t)best : a.face0];  // face -1 reads face 0, as the reference does; the mask covers it
    const int64_t face = best >= 0 ? tr.id : (int64_t)-1;
    const int32_t* fv = a.face_vertices + 3 * (size_t)(best >= 0 ? tr.id : (int64_t)0);
    const float4_t* r0 = reinterpret_cast<const float4_t*>(a.features + 16 * (size_t)fv[0]);
    const float4_t* r1 = reinterpret_cast<const float4_t*>(a.features + 16 * (size_t)fv[1]);
    const float4_t* r2 = reinterpret_cast<const float4_t*>(a.features + 16 * (size_t)fv[2]);
    float4_t f0[4], f1[4], f2[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { f0[q] = r0[q]; f1[q] = r1[q]; f2[q] = r2[q]; }
    const float d = inner ? d1 : d2;
    const V3 dir = inner ? nrm : neg;
    const V3 p_sur{fmaf(d, dir.x, x.x), fmaf(d, dir.y, x.y), fmaf(d, dir.z, x.z)};
    // points_to_barycentric (tools/map.py:85-93)
    const V3 p0 = sub(load3(tr.a), p_sur), p1 = sub(load3(tr.b), p_sur), p2 = sub(load3(tr.c), p_sur);
    const float s0 = norm_plain(cross_plain(p1, p2)), s1 = norm_plain(cross_plain(p2, p0)), s2 = norm_plain(cross_plain(p0, p1));
    const float den = ((s0 + s1) + s2) + 1e-5f;
    const float b0 = s0 / den, b1 = s1 / den, b2 = s2 / den;
    auto narrow = [](float v) {  // (the value rounded to fp32 first, then to half: the conversion is not folded into the sum that produces it)
        asm volatile("" : "+v"(v));
        return (half_t)v;
    };
    half8_t o[2];
#pragma unroll
    for (int c = 0; c < 16; c++) o[c / 8][c % 8] = narrow((f0[c / 4][c % 4] * b0 + f1[c / 4][c % 4] * b1) + f2[c / 4][c % 4] * b2);
    reinterpret_cast<half8_t*>(row)[0] = o[0];
    reinterpret_cast<half8_t*>(row)[1] = o[1];
    mask[i] = (fabsf(sdf) < a.h_limit && best >= 0) ? 1 : 0;
    normal_out[3 * (size_t)i] = nrm.x; normal_out[3 * (size_t)i + 1] = nrm.y; normal_out[3 * (size_t)i + 2] = nrm.z;
    if constexpr (!ROWS) {
        sdf_out[i] = sdf;
        face_idx[i] = face;
        bary_out[3 * (size_t)i] = b0; bary_out[3 * (size_t)i + 1] = b1; bary_out[3 * (size_t)i + 2] = b2;
    }
}

// depth of the BVH-4 (root = 1)
int bvh_depth(const std::vector<Node>& nodes) {
    int deepest = 1;
    std::vector<std::pair<int, int>> st{{0, 1}};
    while (!st.empty()) {
        const auto [n, d] = st.back();
        st.pop_back();
        deepest = std::max(deepest, d);
        if (nodes[n].left >= 0)
            for (int c = 0; c < 4; c++) st.push_back({nodes[n].left + c, d + 1});
    }
    return deepest;
}

}  // namespace
}  // namespace nerftex

using namespace nerftex;

extern "C" int nerftex_create_raytracer(const float* host_vertices, uint32_t n_vertices, const uint32_t* host_triangles, uint32_t n_triangles,
                                        nerftex_raytracer** out) {
    clear_error();
    if (!out || !host_vertices || !host_triangles || n_triangles == 0) {
        set_error("create_raytracer: vertices [V,3] float32 and triangles [F,3] uint32 (F > 0) are required");
        return NERFTEX_ERR_INVALID;
    }
    std::vector<Tri> tris(n_triangles);
    for (uint32_t f = 0; f < n_triangles; f++) {
        for (int k = 0; k < 3; k++) {
            const uint32_t v = host_triangles[3 * (size_t)f + k];
            if (v >= n_vertices) {
                set_error("create_raytracer: triangle %u references vertex %u of %u", f, v, n_vertices);
                return NERFTEX_ERR_INVALID;
            }
            float* dst = k == 0 ? tris[f].a : (k == 1 ? tris[f].b : tris[f].c);
            for (int c = 0; c < 3; c++) dst[c] = host_vertices[3 * (size_t)v + c];
        }
        tris[f].id = (int64_t)f;
    }
    std::vector<Node> nodes;
    build_bvh(tris, nodes);
    // the traversal pops one node and pushes up to four: at most 3 * depth + 1 entries are ever on its stack
    if (3 * bvh_depth(nodes) + 1 > kStack) {
        set_error("create_raytracer: a BVH of depth %d needs a traversal stack of %d entries (the kernel has %d); mesh too large", bvh_depth(nodes),
                  3 * bvh_depth(nodes) + 1, kStack);
        return NERFTEX_ERR_INVALID;
    }

    nerftex_raytracer* rt = new nerftex_raytracer();
    rt->n_nodes = (uint32_t)nodes.size();
    rt->n_triangles = n_triangles;
    for (uint32_t k = 0; k < n_triangles; k++)
        if (tris[k].id == 0) rt->face0 = k;
    if (hipGetDevice(&rt->device) != hipSuccess || hipMalloc(&rt->nodes, sizeof(Node) * nodes.size()) != hipSuccess ||
        hipMalloc(&rt->triangles, sizeof(Tri) * tris.size()) != hipSuccess ||
        hipMemcpy(rt->nodes, nodes.data(), sizeof(Node) * nodes.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(rt->triangles, tris.data(), sizeof(Tri) * tris.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("create_raytracer: device allocation / upload failed");
        if (rt->nodes) (void)hipFree(rt->nodes);
        if (rt->triangles) (void)hipFree(rt->triangles);
        delete rt;
        return NERFTEX_ERR_HIP;
    }
    *out = rt;
    return NERFTEX_OK;
}

extern "C" int nerftex_destroy_raytracer(nerftex_raytracer* rt) {
    clear_error();
    if (!rt) return NERFTEX_OK;
    if (rt->nodes) (void)hipFree(rt->nodes);
    if (rt->triangles) (void)hipFree(rt->triangles);
    delete rt;
    return NERFTEX_OK;
}

extern "C" int nerftex_raytracer_trace(const nerftex_raytracer* rt, const float* rays_o, const float* rays_d, float* positions, float* normals,
                                       float* depth, int64_t* face_idx, uint32_t N, void* stream) {
    clear_error();
    if (!rt) {
        set_error("raytracer_trace: NULL raytracer");
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    {
        KernelTimer kt("raytrace_kernel", as_stream(stream));
        hipLaunchKernelGGL(raytrace_kernel, dim3(div_up(N, 64u)), dim3(64), 0, as_stream(stream), N, rays_o, rays_d, positions, normals, depth, face_idx,
                           static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles));
    }
    return check_launch("raytracer_trace");
}

int nerftex::curved_project_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                                 uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, float dir_vec_wdist,
                                 float h_threshold, float* p_sur, uint8_t* h_mask, float* normal, void* xin, const int32_t* units_dev,
                                 uint32_t rows_per_unit, hipStream_t st, const float* tbn, float* tbn_out) {
    if (!rt || K == 0 || K > (uint32_t)kMaxK || n_verts == 0 || n_verts > 0x7fffffffu || (tbn_out && !tbn)) {
        set_error("curved_field_infer: need a raytracer, 1 <= K <= %d neighbours per point and a non-empty vertex array", kMaxK);
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    const float h_limit = fminf(9.5f, h_threshold);  // depth_threshold of tools/map.py:407
    {
        KernelTimer kt("curved_project_rows_kernel", st);
        hipLaunchKernelGGL(curved_project_rows_kernel, dim3(div_up(2 * N, 64u)), dim3(64), 0, st, N, xyz, dirs, knn_idx, knn_dist, K, mesh_vertices, vertex_normals,
                           (int)n_verts, dir_vec_wdist, h_limit, static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles), p_sur, h_mask, normal,
                           static_cast<half_t*>(xin), units_dev, rows_per_unit, tbn, tbn_out);
    }
    return check_launch("curved_field_infer(project)");
}

extern "C" int nerftex_curved_project(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                                      const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, float dir_vec_wdist, float h_threshold, const float* tbn,
                                      uint32_t n_freqs, float* p_sur, float* sdf, uint8_t* h_mask, float* normal, int64_t* face_idx, float* tbn_out,
                                      float* z_embed, void* stream) {
    clear_error();
    if (!rt || K == 0 || K > (uint32_t)kMaxK || (tbn_out && !tbn) || n_verts == 0 || n_verts > 0x7fffffffu) {
        set_error("curved_project: need a raytracer, 1 <= K <= %d neighbours per point, a non-empty vertex array, and the per-face frames when tbn_out is requested", kMaxK);
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    const float h_limit = fminf(9.5f, h_threshold);  // depth_threshold of tools/map.py:407
    {
        KernelTimer kt("curved_project_kernel", as_stream(stream));
        hipLaunchKernelGGL(curved_project_kernel, dim3(div_up(2 * N, 64u)), dim3(64), 0, as_stream(stream), N, xyz, knn_idx, knn_dist, K, mesh_vertices, vertex_normals,
                           (int)n_verts, dir_vec_wdist, h_limit, static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles), tbn, n_freqs, p_sur, sdf, h_mask,
                           normal, face_idx, tbn_out, z_embed);
    }
    return check_launch("curved_project");
}

// ---- the shape lookup's launches (nerftex_shape_lookup below; nerftex_curved_shape_infer, planar.inc, through curved_shape_rows)
namespace nerftex {
namespace {

// lit: NULL for the unlit lookup; otherwise the LIT instantiation with its maps and outputs (phi: half [4,N,2] with ROWS, fp32 [N,8] without)
template <bool ROWS>
void launch_shape_lookup(hipStream_t st, const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                         uint32_t K, const float* verts, const float* vnormals, uint32_t n_verts, const ShapeLookup& s, float* p_uv, float* sdf, uint8_t* mask,
                         float* normal, int64_t* face_idx, half_t* xin, const int32_t* units_dev, uint32_t rows_per_unit, const ShapeLight* lit = nullptr,
                         int32_t* patch_id = nullptr) {
    const ShapeArgs a{s.map, s.map_h, s.map_w, s.face_uv, s.sdf_scale, s.sdf_offset, s.uv_rate, fminf(9.5f, s.h_threshold), rt->face0};  // depth_threshold of tools/map.py:407
    const dim3 grid(div_up(2 * N, 64u)), block(64);
    if (lit) {
        const ShapeLitArgs t{{lit->phi_map, lit->frame_map, lit->sample_tbn_inv, lit->n_patches}, lit->face_tbn, lit->phi, patch_id, lit->local_tbn, lit->sample_tbn,
                             lit->new_tbn};
        KernelTimer kt("shape_light_lookup_kernel", st);
        hipLaunchKernelGGL((shape_lookup_kernel<ROWS, true>), grid, block, 0, st, N, xyz, dirs, knn_idx, knn_dist, K, verts, vnormals, (int)n_verts,
                           static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles), a, p_uv, sdf, mask, normal, face_idx, xin, units_dev,
                           rows_per_unit, t);
        return;
    }
    KernelTimer kt("shape_lookup_kernel", st);
    hipLaunchKernelGGL((shape_lookup_kernel<ROWS, false>), grid, block, 0, st, N, xyz, dirs, knn_idx, knn_dist, K, verts, vnormals, (int)n_verts,
                       static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles), a, p_uv, sdf, mask, normal, face_idx, xin, units_dev, rows_per_unit,
                       ShapeLitArgs{});
}

}  // namespace
}  // namespace nerftex

uint32_t nerftex::raytracer_triangles(const nerftex_raytracer* rt) { return rt ? rt->n_triangles : 0u; }

const char* nerftex::shape_lookup_refusal(const ShapeLookup& s) {
    auto pos = [](float v) { return v > 0.0f && std::isfinite(v); };
    if (s.map_h == 0 || s.map_h > 16384u || s.map_w == 0 || s.map_w > 16384u) return "the map needs between 1 and 16384 texels along each axis";
    if (s.n_freqs != kInferFreqs) return "the kernel writes the curved field's 12 height bands";
    if ((reinterpret_cast<uintptr_t>(s.map) & 15) || (reinterpret_cast<uintptr_t>(s.xin) & 15)) return "the map and xin must be 16-byte aligned";
    if (!pos(s.sdf_scale) || !pos(s.uv_rate) || !pos(s.h_threshold)) return "sdf_scale, uv_rate and h_threshold must be positive and finite";
    if (!std::isfinite(s.sdf_offset)) return "sdf_offset must be finite";
    return nullptr;
}

int nerftex::curved_shape_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                               const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const ShapeLookup& s, uint8_t* mask, float* normal,
                               const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st) {
    if (N == 0) return NERFTEX_OK;
    launch_shape_lookup<true>(st, rt, xyz, dirs, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, nullptr, nullptr, mask, normal, nullptr,
                              static_cast<half_t*>(s.xin), units_dev, rows_per_unit);
    return check_launch("curved_shape_infer(lookup)");
}

const char* nerftex::shape_light_refusal(const ShapeLight& t, uint32_t n_triangles) {
    auto aligned = [](const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); };
    if (t.n_patches == 0 || t.n_patches > (1u << 24)) return "between 1 and 2^24 patch frames (an id is read from an fp32 texel)";
    if (!t.phi_map || !t.frame_map || !t.sample_tbn_inv || !t.face_tbn || !t.phi || !t.local_tbn || !t.sample_tbn || !t.new_tbn)
        return "the lit maps, the patch frames, the face frames and the lit outputs must not be NULL";
    if (!aligned(t.phi_map) || !aligned(t.frame_map) || !aligned(t.sample_tbn_inv) || !aligned(t.face_tbn) || !aligned(t.phi))
        return "the lit maps, the patch frames, the face frames and phi must be 16-byte aligned";
    if (t.n_tbn_faces != n_triangles) return "face_tbn must hold one frame per face of the raytracer";
    return nullptr;
}

int nerftex::curved_shape_light_rows(const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                                     uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const ShapeLookup& s,
                                     const ShapeLight& t, uint8_t* mask, float* normal, const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st) {
    if (N == 0) return NERFTEX_OK;
    launch_shape_lookup<true>(st, rt, xyz, dirs, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, nullptr, nullptr, mask, normal, nullptr,
                              static_cast<half_t*>(s.xin), units_dev, rows_per_unit, &t);
    return check_launch("curved_light_shape_infer(lookup)");
}

extern "C" int nerftex_shape_light_lookup(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                                          const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const float* face_uv, uint32_t n_faces,
                                          const float* face_tbn, uint32_t n_tbn_faces, const float* map, const float* phi_map, const float* frame_map,
                                          const float* sample_tbn_inv, uint32_t map_h, uint32_t map_w, uint32_t n_patches, float sdf_scale, float sdf_offset,
                                          float uv_rate, float h_threshold, uint32_t n_freqs, float* p_uv, float* sdf, uint8_t* mask, float* normal,
                                          int64_t* face_idx, void* xin, float* phi, int32_t* patch_id, float* local_tbn, float* sample_tbn, float* new_tbn,
                                          void* stream) {
    clear_error();
    // nerftex_shape_lookup's refusals, in its order ...
    if (!rt || !xyz || !knn_idx || !knn_dist || !mesh_vertices || !vertex_normals || !face_uv || !map || !p_uv || !sdf || !mask || !normal || !face_idx || !xin) {
        set_error("shape_light_lookup: the raytracer, inputs, mesh arrays, face_uv, map and outputs must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (K == 0 || K > (uint32_t)kMaxK || n_verts == 0 || n_verts > 0x7fffffffu) {
        set_error("shape_light_lookup: 1 <= K <= %d neighbours per point and between 1 and 2^31 - 1 vertices, but got K = %u, n_verts = %u", kMaxK, K, n_verts);
        return NERFTEX_ERR_INVALID;
    }
    if (n_faces != rt->n_triangles) {
        set_error("shape_light_lookup: face_uv holds %u faces, but the raytracer was built over %u", n_faces, rt->n_triangles);
        return NERFTEX_ERR_INVALID;
    }
    const ShapeLookup s{face_uv, map, map_h, map_w, sdf_scale, sdf_offset, uv_rate, h_threshold, n_freqs, xin};
    if (const char* why = shape_lookup_refusal(s)) {
        set_error("shape_light_lookup: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    // ... then nerftex_planar_light_lookup's over what it adds (n_patches, the lit pointers, their alignment), then the face frames' count
    const ShapeLight t{phi_map, frame_map, sample_tbn_inv, n_patches, face_tbn, n_tbn_faces, phi, local_tbn, sample_tbn, new_tbn};
    const char* why = shape_light_refusal(t, rt->n_triangles);
    if (!why && !patch_id) why = "the lit maps, the patch frames, the face frames and the lit outputs must not be NULL";
    if (why) {
        set_error("shape_light_lookup: %s (n_patches = %u, face_tbn holds %u faces, the raytracer %u)", why, n_patches, n_tbn_faces, rt->n_triangles);
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    if (N > 0x7fffffffu) {
        set_error("shape_light_lookup: at most 2^31 - 1 points per call (two lanes each), but got %u", N);
        return NERFTEX_ERR_INVALID;
    }
    launch_shape_lookup<false>(as_stream(stream), rt, xyz, nullptr, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, p_uv, sdf, mask, normal, face_idx,
                               static_cast<half_t*>(xin), nullptr, 0u, &t, patch_id);
    return check_launch("shape_light_lookup");
}

extern "C" int nerftex_shape_lookup(const nerftex_raytracer* rt, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                                    const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const float* face_uv, uint32_t n_faces, const float* map,
                                    uint32_t map_h, uint32_t map_w, float sdf_scale, float sdf_offset, float uv_rate, float h_threshold, uint32_t n_freqs, float* p_uv,
                                    float* sdf, uint8_t* mask, float* normal, int64_t* face_idx, void* xin, void* stream) {
    clear_error();
    if (!rt || !xyz || !knn_idx || !knn_dist || !mesh_vertices || !vertex_normals || !face_uv || !map || !p_uv || !sdf || !mask || !normal || !face_idx || !xin) {
        set_error("shape_lookup: the raytracer, inputs, mesh arrays, face_uv, map and outputs must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (K == 0 || K > (uint32_t)kMaxK || n_verts == 0 || n_verts > 0x7fffffffu) {
        set_error("shape_lookup: 1 <= K <= %d neighbours per point and between 1 and 2^31 - 1 vertices, but got K = %u, n_verts = %u", kMaxK, K, n_verts);
        return NERFTEX_ERR_INVALID;
    }
    if (n_faces != rt->n_triangles) {
        set_error("shape_lookup: face_uv holds %u faces, but the raytracer was built over %u", n_faces, rt->n_triangles);
        return NERFTEX_ERR_INVALID;
    }
    const ShapeLookup s{face_uv, map, map_h, map_w, sdf_scale, sdf_offset, uv_rate, h_threshold, n_freqs, xin};
    if (const char* why = shape_lookup_refusal(s)) {
        set_error("shape_lookup: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    if (N > 0x7fffffffu) {
        set_error("shape_lookup: at most 2^31 - 1 points per call (two lanes each), but got %u", N);
        return NERFTEX_ERR_INVALID;
    }
    launch_shape_lookup<false>(as_stream(stream), rt, xyz, nullptr, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, p_uv, sdf, mask, normal, face_idx,
                               static_cast<half_t*>(xin), nullptr, 0u);
    return check_launch("shape_lookup");
}

// ---- the vertex lookup's launches (nerftex_vertex_lookup below; nerftex_curved_unhash_infer, unhash.inc, through curved_vertex_rows)
namespace nerftex {
namespace {

template <bool ROWS>
void launch_vertex_lookup(hipStream_t st, const nerftex_raytracer* rt, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                          uint32_t K, const float* verts, const float* vnormals, uint32_t n_verts, const VertexLookup& s, float* sdf, uint8_t* mask, float* normal,
                          int64_t* face_idx, float* bary, const int32_t* units_dev, uint32_t rows_per_unit) {
    const VertexArgs a{s.face_vertices, s.features, s.dir_vec_wdist, s.sdf_scale, s.sdf_offset, fminf(9.5f, s.h_threshold), rt->face0};  // depth_threshold of tools/map.py:407
    KernelTimer kt("vertex_lookup_kernel", st);
    hipLaunchKernelGGL(vertex_lookup_kernel<ROWS>, dim3(div_up(2 * N, 64u)), dim3(64), 0, st, N, xyz, dirs, knn_idx, knn_dist, K, verts, vnormals, (int)n_verts,
                       static_cast<const Node*>(rt->nodes), static_cast<const Tri*>(rt->triangles), a, sdf, mask, normal, face_idx, bary, static_cast<half_t*>(s.xin),
                       units_dev, rows_per_unit);
}

}  // namespace
}  // namespace nerftex

const char* nerftex::vertex_lookup_refusal(const VertexLookup& s) {
    auto pos = [](float v) { return v > 0.0f && std::isfinite(v); };
    if (s.n_fine_verts == 0 || s.n_fine_verts > 0x7fffffffu) return "the fine mesh needs between 1 and 2^31 - 1 vertices";
    if (s.n_freqs != kInferFreqs) return "the kernel writes the curved field's 12 height bands";
    if ((reinterpret_cast<uintptr_t>(s.features) & 15) || (reinterpret_cast<uintptr_t>(s.xin) & 15)) return "vertex_features and xin must be 16-byte aligned";
    if (!pos(s.sdf_scale) || !pos(s.h_threshold)) return "sdf_scale and h_threshold must be positive and finite";
    if (!std::isfinite(s.sdf_offset)) return "sdf_offset must be finite";
    return nullptr;
}

int nerftex::curved_vertex_rows(const nerftex_raytracer* rt_fine, const float* xyz, const float* dirs, const int32_t* knn_idx, const float* knn_dist, uint32_t N,
                                uint32_t K, const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, const VertexLookup& s, uint8_t* mask,
                                float* normal, const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st) {
    if (N == 0) return NERFTEX_OK;
    launch_vertex_lookup<true>(st, rt_fine, xyz, dirs, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, nullptr, mask, normal, nullptr, nullptr,
                               units_dev, rows_per_unit);
    return check_launch("curved_unhash_infer(lookup)");
}

extern "C" int nerftex_vertex_lookup(const nerftex_raytracer* rt_fine, const float* xyz, const int32_t* knn_idx, const float* knn_dist, uint32_t N, uint32_t K,
                                     const float* mesh_vertices, const float* vertex_normals, uint32_t n_verts, float dir_vec_wdist, const float* fine_vertices,
                                     uint32_t n_fine_verts, const int32_t* face_vertices, uint32_t n_faces, const float* vertex_features, float sdf_scale,
                                     float sdf_offset, float h_threshold, uint32_t n_freqs, float* sdf, uint8_t* mask, float* normal, int64_t* face_idx, float* bary,
                                     void* xin, void* stream) {
    clear_error();
    if (!rt_fine || !xyz || !knn_idx || !knn_dist || !mesh_vertices || !vertex_normals || !fine_vertices || !face_vertices || !vertex_features || !sdf || !mask ||
        !normal || !face_idx || !bary || !xin) {
        set_error("vertex_lookup: the raytracer, inputs, both meshes' arrays, face_vertices, vertex_features and outputs must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (K == 0 || K > (uint32_t)kMaxK) {
        set_error("vertex_lookup: 1 <= K <= %d neighbours per point, but got K = %u", kMaxK, K);
        return NERFTEX_ERR_INVALID;
    }
    if (n_verts == 0 || n_verts > 0x7fffffffu) {
        set_error("vertex_lookup: the field's mesh needs between 1 and 2^31 - 1 vertices, but got %u", n_verts);
        return NERFTEX_ERR_INVALID;
    }
    const VertexLookup s{face_vertices, vertex_features, n_fine_verts, dir_vec_wdist, sdf_scale, sdf_offset, h_threshold, n_freqs, xin};
    if (n_fine_verts == 0 || n_fine_verts > 0x7fffffffu) {
        set_error("vertex_lookup: %s, but got %u", vertex_lookup_refusal(s), n_fine_verts);
        return NERFTEX_ERR_INVALID;
    }
    if (n_faces != rt_fine->n_triangles) {
        set_error("vertex_lookup: face_vertices holds %u faces, but the raytracer was built over %u", n_faces, rt_fine->n_triangles);
        return NERFTEX_ERR_INVALID;
    }
    if (const char* why = vertex_lookup_refusal(s)) {
        set_error("vertex_lookup: %s", why);
        return NERFTEX_ERR_INVALID;
    }
    if (N == 0) return NERFTEX_OK;
    if (N > 0x7fffffffu) {
        set_error("vertex_lookup: at most 2^31 - 1 points per call (two lanes each), but got %u", N);
        return NERFTEX_ERR_INVALID;
    }
    launch_vertex_lookup<false>(as_stream(stream), rt_fine, xyz, nullptr, knn_idx, knn_dist, N, K, mesh_vertices, vertex_normals, n_verts, s, sdf, mask, normal, face_idx,
                                bary, nullptr, 0u);
    return check_launch("vertex_lookup");
}

#include "patch_export.inc"
