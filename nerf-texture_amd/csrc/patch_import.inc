// An imported feature PATCH under the curved field (nerftex_patch_lookup, nerftex_patch_light_lookup, and the lookup launch of
// nerftex_curved_patch_infer / nerftex_curved_light_patch_infer, patch_chain.inc): the `imported_type == 'patch'` branch of
// MeshFeatureField.forward (tools/map.py:676-692) over MeshProjector.weighted_project(weighting='DualD') (:435-452) and
// knn(use_dir_vec=False, direct_above_check=True, direct_above_threshold=1., weighting='Shepard') (:454-501).  The patch is an oriented
// point cloud; a sample resamples it from its K = 8 nearest points.  Included at the end of knn.hip: the search is knn_search_point<8>.
//
// Per-point records, every one 16-byte aligned, indexed by the point's ORIGINAL index (what the search returns):
//   geom     [V, 8] fp32   {px, py, pz, 0 | nx, ny, nz, 0}       two 16-byte words  (NERFTEX_PATCH_GEOM_STRIDE)
//   features [V,16] fp32   the 16 texture features                four 16-byte words
//   lit      [V,20] fp32   {phi 0..7 | frame 0..8 | 0 0 0}        five 16-byte words (NERFTEX_PATCH_LIT_STRIDE; the lit lookups only)
// A row gathers 8 x (2 + 4 [+ 5]) words.  The patch of a 128 x 128 export is 16 384 points: 0.5 + 1 + 1.25 MiB, L2-resident.
//
// Lane mapping: one thread per row -- the search, the weights, and all 8 x 4 (+ 8 x 5) gathers, each neighbour's words requested together.  (Four
// adjacent lanes per row measured twice as slow -- DESIGN.md 4.20 -- and was removed.)

namespace nerftex {
namespace {

struct PatchArgs {
    const float* geom;      // [V,8]
    const float* features;  // [V,16]
    const float* lit;       // [V,20], LIT only
    float h_threshold;
};

// what the plain forms write beside the rows forms' outputs (NULL in the rows forms)
struct PatchPlainOut {
    float* sdf;      // [B]
    int32_t* idx;    // [B,8]  nerftex_knn_query's, bit for bit
    float* dis;      // [B,8]  nerftex_knn_query's, bit for bit (BEFORE the direct-above select)
    float* weights;  // [B,8]  the normalised DualD weights
};

// ROWS: the rows contract of nerftex_curved_field_infer's kernels -- rows >= live untouched; a marked slot searches and gathers nothing and gets
// mask 0, normal 0, features 0, z = 0 | ones.  phi_out: ROWS half, level-major [4,B,2] (what curved_light_mid_row reads as n_lbc); plain fp32 [B,8].
template <bool ROWS, bool LIT>
__global__ __launch_bounds__(256) void patch_lookup_kernel(const float* __restrict__ xyz, const float* __restrict__ dirs, const uint32_t B, const GridDesc g,
                                                           const uint32_t* __restrict__ cell_start, const P4* __restrict__ points, const PatchArgs a,
                                                           uint8_t* __restrict__ mask, float* __restrict__ normal_out, half_t* __restrict__ xin,
                                                           void* __restrict__ phi_out, float* __restrict__ tbn_out, const PatchPlainOut po,
                                                           const int32_t* __restrict__ units_dev, const uint32_t rows_per_unit) {
#pragma clang fp contract(off)  // every framework op rounds on its own
    constexpr int K = 8;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (ROWS ? live_rows(B, units_dev, rows_per_unit) : B)) return;
    half_t* row = xin + (size_t)b * 48;
    if (ROWS && slot_unused(dirs, b)) {  // no search, no gather
        mask[b] = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) normal_out[(size_t)b * 3 + c] = 0.0f;
        const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        reinterpret_cast<half8_t*>(row)[0] = zero;
        reinterpret_cast<half8_t*>(row)[1] = zero;
        write_unused_ladder(row);
        return;
    }
    auto narrow = [](float v) {  // (fieldglue.hip's narrow: the value rounded to fp32 first, then to half)
        asm volatile("" : "+v"(v));
        return (half_t)v;
    };
    const float x[3] = {xyz[(size_t)b * 3], xyz[(size_t)b * 3 + 1], xyz[(size_t)b * 3 + 2]};
    float best[K];
    int ids[K];
    knn_search_point<K>(x, g, cell_start, points, best, ids);

    // ---- knn(): neighbours' normals and offsets, the direct-above test, the Shepard-weighted normal (:459-499) ----
    float4_t gp[K], gn[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        // (V >= 8, so the search fills all eight -- unless x is not finite: nothing compares, the ids stay -1 and the row reads record 0 for its NaNs)
        const float4_t* src = reinterpret_cast<const float4_t*>(a.geom + (size_t)max(ids[k], 0) * 8);
        gp[k] = src[0];
        gn[k] = src[1];
    }
    float dv[K][3], dis[K], cr_min = INFINITY;
#pragma unroll
    for (int k = 0; k < K; k++) {
        dis[k] = sqrtf(best[k]);
#pragma unroll
        for (int c = 0; c < 3; c++) dv[k][c] = x[c] - gp[k][c];
        const float len = sqrtf((dv[k][0] * dv[k][0] + dv[k][1] * dv[k][1]) + dv[k][2] * dv[k][2]) + 1e-5f;
        const float d0 = dv[k][0] / len, d1 = dv[k][1] / len, d2 = dv[k][2] / len;
        const float c0 = gn[k][1] * d2 - gn[k][2] * d1, c1 = gn[k][2] * d0 - gn[k][0] * d2, c2 = gn[k][0] * d1 - gn[k][1] * d0;
        cr_min = fminf(cr_min, sqrtf((c0 * c0 + c1 * c1) + c2 * c2));
    }
    const bool above = 2.0f * cr_min < 1.0f;
    if (!ROWS) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            po.idx[(size_t)b * K + k] = ids[k];
            po.dis[(size_t)b * K + k] = dis[k];
        }
    }
    // a select, not a branch: a row that fails the test goes on with the reference's 1e5 in every distance and offset
    float wsum = 0.0f, ws[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        dis[k] = above ? dis[k] : 1e5f;
#pragma unroll
        for (int c = 0; c < 3; c++) dv[k][c] = above ? dv[k][c] : 1e5f;
        ws[k] = 1.0f / (dis[k] + 1e-7f);
        wsum = wsum + ws[k];
    }
    float n[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < K; k++) {
        const float w = ws[k] / wsum;
        const float len = sqrtf((gn[k][0] * gn[k][0] + gn[k][1] * gn[k][1]) + gn[k][2] * gn[k][2]) + 1e-5f;
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = n[c] + (gn[k][c] / len) * w;
    }
    {
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + 1e-5f;
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = n[c] / len;
    }

    // ---- weighted_project(weighting='DualD') (:437-448) ----
    float s[K], t[K], dk = -INFINITY, d1 = INFINITY;
#pragma unroll
    for (int k = 0; k < K; k++) {
        s[k] = (dv[k][0] * n[0] + dv[k][1] * n[1]) + dv[k][2] * n[2];
        float q2[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float r = dv[k][c] - s[k] * n[c];
            q2[c] = r * r;
        }
        t[k] = sqrtf((q2[0] * q2[0] + q2[1] * q2[1]) + q2[2] * q2[2]);  // the 2-norm of the component-wise SQUARES, as :438 has it
        dk = fmaxf(dk, t[k]);
        d1 = fminf(d1, t[k]);
    }
    float w[K], W = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) {
        w[k] = (((dk - t[k]) / ((dk - d1) + 1e-5f)) * (dk + d1)) / (dk + t[k]);
        W = W + w[k];
    }
    float sdf = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) {
        w[k] = w[k] / (W + 1e-5f);
        sdf = sdf + s[k] * w[k];
    }
    mask[b] = (fabsf(sdf) < a.h_threshold && dis[0] < a.h_threshold) ? 1 : 0;  // (dis ascending: dis[0] is the minimum, 1e5 where the test failed)
#pragma unroll
    for (int c = 0; c < 3; c++) normal_out[(size_t)b * 3 + c] = n[c];
    if (!ROWS) {
        po.sdf[b] = sdf;
#pragma unroll
        for (int k = 0; k < K; k++) po.weights[(size_t)b * K + k] = w[k];
    }

    // ---- the gathers (:679-680, :688-691): sum_k w_k record_k, ascending k, every product and sum rounded on its own ----
    constexpr int Q = 4;  // 16-byte words of a feature record
    float4_t f[K][Q];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const float4_t* src = reinterpret_cast<const float4_t*>(a.features + (size_t)max(ids[k], 0) * 16);
#pragma unroll
        for (int j = 0; j < Q; j++) f[k][j] = src[j];
    }
    half4_t o[Q];
#pragma unroll
    for (int j = 0; j < Q; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < K; k++) acc = acc + w[k] * f[k][j][c];
            o[j][c] = narrow(acc);
        }
    half8_t o8[2];
#pragma unroll
    for (int c = 0; c < 16; c++) o8[c / 8][c % 8] = o[c / 4][c % 4];
    reinterpret_cast<half8_t*>(row)[0] = o8[0];
    reinterpret_cast<half8_t*>(row)[1] = o8[1];
    write_height_ladder(sdf, row);

    if constexpr (LIT) {
        // words 0, 1 of a lit record: phi; words 2, 3, 4: the frame (9 floats, three zeros)
#pragma unroll
        for (int word = 0; word < 5; word++) {
            float4_t l[K];
#pragma unroll
            for (int k = 0; k < K; k++) l[k] = reinterpret_cast<const float4_t*>(a.lit + (size_t)max(ids[k], 0) * 20)[word];
            float acc[4];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                acc[c] = 0.0f;
#pragma unroll
                for (int k = 0; k < K; k++) acc[c] = acc[c] + w[k] * l[k][c];
            }
            if (word < 2) {
                if constexpr (ROWS) {  // levels 2 word, 2 word + 1 of the level-major half block
                    half_t* n_lbc = static_cast<half_t*>(phi_out);
#pragma unroll
                    for (int lv = 0; lv < 2; lv++) {
                        const half2_t pair = {narrow(acc[2 * lv]), narrow(acc[2 * lv + 1])};
                        *reinterpret_cast<half2_t*>(n_lbc + ((size_t)(2 * word + lv) * B + b) * 2) = pair;
                    }
                } else {
                    const float4_t v = {acc[0], acc[1], acc[2], acc[3]};
                    reinterpret_cast<float4_t*>(static_cast<float*>(phi_out) + (size_t)b * 8)[word] = v;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int e = 4 * (word - 2) + c;
                    if (e < 9) tbn_out[(size_t)b * 9 + e] = acc[c];
                }
            }
        }
    }
}

template <bool ROWS, bool LIT>
void launch_patch_lookup(hipStream_t st, const nerftex_knn* kn, const float* xyz, const float* dirs, uint32_t B, const PatchArgs& a, uint8_t* mask, float* normal,
                         half_t* xin, void* phi, float* tbn, const PatchPlainOut& po, const int32_t* units_dev, uint32_t rows_per_unit) {
    const GridDesc g = grid_desc(kn);
    const uint32_t* cs = static_cast<const uint32_t*>(kn->cell_start);
    const P4* pts = static_cast<const P4*>(kn->points);
    KernelTimer kt("patch_lookup_kernel", st);
    hipLaunchKernelGGL((patch_lookup_kernel<ROWS, LIT>), dim3(div_up(B, 256u)), dim3(256), 0, st, xyz, dirs, B, g, cs, pts, a, mask, normal, xin, phi, tbn, po,
                       units_dev, rows_per_unit);
}

inline bool aligned16_(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

uint32_t knn_points(const nerftex_knn* kn) { return kn ? kn->n_points : 0u; }

const char* patch_lookup_refusal(const PatchLookup& s, bool lit) {
    if (!s.knn || s.n_points != s.knn->n_points || s.n_points < 8u || s.n_points > 0x7fffffffu)
        return "a neighbour grid over the patch's points is required, n_points must be its point count, and a patch holds between 8 and 2^31 - 1 points";
    if (s.n_freqs != kInferFreqs) return "the kernel writes the curved field's 12 height bands (n_freqs = 12)";
    if (!s.geom || !s.features || (lit && !s.lit)) return "the patch's geom, features and (lit) lit records must not be NULL";
    if (!aligned16_(s.geom) || !aligned16_(s.features) || (lit && !aligned16_(s.lit)) || !aligned16_(s.xin))
        return "the patch's records and xin must be 16-byte aligned";
    if (!(s.h_threshold > 0.0f) || !std::isfinite(s.h_threshold)) return "h_threshold must be positive and finite";
    return nullptr;
}

int patch_lookup_rows(const PatchLookup& s, const float* xyz, const float* dirs, uint32_t N, uint8_t* mask, float* normal, void* n_lbc, float* tbn,
                      const int32_t* units_dev, uint32_t rows_per_unit, hipStream_t st) {
    const PatchArgs a{s.geom, s.features, s.lit, s.h_threshold};
    const PatchPlainOut none{nullptr, nullptr, nullptr, nullptr};
    if (n_lbc)
        launch_patch_lookup<true, true>(st, s.knn, xyz, dirs, N, a, mask, normal, static_cast<half_t*>(s.xin), n_lbc, tbn, none, units_dev, rows_per_unit);
    else
        launch_patch_lookup<true, false>(st, s.knn, xyz, dirs, N, a, mask, normal, static_cast<half_t*>(s.xin), nullptr, nullptr, none, units_dev, rows_per_unit);
    return check_launch("patch_lookup(rows)");
}

}  // namespace nerftex

static int patch_lookup_plain(const char* who, bool lit, const nerftex_knn* knn, const float* xyz, const float* geom, const float* features, const float* lit_records,
                              uint32_t n_points, float h_threshold, uint32_t n_freqs, uint32_t B, float* sdf, uint8_t* mask, float* normal, void* xin, int32_t* idx,
                              float* dis, float* weights, float* phi, float* tbn, void* stream) {
    clear_error();
    // (B == 0 returns before the pointers are looked at; the patch itself is checked first)
    const PatchLookup s{knn, geom, features, lit_records, n_points, h_threshold, n_freqs, xin};
    if (!knn || n_points != knn->n_points || n_points < 8u || n_points > 0x7fffffffu || n_freqs != kInferFreqs) {
        set_error("%s: %s", who, patch_lookup_refusal(PatchLookup{knn, geom, features, lit_records, n_points, 1.0f, n_freqs, nullptr}, lit));
        return NERFTEX_ERR_INVALID;
    }
    if (B == 0) return NERFTEX_OK;
    if (!xyz || !sdf || !mask || !normal || !xin || !idx || !dis || !weights || (lit && (!phi || !tbn || !aligned16_(phi)))) {
        set_error("%s: inputs and outputs must not be NULL, and phi must be 16-byte aligned", who);
        return NERFTEX_ERR_INVALID;
    }
    if (const char* why = patch_lookup_refusal(s, lit)) {
        set_error("%s: %s", who, why);
        return NERFTEX_ERR_INVALID;
    }
    const PatchArgs a{geom, features, lit_records, h_threshold};
    const PatchPlainOut po{sdf, idx, dis, weights};
    hipStream_t st = as_stream(stream);
    if (lit)
        launch_patch_lookup<false, true>(st, knn, xyz, nullptr, B, a, mask, normal, static_cast<half_t*>(xin), phi, tbn, po, nullptr, 0u);
    else
        launch_patch_lookup<false, false>(st, knn, xyz, nullptr, B, a, mask, normal, static_cast<half_t*>(xin), nullptr, nullptr, po, nullptr, 0u);
    return check_launch(who);
}

extern "C" int nerftex_patch_lookup(const nerftex_knn* knn, const float* xyz, const float* geom, const float* features, uint32_t n_points, float h_threshold,
                                    uint32_t n_freqs, uint32_t B, float* sdf, uint8_t* mask, float* normal, void* xin, int32_t* idx, float* dis, float* weights,
                                    void* stream) {
    return patch_lookup_plain("patch_lookup", false, knn, xyz, geom, features, nullptr, n_points, h_threshold, n_freqs, B, sdf, mask, normal, xin, idx, dis, weights,
                              nullptr, nullptr, stream);
}

extern "C" int nerftex_patch_light_lookup(const nerftex_knn* knn, const float* xyz, const float* geom, const float* features, const float* lit, uint32_t n_points,
                                          float h_threshold, uint32_t n_freqs, uint32_t B, float* sdf, uint8_t* mask, float* normal, void* xin, int32_t* idx,
                                          float* dis, float* weights, float* phi, float* local_tbn, void* stream) {
    return patch_lookup_plain("patch_light_lookup", true, knn, xyz, geom, features, lit, n_points, h_threshold, n_freqs, B, sdf, mask, normal, xin, idx, dis, weights,
                              phi, local_tbn, stream);
}
