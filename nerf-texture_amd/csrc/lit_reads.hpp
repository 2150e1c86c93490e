// The lit reads of an imported map at one row's (u, v): the `pred_normal` part MeshFeatureField.forward's 'field' and 'shape' branches share
// (tools/map.py:670-675, :702-707) -- a nearest read of the per-texel frame and patch id, the patch's inverted frame, and a bilinear read of
// the [H, W, 8] phi map.  One body for the planar lit lookup (planar_light.inc, in fieldglue.hip) and the lit shape lookup (raytracer.hip).
#pragma once

#include "bilinear_read.hpp"
#include "common.hpp"

namespace nerftex {

struct PlanarLightArgs {
    const float* phi_map;     // [H, W, 8] fp32, channel-last, 16-byte aligned
    const float* frame_map;   // [H, W, 12] fp32, 16-byte aligned: a texel is three 16-byte words -- the 9 floats of its frame, its patch id, two zeros
    const float* sample_inv;  // [P, 12] fp32, 16-byte aligned: the 9 floats of patch p's inverted frame, three zeros
    uint32_t P;
};

// grid_sample(mode='nearest', align_corners=True, padding zeros)'s texel of a map whose FIRST axis u runs along: ix = ((u + 1) / 2) (size - 1) in
// fp32, rounded half to even; -> false outside the map (zeros; a NaN fails the comparisons).  The index is converted only inside the range.
__device__ __forceinline__ bool nearest_texel(const uint32_t H, const uint32_t W, const float u, const float v, size_t& texel) {
#pragma clang fp contract(off)
    const float iu = ((u + 1.0f) / 2.0f) * (float)(H - 1), iv = ((v + 1.0f) / 2.0f) * (float)(W - 1);
    const float ri = nearbyintf(iu), rj = nearbyintf(iv);
    if (!(ri >= 0.0f && ri <= (float)(H - 1) && rj >= 0.0f && rj <= (float)(W - 1))) return false;
    texel = (size_t)(int)ri * (size_t)W + (size_t)(int)rj;
    return true;
}

// Row b of B at (u, v).  ROWS: phi goes out as half, level-major [4, B, 2] (what curved_light_mid_row reads as n_lbc); id_out is not written.
// Otherwise phi as fp32 [B, 8] (the values the half ones are the narrowing of) and the sampled id [B].  Both: local_tbn [B, 9] the texel's
// frame, sample_tbn [B, 9] row `id` of the inverted patch frames; an id outside [0, P) (the caller's to rule out) reads nothing and gives zeros.
template <bool ROWS>
__device__ __forceinline__ void lit_reads_row(const PlanarLightArgs& l, const uint32_t H, const uint32_t W, const float u, const float v, const uint32_t b,
                                              const uint32_t B, void* __restrict__ phi_out, int32_t* __restrict__ id_out, float* __restrict__ local_tbn,
                                              float* __restrict__ sample_tbn) {
    // the nearest reads first: the patch's frame hangs on the texel's id, the longest chain of dependent loads in the row
    const float4_t zero = {0.0f, 0.0f, 0.0f, 0.0f};
    float4_t f[3] = {zero, zero, zero}, s[3] = {zero, zero, zero};
    size_t texel;
    if (nearest_texel(H, W, u, v, texel)) {
        const float4_t* src = reinterpret_cast<const float4_t*>(l.frame_map + texel * 12);
#pragma unroll
        for (int k = 0; k < 3; k++) f[k] = src[k];
    }
    const float idf = f[2][1];
    const int32_t id = (idf > -1.0f && idf < (float)l.P) ? (int32_t)idf : -1;  // (.long() truncates towards zero)
    if (id >= 0) {
        const float4_t* src = reinterpret_cast<const float4_t*>(l.sample_inv + (size_t)id * 12);
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] = src[k];
    }
    if constexpr (ROWS) {
        half4_t o[2];
        bilinear_read<8>(l.phi_map, H, W, u, v, o);
        half_t* n_lbc = static_cast<half_t*>(phi_out);
#pragma unroll
        for (int lv = 0; lv < 4; lv++) {
            const half2_t pair = {o[lv / 2][2 * (lv % 2)], o[lv / 2][2 * (lv % 2) + 1]};
            *reinterpret_cast<half2_t*>(n_lbc + ((size_t)lv * B + b) * 2) = pair;
        }
    } else {
        float4_t o[2];
        bilinear_read<8, float4_t>(l.phi_map, H, W, u, v, o);
        float4_t* dst = reinterpret_cast<float4_t*>(static_cast<float*>(phi_out) + (size_t)b * 8);
        dst[0] = o[0]; dst[1] = o[1];
        id_out[b] = id;  // (-1: a texel whose id is not in [0, P))
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        local_tbn[(size_t)b * 9 + k] = f[k / 4][k % 4];
        sample_tbn[(size_t)b * 9 + k] = s[k / 4][k % 4];
    }
}

// what a row that reads nothing writes in place of lit_reads_row's outputs: zeros for phi and both frames, id -1 in the plain form
template <bool ROWS>
__device__ __forceinline__ void lit_reads_nothing(const uint32_t b, const uint32_t B, void* __restrict__ phi_out, int32_t* __restrict__ id_out,
                                                  float* __restrict__ local_tbn, float* __restrict__ sample_tbn) {
    if constexpr (ROWS) {
        half_t* n_lbc = static_cast<half_t*>(phi_out);
        const half2_t zero = {0, 0};
#pragma unroll
        for (int lv = 0; lv < 4; lv++) *reinterpret_cast<half2_t*>(n_lbc + ((size_t)lv * B + b) * 2) = zero;
    } else {
        const float4_t zero = {0.0f, 0.0f, 0.0f, 0.0f};
        float4_t* dst = reinterpret_cast<float4_t*>(static_cast<float*>(phi_out) + (size_t)b * 8);
        dst[0] = zero; dst[1] = zero;
        id_out[b] = -1;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        local_tbn[(size_t)b * 9 + k] = 0.0f;
        sample_tbn[(size_t)b * 9 + k] = 0.0f;
    }
}

}  // namespace nerftex
