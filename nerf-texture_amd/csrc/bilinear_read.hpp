// grid_sample(bilinear, align_corners=True, padding zeros) of an imported [H, W, C] fp32 map at (u, v), narrowed to the 16-bit values the
// networks read: the one read of the planar lookup (planar.inc, the 'field' branch of MeshFeatureField.forward), of the shape lookup
// (raytracer.hip, the 'shape' branch) and of the lit lookup's phi map (planar_light.inc, C = 8).  u runs along the map's FIRST axis.
#pragma once

#include "common.hpp"

namespace nerftex {

// The calling thread reads the four corners' 4 C bytes each as C / 4 16-byte loads (all of them independent, in flight together) and gets all C
// features, o[0 .. C / 4 - 1].
// V = half4_t: the values narrowed to half; V = float4_t: the fp32 values those are the narrowing of.
// Every framework op rounds on its own (no contraction); a corner outside [0,H) x [0,W) contributes nothing and is not read; the comparisons are on
// the floats (a NaN or a huge coordinate fails them all) and the index is converted only inside the range, then widened to size_t.
template <int C = 16, typename V = half4_t>
__device__ __forceinline__ void bilinear_read(const float* __restrict__ map, const uint32_t H, const uint32_t W, const float u, const float v, V (&o)[C / 4]) {
#pragma clang fp contract(off)
    static_assert(C % 4 == 0 && C >= 4, "whole 16-byte words per texel");
    auto narrow = [](float x) {  // (fieldglue.hip's narrow: the value rounded to fp32 first, then to half; fp32 out: the value as it is)
        asm volatile("" : "+v"(x));
        if constexpr (sizeof(V) == sizeof(half4_t))
            return (half_t)x;
        else
            return x;
    };
    const float iu = ((u + 1.0f) / 2.0f) * (float)(H - 1), iv = ((v + 1.0f) / 2.0f) * (float)(W - 1);
    const float i0 = floorf(iu), j0 = floorf(iv);
    const float wu1 = iu - i0, wu0 = (i0 + 1.0f) - iu, wv1 = iv - j0, wv0 = (j0 + 1.0f) - iv;
    const float w[4] = {wu0 * wv0, wu1 * wv0, wu0 * wv1, wu1 * wv1};  // texels (i0,j0), (i0+1,j0), (i0,j0+1), (i0+1,j0+1), added in this order
    const float hi_i = (float)(H - 1), hi_j = (float)(W - 1);
    const bool in_i[2] = {i0 >= 0.0f && i0 <= hi_i, i0 + 1.0f >= 0.0f && i0 + 1.0f <= hi_i};
    const bool in_j[2] = {j0 >= 0.0f && j0 <= hi_j, j0 + 1.0f >= 0.0f && j0 + 1.0f <= hi_j};
    constexpr int Q = C / 4;  // 16-byte words of a texel
    float4_t t[4][Q];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int di = k & 1, dj = k >> 1;
        if (in_i[di] && in_j[dj]) {
            const size_t i = (size_t)(int)(i0 + (float)di), j = (size_t)(int)(j0 + (float)dj);
            const float4_t* src = reinterpret_cast<const float4_t*>(map + (i * (size_t)W + j) * C);
#pragma unroll
            for (int qq = 0; qq < Q; qq++) t[k][qq] = src[qq];
        } else {
#pragma unroll
            for (int qq = 0; qq < Q; qq++) t[k][qq] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    // four products and three sums; an absent corner's texel is 0 and its weight finite whenever another corner is present (iu, iv then lie within one
    // texel of the map), so its product adds nothing; with no corner present the weights may be anything and the answer is 0
    const bool any = (in_i[0] || in_i[1]) && (in_j[0] || in_j[1]);
#pragma unroll
    for (int c = 0; c < 4 * Q; c++) {
        const float acc = ((t[0][c / 4][c % 4] * w[0] + t[1][c / 4][c % 4] * w[1]) + t[2][c / 4][c % 4] * w[2]) + t[3][c / 4][c % 4] * w[3];
        o[c / 4][c % 4] = narrow(any ? acc : 0.0f);
    }
}

// the 16 features of a read as the two 16-byte stores of columns 0..15 of the sigma net's input row
__device__ __forceinline__ void store_features(const half4_t (&o)[4], half_t* __restrict__ row48) {
    half8_t o8[2];
#pragma unroll
    for (int c = 0; c < 16; c++) o8[c / 8][c % 8] = o[c / 4][c % 4];
    reinterpret_cast<half8_t*>(row48)[0] = o8[0];
    reinterpret_cast<half8_t*>(row48)[1] = o8[1];
}

}  // namespace nerftex
