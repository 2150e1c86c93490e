// FreqEncoder(height) of the curved field (tools/encoding.py:5-43, 12 log-sampled bands, the input included) as the 16-bit values the sigma net
// reads: the one ladder of the mesh projector's rows form (raytracer.hip) and of the planar lookup of an imported feature map (planar.inc).
#pragma once

#include "common.hpp"

namespace nerftex {

constexpr uint32_t kInferFreqs = 12;  // multires of the curved field: z_embed has 1 + 2 * 12 = 25 columns

// row48: the point's row of the sigma net's [N,48] half input -- columns 16..40 = half(z_embed), 41..47 = the padding ones.
// The fp32 value the plain projector stores is narrowed as nerftex_curved_pack_inputs narrows it after reading it back (the empty asm keeps
// the conversion from being folded into the operation that produces the value).
__device__ __forceinline__ void write_height_ladder(const float sdf, half_t* __restrict__ row48) {
    auto narrow = [](float v) {
        asm volatile("" : "+v"(v));
        return (half_t)v;
    };
    half8_t o[4];
    o[0][0] = narrow(sdf);
    float f = 1.0f;
#pragma unroll
    for (uint32_t k = 0; k < kInferFreqs; k++, f *= 2.0f) {
        o[(1 + 2 * k) / 8][(1 + 2 * k) % 8] = narrow(sinf(sdf * f));
        o[(2 + 2 * k) / 8][(2 + 2 * k) % 8] = narrow(cosf(sdf * f));
    }
#pragma unroll
    for (int c = 1 + 2 * (int)kInferFreqs; c < 32; c++) o[c / 8][c % 8] = (half_t)1.0f;
    half8_t* dst = reinterpret_cast<half8_t*>(row48 + 16);
#pragma unroll
    for (int q = 0; q < 4; q++) dst[q] = o[q];
}

// a slot the march marked unused: z = 0 | ones (column 40 is z's last, 41..47 the padding ones)
__device__ __forceinline__ void write_unused_ladder(half_t* __restrict__ row48) {
    half8_t z8, tail;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        z8[c] = (half_t)0.0f;
        tail[c] = c == 0 ? (half_t)0.0f : (half_t)1.0f;
    }
    half8_t* dst = reinterpret_cast<half8_t*>(row48 + 16);
    dst[0] = z8; dst[1] = z8; dst[2] = z8; dst[3] = tail;
}

}  // namespace nerftex
