// Elementwise glue of the ngp field between / after the two fully-fused MLPs (first step).
//
// nerf/network_ff.py:60-110 strings the two FFMLPs together with a dozen small framework ops per direction: slice the density
// logit and the 15 geometry features out of the sigma net's 16 outputs, cast, trunc_exp (tools/activation.py:5-17), encode the
// view direction (SH degree 4), cast it, append one zero column, concatenate to the colour net's 32 inputs; afterwards slice 3 of
// the 16 colour outputs, sigmoid, cast to fp32 for compositing -- and the mirror image in the backward pass.  On an MI355X
// that is ~25 launches and ~0.2 ms per training step of pure memory traffic.  Here it is two streaming kernels per direction,
// with the arithmetic of the framework ops reproduced step by step (same roundings: fp32 exp of the half logit; SH in fp32
// narrowed to half; sigmoid in fp32 narrowed to half and widened again; gradients narrowed to half where autograd would).
#include "bilinear_read.hpp"
#include "common.hpp"
#include "curved_infer.hpp"
#include "height_ladder.hpp"
#include "lit_reads.hpp"
#include "sh_common.hpp"

#include <cmath>

namespace nerftex {
namespace {

// narrow an fp32 RESULT to half the way the framework does (value rounded to fp32 first, then to half): the empty asm keeps the
// compiler from folding the producing multiply into the conversion (v_fma_mix*_f16 rounds once)
__device__ __forceinline__ half_t narrow(float v) {
    asm volatile("" : "+v"(v));
    return (half_t)v;
}


// h [B,16] half, dirs [B,3] fp32  ->  sigma [B] fp32 = exp(h[:,0]),  cin [B,32] half = [SH4(dir) | h[:,1:16] | 0]
__global__ __launch_bounds__(256) void field_mid_forward_kernel(const half_t* __restrict__ h, const float* __restrict__ dirs, uint32_t B,
                                                               float* __restrict__ sigma, half_t* __restrict__ cin) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const half8_t h0 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16);
    const half8_t h1 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16 + 8);
    sigma[b] = expf((float)h0[0]);
    float r[16];
    sh::eval<4>(dirs[(size_t)b * 3], dirs[(size_t)b * 3 + 1], dirs[(size_t)b * 3 + 2], r);
    half8_t o0, o1, o2, o3;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        o0[i] = narrow(r[i]);
        o1[i] = narrow(r[8 + i]);
    }
#pragma unroll
    for (int i = 0; i < 7; i++) o2[i] = h0[1 + i];
    o2[7] = h1[0];
#pragma unroll
    for (int i = 0; i < 7; i++) o3[i] = h1[1 + i];
    o3[7] = (half_t)0.0f;
    half8_t* out = reinterpret_cast<half8_t*>(cin + (size_t)b * 32);
    out[0] = o0; out[1] = o1; out[2] = o2; out[3] = o3;
}

// grad_sigma [B] fp32, grad_cin [B,32] half, h [B,16] half -> grad_h [B,16] half
//   column 0: trunc_exp backward  g * exp(clamp(x, -15, 15))  in fp32, narrowed;  columns 1..15: the geometry slice of grad_cin
__global__ __launch_bounds__(256) void field_mid_backward_kernel(const float* __restrict__ grad_sigma, const half_t* __restrict__ grad_cin,
                                                                const half_t* __restrict__ h, uint32_t B, half_t* __restrict__ grad_h) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const half8_t g2 = *reinterpret_cast<const half8_t*>(grad_cin + (size_t)b * 32 + 16);
    const half8_t g3 = *reinterpret_cast<const half8_t*>(grad_cin + (size_t)b * 32 + 24);
    const float x = (float)h[(size_t)b * 16];
    const float gs = grad_sigma[b] * expf(fminf(fmaxf(x, -15.0f), 15.0f));
    half8_t o0, o1;
    o0[0] = narrow(gs);
#pragma unroll
    for (int i = 0; i < 7; i++) o0[1 + i] = g2[i];
    o1[0] = g2[7];
#pragma unroll
    for (int i = 0; i < 7; i++) o1[1 + i] = g3[i];
    half8_t* out = reinterpret_cast<half8_t*>(grad_h + (size_t)b * 16);
    out[0] = o0; out[1] = o1;
}

// hc [B,16] half -> rgbs [B,3] fp32 = float(half(sigmoid(hc[:, :3])))
__global__ __launch_bounds__(256) void field_out_forward_kernel(const half_t* __restrict__ hc, uint32_t B, float* __restrict__ rgbs) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const half4_t v = *reinterpret_cast<const half4_t*>(hc + (size_t)b * 16);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float x = (float)v[c];
        rgbs[(size_t)b * 3 + c] = (float)narrow(1.0f / (1.0f + expf(-x)));
    }
}

// grad_rgbs [B,3] fp32, rgbs [B,3] fp32 (the half-valued colours) -> grad_hc [B,16] half:  (g (1 - y)) y  in fp16 arithmetic on the narrowed g
__global__ __launch_bounds__(256) void field_out_backward_kernel(const float* __restrict__ grad_rgbs, const float* __restrict__ rgbs, uint32_t B,
                                                                half_t* __restrict__ grad_hc) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    half8_t o0 = {0, 0, 0, 0, 0, 0, 0, 0};
    const half8_t o1 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // the framework's sigmoid backward for fp16 tensors runs in fp16 ARITHMETIC: (g * (1 - y)) * y with every operation rounded
        // to half (verified against torch on 65 k values: 0 mismatches; the fp32 formula differs in 5 % of them by one half-ulp)
        const half_t g = narrow(grad_rgbs[(size_t)b * 3 + c]);
        const half_t y = (half_t)rgbs[(size_t)b * 3 + c];
        half_t t = (half_t)1.0f - y;
        asm volatile("" : "+v"(t));
        half_t u = g * t;
        asm volatile("" : "+v"(u));
        o0[c] = u * y;
    }
    half8_t* out = reinterpret_cast<half8_t*>(grad_hc + (size_t)b * 16);
    out[0] = o0; out[1] = o1;
}

// ---- the curved field's glue (round 6) -------------------------------------------------------------------------------
// network_curvedfield.py:283-306 + tools/map.py:620-641 string MeshFeatureField, the sigma net and the colour net together with ~30 small framework
// ops per forward (normalisations, the view direction reflected about the normal, SH, pads, concatenations, masks): ~200 us of launch-latency-
// bound kernels per 262 k points.  Three streaming kernels instead, the framework's fp32 arithmetic step by step.

// x_embed [B,16] half, z_embed [B,25] fp32 -> [B,48] half = [x_embed | half(z_embed) | 1 x 7]  (tcnn pads its inputs with ones)
__global__ __launch_bounds__(256) void curved_pack_inputs_kernel(const half_t* __restrict__ x_embed, const float* __restrict__ z_embed, uint32_t B,
                                                                half_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    half8_t o[6];
    o[0] = *reinterpret_cast<const half8_t*>(x_embed + (size_t)b * 16);
    o[1] = *reinterpret_cast<const half8_t*>(x_embed + (size_t)b * 16 + 8);
    const float* z = z_embed + (size_t)b * 25;
#pragma unroll
    for (int i = 0; i < 32; i++) o[2 + i / 8][i % 8] = i < 25 ? (half_t)z[i] : (half_t)1.0f;
    half8_t* dst = reinterpret_cast<half8_t*>(out + (size_t)b * 48);
#pragma unroll
    for (int i = 0; i < 6; i++) dst[i] = o[i];
}

// h [B,16] half (the sigma net's output), normal [B,3] fp32 (MeshFeatureField's normalised coarse normal; eval bit 1: the projector's RAW normal), dirs [B,3] fp32
//   -> sigma [B] half = half(exp(h[:,0]))  (trunc_exp forward, tools/activation.py:5-17, on a half tensor)
//      cin [B,32] half = [SH4(2 ((wr + 1) / 2) - 1) | h[:,1:16] | 1],  wr = the view direction reflected about the normal (:283-306)
__device__ __forceinline__ void curved_mid_row(const uint32_t b, const half_t* __restrict__ h, const float* __restrict__ normal, const float* __restrict__ dirs,
                                               const float fc, const int eval, half_t* __restrict__ sigma, half_t* __restrict__ cin) {
#pragma clang fp contract(off)  // every framework op rounds on its own
    const half8_t h0 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16);
    const half8_t h1 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16 + 8);
    sigma[b] = narrow(expf((float)h0[0]));
    float n[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        n[c] = normal[(size_t)b * 3 + c];
        d[c] = dirs[(size_t)b * 3 + c];
    }
    auto unit = [](float (&v)[3]) {  // v / (|v| + 1e-5)
        const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-5f;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = v[c] / len;
    };
    if (eval & 2) unit(n);  // bit 1: `normal` is the projector's raw normal -- MeshFeatureField's own normalisation (tools/map.py:720) first
    unit(n);
    if (eval & 1) {  // :289-291 with the coarse normal on both sides
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = fc * n[c] + (1 - fc) * n[c];
        unit(n);
    }
    unit(d);
    const float dot = ((-d[0] * n[0]) + (-d[1] * n[1])) + (-d[2] * n[2]);
    float wr[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float w = (2 * dot) * n[c] + d[c];
        wr[c] = ((w + 1) / 2) * 2 - 1;  // tcnn's SH takes [0, 1]; the encoder maps it back
    }
    float r[16];
    sh::eval<4>(wr[0], wr[1], wr[2], r);
    half8_t o0, o1, o2, o3;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        o0[i] = narrow(r[i]);
        o1[i] = narrow(r[8 + i]);
    }
#pragma unroll
    for (int i = 0; i < 7; i++) o2[i] = h0[1 + i];
    o2[7] = h1[0];
#pragma unroll
    for (int i = 0; i < 7; i++) o3[i] = h1[1 + i];
    o3[7] = (half_t)1.0f;
    half8_t* out = reinterpret_cast<half8_t*>(cin + (size_t)b * 32);
    out[0] = o0; out[1] = o1; out[2] = o2; out[3] = o3;
}

__global__ __launch_bounds__(256) void curved_mid_forward_kernel(const half_t* __restrict__ h, const float* __restrict__ normal, const float* __restrict__ dirs,
                                                                uint32_t B, const float fc, const int eval, half_t* __restrict__ sigma,
                                                                half_t* __restrict__ cin) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    curved_mid_row(b, h, normal, dirs, fc, eval, sigma, cin);
}

// hc: the colour net's output rows (3 of `stride` halfs used), sigma_raw [B] half, mask [B] bytes
//   -> sigma [B] half = mask ? sigma_raw : 0,  color [B,3] half = mask ? half(sigmoid(hc)) : 0
//   O: half, or float = the half values widened (what the framework's `.float()` on the half outputs gives)
template <typename O>
__device__ __forceinline__ void curved_out_row(const uint32_t b, const half_t* __restrict__ hc, uint32_t stride, const half_t* __restrict__ sigma_raw,
                                               const uint8_t* __restrict__ mask, O* __restrict__ sigma, O* __restrict__ color) {
    const bool m = mask[b] != 0;
    sigma[b] = (O)(m ? sigma_raw[b] : (half_t)0.0f);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float x = (float)hc[(size_t)b * stride + c];
        color[(size_t)b * 3 + c] = (O)(m ? narrow(1.0f / (1.0f + expf(-x))) : (half_t)0.0f);
    }
}

__global__ __launch_bounds__(256) void curved_out_forward_kernel(const half_t* __restrict__ hc, uint32_t stride, const half_t* __restrict__ sigma_raw,
                                                                const uint8_t* __restrict__ mask, uint32_t B, half_t* __restrict__ sigma,
                                                                half_t* __restrict__ color) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    curved_out_row<half_t>(b, hc, stride, sigma_raw, mask, sigma, color);
}

// ---- the rows forms of nerftex_curved_field_infer: the same rows for the live, unmarked slots of an inference iteration --------------------------------

// the gather's level-major features x_lbc [8, B, 2] half -> columns 0..15 of the sigma net's input xin [B,48] (columns 16..47 are the projector's)
__global__ __launch_bounds__(256) void curved_pack_features_rows_kernel(const half_t* __restrict__ x_lbc, uint32_t B, half_t* __restrict__ xin,
                                                                       const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= live_rows(B, units_dev, rows_per_unit)) return;
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    u4 w[2];
#pragma unroll
    for (int l = 0; l < 8; l++) w[l / 4][l % 4] = *reinterpret_cast<const uint32_t*>(x_lbc + ((size_t)l * B + b) * 2);
    u4* dst = reinterpret_cast<u4*>(xin + (size_t)b * 48);
    dst[0] = w[0]; dst[1] = w[1];
}

__global__ __launch_bounds__(256) void curved_mid_rows_kernel(const half_t* __restrict__ h, const float* __restrict__ normal, const float* __restrict__ dirs,
                                                             uint32_t B, const float fc, const int eval, half_t* __restrict__ sigma, half_t* __restrict__ cin,
                                                             const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= live_rows(B, units_dev, rows_per_unit) || slot_unused(dirs, b)) return;  // (a marked row's cin stays what the scratch held: rows are independent)
    curved_mid_row(b, h, normal, dirs, fc, eval, sigma, cin);
}

// ... and the chain's outputs as fp32: a marked row is exactly sigma = 0, rgb = 0 whatever the networks made of its stale inputs
__global__ __launch_bounds__(256) void curved_out_rows_kernel(const half_t* __restrict__ hc, const half_t* __restrict__ sigma_raw, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ dirs, uint32_t B, float* __restrict__ sigma, float* __restrict__ rgbs,
                                                             const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= live_rows(B, units_dev, rows_per_unit)) return;
    if (slot_unused(dirs, b)) {
        sigma[b] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) rgbs[(size_t)b * 3 + c] = 0.0f;
        return;
    }
    curved_out_row<float>(b, hc, 16, sigma_raw, mask, sigma, rgbs);
}

// ---- the light mid of nerftex_curved_light_infer (the SH light model's chain; its closing kernel and the entry point: curved_light.inc) ------------------
// The factorized fine-normal net (tools/map.py:231-337 as FactorizedNormalNet executes it under fp16 autocast): two LipMLPs in -> 16 -> 16 -> 1.
constexpr int kNnH = 16, kNnBands = 12, kNnPhiIn = 8 + kNnBands, kNnThetaIn = 16 + kNnBands;
constexpr int kNnPhiWeights = kNnH * kNnPhiIn + kNnH * kNnH + kNnH, kNnThetaWeights = kNnH * kNnThetaIn + kNnH * kNnH + kNnH;
constexpr int kNnWeights = kNnPhiWeights + kNnThetaWeights, kNnNetBiases = 2 * kNnH + 1, kNnBiases = 2 * kNnNetBiases;
static_assert(kNnWeights == NERFTEX_NORMAL_NET_WEIGHTS && kNnBiases == NERFTEX_NORMAL_NET_BIASES, "the packed block of include/nerftex_hip.h");

// One LipLayer product as the framework's half GEMM: x and w hold half VALUES (their products are exact in fp32), added in ascending input order in
// fp32, the sum rounded to half; the bias is added and the ReLU applied in fp32.  FP CONTRACTION: off, as in curved_mid_row -- an fma of an exact
// product is the same rounding, but bias, ReLU and everything behind the net are framework ops that round on their own.
template <int IN>
__device__ __forceinline__ float lip_dot(const float (&x)[IN], const float* __restrict__ w) {
#pragma clang fp contract(off)
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < IN; i++) acc = acc + w[i] * x[i];
    return (float)narrow(acc);
}

template <int IN>
__device__ __forceinline__ float lip_mlp_row(const float (&x)[IN], const float* __restrict__ w, const float* __restrict__ bias) {
#pragma clang fp contract(off)
    float a[kNnH], c[kNnH];
#pragma unroll
    for (int o = 0; o < kNnH; o++) {
        const float y = lip_dot<IN>(x, w + o * IN) + bias[o];
        a[o] = (float)narrow(y < 0.0f ? 0.0f : y);  // (the next layer's GEMM takes half inputs; torch.relu keeps a NaN and so does this)
    }
    w += kNnH * IN;
#pragma unroll
    for (int o = 0; o < kNnH; o++) {
        const float y = lip_dot<kNnH>(a, w + o * kNnH) + bias[kNnH + o];
        c[o] = (float)narrow(y < 0.0f ? 0.0f : y);
    }
    return lip_dot<kNnH>(c, w + kNnH * kNnH) + bias[2 * kNnH];
}

// h [B,16] half (the sigma net's output), xin [B,48] half (texture features | height bands | ones), n_lbc [4,B,2] half (the normal table's features,
// level-major), normal [B,3] the projector's RAW coarse normal, tbn [B,9] the hit face's frame, w / bias: the net's weights (half values) and biases in LDS
//   -> sigma_raw [B] fp32 = exp(h[:,0])  (trunc_exp on the half logit widened: _sigma() keeps it fp32)
//      brdf_in [B,16] half = [h[:,1:16] | 1]
//      shading [B,3] fp32: toCoor(phi, theta) rotated by the frame (a half product), normalised twice (tools/map.py:732, network_curvedfield.py:285);
//      eval: fc x fine + (1 - fc) x coarse, renormalised (:293-301), coarse = the raw normal normalised twice (tools/map.py:720, :285)
// TWO (the imported map's chain, planar_light.inc): tbn2 [B,9] is a second frame the rotated normal is rotated by once more (tools/map.py:726-727, the
// sampled patch's inverted frame), the same half product on the first one's half result -- the reference rounds between the two, so the frames are
// not multiplied together.  Without it (the mesh chain) tbn2 is not read.
// FRAMES = 3 (the imported map on a new mesh, shape_light.inc): tbn3 [B,9], the new mesh's hit face's frame, rotates the second rotation's half
// result once more (tools/map.py:728-729) -- the same half product again.  FRAMES counts the rotations: 1 the mesh chain, 2 the planar maps.
template <int FRAMES>
__device__ __forceinline__ void curved_light_mid_row(const uint32_t b, const uint32_t B, const half_t* __restrict__ h, const half_t* __restrict__ xin,
                                                     const half_t* __restrict__ n_lbc, const float* __restrict__ normal, const float* __restrict__ tbn,
                                                     const float* __restrict__ tbn2, const float* __restrict__ tbn3, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float fc, const int eval,
                                                     float* __restrict__ sigma_raw, half_t* __restrict__ brdf_in, float* __restrict__ shading) {
#pragma clang fp contract(off)  // every framework op rounds on its own
    const half8_t h0 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16);
    const half8_t h1 = *reinterpret_cast<const half8_t*>(h + (size_t)b * 16 + 8);
    sigma_raw[b] = expf((float)h0[0]);
    half8_t o0, o1;
#pragma unroll
    for (int i = 0; i < 7; i++) o0[i] = h0[1 + i];
    o0[7] = h1[0];
#pragma unroll
    for (int i = 0; i < 7; i++) o1[i] = h1[1 + i];
    o1[7] = (half_t)1.0f;  // tcnn pads its inputs with ones
    half8_t* out = reinterpret_cast<half8_t*>(brdf_in + (size_t)b * 16);
    out[0] = o0; out[1] = o1;

    const half8_t x0 = *reinterpret_cast<const half8_t*>(xin + (size_t)b * 48);
    const half8_t x1 = *reinterpret_cast<const half8_t*>(xin + (size_t)b * 48 + 8);
    const half8_t z0 = *reinterpret_cast<const half8_t*>(xin + (size_t)b * 48 + 16);
    const half4_t z1 = *reinterpret_cast<const half4_t*>(xin + (size_t)b * 48 + 24);
    float phi_in[kNnPhiIn], theta_in[kNnThetaIn];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const half2_t f = *reinterpret_cast<const half2_t*>(n_lbc + ((size_t)l * B + b) * 2);
        phi_in[2 * l] = (float)f[0];
        phi_in[2 * l + 1] = (float)f[1];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        theta_in[i] = (float)x0[i];
        theta_in[8 + i] = (float)x1[i];
    }
#pragma unroll
    for (int i = 0; i < kNnBands; i++) {
        const float z = i < 8 ? (float)z0[i] : (float)z1[i - 8];
        phi_in[8 + i] = z;
        theta_in[16 + i] = z;
    }
    const float phi = lip_mlp_row<kNnPhiIn>(phi_in, w, bias);
    const float theta = lip_mlp_row<kNnThetaIn>(theta_in, w + kNnPhiWeights, bias + kNnNetBiases);
    const float st = sinf(theta);
    const float local[3] = {st * cosf(phi), st * sinf(phi), cosf(theta)};  // toCoor
    // einsum("nba,nb->na", frame, local) under autocast: a half product -- both operands rounded to half, fp32 sum in ascending b, rounded to half
    float lh[3], th[9], n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) lh[k] = (float)narrow(local[k]);
#pragma unroll
    for (int k = 0; k < 9; k++) th[k] = (float)(half_t)tbn[(size_t)b * 9 + k];
#pragma unroll
    for (int a = 0; a < 3; a++) n[a] = (float)narrow((th[a] * lh[0] + th[3 + a] * lh[1]) + th[6 + a] * lh[2]);
    if constexpr (FRAMES >= 2) {
#pragma unroll
        for (int k = 0; k < 3; k++) lh[k] = n[k];  // (half values already)
#pragma unroll
        for (int k = 0; k < 9; k++) th[k] = (float)(half_t)tbn2[(size_t)b * 9 + k];
#pragma unroll
        for (int a = 0; a < 3; a++) n[a] = (float)narrow((th[a] * lh[0] + th[3 + a] * lh[1]) + th[6 + a] * lh[2]);
    }
    if constexpr (FRAMES >= 3) {
#pragma unroll
        for (int k = 0; k < 3; k++) lh[k] = n[k];  // (the second rotation's half result as it is)
#pragma unroll
        for (int k = 0; k < 9; k++) th[k] = (float)(half_t)tbn3[(size_t)b * 9 + k];
#pragma unroll
        for (int a = 0; a < 3; a++) n[a] = (float)narrow((th[a] * lh[0] + th[3 + a] * lh[1]) + th[6 + a] * lh[2]);
    }
    auto unit = [](float (&v)[3]) {  // v / (|v| + 1e-5)
        const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-5f;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = v[c] / len;
    };
    unit(n);
    unit(n);
    if (eval & 1) {
        float cn[3];
#pragma unroll
        for (int c = 0; c < 3; c++) cn[c] = normal[(size_t)b * 3 + c];
        unit(cn);
        unit(cn);
#pragma unroll
        for (int c = 0; c < 3; c++) n[c] = fc * n[c] + (1 - fc) * cn[c];
        unit(n);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) shading[(size_t)b * 3 + c] = n[c];
}

// One thread per row.  The net's weights (1312 half values, 66 biases: 5.4 KiB as fp32) are staged once per workgroup in LDS -- every lane of a wave
// reads the same word at the same time (a broadcast, no bank conflict), and 1.3 k words per row would not stay in scalar registers.  A workgroup wholly
// past the live rows leaves before it stages anything.  FRAMES: curved_light_mid_row's count of rotations (tbn, then tbn2, then tbn3).
template <int FRAMES>
__global__ __launch_bounds__(256) void curved_light_mid_rows_kernel(const half_t* __restrict__ h, const half_t* __restrict__ xin, const half_t* __restrict__ n_lbc,
                                                                   const float* __restrict__ normal, const float* __restrict__ tbn, const float* __restrict__ tbn2,
                                                                   const float* __restrict__ tbn3, const float* __restrict__ dirs,
                                                                   const half_t* __restrict__ nn_weights, const float* __restrict__ nn_biases, uint32_t B,
                                                                   const float fc, const int eval, float* __restrict__ sigma_raw, half_t* __restrict__ brdf_in,
                                                                   float* __restrict__ shading, const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    __shared__ float w_s[kNnWeights];
    __shared__ float b_s[kNnBiases];
    const uint32_t live = live_rows(B, units_dev, rows_per_unit);
    if (blockIdx.x * blockDim.x >= live) return;  // (the whole workgroup: nobody is left waiting at the barrier)
    for (uint32_t i = threadIdx.x; i < (uint32_t)kNnWeights; i += blockDim.x) w_s[i] = (float)nn_weights[i];
    if (threadIdx.x < (uint32_t)kNnBiases) b_s[threadIdx.x] = nn_biases[threadIdx.x];
    __syncthreads();
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= live) return;
    if (slot_unused(dirs, b)) {  // (its sigma_raw and brdf_in stay what the scratch held: rows are independent, the closing kernel writes the zeros)
#pragma unroll
        for (int c = 0; c < 3; c++) shading[(size_t)b * 3 + c] = 0.0f;
        return;
    }
    curved_light_mid_row<FRAMES>(b, B, h, xin, n_lbc, normal, tbn, tbn2, tbn3, w_s, b_s, fc, eval, sigma_raw, brdf_in, shading);
}

// ---- the front half nerftex_curved_field_infer and nerftex_curved_light_infer (curved_light.inc) share: neighbour search to sigma net ------------------

// carves the caller's scratch into per-row buffers, each starting on a 256-byte boundary (base 0: the offsets alone, `at` ends as the size)
struct ScratchCarver {
    uintptr_t base;
    size_t B, at = 0;
    template <typename T>
    T* take(size_t values_per_row) {
        T* here = reinterpret_cast<T*>(base + at);
        at += (B * values_per_row * sizeof(T) + 255) / 256 * 256;
        return here;
    }
};

inline bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

// the buffers of the front half; each entry's scratch carves them first and its own behind them
struct CurvedFront {
    int32_t* idx;
    float *dist, *p_sur, *normal;
    uint8_t* mask;
    half_t *x_lbc, *xin, *h;
    explicit CurvedFront(ScratchCarver& c)
        : idx(c.take<int32_t>(16)), dist(c.take<float>(16)),  // (sized for the largest K)
          p_sur(c.take<float>(3)), normal(c.take<float>(3)), mask(c.take<uint8_t>(1)), x_lbc(c.take<half_t>(16)), xin(c.take<half_t>(48)), h(c.take<half_t>(16)) {}
};

// the buffers of the back half nerftex_curved_field_infer and nerftex_curved_import_infer (planar.inc) share: mid kernel to the closing kernel
struct CurvedBack {
    half_t *sigma_raw, *cin, *hc;
    explicit CurvedBack(ScratchCarver& c) : sigma_raw(c.take<half_t>(1)), cin(c.take<half_t>(32)), hc(c.take<half_t>(16)) {}
};

// the buffers of the back half the three lit entries (curved_light.inc, planar_light.inc, shape_light.inc) share: light mid kernel to the closing kernel
struct LightBack {
    float* sigma_raw;
    half_t *brdf_in, *brdf;
    float* shading;  // (used when the caller does not ask for the shading normal)
    explicit LightBack(ScratchCarver& c) : sigma_raw(c.take<float>(1)), brdf_in(c.take<half_t>(16)), brdf(c.take<half_t>(16)), shading(c.take<float>(3)) {}
};

// the leading buffers of the two shape entries (planar.inc, shape_light.inc): neighbour search, shape lookup, sigma net
struct ShapeFront {
    int32_t* idx;
    float* dist;
    uint8_t* mask;
    float* normal;
    half_t *xin, *h;
    explicit ShapeFront(ScratchCarver& c)
        : idx(c.take<int32_t>(16)), dist(c.take<float>(16)),  // (sized for the largest K)
          mask(c.take<uint8_t>(1)), normal(c.take<float>(3)), xin(c.take<half_t>(48)), h(c.take<half_t>(16)) {}
};

// the scratch of one nerftex_curved_field_infer call
struct CurvedScratch {
    ScratchCarver carve;
    CurvedFront f;
    CurvedBack back;
    CurvedScratch(void* scratch, size_t B) : carve{reinterpret_cast<uintptr_t>(scratch), B}, f(carve), back(carve) {}
};

// The refusals over the descriptors' shared members (knn .. in_mul, the sigma net, scratch), in the order include/nerftex_hip.h documents: each
// entry calls them one after the other and puts its own conditions beside them.  `who`: the entry's name in the messages.
// batch_ok: what every device-count entry asks first, the ones without a mesh (the import entries) too.
template <typename Desc>
bool batch_ok(const Desc* d, const char* who) {
    if (!d) {
        set_error("%s: NULL descriptor", who);
        return false;
    }
    if (d->B % 128 != 0) {
        set_error("%s: the batch must be a multiple of 128 rows, but got %u", who, d->B);
        return false;
    }
    return true;
}

template <typename Desc>
bool front_batch_ok(const Desc* d, const char* who) {
    if (!batch_ok(d, who)) return false;
    if (d->B != 0 && (d->n_verts == 0 || d->n_verts > 0x7fffffffu)) {
        set_error("%s: the mesh needs between 1 and 2^31 - 1 vertices, but got %u", who, d->n_verts);
        return false;
    }
    if (d->K == 0 || d->K > 16) {
        set_error("%s: 1 <= K <= 16 neighbours per point, but got %u", who, d->K);
        return false;
    }
    return true;
}

// (no message: the entry names its whole set of shapes in one refusal)
template <typename Desc>
bool front_shapes_ok(const Desc* d) {
    return d->n_freqs == 12 && d->D == 3 && d->C == 2 && d->L == 8 && d->sigma_in == 48 && d->sigma_hidden == 32 && d->sigma_layers == 2 && d->sigma_out == 16;
}

// (tbn is the light entry's to ask for: the static light model does not read the frames)
template <typename Desc>
bool front_pointers_ok(const Desc* d, size_t scratch_bytes) {
    return d->knn && d->tracer && d->xyz && d->dirs && d->mesh_vertices && d->vertex_normals && d->table && d->offsets && d->sigma_weights && d->sigma && d->rgbs &&
           d->scratch && !(reinterpret_cast<uintptr_t>(d->scratch) & 255) && d->scratch_bytes >= scratch_bytes;
}

template <typename Desc>
bool front_scales_ok(const Desc* d) {
    return aligned16(d->sigma_weights) && d->in_mul > 0.0f && std::isfinite(d->in_mul);
}

// The launches of the front half, in two parts: the light entry gathers its normal table between them.
// neighbour search -> projector (tbn_out: the hit face's frame, or NULL: no frame is read or written) -> gather of the texture table
template <typename Desc>
int curved_front_gather(const Desc* d, const CurvedFront& f, float* tbn_out, void* stream) {
    int rc = knn_query_rows(d->knn, d->xyz, d->dirs, d->B, d->K, f.idx, f.dist, d->units_dev, d->rows_per_unit, as_stream(stream));
    if (rc != NERFTEX_OK) return rc;
    rc = curved_project_rows(d->tracer, d->xyz, d->dirs, f.idx, f.dist, d->B, d->K, d->mesh_vertices, d->vertex_normals, d->n_verts, d->dir_vec_wdist,
                             d->h_threshold, f.p_sur, f.mask, f.normal, f.xin, d->units_dev, d->rows_per_unit, as_stream(stream), tbn_out ? d->tbn : nullptr,
                             tbn_out);
    if (rc != NERFTEX_OK) return rc;
    // (an exported entry of this library: it clears the error text, which holds nothing at this point, and checks the gather's own arguments)
    return nerftex_grid_encode_forward_rows(f.p_sur, d->table, d->offsets, f.x_lbc, d->B, d->D, d->C, d->L, d->S, d->H, d->gridtype, d->align_corners, NERFTEX_F16,
                                            NERFTEX_LAYOUT_LBC, d->in_add, d->in_mul, d->units_dev, d->rows_per_unit, stream);
}

// pack -> sigma net 48 -> 32 x 2 -> 16;  pack_label: the entry's check_launch label of the pack kernel
template <typename Desc>
int curved_front_sigma(const Desc* d, const CurvedFront& f, const char* pack_label, void* stream) {
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("curved_pack_features_rows_kernel", st);
        hipLaunchKernelGGL(curved_pack_features_rows_kernel, dim3(div_up(d->B, 256u)), dim3(256), 0, st, f.x_lbc, d->B, f.xin, d->units_dev, d->rows_per_unit);
    }
    const int rc = check_launch(pack_label);
    if (rc != NERFTEX_OK) return rc;
    return ffmlp_inference_rows(f.xin, d->sigma_weights, d->B, 48, 32, 2, f.h, d->units_dev, d->rows_per_unit, st);
}

// (no message, as front_shapes_ok)
template <typename Desc>
bool back_shapes_ok(const Desc* d) {
    return d->color_in == 32 && d->color_hidden == 64 && d->color_layers == 3 && d->color_out == 3;
}

// The launches of the back half: mid (trunc_exp, the reflected view direction, SH) -> colour net 32 -> 64 x 3 -> 3 -> sigmoid + mask as fp32.
// h [B,16]: the sigma net's output, normal [B,3]: the raw coarse normal, mask [B]; labels: the entry's check_launch labels of the two kernels.
template <typename Desc>
int curved_back_half(const Desc* d, const half_t* h, const float* normal, const uint8_t* mask, const CurvedBack& k, const char* const (&labels)[2], void* stream) {
    hipStream_t st = as_stream(stream);
    const uint32_t B = d->B, rpu = d->rows_per_unit;
    const int32_t* units = d->units_dev;
    const dim3 grid(div_up(B, 256u)), block(256);
    {
        KernelTimer kt("curved_mid_rows_kernel", st);
        hipLaunchKernelGGL(curved_mid_rows_kernel, grid, block, 0, st, h, normal, d->dirs, B, d->fc_weight, d->eval, k.sigma_raw, k.cin, units, rpu);
    }
    int rc = check_launch(labels[0]);
    if (rc != NERFTEX_OK) return rc;
    rc = ffmlp_inference_rows(k.cin, d->color_weights, B, 32, 64, 3, k.hc, units, rpu, st);
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt("curved_out_rows_kernel", st);
        hipLaunchKernelGGL(curved_out_rows_kernel, grid, block, 0, st, k.hc, k.sigma_raw, mask, d->dirs, B, d->sigma, d->rgbs, units, rpu);
    }
    return check_launch(labels[1]);
}

}  // namespace
}  // namespace nerftex

using namespace nerftex;

extern "C" int nerftex_curved_pack_inputs(const void* x_embed, const float* z_embed, uint32_t B, void* out, void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("curved_pack_inputs_kernel", st);
        hipLaunchKernelGGL(curved_pack_inputs_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, static_cast<const half_t*>(x_embed), z_embed, B, static_cast<half_t*>(out));
    }
    return check_launch("curved_pack_inputs");
}

extern "C" int nerftex_curved_mid_forward(const void* h, const float* normal, const float* dirs, uint32_t B, float fc_weight, int eval, void* sigma, void* cin,
                                          void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("curved_mid_forward_kernel", st);
        hipLaunchKernelGGL(curved_mid_forward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, static_cast<const half_t*>(h), normal, dirs, B, fc_weight, eval,
                           static_cast<half_t*>(sigma), static_cast<half_t*>(cin));
    }
    return check_launch("curved_mid_forward");
}

extern "C" int nerftex_curved_out_forward(const void* hc, uint32_t row_stride, const void* sigma_raw, const uint8_t* mask, uint32_t B, void* sigma, void* color,
                                          void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    if (row_stride < 3) {
        set_error("curved_out_forward: the colour rows hold at least 3 values");
        return NERFTEX_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("curved_out_forward_kernel", st);
        hipLaunchKernelGGL(curved_out_forward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, static_cast<const half_t*>(hc), row_stride,
                           static_cast<const half_t*>(sigma_raw), mask, B, static_cast<half_t*>(sigma), static_cast<half_t*>(color));
    }
    return check_launch("curved_out_forward");
}

extern "C" size_t nerftex_curved_field_infer_scratch_bytes(uint32_t B) { return CurvedScratch(nullptr, B).carve.at; }

extern "C" int nerftex_curved_field_infer(const nerftex_curved_infer_desc* d, void* stream) {
    clear_error();
    if (!front_batch_ok(d, "curved_field_infer")) return NERFTEX_ERR_INVALID;
    if (!front_shapes_ok(d) || !back_shapes_ok(d)) {
        set_error("curved_field_infer: the kernels serve the default curved field only (12 height bands, a 3-D table of 8 levels x 2 features, "
                  "sigma net 48 -> 32 x 2 -> 16, colour net 32 -> 64 x 3 -> 3)");
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0) return NERFTEX_OK;
    const CurvedScratch sc(d->scratch, d->B);
    if (!front_pointers_ok(d, sc.carve.at) || !d->color_weights) {
        set_error("curved_field_infer: handles, inputs, table, weights and outputs must not be NULL, and scratch must be 256-byte aligned and hold %zu bytes",
                  sc.carve.at);
        return NERFTEX_ERR_INVALID;
    }
    if (!front_scales_ok(d) || !aligned16(d->color_weights)) {
        set_error("curved_field_infer: the weight vectors must be 16-byte aligned and the gather's input scale positive and finite");
        return NERFTEX_ERR_INVALID;
    }
    int rc = curved_front_gather(d, sc.f, nullptr, stream);
    if (rc != NERFTEX_OK) return rc;
    if ((rc = curved_front_sigma(d, sc.f, "curved_field_infer(pack)", stream)) != NERFTEX_OK) return rc;
    static const char* const labels[2] = {"curved_field_infer(mid)", "curved_field_infer(out)"};
    return curved_back_half(d, sc.f.h, sc.f.normal, sc.f.mask, sc.back, labels, stream);
}

extern "C" int nerftex_field_mid_forward(const void* h, const float* dirs, uint32_t B, float* sigma, void* cin, void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("field_mid_forward_kernel", st);
        hipLaunchKernelGGL(field_mid_forward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, static_cast<const half_t*>(h), dirs, B, sigma,
                           static_cast<half_t*>(cin));
    }
    return check_launch("field_mid_forward");
}

extern "C" int nerftex_field_mid_backward(const float* grad_sigma, const void* grad_cin, const void* h, uint32_t B, void* grad_h, void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("field_mid_backward_kernel", st);
        hipLaunchKernelGGL(field_mid_backward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, grad_sigma, static_cast<const half_t*>(grad_cin),
                           static_cast<const half_t*>(h), B, static_cast<half_t*>(grad_h));
    }
    return check_launch("field_mid_backward");
}

extern "C" int nerftex_field_out_forward(const void* hc, uint32_t B, float* rgbs, void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("field_out_forward_kernel", st);
        hipLaunchKernelGGL(field_out_forward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, static_cast<const half_t*>(hc), B, rgbs);
    }
    return check_launch("field_out_forward");
}

extern "C" int nerftex_field_out_backward(const float* grad_rgbs, const float* rgbs, uint32_t B, void* grad_hc, void* stream) {
    clear_error();
    if (B == 0) return NERFTEX_OK;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("field_out_backward_kernel", st);
        hipLaunchKernelGGL(field_out_backward_kernel, dim3(div_up(B, 256u)), dim3(256), 0, st, grad_rgbs, rgbs, B, static_cast<half_t*>(grad_hc));
    }
    return check_launch("field_out_backward");
}

// ---- the planar lookup of an imported feature map and its chain (nerftex_planar_lookup, nerftex_curved_import_infer): in front of shlight.inc ------------
#include "planar.inc"

// ---- the field baked onto the vertices of a fine mesh (nerftex_curved_unhash_infer): the vertex lookup (raytracer.hip) in front of the static back half --
#include "unhash.inc"

// ---- the SH light head of the curved field (nerftex_sh_light_forward / _backward) ----------------------------------------------------------------------
#include "shlight.inc"

// ---- the SH light model's inference chain (nerftex_curved_light_infer): its closing kernel shares the head's row function above ----------------------------
#include "curved_light.inc"

// ---- the imported map under the SH light model (nerftex_planar_light_lookup, nerftex_curved_light_import_infer): behind both -----------------------------
#include "planar_light.inc"

// ---- the imported map on a new mesh under the SH light model (nerftex_curved_light_shape_infer): the lit shape lookup (raytracer.hip) in front ----------
#include "shape_light.inc"

// ---- an imported feature patch (nerftex_curved_patch_infer, nerftex_curved_light_patch_infer): the patch lookup (knn.hip) in front of either back half ----
#include "patch_chain.inc"

// ---- fitting SH lighting to an imported environment map (nerftex_envmap_fit): svox2_basis9 comes from shlight.inc -----------------------------------------
#include "envmap.inc"

// ---- the per-probe visibility lighting of an imported map (nerftex_envmap_vis_fit): svox2_basis9 and AdamConsts come from the two above -------------------
#include "envmap_vis.inc"
