// Body of ffmlp.hip, compiled once per storage type (elem_t = _Float16 | __bf16; elem4_t / elem8_t its vectors; mfma16 the matching
// v_mfma_f32_16x16x32 instruction): kernels, launchers and the three entry points.  See ffmlp.hip for the design notes.

constexpr int kBlockThreads = 256;  // 4 waves, one per SIMD
constexpr int kTilesPerWave = 2;    // 2 x 16 batch rows per wave iteration (two independent MFMA chains)
constexpr int kRowsPerBlock = 4 * 16 * kTilesPerWave;  // 128, the reference's batch granule too
constexpr float kAct = 10.0f;       // K_ACT of utils.h:41

enum Act : uint32_t { kRelu = 0, kExp = 1, kSine = 2, kSigmoid = 3, kSquareplus = 4, kSoftplus = 5, kNone = 6 };

__device__ __forceinline__ float act_forward(uint32_t a, float x) {
    switch (a) {
        // integer max on the bit pattern: negative floats (sign bit set, -0 included) are negative ints -> +0, positive ones pass through.
        // One v_max_i32; the float compare-select form comes out as v_max_f32 plus a canonicalising v_max_f32 x, x per element
        case kRelu: return __builtin_bit_cast(float, max(__builtin_bit_cast(int, x), 0));
        case kExp: return expf(x);
        case kSine: return sinf(x);
        case kSigmoid: return 1.0f / (1.0f + expf(-x));
        case kSquareplus: { const float s = x * kAct; return 0.5f * (s + sqrtf(s * s + 4.0f)) / kAct; }
        case kSoftplus: return logf(expf(x * kAct) + 1.0f) / kAct;
        default: return x;
    }
}
// gradient through the activation, expressed with the stored POST-activation value y (utils.h:537-582)
__device__ __forceinline__ float act_backward(uint32_t a, float g, float y) {
    switch (a) {
        case kRelu: return y > 0.0f ? g : 0.0f;
        case kExp: return g * y;
        case kSigmoid: return g * (float)(elem_t)(y * (1.0f - y));
        case kSquareplus: { const float s = y * kAct; return g * (float)(elem_t)(s * s / (s * s + 1.0f)); }
        case kSoftplus: return g * (float)(elem_t)(1.0f - expf(-y * kAct));
        default: return g;  // none, and sine (the reference leaves the gradient untouched, utils.h:552-556)
    }
}

// ACT >= 0: activation known at compile time (the switch folds away -- with a run-time id every element drags a chain of scalar
// compares and branches through all seven formulas: 1100 branches per 32-row step of the fused backward); ACT < 0: run-time id
template <int ACT>
__device__ __forceinline__ float act_fwd(uint32_t act_rt, float x) {
    if constexpr (ACT >= 0) return act_forward((uint32_t)ACT, x);
    else return act_forward(act_rt, x);
}
template <int ACT>
__device__ __forceinline__ float act_bwd(uint32_t act_rt, float g, float y) {
    if constexpr (ACT >= 0) return act_backward((uint32_t)ACT, g, y);
    else return act_backward(act_rt, g, y);
}


// contraction-index map of a 32-deep operand slot (lane group g = lane>>4, element j<8)
//   natural : operand comes from row-major memory, 8 consecutive k per lane
//   permuted: operand is rebuilt from two 16x16 result tiles held in registers (see file header)
__device__ __forceinline__ int kmap(bool permuted, int ks, int g, int j) {
    return permuted ? 32 * ks + 16 * (j >> 2) + 4 * g + (j & 3) : 32 * ks + 8 * g + j;
}

// Stage the A-operand fragments of a matrix view A[m][k] (M x K, M % 16 == 0) into LDS.
//   element (m,k) = transposed ? W[k*ldw + m] : W[m*ldw + k];  k >= K pads with zero.
// Layout: fragment (mt, ks) at ((mt*KS + ks)*64 + lane) * 16 bytes -> one ds_read_b128 per lane, no conflicts.
// Loads are 8- or 16-byte pieces of the row-major weights (rows start 32-byte aligned: ldw % 16 == 0, checked at the entry points):
// element-wise 2-byte gathers go through the texture-address path at about one LANE per clock -- 7-14 k of them per workgroup, four
// workgroups per CU, were 12 us of a 24 us inference launch.
//   as stored  : a lane's 8 values are one 16-byte run of row m (natural k order) or two 8-byte runs (permuted)
//   transposed : a thread takes 8 consecutive m of one k (one 16-byte load) and scatters them into the table with 2-byte LDS stores
__device__ void stage_fragments(elem8_t* __restrict__ dst, const elem_t* __restrict__ W, int ldw, bool transposed, int M, int K,
                                bool permuted) {
    const int KS = (K + 31) / 32;
    const elem8_t zero8{0, 0, 0, 0, 0, 0, 0, 0};
    if (!transposed) {
        const int total = (M / 16) * KS * 64;
        for (int s = threadIdx.x; s < total; s += kBlockThreads) {
            const int frag = s >> 6, lane = s & 63;
            const int mt = frag / KS, ks = frag - mt * KS;
            const int m = 16 * mt + (lane & 15), g = lane >> 4;
            const elem_t* row = W + (size_t)m * ldw;
            elem8_t v;
            if (!permuted) {
                const int k0 = 32 * ks + 8 * g;
                v = k0 < K ? *reinterpret_cast<const elem8_t*>(row + k0) : zero8;
            } else {
                const int ka = 32 * ks + 4 * g, kb = ka + 16;
                const elem4_t z4{0, 0, 0, 0};
                const elem4_t lo = ka < K ? *reinterpret_cast<const elem4_t*>(row + ka) : z4;
                const elem4_t hi = kb < K ? *reinterpret_cast<const elem4_t*>(row + kb) : z4;
                v = elem8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            dst[s] = v;
        }
    } else {
        elem_t* d = reinterpret_cast<elem_t*>(dst);
        const int MP = M / 8;
        for (int s = threadIdx.x; s < KS * 32 * MP; s += kBlockThreads) {
            const int k = s / MP, m0 = 8 * (s - k * MP);
            const elem8_t v = k < K ? *reinterpret_cast<const elem8_t*>(W + (size_t)k * ldw + m0) : zero8;
            const int ks = k >> 5, kk = k & 31;
            const int g = permuted ? (kk & 15) >> 2 : kk >> 3;        // inverse of kmap
            const int j = permuted ? 4 * (kk >> 4) + (kk & 3) : kk & 7;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int m = m0 + i;
                d[((size_t)((m >> 4) * KS + ks) * 64 + (m & 15) + 16 * g) * 8 + j] = v[i];
            }
        }
    }
}

__host__ __device__ constexpr int frag_count(int M, int K) { return (M / 16) * ((K + 31) / 32); }

// two fp32 result tiles (rows 4g+j of tiles 2s, 2s+1) -> the permuted 32-deep B operand of the next layer
__device__ __forceinline__ elem8_t pack_operand(const float4_t& lo, const float4_t& hi) {
    elem8_t b;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        b[j] = (elem_t)lo[j];
        b[4 + j] = (elem_t)hi[j];
    }
    return b;
}

__device__ __forceinline__ void store4(elem_t* p, const float4_t& v) {
    elem4_t h;
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = (elem_t)v[j];
    *reinterpret_cast<elem4_t*>(p) = h;
}

// ------------------------------------------------------------------------------------------------
// forward / inference
// ------------------------------------------------------------------------------------------------
// STREAM (round 5): networks whose weight fragments do not fit the 160 KB LDS of a CU (hidden 256 with >= 3 layers, hidden 128 with many) keep ONE
// layer's fragments in LDS at a time: before a layer's products the workgroup re-stages that layer from global memory (the weights of such a
// network are 0.3-1 MB: L2-resident) between two barriers -- what the reference's threadblock_layer does for every width (ffmlp.cu:47-129 reads
// the layer's weights from global inside the block loop).  The four waves of a workgroup run the same number of row steps (B % 128 == 0), so the
// barriers inside the row loop are uniform.
// ROWS (nerftex_curved_field_infer): only the first units_dev[0] * rows_per_unit rows carry anything (a launch sized by an upper bound of a count
// that lives on the device).  A workgroup whose 128 rows all lie past them exits before it stages a weight; one that holds the last live row runs
// its whole 128-row step -- rows are independent through the MFMA chain (a batch row is one column of every B operand), so what the rows behind
// the live ones compute from stale scratch touches no live row, and the loop stays uniform across the workgroup's four waves.
template <int HIDDEN, bool INFERENCE, bool STAGED, int ACT, int OUT_ACT, bool STREAM = false, bool ROWS = false>  // STAGED: forward_buffer rows leave through an LDS patch; ACT: see act_fwd
__global__ __launch_bounds__(kBlockThreads) void ffmlp_forward_kernel(const elem_t* __restrict__ X, const elem_t* __restrict__ W,
                                                                      elem_t* __restrict__ fwd, elem_t* __restrict__ out, uint32_t B,
                                                                      uint32_t IN, uint32_t NL, uint32_t act, uint32_t out_act,
                                                                      const int32_t* __restrict__ units_dev, uint32_t rows_per_unit) {
    constexpr int OT = HIDDEN / 16;         // result tiles per hidden layer
    constexpr int KSH = (HIDDEN + 31) / 32;  // 32-deep steps over a hidden layer
    constexpr int NT = kTilesPerWave;
    uint32_t live = B;
    if constexpr (ROWS) {
        live = live_rows(B, units_dev, rows_per_unit);
        if (blockIdx.x * kRowsPerBlock >= live) return;  // (the persistent grid walks upwards from here: nothing below `live` is left to this workgroup)
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem8_t* frags = reinterpret_cast<elem8_t*>(smem);

    const int KS0 = (IN + 31) / 32;
    const int base_hidden = OT * KS0;             // first fragment of matrix 1
    const int per_hidden = OT * KSH;
    const int base_out = base_hidden + (NL - 1) * per_hidden;
    const size_t patch_offset = (size_t)(base_out + KSH) * 1024;  // after the last fragment (16 x HIDDEN output matrix)
    static_assert(!(STREAM && STAGED), "the streaming form stores its activations directly (the LDS holds one layer's fragments and nothing else)");
    if constexpr (!STREAM) {
        stage_fragments(frags, W, IN, false, HIDDEN, IN, false);
        for (uint32_t l = 1; l < NL; l++)
            stage_fragments(frags + (size_t)(base_hidden + (l - 1) * per_hidden) * 64, W + (size_t)HIDDEN * IN + (size_t)(l - 1) * HIDDEN * HIDDEN,
                            HIDDEN, false, HIDDEN, HIDDEN, true);
        stage_fragments(frags + (size_t)base_out * 64, W + (size_t)HIDDEN * IN + (size_t)(NL - 1) * HIDDEN * HIDDEN, HIDDEN, false, 16, HIDDEN,
                        true);
        __syncthreads();
    }
    // the fragments of matrix m (0 = input layer, 1 .. NL-1 = hidden, NL = output): resident, or (STREAM) staged now into the one slot
    auto fragments_of = [&](uint32_t m) -> const elem8_t* {
        if constexpr (STREAM) {
            __syncthreads();  // every wave is done with the slot's previous contents
            if (m == 0) stage_fragments(frags, W, IN, false, HIDDEN, IN, false);
            else if (m < NL) stage_fragments(frags, W + (size_t)HIDDEN * IN + (size_t)(m - 1) * HIDDEN * HIDDEN, HIDDEN, false, HIDDEN, HIDDEN, true);
            else stage_fragments(frags, W + (size_t)HIDDEN * IN + (size_t)(NL - 1) * HIDDEN * HIDDEN, HIDDEN, false, 16, HIDDEN, true);
            __syncthreads();
            return frags;
        } else {
            return m == 0 ? frags : (m < NL ? frags + (size_t)(base_hidden + (m - 1) * per_hidden) * 64 : frags + (size_t)base_out * 64);
        }
    };

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const size_t layer_stride = (size_t)B * HIDDEN;
    // training: a wave's 32 x HIDDEN activation block goes through a private LDS patch so that it leaves as whole rows
    // (1 KiB contiguous per store instruction) instead of 8-B pieces of 16 different rows
    constexpr int kRowPitch = HIDDEN + 8;  // halfs; +16 B keeps ds_read_b128 alignment and staggers the banks
    elem_t* patch = reinterpret_cast<elem_t*>(smem + patch_offset) + (size_t)wave * 16 * NT * kRowPitch;

    // (ROWS: the bound is tested on the workgroup's first row, B % 128 == 0 keeps every row of the step inside the buffers)
    for (uint32_t row0 = blockIdx.x * kRowsPerBlock + wave * 16 * NT; ROWS ? row0 - wave * 16 * NT < live : row0 < B; row0 += gridDim.x * kRowsPerBlock) {
        float4_t acc[NT][OT];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int ot = 0; ot < OT; ot++) acc[t][ot] = float4_t{0, 0, 0, 0};

        // ---- layer 0: B operand straight from the row-major input (16 B per lane, 1 KiB per wave load)
        const elem8_t* f0 = fragments_of(0);
        for (int ks = 0; ks < KS0; ks++) {
            elem8_t b[NT];
            const uint32_t k0 = 32 * ks + 8 * g;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                if (k0 < IN) b[t] = *reinterpret_cast<const elem8_t*>(X + (size_t)(row0 + 16 * t + r) * IN + k0);
                else b[t] = elem8_t{0, 0, 0, 0, 0, 0, 0, 0};
            }
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                const elem8_t a = f0[(size_t)(ot * KS0 + ks) * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t][ot] = mfma16(a, b[t], acc[t][ot]);
            }
        }

        elem8_t bop[NT][KSH];
        for (uint32_t l = 0;; l++) {
            // activation, optional write-out of the post-activation values, repack as next B operand
#pragma unroll
            for (int t = 0; t < NT; t++) {
#pragma unroll
                for (int ot = 0; ot < OT; ot++) {
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[t][ot][j] = act_fwd<ACT>(act, acc[t][ot][j]);
                    if constexpr (!INFERENCE) {
                        if constexpr (STAGED) store4(patch + (size_t)(16 * t + r) * kRowPitch + 16 * ot + 4 * g, acc[t][ot]);
                        else store4(fwd + l * layer_stride + (size_t)(row0 + 16 * t + r) * HIDDEN + 16 * ot + 4 * g, acc[t][ot]);
                    }
                }
#pragma unroll
                for (int s = 0; s < KSH; s++) {
                    const float4_t zero{0, 0, 0, 0};
                    bop[t][s] = pack_operand(acc[t][2 * s], (2 * s + 1 < OT) ? acc[t][(2 * s + 1 < OT) ? 2 * s + 1 : 0] : zero);
                }
            }
            if constexpr (!INFERENCE && STAGED) {  // patch -> forward_buffer[l], 16 B per lane, rows are contiguous in memory
                constexpr int kPieces = HIDDEN / 8;  // 16-B pieces per row
                elem_t* dst = fwd + l * layer_stride + (size_t)row0 * HIDDEN;
#pragma unroll
                for (int it = 0; it < 16 * NT * kPieces / 64; it++) {
                    const int c = it * 64 + lane, row = c / kPieces, piece = c % kPieces;
                    *reinterpret_cast<elem8_t*>(dst + (size_t)row * HIDDEN + 8 * piece) =
                        *reinterpret_cast<const elem8_t*>(patch + (size_t)row * kRowPitch + 8 * piece);
                }
            }
            if (l + 1 >= NL) break;
            // ---- hidden matrix l+1
            const elem8_t* fl = fragments_of(l + 1);
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                float4_t c[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KSH; ks++) {
                    const elem8_t a = fl[(size_t)(ot * KSH + ks) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
                }
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t][ot] = c[t];
            }
        }

        // ---- output layer: 16 (padded) outputs = one result tile
        {
            const elem8_t* fo = fragments_of(NL);
            float4_t c[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < KSH; ks++) {
                const elem8_t a = fo[(size_t)ks * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
#pragma unroll
                for (int j = 0; j < 4; j++) c[t][j] = act_fwd<OUT_ACT>(out_act, c[t][j]);
                store4(out + (size_t)(row0 + 16 * t + r) * 16 + 4 * g, c[t]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The ngp field's whole forward chain behind the hash-grid gather in ONE kernel (SURVEY.md 8(f) N1):
//   level-major features [16, B, 2]  ->  sigma net (32 -> 64 -> 64 -> 16)  ->  trunc_exp of output 0 | geometry features 1..15
//   view direction -> SH degree 4 (16 values)  ->  colour net ([SH | geo | 0] -> 64 -> 64 -> 64 -> 16)  ->  sigmoid of outputs 0..2
// i.e. nerf/network_ff.py:85-101 without its level-major -> row transpose, without the sigma net's outputs, the colour net's
// inputs and the colour net's outputs going through memory between four launches.
//   * the sigma net's first B operand comes straight from the level-major layout the XCD-pinned gather kernel writes: a lane's 8
//     contraction slots are 4 levels x 2 channels = four 4-byte loads (64 B contiguous per 16 rows);
//   * the sigma net's 16 outputs land as one result tile with the batch on the lane axis; the colour net's first operand (a row
//     [SH | h 1..15 | 0] in row-major slot order, so that its first layer sums in the stand-alone kernel's order) takes them from there
//     with eight lane permutes per 16 rows; every lane computes the SH values of its row itself;
//   * same roundings as the four-kernel sequence it replaces (tests compare bit for bit): h rounded to 16 bits once, exp of the
//     rounded logit in fp32, SH in fp32 narrowed once, sigmoid in fp32 narrowed once and widened.
// TRAIN: additionally writes what the (unchanged) backward kernels read: the features as rows [B, 32], h [B, 16], the colour
// net's input [B, 32] and output [B, 16].
__device__ __forceinline__ elem_t narrow16(float v) {
    asm volatile("" : "+v"(v));  // keeps a producing multiply from being folded into the conversion (one rounding instead of two)
    return (elem_t)v;
}

// DENSITY: the sigma net alone (nerf/network_ff.py:103-117, `density`): no directions, no colour net -- the occupancy-grid update's query
template <bool TRAIN, bool DENSITY = false>
__global__ __launch_bounds__(kBlockThreads) void field_forward_kernel(const elem_t* __restrict__ feats, const float* __restrict__ dirs,
                                                                      const elem_t* __restrict__ Ws, const elem_t* __restrict__ Wc, uint32_t B,
                                                                      float* __restrict__ sigma, float* __restrict__ rgbs, elem_t* __restrict__ x_rows,
                                                                      elem_t* __restrict__ h_out, elem_t* __restrict__ cin_out,
                                                                      elem_t* __restrict__ hc_out, const int* __restrict__ units_dev,
                                                                      uint32_t rows_per_unit) {
    constexpr int HIDDEN = 64, IN = 32, OT = 4, KSH = 2, NT = kTilesPerWave;
    // rows past units_dev[0] * rows_per_unit carry nothing (the launch was sized by an upper bound of a count that lives on the device)
    const uint32_t live = units_dev ? min(B, (uint32_t)units_dev[0] * unit_rows(rows_per_unit, (uint32_t)units_dev[0])) : B;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem8_t* frags = reinterpret_cast<elem8_t*>(smem);
    // fragment table: sigma net [W0: 4][W1: 8][Wout: 2], colour net [W0: 4][W1: 8][W2: 8][Wout: 2]
    constexpr int kS0 = 0, kS1 = 4, kSo = 12, kC0 = 14, kC1 = 18, kC2 = 26, kCo = 34;
    stage_fragments(frags + kS0 * 64, Ws, IN, false, HIDDEN, IN, false);
    stage_fragments(frags + kS1 * 64, Ws + HIDDEN * IN, HIDDEN, false, HIDDEN, HIDDEN, true);
    stage_fragments(frags + kSo * 64, Ws + HIDDEN * IN + HIDDEN * HIDDEN, HIDDEN, false, 16, HIDDEN, true);
    if constexpr (!DENSITY) {
        stage_fragments(frags + kC0 * 64, Wc, IN, false, HIDDEN, IN, false);
        stage_fragments(frags + kC1 * 64, Wc + HIDDEN * IN, HIDDEN, false, HIDDEN, HIDDEN, true);
        stage_fragments(frags + kC2 * 64, Wc + HIDDEN * IN + HIDDEN * HIDDEN, HIDDEN, false, HIDDEN, HIDDEN, true);
        stage_fragments(frags + kCo * 64, Wc + HIDDEN * IN + 2 * HIDDEN * HIDDEN, HIDDEN, false, 16, HIDDEN, true);
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    // one hidden matrix: acc <- relu'd operand x fragments
    auto hidden = [&](const elem8_t* fl, const elem8_t (&bop)[NT][KSH], float4_t (&acc)[NT][OT]) {
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            float4_t c[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < KSH; ks++) {
                const elem8_t a = fl[(size_t)(ot * KSH + ks) * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
            }
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][ot] = c[t];
        }
    };
    auto relu_pack = [&](float4_t (&acc)[NT][OT], elem8_t (&bop)[NT][KSH]) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
            for (int ot = 0; ot < OT; ot++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[t][ot][j] = act_forward(kRelu, acc[t][ot][j]);
#pragma unroll
            for (int s = 0; s < KSH; s++) bop[t][s] = pack_operand(acc[t][2 * s], acc[t][2 * s + 1]);
        }
    };
    auto out_tile = [&](const elem8_t* fo, const elem8_t (&bop)[NT][KSH], float4_t (&c)[NT]) {
#pragma unroll
        for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KSH; ks++) {
            const elem8_t a = fo[(size_t)ks * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
        }
    };

    for (uint32_t row0 = blockIdx.x * kRowsPerBlock + wave * 16 * NT; row0 < live; row0 += gridDim.x * kRowsPerBlock) {
        if constexpr (!TRAIN && !DENSITY) {
            // inference: the march marks the sample slots a ray leaves unused (direction 1e30, nerftex_march_rays_dev); their outputs are
            // never read -- compositing stops in front of them -- so a wave-step made of such rows only (rays that left the volume, the
            // background of the frame) has nothing to compute
            bool used = false;
#pragma unroll
            for (int t = 0; t < NT; t++) used |= !(dirs[(size_t)(row0 + 16 * t + r) * 3] > 1e29f);
            if (__ballot(used) == 0ull) continue;
        }
        float4_t acc[NT][OT];
        elem8_t bop[NT][KSH];
        // ---- sigma net, layer 0: slots 8g .. 8g+7 = levels 4g .. 4g+3, two channels each, from the level-major features
        {
            elem8_t b[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const size_t row = row0 + 16 * t + r;
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; q++) w[q] = *reinterpret_cast<const uint32_t*>(feats + ((size_t)(4 * g + q) * B + row) * 2);
                typedef uint32_t u4 __attribute__((ext_vector_type(4)));
                if constexpr (kElemIsHalf) {
                    b[t] = __builtin_bit_cast(elem8_t, u4{w[0], w[1], w[2], w[3]});
                } else {
                    // the features are fp16 whatever the networks compute in (the hash table is fp16 under ANY autocast, gridencoder/grid.py:38-41):
                    // each is narrowed to the networks' type here, as the unfused chain's `.to(dtype)` in front of the sigma net does
                    const half8_t hf = __builtin_bit_cast(half8_t, u4{w[0], w[1], w[2], w[3]});
#pragma unroll
                    for (int j = 0; j < 8; j++) b[t][j] = (elem_t)(float)hf[j];
                }
                if constexpr (TRAIN) *reinterpret_cast<elem8_t*>(x_rows + row * IN + 8 * g) = b[t];  // the rows the sigma net's backward re-reads
            }
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                const elem8_t a = frags[(size_t)(kS0 + ot) * 64 + lane];
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t][ot] = mfma16(a, b[t], float4_t{0, 0, 0, 0});
            }
        }
        relu_pack(acc, bop);
        hidden(frags + kS1 * 64, bop, acc);
        relu_pack(acc, bop);
        float4_t h[NT];
        out_tile(frags + kSo * 64, bop, h);  // lane (r, g): outputs 4g .. 4g+3 of row r

        if constexpr (DENSITY) {  // sigma = exp(h0 as the 16-bit value the unfused sequence sees), nothing else
            if (g == 0) {
#pragma unroll
                for (int t = 0; t < NT; t++) sigma[row0 + 16 * t + r] = expf((float)(elem_t)h[t][0]);
            }
            continue;
        }
        // ---- between the networks: density, SH tile, the colour net's first operand
        elem8_t bc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const size_t row = row0 + 16 * t + r;
            float4_t hr;  // h as the 16-bit values every consumer of the unfused sequence sees
#pragma unroll
            for (int j = 0; j < 4; j++) hr[j] = (float)(elem_t)h[t][j];
            if (g == 0) sigma[row] = expf(hr[0]);
            float sh16[16];
            sh::eval<4>(dirs[row * 3], dirs[row * 3 + 1], dirs[row * 3 + 2], sh16);
            // the colour net's input row [SH 0..15 | h 1..15 | 0] in the NATURAL slot order of a row-major operand (lane group g holds
            // inputs 8g .. 8g+7): the matrix core then adds the 32 products of its first layer in the same order as the stand-alone
            // kernel does -- bit-identical results.  Input 16 + i = h[i + 1] sits in lane group (i + 1) / 4, element (i + 1) % 4:
            // for slot j of group g >= 2 that is element (j + 1) % 4 (a compile-time index) of group 2 (g - 2) + (j + 1) / 4.
            elem8_t cv;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float geo = __shfl(hr[(j + 1) & 3], r + 16 * (2 * (g & 1) + ((j + 1) >> 2)), 64);
                float sh_lo = sh16[j], sh_hi = sh16[8 + j];
                asm volatile("" : "+v"(sh_lo), "+v"(sh_hi));  // both in registers: left alone, the select becomes a dynamically indexed load from a scratch copy of sh16
                const float shj = (g & 1) ? sh_hi : sh_lo;
                cv[j] = g < 2 ? narrow16(shj) : ((g == 3 && j == 7) ? (elem_t)0.0f : (elem_t)geo);
            }
            bc[t] = cv;
            if constexpr (TRAIN) {
                store4(h_out + row * 16 + 4 * g, h[t]);
                *reinterpret_cast<elem8_t*>(cin_out + row * IN + 8 * g) = cv;
            }
        }
        // ---- colour net
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            const elem8_t a = frags[(size_t)(kC0 + ot) * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][ot] = mfma16(a, bc[t], float4_t{0, 0, 0, 0});
        }
        relu_pack(acc, bop);
        hidden(frags + kC1 * 64, bop, acc);
        relu_pack(acc, bop);
        hidden(frags + kC2 * 64, bop, acc);
        relu_pack(acc, bop);
        float4_t c[NT];
        out_tile(frags + kCo * 64, bop, c);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const size_t row = row0 + 16 * t + r;
            if constexpr (TRAIN)
                if (hc_out) store4(hc_out + row * 16 + 4 * g, c[t]);  // optional: the backward entry points read rgbs, not hc
            if (g == 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float x = (float)(elem_t)c[t][k];
                    rgbs[row * 3 + k] = (float)narrow16(1.0f / (1.0f + expf(-x)));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, part 1: activation gradients (dL/d pre-activation of every hidden layer) + dL/d input
//   bb[j] holds the gradient at hidden activation NL-1-j (the reference's backward_buffer order)
// ------------------------------------------------------------------------------------------------
template <int HIDDEN, bool STREAM = false>  // STREAM: one matrix's fragments in LDS at a time (see ffmlp_forward_kernel)
__global__ __launch_bounds__(kBlockThreads) void ffmlp_dgrad_kernel(const elem_t* __restrict__ grad, const elem_t* __restrict__ W,
                                                                    const elem_t* __restrict__ fwd, elem_t* __restrict__ bb,
                                                                    elem_t* __restrict__ grad_inputs, uint32_t B, uint32_t IN, uint32_t NL,
                                                                    uint32_t act) {
    constexpr int OT = HIDDEN / 16;
    constexpr int KSH = (HIDDEN + 31) / 32;
    constexpr int NT = kTilesPerWave;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem8_t* frags = reinterpret_cast<elem8_t*>(smem);

    const elem_t* W_hidden = W + (size_t)HIDDEN * IN;
    const elem_t* W_out = W_hidden + (size_t)(NL - 1) * HIDDEN * HIDDEN;
    // fragment table: [W_out^T (HIDDEN x 16)] [W_l^T for l = NL-1 .. 1] [W_0^T (IN x HIDDEN), optional]
    const int per_hidden = OT * KSH;
    const int base_hidden = OT;  // W_out^T has K = 16 -> one 32-deep step per tile
    const int base_in = base_hidden + (NL - 1) * per_hidden;
    if constexpr (!STREAM) {
        stage_fragments(frags, W_out, HIDDEN, true, HIDDEN, 16, false);
        for (uint32_t j = 1; j < NL; j++)
            stage_fragments(frags + (size_t)(base_hidden + (j - 1) * per_hidden) * 64, W_hidden + (size_t)(NL - 1 - j) * HIDDEN * HIDDEN, HIDDEN, true,
                            HIDDEN, HIDDEN, true);
        if (grad_inputs) stage_fragments(frags + (size_t)base_in * 64, W, IN, true, IN, HIDDEN, true);
        __syncthreads();
    }
    // the transposed fragments of step j of the backward chain (0 = W_out^T, 1 .. NL-1 = W_{NL-j}^T, NL = W_0^T): resident, or staged now
    auto fragments_of = [&](uint32_t j) -> const elem8_t* {
        if constexpr (STREAM) {
            __syncthreads();
            if (j == 0) stage_fragments(frags, W_out, HIDDEN, true, HIDDEN, 16, false);
            else if (j < NL) stage_fragments(frags, W_hidden + (size_t)(NL - 1 - j) * HIDDEN * HIDDEN, HIDDEN, true, HIDDEN, HIDDEN, true);
            else stage_fragments(frags, W, IN, true, IN, HIDDEN, true);
            __syncthreads();
            return frags;
        } else {
            return j == 0 ? frags : (j < NL ? frags + (size_t)(base_hidden + (j - 1) * per_hidden) * 64 : frags + (size_t)base_in * 64);
        }
    };

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const size_t layer_stride = (size_t)B * HIDDEN;

    for (uint32_t row0 = blockIdx.x * kRowsPerBlock + wave * 16 * NT; row0 < B; row0 += gridDim.x * kRowsPerBlock) {
        // B operand of the first product: grad^T (16 outputs = lane groups 0,1; groups 2,3 are zero padding)
        elem8_t bg[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (g < 2) bg[t] = *reinterpret_cast<const elem8_t*>(grad + (size_t)(row0 + 16 * t + r) * 16 + 8 * g);
            else bg[t] = elem8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
        float4_t acc[NT][OT];
        const elem8_t* fout = fragments_of(0);
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            const elem8_t a = fout[(size_t)ot * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][ot] = mfma16(a, bg[t], float4_t{0, 0, 0, 0});
        }

        elem8_t bop[NT][KSH];
        for (uint32_t j = 0;; j++) {
            const elem_t* f = fwd + (size_t)(NL - 1 - j) * layer_stride;  // post-activations of the layer being crossed
#pragma unroll
            for (int t = 0; t < NT; t++) {
#pragma unroll
                for (int ot = 0; ot < OT; ot++) {
                    const size_t off = (size_t)(row0 + 16 * t + r) * HIDDEN + 16 * ot + 4 * g;
                    const elem4_t y = *reinterpret_cast<const elem4_t*>(f + off);
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[t][ot][q] = act_backward(act, (float)(elem_t)acc[t][ot][q], (float)y[q]);
                    store4(bb + j * layer_stride + off, acc[t][ot]);
                }
#pragma unroll
                for (int s = 0; s < KSH; s++) {
                    const float4_t zero{0, 0, 0, 0};
                    bop[t][s] = pack_operand(acc[t][2 * s], (2 * s + 1 < OT) ? acc[t][(2 * s + 1 < OT) ? 2 * s + 1 : 0] : zero);
                }
            }
            if (j + 1 >= NL) break;
            const elem8_t* fl = fragments_of(j + 1);  // W_{NL-1-j}^T
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                float4_t c[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KSH; ks++) {
                    const elem8_t a = fl[(size_t)(ot * KSH + ks) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
                }
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t][ot] = c[t];
            }
        }

        if (grad_inputs) {  // dL/dX = W_0^T . dPre_0, no activation (ffmlp.cu:880-887)
            const elem8_t* fi = fragments_of(NL);
            for (uint32_t it = 0; it < IN / 16; it++) {
                float4_t c[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KSH; ks++) {
                    const elem8_t a = fi[(size_t)(it * KSH + ks) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < NT; t++) c[t] = mfma16(a, bop[t][ks], c[t]);
                }
#pragma unroll
                for (int t = 0; t < NT; t++) store4(grad_inputs + (size_t)(row0 + 16 * t + r) * IN + 16 * it + 4 * g, c[t]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, part 2: weight gradients  dW[o,i] = sum_n dPre[n,o] * In[n,i]   (contraction over the batch)
// ------------------------------------------------------------------------------------------------
constexpr int kMaxLayers = 12;
struct WgradLayer {
    const elem_t* dpre;  // [B, ld_d] rows, O valid columns
    const elem_t* in;    // [B, ld_i] rows, K valid columns
    uint32_t ld_d, ld_i, O, K;
    uint32_t w_off;      // offset of this matrix in the flat weight vector
};
struct WgradArgs {
    WgradLayer layer[kMaxLayers];
};

// 16 batch rows x 32 features, natural A-operand form (lane r = batch row, 8 consecutive features)
__device__ __forceinline__ elem8_t load_rows(const elem_t* p, uint32_t ld, uint32_t row, uint32_t col0, uint32_t ncols, int g) {
    const uint32_t c = col0 + 8 * g;
    if (c < ncols) return *reinterpret_cast<const elem8_t*>(p + (size_t)row * ld + c);
    return elem8_t{0, 0, 0, 0, 0, 0, 0, 0};
}

__global__ __launch_bounds__(kBlockThreads) void ffmlp_wgrad_kernel(const WgradArgs args, uint32_t B, float* __restrict__ partials,
                                                                    uint32_t n_params) {
    constexpr int G = 4;  // tiles per group in each direction -> 16 accumulator tiles (64 VGPRs)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);  // [4 waves][G*G tiles][256] fp32, per-workgroup combine

    const WgradLayer L = args.layer[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const uint32_t OT = L.O / 16, IT = L.K / 16;

    // selection matrices: B operand with B[k][col] = (k == col) / (k == 16 + col); A x Sel = transpose into "batch in registers"
    elem8_t sel0, sel1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        sel0[j] = (8 * g + j == r) ? (elem_t)1.0f : (elem_t)0.0f;
        sel1[j] = (8 * g + j == 16 + r) ? (elem_t)1.0f : (elem_t)0.0f;
    }
    const float4_t zero{0, 0, 0, 0};
    float* out = partials + (size_t)blockIdx.x * n_params + L.w_off;

    for (uint32_t og = 0; og < OT; og += G) {
        for (uint32_t ig = 0; ig < IT; ig += G) {
            float4_t acc[G][G];
#pragma unroll
            for (int a = 0; a < G; a++)
#pragma unroll
                for (int b = 0; b < G; b++) acc[a][b] = zero;

            // each wave walks 32-row steps of the batch
            for (uint32_t row0 = (blockIdx.x * 4 + wave) * 32; row0 < B; row0 += gridDim.x * 4 * 32) {
                elem8_t A[G], Bm[G];
                // transposed dPre tiles -> A operands (lane = output neuron, slots = 2 x 4 batch rows)
#pragma unroll
                for (int a = 0; a < G; a += 2) {
                    const uint32_t col0 = 16 * (og + a);  // 32 features feed tiles a, a+1
                    const elem8_t x0 = load_rows(L.dpre, L.ld_d, row0 + r, col0, L.O, g);
                    const elem8_t x1 = load_rows(L.dpre, L.ld_d, row0 + 16 + r, col0, L.O, g);
                    A[a] = pack_operand(mfma16(x0, sel0, zero), mfma16(x1, sel0, zero));
                    A[a + 1] = pack_operand(mfma16(x0, sel1, zero), mfma16(x1, sel1, zero));
                }
#pragma unroll
                for (int b = 0; b < G; b += 2) {
                    const uint32_t col0 = 16 * (ig + b);
                    const elem8_t x0 = load_rows(L.in, L.ld_i, row0 + r, col0, L.K, g);
                    const elem8_t x1 = load_rows(L.in, L.ld_i, row0 + 16 + r, col0, L.K, g);
                    Bm[b] = pack_operand(mfma16(x0, sel0, zero), mfma16(x1, sel0, zero));
                    Bm[b + 1] = pack_operand(mfma16(x0, sel1, zero), mfma16(x1, sel1, zero));
                }
#pragma unroll
                for (int a = 0; a < G; a++)
#pragma unroll
                    for (int b = 0; b < G; b++) acc[a][b] = mfma16(A[a], Bm[b], acc[a][b]);
            }

            // combine the 4 waves in LDS, then one fp32 write per element per workgroup
            __syncthreads();
#pragma unroll
            for (int a = 0; a < G; a++)
#pragma unroll
                for (int b = 0; b < G; b++)
#pragma unroll
                    for (int j = 0; j < 4; j++) red[((wave * G * G + a * G + b) * 4 + j) * 64 + lane] = acc[a][b][j];
            __syncthreads();
            for (int e = threadIdx.x; e < G * G * 256; e += kBlockThreads) {
                const int tile = e >> 8, j = (e >> 6) & 3, ln = e & 63;
                const int a = tile / G, b = tile % G;
                const uint32_t o = 16 * (og + a) + 4 * (ln >> 4) + j, i = 16 * (ig + b) + (ln & 15);
                if (o < L.O && i < L.K) {
                    float s = 0.0f;
#pragma unroll
                    for (int w = 0; w < 4; w++) s += red[((w * G * G + tile) * 4 + j) * 64 + ln];
                    out[(size_t)o * L.K + i] = s;
                }
            }
        }
    }
}

// per-workgroup combine of one weight-gradient matrix held as NA x NB result tiles per wave: LDS sum over the 4 waves, one fp32
// write per element.  Everything is indexed at compile time so the accumulators stay in registers.
// One layer's products for NB 16-row batch tiles: out[t][ot] = sum_ks A(ot, ks) . b[t][ks], the A fragments read from LDS (fr = table
// base + lane).  The fragments of tile ot+1 are requested BEFORE the MFMAs of tile ot and the order is pinned: left alone, the
// scheduler (at the register limit) reloads the same registers right after their last use and waits out the full LDS latency in
// front of every tile -- ~30 exposed round trips per 32-row step of the fused backward.
template <int NTILES, int KS, int NB>
__device__ __forceinline__ void layer_products(const elem8_t* __restrict__ fr, const elem8_t (&b)[NB][KS], float4_t (&out)[NB][NTILES]) {
    elem8_t a[2][KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) a[0][ks] = fr[(size_t)ks * 64];
#pragma unroll
    for (int ot = 0; ot < NTILES; ot++) {
        if (ot + 1 < NTILES) {
#pragma unroll
            for (int ks = 0; ks < KS; ks++) a[(ot + 1) & 1][ks] = fr[(size_t)((ot + 1) * KS + ks) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        float4_t c[NB];
#pragma unroll
        for (int t = 0; t < NB; t++) c[t] = float4_t{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
#pragma unroll
            for (int t = 0; t < NB; t++) c[t] = mfma16(a[ot & 1][ks], b[t][ks], c[t]);
#pragma unroll
        for (int t = 0; t < NB; t++) out[t][ot] = c[t];
    }
}

template <int NA, int NB>
__device__ __forceinline__ void flush_tiles(const float4_t (&tiles)[NA][NB], float* __restrict__ red, float* __restrict__ out, uint32_t K, int wave,
                                            int lane) {
    static_assert(NA * NB <= 16, "combine buffer holds 16 tiles per wave");
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NA; a++)
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) red[((wave * 16 + a * NB + b) * 4 + q) * 64 + lane] = tiles[a][b][q];
    __syncthreads();
    for (int e = threadIdx.x; e < NA * NB * 256; e += kBlockThreads) {
        const int tile = e >> 8, q = (e >> 6) & 3, ln = e & 63;
        const int a = tile / NB, b = tile % NB;
        const uint32_t o = 16 * a + 4 * (ln >> 4) + q, i = 16 * b + (ln & 15);
        float sum = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; w++) sum += red[((w * 16 + tile) * 4 + q) * 64 + ln];
        out[(size_t)o * K + i] = sum;
    }
}

// ------------------------------------------------------------------------------------------------
// backward, fused: activation gradients AND weight gradients in one pass over the batch
// ------------------------------------------------------------------------------------------------
// The dgrad chain already holds, per 32 batch rows, every dPre tile (fp32 result tiles -> the permuted 32-deep operand `bop`)
// and loads every saved activation tile (for the activation derivative) in the same (lane = batch row, slots = features)
// form.  That is exactly the input form of the transposing MFMAs of the weight-gradient kernel above -- so the weight gradients
// are accumulated right here, in fp32 registers that live across the whole batch loop, and
//   * backward_buffer is never written nor read (it is scratch in the reference's contract),
//   * forward_buffer and the inputs are read once instead of twice:  ~52 % less HBM traffic for the whole MLP backward.
// One wave per SIMD (the dW accumulators are 112-176 registers); the loads of a 32-row step are issued together.
// RECOMPUTE: forward_buffer is not read at all -- the saved activations are rebuilt from the inputs with the forward kernel's own
// chain (bit-identical halfs), which costs a few dozen MFMAs per 32 rows and removes 70 % of this kernel's loads; the training
// forward then has no forward_buffer to write either.
// FIELD (RECOMPUTE only): the output gradient is not read but FORMED, from what the step before this network's backward left -- the
// two glue kernels of the ngp field's backward (fieldglue.hip) ride on the load stage:
//   1  colour net: grad = grad_rgbs [B,3] fp32, aux0 = rgbs [B,3] fp32 (half-valued):  dL/dhc[:, :3] = sigmoid backward in fp16 arithmetic
//      (field_out_backward_kernel), the other 13 columns zero;
//   2  sigma net: grad = grad_cin [B,32] (the colour net's dL/dinput), aux0 = grad_sigma [B] fp32, aux1 = h [B,16]:
//      dL/dh = [grad_sigma exp(clamp(h0, -15, 15)) | grad_cin[:, 16:31]]  (field_mid_backward_kernel).
// The weight-gradient operands dPre^T and Y^T are built by 0/1 selection-matrix MFMAs.  Round 4 also built them with gfx950's transposing LDS read
// (ds_read_b64_tr_b16 over a per-wave LDS patch): slower, 64.8 / 49.7 us against 59.6 / 47.0 (profiles/r04_ffmlp_tr_ab.json, DESIGN.md 4.3); removed.
// LIVE (round 6, the two field forms): `step_live` holds one word per 32 consecutive batch rows -- 0: the compositing backward handed exactly zero
// gradients to all 32 samples (raymarching.cu:843-870 past the point where a ray's transmittance has underflowed: 42 % of the samples after 100
// steps of the bench's scene, 99.6 % after 1000).  Such a step adds exact zeros to every weight gradient and has a zero input gradient: a wave
// takes the flags of its next 64 steps as ONE ballot and walks the set bits -- dead steps issue no loads and no MFMAs; the colour net's input
// gradient stays unwritten for them (only the sigma kernel reads it, on live steps), the sigma net's -- which the hash-grid backward reads row by
// row -- is written as zeros.  The step -> wave assignment does not change, so every partial sum
// is the sum of the same terms in the same order minus exact zeros: the gradients are those of the kernel without flags, bit for bit.
// (Round 5's form tested the gradient's CONTENT after loading it -- a skipped step had paid for its loads and the test cost a young field
// 9 %: removed.)
template <int HIDDEN, int NL, int IT, bool RECOMPUTE, int ACT, int FIELD = 0, bool LIVE = false>  // IT = input_dim / 16; ACT: see act_fwd
__global__ __launch_bounds__(kBlockThreads, 1) void ffmlp_backward_fused_kernel(const elem_t* __restrict__ grad, const elem_t* __restrict__ X,
                                                                               const elem_t* __restrict__ W, const elem_t* __restrict__ fwd,
                                                                               elem_t* __restrict__ grad_inputs, uint32_t B, uint32_t act,
                                                                               float* __restrict__ partials, uint32_t n_params,
                                                                               const void* __restrict__ aux0, const void* __restrict__ aux1,
                                                                               const uint32_t* __restrict__ step_live) {
    static_assert(FIELD == 0 || (RECOMPUTE && IT == 2 && HIDDEN == 64), "field forms of the backward: the two 32-input networks, recomputing");
    static_assert(!LIVE || FIELD != 0, "step flags: the field forms only");
    constexpr int OT = HIDDEN / 16;
    constexpr int KSH = (HIDDEN + 31) / 32;
    constexpr int NT = 2;               // 32 batch rows per wave step = one 32-deep contraction step of the weight gradients
    constexpr int IN = 16 * IT;
    constexpr int KS0 = (IN + 31) / 32;
    static_assert(HIDDEN % 32 == 0 && kTilesPerWave == NT, "fused backward: hidden width must be a multiple of 32");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem8_t* frags = reinterpret_cast<elem8_t*>(smem);

    const elem_t* W_hidden = W + (size_t)HIDDEN * IN;
    const elem_t* W_out = W_hidden + (size_t)(NL - 1) * HIDDEN * HIDDEN;
    constexpr int per_hidden = OT * KSH;
    constexpr int base_hidden = OT;
    constexpr int base_in = base_hidden + (NL - 1) * per_hidden;
    stage_fragments(frags, W_out, HIDDEN, true, HIDDEN, 16, false);
    for (int j = 1; j < NL; j++)
        stage_fragments(frags + (size_t)(base_hidden + (j - 1) * per_hidden) * 64, W_hidden + (size_t)(NL - 1 - j) * HIDDEN * HIDDEN, HIDDEN, true,
                        HIDDEN, HIDDEN, true);
    if (grad_inputs) stage_fragments(frags + (size_t)base_in * 64, W, IN, true, IN, HIDDEN, true);
    // forward-orientation fragments for the recomputation: [W_0 (HIDDEN x IN)] [W_l, l = 1 .. NL-1]
    constexpr int base_f0 = base_in + IT * KSH;
    constexpr int base_fh = base_f0 + OT * KS0;
    if constexpr (RECOMPUTE) {
        stage_fragments(frags + (size_t)base_f0 * 64, W, IN, false, HIDDEN, IN, false);
        for (int l = 1; l < NL; l++)
            stage_fragments(frags + (size_t)(base_fh + (l - 1) * per_hidden) * 64, W_hidden + (size_t)(l - 1) * HIDDEN * HIDDEN, HIDDEN, false, HIDDEN,
                            HIDDEN, true);
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const size_t layer_stride = (size_t)B * HIDDEN;
    const float4_t zero{0, 0, 0, 0};

    // 0/1 selection operands: X . Sel moves 16 of the 32 features of X onto the lane axis (batch rows into registers)
    //   natural order (operand read from row-major memory): slot (g, j) <-> feature 8g + j
    //   permuted order (operand packed from two result tiles / two half4 activation loads): j < 4 <-> tile 2s feature 4g + j,
    //                                                                                       j >= 4 <-> tile 2s+1 feature 4g + j - 4
    elem8_t sel0, sel1, selP0, selP1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        sel0[j] = (8 * g + j == r) ? (elem_t)1.0f : (elem_t)0.0f;
        sel1[j] = (8 * g + j == 16 + r) ? (elem_t)1.0f : (elem_t)0.0f;
        selP0[j] = (j < 4 && 4 * g + j == r) ? (elem_t)1.0f : (elem_t)0.0f;
        selP1[j] = (j >= 4 && 4 * g + j - 4 == r) ? (elem_t)1.0f : (elem_t)0.0f;
    }

    float4_t gw_out[1][OT];                         // dW_out [16 x HIDDEN]
    float4_t gw_hid[NL > 1 ? NL - 1 : 1][OT][OT];   // dW_l, l = 1..NL-1 [HIDDEN x HIDDEN]
    float4_t gw_in[OT][IT];                         // dW_0 [HIDDEN x IN]
#pragma unroll
    for (int b = 0; b < OT; b++) gw_out[0][b] = zero;
#pragma unroll
    for (int l = 0; l < NL - 1; l++)
#pragma unroll
        for (int a = 0; a < OT; a++)
#pragma unroll
            for (int b = 0; b < OT; b++) gw_hid[l][a][b] = zero;
#pragma unroll
    for (int a = 0; a < OT; a++)
#pragma unroll
        for (int b = 0; b < IT; b++) gw_in[a][b] = zero;

    // One wave per SIMD: nobody hides the latency of a step's loads, and asking for the NEXT step's operands in registers costs 64
    // of them (tried: the 3-layer instantiation spills, 130 -> 160 us).  With the activations recomputed a step needs only its
    // gradient and input rows -- 4 KiB per wave -- and those are prefetched one step ahead straight into LDS (global_load_lds: no
    // registers, the wave's own counted vmcnt orders its later ds_read), two slots per wave.
    // ring slot = kGradPieces 1-KiB pieces for the output gradient (or what it is formed from), then NT * KS0 input tiles; kLoads = the
    // vector-memory instructions one prefetch issues (what the counted vmcnt below waits on)
    constexpr int kGradPieces = FIELD == 2 ? NT + 1 : NT;
    constexpr int kPieces = kGradPieces + NT * KS0;
    constexpr int kLoads = (FIELD == 0 ? NT : 4) + NT * KS0;
    constexpr size_t kRingOffset = ((size_t)(base_fh + (NL - 1) * per_hidden) * 1024 > 64 * 1024) ? (size_t)(base_fh + (NL - 1) * per_hidden) * 1024 : 64 * 1024;
    elem8_t* ring = reinterpret_cast<elem8_t*>(smem + kRingOffset) + (size_t)wave * 2 * kPieces * 64;
    const uint32_t row_step = gridDim.x * kRowsPerBlock;
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto prefetch = [&](uint32_t rw, int slot) {
        elem8_t* dst = ring + (size_t)slot * kPieces * 64;
        if constexpr (FIELD == 0) {
#pragma unroll
            for (int t = 0; t < NT; t++)  // lane groups 2, 3 have no gradient columns: they fetch a copy of groups 0, 1 and drop it
                __builtin_amdgcn_global_load_lds((gptr_t)(grad + (size_t)(rw + 16 * t + r) * 16 + 8 * (g & 1)), (lptr_t)(dst + t * 64), 16, 0, 0);
        } else if constexpr (FIELD == 1) {
            // 32 rows x 3 floats of grad_rgbs, then of rgbs: 96 consecutive floats each = a 64-lane and a 32-lane dword request
            // (the upper lanes repeat the lower ones' request: the instruction count must not depend on the lane)
            const float* gr = reinterpret_cast<const float*>(grad) + (size_t)rw * 3;
            const float* y = static_cast<const float*>(aux0) + (size_t)rw * 3;
            char* d8 = reinterpret_cast<char*>(dst);
            __builtin_amdgcn_global_load_lds((gptr_t)(gr + lane), (lptr_t)d8, 4, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(gr + 64 + (lane & 31)), (lptr_t)(d8 + 256), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(y + lane), (lptr_t)(d8 + 1024), 4, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(y + 64 + (lane & 31)), (lptr_t)(d8 + 1024 + 256), 4, 0, 0);
        } else {
            // columns 16..31 of the colour net's dL/dinput as two 16-byte chunks per row (lane groups 2, 3 repeat 0, 1), then
            // grad_sigma and the dword holding h[:, 0] of the 32 rows
            const float* gs = static_cast<const float*>(aux0) + rw;
            const elem_t* hh = static_cast<const elem_t*>(aux1) + (size_t)rw * 16;
            char* d8 = reinterpret_cast<char*>(dst + NT * 64);
#pragma unroll
            for (int t = 0; t < NT; t++)
                __builtin_amdgcn_global_load_lds((gptr_t)(grad + (size_t)(rw + 16 * t + r) * 32 + 16 + 8 * (g & 1)), (lptr_t)(dst + t * 64), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(gs + (lane & 31)), (lptr_t)d8, 4, 0, 0);
            __builtin_amdgcn_global_load_lds((gptr_t)(hh + (size_t)(lane & 31) * 16), (lptr_t)(d8 + 256), 4, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < KS0; ks++)
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int k0 = 32 * ks + 8 * g;
                __builtin_amdgcn_global_load_lds((gptr_t)(X + (size_t)(rw + 16 * t + r) * IN + (k0 < IN ? k0 : 0)),
                                                 (lptr_t)(dst + (kGradPieces + ks * NT + t) * 64), 16, 0, 0);
            }
    };
    uint32_t step = 0;
    const uint32_t first = blockIdx.x * kRowsPerBlock + wave * 16 * NT;
    // LIVE: the wave's steps are rows first + k row_step; the flags of 64 of them at a time as a ballot (wave-uniform), consumed bit by bit
    [[maybe_unused]] uint64_t live_mask = 0;
    [[maybe_unused]] uint32_t live_base = first, chunk_next = first;
    auto next_live = [&]() -> uint32_t {  // the wave's next row with a gradient, or >= B
        while (live_mask == 0ull) {
            if (chunk_next >= B) return B;
            live_base = chunk_next;
            const uint64_t rk = (uint64_t)live_base + (uint64_t)lane * row_step;
            const bool in_range = rk < B;
            live_mask = __ballot(in_range && step_live[(uint32_t)rk >> 5] != 0u);
            if constexpr (FIELD == 2) {
                // the sigma net's input gradient feeds the hash-grid backward, which reads every row: a dead step's 32 rows are written as zeros
                // (2 KiB, two 16-byte stores per lane) -- what the plain kernel computes for them
                uint64_t dead = __ballot(in_range) & ~live_mask;
                while (dead != 0ull) {
                    const uint32_t j = (uint32_t)__builtin_ctzll(dead);
                    dead &= dead - 1ull;
                    elem_t* rows = grad_inputs + (size_t)(live_base + j * row_step) * IN;
                    store4(rows + 4 * (2 * lane), zero);
                    store4(rows + 4 * (2 * lane + 1), zero);
                    store4(rows + 4 * (2 * (64 + lane)), zero);
                    store4(rows + 4 * (2 * (64 + lane) + 1), zero);
                }
            }
            chunk_next = (uint64_t)live_base + 64ull * row_step < B ? live_base + 64u * row_step : B;
        }
        const uint32_t j = (uint32_t)__builtin_ctzll(live_mask);
        live_mask &= live_mask - 1ull;
        return live_base + j * row_step;
    };
    uint32_t row0 = first;
    if constexpr (LIVE) row0 = next_live();
    if constexpr (RECOMPUTE) {
        if (row0 < B) prefetch(row0, 0);
    }
    uint32_t next = B;
    for (; row0 < B; row0 = next, step++) {
        if constexpr (LIVE) next = next_live();
        else next = row0 + row_step;
        // ---- all loads of this step first: output gradient, inputs, saved activations of every layer
        elem8_t bg[NT];
        elem8_t xin[NT][KS0];
        if constexpr (RECOMPUTE) {
            prefetch(next < B ? next : row0, (step + 1) & 1);  // past the end: a harmless re-fetch keeps the count below uniform
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLoads) : "memory");  // everything but the pieces just requested has landed
            const elem8_t* src = ring + (size_t)(step & 1) * kPieces * 64;
            const elem8_t zero8{0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (FIELD == 0) {
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const elem8_t v = src[t * 64 + lane];
                    bg[t] = g < 2 ? v : zero8;
                }
            } else if constexpr (FIELD == 1) {
                // field_out_backward_kernel: the framework's sigmoid backward on fp16 tensors runs in fp16 ARITHMETIC, (g (1 - y)) y
                // with every operation rounded to half
                const float* gr = reinterpret_cast<const float*>(src);
                const float* yy = reinterpret_cast<const float*>(src + 64);
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    elem8_t v = zero8;
                    if (g == 0) {
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            // (plain asm, not volatile: it only has to keep the operations from being fused; a volatile one would also pin
                            // this block in front of the recomputation below, whose own volatile statements it may not cross)
                            float gin = gr[(16 * t + r) * 3 + c];
                            asm("" : "+v"(gin));
                            const elem_t go = (elem_t)gin;
                            const elem_t y = (elem_t)yy[(16 * t + r) * 3 + c];
                            elem_t one_minus = (elem_t)1.0f - y;
                            asm("" : "+v"(one_minus));
                            elem_t u = go * one_minus;
                            asm("" : "+v"(u));
                            v[c] = u * y;
                        }
                    }
                    bg[t] = v;
                }
            } else {
                // field_mid_backward_kernel: column 0 = grad_sigma exp(clamp(h0, -15, 15)) in fp32, narrowed; columns 1..15 = columns
                // 16..30 of the colour net's input gradient
                const char* extra = reinterpret_cast<const char*>(src + NT * 64);
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const elem8_t c0 = src[t * 64 + r], c1 = src[t * 64 + 16 + r];  // the row's two chunks (lane groups 0 and 1)
                    elem8_t v = zero8;
                    if (g == 0) {
                        const float gsig = reinterpret_cast<const float*>(extra)[16 * t + r];
                        const elem_t h0 = reinterpret_cast<const elem_t*>(extra + 256)[2 * (16 * t + r)];
                        const float x = (float)h0;
                        float col0 = gsig * expf(fminf(fmaxf(x, -15.0f), 15.0f));
                        asm("" : "+v"(col0));  // the product is rounded to fp32, then to half (see narrow16; plain asm: see above)
                        v[0] = (elem_t)col0;
#pragma unroll
                        for (int i = 0; i < 7; i++) v[1 + i] = c0[i];
                    } else if (g == 1) {
                        v[0] = c0[7];
#pragma unroll
                        for (int i = 0; i < 7; i++) v[1 + i] = c1[i];
                    }
                    bg[t] = v;
                }
            }
#pragma unroll
            for (int ks = 0; ks < KS0; ks++)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const elem8_t v = src[(kGradPieces + ks * NT + t) * 64 + lane];
                    xin[t][ks] = (32 * ks + 8 * g < IN) ? v : zero8;
                }
        } else {
#pragma unroll
            for (int t = 0; t < NT; t++) {
                if (g < 2) bg[t] = *reinterpret_cast<const elem8_t*>(grad + (size_t)(row0 + 16 * t + r) * 16 + 8 * g);
                else bg[t] = elem8_t{0, 0, 0, 0, 0, 0, 0, 0};
            }
#pragma unroll
            for (int ks = 0; ks < KS0; ks++)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    if (32 * ks + 8 * g < IN) xin[t][ks] = *reinterpret_cast<const elem8_t*>(X + (size_t)(row0 + 16 * t + r) * IN + 32 * ks + 8 * g);
                    else xin[t][ks] = elem8_t{0, 0, 0, 0, 0, 0, 0, 0};
                }
        }
        // yop[j][t][s] = post-activations of hidden layer NL-1-j for 16 rows x 32 features, already in the packed-operand form
        // (slot q < 4: feature 16(2s) + 4g + q, slot 4 + q: feature 16(2s+1) + 4g + q of row r): what the recomputation produces anyway,
        // what the transposing MFMAs consume, and what the activation derivative reads element by element
        elem8_t yop[NL][NT][KSH];
        float4_t acc[NT][OT];
        if constexpr (RECOMPUTE) {
            // the forward kernel's chain, verbatim (layer 0 from the row-major input, then register to register), one 16-row tile
            // at a time to keep the transient registers at one tile's worth
#pragma unroll
            for (int t = 0; t < NT; t++) {
                asm volatile("" ::: "memory");  // re-read the weight fragments from LDS per tile instead of keeping 20 of them in registers
                float4_t fa[1][OT];
                elem8_t x1[1][KS0];
#pragma unroll
                for (int ks = 0; ks < KS0; ks++) x1[0][ks] = xin[t][ks];
                layer_products<OT, KS0, 1>(frags + (size_t)base_f0 * 64 + lane, x1, fa);
#pragma unroll
                for (int l = 0; l < NL; l++) {
                    elem8_t fop[1][KSH];
#pragma unroll
                    for (int ot = 0; ot < OT; ot++)
#pragma unroll
                        for (int q = 0; q < 4; q++) fa[0][ot][q] = act_fwd<ACT>(act, fa[0][ot][q]);
#pragma unroll
                    for (int s = 0; s < KSH; s++) {
                        fop[0][s] = pack_operand(fa[0][2 * s], fa[0][2 * s + 1]);
                        yop[NL - 1 - l][t][s] = fop[0][s];
                    }
                    if (l + 1 < NL) layer_products<OT, KSH, 1>(frags + (size_t)(base_fh + l * per_hidden) * 64 + lane, fop, fa);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NL; j++)
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int s = 0; s < KSH; s++) {
                        const elem_t* row = fwd + (size_t)(NL - 1 - j) * layer_stride + (size_t)(row0 + 16 * t + r) * HIDDEN + 4 * g;
                        const elem4_t lo = *reinterpret_cast<const elem4_t*>(row + 16 * (2 * s));
                        const elem4_t hi = *reinterpret_cast<const elem4_t*>(row + 16 * (2 * s + 1));
                        yop[j][t][s] = elem8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    }
        }

        // ---- dL/d(last hidden activation) = W_out^T . grad^T
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
            const elem8_t a = frags[(size_t)ot * 64 + lane];
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][ot] = mfma16(a, bg[t], zero);
        }
        // A operands (lane = output neuron, slots = the 32 batch rows) of the gradient whose matrix comes next: first dL/dOut
        elem8_t Aprev[OT];
        Aprev[0] = pack_operand(mfma16(bg[0], sel0, zero), mfma16(bg[1], sel0, zero));

        elem8_t bop[NT][KSH];
#pragma unroll
        for (int j = 0; j < NL; j++) {
            // B operands (lane = input neuron, slots = batch rows) from the activations of layer NL-1-j = the inputs of the matrix
            // whose gradient Aprev holds
            elem8_t Bm[OT];
#pragma unroll
            for (int s = 0; s < KSH; s++) {
                Bm[2 * s] = pack_operand(mfma16(yop[j][0][s], selP0, zero), mfma16(yop[j][1][s], selP0, zero));
                Bm[2 * s + 1] = pack_operand(mfma16(yop[j][0][s], selP1, zero), mfma16(yop[j][1][s], selP1, zero));
            }
            if (j == 0) {
#pragma unroll
                for (int b = 0; b < OT; b++) gw_out[0][b] = mfma16(Aprev[0], Bm[b], gw_out[0][b]);
            } else {
#pragma unroll
                for (int a = 0; a < OT; a++)
#pragma unroll
                    for (int b = 0; b < OT; b++) gw_hid[NL - 1 - j][a][b] = mfma16(Aprev[a], Bm[b], gw_hid[NL - 1 - j][a][b]);
            }

            // through the activation of layer NL-1-j (same arithmetic as ffmlp_dgrad_kernel), repack as next operand
#pragma unroll
            for (int t = 0; t < NT; t++) {
#pragma unroll
                for (int ot = 0; ot < OT; ot++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const elem_t yv = yop[j][t][ot / 2][4 * (ot & 1) + q];
                        // ReLU: a 0/1 mask commutes with the rounding to half that pack_operand applies next, so the incoming gradient
                        // need not be narrowed and widened first (two conversions per element saved); other activations keep the
                        // dgrad kernel's order (narrow, multiply, narrow)
                        if constexpr (ACT == (int)kRelu) acc[t][ot][q] = yv > (elem_t)0.0f ? acc[t][ot][q] : 0.0f;
                        else acc[t][ot][q] = act_bwd<ACT>(act, (float)(elem_t)acc[t][ot][q], (float)yv);
                    }
#pragma unroll
                for (int s = 0; s < KSH; s++) bop[t][s] = pack_operand(acc[t][2 * s], acc[t][2 * s + 1]);
            }
#pragma unroll
            for (int s = 0; s < KSH; s++) {
                Aprev[2 * s] = pack_operand(mfma16(bop[0][s], selP0, zero), mfma16(bop[1][s], selP0, zero));
                Aprev[2 * s + 1] = pack_operand(mfma16(bop[0][s], selP1, zero), mfma16(bop[1][s], selP1, zero));
            }
            if (j + 1 < NL) layer_products<OT, KSH, NT>(frags + (size_t)(base_hidden + j * per_hidden) * 64 + lane, bop, acc);  // W_{NL-1-j}^T
        }

        // ---- first matrix: dW_0 += dPre_0^T . X
        {
            elem8_t Bx[2 * KS0];
#pragma unroll
            for (int ks = 0; ks < KS0; ks++) {
                Bx[2 * ks] = pack_operand(mfma16(xin[0][ks], sel0, zero), mfma16(xin[1][ks], sel0, zero));
                Bx[2 * ks + 1] = pack_operand(mfma16(xin[0][ks], sel1, zero), mfma16(xin[1][ks], sel1, zero));
            }
#pragma unroll
            for (int a = 0; a < OT; a++)
#pragma unroll
                for (int b = 0; b < IT; b++) gw_in[a][b] = mfma16(Aprev[a], Bx[b], gw_in[a][b]);
        }

        if (grad_inputs) {  // dL/dX = W_0^T . dPre_0, no activation (ffmlp.cu:880-887)
            float4_t gi[NT][IT];
            layer_products<IT, KSH, NT>(frags + (size_t)base_in * 64 + lane, bop, gi);
#pragma unroll
            for (int it = 0; it < IT; it++)
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    if constexpr (FIELD == 2 && !kElemIsHalf) {
                        // ngp field, networks not in fp16: this gradient is the hash-grid backward's input, whose type is the TABLE's (fp16) --
                        // rounded to the networks' type first, then widened / narrowed to half, as autograd's cast back through `.to(dtype)` does
                        half4_t hv;
#pragma unroll
                        for (int j = 0; j < 4; j++) hv[j] = (half_t)(float)(elem_t)gi[t][it][j];
                        *reinterpret_cast<half4_t*>(reinterpret_cast<half_t*>(grad_inputs) + (size_t)(row0 + 16 * t + r) * IN + 16 * it + 4 * g) = hv;
                    } else {
                        store4(grad_inputs + (size_t)(row0 + 16 * t + r) * IN + 16 * it + 4 * g, gi[t][it]);
                    }
                }
        }
    }

    if constexpr (RECOMPUTE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last step's spare prefetch
    // ---- combine the 4 waves in LDS (one matrix at a time, <= 16 tiles = 64 KiB), one fp32 partial row per workgroup
    float* red = reinterpret_cast<float*>(smem);
    float* out = partials + (size_t)blockIdx.x * n_params;
    flush_tiles<OT, IT>(gw_in, red, out, IN, wave, lane);
#pragma unroll
    for (int l = 0; l < NL - 1; l++) flush_tiles<OT, OT>(gw_hid[l], red, out + HIDDEN * IN + l * HIDDEN * HIDDEN, HIDDEN, wave, lane);
    flush_tiles<1, OT>(gw_out, red, out + HIDDEN * IN + (NL - 1) * HIDDEN * HIDDEN, HIDDEN, wave, lane);
}

// sum the per-workgroup partials: kRedParams consecutive parameters x (256 / kRedParams) slices of the partial list per workgroup
// (128-B coalesced reads, twice the workgroups of a 64 x 4 split: the pass is latency-bound), LDS combine of the slices, one
// fp16 store per parameter.  Fixed order: deterministic.  (sum_partials, kRedParams, kRedSlices: step_trailer.hpp -- shared with the form of
// this reduction that rides on the hash-grid backward's fill launch)
static_assert(kBlockThreads == (int)kRedThreads, "the reduction groups are the MLP kernels' workgroup size");
__global__ __launch_bounds__(kBlockThreads) void ffmlp_wgrad_reduce_kernel(const float* __restrict__ partials, uint32_t n_parts,
                                                                           uint32_t n_params, elem_t* __restrict__ grad_weights) {
    __shared__ float red[kRedSlices][kRedParams];
    const uint32_t lane = threadIdx.x % kRedParams, slice = threadIdx.x / kRedParams;
    const uint32_t p = blockIdx.x * kRedParams + lane;
    const float s = p < n_params ? sum_partials(partials, n_parts, n_params, p, slice) : 0.0f;
    red[slice][lane] = s;
    __syncthreads();
    if (slice == 0 && p < n_params) {
        float t = 0.0f;
#pragma unroll
        for (uint32_t i = 0; i < kRedSlices; i++) t += red[i][lane];
        grad_weights[p] = (elem_t)t;
    }
}

// the same reduction for the two networks of the ngp field in one launch (blocks [0, blocks0) take the first set)
struct RedSet { const float* partials; uint32_t n_parts, n_params; elem_t* out; };
// The step's trailer as a launch of its own (step_trailer.hpp: the two reductions + found_inf, the flags' clearing, the loss): workgroup 0 is
// the loss when there is one, the others one reduction group each.
__global__ __launch_bounds__(kBlockThreads) void ffmlp_wgrad_reduce2_kernel(const StepTrailer t) {
    __shared__ float red[kRedSlices * kRedParams];
    for (uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x; i < t.n_consume; i += gridDim.x * kBlockThreads) t.consume[i] = 0u;
    uint32_t block = blockIdx.x;
    if (t.job.err != nullptr) {
        if (block == 0) {
            __shared__ StepLossLds loss_lds;
            step_loss_sum<kBlockThreads>(t.job, loss_lds);
            return;
        }
        block--;
    }
    wgrad_reduce_group(t, block, threadIdx.x, red);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int num_cus() { return device_cus(); }

int validate(uint32_t B, uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
             uint32_t output_activation) {
    if (hidden_dim != 16 && hidden_dim != 32 && hidden_dim != 64 && hidden_dim != 128 && hidden_dim != 256) {
        set_error("hidden_dim should in [16, 32, 64, 128, 256]");
        return NERFTEX_ERR_INVALID;
    }
    if (input_dim == 0 || input_dim % 16 != 0) {
        set_error("FFMLP input_dim should be 16 * m (m  > 0), but got %u", input_dim);
        return NERFTEX_ERR_INVALID;
    }
    if (output_dim != 16) {
        set_error("FFMLP current only supports output dim <= 16 (padded to 16), but got %u", output_dim);
        return NERFTEX_ERR_INVALID;
    }
    if (num_layers < 2 || num_layers + 1 > (uint32_t)kMaxLayers) {
        set_error("FFMLP num_layers should be in [2, %d], but got %u", kMaxLayers - 1, num_layers);
        return NERFTEX_ERR_INVALID;
    }
    if (B % kRowsPerBlock != 0) {
        set_error("ffmlp batch size must be 128 * m (m > 0), but got %u.", B);
        return NERFTEX_ERR_INVALID;
    }
    if (activation > kNone || output_activation > kNone) {
        set_error("FFMLP: unknown activation id");
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

size_t lds_bytes_forward(uint32_t H, uint32_t IN, uint32_t NL, bool training) {
    const size_t frags = (size_t)(frag_count(H, IN) + (NL - 1) * frag_count(H, H) + frag_count(16, H)) * 1024;
    return frags + (training ? (size_t)4 * 16 * kTilesPerWave * (H + 8) * sizeof(elem_t) : 0);  // + the per-wave store patches
}
size_t lds_bytes_dgrad(uint32_t H, uint32_t IN, uint32_t NL, bool with_inputs) {
    return (size_t)(frag_count(H, 16) + (NL - 1) * frag_count(H, H) + (with_inputs ? frag_count(IN, H) : 0)) * 1024;
}
constexpr size_t kLdsLimit = 160 * 1024;
// the streaming forms' one slot: the largest matrix of the chain
size_t lds_bytes_forward_stream(uint32_t H, uint32_t IN) { return (size_t)std::max(std::max(frag_count(H, IN), frag_count(H, H)), frag_count(16, H)) * 1024; }
size_t lds_bytes_dgrad_stream(uint32_t H, uint32_t IN, bool with_inputs) {
    return (size_t)std::max(std::max(frag_count(H, 16), frag_count(H, H)), with_inputs ? frag_count(IN, H) : 0) * 1024;
}

int lds_check(size_t bytes) {
    if (bytes > kLdsLimit) {
        set_error("FFMLP: the weights of this network (%zu KB as MFMA fragments) exceed the 160 KB LDS of a gfx950 CU", bytes / 1024);
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}

template <typename K>
int set_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) NERFTEX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), "hipFuncSetAttribute");
    return NERFTEX_OK;
}

uint32_t persistent_grid(uint32_t B, size_t lds) {
    const uint32_t blocks_needed = B / kRowsPerBlock;
    uint32_t per_cu = lds > 0 ? (uint32_t)(kLdsLimit / lds) : 8;
    const uint32_t wg_cap = knob(kKnobFfmlpWgPerCu) > 0 ? (uint32_t)knob(kKnobFfmlpWgPerCu) : 4u;
    per_cu = per_cu < 1 ? 1 : (per_cu > wg_cap ? wg_cap : per_cu);
    const uint32_t cap = (uint32_t)num_cus() * per_cu;
    return blocks_needed < cap ? (blocks_needed ? blocks_needed : 1) : cap;
}

template <int H, bool INF>
int launch_forward(const void* inputs, const void* weights, uint32_t B, uint32_t IN, uint32_t NL, uint32_t act, uint32_t out_act,
                   void* fwd, void* outputs, hipStream_t st) {
    const bool staged = !INF && lds_bytes_forward(H, IN, NL, true) <= kLdsLimit / 2;  // keep two workgroups per CU
    size_t lds = lds_bytes_forward(H, IN, NL, staged);
    int rc = NERFTEX_OK;
    auto kernel = staged ? ffmlp_forward_kernel<H, INF, true, -1, -1> : ffmlp_forward_kernel<H, INF, false, -1, -1>;
    bool stream = false;
    if constexpr (H >= 128) {  // all fragments do not fit one CU's LDS (hidden 256 x >= 3 layers, hidden 128 x many): one layer at a time
        if (lds > kLdsLimit) {
            stream = true;
            lds = lds_bytes_forward_stream(H, IN);
            kernel = ffmlp_forward_kernel<H, INF, false, -1, -1, true>;
        }
    }
    if ((rc = lds_check(lds)) != NERFTEX_OK) return rc;
    (void)stream;
    if constexpr (H == 64) {  // the field's networks: ReLU inside, no output activation -> both folded in at compile time
        if (act == kRelu && out_act == kNone)
            kernel = staged ? ffmlp_forward_kernel<H, INF, true, (int)kRelu, (int)kNone> : ffmlp_forward_kernel<H, INF, false, (int)kRelu, (int)kNone>;
    }
    rc = set_lds(kernel, lds);
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt(INF ? "ffmlp_inference_kernel" : "ffmlp_forward_kernel", st);
        hipLaunchKernelGGL(kernel, dim3(persistent_grid(B, lds)), dim3(kBlockThreads), lds, st, (const elem_t*)inputs, (const elem_t*)weights,
                           (elem_t*)fwd, (elem_t*)outputs, B, IN, NL, act, out_act, (const int32_t*)nullptr, 0u);
    }
    return check_launch(INF ? "ffmlp_inference" : "ffmlp_forward");
}

// the inference kernel in its rows form, with the template arguments launch_forward<H, true> picks for a ReLU network without an output
// activation: the same instructions per row
template <int H>
int launch_inference_rows(const void* inputs, const void* weights, uint32_t B, uint32_t IN, uint32_t NL, void* outputs, const int32_t* units_dev,
                          uint32_t rows_per_unit, hipStream_t st) {
    const size_t lds = lds_bytes_forward(H, IN, NL, false);
    int rc = lds_check(lds);
    if (rc != NERFTEX_OK) return rc;
    auto kernel = ffmlp_forward_kernel<H, true, false, H == 64 ? (int)kRelu : -1, H == 64 ? (int)kNone : -1, false, true>;
    if ((rc = set_lds(kernel, lds)) != NERFTEX_OK) return rc;
    {
        KernelTimer kt("ffmlp_inference_rows_kernel", st);
        hipLaunchKernelGGL(kernel, dim3(persistent_grid(B, lds)), dim3(kBlockThreads), lds, st, (const elem_t*)inputs, (const elem_t*)weights, (elem_t*)nullptr,
                           (elem_t*)outputs, B, IN, NL, (uint32_t)kRelu, (uint32_t)kNone, units_dev, rows_per_unit);
    }
    return check_launch("curved_field_infer(ffmlp)");
}

template <bool INF>
int dispatch_forward(const void* inputs, const void* weights, uint32_t B, uint32_t IN, uint32_t H, uint32_t NL, uint32_t act,
                     uint32_t out_act, void* fwd, void* outputs, hipStream_t st) {
    switch (H) {
        case 16: return launch_forward<16, INF>(inputs, weights, B, IN, NL, act, out_act, fwd, outputs, st);
        case 32: return launch_forward<32, INF>(inputs, weights, B, IN, NL, act, out_act, fwd, outputs, st);
        case 64: return launch_forward<64, INF>(inputs, weights, B, IN, NL, act, out_act, fwd, outputs, st);
        case 128: return launch_forward<128, INF>(inputs, weights, B, IN, NL, act, out_act, fwd, outputs, st);
        default: return launch_forward<256, INF>(inputs, weights, B, IN, NL, act, out_act, fwd, outputs, st);
    }
}

template <int H>
int launch_dgrad(const void* grad, const void* weights, const void* fwd, void* bb, void* grad_inputs, uint32_t B, uint32_t IN, uint32_t NL,
                 uint32_t act, hipStream_t st) {
    size_t lds = lds_bytes_dgrad(H, IN, NL, grad_inputs != nullptr);
    int rc = NERFTEX_OK;
    auto kernel = ffmlp_dgrad_kernel<H>;
    if constexpr (H >= 128) {
        if (lds > kLdsLimit) {
            lds = lds_bytes_dgrad_stream(H, IN, grad_inputs != nullptr);
            kernel = ffmlp_dgrad_kernel<H, true>;
        }
    }
    if ((rc = lds_check(lds)) != NERFTEX_OK) return rc;
    rc = set_lds(kernel, lds);
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt("ffmlp_dgrad_kernel", st);
        hipLaunchKernelGGL(kernel, dim3(persistent_grid(B, lds)), dim3(kBlockThreads), lds, st, (const elem_t*)grad, (const elem_t*)weights,
                           (const elem_t*)fwd, (elem_t*)bb, (elem_t*)grad_inputs, B, IN, NL, act);
    }
    return check_launch("ffmlp_backward(dgrad)");
}

int weights_aligned(const void* weights);
inline int weights_aligned_fwd(const void* w) { return weights_aligned(w); }

template <int H, int NL, int IT, int ACT, int FIELD = 0>
int launch_fused(const void* grad, const void* inputs, const void* weights, const void* fwd, void* grad_inputs, uint32_t B, uint32_t act,
                 uint32_t n_params, void* grad_weights, hipStream_t st, const void* aux0 = nullptr, const void* aux1 = nullptr,
                 RedSet* defer = nullptr, WorkspaceSlot slot = kWsMlp, const uint32_t* step_live = nullptr) {  // defer: leave the reduction of the partials to the caller
    const bool recompute = fwd == nullptr;
    size_t lds = lds_bytes_dgrad(H, 16 * IT, NL, true) + (recompute ? (size_t)(frag_count(H, 16 * IT) + (NL - 1) * frag_count(H, H)) * 1024 : 0);
    if (lds < 64 * 1024) lds = 64 * 1024;  // the end-of-kernel combine reuses the fragment area
    if (recompute) lds += (size_t)4 * 2 * ((FIELD == 2 ? 3 : 2) + 2 * ((16 * IT + 31) / 32)) * 1024;  // prefetch ring: 4 waves x 2 slots x (grad + input pieces) KiB
    // MEASURED (round 4, profiles/r04_ffmlp_tr_ab.json): transposing LDS reads in place of the selection MFMAs are slower (64.8 / 49.7 us against
    // 59.6 / 47.0; software-pipelined 68.4 / 50.8) -- one wave per SIMD has nobody to hide the LDS round trip behind.  That form is removed.
    int rc = lds_check(lds);
    if (rc != NERFTEX_OK) return rc;
    uint32_t n_parts = B / kRowsPerBlock;
    if (n_parts > (uint32_t)num_cus()) n_parts = (uint32_t)num_cus();  // one workgroup (4 waves, one per SIMD) per CU
    float* partials = static_cast<float*>(workspace(slot, sizeof(float) * (size_t)n_parts * n_params, st));
    if (!partials) return NERFTEX_ERR_HIP;
    auto launch = [&](auto kernel, const char* name) -> int {
        NERFTEX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute");
        KernelTimer kt(name, st);
        hipLaunchKernelGGL(kernel, dim3(n_parts), dim3(kBlockThreads), lds, st, (const elem_t*)grad, (const elem_t*)inputs, (const elem_t*)weights,
                           (const elem_t*)fwd, (elem_t*)grad_inputs, B, act, partials, n_params, aux0, aux1, step_live);
        return NERFTEX_OK;
    };
    if constexpr (FIELD != 0) {
        if (!recompute) {
            set_error("field backward: the recomputing form only");
            return NERFTEX_ERR_INVALID;
        }
        if (step_live)  // the steps the compositing backward flagged as carrying a gradient; the others are not touched
            rc = launch(ffmlp_backward_fused_kernel<H, NL, IT, true, ACT, FIELD, true>, FIELD == 1 ? "field_color_backward_kernel" : "field_sigma_backward_kernel");
        else rc = launch(ffmlp_backward_fused_kernel<H, NL, IT, true, ACT, FIELD>, FIELD == 1 ? "field_color_backward_kernel" : "field_sigma_backward_kernel");
    } else if (recompute) {
        rc = launch(ffmlp_backward_fused_kernel<H, NL, IT, true, ACT>, "ffmlp_backward_recompute_kernel");
    } else {
        rc = launch(ffmlp_backward_fused_kernel<H, NL, IT, false, ACT>, "ffmlp_backward_fused_kernel");
    }
    if (rc != NERFTEX_OK) return rc;
    rc = check_launch("ffmlp_backward(fused)");
    if (rc != NERFTEX_OK) return rc;
    if (defer) {
        *defer = RedSet{partials, n_parts, n_params, static_cast<elem_t*>(grad_weights)};
        return NERFTEX_OK;
    }
    {
        KernelTimer kt("ffmlp_wgrad_reduce_kernel", st);
        hipLaunchKernelGGL(ffmlp_wgrad_reduce_kernel, dim3(div_up(n_params, kRedParams)), dim3(kBlockThreads), 0, st, partials, n_parts, n_params,
                           static_cast<elem_t*>(grad_weights));
    }
    return check_launch("ffmlp_backward(reduce)");
}

// extension entries: the two MLP backward passes of the ngp field with its glue kernels folded into their load stage (FIELD above)
int field_backward_entry(const float* grad_sigma, const float* grad_rgbs, const float* rgbs, const void* h, const void* cin, const void* x_rows,
                         const void* sigma_weights, const void* color_weights, uint32_t B, void* grad_cin, void* grad_x, void* grad_sigma_weights,
                         void* grad_color_weights, float* found_inf, void* stream, const uint32_t* step_live = nullptr, bool consume = false,
                         const StepLossJob* job = nullptr, StepTrailer* trailer_out = nullptr) {  // trailer_out: describe the reduction launch instead of making it
    clear_error();
    if (job != nullptr && (job->n == 0 || job->n > kStepLossMaxRays || job->err == nullptr || job->loss == nullptr)) {
        set_error("field_backward: the step's loss job needs 1 .. %u rays, their errors and a place for the loss", kStepLossMaxRays);
        return NERFTEX_ERR_INVALID;
    }
    if (B % kRowsPerBlock != 0) {
        set_error("field_backward: the batch must be a multiple of %d rows", kRowsPerBlock);
        return NERFTEX_ERR_INVALID;
    }
    if (B == 0) return NERFTEX_OK;
    int rc = weights_aligned_fwd(color_weights);
    if (rc == NERFTEX_OK) rc = weights_aligned_fwd(sigma_weights);
    if (rc != NERFTEX_OK) return rc;
    hipStream_t st = as_stream(stream);
    RedSet colour{}, sig{};  // the two kernels keep their partial sums in different scratch slots: ONE reduction launch for both networks
    rc = launch_fused<64, 3, 2, (int)kRelu, 1>(grad_rgbs, cin, color_weights, nullptr, grad_cin, B, kRelu, 64 * (32 + 64 * 2 + 16), grad_color_weights, st, rgbs,
                                               nullptr, &colour, kWsMlpB, step_live);
    if (rc != NERFTEX_OK) return rc;
    rc = launch_fused<64, 2, 2, (int)kRelu, 2>(grad_cin, x_rows, sigma_weights, nullptr, grad_x, B, kRelu, 64 * (32 + 64 + 16), grad_sigma_weights, st, grad_sigma,
                                               h, &sig, kWsMlp, step_live);
    if (rc != NERFTEX_OK) return rc;
    StepTrailer t{};
    t.set[0] = WgradSet{colour.partials, colour.n_parts, colour.n_params, colour.out};
    t.set[1] = WgradSet{sig.partials, sig.n_parts, sig.n_params, sig.out};
    t.blocks0 = div_up(colour.n_params, kRedParams);
    t.groups = t.blocks0 + div_up(sig.n_params, kRedParams);
    t.bf16 = sizeof(elem_t) == 2 && !std::is_same<elem_t, half_t>::value;
    t.found_inf = found_inf;
    t.consume = consume ? const_cast<uint32_t*>(step_live) : nullptr;
    t.n_consume = consume && step_live ? div_up(B, 32u) : 0u;
    if (job) t.job = *job;
    if (trailer_out) {  // (the caller hands it to the hash-grid backward, or to nerftex_step_trailer_run)
        *trailer_out = t;
        return NERFTEX_OK;
    }
    {
        KernelTimer kt("ffmlp_wgrad_reduce2_kernel", st);
        hipLaunchKernelGGL(ffmlp_wgrad_reduce2_kernel, dim3(t.groups + (job ? 1u : 0u)), dim3(kBlockThreads), 0, st, t);
    }
    return check_launch("field_backward(reduce)");
}

int run_trailer(const StepTrailer& t, void* stream) {
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("ffmlp_wgrad_reduce2_kernel", st);
        hipLaunchKernelGGL(ffmlp_wgrad_reduce2_kernel, dim3(t.groups + (t.job.err ? 1u : 0u)), dim3(kBlockThreads), 0, st, t);
    }
    return check_launch("step_trailer_run");
}

// -1: no fused instantiation for this shape
int launch_backward_fused(const void* grad, const void* inputs, const void* weights, const void* fwd, void* grad_inputs, uint32_t B, uint32_t IN,
                          uint32_t H, uint32_t NL, uint32_t act, uint32_t n_params, void* grad_weights, hipStream_t st) {
    if (H != 64 || IN % 16 != 0 || IN > 64 || NL < 2 || NL > 4) return -1;
    // the two networks of the ngp field (32 inputs, 2 or 3 hidden layers, ReLU) get the activation folded in at compile time
    if (act == kRelu && IN == 32 && NL == 2) return launch_fused<64, 2, 2, (int)kRelu>(grad, inputs, weights, fwd, grad_inputs, B, act, n_params, grad_weights, st);
    if (act == kRelu && IN == 32 && NL == 3) return launch_fused<64, 3, 2, (int)kRelu>(grad, inputs, weights, fwd, grad_inputs, B, act, n_params, grad_weights, st);
#define NERFTEX_FUSED_CASE(nl, it) \
    if (NL == nl && IN == 16 * it) return launch_fused<64, nl, it, -1>(grad, inputs, weights, fwd, grad_inputs, B, act, n_params, grad_weights, st);
    NERFTEX_FUSED_CASE(2, 1) NERFTEX_FUSED_CASE(2, 2) NERFTEX_FUSED_CASE(2, 3) NERFTEX_FUSED_CASE(2, 4)
    NERFTEX_FUSED_CASE(3, 1) NERFTEX_FUSED_CASE(3, 2) NERFTEX_FUSED_CASE(3, 3) NERFTEX_FUSED_CASE(3, 4)
    NERFTEX_FUSED_CASE(4, 1) NERFTEX_FUSED_CASE(4, 2) NERFTEX_FUSED_CASE(4, 3) NERFTEX_FUSED_CASE(4, 4)
#undef NERFTEX_FUSED_CASE
    return -1;
}


// the weight fragments are staged with 16-byte loads of the row-major layers (every layer starts a multiple of 256 halfs into the vector)
int weights_aligned(const void* weights) {
    if (reinterpret_cast<uintptr_t>(weights) & 15) {
        set_error("FFMLP: the weight vector must be 16-byte aligned");
        return NERFTEX_ERR_INVALID;
    }
    return NERFTEX_OK;
}
int forward_entry(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                                     uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                                     void* forward_buffer, void* outputs, void* stream) {
    clear_error();
    int rc = validate(B, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation);
    if (rc != NERFTEX_OK || B == 0) return rc;
    if ((rc = weights_aligned(weights)) != NERFTEX_OK) return rc;
    if (!forward_buffer) {
        set_error("ffmlp_forward: forward_buffer must not be NULL (use ffmlp_inference)");
        return NERFTEX_ERR_INVALID;
    }
    return dispatch_forward<false>(inputs, weights, B, input_dim, hidden_dim, num_layers, activation, output_activation, forward_buffer, outputs,
                                   as_stream(stream));
}

int inference_entry(const void* inputs, const void* weights, uint32_t B, uint32_t input_dim, uint32_t output_dim,
                                       uint32_t hidden_dim, uint32_t num_layers, uint32_t activation, uint32_t output_activation,
                                       void* inference_buffer, void* outputs, void* stream) {
    (void)inference_buffer;  // the reference needs a [B, hidden] scratch; activations stay in registers here
    clear_error();
    int rc = validate(B, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation);
    if (rc != NERFTEX_OK || B == 0) return rc;
    if ((rc = weights_aligned(weights)) != NERFTEX_OK) return rc;
    return dispatch_forward<true>(inputs, weights, B, input_dim, hidden_dim, num_layers, activation, output_activation, nullptr, outputs,
                                  as_stream(stream));
}

int backward_entry(const void* grad, const void* inputs, const void* weights, const void* forward_buffer, uint32_t B,
                                      uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                                      uint32_t output_activation, int calc_grad_inputs, void* backward_buffer, void* grad_inputs,
                                      void* grad_weights, void* stream) {
    clear_error();
    int rc = validate(B, input_dim, output_dim, hidden_dim, num_layers, activation, output_activation);
    if (rc != NERFTEX_OK || B == 0) return rc;
    if ((rc = weights_aligned(weights)) != NERFTEX_OK) return rc;

    hipStream_t st = as_stream(stream);
    const uint32_t H = hidden_dim, IN = input_dim, NL = num_layers;
    void* gi = calc_grad_inputs ? grad_inputs : nullptr;
    const uint32_t n_params = H * (IN + H * (NL - 1) + 16);

    {   // fused activation + weight gradients (the default where instantiated): backward_buffer stays untouched
        if (!knob(kKnobFfmlpBwdSplit)) {  // ffmlp_bwd_split = 1: dgrad kernel, then wgrad kernel through backward_buffer
            rc = launch_backward_fused(grad, inputs, weights, forward_buffer, gi, B, IN, H, NL, activation, n_params, grad_weights, st);
            if (rc >= 0) return rc;  // rc < 0: shape not instantiated -> split path below
        }
    }
    if (!backward_buffer || !forward_buffer) {  // forward_buffer == NULL (recompute the activations) exists in the fused kernel only
        set_error("ffmlp_backward: forward_buffer and backward_buffer must not be NULL for this shape / mode");
        return NERFTEX_ERR_INVALID;
    }

    switch (H) {
        case 16: rc = launch_dgrad<16>(grad, weights, forward_buffer, backward_buffer, gi, B, IN, NL, activation, st); break;
        case 32: rc = launch_dgrad<32>(grad, weights, forward_buffer, backward_buffer, gi, B, IN, NL, activation, st); break;
        case 64: rc = launch_dgrad<64>(grad, weights, forward_buffer, backward_buffer, gi, B, IN, NL, activation, st); break;
        case 128: rc = launch_dgrad<128>(grad, weights, forward_buffer, backward_buffer, gi, B, IN, NL, activation, st); break;
        default: rc = launch_dgrad<256>(grad, weights, forward_buffer, backward_buffer, gi, B, IN, NL, activation, st); break;
    }
    if (rc != NERFTEX_OK) return rc;

    // weight gradients: one launch over (batch chunks, matrices), then the cross-workgroup reduction
    const size_t LS = (size_t)B * H;
    const elem_t* fb = static_cast<const elem_t*>(forward_buffer);
    const elem_t* bb = static_cast<const elem_t*>(backward_buffer);
    WgradArgs args{};
    // matrix 0: dPre = bb[NL-1], In = X
    args.layer[0] = WgradLayer{bb + (size_t)(NL - 1) * LS, static_cast<const elem_t*>(inputs), H, IN, H, IN, 0};
    for (uint32_t l = 1; l < NL; l++)  // hidden matrix l: dPre = bb[NL-1-l], In = fwd[l-1]
        args.layer[l] = WgradLayer{bb + (size_t)(NL - 1 - l) * LS, fb + (size_t)(l - 1) * LS, H, H, H, H, H * IN + (l - 1) * H * H};
    args.layer[NL] = WgradLayer{static_cast<const elem_t*>(grad), fb + (size_t)(NL - 1) * LS, 16, H, 16, H, H * IN + (NL - 1) * H * H};

    uint32_t n_parts = B / 128;  // every wave gets at least one 32-row step
    const uint32_t cap = (uint32_t)num_cus() / 2;
    if (n_parts > cap) n_parts = cap;
    if (n_parts == 0) n_parts = 1;
    float* partials = static_cast<float*>(workspace(kWsMlp, sizeof(float) * (size_t)n_parts * n_params, st));
    if (!partials) return NERFTEX_ERR_HIP;
    const size_t red_bytes = sizeof(float) * 4 * 16 * 256;  // 64 KiB
    {
        KernelTimer kt("ffmlp_wgrad_kernel", st);
        hipLaunchKernelGGL(ffmlp_wgrad_kernel, dim3(n_parts, NL + 1), dim3(kBlockThreads), red_bytes, st, args, B, partials, n_params);
    }
    rc = check_launch("ffmlp_backward(wgrad)");
    if (rc != NERFTEX_OK) return rc;
    {
        KernelTimer kt("ffmlp_wgrad_reduce_kernel", st);
        hipLaunchKernelGGL(ffmlp_wgrad_reduce_kernel, dim3(div_up(n_params, kRedParams)), dim3(kBlockThreads), 0, st, partials, n_parts,
                           n_params, static_cast<elem_t*>(grad_weights));
    }
    return check_launch("ffmlp_backward(reduce)");
}


// extension entry: the fused field forward (field_forward_kernel).  x_rows / h / cin / hc all NULL = inference.
int field_density_entry(const void* feats_lbc, const void* sigma_weights, uint32_t B, float* sigma, void* stream) {
    clear_error();
    if (B % kRowsPerBlock != 0) {
        set_error("field_density: the batch must be a multiple of %d rows", kRowsPerBlock);
        return NERFTEX_ERR_INVALID;
    }
    if (B == 0) return NERFTEX_OK;
    int rc = weights_aligned(sigma_weights);
    if (rc != NERFTEX_OK) return rc;
    const size_t lds = (size_t)14 * 1024;  // the sigma net's 14 fragments
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt("field_density_kernel", st);
        hipLaunchKernelGGL((field_forward_kernel<false, true>), dim3(persistent_grid(B, lds)), dim3(kBlockThreads), lds, st, (const elem_t*)feats_lbc,
                           (const float*)nullptr, (const elem_t*)sigma_weights, (const elem_t*)nullptr, B, sigma, (float*)nullptr, (elem_t*)nullptr,
                           (elem_t*)nullptr, (elem_t*)nullptr, (elem_t*)nullptr, (const int*)nullptr, 0u);
    }
    return check_launch("field_density");
}

int field_forward_entry(const void* feats_lbc, const float* dirs, const void* sigma_weights, const void* color_weights, uint32_t B, float* sigma,
                        float* rgbs, void* x_rows, void* h, void* cin, void* hc, const int32_t* units_dev, uint32_t rows_per_unit, void* stream) {
    clear_error();
    if (B % kRowsPerBlock != 0) {
        set_error("field_forward: the batch must be a multiple of %d rows", kRowsPerBlock);
        return NERFTEX_ERR_INVALID;
    }
    const bool train = x_rows || h || cin || hc;
    if (train && !(x_rows && h && cin)) {
        set_error("field_forward: x_rows, h and cin (and optionally hc) are written together (training) or not at all (inference)");
        return NERFTEX_ERR_INVALID;
    }
    if (B == 0) return NERFTEX_OK;
    int rc = weights_aligned(sigma_weights);
    if (rc == NERFTEX_OK) rc = weights_aligned(color_weights);
    if (rc != NERFTEX_OK) return rc;
    const size_t lds = (size_t)36 * 1024;  // 14 + 22 fragments
    auto kernel = train ? field_forward_kernel<true> : field_forward_kernel<false>;
    hipStream_t st = as_stream(stream);
    {
        KernelTimer kt(train ? "field_forward_train_kernel" : "field_forward_kernel", st);
        hipLaunchKernelGGL(kernel, dim3(persistent_grid(B, lds)), dim3(kBlockThreads), lds, st, (const elem_t*)feats_lbc, dirs, (const elem_t*)sigma_weights,
                           (const elem_t*)color_weights, B, sigma, rgbs, (elem_t*)x_rows, (elem_t*)h, (elem_t*)cin, (elem_t*)hc, units_dev, rows_per_unit);
    }
    return check_launch("field_forward");
}
