// The hash table's clustering regulariser (gridencoder/grid_clustering.py:93-217 of the reference, tools/map.py:747-774): per level, the
// Student-t soft assignment q of every table row to the level's K cluster centres, the detached target p = normalise_rows(q^2 / colsum(q)),
// and KLDivLoss(mean) = mean_{i,k} p (log p - log q); forward and closed-form gradient in one C-ABI call (nerftex_grid_cluster_loss).
// Included by gridencoder.hip (one translation unit per hash-grid family: tests/test_build_flags.py lists the sources).
//
// Four launches, nothing read back, no float atomics (bitwise reproducible, capturable):
//   colsum_kernel   per block: the column sums of q over the block's rows, fixed order -> colpart[slot][K]
//   colsum_reduce   per level: colpart summed in fixed order -> colsum[level][K]
//   kl_kernel       recomputes q, forms p; per row: the KL terms (fp64 sum), the row's gradient added into grad_table, the centres'
//                   gradient partials -> part[slot][1 + K*C]
//   final_kernel    one block: part summed in fixed order per level; loss = weight * sum / (N K) over the levels, grad_centres +=.
// The level is a device int (the trainer picks it on the host for 16 steps at once): -1 = every level summed (pick_level=False), each
// level gets G blocks (blockIdx.y = level); 0..L-1 = one level, all L*G blocks of the grid share its rows; anything else: loss = NaN,
// no gradient touched.  G is sized on the host from the largest level; the kernels grid-stride over the true count from `offsets`.
//
// Forward arithmetic is the framework's, op by op, in fp32 (contraction off: the correctly rounded intrinsics): d = sum_c (x - c)^2,
// r = 1 / (1 + d / alpha), n = r^((alpha + 1) / 2) (alpha = 1: r itself, as `x ** 1.0` is), q = n / sum_k n, p = (q*q / colsum) / sum_k,
// and log p, log q correctly rounded (fp64 log narrowed).  At init scale (rows within 1e-4 of the centres) q is 1/K up to an ulp and
// the loss is rounding noise the reference's fixture pins: the same roundings reproduce it (tests/test_gpu_curved_training.py).
#include <algorithm>

namespace nerftex {
namespace gridclu {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kMaxParts = 4096;  // blocks per launch: bounds the scratch

struct Args {
    const float* table;
    const int32_t* offsets;
    const float* centres;
    const int32_t* level;
    const float* grad_scale;
    float* loss;
    float* grad_table;
    float* grad_centres;
    double* part;    // [L*G][1 + K*C]
    float* colpart;  // [L*G][K]
    float* colsum;   // [L][K]
    float alpha, weight;
    uint32_t L, G, K, C;
    bool vec;  // table 16-byte aligned
};

// which level this block works on, which of the blocks sharing it this one is, and its partial slot; false: nothing to do here
struct BlockLevel {
    uint32_t lvl, bid, nblk, slot;
};
__device__ __forceinline__ bool block_level(const Args& a, BlockLevel& b) {
    const int lv = *a.level;
    b.slot = blockIdx.y * gridDim.x + blockIdx.x;
    if (lv == -1) {
        b.lvl = blockIdx.y, b.bid = blockIdx.x, b.nblk = gridDim.x;
    } else if (lv >= 0 && (uint32_t)lv < a.L) {
        b.lvl = (uint32_t)lv, b.bid = b.slot, b.nblk = gridDim.x * gridDim.y;
    } else {
        return false;
    }
    return true;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);  // butterfly: the same order on every lane and every run
    return v;
}

// rows per work item: 16 bytes of the [rows, C] table (C < 4), one row otherwise
template <int C>
constexpr int rows_per_item() { return C < 4 ? 4 / C : 1; }

// the rows of item j of a level ([off, off + n) of the table) -> x[R][C]; ok[r]: row exists
template <int C>
__device__ __forceinline__ void load_item(const Args& a, uint32_t off, uint32_t n, uint32_t j, bool vec, float (&x)[rows_per_item<C>()][C],
                                          bool (&ok)[rows_per_item<C>()]) {
    constexpr int R = rows_per_item<C>();
    const uint32_t r0 = j * R;
    const float* p = a.table + ((size_t)off + r0) * C;
    if (vec && r0 + R <= n) {
        constexpr int V = (R * C) / 4;
        float v[R * C];
#pragma unroll
        for (int i = 0; i < V; i++) {
            const float4_t t = *reinterpret_cast<const float4_t*>(p + 4 * i);
            v[4 * i] = t[0], v[4 * i + 1] = t[1], v[4 * i + 2] = t[2], v[4 * i + 3] = t[3];
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            ok[r] = true;
#pragma unroll
            for (int c = 0; c < C; c++) x[r][c] = v[r * C + c];
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        ok[r] = r0 + r < n;
#pragma unroll
        for (int c = 0; c < C; c++) x[r][c] = ok[r] ? p[r * C + c] : 0.0f;
    }
}

// n_k = (1 / (1 + |x - c_k|^2 / alpha))^((alpha + 1) / 2), d_k = |x - c_k|^2, s = sum_k n_k (framework order, fp32 roundings)
template <int C, int KM>
__device__ __forceinline__ float numerators(const float (&x)[C], const float* __restrict__ cen, uint32_t K, float alpha, float (&n)[KM],
                                            float (&d)[KM]) {
    const float pw = (alpha + 1.0f) * 0.5f;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < KM; k++) {
        if ((uint32_t)k < K) {
            float dk = 0.0f;
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float t = __fsub_rn(x[c], cen[k * C + c]);
                dk = __fadd_rn(dk, __fmul_rn(t, t));
            }
            const float r = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fdiv_rn(dk, alpha)));
            n[k] = alpha == 1.0f ? r : powf(r, pw);
            d[k] = dk;
            s = __fadd_rn(s, n[k]);
        } else {
            n[k] = 0.0f, d[k] = 0.0f;
        }
    }
    return s;
}

__device__ __forceinline__ float log_cr(float v) { return (float)log((double)v); }

template <int C, int KM>
__global__ __launch_bounds__(kThreads) void colsum_kernel(Args a) {
    BlockLevel b;
    if (!block_level(a, b)) return;
    constexpr int R = rows_per_item<C>();
    const uint32_t K = a.K;
    const uint32_t off = (uint32_t)a.offsets[b.lvl], n = (uint32_t)a.offsets[b.lvl + 1] - off;
    const bool vec = a.vec && (off * C) % 4 == 0;
    const float* cen = a.centres + (size_t)b.lvl * K * C;
    float acc[KM];
#pragma unroll
    for (int k = 0; k < KM; k++) acc[k] = 0.0f;
    const uint32_t items = (n + R - 1) / R;
    for (uint32_t j = b.bid * kThreads + threadIdx.x; j < items; j += b.nblk * kThreads) {
        float x[R][C];
        bool ok[R];
        load_item<C>(a, off, n, j, vec, x, ok);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!ok[r]) continue;
            float nm[KM], d[KM];
            const float s = numerators<C, KM>(x[r], cen, K, a.alpha, nm, d);
#pragma unroll
            for (int k = 0; k < KM; k++) acc[k] += __fdiv_rn(nm[k], s);
        }
    }
    __shared__ float red[kWaves][KM];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KM; k++) {
        const float v = wave_sum(acc[k]);
        if (lane == 0) red[w][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        float v = red[0][threadIdx.x];
        for (int i = 1; i < kWaves; i++) v += red[i][threadIdx.x];
        a.colpart[(size_t)b.slot * K + threadIdx.x] = v;
    }
}

// the partial slots of level index y (all levels: G slots each; one level: every slot of the grid) -> [lo, hi), the level
__device__ __forceinline__ bool level_parts(const Args& a, uint32_t y, uint32_t& lvl, uint32_t& lo, uint32_t& hi) {
    const int lv = *a.level;
    if (lv == -1) {
        if (y >= a.L) return false;
        lvl = y, lo = y * a.G, hi = lo + a.G;
        return true;
    }
    if (lv < 0 || (uint32_t)lv >= a.L || y != 0) return false;
    lvl = (uint32_t)lv, lo = 0, hi = a.L * a.G;
    return true;
}

__global__ __launch_bounds__(kThreads) void colsum_reduce_kernel(Args a) {
    uint32_t lvl, lo, hi;
    if (!level_parts(a, blockIdx.x, lvl, lo, hi)) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t k = w; k < a.K; k += kWaves) {
        float v = 0.0f;
        for (uint32_t p = lo + lane; p < hi; p += 64) v += a.colpart[(size_t)p * a.K + k];
        v = wave_sum(v);
        if (lane == 0) a.colsum[(size_t)lvl * a.K + k] = v;
    }
}

template <int C, int KM>
__global__ __launch_bounds__(kThreads) void kl_kernel(Args a) {
    BlockLevel b;
    if (!block_level(a, b)) return;
    constexpr int R = rows_per_item<C>();
    const uint32_t K = a.K;
    const uint32_t off = (uint32_t)a.offsets[b.lvl], n = (uint32_t)a.offsets[b.lvl + 1] - off;
    const bool vec = a.vec && (off * C) % 4 == 0;
    const float* cen = a.centres + (size_t)b.lvl * K * C;
    float cs[KM];
#pragma unroll
    for (int k = 0; k < KM; k++) cs[k] = (uint32_t)k < K ? a.colsum[(size_t)b.lvl * K + k] : 1.0f;
    // d loss / d d_k = w / (N K) * (p_k - q_k) * ((alpha + 1) / 2) / (alpha + d_k), times the caller's gradient scale
    const float wnk = n ? (float)((double)a.weight / ((double)n * (double)K)) * (a.grad_scale ? *a.grad_scale : 1.0f) : 0.0f;
    const float half_ap1 = (a.alpha + 1.0f) * 0.5f;
    double term = 0.0;
    float gc[KM * C];
#pragma unroll
    for (int i = 0; i < KM * C; i++) gc[i] = 0.0f;
    const uint32_t items = (n + R - 1) / R;
    for (uint32_t j = b.bid * kThreads + threadIdx.x; j < items; j += b.nblk * kThreads) {
        float x[R][C];
        bool ok[R];
        load_item<C>(a, off, n, j, vec, x, ok);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!ok[r]) continue;
            float nm[KM], d[KM], q[KM], p[KM];
            const float s = numerators<C, KM>(x[r], cen, K, a.alpha, nm, d);
            float ps = 0.0f;
#pragma unroll
            for (int k = 0; k < KM; k++) {
                if ((uint32_t)k >= K) continue;
                q[k] = __fdiv_rn(nm[k], s);
                p[k] = __fdiv_rn(__fmul_rn(q[k], q[k]), cs[k]);
                ps = __fadd_rn(ps, p[k]);
            }
            float g[C];
#pragma unroll
            for (int c = 0; c < C; c++) g[c] = 0.0f;
#pragma unroll
            for (int k = 0; k < KM; k++) {
                if ((uint32_t)k >= K) continue;
                p[k] = __fdiv_rn(p[k], ps);
                term += (double)__fmul_rn(p[k], __fsub_rn(log_cr(p[k]), log_cr(q[k])));
                const float coef = (p[k] - q[k]) * (half_ap1 / (a.alpha + d[k])) * wnk;
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const float gx = coef * 2.0f * (x[r][c] - cen[k * C + c]);
                    g[c] += gx;
                    gc[k * C + c] -= gx;
                }
            }
            if (a.grad_table) {
                float* dst = a.grad_table + ((size_t)off + j * R + r) * C;
#pragma unroll
                for (int c = 0; c < C; c++) dst[c] += g[c];
            }
        }
    }
    // block partials: the KL sum and the K*C centre gradients, in fp64, fixed order (wave butterfly, then the waves in order)
    __shared__ double red[kWaves][1 + KM * C];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t V = 1 + K * C;
    {
        const double v = wave_sum(term);
        if (lane == 0) red[w][0] = v;
    }
#pragma unroll
    for (int i = 0; i < KM * C; i++) {
        if ((uint32_t)i < K * C) {
            const double v = wave_sum((double)gc[i]);
            if (lane == 0) red[w][1 + i] = v;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < V; i += kThreads) {
        double v = red[0][i];
        for (int s = 1; s < kWaves; s++) v += red[s][i];
        a.part[(size_t)b.slot * V + i] = v;
    }
}

__global__ __launch_bounds__(kThreads) void final_kernel(Args a) {
    const int lv = *a.level;
    if (lv < -1 || lv >= (int)a.L) {
        if (threadIdx.x == 0) *a.loss = __builtin_nanf("");
        return;
    }
    const uint32_t KC = a.K * a.C, V = 1 + KC, nlev = lv == -1 ? a.L : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __shared__ double val[1 + 16 * 8];
    double total = 0.0;
    for (uint32_t y = 0; y < nlev; y++) {
        uint32_t lvl, lo, hi;
        level_parts(a, y, lvl, lo, hi);
        for (uint32_t v = w; v < V; v += kWaves) {
            double s = 0.0;
            for (uint32_t p = lo + lane; p < hi; p += 64) s += a.part[(size_t)p * V + v];
            s = wave_sum(s);
            if (lane == 0) val[v] = s;
        }
        __syncthreads();
        const uint32_t n = (uint32_t)(a.offsets[lvl + 1] - a.offsets[lvl]);
        if (threadIdx.x == 0 && n) total += val[0] / ((double)n * (double)a.K);
        if (a.grad_centres)
            for (uint32_t i = threadIdx.x; i < KC; i += kThreads) a.grad_centres[(size_t)lvl * KC + i] += (float)val[1 + i];
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.loss = (float)((double)a.weight * total);
}

// host: the launch geometry and the scratch layout of a descriptor; NERFTEX_OK or NERFTEX_ERR_INVALID (message set)
struct Plan {
    uint32_t G;
    size_t part_off, colpart_off, colsum_off, bytes;
};
inline int plan(const nerftex_grid_cluster_desc* d, Plan& pl) {
    if (!d) {
        set_error("grid_cluster_loss: null descriptor");
        return NERFTEX_ERR_INVALID;
    }
    const uint32_t C = d->C, K = d->K, L = d->L;
    if (!(C == 1 || C == 2 || C == 4 || C == 8) || K < 1 || K > 16 || L < 1 || L > (uint32_t)gridenc::kMaxLevels || !(d->alpha > 0.0f)) {
        set_error("grid_cluster_loss: need C in {1, 2, 4, 8}, 1 <= K <= 16, 1 <= L <= %d, alpha > 0 (got C=%u K=%u L=%u alpha=%g)",
                  gridenc::kMaxLevels, C, K, L, (double)d->alpha);
        return NERFTEX_ERR_INVALID;
    }
    const uint32_t R = C < 4 ? 4 / C : 1;
    const uint64_t items = ((uint64_t)d->max_level_rows + R - 1) / R;
    const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((items + kThreads - 1) / kThreads, 1), kMaxParts);
    pl.G = (uint32_t)std::max<uint64_t>((blocks + L - 1) / L, 1);
    const size_t slots = (size_t)L * pl.G;
    pl.part_off = 0;
    pl.colpart_off = slots * (1 + K * C) * sizeof(double);
    pl.colsum_off = pl.colpart_off + (slots * K * sizeof(float) + 15) / 16 * 16;
    pl.bytes = pl.colsum_off + (size_t)L * K * sizeof(float);
    return NERFTEX_OK;
}

template <int C, int KM>
void launch_rows(const Args& a, dim3 grid, hipStream_t st, bool kl) {
    if (kl) {
        KernelTimer kt("grid_cluster_kl_kernel", st);
        hipLaunchKernelGGL((kl_kernel<C, KM>), grid, dim3(kThreads), 0, st, a);
    } else {
        KernelTimer kt("grid_cluster_colsum_kernel", st);
        hipLaunchKernelGGL((colsum_kernel<C, KM>), grid, dim3(kThreads), 0, st, a);
    }
}

template <int C>
void launch_rows_c(const Args& a, dim3 grid, hipStream_t st, bool kl) {
    if (a.K <= 4)
        launch_rows<C, 4>(a, grid, st, kl);
    else if (a.K <= 8)
        launch_rows<C, 8>(a, grid, st, kl);
    else
        launch_rows<C, 16>(a, grid, st, kl);
}

inline void launch_rows_any(const Args& a, dim3 grid, hipStream_t st, bool kl) {
    switch (a.C) {
        case 1: launch_rows_c<1>(a, grid, st, kl); break;
        case 2: launch_rows_c<2>(a, grid, st, kl); break;
        case 4: launch_rows_c<4>(a, grid, st, kl); break;
        default: launch_rows_c<8>(a, grid, st, kl); break;
    }
}

}  // namespace gridclu
}  // namespace nerftex

extern "C" int nerftex_grid_cluster_scratch_bytes(const nerftex_grid_cluster_desc* desc, size_t* bytes) {
    using namespace nerftex;
    clear_error();
    gridclu::Plan pl;
    const int rc = gridclu::plan(desc, pl);
    if (rc != NERFTEX_OK) return rc;
    if (!bytes) {
        set_error("grid_cluster_scratch_bytes: null output");
        return NERFTEX_ERR_INVALID;
    }
    *bytes = pl.bytes;
    return NERFTEX_OK;
}

extern "C" int nerftex_grid_cluster_loss(const nerftex_grid_cluster_desc* d, void* stream) {
    using namespace nerftex;
    using namespace nerftex::gridclu;
    clear_error();
    Plan pl;
    int rc = plan(d, pl);
    if (rc != NERFTEX_OK) return rc;
    if (!d->table || !d->offsets || !d->centres || !d->level || !d->loss || !d->scratch) {
        set_error("grid_cluster_loss: table, offsets, centres, level, loss and scratch are required");
        return NERFTEX_ERR_INVALID;
    }
    if (d->scratch_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(d->scratch) & 15) != 0) {
        set_error("grid_cluster_loss: scratch of %zu bytes, 16-byte aligned, needed (got %zu)", pl.bytes, d->scratch_bytes);
        return NERFTEX_ERR_INVALID;
    }
    Args a;
    a.table = d->table, a.offsets = d->offsets, a.centres = d->centres, a.level = d->level, a.grad_scale = d->grad_scale;
    a.loss = d->loss, a.grad_table = d->grad_table, a.grad_centres = d->grad_centres;
    char* s = static_cast<char*>(d->scratch);
    a.part = reinterpret_cast<double*>(s + pl.part_off);
    a.colpart = reinterpret_cast<float*>(s + pl.colpart_off);
    a.colsum = reinterpret_cast<float*>(s + pl.colsum_off);
    a.alpha = d->alpha, a.weight = d->weight;
    a.L = d->L, a.G = pl.G, a.K = d->K, a.C = d->C;
    a.vec = (reinterpret_cast<uintptr_t>(d->table) & 15) == 0;
    const hipStream_t st = as_stream(stream);
    const dim3 grid(pl.G, d->L);
    launch_rows_any(a, grid, st, false);
    if ((rc = check_launch("grid_cluster_loss(colsum)")) != NERFTEX_OK) return rc;
    {
        KernelTimer kt("grid_cluster_colsum_reduce_kernel", st);
        hipLaunchKernelGGL(colsum_reduce_kernel, dim3(d->L), dim3(kThreads), 0, st, a);
    }
    if ((rc = check_launch("grid_cluster_loss(colsum_reduce)")) != NERFTEX_OK) return rc;
    launch_rows_any(a, grid, st, true);
    if ((rc = check_launch("grid_cluster_loss(kl)")) != NERFTEX_OK) return rc;
    {
        KernelTimer kt("grid_cluster_final_kernel", st);
        hipLaunchKernelGGL(final_kernel, dim3(1), dim3(kThreads), 0, st, a);
    }
    return check_launch("grid_cluster_loss(final)");
}
