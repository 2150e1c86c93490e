// The planar texture synthesized from exported patches: image quilting with minimum-error boundary cuts, cell by cell on the device.
//
// Role in the reference: patch_matching_and_quilting.py, class patchBasedTextureSynthesis as its __main__ runs it (mode 'Cut', quilt off,
// coarse_KDtree, rotate off, picked_vertices given), and the closing lines of __main__ (:485-511).  include/nerftex_hip.h states the contract.
//
// Per cell, four launches and no host synchronisation (the chosen id never leaves the device):
//   query     the canvas's overlap strips, block-summed along the patch axis into a float64 workspace vector [top | left]
//   distance  grid = slices of the strip x examples: 16-byte loads of the fp32 database rows, (q - db)^2 summed in float64 per thread, then
//             over the workgroup in a fixed order, one partial per (example, slice).  Streams both databases once: the launch that matters.
//   select    ONE workgroup: the partials summed in slice order; the ranked examples extracted one by one as the smallest (distance, id) above
//             the last one -- a scan of the distances (device memory, L2-resident), so no example count is too large for it --; the close-patch
//             filter, k doubled while nothing survives (k above the example set: a status word, and every later launch does nothing);
//             probabilities, cdf and draw in float64 on one lane; then the two cuts: the error strip by the whole workgroup, the row-sequential
//             dynamic program on one wave with the columns across its lanes, the trace back on one lane.  The cuts sit here and not in the copy
//             launch because the copy needs the finished traces and both are one-workgroup work.
//   place     the whole grid: every value of the S x S x C patch is the example's, the canvas's (left of / above a trace) or their mean (on it).
// The canvas is fp32.  A mean is formed in float64 and stored as the fp32 value plus an fp32 residual (a second plane, zero off the seams) that the
// queries, the cuts and a second mean in a corner read with it: the canvas value stays the correctly rounded float64 result however often a corner
// pixel is averaged, and the decisions see the float64 value.
// Included at the end of csrc/knn.hip (its headers, its `#pragma clang fp contract(off)`): one more handle-style entry group of that translation unit.
namespace nerftex {
namespace {

constexpr int kLogStride = NERFTEX_SYNTH_LOG_STRIDE, kLogRanks = 16;
constexpr int kSelectThreads = 1024, kSelectWaves = kSelectThreads / kWave;
constexpr int kDistThreads = 256, kSliceVec = 1024;  // float4 loads per (example, slice): four a thread
constexpr uint32_t kMaxOverlap = 256;                // two float64 rows of the dynamic program in LDS
constexpr uint32_t kTraceLds = 8192;                 // back pointers (one byte each) kept in LDS up to this many strip pixels, else in device memory
constexpr uint32_t kErrLds = 6144;                   // the error strip (float64) kept in LDS up to this many pixels (S = 128: 128 x 48), else in device memory
constexpr uint32_t kLdsRanks = 64;                   // ranked examples and survivors one lane walks: the first ones in LDS, the rest in device memory
constexpr int kStatusOk = 0, kStatusExhausted = 1, kStatusForced = 2, kStatusNotFinite = 3;

struct Geo {
    uint32_t P, E, S, C, md, ps, ov, block, nb, D, Dp, n, side, hor, vert, att;
};

// example e's pixel (i, j): the patches, their row-flipped copies, the column-flipped copies of all of those
__device__ __forceinline__ const float* example_pixel(const Geo& g, const float* __restrict__ patches, uint32_t e, uint32_t i, uint32_t j) {
    const uint32_t base = e % g.P, m = e / g.P;
    const bool h = g.hor && (m & 1u), v = g.vert && (g.hor ? (m >> 1) : m);
    const uint32_t ii = h ? g.S - 1 - i : i, jj = v ? g.S - 1 - j : j;
    return patches + (((size_t)base * g.S + ii) * g.S + jj) * g.C;
}

// a canvas value as the cuts and the queries read it: the fp32 canvas plus the residual a seam's mean left behind (zero on every copied pixel), so
// that a pixel averaged again in a corner starts from the unrounded mean and the fp32 canvas stays the correctly rounded float64 result
__device__ __forceinline__ double canvas_value(const float* __restrict__ canvas, const float* __restrict__ resid, size_t at) {
    return (double)canvas[at] + (double)resid[at];
}

// the two coarse databases: top [E][ov][nb][md] summed over blocks of columns, left [E][nb][ov][md] summed over blocks of rows; rows padded to Dp
__global__ __launch_bounds__(256) void synth_database_kernel(const Geo g, const float* __restrict__ patches, float* __restrict__ db_top, float* __restrict__ db_left) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
    if (idx >= 2 * g.D) return;
    const bool left = idx >= g.D;
    const uint32_t t = left ? idx - g.D : idx, c = t % g.md;
    double s = 0.0;
    if (!left) {
        const uint32_t b = (t / g.md) % g.nb, i = t / (g.md * g.nb);
        for (uint32_t j = b * g.block; j < min((b + 1) * g.block, g.S); j++) s += (double)example_pixel(g, patches, e, i, j)[c];
    } else {
        const uint32_t j = (t / g.md) % g.ov, b = t / (g.md * g.ov);
        for (uint32_t i = b * g.block; i < min((b + 1) * g.block, g.S); i++) s += (double)example_pixel(g, patches, e, i, j)[c];
    }
    (left ? db_left : db_top)[(size_t)e * g.Dp + t] = (float)s;
}

// (a) the coarse query of a cell: [top (Dp) | left (Dp)] float64, the padding stays zero
__global__ __launch_bounds__(256) void synth_query_kernel(const Geo g, uint32_t cell, const float* __restrict__ canvas, const float* __restrict__ resid,
                                                          double* __restrict__ query, const int32_t* __restrict__ status) {
    if (status[0] != kStatusOk) return;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * g.D) return;
    const uint32_t r = cell / g.n, cc = cell % g.n;
    const bool left = idx >= g.D;
    if (left ? cc == 0 : r == 0) return;
    const uint32_t t = left ? idx - g.D : idx, c = t % g.md;
    const size_t y0 = (size_t)(g.ps + g.ov) * r, x0 = (size_t)(g.ps + g.ov) * cc;
    double s = 0.0;
    if (!left) {
        const uint32_t b = (t / g.md) % g.nb, i = t / (g.md * g.nb);
        for (uint32_t j = b * g.block; j < min((b + 1) * g.block, g.S); j++) s += canvas_value(canvas, resid, ((y0 + i) * g.side + x0 + j) * g.C + c);
    } else {
        const uint32_t j = (t / g.md) % g.ov, b = t / (g.md * g.ov);
        for (uint32_t i = b * g.block; i < min((b + 1) * g.block, g.S); i++) s += canvas_value(canvas, resid, ((y0 + i) * g.side + x0 + j) * g.C + c);
    }
    query[(left ? g.Dp : 0u) + t] = s;
}

// (b) squared distances: block (slice, example) sums its float4s of the present strips in a fixed order
__global__ __launch_bounds__(kDistThreads) void synth_distance_kernel(const Geo g, uint32_t cell, uint32_t slices, const float* __restrict__ db_top,
                                                                      const float* __restrict__ db_left, const double* __restrict__ query,
                                                                      double* __restrict__ partial, const int32_t* __restrict__ status) {
    if (status[0] != kStatusOk) return;
    __shared__ double wave_sum[kDistThreads / kWave];
    const uint32_t r = cell / g.n, cc = cell % g.n, e = blockIdx.y, slice = blockIdx.x;
    const uint32_t vec = g.Dp / 4, ntop = r > 0 ? vec : 0u, total = ntop + (cc > 0 ? vec : 0u);
    const uint32_t end = min((slice + 1) * (uint32_t)kSliceVec, total);
    const float4_t* top = reinterpret_cast<const float4_t*>(db_top + (size_t)e * g.Dp);
    const float4_t* left = reinterpret_cast<const float4_t*>(db_left + (size_t)e * g.Dp);
    double acc = 0.0;
    for (uint32_t t = slice * kSliceVec + threadIdx.x; t < end; t += kDistThreads) {
        const bool is_top = t < ntop;
        const uint32_t o = is_top ? t : t - ntop;
        const float4_t v = is_top ? top[o] : left[o];
        const double* q = query + (is_top ? 0u : g.Dp) + 4 * (size_t)o;
        const double d0 = q[0] - (double)v.x, d1 = q[1] - (double)v.y, d2 = q[2] - (double)v.z, d3 = q[3] - (double)v.w;
        acc += d0 * d0;
        acc += d1 * d1;
        acc += d2 * d2;
        acc += d3 * d3;
    }
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) acc += __shfl_xor(acc, m, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < kDistThreads / kWave; w++) s += wave_sum[w];
        partial[(size_t)e * slices + slice] = s;
    }
}

struct SelectBuffers {
    const double* partial;  // [E, slices]
    double* d2;             // [E] squared distances
    int32_t* rank_id;       // [E] ranked ids, as far as extracted
    double* rank_d;         // [E] their distances
    int32_t* surv_id;       // [E] survivors of the last chunk
    double* surv_p;         // [E] their distances, then probabilities
    double* ebuf;           // [S * ov] the error strip
    int8_t* tbuf;           // [S * ov] back pointers when they do not fit into LDS
    int32_t* trace;         // [2 S]: left cut per row, top cut per column
    int32_t* id_map;        // [n * n]
    int32_t* log_ids;       // [n * n, kLogStride]
    double* log_dist;       // [n * n, kLogRanks]
    int32_t* status;        // [0] status, [1] the cell that set it, [2] the chosen id of the current cell
};

// the row-sequential dynamic program of MinErrBouCut over e [H, W] on ONE wave (columns across lanes), and the trace back on its lane 0.
// The window is j-1 .. j+1 clipped, the first minimum wins; the trace starts at the first minimum of the last row.
__device__ void cut_trace(const double* e, uint32_t H, uint32_t W, double (*rows)[kMaxOverlap], int8_t* back, int32_t* __restrict__ trace) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t j = lane; j < W; j += kWave) rows[0][j] = e[j];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i0 = 1; i0 < H; i0 += 8) {
        double ahead[8];  // this lane's first column of the next eight rows, requested together
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) ahead[b] = (i0 + b < H && lane < W) ? e[(size_t)(i0 + b) * W + lane] : 0.0;
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const uint32_t i = i0 + b;
            if (i < H) {
                const double* prev = rows[(i - 1) & 1];
                double* cur = rows[i & 1];
                for (uint32_t j = lane; j < W; j += kWave) {
                    const uint32_t lo = j > 0 ? j - 1 : 0, hi = min(j + 1, W - 1);
                    double best = prev[lo];
                    uint32_t bj = lo;
                    for (uint32_t jj = lo + 1; jj <= hi; jj++) {
                        const double v = prev[jj];
                        if (v < best) { best = v; bj = jj; }
                    }
                    const double ev = j == lane ? ahead[b] : e[(size_t)i * W + j];
                    cur[j] = ev + best;
                    back[(size_t)i * W + j] = (int8_t)((int)bj - (int)j);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0) {
        const double* last = rows[(H - 1) & 1];
        uint32_t t = 0;
        for (uint32_t j = 1; j < W; j++)
            if (last[j] < last[t]) t = j;
        trace[H - 1] = (int32_t)t;
        for (uint32_t i = H - 1; i > 0; i--) {
            t = (uint32_t)((int)t + (int)back[(size_t)i * W + t]);
            trace[i - 1] = (int32_t)t;
        }
    }
}

// (c) the selection and the cuts of one cell
__global__ __launch_bounds__(kSelectThreads) void synth_select_kernel(const Geo g, uint32_t cell, uint32_t slices, const float* __restrict__ patches,
                                                                      const float* __restrict__ picked, const float* __restrict__ canvas, const float* __restrict__ resid,
                                                                      const double* __restrict__ draws,
                                                                      const int32_t* __restrict__ forced, double limit, const SelectBuffers w) {
    if (w.status[0] != kStatusOk) return;
    __shared__ double rows[2][kMaxOverlap];
    __shared__ int8_t back_lds[kTraceLds];
    __shared__ double err_lds[kErrLds];
    __shared__ double rank_d_l[kLdsRanks], surv_p_l[kLdsRanks];
    __shared__ int32_t rank_id_l[kLdsRanks], surv_id_l[kLdsRanks];
    // (a dependent read of device memory costs a lane about a microsecond: the lists one lane walks sit in LDS as far as they fit)
    auto rank_id = [&](uint32_t q) { return q < kLdsRanks ? rank_id_l[q] : w.rank_id[q]; };
    auto rank_d = [&](uint32_t q) { return q < kLdsRanks ? rank_d_l[q] : w.rank_d[q]; };
    auto surv_id = [&](uint32_t q) { return q < kLdsRanks ? surv_id_l[q] : w.surv_id[q]; };
    auto surv_p = [&](uint32_t q) { return q < kLdsRanks ? surv_p_l[q] : w.surv_p[q]; };
    auto set_surv_p = [&](uint32_t q, double v) { if (q < kLdsRanks) surv_p_l[q] = v; else w.surv_p[q] = v; };
    __shared__ double wave_d[kSelectWaves];
    __shared__ int32_t wave_id[kSelectWaves];
    __shared__ double last_d;
    __shared__ int32_t last_id, n_surv_s, chosen_s, fail_s;
    const uint32_t tid = threadIdx.x, r = cell / g.n, cc = cell % g.n;

    for (uint32_t e = tid; e < g.E; e += kSelectThreads) {
        double s = 0.0;
        for (uint32_t k = 0; k < slices; k++) s += w.partial[(size_t)e * slices + k];
        w.d2[e] = s;
    }
    if (tid == 0) { last_d = -1.0; last_id = -1; n_surv_s = 0; fail_s = kStatusOk; }
    __syncthreads();

    uint32_t k = 16, done = 0;
    for (;;) {
        if (k > g.E) {  // sklearn's "k must be less than or equal to the number of training points"
            if (tid == 0) { w.status[1] = (int32_t)cell; w.status[0] = kStatusExhausted; }
            return;
        }
        for (; done < k; done++) {  // rank `done`: the smallest (d2, id) above the last one
            const double ld = last_d;
            const int32_t li = last_id;
            double bd = INFINITY;
            int32_t bi = 0x7fffffff;
            for (uint32_t e = tid; e < g.E; e += kSelectThreads) {
                const double d = w.d2[e];
                const bool above = d > ld || (d == ld && (int32_t)e > li);
                if (above && (d < bd || (d == bd && (int32_t)e < bi))) { bd = d; bi = (int32_t)e; }
            }
#pragma unroll
            for (int m = kWave / 2; m > 0; m >>= 1) {
                const double od = __shfl_xor(bd, m, kWave);
                const int32_t oi = __shfl_xor(bi, m, kWave);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            if ((tid & (kWave - 1)) == 0) { wave_d[tid / kWave] = bd; wave_id[tid / kWave] = bi; }
            __syncthreads();
            if (tid == 0) {
                for (int v = 1; v < kSelectWaves; v++)
                    if (wave_d[v] < bd || (wave_d[v] == bd && wave_id[v] < bi)) { bd = wave_d[v]; bi = wave_id[v]; }
                if (bi == 0x7fffffff) {
                    fail_s = kStatusNotFinite;  // fewer than k comparable distances: a NaN or an infinity among them
                } else {
                    last_d = bd;
                    last_id = bi;
                    if (done < kLdsRanks) { rank_id_l[done] = bi; rank_d_l[done] = sqrt(bd); }
                    else { w.rank_id[done] = bi; w.rank_d[done] = sqrt(bd); }
                }
            }
            __syncthreads();
            if (fail_s != kStatusOk) {
                if (tid == 0) { w.status[1] = (int32_t)cell; w.status[0] = fail_s; }
                return;
            }
        }
        if (tid == 0) {  // the filter over the new ranks (the earlier ones were all removed): close_patch_check
            const bool filter = g.hor || g.vert;
            const int32_t top = r > 0 ? w.id_map[cell - g.n] % (int32_t)g.P : -1, left = cc > 0 ? w.id_map[cell - 1] % (int32_t)g.P : -1;
            int32_t ns = 0;
            for (uint32_t q = k == 16 ? 0 : k / 2; q < k; q++) {
                const int32_t id = rank_id(q);
                bool keep = true;
                if (filter) {
                    const float* a = picked + 3 * (size_t)(id % (int32_t)g.P);
                    for (int side = 0; side < 2; side++) {
                        const int32_t nb = side ? left : top;
                        if (nb < 0) continue;
                        const float* b = picked + 3 * (size_t)nb;
                        const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
                        if (sqrt((dx * dx + dy * dy) + dz * dz) < limit) keep = false;
                    }
                }
                if (keep) {
                    if ((uint32_t)ns < kLdsRanks) surv_id_l[ns] = id; else w.surv_id[ns] = id;
                    set_surv_p((uint32_t)ns, rank_d(q));
                    ns++;
                }
            }
            n_surv_s = ns;
        }
        __syncthreads();
        if (n_surv_s > 0) break;
        k *= 2;
    }

    if (tid == 0) {  // distances2probability, then the legacy np.random.choice: cdf = cumsum(p) / its last entry, searchsorted(u, 'right')
        const int32_t ns = n_surv_s;
        double dmax = surv_p(0);
        for (int32_t q = 1; q < ns; q++) dmax = fmax(dmax, surv_p(q));
        double s = 0.0;
        for (int32_t q = 0; q < ns; q++) { const double p = 1.0 - surv_p(q) / dmax; set_surv_p(q, p); s += p; }
        double s2 = 0.0;
        for (int32_t q = 0; q < ns; q++) {
            double p = surv_p(q) / s;
            p = p * (p > 0.0 ? 1.0 : 0.0);
            p = g.att == 3 ? p * p * p : p;
            set_surv_p(q, p);
            s2 += p;
        }
        bool nan = false;
        for (int32_t q = 0; q < ns; q++) { const double p = surv_p(q) / s2; set_surv_p(q, p); nan = nan || p != p; }
        if (nan)
            for (int32_t q = 0; q < ns; q++) set_surv_p(q, 1.0 / (double)ns);
        double total = 0.0;
        for (int32_t q = 0; q < ns; q++) total += surv_p(q);
        const double u = draws[cell];
        double run = 0.0;
        int32_t pick = 0;
        for (int32_t q = 0; q < ns; q++) {
            run += surv_p(q);
            if (run / total <= u) pick = q + 1;
        }
        const int32_t drawn = surv_id((uint32_t)min(pick, ns - 1));
        int32_t placed = forced ? forced[cell] : drawn;
        if (placed < 0 || placed >= (int32_t)g.E) { fail_s = kStatusForced; placed = drawn; }
        int32_t* li = w.log_ids + (size_t)cell * kLogStride;
        li[0] = (int32_t)k; li[1] = ns; li[2] = drawn; li[3] = placed;
        for (int q = 0; q < kLogRanks; q++) {
            li[4 + q] = rank_id(q);  // (k >= 16 ranks exist)
            li[4 + kLogRanks + q] = q < ns ? surv_id(q) : -1;
            w.log_dist[(size_t)cell * kLogRanks + q] = rank_d(q);
        }
        w.id_map[cell] = placed;
        w.status[2] = placed;
        chosen_s = placed;
    }
    __syncthreads();
    if (fail_s != kStatusOk) {
        if (tid == 0) { w.status[1] = (int32_t)cell; w.status[0] = fail_s; }
        return;
    }

    // ---- the cuts: left first, then top on the patch as the left cut left it (on the transposed strip) ----
    const uint32_t chosen = (uint32_t)chosen_s, npix = g.S * g.ov;
    const size_t y0 = (size_t)(g.ps + g.ov) * r, x0 = (size_t)(g.ps + g.ov) * cc;
    int8_t* back = npix <= kTraceLds ? back_lds : w.tbuf;
    double* ebuf = npix <= kErrLds ? err_lds : w.ebuf;
    if (cc > 0) {
        for (uint32_t p = tid; p < npix; p += kSelectThreads) {
            const uint32_t i = p / g.ov, j = p % g.ov;
            const size_t cv = ((y0 + i) * g.side + x0 + j) * g.C;
            const float* pv = example_pixel(g, patches, chosen, i, j);
            double s = 0.0;
            for (uint32_t c = 0; c < g.md; c++) { const double d = canvas_value(canvas, resid, cv + c) - (double)pv[c]; s += d * d; }
            ebuf[p] = s;
        }
        __syncthreads();
        if (tid < kWave) cut_trace(ebuf, g.S, g.ov, rows, back, w.trace);
        __syncthreads();
    }
    if (r > 0) {
        for (uint32_t p = tid; p < npix; p += kSelectThreads) {
            const uint32_t j = p / g.ov, i = p % g.ov;  // strip row = the cell's column j, strip column = the cell's row i
            const size_t cv = ((y0 + i) * g.side + x0 + j) * g.C;
            const float* pv = example_pixel(g, patches, chosen, i, j);
            const int32_t t = (cc > 0 && j < g.ov) ? w.trace[i] : -1;
            double s = 0.0;
            if (!(t >= 0 && (int32_t)j < t)) {  // (left of the left trace the patch already is the canvas: error 0)
                for (uint32_t c = 0; c < g.md; c++) {
                    const double cvc = canvas_value(canvas, resid, cv + c);
                    const double pc = (int32_t)j == t ? (cvc + (double)pv[c]) / 2 : (double)pv[c];
                    const double d = cvc - pc;
                    s += d * d;
                }
            }
            ebuf[p] = s;
        }
        __syncthreads();
        if (tid < kWave) cut_trace(ebuf, g.S, g.ov, rows, back, w.trace + g.S);
    }
}

// cell 0: first_patch, uncut
__global__ void synth_first_kernel(int32_t first, int32_t* __restrict__ id_map, int32_t* __restrict__ log_ids, double* __restrict__ log_dist, int32_t* __restrict__ status) {
    if (threadIdx.x != 0 || status[0] != kStatusOk) return;
    id_map[0] = first;
    status[2] = first;
    log_ids[0] = 0; log_ids[1] = 0; log_ids[2] = first; log_ids[3] = first;
    for (int q = 0; q < 2 * kLogRanks; q++) log_ids[4 + q] = -1;
    for (int q = 0; q < kLogRanks; q++) log_dist[q] = 0.0;
}

// (d) the masked copy: one thread per value of the S x S x C patch
__global__ __launch_bounds__(256) void synth_place_kernel(const Geo g, uint32_t cell, const float* __restrict__ patches, float* __restrict__ canvas,
                                                          float* __restrict__ resid, int32_t* __restrict__ canvas_id, const int32_t* __restrict__ trace, const int32_t* __restrict__ status) {
    if (status[0] != kStatusOk) return;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)g.S * g.S * g.C) return;
    const uint32_t c = (uint32_t)(idx % g.C), j = (uint32_t)((idx / g.C) % g.S), i = (uint32_t)(idx / ((size_t)g.C * g.S));
    const uint32_t r = cell / g.n, cc = cell % g.n, chosen = (uint32_t)status[2];
    const size_t pix = ((size_t)(g.ps + g.ov) * r + i) * g.side + (size_t)(g.ps + g.ov) * cc + j;
    const float pv = example_pixel(g, patches, chosen, i, j)[c];
    const bool in_left = cc > 0 && j < g.ov, in_top = r > 0 && i < g.ov;
    if (!in_left && !in_top) {
        canvas[pix * g.C + c] = pv;
        resid[pix * g.C + c] = 0.0f;
        if (c == 0) canvas_id[pix] = (int32_t)chosen;
        return;
    }
    const double cv = canvas_value(canvas, resid, pix * g.C + c);
    // 0: the patch's value, 1: the mean, 2: the canvas's
    const int32_t tl = in_left ? trace[i] : -1, tt = in_top ? trace[g.S + j] : -1;
    const int left = !in_left ? 0 : ((int32_t)j < tl ? 2 : ((int32_t)j == tl ? 1 : 0));
    const int top = !in_top ? 0 : ((int32_t)i < tt ? 2 : ((int32_t)i == tt ? 1 : 0));
    // (where the value stays the canvas's, canvas and residual are written back unchanged: |residual| is at most half an ulp of the canvas value)
    double v = (double)pv;
    if (left == 2) v = cv;
    else if (left == 1) v = (cv + v) / 2;
    if (top == 2) v = cv;
    else if (top == 1) v = (cv + v) / 2;
    const float hi = (float)v;
    canvas[pix * g.C + c] = hi;
    resid[pix * g.C + c] = (float)(v - (double)hi);
    if (c == 0) {
        int32_t id = (int32_t)chosen;
        if (left == 2) id = canvas_id[pix];
        if (top == 2) id = canvas_id[pix];
        canvas_id[pix] = id;
    }
}

// ---- the closing remap ----
__global__ __launch_bounds__(256) void synth_mark_kernel(const int32_t* __restrict__ canvas_id, size_t npix, int32_t* __restrict__ flag) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int32_t id = canvas_id[p];
    if (id >= 0) flag[id] = 1;  // (every writer stores the same word)
}

// flag [E] -> pos [E] (position among the used ids), total_id, their count, sample_tbn [count, 9] through the flips; one workgroup
__global__ __launch_bounds__(kSelectThreads) void synth_scan_kernel(const Geo g, const int32_t* __restrict__ flag, int32_t* __restrict__ pos, int32_t* __restrict__ total_id,
                                                                    int32_t* __restrict__ count, const float* __restrict__ sample_tbn, float* __restrict__ tbn_out) {
    __shared__ int32_t chunk_sum[kSelectThreads];
    const uint32_t tid = threadIdx.x, per = div_up(g.E, (uint32_t)kSelectThreads), a = min(tid * per, g.E), b = min(a + per, g.E);
    int32_t s = 0;
    for (uint32_t e = a; e < b; e++) s += flag[e];
    chunk_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int32_t run = 0;
        for (int t = 0; t < kSelectThreads; t++) { const int32_t v = chunk_sum[t]; chunk_sum[t] = run; run += v; }
        count[0] = run;
    }
    __syncthreads();
    int32_t at = chunk_sum[tid];
    for (uint32_t e = a; e < b; e++) {
        pos[e] = flag[e] ? at : -1;
        if (flag[e]) {
            total_id[at] = (int32_t)e;
            const uint32_t base = e % g.P, m = e / g.P;
            const bool h = g.hor && (m & 1u), v = g.vert && (g.hor ? (m >> 1) : m);
            for (int q = 0; q < 9; q++) {
                const float x = sample_tbn[9 * (size_t)base + q];
                tbn_out[9 * (size_t)at + q] = ((q % 3 == 0 && h) != (q % 3 == 1 && v)) ? -x : x;
            }
            at++;
        }
    }
}

__global__ __launch_bounds__(256) void synth_remap_kernel(const int32_t* __restrict__ canvas_id, size_t npix, const int32_t* __restrict__ pos, int32_t* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int32_t id = canvas_id[p];
    out[p] = id >= 0 ? pos[id] : -1;
}

}  // namespace
}  // namespace nerftex

struct nerftex_synth {
    Geo g{};
    nerftex_synth_desc d{};
    uint32_t slices = 1, next_cell = 0, n_total = 0;
    double limit = 0.0;
    void* slab = nullptr;  // one allocation, carved below
    float *db_top = nullptr, *db_left = nullptr, *canvas = nullptr, *resid = nullptr, *tbn_out = nullptr;
    double *query = nullptr, *partial = nullptr, *d2 = nullptr, *rank_d = nullptr, *surv_p = nullptr, *ebuf = nullptr, *log_dist = nullptr;
    int32_t *canvas_id = nullptr, *id_map = nullptr, *log_ids = nullptr, *rank_id = nullptr, *surv_id = nullptr, *trace = nullptr, *status = nullptr, *flag = nullptr,
            *pos = nullptr, *total_id = nullptr, *count = nullptr, *tbn_ids = nullptr;
    int8_t* tbuf = nullptr;
};

extern "C" int nerftex_synth_create(const nerftex_synth_desc* d, nerftex_synth** out) {
    clear_error();
    if (!d || !out) { set_error("synth_create: NULL descriptor or output"); return NERFTEX_ERR_INVALID; }
    *out = nullptr;
    if (d->mode != NERFTEX_SYNTH_CUT) { set_error("synth_create: only mode 'Cut' is built (mode 'blend' is refused)"); return NERFTEX_ERR_INVALID; }
    if (d->quilt) { set_error("synth_create: quilt=True is refused (the reference's script runs without quilting)"); return NERFTEX_ERR_INVALID; }
    if (!d->picked_vertices) {
        set_error("synth_create: picked_vertices are required (the picked_vertices=None neighbour filter, checkForMirrors, is refused)");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->patches || !d->sample_tbn) { set_error("synth_create: patches and sample_tbn must not be NULL"); return NERFTEX_ERR_INVALID; }
    if (d->P == 0 || d->S == 0 || d->C == 0) { set_error("synth_create: P, S and C must be positive"); return NERFTEX_ERR_INVALID; }
    if (d->match_dim == 0 || d->match_dim > d->C) { set_error("synth_create: match_dim %u is outside 1..C = %u", d->match_dim, d->C); return NERFTEX_ERR_INVALID; }
    if (d->overlap_size == 0 || d->overlap_size > kMaxOverlap) { set_error("synth_create: overlap_size %u is outside 1..%u", d->overlap_size, kMaxOverlap); return NERFTEX_ERR_INVALID; }
    if ((uint64_t)d->overlap_size * 2 + d->patch_size != d->S) {
        set_error("synth_create: overlap_size * 2 + patch_size = %llu is not the patch side S = %u", (unsigned long long)d->overlap_size * 2 + d->patch_size, d->S);
        return NERFTEX_ERR_INVALID;
    }
    if (d->output_h != d->output_w) { set_error("synth_create: a non-square output (%u x %u) is refused", d->output_h, d->output_w); return NERFTEX_ERR_INVALID; }
    if (d->output_h <= d->overlap_size) { set_error("synth_create: the output (%u) must be larger than the overlap (%u)", d->output_h, d->overlap_size); return NERFTEX_ERR_INVALID; }
    if (d->attenuation != 1 && d->attenuation != 3) { set_error("synth_create: attenuation is 3 (strict_match) or 1, not %u", d->attenuation); return NERFTEX_ERR_INVALID; }
    if (d->max_patch_res == 0) { set_error("synth_create: max_patch_res must be positive"); return NERFTEX_ERR_INVALID; }
    if (!(d->close_threshold >= 0.0) || !(d->patch_length >= 0.0)) { set_error("synth_create: close_threshold and patch_length must be non-negative numbers"); return NERFTEX_ERR_INVALID; }
    const uint32_t step = d->patch_size + d->overlap_size;
    const uint64_t n = ((uint64_t)(d->output_h - d->overlap_size) + step - 1) / step, side = n * d->patch_size + (n + 1) * d->overlap_size;
    if (side > 16384) { set_error("synth_create: the canvas side %llu is above 16384", (unsigned long long)side); return NERFTEX_ERR_INVALID; }
    const uint64_t E = (uint64_t)d->P * (d->mirror_hor ? 2 : 1) * (d->mirror_vert ? 2 : 1);
    const uint32_t block = d->S / d->max_patch_res > 1 ? d->S / d->max_patch_res : 1, nb = (d->S + block - 1) / block;
    const uint64_t D = (uint64_t)d->overlap_size * nb * d->match_dim, Dp = (D + 3) / 4 * 4;
    if (E > 0x7fffffffull || E * Dp > 0x7fffffffull * 4 || Dp > 0x3fffffffull || E > 65535) {
        set_error("synth_create: %llu examples of %llu coarse values are more than one launch holds (65535 examples)", (unsigned long long)E, (unsigned long long)D);
        return NERFTEX_ERR_INVALID;
    }
    nerftex_synth* s = new nerftex_synth();
    s->d = *d;
    s->g = Geo{d->P, (uint32_t)E, d->S, d->C, d->match_dim, d->patch_size, d->overlap_size, block, nb, (uint32_t)D, (uint32_t)Dp, (uint32_t)n, (uint32_t)side,
               d->mirror_hor ? 1u : 0u, d->mirror_vert ? 1u : 0u, d->attenuation};
    s->limit = d->close_threshold * d->patch_length;
    s->slices = (uint32_t)div_up<uint64_t>(2 * Dp / 4, kSliceVec);
    const Geo& g = s->g;
    const size_t cells = (size_t)g.n * g.n, npix = (size_t)g.side * g.side, strip = (size_t)g.S * g.ov;
    // the carve: every array 256-byte aligned
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t a = at; at += (bytes + 255) / 256 * 256; return a; };
    const size_t o_dbt = take(sizeof(float) * E * Dp), o_dbl = take(sizeof(float) * E * Dp), o_canvas = take(sizeof(float) * npix * g.C), o_resid = take(sizeof(float) * npix * g.C), o_cid = take(4 * npix),
                 o_tids = take(4 * npix), o_idmap = take(4 * cells), o_logi = take(4 * cells * kLogStride), o_logd = take(8 * cells * kLogRanks), o_query = take(8 * 2 * Dp),
                 o_partial = take(8 * E * s->slices), o_d2 = take(8 * E), o_rankd = take(8 * E), o_survp = take(8 * E), o_ranki = take(4 * E), o_survi = take(4 * E),
                 o_ebuf = take(8 * strip), o_tbuf = take(strip), o_trace = take(4 * 2 * (size_t)g.S), o_status = take(16), o_flag = take(4 * E), o_pos = take(4 * E),
                 o_total = take(4 * E), o_count = take(4), o_tbn = take(sizeof(float) * 9 * E);
    if (hipMalloc(&s->slab, at) != hipSuccess) {
        set_error("synth_create: device allocation of %zu bytes failed", at);
        delete s;
        return NERFTEX_ERR_HIP;
    }
    char* b = static_cast<char*>(s->slab);
    s->db_top = (float*)(b + o_dbt); s->db_left = (float*)(b + o_dbl); s->canvas = (float*)(b + o_canvas); s->resid = (float*)(b + o_resid); s->canvas_id = (int32_t*)(b + o_cid);
    s->tbn_ids = (int32_t*)(b + o_tids); s->id_map = (int32_t*)(b + o_idmap); s->log_ids = (int32_t*)(b + o_logi); s->log_dist = (double*)(b + o_logd);
    s->query = (double*)(b + o_query); s->partial = (double*)(b + o_partial); s->d2 = (double*)(b + o_d2); s->rank_d = (double*)(b + o_rankd);
    s->surv_p = (double*)(b + o_survp); s->rank_id = (int32_t*)(b + o_ranki); s->surv_id = (int32_t*)(b + o_survi); s->ebuf = (double*)(b + o_ebuf);
    s->tbuf = (int8_t*)(b + o_tbuf); s->trace = (int32_t*)(b + o_trace); s->status = (int32_t*)(b + o_status); s->flag = (int32_t*)(b + o_flag);
    s->pos = (int32_t*)(b + o_pos); s->total_id = (int32_t*)(b + o_total); s->count = (int32_t*)(b + o_count); s->tbn_out = (float*)(b + o_tbn);
    // zeros everywhere (canvas, padding of the databases and of the query, status), -1 in the ids and the id map
    if (hipMemsetAsync(s->slab, 0, at, nullptr) != hipSuccess || hipMemsetAsync(s->canvas_id, 0xff, 4 * npix, nullptr) != hipSuccess ||
        hipMemsetAsync(s->id_map, 0xff, 4 * cells, nullptr) != hipSuccess || hipMemsetAsync(s->log_ids, 0xff, 4 * cells * kLogStride, nullptr) != hipSuccess) {
        set_error("synth_create: clearing the device arrays failed");
        (void)hipFree(s->slab);
        delete s;
        return NERFTEX_ERR_HIP;
    }
    {
        KernelTimer kt("synth_database_kernel", nullptr);
        hipLaunchKernelGGL(synth_database_kernel, dim3(div_up(2 * g.D, 256u), g.E), dim3(256), 0, nullptr, g, d->patches, s->db_top, s->db_left);
    }
    int rc = check_launch("synth_create(databases)");
    if (rc == NERFTEX_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
        set_error("synth_create: building the databases failed");
        rc = NERFTEX_ERR_HIP;
    }
    if (rc != NERFTEX_OK) {
        (void)hipFree(s->slab);
        delete s;
        return rc;
    }
    *out = s;
    return NERFTEX_OK;
}

extern "C" int nerftex_synth_destroy(nerftex_synth* s) {
    clear_error();
    if (!s) return NERFTEX_OK;
    if (s->slab) (void)hipFree(s->slab);
    delete s;
    return NERFTEX_OK;
}

extern "C" int nerftex_synth_resolve(nerftex_synth* s, uint32_t first_patch, const double* draws, const int32_t* forced, uint32_t cell_begin, uint32_t cell_end,
                                     void* stream) {
    clear_error();
    if (!s) { set_error("synth_resolve: NULL handle"); return NERFTEX_ERR_INVALID; }
    const Geo& g = s->g;
    if (first_patch >= g.E) { set_error("synth_resolve: first_patch %u is outside the %u examples", first_patch, g.E); return NERFTEX_ERR_INVALID; }
    if (cell_begin > cell_end || cell_end > g.n * g.n) { set_error("synth_resolve: cells [%u, %u) are outside the %u x %u canvas", cell_begin, cell_end, g.n, g.n); return NERFTEX_ERR_INVALID; }
    if (cell_begin != s->next_cell) { set_error("synth_resolve: cells are resolved in raster order; the next one is %u, not %u", s->next_cell, cell_begin); return NERFTEX_ERR_INVALID; }
    if (!draws && cell_end > 1) { set_error("synth_resolve: draws must not be NULL"); return NERFTEX_ERR_INVALID; }
    hipStream_t st = as_stream(stream);
    const SelectBuffers w{s->partial, s->d2, s->rank_id, s->rank_d, s->surv_id, s->surv_p, s->ebuf, s->tbuf, s->trace, s->id_map, s->log_ids, s->log_dist, s->status};
    const size_t values = (size_t)g.S * g.S * g.C;
    for (uint32_t cell = cell_begin; cell < cell_end; cell++) {
        if (cell == 0) {
            hipLaunchKernelGGL(synth_first_kernel, dim3(1), dim3(kWave), 0, st, (int32_t)first_patch, s->id_map, s->log_ids, s->log_dist, s->status);
        } else {
            {
                KernelTimer kt("synth_query_kernel", st);
                hipLaunchKernelGGL(synth_query_kernel, dim3(div_up(2 * g.D, 256u)), dim3(256), 0, st, g, cell, s->canvas, s->resid, s->query, s->status);
            }
            {
                KernelTimer kt("synth_distance_kernel", st);
                hipLaunchKernelGGL(synth_distance_kernel, dim3(s->slices, g.E), dim3(kDistThreads), 0, st, g, cell, s->slices, s->db_top, s->db_left, s->query, s->partial,
                                   s->status);
            }
            {
                KernelTimer kt("synth_select_kernel", st);
                hipLaunchKernelGGL(synth_select_kernel, dim3(1), dim3(kSelectThreads), 0, st, g, cell, s->slices, s->d.patches, s->d.picked_vertices, s->canvas, s->resid, draws,
                                   forced, s->limit, w);
            }
        }
        {
            KernelTimer kt("synth_place_kernel", st);
            hipLaunchKernelGGL(synth_place_kernel, dim3((uint32_t)div_up<size_t>(values, 256)), dim3(256), 0, st, g, cell, s->d.patches, s->canvas, s->resid, s->canvas_id, s->trace,
                               s->status);
        }
        const int rc = check_launch("synth_resolve");
        if (rc != NERFTEX_OK) return rc;
        s->next_cell = cell + 1;
    }
    return NERFTEX_OK;
}

extern "C" int nerftex_synth_finish(nerftex_synth* s, void* stream) {
    clear_error();
    if (!s) { set_error("synth_finish: NULL handle"); return NERFTEX_ERR_INVALID; }
    const Geo& g = s->g;
    hipStream_t st = as_stream(stream);
    const size_t npix = (size_t)g.side * g.side;
    NERFTEX_HIP_TRY(hipMemsetAsync(s->flag, 0, 4 * (size_t)g.E, st), "synth_finish");
    hipLaunchKernelGGL(synth_mark_kernel, dim3((uint32_t)div_up<size_t>(npix, 256)), dim3(256), 0, st, s->canvas_id, npix, s->flag);
    hipLaunchKernelGGL(synth_scan_kernel, dim3(1), dim3(kSelectThreads), 0, st, g, s->flag, s->pos, s->total_id, s->count, s->d.sample_tbn, s->tbn_out);
    hipLaunchKernelGGL(synth_remap_kernel, dim3((uint32_t)div_up<size_t>(npix, 256)), dim3(256), 0, st, s->canvas_id, npix, s->pos, s->tbn_ids);
    const int rc = check_launch("synth_finish");
    if (rc != NERFTEX_OK) return rc;
    int32_t host[4] = {0, 0, 0, 0}, count = 0;
    NERFTEX_HIP_TRY(hipMemcpyAsync(host, s->status, sizeof(host), hipMemcpyDeviceToHost, st), "synth_finish");
    NERFTEX_HIP_TRY(hipMemcpyAsync(&count, s->count, sizeof(count), hipMemcpyDeviceToHost, st), "synth_finish");
    NERFTEX_HIP_TRY(hipStreamSynchronize(st), "synth_finish");
    s->n_total = (uint32_t)count;
    if (host[0] == kStatusExhausted) {
        set_error("synth: cell %d: the close-patch filter removed every candidate and the next k exceeds the %u examples", host[1], g.E);
        return NERFTEX_ERR_EXHAUSTED;
    }
    if (host[0] == kStatusForced) { set_error("synth: cell %d: the forced id is outside the %u examples", host[1], g.E); return NERFTEX_ERR_INVALID; }
    if (host[0] == kStatusNotFinite) { set_error("synth: cell %d: the strip distances are not finite", host[1]); return NERFTEX_ERR_INVALID; }
    return NERFTEX_OK;
}

extern "C" int nerftex_synth_result(const nerftex_synth* s, nerftex_synth_view* out) {
    clear_error();
    if (!s || !out) { set_error("synth_result: NULL handle or output"); return NERFTEX_ERR_INVALID; }
    const Geo& g = s->g;
    *out = nerftex_synth_view{s->canvas, s->canvas_id, s->id_map, s->log_ids, s->log_dist, s->tbn_ids, s->tbn_out, s->total_id,
                              g.side, g.n, g.E, g.C, g.block, g.D, s->slices, s->n_total};
    return NERFTEX_OK;
}

extern "C" int nerftex_synth_read(const nerftex_synth* s, uint32_t what, void* dst, size_t bytes, void* stream) {
    clear_error();
    if (!s || !dst) { set_error("synth_read: NULL handle or destination"); return NERFTEX_ERR_INVALID; }
    const Geo& g = s->g;
    const size_t cells = (size_t)g.n * g.n, npix = (size_t)g.side * g.side;
    const void* src = nullptr;
    size_t size = 0;
    switch (what) {
        case NERFTEX_SYNTH_CANVAS: src = s->canvas; size = sizeof(float) * npix * g.C; break;
        case NERFTEX_SYNTH_CANVAS_ID: src = s->canvas_id; size = 4 * npix; break;
        case NERFTEX_SYNTH_ID_MAP: src = s->id_map; size = 4 * cells; break;
        case NERFTEX_SYNTH_LOG_IDS: src = s->log_ids; size = 4 * cells * kLogStride; break;
        case NERFTEX_SYNTH_LOG_DIST: src = s->log_dist; size = 8 * cells * kLogRanks; break;
        case NERFTEX_SYNTH_TBN_IDS: src = s->tbn_ids; size = 4 * npix; break;
        case NERFTEX_SYNTH_TBN: src = s->tbn_out; size = sizeof(float) * 9 * (size_t)s->n_total; break;
        case NERFTEX_SYNTH_TOTAL_ID: src = s->total_id; size = 4 * (size_t)s->n_total; break;
        default: set_error("synth_read: unknown array %u", what); return NERFTEX_ERR_INVALID;
    }
    if (bytes != size) { set_error("synth_read: array %u holds %zu bytes, not %zu", what, size, bytes); return NERFTEX_ERR_INVALID; }
    if (size == 0) return NERFTEX_OK;
    NERFTEX_HIP_TRY(hipMemcpyAsync(dst, src, size, hipMemcpyDeviceToDevice, as_stream(stream)), "synth_read");
    return NERFTEX_OK;
}
