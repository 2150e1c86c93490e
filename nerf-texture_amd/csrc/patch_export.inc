// The front of the patch export (nerftex_patch_front, include/nerftex_hip.h): the per-candidate part of MeshFeatureField.sample_patches
// (tools/map.py:1030-1084, use_trimesh_raycast=False) for a chunk of B candidates at once.  Included by raytracer.hip behind closest_hit;
// the scan launch lives beside the neighbour search (knn.hip: patch_scan).
//   patch_cast_kernel    one pixel per lane: the ray of the pixel from the candidate's frame, the trace, the per-patch maximum depth / NaN flag
//   patch_select_kernel  one workgroup: the verdicts in candidate order, the ordered prefix over the accepted ones
// Per-patch words: stats[4 b + {0: bits(max depth), 1: NaN flag, 2: bits(max scan distance), 3: unused}].  A depth and a distance are never
// negative and never NaN (closest_hit answers 10 where nothing compares; the search answers +inf), and a non-negative float orders as its bits,
// so the maximum is an integer atomicMax -- one per wave, behind a shuffle reduction.

namespace nerftex {
namespace {

constexpr uint32_t kVerdictAccepted = 0, kVerdictNan = 2, kVerdictFar = 3, kVerdictMissed = 4, kVerdictNotNeeded = 5;  // (1 is the host's: below y = 0)
constexpr float kPatchLift = 0.1f, kPatchMissDepth = 9.5f;  // tools/map.py:1080, :1083

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, kWave));
    return v;
}

__global__ __launch_bounds__(64) void patch_cast_kernel(const uint32_t S, const float* __restrict__ frames, const float* __restrict__ calibration,
                                                        const Node* __restrict__ nodes, const Tri* __restrict__ tris, float* __restrict__ origins,
                                                        float* __restrict__ intersections, float* __restrict__ rays, uint32_t* __restrict__ stats) {
    const uint32_t b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x, S2 = S * S;
    uint32_t depth_bits = 0u, nan_flag = 0u;  // what a lane past S^2 contributes: nothing
    if (p < S2) {
        const float* T = frames + 12 * (size_t)b;
        const float x = calibration[p / S], y = calibration[p % S];  // meshgrid(indexing='ij'): pixel i S + j sits at (cal[i], cal[j])
        float o[3], ro[3], rd[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            // every product and sum rounded on its own: plain operators under this file's `fp contract(off)` (as dot_plain above).  NOT __fmul_rn /
            // __fadd_rn: the header defines them as x * y and x + y compiled with contraction allowed, and once inlined the backend fuses them
            const float tx = T[4 * a] * x, ty = T[4 * a + 1] * y, lift = kPatchLift * T[4 * a + 2];
            const float txy = tx + ty;
            o[a] = txy + T[4 * a + 3];
            ro[a] = o[a] + lift;
            rd[a] = -T[4 * a + 2];
        }
        int best;
        float mint = closest_hit(V3{ro[0], ro[1], ro[2]}, V3{rd[0], rd[1], rd[2]}, nodes, tris, best);
        const size_t row = (size_t)b * S2 + p;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            origins[3 * row + a] = o[a];
            intersections[3 * row + a] = fmaf(mint, rd[a], ro[a]);  // raytrace_kernel's position
            if (rays) {
                rays[6 * row + a] = ro[a];
                rays[6 * row + 3 + a] = rd[a];
            }
        }
        depth_bits = __float_as_uint(mint) & 0x7fffffffu;  // (a depth of -0 would order above every other as bits)
        nan_flag = (o[0] != o[0] || o[1] != o[1] || o[2] != o[2]) ? 1u : 0u;
    }
    depth_bits = wave_max_u32(depth_bits);
    nan_flag = wave_max_u32(nan_flag);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicMax(stats + 4 * (size_t)b, depth_bits);
        if (nan_flag) atomicOr(stats + 4 * (size_t)b + 1, 1u);
    }
}

constexpr int kSelectThreads = 256;

// One workgroup walks the chunk in tiles of 256 candidates.  A candidate's own test (NaN, then scan distance, then depth: the reference's order)
// gives `pass`; accepted-before = count[0] + the passes in front of it; whoever has max_patch_num accepted before it gets "not needed" -- passing or
// not, as the reference's loop has ended there -- so acceptance is in candidate order and stops exactly at max_patch_num.
__global__ __launch_bounds__(kSelectThreads) void patch_select_kernel(const uint32_t B, const uint32_t* __restrict__ stats, const int has_scan,
                                                                      const float max_scan_dist, const uint32_t max_patch_num,
                                                                      uint8_t* __restrict__ verdict, int32_t* __restrict__ slot, uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_pass[kSelectThreads / kWave];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t before = count[0];  // accepted in front of this tile (uncapped within the call: compared with max_patch_num below)
    for (uint32_t base = 0; base < B; base += kSelectThreads) {
        const uint32_t b = base + threadIdx.x;
        uint32_t code = kVerdictAccepted;
        if (b < B) {
            const float depth = __uint_as_float(stats[4 * (size_t)b]), far = __uint_as_float(stats[4 * (size_t)b + 2]);
            if (stats[4 * (size_t)b + 1]) code = kVerdictNan;
            else if (has_scan && far > max_scan_dist) code = kVerdictFar;
            else if (depth > kPatchMissDepth) code = kVerdictMissed;
        }
        const bool pass = b < B && code == kVerdictAccepted;
        const unsigned long long votes = __ballot(pass);
        if (lane == 0) wave_pass[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t rank = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kSelectThreads / kWave; w++) {
            if (w < wave) rank += wave_pass[w];
            total += wave_pass[w];
        }
        __syncthreads();  // (wave_pass is rewritten by the next tile)
        if (b < B) {
            const uint32_t ahead = before + rank;
            const bool open = ahead < max_patch_num;
            verdict[b] = (uint8_t)(open ? code : kVerdictNotNeeded);
            slot[b] = (open && pass) ? (int32_t)ahead : -1;
        }
        before = min(before + total, max_patch_num);
    }
    if (threadIdx.x == 0) count[0] = before;
}

}  // namespace
}  // namespace nerftex

extern "C" int nerftex_patch_front(const nerftex_patch_front_desc* d, void* stream) {
    using namespace nerftex;
    clear_error();
    if (!d) {
        set_error("patch_front: NULL descriptor");
        return NERFTEX_ERR_INVALID;
    }
    if (!d->tracer || !d->frames || !d->calibration || !d->origins || !d->intersections || !d->stats || !d->verdict || !d->slot || !d->count) {
        set_error("patch_front: the tracer, frames, calibration, origins, intersections, stats, verdict, slot and count must not be NULL");
        return NERFTEX_ERR_INVALID;
    }
    if (d->B == 0 || d->S == 0 || d->max_patch_num == 0) {
        set_error("patch_front: at least one candidate, one pixel per side and one patch to take, but got B = %u, S = %u, max_patch_num = %u", d->B, d->S,
                  d->max_patch_num);
        return NERFTEX_ERR_INVALID;
    }
    const uint64_t S2 = (uint64_t)d->S * d->S;
    if (S2 > 0xffffffffull || S2 * d->B > 0xffffffffull || d->B > 65535u) {
        set_error("patch_front: S^2 B must fit 32 bits and a chunk holds at most 65535 candidates (one grid row each), but got B = %u, S = %u", d->B, d->S);
        return NERFTEX_ERR_INVALID;
    }
    const hipStream_t st = as_stream(stream);
    NERFTEX_HIP_TRY(hipMemsetAsync(d->stats, 0, sizeof(uint32_t) * 4 * (size_t)d->B, st), "patch_front(stats)");
    {
        KernelTimer kt("patch_cast_kernel", st);
        hipLaunchKernelGGL(patch_cast_kernel, dim3(div_up((uint32_t)S2, 64u), d->B), dim3(64), 0, st, d->S, d->frames, d->calibration,
                           static_cast<const Node*>(d->tracer->nodes), static_cast<const Tri*>(d->tracer->triangles), d->origins, d->intersections, d->rays,
                           d->stats);
    }
    if (int rc = check_launch("patch_front(cast)")) return rc;
    if (d->scan)
        if (int rc = patch_scan(d->scan, d->origins, d->B, (uint32_t)S2, d->stats, st)) return rc;
    {
        KernelTimer kt("patch_select_kernel", st);
        hipLaunchKernelGGL(patch_select_kernel, dim3(1), dim3(kSelectThreads), 0, st, d->B, d->stats, d->scan ? 1 : 0, d->max_scan_dist, d->max_patch_num,
                           d->verdict, d->slot, d->count);
    }
    return check_launch("patch_front(select)");
}
