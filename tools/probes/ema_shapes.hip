// Timing probe, not part of the library: launch shapes and ticket placements of the parameter-EMA stream (csrc/trainstep.hip ema_kernel) at the
// benchmark field's table size, against a one-group-per-thread kernel with no counter as the floor.  Each variant: <threads> x <blocks per CU>,
// u<16-byte groups in flight per thread>, the ticket (none / at the end / early), how the two device words are read.  Medians of 9 blocks of
// 50 launches, variants interleaved.  profiles/ema_shapes_probe.txt is one run.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Xclang -target-feature -Xclang -packed-fp32-ops -fno-slp-vectorize -mllvm -disable-vector-combine \
//         tools/probes/ema_shapes.hip -o tools/probes/_bin/ema_shapes
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

__device__ __forceinline__ float ema_one(const float s, const float p, const float w) {
#pragma clang fp contract(off)
    float tmp = s - p;
    tmp = tmp * w;
    return s - tmp;
}
__device__ __forceinline__ float4 ema4(float4 a, float4 p, float w) {
    return float4{ema_one(a.x, p.x, w), ema_one(a.y, p.y, w), ema_one(a.z, p.z, w), ema_one(a.w, p.w, w)};
}

// TICKET: 0 none, 1 at the end, 2 early (looked at at the end).  WORDS: 0 thread 0 + LDS, 1 every thread reads them itself
template <int THREADS, int UNROLL, int TICKET, int WORDS>
__global__ __launch_bounds__(THREADS) void k(float* __restrict__ s, const float* __restrict__ p, uint64_t n, double decay, uint32_t* num_updates,
                                             uint32_t* ticket, const uint32_t* live) {
    __shared__ uint32_t words[2];
    uint32_t num_v, live_v;
    if (WORDS == 0) {
        if (threadIdx.x == 0) { words[0] = *num_updates; words[1] = live ? *live : 0u; }
        __syncthreads();
        num_v = words[0]; live_v = words[1];
    } else {
        num_v = *num_updates; live_v = live ? *live : 0u;
    }
    uint32_t mine = 0;
    if (TICKET == 2 && threadIdx.x == 0) mine = atomicAdd(ticket, 1u);
    const double nu = (double)num_v + 1.0;
    const float w = (float)(1.0 - fmin(decay, (1.0 + nu) / (10.0 + nu)));
    if (live_v & 1u) p += 4;  // (keeps live_v alive; never taken here)
    const uint64_t groups = n / 4, stride = (uint64_t)gridDim.x * THREADS;
    float4* s4 = reinterpret_cast<float4*>(s);
    const float4* p4 = reinterpret_cast<const float4*>(p);
    uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    for (; i + (UNROLL - 1) * stride < groups; i += UNROLL * stride) {
        float4 a[UNROLL], b[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) { a[u] = s4[i + u * stride]; b[u] = p4[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) s4[i + u * stride] = ema4(a[u], b[u], w);
    }
    for (; i < groups; i += stride) s4[i] = ema4(s4[i], p4[i], w);
    if (TICKET == 1 && threadIdx.x == 0) mine = atomicAdd(ticket, 1u);
    if (TICKET != 0 && threadIdx.x == 0 && mine == gridDim.x - 1) { *num_updates = num_v + 1u; *ticket = 0u; }
}

__global__ void copyish(float* __restrict__ s, const float* __restrict__ p, uint64_t n, float w) {  // one group per thread, nothing else: the floor
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n / 4) reinterpret_cast<float4*>(s)[i] = ema4(reinterpret_cast<float4*>(s)[i], reinterpret_cast<const float4*>(p)[i], w);
}

struct Variant { const char* name; void (*launch)(float*, const float*, uint64_t, uint32_t*, uint32_t*, int cus); };
#define V(NAME, THREADS, PERCU, UNROLL, TICKET, WORDS) \
    Variant{NAME, [](float* s, const float* p, uint64_t n, uint32_t* num, uint32_t* tk, int cus) { \
        hipLaunchKernelGGL((k<THREADS, UNROLL, TICKET, WORDS>), dim3(cus * PERCU), dim3(THREADS), 0, 0, s, p, n, 0.95, num, tk, (const uint32_t*)nullptr); }}

int main() {
    const uint64_t n = 12599920;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    float *s, *p; uint32_t* words;
    CK(hipMalloc(&s, n * 4)); CK(hipMalloc(&p, n * 4)); CK(hipMalloc(&words, 64));
    CK(hipMemset(s, 0, n * 4)); CK(hipMemset(p, 0, n * 4)); CK(hipMemset(words, 0, 64));
    std::vector<Variant> vs = {
        V("256x8 u2 end lds (shipped)", 256, 8, 2, 1, 0), V("256x8 u2 none lds", 256, 8, 2, 0, 0), V("256x8 u2 none direct", 256, 8, 2, 0, 1),
        V("256x8 u2 early lds", 256, 8, 2, 2, 0), V("256x4 u4 end lds", 256, 4, 4, 1, 0), V("256x4 u4 none lds", 256, 4, 4, 0, 0),
        V("512x2 u4 end lds", 512, 2, 4, 1, 0), V("512x2 u4 none lds", 512, 2, 4, 0, 0), V("1024x1 u4 end lds", 1024, 1, 4, 1, 0),
        V("1024x1 u4 none lds", 1024, 1, 4, 0, 0), V("1024x1 u4 early lds", 1024, 1, 4, 2, 0), V("1024x2 u2 end lds", 1024, 2, 2, 1, 0),
        V("1024x2 u2 none lds", 1024, 2, 2, 0, 0), V("1024x1 u8 end lds", 1024, 1, 8, 1, 0), V("512x4 u2 end lds", 512, 4, 2, 1, 0),
        V("256x16 u1 none lds", 256, 16, 1, 0, 0), V("256x16 u1 end lds", 256, 16, 1, 1, 0),
        Variant{"copyish (floor)", [](float* s, const float* p, uint64_t n, uint32_t*, uint32_t*, int) {
            hipLaunchKernelGGL(copyish, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, 0, s, p, n, 0.05f); }},
    };
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    const int reps = 50, rounds = 9;
    std::vector<std::vector<float>> us(vs.size());
    for (int r = 0; r < rounds + 1; r++)
        for (size_t v = 0; v < vs.size(); v++) {
            CK(hipEventRecord(a, 0));
            for (int i = 0; i < reps; i++) vs[v].launch(s, p, n, words, words + 1, cus);
            CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, a, b));
            if (r) us[v].push_back(ms * 1e3f / reps);
        }
    uint32_t h[2]; CK(hipMemcpy(h, words, 8, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < vs.size(); v++) {
        std::sort(us[v].begin(), us[v].end());
        printf("%-32s median %7.2f us  min %7.2f  max %7.2f\n", vs[v].name, us[v][us[v].size() / 2], us[v].front(), us[v].back());
    }
    printf("num_updates %u ticket %u cus %d\n", h[0], h[1], cus);
    return 0;
}
