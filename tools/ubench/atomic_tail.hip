// atomic_tail.hip — what the counter sum at the end of a streaming kernel costs (gfx950).  A grid-stride kernel of 256-thread workgroups reads
// n uint32 and reduces a 64-bit sum; the variants differ only in how the sum reaches global memory.  Prints the HIP-event time per launch
// (median of 20 after 3 warm-ups) and the nanoseconds per atomic derived from (b) - (a).   hipcc --offload-arch=gfx950 -O3 atomic_tail.hip -o atomic_tail
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

enum { NONE, WAVE, BLOCK, STRIPED, RETURNING };

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// out[0..63]: the counters (WAVE / BLOCK / RETURNING use out[0], STRIPED one of 64 words 64 bytes apart); sink: one word per thread for NONE / RETURNING
template <int KIND>
__global__ void __launch_bounds__(256) k(const uint32_t *in, uint32_t n, unsigned long long *out, unsigned long long *sink) {
    __shared__ unsigned long long part[4];
    unsigned long long v = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) v += in[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const bool lead = (threadIdx.x & 63) == 0;
    if (KIND == NONE) { if (lead && v == 0x123456789abcull) sink[blockIdx.x] = v; }     // keeps the loads alive; never true for the input used
    if (KIND == WAVE) { if (lead && v) atomicAdd(out, v); }
    if (KIND == STRIPED) { if (lead && v) atomicAdd(out + 8 * ((blockIdx.x * 4 + (threadIdx.x >> 6)) & 63), v); }
    if (KIND == RETURNING) { if (lead && v) { const unsigned long long old = atomicAdd(out, v); if (old == 0x123456789abcull) sink[blockIdx.x] = old; } }
    if (KIND == BLOCK) {
        if (lead) part[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) { const unsigned long long s = part[0] + part[1] + part[2] + part[3]; if (s) atomicAdd(out, s); }
    }
}

template <int KIND>
static int run(const char *name, const uint32_t *in, uint32_t n, uint32_t cap, unsigned long long *out, unsigned long long *sink, unsigned long long want, double *ms_out) {
    const uint32_t blocks = std::min<uint32_t>((n + 255) / 256, cap);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int r = 0; r < 23; r++) {
        CHECK(hipMemsetAsync(out, 0, 64 * 8 * 8, 0));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, in, n, out, sink);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float t; CHECK(hipEventElapsedTime(&t, e0, e1));
        if (r >= 3) ms.push_back(t);
    }
    unsigned long long h[64 * 8];
    CHECK(hipMemcpy(h, out, sizeof h, hipMemcpyDeviceToHost));
    unsigned long long sum = 0;
    for (int i = 0; i < 64; i++) sum += h[8 * i];
    if (KIND != NONE && sum != want) { fprintf(stderr, "%s: sum %llu, expected %llu\n", name, sum, want); return 1; }
    std::sort(ms.begin(), ms.end());
    const double med = 0.5 * (ms[9] + ms[10]);
    const uint32_t atomics = KIND == NONE ? 0 : KIND == BLOCK ? blocks : blocks * 4;
    printf("  %-44s grid %5u  atomics %6u  median %8.4f ms  (min %.4f, max %.4f)\n", name, blocks, atomics, med, ms.front(), ms.back());
    *ms_out = med;
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return 0;
}

int main() {
    const uint32_t sizes[2] = {5000000u, 14000000u};
    uint32_t *in;
    unsigned long long *out, *sink;
    CHECK(hipMalloc(&in, (size_t)sizes[1] * 4));
    CHECK(hipMalloc(&out, 64 * 8 * 8));
    CHECK(hipMalloc(&sink, 16384 * 8));
    std::vector<uint32_t> h(sizes[1]);
    for (uint32_t i = 0; i < sizes[1]; i++) h[i] = (i * 2654435761u >> 20) + 1;     // 1 .. 4096: no wave sums to zero
    CHECK(hipMemcpy(in, h.data(), (size_t)sizes[1] * 4, hipMemcpyHostToDevice));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("atomic_tail: %s, %d CUs; 256-thread workgroups, 64-bit sum of n uint32, HIP-event time per launch, median of 20 after 3 warm-ups\n", prop.gcnArchName, prop.multiProcessorCount);
    for (int s = 0; s < 2; s++) {
        const uint32_t n = sizes[s];
        unsigned long long want = 0;
        for (uint32_t i = 0; i < n; i++) want += h[i];
        printf("n = %u\n", n);
        double a, b, c, d, e, f;
        if (run<NONE>("(a) no atomic", in, n, 16384, out, sink, want, &a)) return 1;
        if (run<WAVE>("(b) one atomicAdd per wave, one address", in, n, 16384, out, sink, want, &b)) return 1;
        if (run<BLOCK>("(c) one per workgroup", in, n, 16384, out, sink, want, &c)) return 1;
        for (uint32_t cap : {4096u, 2048u, 1024u})
            if (run<BLOCK>("(d) one per workgroup, grid capped", in, n, cap, out, sink, want, &d)) return 1;
        for (uint32_t cap : {4096u, 2048u, 1024u})
            if (run<NONE>("(a') no atomic, grid capped", in, n, cap, out, sink, want, &d)) return 1;
        if (run<STRIPED>("(e) one per wave, striped over 64 addresses", in, n, 16384, out, sink, want, &e)) return 1;
        if (run<RETURNING>("(f) one per wave, returning, old value used", in, n, 16384, out, sink, want, &f)) return 1;
        const uint32_t nat = std::min<uint32_t>((n + 255) / 256, 16384) * 4;
        printf("  (b) - (a) = %.4f ms over %u atomics = %.2f ns per same-address atomic; (f) - (a) = %.4f ms = %.2f ns per returning atomic; (c) - (a) = %.4f ms\n",
               b - a, nat, (b - a) * 1e6 / nat, f - a, (f - a) * 1e6 / nat, c - a);
    }
    return 0;
}
