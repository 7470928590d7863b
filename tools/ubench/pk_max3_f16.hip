// pk_max3_f16.hip — does v_pk_maximum3_f16 on gfx950 order non-negative 16-bit integers (< 0x7C00) like an unsigned
// integer max, including the f16-denormal range (< 0x0400)?  And what does it cost?  Exhaustive check over all
// (a, b) pairs against 64 c values per pair + issue-rate measurement.
//   hipcc --offload-arch=gfx950 -O3 pk_max3_f16.hip -o pk_max3_f16
#include <hip/hip_runtime.h>
#include <cstdio>
__device__ __forceinline__ uint32_t pkmax3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm volatile("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__global__ void check(unsigned long long *bad, unsigned long long *nan_small) {
    // a = blockIdx (0..0x7FFF), b = thread-strided over 0..0x7FFF, c = 64 spread values; halves carry different data
    const uint32_t a = blockIdx.x;
    unsigned long long nb = 0, ns = 0;
    for (uint32_t b = threadIdx.x; b < 0x8000; b += blockDim.x)
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t c = (k * 0x1F3u + b * 7u) & 0x7FFFu;
            const uint32_t a2 = (a * 3u + 1u) & 0x7FFFu, b2 = (b * 5u + 2u) & 0x7FFFu, c2 = (c * 7u + 3u) & 0x7FFFu;
            const uint32_t r = pkmax3(a | (a2 << 16), b | (b2 << 16), c | (c2 << 16));
            const uint32_t lo = max(max(a, b), c), hi = max(max(a2, b2), c2);
            const uint32_t mlo = max(max(a, b), c), mhi = hi;
            // claim 1: all operands < 0x7C00  => exact integer max
            if (mlo < 0x7C00u && (r & 0xFFFFu) != lo) nb++;
            if (mhi < 0x7C00u && (r >> 16) != hi) nb++;
            // claim 2: some operand >= 0x7C00 (inf / NaN patterns) => result >= 0x7C00 (so an overflow is never lost)
            if (mlo >= 0x7C00u && (r & 0xFFFFu) < 0x7C00u) ns++;
            if (mhi >= 0x7C00u && (r >> 16) < 0x7C00u) ns++;
        }
    if (nb) atomicAdd(bad, nb);
    if (ns) atomicAdd(nan_small, ns);
}
// The biased score domain of uc_sw_pk_impl.hpp rests on two more properties (its header comment, "overflow"):
//  claim 3: an operand in [0x7C00, 0x7FFF] (+inf, NaN with a clear sign bit) gives a result in [0x7C00, 0x7FFF], whatever the other two are - positive
//           numbers, the negative patterns 0x8000 .. 0x807E an unfloored x' can take, or NaN themselves - and in whichever operand slot it stands:
//           a stored H', E' never has its sign bit set, so the plain 32-bit add of the next x' cannot carry into the neighbouring half;
//  claim 4: x' in [0x8000, 0x807E] loses against e' >= 0x0080: max3(x', e', f') = max(e', f') as unsigned integers (e', f' < 0x7C00).
__global__ void check_biased(unsigned long long *bad_nan, unsigned long long *bad_neg) {
    const uint32_t n = 0x7C00u + blockIdx.x;            // 1024 blocks: every pattern of [0x7C00, 0x7FFF]
    unsigned long long b3 = 0, b4 = 0;
    for (uint32_t o = threadIdx.x; o <= 0x807Eu; o += blockDim.x) {
        const uint32_t others[6] = {0x0080u, 0u, 0x7BFFu, 0x8000u, 0x807Eu, 0x7E00u};
        for (int k = 0; k < 6; k++) {
            const uint32_t p = others[k];
            // low half: (n, o, p) in the three rotations; high half: the same with o and p exchanged
            const uint32_t r0 = pkmax3(n | (n << 16), o | (p << 16), p | (o << 16));
            const uint32_t r1 = pkmax3(o | (p << 16), n | (n << 16), p | (o << 16));
            const uint32_t r2 = pkmax3(o | (p << 16), p | (o << 16), n | (n << 16));
            const uint32_t rs[3] = {r0, r1, r2};
            for (int j = 0; j < 3; j++) {
                const uint32_t lo = rs[j] & 0xFFFFu, hi = rs[j] >> 16;
                if (lo < 0x7C00u || lo > 0x7FFFu) b3++;
                if (hi < 0x7C00u || hi > 0x7FFFu) b3++;
            }
        }
    }
    // claim 4: x' = 0x8000 + (block % 127), e' over [0x0080, 0x7BFF], f' spread over [0, 0x7BFF]
    const uint32_t x = 0x8000u + blockIdx.x % 127u;
    for (uint32_t e = 0x0080u + threadIdx.x; e < 0x7C00u; e += blockDim.x)
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t f = (k * 0x7C1u + e * 13u + blockIdx.x) % 0x7C00u, e2 = 0x0080u + (e * 7u + k) % (0x7C00u - 0x0080u), f2 = (f * 5u + 1u) % 0x7C00u;
            const uint32_t r = pkmax3(x | (x << 16), e | (e2 << 16), f | (f2 << 16));
            if ((r & 0xFFFFu) != max(e, f)) b4++;
            if ((r >> 16) != max(e2, f2)) b4++;
        }
    if (b3) atomicAdd(bad_nan, b3);
    if (b4) atomicAdd(bad_neg, b4);
}
__global__ void __launch_bounds__(256) rate(uint32_t *out, int iters, uint32_t seed) {
    uint32_t a[8];
    for (int i = 0; i < 8; i++) a[i] = (seed * (threadIdx.x + 1) + i * 77) & 0x3FFF3FFFu;
    uint32_t b = seed & 0x1FFF1FFFu;
    for (int it = 0; it < iters; it++)
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int i = 0; i < 8; i++) a[i] = pkmax3(a[i], b, (uint32_t)(i + u * 8));
    uint32_t s = 0;
    for (int i = 0; i < 8; i++) s ^= a[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
int main() {
    unsigned long long *d, h[2] = {0, 0};
    hipMalloc(&d, 16); hipMemset(d, 0, 16);
    hipLaunchKernelGGL(check, dim3(0x8000), dim3(256), 0, 0, d, d + 1);
    hipMemcpy(h, d, 16, hipMemcpyDeviceToHost);
    printf("mismatches below 0x7C00: %llu   lost overflows: %llu   (of %.3g packed triples)\n", h[0], h[1], 32768.0 * 32768.0 * 64);
    unsigned long long h2[2] = {0, 0};
    hipMemset(d, 0, 16);
    hipLaunchKernelGGL(check_biased, dim3(1024), dim3(256), 0, 0, d, d + 1);
    hipMemcpy(h2, d, 16, hipMemcpyDeviceToHost);
    printf("biased domain: results outside [0x7C00, 0x7FFF] with an operand inside it: %llu   negative x' winning against e' >= 0x0080: %llu\n", h2[0], h2[1]);
    uint32_t *o; hipMalloc(&o, 256 * 8 * 256 * 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 20000, blocks = 256 * 8;
    hipLaunchKernelGGL(rate, dim3(blocks), dim3(256), 0, 0, o, 100, 12345u);
    hipEventRecord(e0);
    hipLaunchKernelGGL(rate, dim3(blocks), dim3(256), 0, 0, o, iters, 12345u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("v_pk_maximum3_f16 %8.3f ms  %.2f cycles/wave-instr/SIMD @2.4GHz\n", ms, ms * 1e-3 * 2.4e9 / ((double)blocks * 4 * iters * 32 / 1024.0));
    return 0;
}
