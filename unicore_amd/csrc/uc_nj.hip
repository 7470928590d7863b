// uc_nj.hip — the counts of the tree builder `nj` on the device (rule UC-N/D).
//   consumes  NjCountArgs: n rows of w bytes, validated by nj_counts_validate
//   produces  comp / diff of every row pair as uint32 triangles, equal to nj_counts_host's.  The joins on the resulting matrix are uc_nj_join.hip's
//   encode    bytes -> codes (0 = uninformative, 1 .. 26 = letters), four columns per dword, laid out [dword][row] with the rows padded to the tile
//             and the dwords to the LDS chunk: padding is code 0 and counts nothing, so no loop below has a tail
//   counts    one workgroup per NJ_TILE x NJ_TILE tile of row pairs (upper triangle of tiles); a chunk of both row tiles is fetched as contiguous
//             16-byte cells of the encoded rows, one chunk ahead in registers, and staged as it is.  The arithmetic on a staged chunk and the
//             write-out are uc_nj_device.h's, shared with the bootstrap's gathering kernel.  A call beyond the byte budget runs slice after slice
//             of columns on one stream and the kernel adds into the triangles
// Scratch is hipMalloc'ed and freed inside the call, as in uc_msa.hip.
#include "uc_nj.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "uc_engine.h"
#include "uc_nj_device.h"

namespace uc {

namespace {

__global__ void __launch_bounds__(256) nj_encode_kernel(const uint8_t *raw, uint32_t n, uint64_t ws, uint32_t np, uint64_t wq, uint32_t *E) {
    const uint64_t total = wq * np;
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (uint64_t)gridDim.x * 256) {
        const uint32_t row = (uint32_t)(x % np);
        const uint64_t col = x / np * 4;
        uint32_t v = 0;
        if (row < n)
            for (uint32_t b = 0; b < 4; b++)
                if (col + b < ws) v |= (uint32_t)nj_code(raw[(uint64_t)row * ws + col + b]) << (8 * b);
        E[x] = v;
    }
}

// E: [n_chunks * NJ_CW][np] dwords, np a multiple of NJ_TILE.  grid (np / NJ_TILE, np / NJ_TILE); tiles below the diagonal leave at once
__global__ void __launch_bounds__(256) nj_count_kernel(const uint32_t *E, uint32_t n, uint32_t np, uint32_t n_chunks, uint32_t *comp, uint32_t *diff) {
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ uint4 sA[NJ_CW * (NJ_TILE / 4)], sB[NJ_CW * (NJ_TILE / 4)];
    constexpr uint32_t Q = NJ_TILE / 4, PER = NJ_CW * Q / 256;      // uint4 per dword row of a tile; staging loads per thread and tile
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const uint4 *E4 = (const uint4 *)E;
    const uint64_t np4 = np / 4;
    uint32_t c[NJ_TR][NJ_TR], d[NJ_TR][NJ_TR];
    for (uint32_t r = 0; r < NJ_TR; r++)
        for (uint32_t s = 0; s < NJ_TR; s++) c[r][s] = d[r][s] = 0;
    static_assert(PER == 4, "the staging registers are written out below");
    uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
    // chunk k of both row tiles into registers: uint4 q of a tile is rows 4 (q % Q) .. + 3 of dword q / Q
#define NJ_FETCH1(k, u, A, B)                                                            \
    {                                                                                    \
        const uint32_t q = tid + 256 * (u);                                              \
        const uint64_t base = ((uint64_t)(k) * NJ_CW + q / Q) * np4 + q % Q;             \
        A = E4[base + (uint64_t)ti * Q];                                                 \
        B = E4[base + (uint64_t)tj * Q];                                                 \
    }
#define NJ_FETCH(k) NJ_FETCH1(k, 0, ra0, rb0) NJ_FETCH1(k, 1, ra1, rb1) NJ_FETCH1(k, 2, ra2, rb2) NJ_FETCH1(k, 3, ra3, rb3)
    NJ_FETCH(0)
    for (uint32_t k = 0; k < n_chunks; k++) {
        __syncthreads();      // the chunk before is read
        sA[tid] = ra0; sA[tid + 256] = ra1; sA[tid + 512] = ra2; sA[tid + 768] = ra3;
        sB[tid] = rb0; sB[tid + 256] = rb1; sB[tid + 512] = rb2; sB[tid + 768] = rb3;
        __syncthreads();
        if (k + 1 < n_chunks) { NJ_FETCH(k + 1) }
        nj_count_chunk(sA, sB, ty, tx, c, d);
    }
#undef NJ_FETCH
#undef NJ_FETCH1
    nj_count_store(ti, tj, ty, tx, n, c, d, comp, diff);
}

}  // namespace

void nj_counts_device(int device, const NjCountArgs &a) {
    use_device(device, NJ_NO_FALLBACK);
    const uint32_t n = a.n, np = (n + NJ_TILE - 1) / NJ_TILE * NJ_TILE;
    const uint64_t tri = (uint64_t)n * (n - 1) / 2;
    uint64_t slice = std::max<uint64_t>(tree_budget_bytes() / n, 1);      // columns of one slice: n x slice raw bytes
    if (slice >= NJ_CHUNK) slice -= slice % NJ_CHUNK;
    slice = std::min<uint64_t>(slice, a.w);
    const uint64_t slice_pad = (slice + NJ_CHUNK - 1) / NJ_CHUNK * NJ_CHUNK;
    hipStream_t s = nullptr;
    DevBuf<uint8_t> d_raw;
    DevBuf<uint32_t> d_E, d_comp, d_diff;
    d_raw.reserve_exact((size_t)n * slice);
    d_E.reserve_exact((size_t)np * (slice_pad / 4));
    d_comp.reserve_exact(tri); d_diff.reserve_exact(tri);
    UC_HIP(hipMemsetAsync(d_comp.p, 0, tri * 4, s));
    UC_HIP(hipMemsetAsync(d_diff.p, 0, tri * 4, s));
    const bool timing = getenv("UC_TIMING") != nullptr;      // the count kernel alone, between two events per slice
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (timing) { UC_HIP(hipEventCreate(&ev0)); UC_HIP(hipEventCreate(&ev1)); }
    double kernel_ms = 0.0;
    uint32_t n_slices = 0;
    for (uint64_t c0 = 0; c0 < a.w; c0 += slice, n_slices++) {
        const uint64_t ws = std::min<uint64_t>(slice, a.w - c0), wq = (ws + NJ_CHUNK - 1) / NJ_CHUNK * NJ_CW;
        UC_HIP(hipMemcpy2D(d_raw.p, ws, a.cells + c0, a.w, ws, n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nj_encode_kernel, grid_for(wq * np), dim3(256), 0, s, (const uint8_t *)d_raw.p, n, ws, np, wq, d_E.p);
        if (timing) UC_HIP(hipEventRecord(ev0, s));
        hipLaunchKernelGGL(nj_count_kernel, dim3(np / NJ_TILE, np / NJ_TILE), dim3(256), 0, s, (const uint32_t *)d_E.p, n, np, (uint32_t)(wq / NJ_CW), d_comp.p, d_diff.p);
        if (timing) UC_HIP(hipEventRecord(ev1, s));
        UC_HIP(hipGetLastError());
        UC_HIP(hipStreamSynchronize(s));      // d_raw is refilled by the next slice
        if (timing) { float ms = 0.f; UC_HIP(hipEventElapsedTime(&ms, ev0, ev1)); kernel_ms += ms; }
    }
    if (timing) {
        (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
        fprintf(stderr, "unicore-cluster[timing]: nj counts: %u rows x %llu columns in %u slice(s): count kernel %.3f ms = %.4g pair-columns/s\n", n, (unsigned long long)a.w,
                n_slices, kernel_ms, kernel_ms > 0.0 ? (double)tri * (double)a.w / (kernel_ms * 1e-3) : 0.0);
    }
    UC_HIP(hipMemcpy(a.comp, d_comp.p, tri * 4, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.diff, d_diff.p, tri * 4, hipMemcpyDeviceToHost));
}

}  // namespace uc
