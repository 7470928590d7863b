// uc_nj_device.h — the count arithmetic of rule UC-N/D on the device, shared by nj_count_kernel (uc_nj.hip) and nj_boot_count_kernel
// (uc_nj_boot.hip) and included by those two files alone.  A workgroup of 16 x 16 threads takes an NJ_TILE x NJ_TILE tile of row pairs, a thread 4 x 4
// of them with comp / diff in registers; NJ_CHUNK columns of both row tiles stand in LDS as [dword][row] (a dword is four columns of a row; a thread's
// four rows are one 16-byte read, the wave's reads are 4 resp. 16 distinct addresses).  How a chunk reaches LDS is the kernels' own: contiguous rows
// there, gathered draws here.
#pragma once
#include <hip/hip_runtime.h>

#include "uc_nj.h"

namespace uc {

constexpr uint32_t NJ_TR = NJ_TILE / 16;            // rows of a thread's block of pairs, both ways (16 x 16 threads)
constexpr uint32_t NJ_CW = NJ_CHUNK / 4;            // dwords of a chunk
static_assert(NJ_TR == 4 && NJ_TILE % 4 == 0, "a thread reads its rows as one uint4");
static_assert((NJ_CW * (NJ_TILE / 4)) % 256 == 0, "the staging loop has no tail");

// the non-zero bytes of x, marked in their top bits: codes stay below 0x80, so no byte carries into the next
__device__ __forceinline__ uint32_t nj_nz(uint32_t x) { return (x + 0x7f7f7f7fu) & 0x80808080u; }

// the NJ_CW dwords of a staged chunk: comp += popc(nz(a) & nz(b)), diff += popc(nz(a) & nz(b) & nz(a ^ b)) for the thread's 4 x 4 pairs
__device__ __forceinline__ void nj_count_chunk(const uint4 *sA, const uint4 *sB, uint32_t ty, uint32_t tx, uint32_t (&c)[NJ_TR][NJ_TR], uint32_t (&d)[NJ_TR][NJ_TR]) {
#pragma unroll 2
    for (uint32_t w = 0; w < NJ_CW; w++) {
        const uint4 a4 = sA[w * (NJ_TILE / 4) + ty], b4 = sB[w * (NJ_TILE / 4) + tx];
        const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
        uint32_t na[4], nb[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) { na[r] = nj_nz(a[r]); nb[r] = nj_nz(b[r]); }
#pragma unroll
        for (uint32_t r = 0; r < 4; r++)
#pragma unroll
            for (uint32_t s = 0; s < 4; s++) {
                const uint32_t m = na[r] & nb[s];
                c[r][s] += __popc(m);
                d[r][s] += __popc(m & ((a[r] ^ b[s]) + 0x7f7f7f7fu));
            }
    }
}

// adds the thread's counts of tile pair (ti, tj) into the triangles of n rows: a pair belongs to one thread, so no atomics
__device__ __forceinline__ void nj_count_store(uint32_t ti, uint32_t tj, uint32_t ty, uint32_t tx, uint32_t n, const uint32_t (&c)[NJ_TR][NJ_TR], const uint32_t (&d)[NJ_TR][NJ_TR],
                                               uint32_t *comp, uint32_t *diff) {
#pragma unroll
    for (uint32_t r = 0; r < NJ_TR; r++)
#pragma unroll
        for (uint32_t s = 0; s < NJ_TR; s++) {
            const uint64_t i = (uint64_t)ti * NJ_TILE + ty * NJ_TR + r, j = (uint64_t)tj * NJ_TILE + tx * NJ_TR + s;
            if (i < j && j < n) {
                const uint64_t x = i * n - i * (i + 1) / 2 + (j - i - 1);
                comp[x] += c[r][s]; diff[x] += d[r][s];
            }
        }
}

}  // namespace uc
