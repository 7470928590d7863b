// uc_nj_boot.hip — the replicate counts of bootstrap support for the tree builder `nj` on the device (rule UC-N/B).  The replicate is
// a grid dimension of every kernel here.
//   consumes  NjBootCountArgs: n rows of w bytes, a seed and a range of replicates, validated by nj_boot_counts_validate
//   produces  comp / diff of every row pair of every replicate, [replicate][triangle], equal to nj_boot_counts_host's.  The replicates' joins are
//             uc_nj_join.hip's
//   encode    bytes -> codes, once per call (per source slice), laid out [row tile][column][row of the tile]: the NJ_TILE codes of a column are one
//             64-byte run, and every tile has one more column of zeros behind its last
//   draws     one workgroup per replicate: col(b, t) from (seed, b, t) as uc_nj.h writes it, compacted (ballot + popcount, no atomics) to the draws
//             that fall into the source slice on the device, minus the slice's first column; the list is padded to the chunk with the zero column
//             - code 0 counts nothing, so the count loop keeps no tail - and its length in chunks is stored per replicate.  Counts are sums over
//             draws: their order in the list is free
//   counts    nj_boot_count_kernel, grid (tile pairs on and above the diagonal) x (replicates): uc_nj_device.h's arithmetic (the same calls as
//             nj_count_kernel's) on a *gathered* chunk: the 256 columns staged are 256 draws of the replicate.  The gather packs straight into
//             LDS.  Bytes moved, per replicate and tile pair:
//             both ways read 2 x NJ_TILE x W code bytes; the direct gather reads them as 64-byte runs of the encoded source, which all
//             replicates and tile pairs share (L2 / Infinity Cache for the module's usual 20 - 200 rows: 200 rows x 200k columns are 51 MB); a
//             resampled copy per replicate would add n x W bytes written and n x W x batch bytes resident (2000 x 200k x 100 = 40 GB) to make
//             the same reads contiguous.  A thread takes four draws x four rows: four dword loads (a wave's 16 lanes of one draw read its whole
//             run), a 4 x 4 byte transpose in registers, one 16-byte LDS store in nj_count_kernel's [dword][row] layout.
// 256-thread blocks, vector stores, no atomics, no cooperative launch.  Scratch is hipMalloc'ed and freed inside the call; batches of replicates and
// source slices are sized against UC_TREE_BUDGET_BYTES.
#include "uc_nj.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "uc_engine.h"
#include "uc_nj_device.h"

namespace uc {

namespace {

constexpr uint32_t NJ_RUN = NJ_TILE / 4;            // dwords of a column's run in the encoded source
constexpr uint64_t NJ_SLICE_MAX = 1ull << 24;        // source columns of a slice: a run's byte offset inside a tile stays below 2^32
constexpr uint32_t NJ_BATCH_MAX = 32768;            // replicates of a launch (gridDim.y)
static_assert(NJ_TR == 4 && NJ_TILE == 64 && NJ_CHUNK == 256, "the staging below is written for 64-row tiles and 256-column chunks");

// S: [tile][ws + 1][NJ_RUN] dwords; raw: n x ws bytes.  Consecutive threads take consecutive columns (the reads are the wide side)
__global__ void __launch_bounds__(256) nj_boot_encode_kernel(const uint8_t *raw, uint32_t n, uint64_t ws, uint32_t nt, uint32_t *S) {
    const uint64_t ws1 = ws + 1, total = (uint64_t)nt * NJ_RUN * ws1;
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (uint64_t)gridDim.x * 256) {
        const uint64_t c = x % ws1, tg = x / ws1, g = tg % NJ_RUN, t = tg / NJ_RUN;
        uint32_t v = 0;
        if (c < ws)
            for (uint32_t r = 0; r < 4; r++) {
                const uint64_t row = t * NJ_TILE + g * 4 + r;
                if (row < n) v |= (uint32_t)nj_code(raw[row * ws + c]) << (8 * r);
            }
        S[(t * ws1 + c) * NJ_RUN + g] = v;
    }
}

// cols: [replicate][wpad] (wpad = w rounded up to the chunk); nch: chunks of every replicate's list
__global__ void __launch_bounds__(256) nj_boot_draw_kernel(uint64_t seed, uint32_t rep0, uint64_t w, uint64_t c0, uint64_t ws, uint64_t wpad, uint32_t *cols, uint32_t *nch) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t key = nj_boot_key(seed, rep0 + b);
    uint32_t *out = cols + (uint64_t)b * wpad;
    uint64_t base = 0;
    for (uint64_t t0 = 0; t0 < w; t0 += 256) {
        const uint64_t t = t0 + tid;
        uint64_t c = 0;
        bool in = false;
        if (t < w) { c = nj_boot_col(key, t, w); in = c >= c0 && c < c0 + ws; }
        const uint64_t mask = __ballot(in);
        if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t u = 0; u < 4; u++) { if (u < wv) before += s_cnt[u]; total += s_cnt[u]; }
        if (in) out[base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = (uint32_t)(c - c0);
        base += total;
        __syncthreads();      // s_cnt is written again
    }
    const uint64_t end = (base + NJ_CHUNK - 1) / NJ_CHUNK * NJ_CHUNK;      // <= wpad: base <= w
    for (uint64_t x = base + tid; x < end; x += 256) out[x] = (uint32_t)ws;      // the zero column
    if (tid == 0) nch[b] = (uint32_t)(end / NJ_CHUNK);
}

// d[r]: rows 4 g .. 4 g + 3 of draw r (a byte each).  Returns rows 4 g .. 4 g + 3 as dwords of four draws: nj_count_kernel's LDS cell
__device__ __forceinline__ uint4 nj_transpose(const uint32_t d[4]) {
    uint4 o;
    o.x = (d[0] & 0xffu) | ((d[1] & 0xffu) << 8) | ((d[2] & 0xffu) << 16) | (d[3] << 24);
    o.y = ((d[0] >> 8) & 0xffu) | (d[1] & 0xff00u) | ((d[2] & 0xff00u) << 8) | ((d[3] & 0xff00u) << 16);
    o.z = ((d[0] >> 16) & 0xffu) | ((d[1] >> 8) & 0xff00u) | (d[2] & 0xff0000u) | ((d[3] & 0xff0000u) << 8);
    o.w = (d[0] >> 24) | ((d[1] >> 16) & 0xff00u) | ((d[2] >> 8) & 0xff0000u) | (d[3] & 0xff000000u);
    return o;
}

// chunk k of both row tiles into registers: cell q = tid + 256 u of a tile is rows 4 (q % NJ_RUN) .. + 3 of draws 4 (q / NJ_RUN) .. + 3
__device__ __forceinline__ void nj_boot_fetch(const uint32_t *SA, const uint32_t *SB, const uint32_t *list, uint32_t k, uint32_t tid, uint32_t (&ra)[4][4], uint32_t (&rb)[4][4]) {
    const bool diagonal = SA == SB;      // uniform: a tile against itself (every tree of up to NJ_TILE rows) reads its runs once
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t q = tid + 256 * u, wd = q / NJ_RUN, g = q % NJ_RUN;
        const uint4 c4 = *(const uint4 *)(list + (uint64_t)k * NJ_CHUNK + 4 * wd);
        const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t off = (c[r] * NJ_RUN + g) * 4;      // bytes; a slice has at most NJ_SLICE_MAX columns, so 32 bits hold it: one VGPR per address
            ra[u][r] = *(const uint32_t *)((const char *)SA + off);
            rb[u][r] = diagonal ? ra[u][r] : *(const uint32_t *)((const char *)SB + off);
        }
    }
}

// grid (nt (nt + 1) / 2, replicates).  S: the encoded source slice, ws1 columns per tile (the last is zero); the kernel adds into the triangles
__global__ void __launch_bounds__(256, 2) nj_boot_count_kernel(const uint32_t *S, uint32_t n, uint32_t nt, uint64_t ws1, const uint32_t *cols, uint64_t wpad, const uint32_t *nch,
                                                            uint32_t *comp, uint32_t *diff, uint64_t tri) {
    uint32_t ti = 0, p = blockIdx.x;
    while (p >= nt - ti) { p -= nt - ti; ti++; }      // pair p of the upper triangle of tiles, row-major
    const uint32_t tj = ti + p, b = blockIdx.y;
    __shared__ uint4 sA[NJ_CW * NJ_RUN], sB[NJ_CW * NJ_RUN];
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const uint32_t *SA = S + (uint64_t)ti * ws1 * NJ_RUN, *SB = S + (uint64_t)tj * ws1 * NJ_RUN, *list = cols + (uint64_t)b * wpad;
    const uint32_t n_chunks = nch[b];
    uint32_t c[NJ_TR][NJ_TR], d[NJ_TR][NJ_TR];
#pragma unroll
    for (uint32_t r = 0; r < NJ_TR; r++)
#pragma unroll
        for (uint32_t s = 0; s < NJ_TR; s++) c[r][s] = d[r][s] = 0;
    uint32_t ra[4][4], rb[4][4];
    if (n_chunks) nj_boot_fetch(SA, SB, list, 0, tid, ra, rb);
    for (uint32_t k = 0; k < n_chunks; k++) {
        __syncthreads();      // the chunk before is read
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) { sA[tid + 256 * u] = nj_transpose(ra[u]); sB[tid + 256 * u] = nj_transpose(rb[u]); }
        __syncthreads();
        if (k + 1 < n_chunks) nj_boot_fetch(SA, SB, list, k + 1, tid, ra, rb);
        nj_count_chunk(sA, sB, ty, tx, c, d);
    }
    nj_count_store(ti, tj, ty, tx, n, c, d, comp + (uint64_t)b * tri, diff + (uint64_t)b * tri);
}

}  // namespace

void nj_boot_counts_device(int device, const NjBootCountArgs &a) {
    use_device(device, NJ_NO_FALLBACK);
    const uint32_t n = a.n, nt = (n + NJ_TILE - 1) / NJ_TILE, n_pairs = nt * (nt + 1) / 2;
    const uint64_t w = a.w, tri = (uint64_t)n * (n - 1) / 2, wpad = (w + NJ_CHUNK - 1) / NJ_CHUNK * NJ_CHUNK, budget = tree_budget_bytes();
    const uint64_t slice = std::min<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(budget / n, 1), NJ_SLICE_MAX), w);                                     // source columns on the device at a time
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(a.n_rep, NJ_BATCH_MAX), budget / (wpad * 4 + tri * 8 + 4)));
    const bool one_slice = slice >= w;
    hipStream_t s = nullptr;
    DevBuf<uint8_t> d_raw;
    DevBuf<uint32_t> d_S, d_cols, d_nch, d_comp, d_diff;
    d_raw.reserve_exact((size_t)n * slice);
    d_S.reserve_exact((size_t)nt * (slice + 1) * NJ_RUN);
    d_cols.reserve_exact((size_t)batch * wpad); d_nch.reserve_exact(batch);
    d_comp.reserve_exact((size_t)batch * tri); d_diff.reserve_exact((size_t)batch * tri);
    const bool timing = getenv("UC_TIMING") != nullptr;      // the count kernel alone, between two events per launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (timing) { UC_HIP(hipEventCreate(&ev0)); UC_HIP(hipEventCreate(&ev1)); }
    double kernel_ms = 0.0;
    auto load_slice = [&](uint64_t c0, uint64_t ws) {
        UC_HIP(hipMemcpy2D(d_raw.p, ws, a.cells + c0, w, ws, n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nj_boot_encode_kernel, grid_for((uint64_t)nt * NJ_RUN * (ws + 1)), dim3(256), 0, s, (const uint8_t *)d_raw.p, n, ws, nt, d_S.p);
    };
    if (one_slice) load_slice(0, w);
    uint32_t n_batches = 0, n_slices = 0;
    for (uint32_t b0 = 0; b0 < a.n_rep; b0 += batch, n_batches++) {
        const uint32_t nb = std::min<uint32_t>(batch, a.n_rep - b0);
        UC_HIP(hipMemsetAsync(d_comp.p, 0, (size_t)nb * tri * 4, s));
        UC_HIP(hipMemsetAsync(d_diff.p, 0, (size_t)nb * tri * 4, s));
        n_slices = 0;
        for (uint64_t c0 = 0; c0 < w; c0 += slice, n_slices++) {
            const uint64_t ws = std::min<uint64_t>(slice, w - c0);
            if (!one_slice) load_slice(c0, ws);
            hipLaunchKernelGGL(nj_boot_draw_kernel, dim3(nb), dim3(256), 0, s, a.seed, a.rep0 + b0, w, c0, ws, wpad, d_cols.p, d_nch.p);
            if (timing) UC_HIP(hipEventRecord(ev0, s));
            hipLaunchKernelGGL(nj_boot_count_kernel, dim3(n_pairs, nb), dim3(256), 0, s, (const uint32_t *)d_S.p, n, nt, ws + 1, (const uint32_t *)d_cols.p, wpad,
                               (const uint32_t *)d_nch.p, d_comp.p, d_diff.p, tri);
            if (timing) UC_HIP(hipEventRecord(ev1, s));
            UC_HIP(hipGetLastError());
            if (!one_slice || timing) UC_HIP(hipStreamSynchronize(s));      // d_raw and d_S are refilled by the next slice
            if (timing) { float ms = 0.f; UC_HIP(hipEventElapsedTime(&ms, ev0, ev1)); kernel_ms += ms; }
        }
        UC_HIP(hipMemcpy(a.comp + (uint64_t)b0 * tri, d_comp.p, (size_t)nb * tri * 4, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.diff + (uint64_t)b0 * tri, d_diff.p, (size_t)nb * tri * 4, hipMemcpyDeviceToHost));
    }
    if (timing) {
        (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
        fprintf(stderr, "unicore-cluster[timing]: nj boot counts: %u rows x %llu columns, %u replicates in %u batch(es) of %u slice(s): count kernel %.3f ms = %.4g pair-columns/s\n", n,
                (unsigned long long)w, a.n_rep, n_batches, n_slices, kernel_ms, kernel_ms > 0.0 ? (double)tri * (double)w * a.n_rep / (kernel_ms * 1e-3) : 0.0);
    }
}

}  // namespace uc
