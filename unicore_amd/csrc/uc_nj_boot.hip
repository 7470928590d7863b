// uc_nj_boot.hip — the device side of bootstrap support for the tree builder `nj` (rule UC-N/B).  The replicate is a grid dimension
// of every kernel here: a tree of 50 rows no longer means one workgroup and three launches per join step.
//   encode    bytes -> codes, once per call (per source slice), laid out [row tile][column][row of the tile]: the NJ_TILE codes of a column are one
//             64-byte run, and every tile has one more column of zeros behind its last
//   draws     one workgroup per replicate: col(b, t) from (seed, b, t) as uc_nj.h writes it, compacted (ballot + popcount, no atomics) to the draws
//             that fall into the source slice on the device, minus the slice's first column; the list is padded to the chunk with the zero column
//             - code 0 counts nothing, so the count loop keeps no tail - and its length in chunks is stored per replicate.  Counts are sums over
//             draws: their order in the list is free
//   counts    nj_boot_count_kernel, grid (tile pairs on and above the diagonal) x (replicates): nj_count_kernel's arithmetic (nz / popc on four
//             columns per dword, 4 x 4 pairs per thread, NJ_CHUNK columns of both row tiles through LDS at a time) on a *gathered* chunk: the 256
//             columns staged are 256 draws of the replicate.  The gather packs straight into LDS.  Bytes moved, per replicate and tile pair:
//             both ways read 2 x NJ_TILE x W code bytes; the direct gather reads them as 64-byte runs of the encoded source, which all
//             replicates and tile pairs share (L2 / Infinity Cache for the module's usual 20 - 200 rows: 200 rows x 200k columns are 51 MB); a
//             resampled copy per replicate would add n x W bytes written and n x W x batch bytes resident (2000 x 200k x 100 = 40 GB) to make
//             the same reads contiguous.  A thread takes four draws x four rows: four dword loads (a wave's 16 lanes of one draw read its whole
//             run), a 4 x 4 byte transpose in registers, one 16-byte LDS store in nj_count_kernel's [dword][row] layout.
//   joins     n <= NJ_LDS_ROWS: nj_join_lds_kernel, one workgroup per replicate, one launch per batch.  D (row stride n | 1 doubles), r, the
//             active flags and the node ids stay in LDS for all n - 3 steps and the root.  Row sums: one thread per active row, ascending k - the
//             order is the rule - reading D by column (D is symmetric), so a wave reads consecutive doubles and no two lanes share a bank; the odd
//             stride keeps the update's column store (k x stride) off one bank, which a stride of 128 doubles would hit 16 ways.  The (Q, i, j)
//             minimum is a shuffle reduction per wave and four LDS slots.
//             n > NJ_LDS_ROWS: uc_nj.hip's three launches per step with the replicate as blockIdx.y and per-replicate D, act, node, r,
//             partials, active count and error mark; one host sync per batch.
// 256-thread blocks, vector stores, no atomics, no cooperative launch.  fp64 of UC-N/J: uc_nj.h is included first and turns contraction off for
// the whole file.  Scratch is hipMalloc'ed and freed inside the call; batches of replicates and source slices are sized against UC_TREE_BUDGET_BYTES.
#include "uc_nj.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "uc_engine.h"

namespace uc {

namespace {

constexpr uint32_t NJ_TR = NJ_TILE / 16;            // rows of a thread's block of pairs, both ways (16 x 16 threads)
constexpr uint32_t NJ_CW = NJ_CHUNK / 4;            // dwords of a chunk
constexpr uint32_t NJ_RUN = NJ_TILE / 4;            // dwords of a column's run in the encoded source
constexpr uint32_t NJ_NONE = 0xffffffffu;
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

__device__ __forceinline__ uint32_t nj_nz(uint32_t x) { return (x + 0x7f7f7f7fu) & 0x80808080u; }

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
#pragma unroll 2
        for (uint32_t w = 0; w < NJ_CW; w++) {
            const uint4 a4 = sA[w * NJ_RUN + ty], b4 = sB[w * NJ_RUN + tx];
            const uint32_t av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            uint32_t na[4], nb[4];
#pragma unroll
            for (uint32_t r = 0; r < 4; r++) { na[r] = nj_nz(av[r]); nb[r] = nj_nz(bv[r]); }
#pragma unroll
            for (uint32_t r = 0; r < 4; r++)
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) {
                    const uint32_t m = na[r] & nb[s];
                    c[r][s] += __popc(m);
                    d[r][s] += __popc(m & ((av[r] ^ bv[s]) + 0x7f7f7f7fu));
                }
        }
    }
    uint32_t *co = comp + (uint64_t)b * tri, *di = diff + (uint64_t)b * tri;
#pragma unroll
    for (uint32_t r = 0; r < NJ_TR; r++)
#pragma unroll
        for (uint32_t s = 0; s < NJ_TR; s++) {
            const uint64_t i = (uint64_t)ti * NJ_TILE + ty * NJ_TR + r, j = (uint64_t)tj * NJ_TILE + tx * NJ_TR + s;
            if (i < j && j < n) {
                const uint64_t x = i * n - i * (i + 1) / 2 + (j - i - 1);
                co[x] += c[r][s]; di[x] += d[r][s];
            }
        }
}

// ---- joins
struct NjKey { double q; uint32_t i, j; };
__device__ __forceinline__ bool nj_less(double q, uint32_t i, uint32_t j, const NjKey &b) {
    return b.i == NJ_NONE || (i != NJ_NONE && (q < b.q || (q == b.q && (i < b.i || (i == b.i && j < b.j)))));
}
// the smallest key of the wave in every lane: the order is total on the keys that name a pair, so the butterfly agrees
__device__ __forceinline__ NjKey nj_wave_min(NjKey k) {
    for (int o = 32; o > 0; o >>= 1) {
        const double q = __shfl_xor(k.q, o);
        const uint32_t i = __shfl_xor(k.i, o), j = __shfl_xor(k.j, o);
        if (nj_less(q, i, j, k)) k = NjKey{q, i, j};
    }
    return k;
}

// LDS of a workgroup: D [n][ld] | r [n] | wave keys q [4] | i [4] | j [4] | node [n] | act [n]
__host__ __device__ inline size_t nj_lds_bytes(uint32_t n, uint32_t ld) { return ((size_t)n * ld + n + 4) * 8 + (8 + (size_t)n) * 4 + n; }

// one workgroup per replicate; Dg [replicate][n][n]; records [replicate][n - 3], roots [replicate][3]; word [replicate][2]: the error mark is the second
__global__ void __launch_bounds__(256) nj_join_lds_kernel(const double *Dg, uint32_t n, uint32_t ld, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b,
                                                          uint32_t *root_node, double *root_len, uint32_t *word) {
    extern __shared__ double nj_lds[];
    double *D = nj_lds, *r = D + (size_t)n * ld, *s_q = r + n;
    uint32_t *s_i = (uint32_t *)(s_q + 4), *s_j = s_i + 4, *node = s_j + 4;
    uint8_t *act = (uint8_t *)(node + n);
    const uint32_t b = blockIdx.x, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, steps = n - 3;
    const double *src = Dg + (uint64_t)b * n * n;
    for (uint32_t x = tid; x < n * n; x += 256) D[(x / n) * ld + x % n] = src[x];
    if (tid < n) { node[tid] = tid; act[tid] = 1; r[tid] = 0.0; }
    __syncthreads();
    uint32_t m = n;
    for (uint32_t s = 0; s < steps; s++, m--) {
        if (tid < n && act[tid]) {      // ascending k from 0.0; D[k][tid] = d(tid, k)
            double sum = 0.0;
            for (uint32_t k = 0; k < n; k++)
                if (act[k] && k != tid) sum += D[k * ld + tid];
            r[tid] = sum;
        }
        __syncthreads();
        NjKey best{0.0, NJ_NONE, NJ_NONE};
        for (uint32_t i = ty; i < n; i += 16) {
            if (!act[i]) continue;
            const double ri = r[i];
            for (uint32_t j = i + 1 + tx; j < n; j += 16) {
                if (!act[j]) continue;
                const double q = nj_q(m, D[i * ld + j], ri, r[j]);
                if (nj_less(q, i, j, best)) best = NjKey{q, i, j};
            }
        }
        best = nj_wave_min(best);
        if ((tid & 63) == 0) { s_q[tid >> 6] = best.q; s_i[tid >> 6] = best.i; s_j[tid >> 6] = best.j; }
        __syncthreads();
        best = NjKey{s_q[0], s_i[0], s_j[0]};
        for (uint32_t u = 1; u < 4; u++)
            if (nj_less(s_q[u], s_i[u], s_j[u], best)) best = NjKey{s_q[u], s_i[u], s_j[u]};
        const uint32_t i = best.i, j = best.j;
        if (i >= n || j >= n || i >= j) { if (tid == 0) word[2 * b + 1] = 1; return; }      // uniform: every thread holds the same key
        const double dij = D[i * ld + j];
        if (tid == 0) {
            double li, lj;
            nj_branch(m, dij, r[i], r[j], li, lj);
            const uint64_t o = (uint64_t)b * steps + s;
            join_a[o] = node[i]; join_b[o] = node[j];
            len_a[o] = li; len_b[o] = lj;
        }
        if (tid < n && act[tid] && tid != i && tid != j) {
            const double v = nj_new(D[i * ld + tid], D[j * ld + tid], dij);
            D[i * ld + tid] = v;
            D[tid * ld + i] = v;
        }
        __syncthreads();      // node[i], act[j], r and the wave keys are read above
        if (tid == 0) { node[i] = n + s; act[j] = 0; }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t x[3], c = 0;
        for (uint32_t i = 0; i < n; i++)
            if (act[i]) { if (c < 3) x[c] = i; c++; }
        if (c != 3) { word[2 * b + 1] = 2; return; }
        for (int t = 0; t < 3; t++) root_node[(uint64_t)b * 3 + t] = node[x[t]];
        nj_root3(D[x[0] * ld + x[1]], D[x[0] * ld + x[2]], D[x[1] * ld + x[2]], root_len + (uint64_t)b * 3);
    }
}

// the three launches of uc_nj.hip's step with the replicate as blockIdx.y.  word: [replicate][2] = the active count, the error mark
__global__ void __launch_bounds__(256) nj_boot_rowsum_kernel(const double *D, uint32_t n, const uint8_t *act, double *r) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    D += (uint64_t)b * n * n; act += (uint64_t)b * n; r += (uint64_t)b * n;
    if (i >= n || !act[i]) return;
    double sum = 0.0;
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) {      // eight loads in flight, added in order
        double v[8];
        for (uint32_t u = 0; u < 8; u++) v[u] = D[(uint64_t)(k + u) * n + i];
        for (uint32_t u = 0; u < 8; u++) if (act[k + u] && k + u != i) sum += v[u];
    }
    for (; k < n; k++) if (act[k] && k != i) sum += D[(uint64_t)k * n + i];
    r[i] = sum;
}

// the smallest key of the workgroup in every thread
__device__ __forceinline__ NjKey nj_block_min(NjKey k) {
    __shared__ double s_q[4];
    __shared__ uint32_t s_i[4], s_j[4];
    k = nj_wave_min(k);
    if ((threadIdx.x & 63) == 0) { s_q[threadIdx.x >> 6] = k.q; s_i[threadIdx.x >> 6] = k.i; s_j[threadIdx.x >> 6] = k.j; }
    __syncthreads();
    k = NjKey{s_q[0], s_i[0], s_j[0]};
    for (uint32_t u = 1; u < 4; u++)
        if (nj_less(s_q[u], s_i[u], s_j[u], k)) k = NjKey{s_q[u], s_i[u], s_j[u]};
    return k;
}

__global__ void __launch_bounds__(256) nj_boot_qmin_kernel(const double *D, uint32_t n, const uint8_t *act, const double *r, const uint32_t *word, double *pq, uint32_t *pi,
                                                           uint32_t *pj) {
    const uint32_t b = blockIdx.y, n_part = gridDim.x;
    D += (uint64_t)b * n * n; act += (uint64_t)b * n; r += (uint64_t)b * n;
    const uint32_t m = word[2 * b];
    NjKey best{0.0, NJ_NONE, NJ_NONE};
    for (uint32_t i = blockIdx.x; i < n; i += n_part) {
        if (!act[i]) continue;      // uniform over the workgroup
        const double ri = r[i];
        for (uint32_t j = i + 1 + threadIdx.x; j < n; j += 256) {
            if (!act[j]) continue;
            const double q = nj_q(m, D[(uint64_t)i * n + j], ri, r[j]);
            if (nj_less(q, i, j, best)) best = NjKey{q, i, j};
        }
    }
    best = nj_block_min(best);
    const uint64_t o = (uint64_t)b * n_part + blockIdx.x;
    if (threadIdx.x == 0) { pq[o] = best.q; pi[o] = best.i; pj[o] = best.j; }
}

// one workgroup per replicate.  A replicate whose error mark is set skips its steps: nothing is indexed with a key that names no pair
__global__ void __launch_bounds__(256) nj_boot_join_kernel(double *D, uint32_t n, uint8_t *act, uint32_t *node, const double *r, uint32_t *word, uint32_t n_part, const double *pq,
                                                           const uint32_t *pi, const uint32_t *pj, uint32_t step, uint32_t *join_a, uint32_t *join_b, double *len_a,
                                                           double *len_b) {
    const uint32_t b = blockIdx.x, steps = n - 3;
    D += (uint64_t)b * n * n; act += (uint64_t)b * n; node += (uint64_t)b * n; r += (uint64_t)b * n; word += 2 * (uint64_t)b;
    pq += (uint64_t)b * n_part; pi += (uint64_t)b * n_part; pj += (uint64_t)b * n_part;
    if (word[1]) return;      // uniform
    NjKey best{0.0, NJ_NONE, NJ_NONE};
    for (uint32_t p = threadIdx.x; p < n_part; p += 256)
        if (nj_less(pq[p], pi[p], pj[p], best)) best = NjKey{pq[p], pi[p], pj[p]};
    best = nj_block_min(best);
    const uint32_t i = best.i, j = best.j;
    if (i >= n || j >= n || i >= j) { if (threadIdx.x == 0) word[1] = 1; return; }      // uniform: every thread holds the same key
    const uint32_t m = word[0];
    const double dij = D[(uint64_t)i * n + j];
    if (threadIdx.x == 0) {
        double li, lj;
        nj_branch(m, dij, r[i], r[j], li, lj);
        const uint64_t o = (uint64_t)b * steps + step;
        join_a[o] = node[i]; join_b[o] = node[j];
        len_a[o] = li; len_b[o] = lj;
    }
    for (uint32_t k = threadIdx.x; k < n; k += 256) {
        if (!act[k] || k == i || k == j) continue;
        const double v = nj_new(D[(uint64_t)i * n + k], D[(uint64_t)j * n + k], dij);
        D[(uint64_t)i * n + k] = v;
        D[(uint64_t)k * n + i] = v;
    }
    __syncthreads();      // node[i], act[j] and the count are read above
    if (threadIdx.x == 0) { node[i] = n + step; act[j] = 0; word[0] = m - 1; }
}

// one thread per replicate
__global__ void __launch_bounds__(256) nj_boot_root_kernel(const double *D, uint32_t n, uint32_t n_rep, const uint8_t *act, const uint32_t *node, uint32_t *root_node,
                                                           double *root_len, uint32_t *word) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_rep || word[2 * (uint64_t)b + 1]) return;
    D += (uint64_t)b * n * n; act += (uint64_t)b * n; node += (uint64_t)b * n;
    uint32_t x[3], c = 0;
    for (uint32_t i = 0; i < n; i++)
        if (act[i]) { if (c < 3) x[c] = i; c++; }
    if (c != 3) { word[2 * (uint64_t)b + 1] = 2; return; }
    for (int t = 0; t < 3; t++) root_node[(uint64_t)b * 3 + t] = node[x[t]];
    nj_root3(D[(uint64_t)x[0] * n + x[1]], D[(uint64_t)x[0] * n + x[2]], D[(uint64_t)x[1] * n + x[2]], root_len + (uint64_t)b * 3);
}

void nj_boot_use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(UC_ERR_DEVICE, "no HIP device available; the device side of nj has no CPU fallback (the host twins are separate entry points)");
    if (device < 0) UC_HIP(hipGetDevice(&device));
    if (device >= ndev) fail(UC_ERR_DEVICE, "device %d requested but only %d visible", device, ndev);
    UC_HIP(hipSetDevice(device));
}

}  // namespace

void nj_boot_counts_device(int device, const NjBootCountArgs &a) {
    nj_boot_use_device(device);
    const uint32_t n = a.n, nt = (n + NJ_TILE - 1) / NJ_TILE, n_pairs = nt * (nt + 1) / 2;
    const uint64_t w = a.w, tri = (uint64_t)n * (n - 1) / 2, wpad = (w + NJ_CHUNK - 1) / NJ_CHUNK * NJ_CHUNK, budget = nj_tree_budget();
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

void nj_join_batch_device(int device, const NjJoinBatchArgs &a) {
    if (a.n == 2) { nj_join_batch_host(a); return; }      // nothing to reduce: both leaves at half their distance
    nj_boot_use_device(device);
    const uint32_t n = a.n, steps = n - 3, n_part = std::min<uint32_t>(n, 1024), ld = n | 1;
    const uint64_t nn = (uint64_t)n * n;
    const bool in_lds = n <= NJ_LDS_ROWS;
    const uint64_t per_rep = nn * 8 + (uint64_t)n * 13 + (uint64_t)n_part * 16 + (uint64_t)steps * 24 + 44;
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(a.n_rep, NJ_BATCH_MAX), nj_tree_budget() / per_rep));
    hipStream_t s = nullptr;
    DevBuf<double> d_D, d_r, d_pq, d_la, d_lb, d_rlen;
    DevBuf<uint32_t> d_node, d_pi, d_pj, d_ja, d_jb, d_root, d_word;
    DevBuf<uint8_t> d_act;
    const size_t rec = std::max<size_t>((size_t)batch * steps, 1);
    d_D.reserve_exact((size_t)batch * nn);
    d_la.reserve_exact(rec); d_lb.reserve_exact(rec); d_ja.reserve_exact(rec); d_jb.reserve_exact(rec);
    d_rlen.reserve_exact((size_t)batch * 3); d_root.reserve_exact((size_t)batch * 3); d_word.reserve_exact((size_t)batch * 2);
    std::vector<uint32_t> node, word((size_t)batch * 2);
    if (in_lds) UC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nj_join_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)nj_lds_bytes(n, ld)));
    else {
        d_r.reserve_exact((size_t)batch * n); d_node.reserve_exact((size_t)batch * n); d_act.reserve_exact((size_t)batch * n);
        d_pq.reserve_exact((size_t)batch * n_part); d_pi.reserve_exact((size_t)batch * n_part); d_pj.reserve_exact((size_t)batch * n_part);
        node.resize((size_t)batch * n);
        for (size_t x = 0; x < node.size(); x++) node[x] = (uint32_t)(x % n);
    }
    for (uint32_t b0 = 0; b0 < a.n_rep; b0 += batch) {
        const uint32_t nb = std::min<uint32_t>(batch, a.n_rep - b0);
        UC_HIP(hipMemcpy(d_D.p, a.D + (uint64_t)b0 * nn, (size_t)nb * nn * 8, hipMemcpyHostToDevice));
        for (uint32_t b = 0; b < nb; b++) { word[2 * b] = n; word[2 * b + 1] = 0; }
        UC_HIP(hipMemcpy(d_word.p, word.data(), (size_t)nb * 8, hipMemcpyHostToDevice));
        if (in_lds) {      // the active count lives in a register there: the kernel takes the error marks alone, behind the counts
            hipLaunchKernelGGL(nj_join_lds_kernel, dim3(nb), dim3(256), nj_lds_bytes(n, ld), s, (const double *)d_D.p, n, ld, d_ja.p, d_jb.p, d_la.p, d_lb.p, d_root.p, d_rlen.p,
                               d_word.p);
            UC_HIP(hipGetLastError());
            UC_HIP(hipStreamSynchronize(s));
            UC_HIP(hipMemcpy(word.data(), d_word.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
        } else {
            UC_HIP(hipMemcpy(d_node.p, node.data(), (size_t)nb * n * 4, hipMemcpyHostToDevice));
            UC_HIP(hipMemsetAsync(d_act.p, 1, (size_t)nb * n, s));
            UC_HIP(hipMemsetAsync(d_r.p, 0, (size_t)nb * n * 8, s));
            for (uint32_t st = 0; st < steps; st++) {
                hipLaunchKernelGGL(nj_boot_rowsum_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, d_r.p);
                hipLaunchKernelGGL(nj_boot_qmin_kernel, dim3(n_part, nb), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, (const double *)d_r.p,
                                   (const uint32_t *)d_word.p, d_pq.p, d_pi.p, d_pj.p);
                hipLaunchKernelGGL(nj_boot_join_kernel, dim3(nb), dim3(256), 0, s, d_D.p, n, d_act.p, d_node.p, (const double *)d_r.p, d_word.p, n_part, (const double *)d_pq.p,
                                   (const uint32_t *)d_pi.p, (const uint32_t *)d_pj.p, st, d_ja.p, d_jb.p, d_la.p, d_lb.p);
            }
            hipLaunchKernelGGL(nj_boot_root_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, (const double *)d_D.p, n, nb, (const uint8_t *)d_act.p, (const uint32_t *)d_node.p,
                               d_root.p, d_rlen.p, d_word.p);
            UC_HIP(hipGetLastError());
            UC_HIP(hipStreamSynchronize(s));
            UC_HIP(hipMemcpy(word.data(), d_word.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
        }
        for (uint32_t b = 0; b < nb; b++)
            if (word[2 * b + 1]) fail(UC_ERR_GENERIC, "nj: the join loop of replicate %u found no pair to join (mark %u)", b0 + b, word[2 * b + 1]);
        if (steps) {
            UC_HIP(hipMemcpy(a.join_a + (uint64_t)b0 * steps, d_ja.p, (size_t)nb * steps * 4, hipMemcpyDeviceToHost));
            UC_HIP(hipMemcpy(a.join_b + (uint64_t)b0 * steps, d_jb.p, (size_t)nb * steps * 4, hipMemcpyDeviceToHost));
            UC_HIP(hipMemcpy(a.len_a + (uint64_t)b0 * steps, d_la.p, (size_t)nb * steps * 8, hipMemcpyDeviceToHost));
            UC_HIP(hipMemcpy(a.len_b + (uint64_t)b0 * steps, d_lb.p, (size_t)nb * steps * 8, hipMemcpyDeviceToHost));
        }
        UC_HIP(hipMemcpy(a.root_node + (uint64_t)b0 * 3, d_root.p, (size_t)nb * 12, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.root_len + (uint64_t)b0 * 3, d_rlen.p, (size_t)nb * 24, hipMemcpyDeviceToHost));
    }
}

}  // namespace uc
