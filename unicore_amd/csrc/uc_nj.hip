// uc_nj.hip — the device side of the tree builder `nj` (rule UC-N).
//   encode    bytes -> codes (0 = uninformative, 1 .. 26 = letters), four columns per dword, laid out [dword][row] with the rows padded to the tile
//             and the dwords to the LDS chunk: padding is code 0 and counts nothing, so no loop below has a tail
//   counts    one workgroup per NJ_TILE x NJ_TILE tile of row pairs (upper triangle of tiles), one thread per 4 x 4 pairs with comp / diff in
//             registers; NJ_CHUNK columns of both row tiles go through LDS at a time ([dword][row]: a thread's four rows are one 16-byte read, the
//             wave's reads are 4 resp. 16 distinct addresses).  nz(x) = (x + 0x7f7f7f7f) & 0x80808080 marks the non-zero bytes (codes stay below
//             0x80: no carry between bytes); comp += popc(nz(a) & nz(b)), diff += popc(nz(a) & nz(b) & nz(a ^ b)).  A pair belongs to one thread:
//             no atomics; a call beyond the byte budget runs slice after slice of columns on one stream and the kernel adds into the triangles
//   joins     three launches per step on one stream, one host sync at the end: row sums (one thread per active row, ascending k, D read by
//             column - D is symmetric - so the wave's loads coalesce), the smallest (Q, i, j) per workgroup, then one workgroup that reduces
//             the partials, writes the join record, rewrites row and column i and retires slot j.  The active count lives in device memory.
// fp64 of UC-N/J: every operation is rounded on its own.  hipcc contracts a * b + c into an FMA in device code by default; uc_nj.h sets
// `#pragma clang fp contract(off)` in front of the shared arithmetic and it holds for this whole file (it is included first).  The host build has no
// -march and so forms none either: both sides give the same bits.
// Scratch is hipMalloc'ed and freed inside the call, as in uc_msa.hip.
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
constexpr uint32_t NJ_NONE = 0xffffffffu;
static_assert(NJ_TR == 4 && NJ_TILE % 4 == 0, "a thread reads its rows as one uint4");
static_assert((NJ_CW * (NJ_TILE / 4)) % 256 == 0, "the staging loop has no tail");

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

__device__ __forceinline__ uint32_t nj_nz(uint32_t x) { return (x + 0x7f7f7f7fu) & 0x80808080u; }

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
#pragma unroll 2
        for (uint32_t w = 0; w < NJ_CW; w++) {
            const uint4 a4 = sA[w * Q + ty], b4 = sB[w * Q + tx];
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
#undef NJ_FETCH
#undef NJ_FETCH1
    for (uint32_t r = 0; r < NJ_TR; r++)
        for (uint32_t s = 0; s < NJ_TR; s++) {
            const uint64_t i = (uint64_t)ti * NJ_TILE + ty * NJ_TR + r, j = (uint64_t)tj * NJ_TILE + tx * NJ_TR + s;
            if (i < j && j < n) {
                const uint64_t x = i * n - i * (i + 1) / 2 + (j - i - 1);
                comp[x] += c[r][s]; diff[x] += d[r][s];
            }
        }
}

// r[i] = the sum of d(i, k) over the active k != i, ascending from 0.0.  D[k n + i] = d(i, k): consecutive threads read consecutive doubles
__global__ void __launch_bounds__(256) nj_rowsum_kernel(const double *D, uint32_t n, const uint8_t *act, double *r) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
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

struct NjKey { double q; uint32_t i, j; };
__device__ __forceinline__ bool nj_less(double q, uint32_t i, uint32_t j, const NjKey &b) {
    return b.i == NJ_NONE || (i != NJ_NONE && (q < b.q || (q == b.q && (i < b.i || (i == b.i && j < b.j)))));
}
// the smallest key of the workgroup, returned to every thread (one call per kernel: the arrays are one LDS allocation)
__device__ __forceinline__ NjKey nj_block_min(NjKey k) {
    __shared__ double s_q[256];
    __shared__ uint32_t s_i[256], s_j[256];
    s_q[threadIdx.x] = k.q; s_i[threadIdx.x] = k.i; s_j[threadIdx.x] = k.j;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const NjKey mine{s_q[threadIdx.x], s_i[threadIdx.x], s_j[threadIdx.x]};
            const uint32_t t = threadIdx.x + o;
            if (nj_less(s_q[t], s_i[t], s_j[t], mine)) { s_q[threadIdx.x] = s_q[t]; s_i[threadIdx.x] = s_i[t]; s_j[threadIdx.x] = s_j[t]; }
        }
        __syncthreads();
    }
    return NjKey{s_q[0], s_i[0], s_j[0]};
}

__global__ void __launch_bounds__(256) nj_qmin_kernel(const double *D, uint32_t n, const uint8_t *act, const double *r, const uint32_t *n_act, double *pq, uint32_t *pi,
                                                      uint32_t *pj) {
    const uint32_t m = *n_act;
    NjKey best{0.0, NJ_NONE, NJ_NONE};
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        if (!act[i]) continue;      // uniform over the workgroup
        const double ri = r[i];
        for (uint32_t j = i + 1 + threadIdx.x; j < n; j += 256) {
            if (!act[j]) continue;
            const double q = nj_q(m, D[(uint64_t)i * n + j], ri, r[j]);
            if (nj_less(q, i, j, best)) best = NjKey{q, i, j};
        }
    }
    best = nj_block_min(best);
    if (threadIdx.x == 0) { pq[blockIdx.x] = best.q; pi[blockIdx.x] = best.i; pj[blockIdx.x] = best.j; }
}

// one workgroup.  err: set when no pair is found (the step is then skipped: nothing is indexed with it)
__global__ void __launch_bounds__(256) nj_join_kernel(double *D, uint32_t n, uint8_t *act, uint32_t *node, const double *r, uint32_t *n_act, uint32_t n_part, const double *pq,
                                                      const uint32_t *pi, const uint32_t *pj, uint32_t step, uint32_t *join_a, uint32_t *join_b, double *len_a,
                                                      double *len_b, uint32_t *err) {
    NjKey best{0.0, NJ_NONE, NJ_NONE};
    for (uint32_t p = threadIdx.x; p < n_part; p += 256)
        if (nj_less(pq[p], pi[p], pj[p], best)) best = NjKey{pq[p], pi[p], pj[p]};
    best = nj_block_min(best);
    const uint32_t i = best.i, j = best.j;
    if (i >= n || j >= n || i >= j) { if (threadIdx.x == 0) *err = 1; return; }      // uniform: every thread holds the same key
    const uint32_t m = *n_act;
    const double dij = D[(uint64_t)i * n + j];
    if (threadIdx.x == 0) {
        double li, lj;
        nj_branch(m, dij, r[i], r[j], li, lj);
        join_a[step] = node[i]; join_b[step] = node[j];
        len_a[step] = li; len_b[step] = lj;
    }
    for (uint32_t k = threadIdx.x; k < n; k += 256) {
        if (!act[k] || k == i || k == j) continue;
        const double v = nj_new(D[(uint64_t)i * n + k], D[(uint64_t)j * n + k], dij);
        D[(uint64_t)i * n + k] = v;
        D[(uint64_t)k * n + i] = v;
    }
    __syncthreads();      // node[i], act[j] and the count are read above
    if (threadIdx.x == 0) { node[i] = n + step; act[j] = 0; *n_act = m - 1; }
}

__global__ void nj_root_kernel(const double *D, uint32_t n, const uint8_t *act, const uint32_t *node, uint32_t *root_node, double *root_len, uint32_t *err) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t x[3], c = 0;
    for (uint32_t i = 0; i < n; i++)
        if (act[i]) { if (c < 3) x[c] = i; c++; }
    if (c != 3) { *err = 2; return; }
    for (int t = 0; t < 3; t++) root_node[t] = node[x[t]];
    nj_root3(D[(uint64_t)x[0] * n + x[1]], D[(uint64_t)x[0] * n + x[2]], D[(uint64_t)x[1] * n + x[2]], root_len);
}

void nj_use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(UC_ERR_DEVICE, "no HIP device available; the device side of nj has no CPU fallback (the host twins are separate entry points)");
    if (device < 0) UC_HIP(hipGetDevice(&device));
    if (device >= ndev) fail(UC_ERR_DEVICE, "device %d requested but only %d visible", device, ndev);
    UC_HIP(hipSetDevice(device));
}

}  // namespace

void nj_counts_device(int device, const NjCountArgs &a) {
    nj_use_device(device);
    const uint32_t n = a.n, np = (n + NJ_TILE - 1) / NJ_TILE * NJ_TILE;
    const uint64_t tri = (uint64_t)n * (n - 1) / 2;
    uint64_t budget = 512ull << 20;
    if (const char *b = getenv("UC_TREE_BUDGET_BYTES")) budget = std::max<uint64_t>(strtoull(b, nullptr, 10), 1);
    uint64_t slice = std::max<uint64_t>(budget / n, 1);      // columns of one slice: n x slice raw bytes
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

void nj_join_device(int device, const NjJoinArgs &a) {
    if (a.n == 2) { nj_join_host(a); return; }      // nothing to reduce: both leaves at half their distance
    nj_use_device(device);
    const uint32_t n = a.n, steps = n - 3, n_part = std::min<uint32_t>(n, 1024);
    hipStream_t s = nullptr;
    DevBuf<double> d_D, d_r, d_pq, d_la, d_lb, d_rlen;
    DevBuf<uint32_t> d_node, d_pi, d_pj, d_ja, d_jb, d_root, d_word;      // d_word: [0] the active count, [1] the error mark
    DevBuf<uint8_t> d_act;
    d_D.reserve_exact((size_t)n * n); d_r.reserve_exact(n); d_pq.reserve_exact(n_part); d_pi.reserve_exact(n_part); d_pj.reserve_exact(n_part);
    d_la.reserve_exact(std::max<uint32_t>(steps, 1)); d_lb.reserve_exact(std::max<uint32_t>(steps, 1));
    d_ja.reserve_exact(std::max<uint32_t>(steps, 1)); d_jb.reserve_exact(std::max<uint32_t>(steps, 1));
    d_rlen.reserve_exact(3); d_root.reserve_exact(3); d_node.reserve_exact(n); d_word.reserve_exact(2); d_act.reserve_exact(n);
    std::vector<uint32_t> node(n);
    for (uint32_t i = 0; i < n; i++) node[i] = i;
    const uint32_t word[2] = {n, 0};
    UC_HIP(hipMemcpy(d_D.p, a.D, (size_t)n * n * 8, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_node.p, node.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_word.p, word, 8, hipMemcpyHostToDevice));
    UC_HIP(hipMemsetAsync(d_act.p, 1, n, s));
    UC_HIP(hipMemsetAsync(d_r.p, 0, (size_t)n * 8, s));
    for (uint32_t st = 0; st < steps; st++) {
        hipLaunchKernelGGL(nj_rowsum_kernel, grid_for(n), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, d_r.p);
        hipLaunchKernelGGL(nj_qmin_kernel, dim3(n_part), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, (const double *)d_r.p,
                           (const uint32_t *)d_word.p, d_pq.p, d_pi.p, d_pj.p);
        hipLaunchKernelGGL(nj_join_kernel, dim3(1), dim3(256), 0, s, d_D.p, n, d_act.p, d_node.p, (const double *)d_r.p, d_word.p, n_part, (const double *)d_pq.p,
                           (const uint32_t *)d_pi.p, (const uint32_t *)d_pj.p, st, d_ja.p, d_jb.p, d_la.p, d_lb.p, d_word.p + 1);
    }
    hipLaunchKernelGGL(nj_root_kernel, dim3(1), dim3(64), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, (const uint32_t *)d_node.p, d_root.p, d_rlen.p,
                       d_word.p + 1);
    UC_HIP(hipGetLastError());
    UC_HIP(hipStreamSynchronize(s));
    uint32_t back[2];
    UC_HIP(hipMemcpy(back, d_word.p, 8, hipMemcpyDeviceToHost));
    if (back[1]) fail(UC_ERR_GENERIC, "nj: the join loop found no pair to join (mark %u, %u slots left)", back[1], back[0]);
    if (steps) {
        UC_HIP(hipMemcpy(a.join_a, d_ja.p, (size_t)steps * 4, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.join_b, d_jb.p, (size_t)steps * 4, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.len_a, d_la.p, (size_t)steps * 8, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.len_b, d_lb.p, (size_t)steps * 8, hipMemcpyDeviceToHost));
    }
    UC_HIP(hipMemcpy(a.root_node, d_root.p, 12, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.root_len, d_rlen.p, 24, hipMemcpyDeviceToHost));
}

}  // namespace uc
