// uc_nj_join.hip — the join loop of the tree builder `nj` on the device (rule UC-N/J), written once: the main tree is a batch of one
// replicate.
//   consumes  NjJoinBatchArgs: n_rep distance matrices of n x n doubles, each validated by nj_join_validate (finite, >= 0, symmetric, zero
//             diagonal); nj_join_device wraps its single matrix as a batch of one
//   produces  per replicate the n - 3 join records (join_a, join_b, len_a, len_b) and the three root nodes and lengths, integers and fp64 bits equal
//             to nj_join_host's
//   routes    n <= NJ_LDS_ROWS and more than one replicate: nj_join_lds_kernel, one workgroup per replicate, one launch per batch.  D (row stride
//             n | 1 doubles), r, the active flags and the node ids stay in LDS for all n - 3 steps and the root.  Row sums: one thread per active
//             row, ascending k - the order is the rule - reading D by column (D is symmetric), so a wave reads consecutive doubles and no two
//             lanes share a bank; the odd stride keeps the update's column store (k x stride) off one bank, which a stride of 128 doubles would
//             hit 16 ways.
//             otherwise: three launches per step on one stream with the replicate as a grid dimension and per-replicate D, act, node, r,
//             partials, active count and error mark: row sums (one thread per active row, ascending k, D read by column so the wave's loads
//             coalesce), the smallest (Q, i, j) per workgroup, then one workgroup per replicate that reduces the partials, writes the join record,
//             rewrites row and column i and retires slot j.  One host sync per batch.
//             A single tree takes the three launches at every n: one workgroup's latency in the LDS kernel is 10.3 us per step at n = 50 but
//             18.8 us at n = 128, against 15.1 and 15.3 us for the three launches (profiles/nj_join_merge); the LDS kernel pays when its
//             workgroups run side by side.
//   minimum   the smallest (Q, i, j) of a workgroup is a shuffle reduction per wave and four LDS slots, in both routes.
// 256-thread blocks, vector stores, no atomics, no cooperative launch.  fp64 of UC-N/J: every operation is rounded on its own.  hipcc contracts
// a * b + c into an FMA in device code by default; uc_nj.h sets `#pragma clang fp contract(off)` in front of the shared arithmetic and it holds for
// this whole file (it is included first).  Scratch is hipMalloc'ed and freed inside the call; batches are sized against UC_TREE_BUDGET_BYTES.
#include "uc_nj.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "uc_engine.h"

namespace uc {

namespace {

constexpr uint32_t NJ_NONE = 0xffffffffu;
constexpr uint32_t NJ_BATCH_MAX = 32768;            // replicates of a launch (a grid dimension)

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

// the three launches of a step, the replicate as blockIdx.y.  word: [replicate][2] = the active count, the error mark
// r[i] = the sum of d(i, k) over the active k != i, ascending from 0.0.  D[k n + i] = d(i, k): consecutive threads read consecutive doubles
__global__ void __launch_bounds__(256) nj_rowsum_kernel(const double *D, uint32_t n, const uint8_t *act, double *r) {
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

__global__ void __launch_bounds__(256) nj_qmin_kernel(const double *D, uint32_t n, const uint8_t *act, const double *r, const uint32_t *word, double *pq, uint32_t *pi,
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
__global__ void __launch_bounds__(256) nj_join_kernel(double *D, uint32_t n, uint8_t *act, uint32_t *node, const double *r, uint32_t *word, uint32_t n_part, const double *pq,
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
__global__ void __launch_bounds__(256) nj_root_kernel(const double *D, uint32_t n, uint32_t n_rep, const uint8_t *act, const uint32_t *node, uint32_t *root_node,
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

}  // namespace

void nj_join_batch_device(int device, const NjJoinBatchArgs &a) {
    if (a.n == 2) { nj_join_batch_host(a); return; }      // nothing to reduce: both leaves at half their distance
    use_device(device, NJ_NO_FALLBACK);
    const uint32_t n = a.n, steps = n - 3, n_part = std::min<uint32_t>(n, 1024), ld = n | 1;
    const uint64_t nn = (uint64_t)n * n;
    const bool in_lds = n <= NJ_LDS_ROWS && a.n_rep > 1;      // one replicate: see the head comment
    // bytes of a replicate in the three-launch route: D | r, node, act | the partials | the records | roots and word
    const uint64_t per_rep = nn * 8 + (uint64_t)n * 13 + (uint64_t)n_part * 16 + (uint64_t)steps * 24 + 44;
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(a.n_rep, NJ_BATCH_MAX), tree_budget_bytes() / per_rep));
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
        } else {
            UC_HIP(hipMemcpy(d_node.p, node.data(), (size_t)nb * n * 4, hipMemcpyHostToDevice));
            UC_HIP(hipMemsetAsync(d_act.p, 1, (size_t)nb * n, s));
            UC_HIP(hipMemsetAsync(d_r.p, 0, (size_t)nb * n * 8, s));
            for (uint32_t st = 0; st < steps; st++) {
                hipLaunchKernelGGL(nj_rowsum_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, d_r.p);
                hipLaunchKernelGGL(nj_qmin_kernel, dim3(n_part, nb), dim3(256), 0, s, (const double *)d_D.p, n, (const uint8_t *)d_act.p, (const double *)d_r.p,
                                   (const uint32_t *)d_word.p, d_pq.p, d_pi.p, d_pj.p);
                hipLaunchKernelGGL(nj_join_kernel, dim3(nb), dim3(256), 0, s, d_D.p, n, d_act.p, d_node.p, (const double *)d_r.p, d_word.p, n_part, (const double *)d_pq.p,
                                   (const uint32_t *)d_pi.p, (const uint32_t *)d_pj.p, st, d_ja.p, d_jb.p, d_la.p, d_lb.p);
            }
            hipLaunchKernelGGL(nj_root_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, (const double *)d_D.p, n, nb, (const uint8_t *)d_act.p, (const uint32_t *)d_node.p,
                               d_root.p, d_rlen.p, d_word.p);
        }
        UC_HIP(hipGetLastError());
        UC_HIP(hipStreamSynchronize(s));
        UC_HIP(hipMemcpy(word.data(), d_word.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
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

// the main tree: a batch of one replicate
void nj_join_device(int device, const NjJoinArgs &a) {
    nj_join_batch_device(device, NjJoinBatchArgs{a.n, 1, a.D, a.join_a, a.join_b, a.len_a, a.len_b, a.root_node, a.root_len, 1});
}

}  // namespace uc
