// uc_nj_transfer.hip — the device side of transfer bootstrap support for the tree builder `nj` (rule UC-N/T).
//   sets      the leaf sets of every join of the main tree and of a batch of replicates, as bit sets of 32-bit words, from the join records in
//             one launch.  One thread per (tree, word): it walks the tree in join order, row(n + s) = row(a) | row(b), a child below n is a
//             single bit.  A word of a row depends on the same word of earlier rows alone, so a thread reads what it wrote itself: no barrier.
//             A tree is laid out [word][split], the splits padded to the tile and the words to the chunk; padding is zero (the buffer is
//             cleared once) and bits at positions >= n are never set.  Not hot: n - 3 dependent steps per thread
//   compare   nj_transfer_kernel, grid (tiles of NJ_T_TILE main splits) x (replicates).  A workgroup loops over all split tiles of its
//             replicate, so the minimum never leaves it.  nj_count_kernel's shape: a thread owns 4 x 4 (main split, replicate split) pairs
//             and 16 Hamming accumulators; NJ_T_CHUNK words of both tiles go through LDS at a time, [word][split]: a thread's four splits
//             are one 16-byte read, a wave reads 4 resp. 16 distinct cells (the 16 are one 256-byte row: no two lanes of a read group share a
//             bank); the next chunk's loads are issued before the current chunk is counted.  Per pair and word: one XOR, one popcount-add.
//             After the last word delta = min(h, n - h) goes into a running minimum per main split, *unless the replicate split is a padded
//             row of a partial tile*: an all-zero row has h = |L_s|, which can undercut every true distance.  The minimum is reduced over
//             the 16 lanes that share the main split (shuffles), capped at light - 1 and stored once.  A tree of up to 32 NJ_T_CHUNK leaves
//             has one chunk: the main tile then stays in LDS for the whole loop.
// 256-thread blocks, vector stores, no atomics, no cooperative launch, no scratch.  Scratch memory is hipMalloc'ed and freed inside the call;
// batches of replicates are sized against UC_TREE_BUDGET_BYTES.
#include "uc_nj.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "uc_engine.h"

namespace uc {

namespace {

constexpr uint32_t T_Q = NJ_T_TILE / 4;              // 16-byte cells of a word's row of a tile
constexpr uint32_t T_BATCH_MAX = 32768;              // replicates of a launch (gridDim.y)
static_assert(NJ_T_TILE == 64 && NJ_T_CHUNK * T_Q == 256, "a thread stages one cell of either tile per chunk and owns 4 x 4 pairs");

// ja / jb: [trees][n - 3]; bits: [trees][wp][sp] dwords; trees t0 .. t0 + n_trees - 1
__global__ void __launch_bounds__(256) nj_transfer_sets_kernel(const uint32_t *ja, const uint32_t *jb, uint32_t n, uint32_t words, uint32_t sp, uint64_t stride, uint32_t t0,
                                                               uint32_t n_trees, uint32_t *bits) {
    const uint32_t steps = n - 3;
    const uint64_t total = (uint64_t)n_trees * words;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        const uint32_t t = t0 + (uint32_t)(g / words), x = (uint32_t)(g % words);
        const uint32_t *a = ja + (uint64_t)t * steps, *b = jb + (uint64_t)t * steps;
        uint32_t *row = bits + (uint64_t)t * stride + (uint64_t)x * sp;
        for (uint32_t s = 0; s < steps; s++) {      // the host has checked the records: a child of step s is below n + s
            const uint32_t ca = a[s], cb = b[s];
            const uint32_t va = ca < n ? ((ca >> 5) == x ? 1u << (ca & 31) : 0u) : row[ca - n];
            const uint32_t vb = cb < n ? ((cb >> 5) == x ? 1u << (cb & 31) : 0u) : row[cb - n];
            row[s] = va | vb;
        }
    }
}

// h += popcount(x) as the one instruction it is.  Written as h += __popc(x), two words of an unrolled loop become two counts from zero and a
// three-way add: 2.5 VALU instructions per pair and word where the rule needs 2
__device__ __forceinline__ void nj_popc_add(uint32_t &h, uint32_t x) { asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(h) : "v"(x)); }

// A: the main tree's sets, R: the batch's ([replicate][wp][sp]); cap [n - 3] = light - 1; phi [replicate][n - 3]
__global__ void __launch_bounds__(256) nj_transfer_kernel(const uint32_t *A, const uint32_t *R, uint64_t stride, uint32_t n, uint32_t sp, uint32_t n_chunks, const uint32_t *cap,
                                                          uint32_t *phi) {
    const uint32_t ti = blockIdx.x, b = blockIdx.y, steps = n - 3, nt = sp / NJ_T_TILE, sp4 = sp / 4;
    __shared__ uint4 sA[NJ_T_CHUNK * T_Q], sB[NJ_T_CHUNK * T_Q];
    const uint32_t tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const uint4 *A4 = (const uint4 *)A + (uint64_t)ti * T_Q, *R4 = (const uint4 *)(R + (uint64_t)b * stride);
    const bool keep_a = n_chunks == 1;      // uniform: the main tile is staged once
    uint32_t h[4][4], mn[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        mn[r] = 0xffffffffu;
#pragma unroll
        for (uint32_t s = 0; s < 4; s++) h[r][s] = 0;
    }
    // cell tid of a chunk is word ty of the chunk, splits 4 tx .. 4 tx + 3 of the tile
    uint4 ra = A4[(uint64_t)ty * sp4 + tx], rb = R4[(uint64_t)ty * sp4 + tx];
    uint32_t tj = 0, k = 0;
    for (uint32_t it = 0, total = nt * n_chunks; it < total; it++) {
        __syncthreads();      // the chunk before is read
        if (!keep_a || it == 0) sA[tid] = ra;
        sB[tid] = rb;
        __syncthreads();
        const bool last = k + 1 == n_chunks;
        const uint32_t tj2 = last ? tj + 1 : tj, k2 = last ? 0 : k + 1;
        if (it + 1 < total) {
            const uint64_t base = ((uint64_t)k2 * NJ_T_CHUNK + ty) * sp4 + tx;
            if (!keep_a) ra = A4[base];
            rb = R4[base + (uint64_t)tj2 * T_Q];
        }
#pragma unroll 4
        for (uint32_t w = 0; w < NJ_T_CHUNK; w++) {
            const uint4 a4 = sA[w * T_Q + ty], b4 = sB[w * T_Q + tx];
            const uint32_t av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (uint32_t r = 0; r < 4; r++)
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) nj_popc_add(h[r][s], av[r] ^ bv[s]);
        }
        if (last) {      // uniform: the tile's last word is counted
#pragma unroll
            for (uint32_t s = 0; s < 4; s++) {
                const bool real = tj * NJ_T_TILE + tx * 4 + s < steps;      // a padded row of the partial tile is no split
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    const uint32_t d = min(h[r][s], n - h[r][s]);
                    if (real) mn[r] = min(mn[r], d);
                    h[r][s] = 0;
                }
            }
        }
        tj = tj2; k = k2;
    }
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        uint32_t v = mn[r];
        for (int o = 1; o < 16; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));      // the 16 lanes of a main split are neighbours
        const uint32_t i = ti * NJ_T_TILE + ty * 4 + r;
        if (tx == 0 && i < steps) phi[(uint64_t)b * steps + i] = min(v, cap[i]);
    }
}

}  // namespace

void nj_transfer_device(int device, const NjTransferArgs &a) {
    if (a.n <= 3 || !a.n_rep) return;
    use_device(device, NJ_NO_FALLBACK);
    const uint32_t n = a.n, steps = n - 3, words = (n + 31) / 32, n_chunks = (words + NJ_T_CHUNK - 1) / NJ_T_CHUNK, wp = n_chunks * NJ_T_CHUNK;
    const uint32_t sp = (steps + NJ_T_TILE - 1) / NJ_T_TILE * NJ_T_TILE, nt = sp / NJ_T_TILE;
    const uint64_t stride = (uint64_t)wp * sp, per_tree = stride * 4 + (uint64_t)steps * 12, budget = tree_budget_bytes();      // bit sets, join records and phi
    const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(a.n_rep, T_BATCH_MAX), (budget - std::min(budget, per_tree)) / per_tree));
    hipStream_t s = nullptr;
    DevBuf<uint32_t> d_bits, d_ja, d_jb, d_cap, d_phi;
    d_bits.reserve_exact((size_t)(1 + batch) * stride);      // tree 0 is the main tree
    d_ja.reserve_exact((size_t)(1 + batch) * steps); d_jb.reserve_exact((size_t)(1 + batch) * steps);
    d_cap.reserve_exact(steps); d_phi.reserve_exact((size_t)batch * steps);
    UC_HIP(hipMemsetAsync(d_bits.p, 0, (size_t)(1 + batch) * stride * 4, s));      // the padding is never written again
    std::vector<uint32_t> cap(steps);
    for (uint32_t x = 0; x < steps; x++) cap[x] = a.light[x] - 1;
    UC_HIP(hipMemcpy(d_cap.p, cap.data(), (size_t)steps * 4, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_ja.p, a.join_a, (size_t)steps * 4, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_jb.p, a.join_b, (size_t)steps * 4, hipMemcpyHostToDevice));
    const bool timing = getenv("UC_TIMING") != nullptr;      // the comparison kernel alone, between two events per launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (timing) { UC_HIP(hipEventCreate(&ev0)); UC_HIP(hipEventCreate(&ev1)); }
    double kernel_ms = 0.0;
    uint32_t n_batches = 0;
    for (uint32_t b0 = 0; b0 < a.n_rep; b0 += batch, n_batches++) {
        const uint32_t nb = std::min<uint32_t>(batch, a.n_rep - b0), t0 = b0 ? 1 : 0, n_trees = nb + 1 - t0;
        UC_HIP(hipMemcpy(d_ja.p + steps, a.rep_join_a + (uint64_t)b0 * steps, (size_t)nb * steps * 4, hipMemcpyHostToDevice));
        UC_HIP(hipMemcpy(d_jb.p + steps, a.rep_join_b + (uint64_t)b0 * steps, (size_t)nb * steps * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nj_transfer_sets_kernel, grid_for((uint64_t)n_trees * words), dim3(256), 0, s, (const uint32_t *)d_ja.p, (const uint32_t *)d_jb.p, n, words, sp, stride, t0,
                           n_trees, d_bits.p);
        if (timing) UC_HIP(hipEventRecord(ev0, s));
        hipLaunchKernelGGL(nj_transfer_kernel, dim3(nt, nb), dim3(256), 0, s, (const uint32_t *)d_bits.p, (const uint32_t *)(d_bits.p + stride), stride, n, sp, n_chunks,
                           (const uint32_t *)d_cap.p, d_phi.p);
        if (timing) UC_HIP(hipEventRecord(ev1, s));
        UC_HIP(hipGetLastError());
        UC_HIP(hipMemcpy(a.phi + (uint64_t)b0 * steps, d_phi.p, (size_t)nb * steps * 4, hipMemcpyDeviceToHost));
        if (timing) { float ms = 0.f; UC_HIP(hipEventElapsedTime(&ms, ev0, ev1)); kernel_ms += ms; }
    }
    if (timing) {
        (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
        fprintf(stderr, "unicore-cluster[timing]: nj transfer: %u leaves, %u replicates in %u batch(es): comparison kernel %.3f ms = %.4g pair-words/s\n", n, a.n_rep, n_batches,
                kernel_ms, kernel_ms > 0.0 ? (double)steps * steps * words * a.n_rep / (kernel_ms * 1e-3) : 0.0);
    }
}

}  // namespace uc
