// uc_profile.hip — the device counter of `unicore profile` (rule UC-P; /root/reference/src/modules/profile.rs:79-84,121-143).
//   1 expand   rows -> one (group << 24 | species, gene) pair per (row, species): row counts, an exclusive scan, one thread per pair
//   2 sort     stable radix sort of the pairs over the 48 used key bits: a (group, species) run holds its genes in row order
//   3 runs     heads of the runs, their index by an inclusive scan; a run's start, key and first gene, and whether any gene of it differs
//              from its predecessor - one comparison per element, a run can be the whole input
//   4 groups   a group's runs by two lower bounds; single / multiple / file lines from one exclusive scan of the packed run flags
//              (run of length 1 | run of one distinct gene << 32); the core test in 64-bit integers; core_off by a scan of the line counts
//   5 emit     full[s] by atomicAdd for the length-1 runs of core groups; the file lines at core_off[g] + the run's rank among the group's
//              one-gene runs: ascending species, no atomics, the same bytes on every run
// Scratch is hipMalloc'ed and freed inside the call: this is not a warm path and the engine's scratch sets are not involved.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_engine.h"
#include "uc_profile.h"

namespace uc {

namespace {

constexpr uint32_t PF_SP_BITS = 24;
constexpr uint64_t PF_SP_MASK = (1ull << PF_SP_BITS) - 1;
constexpr uint64_t PF_ONE_GENE = 1ull << 32;      // run flags: bit 0 = one row, bit 32 = one distinct gene; scanned together, both sums stay below 2^32

__global__ void __launch_bounds__(256) pf_rowcount_kernel(uint64_t n_rows, const uint32_t *gene, const uint64_t *sp_off, uint32_t *cnt) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (uint64_t)gridDim.x * 256) {
        const uint32_t g = gene[i];
        cnt[i] = g == UC_NO_GENE ? 0u : (uint32_t)(sp_off[g + 1] - sp_off[g]);
    }
}
// pair p belongs to the last row whose first pair is <= p (rows without pairs share their successor's position and are stepped over)
__global__ void __launch_bounds__(256) pf_expand_kernel(uint64_t n_pairs, uint64_t n_rows, const uint32_t *row_pos, const uint32_t *group, const uint32_t *gene,
                                                        const uint64_t *sp_off, const uint32_t *sp, uint64_t *key, uint32_t *val) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256) {
        uint64_t lo = 0, hi = n_rows;      // first row with row_pos > p
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (row_pos[mid] <= p) lo = mid + 1; else hi = mid; }
        const uint64_t row = lo - 1;
        const uint32_t g = gene[row];
        key[p] = ((uint64_t)group[row] << PF_SP_BITS) | sp[sp_off[g] + (p - row_pos[row])];
        val[p] = g;
    }
}
__global__ void __launch_bounds__(256) pf_head_kernel(uint64_t n_pairs, const uint64_t *key, uint32_t *head) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256)
        head[p] = p == 0 || key[p] != key[p - 1] ? 1u : 0u;
}
// rid = inclusive scan of the heads; run_multi is zeroed before: every lane that sees a change of gene inside a run stores the same 1
__global__ void __launch_bounds__(256) pf_run_kernel(uint64_t n_pairs, const uint64_t *key, const uint32_t *val, const uint32_t *rid, uint32_t *run_start,
                                                     uint64_t *run_key, uint32_t *run_gene, uint32_t *run_multi) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256) {
        const uint32_t r = rid[p] - 1;
        const uint64_t k = key[p];
        const uint32_t v = val[p];
        if (p == 0 || k != key[p - 1]) { run_start[r] = (uint32_t)p; run_key[r] = k; run_gene[r] = v; }
        else if (v != val[p - 1]) run_multi[r] = 1u;
    }
}
// n_runs + 1 flags, the last one 0: the exclusive scan then ends with the totals
__global__ void __launch_bounds__(256) pf_flag_kernel(uint32_t n_runs, uint32_t n_pairs, const uint32_t *run_start, const uint32_t *run_multi, uint64_t *flag) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= n_runs; r += (uint64_t)gridDim.x * 256) {
        uint64_t f = 0;
        if (r < n_runs) {
            const uint32_t len = (r + 1 < n_runs ? run_start[r + 1] : n_pairs) - run_start[r];
            f = (len == 1 ? 1ull : 0ull) | (run_multi[r] ? 0ull : PF_ONE_GENE);
        }
        flag[r] = f;
    }
}
// first run of group g (g = n_groups: n_runs)
__global__ void __launch_bounds__(256) pf_bound_kernel(uint32_t n_groups, uint32_t n_runs, const uint64_t *run_key, uint32_t *glo) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * 256) {
        const uint64_t want = g << PF_SP_BITS;
        uint32_t lo = 0, hi = n_runs;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (run_key[mid] < want) lo = mid + 1; else hi = mid; }
        glo[g] = lo;
    }
}
// thr_s = threshold * S (profile.rs:134); n_groups + 1 line counts, the last one 0
__global__ void __launch_bounds__(256) pf_group_kernel(uint32_t n_groups, const uint32_t *glo, const uint64_t *fsum, uint64_t thr_s, uint32_t *single, uint32_t *multiple,
                                                       uint8_t *core, uint64_t *n_lines) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g <= n_groups; g += (uint64_t)gridDim.x * 256) {
        uint64_t lines = 0;
        if (g < n_groups) {
            const uint32_t lo = glo[g], hi = glo[g + 1];
            const uint64_t d = fsum[hi] - fsum[lo];      // both halves are sums of a prefix: neither borrows
            const uint32_t sg = (uint32_t)d;
            const bool c = (uint64_t)sg * 100 >= thr_s;
            single[g] = sg; multiple[g] = hi - lo; core[g] = c ? 1 : 0;
            if (c) lines = d >> 32;
        }
        n_lines[g] = lines;
    }
}
__global__ void __launch_bounds__(256) pf_emit_kernel(uint32_t n_runs, const uint64_t *run_key, const uint32_t *run_gene, const uint64_t *flag, const uint64_t *fsum,
                                                      const uint32_t *glo, const uint8_t *core, const uint64_t *core_off, uint32_t *core_gene, uint32_t *core_species,
                                                      uint32_t *full) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * 256) {
        const uint64_t k = run_key[r], f = flag[r];
        const uint32_t g = (uint32_t)(k >> PF_SP_BITS), s = (uint32_t)(k & PF_SP_MASK);
        if (!core[g]) continue;
        if (f & 1) atomicAdd(&full[s], 1u);
        if (f & PF_ONE_GENE) {
            const uint64_t pos = core_off[g] + ((fsum[r] >> 32) - (fsum[glo[g]] >> 32));
            core_gene[pos] = run_gene[r];
            core_species[pos] = s;
        }
    }
}

struct PfEvents {      // stage boundaries on the null stream, only when the caller asked for times
    hipEvent_t e[6] = {};
    int n = 0;
    bool on;
    explicit PfEvents(bool on_) : on(on_) { if (on) for (auto &x : e) UC_HIP(hipEventCreate(&x)); }
    ~PfEvents() { if (on) for (auto &x : e) if (x) (void)hipEventDestroy(x); }
    void mark() { if (on && n < 6) UC_HIP(hipEventRecord(e[n++], nullptr)); }
};

}  // namespace

void profile_count_device(int device, const ProfileArgs &a, uint64_t n_pairs, float *ms) {
    use_device(device, "the profile counter's device path has no CPU fallback (UC_PROFILE_HOST=1 selects the host counter)");
    const uint32_t ng = a.n_groups, ns = a.n_species;
    const uint64_t thr_s = (uint64_t)a.threshold * ns;
    if (ms) std::fill(ms, ms + 6, 0.f);
    if (ng) { memset(a.single, 0, (size_t)ng * 4); memset(a.multiple, 0, (size_t)ng * 4); }
    memset(a.core_off, 0, ((size_t)ng + 1) * 8);
    if (ns) memset(a.full, 0, (size_t)ns * 4);
    if (n_pairs == 0) {      // nothing is launched: no group has a mapped row, and such a group is core only under threshold * S == 0
        if (ng) memset(a.core, thr_s == 0 ? 1 : 0, ng);
        return;
    }
    hipStream_t s = nullptr;
    const uint64_t n_rows = a.n_rows, P = n_pairs;
    PfEvents ev(ms != nullptr);
    DevBuf<char> tmp;
    DevBuf<uint32_t> d_group, d_gene, d_sp, d_cnt, d_pos, d_val, d_val2, d_head, d_rid;
    DevBuf<uint64_t> d_spoff, d_key, d_key2;

    // ---- 1: expand
    d_group.reserve_exact(n_rows); d_gene.reserve_exact(n_rows); d_cnt.reserve_exact(n_rows); d_pos.reserve_exact(n_rows);
    d_spoff.reserve_exact((size_t)a.n_genes + 1); d_sp.reserve_exact(a.sp_off[a.n_genes]);
    d_key.reserve_exact(P); d_key2.reserve_exact(P); d_val.reserve_exact(P); d_val2.reserve_exact(P);
    UC_HIP(hipMemcpy(d_group.p, a.group, n_rows * 4, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_gene.p, a.gene, n_rows * 4, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_spoff.p, a.sp_off, ((size_t)a.n_genes + 1) * 8, hipMemcpyHostToDevice));
    UC_HIP(hipMemcpy(d_sp.p, a.sp, a.sp_off[a.n_genes] * 4, hipMemcpyHostToDevice));
    ev.mark();
    hipLaunchKernelGGL(pf_rowcount_kernel, grid_for(n_rows), dim3(256), 0, s, n_rows, (const uint32_t *)d_gene.p, (const uint64_t *)d_spoff.p, d_cnt.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_cnt.p, d_pos.p, 0u, (size_t)n_rows, rocprim::plus<uint32_t>(), s); });
    hipLaunchKernelGGL(pf_expand_kernel, grid_for(P), dim3(256), 0, s, P, n_rows, (const uint32_t *)d_pos.p, (const uint32_t *)d_group.p, (const uint32_t *)d_gene.p,
                       (const uint64_t *)d_spoff.p, (const uint32_t *)d_sp.p, d_key.p, d_val.p);
    ev.mark();

    // ---- 2: sort (stable; bits 0 .. 48 hold group << 24 | species)
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, d_key.p, d_key2.p, d_val.p, d_val2.p, (size_t)P, 0u, 2 * PF_SP_BITS, s); });
    ev.mark();

    // ---- 3: runs
    d_head.reserve_exact(P); d_rid.reserve_exact(P);
    hipLaunchKernelGGL(pf_head_kernel, grid_for(P), dim3(256), 0, s, P, (const uint64_t *)d_key2.p, d_head.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, d_head.p, d_rid.p, (size_t)P, rocprim::plus<uint32_t>(), s); });
    uint32_t R = 0;
    UC_HIP(hipMemcpy(&R, d_rid.p + (P - 1), 4, hipMemcpyDeviceToHost));
    UC_HIP(hipGetLastError());
    if (R == 0 || R > P) fail(UC_ERR_GENERIC, "profile: run bookkeeping mismatch (%u runs of %llu pairs)", R, (unsigned long long)P);
    DevBuf<uint32_t> d_rstart, d_rgene, d_rmulti, d_glo, d_single, d_multiple, d_full, d_cgene, d_cspecies;
    DevBuf<uint64_t> d_rkey, d_flag, d_fsum, d_nlines, d_coff;
    DevBuf<uint8_t> d_core;
    d_rstart.reserve_exact(R); d_rgene.reserve_exact(R); d_rmulti.reserve_exact(R); d_rkey.reserve_exact(R);
    d_flag.reserve_exact((size_t)R + 1); d_fsum.reserve_exact((size_t)R + 1);
    UC_HIP(hipMemsetAsync(d_rmulti.p, 0, (size_t)R * 4, s));
    hipLaunchKernelGGL(pf_run_kernel, grid_for(P), dim3(256), 0, s, P, (const uint64_t *)d_key2.p, (const uint32_t *)d_val2.p, (const uint32_t *)d_rid.p, d_rstart.p,
                       d_rkey.p, d_rgene.p, d_rmulti.p);
    hipLaunchKernelGGL(pf_flag_kernel, grid_for((uint64_t)R + 1), dim3(256), 0, s, R, (uint32_t)P, (const uint32_t *)d_rstart.p, (const uint32_t *)d_rmulti.p, d_flag.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_flag.p, d_fsum.p, (uint64_t)0, (size_t)R + 1, rocprim::plus<uint64_t>(), s); });
    ev.mark();

    // ---- 4: groups
    d_glo.reserve_exact((size_t)ng + 1); d_single.reserve_exact(ng); d_multiple.reserve_exact(ng); d_core.reserve_exact(ng);
    d_nlines.reserve_exact((size_t)ng + 1); d_coff.reserve_exact((size_t)ng + 1);
    hipLaunchKernelGGL(pf_bound_kernel, grid_for((uint64_t)ng + 1), dim3(256), 0, s, ng, R, (const uint64_t *)d_rkey.p, d_glo.p);
    hipLaunchKernelGGL(pf_group_kernel, grid_for((uint64_t)ng + 1), dim3(256), 0, s, ng, (const uint32_t *)d_glo.p, (const uint64_t *)d_fsum.p, thr_s, d_single.p,
                       d_multiple.p, d_core.p, d_nlines.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_nlines.p, d_coff.p, (uint64_t)0, (size_t)ng + 1, rocprim::plus<uint64_t>(), s); });
    ev.mark();

    // ---- 5: emit (at most one line per run: R <= P, the capacity the caller gave core_gene / core_species)
    d_full.reserve_exact(ns); d_cgene.reserve_exact(R); d_cspecies.reserve_exact(R);
    UC_HIP(hipMemsetAsync(d_full.p, 0, (size_t)ns * 4, s));
    hipLaunchKernelGGL(pf_emit_kernel, grid_for(R), dim3(256), 0, s, R, (const uint64_t *)d_rkey.p, (const uint32_t *)d_rgene.p, (const uint64_t *)d_flag.p,
                       (const uint64_t *)d_fsum.p, (const uint32_t *)d_glo.p, (const uint8_t *)d_core.p, (const uint64_t *)d_coff.p, d_cgene.p, d_cspecies.p, d_full.p);
    ev.mark();
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipGetLastError());
    UC_HIP(hipMemcpy(a.core_off, d_coff.p, ((size_t)ng + 1) * 8, hipMemcpyDeviceToHost));
    const uint64_t n_lines = a.core_off[ng];
    if (n_lines > R) fail(UC_ERR_GENERIC, "profile: %llu file lines from %u runs", (unsigned long long)n_lines, R);
    UC_HIP(hipMemcpy(a.single, d_single.p, (size_t)ng * 4, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.multiple, d_multiple.p, (size_t)ng * 4, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.core, d_core.p, ng, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.full, d_full.p, (size_t)ns * 4, hipMemcpyDeviceToHost));
    if (n_lines) {
        UC_HIP(hipMemcpy(a.core_gene, d_cgene.p, n_lines * 4, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.core_species, d_cspecies.p, n_lines * 4, hipMemcpyDeviceToHost));
    }
    if (ms) {
        for (int i = 0; i < 5; i++) UC_HIP(hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]));
        UC_HIP(hipEventElapsedTime(&ms[5], ev.e[0], ev.e[5]));
    }
}

}  // namespace uc
