// uc_reassign.hip — the stage behind --cluster-reassign (rule UC-1/R): after the last round of the workflow every member is verified against the
// representative the transitive merge gave it, the members that fail are searched again against the representatives and each other, and the
// clustering rule runs once more on the graph of what was accepted.
//   1 verify      hit lists grouped by representative (query = representative, targets = its members, ascending) -> the gapped stage on the full database
//   2 seeds       D' = representatives (ascending) ++ rejected members (ascending)
//   3 re-search   prefilter of the rejected members against D', the gapped stage on those lists as they are (E-value against D')
//   4 re-cluster  {A[x], x} of every member that passed + the accepted pairs of 3 in global ids -> Engine::cluster_graph_dev_edges
// The lists of 1, the verdict, the seeds and the edge list are built and kept on the device; the host sees the per-representative list lengths (the
// engine keeps hit_cnt / hit_off on the host for every hit list), the counters, the id list of D' (upload_sub_db computes its layout on the host)
// and the final assignment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

namespace {

constexpr uint64_t RA_NO_KEY = ~0ull;      // a representative has no key: sorted last

// wave-aggregated append: the lanes with `take` get consecutive slots behind one atomicAdd per wave (returns the lane's slot; undefined without `take`)
__device__ __forceinline__ uint32_t ra_wave_slot(bool take, uint32_t *counter) {
    const unsigned long long m = __ballot(take);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (m && lane == (uint32_t)(__ffsll((long long)m) - 1)) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, m ? __ffsll((long long)m) - 1 : 0, 64);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

// ctr: [0] edges in the buffer, [1] rejected members, [2] accepted re-search pairs (self pairs dropped), [3] members, [4] malformed entries of A
// A must be idempotent and in range; a member's key is (representative << 32 | member)
__global__ void __launch_bounds__(256) ra_key_kernel(uint32_t n, const uint32_t *A, uint64_t *key, uint32_t *ctr) {
    unsigned long long n_member = 0, n_bad = 0;
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n; x += gridDim.x * 256) {
        const uint32_t a = A[x];
        const bool bad = a >= n || A[a] != a;
        const bool member = !bad && a != x;
        key[x] = member ? ((uint64_t)a << 32) | x : RA_NO_KEY;
        n_member += member; n_bad += bad;
    }
    block_add2(n_member, n_bad, &ctr[3], &ctr[4]);
}
// the sorted member keys are the hit lists: query = representative, target = member, score = diag = 0; the last member of a run finds the
// run's start (lower bound of representative << 32) and writes the list length
__global__ void __launch_bounds__(256) ra_lists_kernel(uint64_t nm, const uint64_t *key, uint32_t *hq, uint32_t *ht, int32_t *hs, int32_t *hd, uint32_t *cnt) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nm; i += (uint64_t)gridDim.x * 256) {
        const uint64_t k = key[i];
        const uint32_t rep = (uint32_t)(k >> 32);
        hq[i] = rep; ht[i] = (uint32_t)k; hs[i] = 0; hd[i] = 0;
        if (i + 1 == nm || (uint32_t)(key[i + 1] >> 32) != rep) {
            const uint64_t want = (uint64_t)rep << 32;
            uint64_t lo = 0, hi = i;
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (key[mid] < want) lo = mid + 1; else hi = mid; }
            cnt[rep] = (uint32_t)(i + 1 - lo);
        }
    }
}
// one pass over the records of those lists: the member's flag, the accepted (representative, member) appended to the edge buffer, both counted
__global__ void __launch_bounds__(256) ra_verdict_kernel(uint64_t nm, const uc_aln *alns, const uint32_t *hq, const uint32_t *ht, uint32_t *rej, uint32_t *edges, uint32_t *ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256, nm_up = (nm + 63) & ~63ull;      // whole waves enter the loop: the ballot of ra_wave_slot sees every lane
    unsigned long long n_rej = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nm_up; i += stride) {
        const bool in = i < nm;
        const bool acc = in && alns[i].accepted == 1;
        const uint32_t slot = ra_wave_slot(acc, &ctr[0]);
        if (acc) { edges[2ull * slot] = hq[i]; edges[2ull * slot + 1] = ht[i]; }
        if (in && !acc) rej[ht[i]] = 1u;
        n_rej += in && !acc;
    }
    block_add(n_rej, &ctr[1]);
}
__global__ void __launch_bounds__(256) ra_rep_flag_kernel(uint32_t n, const uint32_t *A, uint32_t *is_rep) {
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n; x += gridDim.x * 256) is_rep[x] = A[x] == x ? 1u : 0u;
}
// ids = representatives ascending, then rejected members ascending (pos_*: exclusive scans of the flags)
__global__ void __launch_bounds__(256) ra_seeds_kernel(uint32_t n, const uint32_t *is_rep, const uint32_t *pos_rep, const uint32_t *rej, const uint32_t *pos_rej,
                                                       uint32_t n_rep, uint32_t *ids) {
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n; x += gridDim.x * 256) {
        if (is_rep[x]) ids[pos_rep[x]] = x;
        else if (rej[x]) ids[n_rep + pos_rej[x]] = x;
    }
}
// the accepted pairs of the re-search, local ids of D' -> global ids, appended behind the verified edges (m = sequences of D': bounds the lookup)
__global__ void __launch_bounds__(256) ra_map_kernel(uint64_t ne, const uint32_t *local, const uint32_t *ids, uint32_t m, uint32_t *edges, uint32_t *ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * 256, ne_up = (ne + 63) & ~63ull;
    unsigned long long n_take = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < ne_up; i += stride) {
        uint32_t a = 0, b = 0;
        bool take = false;
        if (i < ne) {
            const uint32_t la = local[2 * i], lb = local[2 * i + 1];
            if (la < m && lb < m) { a = ids[la]; b = ids[lb]; take = a != b; }
        }
        const uint32_t slot = ra_wave_slot(take, &ctr[0]);
        if (take) { edges[2ull * slot] = a; edges[2ull * slot + 1] = b; }
        n_take += take;
    }
    block_add(n_take, &ctr[2]);
}

}  // namespace

void Engine::reassign(const uint32_t *assign_in, uint32_t *assign_out, uint8_t *rejected_out, uint64_t counts[4]) {
    PressureScope ps(*this, 1);      // pins the gapped stage's scratch set, which holds this stage's buffers, across the prefilter of step 3
    if (!have_db) fail(UC_ERR_ARGS, "reassign: no database loaded");
    if (!p.min_score_table.empty()) fail(UC_ERR_ARGS, "--cluster-reassign cannot be combined with --min-score-table (the re-search runs on a sub-database)");
    UC_HIP(hipSetDevice(device));
    const uint32_t n = hdb.n;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n == 0) return;
    const bool timing = getenv("UC_TIMING") != nullptr;
    Timer t_all, t_part;
    double ms_lists = 0, ms_verify = 0, ms_verdict = 0, ms_research = 0, ms_cluster = 0;
    auto lap = [&](double &acc) { acc += t_part.seconds() * 1e3; t_part = Timer(); };
    hipStream_t s = stream;
    ReassignScratch &S = scratch_of(*this).ra;

    // ---- 1: member lists from A
    S.assign.reserve(n); S.key.reserve(n); S.key2.reserve(n); S.ctr.reserve(8); S.cnt.reserve(n); S.rej.reserve(n);
    UC_HIP(hipMemcpyAsync(S.assign.p, assign_in, (size_t)n * 4, hipMemcpyHostToDevice, s));
    UC_HIP(hipMemsetAsync(S.ctr.p, 0, 8 * 4, s));
    UC_HIP(hipMemsetAsync(S.cnt.p, 0, (size_t)n * 4, s));
    UC_HIP(hipMemsetAsync(S.rej.p, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(ra_key_kernel, grid_for(n, count_grid_cap), dim3(256), 0, s, n, (const uint32_t *)S.assign.p, S.key.p, S.ctr.p);
    uint32_t h_ctr[8] = {};
    UC_HIP(hipMemcpyAsync(h_ctr, S.ctr.p, 8 * 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipGetLastError());
    if (h_ctr[4]) fail(UC_ERR_ARGS, "reassign: %u entries of the assignment are out of range or name a sequence that is not its own representative", h_ctr[4]);
    const uint64_t nm = h_ctr[3];
    const uint32_t n_rep = n - (uint32_t)nm;
    hit_cnt.assign(n, 0);
    hit_off.assign((size_t)n + 1, 0);
    n_hits = 0;
    alns_valid = false;
    clear_edges();
    if (nm) {
        // all 64 bits: a representative's all-ones key must stay behind the member keys
        rocprim_call(S.tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, S.key.p, S.key2.p, (size_t)n, 0u, 64u, s); });
        d_hq.reserve(nm); d_ht.reserve(nm); d_hs.reserve(nm); d_hd.reserve(nm);
        hipLaunchKernelGGL(ra_lists_kernel, grid_for(nm), dim3(256), 0, s, nm, (const uint64_t *)S.key2.p, d_hq.p, d_ht.p, d_hs.p, d_hd.p, S.cnt.p);
        UC_HIP(hipMemcpyAsync(hit_cnt.data(), S.cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        UC_HIP(hipGetLastError());
        for (uint32_t q = 0; q < n; q++) hit_off[q + 1] = hit_off[q] + hit_cnt[q];
        n_hits = hit_off[n];
        if (n_hits != nm) fail(UC_ERR_GENERIC, "reassign: member list bookkeeping mismatch (%llu listed, %llu members)", (unsigned long long)n_hits, (unsigned long long)nm);
    }
    lap(ms_lists);

    // ---- 1: verify, verdict
    S.edges.reserve(2 * std::max<uint64_t>(nm, 1));
    if (nm) {
        align(0, n);
        UC_HIP(hipStreamSynchronize(s));
        lap(ms_verify);
        hipLaunchKernelGGL(ra_verdict_kernel, grid_for(nm), dim3(256), 0, s, nm, (const uc_aln *)d_alns.p, (const uint32_t *)d_hq.p, (const uint32_t *)d_ht.p,
                           S.rej.p, S.edges.p, S.ctr.p);
        UC_HIP(hipMemcpyAsync(h_ctr, S.ctr.p, 8 * 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        UC_HIP(hipGetLastError());
        if ((uint64_t)h_ctr[0] + h_ctr[1] != nm) fail(UC_ERR_GENERIC, "reassign: %llu members became %u accepted + %u rejected", (unsigned long long)nm, h_ctr[0], h_ctr[1]);
    }
    const uint32_t n_acc = h_ctr[0], n_rej = h_ctr[1];
    if (rejected_out) {
        std::vector<uint32_t> hr(n);
        UC_HIP(hipMemcpyAsync(hr.data(), S.rej.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        for (uint32_t x = 0; x < n; x++) rejected_out[x] = hr[x] ? 1 : 0;
    }
    lap(ms_verdict);

    // ---- 2 + 3: seeds, re-search of the rejected members against D'
    uint64_t n_total = n_acc;
    if (n_rej) {
        const uint32_t m = n_rep + n_rej;
        S.flag.reserve(n); S.pos.reserve(n); S.pos2.reserve(n); S.ids.reserve(m);
        hipLaunchKernelGGL(ra_rep_flag_kernel, grid_for(n), dim3(256), 0, s, n, (const uint32_t *)S.assign.p, S.flag.p);
        rocprim_call(S.tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, S.flag.p, S.pos.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), s); });
        rocprim_call(S.tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, S.rej.p, S.pos2.p, 0u, (size_t)n, rocprim::plus<uint32_t>(), s); });
        hipLaunchKernelGGL(ra_seeds_kernel, grid_for(n), dim3(256), 0, s, n, (const uint32_t *)S.flag.p, (const uint32_t *)S.pos.p, (const uint32_t *)S.rej.p,
                           (const uint32_t *)S.pos2.p, n_rep, S.ids.p);
        std::vector<uint32_t> ids(m);
        UC_HIP(hipMemcpyAsync(ids.data(), S.ids.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        UC_HIP(hipGetLastError());
        // the sub-database is gathered on the device from the raw tracks of the full one: they go up now unless the workflow kept them
        if (!raw_resident) {
            if (hdb.s3.size() != hdb.residues() || hdb.sa.size() != hdb.residues()) fail(UC_ERR_GENERIC, "reassign: the database's letters are neither on the device nor on the host");
            upload_db(/*keep_raw=*/true);
        }
        HostDb full = std::move(hdb);
        const uint64_t ev_saved = evalue_residues;
        evalue_residues = 0;                       // E-value against the residues of D'
        upload_sub_db(ids, full.off);
        prefilter(0, m, n_rep, m);
        align(n_rep, m);
        const uint64_t ne3 = edges_on_host ? 0 : n_edges_dev;
        if (ne3) {
            S.edges.grow_preserve(2 * ((uint64_t)n_acc + ne3), 2 * (uint64_t)n_acc, s);
            hipLaunchKernelGGL(ra_map_kernel, grid_for(ne3), dim3(256), 0, s, ne3, (const uint32_t *)d_edges.p, (const uint32_t *)S.ids.p, m, S.edges.p, S.ctr.p);
            UC_HIP(hipMemcpyAsync(h_ctr, S.ctr.p, 8 * 4, hipMemcpyDeviceToHost, s));
            UC_HIP(hipStreamSynchronize(s));
            UC_HIP(hipGetLastError());
            if ((uint64_t)h_ctr[0] != (uint64_t)n_acc + h_ctr[2] || h_ctr[2] > ne3) fail(UC_ERR_GENERIC, "reassign: edge buffer bookkeeping mismatch");
        }
        n_total = h_ctr[0];
        // the full database again: step 4 ranks its lengths, and the caller's engine is left as it was found
        ids.resize(n);
        std::iota(ids.begin(), ids.end(), 0u);
        upload_sub_db(ids, full.off);
        hdb = std::move(full);
        evalue_residues = ev_saved;
        lap(ms_research);
    }

    // ---- 4: the run's clustering rule on the graph of everything that was accepted
    cluster_graph_dev_edges(n, S.edges.p, n_total, assign_out);
    lap(ms_cluster);
    uint64_t n_clu = 0;
    for (uint32_t x = 0; x < n; x++) n_clu += assign_out[x] == x ? 1 : 0;
    counts[0] = nm; counts[1] = n_rej; counts[2] = h_ctr[2]; counts[3] = n_clu;
    if (timing)
        fprintf(stderr, "unicore-cluster[timing]: reassign: %llu members in %u lists; lists %.2f ms, verify (gapped stage) %.2f ms, verdict %.2f ms, "
                        "re-search of %u rejected %.2f ms, re-cluster of %llu edges %.2f ms, total %.2f ms\n",
                (unsigned long long)nm, n_rep, ms_lists, ms_verify, ms_verdict, n_rej, ms_research, (unsigned long long)n_total, ms_cluster, t_all.seconds() * 1e3);
}

}  // namespace uc
