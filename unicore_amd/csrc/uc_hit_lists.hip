// uc_hit_lists.hip - prefilter stages E3 / E4 and everything that works on installed hit lists.
// Consumes a batch's candidates (uc_diag_select.hip, or the tiles of --prefilter-mode 1) and record lists handed in by the chunk loop or by other ranks.
// Produces the engine's device-resident hit lists (query, target, ungapped score, diagonal; grouped by query, score descending, target ascending, at most
// max_seqs per query) and the per-query counts / offsets on the host: rescore_ungapped (E3), select_and_append (E4: sort by (query, score desc, target), rank
// inside the query's run, scatter), merge_hits_dev (two lists merged under the same order and truncated: chunk accumulator, shards of other ranks),
// partition_hits_by_owner / import_hits_dev / export_hits_dev (multi-GPU: pair ownership), ungapped_select (kernel-level entry point).  spec UC-1 E3-E4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_prefilter_internal.h"

namespace uc {

// E4 sort key: [ query : 32 | 255 - score : 8 | target : 24 ]; score < min -> all-ones (sorted last)
__global__ void __launch_bounds__(256) select_key_kernel(uint64_t n, const uint32_t *cq, const uint32_t *ct, const int32_t *score,
                                                         int min_score, uint64_t *key, unsigned long long *n_kept) {
    unsigned long long kept = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int s = score[i];
        const bool ok = s >= min_score;
        key[i] = ok ? ((uint64_t)cq[i] << 32) | ((uint64_t)(255 - s) << 24) | ct[i] : ~0ull;
        kept += ok;
    }
    block_add(kept, n_kept);
}

// E4 truncation: entry i of the (query, score desc, target) sorted list survives iff its rank inside its
// query's run is < max_seqs
__global__ void __launch_bounds__(256) rank_flag_kernel(const uint64_t *skey, uint64_t n, uint32_t max_seqs, uint32_t *flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        // rank inside the query's run < max_seqs  <=>  the entry max_seqs places earlier belongs to another (smaller) query: ONE load (r04; a binary
        // search for the run's first entry cost ~30 dependent loads per entry: 315 GB of fetches per configs[2] pass)
        const uint64_t qk = skey[i] & 0xFFFFFFFF00000000ull;
        flag[i] = (i < max_seqs || skey[i - max_seqs] < qk) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(256) hit_scatter_kernel(const uint64_t *skey, const int32_t *sdiag, uint64_t n, const uint32_t *flag,
                                                          const uint64_t *pos, uint32_t *hq, uint32_t *ht, int32_t *hs, int32_t *hd) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint64_t k = skey[i], w = pos[i];
        hq[w] = (uint32_t)(k >> 32);
        ht[w] = (uint32_t)(k & 0xFFFFFFu);
        hs[w] = 255 - (int32_t)((k >> 24) & 0xFF);
        hd[w] = sdiag[i];
    }
}

// per-query hit counts from the query-sorted hit array
__global__ void __launch_bounds__(256) hit_count_kernel(const uint32_t *hq, uint64_t n_hits, uint32_t n, uint32_t *cnt) {
    for (uint32_t q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
        uint64_t lo = 0, hi = n_hits;
        while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (hq[m] < q) lo = m + 1; else hi = m; }
        const uint64_t b = lo;
        hi = n_hits;
        while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (hq[m] <= q) lo = m + 1; else hi = m; }
        cnt[q] = (uint32_t)(lo - b);
    }
}

// ---- multi-GPU: merge of the all-gathered shard lists + pair ownership, on the device ----
// owner of the unordered pair {a,b}: mutual hits (q,t)/(t,q) must meet on one rank to share their DP.  The owner is a
// hash of the pair's REPRESENTATIVE QUERY (the shorter sequence, ties: smaller id - the orientation uc_align.hip computes),
// so a rank owns whole queries of the forward pass: its workgroup tasks stay as large as on one GPU (a hash of the pair
// itself scattered every query's pairs over all ranks: 8 x smaller tasks, the gapped stage scaled 3.7x on 8 ranks, not 8x)
__device__ __forceinline__ uint32_t pair_owner(uint32_t a, uint32_t b, const uint32_t *len, uint32_t world) {
    const uint32_t la = len[a], lb = len[b];
    const uint32_t rep = (la < lb || (la == lb && a < b)) ? a : b;
    uint32_t h = rep * 0x9E3779B1u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h % world;
}
__global__ void __launch_bounds__(256) merge_key_kernel(uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *score,
                                                        uint32_t nseq, uint64_t *key, uint32_t *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int s = score[i];
        if (q[i] >= nseq || t[i] >= nseq || s < 0 || s > 255) atomicAdd(bad, 1u);
        key[i] = ((uint64_t)q[i] << 32) | ((uint64_t)(255 - (s & 255)) << 24) | (t[i] & 0xFFFFFFu);
    }
}
__global__ void __launch_bounds__(256) owner_flag_kernel(const uint64_t *skey, uint64_t n, const uint32_t *len, uint32_t rank, uint32_t world, uint32_t *flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (flag[i] && pair_owner((uint32_t)(skey[i] >> 32), (uint32_t)(skey[i] & 0xFFFFFFu), len, world) != rank) flag[i] = 0;
}

// owner rank per installed hit + identity index (input of the stable partition by owner)
__global__ void __launch_bounds__(256) owner_key_kernel(uint64_t n, const uint32_t *hq, const uint32_t *ht, const uint32_t *len, uint32_t world,
                                                        uint32_t *okey, uint32_t *idx, unsigned long long *count /* world */) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t o = pair_owner(hq[i], ht[i], len, world);
        okey[i] = o;
        idx[i] = (uint32_t)i;
        // one atomic per wave and owner: the lanes of a wave that share an owner elect a leader
        for (uint32_t w = 0; w < world; w++) {
            const unsigned long long m = __ballot(o == w);
            if (m && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1) atomicAdd(count + w, (unsigned long long)__popcll(m));
        }
    }
}
__global__ void __launch_bounds__(256) owner_gather_kernel(uint64_t n, const uint32_t *idx, const uint32_t *hq, const uint32_t *ht, const int32_t *hs,
                                                           const int32_t *hd, uint32_t *oq, uint32_t *ot, int32_t *os, int32_t *od) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t j = idx[i];
        oq[i] = hq[j]; ot[i] = ht[j]; os[i] = hs[j]; od[i] = hd[j];
    }
}

// the engine's four hit arrays (query, target, score, diagonal) as a unit: exchanged with another set (no copy) ...
void swap_hits(Engine &E, DevBuf<uint32_t> &q, DevBuf<uint32_t> &t, DevBuf<int32_t> &s, DevBuf<int32_t> &d) {
    q.swap(E.d_hq); t.swap(E.d_ht); s.swap(E.d_hs); d.swap(E.d_hd);
}
// ... and copied on the device into arrays with room for n_hits records (complete on return)
void copy_hits_dev(const Engine &E, uint32_t *dq, uint32_t *dt, int32_t *ds, int32_t *dd) {
    UC_HIP(hipMemcpyAsync(dq, E.d_hq.p, E.n_hits * 4, hipMemcpyDeviceToDevice, E.stream));
    UC_HIP(hipMemcpyAsync(dt, E.d_ht.p, E.n_hits * 4, hipMemcpyDeviceToDevice, E.stream));
    UC_HIP(hipMemcpyAsync(ds, E.d_hs.p, E.n_hits * 4, hipMemcpyDeviceToDevice, E.stream));
    UC_HIP(hipMemcpyAsync(dd, E.d_hd.p, E.n_hits * 4, hipMemcpyDeviceToDevice, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
}
// per-query counts / offsets of the installed (query-grouped) device lists: the host only keeps these two small arrays (hit_cnt is all zero on entry)
void Engine::finish_hit_lists(const char *who) {
    const uint32_t n = hdb.n;
    if (n_hits) {
        pre->sel.d_cnt.reserve(n);
        hipLaunchKernelGGL(hit_count_kernel, grid_for(n), dim3(256), 0, stream, d_hq.p, n_hits, n, pre->sel.d_cnt.p);
        UC_HIP(hipMemcpyAsync(hit_cnt.data(), pre->sel.d_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        UC_HIP(hipStreamSynchronize(stream));
    }
    for (uint32_t q = 0; q < n; q++) hit_off[q + 1] = hit_off[q] + hit_cnt[q];
    if (hit_off[n] != n_hits) fail(UC_ERR_GENERIC, "%s: hit list bookkeeping mismatch", who);
}

// E3.  consumes the n_cand candidates; produces their ungapped scores (d_score) and the overlap residue count in d_counters[2]
void rescore_ungapped(Engine &E, PrefilterPass &PP, uint64_t n_cand) {
    PrefilterScratch &S = *E.pre;
    Timer t_u;
    E.timed_ms_begin();
    S.sel.d_score.reserve(n_cand);
    launch_ungapped(E.ddb, n_cand, S.cand.d_cq.p, S.cand.d_ct.p, S.cand.d_cd.p, S.sel.d_score.p, S.shared.d_counters.p + 2, E.stream);
    UC_HIP(hipGetLastError());
    PP.gpu_ms += E.timed_ms_end();
    PP.t_ung += t_u.seconds();
}

// E4.  consumes the scored candidates; produces the batch's hits (score >= min_ungapped, rank < max_seqs in their query's run) appended to the device lists
void select_and_append(Engine &E, PrefilterPass &PP, uint64_t n_cand) {
    PrefilterScratch &S = *E.pre;
    Timer t_s;
    E.timed_ms_begin();
    S.sel.d_skey.reserve(n_cand); S.sel.d_skey2.reserve(n_cand); S.sel.d_cd2.reserve(n_cand);
    UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 1, 0, 8, E.stream));
    hipLaunchKernelGGL(select_key_kernel, grid_for(n_cand, E.count_grid_cap), dim3(256), 0, E.stream, n_cand, S.cand.d_cq.p, S.cand.d_ct.p, S.sel.d_score.p, E.p.min_ungapped, S.sel.d_skey.p, S.shared.d_counters.p + 1);
    unsigned kb = 33;      // the query field ends below bit 32 + log2(n) + 1: the all-ones key of a dropped candidate still sorts behind every kept one
    while (kb < 64 && (1ull << (kb - 32)) <= E.hdb.n) kb++;
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, S.sel.d_skey.p, S.sel.d_skey2.p, S.cand.d_cd.p, S.sel.d_cd2.p, (size_t)n_cand, 0u, kb, E.stream); });
    unsigned long long kept = 0;
    UC_HIP(hipMemcpyAsync(&kept, S.shared.d_counters.p + 1, 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    if (kept) {   // rank inside each query's run, keep the first max_seqs, append to the device hit lists
        S.sel.d_flag.reserve(kept); S.sel.d_pos.reserve(kept);
        hipLaunchKernelGGL(rank_flag_kernel, grid_for(kept), dim3(256), 0, E.stream, S.sel.d_skey2.p, (uint64_t)kept, (uint32_t)E.p.max_seqs, S.sel.d_flag.p);
        const uint64_t add = compact_u64(E, S.shared.d_temp, S.sel.d_flag.p, S.sel.d_pos.p, kept), n_hits = E.n_hits;
        E.d_hq.grow_preserve(n_hits + add, n_hits, E.stream); E.d_ht.grow_preserve(n_hits + add, n_hits, E.stream);
        E.d_hs.grow_preserve(n_hits + add, n_hits, E.stream); E.d_hd.grow_preserve(n_hits + add, n_hits, E.stream);
        hipLaunchKernelGGL(hit_scatter_kernel, grid_for(kept), dim3(256), 0, E.stream, S.sel.d_skey2.p, S.sel.d_cd2.p, (uint64_t)kept, S.sel.d_flag.p, S.sel.d_pos.p,
                           E.d_hq.p + n_hits, E.d_ht.p + n_hits, E.d_hs.p + n_hits, E.d_hd.p + n_hits);
        E.n_hits += add;
    }
    UC_HIP(hipGetLastError());
    PP.gpu_ms += E.timed_ms_end();
    PP.t_sel += t_s.seconds();
}

void Engine::export_hits_dev(uint32_t *dq, uint32_t *dt, int32_t *ds, int32_t *dd) const {
    if (!n_hits) return;
    UC_HIP(hipSetDevice(device));
    copy_hits_dev(*this, dq, dt, ds, dd);
}

// Multi-GPU phase 2: the engine's (merged, truncated) lists regrouped by the rank that owns each pair.  The partition is a
// STABLE radix sort on ceil(log2 world) bits, so every owner's segment keeps the list order (query, score desc, target asc).
// dq..dd: caller-owned device arrays of n_hits elements; counts[world] on the host.
void Engine::partition_hits_by_owner(uint32_t world, uint32_t *dq, uint32_t *dt, int32_t *ds, int32_t *dd, uint64_t *counts) {
    PressureScope ps(*this, 0);
    for (uint32_t w = 0; w < world; w++) counts[w] = 0;
    if (!n_hits) return;
    if (n_hits >= (1ull << 32)) fail(UC_ERR_GENERIC, "partition_hits_by_owner: %llu records exceed the 32-bit index", (unsigned long long)n_hits);
    UC_HIP(hipSetDevice(device));
    if (!pre) pre = ParkedScratch<PrefilterScratch>::take_or_new(device);
    DevBuf<uint32_t> &okey = pre->cand.d_cq, &okey2 = pre->cand.d_ct, &idx = pre->sel.d_flag, &idx2 = pre->sel.d_cnt;
    DevBuf<unsigned long long> cnt;
    okey.reserve(n_hits); okey2.reserve(n_hits); idx.reserve(n_hits); idx2.reserve(n_hits); cnt.reserve(world);
    UC_HIP(hipMemsetAsync(cnt.p, 0, (size_t)world * 8, stream));
    hipLaunchKernelGGL(owner_key_kernel, grid_for(n_hits), dim3(256), 0, stream, n_hits, d_hq.p, d_ht.p, ddb.len, world, okey.p, idx.p, cnt.p);
    unsigned bits = 1;
    while ((1u << bits) < world) bits++;
    rocprim_call(pre->shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, okey.p, okey2.p, idx.p, idx2.p, (size_t)n_hits, 0u, bits, stream); });
    hipLaunchKernelGGL(owner_gather_kernel, grid_for(n_hits), dim3(256), 0, stream, n_hits, idx2.p, d_hq.p, d_ht.p, d_hs.p, d_hd.p, dq, dt, ds, dd);
    std::vector<unsigned long long> hc(world);
    UC_HIP(hipMemcpyAsync(hc.data(), cnt.p, (size_t)world * 8, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
    for (uint32_t w = 0; w < world; w++) counts[w] = hc[w];
}

uint64_t Engine::import_hits_dev(uint64_t n_in, const uint32_t *dq, const uint32_t *dt, const int32_t *ds, const int32_t *dd,
                                 uint32_t rank, uint32_t world) {
    return merge_hits_dev(0, nullptr, nullptr, nullptr, nullptr, n_in, dq, dt, ds, dd, false, rank, world);
}

// The union of two record lists, merged per query under the frozen order (score desc, target asc), truncated to max_seqs and installed.  List 1 is
// ALREADY in key order (a running top-M accumulator, i.e. the output of an earlier merge or a grouped pass); list 2 is sorted here unless the caller says
// it is in key order as well.  r06: the chunk loop (prefilter_chunks) used to radix-sort accumulator + chunk after every pass - at nominal configs[3] the
// accumulator of up to max_seqs x queries records went through ~7 sort passes (~170 B of traffic per record) once per target chunk, 8.9 s of the call.
// Now only the chunk's records are sorted and the two runs are merged (one read + one write of every record); the result is the stable sort's, record for record
// (the passes' candidate sets are disjoint, so no two keys are equal; rocprim::merge takes list 1 first on ties, as the stable sort of the concatenation did).
uint64_t Engine::merge_hits_dev(uint64_t n1, const uint32_t *q1, const uint32_t *t1, const int32_t *s1, const int32_t *d1,
                                uint64_t n2, const uint32_t *q2, const uint32_t *t2, const int32_t *s2, const int32_t *d2, bool sorted2,
                                uint32_t rank, uint32_t world) {
    PressureScope ps(*this, 0);
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    UC_HIP(hipSetDevice(device));
    const uint32_t n = hdb.n;
    if (n > (1u << 24)) fail(UC_ERR_GENERIC, "hits_import_dev: %u sequences exceed the 2^24 limit of the hit keys", n);
    hit_cnt.assign(n, 0);
    hit_off.assign((size_t)n + 1, 0);
    n_hits = 0;
    alns_valid = false;
    clear_edges();
    const uint64_t n_in = n1 + n2;
    if (!n_in) return 0;
    Timer tm;
    timed_ms_begin();
    // work buffers from the engine's prefilter scratch: a chunked or sharded run merges once per chunk / shard, and allocating
    // ~50 B per record anew every time was most of the merge time at 10^9 records
    if (!pre) pre = ParkedScratch<PrefilterScratch>::take_or_new(device);
    DevBuf<uint64_t> &skey = pre->sel.d_skey, &skey2 = pre->sel.d_skey2, &pos = pre->sel.d_pos;
    DevBuf<int32_t> &cd2 = pre->sel.d_cd2, &mval = pre->merge.d_mval;
    DevBuf<uint32_t> &flag = pre->sel.d_flag;
    DevBuf<uint32_t> bad;
    DevBuf<char> &tmp = pre->shared.d_temp;
    // the merge path (rocprim::merge partitions with 32-bit indices) - UC_MERGE_SORTED=0 keeps the plain sort of everything for A/B runs
    static const bool merge_ok = [] { const char *e = getenv("UC_MERGE_SORTED"); return !(e && atoi(e) == 0); }();
    const bool merging = n1 > 0 && n2 > 0 && merge_ok && n_in < (1ull << 32) - (1ull << 20);
    const bool presorted = n1 > 0 && n2 == 0 && merge_ok;              // nothing to add: only truncation / ownership / counts
    skey.reserve(n_in); flag.reserve(n_in); pos.reserve(n_in); bad.reserve(1);
    UC_HIP(hipMemsetAsync(bad.p, 0, 4, stream));
    if (n1) hipLaunchKernelGGL(merge_key_kernel, grid_for(n1), dim3(256), 0, stream, n1, q1, t1, s1, n, skey.p, bad.p);
    if (n2) hipLaunchKernelGGL(merge_key_kernel, grid_for(n2), dim3(256), 0, stream, n2, q2, t2, s2, n, skey.p + n1, bad.p);
    unsigned kb = 33;                              // [query | 255 - score : 8 | target : 24]: the query field ends at bit 32 + log2 n
    while (kb < 64 && (1ull << (kb - 32)) < n) kb++;
    const uint64_t *sk = nullptr;                  // the sorted keys and their diagonals
    const int32_t *sd = nullptr;
    if (presorted) { sk = skey.p; sd = d1; }
    else if (merging) {
        const uint64_t *k2 = skey.p + n1;
        const int32_t *v2 = d2;
        if (!sorted2) {
            skey2.reserve(n2); cd2.reserve(n2);
            rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, skey.p + n1, skey2.p, d2, cd2.p, (size_t)n2, 0u, kb, stream); });
            k2 = skey2.p; v2 = cd2.p;
        }
        DevBuf<uint64_t> &mkey = pre->merge.d_mkey;
        mkey.reserve(n_in); mval.reserve(n_in);
        rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::merge(t, b, skey.p, k2, mkey.p, d1, v2, mval.p, (size_t)n1, (size_t)n2, rocprim::less<uint64_t>(), stream); });
        sk = mkey.p; sd = mval.p;
    } else {
        // one list (or the A/B switch): the diagonals of the two inputs have to be one array for the pair sort
        const int32_t *dd = n1 ? nullptr : d2;
        skey2.reserve(n_in); cd2.reserve(n_in);
        if (n1) {
            mval.reserve(n_in);
            UC_HIP(hipMemcpyAsync(mval.p, d1, n1 * 4, hipMemcpyDeviceToDevice, stream));
            if (n2) UC_HIP(hipMemcpyAsync(mval.p + n1, d2, n2 * 4, hipMemcpyDeviceToDevice, stream));
            dd = mval.p;
        }
        rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, skey.p, skey2.p, dd, cd2.p, (size_t)n_in, 0u, kb, stream); });
        sk = skey2.p; sd = cd2.p;
    }
    hipLaunchKernelGGL(rank_flag_kernel, grid_for(n_in), dim3(256), 0, stream, sk, n_in, (uint32_t)p.max_seqs, flag.p);
    if (world > 1) hipLaunchKernelGGL(owner_flag_kernel, grid_for(n_in), dim3(256), 0, stream, sk, n_in, ddb.len, rank, world, flag.p);
    uint32_t hbad = 0;
    const uint64_t keep = compact_u64(*this, tmp, flag.p, pos.p, n_in, bad.p, &hbad);
    if (hbad) fail(UC_ERR_ARGS, "hits_import_dev: %u records with a sequence id or score out of range", hbad);
    if (keep) {
        // (list 1 or 2 may BE the engine's own arrays: the scatter reads only keys and the sorted diagonals, never q / t / s / d of the inputs - but the
        // diagonals of a presorted or merged input are read from d1 / d2 themselves, so the output must not overwrite them in place)
        const bool alias = (sd == d1 && d1 == d_hd.p) || (sd == d2 && d2 == d_hd.p);
        if (alias) {
            mval.reserve(n_in);
            UC_HIP(hipMemcpyAsync(mval.p, sd, n_in * 4, hipMemcpyDeviceToDevice, stream));
            sd = mval.p;
        }
        d_hq.reserve(keep); d_ht.reserve(keep); d_hs.reserve(keep); d_hd.reserve(keep);
        hipLaunchKernelGGL(hit_scatter_kernel, grid_for(n_in), dim3(256), 0, stream, sk, sd, n_in, flag.p, pos.p, d_hq.p, d_ht.p, d_hs.p, d_hd.p);
        n_hits = keep;
    }
    finish_hit_lists("hits_import_dev");
    UC_HIP(hipGetLastError());
    stats.prefilter_kernel_ms += timed_ms_end();
    stats.stage_seconds[UC_ST_SELECT] += tm.seconds();
    return keep;
}

// E3 and the key pass of E4 on an explicit candidate list, with the launches of rescore_ungapped / select_and_append: the scores, the overlap residues
// that E3 adds to the stage's algorithmic bytes and the number of candidates E4 keeps (score >= min_score)
void Engine::ungapped_select(uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *diag, int min_score, int32_t *score_out,
                             uint64_t *overlap_out, uint64_t *kept_out) {
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    *overlap_out = 0; *kept_out = 0;
    if (n == 0) return;
    UC_HIP(hipSetDevice(device));
    for (uint64_t i = 0; i < n; i++)
        if (q[i] >= hdb.n || t[i] >= hdb.n) fail(UC_ERR_ARGS, "ungapped_select: sequence id out of range");
    DevBuf<uint32_t> dq, dt;
    DevBuf<int32_t> dd, ds;
    DevBuf<uint64_t> key;
    DevBuf<unsigned long long> ctr;
    dq.reserve(n); dt.reserve(n); dd.reserve(n); ds.reserve(n); key.reserve(n); ctr.reserve(2);
    UC_HIP(hipMemcpyAsync(dq.p, q, n * 4, hipMemcpyHostToDevice, stream));
    UC_HIP(hipMemcpyAsync(dt.p, t, n * 4, hipMemcpyHostToDevice, stream));
    UC_HIP(hipMemcpyAsync(dd.p, diag, n * 4, hipMemcpyHostToDevice, stream));
    UC_HIP(hipMemsetAsync(ctr.p, 0, 16, stream));
    launch_ungapped(ddb, n, dq.p, dt.p, dd.p, ds.p, ctr.p, stream);
    hipLaunchKernelGGL(select_key_kernel, grid_for(n, count_grid_cap), dim3(256), 0, stream, n, dq.p, dt.p, ds.p, min_score, key.p, ctr.p + 1);
    UC_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    UC_HIP(hipMemcpyAsync(h, ctr.p, 16, hipMemcpyDeviceToHost, stream));
    if (score_out) UC_HIP(hipMemcpyAsync(score_out, ds.p, n * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    *overlap_out = h[0]; *kept_out = h[1];
}

void preload_hit_lists_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)select_key_kernel); }
}  // namespace uc
