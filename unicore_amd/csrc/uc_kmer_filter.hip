// uc_kmer_filter.hip - prefilter stage E2 from the run lists to the surviving hit keys.
// Consumes the plan of the batch's super-batch (plan_superbatch, uc_kmer_match.hip: the sorted run lists of the distinct k-mers, per query position where
// its list starts and the running sum of the list lengths, per query its hits and runs) and the chunk's index entries.  There is no per-position copy
// of the runs: run r of a query belongs to the last position whose run prefix is <= r and is read from that position's list (FILTER_PW below).
// Produces the batch's (query, target, diagonal) keys, dense and sorted (QueryBatch::sorted / n_sort).  With min_diag_hits >= 2 (expand_keys_filtered) one
// workgroup per query expands the query's runs through the double-hit filter in LDS (filter_kernel: two Bloom bitmaps, two levels) and only the keys that
// share (target, diagonal) with another hit survive; queries of at most td_cap survivors are then sorted and evaluated on chip at once (launch_td_select,
// uc_diag_select.hip) and leave their candidates in their regions, the rest is compacted and radix-sorted for select_diagonals.  Otherwise
// (expand_keys_plain) every hit becomes a key (expand_kernel).  spec UC-1 E2; DESIGN.md 4.3.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "uc_prefilter_internal.h"

namespace uc {

// one index entry -> (global target id, position)
template <bool C>
__device__ __forceinline__ void ent_decode(const void *ent, uint32_t idx, const KeyFmt &fmt, uint32_t &t, uint32_t &pos) {
    if (C) {
        const uint32_t e = ((const uint32_t *)ent)[idx];
        t = (e >> (fmt.dbits - 1)) + fmt.tbase;
        pos = e & ((1u << (fmt.dbits - 1)) - 1u);
    } else {
        const uint64_t e = ((const uint64_t *)ent)[idx];
        t = (uint32_t)(e >> 16);
        pos = (uint32_t)(e & 0xFFFF);
    }
}

// ---- E2 pass 2: expand runs into hit keys, load-balanced ----
// A workgroup takes 256 runs, scans their lengths, reserves the tile's key range with one atomic and then lets
// thread k write key k of the tile (binary search in the LDS prefix): loads of index entries touch a handful of
// lines per wave and the key stores are fully coalesced.
__global__ void __launch_bounds__(256) expand_kernel(const DeviceDb db, uint32_t qbegin, uint32_t qend, uint32_t P0, uint32_t b0, uint32_t b1,
                                                     const uint32_t *src, const uint64_t *cumr, const uint64_t *drv, uint64_t n_runs, const void *ent,
                                                     KeyFmt fmt, unsigned long long *key_cursor, uint64_t *keys, uint64_t key_cap) {
    __shared__ uint64_t s_pref[257];
    __shared__ uint64_t s_qb[256];
    __shared__ uint32_t s_e0[256];
    __shared__ int32_t s_i[256];
    __shared__ uint64_t s_wsum[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t rbase = cumr[b0];
    for (uint64_t tile = blockIdx.x; tile * 256 < n_runs; tile += gridDim.x) {
        const uint64_t r = tile * 256 + tid;
        uint64_t c = 0;
        if (r < n_runs) {
            // the run's position: the last one of the batch [b0, b1) whose run prefix is <= r (a position without runs shares its prefix with the next
            // one and is never the last); the run itself lies where the plan left it, in the list of the position's k-mer
            uint32_t lo = b0, hi = b1;
            while (hi - lo > 1) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (cumr[mid] - rbase <= r) lo = mid; else hi = mid;
            }
            const uint64_t rv = drv[src[lo] + (uint32_t)(r - (cumr[lo] - rbase))];
            c = rv >> 32;
            const uint32_t p = P0 + lo;
            const uint32_t s = find_seq(db.off, qbegin, qend, p);
            s_e0[tid] = (uint32_t)rv;
            s_i[tid] = (int32_t)(p - db.off[s]) + fmt.dbias;
            s_qb[tid] = (uint64_t)(s - qbegin) << (fmt.tbits + fmt.dbits);
        }
        uint64_t inc = c;   // inclusive scan inside the wave, then across the 4 waves
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) s_wsum[wv] = inc;
        __syncthreads();
        uint64_t woff = 0;
        for (int w = 0; w < wv; w++) woff += s_wsum[w];
        s_pref[tid] = woff + inc - c;
        if (tid == 255) {
            const uint64_t total = woff + inc;
            s_pref[256] = total;
            s_base = total ? atomicAdd(key_cursor, (unsigned long long)total) : 0ull;
        }
        __syncthreads();
        const uint64_t total = s_pref[256], base = s_base;
        for (uint64_t k = tid; k < total; k += 256) {
            int lo = 0, hi = 256;          // last run with pref <= k
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pref[mid] <= k) lo = mid; else hi = mid;
            }
            uint32_t et, epos;
            if (fmt.compact) ent_decode<true>(ent, s_e0[lo] + (uint32_t)(k - s_pref[lo]), fmt, et, epos);
            else ent_decode<false>(ent, s_e0[lo] + (uint32_t)(k - s_pref[lo]), fmt, et, epos);
            const uint64_t key = s_qb[lo] | ((uint64_t)et << fmt.dbits) | (uint64_t)(s_i[lo] - (int32_t)epos);
            if (base + k < key_cap) keys[base + k] = key;
        }
        __syncthreads();
    }
}

// ---- E2 pass 2 (min_diag_hits >= 2): expand + double-hit filter, one workgroup per query ----
// Only hits that share (target, diagonal) with another hit of the same query can make a candidate, and they are a
// few percent of all hits.  With the runs sorted by query position a workgroup owns one query:
//   sweep 1 expands the query's runs (load-balanced: thread k takes KPT consecutive keys of the tile by one binary
//           search in the LDS prefix of the run lengths), records every (target, diagonal) hash in two LDS bitmaps
//           (seen once / seen twice, two hash positions per key) and STREAMS the (target, diagonal) keys it computed
//           into the query's region of the key buffer (coalesced 16-byte stores);
//   sweep 2 reads that stream back — a coalesced scan instead of a second round of binary searches and index gathers
//           (the gathers were the kernel's critical path: 69 % of its cycles waited on them, profiles/r2b) — keeps the
//           keys whose two hash positions were both seen twice, and compacts them in place;
//   level 2 repeats the once/twice test over the survivors alone with independent hash functions (below).
// Every key of a real multi-hit diagonal survives, plus a few collisions which the exact diagonal count after the sort
// discards again.  The region is sized by the query's exact hit total (from sim_runs), so nothing can overflow.
constexpr int FB_LOG2 = 19;            // bits per bitmap: 2 x 64 KiB of the CU's 160 KiB LDS
constexpr int FT = 1024;               // threads per workgroup
constexpr int KPT = 4;                 // consecutive keys per thread and binary search
// runs per tile = RPT x FT.  RPT = 2 (r4): half as many tile hand-overs (three workgroup barriers and the drain of 16 waves each) per
// query; the prefix search takes 11 probes instead of 10
constexpr int FILTER_RPT = 2;
// The filter reads a query's runs where the plan left them (plan_superbatch, uc_kmer_match.hip): run r of the query belongs to the last position whose run
// prefix (d_cumr, relative to the query's first position) is <= r, and is entry r - prefix of the list of that position's k-mer (d_src into d_drv2).  The
// prefix is staged in LDS once per workgroup so that finding a position costs no global load: FILTER_PW entries of prefix and list start are what fits
// beside the bitmaps and the tile (160 KiB - filter_lds(RPT) < 100 B).  A query of at most FILTER_PW positions - nearly every protein - holds all of them and
// a tile's runs cost one dependent global load, as they did when they were read from a copy.  A longer query keeps every 2^sh-th prefix entry, and a run
// then takes sh probes of d_cumr and one load of d_src on top (L2 hits: a tile spans few positions): these queries have tens of tiles of ~40 us each,
// behind whose expansion the next tile's fetch runs, and searching d_cumr alone would put ~10-16 such probes before every tile of EVERY query.
constexpr int FILTER_PW = 1000;
constexpr size_t filter_lds(int rpt) {
    return 2 * ((size_t)1 << FB_LOG2) / 8 + ((size_t)rpt * FT + 1) * 4 + (size_t)rpt * FT * 8 + 16 * 4 + 64 + ((size_t)FILTER_PW + 1) * 4 + (size_t)FILTER_PW * 4;
}
static_assert(filter_lds(FILTER_RPT) <= 160 * 1024, "filter_kernel: one workgroup must fit the CU's LDS");

// launch order of the filter workgroups: queries with the most runs first (longest-processing-time-first: a batch then ends
// with many short queries instead of a few long ones; the tail was ~20 % of the kernel).  qrn: the plan's runs per query, from the batch's first query on
__global__ void __launch_bounds__(256) run_order_key_kernel(uint32_t nq, const uint64_t *qrn, uint32_t *key, uint32_t *idx) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nq; i += gridDim.x * 256) {
        const uint64_t c = qrn[i];
        key[i] = 0xFFFFFFFFu - (uint32_t)min<uint64_t>(c, 0xFFFFFFFFull);
        idx[i] = i;
    }
}

template <bool C> struct TdType { using type = uint64_t; };
template <> struct TdType<true> { using type = uint32_t; };

// (Measured and removed, profiles/r03_filter_ab.log: 1024-run tiles — 2.5 % slower; a blocked Bloom filter with both hash positions of a key in one
// 64-bit LDS word, one ds_or_rtn_b64 instead of two dependent 32-bit atomic pairs — no gain: the kernel is not bound by its LDS atomics.)
template <bool C>
__global__ void __launch_bounds__(FT) filter_kernel(const DeviceDb db, uint32_t qbegin, uint32_t P0, const uint32_t *psrc, const uint64_t *cumr,
                                                    const uint64_t *drv, const uint64_t *qh, const uint32_t *order, const void *ent, KeyFmt fmt,
                                                    unsigned long long *region_cursor, void *region_v, uint64_t region_cap,
                                                    uint64_t *qbase, uint32_t *qsurv) {
    using TD = typename TdType<C>::type;
    struct __attribute__((aligned(4))) TD4 { TD v[KPT]; };        // KPT keys of one thread: dword-aligned vector access
    TD *region = (TD *)region_v;
    extern __shared__ __attribute__((aligned(16))) uint32_t f_lds[];
    constexpr int BW = 1 << (FB_LOG2 - 5);          // words per bitmap
    constexpr int RPT = FILTER_RPT;
    constexpr int TR = RPT * FT;                    // runs per tile
    uint32_t *B1 = f_lds, *B2 = f_lds + BW;
    uint2 *s_run = (uint2 *)(f_lds + 2 * BW);                   // TR: {first index entry - prefix, query position + bias}: ONE 8-byte read per key
    uint32_t *s_pref = (uint32_t *)(s_run + TR);                // TR + 1 (hits of one query < 2^32: checked by the host)
    uint32_t *s_wsum = s_pref + TR + 1;                         // 16
    uint64_t *s_misc = (uint64_t *)(((uintptr_t)(s_wsum + 16) + 7) & ~(uintptr_t)7);   // [2] region base, [3] cursors (2 x u32)
    uint32_t *s_pp = (uint32_t *)(s_misc + 4);                  // FILTER_PW + 1: run prefix of every 2^sh-th position of the query (runs of one query < 2^32)
    uint32_t *s_src = s_pp + FILTER_PW + 1;                     // FILTER_PW: where the run list of position i starts in drv (sh == 0 only)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t qi = order[blockIdx.x];                      // query of this workgroup (index inside the batch)
    const uint32_t q = qbegin + qi;
    const uint32_t pq = db.off[q] - P0, L = db.off[q + 1] - db.off[q];     // the query's positions in the plan: [pq, pq + L)
    const uint64_t c0 = cumr[pq];
    const uint64_t r0 = 0, r1 = cumr[pq + L] - c0;              // its runs, counted from its first one
    TD *surv = region + region_cap;                             // second area of the same size: survivors of sweep 2
    for (int w = tid; w < 2 * BW; w += FT) f_lds[w] = 0;
    if (r0 == r1) {
        if (tid == 0) { qbase[qi] = 0; qsurv[qi] = 0; }
        return;
    }
    // the position prefix (comment at FILTER_PW): ns samples, one per 2^sh positions
    int sh = 0;
    while (((L + (1u << sh) - 1) >> sh) > (uint32_t)FILTER_PW) sh++;
    const int ns = (int)((L + (1u << sh) - 1) >> sh);
    for (int i = tid; i < ns; i += FT) {
        s_pp[i] = (uint32_t)(cumr[pq + ((uint32_t)i << sh)] - c0);
        if (sh == 0) s_src[i] = psrc[pq + i];
    }

    // loads one tile of runs, leaves the exclusive prefix of their lengths in s_pref[0..FT] (s_pref[FT] = total)
    // the run of the NEXT tile is fetched while the current one is expanded (the loads' latency would otherwise sit between
    // two barriers with nothing else to run: one workgroup per CU)
    uint64_t pf_rv[RPT] = {};
    uint32_t pf_pi[RPT] = {};
    auto prefetch_tile = [&](uint64_t tile) {      // thread tid owns runs tile + RPT * tid .. + RPT - 1 (consecutive: the prefix stays a plain scan)
        // the last sample whose prefix is <= r: a position without runs has the prefix of the one behind it and is never the last.  One search for the
        // thread's first run; the following ones are in the same sample or a few further on
        int lo = 0, hi = ns;
        if (tile + (uint64_t)RPT * tid < r1)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pp[mid] <= (uint32_t)(tile + (uint64_t)RPT * tid)) lo = mid; else hi = mid;
            }
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const uint64_t r = tile + (uint64_t)RPT * tid + j;
            if (r < r1) {
                if (j) while (lo + 1 < ns && s_pp[lo + 1] <= (uint32_t)r) lo++;
                uint32_t pos = (uint32_t)lo << sh, pre = s_pp[lo], first;
                if (sh) {                          // ... and the last position of that sample's 2^sh
                    uint32_t phi = min(pos + (1u << sh), L);
                    while (phi - pos > 1) {
                        const uint32_t mid = pos + ((phi - pos) >> 1), v = (uint32_t)(cumr[pq + mid] - c0);
                        if (v <= (uint32_t)r) { pos = mid; pre = v; } else phi = mid;
                    }
                    first = psrc[pq + pos];
                } else first = s_src[pos];
                pf_rv[j] = drv[first + ((uint32_t)r - pre)];
                pf_pi[j] = pos;                    // position inside the query
            }
        }
    };
    auto load_tile = [&](uint64_t tile) {
        uint32_t c[RPT], csum = 0;
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const uint64_t r = tile + (uint64_t)RPT * tid + j;
            c[j] = r < r1 ? (uint32_t)(pf_rv[j] >> 32) : 0u;
            csum += c[j];
        }
        uint32_t inc = csum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) s_wsum[wv] = inc;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wv; w++) woff += s_wsum[w];
        uint32_t pre = woff + inc - csum;
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            s_pref[RPT * tid + j] = pre;
            s_run[RPT * tid + j] = make_uint2((uint32_t)pf_rv[j] - pre, (uint32_t)((int32_t)pf_pi[j] + fmt.dbias));
            pre += c[j];
        }
        if (tid == FT - 1) s_pref[TR] = pre;
        __syncthreads();
    };
    // keys k4 .. k4+KPT-1 of the current tile: one binary search finds the run of the first key; every run holds at least
    // one key, so each following key is in the same run or the next one (a branch-free step).  locate() is pure LDS work
    // with a fixed trip count, so the two groups a thread handles per iteration interleave and their 2 x KPT index loads
    // are in flight together (the kernel is bound by the latency of search -> gather -> mark, one workgroup per CU).
    auto locate = [&](uint32_t k4, uint32_t T, uint32_t (&idx)[KPT], int32_t (&si)[KPT]) -> int {
        int lo = 0;
#pragma unroll
        for (int step = TR / 2; step >= 1; step >>= 1)            // TR = 2^10 / 2^11: ten / eleven probes
            if (s_pref[lo + step] <= k4) lo += step;
        const int n = k4 >= T ? 0 : (T - k4 < (uint32_t)KPT ? (int)(T - k4) : KPT);
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            if (i > 0 && i < n) lo += (s_pref[lo + 1] <= k4 + i) ? 1 : 0;
            const uint2 rr = s_run[lo];
            idx[i] = rr.x + (k4 + i);
            si[i] = (int32_t)rr.y;
        }
#pragma unroll
        for (int i = 1; i < KPT; i++) if (i >= n) { idx[i] = idx[0]; si[i] = si[0]; }
        return n;
    };
    auto gather = [&](const uint32_t (&idx)[KPT], typename std::conditional<C, uint32_t, uint64_t>::type (&e)[KPT]) {
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            if (C) e[i] = ((const uint32_t *)ent)[idx[i]];
            else e[i] = ((const uint64_t *)ent)[idx[i]];
        }
    };
    auto to_td = [&](const typename std::conditional<C, uint32_t, uint64_t>::type (&e)[KPT], const int32_t (&si)[KPT], TD (&td)[KPT]) {
        const uint32_t pm = (1u << (fmt.dbits - 1)) - 1u;
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            if (C) td[i] = (TD)((((uint32_t)e[i] >> (fmt.dbits - 1)) << fmt.dbits) | (uint32_t)(si[i] - (int32_t)((uint32_t)e[i] & pm)));
            else td[i] = (TD)((((uint64_t)e[i] >> 16) << fmt.dbits) | (uint64_t)(si[i] - (int32_t)((uint64_t)e[i] & 0xFFFF)));
        }
    };
    // two independent hash positions per (target, diagonal): a key survives only if BOTH were seen twice (a Bloom
    // filter with k = 2: collisions let ~2 % of the single hits through instead of ~11 %, which is what the sort pays for)
    auto slot_of = [&](uint64_t td, uint32_t &h2) -> uint32_t {
        const uint32_t x = (uint32_t)td * 0x9E3779B1u ^ (uint32_t)(td >> 32) * 0x85EBCA6Bu;
        h2 = ((x ^ (x >> 15)) * 0x846CA68Bu) >> (32 - FB_LOG2);
        return (x * 0x2C1B3C6Du) >> (32 - FB_LOG2);
    };
    auto mark1 = [&](uint64_t td) {
        uint32_t g;
        const uint32_t h = slot_of(td, g), bit = 1u << (h & 31), gbit = 1u << (g & 31);
        const uint32_t old = atomicOr(&B1[h >> 5], bit);
        if (old & bit) atomicOr(&B2[h >> 5], bit);
        const uint32_t gold = atomicOr(&B1[g >> 5], gbit);
        if (gold & gbit) atomicOr(&B2[g >> 5], gbit);
    };
    auto twice1 = [&](uint64_t td) -> uint32_t {
        uint32_t g;
        const uint32_t h = slot_of(td, g);
        return ((B2[h >> 5] >> (h & 31)) & (B2[g >> 5] >> (g & 31))) & 1u;
    };

    // the query's region: its exact hit total is the plan's (d_qh); reserve it first (rounded up to KPT keys).  The barrier also publishes the prefix
    if (tid == 0) {
        s_misc[2] = atomicAdd(region_cursor, (unsigned long long)((qh[qi] + KPT - 1) / KPT * KPT));
        ((uint32_t *)&s_misc[3])[0] = 0;
        ((uint32_t *)&s_misc[3])[1] = 0;
    }
    __syncthreads();
    const uint64_t base = s_misc[2];
    uint32_t *cur = (uint32_t *)&s_misc[3];
    uint32_t total = 0;
    prefetch_tile(r0);
    for (uint64_t tile = r0; tile < r1; tile += TR) {
        load_tile(tile);
        // the next tile's fetch starts behind the first gathers of this one: its search in the LDS prefix (~10 dependent reads) then runs while the
        // index entries are on their way, instead of between the barrier and the first gather
        bool fetched = false;
        const uint32_t T = s_pref[TR];
        using ET = typename std::conditional<C, uint32_t, uint64_t>::type;
        auto mark_store = [&](TD4 &td, int n, uint32_t k4) {
#pragma unroll
            for (int i = 0; i < KPT; i++) {
                if (i >= n) { td.v[i] = td.v[0]; continue; }
                mark1(td.v[i]);
            }
            const uint64_t w = base + total + k4;
            if (n && w + KPT <= region_cap) {
                if (n == KPT) *(TD4 *)(region + w) = td;
                else {
#pragma unroll
                    for (int i = 0; i < KPT; i++) if (i < n) region[w + i] = td.v[i];     // (a runtime trip count would put td into scratch)
                }
            }
        };
        for (uint32_t k4 = (uint32_t)KPT * tid; k4 < T; k4 += 2u * KPT * FT) {
            const uint32_t k4b = k4 + (uint32_t)KPT * FT;
            uint32_t ia[KPT], ib[KPT];
            int32_t sa[KPT], sb[KPT];
            const int na = locate(k4, T, ia, sa);
            const int nb = locate(k4b < T ? k4b : k4, T, ib, sb);
            ET ea[KPT], eb[KPT];
            gather(ia, ea);
            gather(ib, eb);
            if (!fetched) { prefetch_tile(tile + TR); fetched = true; }
            TD4 ta, tb;
            to_td(ea, sa, ta.v);
            mark_store(ta, na, k4);
            to_td(eb, sb, tb.v);
            mark_store(tb, k4b < T ? nb : 0, k4b);
        }
        if (!fetched) prefetch_tile(tile + TR);      // (a thread without a key in this tile)
        total += T;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // sweep 2: stream the keys back, keep those whose two positions were both seen twice and append them to the query's
    // slice of the survivor area (same offsets as its region): no barrier and no in-place hazard, so the loads of successive
    // iterations overlap.
    const uint32_t n0 = (uint32_t)min<uint64_t>(total, region_cap > base ? region_cap - base : 0);
    const uint32_t n0r = n0;                 // (a wave's lanes enter the loop together: their k4 differ by < 64 * KPT <= the loop stride; the ballots below only need the lanes that are in)
    for (uint32_t k4 = (uint32_t)KPT * tid; k4 < n0r; k4 += 2u * KPT * FT) {
        // two groups of KPT keys per thread and iteration: both loads are in flight before either is tested
        TD4 td[2] = {};
        int nn[2];
#pragma unroll
        for (int g2 = 0; g2 < 2; g2++) {
            const uint32_t k = k4 + (uint32_t)g2 * KPT * FT;
            nn[g2] = k >= n0 ? 0 : (n0 - k < (uint32_t)KPT ? (int)(n0 - k) : KPT);
            if (nn[g2] == KPT) td[g2] = *(const TD4 *)(region + base + k);
            else {
#pragma unroll
                for (int i = 0; i < KPT; i++) if (i < nn[g2]) td[g2].v[i] = region[base + k + i];
            }
        }
        uint32_t keep = 0;                      // bit 4 * g2 + i: key i of group g2 survives
#pragma unroll
        for (int g2 = 0; g2 < 2; g2++)
#pragma unroll
            for (int i = 0; i < KPT; i++)
                if (i < nn[g2]) keep |= twice1(td[g2].v[i]) << (KPT * g2 + i);
        // wave-level compaction by ballots (the order of the survivors is irrelevant: they get sorted): rank of key j of
        // this lane = survivors of keys < j over the whole wave + survivors of key j in the lanes below
        uint32_t rank[2 * KPT];
        uint32_t wave_total = 0;
#pragma unroll
        for (int j = 0; j < 2 * KPT; j++) {
            const uint64_t m = __builtin_amdgcn_ballot_w64((keep >> j) & 1u);
            rank[j] = wave_total + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            wave_total += (uint32_t)__popcll(m);
        }
        if (wave_total) {
            uint32_t s0 = 0;
            if (lane == 0) s0 = atomicAdd(cur, wave_total);
            s0 = (uint32_t)__shfl((int)s0, 0, 64);
#pragma unroll
            for (int j = 0; j < 2 * KPT; j++)
                if ((keep >> j) & 1u) surv[base + s0 + rank[j]] = td[j / KPT].v[j % KPT];
        }
    }
    // ---- second level: the same once / twice test over the SURVIVORS only, with independent hash functions ----
    // Long queries load the bitmaps so heavily that most first-level survivors are single hits whose two positions were
    // set by other keys (C2: 0.55 G survivors for ~0.03 G keys of real double-hit diagonals).  Every key of a diagonal with
    // >= 2 hits survives level 1 together with its twins, so repeating the test over the ~10x shorter survivor list (a
    // coalesced read of the query's own slice, no index lookups) keeps all of them and drops nearly all the rest; the final
    // keys go back to the head of the query's region.
    __threadfence_block();
    __syncthreads();
    const uint32_t n1 = *cur;
    for (int w = tid; w < 2 * BW; w += FT) f_lds[w] = 0;
    uint32_t *cur2 = cur + 1;
    __syncthreads();
    auto slot2_of = [&](uint64_t key, uint32_t &h2) -> uint32_t {
        const uint32_t x = (uint32_t)key * 0xC2B2AE35u ^ (uint32_t)(key >> 32) * 0x27D4EB2Fu;
        h2 = ((x ^ (x >> 13)) * 0x165667B1u) >> (32 - FB_LOG2);
        return (x * 0x9E3779B1u) >> (32 - FB_LOG2);
    };
    for (uint32_t k = tid; k < n1; k += FT) {
        uint32_t g;
        const uint32_t h = slot2_of(surv[base + k], g), bit = 1u << (h & 31), gbit = 1u << (g & 31);
        const uint32_t old = atomicOr(&B1[h >> 5], bit);
        if (old & bit) atomicOr(&B2[h >> 5], bit);
        const uint32_t gold = atomicOr(&B1[g >> 5], gbit);
        if (gold & gbit) atomicOr(&B2[g >> 5], gbit);
    }
    __syncthreads();
    const uint32_t n1r = (n1 + 63) / 64 * 64;
    for (uint32_t k = tid; k < n1r; k += FT) {
        TD key = 0;
        bool keep = false;
        if (k < n1) {
            key = surv[base + k];
            uint32_t g;
            const uint32_t h = slot2_of(key, g);
            keep = ((B2[h >> 5] >> (h & 31)) & (B2[g >> 5] >> (g & 31))) & 1u;
        }
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        if (m) {
            uint32_t s0 = 0;
            if (lane == 0) s0 = atomicAdd(cur2, (uint32_t)__popcll(m));
            s0 = (uint32_t)__shfl((int)s0, 0, 64);
            if (keep) region[base + s0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = key;
        }
    }
    __syncthreads();
    if (tid == 0) { qbase[qi] = base; qsurv[qi] = *cur2; }
}

// moves every query's surviving (target, diagonal) keys from its region to a dense array of full sort keys
// [ query - qbegin | target | diagonal + dbias ]
template <bool C>
__global__ void __launch_bounds__(256) compact_kernel(const void *region_v, const uint64_t *qbase, const uint32_t *qsurv,
                                                      const uint64_t *soff, uint32_t nq, KeyFmt fmt, uint64_t *out) {
    using TD = typename TdType<C>::type;
    const TD *region = (const TD *)region_v;
    const uint64_t dmask = (1ull << fmt.dbits) - 1;
    for (uint32_t b = blockIdx.x; b < nq; b += gridDim.x) {
        const uint64_t src = qbase[b], dst = soff[b];
        const uint32_t n = qsurv[b];
        const uint64_t qbits = (uint64_t)b << (fmt.tbits + fmt.dbits);
        for (uint32_t k = threadIdx.x; k < n; k += 256) {
            const uint64_t td = region[src + k];
            out[dst + k] = C ? (qbits | (((td >> fmt.dbits) + fmt.tbase) << fmt.dbits) | (td & dmask)) : (qbits | td);
        }
    }
}

// n > 0 counts (0/1 flags, survivors per query) -> their exclusive scan in u64 positions (where each entry's share goes) -> the total (one host
// synchronisation, the u64 form of uc_sw_plan.hip's compact(); it also fetches the u32 at `also` for a caller that has one more value to read)
uint64_t compact_u64(Engine &E, DevBuf<char> &tmp, uint32_t *cnt, uint64_t *pos, uint64_t n, const uint32_t *also, uint32_t *also_out) {
    auto in = rocprim::make_transform_iterator(cnt, WidenU32());
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, pos, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), E.stream); });
    uint64_t lp = 0; uint32_t lc = 0;
    UC_HIP(hipMemcpyAsync(&lp, pos + (n - 1), 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipMemcpyAsync(&lc, cnt + (n - 1), 4, hipMemcpyDeviceToHost, E.stream));
    if (also) UC_HIP(hipMemcpyAsync(also_out, also, 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    return lp + lc;
}

// pass 2 with the double-hit filter.  consumes the batch's runs; produces its keys that survive filter_kernel<C>, dense and sorted (B.sorted / n_sort)
void expand_keys_filtered(Engine &E, PrefilterPass &PP, QueryBatch &B) {
    PrefilterScratch &S = *E.pre;
    const KeyFmt &fmt = PP.fmt;
    const uint32_t qa = B.qa, nq = B.qb - B.qa;
    S.batch.d_qbase.reserve(nq); S.batch.d_qsurv.reserve(nq); S.batch.d_soff.reserve((size_t)nq + 1);
    // the query regions hold (target, diagonal) keys: u32 in compact mode (half of the u64 buffer stays unused),
    // every region rounded up to KPT keys
    const uint64_t region_cap = B.total_hits + (uint64_t)KPT * nq;
    S.batch.d_keys.reserve(fmt.compact ? region_cap : 2 * region_cap);       // regions + survivor area of the same size
    S.batch.d_okey.reserve(nq); S.batch.d_okey2.reserve(nq); S.batch.d_oidx.reserve(nq); S.batch.d_order.reserve(nq);
    hipLaunchKernelGGL(run_order_key_kernel, grid_for(nq), dim3(256), 0, E.stream, nq, S.plan.d_qrn.p + (qa - B.plan_q0), S.batch.d_okey.p, S.batch.d_oidx.p);
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, S.batch.d_okey.p, S.batch.d_okey2.p, S.batch.d_oidx.p, S.batch.d_order.p, (size_t)nq, 0u, 32u, E.stream); });
    auto launch = [&](auto kern) {
        static PerDeviceOnce once[2];
        once[fmt.compact ? 1 : 0]([&] { UC_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)filter_lds(FILTER_RPT))); });
        hipLaunchKernelGGL(kern, dim3(nq), dim3(FT), filter_lds(FILTER_RPT), E.stream, E.ddb, qa, B.plan_p0, S.plan.d_src.p, S.plan.d_cumr.p, S.plan.d_drv2.p, S.plan.d_qh.p + (qa - B.plan_q0), S.batch.d_order.p, PP.ent_p, fmt,
                           S.shared.d_counters.p + 5, (void *)S.batch.d_keys.p, region_cap, S.batch.d_qbase.p, S.batch.d_qsurv.p);
    };
    if (fmt.compact) launch(filter_kernel<true>);
    else launch(filter_kernel<false>);
    // queries of at most td_cap survivors are sorted and evaluated on chip (td_select_kernel); the batch sort below only sees the rest
    unsigned long long taken = 0;
    uint32_t last_rec = 0;
    const bool onchip = fmt.compact && PP.td_cap > 0;
    if (onchip) {
        S.cand.d_qcand.reserve(nq); S.cand.d_qmir.reserve(nq); S.cand.d_qrec.reserve(nq); S.cand.d_coff.reserve(nq);
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 7, 0, 8, E.stream));
        launch_td_select(E, PP, qa, nq);
        auto rin = rocprim::make_transform_iterator(S.cand.d_qrec.p, WidenU32());
        rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, rin, S.cand.d_coff.p, (uint64_t)0, (size_t)nq, rocprim::plus<uint64_t>(), E.stream); });
        // (fetched by the one synchronisation of the scan below)
        UC_HIP(hipMemcpyAsync(&B.n_rec, S.cand.d_coff.p + (nq - 1), 8, hipMemcpyDeviceToHost, E.stream));
        UC_HIP(hipMemcpyAsync(&taken, S.shared.d_counters.p + 7, 8, hipMemcpyDeviceToHost, E.stream));
    }
    const uint64_t n_sort = compact_u64(E, S.shared.d_temp, S.batch.d_qsurv.p, S.batch.d_soff.p, nq, onchip ? S.cand.d_qrec.p + (nq - 1) : nullptr, &last_rec);
    B.n_rec += last_rec;
    const uint64_t taken_keys = taken & ((1ull << 40) - 1);
    PP.td_queries += taken >> 40; PP.td_keys += taken_keys; PP.filt_queries += nq; PP.filt_keys += n_sort + taken_keys;
    E.td_onchip[0] += taken >> 40; E.td_onchip[1] += nq; E.td_onchip[2] += taken_keys; E.td_onchip[3] += n_sort + taken_keys;
    if (n_sort) {
        S.batch.d_keys2.reserve(2 * n_sort);              // dense keys + the sort's output
        hipLaunchKernelGGL(fmt.compact ? compact_kernel<true> : compact_kernel<false>, dim3(std::min<uint32_t>(nq, 65535u)), dim3(256), 0, E.stream,
                           (const void *)S.batch.d_keys.p, S.batch.d_qbase.p, S.batch.d_qsurv.p, S.batch.d_soff.p, nq, fmt, S.batch.d_keys2.p);
        rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, S.batch.d_keys2.p, S.batch.d_keys2.p + n_sort, (size_t)n_sort, 0u, B.kbits, E.stream); });
    }
    B.sorted = S.batch.d_keys2.p + n_sort; B.n_sort = n_sort;
    E.stats.n_filtered_hits += n_sort + taken_keys;
}

// pass 2 without the filter (min_diag_hits < 2, or a single query beyond 2^32 hits).  consumes the batch's runs; produces all its keys, sorted
void expand_keys_plain(Engine &E, PrefilterPass &PP, QueryBatch &B) {
    PrefilterScratch &S = *E.pre;
    S.batch.d_keys.reserve(B.total_hits); S.batch.d_keys2.reserve(B.total_hits);
    hipLaunchKernelGGL(expand_kernel, grid_for(B.n_runs), dim3(256), 0, E.stream, E.ddb, B.qa, B.qb, B.plan_p0, B.qp0 - B.plan_p0, B.qp1 - B.plan_p0,
                       S.plan.d_src.p, S.plan.d_cumr.p, S.plan.d_drv2.p, B.n_runs, PP.ent_p, PP.fmt,
                       S.shared.d_counters.p + 5, S.batch.d_keys.p, B.total_hits);
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, S.batch.d_keys.p, S.batch.d_keys2.p, (size_t)B.total_hits, 0u, B.kbits, E.stream); });
    B.sorted = S.batch.d_keys2.p; B.n_sort = B.total_hits;
    E.stats.n_filtered_hits += B.n_sort;
}

void preload_kmer_filter_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)run_order_key_kernel); }
}  // namespace uc
