// uc_diag_select.hip - prefilter stage E2 from the surviving hit keys to the candidates.
// Consumes a batch's sorted keys [query | target | diagonal] (uc_kmer_filter.hip) and, in compact mode, the query regions filter_kernel left behind.
// Produces the batch's candidates (query, target, best diagonal: most hits, then the smallest diagonal; in a symmetric pass also the pair the other way
// round) in cand.d_cq / d_ct / d_cd.  Two routes under one rule: diag_select_kernel / diag_long_kernel run-length-count the diagonals of the batch-sorted
// keys; td_select_kernel sorts a query's survivors in LDS right behind the filter (rocprim::block_radix_sort) and cand_gather_kernel collects what it
// left in the regions.  spec UC-1 E2; DESIGN.md 4.3.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_prefilter_internal.h"

namespace uc {

// one pass over the sorted hit keys: per (query,target) group the diagonals are run-length-counted and the best one
// (count desc, diagonal asc) is kept.  Candidates are staged per wave in LDS and
// appended in blocks of >= 64 behind one global atomic (one atomic per wave ballot serialised on a single
// address: +90 ms per step, profiles/r1g); their order is irrelevant (E4 sorts on a unique key).
//
// Symmetric passes (mirror_q0 < UINT32_MAX; Engine::prefilter, all-vs-all over several target chunks under a symmetric matrix): the k-mer hit
// relation is symmetric — query position i hits target position j iff S(kmer_q(i), kmer_t(j)) >= thr — so the hits of (t, q) are those of
// (q, t) with the diagonal negated.  A pass over target chunk c then only matches the queries from chunk c onwards, and every group (q, t)
// whose query lies BEHIND the chunk (q >= mirror_q0) also emits the candidate of the pair the other way round, (t, q), under ITS tie-break:
// most hits, then the smallest diagonal of (t, q) = the LARGEST diagonal of (q, t).
// Long groups: a sequence against itself (and close homologs) gives groups of hundreds to thousands of keys with one run — diagonal 0 — as long as
// the sequence; a lane walking such a group or run key by key (dependent loads) was the kernel's whole duration (~2.5 ms per launch at configs[1]
// whatever the other 99 % of the keys cost).  A group that covers the whole NEXT window is therefore only flagged here (wflag[window] = lane + 1)
// and evaluated by diag_long_kernel, a wave per long group; every serial walk left in this kernel is bounded by 64 keys.
__global__ void __launch_bounds__(256) diag_select_kernel(const uint64_t *keys, uint64_t n, int min_hits, KeyFmt fmt, uint32_t qbegin,
                                                          unsigned long long *n_cand, uint64_t cap,
                                                          uint32_t *cq, uint32_t *ct, int32_t *cd, uint32_t mirror_q0, uint8_t *wflag) {
    // candidates are staged per wave and appended behind ONE global cursor in blocks of >= 64 (a 512-entry stage was measured SLOWER, 16 vs 11 ms:
    // the appends are not what bounds the kernel — the serial walks of the long groups were, see below)
    constexpr int DS_SLOTS = 128, DS_DRAIN = 64;
    __shared__ uint32_t s_q[4][DS_SLOTS], s_t[4][DS_SLOTS];
    __shared__ int32_t s_d[4][DS_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t dmask = (1ull << fmt.dbits) - 1, tmask = (1ull << fmt.tbits) - 1;
    const uint64_t nround = (n + 255) / 256 * 256;   // whole waves stay in the loop (ballot below)
    uint32_t staged = 0;                             // wave-uniform
    auto drain = [&]() {
        uint32_t blo = 0, bhi = 0;
        if (lane == 0) {
            const unsigned long long b = atomicAdd(n_cand, (unsigned long long)staged);
            blo = (uint32_t)b; bhi = (uint32_t)(b >> 32);
        }
        blo = (uint32_t)__shfl((int)blo, 0, 64);
        bhi = (uint32_t)__shfl((int)bhi, 0, 64);
        const uint64_t base = ((uint64_t)bhi << 32) | blo;
        for (uint32_t k = lane; k < staged; k += 64) {
            const uint64_t w = base + k;
            if (w < cap) { cq[w] = s_q[wv][k]; ct[w] = s_t[wv][k]; cd[w] = s_d[wv][k]; }
        }
        staged = 0;
        __builtin_amdgcn_wave_barrier();
    };
    // A wave looks at 64 consecutive keys at a time (one coalesced load; r04 — until then the first key of every group walked its group alone with
    // dependent loads while the other lanes of the wave idled: 9.4 ms for 0.22 G keys at configs[1], ~0.2 TB/s).  Run starts (key differs from its
    // predecessor) and group starts come from two ballots; a run's length is the distance to the next run start; the group's first lane folds the
    // (length, diagonal) pairs of its runs out of LDS.  Only the ONE run and the ONE group that reach past the wave's 64 keys are finished serially.
    __shared__ uint64_t s_v1[4][64], s_v2[4][64];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nround; i += (uint64_t)gridDim.x * 256) {
        bool cand = false, deferred = false;
        int best_d = 0, last_d = 0;
        uint64_t grp = 0;
        const uint64_t wbase = i - (uint64_t)lane;                    // first key of this wave's window
        const bool valid = i < n;
        const uint64_t k = valid ? keys[i] : ~0ull;
        uint64_t kp = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
        if (lane == 0) kp = (valid && i > 0) ? keys[i - 1] : ~k;
        const bool run_start = valid && kp != k;
        const bool grp_start = valid && (i == 0 || (kp >> fmt.dbits) != (k >> fmt.dbits));
        const uint64_t starts = __builtin_amdgcn_ballot_w64(run_start), gstarts = __builtin_amdgcn_ballot_w64(grp_start);
        const uint64_t above = lane == 63 ? 0ull : (~0ull << (lane + 1));
        const uint64_t wend = wbase + 64 < n ? wbase + 64 : n;        // first key behind the window (or the end of the list)
        // the window's last group — the only one that can reach behind it — is LONG if it covers the whole next window: decided first (one load by its
        // first lane), so that the window's last run, which belongs to that group, is not walked for nothing
        if (grp_start && !(gstarts & above) && wend < n) {
            const uint64_t far = wend + 63 < n ? wend + 63 : n - 1;
            deferred = (keys[far] >> fmt.dbits) == (k >> fmt.dbits);
        }
        const bool long_tail = __builtin_amdgcn_ballot_w64(deferred) != 0;
        uint64_t v1 = 0, v2 = 0;
        if (run_start) {
            const uint64_t nx = starts & above;
            uint64_t cnt;
            if (nx) cnt = (uint64_t)(__builtin_ctzll(nx) - lane);
            else {                                                     // the window's last run: it may go on behind the window, for < 64 keys
                uint64_t e = wend;                                     // (otherwise its group is long and nothing here is used)
                const uint64_t lim = wend + 64 < n ? wend + 64 : n;
                if (!long_tail) while (e < lim && keys[e] == k) e++;
                cnt = e - i;
            }
            const uint64_t d = k & dmask;                              // diagonal + bias
            v1 = (cnt << 32) | (0xFFFFFFFFull - d);                    // max: most hits, then the SMALLEST diagonal
            v2 = (cnt << 32) | d;                                      // max: most hits, then the LARGEST diagonal (the pair the other way round)
        }
        s_v1[wv][lane] = v1; s_v2[wv][lane] = v2;
        __builtin_amdgcn_wave_barrier();
        if (grp_start) {
            grp = k >> fmt.dbits;
            const uint64_t ng = gstarts & above;
            const int gend = ng ? __builtin_ctzll(ng) : 64;            // this group's lanes inside the window: [lane, gend)
            uint64_t b1 = 0, b2 = 0;
            uint64_t runs = starts & (~0ull << lane) & (gend == 64 ? ~0ull : ((1ull << gend) - 1ull));
            while (runs) {
                const int r = __builtin_ctzll(runs);
                runs &= runs - 1;
                const uint64_t a = s_v1[wv][r], c2 = s_v2[wv][r];
                b1 = a > b1 ? a : b1; b2 = c2 > b2 ? c2 : b2;
            }
            if (gend == 64 && wend < n && !deferred) {                 // the group ends inside the next window: the rest of it, run by run
                uint64_t e = wend;
                // skip what is left of the window's last run (already counted by its own lane), then walk the following runs of the group
                const uint64_t kw = keys[wend - 1];
                while (e < n && keys[e] == kw) e++;
                while (e < n && (keys[e] >> fmt.dbits) == grp) {
                    const uint64_t kb = keys[e];
                    uint64_t f = e + 1;
                    while (f < n && keys[f] == kb) f++;
                    const uint64_t cnt = f - e, d = kb & dmask;
                    const uint64_t a = (cnt << 32) | (0xFFFFFFFFull - d), c2 = (cnt << 32) | d;
                    b1 = a > b1 ? a : b1; b2 = c2 > b2 ? c2 : b2;
                    e = f;
                }
            }
            cand = !deferred && (int)(b1 >> 32) >= min_hits;
            best_d = (int)(0xFFFFFFFFull - (b1 & 0xFFFFFFFFull)) - fmt.dbias;
            last_d = (int)(b2 & 0xFFFFFFFFull) - fmt.dbias;
        }
        __builtin_amdgcn_wave_barrier();                               // the LDS rows are rewritten in the next round
        {   // at most one group of a window can be long (it reaches the window's end): one flag byte per window
            const uint64_t dm = __builtin_amdgcn_ballot_w64(deferred);
            if (lane == 0 && wbase < n) wflag[wbase >> 6] = dm ? (uint8_t)(__builtin_ctzll(dm) + 1) : (uint8_t)0;
        }
        const uint32_t gq = qbegin + (uint32_t)(grp >> fmt.tbits), gt = (uint32_t)(grp & tmask);
        const uint64_t m = __builtin_amdgcn_ballot_w64(cand);
        if (m) {
            if (cand) {
                const uint32_t k = staged + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                s_q[wv][k] = gq;
                s_t[wv][k] = gt;
                s_d[wv][k] = best_d;
            }
            staged += (uint32_t)__popcll(m);
            __builtin_amdgcn_wave_barrier();
            if (staged >= DS_DRAIN) drain();
        }
        // the pair the other way round (a second round of at most 64 entries: a stage that was below DS_DRAIN cannot overflow)
        const bool mcand = cand && gq >= mirror_q0;
        const uint64_t mm = __builtin_amdgcn_ballot_w64(mcand);
        if (mm) {
            if (mcand) {
                const uint32_t k = staged + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
                s_q[wv][k] = gt;
                s_t[wv][k] = gq;
                s_d[wv][k] = -last_d;
            }
            staged += (uint32_t)__popcll(mm);
            __builtin_amdgcn_wave_barrier();
            if (staged >= DS_DRAIN) drain();
        }
    }
    if (staged) drain();
}

// the long groups flagged by diag_select_kernel: a wave per group scans it 64 keys at a time; a run that reaches the end of a window is carried
// (key, length so far) into the next one, so nothing is walked key by key.  Same result rule, same staging of the candidates.
__global__ void __launch_bounds__(256) diag_long_kernel(const uint64_t *keys, uint64_t n, int min_hits, KeyFmt fmt, uint32_t qbegin,
                                                        unsigned long long *n_cand, uint64_t cap,
                                                        uint32_t *cq, uint32_t *ct, int32_t *cd, uint32_t mirror_q0, const uint8_t *wflag) {
    __shared__ uint32_t s_q[4][128], s_t[4][128];
    __shared__ int32_t s_d[4][128];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t dmask = (1ull << fmt.dbits) - 1, tmask = (1ull << fmt.tbits) - 1;
    const uint64_t nwin = (n + 63) >> 6;
    uint32_t staged = 0;
    auto drain = [&]() {
        uint32_t blo = 0, bhi = 0;
        if (lane == 0) {
            const unsigned long long b = atomicAdd(n_cand, (unsigned long long)staged);
            blo = (uint32_t)b; bhi = (uint32_t)(b >> 32);
        }
        blo = (uint32_t)__shfl((int)blo, 0, 64);
        bhi = (uint32_t)__shfl((int)bhi, 0, 64);
        const uint64_t base = ((uint64_t)bhi << 32) | blo;
        for (uint32_t k = lane; k < staged; k += 64) {
            const uint64_t w = base + k;
            if (w < cap) { cq[w] = s_q[wv][k]; ct[w] = s_t[wv][k]; cd[w] = s_d[wv][k]; }
        }
        staged = 0;
        __builtin_amdgcn_wave_barrier();
    };
    auto wmax = [&](uint64_t v) -> uint64_t {
        for (int o = 32; o > 0; o >>= 1) { const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)v, o, 64); v = x > v ? x : v; }
        return v;
    };
    const uint64_t nw64 = (nwin + 63) >> 6;                            // a wave looks at the flags of 64 windows at a time
    for (uint64_t wb = (uint64_t)blockIdx.x * 4 + wv; wb < nw64; wb += (uint64_t)gridDim.x * 4) {
        const uint64_t w = wb * 64 + lane;
        const uint32_t fl = w < nwin ? wflag[w] : 0u;
        uint64_t pending = __builtin_amdgcn_ballot_w64(fl != 0);
        while (pending) {                                              // wave-uniform loop over the flagged windows
            const int src = __builtin_ctzll(pending);
            pending &= pending - 1;
            const uint32_t f = (uint32_t)__shfl((int)fl, src, 64);
            const uint64_t i0 = ((wb * 64 + (uint64_t)src) << 6) + (f - 1);      // first key of the long group
            const uint64_t grp = keys[i0] >> fmt.dbits;
            uint64_t b1 = 0, b2 = 0, carry_key = 0, carry_cnt = 0;
            bool carry = false;
            for (uint64_t pos = i0;; pos += 64) {
                const uint64_t idx = pos + lane;
                const uint64_t k = idx < n ? keys[idx] : ~0ull;
                const bool in = idx < n && (k >> fmt.dbits) == grp;
                const uint64_t inmask = __builtin_amdgcn_ballot_w64(in);
                const int nin = inmask == ~0ull ? 64 : __builtin_ctzll(~inmask);          // the group's keys are contiguous: leading lanes
                if (nin == 0) break;
                uint64_t kp = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
                if (lane == 0) kp = carry ? carry_key : ~k;
                const bool rs = lane < nin && kp != k;
                const uint64_t starts = __builtin_amdgcn_ballot_w64(rs);
                const int lead = starts ? __builtin_ctzll(starts) : nin;                  // keys that continue the carried run
                if (carry) {
                    carry_cnt += (uint64_t)lead;
                    if (lead < nin || nin < 64) {                                          // the carried run ends in this window
                        const uint64_t d = carry_key & dmask, a = (carry_cnt << 32) | (0xFFFFFFFFull - d), c2 = (carry_cnt << 32) | d;
                        b1 = a > b1 ? a : b1; b2 = c2 > b2 ? c2 : b2;
                        carry = false;
                    }
                }
                const uint64_t above = lane == 63 ? 0ull : (~0ull << (lane + 1));
                uint64_t v1 = 0, v2 = 0;
                bool open = false;                                                         // this lane's run reaches the window's end inside the group
                if (rs) {
                    const uint64_t nx = starts & above;
                    const int end = nx ? __builtin_ctzll(nx) : nin;
                    const uint64_t cnt = (uint64_t)(end - lane), d = k & dmask;
                    open = !nx && nin == 64;
                    if (!open) { v1 = (cnt << 32) | (0xFFFFFFFFull - d); v2 = (cnt << 32) | d; }
                }
                v1 = wmax(v1); v2 = wmax(v2);
                b1 = v1 > b1 ? v1 : b1; b2 = v2 > b2 ? v2 : b2;
                const uint64_t om = __builtin_amdgcn_ballot_w64(open);
                if (om) {                                                                  // the new carried run (at most one)
                    const int ol = __builtin_ctzll(om);
                    carry_key = (uint64_t)__shfl((unsigned long long)k, ol, 64);
                    carry_cnt = (uint64_t)(64 - ol);
                    carry = true;
                }
                if (nin < 64) break;
            }
            if (carry) {                                                                   // the group ended exactly at a window boundary
                const uint64_t d = carry_key & dmask, a = (carry_cnt << 32) | (0xFFFFFFFFull - d), c2 = (carry_cnt << 32) | d;
                b1 = a > b1 ? a : b1; b2 = c2 > b2 ? c2 : b2;
            }
            if ((int)(b1 >> 32) >= min_hits) {                                             // wave-uniform
                const uint32_t gq = qbegin + (uint32_t)(grp >> fmt.tbits), gt = (uint32_t)(grp & tmask);
                const bool mir = gq >= mirror_q0;
                if (lane == 0) {
                    s_q[wv][staged] = gq; s_t[wv][staged] = gt; s_d[wv][staged] = (int)(0xFFFFFFFFull - (b1 & 0xFFFFFFFFull)) - fmt.dbias;
                    if (mir) { s_q[wv][staged + 1] = gt; s_t[wv][staged + 1] = gq; s_d[wv][staged + 1] = -((int)(b2 & 0xFFFFFFFFull) - fmt.dbias); }
                }
                staged += mir ? 2u : 1u;
                __builtin_amdgcn_wave_barrier();
                if (staged >= 64) drain();
            }
        }
    }
    if (staged) drain();
}

// ---- E2 diagonal selection on chip (compact mode): one workgroup per query, right behind filter_kernel ----
// filter_kernel leaves a query's surviving u32 keys [target - tbase | diagonal + dbias] at the head of the query's own region, so they are grouped by
// query already; widening them to u64, prepending the query bits and radix-sorting the whole batch only restores that order.  A query with at most
// TDS_CAP survivors is sorted here in LDS (rocprim::block_radix_sort over the significant bits, all-ones padding, items per thread chosen from n by a
// workgroup-uniform branch), its runs and groups are evaluated under diag_select_kernel's rule by three max-scans over the sorted keys:
//   A   index of the last run start at or before i            -> a run's length at its last key
//   B1  [ group | length | dmask - diagonal ] at the run ends -> most hits, then the SMALLEST diagonal, at the group's last key
//   B2  [ group | length | diagonal ]                         -> most hits, then the LARGEST diagonal (the pair the other way round)
// (the group field leads, the keys are sorted, so a plain max-scan is the segmented one), and the chosen keys go back to the head of the region: plain
// candidates first, the mirrored ones (still [target | largest diagonal]: cand_gather_kernel swaps and negates) behind them.  A candidate's group holds
// >= min_hits >= 2 keys, so up to two records per group fit; every key is in registers before the first store (the sort's barriers).  No key-by-key walk:
// a thread folds its own TDS_T-th of the sorted array whatever the runs look like.  Queries with no or more than `cap` survivors are left to the batch sort.
// Measured at configs[1] (profiles/td_onchip): 99 % of the queries and 91 % of the surviving keys are taken here.
constexpr int TDS_T = 256;             // threads per workgroup: several workgroups per CU
constexpr int TDS_MAX_IPT = 32;
static_assert(TDS_CAP == TDS_T * TDS_MAX_IPT, "uc_prefilter_internal.h carries the number for the driver");
template <int IPT> using TdSort = rocprim::block_radix_sort<uint32_t, TDS_T, IPT>;
constexpr size_t tds_max(size_t a, size_t b) { return a > b ? a : b; }
// two launches share the work: the registers and the LDS of the 16- and 32-item sorts would leave the common short queries three workgroups per CU
constexpr int TDS_SMALL_IPT = 8;       // td_select_kernel<false>: n <= 8 x TDS_T, td_select_kernel<true>: the rest up to TDS_CAP
constexpr size_t TDS_SORT_BYTES_SMALL =
    tds_max(tds_max(sizeof(TdSort<1>::storage_type), sizeof(TdSort<2>::storage_type)), tds_max(sizeof(TdSort<4>::storage_type), sizeof(TdSort<8>::storage_type)));
constexpr size_t TDS_SORT_BYTES_BIG = tds_max(sizeof(TdSort<16>::storage_type), sizeof(TdSort<32>::storage_type));

struct TdsMax { template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct TdsSum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
// exclusive scan of one value per thread over the workgroup (identity 0); *total = the fold of all of them.  s_w: TDS_T / 64 slots, free again on return
template <class T, class Op>
__device__ __forceinline__ T tds_block_excl(T v, Op op, T *s_w, T *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = (T)__shfl_up((unsigned long long)inc, o, 64);
        if (lane >= o) inc = op(u, inc);
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    T ex = (T)__shfl_up((unsigned long long)inc, 1, 64), all = 0;
    if (lane == 0) ex = 0;
    for (int w = 0; w < TDS_T / 64; w++) {
        const T u = s_w[w];
        if (w < wv) ex = op(u, ex);
        all = op(all, u);
    }
    __syncthreads();
    if (total) *total = all;
    return ex;
}

// the same for two values at once under max (one pair of barriers).  s_w: 2 x TDS_T / 64 slots
__device__ __forceinline__ void tds_block_excl_max2(uint64_t a, uint64_t b, uint64_t *s_w, uint64_t &ea, uint64_t &eb) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t ua = (uint64_t)__shfl_up((unsigned long long)a, o, 64), ub = (uint64_t)__shfl_up((unsigned long long)b, o, 64);
        if (lane >= o) { a = ua > a ? ua : a; b = ub > b ? ub : b; }
    }
    if (lane == 63) { s_w[2 * wv] = a; s_w[2 * wv + 1] = b; }
    __syncthreads();
    ea = (uint64_t)__shfl_up((unsigned long long)a, 1, 64); eb = (uint64_t)__shfl_up((unsigned long long)b, 1, 64);
    if (lane == 0) ea = eb = 0;
    for (int w = 0; w < wv; w++) {
        const uint64_t ua = s_w[2 * w], ub = s_w[2 * w + 1];
        ea = ua > ea ? ua : ea; eb = ub > eb ? ub : eb;
    }
    __syncthreads();
}

template <int IPT>
__device__ __forceinline__ uint32_t td_select_sorted(uint32_t *reg, uint32_t n, int min_hits, int dbits, unsigned end_bit, bool mirror, void *s_sort,
                                                     uint32_t (*s_edge)[TDS_T], uint64_t *s_w) {
    const int tid = threadIdx.x;
    const uint32_t dmask = (1u << dbits) - 1u;
    uint32_t keys[IPT];
#pragma unroll
    for (int j = 0; j < IPT; j++) {
        const uint32_t i = (uint32_t)j * TDS_T + tid;
        keys[j] = i < n ? reg[i] : 0xFFFFFFFFu;
    }
    TdSort<IPT>().sort(keys, *reinterpret_cast<typename TdSort<IPT>::storage_type *>(s_sort), 0u, end_bit);
    // blocked: this thread holds the sorted keys i0 .. i0 + IPT - 1 (the padding sorts behind the n keys: only i < n is looked at)
    const uint32_t i0 = (uint32_t)tid * IPT;
    s_edge[0][tid] = keys[0]; s_edge[1][tid] = keys[IPT - 1];
    __syncthreads();
    const uint32_t kprev = tid ? s_edge[1][tid - 1] : 0u, knext = tid < TDS_T - 1 ? s_edge[0][tid + 1] : 0u;
    __syncthreads();
    uint32_t rs = 0;
    uint64_t m1 = 0, m2 = 0;
    // folds the sorted key i0 + j into (rs, m1, m2); true: it is the last key of its group
    auto step = [&](int j) -> bool {
        const uint32_t i = i0 + (uint32_t)j, k = keys[j];
        const uint32_t kp = j ? keys[j ? j - 1 : 0] : kprev, kn = j < IPT - 1 ? keys[j < IPT - 1 ? j + 1 : j] : knext;
        if (i >= n) return false;
        if (i == 0 || kp != k) rs = i;
        const bool last = i == n - 1;
        if (last || kn != k) {
            const uint64_t g = ((uint64_t)(k >> dbits) << 32) | ((uint64_t)(i + 1 - rs) << dbits);
            const uint64_t a = g | (uint64_t)(dmask - (k & dmask)), b = g | (uint64_t)(k & dmask);
            m1 = a > m1 ? a : m1; m2 = b > m2 ? b : m2;
        }
        return last || (kn >> dbits) != (k >> dbits);
    };
    // A
#pragma unroll
    for (int j = 0; j < IPT; j++) {
        const uint32_t i = i0 + (uint32_t)j, kp = j ? keys[j ? j - 1 : 0] : kprev;
        if (i < n && (i == 0 || kp != keys[j])) rs = i;
    }
    const uint32_t rs0 = (uint32_t)tds_block_excl<uint64_t>((uint64_t)rs, TdsMax(), s_w, nullptr);
    // B1 / B2
    rs = rs0;
#pragma unroll
    for (int j = 0; j < IPT; j++) (void)step(j);
    uint64_t e1, e2;
    tds_block_excl_max2(m1, m2, s_w, e1, e2);
    // the candidates of this thread's group ends, counted, then written behind those of the threads below
    uint32_t mine = 0;
    rs = rs0; m1 = e1; m2 = e2;
#pragma unroll
    for (int j = 0; j < IPT; j++)
        if (step(j)) mine += (int)((uint32_t)m1 >> dbits) >= min_hits ? 1u : 0u;
    uint64_t tot64 = 0;
    uint32_t w = (uint32_t)tds_block_excl<uint64_t>((uint64_t)mine, TdsSum(), s_w, &tot64);
    const uint32_t ncand = (uint32_t)tot64;
    if (mine) {
        rs = rs0; m1 = e1; m2 = e2;
#pragma unroll
        for (int j = 0; j < IPT; j++)
            if (step(j) && (int)((uint32_t)m1 >> dbits) >= min_hits) {
                const uint32_t g = (keys[j] >> dbits) << dbits;
                reg[w] = g | (dmask - ((uint32_t)m1 & dmask));
                if (mirror) reg[ncand + w] = g | ((uint32_t)m2 & dmask);      // (2 ncand <= n: every candidate group holds >= min_hits >= 2 keys)
                w++;
            }
    }
    return ncand;
}

template <bool BIG>
__global__ void __launch_bounds__(TDS_T) td_select_kernel(uint32_t *region, const uint64_t *qbase, uint32_t *qsurv, const uint32_t *order, uint32_t qbegin,
                                                          uint32_t mirror_q0, int min_hits, int dbits, unsigned end_bit, uint32_t cap,
                                                          uint32_t *qcand, uint32_t *qmir, uint32_t *qrec, unsigned long long *n_taken) {
    __shared__ __attribute__((aligned(16))) char s_sort[BIG ? TDS_SORT_BYTES_BIG : TDS_SORT_BYTES_SMALL];
    __shared__ uint32_t s_edge[2][TDS_T];
    __shared__ uint64_t s_w[2 * TDS_T / 64];
    constexpr uint32_t SMALL = (uint32_t)TDS_SMALL_IPT * TDS_T;
    const uint32_t qi = order[blockIdx.x];
    const uint32_t n = qsurv[qi];
    if (n == 0 || n > cap) {                   // (workgroup-uniform, and so is every branch on n below)
        if (!BIG && threadIdx.x == 0) { qcand[qi] = 0; qmir[qi] = 0; qrec[qi] = 0; }
        return;
    }
    if (BIG != (n > SMALL)) return;            // the other launch's query (<true> runs behind <false>: qsurv of a query taken there is 0 by now)
    uint32_t *reg = region + qbase[qi];
    const bool mirror = mirror_q0 != UINT32_MAX && qbegin + qi >= mirror_q0;
    uint32_t nc;
    if (BIG) {
        if (n <= 16u * TDS_T) nc = td_select_sorted<16>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
        else nc = td_select_sorted<32>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
    } else {
        if (n <= 1u * TDS_T) nc = td_select_sorted<1>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
        else if (n <= 2u * TDS_T) nc = td_select_sorted<2>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
        else if (n <= 4u * TDS_T) nc = td_select_sorted<4>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
        else nc = td_select_sorted<8>(reg, n, min_hits, dbits, end_bit, mirror, s_sort, s_edge, s_w);
    }
    if (threadIdx.x == 0) {
        qcand[qi] = nc; qmir[qi] = mirror ? nc : 0u; qrec[qi] = mirror ? 2u * nc : nc;
        qsurv[qi] = 0;
        atomicAdd(n_taken, (1ull << 40) | (unsigned long long)n);      // [ queries : 24 | keys : 40 ] of the batch that were taken here
    }
}

// the region-resident records of td_select_kernel -> candidates at out0 + coff[query] (coff: exclusive scan of qcand + qmir), a wave per query
__global__ void __launch_bounds__(256) cand_gather_kernel(const uint32_t *region, const uint64_t *qbase, const uint32_t *qcand, const uint32_t *qmir,
                                                          const uint64_t *coff, uint32_t nq, KeyFmt fmt, uint32_t qbegin, uint64_t out0,
                                                          uint32_t *cq, uint32_t *ct, int32_t *cd) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t dmask = (1u << fmt.dbits) - 1u;
    for (uint32_t qi = blockIdx.x * 4 + wv; qi < nq; qi += gridDim.x * 4) {
        const uint32_t nc = qcand[qi], nr = nc + qmir[qi];
        if (!nr) continue;
        const uint64_t src = qbase[qi], dst = out0 + coff[qi];
        const uint32_t q = qbegin + qi;
        for (uint32_t k = lane; k < nr; k += 64) {
            const uint32_t td = region[src + k];
            const uint32_t t = (td >> fmt.dbits) + fmt.tbase;
            const int32_t d = (int32_t)(td & dmask) - fmt.dbias;
            const bool plain = k < nc;
            cq[dst + k] = plain ? q : t; ct[dst + k] = plain ? t : q; cd[dst + k] = plain ? d : -d;
        }
    }
}

// the two launches of the on-chip selection for expand_keys_filtered (uc_kmer_filter.hip), which has reserved and zeroed what they write
void launch_td_select(Engine &E, const PrefilterPass &PP, uint32_t qa, uint32_t nq) {
    PrefilterScratch &S = *E.pre;
    const KeyFmt &fmt = PP.fmt;
    int rbits = 1;                             // bits of (target - tbase), as in key_format
    while ((1ull << rbits) < (uint64_t)std::max<uint32_t>(PP.tend - PP.tbegin, 1)) rbits++;
    hipLaunchKernelGGL(td_select_kernel<false>, dim3(nq), dim3(TDS_T), 0, E.stream, (uint32_t *)S.batch.d_keys.p, S.batch.d_qbase.p, S.batch.d_qsurv.p, S.batch.d_order.p, qa, PP.mirror_q0,
                       E.p.min_diag_hits, fmt.dbits, (unsigned)std::min(32, rbits + fmt.dbits), PP.td_cap, S.cand.d_qcand.p, S.cand.d_qmir.p, S.cand.d_qrec.p, S.shared.d_counters.p + 7);
    if (PP.td_cap > (uint32_t)TDS_SMALL_IPT * TDS_T)
        hipLaunchKernelGGL(td_select_kernel<true>, dim3(nq), dim3(TDS_T), 0, E.stream, (uint32_t *)S.batch.d_keys.p, S.batch.d_qbase.p, S.batch.d_qsurv.p, S.batch.d_order.p, qa, PP.mirror_q0,
                           E.p.min_diag_hits, fmt.dbits, (unsigned)std::min(32, rbits + fmt.dbits), PP.td_cap, S.cand.d_qcand.p, S.cand.d_qmir.p, S.cand.d_qrec.p, S.shared.d_counters.p + 7);
}

// consumes the batch's sorted keys; produces its candidates (d_cq / d_ct / d_cd: query, target, best diagonal; mirrored pairs twice) and their number
uint64_t select_diagonals(Engine &E, PrefilterPass &PP, const QueryBatch &B) {
    PrefilterScratch &S = *E.pre;
    PP.cand_cap = std::max<uint64_t>(PP.cand_cap, std::max<uint64_t>(1u << 20, B.total_hits / 32));
    for (;;) {
        S.cand.d_cq.reserve(PP.cand_cap + B.n_rec); S.cand.d_ct.reserve(PP.cand_cap + B.n_rec); S.cand.d_cd.reserve(PP.cand_cap + B.n_rec);      // (room for the region-resident records behind them)
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 6, 0, 8, E.stream));
        if (B.n_sort) {
            S.cand.d_wflag.reserve((B.n_sort + 63) / 64 + 64);
            // every wave ends on one returning atomic on the candidate cursor (its last, partial stage): the capped grid bounds them
            hipLaunchKernelGGL(diag_select_kernel, grid_for(B.n_sort, E.count_grid_cap), dim3(256), 0, E.stream, B.sorted, B.n_sort, E.p.min_diag_hits, PP.fmt, B.qa,
                               S.shared.d_counters.p + 6, PP.cand_cap, S.cand.d_cq.p, S.cand.d_ct.p, S.cand.d_cd.p, PP.mirror_q0, S.cand.d_wflag.p);
            hipLaunchKernelGGL(diag_long_kernel, grid_for((B.n_sort + 63) / 64), dim3(256), 0, E.stream, B.sorted, B.n_sort, E.p.min_diag_hits, PP.fmt, B.qa,
                               S.shared.d_counters.p + 6, PP.cand_cap, S.cand.d_cq.p, S.cand.d_ct.p, S.cand.d_cd.p, PP.mirror_q0, (const uint8_t *)S.cand.d_wflag.p);
        }
        unsigned long long nc = 0;
        UC_HIP(hipMemcpyAsync(&nc, S.shared.d_counters.p + 6, 8, hipMemcpyDeviceToHost, E.stream));
        UC_HIP(hipStreamSynchronize(E.stream));
        if (nc <= PP.cand_cap) {
            if (getenv("UC_TIMING"))
                fprintf(stderr, "unicore-cluster[timing]: diagonal selection: %llu candidates of %llu sorted keys, %llu selected on chip\n", nc, (unsigned long long)B.n_sort, (unsigned long long)B.n_rec);
            if (B.n_rec)      // their number is known exactly: no cap, cursor or retry
                hipLaunchKernelGGL(cand_gather_kernel, grid_for((uint64_t)(B.qb - B.qa) * 64), dim3(256), 0, E.stream, (const uint32_t *)S.batch.d_keys.p, S.batch.d_qbase.p,
                                   S.cand.d_qcand.p, S.cand.d_qmir.p, S.cand.d_coff.p, B.qb - B.qa, PP.fmt, B.qa, (uint64_t)nc, S.cand.d_cq.p, S.cand.d_ct.p, S.cand.d_cd.p);
            return nc + B.n_rec;
        }
        PP.cand_cap = nc;     // rare: more candidates than provisioned, run the selection again
    }
}

void preload_diag_select_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)diag_select_kernel); }
}  // namespace uc
