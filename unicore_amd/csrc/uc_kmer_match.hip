// uc_kmer_match.hip - prefilter stage E1 and stage E2 up to the run lists.
// Consumes the resident database: the 3Di track of a target chunk and of the queries matched against it.
// Produces (a) the chunk's k-mer index (build_index): (k-mer, sequence, position) per target residue -> radix sort by k-mer -> offsets per k-mer slot
// (20^6 + 1 u32) and an 8 MB presence bitmap of the k-mers that occur; (b) the plan of a query super-batch (plan_superbatch): the DISTINCT k-mers of its
// queries, the similar k-mers of each (sim_runs_kernel: sorted-letter DFS with a score bound as a per-lane state machine, the bitmap in front of the
// offset table) as index ranges ("runs") sorted by k-mer rank, and per query position the length and source of its run list and its k-mer hits;
// with the running sums of both and the totals per query; (c) an exact query batch (cut_batch): the queries whose hits and runs fit the key buffers, cut
// on the plan's per-query totals.  Nothing is copied for it: uc_kmer_filter.hip reads a batch's runs where the plan left them.
// Sort and scan primitives come from rocPRIM; every kernel below is hand-written for wave64 (spec UC-1 E1-E2).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_prefilter_internal.h"

namespace uc {

constexpr uint32_t KMER_INVALID = 0xFFFFFFFFu;

// ---------------------------------------------------------------- E1: index build
__global__ void __launch_bounds__(256) kmer_extract_kernel(const DeviceDb db, uint32_t tbegin, uint32_t tend, KmerCfg cfg,
                                                           uint32_t p0, uint32_t p1, uint32_t *keys, uint64_t *vals,
                                                           uint32_t *vals32 /* compact entries instead of vals */, int pshift) {
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < p1 - p0; idx += (uint64_t)gridDim.x * 256) {
        const uint32_t p = p0 + (uint32_t)idx;
        const uint32_t s = find_seq(db.off, tbegin, tend, p);
        const uint32_t j = p - db.off[s], len = db.len[s];
        uint32_t key = KMER_INVALID;
        if (j + cfg.span <= len && j <= 65535u) {
            uint32_t v = 0, mul = 1;
            bool ok = true;
#pragma unroll
            for (int m = 0; m < K; m++) {
                const uint32_t c = db.s3[p + cfg.koff[m]];
                ok &= c < KA;
                v += c * mul;
                mul *= KA;
            }
            if (ok) key = v;
        }
        keys[idx] = key;
        if (vals32) vals32[idx] = ((s - tbegin) << pshift) | (j & ((1u << pshift) - 1u));
        else vals[idx] = ((uint64_t)s << 16) | j;
    }
}

__global__ void __launch_bounds__(256) kmer_offsets_kernel(const uint32_t *keys, uint32_t n, uint32_t *koff) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k <= KSPACE; k += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = n;   // first index with key >= k
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < (uint32_t)k) lo = mid + 1; else hi = mid;
        }
        koff[k] = lo;
    }
}

// presence bitmap of the chunk's k-mers (bit v = the index holds k-mer v): 8 MB for the 20^6 k-mers — resident in every XCD's L2, where the
// 256 MB offset table is not.  At high sensitivity the target chunks are small (density cuts: ~5 M residues at 100 proteomes, < 10 % of the
// k-mer space occupied) and nine of ten similar k-mers miss; the bitmap answers those without touching the offset table (r4: prefilter
// kernels 7.67 -> 6.93 s at 50 proteomes, 26.0 -> 23.5 s at 100 proteomes with configs[3]'s options; nothing at -s 4, where most k-mers occur).
__global__ void __launch_bounds__(256) kmer_bits_kernel(const uint32_t *koff, uint32_t *bits) {
    for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < (KSPACE + 31) / 32; w += (uint64_t)gridDim.x * 256) {
        uint32_t m = 0;
        const uint64_t v0 = w * 32;
        uint32_t prev = koff[v0];
        for (int b = 0; b < 32 && v0 + b < KSPACE; b++) {
            const uint32_t nxt = koff[v0 + b + 1];
            m |= (nxt != prev ? 1u : 0u) << b;
            prev = nxt;
        }
        bits[w] = m;
    }
}

// ---------------------------------------------------------------- E2: similar k-mers
constexpr int SIM_NEED_MAX = 49;   // substitution scores lie in [-48, 48] (checked by the host): a needed score beyond either end selects all / no letters
struct SimTables {           // LDS: per query letter a, target letters sorted by score descending
    int8_t sc[KA][KA];
    uint8_t ord[KA][KA];
    int8_t rowmax[KA];
    uint8_t lcnt[KA][2 * SIM_NEED_MAX + 1];    // [a][need + SIM_NEED_MAX]: how many letters b have S(a, b) >= need (they are the first lcnt of the sorted row) ...
    uint32_t pmask[KA][KA + 1];                // ... and [a][n]: the first n letters of a's sorted row as a bit mask (r05: the DFS's last level in ONE step)
};

__device__ void build_sim_tables(SimTables &t, const int8_t *S3) {
    for (int a = threadIdx.x; a < KA; a += blockDim.x) {
        int8_t sc[KA];
        uint8_t ord[KA];
        for (int b = 0; b < KA; b++) { sc[b] = S3[a * 21 + b]; ord[b] = (uint8_t)b; }
        for (int i = 1; i < KA; i++) {   // insertion sort: score desc, letter asc
            const int8_t s = sc[i];
            const uint8_t o = ord[i];
            int k = i - 1;
            while (k >= 0 && (sc[k] < s)) { sc[k + 1] = sc[k]; ord[k + 1] = ord[k]; k--; }
            sc[k + 1] = s;
            ord[k + 1] = o;
        }
        for (int b = 0; b < KA; b++) { t.sc[a][b] = sc[b]; t.ord[a][b] = ord[b]; }
        t.rowmax[a] = sc[0];
    }
    for (int i = threadIdx.x; i < KA * (2 * SIM_NEED_MAX + 1); i += blockDim.x) {
        const int a = i / (2 * SIM_NEED_MAX + 1), need = i % (2 * SIM_NEED_MAX + 1) - SIM_NEED_MAX;
        int n = 0;
        for (int b = 0; b < KA; b++) n += S3[a * 21 + b] >= need ? 1 : 0;
        t.lcnt[a][i % (2 * SIM_NEED_MAX + 1)] = (uint8_t)n;
    }
    __syncthreads();                            // (ord is read below)
    for (int i = threadIdx.x; i < KA * (KA + 1); i += blockDim.x) {
        const int a = i / (KA + 1), n = i % (KA + 1);
        uint32_t m = 0;
        for (int j = 0; j < n; j++) m |= 1u << t.ord[a][j];
        t.pmask[a][n] = m;
    }
}

// shared by the count and the emit pass: decode the query position handled by this thread
__device__ __forceinline__ bool query_kmer_at(const DeviceDb &db, const KmerCfg &cfg, uint32_t qbegin, uint32_t qend,
                                              uint32_t p, uint32_t *q, uint32_t *i, uint32_t c[K]) {
    const uint32_t s = find_seq(db.off, qbegin, qend, p);
    const uint32_t j = p - db.off[s], len = db.len[s];
    *q = s;
    *i = j;
    if (!(j + cfg.span <= len && j <= 65535u)) return false;
    bool ok = true;
#pragma unroll
    for (int m = 0; m < K; m++) { c[m] = db.s3[p + cfg.koff[m]]; ok &= c[m] < KA; }
    return ok;
}

// ---- E2 pass 1: enumerate similar k-mers (sorted-letter DFS with score bound), keep the non-empty index ranges ("runs") ----
// A run is (first index entry, entry count, query position inside the batch); run order is irrelevant (keys get sorted).
// A lane per query position running its own nested loops leaves most lanes idle: the number of similar k-mers per
// position is heavy-tailed (mean ~20, maximum > 1000), a wave lasts as long as its worst position (~0.18 SIMD
// efficiency).  Here the DFS is an explicit state machine (level, index per level and the six letters packed into
// registers; score and value so far kept incrementally): every wave step advances every lane by ONE node, and a lane that
// finishes its position takes the next one of the wave's region at once, so all lanes stay busy until the region is
// exhausted — which pays once a lane works through many positions, hence one contiguous region per wave and query
// batches as large as the key buffer allows.  Positions are decoded 64 at a time into a small pool (the sequence search
// and letter loads are ~10 us of dependent loads that must not sit in front of every hand-out).  Leaves (k-mer value,
// position) are appended to a wave queue by ballot rank — no per-lane atomics under divergence — and the offset-table
// lookups are done 64 at a time when the queue fills, fully parallel and off the enumeration's critical path; the
// non-empty ranges are staged per wave and written out behind ONE global atomic per RUN_STAGE runs.
constexpr int RUN_STAGE = 256;      // staged runs per wave

// counters: the legend of d_counters[0..7] is in uc_prefilter_internal.h
constexpr int LEAFQ = 256;          // leaf queue entries per wave
constexpr int POSQ = 128;           // decoded positions per wave (ring)
constexpr int SIM_MIN_WAVE_POS = 256;   // fewer positions per wave than this: fewer workgroups
constexpr int SIM_MAX_BLOCKS = 1024;     // 256 CUs x 4 resident workgroups (37 KB of LDS each)

__global__ void __launch_bounds__(256) sim_runs_kernel(const DeviceDb db, KmerCfg cfg, uint32_t qbegin, uint32_t qend,
                                                            uint32_t p0, uint32_t p1, const uint32_t *koff, RunList out,
                                                            unsigned long long *counters,
                                                            const uint32_t *dk /* distinct mode: work item i = k-mer value dk[i] */,
                                                            uint32_t *nsim_k /* distinct mode: similar k-mers per work item */,
                                                            uint32_t item_stride /* distinct mode: every item_stride-th item only (run-count estimate) */,
                                                            const uint32_t *kbits = nullptr /* presence bitmap of the chunk's k-mers (nullable) */) {
    __shared__ SimTables tab;
    __shared__ uint32_t s_mul[K];
    __shared__ uint32_t s_n[4];
    __shared__ uint64_t s_val[4][RUN_STAGE];
    __shared__ uint32_t s_pi[4][RUN_STAGE];
    __shared__ uint32_t s_qv[4][LEAFQ], s_qp[4][LEAFQ], s_qm[4][LEAFQ];
    __shared__ uint32_t s_pc[4][POSQ], s_pp[4][POSQ];
    __shared__ uint64_t s_pr[4][POSQ];
    build_sim_tables(tab, db.S3);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // level L of the DFS decides k-mer position K - 1 - L, so the LAST level is the least significant digit of the k-mer value: the (up to 20) similar
    // k-mers under one five-letter prefix are consecutive values - one or two words of the presence bitmap, neighbouring entries of the offset table
    if (threadIdx.x < K) { uint32_t m = 1; for (int i = 0; i < K - 1 - (int)threadIdx.x; i++) m *= KA; s_mul[threadIdx.x] = m; }
    if (lane == 0) s_n[wv] = 0;
    __syncthreads();
    volatile uint32_t *vn = &s_n[wv];
    volatile uint64_t *vval = s_val[wv];
    volatile uint32_t *vpi = s_pi[wv];
    volatile uint32_t *qv = s_qv[wv], *qp = s_qp[wv], *qm = s_qm[wv];
    volatile uint32_t *pc = s_pc[wv], *pp = s_pp[wv];
    volatile uint64_t *pr = s_pr[wv];
    const int thr = cfg.thr, thrb = thr + 256;     // thrb: the threshold against the biased fields of restpack

    auto flush_runs = [&]() {   // whole wave
        const uint32_t n = *vn;
        uint32_t blo = 0, bhi = 0;
        if (lane == 0) {
            const unsigned long long b = atomicAdd(counters + 3, (unsigned long long)n);
            blo = (uint32_t)b; bhi = (uint32_t)(b >> 32);
        }
        blo = (uint32_t)__shfl((int)blo, 0, 64);
        bhi = (uint32_t)__shfl((int)bhi, 0, 64);
        const uint64_t base = ((uint64_t)bhi << 32) | blo;
        for (uint32_t k = lane; k < n; k += 64) {
            const uint64_t w = base + k;
            if (w < out.cap) { out.pidx[w] = vpi[k]; out.val[w] = vval[k]; }
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) *vn = 0;
        __builtin_amdgcn_wave_barrier();
    };
    unsigned long long nhit = 0;
    // A queued leaf GROUP is a five-letter prefix (its value with the last digit 0) and the mask of the last letters that keep the k-mer similar.  64 groups at a
    // time (whole wave): the group's 20 presence bits are one or two words of the bitmap; only the k-mers that occur in the index are looked up in the offset
    // table (neighbouring entries), and the non-empty index ranges are staged.  (r04 probed the bitmap and the table once per similar k-mer, 3.2e10 times per
    // configs[3] @ 500 call, the last level one DFS step per letter.)
    auto drain_leaves = [&](uint32_t qn) {
        for (uint32_t b = 0; b < qn; b += 64) {
            const uint32_t i = b + lane;
            uint32_t m = 0, v0 = 0, pi = 0;
            if (i < qn) {
                v0 = qv[i]; pi = qp[i]; m = qm[i];
                if (kbits) {
                    const uint32_t w = v0 >> 5, sh = v0 & 31;
                    const uint64_t two = (uint64_t)kbits[w] | ((uint64_t)(sh > 32 - KA ? kbits[w + 1] : 0u) << 32);
                    m &= (uint32_t)(two >> sh);
                }
            }
            // FOUR k-mers of a group per round trip: the kernel's waves spend two thirds of their cycles waiting (PMC, profiles/r05/sim_runs_filter_pmc.txt),
            // mostly for these dependent offset-table loads - eight of them in flight per lane instead of two
            while (__builtin_amdgcn_ballot_w64(m != 0) != 0) {
                uint32_t e0[4], n[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    e0[u] = 0; n[u] = 0;
                    if (m) {
                        const uint32_t v = v0 + (uint32_t)__builtin_ctz(m);
                        m &= m - 1;
                        e0[u] = koff[v];
                        n[u] = koff[v + 1];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t nn = n[u] - e0[u];           // (both 0 for a lane without a k-mer in this slot)
                    nhit += nn;
                    const uint64_t bm = __builtin_amdgcn_ballot_w64(nn != 0);
                    if (bm) {
                        if (*vn + 64 > RUN_STAGE) flush_runs();
                        const uint32_t slot = *vn + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
                        if (nn) { vval[slot] = ((uint64_t)nn << 32) | e0[u]; vpi[slot] = pi; }
                        __builtin_amdgcn_wave_barrier();
                        if (lane == 0) *vn = *vn + (uint32_t)__popcll(bm);
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        }
    };

    unsigned long long nsim = 0;
    const uint64_t npos = dk ? ((uint64_t)p1 - p0 + item_stride - 1) / item_stride : (uint64_t)p1 - p0;   // distinct mode: p1 - p0 items, sampled
    // one contiguous region per wave: the more positions a lane works through, the less the heaviest single position weighs
    const uint64_t nwaves = (uint64_t)gridDim.x * 4, region = (npos + nwaves - 1) / nwaves;
    {
        const uint64_t rg = (uint64_t)blockIdx.x * 4 + wv;
        // distinct mode: every wave walks the logical range [0, region) of its own stride-nwaves item sequence
        const uint64_t rbeg = dk ? 0 : min(rg * region, npos), rend = dk ? region : min(rbeg + region, npos);
        uint64_t next = rbeg;                      // wave-uniform cursor into the region
        uint32_t qn = 0;                           // wave-uniform fill of the leaf queue
        uint32_t head = 0, tail = 0;               // wave-uniform: pool of decoded positions (ring of POSQ entries)
        // per-lane DFS state
        bool idle = true, out_of_work = false;
        uint32_t cpack = 0, kpack = 0, pidx = 0, vcur = 0;
        uint32_t lc = 0;                           // leaves of the work item in hand
        bool has_item = false;
        int L = 0, scur = 0;
        uint64_t restpack = 0;                     // rest[m] (m = 1..6) in 10-bit fields, biased by 256: five letters of a matrix in [-48, 48] add -240 .. 240
        for (;;) {
            // ---- decode the next 64 positions together (sequence search + letter loads: ~10 us of dependent loads that
            //      must not sit in front of every single hand-out) ----
            if (tail - head <= POSQ - 64 && next < rend) {
                const uint64_t mine = next + lane;
                // distinct mode: k-mer values come sorted and neighbours cost alike, so a wave takes every nwaves-th item
                // instead of a contiguous region
                const uint64_t item = dk ? (mine * nwaves + rg) * item_stride : mine;
                bool ok = false;
                uint32_t cp = 0;
                uint64_t rp = 0;
                if (mine < rend && item < (dk ? (uint64_t)p1 - p0 : npos)) {
                    uint32_t q, i, c[K];
                    bool valid;
                    if (dk) {
                        uint32_t v = dk[item];
#pragma unroll
                        for (int m = 0; m < K; m++) { c[m] = v % (uint32_t)KA; v /= (uint32_t)KA; }
                        valid = true;
                    } else {
                        valid = query_kmer_at(db, cfg, qbegin, qend, p0 + (uint32_t)mine, &q, &i, c);
                    }
                    if (valid) {
                        int rest = 0;
#pragma unroll
                        for (int L_ = K - 1; L_ >= 0; L_--) {                         // level L_ decides position K - 1 - L_
                            rp |= (uint64_t)(uint32_t)(rest + 256) << (10 * L_);    // field L_ holds the best score the levels behind L_ can still add
                            rest += tab.rowmax[c[K - 1 - L_]];
                            cp |= c[K - 1 - L_] << (5 * L_);
                        }
                        ok = rest >= thr;
                    }
                }
                const uint64_t om = __builtin_amdgcn_ballot_w64(ok);
                if (ok) {
                    const uint32_t slot = (tail + (uint32_t)__popcll(om & ((1ull << lane) - 1ull))) % POSQ;
                    pc[slot] = cp; pr[slot] = rp; pp[slot] = (uint32_t)item;
                }
                tail += (uint32_t)__popcll(om);
                next = min(next + 64, rend);
                __builtin_amdgcn_wave_barrier();
                continue;
            }
            // ---- hand out decoded positions ----
            const uint64_t want = __builtin_amdgcn_ballot_w64(idle && !out_of_work);
            if (want) {
                const uint32_t take = head + (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                if (idle && !out_of_work) {
                    if (take < tail) {
                        if (nsim_k && has_item) nsim_k[pidx] = lc;
                        lc = 0; has_item = true;
                        const uint32_t slot = take % POSQ;
                        cpack = pc[slot]; restpack = pr[slot]; pidx = pp[slot];
                        kpack = 0; L = 0; scur = 0; vcur = 0; idle = false;
                    } else if (next >= rend) out_of_work = true;       // pool empty and nothing left to decode
                }
                head = min(head + (uint32_t)__popcll(want), tail);
            }
            if (__builtin_amdgcn_ballot_w64(!idle) == 0) {
                if (next >= rend && head == tail) break;                       // region exhausted
                continue;
            }
            // ---- one DFS node per lane, branch-free: probe (L, k[L]); descend, emit a leaf, or step back to level L-1 ----
            // (three divergent paths would run one after the other in nearly every step; selects cost fewer issue slots)
            bool leaf = false;
            uint32_t leafv = 0, leafm = 0;
            {
                const int Lm = L > 0 ? L - 1 : 0;
                const uint32_t a = (cpack >> (5 * L)) & 31u, k = (kpack >> (5 * L)) & 31u;
                const uint32_t a2 = (cpack >> (5 * Lm)) & 31u, k2 = (kpack >> (5 * Lm)) & 31u;
                const uint32_t kk = k < (uint32_t)KA ? k : 0u, kk2 = k2 < (uint32_t)KA ? k2 : 0u;
                const int sc1 = tab.sc[a][kk], sc2 = tab.sc[a2][kk2];
                const uint32_t o1 = tab.ord[a][kk], o2 = tab.ord[a2][kk2];
                const uint32_t mulL = s_mul[L], mulM = s_mul[Lm];
                const int restb = (int)((restpack >> (10 * L)) & 0x3ffu);       // still biased: compared against thr + 256
                const int cand = scur + sc1;
                const bool act = !idle;
                const bool ok = act && k < (uint32_t)KA && cand + restb >= thrb;
                const bool push = ok && L < K - 2, pop = act && !ok && L > 0;
                leaf = ok && L == K - 2;                                        // the last level is taken in one step: every letter that keeps cand + S >= thr
                leafv = vcur + o1 * mulL;
                {
                    const int need = min(max(thr - cand, -SIM_NEED_MAX), SIM_NEED_MAX);
                    const uint32_t al = (cpack >> (5 * (K - 1))) & 31u;
                    leafm = leaf ? tab.pmask[al][tab.lcnt[al][need + SIM_NEED_MAX]] : 0u;
                }
                lc += (uint32_t)__popc(leafm);
                idle = idle || (act && !ok && L == 0);
                scur = push ? cand : (pop ? scur - sc2 : scur);
                vcur = push ? leafv : (pop ? vcur - o2 * mulM : vcur);
                const uint32_t kp_leaf = kpack + (1u << (5 * (K - 2)));
                const uint32_t kp_push = kpack & ~(31u << (5 * (L + 1)));       // L + 1 <= K - 2 when push
                const uint32_t kp_pop = kpack + (1u << (5 * Lm));
                kpack = leaf ? kp_leaf : (push ? kp_push : (pop ? kp_pop : kpack));
                L = push ? L + 1 : (pop ? L - 1 : L);
            }
            const uint64_t lm = __builtin_amdgcn_ballot_w64(leaf);
            if (lm) {
                if (leaf) { const uint32_t slot = qn + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull)); qv[slot] = leafv; qp[slot] = pidx; qm[slot] = leafm; }
                qn += (uint32_t)__popcll(lm);
                nsim += (unsigned long long)__popc(leafm);
                if (qn > LEAFQ - 64) { __builtin_amdgcn_wave_barrier(); drain_leaves(qn); qn = 0; }
            }
        }
        __builtin_amdgcn_wave_barrier();
        drain_leaves(qn);
        if (nsim_k && has_item) nsim_k[pidx] = lc;
    }
    __builtin_amdgcn_wave_barrier();
    flush_runs();
    for (int o = 32; o > 0; o >>= 1) { nsim += __shfl_down(nsim, o, 64); nhit += __shfl_down(nhit, o, 64); }
    if (lane == 0) {
        if (nsim) atomicAdd(counters + 0, nsim);
        if (nhit) atomicAdd(counters + 4, nhit);
    }
}

// ---- E2, distinct mode: the similar k-mers of a k-mer do not depend on where it occurs, and a batch of queries holds every
// k-mer several times (C2: 46.0 M positions, 14.9 M distinct k-mers; the ratio grows with the database).  So the DFS and the
// offset-table lookups run once per DISTINCT k-mer of the batch, the resulting run lists are sorted by k-mer rank (a third of
// the runs, 24-bit keys) and a copy kernel lays them out per query position, already in position order - the big sort of
// all runs by position is gone.
__global__ void __launch_bounds__(256) query_kmer_kernel(const DeviceDb db, KmerCfg cfg, uint32_t qbegin, uint32_t qend, uint32_t p0, uint32_t p1,
                                                         uint32_t *qk, uint8_t *flag) {
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < p1 - p0; idx += (uint64_t)gridDim.x * 256) {
        uint32_t q, i, c[K];
        uint32_t key = KMER_INVALID;
        if (query_kmer_at(db, cfg, qbegin, qend, p0 + (uint32_t)idx, &q, &i, c)) {
            uint32_t v = 0, mul = 1;
#pragma unroll
            for (int m = 0; m < K; m++) { v += c[m] * mul; mul *= KA; }
            key = v;
            flag[v] = 1;
        }
        qk[idx] = key;
    }
}

struct FlagToU32 {
    __host__ __device__ uint32_t operator()(uint8_t x) const { return (uint32_t)x; }
};

__global__ void __launch_bounds__(256) distinct_kmer_kernel(const uint8_t *flag, const uint32_t *kid, uint32_t *dk) {
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < KSPACE; v += (uint64_t)gridDim.x * 256)
        if (flag[v]) dk[kid[v]] = (uint32_t)v;
}

// first run of every k-mer rank in the runs sorted by rank (nd + 1 entries), and the rank's hit total
__global__ void __launch_bounds__(256) rank_offsets_kernel(const uint32_t *rk, uint32_t n_runs, uint32_t nd, uint32_t *roff) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k <= nd; k += (uint64_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = n_runs;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (rk[mid] < (uint32_t)k) lo = mid + 1; else hi = mid;
        }
        roff[k] = lo;
    }
}

__global__ void __launch_bounds__(256) rank_rec_kernel(const uint32_t *roff, const uint64_t *val, const uint32_t *nsim_k, uint32_t nd, RankRec *rec) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < nd; k += (uint64_t)gridDim.x * 256) {
        uint64_t h = 0;
        const uint32_t r0 = roff[k], r1 = roff[k + 1];
        for (uint32_t r = r0; r < r1; r++) h += val[r] >> 32;
        RankRec x;
        x.roff = r0; x.nr = r1 - r0; x.nsim = nsim_k[k];
        x.hits = (uint32_t)min(h, (uint64_t)0xffffffffu);      // <= number of index entries < 2^32
        rec[k] = x;
    }
}

// per query position: runs, first run of its k-mer's list, k-mer hits; similar k-mers summed into counters[0]
__global__ void __launch_bounds__(256) position_runs_kernel(const uint32_t *qk, uint32_t npos, const uint32_t *kid, const RankRec *rec, uint32_t *nr,
                                                            uint32_t *src, uint32_t *ph, unsigned long long *counters) {
    unsigned long long sims = 0;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < npos; idx += (uint64_t)gridDim.x * 256) {
        const uint32_t v = qk[idx];
        RankRec x = {0, 0, 0, 0};
        if (v != KMER_INVALID) x = rec[kid[v]];
        nr[idx] = x.nr; src[idx] = x.roff; ph[idx] = x.hits;
        sims += x.nsim;
    }
    block_add(sims, counters + 0);
}

// per query: k-mer hits and runs (differences of the running sums over positions at the sequence boundaries)
__global__ void __launch_bounds__(256) query_totals_kernel(const uint32_t *off, uint32_t qbegin, uint32_t nq, uint32_t p0, const uint64_t *cumh,
                                                           const uint64_t *cumr, uint64_t *qh, uint64_t *qr) {
    for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256) {
        const uint32_t a = off[qbegin + q] - p0, b = off[qbegin + q + 1] - p0;
        qh[q] = cumh[b] - cumh[a];
        qr[q] = cumr[b] - cumr[a];
    }
}

// consumes max_len, the sequence count and the chunk's target range; produces the layout of the (query, target, diagonal) keys
KeyFmt key_format(const Engine &E, uint32_t tbegin, uint32_t tend) {
    KeyFmt fmt;
    const uint32_t m = std::min<uint32_t>(std::max<uint32_t>(E.max_len, 2), 65536u);
    fmt.dbits = 1;
    while ((1u << (fmt.dbits - 1)) < m) fmt.dbits++;
    fmt.dbias = 1 << (fmt.dbits - 1);
    fmt.tbits = 1;
    while ((1u << fmt.tbits) < E.hdb.n) fmt.tbits++;
    int rbits = 1;                                   // bits of a target id relative to this chunk
    while ((1ull << rbits) < (uint64_t)std::max<uint32_t>(tend - tbegin, 1)) rbits++;
    fmt.compact = rbits + fmt.dbits <= 32 && !getenv("UC_PREFILTER_WIDE");
    fmt.tbase = tbegin;
    return fmt;
}

// E1.  consumes the target chunk; produces its k-mer index (d_koff offsets, d_kbits presence bitmap, entries sorted by k-mer: d_ent wide [sequence : 32 |
// position : 16] or d_ent32 compact [sequence - tbegin | position : dbits - 1]), PP.fmt / ent_p / n_entries and the E1 stats
void build_index(Engine &E, PrefilterPass &PP) {
    PrefilterScratch &S = *E.pre;
    Timer t_index;
    E.timed_ms_begin();
    const uint32_t tp0 = E.h_poff[PP.tbegin], tp1 = E.h_poff[PP.tend];
    const uint32_t nres = tp1 - tp0;
    S.index.d_koff.reserve((size_t)KSPACE + 1);
    PP.fmt = key_format(E, PP.tbegin, PP.tend);
    const KeyFmt &fmt = PP.fmt;
    const size_t cap = std::max<uint32_t>(nres, 1);
    S.index.k_in.reserve(cap); S.index.k_out.reserve(cap);
    if (fmt.compact) { S.index.v_in32.reserve(cap); S.index.d_ent32.reserve(cap); PP.ent_p = S.index.d_ent32.p; }
    else { S.index.v_in.reserve(cap); S.index.d_ent.reserve(cap); PP.ent_p = S.index.d_ent.p; }
    if (nres) {
        hipLaunchKernelGGL(kmer_extract_kernel, grid_for(nres), dim3(256), 0, E.stream, E.ddb, PP.tbegin, PP.tend, PP.cfg, tp0, tp1, S.index.k_in.p,
                           fmt.compact ? nullptr : S.index.v_in.p, fmt.compact ? S.index.v_in32.p : nullptr, fmt.dbits - 1);
        if (fmt.compact)
            rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, S.index.k_in.p, S.index.k_out.p, S.index.v_in32.p, S.index.d_ent32.p, (size_t)nres, 0u, 32u, E.stream); });
        else
            rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, S.index.k_in.p, S.index.k_out.p, S.index.v_in.p, S.index.d_ent.p, (size_t)nres, 0u, 32u, E.stream); });
    }
    // number of valid entries = first index with key >= KSPACE: the offsets kernel's last slot
    hipLaunchKernelGGL(kmer_offsets_kernel, grid_for((uint64_t)KSPACE + 1), dim3(256), 0, E.stream, S.index.k_out.p, nres, S.index.d_koff.p);
    S.index.d_kbits.reserve((KSPACE + 31) / 32);
    hipLaunchKernelGGL(kmer_bits_kernel, grid_for((KSPACE + 31) / 32), dim3(256), 0, E.stream, (const uint32_t *)S.index.d_koff.p, S.index.d_kbits.p);
    UC_HIP(hipMemcpyAsync(&PP.n_entries, S.index.d_koff.p + KSPACE, 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    UC_HIP(hipGetLastError());
    PP.gpu_ms = E.timed_ms_end();
    E.stats.n_index_entries += PP.n_entries;
    E.stats.algorithmic_bytes[UC_ST_INDEX] += 6ull * PP.n_entries + 8ull * KSPACE;
    E.stats.stage_seconds[UC_ST_INDEX] += t_index.seconds();
}

dim3 sim_grid(uint64_t items) {
    return dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (items + 4 * SIM_MIN_WAVE_POS - 1) / (4 * SIM_MIN_WAVE_POS)), SIM_MAX_BLOCKS));
}

// consumes the nd distinct k-mers; produces the index ranges ("runs") of their similar k-mers tagged with the k-mer's rank (d_drk / d_drv, n_druns of
// them in buffers of drun_cap) and d_nsimk.  Returns 0, or the run count (estimated or exact) that exceeds DRUN_MAX: the super-batch has to be cut
uint64_t distinct_runs(Engine &E, PrefilterPass &PP, const SuperBatch &SB, uint32_t nd, uint64_t &n_druns, uint64_t &drun_cap) {
    PrefilterScratch &S = *E.pre;
    const uint32_t nqa = SB.end - SB.begin;
    if (nqa > 1 && nd > (1u << 16)) {   // run-count estimate from every 64th distinct k-mer: cut the super-batch BEFORE the full enumeration
        const uint32_t st = 64;
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 3, 0, 32, E.stream));
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p, 0, 8, E.stream));
        hipLaunchKernelGGL(sim_runs_kernel, sim_grid((nd + st - 1) / st), dim3(256), 0, E.stream, E.ddb, PP.cfg, 0u, 0u, 0u, nd, S.index.d_koff.p, RunList{nullptr, nullptr, 0},
                           S.shared.d_counters.p, S.plan.d_dk.p, (uint32_t *)nullptr, st, (const uint32_t *)S.index.d_kbits.p);
        unsigned long long c5[5];
        UC_HIP(hipMemcpyAsync(c5, S.shared.d_counters.p, 40, hipMemcpyDeviceToHost, E.stream));
        UC_HIP(hipStreamSynchronize(E.stream));
        if ((double)c5[3] * st > 0.9 * (double)PP.DRUN_MAX) return (uint64_t)((double)c5[3] * st / 0.9);
    }
    n_druns = 0; drun_cap = S.plan.d_drk.cap;
    for (;;) {   // runs of the distinct k-mers, tagged with the k-mer's rank
        drun_cap = std::min<uint64_t>(1ull << 32, std::max<uint64_t>(drun_cap, std::max<uint64_t>(1u << 20, std::min<uint64_t>(PP.DRUN_MAX, (uint64_t)nd * 16))));
        S.plan.d_drk.reserve(drun_cap); S.plan.d_drv.reserve(drun_cap);
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 3, 0, 32, E.stream));
        UC_HIP(hipMemsetAsync(S.shared.d_counters.p, 0, 8, E.stream));
        const RunList rl{S.plan.d_drk.p, S.plan.d_drv.p, drun_cap};
        hipLaunchKernelGGL(sim_runs_kernel, sim_grid(nd), dim3(256), 0, E.stream, E.ddb, PP.cfg, 0u, 0u, 0u, nd, S.index.d_koff.p, rl, S.shared.d_counters.p, S.plan.d_dk.p, S.plan.d_nsimk.p, 1u,
                           (const uint32_t *)S.index.d_kbits.p);
        unsigned long long c5[5];
        UC_HIP(hipMemcpyAsync(c5, S.shared.d_counters.p, 40, hipMemcpyDeviceToHost, E.stream));
        UC_HIP(hipStreamSynchronize(E.stream));
        n_druns = c5[3];
        if (getenv("UC_TIMING")) fprintf(stderr, "unicore-cluster[timing]: similar k-mers of %u distinct k-mers: %llu index runs\n", nd, (unsigned long long)n_druns);
        if (n_druns > PP.DRUN_MAX && nqa > 1) return n_druns;
        if (n_druns > drun_cap) {
            if (n_druns >= (1ull << 32)) fail(UC_ERR_GENERIC, "%u distinct k-mers of query %u produce %llu index ranges", nd, SB.begin, (unsigned long long)n_druns);
            drun_cap = n_druns;
            UC_HIP(hipMemsetAsync(S.plan.d_nsimk.p, 0, (size_t)std::max<uint32_t>(nd, 1) * 4, E.stream));
            continue;
        }
        return 0;
    }
}

// ---- distinct mode, once per target chunk and query "super-batch" [sa, sb) (normally all queries; cut when the run lists
//      of its distinct k-mers exceed DRUN_MAX, i.e. at high sensitivity): similar k-mers and index ranges of every
//      DISTINCT query k-mer, then per query position the length and source of its run list and its k-mer hits; exact
//      per-query totals for the batch plan ----
// consumes the index and queries [sa, sb); produces SB and the sorted runs (d_drv2) with d_nr / d_src / d_cumr per position and d_qh / d_qrn per query, which the filter reads
PlanResult plan_superbatch(Engine &E, PrefilterPass &PP, SuperBatch &SB, uint32_t sa, uint32_t sb) {
    PrefilterScratch &S = *E.pre;
    uint64_t plan_hits = 0;
    SB.begin = sa; SB.end = sb;
    SB.P0 = E.h_poff[sa]; SB.NP = E.h_poff[sb] - SB.P0;
    const uint32_t NP = SB.NP, nqa = sb - sa;
    Timer t_p;
    E.timed_ms_begin();
    S.plan.d_qk.reserve((size_t)NP + 1); S.plan.d_kflag.reserve((size_t)KSPACE + 1); S.plan.d_kid.reserve((size_t)KSPACE + 1);
    UC_HIP(hipMemsetAsync(S.plan.d_kflag.p, 0, (size_t)KSPACE + 1, E.stream));
    hipLaunchKernelGGL(query_kmer_kernel, grid_for(NP), dim3(256), 0, E.stream, E.ddb, PP.cfg, sa, sb, SB.P0, SB.P0 + NP, S.plan.d_qk.p, S.plan.d_kflag.p);
    auto fin = rocprim::make_transform_iterator(S.plan.d_kflag.p, FlagToU32());
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, fin, S.plan.d_kid.p, 0u, (size_t)KSPACE + 1, rocprim::plus<uint32_t>(), E.stream); });
    uint32_t nd = 0;                           // distinct k-mers of the super-batch: d_kid ranks every k-mer among them, d_dk lists them
    UC_HIP(hipMemcpyAsync(&nd, S.plan.d_kid.p + KSPACE, 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    S.plan.d_dk.reserve(std::max<uint32_t>(nd, 1)); S.plan.d_nsimk.reserve(std::max<uint32_t>(nd, 1));
    UC_HIP(hipMemsetAsync(S.plan.d_nsimk.p, 0, (size_t)std::max<uint32_t>(nd, 1) * 4, E.stream));
    hipLaunchKernelGGL(distinct_kmer_kernel, grid_for(KSPACE), dim3(256), 0, E.stream, S.plan.d_kflag.p, S.plan.d_kid.p, S.plan.d_dk.p);
    uint64_t n_druns = 0, drun_cap = 0;
    if (const uint64_t over_runs = distinct_runs(E, PP, SB, nd, n_druns, drun_cap)) {
        PP.gpu_ms += E.timed_ms_end();
        PP.t_kmer += t_p.seconds();
        return {PlanStatus::too_many_runs, over_runs};
    }
    unsigned dbits = 1;
    while ((1ull << dbits) < nd) dbits++;
    S.plan.d_drk2.reserve(drun_cap); S.plan.d_drv2.reserve(drun_cap);
    if (n_druns)
        rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, S.plan.d_drk.p, S.plan.d_drk2.p, S.plan.d_drv.p, S.plan.d_drv2.p, (size_t)n_druns, 0u, dbits, E.stream); });
    S.plan.d_roff.reserve((size_t)nd + 1); S.plan.d_rec.reserve(std::max<uint32_t>(nd, 1));
    hipLaunchKernelGGL(rank_offsets_kernel, grid_for((uint64_t)nd + 1), dim3(256), 0, E.stream, S.plan.d_drk2.p, (uint32_t)n_druns, nd, S.plan.d_roff.p);
    if (nd) hipLaunchKernelGGL(rank_rec_kernel, grid_for(nd), dim3(256), 0, E.stream, S.plan.d_roff.p, S.plan.d_drv2.p, S.plan.d_nsimk.p, nd, S.plan.d_rec.p);
    // per position (one trailing zero element so that the exclusive sums end with the totals)
    S.plan.d_nr.reserve((size_t)NP + 1); S.plan.d_src.reserve((size_t)NP + 1); S.plan.d_ph.reserve((size_t)NP + 1);
    S.plan.d_cumh.reserve((size_t)NP + 1); S.plan.d_cumr.reserve((size_t)NP + 1);
    UC_HIP(hipMemsetAsync(S.shared.d_counters.p, 0, 8, E.stream));
    UC_HIP(hipMemsetAsync(S.plan.d_nr.p + NP, 0, 4, E.stream));
    UC_HIP(hipMemsetAsync(S.plan.d_ph.p + NP, 0, 4, E.stream));
    hipLaunchKernelGGL(position_runs_kernel, grid_for(NP, E.count_grid_cap), dim3(256), 0, E.stream, S.plan.d_qk.p, NP, S.plan.d_kid.p, S.plan.d_rec.p, S.plan.d_nr.p, S.plan.d_src.p, S.plan.d_ph.p, S.shared.d_counters.p);
    auto hin = rocprim::make_transform_iterator(S.plan.d_ph.p, WidenU32());
    auto rin = rocprim::make_transform_iterator(S.plan.d_nr.p, WidenU32());
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, hin, S.plan.d_cumh.p, (uint64_t)0, (size_t)NP + 1, rocprim::plus<uint64_t>(), E.stream); });
    rocprim_call(S.shared.d_temp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, rin, S.plan.d_cumr.p, (uint64_t)0, (size_t)NP + 1, rocprim::plus<uint64_t>(), E.stream); });
    S.plan.d_qh.reserve(nqa); S.plan.d_qrn.reserve(nqa);
    hipLaunchKernelGGL(query_totals_kernel, grid_for(nqa), dim3(256), 0, E.stream, E.ddb.off, sa, nqa, SB.P0, S.plan.d_cumh.p, S.plan.d_cumr.p, S.plan.d_qh.p, S.plan.d_qrn.p);
    SB.h_qh.resize(nqa); SB.h_qr.resize(nqa);
    unsigned long long c0 = 0;
    UC_HIP(hipMemcpyAsync(SB.h_qh.data(), S.plan.d_qh.p, (size_t)nqa * 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipMemcpyAsync(SB.h_qr.data(), S.plan.d_qrn.p, (size_t)nqa * 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipMemcpyAsync(&c0, S.shared.d_counters.p, 8, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    for (uint32_t i = 0; i < nqa; i++) plan_hits += SB.h_qh[i];
    SB.hit_cap = plan_hits > 16 * PP.HIT_CAP ? PP.HIT_CAP_BIG : PP.HIT_CAP;
    PP.gpu_ms += E.timed_ms_end();
    PP.t_kmer += t_p.seconds();
    if (sa == PP.qbegin) {
        if (PP.density_out) *PP.density_out = (double)plan_hits / std::max<uint32_t>(1, NP);
        if (PP.density_limit > 0 && E.p.min_diag_hits >= 2 && PP.tend - PP.tbegin > 1 && (double)plan_hits / std::max<uint32_t>(1, NP) > PP.density_limit)
            return {PlanStatus::too_dense, 0};
    }
    if (PP.count_sims) E.stats.n_sim_kmers += c0;
    return {PlanStatus::planned, 0};
}

// consumes the first query qa without a plan; produces the plan of the next super-batch, as large as the run lists allow.  false: the chunk is too dense
bool choose_superbatch(Engine &E, PrefilterPass &PP, SuperBatch &SB, uint32_t qa) {
    for (;;) {
        const uint32_t left = PP.qend - qa;
        const uint32_t sb = SB.frac >= 1.0 ? PP.qend : qa + std::max<uint32_t>(1, std::min<uint32_t>(left, (uint32_t)(left * SB.frac)));
        const PlanResult r = plan_superbatch(E, PP, SB, qa, sb);
        if (r.status == PlanStatus::too_dense) {   // undo what this abandoned attempt counted
            E.stats.n_index_entries -= PP.n_entries;
            E.stats.algorithmic_bytes[UC_ST_INDEX] -= 6ull * PP.n_entries + 8ull * KSPACE;
            E.stats.prefilter_kernel_ms += PP.gpu_ms;
            return false;
        }
        if (r.status == PlanStatus::too_many_runs) {   // distinct k-mers grow sublinearly with the queries: cut a little deeper than proportionally
            SB.frac = (double)(sb - qa) / left * 0.8 * (double)PP.DRUN_MAX / (double)r.over_runs;
            continue;
        }
        if (SB.frac < 1.0) SB.frac = std::min(1.0, (double)(sb - qa) / std::max<uint32_t>(1, PP.qend - sb));   // the same number of queries again
        return true;
    }
}

// consumes the plan of SB and the first query qa; produces the exact batch [qa, qb).  It launches nothing: the batch's runs stay where the plan left them
QueryBatch cut_batch(Engine &E, PrefilterPass &PP, const SuperBatch &SB, uint32_t qa) {
    PrefilterScratch &S = *E.pre;
    QueryBatch B;
    B.qa = B.qb = qa;
    uint64_t mirror_hits = 0;
    // exact plan: as many queries as fit the key and run buffers (a single query may exceed them and takes the wide path)
    while (B.qb < SB.end && B.qb - qa < (1u << 23) - 1) {
        const uint64_t h = SB.h_qh[B.qb - SB.begin], r = SB.h_qr[B.qb - SB.begin];
        if (B.qb > qa && (B.total_hits + h > SB.hit_cap || B.n_runs + r > RUN_MAX)) break;
        B.total_hits += h; B.n_runs += r;
        if (B.qb >= PP.mirror_q0) mirror_hits += h;       // these hits stand for the hits of the pairs the other way round as well
        B.qb++;
    }
    if (B.n_runs >= (1ull << 32)) fail(UC_ERR_GENERIC, "query %u alone produces %llu index ranges", qa, (unsigned long long)B.n_runs);
    B.qp0 = E.h_poff[qa]; B.qp1 = E.h_poff[B.qb]; B.nq_res = B.qp1 - B.qp0;
    B.plan_p0 = SB.P0; B.plan_q0 = SB.begin;
    UC_HIP(hipMemsetAsync(S.shared.d_counters.p + 3, 0, 32, E.stream));   // run cursor, batch hits, key cursor, candidate cursor
    if (B.total_hits > (1ull << 34)) fail(UC_ERR_GENERIC, "query %u alone produces %llu k-mer hits", qa, (unsigned long long)B.total_hits);
    PP.n_hits_total += B.total_hits + mirror_hits;
    unsigned qbits = 1;
    while ((1u << qbits) < B.qb - qa) qbits++;
    B.kbits = (unsigned)(PP.fmt.dbits + PP.fmt.tbits) + qbits;
    return B;
}

void preload_kmer_match_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)kmer_extract_kernel); }
}  // namespace uc
