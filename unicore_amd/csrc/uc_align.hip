// uc_align.hip — stage E5/E6 orchestration, device-resident.
// The prefilter leaves its hit lists in HBM; everything between them and the accepted edge list stays on
// the GPU: the planner sorts the pairs by (length class, query, target length), cuts them into workgroup
// tasks and gathers the kernel inputs; the gates (E-value on the corrected score, coverage) are small
// kernels with scan-based compaction.  The host only sees a handful of counters and, at the end, the
// accepted edges (stands for Foldseek's structurealign result handling; spec UC-1 E5/E6).
// Work that is never launched: the reversed-query pass of pairs below the E-value threshold (UC-1.1),
// and one of the two DPs of a mutual hit (q,t)/(t,q) in the forward, reversed-query, start and traceback passes
// whenever the result of the other orientation is provably the transposed one.
#include <mutex>
#include <hip/hip_runtime.h>

#include <cmath>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_engine.h"

namespace uc {

constexpr int SW_PK_OVF_HOST = 0x7C00 - 256;   // == SW_PK_OVF of uc_sw_pk_impl.hpp

// scratch for the traceback-byte matrices of one batch (MODE 7): up to 64 GiB (r06; 144 GiB until r05), never more than 55 % of what
// is free right now (plus what the scratch buffer already holds); UC_TB_BUDGET_MB overrides (tests).  Why 64: taking device memory costs 25-40 ms per GiB
// whenever the box's memory is not warm for this process (one 108 GiB buffer: 4.2 s of a 14 s call at 500 proteomes in the first process on a fresh box,
// profiles/r06/c4_p500_alloc.txt), while the batches a smaller buffer adds cost a launch tail each (r05: halving the batches of nominal configs[3] cost 3 %
// of the pass)
// The plan of a MODE 7 call costs ~110 B per pair beside the matrices: the flagged list is worked off in segments of 32 M pairs (nominal
// configs[3]: 170 M flagged pairs per 256 M-pair batch of the stage), each planned and cut into matrix batches on its own; a segment
// still holds ~1.5 TB of matrices, i.e. dozens of one-class batches.  (Tests: a forced matrix budget also forces 1000-pair segments.)
struct TbBudget {
    unsigned long long forced = 0;   // UC_TB_BUDGET_MB in bytes, 0 if unset
    TbBudget() {
        if (const char *e = getenv("UC_TB_BUDGET_MB")) forced = std::max<unsigned long long>(1, strtoull(e, nullptr, 10)) << 20;
    }
    uint32_t segment_pairs() const { return forced ? 1000u : (32u << 20); }
    // matrix bytes of one batch, for a segment whose matrices take `total` bytes and a buffer that holds `held` already
    unsigned long long batch_bytes(unsigned long long total, size_t held) const {
        if (forced) return forced;
        size_t free_b = 0, total_b = 0;
        unsigned long long cap = 64ull << 30;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            cap = std::min<unsigned long long>(cap, (unsigned long long)((free_b + held) * 0.55));
        const unsigned long long budget = std::max<unsigned long long>(cap, 256ull << 20);
        // Fresh device memory is not free: 25-60 ms per GiB on a box whose memory has been used before (tools/ubench/alloc_cost.hip,
        // profiles/r04/alloc_*.log), so a call whose matrices would fit a few times over takes a third of them at a time, at least
        // 16 GiB (about the buffer r04 took for an eighth of its whole-box matrices).  What the buffer already holds is free to use.
        // A buffer of a useful size that is there already IS the budget: a segment whose batches would be a little larger than
        // the last one's must not take a new block (r06)
        if (held >= ((size_t)8 << 30)) return (unsigned long long)held - 64;
        const unsigned long long want = std::max<unsigned long long>(16ull << 30, total / 3);
        return std::min(budget, std::max<unsigned long long>(want, (unsigned long long)held));
    }
};

namespace {

// Length classes.  Table 0: int32 kernel for everything (16 systolic classes + the row-blocked long-query kernel).  Table 1: the packed
// 16-bit kernel for all systolic classes: queries <= 2048 rows in 28 classes with even R (~6R + 60 live registers).
constexpr int MAXCLS = 28;
struct ClassTable {
    int n;                 // systolic classes; index n = long queries (> cap[n-1] rows): uc_sw_long.hip
    int cap[MAXCLS], G[MAXCLS], R[MAXCLS], pk[MAXCLS];
    uint32_t tcap[MAXCLS]; // pairs per workgroup task
};
// pairs per task: the long-query classes have few queries, so their pair lists are cut finer to keep every
// CU busy (rebuilding the LDS profile per task is negligible against >= 16 long alignments)
const ClassTable h_tab[4] = {
    {16,
     {64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024, 1280, 1536, 1792, 2048},
     {16, 16, 16, 16, 16, 16, 16, 16, 32, 32, 32, 32, 64, 64, 64, 64},
     {4, 8, 12, 16, 20, 24, 28, 32, 20, 24, 28, 32, 20, 24, 28, 32},
     {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
     {256, 256, 256, 256, 256, 256, 256, 256, 64, 64, 64, 64, 24, 24, 24, 24}},
    {28,
     {32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384, 448, 512, 576, 640, 704, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048},
     {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 32, 32, 32, 32, 32, 32, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64},
     {2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 14, 16, 18, 20, 22, 24, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32},
     {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
     {64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 48, 48, 48, 48, 48, 48, 24, 24, 24, 24}},
    // Table 2: the int32 kernel in MODE 3 (traceback statistics) carries two more register arrays: R <= 16 keeps it at
    // <= 193 VGPRs without AGPR/scratch spills up to 1024 rows (R = 24..32 needed 275-353 registers and spilled)
    {12,
     {64, 128, 192, 256, 384, 512, 768, 1024, 1280, 1536, 1792, 2048},
     {16, 16, 16, 16, 32, 32, 64, 64, 64, 64, 64, 64},
     {4, 8, 12, 16, 12, 16, 12, 16, 20, 24, 28, 32},
     {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
     {256, 256, 256, 256, 64, 64, 24, 24, 24, 24, 24, 24}},
    // Table 3 (r06): the packed kernel for SPARSE plans - the known-score passes that re-run a handful of pairs per query (MODE 4: ambiguous end rows;
    // the second MODE 6 round: mirrors that could not take their partner's start).  With one or two pairs per query a task is ONE slot: in the classes of
    // table 1 it keeps one lane group of its workgroup busy (G = 16: an eighth of the lanes) while every wave instruction is issued for all of them - those
    // passes ran at 1.5-2.1 T cells/s against 5-6 T for the dense ones (profiles/r05/sw_pass_timing_c2_c3.txt).  Here every class spans the whole wave
    // (G = 64, R = rows / 64): the one slot of a task uses all 64 lanes; the price is the longer pipeline fill (Lt + 63 steps) and fewer rows per step to
    // amortise the per-step overhead, still ~2x fewer issued instructions per sparse pair.  R < 14: two-wave workgroups (sw_pk_kernel<64, R, 4|6, 2>).
    {16,
     {128, 256, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048},
     {64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64},
     {2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32},
     {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
     {8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16}},
};
__device__ __constant__ ClassTable c_tab[4];
// which table a known-score pass of the packed path plans with: sparse (table 3) when the plan holds fewer than 2.5 pairs per query of the call
// (UC_SW_SPARSE=0: always table 1, for A/B runs; results do not depend on the table - every class computes the exact DP)
static int pk_known_tab(uint32_t n_pairs, uint32_t n_queries) {
    static const bool on = !(getenv("UC_SW_SPARSE") && atoi(getenv("UC_SW_SPARSE")) == 0);
    return on && (double)n_pairs < 2.5 * (double)n_queries ? 3 : 1;
}

// Mutual hits take both tie-break answers from one known-score DP (uc_sw_pk_impl.hpp key2).  UC_DUAL_TIEBREAK=0: the earlier sharing rule, for A/B
// runs - a mirror shares only where one row holds every optimal cell and is otherwise computed on its own.  The records are the same either way.
static bool dual_tiebreak_on() {
    static const bool on = !(getenv("UC_DUAL_TIEBREAK") && atoi(getenv("UC_DUAL_TIEBREAK")) == 0);
    return on;
}

__device__ __forceinline__ int class_of(int lq, int tab) {
    int c = 0;
    while (c < c_tab[tab].n && c_tab[tab].cap[c] < lq) c++;
    return c;
}
__device__ __forceinline__ uint32_t task_cap(int c, int tab) { return c < c_tab[tab].n ? c_tab[tab].tcap[c] : SW_LONG_TASK_PAIRS; }   // long queries: one pair per wave (uc_sw_long.hip)

// key = [ class : 5 | query : 24 | 65535 - effective target length : 16 ]
__global__ void __launch_bounds__(256) plan_key_kernel(uint32_t n, const uint32_t *q, const uint32_t *t, const int32_t *qe,
                                                       const int32_t *te, const int32_t *qs, const int32_t *ts,
                                                       const uint32_t *len, int tab, uint64_t *key, uint32_t *idx,
                                                       unsigned long long *alg_bytes /* [0] bytes, [1] DP cells */) {
    unsigned long long bytes = 0, cells = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t qq = q[i];
        const uint32_t lq = len[qq];
        const uint32_t tl = te ? (uint32_t)(te[i] + 1 - (ts ? ts[i] : 0)) : len[t[i]];
        const uint32_t ql = qe ? (uint32_t)(qe[i] + 1 - (qs ? qs[i] : 0)) : lq;
        key[i] = ((uint64_t)class_of((int)lq, tab) << 40) | ((uint64_t)qq << 16) | (uint64_t)(65535u - tl);
        idx[i] = i;
        bytes += 2ull * (ql + tl) + 32;
        cells += (unsigned long long)ql * tl;
    }
    block_add2(bytes, cells, alg_bytes, alg_bytes + 1);
}

__global__ void __launch_bounds__(256) plan_gather_kernel(uint32_t n, const uint64_t *key, const uint32_t *idx, const uint32_t *t,
                                                          const int32_t *qe, const int32_t *te, const int32_t *qs, const int32_t *ts,
                                                          uint32_t *sq, uint32_t *st, int32_t *sqe, int32_t *ste, int32_t *sqs,
                                                          int32_t *sts, uint32_t *head) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint64_t k = key[i];
        const uint32_t o = idx[i];
        sq[i] = (uint32_t)(k >> 16) & 0xFFFFFFu;
        st[i] = t[o];
        if (qe) { sqe[i] = qe[o]; ste[i] = te[o]; }
        if (qs) { sqs[i] = qs[o]; sts[i] = ts[o]; }
        head[i] = (i == 0 || (key[i - 1] >> 16) != (k >> 16)) ? i : 0u;
    }
}

__global__ void __launch_bounds__(256) plan_aux_kernel(uint32_t n, const uint32_t *idx, const int32_t *aux, int32_t *saux) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) saux[i] = aux[idx[i]];
}

__global__ void __launch_bounds__(256) plan_taskflag_kernel(uint32_t n, const uint64_t *key, const uint32_t *segstart, int tab, uint32_t *flag) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        flag[i] = ((i - segstart[i]) % task_cap((int)(key[i] >> 40), tab)) == 0 ? 1u : 0u;
}

__global__ void __launch_bounds__(256) plan_taskfill_kernel(uint32_t n, const uint64_t *key, const uint32_t *flag, const uint32_t *tpos,
                                                            SwTask *tasks, uint32_t *tcls) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint64_t k = key[i];
        const uint32_t w = tpos[i];
        tasks[w].q = (uint32_t)(k >> 16) & 0xFFFFFFu;
        tasks[w].begin = i;
        tcls[w] = (uint32_t)(k >> 40);
    }
}

// count per task + an LPT sort key: [ class : 5 | ~work : 32 ], work = pairs x longest target of the task
__global__ void __launch_bounds__(256) plan_taskcount_kernel(uint32_t ntasks, uint32_t n, SwTask *tasks, const uint32_t *tcls,
                                                             const uint64_t *key, uint64_t *tkey, uint32_t *tidx) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < ntasks; k += gridDim.x * 256) {
        const uint32_t b = tasks[k].begin;
        const uint32_t cnt = (k + 1 < ntasks ? tasks[k + 1].begin : n) - b;
        tasks[k].count = cnt;
        const uint32_t work = cnt * (65535u - (uint32_t)(key[b] & 0xFFFF));
        tkey[k] = ((uint64_t)tcls[k] << 32) | (uint64_t)(0xFFFFFFFFu - work);
        tidx[k] = k;
    }
}

__global__ void __launch_bounds__(256) plan_taskgather_kernel(uint32_t ntasks, const uint32_t *tidx, const SwTask *in, SwTask *out) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < ntasks; k += gridDim.x * 256) out[k] = in[tidx[k]];
}

// bounds[c] = first task of class >= c, bounds[NB + c] = first sorted pair of class >= c   (c = 0..NB-1)
constexpr int NB = MAXCLS + 2;
__global__ void plan_bounds_kernel(uint32_t ntasks, const uint32_t *tcls, uint32_t n, const uint64_t *key, uint32_t *bounds) {
    const uint32_t c = threadIdx.x;
    if (c >= NB) return;
    uint32_t lo = 0, hi = ntasks;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (tcls[m] < c) lo = m + 1; else hi = m; }
    bounds[c] = lo;
    lo = 0; hi = n;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if ((uint32_t)(key[m] >> 40) < c) lo = m + 1; else hi = m; }
    bounds[NB + c] = lo;
}

__global__ void __launch_bounds__(256) scatter3_kernel(uint32_t n, const uint32_t *idx, const int32_t *a, const int32_t *b,
                                                       const int32_t *c, int32_t *oa, int32_t *ob, int32_t *oc) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t o = idx[i];
        oa[o] = a[i];
        if (b) { ob[o] = b[i]; oc[o] = c[i]; }
    }
}

// ---- gates --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gate_kernel(uint32_t n, const uint32_t *sq, const int32_t *s0, const int32_t *s1,
                                                   const int32_t *minscore, uint32_t qbase, uint32_t *flag) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int32_t rev = s1 ? s1[i] : 0;
        flag[i] = (s0[i] > 0 && s0[i] - rev >= minscore[sq[i] - qbase]) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(256) pair_gather_kernel(uint32_t n, const uint32_t *flag, const uint32_t *pos, const uint32_t *sq,
                                                          const uint32_t *st, uint32_t *q1, uint32_t *t1, uint32_t *link) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        q1[w] = sq[i]; t1[w] = st[i]; link[w] = i;
    }
}
// results of a sub-plan (sorted order idx over the gathered list) back to the parent list's positions
__global__ void __launch_bounds__(256) rev_putback_kernel(uint32_t n1, const uint32_t *idx1, const uint32_t *link, const int32_t *s, int32_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n1; i += gridDim.x * 256) out[link[idx1[i]]] = s[i];
}

// ---- mutual hits: (q,t) and (t,q) have the same forward and reversed-query score when both substitution
// matrices are symmetric (the recurrence treats the two gap directions alike), so one DP serves both ----
// key = [ min(q,t) : 24 | max(q,t) : 24 | direction : 1 ]; direction 0 = the orientation with the shorter query
// (fewer DP rows -> smaller systolic group -> less pipeline fill per pair; ties: q < t)
__global__ void __launch_bounds__(256) ukey_kernel(uint32_t n, const uint32_t *q, const uint32_t *t, const uint32_t *len,
                                                   uint64_t *key, uint32_t *idx) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t a = q[i], b = t[i], lo = min(a, b), hi = max(a, b);
        const uint32_t la = len[a], lb = len[b];
        const uint32_t worse = (la > lb || (la == lb && a > b)) ? 1u : 0u;
        key[i] = ((((uint64_t)lo << 24) | hi) << 1) | worse;
        idx[i] = i;
    }
}
// over the key-sorted list: entry j is a mirror iff its predecessor is the same unordered pair
__global__ void __launch_bounds__(256) umark_kernel(uint32_t n, const uint64_t *key, const uint32_t *idx, const uint32_t *q,
                                                    const uint32_t *t, uint32_t *fq, uint32_t *ft, uint32_t *mirror, uint32_t *rep) {
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const uint32_t m = (j > 0 && (key[j] >> 1) == (key[j - 1] >> 1)) ? 1u : 0u;
        mirror[j] = m;
        rep[j] = m ^ 1u;
        fq[j] = q[idx[j]];
        ft[j] = t[idx[j]];
    }
}
__global__ void __launch_bounds__(256) ugather_kernel(uint32_t n, const uint32_t *rep, const uint32_t *rpos, const uint32_t *fq,
                                                      const uint32_t *ft, uint32_t *qr, uint32_t *tr, uint32_t *jrep) {
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        if (!rep[j]) continue;
        const uint32_t w = rpos[j];
        qr[w] = fq[j]; tr[w] = ft[j]; jrep[w] = j;
    }
}
// forward results of the representatives (plan order) -> full key-sorted list.  A mirror gets the score; its end
// position is the representative's end with the roles swapped WHEN the packed kernel saw exactly one query row
// reach the optimum (then that row's first optimal column is the overall first optimal column, so both tie-break
// orders pick the same cell).  Otherwise it gets the "end unknown" mark (-2), which the exact re-run resolves for
// the pairs that pass the E-value gate.  k < n_pk: the representative ran in a packed class (unique-row guarantee).
__global__ void __launch_bounds__(256) uscatter_kernel(uint32_t nu, uint32_t n, const uint32_t *pidx, const uint32_t *jrep,
                                                       const uint32_t *mirror, const int32_t *su, const int32_t *qeu, const int32_t *teu,
                                                       uint32_t n_pk, int ovf, int32_t *s0, int32_t *qe0, int32_t *te0) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nu; k += gridDim.x * 256) {
        const uint32_t j = jrep[pidx[k]];
        s0[j] = su[k]; qe0[j] = qeu[k]; te0[j] = teu[k];
        if (j + 1 < n && mirror[j + 1]) {
            const bool swap_ok = k < n_pk && su[k] < ovf && qeu[k] >= 0;
            s0[j + 1] = su[k];
            qe0[j + 1] = su[k] > 0 ? (swap_ok ? teu[k] : -2) : -1;
            te0[j + 1] = su[k] > 0 ? (swap_ok ? qeu[k] : -2) : -1;
        }
    }
}
// reversed-query pass: a flagged mirror whose representative is flagged too takes its value instead of running
__global__ void __launch_bounds__(256) rev_dedup_kernel(uint32_t n, const uint32_t *mirror, uint32_t *flag, uint32_t *copy) {
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) copy[j] = (mirror[j] && flag[j] && flag[j - 1]) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) rev_unflag_kernel(uint32_t n, const uint32_t *copy, uint32_t *flag) {
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) if (copy[j]) flag[j] = 0;
}
__global__ void __launch_bounds__(256) rev_copy_kernel(uint32_t n, const uint32_t *copy, int32_t *s1) {
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) if (copy[j]) s1[j] = s1[j - 1];
}
// algorithmic DP cells (Lq x Lt) of the listed (optionally flagged) pairs
__global__ void __launch_bounds__(256) cells_kernel(uint32_t n, const uint32_t *q, const uint32_t *t, const uint32_t *flag,
                                                    const uint32_t *len, unsigned long long *out) {
    unsigned long long c = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (!flag || flag[i]) c += (unsigned long long)len[q[i]] * len[t[i]];
    block_add(c, out);
}

// ---- start pass shared between mutual hits ----
// The start pass of (q,t) with end cell (qe,te) and the one of its mirror (t,q) with end cell (te,qe) are transposed
// DPs.  If the packed kernel saw exactly ONE row of the representative's DP reach the optimum, both tie-break orders
// select the same cell, so the mirror's result is the representative's with the roles swapped; otherwise the mirror
// is computed on its own (second round).
__global__ void __launch_bounds__(256) sm_flag_kernel(uint32_t n2, const uint32_t *link, const uint32_t *mirror, const uint32_t *gflag,
                                                      const uint32_t *gpos, const int32_t *qe2, const int32_t *te2, const int32_t *qe0,
                                                      const int32_t *te0, uint32_t *keep, uint32_t *partner) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const uint32_t j = link[i];
        const bool sm = mirror[j] && j > 0 && gflag[j - 1] && qe0[j - 1] >= 0 && qe2[i] == te0[j - 1] && te2[i] == qe0[j - 1];
        keep[i] = sm ? 0u : 1u;
        partner[i] = sm ? gpos[j - 1] : 0xFFFFFFFFu;
    }
}
__global__ void __launch_bounds__(256) sm_gather_kernel(uint32_t n2, const uint32_t *flag, const uint32_t *pos, const uint32_t *q2,
                                                        const uint32_t *t2, const int32_t *qe2, const int32_t *te2, uint32_t *qa,
                                                        uint32_t *ta, int32_t *qea, int32_t *tea, uint32_t *map) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        qa[w] = q2[i]; ta[w] = t2[i]; qea[w] = qe2[i]; tea[w] = te2[i]; map[w] = i;
    }
}
// results of a sub-plan (plan order k) -> natural order of the gate-passer list; uniq = the packed known-score kernel
// found every optimal cell in one row (SW_TE_UNIQUE on the column output; results of the int32 kernel never carry it).
// qo2 / to2 (optional): the second answer of the packed known-score kernel (-2 where the result came from another kernel)
__global__ void __launch_bounds__(256) sm_scatter_kernel(uint32_t na, const uint32_t *idx, const uint32_t *map, const int32_t *s,
                                                         const int32_t *qo, const int32_t *to, int32_t *s2,
                                                         int32_t *q2o, int32_t *t2o, uint32_t *uniq,
                                                         const int32_t *qo2, const int32_t *to2, int32_t *q2o2, int32_t *t2o2) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < na; k += gridDim.x * 256) {
        const uint32_t i = map ? map[idx[k]] : idx[k];
        const int32_t te = to[k];
        const bool u = te >= 0 && (te & SW_TE_UNIQUE) != 0;
        s2[i] = s[k]; q2o[i] = qo[k]; t2o[i] = te >= 0 ? (te & ~SW_TE_UNIQUE) : te;
        if (uniq) uniq[i] = (u && qo[k] >= 0) ? 1u : 0u;
        if (q2o2) { q2o2[i] = qo2[k]; t2o2[i] = to2[k]; }
    }
}
// a mirror takes its partner's second answer (first optimal row, then first column of the partner's DP = first optimal column, then first row
// of its own, transposed one) with the roles swapped.  Where the partner has none (q2o2 null or -2: its result is not the packed known-score
// kernel's) the one-row rule decides: share the first answer if a single row holds every optimal cell, else a run of its own (-2, round 2)
__global__ void __launch_bounds__(256) sm_resolve_kernel(uint32_t n2, const uint32_t *partner, const uint32_t *uniq, int32_t *s2,
                                                         int32_t *q2o, int32_t *t2o, const int32_t *q2o2, const int32_t *t2o2) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const uint32_t pr = partner[i];
        if (pr == 0xFFFFFFFFu) continue;
        if (q2o2 && q2o2[pr] >= 0 && t2o2[pr] >= 0) { s2[i] = s2[pr]; q2o[i] = t2o2[pr]; t2o[i] = q2o2[pr]; }
        else if (uniq[pr]) { s2[i] = s2[pr]; q2o[i] = t2o[pr]; t2o[i] = q2o[pr]; }
        else q2o[i] = -2;
    }
}
// the start pass reaches exactly the forward score: known score of entry k of a gathered sub-list
__global__ void __launch_bounds__(256) sm_score_kernel(uint32_t nb, const uint32_t *map, const uint32_t *link, const int32_t *s0, int32_t *out) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nb; k += gridDim.x * 256) out[k] = s0[link[map[k]]];
}
__global__ void __launch_bounds__(256) iota_kernel(uint32_t n, uint32_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = i;
}
// rule UC-1/L (optional): flag = the lengths of the pair leave the coverage threshold reachable (float division, as the checker's)
__global__ void __launch_bounds__(256) len_gate_kernel(uint32_t n, const uint32_t *q, const uint32_t *t, const uint32_t *len, float cov, int cov_mode,
                                                       uint32_t *flag) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float ql = (float)len[q[i]], tl = (float)len[t[i]];
        const bool ok = len[q[i]] && len[t[i]] &&
                        (cov_mode == 0 ? (ql / tl >= cov && tl / ql >= cov) : cov_mode == 1 ? (ql / tl >= cov) : (tl / ql >= cov));
        flag[i] = ok ? 1u : 0u;
    }
}
__global__ void __launch_bounds__(256) len_gate_gather_kernel(uint32_t n, const uint32_t *flag, const uint32_t *pos, const uint32_t *q, const uint32_t *t,
                                                              uint32_t *qc, uint32_t *tc, uint32_t *map) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        qc[w] = q[i]; tc[w] = t[i]; map[w] = i;
    }
}
// records of the compacted pair list -> their places in the hit-list order (the gated pairs keep the all-zero record)
__global__ void __launch_bounds__(256) len_gate_putback_kernel(uint32_t nc, const uint32_t *map, const uc_aln *src, uc_aln *dst) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nc; i += gridDim.x * 256) dst[map[i]] = src[i];
}
// algorithmic cells of the traceback pass: the box of every entry whose statistics are asked for
__global__ void __launch_bounds__(256) cells_tb_kernel(uint32_t n2, const uint32_t *eflag, const uint32_t *link, const uint32_t *idx0, const uc_aln *alns,
                                                       unsigned long long *out) {
    unsigned long long c = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256)
        if (eflag[i]) {
            const uc_aln a = alns[idx0[link[i]]];
            c += (unsigned long long)(a.qend - a.qstart + 1) * (unsigned long long)(a.tend - a.tstart + 1);
        }
    block_add(c, out);
}
// algorithmic cells of the start pass: (qEnd+1) x (tEnd+1) per gate passer
__global__ void __launch_bounds__(256) cells_box_kernel(uint32_t n, const int32_t *qe, const int32_t *te, unsigned long long *out) {
    unsigned long long c = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) c += (unsigned long long)(qe[i] + 1) * (unsigned long long)(te[i] + 1);
    block_add(c, out);
}

__global__ void __launch_bounds__(256) gate_scatter_kernel(uint32_t n, const uint32_t *flag, const uint32_t *pos, const uint32_t *sq,
                                                           const uint32_t *st, const int32_t *qe, const int32_t *te, uint32_t *q2,
                                                           uint32_t *t2, int32_t *qe2, int32_t *te2, uint32_t *link) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        q2[w] = sq[i]; t2[w] = st[i]; qe2[w] = qe[i]; te2[w] = te[i]; link[w] = i;
    }
}

__global__ void __launch_bounds__(256) aln_basic_kernel(uint32_t n, const uint32_t *idx, const int32_t *s0, const int32_t *s1,
                                                        const int32_t *qe, const int32_t *te, const uint32_t *pass, uc_aln *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        uc_aln a;
        a.score = s0[i]; a.score_rev = s1 ? s1[i] : 0; a.corrected = a.score - a.score_rev;
        // positions are only defined (and only exact) for pairs that pass the E-value gate
        a.qstart = -1; a.qend = pass[i] ? qe[i] : -1; a.tstart = -1; a.tend = pass[i] ? te[i] : -1;
        a.aln_len = 0; a.idents = 0; a.pass_evalue = (int32_t)pass[i]; a.accepted = 0; a.gap_opens = 0;
        out[idx[i]] = a;
    }
}

// over the start-pass results (sorted order of plan 2): start positions, coverage gate, edge flag
__global__ void __launch_bounds__(256) finalize_kernel(uint32_t n2, const uint32_t *idx2, const uint32_t *link, const uint32_t *idx0,
                                                       const uint32_t *sq2, const uint32_t *st2, const int32_t *s2, const int32_t *q2o,
                                                       const int32_t *t2o, const uint32_t *len, float cov, int cov_mode, uc_aln *alns,
                                                       uint32_t *eflag, uint32_t *mismatch) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        uc_aln &a = alns[idx0[link[idx2[i]]]];
        if (s2[i] != a.score) atomicAdd(mismatch, 1u);
        a.qstart = a.qend - q2o[i];
        a.tstart = a.tend - t2o[i];
        const float qcov = (float)(a.qend - a.qstart + 1) / (float)len[sq2[i]];
        const float tcov = (float)(a.tend - a.tstart + 1) / (float)len[st2[i]];
        const bool ok = cov_mode == 0 ? (qcov >= cov && tcov >= cov) : cov_mode == 1 ? (tcov >= cov) : (qcov >= cov);
        a.accepted = ok;
        eflag[i] = ok;
    }
}

// seq-id stage (only with --min-seq-id > 0): pairs that passed the coverage gate get their traceback statistics
// Every statistic of a traceback travels in a 32-bit word of its own, the count in bits 0..30 and the gap-direction tie mark of the walk that
// counted it in bit 31: alignment length (at most lq + lt = 131,070 columns), identities (at most 65,535), gaps (at most the length).  One word
// cannot hold two of them: 17 + 16 bits and the mark.
constexpr uint32_t TB_COUNT = 0x7FFFFFFFu;
constexpr uint32_t TB_BAND_MISS = 0x7FFFFFFFu;     // in the length word: "the walk left the stored band" (no traceback has 2^31 - 1 columns)
__global__ void __launch_bounds__(256) tb_gather_kernel(uint32_t n2, const uint32_t *eflag, const uint32_t *epos, const uint32_t *idx2,
                                                        const uint32_t *link, const uint32_t *idx0, const uint32_t *sq2, const uint32_t *st2,
                                                        const uc_aln *alns, uint32_t *q3, uint32_t *t3, int32_t *qs3, int32_t *qe3,
                                                        int32_t *ts3, int32_t *te3, uint32_t *src3, int32_t *sc3) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        if (!eflag[i]) continue;
        const uint32_t w = epos[i], o = idx0[link[idx2[i]]];
        const uc_aln a = alns[o];
        q3[w] = sq2[i]; t3[w] = st2[i]; qs3[w] = a.qstart; qe3[w] = a.qend; ts3[w] = a.tstart; te3[w] = a.tend;
        src3[w] = i;
        sc3[w] = a.score;                                   // H of the box's end cell: where the walk over the H bytes starts
    }
}
__global__ void __launch_bounds__(256) tb_apply_kernel(uint32_t n3, const uint32_t *idx3, const uint32_t *src3, const int32_t *pack,
                                                       const int32_t *ident, const int32_t *gaps, const uint32_t *idx2, const uint32_t *link, const uint32_t *idx0,
                                                       float min_seq_id, uc_aln *alns, uint32_t *eflag, uint32_t *tie, uint32_t *miss) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n3; i += gridDim.x * 256) {
        const uint32_t i2 = src3[idx3[i]];
        uc_aln &a = alns[idx0[link[idx2[i2]]]];
        const uint32_t pk = (uint32_t)pack[i];
        if (miss) {                                          // banded MODE 7: the walk left the stored band - the record is not touched, the pair is redone
            miss[i2] = pk == TB_BAND_MISS;
            if (pk == TB_BAND_MISS) continue;
        }
        a.aln_len = (int32_t)(pk & TB_COUNT);
        a.idents = (int32_t)((uint32_t)ident[i] & TB_COUNT);
        if (tie) tie[i2] = pk >> 31;
        if (gaps) a.gap_opens = (int32_t)((uint32_t)gaps[i] & TB_COUNT);
        if (min_seq_id > 0.0f) {
            const float sid = a.aln_len > 0 ? (float)a.idents / (float)a.aln_len : 0.0f;
            const bool ok = sid >= min_seq_id;
            a.accepted = ok;
            eflag[i2] = ok;
        }
    }
}

// ---- traceback bytes (packed MODE 7) + walk --------------------------------------------------------------------
// bytes of pair p's matrix: (longer box of its slot + G + 4) steps x NL lanes (those inside the pair's band, tb_band_of) x RB row bytes; the
// slot partner is the neighbour inside the workgroup task (pairs 2i, 2i+1 of the task), see sw_pk_kernel::start_slot
__global__ void __launch_bounds__(256) tb_size_kernel(uint32_t n_pk, const uint64_t *key, const uint32_t *segstart, const int32_t *ste,
                                                      const int32_t *sts, const int32_t *sqs, const int32_t *sqe, int band, int tab, unsigned long long *size) {
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_pk; p += gridDim.x * 256) {
        const int cls = (int)(key[p] >> 40);
        const uint32_t tcap = task_cap(cls, tab), seg = segstart[p];
        const uint32_t tb = seg + (p - seg) / tcap * tcap, pp = tb + ((p - tb) ^ 1u);
        int tl = ste[p] - sts[p] + 1;
        if (pp < n_pk && segstart[pp] == seg && (pp - seg) / tcap == (p - seg) / tcap && (key[pp] >> 16) == (key[p] >> 16))
            tl = max(tl, ste[pp] - sts[pp] + 1);
        const int G = c_tab[tab].G[cls], R = c_tab[tab].R[cls], RB = 4 * ((R + 3) / 4);
        const int nl = tb_band_of(sqs[p], sqe[p], ste[p] - sts[p] + 1, G, R, band).nl;     // lanes per step inside the pair's stored band
        size[p] = (unsigned long long)(tl + G + 4) * (unsigned long long)(nl * RB);      // (the kernel's step count is rounded up to its loop trip of 2 or 4 steps)
    }
}
// one thread per pair walks its matrix of H bytes (packed MODE 7) from the end cell (oracle: traceback(), diag > F > E, a gap is left
// as soon as it can be): alignment length | tie << 31, identities and the number of gaps, a word each.
// The end cell's H is the pair's score; a cell next to one whose H is known differs from it by less than 128 (vertical / horizontal
// neighbours: -open .. M + open, diagonal: min score .. M, M = the largest substitution score; the host checks M + open <= 127 and
// sends everything else through the int32 pass), so its byte gives its H exactly.  Every decision the traceback takes is a comparison
// of such values:  diagonal iff H(i,j) == H(i-1,j-1) + s(i,j);  H(i,j) == F(i,j) iff some k has H(i-k,j) - open - (k-1) ext == H(i,j),
// and the search up the column ends at the first k with H(i-k,j) < H(i,j) + k ext (F <= H in every cell, so no gap that long or longer
// can reach H(i,j));  inside a gap of value f the gap was opened from the neighbour iff H(neighbour) - open == f.  E likewise along the row.
//
// Backtraces (-a).  EMIT = 0: statistics only, the kernel of every call without -a.  EMIT = 1: the same walk also counts the runs of its path
// (maximal stretches of one operation: M diagonal, I query residue only, D target residue only) into bt_cnt[p], 0 for a pair that left its band.
// EMIT = 2: the walk again, writing run r of pair p as (length << 2 | op) into its slice bt_runs[bt_off[p] ..+ bt_cnt[p]) FROM THE TAIL (the walk goes
// from the end of the alignment to its start), and where the slice lies in the engine's buffer into bt_pos[p].  A run that would fall outside
// the slice is not written and raises *bt_err (the counts come from the same walk over the same bytes, so this never happens).
// PLAIN = 1: the matrix is not the packed kernel's banded byte layout but a row-major int32 H of the box (tb_plain_dp_kernel), for the pairs the
// packed kernel does not serve; everything else is the same walk.
constexpr uint32_t BT_M = 0u, BT_I = 1u, BT_D = 2u, BT_NONE = 3u;
template <int EMIT>
struct BtSink {
    uint32_t op = BT_NONE, len = 0, n = 0;
    uint32_t *out = nullptr;     // the pair's slice
    int w = 0;                   // next slot, counting down
    bool ovf = false;
    __device__ __forceinline__ void flush() {
        if (op == BT_NONE) return;
        if (EMIT == 2) { if (w >= 0) out[w] = (len << 2) | op; else ovf = true; w--; }
        n++;
    }
    __device__ __forceinline__ void step(uint32_t o) {
        if (o == op) { len++; return; }
        flush();
        op = o; len = 1;
    }
};
template <int EMIT, int PLAIN>
__global__ void __launch_bounds__(256) tb_walk_kernel(uint32_t p_begin, uint32_t n_pk /* pairs [p_begin, n_pk) of the plan */, const DeviceDb db, const uint64_t *key, const uint32_t *st,
                                                      const int32_t *sqs, const int32_t *sqe, const int32_t *sts, const int32_t *ste,
                                                      const int32_t *score, int open, int ext, int band,
                                                      int tab, const uint8_t *tbm, const unsigned long long *tboff, int32_t *pack,
                                                      int32_t *ident_out, int32_t *gaps_out, uint32_t *bt_cnt, const uint32_t *bt_off, uint32_t *bt_runs,
                                                      unsigned long long bt_base, unsigned long long *bt_pos, uint32_t *bt_plain, uint32_t *bt_err) {
    __shared__ int8_t s_S3[21 * 21], s_SA[21 * 21];
    for (int k = threadIdx.x; k < 21 * 21; k += 256) { s_S3[k] = db.S3[k]; s_SA[k] = db.SA[k]; }
    __syncthreads();
    for (uint32_t p = p_begin + blockIdx.x * 256 + threadIdx.x; p < n_pk; p += gridDim.x * 256) {
        if (EMIT == 2 && bt_cnt[p] == 0) continue;                    // left its band: nothing to write, the pair is redone
        const int cls = (int)(key[p] >> 40);
        const uint32_t q = (uint32_t)(key[p] >> 16) & 0xFFFFFFu, t = st[p];
        const int G = PLAIN ? 1 : c_tab[tab].G[cls], R = PLAIN ? 1 : c_tab[tab].R[cls], RB = 4 * ((R + 3) / 4);
        const int qs = sqs[p], ts = sts[p];
        const TbBand bd = PLAIN ? TbBand{1, 0, 0} : tb_band_of(qs, sqe[p], ste[p] - ts + 1, G, R, band);
        const bool full = PLAIN || bd.nl >= G;
        const unsigned long long trow = (unsigned long long)(bd.nl * RB);
        bool miss = false;           // the walk asked for a cell outside the stored band: the pair is redone with the whole box stored
        const uint8_t *m = tbm + tboff[p];
        const int32_t *m32 = (const int32_t *)m;                      // PLAIN: H(ii, jj) at (ii - qs) * pw + (jj - ts)
        const size_t pw = (size_t)(ste[p] - ts + 1);
        const uint16_t *ql = db.lt + db.off[q], *tl = db.lt + db.off[t];   // 3Di | AA << 8 per residue
        BtSink<EMIT> sink;
        if (EMIT == 2) { sink.out = bt_runs + bt_off[p]; sink.w = (int)bt_cnt[p] - 1; }
        // full H of cell (ii, jj), a neighbour of a cell (or gap state) whose value is within 127 of it: ref
        auto H_at = [&](int ii, int jj, int ref) -> int {
            if (ii < qs || jj < ts) return 0;
            if (PLAIN) return m32[(size_t)(ii - qs) * pw + (size_t)(jj - ts)];
            const int lane = ii / R, stp = jj - ts + lane;
            if (!full && (stp < lane * (R + 1) - bd.dhi || stp > lane * (R + 1) + R - 1 - bd.dlo)) { miss = true; return ref; }
            const uint32_t b = m[(unsigned long long)stp * trow + (unsigned long long)((lane % bd.nl) * RB + (ii - lane * R))];
            return ref + (int)(int8_t)(uint8_t)(b - (uint32_t)ref);
        };
        int i = sqe[p], j = ste[p], state = 0;
        int h = PLAIN ? m32[(size_t)(sqe[p] - qs) * pw + (size_t)(ste[p] - ts)] : score[p];   // state 0: H(i,j);  states 1 / 2: the value of the gap state the walk is in
        uint32_t len = 0, id = 0, gaps = 0, tie = 0;
        while (i >= qs && j >= ts && !miss) {
            if (state == 0) {
                if (h <= 0) break;                                      // H == 0
                // A traceback is mostly diagonal steps, and a step's three loads (two residues, the byte of the diagonal neighbour) depend on the path
                // taken so far, not on loaded values: the next SPEC diagonal steps are fetched together and then taken one by one from registers - one
                // memory round trip per run of up to SPEC matches instead of one per step (r05: the walk, one thread per pair on the engine's stream
                // behind every MODE 7 batch, had grown to a fifth of the pass).
                constexpr int SPEC = 8;      // (r06: 16 measured - SW + traceback kernels of configs[3] options @ 500 8,090 -> 8,230 ms: longer runs are rarer than the registers and wasted fetches cost)
                uint32_t lqv[SPEC], ltv[SPEC], bv[SPEC];                // bv: the neighbour's byte; 0x100 = outside the box (H = 0), 0x200 = outside the band
#pragma unroll
                for (int k = 0; k < SPEC; k++) {
                    const int ii = i - k, jj = j - k;
                    const bool in = ii >= qs && jj >= ts;
                    lqv[k] = in ? ql[ii] : 0u;
                    ltv[k] = in ? tl[jj] : 0u;
                    uint32_t b = 0x100u;
                    if (PLAIN) b = (in && ii - 1 >= qs && jj - 1 >= ts) ? (uint32_t)m32[(size_t)(ii - 1 - qs) * pw + (size_t)(jj - 1 - ts)] : 0u;   // H itself
                    else if (in && ii - 1 >= qs && jj - 1 >= ts) {
                        const int lane = (ii - 1) / R, stp = jj - 1 - ts + lane;
                        if (!full && (stp < lane * (R + 1) - bd.dhi || stp > lane * (R + 1) + R - 1 - bd.dlo)) b = 0x200u;
                        else b = m[(unsigned long long)stp * trow + (unsigned long long)((lane % bd.nl) * RB + (ii - 1 - lane * R))];
                    }
                    bv[k] = b;
                }
                bool off_diag = false;
                uint32_t lq = 0, lt = 0;
#pragma unroll
                for (int k = 0; k < SPEC; k++) {
                    if (off_diag || miss || i < qs || j < ts || h <= 0) continue;
                    lq = lqv[k]; lt = ltv[k];
                    if (!PLAIN && bv[k] == 0x200u) { miss = true; continue; }
                    const int hd = PLAIN ? (int)bv[k] : bv[k] == 0x100u ? 0 : h + (int)(int8_t)(uint8_t)(bv[k] - (uint32_t)h);
                    const int sc = (int)s_S3[(lq & 0xffu) * 21 + (lt & 0xffu)] + (int)s_SA[(lq >> 8) * 21 + (lt >> 8)];
                    if (h == hd + sc) { len++; id += (lq >> 8) == (lt >> 8); i--; j--; h = hd; if (EMIT) sink.step(BT_M); }
                    else off_diag = true;
                }
                if (!off_diag) continue;                                // the run ended on a diagonal step (or the walk is over): next run
                bool fv = false, ev = false;
                {
                    int hu = h;
                    for (int k = 1; i - k >= qs; k++) {
                        hu = H_at(i - k, j, hu);
                        if (hu == h + open + (k - 1) * ext) { fv = true; break; }
                        if (hu < h + k * ext) break;
                    }
                }
                if (fv) {   // the tie mark: H == E as well (the transposed path of a mutual hit would take the other gap first)
                    int hl = h;
                    for (int k = 1; j - k >= ts; k++) {
                        hl = H_at(i, j - k, hl);
                        if (hl == h + open + (k - 1) * ext) { ev = true; break; }
                        if (hl < h + k * ext) break;
                    }
                    tie |= ev ? 1u : 0u;
                    state = 1;
                } else state = 2;
                gaps++;
            } else if (state == 1) {                                    // gap consuming query residue i, value h = F(i,j)
                len++;
                if (EMIT) sink.step(BT_I);
                if (i - 1 < qs) state = 0;
                else {
                    const int hu = H_at(i - 1, j, h);                   // F(i,j) = max(F(i-1,j) - ext, H(i-1,j) - open): ext .. open above h
                    if (hu - open == h) { state = 0; h = hu; } else h += ext;
                }
                i--;
            } else {                                                    // gap consuming target residue j, value h = E(i,j)
                len++;
                if (EMIT) sink.step(BT_D);
                if (j - 1 < ts) state = 0;
                else {
                    const int hl = H_at(i, j - 1, h);
                    if (hl - open == h) { state = 0; h = hl; } else h += ext;
                }
                j--;
            }
        }
        if (EMIT) sink.flush();
        if (EMIT == 2) {
            if (sink.ovf || sink.w != -1) atomicOr(bt_err, 1u);
            bt_pos[p] = bt_base + bt_off[p];
            bt_plain[p] = PLAIN;
            continue;                                                  // the statistics were written by the counting walk
        }
        if (EMIT == 1) bt_cnt[p] = miss ? 0u : sink.n;
        pack[p] = miss ? (int32_t)TB_BAND_MISS : (int32_t)(len | (tie << 31));
        ident_out[p] = (int32_t)id;
        if (gaps_out) gaps_out[p] = (int32_t)gaps;
    }
}
// byte offset of the first matrix of every task of the traceback plan (the batches are cut at task boundaries)
__global__ void __launch_bounds__(256) tb_taskoff_kernel(uint32_t ntasks, const SwTask *tasks, const unsigned long long *tboff, unsigned long long *out) {
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < ntasks; k += gridDim.x * 256) out[k] = tboff[tasks[k].begin];
}
// ---- the stored-matrix pass of the pairs the packed kernel does not serve (backtraces only) --------------------------------------
// Scores beyond the packed range, queries beyond the systolic classes and the all-int32 configuration take their statistics from int32 MODE 3, which
// carries them through the DP and stores nothing.  With -a those pairs need a path: a plain int32 DP of the box that keeps H of every cell, row-major,
// and the walk above with that address function (PLAIN).  int32 per cell whatever the matrices and gap costs (no byte-difference argument needed).
// One workgroup per pair, one anti-diagonal per barrier; E of the cell to the left lives per row, F of the cell above per column (each is touched by
// exactly one thread per anti-diagonal).  Rare routes: simple, not fast.
// bytes of pair p: 4 * (rows * cols + rows + cols), rounded up to 8
__global__ void __launch_bounds__(256) tb_plain_size_kernel(uint32_t p_begin, uint32_t p_end, const int32_t *sqs, const int32_t *sqe, const int32_t *sts,
                                                            const int32_t *ste, unsigned long long *size) {
    for (uint32_t p = p_begin + blockIdx.x * 256 + threadIdx.x; p < p_end; p += gridDim.x * 256) {
        const unsigned long long r = (unsigned long long)(sqe[p] - sqs[p] + 1), c = (unsigned long long)(ste[p] - sts[p] + 1);
        size[p] = (4ull * (r * c + r + c) + 7ull) & ~7ull;
    }
}
__global__ void __launch_bounds__(256) tb_plain_dp_kernel(uint32_t p_begin, uint32_t p_end, const DeviceDb db, const uint64_t *key, const uint32_t *st,
                                                          const int32_t *sqs, const int32_t *sqe, const int32_t *sts, const int32_t *ste, int open, int ext,
                                                          uint8_t *tbm, const unsigned long long *tboff) {
    __shared__ int8_t s_S3[21 * 21], s_SA[21 * 21];
    for (int k = threadIdx.x; k < 21 * 21; k += 256) { s_S3[k] = db.S3[k]; s_SA[k] = db.SA[k]; }
    __syncthreads();
    for (uint32_t p = p_begin + blockIdx.x; p < p_end; p += gridDim.x) {
        const uint32_t q = (uint32_t)(key[p] >> 16) & 0xFFFFFFu, t = st[p];
        const int nr = sqe[p] - sqs[p] + 1, nc = ste[p] - sts[p] + 1;
        const uint16_t *ql = db.lt + db.off[q] + sqs[p], *tl = db.lt + db.off[t] + sts[p];
        int32_t *H = (int32_t *)(tbm + tboff[p]);
        int32_t *Er = H + (size_t)nr * (size_t)nc, *Fc = Er + nr;
        constexpr int32_t NEG = -(1 << 28);
        for (int k = threadIdx.x; k < nr + nc; k += 256) Er[k] = NEG;
        __syncthreads();
        for (int d = 0; d < nr + nc - 1; d++) {
            const int lo = max(0, d - nc + 1), hi = min(nr - 1, d);
            for (int i = lo + (int)threadIdx.x; i <= hi; i += 256) {
                const int j = d - i;
                const size_t at = (size_t)i * (size_t)nc + (size_t)j;
                const int hl = j > 0 ? H[at - 1] : 0, hu = i > 0 ? H[at - (size_t)nc] : 0, hd = (i > 0 && j > 0) ? H[at - (size_t)nc - 1] : 0;
                const uint32_t lq = ql[i], lt = tl[j];
                const int sc = (int)s_S3[(lq & 0xffu) * 21 + (lt & 0xffu)] + (int)s_SA[(lq >> 8) * 21 + (lt >> 8)];
                const int e = max(Er[i] - ext, hl - open), f = max(Fc[j] - ext, hu - open);
                H[at] = max(max(0, hd + sc), max(e, f));
                Er[i] = e; Fc[j] = f;
            }
            __syncthreads();
        }
    }
}
// the slices of the walked pairs of a traceback plan -> the per-record (position, runs) pair of the batch; a pair that left its band writes nothing
constexpr uint32_t BT_SWAP = 0x80000000u, BT_PLAIN = 0x40000000u;    // marks in the per-record run count: I / D exchanged when read; served by the stored-matrix pass
__global__ void __launch_bounds__(256) bt_apply_kernel(uint32_t n3, const uint32_t *idx3, const uint32_t *src3, const uint32_t *cnt, const unsigned long long *pos,
                                                       const uint32_t *plain, const uint32_t *idx2, const uint32_t *link, const uint32_t *idx0,
                                                       unsigned long long *rpos, uint32_t *rn) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n3; i += gridDim.x * 256) {
        if (!cnt[i]) continue;
        const uint32_t o = idx0[link[idx2[src3[idx3[i]]]]];
        rpos[o] = pos[i];
        rn[o] = cnt[i] | (plain[i] ? BT_PLAIN : 0u);
    }
}
// a mirror that took its representative's statistics (tbm_resolve_kernel) takes its slice too: the transposed path is the same runs with I and D exchanged
__global__ void __launch_bounds__(256) bt_mirror_kernel(uint32_t n2, const uint32_t *partner, const uint32_t *tie, const uint32_t *link, const uint32_t *idx0,
                                                        unsigned long long *rpos, uint32_t *rn) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const uint32_t pr = partner[i];
        if (pr == 0xFFFFFFFFu || tie[pr]) continue;
        const uint32_t om = idx0[link[i]], orp = idx0[link[pr]];
        rpos[om] = rpos[orp];
        rn[om] = rn[orp] ^ BT_SWAP;
    }
}
__global__ void __launch_bounds__(256) bt_putback_kernel(uint32_t nc, const uint32_t *map, const unsigned long long *spos, const uint32_t *sn,
                                                         unsigned long long *dpos, uint32_t *dn) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nc; i += gridDim.x * 256) { dpos[map[i]] = spos[i]; dn[map[i]] = sn[i]; }
}
// accepted pairs by forward score: the packed DP of MODE 7 is only valid below its score range
__global__ void __launch_bounds__(256) tb_split_kernel(uint32_t n2, const uint32_t *flag, const uint32_t *link, const uint32_t *idx0,
                                                       const uc_aln *alns, int ovf, uint32_t *lo, uint32_t *hi) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const bool big = flag[i] && alns[idx0[link[i]]].score >= ovf;
        lo[i] = flag[i] && !big;
        hi[i] = big;
    }
}
__global__ void __launch_bounds__(256) tb_chunk_kernel(uint32_t n2, const uint32_t *flag, const uint32_t *pos, uint32_t lo, uint32_t hi, uint32_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) out[i] = (flag[i] && pos[i] >= lo && pos[i] < hi) ? 1u : 0u;
}

// traceback statistics shared between mutual hits: the box of (t,q) is the transposed box of (q,t); if the
// representative's traceback never had to choose between the two gap directions, the mirror's path is the transposed
// path and (alignment length, identities, gaps) are the same
__global__ void __launch_bounds__(256) tbm_flag_kernel(uint32_t n2, const uint32_t *eflag, const uint32_t *link, const uint32_t *idx0,
                                                       const uint32_t *mirror, const uint32_t *gflag, const uint32_t *gpos,
                                                       const uc_aln *alns, uint32_t *run, uint32_t *partner) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        uint32_t r = eflag[i], pr = 0xFFFFFFFFu;
        if (r) {
            const uint32_t j = link[i];
            if (mirror[j] && j > 0 && gflag[j - 1]) {
                const uint32_t ir = gpos[j - 1];
                if (eflag[ir]) {
                    const uc_aln am = alns[idx0[j]], ar = alns[idx0[j - 1]];
                    if (am.qstart == ar.tstart && am.qend == ar.tend && am.tstart == ar.qstart && am.tend == ar.qend) { r = 0; pr = ir; }
                }
            }
        }
        run[i] = r;
        partner[i] = pr;
    }
}
__global__ void __launch_bounds__(256) tbm_resolve_kernel(uint32_t n2, const uint32_t *partner, const uint32_t *tie, const uint32_t *link,
                                                          const uint32_t *idx0, float min_seq_id, uc_aln *alns, uint32_t *eflag_out,
                                                          uint32_t *run2) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const uint32_t pr = partner[i];
        uint32_t need = 0;
        if (pr != 0xFFFFFFFFu) {
            if (tie[pr]) need = 1;
            else {
                uc_aln &am = alns[idx0[link[i]]];
                const uc_aln ar = alns[idx0[link[pr]]];
                am.aln_len = ar.aln_len; am.idents = ar.idents; am.gap_opens = ar.gap_opens;
                if (min_seq_id > 0.0f) {
                    const float sid = am.aln_len > 0 ? (float)am.idents / (float)am.aln_len : 0.0f;
                    const bool ok = sid >= min_seq_id;
                    am.accepted = ok;
                    eflag_out[i] = ok;
                }
            }
        }
        run2[i] = need;
    }
}

__global__ void __launch_bounds__(256) edge_scatter_kernel(uint32_t n2, const uint32_t *eflag, const uint32_t *epos, const uint32_t *sq2,
                                                           const uint32_t *st2, uint32_t *edges) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        if (!eflag[i]) continue;
        edges[2 * epos[i]] = sq2[i];
        edges[2 * epos[i] + 1] = st2[i];
    }
}

struct MaxU32 {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

}  // namespace

// ---- planner -----------------------------------------------------------------------------------------
struct SwPlan {
    uint32_t n = 0, ntasks = 0;
    DevBuf<uint64_t> key, key2;
    DevBuf<uint32_t> idx_in, idx, sq, st, head, segstart, flag, tpos, tcls, bounds;
    DevBuf<int32_t> sqe, ste, sqs, sts, saux;
    DevBuf<SwTask> tasks, tasks_in;
    DevBuf<uint64_t> tkey, tkey2;
    DevBuf<uint32_t> tidx, tidx2;
    DevBuf<unsigned long long> bytes;
    uint32_t task_base[NB] = {0}, pair_base[NB] = {0};
    uint64_t alg_bytes = 0, cells = 0;
    bool has_ends = false, has_starts = false, has_aux = false;
    int tab = 0;
    uint8_t *tbm = nullptr;                      // packed mode 7: traceback-byte matrices and per-pair offsets
    const unsigned long long *tboff = nullptr;
    int tb_band = 0;                             // ... and the half-width of the stored diagonal band (0 = the whole box)
    // the plan's device arrays back to the allocator (a plan that has run is dead weight: ~70 B per pair; the next build_plan reserves again)
    void release() {
        key.release(); key2.release(); idx_in.release(); idx.release(); sq.release(); st.release(); head.release(); segstart.release(); flag.release(); tpos.release();
        tcls.release(); bounds.release(); sqe.release(); ste.release(); sqs.release(); sts.release(); saux.release(); tasks.release(); tasks_in.release();
        tkey.release(); tkey2.release(); tidx.release(); tidx2.release(); bytes.release();
        n = ntasks = 0;
    }
};

// running maximum (inclusive) of a u32 array
static void max_scan_u32(Engine &E, DevBuf<char> &tmp, const uint32_t *in, uint32_t *out, uint32_t n) {
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, (size_t)n, MaxU32(), E.stream); });
}

// a 0/1 flag array -> its exclusive scan in pos (where each flagged entry goes) -> the number of flagged entries (one host synchronisation)
static uint32_t compact(Engine &E, DevBuf<char> &tmp, const uint32_t *flag, uint32_t *pos, uint32_t n) {
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), E.stream); });
    if (!n) return 0;
    uint32_t a = 0, b = 0;
    UC_HIP(hipMemcpyAsync(&a, pos + (n - 1), 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipMemcpyAsync(&b, flag + (n - 1), 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    return a + b;
}

// the packed classes form a prefix of a plan's sorted pair list, and their tasks a prefix of its task list
struct PackedPrefix { uint32_t pairs, tasks; };
static PackedPrefix packed_prefix(const SwPlan &P) {
    const ClassTable &tab = h_tab[P.tab];
    int c = 0;
    while (c < tab.n && tab.pk[c]) c++;
    return {P.pair_base[c], P.task_base[c]};
}

static void build_plan(Engine &E, SwPlan &P, DevBuf<char> &tmp, uint32_t n, const uint32_t *q, const uint32_t *t,
                       const int32_t *qe, const int32_t *te, int tab, const int32_t *qs = nullptr, const int32_t *ts = nullptr,
                       const int32_t *aux = nullptr /* one value per pair carried into plan order (known scores) */,
                       bool lpt = true /* false: tasks stay in pair order (the traceback plan is cut into byte-budgeted pair ranges) */) {
    {   // a __constant__ symbol exists once per DEVICE: upload the class tables to every device an engine plans on
        static std::mutex mu;
        static bool uploaded[64] = {};
        std::lock_guard<std::mutex> g(mu);
        if (E.device < 0 || E.device >= 64 || !uploaded[E.device]) {
            ClassTable t[4];
            memcpy(t, h_tab, sizeof t);
            UC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_tab), t, sizeof t));
            if (E.device >= 0 && E.device < 64) uploaded[E.device] = true;
        }
    }
    P.n = n; P.ntasks = 0; P.alg_bytes = 0; P.cells = 0; P.has_ends = qe != nullptr; P.has_starts = qs != nullptr; P.tab = tab;
    P.has_aux = aux != nullptr;
    memset(P.task_base, 0, sizeof P.task_base);
    memset(P.pair_base, 0, sizeof P.pair_base);
    if (!n) return;
    hipStream_t s = E.stream;
    P.key.reserve(n); P.key2.reserve(n); P.idx_in.reserve(n); P.idx.reserve(n);
    P.sq.reserve(n); P.st.reserve(n); P.head.reserve(n); P.segstart.reserve(n); P.flag.reserve(n); P.tpos.reserve(n);
    if (qe) { P.sqe.reserve(n); P.ste.reserve(n); }
    if (qs) { P.sqs.reserve(n); P.sts.reserve(n); }
    P.bytes.reserve(2); P.bounds.reserve(2 * NB);
    UC_HIP(hipMemsetAsync(P.bytes.p, 0, 16, s));
    hipLaunchKernelGGL(plan_key_kernel, grid_for(n, E.count_grid_cap), dim3(256), 0, s, n, q, t, qe, te, qs, ts, E.ddb.len, tab, P.key.p, P.idx_in.p, P.bytes.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, P.key.p, P.key2.p, P.idx_in.p, P.idx.p, (size_t)n, 0u, 45u, s); });
    hipLaunchKernelGGL(plan_gather_kernel, grid_for(n), dim3(256), 0, s, n, P.key2.p, P.idx.p, t, qe, te, qs, ts, P.sq.p, P.st.p, P.sqe.p, P.ste.p, P.sqs.p, P.sts.p, P.head.p);
    if (aux) {
        P.saux.reserve(n);
        hipLaunchKernelGGL(plan_aux_kernel, grid_for(n), dim3(256), 0, s, n, P.idx.p, aux, P.saux.p);
    }
    max_scan_u32(E, tmp, P.head.p, P.segstart.p, n);
    hipLaunchKernelGGL(plan_taskflag_kernel, grid_for(n), dim3(256), 0, s, n, P.key2.p, P.segstart.p, tab, P.flag.p);
    P.ntasks = compact(E, tmp, P.flag.p, P.tpos.p, n);
    P.tasks.reserve(P.ntasks); P.tcls.reserve(P.ntasks);
    hipLaunchKernelGGL(plan_taskfill_kernel, grid_for(n), dim3(256), 0, s, n, P.key2.p, P.flag.p, P.tpos.p, P.tasks.p, P.tcls.p);
    // longest-processing-time-first inside each class: the big tasks start first, the small ones fill the tail
    P.tasks_in.reserve(P.ntasks); P.tkey.reserve(P.ntasks); P.tkey2.reserve(P.ntasks); P.tidx.reserve(P.ntasks); P.tidx2.reserve(P.ntasks);
    hipLaunchKernelGGL(plan_taskcount_kernel, grid_for(P.ntasks), dim3(256), 0, s, P.ntasks, n, P.tasks.p, P.tcls.p, P.key2.p, P.tkey.p, P.tidx.p);
    if (lpt) {
        rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, P.tkey.p, P.tkey2.p, P.tidx.p, P.tidx2.p, (size_t)P.ntasks, 0u, 37u, s); });
        UC_HIP(hipMemcpyAsync(P.tasks_in.p, P.tasks.p, (size_t)P.ntasks * sizeof(SwTask), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(plan_taskgather_kernel, grid_for(P.ntasks), dim3(256), 0, s, P.ntasks, P.tidx2.p, P.tasks_in.p, P.tasks.p);
    }
    hipLaunchKernelGGL(plan_bounds_kernel, dim3(1), dim3(64), 0, s, P.ntasks, P.tcls.p, n, P.key2.p, P.bounds.p);
    uint32_t hb[2 * NB];
    unsigned long long bytes[2] = {0, 0};
    UC_HIP(hipMemcpyAsync(hb, P.bounds.p, sizeof hb, hipMemcpyDeviceToHost, s));
    UC_HIP(hipMemcpyAsync(bytes, P.bytes.p, 16, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipGetLastError());
    memcpy(P.task_base, hb, NB * 4);
    memcpy(P.pair_base, hb + NB, NB * 4);
    P.alg_bytes = bytes[0];
    P.cells = bytes[1];
}

// the second answer of a packed known-score pass (uc_sw_pk_impl.hpp key2): end under the order (first optimal row, then first column)
struct SwSecond { int32_t *qe, *te; };
__global__ void __launch_bounds__(256) fill2_kernel(uint32_t n, int32_t v, int32_t *a, int32_t *b) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { a[i] = v; b[i] = v; }
}

// one launch per populated class; outputs are in the plan's sorted order.  Returns the number of launches.
// [t0, t1): only the tasks of that range of the plan's task list (the byte-budgeted batches of the traceback plan); skip_long: not the long-query launch
// sec (MODE 4 / 6): where the packed known-score classes put their second answer, plan order; every other pair of the plan keeps -2 there
static uint64_t launch_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
                            const uint32_t *tb = nullptr, bool only_long = false, uint32_t t0 = 0, uint32_t t1 = 0xFFFFFFFFu, bool skip_long = false,
                            const SwSecond *sec = nullptr) {
    const ClassTable &tab = h_tab[P.tab];
    SwArgs a;
    if (sec) {
        if (mode != 4 && mode != 6) fail(UC_ERR_GENERIC, "second tie-break answer asked of a pass that has none");
        hipLaunchKernelGGL(fill2_kernel, grid_for(P.n), dim3(256), 0, E.stream, P.n, -2, sec->qe, sec->te);
        a.oqe2 = sec->qe; a.ote2 = sec->te;
    }
    a.db = E.ddb; a.tasks = P.tasks.p; a.pt = P.st.p; a.pqe = P.sqe.p; a.pte = P.ste.p;
    a.pqs = P.has_starts ? P.sqs.p : nullptr; a.pts = P.has_starts ? P.sts.p : nullptr;
    a.oscore = os; a.oqe = oqe; a.ote = ote; a.open = E.p.gap_open; a.ext = E.p.gap_ext;
    if (tb) { a.tb_diag = tb[0]; a.tb_ident = tb[1]; a.tb_open = tb[2]; a.tb_ext = tb[3]; }
    a.pscore = P.has_aux ? P.saux.p : nullptr;
    const int imode = mode >= 4 ? mode - 4 : mode;   // the int32 and long-query kernels have no known-score variant (they are exact anyway)
    if ((mode == 4 || mode == 6) && !P.has_aux) fail(UC_ERR_GENERIC, "known-score pass without scores");
    a.tbm = P.tbm; a.tboff = P.tboff; a.tb_band = P.tb_band;
    uint64_t launches = 0;
    const uint32_t gb = P.pair_base[tab.n], ngen = P.n - gb;
    uint32_t long_stride = 0;                        // queries beyond the largest systolic class: row-blocked kernel (uc_sw_long.hip)
    if (ngen) work.reserve(sw_long_work_ints(imode, ngen, E.max_len, &long_stride));
    // fork: the classes run concurrently on the auxiliary streams, largest classes first on distinct streams
    UC_HIP(hipEventRecord(E.ev_fork, E.stream));
    for (int i = 0; i < E.n_streams - 1; i++) UC_HIP(hipStreamWaitEvent(E.aux[i], E.ev_fork, 0));
    int slot = 0;
    if (ngen && !skip_long) {                        // the longest-running launch goes first
        SwArgs al = a;
        al.tasks = P.tasks.p + P.task_base[tab.n];
        launch_sw_long(imode, al, P.task_base[tab.n + 1] - P.task_base[tab.n], gb, work.p, long_stride, E.stream);
        UC_HIP(hipGetLastError());
        slot++;
        launches++;
    }
    for (int c = tab.n - 1; c >= 0 && !only_long; c--) {
        const uint32_t c0 = std::max(P.task_base[c], t0), c1 = std::min(P.task_base[c + 1], t1);
        if (c0 >= c1) continue;
        const uint32_t nt = c1 - c0;
        SwArgs ac = a;
        ac.tasks = P.tasks.p + c0;
        hipStream_t st = slot % E.n_streams == 0 ? E.stream : E.aux[slot % E.n_streams - 1];
        slot++;
        if (tab.pk[c]) launch_sw_pk_class(tab.G[c], tab.R[c], mode, ac, nt, st);
        else launch_sw_class(tab.G[c], tab.R[c], imode, ac, nt, st);
        UC_HIP(hipGetLastError());
        launches++;
    }
    for (int i = 0; i < E.n_streams - 1; i++) {   // join
        UC_HIP(hipEventRecord(E.ev_join[i], E.aux[i]));
        UC_HIP(hipStreamWaitEvent(E.stream, E.ev_join[i], 0));
    }
    return launches;
}

// pairs of the packed classes whose result is not final: ambiguous end row (qe == -2) or a value near the
// u16 range -> they are re-run by the int32 kernel
__global__ void __launch_bounds__(256) pk_flag_kernel(uint32_t n_pk, const int32_t *os, const int32_t *oqe, int ovf, int ovf_only, uint32_t *flag) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_pk; i += gridDim.x * 256)
        flag[i] = (os[i] >= ovf || (!ovf_only && oqe && oqe[i] == -2)) ? 1u : 0u;
}
// deferred variant: only the pairs that passed the E-value gate need their exact end row
__global__ void __launch_bounds__(256) amb_flag_kernel(uint32_t n2, const int32_t *qe2, uint32_t *flag) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) flag[i] = qe2[i] == -2 ? 1u : 0u;
}
// Both tie-break answers from one DP: a flagged mirror (mirror[link[i]]) whose representative sits right before it in the gate-passer list and
// is flagged too does not run - the representative's known-score re-run reports the mirror's end as its second answer (dual[i - 1] = 1).  A flagged
// representative got its -2 from a packed class of the forward pass, with a score below the packed range: every table of the known-score
// pass holds it in a packed class again (pk_cap: their common row limit), and its re-run cannot overflow.
__global__ void __launch_bounds__(256) amb_dual_kernel(uint32_t n2, const int32_t *qe2, const uint32_t *q2, const uint32_t *link, const uint32_t *mirror,
                                                       const uint32_t *len, uint32_t pk_cap, uint32_t *flag, uint32_t *dual) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const bool f = qe2[i] == -2;
        const uint32_t j = link[i];
        const bool shared = f && i > 0 && mirror[j] && !mirror[j - 1] && link[i - 1] == j - 1 && qe2[i - 1] == -2 && len[q2[i - 1]] <= pk_cap;
        flag[i] = (f && !shared) ? 1u : 0u;
        const bool serves = qe2[i] == -2 && !mirror[j] && i + 1 < n2 && link[i + 1] == j + 1 && mirror[j + 1] && qe2[i + 1] == -2 && len[q2[i]] <= pk_cap;
        dual[i] = serves ? 1u : 0u;
    }
}
__global__ void __launch_bounds__(256) amb_gather_kernel(uint32_t n2, const uint32_t *flag, const uint32_t *pos, const uint32_t *q2,
                                                         const uint32_t *t2, const uint32_t *link, const int32_t *s0, uint32_t *q3,
                                                         uint32_t *t3, uint32_t *link3, int32_t *s3) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        q3[w] = q2[i]; t3[w] = t2[i]; link3[w] = i; s3[w] = s0[link[i]];
    }
}
// dual (optional): entry j + 1 of the gate-passer list is the mirror that entry j's run serves - its end is the second answer, roles swapped
__global__ void __launch_bounds__(256) amb_putback_kernel(uint32_t n3, const uint32_t *idx3, const uint32_t *link3, const uint32_t *link,
                                                          const int32_t *qe3, const int32_t *te3, int32_t *qe2, int32_t *te2,
                                                          int32_t *qe0, int32_t *te0, const uint32_t *dual, const int32_t *qe3b,
                                                          const int32_t *te3b, uint32_t *err) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n3; i += gridDim.x * 256) {
        const uint32_t j = link3[idx3[i]];
        qe2[j] = qe3[i]; te2[j] = te3[i];
        qe0[link[j]] = qe3[i]; te0[link[j]] = te3[i];
        if (dual && dual[j]) {
            const int32_t mq = te3b[i], mt = qe3b[i];
            if (mq < 0 || mt < 0) atomicAdd(err, 1u);   // cannot happen (amb_dual_kernel); checked by the host at the stage's next synchronisation
            qe2[j + 1] = mq; te2[j + 1] = mt;
            qe0[link[j + 1]] = mq; te0[link[j + 1]] = mt;
        }
    }
}
__global__ void __launch_bounds__(256) pk_gather_kernel(uint32_t n_pk, const uint32_t *flag, const uint32_t *pos, const uint32_t *sq,
                                                        const uint32_t *st, const int32_t *sqe, const int32_t *ste, uint32_t *q2,
                                                        uint32_t *t2, int32_t *qe2, int32_t *te2, uint32_t *link) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n_pk; i += gridDim.x * 256) {
        if (!flag[i]) continue;
        const uint32_t w = pos[i];
        q2[w] = sq[i]; t2[w] = st[i]; link[w] = i;
        if (sqe) { qe2[w] = sqe[i]; te2[w] = ste[i]; }
    }
}
__global__ void __launch_bounds__(256) pk_putback_kernel(uint32_t n2, const uint32_t *idx2, const uint32_t *link, const int32_t *s,
                                                         const int32_t *qe, const int32_t *te, int32_t *os, int32_t *oqe, int32_t *ote,
                                                         int32_t *oqe2, int32_t *ote2) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        const uint32_t o = link[idx2[i]];
        os[o] = s[i];
        if (oqe) { oqe[o] = qe[i]; ote[o] = te[i]; }
        if (oqe2) { oqe2[o] = -2; ote2[o] = -2; }   // the int32 kernel reports one tie-break order only
    }
}


struct RerunBufs {
    DevBuf<uint32_t> flag, pos, q2, t2, link, dual, err;
    DevBuf<int32_t> qe2, te2, s, qe, te, sin, qeb, teb;
};

// Work buffers of the gapped stage and of the set-cover graph build.  ONE set per engine (parked per device between
// engines): nothing in this file is process-wide, so engines on different devices - or several engines on one device,
// each driven by its own host thread as uc_cluster does for num_gpus > 1 - never share or race on a buffer.
struct AlignScratch {
    DevBuf<int32_t> d_ms, s0, qe0, te0, s1, s1c, qe2, te2, s2, q2o, t2o, work;
    DevBuf<uint32_t> gflag, gpos, q1, t1, link1, q2, t2, link, eflag, epos, mism, d_e;
    DevBuf<uint64_t> ukey, ukey2;
    DevBuf<uint32_t> uidx_in, uidx, fq, ft, mirror, rep, rpos, qr, tr, jrep, rcopy;
    DevBuf<int32_t> su, qeu, teu, s2s, q2os, t2os, qe2a, te2a, sknown, q2os2, t2os2, q2o2, t2o2;
    DevBuf<uint32_t> iota2, smkeep, smpos, partner, uniq, q2a, t2a, mapa;
    DevBuf<uint32_t> lg_q, lg_t, lg_map, lg_flag, lg_pos;   // rule UC-1/L: the compacted pair list of a batch and its records
    DevBuf<uc_aln> lg_alns;
    DevBuf<unsigned long long> d_cells;
    DevBuf<char> tmp;
    SwPlan P0, P1, P2, P2b;
    // packed-range / ambiguous-end re-runs (run_plan, fix_ambiguous_ends)
    RerunBufs rr_B, amb_B;
    SwPlan rr_P2, amb_P3;
    // traceback statistics (align: --min-seq-id / search)
    DevBuf<uint32_t> tb_q3, tb_t3, tb_src3, tb_trun, tb_tpos, tb_tpart, tb_ttie, tb_tlo, tb_thi, tb_tmiss, tb_tchunk, tb_tcpos;
    DevBuf<unsigned long long> tb_tbsize, tb_tboff, tb_toff;
    DevBuf<uint8_t> tb_tbm;
    bool tb_tbm_live = false;        // inside the batch loop of a MODE 7 call: the one time the matrices may not be given back (release_tb_matrices)
    DevBuf<int32_t> tb_qs3, tb_qe3, tb_ts3, tb_te3, tb_pack3, tb_id3, tb_gaps3, tb_sc3;
    SwPlan tb_P3;
    // backtraces (-a): runs per pair of the traceback plan, slice offsets inside a matrix batch, where each slice went, which kernel walked it
    DevBuf<uint32_t> bt_cnt3, bt_off3, bt_plain3, bt_err, lg_btn;
    DevBuf<unsigned long long> bt_pos3, lg_btpos;
    // set-cover graph build + greedy cover (set_cover_graph)
    DevBuf<uint32_t> sc_e, sc_flag, sc_pos, sc_dadj, sc_bad, sc_assign, sc_cnt, sc_work, sc_work2, sc_picks, sc_newly, sc_ctr;
    DevBuf<uint64_t> sc_m1;
    DevBuf<uint64_t> sc_key, sc_key2, sc_ukey, sc_doff;
    DevBuf<char> sc_tmp;
    GreedyIncScratch gi;             // --cluster-mode 2 (uc_greedy_inc.hip): same graph buffers, its own round state
    ReassignScratch ra;              // --cluster-reassign (uc_reassign.hip): member keys, flags, seeds, the stage's edge list
};
static AlignScratch &scratch_of(Engine &E) {
    if (!E.aln) E.aln = ParkedScratch<AlignScratch>::take_or_new(E.device);
    return *E.aln;
}

// ovf_only: re-run immediately only what saturated; ambiguous end rows (qe == -2) are left for the caller
static void run_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
                     DevBuf<char> &tmp, bool ovf_only = false, const SwSecond *sec = nullptr) {
    if (!P.n) return;
    E.timed_ms_begin();
    uint64_t launches = launch_plan(E, P, mode, os, oqe, ote, work, nullptr, false, 0, 0xFFFFFFFFu, false, sec);
    double ms = E.timed_ms_end();
    const uint32_t n_pk = packed_prefix(P).pairs;
    if (n_pk) {
        RerunBufs &B = scratch_of(E).rr_B;
        SwPlan &P2 = scratch_of(E).rr_P2;
        hipStream_t s = E.stream;
        B.flag.reserve(n_pk); B.pos.reserve(n_pk);
        hipLaunchKernelGGL(pk_flag_kernel, grid_for(n_pk), dim3(256), 0, s, n_pk, os, oqe, SW_PK_OVF_HOST, ovf_only ? 1 : 0, B.flag.p);
        const uint32_t n2 = compact(E, tmp, B.flag.p, B.pos.p, n_pk);
        E.stats.n_pk_reruns += n2;
        if (n2) {
            B.q2.reserve(n2); B.t2.reserve(n2); B.link.reserve(n2); B.s.reserve(n2);
            if (P.has_ends) { B.qe2.reserve(n2); B.te2.reserve(n2); }
            if (oqe) { B.qe.reserve(n2); B.te.reserve(n2); }
            hipLaunchKernelGGL(pk_gather_kernel, grid_for(n_pk), dim3(256), 0, s, n_pk, B.flag.p, B.pos.p, P.sq.p, P.st.p,
                               P.has_ends ? P.sqe.p : nullptr, P.has_ends ? P.ste.p : nullptr, B.q2.p, B.t2.p, B.qe2.p, B.te2.p, B.link.p);
            build_plan(E, P2, tmp, n2, B.q2.p, B.t2.p, P.has_ends ? B.qe2.p : nullptr, P.has_ends ? B.te2.p : nullptr, 0);
            E.timed_ms_begin();
            launches += launch_plan(E, P2, mode >= 4 ? mode - 4 : mode, B.s.p, oqe ? B.qe.p : nullptr, oqe ? B.te.p : nullptr, work);
            ms += E.timed_ms_end();
            E.stats.cells_run += P2.cells;
            E.stats.n_sw_runs += P2.n;
            hipLaunchKernelGGL(pk_putback_kernel, grid_for(n2), dim3(256), 0, s, n2, P2.idx.p, B.link.p, B.s.p,
                               oqe ? B.qe.p : nullptr, oqe ? B.te.p : nullptr, os, oqe, ote, sec ? sec->qe : nullptr, sec ? sec->te : nullptr);
            UC_HIP(hipGetLastError());
        }
    }
    E.stats.sw_kernel_ms += ms;
    E.stats.sw_kernel_launches += launches;
    E.stats.sw_algorithmic_bytes += P.alg_bytes;
    E.stats.cells_run += P.cells;
    E.stats.n_sw_runs += P.n;
    if (getenv("UC_TIMING")) fprintf(stderr, "unicore-cluster[timing]: sw pass mode %d: %u pairs, %llu cells, %.2f ms (%llu launches)\n", mode, P.n, (unsigned long long)P.cells, ms, (unsigned long long)launches);
}

// exact (qEnd, tEnd) for the gate-passing pairs whose end is still unknown (ambiguous end row of the packed kernel, or a
// mirror that could not take its representative's end): a second forward pass that KNOWS the optimum score (packed
// MODE 4; int32 kernel for --sw-kernel i32 and for queries beyond the systolic classes)
// mirror (null: no mutual-hit sharing in this batch): with the packed kernel, the run of a flagged representative also serves its flagged mirror
// (amb_dual_kernel) - one DP, both tie-break answers
static void fix_ambiguous_ends(Engine &E, uint32_t n2, const uint32_t *q2, const uint32_t *t2, int32_t *qe2, int32_t *te2,
                               const uint32_t *link, const int32_t *s0, int32_t *qe0, int32_t *te0, DevBuf<int32_t> &work,
                               DevBuf<char> &tmp, uint32_t n_queries, const uint32_t *mirror) {
    RerunBufs &B = scratch_of(E).amb_B;
    SwPlan &P3 = scratch_of(E).amb_P3;
    hipStream_t s = E.stream;
    const bool pk = E.p.sw_pk != 0;
    const bool dual = pk && mirror && dual_tiebreak_on();
    B.flag.reserve(n2); B.pos.reserve(n2);
    if (dual) {
        B.dual.reserve(n2);
        if (!B.err.p) { B.err.reserve(1); UC_HIP(hipMemsetAsync(B.err.p, 0, 4, s)); }
        hipLaunchKernelGGL(amb_dual_kernel, grid_for(n2), dim3(256), 0, s, n2, qe2, q2, link, mirror, E.ddb.len,
                           (uint32_t)std::min(h_tab[1].cap[h_tab[1].n - 1], h_tab[3].cap[h_tab[3].n - 1]), B.flag.p, B.dual.p);
    } else {
        hipLaunchKernelGGL(amb_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, qe2, B.flag.p);
    }
    const uint32_t n3 = compact(E, tmp, B.flag.p, B.pos.p, n2);
    E.stats.n_pk_reruns += n3;
    if (!n3) return;
    B.q2.reserve(n3); B.t2.reserve(n3); B.link.reserve(n3); B.s.reserve(n3); B.qe.reserve(n3); B.te.reserve(n3); B.sin.reserve(n3);
    if (dual) { B.qeb.reserve(n3); B.teb.reserve(n3); }
    hipLaunchKernelGGL(amb_gather_kernel, grid_for(n2), dim3(256), 0, s, n2, B.flag.p, B.pos.p, q2, t2, link, s0, B.q2.p, B.t2.p, B.link.p, B.sin.p);
    build_plan(E, P3, tmp, n3, B.q2.p, B.t2.p, nullptr, nullptr, pk ? pk_known_tab(n3, n_queries) : 0, nullptr, nullptr, pk ? B.sin.p : nullptr);
    const SwSecond sec{B.qeb.p, B.teb.p};
    run_plan(E, P3, pk ? 4 : 0, B.s.p, B.qe.p, B.te.p, work, tmp, false, dual ? &sec : nullptr);
    hipLaunchKernelGGL(amb_putback_kernel, grid_for(n3), dim3(256), 0, s, n3, P3.idx.p, B.link.p, link, B.qe.p, B.te.p, qe2, te2, qe0, te0,
                       dual ? B.dual.p : nullptr, B.qeb.p, B.teb.p, B.err.p);
    UC_HIP(hipGetLastError());
}

void free_scratch(AlignScratch *p) { delete p; }

// memory pressure inside the gapped stage: the traceback-byte buffer (up to 144 GiB, kept between calls because fresh memory is slow) is dead weight
// outside the batch loop of a MODE 7 call - the engine's out-of-memory handler gives it back before it gives up
bool release_tb_matrices(AlignScratch *p) {
    if (!p || p->tb_tbm_live || !p->tb_tbm.cap) return false;
    p->tb_tbm.release();
    return true;
}

// ---- kernel-level entry point: arbitrary pair list from the host -----------------------------------
void Engine::sw_batch(int mode, const std::vector<PairIn> &pairs, int32_t *score, int32_t *qe, int32_t *te) {
    PressureScope ps(*this, 1);
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    const size_t n = pairs.size();
    if (n == 0) return;
    if (n >= (1ull << 31)) fail(UC_ERR_ARGS, "sw_batch: too many pairs");
    UC_HIP(hipSetDevice(device));
    const bool track = mode != 1;
    std::vector<uint32_t> hq(n), ht(n);
    std::vector<int32_t> hqe, hte;
    if (mode == 2) { hqe.resize(n); hte.resize(n); }
    for (size_t i = 0; i < n; i++) {
        const PairIn &x = pairs[i];
        if (x.q >= hdb.n || x.t >= hdb.n) fail(UC_ERR_ARGS, "sw_batch: sequence id out of range");
        if (mode == 2 && (x.qe < 0 || x.te < 0 || (uint32_t)x.qe >= h_len[x.q] || (uint32_t)x.te >= h_len[x.t]))
            fail(UC_ERR_ARGS, "sw_batch: end position out of range");
        hq[i] = x.q; ht[i] = x.t;
        if (mode == 2) { hqe[i] = x.qe; hte[i] = x.te; }
    }
    DevBuf<uint32_t> dq, dt;
    DevBuf<int32_t> dqe, dte, os, oq, ot, rs, rq, rt, work;
    DevBuf<char> tmp;
    dq.reserve(n); dt.reserve(n); os.reserve(n); rs.reserve(n);
    UC_HIP(hipMemcpyAsync(dq.p, hq.data(), n * 4, hipMemcpyHostToDevice, stream));
    UC_HIP(hipMemcpyAsync(dt.p, ht.data(), n * 4, hipMemcpyHostToDevice, stream));
    if (mode == 2) {
        dqe.reserve(n); dte.reserve(n);
        UC_HIP(hipMemcpyAsync(dqe.p, hqe.data(), n * 4, hipMemcpyHostToDevice, stream));
        UC_HIP(hipMemcpyAsync(dte.p, hte.data(), n * 4, hipMemcpyHostToDevice, stream));
    }
    if (track) { oq.reserve(n); ot.reserve(n); rq.reserve(n); rt.reserve(n); }
    SwPlan P;
    build_plan(*this, P, tmp, (uint32_t)n, dq.p, dt.p, dqe.p, dte.p, p.sw_pk ? 1 : 0);
    run_plan(*this, P, mode, os.p, oq.p, ot.p, work, tmp);
    hipLaunchKernelGGL(scatter3_kernel, grid_for(n), dim3(256), 0, stream, (uint32_t)n, P.idx.p, os.p, oq.p, ot.p, rs.p, rq.p, rt.p);
    UC_HIP(hipMemcpyAsync(score, rs.p, n * 4, hipMemcpyDeviceToHost, stream));
    if (track && qe) UC_HIP(hipMemcpyAsync(qe, rq.p, n * 4, hipMemcpyDeviceToHost, stream));
    if (track && te) UC_HIP(hipMemcpyAsync(te, rt.p, n * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
}

// ---- stage E5 + E6 for queries [qbegin, qend) of the device-resident hit lists ----------------------
// one device batch of Engine::align: the queries [qa, qb) and the pair list its passes work on
struct AlignBatch {
    uint32_t qbegin, qa, qb;          // qbegin: first query of the call (d_ms is indexed from it)
    uint32_t n;                       // pairs of the batch (after the length gate)
    const uint32_t *dq, *dt;
    uc_aln *alns_b;                   // where record i of the batch's pair list goes
    uc_aln *alns_list;                // the batch's records in the hit lists (== alns_b unless the length gate compacted the list)
    bool dedup;
    int tab;
    // the directed pair list the gates work on: sorted (query, target) + position in the hit list
    const uint32_t *Lsq = nullptr, *Lst = nullptr, *Lidx = nullptr;
    uint32_t n2 = 0;                  // pairs that passed the E-value gate
    // backtraces (-a): slice position and run count per record, indexed like alns_b (null: not emitted)
    unsigned long long *bt_pos_b = nullptr;
    uint32_t *bt_n_b = nullptr;
};

// rule UC-1/L (optional): the stage works on the pairs the length gate lets through - a compacted copy of the batch's pair list with its own
// record array; the records return to their places in the hit-list order at the end of the batch, the gated pairs keep all-zero records
static void length_gate(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.lg_flag.reserve(n); A.lg_pos.reserve(n);
    hipLaunchKernelGGL(len_gate_kernel, grid_for(n), dim3(256), 0, s, n, B.dq, B.dt, E.ddb.len, E.p.cov, E.p.cov_mode, A.lg_flag.p);
    const uint32_t nc = compact(E, A.tmp, A.lg_flag.p, A.lg_pos.p, n);
    A.lg_q.reserve(std::max<uint32_t>(nc, 1)); A.lg_t.reserve(std::max<uint32_t>(nc, 1)); A.lg_map.reserve(std::max<uint32_t>(nc, 1));
    A.lg_alns.reserve(std::max<uint32_t>(nc, 1));
    hipLaunchKernelGGL(len_gate_gather_kernel, grid_for(n), dim3(256), 0, s, n, A.lg_flag.p, A.lg_pos.p, B.dq, B.dt, A.lg_q.p, A.lg_t.p, A.lg_map.p);
    if (nc) UC_HIP(hipMemsetAsync(A.lg_alns.p, 0, (size_t)nc * sizeof(uc_aln), s));
    UC_HIP(hipMemsetAsync(B.alns_list, 0, (size_t)n * sizeof(uc_aln), s));
    if (B.bt_pos_b) {
        A.lg_btpos.reserve(std::max<uint32_t>(nc, 1)); A.lg_btn.reserve(std::max<uint32_t>(nc, 1));
        UC_HIP(hipMemsetAsync(A.lg_btn.p, 0, (size_t)std::max<uint32_t>(nc, 1) * 4, s));
        UC_HIP(hipMemsetAsync(B.bt_n_b, 0, (size_t)n * 4, s));
        B.bt_pos_b = A.lg_btpos.p; B.bt_n_b = A.lg_btn.p;
    }
    B.dq = A.lg_q.p; B.dt = A.lg_t.p; B.alns_b = A.lg_alns.p; B.n = nc;
}

// forward pass: s0 / qe0 / te0 of every pair, and the directed pair list (Lsq, Lst, Lidx)
static void forward_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.s0.reserve(n); A.qe0.reserve(n); A.te0.reserve(n); A.gflag.reserve(n); A.gpos.reserve(n);
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 16, s));
    if (!B.dedup) {
        build_plan(E, A.P0, A.tmp, n, B.dq, B.dt, nullptr, nullptr, B.tab);
        run_plan(E, A.P0, 0, A.s0.p, A.qe0.p, A.te0.p, A.work, A.tmp, /*ovf_only=*/true);
        E.stats.cells_fwd += A.P0.cells;
        B.Lsq = A.P0.sq.p; B.Lst = A.P0.st.p; B.Lidx = A.P0.idx.p;
        return;
    }
    // mutual hits share one forward DP, computed in the orientation with the shorter query
    A.ukey.reserve(n); A.ukey2.reserve(n); A.uidx_in.reserve(n); A.uidx.reserve(n);
    A.fq.reserve(n); A.ft.reserve(n); A.mirror.reserve(n); A.rep.reserve(n); A.rpos.reserve(n);
    hipLaunchKernelGGL(ukey_kernel, grid_for(n), dim3(256), 0, s, n, B.dq, B.dt, E.ddb.len, A.ukey.p, A.uidx_in.p);
    rocprim_call(A.tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, A.ukey.p, A.ukey2.p, A.uidx_in.p, A.uidx.p, (size_t)n, 0u, 49u, s); });
    hipLaunchKernelGGL(umark_kernel, grid_for(n), dim3(256), 0, s, n, A.ukey2.p, A.uidx.p, B.dq, B.dt, A.fq.p, A.ft.p, A.mirror.p, A.rep.p);
    const uint32_t nu = compact(E, A.tmp, A.rep.p, A.rpos.p, n);
    A.qr.reserve(nu); A.tr.reserve(nu); A.jrep.reserve(nu); A.su.reserve(nu); A.qeu.reserve(nu); A.teu.reserve(nu);
    hipLaunchKernelGGL(ugather_kernel, grid_for(n), dim3(256), 0, s, n, A.rep.p, A.rpos.p, A.fq.p, A.ft.p, A.qr.p, A.tr.p, A.jrep.p);
    build_plan(E, A.P0, A.tmp, nu, A.qr.p, A.tr.p, nullptr, nullptr, B.tab);
    run_plan(E, A.P0, 0, A.su.p, A.qeu.p, A.teu.p, A.work, A.tmp, /*ovf_only=*/true);
    hipLaunchKernelGGL(uscatter_kernel, grid_for(nu), dim3(256), 0, s, nu, n, A.P0.idx.p, A.jrep.p, A.mirror.p, A.su.p, A.qeu.p, A.teu.p,
                       packed_prefix(A.P0).pairs, SW_PK_OVF_HOST, A.s0.p, A.qe0.p, A.te0.p);
    hipLaunchKernelGGL(cells_kernel, grid_for(n, E.count_grid_cap), dim3(256), 0, s, n, A.fq.p, A.ft.p, (const uint32_t *)nullptr, E.ddb.len, A.d_cells.p);
    B.Lsq = A.fq.p; B.Lst = A.ft.p; B.Lidx = A.uidx.p;
}

// spec UC-1.1: the reversed-query pass only runs for pairs whose forward score reaches the E-value
// threshold (corrected <= score, so the others cannot pass); their score_rev is reported as 0
static void rev_correction_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.s1.reserve(n);
    UC_HIP(hipMemsetAsync(A.s1.p, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(gate_kernel, grid_for(n), dim3(256), 0, s, n, B.Lsq, A.s0.p, (const int32_t *)nullptr, A.d_ms.p, B.qbegin, A.gflag.p);
    if (B.dedup) {
        A.rcopy.reserve(n);
        hipLaunchKernelGGL(cells_kernel, grid_for(n, E.count_grid_cap), dim3(256), 0, s, n, B.Lsq, B.Lst, A.gflag.p, E.ddb.len, A.d_cells.p + 1);
        hipLaunchKernelGGL(rev_dedup_kernel, grid_for(n), dim3(256), 0, s, n, A.mirror.p, A.gflag.p, A.rcopy.p);
        hipLaunchKernelGGL(rev_unflag_kernel, grid_for(n), dim3(256), 0, s, n, A.rcopy.p, A.gflag.p);
    }
    const uint32_t n1 = compact(E, A.tmp, A.gflag.p, A.gpos.p, n);
    if (n1) {
        A.q1.reserve(n1); A.t1.reserve(n1); A.link1.reserve(n1); A.s1c.reserve(n1);
        hipLaunchKernelGGL(pair_gather_kernel, grid_for(n), dim3(256), 0, s, n, A.gflag.p, A.gpos.p, B.Lsq, B.Lst, A.q1.p, A.t1.p, A.link1.p);
        build_plan(E, A.P1, A.tmp, n1, A.q1.p, A.t1.p, nullptr, nullptr, B.tab);
        run_plan(E, A.P1, 1, A.s1c.p, nullptr, nullptr, A.work, A.tmp);
        hipLaunchKernelGGL(rev_putback_kernel, grid_for(n1), dim3(256), 0, s, n1, A.P1.idx.p, A.link1.p, A.s1c.p, A.s1.p);
        if (!B.dedup) E.stats.cells_rev += A.P1.cells;
    }
    if (B.dedup) hipLaunchKernelGGL(rev_copy_kernel, grid_for(n), dim3(256), 0, s, n, A.rcopy.p, A.s1.p);
}

// E-value gate on the corrected score: the gate passers (q2, t2, qe2, te2, link) with their exact end rows, and the records of every pair
static void evalue_gate(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    const int32_t *s1p = E.p.rev_correction ? A.s1.p : nullptr;
    hipLaunchKernelGGL(gate_kernel, grid_for(n), dim3(256), 0, s, n, B.Lsq, A.s0.p, s1p, A.d_ms.p, B.qbegin, A.gflag.p);
    const uint32_t n2 = B.n2 = compact(E, A.tmp, A.gflag.p, A.gpos.p, n);
    if (n2) {
        A.q2.reserve(n2); A.t2.reserve(n2); A.qe2.reserve(n2); A.te2.reserve(n2); A.link.reserve(n2);
        A.s2.reserve(n2); A.q2o.reserve(n2); A.t2o.reserve(n2); A.eflag.reserve(n2); A.epos.reserve(n2);
        hipLaunchKernelGGL(gate_scatter_kernel, grid_for(n), dim3(256), 0, s, n, A.gflag.p, A.gpos.p, B.Lsq, B.Lst, A.qe0.p, A.te0.p,
                           A.q2.p, A.t2.p, A.qe2.p, A.te2.p, A.link.p);
        if (E.p.sw_pk || B.dedup)
            fix_ambiguous_ends(E, n2, A.q2.p, A.t2.p, A.qe2.p, A.te2.p, A.link.p, A.s0.p, A.qe0.p, A.te0.p, A.work, A.tmp, B.qb - B.qa,
                               B.dedup ? A.mirror.p : nullptr);
    }
    hipLaunchKernelGGL(aln_basic_kernel, grid_for(n), dim3(256), 0, s, n, B.Lidx, A.s0.p, s1p, A.qe0.p, A.te0.p, A.gflag.p, B.alns_b);
}

// one known-score start pass (packed MODE 6; the optimum of the start pass is the forward score) over the m gate passers flagged in smkeep
// dual: round 1 - the second answer of every pair goes to q2o2 / t2o2 for the mirrors that share the DP
static void known_start_round(Engine &E, const AlignBatch &B, SwPlan &P, uint32_t m, int tab, uint32_t *uniq, bool dual) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    A.q2a.reserve(m); A.t2a.reserve(m); A.qe2a.reserve(m); A.te2a.reserve(m); A.mapa.reserve(m);
    hipLaunchKernelGGL(sm_gather_kernel, grid_for(B.n2), dim3(256), 0, s, B.n2, A.smkeep.p, A.smpos.p, A.q2.p, A.t2.p, A.qe2.p, A.te2.p,
                       A.q2a.p, A.t2a.p, A.qe2a.p, A.te2a.p, A.mapa.p);
    A.sknown.reserve(m);
    hipLaunchKernelGGL(sm_score_kernel, grid_for(m), dim3(256), 0, s, m, A.mapa.p, A.link.p, A.s0.p, A.sknown.p);
    build_plan(E, P, A.tmp, m, A.q2a.p, A.t2a.p, A.qe2a.p, A.te2a.p, tab, nullptr, nullptr, A.sknown.p);
    if (dual) { A.q2os2.reserve(m); A.t2os2.reserve(m); }
    const SwSecond sec{A.q2os2.p, A.t2os2.p};
    run_plan(E, P, 6, A.s2s.p, A.q2os.p, A.t2os.p, A.work, A.tmp, false, dual ? &sec : nullptr);
    hipLaunchKernelGGL(sm_scatter_kernel, grid_for(m), dim3(256), 0, s, m, P.idx.p, A.mapa.p, A.s2s.p, A.q2os.p, A.t2os.p,
                       A.s2.p, A.q2o.p, A.t2o.p, uniq, dual ? A.q2os2.p : nullptr, dual ? A.t2os2.p : nullptr,
                       dual ? A.q2o2.p : nullptr, dual ? A.t2o2.p : nullptr);
}

// start pass of the shared-DP path on the packed kernel
static void start_pass_known(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    A.smkeep.reserve(n2); A.smpos.reserve(n2); A.partner.reserve(n2); A.uniq.reserve(n2);
    UC_HIP(hipMemsetAsync(A.uniq.p, 0, (size_t)n2 * 4, s));
    hipLaunchKernelGGL(sm_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.link.p, A.mirror.p, A.gflag.p, A.gpos.p, A.qe2.p, A.te2.p,
                       A.qe0.p, A.te0.p, A.smkeep.p, A.partner.p);
    // round 1: exact in one pass; it reports both tie-break answers, and whether a single row holds every optimal cell
    const bool dual = dual_tiebreak_on();
    if (dual) { A.q2o2.reserve(n2); A.t2o2.reserve(n2); }
    known_start_round(E, B, A.P2, compact(E, A.tmp, A.smkeep.p, A.smpos.p, n2), B.tab, A.uniq.p, dual);
    hipLaunchKernelGGL(sm_resolve_kernel, grid_for(n2), dim3(256), 0, s, n2, A.partner.p, A.uniq.p, A.s2.p, A.q2o.p, A.t2o.p,
                       dual ? A.q2o2.p : nullptr, dual ? A.t2o2.p : nullptr);
    // round 2: the mirrors that could not take their partner's result - with both answers at hand only those whose partner's result came from
    // another kernel than the packed known-score one (int32 re-runs, queries beyond the systolic classes)
    hipLaunchKernelGGL(amb_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.q2o.p, A.smkeep.p);
    const uint32_t n2b = compact(E, A.tmp, A.smkeep.p, A.smpos.p, n2);
    if (!n2b) return;
    known_start_round(E, B, A.P2b, n2b, pk_known_tab(n2b, B.qb - B.qa), nullptr, false);
    E.stats.n_pk_reruns += n2b;
}

// start pass; results end up in the natural order of the gate-passer list (iota2 stands for the plan order).  Then the records of the gate
// passers, the coverage gate and the edge flags (eflag)
static void start_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    A.iota2.reserve(n2); A.s2s.reserve(n2); A.q2os.reserve(n2); A.t2os.reserve(n2);
    hipLaunchKernelGGL(iota_kernel, grid_for(n2), dim3(256), 0, s, n2, A.iota2.p);
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 8, s));
    hipLaunchKernelGGL(cells_box_kernel, grid_for(n2, E.count_grid_cap), dim3(256), 0, s, n2, A.qe2.p, A.te2.p, A.d_cells.p);
    if (B.dedup && B.tab == 1) {
        start_pass_known(E, B);
    } else {
        build_plan(E, A.P2, A.tmp, n2, A.q2.p, A.t2.p, A.qe2.p, A.te2.p, B.tab);
        run_plan(E, A.P2, 2, A.s2s.p, A.q2os.p, A.t2os.p, A.work, A.tmp);
        hipLaunchKernelGGL(sm_scatter_kernel, grid_for(n2), dim3(256), 0, s, n2, A.P2.idx.p, (const uint32_t *)nullptr, A.s2s.p, A.q2os.p,
                           A.t2os.p, A.s2.p, A.q2o.p, A.t2o.p, (uint32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr,
                           (int32_t *)nullptr, (int32_t *)nullptr);
    }
    unsigned long long hc = 0;
    uint32_t dual_err = 0;
    UC_HIP(hipMemcpyAsync(&hc, A.d_cells.p, 8, hipMemcpyDeviceToHost, s));
    if (A.amb_B.err.p) UC_HIP(hipMemcpyAsync(&dual_err, A.amb_B.err.p, 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    if (dual_err) fail(UC_ERR_GENERIC, "gapped stage: %u shared end re-runs came back without a second answer", dual_err);
    E.stats.cells_start += hc;
    hipLaunchKernelGGL(finalize_kernel, grid_for(n2), dim3(256), 0, s, n2, A.iota2.p, A.link.p, B.Lidx, A.q2.p, A.t2.p, A.s2.p,
                       A.q2o.p, A.t2o.p, E.ddb.len, E.p.cov, E.p.cov_mode, B.alns_b, A.eflag.p, A.mism.p);
}

// the walk over H bytes needs neighbouring cells within 127 of each other: largest substitution score + gap open
// (uc_align.hip tb_walk_kernel); anything else takes the int32 pass
static bool tb_bytes_ok(const Params &p) {
    int m3 = -128, ma = -128, n3 = 127, na = 127;
    for (int k = 0; k < 21 * 21; k++) {
        m3 = std::max<int>(m3, p.S3[k]); ma = std::max<int>(ma, p.SA[k]);
        n3 = std::min<int>(n3, p.S3[k]); na = std::min<int>(na, p.SA[k]);
    }
    return p.gap_open >= p.gap_ext && p.gap_ext >= 0 && m3 + ma + p.gap_open <= 127 && n3 + na >= -127;
}

// MODE 3 weights (diagonal, identity, open, extension), one pass per statistic: columns of the alignment, identities, gaps
constexpr uint32_t TB_LEN[4] = {1u, 0u, 1u, 1u}, TB_IDENT[4] = {0u, 1u, 0u, 0u}, TB_GAPS[4] = {0u, 0u, 1u, 0u};

// the walk over the matrices of pairs [p0, p1) of the plan tb_P3 that are resident now.  Without -a: the statistics walk.  With -a (E.emit_bt):
// count (statistics + runs per pair), scan, make room in the engine's run buffer for exactly that many, write.
template <int PLAIN>
static void tb_walk(Engine &E, uint32_t p0, uint32_t p1, int band, const uint8_t *tbm, const unsigned long long *tboff) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb_P3;
    hipStream_t s = E.stream;
    if (p1 <= p0) return;
    const dim3 grid = grid_for(p1 - p0);
#define UC_TB_WALK(EMIT, base)                                                                                                                   \
    hipLaunchKernelGGL((tb_walk_kernel<EMIT, PLAIN>), grid, dim3(256), 0, s, p0, p1, E.ddb, P3.key2.p, P3.st.p, P3.sqs.p, P3.sqe.p, P3.sts.p, P3.ste.p,  \
                       P3.saux.p, E.p.gap_open, E.p.gap_ext, band, 1, tbm, tboff, A.tb_pack3.p, A.tb_id3.p, A.tb_gaps3.p, A.bt_cnt3.p, A.bt_off3.p,              \
                       E.d_bt_runs.p + (base), (unsigned long long)(base), A.bt_pos3.p, A.bt_plain3.p, A.bt_err.p)
    if (!E.emit_bt) {
        if constexpr (PLAIN == 0) UC_TB_WALK(0, 0);
        else fail(UC_ERR_GENERIC, "the stored-matrix pass runs for backtraces only");
        return;
    }
    UC_TB_WALK(1, 0);
    const size_t k = p1 - p0;
    rocprim_call(A.tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, A.bt_cnt3.p + p0, A.bt_off3.p + p0, 0u, k, rocprim::plus<uint32_t>(), s); });
    uint32_t lo = 0, lc = 0;
    UC_HIP(hipMemcpyAsync(&lo, A.bt_off3.p + (p1 - 1), 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipMemcpyAsync(&lc, A.bt_cnt3.p + (p1 - 1), 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    const uint64_t total = (uint64_t)lo + lc;
    if (total >= (1ull << 31)) fail(UC_ERR_GENERIC, "backtraces: %llu runs in one matrix batch", (unsigned long long)total);
    if (!total) return;
    E.d_bt_runs.grow_preserve(E.bt_used + total, E.bt_used, s);
    UC_TB_WALK(2, E.bt_used);
    E.bt_used += total;
#undef UC_TB_WALK
}

// -a, the pairs [p0, p1) of the plan tb_P3 that the packed kernel does not serve: plain int32 H matrices (tb_plain_dp_kernel) in batches of the same
// budget as the byte matrices, in pair order; a single pair always runs.  Returns the launches.
static uint64_t tb_run_plain(Engine &E, uint32_t p0, uint32_t p1, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb_P3;
    hipStream_t s = E.stream;
    if (p1 <= p0) return 0;
    const size_t k = p1 - p0;
    A.tb_tbsize.reserve((size_t)P3.n + 1); A.tb_tboff.reserve((size_t)P3.n + 1);
    hipLaunchKernelGGL(tb_plain_size_kernel, grid_for(k), dim3(256), 0, s, p0, p1, P3.sqs.p, P3.sqe.p, P3.sts.p, P3.ste.p, A.tb_tbsize.p);
    std::vector<unsigned long long> h_size(k);
    UC_HIP(hipMemcpyAsync(h_size.data(), A.tb_tbsize.p + p0, k * 8, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> h_off(k + 1, 0);
    for (size_t i = 0; i < k; i++) h_off[i + 1] = h_off[i] + h_size[i];
    UC_HIP(hipMemcpyAsync(A.tb_tboff.p + p0, h_off.data(), k * 8, hipMemcpyHostToDevice, s));
    const unsigned long long batch_bytes = budget.batch_bytes(h_off[k], A.tb_tbm.cap);
    A.tb_tbm_live = true;
    struct Live { bool &f; ~Live() { f = false; } } live{A.tb_tbm_live};
    std::vector<std::pair<size_t, size_t>> batches;
    unsigned long long max_bytes = 0;
    for (size_t a = 0; a < k;) {
        size_t b = a + 1;
        while (b < k && h_off[b + 1] - h_off[a] <= batch_bytes) b++;
        batches.emplace_back(a, b);
        max_bytes = std::max(max_bytes, h_off[b] - h_off[a]);
        a = b;
    }
    A.tb_tbm.reserve_exact(max_bytes + 64);
    uint64_t launches = 0;
    double ms = 0;
    for (const auto &bt : batches) {
        const uint32_t a = p0 + (uint32_t)bt.first, b = p0 + (uint32_t)bt.second;
        uint8_t *base = A.tb_tbm.p - h_off[bt.first];                 // (a pair's offset counts from the first pair of the range)
        E.timed_ms_begin();
        hipLaunchKernelGGL(tb_plain_dp_kernel, dim3(std::min<uint32_t>(b - a, 4096u)), dim3(256), 0, s, a, b, E.ddb, P3.key2.p, P3.st.p, P3.sqs.p, P3.sqe.p,
                           P3.sts.p, P3.ste.p, E.p.gap_open, E.p.gap_ext, base, A.tb_tboff.p);
        tb_walk<1>(E, a, b, 0, base, A.tb_tboff.p);
        ms += E.timed_ms_end();
        launches += 3;
    }
    E.stats.sw_kernel_ms += ms;
    if (getenv("UC_TIMING")) fprintf(stderr, "unicore-cluster[timing]: sw pass stored int32 matrices: %zu pairs, %.2f ms, %llu matrix bytes, %zu batch(es)\n",
                                     k, ms, h_off[k], batches.size());
    return launches;
}

// packed MODE 7 for the plan tb_P3 (built in pair order): H bytes of the box's diagonal band (tb_band_of) + walk kernel; queries beyond the
// systolic classes take int32 MODE 3.  Returns the launches.
//
// r05, pk: ONE plan for all flagged pairs of the call, and the byte matrices are produced in batches cut ALONG that plan - a batch is
// a range of its class-sorted task list that fits the matrix budget, i.e. thousands of tasks of one or two length classes per
// launch.  (r04 cut the flagged LIST into batches and planned each: every batch then ran all 28 class kernels with a handful of
// tasks each - 442 batches at nominal configs[3], MODE 7 at 1.5 T cells/s against 5 T for the other passes:
// profiles/r05/sw_pass_timing_*.txt.)
static uint64_t tb_run_bytes(Engine &E, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb_P3;
    hipStream_t s = E.stream;
    const PackedPrefix pk = packed_prefix(P3);           // every systolic class of table 1 is packed, and their tasks come first, in pair order
    const uint32_t n_pk3 = pk.pairs, nt_pk = pk.tasks;
    uint64_t launches = 0;
    double tb_ms = 0;
    unsigned long long total = 0;
    uint32_t nbatch = 0;
    if (P3.n > n_pk3 && E.emit_bt) launches += tb_run_plain(E, n_pk3, P3.n, budget);   // -a: long queries need a stored matrix
    else if (P3.n > n_pk3) {                              // long queries: int32 MODE 3 (no matrices)
        E.timed_ms_begin();
        launches += launch_plan(E, P3, 7, A.tb_pack3.p, nullptr, nullptr, A.work, TB_LEN, /*only_long=*/true);
        launches += launch_plan(E, P3, 3, A.tb_id3.p, nullptr, nullptr, A.work, TB_IDENT, /*only_long=*/true);
        if (E.p.want_tb) launches += launch_plan(E, P3, 3, A.tb_gaps3.p, nullptr, nullptr, A.work, TB_GAPS, /*only_long=*/true);
        tb_ms += E.timed_ms_end();
    }
    if (n_pk3) {
        DevBuf<unsigned long long> &tbsize = A.tb_tbsize, &tboff = A.tb_tboff, &toff = A.tb_toff;
        DevBuf<uint8_t> &tbm = A.tb_tbm;
        tbsize.reserve((size_t)n_pk3 + 1); tboff.reserve((size_t)n_pk3 + 1);
        hipLaunchKernelGGL(tb_size_kernel, grid_for(n_pk3), dim3(256), 0, s, n_pk3, P3.key2.p, P3.segstart.p, P3.ste.p,
                           P3.sts.p, P3.sqs.p, P3.sqe.p, band, 1, tbsize.p);
        rocprim_call(A.tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, tbsize.p, tboff.p, 0ull, (size_t)n_pk3, rocprim::plus<unsigned long long>(), s); });
        // where every task's matrices begin, and its first pair: the host cuts the batches at task boundaries
        toff.reserve((size_t)nt_pk + 1);
        hipLaunchKernelGGL(tb_taskoff_kernel, grid_for(nt_pk), dim3(256), 0, s, nt_pk, P3.tasks.p, tboff.p, toff.p);
        std::vector<unsigned long long> h_toff((size_t)nt_pk + 1);
        std::vector<SwTask> h_task(nt_pk);
        unsigned long long lo_ = 0, ls_ = 0;
        UC_HIP(hipMemcpyAsync(h_toff.data(), toff.p, (size_t)nt_pk * 8, hipMemcpyDeviceToHost, s));
        UC_HIP(hipMemcpyAsync(h_task.data(), P3.tasks.p, (size_t)nt_pk * sizeof(SwTask), hipMemcpyDeviceToHost, s));
        UC_HIP(hipMemcpyAsync(&lo_, tboff.p + (n_pk3 - 1), 8, hipMemcpyDeviceToHost, s));
        UC_HIP(hipMemcpyAsync(&ls_, tbsize.p + (n_pk3 - 1), 8, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        total = lo_ + ls_;
        h_toff[nt_pk] = total;
        const unsigned long long batch_bytes = budget.batch_bytes(total, tbm.cap);
        A.tb_tbm_live = true;
        struct Live { bool &f; ~Live() { f = false; } } live{A.tb_tbm_live};
        // the batches first, then ONE buffer for the largest of them (r06: every batch that was a little larger than the buffer the first
        // one had sized took a new ~30 GiB block - 12 allocations of 0.8 s each in a 14 s call at 500 proteomes on a box with untouched memory)
        std::vector<std::pair<uint32_t, uint32_t>> batches;
        unsigned long long max_bytes = 0;
        for (uint32_t t0 = 0; t0 < nt_pk;) {
            uint32_t t1 = t0 + 1;                      // (a single task always runs, whatever the budget: tests force tiny budgets)
            while (t1 < nt_pk && h_toff[t1 + 1] - h_toff[t0] <= batch_bytes) t1++;
            batches.emplace_back(t0, t1);
            max_bytes = std::max(max_bytes, h_toff[t1] - h_toff[t0]);
            t0 = t1;
        }
        tbm.reserve_exact(std::max<unsigned long long>(max_bytes, std::min<unsigned long long>(total, batch_bytes)) + 64);
        for (const auto &bt : batches) {
            const uint32_t t0 = bt.first, t1 = bt.second;
            const unsigned long long base = h_toff[t0];
            const uint32_t p0 = h_task[t0].begin, p1 = t1 < nt_pk ? h_task[t1].begin : n_pk3;
            P3.tbm = tbm.p - base; P3.tboff = tboff.p; P3.tb_band = band;      // (a pair's offset counts from the start of the WHOLE plan)
            E.timed_ms_begin();
            launches += launch_plan(E, P3, 7, A.tb_pack3.p, nullptr, nullptr, A.work, nullptr, false, t0, t1, /*skip_long=*/true);
            tb_walk<0>(E, p0, p1, band, tbm.p - base, tboff.p);
            tb_ms += E.timed_ms_end();
            nbatch++;
        }
        P3.tbm = nullptr; P3.tboff = nullptr; P3.tb_band = 0;
    }
    E.stats.sw_kernel_ms += tb_ms;
    if (getenv("UC_TIMING")) fprintf(stderr, "unicore-cluster[timing]: sw pass mode 7: %u pairs, %llu cells, %.2f ms (%llu launches), %llu matrix bytes, band %d, %u batch(es)\n",
                        P3.n, (unsigned long long)P3.cells, tb_ms, (unsigned long long)launches, total, band, nbatch);
    return launches;
}

// the traceback statistics of the flagged gate passers: gather, plan, run, apply.  pk: packed MODE 7 (tb_run_bytes); otherwise the int32
// kernel carries the statistics through the DP (MODE 3, one pass per statistic: TB_LEN, TB_IDENT, TB_GAPS).  band > 0: the walk marks the pairs whose path left the
// band in tb_tmiss.
static void tb_batch(Engine &E, const AlignBatch &B, const uint32_t *flag, bool pk, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    const uint32_t nt = compact(E, A.tmp, flag, A.tb_tpos.p, n2);
    if (!nt) return;
    A.tb_q3.reserve(nt); A.tb_t3.reserve(nt); A.tb_src3.reserve(nt); A.tb_qs3.reserve(nt); A.tb_qe3.reserve(nt); A.tb_ts3.reserve(nt); A.tb_te3.reserve(nt);
    A.tb_pack3.reserve(nt); A.tb_id3.reserve(nt); A.tb_gaps3.reserve(nt); A.tb_sc3.reserve(nt);
    hipLaunchKernelGGL(tb_gather_kernel, grid_for(n2), dim3(256), 0, s, n2, flag, A.tb_tpos.p, A.iota2.p, A.link.p, B.Lidx, A.q2.p,
                       A.t2.p, B.alns_b, A.tb_q3.p, A.tb_t3.p, A.tb_qs3.p, A.tb_qe3.p, A.tb_ts3.p, A.tb_te3.p, A.tb_src3.p, A.tb_sc3.p);
    SwPlan &P3 = A.tb_P3;
    uint64_t launches = 0;
    int passes = 1;
    if (E.emit_bt) {
        A.bt_cnt3.reserve(nt); A.bt_off3.reserve(nt); A.bt_plain3.reserve(nt); A.bt_pos3.reserve(nt); A.bt_err.reserve(1);
        UC_HIP(hipMemsetAsync(A.bt_cnt3.p, 0, (size_t)nt * 4, s));
        UC_HIP(hipMemsetAsync(A.bt_err.p, 0, 4, s));
    }
    if (!pk && E.emit_bt) {   // -a: MODE 3 has no path to give; every pair takes the stored int32 matrix and the walk
        build_plan(E, P3, A.tmp, nt, A.tb_q3.p, A.tb_t3.p, A.tb_qe3.p, A.tb_te3.p, 1, A.tb_qs3.p, A.tb_ts3.p, A.tb_sc3.p, /*lpt=*/false);
        launches = tb_run_plain(E, 0, P3.n, budget);
    } else if (!pk) {
        build_plan(E, P3, A.tmp, nt, A.tb_q3.p, A.tb_t3.p, A.tb_qe3.p, A.tb_te3.p, 2, A.tb_qs3.p, A.tb_ts3.p);
        E.timed_ms_begin();
        launches = launch_plan(E, P3, 3, A.tb_pack3.p, nullptr, nullptr, A.work, TB_LEN);
        launches += launch_plan(E, P3, 3, A.tb_id3.p, nullptr, nullptr, A.work, TB_IDENT);
        passes = 2;
        if (E.p.want_tb) {   // third statistic of the same traceback: number of gaps (BLAST-tab "gapopen")
            launches += launch_plan(E, P3, 3, A.tb_gaps3.p, nullptr, nullptr, A.work, TB_GAPS);
            passes = 3;
        }
        E.stats.sw_kernel_ms += E.timed_ms_end();
    } else {
        build_plan(E, P3, A.tmp, nt, A.tb_q3.p, A.tb_t3.p, A.tb_qe3.p, A.tb_te3.p, 1, A.tb_qs3.p, A.tb_ts3.p, A.tb_sc3.p, /*lpt=*/false);
        launches = tb_run_bytes(E, band, budget);
    }
    E.stats.sw_kernel_launches += launches;
    E.stats.sw_algorithmic_bytes += passes * P3.alg_bytes;
    E.stats.cells_run += passes * P3.cells;
    E.stats.n_sw_runs += (uint64_t)passes * P3.n;
    hipLaunchKernelGGL(tb_apply_kernel, grid_for(nt), dim3(256), 0, s, nt, P3.idx.p, A.tb_src3.p, A.tb_pack3.p, A.tb_id3.p,
                       E.p.want_tb ? A.tb_gaps3.p : (const int32_t *)nullptr, A.iota2.p, A.link.p, B.Lidx, E.p.min_seq_id, B.alns_b,
                       A.eflag.p, A.tb_ttie.p, (pk && band > 0) ? A.tb_tmiss.p : (uint32_t *)nullptr);
    if (E.emit_bt) {
        if (!B.bt_pos_b) fail(UC_ERR_GENERIC, "backtraces: the batch has no place for them");
        hipLaunchKernelGGL(bt_apply_kernel, grid_for(nt), dim3(256), 0, s, nt, P3.idx.p, A.tb_src3.p, A.bt_cnt3.p, A.bt_pos3.p, A.bt_plain3.p,
                           A.iota2.p, A.link.p, B.Lidx, B.bt_pos_b, B.bt_n_b);
        uint32_t err = 0;
        UC_HIP(hipMemcpyAsync(&err, A.bt_err.p, 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        if (err) fail(UC_ERR_GENERIC, "backtraces: a path did not fit the slice its own count had sized");
    }
}

// packed MODE 7 for the flagged pairs, in segments of budget.segment_pairs() pairs (TbBudget)
static void tb_segments(Engine &E, const AlignBatch &B, const uint32_t *flag, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    const uint32_t n2 = B.n2, seg = budget.segment_pairs();
    const uint32_t nlo = compact(E, A.tmp, flag, A.tb_tcpos.p, n2);
    if (nlo <= seg) { if (nlo) tb_batch(E, B, flag, true, band, budget); return; }
    for (uint32_t lo = 0; lo < nlo; lo += seg) {
        hipLaunchKernelGGL(tb_chunk_kernel, grid_for(n2), dim3(256), 0, E.stream, n2, flag, A.tb_tcpos.p, lo, std::min<uint32_t>(nlo, lo + seg), A.tb_tchunk.p);
        tb_batch(E, B, A.tb_tchunk.p, true, band, budget);
    }
}

// the traceback statistics of the flagged gate passers, on the packed kernel where its range and the byte walk allow it
static void run_tb(Engine &E, const AlignBatch &B, const uint32_t *flag, int band_w, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    const uint32_t n2 = B.n2;
    if (!E.p.sw_pk || !tb_bytes_ok(E.p)) { tb_batch(E, B, flag, false, 0, budget); return; }
    A.tb_tlo.reserve(n2); A.tb_thi.reserve(n2); A.tb_tmiss.reserve(n2); A.tb_tchunk.reserve(n2); A.tb_tcpos.reserve(n2);
    hipLaunchKernelGGL(tb_split_kernel, grid_for(n2), dim3(256), 0, E.stream, n2, flag, A.link.p, B.Lidx, B.alns_b, SW_PK_OVF_HOST, A.tb_tlo.p, A.tb_thi.p);
    tb_batch(E, B, A.tb_thi.p, false, 0, budget);                       // scores beyond the packed range: int32 MODE 3
    if (band_w > 0) UC_HIP(hipMemsetAsync(A.tb_tmiss.p, 0, (size_t)n2 * 4, E.stream));
    tb_segments(E, B, A.tb_tlo.p, band_w, budget);
    if (band_w > 0) tb_segments(E, B, A.tb_tmiss.p, 0, budget);          // tracebacks that left their band: the whole box
}

// the class a plan of table `tab` puts each pair in (class_of, as plan_key_kernel keys it; c_tab[tab].n = long-query kernel)
__global__ void __launch_bounds__(256) pass_class_kernel(uint32_t n, const uint32_t *q, const uint32_t *len, int tab, int32_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = class_of((int)len[q[i]], tab);
}
// the records the traceback passes read their boxes and end-cell scores from
__global__ void __launch_bounds__(256) pass_records_kernel(uint32_t n, const int32_t *qs, const int32_t *qe, const int32_t *ts, const int32_t *te,
                                                           const int32_t *known, uc_aln *out, uint32_t *iota, uint32_t *all) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        uc_aln a = {};
        a.score = known ? known[i] : 0;
        a.qstart = qs[i]; a.qend = qe[i]; a.tstart = ts[i]; a.tend = te[i];
        a.aln_len = -1; a.idents = -1; a.gap_opens = -1;
        out[i] = a;
        iota[i] = i;
        all[i] = 1u;
    }
}

// ---- kernel-level entry point: ONE gapped pass (table, mode) on a pair list from the host -----------
// The passes of Engine::align on a list the caller chooses: build_plan + launch_plan (raw) or run_plan (the library's re-run rules) for
// MODE 0/1/2/4/6; the traceback passes through run_tb / tb_batch / tb_run_bytes on a batch whose gate passers are exactly the listed pairs.
static bool sw_pass_allowed(int tab, int mode) {
    switch (tab) {
    case 0: return mode == 0 || mode == 1 || mode == 2;
    case 1: return mode == 0 || mode == 1 || mode == 2 || mode == 4 || mode == 6 || mode == 7;
    case 2: return mode == 3;
    case 3: return mode == 4 || mode == 6;
    default: return false;
    }
}

// slices of records (pos, n) cut from the host copy `hruns` of the run buffer from element `base` on; bit 31 of n exchanges I and D
static void bt_assemble(size_t n, const unsigned long long *pos, const uint32_t *cnt, const uc_aln *alns /* null: every record counts */,
                        const uint32_t *hruns, uint64_t base, uint64_t *run_off, std::vector<uint32_t> &runs) {
    runs.clear();
    for (size_t i = 0; i < n; i++) {
        run_off[i] = runs.size();
        if (alns && !alns[i].accepted) continue;
        const uint32_t k = cnt[i] & 0x3FFFFFFFu;
        const bool swap = (cnt[i] >> 31) != 0;
        const uint32_t *r = k ? hruns + (pos[i] - base) : nullptr;
        for (uint32_t x = 0; x < k; x++) {
            uint32_t v = r[x];
            if (swap && (v & 3u)) v ^= 3u;                 // I (1) <-> D (2)
            runs.push_back(v);
        }
    }
    run_off[n] = runs.size();
}

void Engine::get_backtraces(uint64_t begin, uint64_t n, uint64_t *run_off, std::vector<uint32_t> &runs) const {
    runs.clear();
    if (!n) { run_off[0] = 0; return; }
    if (!emit_bt || !alns_valid || !d_bt_n.p) fail(UC_ERR_ARGS, "backtraces: this engine has not aligned with -a");
    UC_HIP(hipSetDevice(device));
    std::vector<unsigned long long> pos(n);
    std::vector<uint32_t> cnt(n), hr(std::max<uint64_t>(bt_used, 1));
    std::vector<uc_aln> al(n);
    UC_HIP(hipMemcpy(pos.data(), d_bt_pos.p + begin, n * 8, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(cnt.data(), d_bt_n.p + begin, n * 4, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(al.data(), d_alns.p + begin, n * sizeof(uc_aln), hipMemcpyDeviceToHost));
    if (bt_used) UC_HIP(hipMemcpy(hr.data(), d_bt_runs.p, bt_used * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++)
        if (al[i].accepted && ((cnt[i] & 0x3FFFFFFFu) == 0 || pos[i] + (cnt[i] & 0x3FFFFFFFu) > bt_used))
            fail(UC_ERR_GENERIC, "backtraces: accepted hit %llu has no path", (unsigned long long)(begin + i));
    bt_assemble(n, pos.data(), cnt.data(), al.data(), hr.data(), 0, run_off, runs);
}

void Engine::tb_emit_pass(int route, int band, const std::vector<SwPassPair> &pairs, const SwPassOut &o, BtPassOut &bt) {
    if (route < 0 || route > 3) fail(UC_ERR_ARGS, "tb_emit_pass: route must be 0..3");
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    const uint32_t sys_cap = (uint32_t)h_tab[1].cap[h_tab[1].n - 1];
    for (const SwPassPair &x : pairs) {
        if (x.q >= hdb.n) fail(UC_ERR_ARGS, "tb_emit_pass: sequence id out of range");
        if (route == 3 && h_len[x.q] <= sys_cap) fail(UC_ERR_ARGS, "tb_emit_pass: the long-query route takes queries of more than %u residues", sys_cap);
        if (route <= 1 && h_len[x.q] > sys_cap) fail(UC_ERR_ARGS, "tb_emit_pass: the packed route takes queries of up to %u residues", sys_cap);
    }
    if (route == 2) sw_pass(2, 3, 0, true, pairs, o, &bt);
    else sw_pass(1, 7, route == 1 ? 0 : band, true, pairs, o, &bt);
}

void Engine::sw_pass(int tab, int mode, int band, bool raw, const std::vector<SwPassPair> &pairs, const SwPassOut &o, BtPassOut *bt) {
    PressureScope ps(*this, 1);
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    if (!sw_pass_allowed(tab, mode)) fail(UC_ERR_ARGS, "sw_pass: no such (table, mode)");
    if (mode == 7 && (!tb_bytes_ok(p) || !p.sw_pk)) fail(UC_ERR_ARGS, "sw_pass: MODE 7 needs the byte walk's score range and the packed kernel");
    if (band < 0) fail(UC_ERR_ARGS, "sw_pass: negative band");
    const size_t n = pairs.size();
    if (bt) { bt->run_off.assign(n + 1, 0); bt->runs.clear(); bt->plain.assign(n, 0); }
    if (n == 0) return;
    if (n >= (1ull << 31)) fail(UC_ERR_ARGS, "sw_pass: too many pairs");
    const bool ends = mode == 2 || mode == 6, box = mode == 3 || mode == 7, known = mode == 4 || mode == 6 || mode == 7;
    for (size_t i = 0; i < n; i++) {
        const SwPassPair &x = pairs[i];
        if (x.q >= hdb.n || x.t >= hdb.n) fail(UC_ERR_ARGS, "sw_pass: sequence id out of range");
        const int lq = (int)h_len[x.q], lt = (int)h_len[x.t];
        if ((ends || box) && (x.qe < 0 || x.te < 0 || x.qe >= lq || x.te >= lt)) fail(UC_ERR_ARGS, "sw_pass: end position out of range");
        if (box && (x.qs < 0 || x.ts < 0 || x.qs > x.qe || x.ts > x.te)) fail(UC_ERR_ARGS, "sw_pass: box start out of range");
        if (known && x.known <= 0) fail(UC_ERR_ARGS, "sw_pass: known score missing");
    }
    UC_HIP(hipSetDevice(device));
    std::vector<uint32_t> hq(n), ht(n);
    std::vector<int32_t> hqs(n), hqe(n), hts(n), hte(n), hk(n);
    for (size_t i = 0; i < n; i++) {
        const SwPassPair &x = pairs[i];
        hq[i] = x.q; ht[i] = x.t; hqs[i] = x.qs; hqe[i] = x.qe; hts[i] = x.ts; hte[i] = x.te; hk[i] = x.known;
    }
    const uint32_t nn = (uint32_t)n;
    DevBuf<uint32_t> dq, dt;
    DevBuf<int32_t> dqs, dqe, dts, dte, dk, os, oq, ot, rs, rq, rt, cls;
    auto up = [&](auto &d, const auto &h) { d.reserve(n); UC_HIP(hipMemcpyAsync(d.p, h.data(), n * 4, hipMemcpyHostToDevice, stream)); };
    up(dq, hq); up(dt, ht); up(dqs, hqs); up(dqe, hqe); up(dts, hts); up(dte, hte); up(dk, hk);
    cls.reserve(n);
    auto down = [&](int32_t *h, const int32_t *d) { if (h) UC_HIP(hipMemcpyAsync(h, d, n * 4, hipMemcpyDeviceToHost, stream)); };
    // (after the pass: build_plan is what puts the class tables into this device's constant memory)
    auto classes = [&] {
        hipLaunchKernelGGL(pass_class_kernel, grid_for(nn), dim3(256), 0, stream, nn, dq.p, ddb.len, tab, cls.p);
        down(o.cls, cls.p);
    };
    if (!box) {
        const bool track = mode != 1;
        DevBuf<int32_t> work;
        DevBuf<char> tmp;
        os.reserve(n); rs.reserve(n);
        if (track) { oq.reserve(n); ot.reserve(n); rq.reserve(n); rt.reserve(n); }
        // the second tie-break answer of the known-score modes (-2 for a pair that the packed known-score kernel did not compute)
        const bool second = o.qe2 || o.te2;
        if (second && mode != 4 && mode != 6) fail(UC_ERR_ARGS, "sw_pass: only modes 4 and 6 have a second answer");
        DevBuf<int32_t> oq2, ot2, rq2, rt2;
        if (second) { oq2.reserve(n); ot2.reserve(n); rq2.reserve(n); rt2.reserve(n); }
        const SwSecond sec{oq2.p, ot2.p};
        SwPlan P;
        build_plan(*this, P, tmp, nn, dq.p, dt.p, ends ? dqe.p : nullptr, ends ? dte.p : nullptr, tab, nullptr, nullptr, known ? dk.p : nullptr);
        if (raw) {      // (event-timed like run_plan's launches: tools/ungapped_all_rate.py reads the pass's kernel time)
            timed_ms_begin();
            launch_plan(*this, P, mode, os.p, oq.p, ot.p, work, nullptr, false, 0, 0xFFFFFFFFu, false, second ? &sec : nullptr);
            stats.sw_kernel_ms += timed_ms_end();
        }
        else run_plan(*this, P, mode, os.p, oq.p, ot.p, work, tmp, false, second ? &sec : nullptr);
        hipLaunchKernelGGL(scatter3_kernel, grid_for(nn), dim3(256), 0, stream, nn, P.idx.p, os.p, oq.p, ot.p, rs.p, rq.p, rt.p);
        if (second) hipLaunchKernelGGL(scatter3_kernel, grid_for(nn), dim3(256), 0, stream, nn, P.idx.p, oq2.p, oq2.p, ot2.p, rq2.p, rq2.p, rt2.p);
        classes();
        down(o.score, rs.p);
        if (track) { down(o.qe, rq.p); down(o.te, rt.p); }
        if (second) { down(o.qe2, rq2.p); down(o.te2, rt2.p); }
        UC_HIP(hipStreamSynchronize(stream));
        UC_HIP(hipGetLastError());
        return;
    }
    // traceback statistics: a batch whose gate passers are the listed pairs, in list order, with their boxes in the records
    AlignScratch &A = scratch_of(*this);
    DevBuf<uc_aln> recs;
    DevBuf<uint32_t> iota, all;
    recs.reserve(n); iota.reserve(n); all.reserve(n);
    hipLaunchKernelGGL(pass_records_kernel, grid_for(nn), dim3(256), 0, stream, nn, dqs.p, dqe.p, dts.p, dte.p, dk.p, recs.p, iota.p, all.p);
    A.q2.reserve(n); A.t2.reserve(n); A.link.reserve(n); A.iota2.reserve(n); A.eflag.reserve(n);
    A.tb_trun.reserve(n); A.tb_tpos.reserve(n); A.tb_tpart.reserve(n); A.tb_ttie.reserve(n); A.tb_tmiss.reserve(n);
    UC_HIP(hipMemcpyAsync(A.q2.p, dq.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.t2.p, dt.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.link.p, iota.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.iota2.p, iota.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.eflag.p, all.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemsetAsync(A.tb_ttie.p, 0, n * 4, stream));
    UC_HIP(hipMemsetAsync(A.tb_tmiss.p, 0, n * 4, stream));
    AlignBatch B{};
    B.n = nn; B.n2 = nn; B.dq = dq.p; B.dt = dt.p; B.alns_b = recs.p; B.alns_list = recs.p; B.tab = tab; B.Lidx = iota.p;
    struct Keep { Params &p; Params saved; ~Keep() { p = saved; } } keep{p, p};
    // with emission: the slices go behind whatever the engine's run buffer holds and are given back at the end; the per-record arrays are the pass's own
    struct KeepBt { Engine &E; bool emit; uint64_t used; ~KeepBt() { E.emit_bt = emit; E.bt_used = used; } } keep_bt{*this, emit_bt, bt_used};
    DevBuf<unsigned long long> bpos;
    DevBuf<uint32_t> bn;
    emit_bt = bt != nullptr;
    if (bt) {
        bpos.reserve(n); bn.reserve(n);
        UC_HIP(hipMemsetAsync(bn.p, 0, n * 4, stream));
        B.bt_pos_b = bpos.p; B.bt_n_b = bn.p;
    }
    p.want_tb = 1;         // every statistic: alignment length, identities and the gap count (the TB_GAPS weighting of MODE 3)
    p.min_seq_id = 0.0f;   // no gate on the result
    const TbBudget budget;
    if (mode == 3) tb_batch(*this, B, all.p, false, 0, budget);
    else if (raw) tb_batch(*this, B, all.p, true, band, budget);
    else run_tb(*this, B, all.p, band, budget);
    classes();
    std::vector<uc_aln> h(n);
    UC_HIP(hipMemcpyAsync(h.data(), recs.p, n * sizeof(uc_aln), hipMemcpyDeviceToHost, stream));
    if (o.miss) UC_HIP(hipMemcpyAsync(o.miss, A.tb_tmiss.p, n * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
    if (o.miss && (mode != 7 || band == 0)) memset(o.miss, 0, n * 4);
    if (bt) {
        std::vector<unsigned long long> pos(n);
        std::vector<uint32_t> cnt(n), hr(std::max<uint64_t>(bt_used - keep_bt.used, 1));
        UC_HIP(hipMemcpy(pos.data(), bpos.p, n * 8, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(cnt.data(), bn.p, n * 4, hipMemcpyDeviceToHost));
        if (bt_used > keep_bt.used) UC_HIP(hipMemcpy(hr.data(), d_bt_runs.p + keep_bt.used, (bt_used - keep_bt.used) * 4, hipMemcpyDeviceToHost));
        bt_assemble(n, pos.data(), cnt.data(), nullptr, hr.data(), keep_bt.used, bt->run_off.data(), bt->runs);
        for (size_t i = 0; i < n; i++) bt->plain[i] = (cnt[i] >> 30) & 1;
    }
    for (size_t i = 0; i < n; i++) {
        if (o.score) o.score[i] = h[i].score;
        if (o.aln_len) o.aln_len[i] = h[i].aln_len;
        if (o.idents) o.idents[i] = h[i].idents;
        if (o.gaps) o.gaps[i] = h[i].gap_opens;
    }
}

// sequence-identity gate / BLAST-tab statistics: (alignment length, identities[, gaps]) of the traceback on
// the box, for the pairs that passed the coverage gate
static void traceback_stats(Engine &E, const AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    // the plans of the passes behind us are dead (their results have been scattered): at sizes where the matrix budget is what is left of the
    // device (nominal configs[3]: ~35 GB of plan arrays beside ~57 GiB of matrices per batch) they go back before the matrices are sized
    // (r06, ADVICE r05: only when memory IS short, i.e. when what is free would not give the matrix buffer its full budget (64 GiB = 55 % of 116 GiB) -
    // re-allocating ~35 GB of plan arrays in the next 256 M-pair batch costs 1-2 s, more than the few batches the room buys: UC_ALLOC_LOG at nominal
    // configs[3] showed 443 GiB of 1-2 GiB blocks, 10-12 s per call, profiles/r06/c4_nominal_alloc.txt)
    size_t free_now = 0, total_now = 0;
    const bool mem_short = hipMemGetInfo(&free_now, &total_now) != hipSuccess || free_now + A.tb_tbm.cap < (120ull << 30);
    if (n2 >= (8u << 20) && mem_short) {
        UC_HIP(hipStreamSynchronize(s));
        A.P1.release(); A.P2.release(); A.P2b.release(); A.rr_P2.release(); A.amb_P3.release();
        if (B.dedup) A.P0.release();                   // (without sharing, Lsq / Lst / Lidx ARE P0's arrays)
    }
    A.tb_trun.reserve(n2); A.tb_tpos.reserve(n2); A.tb_tpart.reserve(n2); A.tb_ttie.reserve(n2);
    UC_HIP(hipMemsetAsync(A.tb_ttie.p, 0, (size_t)n2 * 4, s));
    unsigned long long hc = 0;
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 8, s));
    hipLaunchKernelGGL(cells_tb_kernel, grid_for(n2, E.count_grid_cap), dim3(256), 0, s, n2, A.eflag.p, A.link.p, B.Lidx, B.alns_b, A.d_cells.p);
    UC_HIP(hipMemcpyAsync(&hc, A.d_cells.p, 8, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    E.stats.cells_tb += hc;
    // r05: MODE 7 stores a diagonal band of the box, not the box (tb_band_of); the few pairs whose traceback leaves the band are redone
    // with everything stored.  UC_TB_BAND = half-width W (default 48; 0 = always the whole box; the tests force 1 and 4)
    const int band_w = getenv("UC_TB_BAND") ? std::max(0, atoi(getenv("UC_TB_BAND"))) : 48;
    const TbBudget budget;
    if (B.dedup) {
        hipLaunchKernelGGL(tbm_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.eflag.p, A.link.p, B.Lidx, A.mirror.p, A.gflag.p, A.gpos.p,
                           B.alns_b, A.tb_trun.p, A.tb_tpart.p);
        run_tb(E, B, A.tb_trun.p, band_w, budget);
        hipLaunchKernelGGL(tbm_resolve_kernel, grid_for(n2), dim3(256), 0, s, n2, A.tb_tpart.p, A.tb_ttie.p, A.link.p, B.Lidx, E.p.min_seq_id,
                           B.alns_b, A.eflag.p, A.tb_trun.p);
        if (E.emit_bt) hipLaunchKernelGGL(bt_mirror_kernel, grid_for(n2), dim3(256), 0, s, n2, A.tb_tpart.p, A.tb_ttie.p, A.link.p, B.Lidx, B.bt_pos_b, B.bt_n_b);
        run_tb(E, B, A.tb_trun.p, band_w, budget);   // mirrors whose representative had a gap-direction tie on its traceback
    } else {
        UC_HIP(hipMemcpyAsync(A.tb_trun.p, A.eflag.p, (size_t)n2 * 4, hipMemcpyDeviceToDevice, s));
        run_tb(E, B, A.tb_trun.p, band_w, budget);
    }
}

// the accepted edges of the batch (ne flagged in eflag / epos) appended to the engine's device edge list
static void append_edges(Engine &E, const AlignBatch &B, uint32_t ne) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    A.d_e.reserve(2 * (size_t)ne);
    hipLaunchKernelGGL(edge_scatter_kernel, grid_for(B.n2), dim3(256), 0, s, B.n2, A.eflag.p, A.epos.p, A.q2.p, A.t2.p, A.d_e.p);
    if (E.edges_on_host && !E.edges.empty()) {   // a host list from an earlier call that was read back: continue on the device
        E.d_edges.reserve(E.edges.size());
        UC_HIP(hipMemcpyAsync(E.d_edges.p, E.edges.data(), E.edges.size() * 4, hipMemcpyHostToDevice, s));
        E.n_edges_dev = E.edges.size() / 2;
    }
    E.d_edges.grow_preserve(2 * (E.n_edges_dev + ne), 2 * E.n_edges_dev, s);
    UC_HIP(hipMemcpyAsync(E.d_edges.p + 2 * E.n_edges_dev, A.d_e.p, 2 * (size_t)ne * 4, hipMemcpyDeviceToDevice, s));
    E.n_edges_dev += ne;
    E.edges_on_host = false;
}

// end of a batch: every start-pass score must equal its forward score; the records of a length-gated list go back to the hit-list order
static void finish_batch(Engine &E, const AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    uint32_t bad = 0;
    UC_HIP(hipMemcpyAsync(&bad, A.mism.p, 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipGetLastError());
    if (bad) fail(UC_ERR_GENERIC, "start pass score differs from the forward score for %u pairs", bad);
    E.stats.n_gapped_alignments += B.n;
    E.stats.n_start_alignments += B.n2;
    if (B.alns_b != B.alns_list) {
        hipLaunchKernelGGL(len_gate_putback_kernel, grid_for(B.n), dim3(256), 0, s, B.n, A.lg_map.p, (const uc_aln *)B.alns_b, B.alns_list);
        if (B.bt_pos_b) hipLaunchKernelGGL(bt_putback_kernel, grid_for(B.n), dim3(256), 0, s, B.n, A.lg_map.p, A.lg_btpos.p, A.lg_btn.p, E.d_bt_pos.p + E.hit_off[B.qa], E.d_bt_n.p + E.hit_off[B.qa]);
        UC_HIP(hipStreamSynchronize(s));
    }
}

void Engine::align(uint32_t qbegin, uint32_t qend) {
    PressureScope ps(*this, 1);
    if (!have_db) fail(UC_ERR_ARGS, "no database loaded");
    if (qbegin > qend || qend > hdb.n) fail(UC_ERR_ARGS, "align: bad query range");
    UC_HIP(hipSetDevice(device));
    Timer tm;
    hipStream_t s = stream;
    const uint64_t dbres = evalue_residues ? evalue_residues : hdb.residues();
    // records of queries outside [qbegin,qend) must read as "not aligned" (all zero), never as leftovers of an earlier hit
    // list: the array is cleared whenever the hit lists changed since the last align (0.2 ms at 14 M records)
    d_alns.reserve(std::max<uint64_t>(n_hits, 1));
    if (!alns_valid && n_hits) UC_HIP(hipMemsetAsync(d_alns.p, 0, n_hits * sizeof(uc_aln), s));
    if (emit_bt) {   // -a: slice position and run count per hit, parallel to d_alns; the runs of earlier calls on these hit lists stay
        if (!alns_valid) { bt_used = 0; d_bt_pos.release(); d_bt_n.release(); }
        if (!d_bt_n.p) {
            d_bt_pos.reserve(std::max<uint64_t>(n_hits, 1)); d_bt_n.reserve(std::max<uint64_t>(n_hits, 1));
            UC_HIP(hipMemsetAsync(d_bt_n.p, 0, std::max<uint64_t>(n_hits, 1) * 4, s));
        }
        if (hit_off[qend] > hit_off[qbegin]) UC_HIP(hipMemsetAsync(d_bt_n.p + hit_off[qbegin], 0, (hit_off[qend] - hit_off[qbegin]) * 4, s));
    }
    // E-value gate as an integer threshold per query length (host; exp() evaluated once per distinct length)
    std::vector<int32_t> ms_by_len(65536, -1), h_ms(qend - qbegin);
    if (!p.min_score_table.empty() && p.min_score_table.size() != hdb.n)
        fail(UC_ERR_ARGS, "--min-score-table holds %zu thresholds, the database has %u sequences", p.min_score_table.size(), hdb.n);
    for (uint32_t q = qbegin; q < qend; q++) {
        if (!p.min_score_table.empty()) { h_ms[q - qbegin] = p.min_score_table[q]; continue; }     // rule UC-1/E (optional): thresholds of a fitted per-query model
        int32_t &m = ms_by_len[h_len[q]];
        if (m < 0) m = min_score_for(p, (int)h_len[q], dbres);
        h_ms[q - qbegin] = m;
    }
    AlignScratch &A = scratch_of(*this);
    A.d_cells.reserve(2);
    A.d_ms.reserve(std::max<size_t>(h_ms.size(), 1));
    if (!h_ms.empty()) UC_HIP(hipMemcpyAsync(A.d_ms.p, h_ms.data(), h_ms.size() * 4, hipMemcpyHostToDevice, s));
    A.mism.reserve(1);
    UC_HIP(hipMemsetAsync(A.mism.p, 0, 4, s));

    const uint64_t CHUNK = 256ull << 20;  // pairs per device batch (~150 B of plan/result state per pair; mutual hits only share a DP inside a batch)
    for (uint32_t qa = qbegin; qa < qend;) {
        uint32_t qb = qa;
        while (qb < qend && (qb == qa || hit_off[qb + 1] - hit_off[qa] <= CHUNK)) qb++;
        const uint64_t b = hit_off[qa];
        AlignBatch B{qbegin, qa, qb, (uint32_t)(hit_off[qb] - b), d_hq.p + b, d_ht.p + b, d_alns.p + b, d_alns.p + b, false, p.sw_pk ? 1 : 0};
        if (emit_bt) { B.bt_pos_b = d_bt_pos.p + b; B.bt_n_b = d_bt_n.p + b; }
        qa = qb;
        if (p.len_gate && p.cov > 0.0f && B.n) length_gate(*this, B);
        if (!B.n) continue;
        B.dedup = p.sym_dedup && p.mat_symmetric && B.n >= 2 && hdb.n <= (1u << 24);
        forward_pass(*this, B);
        if (p.rev_correction) rev_correction_pass(*this, B);
        if (B.dedup) {   // the shared-DP passes count their cells on the device
            unsigned long long hc[2] = {0, 0};
            UC_HIP(hipMemcpyAsync(hc, A.d_cells.p, 16, hipMemcpyDeviceToHost, s));
            UC_HIP(hipStreamSynchronize(s));
            stats.cells_fwd += hc[0];
            stats.cells_rev += hc[1];
        }
        evalue_gate(*this, B);
        if (B.n2) {
            start_pass(*this, B);
            uint32_t ne = compact(*this, A.tmp, A.eflag.p, A.epos.p, B.n2);
            if ((p.min_seq_id > 0.0f || p.want_tb) && ne) {
                traceback_stats(*this, B);
                ne = compact(*this, A.tmp, A.eflag.p, A.epos.p, B.n2);
            }
            if (ne) append_edges(*this, B, ne);
        }
        finish_batch(*this, B);
    }
    alns_valid = true;
    last_align_hits = qbegin == 0 && qend == hdb.n ? n_hits : 0;      // what the buffers of this set have just served (uc_prefilter.hip: scratch_release_target)
    stats.n_edges = edges_on_host ? edges.size() / 2 : n_edges_dev;
    stats.algorithmic_bytes[UC_ST_GAPPED] = stats.sw_algorithmic_bytes;
    stats.stage_seconds[UC_ST_GAPPED] += tm.seconds();
}

// ---- E7 graph construction on the device (the greedy cover follows below; uc_setcover.cpp is the all-host variant behind uc_setcover) ----
// both directions of every accepted pair as 64-bit keys, self loops -> all-ones (sorted last, dropped)
__global__ void __launch_bounds__(256) edge_key_kernel(uint64_t n_edges, const uint32_t *e, uint32_t n, uint64_t *key, uint32_t *bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_edges; i += (uint64_t)gridDim.x * 256) {
        const uint32_t a = e[2 * i], b = e[2 * i + 1];
        if (a >= n || b >= n) { atomicAdd(bad, 1u); key[2 * i] = ~0ull; key[2 * i + 1] = ~0ull; continue; }
        key[2 * i] = a == b ? ~0ull : ((uint64_t)a << 32) | b;
        key[2 * i + 1] = a == b ? ~0ull : ((uint64_t)b << 32) | a;
    }
}
__global__ void __launch_bounds__(256) edge_uniq_kernel(uint64_t m, const uint64_t *key, uint32_t *flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256)
        flag[i] = (key[i] != ~0ull && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) edge_adj_kernel(uint64_t m, const uint64_t *key, const uint32_t *flag, const uint32_t *pos,
                                                       uint64_t *ukey, uint32_t *adj) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256)
        if (flag[i]) { ukey[pos[i]] = key[i]; adj[pos[i]] = (uint32_t)key[i]; }
}
__global__ void __launch_bounds__(256) edge_off_kernel(uint32_t n, const uint64_t *ukey, uint64_t mu, uint64_t *off) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= n; i += gridDim.x * 256) {
        const uint64_t want = (uint64_t)i << 32;
        uint64_t lo = 0, hi = mu;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ukey[mid] < want) lo = mid + 1; else hi = mid; }
        off[i] = lo;
    }
}

const std::vector<uint32_t> &Engine::host_edges() {
    if (!edges_on_host) {
        UC_HIP(hipSetDevice(device));
        edges.resize(2 * n_edges_dev);
        if (n_edges_dev) UC_HIP(hipMemcpy(edges.data(), d_edges.p, 2 * n_edges_dev * 4, hipMemcpyDeviceToHost));
        edges_on_host = true;
    }
    return edges;
}

// ---- E7 on the device: the SAME greedy cover as uc_setcover.cpp (most unassigned nodes covered first, ties: smallest id), in parallel rounds ----
// The sequential rule picks the unassigned node u with the largest key (count, -id), count = 1 + unassigned neighbours.  A pick changes counts only
// within two hops THROUGH UNASSIGNED nodes (it assigns its unassigned neighbours v, which lowers the count of their unassigned neighbours w), and counts
// only ever fall.  So a node whose key is the maximum of its two-hop neighbourhood through unassigned nodes will be picked by the sequential rule with
// exactly its present count before anything near it changes: every such local maximum can be picked AT ONCE (no two of them share an unassigned
// neighbour: they would be within two hops of each other).  Rounds of (1) m1[v] = max key over the unassigned closed neighbourhood of v, (2) u is picked
// iff key(u) = max m1 over its unassigned closed neighbourhood, (3) picks take their unassigned neighbours, (4) the counts of the unassigned neighbours
// of everything newly assigned drop.  Identical assignment to the host cover (tests/test_gpu_parity.py, random graphs included); a wave per node.
constexpr uint32_t SC_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint64_t sc_key(uint32_t w, const uint32_t *assign, const uint32_t *cnt) {
    return assign[w] == SC_NONE ? ((uint64_t)cnt[w] << 32) | (uint64_t)(0xFFFFFFFFu - w) : 0ull;
}
__device__ __forceinline__ uint64_t sc_wave_max(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) { const uint64_t x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return v;
}
__global__ void __launch_bounds__(256) sc_init_kernel(uint32_t n, const uint64_t *off, uint32_t *assign, uint32_t *cnt, uint32_t *work) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        assign[i] = SC_NONE; cnt[i] = (uint32_t)(off[i + 1] - off[i]) + 1u; work[i] = i;
    }
}
// ctr: [0] nodes in `work`, [1] picks, [2] newly assigned, [3] nodes in the next work list
__global__ void __launch_bounds__(256) sc_m1_kernel(const uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                    const uint32_t *cnt, uint64_t *m1) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t v = work[i];
        uint64_t best = 0;
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) { const uint64_t k = sc_key(adj[e], assign, cnt); best = k > best ? k : best; }
        best = sc_wave_max(best);
        const uint64_t own = sc_key(v, assign, cnt);
        if (lane == 0) m1[v] = own > best ? own : best;
    }
}
__global__ void __launch_bounds__(256) sc_pick_kernel(uint32_t *ctr, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                      const uint32_t *cnt, const uint64_t *m1, uint32_t *picks) {
    const uint32_t nw = ctr[0], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nw; i += gridDim.x * 4) {
        const uint32_t u = work[i];
        uint64_t best = 0;
        for (uint64_t e = off[u] + lane; e < off[u + 1]; e += 64) {
            const uint32_t w = adj[e];
            const uint64_t k = assign[w] == SC_NONE ? m1[w] : 0ull;
            best = k > best ? k : best;
        }
        best = sc_wave_max(best);
        const uint64_t mine = m1[u];
        best = mine > best ? mine : best;
        if (lane == 0 && best == sc_key(u, assign, cnt)) picks[atomicAdd(&ctr[1], 1u)] = u;
    }
}
__global__ void __launch_bounds__(256) sc_apply_kernel(uint32_t *ctr, const uint32_t *picks, const uint64_t *off, const uint32_t *adj, uint32_t *assign, uint32_t *newly) {
    const uint32_t np = ctr[1], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < np; i += gridDim.x * 4) {
        const uint32_t u = picks[i];
        if (lane == 0) { assign[u] = u; newly[atomicAdd(&ctr[2], 1u)] = u; }
        for (uint64_t e = off[u] + lane; e < off[u + 1]; e += 64) {
            const uint32_t w = adj[e];
            if (assign[w] == SC_NONE) { assign[w] = u; newly[atomicAdd(&ctr[2], 1u)] = w; }     // no other pick of this round can reach w
        }
    }
}
__global__ void __launch_bounds__(256) sc_dec_kernel(const uint32_t *ctr, const uint32_t *newly, const uint64_t *off, const uint32_t *adj, const uint32_t *assign, uint32_t *cnt) {
    const uint32_t nn = ctr[2], lane = threadIdx.x & 63;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < nn; i += gridDim.x * 4) {
        const uint32_t v = newly[i];
        for (uint64_t e = off[v] + lane; e < off[v + 1]; e += 64) {
            const uint32_t w = adj[e];
            if (assign[w] == SC_NONE) atomicSub(&cnt[w], 1u);
        }
    }
}
__global__ void __launch_bounds__(256) sc_compact_kernel(uint32_t *ctr, const uint32_t *work, const uint32_t *assign, uint32_t *next) {
    const uint32_t nw = ctr[0];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nw; i += gridDim.x * 256) {
        const uint32_t v = work[i];
        if (assign[v] == SC_NONE) next[atomicAdd(&ctr[3], 1u)] = v;
    }
}
// the edges among the still-unassigned nodes of the work list (v < w once each): out == nullptr counts them, else appends them behind an atomic cursor
__global__ void __launch_bounds__(256) sc_induced_kernel(uint32_t left, const uint32_t *work, const uint64_t *off, const uint32_t *adj, const uint32_t *assign,
                                                         uint32_t *out, unsigned long long *cursor) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < left; i += gridDim.x * 256) {
        const uint32_t v = work[i];
        if (assign[v] != SC_NONE) continue;
        uint32_t c = 0;
        for (uint64_t k = off[v]; k < off[(size_t)v + 1]; k++) { const uint32_t w = adj[k]; c += (w > v && assign[w] == SC_NONE) ? 1u : 0u; }
        if (!c) continue;
        const unsigned long long base = atomicAdd(cursor, (unsigned long long)c);
        if (!out) continue;
        unsigned long long o = base;
        for (uint64_t k = off[v]; k < off[(size_t)v + 1]; k++) {
            const uint32_t w = adj[k];
            if (w > v && assign[w] == SC_NONE) { out[2 * o] = v; out[2 * o + 1] = w; o++; }
        }
    }
}
__global__ void sc_next_round_kernel(uint32_t *ctr) { ctr[0] = ctr[3]; ctr[1] = 0; ctr[2] = 0; ctr[3] = 0; }

void Engine::set_cover_own_edges(uint32_t n, uint32_t *assign) {
    if (p.cluster_mode != 0) {      // --cluster-mode 2: the same three sources, the greedy incremental rule (uc_greedy_inc.hip)
        if (edges_on_host) cluster_graph_device(p.cluster_mode, n, edges.data(), edges.size() / 2, assign);
        else if (n_edges_dev >= (1ull << 31)) { const std::vector<uint32_t> &h = host_edges(); cluster_graph(n, h.data(), h.size() / 2, h_len.data(), p.cluster_mode, assign); }
        else cluster_graph_dev_edges(n, d_edges.p, n_edges_dev, assign);
        return;
    }
    if (edges_on_host) { set_cover_device(n, edges.data(), edges.size() / 2, assign); return; }
    if (n_edges_dev >= (1ull << 31)) { const std::vector<uint32_t> &h = host_edges(); set_cover(n, h.data(), h.size() / 2, assign); return; }
    set_cover_graph(n, nullptr, d_edges.p, n_edges_dev, assign);
}

void Engine::set_cover_device(uint32_t n, const uint32_t *h_edges, uint64_t n_edges, uint32_t *assign) {
    if (n_edges >= (1ull << 31)) { set_cover(n, h_edges, n_edges, assign); return; }   // 32-bit scan positions below
    set_cover_graph(n, h_edges, nullptr, n_edges, assign);
}

GreedyIncScratch &Engine::greedy_inc_scratch() { return scratch_of(*this).gi; }
ReassignScratch &Engine::reassign_scratch() { return scratch_of(*this).ra; }

// the graph (CSR, both directions, duplicates and self loops removed) on the device from a host or a device edge list (n_edges > 0): the step
// both clustering rules start from.  The arrays live in the engine's scratch and stay valid until the next graph build
DevGraph Engine::build_cluster_graph(uint32_t n, const uint32_t *h_edges, const uint32_t *dev_edges, uint64_t n_edges) {
    Timer t_graph;
    AlignScratch &A = scratch_of(*this);
    const uint64_t m = 2 * n_edges;
    DevBuf<uint32_t> &d_e = A.sc_e, &flag = A.sc_flag, &pos = A.sc_pos, &d_adj = A.sc_dadj, &bad = A.sc_bad;
    DevBuf<uint64_t> &key = A.sc_key, &key2 = A.sc_key2, &ukey = A.sc_ukey, &d_off = A.sc_doff;
    DevBuf<char> &tmp = A.sc_tmp;
    key.reserve(m); key2.reserve(m); flag.reserve(m); pos.reserve(m); bad.reserve(1); d_off.reserve((size_t)n + 1);
    const uint32_t *e_in = dev_edges;
    if (!e_in) {
        d_e.reserve(m);
        UC_HIP(hipMemcpyAsync(d_e.p, h_edges, m * 4, hipMemcpyHostToDevice, stream));
        e_in = d_e.p;
    }
    UC_HIP(hipMemsetAsync(bad.p, 0, 4, stream));
    hipLaunchKernelGGL(edge_key_kernel, grid_for(n_edges), dim3(256), 0, stream, n_edges, e_in, n, key.p, bad.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, key.p, key2.p, (size_t)m, 0u, 64u, stream); });
    hipLaunchKernelGGL(edge_uniq_kernel, grid_for(m), dim3(256), 0, stream, m, key2.p, flag.p);
    const uint32_t mu = compact(*this, tmp, flag.p, pos.p, (uint32_t)m);
    uint32_t hbad = 0;
    UC_HIP(hipMemcpy(&hbad, bad.p, 4, hipMemcpyDeviceToHost));
    if (hbad) fail(UC_ERR_ARGS, "set cover: %u edges with an endpoint out of range", hbad);
    ukey.reserve(std::max<uint32_t>(mu, 1)); d_adj.reserve(std::max<uint32_t>(mu, 1));
    hipLaunchKernelGGL(edge_adj_kernel, grid_for(m), dim3(256), 0, stream, m, key2.p, flag.p, pos.p, ukey.p, d_adj.p);
    hipLaunchKernelGGL(edge_off_kernel, grid_for((uint64_t)n + 1), dim3(256), 0, stream, n, ukey.p, (uint64_t)mu, d_off.p);
    UC_HIP(hipGetLastError());
    if (getenv("UC_TIMING")) { UC_HIP(hipStreamSynchronize(stream)); fprintf(stderr, "set_cover_device: graph on the GPU %.2f ms\n", t_graph.seconds() * 1e3); }
    return DevGraph{d_off.p, d_adj.p, mu};
}

// the subgraph the still-undecided nodes (mark[v] == SC_NONE) of the work list induce, for a host finish: their ids ascending (`back`) and the edges
// among them in that numbering (`e2`, each once), gathered on the device (count pass, then an append pass; the order of the edge list does not matter)
void Engine::induced_subgraph(const DevGraph &G, uint32_t left, const uint32_t *d_work, const uint32_t *d_mark, std::vector<uint32_t> &back, std::vector<uint32_t> &e2) {
    DevBuf<unsigned long long> ecnt;
    ecnt.reserve(1);
    UC_HIP(hipMemsetAsync(ecnt.p, 0, 8, stream));
    hipLaunchKernelGGL(sc_induced_kernel, grid_for(left), dim3(256), 0, stream, left, d_work, G.off, G.adj, d_mark, (uint32_t *)nullptr, ecnt.p);
    unsigned long long ne2 = 0;
    UC_HIP(hipMemcpyAsync(&ne2, ecnt.p, 8, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    DevBuf<uint32_t> de2;
    de2.reserve(2 * std::max<unsigned long long>(ne2, 1));
    UC_HIP(hipMemsetAsync(ecnt.p, 0, 8, stream));
    if (ne2) hipLaunchKernelGGL(sc_induced_kernel, grid_for(left), dim3(256), 0, stream, left, d_work, G.off, G.adj, d_mark, de2.p, ecnt.p);
    back.resize(left); e2.resize(2 * (size_t)ne2);
    UC_HIP(hipMemcpyAsync(back.data(), d_work, (size_t)left * 4, hipMemcpyDeviceToHost, stream));
    if (ne2) UC_HIP(hipMemcpyAsync(e2.data(), de2.p, 2 * (size_t)ne2 * 4, hipMemcpyDeviceToHost, stream));
    UC_HIP(hipStreamSynchronize(stream));
    UC_HIP(hipGetLastError());
    std::sort(back.begin(), back.end());                                   // ids keep their order: so do the ties
    auto sub = [&](uint32_t v) { return (uint32_t)(std::lower_bound(back.begin(), back.end(), v) - back.begin()); };
    for (uint32_t &x : e2) x = sub(x);
}

// the graph on the device (build_cluster_graph), then the greedy cover on the device as well (parallel rounds of local maxima: the host cover's
// assignment, uc_setcover.cpp, exactly)
void Engine::set_cover_graph(uint32_t n, const uint32_t *h_edges, const uint32_t *dev_edges, uint64_t n_edges, uint32_t *assign) {
    PressureScope ps(*this, 1);
    UC_HIP(hipSetDevice(device));
    AlignScratch &A = scratch_of(*this);
    if (n_edges) {
        const DevGraph G = build_cluster_graph(n, h_edges, dev_edges, n_edges);
        const uint64_t *d_off = G.off;
        const uint32_t *d_adj = G.adj;
        const bool timing = getenv("UC_TIMING") != nullptr;
        // the greedy cover itself, on the device too (parallel rounds, see above): neither the adjacency (2 x edges x 4 bytes) nor the serial
        // host sweep — rank 0's Amdahl term of an N-GPU pass — is left; only the assignment comes back
        Timer t_greedy;
        DevBuf<uint32_t> &d_assign = A.sc_assign, &d_cnt = A.sc_cnt, &w0 = A.sc_work, &w1 = A.sc_work2, &picks = A.sc_picks, &newly = A.sc_newly, &ctr = A.sc_ctr;
        DevBuf<uint64_t> &m1 = A.sc_m1;
        d_assign.reserve(n); d_cnt.reserve(n); w0.reserve(n); w1.reserve(n); picks.reserve(n); newly.reserve(n); ctr.reserve(4); m1.reserve(n);
        hipLaunchKernelGGL(sc_init_kernel, grid_for(n), dim3(256), 0, stream, n, d_off, d_assign.p, d_cnt.p, w0.p);
        const uint32_t h_ctr[4] = {n, 0, 0, 0};
        UC_HIP(hipMemcpyAsync(ctr.p, h_ctr, 16, hipMemcpyHostToDevice, stream));
        uint32_t left = n, rounds = 0;
        bool host_tail = false;
        uint32_t *cur = w0.p, *nxt = w1.p;
        while (left) {
            const dim3 gw((uint32_t)std::min<uint64_t>(((uint64_t)left + 3) / 4, 1u << 16));
            hipLaunchKernelGGL(sc_m1_kernel, gw, dim3(256), 0, stream, (const uint32_t *)ctr.p, (const uint32_t *)cur, d_off, d_adj, d_assign.p, d_cnt.p, m1.p);
            hipLaunchKernelGGL(sc_pick_kernel, gw, dim3(256), 0, stream, ctr.p, (const uint32_t *)cur, d_off, d_adj, d_assign.p, d_cnt.p, m1.p, picks.p);
            hipLaunchKernelGGL(sc_apply_kernel, gw, dim3(256), 0, stream, ctr.p, (const uint32_t *)picks.p, d_off, d_adj, d_assign.p, newly.p);
            hipLaunchKernelGGL(sc_dec_kernel, gw, dim3(256), 0, stream, (const uint32_t *)ctr.p, (const uint32_t *)newly.p, d_off, d_adj, d_assign.p, d_cnt.p);
            hipLaunchKernelGGL(sc_compact_kernel, grid_for(left), dim3(256), 0, stream, ctr.p, (const uint32_t *)cur, d_assign.p, nxt);
            uint32_t h[4];
            UC_HIP(hipMemcpyAsync(h, ctr.p, 16, hipMemcpyDeviceToHost, stream));
            hipLaunchKernelGGL(sc_next_round_kernel, dim3(1), dim3(1), 0, stream, ctr.p);
            UC_HIP(hipStreamSynchronize(stream));
            if (h[1] == 0) fail(UC_ERR_GENERIC, "set cover: a round picked nothing with %u nodes left", left);    // cannot happen: the global maximum is always a local one
            left = h[3];
            std::swap(cur, nxt);
            rounds++;
            // Family graphs finish in a handful of rounds; a chain-like remainder (equal counts, ids ascending along a path) gives ONE pick per round -
            // n / 3 rounds of six launches and a host synchronisation each.  When the rounds stop paying, the rest - the greedy cover of
            // the subgraph the unassigned nodes induce, which is all the sequential rule still looks at - is finished by the host cover.
            if (left && rounds >= 32 && h[1] < 64) { host_tail = true; break; }
        }
        UC_HIP(hipMemcpyAsync(assign, d_assign.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        UC_HIP(hipStreamSynchronize(stream));
        UC_HIP(hipGetLastError());
        if (host_tail) {
            // r06: only the subgraph the `left` unassigned nodes induce goes to the host - their ids and the edges among them - not the whole
            // adjacency (4 B x 10^9 entries over PCIe plus an O(n) scan at nominal sizes, however few nodes were left)
            std::vector<uint32_t> back, e2;
            induced_subgraph(G, left, cur, d_assign.p, back, e2);
            std::vector<uint32_t> a2(back.size());
            set_cover((uint32_t)back.size(), e2.data(), e2.size() / 2, a2.data());
            for (size_t i = 0; i < back.size(); i++) assign[back[i]] = back[a2[i]];
        }
        if (timing) fprintf(stderr, "set_cover_device: greedy cover on the GPU %.2f ms in %u rounds%s\n", t_greedy.seconds() * 1e3, rounds,
                            host_tail ? ", the chain-like rest on the host" : "");
        return;
    }
    for (uint32_t i = 0; i < n; i++) assign[i] = i;      // no edges: every node is its own representative
}

void preload_align_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)plan_key_kernel); }
}  // namespace uc
