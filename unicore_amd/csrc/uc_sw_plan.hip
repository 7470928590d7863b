// uc_sw_plan.hip - the planner and launcher of one gapped pass, and the class tables it plans with.
// A pass is a pair list: the planner sorts it by (length class, query, target length), cuts it into workgroup tasks, gathers the kernel inputs
// (build_plan), launches one kernel per populated class (launch_plan) and re-runs on the int32 kernel what the packed classes could not finish
// (run_plan).  The tables live here once, on the host (h_tab) and in constant memory (c_tab), together with EVERY kernel that reads c_tab - a
// __constant__ symbol exists once per code object - which is why the two traceback kernels that look up a class geometry (tb_size_kernel,
// tb_walk_kernel) are in this file, behind launch_tb_size / launch_tb_walk, and not with the rest of the traceback in uc_traceback.hip
// (planner, classes; 4.2b: the walk).
#include <mutex>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

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

namespace {

__device__ __constant__ ClassTable c_tab[4];

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

struct MaxU32 {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

}  // namespace

// which table a known-score pass of the packed path plans with: sparse (table 3) when the plan holds fewer than 2.5 pairs per query of the call
// (UC_SW_SPARSE=0: always table 1, for A/B runs; results do not depend on the table - every class computes the exact DP)
int pk_known_tab(uint32_t n_pairs, uint32_t n_queries) {
    static const bool on = !(getenv("UC_SW_SPARSE") && atoi(getenv("UC_SW_SPARSE")) == 0);
    return on && (double)n_pairs < 2.5 * (double)n_queries ? 3 : 1;
}

// below how many slots per task (mean over a class of a pass) the packed kernel serves several tasks per workgroup: a host-side choice like the one
// above, results do not depend on it (UC_SW_TASK_QUERIES=1: never, for A/B runs; UC_SW_TASK_SLOTS: the threshold, for sweeps)
static double sw_task_queries_slots() {
    static const double v = [] {
        if (getenv("UC_SW_TASK_QUERIES") && atoi(getenv("UC_SW_TASK_QUERIES")) == 1) return 0.0;
        return getenv("UC_SW_TASK_SLOTS") ? atof(getenv("UC_SW_TASK_SLOTS")) : 24.0;
    }();
    return v;
}

// running maximum (inclusive) of a u32 array
void max_scan_u32(Engine &E, DevBuf<char> &tmp, const uint32_t *in, uint32_t *out, uint32_t n) {
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, (size_t)n, MaxU32(), E.stream); });
}

// a 0/1 flag array -> its exclusive scan in pos (where each flagged entry goes) -> the number of flagged entries (one host synchronisation)
uint32_t compact(Engine &E, DevBuf<char> &tmp, const uint32_t *flag, uint32_t *pos, uint32_t n) {
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, flag, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), E.stream); });
    if (!n) return 0;
    uint32_t a = 0, b = 0;
    UC_HIP(hipMemcpyAsync(&a, pos + (n - 1), 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipMemcpyAsync(&b, flag + (n - 1), 4, hipMemcpyDeviceToHost, E.stream));
    UC_HIP(hipStreamSynchronize(E.stream));
    return a + b;
}

// the packed classes form a prefix of a plan's sorted pair list, and their tasks a prefix of its task list
PackedPrefix packed_prefix(const SwPlan &P) {
    const ClassTable &tab = h_tab[P.tab];
    int c = 0;
    while (c < tab.n && tab.pk[c]) c++;
    return {P.pair_base[c], P.task_base[c]};
}

void build_plan(Engine &E, SwPlan &P, DevBuf<char> &tmp, uint32_t n, const uint32_t *q, const uint32_t *t,
                const int32_t *qe, const int32_t *te, int tab, const int32_t *qs, const int32_t *ts, const int32_t *aux, bool lpt) {
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

__global__ void __launch_bounds__(256) fill2_kernel(uint32_t n, int32_t v, int32_t *a, int32_t *b) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { a[i] = v; b[i] = v; }
}

// one launch per populated class; outputs are in the plan's sorted order.  Returns the number of launches.
// [t0, t1): only the tasks of that range of the plan's task list (the byte-budgeted batches of the traceback plan); skip_long: not the long-query launch
// sec (MODE 4 / 6): where the packed known-score classes put their second answer, plan order; every other pair of the plan keeps -2 there
uint64_t launch_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
                     const uint32_t *tb, bool only_long, uint32_t t0, uint32_t t1, bool skip_long, const SwSecond *sec) {
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
        if (tab.pk[c]) {
            // short lists (few slots per task): the workgroups of the class serve several tasks each (sw_pk_kernel, K > 1)
            const double slots = 0.5 * (double)(P.pair_base[c + 1] - P.pair_base[c]) / (double)(P.task_base[c + 1] - P.task_base[c]);
            const int k = launch_sw_pk_class(tab.G[c], tab.R[c], mode, ac, nt, st, slots < sw_task_queries_slots() ? 2 : 1, tab.tcap[c]);
            if (k > 1) { E.sw_task_queries[0]++; E.sw_task_queries[1] += nt; }
        } else launch_sw_class(tab.G[c], tab.R[c], imode, ac, nt, st);
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

// ovf_only: re-run immediately only what saturated; ambiguous end rows (qe == -2) are left for the caller
void run_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
              DevBuf<char> &tmp, bool ovf_only, const SwSecond *sec) {
    if (!P.n) return;
    E.timed_ms_begin();
    uint64_t launches = launch_plan(E, P, mode, os, oqe, ote, work, nullptr, false, 0, 0xFFFFFFFFu, false, sec);
    double ms = E.timed_ms_end();
    const uint32_t n_pk = packed_prefix(P).pairs;
    if (n_pk) {
        RerunScratch &B = scratch_of(E).rr;
        SwPlan &P2 = B.P;
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

// the class a plan of table `tab` puts each pair in (class_of, as plan_key_kernel keys it; c_tab[tab].n = long-query kernel)
__global__ void __launch_bounds__(256) pass_class_kernel(uint32_t n, const uint32_t *q, const uint32_t *len, int tab, int32_t *out) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = class_of((int)len[q[i]], tab);
}
void pass_classes(Engine &E, uint32_t n, const uint32_t *q, int tab, int32_t *out) {
    hipLaunchKernelGGL(pass_class_kernel, grid_for(n), dim3(256), 0, E.stream, n, q, E.ddb.len, tab, out);
}

void launch_tb_size(Engine &E, uint32_t n_pk, int band, unsigned long long *size) {
    const SwPlan &P3 = scratch_of(E).tb.P3;
    hipLaunchKernelGGL(tb_size_kernel, grid_for(n_pk), dim3(256), 0, E.stream, n_pk, P3.key2.p, P3.segstart.p, P3.ste.p,
                       P3.sts.p, P3.sqs.p, P3.sqe.p, band, 1, size);
}

// emit / plain: the walk kernel's EMIT and PLAIN; base: where the slices of an emitting walk (EMIT = 2) begin in the engine's run buffer
void launch_tb_walk(Engine &E, int emit, int plain, uint32_t p0, uint32_t p1, int band, const uint8_t *tbm, const unsigned long long *tboff, uint64_t base) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb.P3;
    hipStream_t s = E.stream;
    const dim3 grid = grid_for(p1 - p0);
#define UC_TB_WALK(EMIT, PLAIN)                                                                                                                  \
    hipLaunchKernelGGL((tb_walk_kernel<EMIT, PLAIN>), grid, dim3(256), 0, s, p0, p1, E.ddb, P3.key2.p, P3.st.p, P3.sqs.p, P3.sqe.p, P3.sts.p, P3.ste.p,  \
                       P3.saux.p, E.p.gap_open, E.p.gap_ext, band, 1, tbm, tboff, A.tb.pack3.p, A.tb.id3.p, A.tb.gaps3.p, A.tb.bt_cnt3.p, A.tb.bt_off3.p,              \
                       E.d_bt_runs.p + (base), (unsigned long long)(base), A.tb.bt_pos3.p, A.tb.bt_plain3.p, A.tb.bt_err.p)
    switch (2 * emit + plain) {
    case 0: UC_TB_WALK(0, 0); break;
    case 2: UC_TB_WALK(1, 0); break;
    case 3: UC_TB_WALK(1, 1); break;
    case 4: UC_TB_WALK(2, 0); break;
    case 5: UC_TB_WALK(2, 1); break;
    default: fail(UC_ERR_GENERIC, "the stored-matrix pass runs for backtraces only");
    }
#undef UC_TB_WALK
}

void preload_sw_plan_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)plan_key_kernel); }
}  // namespace uc
