// uc_traceback.hip - traceback statistics and backtraces of the gapped stage.
// For the pairs that passed the coverage gate (--min-seq-id, search output, -a): alignment length, identities and gaps of the traceback on the box,
// either from stored H bytes of the packed kernel (MODE 7) and a walk over them, in segments and byte-budgeted matrix batches (TbBudget), or
// carried through the DP by the int32 kernel (MODE 3); with -a the same walk emits the run-length path, and the pairs the packed kernel does
// not serve take a stored int32 matrix.  Mutual hits share one traceback where the path cannot differ.  The walk kernel itself and the kernel that
// sizes the byte matrices read the class table and live beside it in uc_sw_plan.hip (launch_tb_walk, launch_tb_size).
// (stands for Foldseek's backtrace / seq-id handling of structurealign)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

// scratch for the traceback-byte matrices of one batch (MODE 7): up to 64 GiB (r06; 144 GiB until r05), never more than 55 % of what
// is free right now (plus what the scratch buffer already holds); UC_TB_BUDGET_MB overrides (tests).  Why 64: taking device memory costs 25-40 ms per GiB
// whenever the box's memory is not warm for this process (one 108 GiB buffer: 4.2 s of a 14 s call at 500 proteomes in the first process on a fresh box,
// profiles/r06/c4_p500_alloc.txt), while the batches a smaller buffer adds cost a launch tail each (r05: halving the batches of nominal configs[3] cost 3 %
// of the pass)
// The plan of a MODE 7 call costs ~110 B per pair beside the matrices: the flagged list is worked off in segments of 32 M pairs (nominal
// configs[3]: 170 M flagged pairs per 256 M-pair batch of the stage), each planned and cut into matrix batches on its own; a segment
// still holds ~1.5 TB of matrices, i.e. dozens of one-class batches.  (Tests: a forced matrix budget also forces 1000-pair segments.)
TbBudget::TbBudget() {
    if (const char *e = getenv("UC_TB_BUDGET_MB")) forced = std::max<unsigned long long>(1, strtoull(e, nullptr, 10)) << 20;
}
uint32_t TbBudget::segment_pairs() const { return forced ? 1000u : (32u << 20); }
unsigned long long TbBudget::batch_bytes(unsigned long long total, size_t held) const {
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

namespace {

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
// seq-id stage (only with --min-seq-id > 0): pairs that passed the coverage gate get their traceback statistics
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

}  // namespace

// memory pressure inside the gapped stage: the traceback-byte buffer (up to 144 GiB, kept between calls because fresh memory is slow) is dead weight
// outside the batch loop of a MODE 7 call - the engine's out-of-memory handler gives it back before it gives up
bool release_tb_matrices(AlignScratch *p) {
    if (!p || p->tb.tbm_live || !p->tb.tbm.cap) return false;
    p->tb.tbm.release();
    return true;
}

// the walk over H bytes needs neighbouring cells within 127 of each other: largest substitution score + gap open
// (uc_sw_plan.hip tb_walk_kernel); anything else takes the int32 pass
bool tb_bytes_ok(const Params &p) {
    int m3 = -128, ma = -128, n3 = 127, na = 127;
    for (int k = 0; k < 21 * 21; k++) {
        m3 = std::max<int>(m3, p.S3[k]); ma = std::max<int>(ma, p.SA[k]);
        n3 = std::min<int>(n3, p.S3[k]); na = std::min<int>(na, p.SA[k]);
    }
    return p.gap_open >= p.gap_ext && p.gap_ext >= 0 && m3 + ma + p.gap_open <= 127 && n3 + na >= -127;
}

// MODE 3 weights (diagonal, identity, open, extension), one pass per statistic: columns of the alignment, identities, gaps
constexpr uint32_t TB_LEN[4] = {1u, 0u, 1u, 1u}, TB_IDENT[4] = {0u, 1u, 0u, 0u}, TB_GAPS[4] = {0u, 0u, 1u, 0u};

// the walk over the matrices of pairs [p0, p1) of the plan tb.P3 that are resident now.  Without -a: the statistics walk.  With -a (E.emit_bt):
// count (statistics + runs per pair), scan, make room in the engine's run buffer for exactly that many, write.
static void tb_walk(Engine &E, int plain, uint32_t p0, uint32_t p1, int band, const uint8_t *tbm, const unsigned long long *tboff) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    if (p1 <= p0) return;
    if (!E.emit_bt) { launch_tb_walk(E, 0, plain, p0, p1, band, tbm, tboff, 0); return; }
    launch_tb_walk(E, 1, plain, p0, p1, band, tbm, tboff, 0);
    const size_t k = p1 - p0;
    rocprim_call(A.tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, A.tb.bt_cnt3.p + p0, A.tb.bt_off3.p + p0, 0u, k, rocprim::plus<uint32_t>(), s); });
    uint32_t lo = 0, lc = 0;
    UC_HIP(hipMemcpyAsync(&lo, A.tb.bt_off3.p + (p1 - 1), 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipMemcpyAsync(&lc, A.tb.bt_cnt3.p + (p1 - 1), 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    const uint64_t total = (uint64_t)lo + lc;
    if (total >= (1ull << 31)) fail(UC_ERR_GENERIC, "backtraces: %llu runs in one matrix batch", (unsigned long long)total);
    if (!total) return;
    E.d_bt_runs.grow_preserve(E.bt_used + total, E.bt_used, s);
    launch_tb_walk(E, 2, plain, p0, p1, band, tbm, tboff, E.bt_used);
    E.bt_used += total;
}

// -a, the pairs [p0, p1) of the plan tb.P3 that the packed kernel does not serve: plain int32 H matrices (tb_plain_dp_kernel) in batches of the same
// budget as the byte matrices, in pair order; a single pair always runs.  Returns the launches.
static uint64_t tb_run_plain(Engine &E, uint32_t p0, uint32_t p1, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb.P3;
    hipStream_t s = E.stream;
    if (p1 <= p0) return 0;
    const size_t k = p1 - p0;
    A.tb.tbsize.reserve((size_t)P3.n + 1); A.tb.tboff.reserve((size_t)P3.n + 1);
    hipLaunchKernelGGL(tb_plain_size_kernel, grid_for(k), dim3(256), 0, s, p0, p1, P3.sqs.p, P3.sqe.p, P3.sts.p, P3.ste.p, A.tb.tbsize.p);
    std::vector<unsigned long long> h_size(k);
    UC_HIP(hipMemcpyAsync(h_size.data(), A.tb.tbsize.p + p0, k * 8, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    std::vector<unsigned long long> h_off(k + 1, 0);
    for (size_t i = 0; i < k; i++) h_off[i + 1] = h_off[i] + h_size[i];
    UC_HIP(hipMemcpyAsync(A.tb.tboff.p + p0, h_off.data(), k * 8, hipMemcpyHostToDevice, s));
    const unsigned long long batch_bytes = budget.batch_bytes(h_off[k], A.tb.tbm.cap);
    A.tb.tbm_live = true;
    struct Live { bool &f; ~Live() { f = false; } } live{A.tb.tbm_live};
    std::vector<std::pair<size_t, size_t>> batches;
    unsigned long long max_bytes = 0;
    for (size_t a = 0; a < k;) {
        size_t b = a + 1;
        while (b < k && h_off[b + 1] - h_off[a] <= batch_bytes) b++;
        batches.emplace_back(a, b);
        max_bytes = std::max(max_bytes, h_off[b] - h_off[a]);
        a = b;
    }
    A.tb.tbm.reserve_exact(max_bytes + 64);
    uint64_t launches = 0;
    double ms = 0;
    for (const auto &bt : batches) {
        const uint32_t a = p0 + (uint32_t)bt.first, b = p0 + (uint32_t)bt.second;
        uint8_t *base = A.tb.tbm.p - h_off[bt.first];                 // (a pair's offset counts from the first pair of the range)
        E.timed_ms_begin();
        hipLaunchKernelGGL(tb_plain_dp_kernel, dim3(std::min<uint32_t>(b - a, 4096u)), dim3(256), 0, s, a, b, E.ddb, P3.key2.p, P3.st.p, P3.sqs.p, P3.sqe.p,
                           P3.sts.p, P3.ste.p, E.p.gap_open, E.p.gap_ext, base, A.tb.tboff.p);
        tb_walk(E, 1, a, b, 0, base, A.tb.tboff.p);
        ms += E.timed_ms_end();
        launches += 3;
    }
    E.stats.sw_kernel_ms += ms;
    if (getenv("UC_TIMING")) fprintf(stderr, "unicore-cluster[timing]: sw pass stored int32 matrices: %zu pairs, %.2f ms, %llu matrix bytes, %zu batch(es)\n",
                                     k, ms, h_off[k], batches.size());
    return launches;
}

// packed MODE 7 for the plan tb.P3 (built in pair order): H bytes of the box's diagonal band (tb_band_of) + walk kernel; queries beyond the
// systolic classes take int32 MODE 3.  Returns the launches.
//
// r05, pk: ONE plan for all flagged pairs of the call, and the byte matrices are produced in batches cut ALONG that plan - a batch is
// a range of its class-sorted task list that fits the matrix budget, i.e. thousands of tasks of one or two length classes per
// launch.  (r04 cut the flagged LIST into batches and planned each: every batch then ran all 28 class kernels with a handful of
// tasks each - 442 batches at nominal configs[3], MODE 7 at 1.5 T cells/s against 5 T for the other passes:
// profiles/r05/sw_pass_timing_*.txt.)
static uint64_t tb_run_bytes(Engine &E, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    SwPlan &P3 = A.tb.P3;
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
        launches += launch_plan(E, P3, 7, A.tb.pack3.p, nullptr, nullptr, A.work, TB_LEN, /*only_long=*/true);
        launches += launch_plan(E, P3, 3, A.tb.id3.p, nullptr, nullptr, A.work, TB_IDENT, /*only_long=*/true);
        if (E.p.want_tb) launches += launch_plan(E, P3, 3, A.tb.gaps3.p, nullptr, nullptr, A.work, TB_GAPS, /*only_long=*/true);
        tb_ms += E.timed_ms_end();
    }
    if (n_pk3) {
        DevBuf<unsigned long long> &tbsize = A.tb.tbsize, &tboff = A.tb.tboff, &toff = A.tb.toff;
        DevBuf<uint8_t> &tbm = A.tb.tbm;
        tbsize.reserve((size_t)n_pk3 + 1); tboff.reserve((size_t)n_pk3 + 1);
        launch_tb_size(E, n_pk3, band, tbsize.p);
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
        A.tb.tbm_live = true;
        struct Live { bool &f; ~Live() { f = false; } } live{A.tb.tbm_live};
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
            launches += launch_plan(E, P3, 7, A.tb.pack3.p, nullptr, nullptr, A.work, nullptr, false, t0, t1, /*skip_long=*/true);
            tb_walk(E, 0, p0, p1, band, tbm.p - base, tboff.p);
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
// band in tb.tmiss.
void tb_batch(Engine &E, const AlignBatch &B, const uint32_t *flag, bool pk, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    const uint32_t nt = compact(E, A.tmp, flag, A.tb.tpos.p, n2);
    if (!nt) return;
    A.tb.q3.reserve(nt); A.tb.t3.reserve(nt); A.tb.src3.reserve(nt); A.tb.qs3.reserve(nt); A.tb.qe3.reserve(nt); A.tb.ts3.reserve(nt); A.tb.te3.reserve(nt);
    A.tb.pack3.reserve(nt); A.tb.id3.reserve(nt); A.tb.gaps3.reserve(nt); A.tb.sc3.reserve(nt);
    hipLaunchKernelGGL(tb_gather_kernel, grid_for(n2), dim3(256), 0, s, n2, flag, A.tb.tpos.p, A.start.iota2.p, A.gate.link.p, B.Lidx, A.gate.q2.p,
                       A.gate.t2.p, B.alns_b, A.tb.q3.p, A.tb.t3.p, A.tb.qs3.p, A.tb.qe3.p, A.tb.ts3.p, A.tb.te3.p, A.tb.src3.p, A.tb.sc3.p);
    SwPlan &P3 = A.tb.P3;
    uint64_t launches = 0;
    int passes = 1;
    if (E.emit_bt) {
        A.tb.bt_cnt3.reserve(nt); A.tb.bt_off3.reserve(nt); A.tb.bt_plain3.reserve(nt); A.tb.bt_pos3.reserve(nt); A.tb.bt_err.reserve(1);
        UC_HIP(hipMemsetAsync(A.tb.bt_cnt3.p, 0, (size_t)nt * 4, s));
        UC_HIP(hipMemsetAsync(A.tb.bt_err.p, 0, 4, s));
    }
    if (!pk && E.emit_bt) {   // -a: MODE 3 has no path to give; every pair takes the stored int32 matrix and the walk
        build_plan(E, P3, A.tmp, nt, A.tb.q3.p, A.tb.t3.p, A.tb.qe3.p, A.tb.te3.p, 1, A.tb.qs3.p, A.tb.ts3.p, A.tb.sc3.p, /*lpt=*/false);
        launches = tb_run_plain(E, 0, P3.n, budget);
    } else if (!pk) {
        build_plan(E, P3, A.tmp, nt, A.tb.q3.p, A.tb.t3.p, A.tb.qe3.p, A.tb.te3.p, 2, A.tb.qs3.p, A.tb.ts3.p);
        E.timed_ms_begin();
        launches = launch_plan(E, P3, 3, A.tb.pack3.p, nullptr, nullptr, A.work, TB_LEN);
        launches += launch_plan(E, P3, 3, A.tb.id3.p, nullptr, nullptr, A.work, TB_IDENT);
        passes = 2;
        if (E.p.want_tb) {   // third statistic of the same traceback: number of gaps (BLAST-tab "gapopen")
            launches += launch_plan(E, P3, 3, A.tb.gaps3.p, nullptr, nullptr, A.work, TB_GAPS);
            passes = 3;
        }
        E.stats.sw_kernel_ms += E.timed_ms_end();
    } else {
        build_plan(E, P3, A.tmp, nt, A.tb.q3.p, A.tb.t3.p, A.tb.qe3.p, A.tb.te3.p, 1, A.tb.qs3.p, A.tb.ts3.p, A.tb.sc3.p, /*lpt=*/false);
        launches = tb_run_bytes(E, band, budget);
    }
    E.stats.sw_kernel_launches += launches;
    E.stats.sw_algorithmic_bytes += passes * P3.alg_bytes;
    E.stats.cells_run += passes * P3.cells;
    E.stats.n_sw_runs += (uint64_t)passes * P3.n;
    hipLaunchKernelGGL(tb_apply_kernel, grid_for(nt), dim3(256), 0, s, nt, P3.idx.p, A.tb.src3.p, A.tb.pack3.p, A.tb.id3.p,
                       E.p.want_tb ? A.tb.gaps3.p : (const int32_t *)nullptr, A.start.iota2.p, A.gate.link.p, B.Lidx, E.p.min_seq_id, B.alns_b,
                       A.gate.eflag.p, A.tb.ttie.p, (pk && band > 0) ? A.tb.tmiss.p : (uint32_t *)nullptr);
    if (E.emit_bt) {
        if (!B.bt_pos_b) fail(UC_ERR_GENERIC, "backtraces: the batch has no place for them");
        hipLaunchKernelGGL(bt_apply_kernel, grid_for(nt), dim3(256), 0, s, nt, P3.idx.p, A.tb.src3.p, A.tb.bt_cnt3.p, A.tb.bt_pos3.p, A.tb.bt_plain3.p,
                           A.start.iota2.p, A.gate.link.p, B.Lidx, B.bt_pos_b, B.bt_n_b);
        uint32_t err = 0;
        UC_HIP(hipMemcpyAsync(&err, A.tb.bt_err.p, 4, hipMemcpyDeviceToHost, s));
        UC_HIP(hipStreamSynchronize(s));
        if (err) fail(UC_ERR_GENERIC, "backtraces: a path did not fit the slice its own count had sized");
    }
}

// packed MODE 7 for the flagged pairs, in segments of budget.segment_pairs() pairs (TbBudget)
static void tb_segments(Engine &E, const AlignBatch &B, const uint32_t *flag, int band, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    const uint32_t n2 = B.n2, seg = budget.segment_pairs();
    const uint32_t nlo = compact(E, A.tmp, flag, A.tb.tcpos.p, n2);
    if (nlo <= seg) { if (nlo) tb_batch(E, B, flag, true, band, budget); return; }
    for (uint32_t lo = 0; lo < nlo; lo += seg) {
        hipLaunchKernelGGL(tb_chunk_kernel, grid_for(n2), dim3(256), 0, E.stream, n2, flag, A.tb.tcpos.p, lo, std::min<uint32_t>(nlo, lo + seg), A.tb.tchunk.p);
        tb_batch(E, B, A.tb.tchunk.p, true, band, budget);
    }
}

// the traceback statistics of the flagged gate passers, on the packed kernel where its range and the byte walk allow it
void run_tb(Engine &E, const AlignBatch &B, const uint32_t *flag, int band_w, const TbBudget &budget) {
    AlignScratch &A = scratch_of(E);
    const uint32_t n2 = B.n2;
    if (!E.p.sw_pk || !tb_bytes_ok(E.p)) { tb_batch(E, B, flag, false, 0, budget); return; }
    A.tb.tlo.reserve(n2); A.tb.thi.reserve(n2); A.tb.tmiss.reserve(n2); A.tb.tchunk.reserve(n2); A.tb.tcpos.reserve(n2);
    hipLaunchKernelGGL(tb_split_kernel, grid_for(n2), dim3(256), 0, E.stream, n2, flag, A.gate.link.p, B.Lidx, B.alns_b, SW_PK_OVF_HOST, A.tb.tlo.p, A.tb.thi.p);
    tb_batch(E, B, A.tb.thi.p, false, 0, budget);                       // scores beyond the packed range: int32 MODE 3
    if (band_w > 0) UC_HIP(hipMemsetAsync(A.tb.tmiss.p, 0, (size_t)n2 * 4, E.stream));
    tb_segments(E, B, A.tb.tlo.p, band_w, budget);
    if (band_w > 0) tb_segments(E, B, A.tb.tmiss.p, 0, budget);          // tracebacks that left their band: the whole box
}

// slices of records (pos, n) cut from the host copy `hruns` of the run buffer from element `base` on; bit 31 of n exchanges I and D
void bt_assemble(size_t n, const unsigned long long *pos, const uint32_t *cnt, const uc_aln *alns /* null: every record counts */,
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

// sequence-identity gate / BLAST-tab statistics: (alignment length, identities[, gaps]) of the traceback on
// the box, for the pairs that passed the coverage gate
void traceback_stats(Engine &E, const AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    // the plans of the passes behind us are dead (their results have been scattered): at sizes where the matrix budget is what is left of the
    // device (nominal configs[3]: ~35 GB of plan arrays beside ~57 GiB of matrices per batch) they go back before the matrices are sized
    // (r06, ADVICE r05: only when memory IS short, i.e. when what is free would not give the matrix buffer its full budget (64 GiB = 55 % of 116 GiB) -
    // re-allocating ~35 GB of plan arrays in the next 256 M-pair batch costs 1-2 s, more than the few batches the room buys: UC_ALLOC_LOG at nominal
    // configs[3] showed 443 GiB of 1-2 GiB blocks, 10-12 s per call, profiles/r06/c4_nominal_alloc.txt)
    size_t free_now = 0, total_now = 0;
    const bool mem_short = hipMemGetInfo(&free_now, &total_now) != hipSuccess || free_now + A.tb.tbm.cap < (120ull << 30);
    if (n2 >= (8u << 20) && mem_short) {
        UC_HIP(hipStreamSynchronize(s));
        A.rev.P1.release(); A.start.P2.release(); A.start.P2b.release(); A.rr.P.release(); A.amb.P.release();
        if (B.dedup) A.fwd.P0.release();                   // (without sharing, Lsq / Lst / Lidx ARE P0's arrays)
    }
    A.tb.trun.reserve(n2); A.tb.tpos.reserve(n2); A.tb.tpart.reserve(n2); A.tb.ttie.reserve(n2);
    UC_HIP(hipMemsetAsync(A.tb.ttie.p, 0, (size_t)n2 * 4, s));
    unsigned long long hc = 0;
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 8, s));
    hipLaunchKernelGGL(cells_tb_kernel, grid_for(n2, E.count_grid_cap), dim3(256), 0, s, n2, A.gate.eflag.p, A.gate.link.p, B.Lidx, B.alns_b, A.d_cells.p);
    UC_HIP(hipMemcpyAsync(&hc, A.d_cells.p, 8, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    E.stats.cells_tb += hc;
    // r05: MODE 7 stores a diagonal band of the box, not the box (tb_band_of); the few pairs whose traceback leaves the band are redone
    // with everything stored.  UC_TB_BAND = half-width W (default 48; 0 = always the whole box; the tests force 1 and 4)
    const int band_w = getenv("UC_TB_BAND") ? std::max(0, atoi(getenv("UC_TB_BAND"))) : 48;
    const TbBudget budget;
    if (B.dedup) {
        hipLaunchKernelGGL(tbm_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.gate.eflag.p, A.gate.link.p, B.Lidx, A.fwd.mirror.p, A.gate.gflag.p, A.gate.gpos.p,
                           B.alns_b, A.tb.trun.p, A.tb.tpart.p);
        run_tb(E, B, A.tb.trun.p, band_w, budget);
        hipLaunchKernelGGL(tbm_resolve_kernel, grid_for(n2), dim3(256), 0, s, n2, A.tb.tpart.p, A.tb.ttie.p, A.gate.link.p, B.Lidx, E.p.min_seq_id,
                           B.alns_b, A.gate.eflag.p, A.tb.trun.p);
        if (E.emit_bt) hipLaunchKernelGGL(bt_mirror_kernel, grid_for(n2), dim3(256), 0, s, n2, A.tb.tpart.p, A.tb.ttie.p, A.gate.link.p, B.Lidx, B.bt_pos_b, B.bt_n_b);
        run_tb(E, B, A.tb.trun.p, band_w, budget);   // mirrors whose representative had a gap-direction tie on its traceback
    } else {
        UC_HIP(hipMemcpyAsync(A.tb.trun.p, A.gate.eflag.p, (size_t)n2 * 4, hipMemcpyDeviceToDevice, s));
        run_tb(E, B, A.tb.trun.p, band_w, budget);
    }
}

void preload_traceback_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)tb_gather_kernel); }
}  // namespace uc
