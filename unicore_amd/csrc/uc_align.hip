// uc_align.hip - stage E5/E6 orchestration, device-resident: the driver of the gapped stage.
// The prefilter leaves its hit lists in HBM; everything between them and the accepted edge list stays on the GPU.  Engine::align cuts the lists
// into device batches and runs the named passes on each: length gate, forward pass, reversed-query pass, E-value gate (with the exact end rows),
// start pass, coverage gate, traceback statistics (uc_traceback.hip), accepted edges.  Every pass hands a pair list to the planner
// (uc_sw_plan.hip: build_plan / run_plan); the gates between them are the small kernels of this file with scan-based compaction.  The host only
// sees a handful of counters and, at the end, the accepted edges (stands for Foldseek's structurealign result handling; spec UC-1
// E5/E6).  Also here: the kernel-level entry points on a pair list from the host (sw_batch, sw_pass, tb_emit_pass).
// Work that is never launched: the reversed-query pass of pairs below the E-value threshold (UC-1.1),
// and one of the two DPs of a mutual hit (q,t)/(t,q) in the forward, reversed-query, start and traceback passes
// whenever the result of the other orientation is provably the transposed one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_align_internal.h"

namespace uc {

namespace {

// Mutual hits take both tie-break answers from one known-score DP (uc_sw_pk_impl.hpp key2).  UC_DUAL_TIEBREAK=0: the earlier sharing rule, for A/B
// runs - a mirror shares only where one row holds every optimal cell and is otherwise computed on its own.  The records are the same either way.
static bool dual_tiebreak_on() {
    static const bool on = !(getenv("UC_DUAL_TIEBREAK") && atoi(getenv("UC_DUAL_TIEBREAK")) == 0);
    return on;
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

__global__ void __launch_bounds__(256) bt_putback_kernel(uint32_t nc, const uint32_t *map, const unsigned long long *spos, const uint32_t *sn,
                                                         unsigned long long *dpos, uint32_t *dn) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nc; i += gridDim.x * 256) { dpos[map[i]] = spos[i]; dn[map[i]] = sn[i]; }
}
__global__ void __launch_bounds__(256) edge_scatter_kernel(uint32_t n2, const uint32_t *eflag, const uint32_t *epos, const uint32_t *sq2,
                                                           const uint32_t *st2, uint32_t *edges) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n2; i += gridDim.x * 256) {
        if (!eflag[i]) continue;
        edges[2 * epos[i]] = sq2[i];
        edges[2 * epos[i] + 1] = st2[i];
    }
}

}  // namespace

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

// exact (qEnd, tEnd) for the gate-passing pairs whose end is still unknown (ambiguous end row of the packed kernel, or a
// mirror that could not take its representative's end): a second forward pass that KNOWS the optimum score (packed
// MODE 4; int32 kernel for --sw-kernel i32 and for queries beyond the systolic classes)
// mirror (null: no mutual-hit sharing in this batch): with the packed kernel, the run of a flagged representative also serves its flagged mirror
// (amb_dual_kernel) - one DP, both tie-break answers
static void fix_ambiguous_ends(Engine &E, uint32_t n2, const uint32_t *q2, const uint32_t *t2, int32_t *qe2, int32_t *te2,
                               const uint32_t *link, const int32_t *s0, int32_t *qe0, int32_t *te0, DevBuf<int32_t> &work,
                               DevBuf<char> &tmp, uint32_t n_queries, const uint32_t *mirror) {
    RerunScratch &B = scratch_of(E).amb;
    SwPlan &P3 = B.P;
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
// rule UC-1/L (optional): the stage works on the pairs the length gate lets through - a compacted copy of the batch's pair list with its own
// record array; the records return to their places in the hit-list order at the end of the batch, the gated pairs keep all-zero records
static void length_gate(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.len_gate.flag.reserve(n); A.len_gate.pos.reserve(n);
    hipLaunchKernelGGL(len_gate_kernel, grid_for(n), dim3(256), 0, s, n, B.dq, B.dt, E.ddb.len, E.p.cov, E.p.cov_mode, A.len_gate.flag.p);
    const uint32_t nc = compact(E, A.tmp, A.len_gate.flag.p, A.len_gate.pos.p, n);
    A.len_gate.q.reserve(std::max<uint32_t>(nc, 1)); A.len_gate.t.reserve(std::max<uint32_t>(nc, 1)); A.len_gate.map.reserve(std::max<uint32_t>(nc, 1));
    A.len_gate.alns.reserve(std::max<uint32_t>(nc, 1));
    hipLaunchKernelGGL(len_gate_gather_kernel, grid_for(n), dim3(256), 0, s, n, A.len_gate.flag.p, A.len_gate.pos.p, B.dq, B.dt, A.len_gate.q.p, A.len_gate.t.p, A.len_gate.map.p);
    if (nc) UC_HIP(hipMemsetAsync(A.len_gate.alns.p, 0, (size_t)nc * sizeof(uc_aln), s));
    UC_HIP(hipMemsetAsync(B.alns_list, 0, (size_t)n * sizeof(uc_aln), s));
    if (B.bt_pos_b) {
        A.len_gate.btpos.reserve(std::max<uint32_t>(nc, 1)); A.len_gate.btn.reserve(std::max<uint32_t>(nc, 1));
        UC_HIP(hipMemsetAsync(A.len_gate.btn.p, 0, (size_t)std::max<uint32_t>(nc, 1) * 4, s));
        UC_HIP(hipMemsetAsync(B.bt_n_b, 0, (size_t)n * 4, s));
        B.bt_pos_b = A.len_gate.btpos.p; B.bt_n_b = A.len_gate.btn.p;
    }
    B.dq = A.len_gate.q.p; B.dt = A.len_gate.t.p; B.alns_b = A.len_gate.alns.p; B.n = nc;
}

// forward pass: s0 / qe0 / te0 of every pair, and the directed pair list (Lsq, Lst, Lidx)
static void forward_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.fwd.s0.reserve(n); A.fwd.qe0.reserve(n); A.fwd.te0.reserve(n); A.gate.gflag.reserve(n); A.gate.gpos.reserve(n);
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 16, s));
    if (!B.dedup) {
        build_plan(E, A.fwd.P0, A.tmp, n, B.dq, B.dt, nullptr, nullptr, B.tab);
        run_plan(E, A.fwd.P0, 0, A.fwd.s0.p, A.fwd.qe0.p, A.fwd.te0.p, A.work, A.tmp, /*ovf_only=*/true);
        E.stats.cells_fwd += A.fwd.P0.cells;
        B.Lsq = A.fwd.P0.sq.p; B.Lst = A.fwd.P0.st.p; B.Lidx = A.fwd.P0.idx.p;
        return;
    }
    // mutual hits share one forward DP, computed in the orientation with the shorter query
    A.fwd.ukey.reserve(n); A.fwd.ukey2.reserve(n); A.fwd.uidx_in.reserve(n); A.fwd.uidx.reserve(n);
    A.fwd.fq.reserve(n); A.fwd.ft.reserve(n); A.fwd.mirror.reserve(n); A.fwd.rep.reserve(n); A.fwd.rpos.reserve(n);
    hipLaunchKernelGGL(ukey_kernel, grid_for(n), dim3(256), 0, s, n, B.dq, B.dt, E.ddb.len, A.fwd.ukey.p, A.fwd.uidx_in.p);
    rocprim_call(A.tmp, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, A.fwd.ukey.p, A.fwd.ukey2.p, A.fwd.uidx_in.p, A.fwd.uidx.p, (size_t)n, 0u, 49u, s); });
    hipLaunchKernelGGL(umark_kernel, grid_for(n), dim3(256), 0, s, n, A.fwd.ukey2.p, A.fwd.uidx.p, B.dq, B.dt, A.fwd.fq.p, A.fwd.ft.p, A.fwd.mirror.p, A.fwd.rep.p);
    const uint32_t nu = compact(E, A.tmp, A.fwd.rep.p, A.fwd.rpos.p, n);
    A.fwd.qr.reserve(nu); A.fwd.tr.reserve(nu); A.fwd.jrep.reserve(nu); A.fwd.su.reserve(nu); A.fwd.qeu.reserve(nu); A.fwd.teu.reserve(nu);
    hipLaunchKernelGGL(ugather_kernel, grid_for(n), dim3(256), 0, s, n, A.fwd.rep.p, A.fwd.rpos.p, A.fwd.fq.p, A.fwd.ft.p, A.fwd.qr.p, A.fwd.tr.p, A.fwd.jrep.p);
    build_plan(E, A.fwd.P0, A.tmp, nu, A.fwd.qr.p, A.fwd.tr.p, nullptr, nullptr, B.tab);
    run_plan(E, A.fwd.P0, 0, A.fwd.su.p, A.fwd.qeu.p, A.fwd.teu.p, A.work, A.tmp, /*ovf_only=*/true);
    hipLaunchKernelGGL(uscatter_kernel, grid_for(nu), dim3(256), 0, s, nu, n, A.fwd.P0.idx.p, A.fwd.jrep.p, A.fwd.mirror.p, A.fwd.su.p, A.fwd.qeu.p, A.fwd.teu.p,
                       packed_prefix(A.fwd.P0).pairs, SW_PK_OVF_HOST, A.fwd.s0.p, A.fwd.qe0.p, A.fwd.te0.p);
    hipLaunchKernelGGL(cells_kernel, grid_for(n, E.count_grid_cap), dim3(256), 0, s, n, A.fwd.fq.p, A.fwd.ft.p, (const uint32_t *)nullptr, E.ddb.len, A.d_cells.p);
    B.Lsq = A.fwd.fq.p; B.Lst = A.fwd.ft.p; B.Lidx = A.fwd.uidx.p;
}

// spec UC-1.1: the reversed-query pass only runs for pairs whose forward score reaches the E-value
// threshold (corrected <= score, so the others cannot pass); their score_rev is reported as 0
static void rev_correction_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    A.rev.s1.reserve(n);
    UC_HIP(hipMemsetAsync(A.rev.s1.p, 0, (size_t)n * 4, s));
    hipLaunchKernelGGL(gate_kernel, grid_for(n), dim3(256), 0, s, n, B.Lsq, A.fwd.s0.p, (const int32_t *)nullptr, A.gate.d_ms.p, B.qbegin, A.gate.gflag.p);
    if (B.dedup) {
        A.rev.rcopy.reserve(n);
        hipLaunchKernelGGL(cells_kernel, grid_for(n, E.count_grid_cap), dim3(256), 0, s, n, B.Lsq, B.Lst, A.gate.gflag.p, E.ddb.len, A.d_cells.p + 1);
        hipLaunchKernelGGL(rev_dedup_kernel, grid_for(n), dim3(256), 0, s, n, A.fwd.mirror.p, A.gate.gflag.p, A.rev.rcopy.p);
        hipLaunchKernelGGL(rev_unflag_kernel, grid_for(n), dim3(256), 0, s, n, A.rev.rcopy.p, A.gate.gflag.p);
    }
    const uint32_t n1 = compact(E, A.tmp, A.gate.gflag.p, A.gate.gpos.p, n);
    if (n1) {
        A.rev.q1.reserve(n1); A.rev.t1.reserve(n1); A.rev.link1.reserve(n1); A.rev.s1c.reserve(n1);
        hipLaunchKernelGGL(pair_gather_kernel, grid_for(n), dim3(256), 0, s, n, A.gate.gflag.p, A.gate.gpos.p, B.Lsq, B.Lst, A.rev.q1.p, A.rev.t1.p, A.rev.link1.p);
        build_plan(E, A.rev.P1, A.tmp, n1, A.rev.q1.p, A.rev.t1.p, nullptr, nullptr, B.tab);
        run_plan(E, A.rev.P1, 1, A.rev.s1c.p, nullptr, nullptr, A.work, A.tmp);
        hipLaunchKernelGGL(rev_putback_kernel, grid_for(n1), dim3(256), 0, s, n1, A.rev.P1.idx.p, A.rev.link1.p, A.rev.s1c.p, A.rev.s1.p);
        if (!B.dedup) E.stats.cells_rev += A.rev.P1.cells;
    }
    if (B.dedup) hipLaunchKernelGGL(rev_copy_kernel, grid_for(n), dim3(256), 0, s, n, A.rev.rcopy.p, A.rev.s1.p);
}

// E-value gate on the corrected score: the gate passers (q2, t2, qe2, te2, link) with their exact end rows, and the records of every pair
static void evalue_gate(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n = B.n;
    const int32_t *s1p = E.p.rev_correction ? A.rev.s1.p : nullptr;
    hipLaunchKernelGGL(gate_kernel, grid_for(n), dim3(256), 0, s, n, B.Lsq, A.fwd.s0.p, s1p, A.gate.d_ms.p, B.qbegin, A.gate.gflag.p);
    const uint32_t n2 = B.n2 = compact(E, A.tmp, A.gate.gflag.p, A.gate.gpos.p, n);
    if (n2) {
        A.gate.q2.reserve(n2); A.gate.t2.reserve(n2); A.gate.qe2.reserve(n2); A.gate.te2.reserve(n2); A.gate.link.reserve(n2);
        A.start.s2.reserve(n2); A.start.q2o.reserve(n2); A.start.t2o.reserve(n2); A.gate.eflag.reserve(n2); A.gate.epos.reserve(n2);
        hipLaunchKernelGGL(gate_scatter_kernel, grid_for(n), dim3(256), 0, s, n, A.gate.gflag.p, A.gate.gpos.p, B.Lsq, B.Lst, A.fwd.qe0.p, A.fwd.te0.p,
                           A.gate.q2.p, A.gate.t2.p, A.gate.qe2.p, A.gate.te2.p, A.gate.link.p);
        if (E.p.sw_pk || B.dedup)
            fix_ambiguous_ends(E, n2, A.gate.q2.p, A.gate.t2.p, A.gate.qe2.p, A.gate.te2.p, A.gate.link.p, A.fwd.s0.p, A.fwd.qe0.p, A.fwd.te0.p, A.work, A.tmp, B.qb - B.qa,
                               B.dedup ? A.fwd.mirror.p : nullptr);
    }
    hipLaunchKernelGGL(aln_basic_kernel, grid_for(n), dim3(256), 0, s, n, B.Lidx, A.fwd.s0.p, s1p, A.fwd.qe0.p, A.fwd.te0.p, A.gate.gflag.p, B.alns_b);
}

// one known-score start pass (packed MODE 6; the optimum of the start pass is the forward score) over the m gate passers flagged in smkeep
// dual: round 1 - the second answer of every pair goes to q2o2 / t2o2 for the mirrors that share the DP
static void known_start_round(Engine &E, const AlignBatch &B, SwPlan &P, uint32_t m, int tab, uint32_t *uniq, bool dual) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    A.start.q2a.reserve(m); A.start.t2a.reserve(m); A.start.qe2a.reserve(m); A.start.te2a.reserve(m); A.start.mapa.reserve(m);
    hipLaunchKernelGGL(sm_gather_kernel, grid_for(B.n2), dim3(256), 0, s, B.n2, A.start.smkeep.p, A.start.smpos.p, A.gate.q2.p, A.gate.t2.p, A.gate.qe2.p, A.gate.te2.p,
                       A.start.q2a.p, A.start.t2a.p, A.start.qe2a.p, A.start.te2a.p, A.start.mapa.p);
    A.start.sknown.reserve(m);
    hipLaunchKernelGGL(sm_score_kernel, grid_for(m), dim3(256), 0, s, m, A.start.mapa.p, A.gate.link.p, A.fwd.s0.p, A.start.sknown.p);
    build_plan(E, P, A.tmp, m, A.start.q2a.p, A.start.t2a.p, A.start.qe2a.p, A.start.te2a.p, tab, nullptr, nullptr, A.start.sknown.p);
    if (dual) { A.start.q2os2.reserve(m); A.start.t2os2.reserve(m); }
    const SwSecond sec{A.start.q2os2.p, A.start.t2os2.p};
    run_plan(E, P, 6, A.start.s2s.p, A.start.q2os.p, A.start.t2os.p, A.work, A.tmp, false, dual ? &sec : nullptr);
    hipLaunchKernelGGL(sm_scatter_kernel, grid_for(m), dim3(256), 0, s, m, P.idx.p, A.start.mapa.p, A.start.s2s.p, A.start.q2os.p, A.start.t2os.p,
                       A.start.s2.p, A.start.q2o.p, A.start.t2o.p, uniq, dual ? A.start.q2os2.p : nullptr, dual ? A.start.t2os2.p : nullptr,
                       dual ? A.start.q2o2.p : nullptr, dual ? A.start.t2o2.p : nullptr);
}

// start pass of the shared-DP path on the packed kernel
static void start_pass_known(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    A.start.smkeep.reserve(n2); A.start.smpos.reserve(n2); A.start.partner.reserve(n2); A.start.uniq.reserve(n2);
    UC_HIP(hipMemsetAsync(A.start.uniq.p, 0, (size_t)n2 * 4, s));
    hipLaunchKernelGGL(sm_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.gate.link.p, A.fwd.mirror.p, A.gate.gflag.p, A.gate.gpos.p, A.gate.qe2.p, A.gate.te2.p,
                       A.fwd.qe0.p, A.fwd.te0.p, A.start.smkeep.p, A.start.partner.p);
    // round 1: exact in one pass; it reports both tie-break answers, and whether a single row holds every optimal cell
    const bool dual = dual_tiebreak_on();
    if (dual) { A.start.q2o2.reserve(n2); A.start.t2o2.reserve(n2); }
    known_start_round(E, B, A.start.P2, compact(E, A.tmp, A.start.smkeep.p, A.start.smpos.p, n2), B.tab, A.start.uniq.p, dual);
    hipLaunchKernelGGL(sm_resolve_kernel, grid_for(n2), dim3(256), 0, s, n2, A.start.partner.p, A.start.uniq.p, A.start.s2.p, A.start.q2o.p, A.start.t2o.p,
                       dual ? A.start.q2o2.p : nullptr, dual ? A.start.t2o2.p : nullptr);
    // round 2: the mirrors that could not take their partner's result - with both answers at hand only those whose partner's result came from
    // another kernel than the packed known-score one (int32 re-runs, queries beyond the systolic classes)
    hipLaunchKernelGGL(amb_flag_kernel, grid_for(n2), dim3(256), 0, s, n2, A.start.q2o.p, A.start.smkeep.p);
    const uint32_t n2b = compact(E, A.tmp, A.start.smkeep.p, A.start.smpos.p, n2);
    if (!n2b) return;
    known_start_round(E, B, A.start.P2b, n2b, pk_known_tab(n2b, B.qb - B.qa), nullptr, false);
    E.stats.n_pk_reruns += n2b;
}

// start pass; results end up in the natural order of the gate-passer list (iota2 stands for the plan order).  Then the records of the gate
// passers, the coverage gate and the edge flags (eflag)
static void start_pass(Engine &E, AlignBatch &B) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    const uint32_t n2 = B.n2;
    A.start.iota2.reserve(n2); A.start.s2s.reserve(n2); A.start.q2os.reserve(n2); A.start.t2os.reserve(n2);
    hipLaunchKernelGGL(iota_kernel, grid_for(n2), dim3(256), 0, s, n2, A.start.iota2.p);
    UC_HIP(hipMemsetAsync(A.d_cells.p, 0, 8, s));
    hipLaunchKernelGGL(cells_box_kernel, grid_for(n2, E.count_grid_cap), dim3(256), 0, s, n2, A.gate.qe2.p, A.gate.te2.p, A.d_cells.p);
    if (B.dedup && B.tab == 1) {
        start_pass_known(E, B);
    } else {
        build_plan(E, A.start.P2, A.tmp, n2, A.gate.q2.p, A.gate.t2.p, A.gate.qe2.p, A.gate.te2.p, B.tab);
        run_plan(E, A.start.P2, 2, A.start.s2s.p, A.start.q2os.p, A.start.t2os.p, A.work, A.tmp);
        hipLaunchKernelGGL(sm_scatter_kernel, grid_for(n2), dim3(256), 0, s, n2, A.start.P2.idx.p, (const uint32_t *)nullptr, A.start.s2s.p, A.start.q2os.p,
                           A.start.t2os.p, A.start.s2.p, A.start.q2o.p, A.start.t2o.p, (uint32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr,
                           (int32_t *)nullptr, (int32_t *)nullptr);
    }
    unsigned long long hc = 0;
    uint32_t dual_err = 0;
    UC_HIP(hipMemcpyAsync(&hc, A.d_cells.p, 8, hipMemcpyDeviceToHost, s));
    if (A.amb.err.p) UC_HIP(hipMemcpyAsync(&dual_err, A.amb.err.p, 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    if (dual_err) fail(UC_ERR_GENERIC, "gapped stage: %u shared end re-runs came back without a second answer", dual_err);
    E.stats.cells_start += hc;
    hipLaunchKernelGGL(finalize_kernel, grid_for(n2), dim3(256), 0, s, n2, A.start.iota2.p, A.gate.link.p, B.Lidx, A.gate.q2.p, A.gate.t2.p, A.start.s2.p,
                       A.start.q2o.p, A.start.t2o.p, E.ddb.len, E.p.cov, E.p.cov_mode, B.alns_b, A.gate.eflag.p, A.gate.mism.p);
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
        pass_classes(*this, nn, dq.p, tab, cls.p);
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
    A.gate.q2.reserve(n); A.gate.t2.reserve(n); A.gate.link.reserve(n); A.start.iota2.reserve(n); A.gate.eflag.reserve(n);
    A.tb.trun.reserve(n); A.tb.tpos.reserve(n); A.tb.tpart.reserve(n); A.tb.ttie.reserve(n); A.tb.tmiss.reserve(n);
    UC_HIP(hipMemcpyAsync(A.gate.q2.p, dq.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.gate.t2.p, dt.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.gate.link.p, iota.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.start.iota2.p, iota.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemcpyAsync(A.gate.eflag.p, all.p, n * 4, hipMemcpyDeviceToDevice, stream));
    UC_HIP(hipMemsetAsync(A.tb.ttie.p, 0, n * 4, stream));
    UC_HIP(hipMemsetAsync(A.tb.tmiss.p, 0, n * 4, stream));
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
    if (o.miss) UC_HIP(hipMemcpyAsync(o.miss, A.tb.tmiss.p, n * 4, hipMemcpyDeviceToHost, stream));
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

// the accepted edges of the batch (ne flagged in eflag / epos) appended to the engine's device edge list
static void append_edges(Engine &E, const AlignBatch &B, uint32_t ne) {
    AlignScratch &A = scratch_of(E);
    hipStream_t s = E.stream;
    A.d_e.reserve(2 * (size_t)ne);
    hipLaunchKernelGGL(edge_scatter_kernel, grid_for(B.n2), dim3(256), 0, s, B.n2, A.gate.eflag.p, A.gate.epos.p, A.gate.q2.p, A.gate.t2.p, A.d_e.p);
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
    UC_HIP(hipMemcpyAsync(&bad, A.gate.mism.p, 4, hipMemcpyDeviceToHost, s));
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipGetLastError());
    if (bad) fail(UC_ERR_GENERIC, "start pass score differs from the forward score for %u pairs", bad);
    E.stats.n_gapped_alignments += B.n;
    E.stats.n_start_alignments += B.n2;
    if (B.alns_b != B.alns_list) {
        hipLaunchKernelGGL(len_gate_putback_kernel, grid_for(B.n), dim3(256), 0, s, B.n, A.len_gate.map.p, (const uc_aln *)B.alns_b, B.alns_list);
        if (B.bt_pos_b) hipLaunchKernelGGL(bt_putback_kernel, grid_for(B.n), dim3(256), 0, s, B.n, A.len_gate.map.p, A.len_gate.btpos.p, A.len_gate.btn.p, E.d_bt_pos.p + E.hit_off[B.qa], E.d_bt_n.p + E.hit_off[B.qa]);
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
    A.gate.d_ms.reserve(std::max<size_t>(h_ms.size(), 1));
    if (!h_ms.empty()) UC_HIP(hipMemcpyAsync(A.gate.d_ms.p, h_ms.data(), h_ms.size() * 4, hipMemcpyHostToDevice, s));
    A.gate.mism.reserve(1);
    UC_HIP(hipMemsetAsync(A.gate.mism.p, 0, 4, s));

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
            uint32_t ne = compact(*this, A.tmp, A.gate.eflag.p, A.gate.epos.p, B.n2);
            if ((p.min_seq_id > 0.0f || p.want_tb) && ne) {
                traceback_stats(*this, B);
                ne = compact(*this, A.tmp, A.gate.eflag.p, A.gate.epos.p, B.n2);
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

void preload_align_module() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)gate_kernel); }
}  // namespace uc
