// uc_align_internal.h - what the four translation units of the gapped stage and of the clustering graph share on the host: the shape of the class
// tables, the plan of one gapped pass, the scratch of every pass grouped by the pass that fills it, and the functions that cross files
// (uc_sw_plan.hip: planner and launcher; uc_align.hip: the driver; uc_traceback.hip: traceback statistics and backtraces; uc_cluster_graph.hip:
// stage E7 on the device).  Host-side declarations only: no kernel lives here, and nothing that instantiates a rocPRIM kernel.
#pragma once
#include "uc_engine.h"

namespace uc {

constexpr int SW_PK_OVF_HOST = 0x7C00 - 256;   // == SW_PK_OVF of uc_sw_pk_impl.hpp

// Every statistic of a traceback travels in a 32-bit word of its own, the count in bits 0..30 and the gap-direction tie mark of the walk that
// counted it in bit 31: alignment length (at most lq + lt = 131,070 columns), identities (at most 65,535), gaps (at most the length).  One word
// cannot hold two of them: 17 + 16 bits and the mark.
constexpr uint32_t TB_COUNT = 0x7FFFFFFFu;
constexpr uint32_t TB_BAND_MISS = 0x7FFFFFFFu;     // in the length word: "the walk left the stored band" (no traceback has 2^31 - 1 columns)

// Length classes (the tables themselves: uc_sw_plan.hip).  Table 0: int32 kernel for everything (16 systolic classes + the row-blocked long-query kernel).
// Table 1: the packed 16-bit kernel for all systolic classes: queries <= 2048 rows in 28 classes with even R (~6R + 60 live registers).
constexpr int MAXCLS = 28;
struct ClassTable {
    int n;                 // systolic classes; index n = long queries (> cap[n-1] rows): uc_sw_long.hip
    int cap[MAXCLS], G[MAXCLS], R[MAXCLS], pk[MAXCLS];
    uint32_t tcap[MAXCLS]; // pairs per workgroup task
};
extern const ClassTable h_tab[4];
constexpr int NB = MAXCLS + 2;   // class bounds of a plan: the systolic classes, the long-query class, the end

// the matrix budget of the traceback passes: the rule and its constants are in uc_traceback.hip
struct TbBudget {
    unsigned long long forced = 0;   // UC_TB_BUDGET_MB in bytes, 0 if unset
    TbBudget();
    uint32_t segment_pairs() const;
    // matrix bytes of one batch, for a segment whose matrices take `total` bytes and a buffer that holds `held` already
    unsigned long long batch_bytes(unsigned long long total, size_t held) const;
};

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

// the packed classes form a prefix of a plan's sorted pair list, and their tasks a prefix of its task list
struct PackedPrefix { uint32_t pairs, tasks; };

// the second answer of a packed known-score pass (uc_sw_pk_impl.hpp key2): end under the order (first optimal row, then first column)
struct SwSecond { int32_t *qe, *te; };

// ---- scratch, grouped by the pass that fills it ------------------------------------------------------------------------
// A buffer belongs to the pass that writes it; a later pass that reads it names the owner (A.gate.link, A.fwd.mirror).
// length_gate: the compacted pair list of a batch and its records (rule UC-1/L); finish_batch puts the records (and, with -a, btpos / btn) back
struct LenGateScratch {
    DevBuf<uint32_t> q, t, map, flag, pos, btn;
    DevBuf<uc_aln> alns;
    DevBuf<unsigned long long> btpos;
};
// forward_pass: scores and ends of every pair (s0, qe0, te0; fix_ambiguous_ends overwrites the ends it resolves) and the mutual-hit list (fq, ft,
// mirror); read by every later pass of the batch
struct ForwardScratch {
    DevBuf<int32_t> s0, qe0, te0, su, qeu, teu;
    DevBuf<uint64_t> ukey, ukey2;
    DevBuf<uint32_t> uidx_in, uidx, fq, ft, mirror, rep, rpos, qr, tr, jrep;
    SwPlan P0;
};
// rev_correction_pass: s1 of every pair; read by evalue_gate
struct RevScratch {
    DevBuf<int32_t> s1, s1c;
    DevBuf<uint32_t> q1, t1, link1, rcopy;
    SwPlan P1;
};
// evalue_gate: the gate flags of every pair (gflag / gpos: forward_pass reserves them, the reversed-query pass borrows them for its own gate) and
// the gate-passer list (q2 .. link); d_ms and mism are set up by Engine::align per call; eflag / epos: the edge flags - start_pass fills them
// (finalize_kernel), the traceback narrows them, Engine::align compacts them.  Read by the start pass, the traceback and append_edges
struct GateScratch {
    DevBuf<int32_t> d_ms, qe2, te2;
    DevBuf<uint32_t> gflag, gpos, q2, t2, link, eflag, epos, mism;
};
// start_pass / start_pass_known / known_start_round: starts of the gate passers in list order (s2, q2o, t2o: evalue_gate reserves them); iota2
// stands for the plan order and is read by the traceback
struct StartScratch {
    DevBuf<int32_t> s2, q2o, t2o, s2s, q2os, t2os, qe2a, te2a, sknown, q2os2, t2os2, q2o2, t2o2;
    DevBuf<uint32_t> iota2, smkeep, smpos, partner, uniq, q2a, t2a, mapa;
    SwPlan P2, P2b;
};
// one re-run of a pair list by a second plan: run_plan's packed-range re-run (rr) and fix_ambiguous_ends (amb); start_pass reads amb.err
struct RerunScratch {
    DevBuf<uint32_t> flag, pos, q2, t2, link, dual, err;
    DevBuf<int32_t> qe2, te2, s, qe, te, sin, qeb, teb;
    SwPlan P;
};
// traceback_stats / run_tb / tb_batch (--min-seq-id, search) and, with -a, the backtraces: runs per pair of the traceback plan, slice offsets
// inside a matrix batch, where each slice went, which kernel walked it.  Engine::sw_pass sets up trun .. tmiss for its own one-pass batch
struct TracebackScratch {
    DevBuf<uint32_t> q3, t3, src3, trun, tpos, tpart, ttie, tlo, thi, tmiss, tchunk, tcpos;
    DevBuf<unsigned long long> tbsize, tboff, toff;
    DevBuf<uint8_t> tbm;
    bool tbm_live = false;           // inside the batch loop of a MODE 7 call: the one time the matrices may not be given back (release_tb_matrices)
    DevBuf<int32_t> qs3, qe3, ts3, te3, pack3, id3, gaps3, sc3;
    SwPlan P3;
    DevBuf<uint32_t> bt_cnt3, bt_off3, bt_plain3, bt_err;
    DevBuf<unsigned long long> bt_pos3;
};

// Work buffers of the gapped stage and of the set-cover graph build.  ONE set per engine (parked per device between
// engines): nothing in the four files is process-wide, so engines on different devices - or several engines on one device,
// each driven by its own host thread as uc_cluster does for num_gpus > 1 - never share or race on a buffer.
struct AlignScratch {
    DevBuf<char> tmp;                // shared by every pass: rocPRIM's temporary storage,
    DevBuf<int32_t> work;            // the long-query kernel's work area,
    DevBuf<unsigned long long> d_cells;   // and the cell counters a pass hands to the host
    LenGateScratch len_gate;
    ForwardScratch fwd;
    RevScratch rev;
    GateScratch gate;
    StartScratch start;
    RerunScratch rr, amb;
    TracebackScratch tb;
    DevBuf<uint32_t> d_e;            // append_edges: the accepted edges of the batch
    SetCoverScratch sc;              // build_cluster_graph + set_cover_graph (uc_cluster_graph.hip)
    GreedyIncScratch gi;             // --cluster-mode 2 (uc_greedy_inc.hip): same graph buffers, its own round state
    ReassignScratch ra;              // --cluster-reassign (uc_reassign.hip): member keys, flags, seeds, the stage's edge list
};
inline AlignScratch &scratch_of(Engine &E) {
    if (!E.aln) E.aln = ParkedScratch<AlignScratch>::take_or_new(E.device);
    return *E.aln;
}

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

// ---- uc_sw_plan.hip ----
int pk_known_tab(uint32_t n_pairs, uint32_t n_queries);
void max_scan_u32(Engine &E, DevBuf<char> &tmp, const uint32_t *in, uint32_t *out, uint32_t n);
uint32_t compact(Engine &E, DevBuf<char> &tmp, const uint32_t *flag, uint32_t *pos, uint32_t n);
PackedPrefix packed_prefix(const SwPlan &P);
void build_plan(Engine &E, SwPlan &P, DevBuf<char> &tmp, uint32_t n, const uint32_t *q, const uint32_t *t,
                const int32_t *qe, const int32_t *te, int tab, const int32_t *qs = nullptr, const int32_t *ts = nullptr,
                const int32_t *aux = nullptr /* one value per pair carried into plan order (known scores) */,
                bool lpt = true /* false: tasks stay in pair order (the traceback plan is cut into byte-budgeted pair ranges) */);
uint64_t launch_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
                     const uint32_t *tb = nullptr, bool only_long = false, uint32_t t0 = 0, uint32_t t1 = 0xFFFFFFFFu, bool skip_long = false,
                     const SwSecond *sec = nullptr);
void run_plan(Engine &E, SwPlan &P, int mode, int32_t *os, int32_t *oqe, int32_t *ote, DevBuf<int32_t> &work,
              DevBuf<char> &tmp, bool ovf_only = false, const SwSecond *sec = nullptr);
// the class a plan of table `tab` puts each of the n queries q[] in, on the engine's stream (after a build_plan on this device)
void pass_classes(Engine &E, uint32_t n, const uint32_t *q, int tab, int32_t *out);
// the two traceback kernels that read the class table, over the plan tb.P3 (table 1): matrix bytes of its first n_pk pairs; the walk of pairs [p0, p1)
void launch_tb_size(Engine &E, uint32_t n_pk, int band, unsigned long long *size);
void launch_tb_walk(Engine &E, int emit, int plain, uint32_t p0, uint32_t p1, int band, const uint8_t *tbm, const unsigned long long *tboff, uint64_t base);
// ---- uc_traceback.hip ----
bool tb_bytes_ok(const Params &p);
void tb_batch(Engine &E, const AlignBatch &B, const uint32_t *flag, bool pk, int band, const TbBudget &budget);
void run_tb(Engine &E, const AlignBatch &B, const uint32_t *flag, int band_w, const TbBudget &budget);
void traceback_stats(Engine &E, const AlignBatch &B);
void bt_assemble(size_t n, const unsigned long long *pos, const uint32_t *cnt, const uc_aln *alns /* null: every record counts */,
                 const uint32_t *hruns, uint64_t base, uint64_t *run_off, std::vector<uint32_t> &runs);

}  // namespace uc
