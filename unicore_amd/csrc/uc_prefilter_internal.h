// uc_prefilter_internal.h - what the five translation units of the prefilter (stages E1-E4) share: the k-mer pattern and the layout of the hit keys, the
// two device helpers used in more than one file, the scratch of every pass grouped by the pass that fills it, the state of one target-chunk pass and of
// its query batches, and the passes that cross files (uc_kmer_match.hip: index, similar k-mers, run lists; uc_kmer_filter.hip: runs to surviving keys;
// uc_diag_select.hip: keys to candidates; uc_hit_lists.hip: E3 / E4 and the installed hit lists; uc_prefilter.hip: the driver).  No kernel lives here
// and nothing that instantiates a rocPRIM kernel: a kernel stays in the file of the host pass that launches it.
#pragma once
#include <hip/hip_runtime.h>

#include "uc_engine.h"

namespace uc {

struct KmerCfg {
    int koff[K];
    int span;
    int thr;
};

// sequence id containing padded residue offset p, searched in off[lo..hi)
__device__ __forceinline__ uint32_t find_seq(const uint32_t *off, uint32_t lo, uint32_t hi, uint32_t p) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

struct RunList {
    uint32_t *pidx;     // query position inside the batch
    uint64_t *val;      // [ entry count : 32 | first index entry : 32 ]
    uint64_t cap;
};

struct RankRec { uint32_t roff, nr, hits, nsim; };   // one 16-byte record per distinct k-mer: first run, runs, k-mer hits, similar k-mers

// hit key: [ query - qbegin | target : tbits | diagonal + dbias : dbits ]; the field widths follow the database
// (number of sequences, longest sequence) so that the radix sort touches as few digits as possible
struct KeyFmt {
    int dbits, tbits;
    int dbias;
    // compact mode (the common case): when (target - tbase) and the diagonal fit 32 bits together, index entries are
    // u32 [target - tbase | position : dbits - 1] and the per-query (target, diagonal) keys of the double-hit filter are
    // u32 [target - tbase | diagonal + dbias : dbits] - half the bytes of the wide u64 forms on every gather and stream
    int compact;
    uint32_t tbase;
};

struct WidenU32 {
    __host__ __device__ uint64_t operator()(uint32_t x) const { return (uint64_t)x; }
};

// td_select_kernel takes the queries with at most this many surviving keys (uc_diag_select.hip: TDS_T threads x TDS_MAX_IPT keys, asserted there)
constexpr uint32_t TDS_CAP = 8192;

// ---- the counters of a pass: shared.d_counters[0..7], one unsigned long long each -----------------------------------------------------------------------
//   [0] similar k-mers (sim_runs_kernel per distinct k-mer, position_runs_kernel per query position)
//   [1] candidates E4 keeps, score >= min_ungapped (select_key_kernel)
//   [2] ungapped overlap residues of E3 (launch_ungapped), summed over the chunk and read by finish_chunk
//   [3] run cursor (sim_runs_kernel)
//   [4] k-mer hits of the runs (sim_runs_kernel)
//   [5] key cursor (expand_kernel), region cursor (filter_kernel)
//   [6] candidate cursor (diag_select_kernel, diag_long_kernel; ungapped_all_candidates in --prefilter-mode 1)
//   [7] [ queries : 24 | keys : 40 ] of the batch that td_select_kernel took
// prefilter_one zeroes all eight; distinct_runs zeroes [0] and [3]-[6] before each enumeration, plan_superbatch [0] before position_runs_kernel,
// cut_batch [3]-[6], expand_keys_filtered [7], select_diagonals [6] before each attempt, select_and_append [1].

// ---- scratch, grouped by the pass that fills it ----------------------------------------------------------------------------------------------------------
// A buffer belongs to the pass that writes it first in the pipeline; a pass that reads or borrows it is named in the owner's comment.  Every group lists
// its buffers in each() directly under them, and the assert behind the group compares the group's size with that list: a DevBuf<T> is a pointer and a
// size whatever T is, so a buffer added to a group without adding it to each() (and raising the count) does not compile.  What each() leaves out
// would be missing from PrefilterScratch::bytes() and would never be given back by release_bytes().
#define UC_LISTS_EVERY_BUFFER(group, count) \
    static_assert(sizeof(group) == (count) * sizeof(DevBuf<char>), #group ": a buffer was added or removed; list it in each() and correct the count")

// every pass: the counters (legend above) and rocPRIM's temporary storage (build_index, plan_superbatch, expand_keys_*, select_and_append,
// partition_hits_by_owner, merge_hits_dev)
struct SharedScratch {
    DevBuf<unsigned long long> d_counters;
    DevBuf<char> d_temp;
    template <class F> void each(F &f) { f(d_counters); f(d_temp); }
};
UC_LISTS_EVERY_BUFFER(SharedScratch, 2);
// build_index: the chunk's k-mer index - offsets per k-mer, sort input and output, the entries in compact (d_ent32) or wide (d_ent) form, the presence
// bitmap.  d_koff / d_kbits and the entries are read by sim_runs_kernel, expand_kernel and filter_kernel
struct IndexScratch {
    DevBuf<uint32_t> d_koff, k_in, k_out, d_ent32, v_in32;
    DevBuf<uint64_t> d_ent, v_in;
    DevBuf<uint32_t> d_kbits;       // presence bitmap of the chunk's k-mers
    template <class F> void each(F &f) { f(d_koff); f(k_in); f(k_out); f(d_ent32); f(v_in32); f(d_ent); f(v_in); f(d_kbits); }
};
UC_LISTS_EVERY_BUFFER(IndexScratch, 8);
// expand_keys_filtered / expand_keys_plain: the launch order of the filter's workgroups (d_okey .. d_order), the key regions (d_keys), where a query's
// survivors lie and how many they are (d_qbase / d_qsurv / d_soff), the dense keys and the sort's output (d_keys2).  td_select_kernel sorts inside d_keys
// and zeroes d_qsurv of the queries it took; cand_gather_kernel reads the records it left in d_keys.  cut_batch fills nothing here: a batch's runs are
// read where the plan left them (PlanScratch)
struct BatchScratch {
    DevBuf<uint32_t> d_okey, d_okey2, d_oidx, d_order;
    DevBuf<uint32_t> d_qsurv;
    DevBuf<uint64_t> d_keys, d_keys2, d_qbase, d_soff;
    template <class F> void each(F &f) { f(d_okey); f(d_okey2); f(d_oidx); f(d_order); f(d_qsurv); f(d_keys); f(d_keys2); f(d_qbase); f(d_soff); }
};
UC_LISTS_EVERY_BUFFER(BatchScratch, 9);
// rescore_ungapped (E3): d_score, which prefilter_exhaustive fills from its tiles instead; select_and_append (E4) and merge_hits_dev, which run the same
// sort / rank / truncate / scatter: sort keys and the sorted diagonals (d_skey / d_skey2 / d_cd2), the rank flags and their positions (d_flag / d_pos);
// finish_hit_lists: d_cnt.  partition_hits_by_owner borrows d_flag and d_cnt as its index arrays
struct SelectScratch {
    DevBuf<uint32_t> d_cnt, d_flag;
    DevBuf<uint64_t> d_pos, d_skey, d_skey2;
    DevBuf<int32_t> d_cd2, d_score;
    template <class F> void each(F &f) { f(d_cnt); f(d_flag); f(d_pos); f(d_skey); f(d_skey2); f(d_cd2); f(d_score); }
};
UC_LISTS_EVERY_BUFFER(SelectScratch, 7);
// select_diagonals: the candidates of a batch (d_cq / d_ct / d_cd: query, target, diagonal), which prefilter_exhaustive fills from its tiles instead, and
// the long-group flags of diag_select_kernel (d_wflag); expand_keys_filtered reserves what td_select_kernel writes: the region-resident candidates per
// query (plain, mirrored, both) and where cand_gather_kernel puts them (d_coff).  Read by E3 / E4; partition_hits_by_owner borrows d_cq and d_ct as its keys
struct CandScratch {
    DevBuf<uint32_t> d_cq, d_ct;
    DevBuf<int32_t> d_cd;
    DevBuf<uint8_t> d_wflag;
    DevBuf<uint32_t> d_qcand, d_qmir, d_qrec;
    DevBuf<uint64_t> d_coff;
    template <class F> void each(F &f) { f(d_cq); f(d_ct); f(d_cd); f(d_wflag); f(d_qcand); f(d_qmir); f(d_qrec); f(d_coff); }
};
UC_LISTS_EVERY_BUFFER(CandScratch, 8);
// plan_superbatch / distinct_runs: the distinct k-mers of a super-batch (d_kflag, d_kid: rank of every k-mer, d_dk: the list, d_nsimk), their runs unsorted
// (d_drk / d_drv) and sorted by rank (d_drk2 / d_drv2), per rank d_roff / d_rec, per query position d_qk / d_nr / d_src / d_ph and the running sums d_cumh /
// d_cumr, per query d_qh / d_qrn.  filter_kernel and expand_kernel read the runs of an exact batch from here (d_src, d_cumr, d_drv2, d_qh), the launch
// order of the filter's workgroups comes from d_qrn
struct PlanScratch {
    DevBuf<uint8_t> d_kflag;
    DevBuf<uint32_t> d_qk, d_kid, d_dk, d_nsimk, d_drk, d_drk2, d_roff, d_nr, d_src, d_ph;
    DevBuf<uint64_t> d_drv, d_drv2, d_cumh, d_cumr, d_qh, d_qrn;
    DevBuf<RankRec> d_rec;
    template <class F> void each(F &f) {
        f(d_kflag); f(d_qk); f(d_kid); f(d_dk); f(d_nsimk); f(d_drk); f(d_drk2); f(d_roff); f(d_nr); f(d_src); f(d_ph); f(d_drv); f(d_drv2); f(d_cumh); f(d_cumr);
        f(d_qh); f(d_qrn); f(d_rec);
    }
};
UC_LISTS_EVERY_BUFFER(PlanScratch, 18);
// merge_hits_dev: the output of the sorted-run merge (d_mkey / d_mval; d_mval also carries the diagonals where they must not be overwritten in place);
// prefilter_chunks / prefilter_exhaustive: the running top-M accumulator and the lists of the pass or tile, swapped in and out of the engine
struct MergeScratch {
    DevBuf<uint64_t> d_mkey;
    DevBuf<int32_t> d_mval;
    DevBuf<uint32_t> acc_q, acc_t, pass_q, pass_t;
    DevBuf<int32_t> acc_s, acc_d, pass_s, pass_d;
    template <class F> void each(F &f) { f(d_mkey); f(d_mval); f(acc_q); f(acc_t); f(pass_q); f(pass_t); f(acc_s); f(acc_d); f(pass_s); f(pass_d); }
};
UC_LISTS_EVERY_BUFFER(MergeScratch, 10);
UC_LISTS_EVERY_BUFFER(UngappedAllWork, 5);      // (uc_engine.h; listed by PrefilterScratch::each below)
#undef UC_LISTS_EVERY_BUFFER

// work buffers of the prefilter, kept by the engine between calls (hipMalloc / hipFree of multi-GB buffers on every
// call cost tens of ms per step and, now and then, seconds)
struct PrefilterScratch {
    SharedScratch shared;
    IndexScratch index;
    BatchScratch batch;
    SelectScratch sel;
    CandScratch cand;
    PlanScratch plan;
    MergeScratch merge;
    UngappedAllWork ua;             // rule UC-1/X: the score / diagonal tile, the query pairs and the long-class profiles (kept like everything here)
    // every buffer (for the size bookkeeping below), in a FIXED order: release_bytes frees the first buffer of the largest size in this order, and the
    // UC_TIMING line prints indices into it.  The groups stand in the order of their first buffer in the flat list this struct used to be, and every
    // group keeps that list's order inside (profiles/prefilter_split/README.md: which equal-sized buffers changed places)
    template <class F> void each(F f) {
        shared.each(f); index.each(f); batch.each(f); sel.each(f); cand.each(f); plan.each(f); merge.each(f);
        f(ua.score); f(ua.diag); f(ua.pairs); f(ua.prof); f(ua.prof_off);
    }
    size_t bytes() {
        size_t b = 0;
        each([&](auto &x) { b += x.cap * sizeof(*x.p); });
        return b;
    }
    // Large databases grow this set to well over 100 GB (per-position arrays, run lists, 30 GiB of key regions); the gapped
    // stage sizes its own batches by the memory that is FREE, so above `limit` the big buffers go back before it starts
    // (re-allocating them costs milliseconds per step at a scale where a step takes a minute; small databases keep everything).
    void release_bytes(size_t target) {      // largest buffers first until `target` bytes are back (target >= bytes(): everything of 1 GiB and more, the r01-r05 trim)
        if (getenv("UC_TIMING")) {
            fprintf(stderr, "unicore-cluster[timing]: prefilter scratch %.1f GiB, %.1f GiB to give back before the gapped stage; buffers >= 2 GiB (index in PrefilterScratch::each: GiB):", bytes() / 1073741824.0, target / 1073741824.0);
            int i = 0;
            each([&](auto &x) { const double g = x.cap * sizeof(*x.p) / 1073741824.0; if (g >= 2.0) fprintf(stderr, " %d:%.1f", i, g); i++; });
            fprintf(stderr, "\n");
        }
        if (!target) return;
        if (target >= bytes()) { each([&](auto &x) { if (x.cap * sizeof(*x.p) >= ((size_t)1 << 30)) x.release(); }); return; }
        size_t freed = 0;
        while (freed < target) {
            size_t best = 0;
            each([&](auto &x) { best = std::max(best, x.cap * sizeof(*x.p)); });
            if (best < ((size_t)256 << 20)) break;
            bool done = false;
            each([&](auto &x) { if (!done && x.cap * sizeof(*x.p) == best) { x.release(); done = true; } });
            freed += best;
        }
    }
};

// ---- E1-E4 for ONE target chunk (prefilter_one): a short driver over passes that share this state ----------
constexpr uint64_t RUN_MAX = 1ull << 29;       // runs per batch (the bound of the batches since they had run buffers of their own; kept: it decides the cuts)
struct PrefilterPass {
    KmerCfg cfg;
    KeyFmt fmt;
    uint32_t tbegin = 0, tend = 0;             // the target chunk
    uint32_t qbegin = 0, qend = 0;             // the queries matched against it
    uint32_t mirror_q0 = UINT32_MAX;           // symmetric pass (diag_select_kernel): queries from here on also yield the pair the other way round
    bool count_sims = false;
    double density_limit = 0.0, *density_out = nullptr;
    const void *ent_p = nullptr;               // the chunk's n_entries index entries sorted by k-mer (compact or wide, fmt.compact)
    uint32_t n_entries = 0;
    uint64_t HIT_CAP = 0, HIT_CAP_BIG = 0, DRUN_MAX = 0;
    uint64_t td_queries = 0, td_keys = 0, filt_queries = 0, filt_keys = 0;   // what td_select_kernel took of the filter's queries and survivors (UC_TIMING)
    uint32_t td_cap = 0;                       // td_select_kernel takes the queries with at most this many survivors (0: none, UC_TD_ONCHIP=0)
    uint64_t n_hits_total = 0, n_cand_total = 0, cand_cap = 0;
    double t_kmer = 0, t_ung = 0, t_sel = 0, gpu_ms = 0;   // host seconds of E2 / E3 / E4 and the event time of everything
};
// a query "super-batch" [begin, end) of the chunk with what its plan leaves for the exact batches
struct SuperBatch {
    uint32_t begin = 0, end = 0;
    uint32_t P0 = 0, NP = 0;                   // its residue positions [P0, P0 + NP)
    std::vector<uint64_t> h_qh, h_qr;          // k-mer hits / runs per query of the super-batch
    uint64_t hit_cap = 0;                      // keys per exact batch
    double frac = 1.0;                         // share of the remaining queries to try as the next super-batch
};
// one exact batch of queries [qa, qb): as many as fit the key and run buffers
struct QueryBatch {
    uint32_t qa = 0, qb = 0;
    uint64_t total_hits = 0, n_runs = 0;
    uint32_t qp0 = 0, qp1 = 0, nq_res = 0;     // its residue positions
    uint32_t plan_p0 = 0, plan_q0 = 0;         // first position and first query of its super-batch: the plan's per-position arrays are indexed by position -
                                               // plan_p0, the per-query ones by query - plan_q0
    unsigned kbits = 0;                        // significant bits of its keys [query - qa | target | diagonal]
    const uint64_t *sorted = nullptr;          // the n_sort keys in that order
    uint64_t n_sort = 0;
    uint64_t n_rec = 0;                        // candidates that td_select_kernel left in the query regions (cand_gather_kernel)
};
enum class PlanStatus { planned, too_dense /* density limit exceeded (first super-batch only) */, too_many_runs /* over_runs says how many */ };
struct PlanResult { PlanStatus status; uint64_t over_runs; };

// ---- uc_kmer_match.hip ----
KeyFmt key_format(const Engine &E, uint32_t tbegin, uint32_t tend);
void build_index(Engine &E, PrefilterPass &PP);
dim3 sim_grid(uint64_t items);
uint64_t distinct_runs(Engine &E, PrefilterPass &PP, const SuperBatch &SB, uint32_t nd, uint64_t &n_druns, uint64_t &drun_cap);
PlanResult plan_superbatch(Engine &E, PrefilterPass &PP, SuperBatch &SB, uint32_t sa, uint32_t sb);
bool choose_superbatch(Engine &E, PrefilterPass &PP, SuperBatch &SB, uint32_t qa);
QueryBatch cut_batch(Engine &E, PrefilterPass &PP, const SuperBatch &SB, uint32_t qa);
// ---- uc_kmer_filter.hip ----
uint64_t compact_u64(Engine &E, DevBuf<char> &tmp, uint32_t *cnt, uint64_t *pos, uint64_t n, const uint32_t *also = nullptr, uint32_t *also_out = nullptr);
void expand_keys_filtered(Engine &E, PrefilterPass &PP, QueryBatch &B);
void expand_keys_plain(Engine &E, PrefilterPass &PP, QueryBatch &B);
// ---- uc_diag_select.hip ----
// the two td_select_kernel launches right behind filter_kernel, over the nq query regions of the batch that starts at query qa (compact mode, td_cap > 0)
void launch_td_select(Engine &E, const PrefilterPass &PP, uint32_t qa, uint32_t nq);
uint64_t select_diagonals(Engine &E, PrefilterPass &PP, const QueryBatch &B);
// ---- uc_hit_lists.hip ----
void swap_hits(Engine &E, DevBuf<uint32_t> &q, DevBuf<uint32_t> &t, DevBuf<int32_t> &s, DevBuf<int32_t> &d);
void copy_hits_dev(const Engine &E, uint32_t *dq, uint32_t *dt, int32_t *ds, int32_t *dd);
void rescore_ungapped(Engine &E, PrefilterPass &PP, uint64_t n_cand);
void select_and_append(Engine &E, PrefilterPass &PP, uint64_t n_cand);

}  // namespace uc
