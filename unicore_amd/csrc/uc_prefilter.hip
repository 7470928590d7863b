// uc_prefilter.hip - the driver of stages E1-E4 on the GPU: the k-mer prefilter that stands for the MMseqs2-style prefilter inside `foldseek cluster`
// (algorithm SURVEY.md A.2; spec UC-1 E1-E4).  The passes and their kernels live in four files beside this one (uc_prefilter_internal.h); all of it is
// HBM-bound gather / scan / sort work.  The pipeline of one target chunk (prefilter_one):
//   E1  build_index (uc_kmer_match.hip): (k-mer, sequence, position) per target residue -> radix sort by k-mer -> offsets per k-mer slot (20^6 + 1 u32 =
//       256 MB) and an 8 MB presence bitmap of the k-mers that occur, which answers most lookups at high sensitivity without touching the offset table.
//   E2  plan_superbatch: the similar k-mers (sorted-letter DFS with score bound) and their non-empty index ranges ("runs") are enumerated once per DISTINCT
//       k-mer of a query super-batch and sorted by k-mer rank; per query position the plan keeps where its k-mer's list starts and the running sum of
//       the list lengths.  cut_batch cuts exact batches that fit the key buffers on the plan's per-query totals and copies nothing: the filter reads a
//       query's runs from the lists.  A super-batch whose run lists would exceed DRUN_MAX is cut (choose_superbatch).
//       expand_keys_filtered (uc_kmer_filter.hip): one workgroup per query expands its runs through the same-diagonal double-hit filter in LDS and keeps
//       the (target, diagonal) keys seen twice; min_diag_hits 1 uses a plain expansion (expand_keys_plain).
//       select_diagonals (uc_diag_select.hip): per (query, target) the diagonal with the most hits.  Queries of at most TDS_CAP surviving keys are sorted and
//       evaluated on chip right behind the filter (td_select_kernel); only the rest goes through the batch's radix sort and diag_select_kernel.
//   E3  rescore_ungapped (uc_hit_lists.hip): ungapped diagonal score per candidate.
//   E4  select_and_append: sort by (query, score desc, target), rank inside the query's run < max_seqs, scatter into the device-resident hit lists.
// A target range larger than prefilter_chunk_residues is indexed in chunks (prefilter_chunks): one pass per chunk, the per-query lists merged on the
// device into a running top-M accumulator; a chunk whose first batch shows more than 400 k-mer hits per query residue is abandoned and the range re-cut
// (-s 7.5).  All-vs-all under a symmetric matrix runs only the upper triangle of the chunk x chunk grid: the pass over chunk c matches the queries from
// c onwards, and the pairs with the query behind the chunk also yield the candidate of the pair the other way round (mirror_q0).
// --prefilter-mode 1 (prefilter_exhaustive, rule UC-1/X) has no E1 / E2: every (query, target) pair of a tile is scored on every diagonal
// (uc_ungapped_all.hip), the pairs that pass --min-ungapped-score go through E4 and the tiles' lists into the same accumulator.
// Before the gapped stage starts, the scratch of all this goes back as far as scratch_release_target asks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "uc_prefilter_internal.h"

namespace uc {

void free_scratch(PrefilterScratch *p) { delete p; }

// the prefilter's work buffers stay allocated between steps (re-allocating the 34 GiB key regions alone costs a second per
// step at configs[1]) unless they hold more than 40 % of the device memory: then the gapped stage, which sizes its batches by
// the free memory, gets them back (2.5 M sequences: 170 GB)
// r06: the 40 % rule only where the gapped stage really sizes something by the free memory - the traceback-byte matrices of --min-seq-id / search (MODE 7).
// Without them the gapped stage needs ~150 B per pair of a 256 M-pair batch and nothing else: the prefilter's buffers stay up to 65 % of the device, and if
// that is ever too much the stage's out-of-memory handler gives them back (Engine::relieve_pressure).  Why it matters: releasing ~100 GB after every pass
// means allocating them again in the next one, and on a box whose device memory has not been touched since it came up that costs seconds PER PASS for as long
// as untouched memory is left (configs[2], first process on such a box: prefilter 9.2 s instead of 5.3 s per pass - profiles/r06/c3_first_process.txt).
// -> bytes of the prefilter's buffers to give back before the gapped stage starts (0 = keep everything)
static size_t scratch_release_target(bool gapped_stage_sizes_by_free_memory, uint64_t n_hits, size_t scratch_bytes, bool gapped_scratch_warm) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || tot == 0) return scratch_bytes > ((size_t)96 << 30) ? scratch_bytes : 0;
    if (gapped_stage_sizes_by_free_memory) return scratch_bytes > (size_t)((double)tot * 0.4) ? scratch_bytes : 0;       // the 40 % rule of r01-r05: everything >= 1 GiB
    // ... otherwise only what the gapped stage will not fit beside: its plans and pass arrays take up to ~600 B per pair of a 256 M-pair batch (measured at
    // configs[2]: it ran out of memory beside 133 GiB of kept buffers with 126 GiB free) + 44 B of records per listed pair.  Kept buffers that the stage's
    // out-of-memory handler has to take back after all cost more than releasing them here: the block allocated right behind a 130 GiB release waits seconds
    // for it (configs[2]: 41.4 s per pass instead of 33.3, profiles/r06/c3_memory_edge.txt).  The largest buffers go first, only as many as needed.
    // (warm: the gapped stage still holds the buffers of a call at least this large - repeated steps, the shrinking rounds of a cascade: only the margin)
    const size_t need = gapped_scratch_warm ? ((size_t)8 << 30)
                                            : (size_t)600 * (size_t)std::min<uint64_t>(n_hits, 256ull << 20) + (size_t)44 * (size_t)n_hits + ((size_t)8 << 30);
    return fr >= need ? 0 : std::min(scratch_bytes, need - fr);
}
// gives prefilter scratch back before the gapped stage starts on the installed lists, as far as the rule above asks
static void release_scratch_for_gapped_stage(Engine &E) {
    if (!E.pre) return;
    E.pre->release_bytes(scratch_release_target(E.p.min_seq_id > 0.0f || E.p.want_tb, E.n_hits, E.pre->bytes(),
                                                E.aln != nullptr && (double)E.last_align_hits >= 0.9 * (double)E.n_hits));
}

// consumes the totals of the chunk; produces the per-query counts / offsets (unless the lists leave ungrouped) and the chunk's share of the statistics
static void finish_chunk(Engine &E, const PrefilterPass &PP, uint64_t sims_before) {
    if (PP.mirror_q0 == UINT32_MAX) E.finish_hit_lists("prefilter");
    if (getenv("UC_TIMING") && PP.filt_queries)
        fprintf(stderr, "unicore-cluster[timing]: on-chip diagonal selection (cap %u): %llu of %llu queries, %llu of %llu surviving keys\n", PP.td_cap,
                (unsigned long long)PP.td_queries, (unsigned long long)PP.filt_queries, (unsigned long long)PP.td_keys, (unsigned long long)PP.filt_keys);
    uc_stats &stats = E.stats;
    unsigned long long ovl = 0;
    UC_HIP(hipMemcpy(&ovl, E.pre->shared.d_counters.p + 2, 8, hipMemcpyDeviceToHost));
    stats.n_kmer_hits += PP.n_hits_total;
    stats.n_candidates += PP.n_cand_total;
    stats.algorithmic_bytes[UC_ST_KMER] += 8ull * (stats.n_sim_kmers - sims_before) + 6ull * PP.n_hits_total + 8ull * PP.n_cand_total;
    stats.algorithmic_bytes[UC_ST_UNGAPPED] += ovl + 16ull * PP.n_cand_total;   // (overlap + 16) B per candidate, SURVEY.md 8(d)
    stats.algorithmic_bytes[UC_ST_SELECT] += 16ull * PP.n_cand_total;
    stats.stage_seconds[UC_ST_KMER] += PP.t_kmer;
    stats.stage_seconds[UC_ST_UNGAPPED] += PP.t_ung;
    stats.stage_seconds[UC_ST_SELECT] += PP.t_sel;
    stats.prefilter_kernel_ms += PP.gpu_ms;
}

// one target chunk [tbegin, tend) against queries [qbegin, qend).  Returns false (nothing installed) if density_limit > 0 and the first query batch
// exceeds it; *density_out = k-mer hits per query residue of that batch.  mirror_q0 != UINT32_MAX: symmetric pass (diag_select_kernel): the lists
// leave this function ungrouped, the caller merges them
static bool prefilter_one(Engine &E, uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend, bool count_sims, double density_limit,
                          double *density_out, uint32_t mirror_q0) {
    UC_HIP(hipSetDevice(E.device));
    const uint32_t n = E.hdb.n;
    PrefilterPass PP;
    for (int m = 0; m < K; m++) PP.cfg.koff[m] = E.p.koff[m];
    PP.cfg.span = E.p.span; PP.cfg.thr = E.p.kmer_thr;
    PP.tbegin = tbegin; PP.tend = tend; PP.qbegin = qbegin; PP.qend = qend; PP.mirror_q0 = mirror_q0;
    PP.count_sims = count_sims; PP.density_limit = density_limit; PP.density_out = density_out;
    // keys per batch (the filter's regions hold < 2^32 keys).  1.5 G keys = 12 GiB of regions: a one-shot `foldseek cluster` process
    // pays for every byte it allocates (34 GiB of regions at 3.75 G keys: 5.2 s from process start to clust.tsv at configs[1]
    // instead of 1.25 s), and a resident engine loses nothing measurable (681 vs 681 ms per step; UC_HIT_CAP overrides)
    const char *hc = getenv("UC_HIT_CAP");
    PP.HIT_CAP = hc ? std::max<uint64_t>(1u << 20, strtoull(hc, nullptr, 10)) : (3ull << 29);
    // ... unless the chunk has so many hits that the batches would run into the hundreds (2.5 M sequences: 1.5e12 hits): then the
    // per-batch costs outweigh the allocation and the regions take 3.75 G keys (30 GiB)
    PP.HIT_CAP_BIG = hc ? PP.HIT_CAP : (15ull << 28);
    const char *dm = getenv("UC_DRUN_MAX");
    PP.DRUN_MAX = dm ? std::max<uint64_t>(1, strtoull(dm, nullptr, 10)) : (1ull << 31);   // 24 GiB + 24 GiB sort double buffer (env: tests)
    // UC_TD_ONCHIP=0: every query through the batch sort (A/B runs); UC_TD_ONCHIP_CAP=<keys>: a lower cap, rounded down to a power of two >= 64 (tests)
    const char *to = getenv("UC_TD_ONCHIP"), *tc = getenv("UC_TD_ONCHIP_CAP");
    PP.td_cap = to && atoi(to) == 0 ? 0u : TDS_CAP;
    if (PP.td_cap && tc) {
        const uint64_t want = strtoull(tc, nullptr, 10);
        uint32_t c = 64;
        while (c < TDS_CAP && 2ull * c <= want) c *= 2;
        PP.td_cap = c;
    }

    E.hit_cnt.assign(n, 0);
    E.hit_off.assign((size_t)n + 1, 0);
    E.n_hits = 0;
    E.alns_valid = false;
    E.clear_edges();
    const uint64_t sims_before = E.stats.n_sim_kmers;   // stats accumulate over calls: the byte count below needs THIS call's share

    if (n > (1u << 24)) fail(UC_ERR_GENERIC, "prefilter: %u sequences exceed the 2^24 limit of the hit keys", n);
    // the eight counters of the pass (legend and who zeroes which: uc_prefilter_internal.h)
    if (!E.pre) E.pre = ParkedScratch<PrefilterScratch>::take_or_new(E.device);
    E.pre->shared.d_counters.reserve(8);
    UC_HIP(hipMemsetAsync(E.pre->shared.d_counters.p, 0, 64, E.stream));

    build_index(E, PP);                        // E1: index of targets [tbegin, tend)
    // E2-E4 over query batches
    SuperBatch SB;
    SB.begin = SB.end = qbegin;                // nothing planned yet
    for (uint32_t qa = qbegin; qa < qend;) {
        if (qa >= SB.end && !choose_superbatch(E, PP, SB, qa)) return false;
        Timer t_b;
        E.timed_ms_begin();
        QueryBatch B = cut_batch(E, PP, SB, qa);
        uint64_t n_cand = 0;
        if (B.total_hits) {
            // pass 2: expand runs into keys (filtered to double hits when the rule allows), sort them
            if (E.p.min_diag_hits >= 2 && B.total_hits < (1ull << 32)) expand_keys_filtered(E, PP, B);
            else expand_keys_plain(E, PP, B);
            n_cand = select_diagonals(E, PP, B);
        }
        UC_HIP(hipGetLastError());
        PP.gpu_ms += E.timed_ms_end();
        PP.t_kmer += t_b.seconds();
        PP.n_cand_total += n_cand;
        if (n_cand) {
            rescore_ungapped(E, PP, n_cand);
            select_and_append(E, PP, n_cand);
        }
        qa = B.qb;
    }
    finish_chunk(E, PP, sims_before);
    return true;
}

// ---- E1-E4 for a target range ---------------------------------------------------------------------------------
// The chunks of a range, one prefilter_one pass each, their lists merged into a running top-M accumulator; false: the first chunk was too dense
// (density says by how much), nothing is installed.
// All-vs-all over several chunks under a symmetric matrix (triangle): the k-mer hit relation is symmetric, so the chunk x chunk grid needs only its
// upper triangle.  The pass over chunk c matches the queries FROM chunk c onwards; the pairs (query behind the chunk, target in it) also
// yield the candidates of the pairs the other way round (diag_select_kernel), i.e. what the skipped passes (query in c, target chunk
// behind it) would have found: ~(1 + 1/C) / 2 of the k-mer hits are expanded.  The lists of a pass come back ungrouped and are merged
// like the chunk lists always were (lossless: per-pass top-M of disjoint candidate sets).  UC_PREFILTER_SYMMETRIC=0: every pass matches all queries.
static bool prefilter_chunks(Engine &E, const std::vector<std::pair<uint32_t, uint32_t>> &chunks, uint32_t qbegin, uint32_t qend, bool triangle,
                             bool mirror_all, double limit, double *density) {
    // (Measured and reverted in r04: concatenating the per-pass lists and merging ONCE at the end — 1.5-2 G records in one sort instead of a
    // running top-M accumulator of <= max_seqs x queries — made configs[2] SLOWER, 35.7 -> 39.3 s per pass: the single merge needs ~64 B per
    // record of work buffers at the moment the key regions are largest.  The accumulator is merged after every pass.)
    // (r06: the accumulator / pass arrays live in the scratch set - up to 4 x 7 GB at configs[2] were allocated and freed by every call)
    if (!E.pre) E.pre = ParkedScratch<PrefilterScratch>::take_or_new(E.device);
    PrefilterScratch &S = *E.pre;
    const auto swap_acc = [&] { swap_hits(E, S.merge.acc_q, S.merge.acc_t, S.merge.acc_s, S.merge.acc_d); };
    uint64_t acc_n = 0;
    bool installed = false;       // the last pass's merge leaves its result installed in the engine: no second merge of the accumulator
    for (size_t c = 0; c < chunks.size(); c++) {
        const bool mir = mirror_all || (triangle && c + 1 < chunks.size());       // (the last chunk has no queries behind it: a plain pass over its own queries)
        if (!prefilter_one(E, chunks[c].first, chunks[c].second, triangle ? chunks[c].first : qbegin, qend, c == 0, c == 0 ? limit : 0.0, density,
                           mirror_all ? qbegin : mir ? chunks[c].second : UINT32_MAX))
            return false;
        if (!mir && (c == 0 || acc_n == 0)) {
            swap_acc();
            acc_n = E.n_hits;
        } else if (E.n_hits) {       // (a mirrored pass always comes here: its lists are ungrouped)
            // the pass's lists leave the engine (swap, no copy), the merge installs accumulator + pass in their place.  The accumulator is in key
            // order, a plain pass's lists are too: only a mirrored pass's records are sorted before the two runs are merged (merge_hits_dev)
            const uint64_t n_pass = E.n_hits;
            swap_hits(E, S.merge.pass_q, S.merge.pass_t, S.merge.pass_s, S.merge.pass_d);
            acc_n = E.merge_hits_dev(acc_n, S.merge.acc_q.p, S.merge.acc_t.p, S.merge.acc_s.p, S.merge.acc_d.p, n_pass, S.merge.pass_q.p, S.merge.pass_t.p, S.merge.pass_s.p, S.merge.pass_d.p, /*sorted2=*/!mir, 0, 1);      // merge + truncate to max_seqs
            if (c + 1 == chunks.size()) installed = true;
            else swap_acc();
        }
    }
    // install the accumulated lists (also rebuilds the per-query counts) unless the last merge already did
    if (!installed) E.merge_hits_dev(acc_n, S.merge.acc_q.p, S.merge.acc_t.p, S.merge.acc_s.p, S.merge.acc_d.p, 0, nullptr, nullptr, nullptr, nullptr, true, 0, 1);     // (in key order already: counts only)
    return true;
}

// ---- rule UC-1/X (--prefilter-mode 1): E3x on every (query, target) pair of the ranges instead of E1/E2 ------------------------------------
// Tiles of (query batch x target chunk) under the byte budget UNGAPPED_ALL_TILE_BYTES (uc_ungapped_all.hip): the pairs of a tile that pass
// --min-ungapped-score go through the E4 selection of the k-mer path (sort, rank, truncate to max_seqs per query) and the tile's lists are merged
// into the running top-M accumulator of the chunked k-mer path (lossless: the tiles' pair sets are disjoint).
static void prefilter_exhaustive(Engine &E, uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend) {
    UC_HIP(hipSetDevice(E.device));
    if (E.hdb.n > (1u << 24)) fail(UC_ERR_GENERIC, "prefilter: %u sequences exceed the 2^24 limit of the hit keys", E.hdb.n);
    logf(3, "unicore-cluster: --prefilter-mode 1: all %u x %u pairs are scored on every diagonal; --k-score, --min-diag-hits and -s have no effect\n", qend - qbegin, tend - tbegin);
    if (!E.pre) E.pre = ParkedScratch<PrefilterScratch>::take_or_new(E.device);
    PrefilterScratch &S = *E.pre;
    S.shared.d_counters.reserve(8);
    UC_HIP(hipMemsetAsync(S.shared.d_counters.p, 0, 64, E.stream));
    uint64_t budget = UNGAPPED_ALL_TILE_BYTES;
    if (const char *ev = getenv("UC_UNGAPPED_TILE_BYTES")) budget = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    uint32_t QB = 1, TC = 1;
    ungapped_all_plan(budget, qend - qbegin, tend - tbegin, &QB, &TC);
    UngappedAllWork &W = S.ua;
    PrefilterPass PP;
    bool installed = false;       // the last tile's merge left accumulator + tile installed in the engine: no second pass over the accumulator at the end
    const auto swap_acc = [&] { swap_hits(E, S.merge.acc_q, S.merge.acc_t, S.merge.acc_s, S.merge.acc_d); };
    uint64_t acc_n = 0, cells = 0;
    for (uint32_t qa = qbegin; qa < qend; qa += std::min(QB, qend - qa))
        for (uint32_t ta = tbegin; ta < tend; ta += std::min(TC, tend - ta)) {
            const uint32_t nq = std::min(QB, qend - qa), nt = std::min(TC, tend - ta);
            const uint64_t np = (uint64_t)nq * nt;
            Timer t_u;
            E.timed_ms_begin();
            ungapped_all_tile(E, W, qa, qa + nq, ta, ta + nt);
            S.cand.d_cq.reserve(np); S.cand.d_ct.reserve(np); S.sel.d_score.reserve(np); S.cand.d_cd.reserve(np);
            const uint64_t n_cand = ungapped_all_candidates(E, W, qa, nq, ta, nt, E.p.min_ungapped, S.cand.d_cq.p, S.cand.d_ct.p, S.sel.d_score.p, S.cand.d_cd.p, S.shared.d_counters.p + 6);
            PP.gpu_ms += E.timed_ms_end();
            PP.t_ung += t_u.seconds();
            PP.n_cand_total += np;
            for (uint32_t q = qa; q < qa + nq; q++) cells += (uint64_t)E.h_len[q] * (uint64_t)(E.h_poff[ta + nt] - E.h_poff[ta]);   // (padded target residues: an upper bound)
            if (!n_cand) continue;
            if (installed) { swap_acc(); installed = false; }       // the installed lists are the accumulator again
            E.n_hits = 0;
            select_and_append(E, PP, n_cand);
            if (!E.n_hits) continue;
            if (!acc_n) { swap_acc(); acc_n = E.n_hits; E.n_hits = 0; continue; }
            const uint64_t n_pass = E.n_hits;
            swap_hits(E, S.merge.pass_q, S.merge.pass_t, S.merge.pass_s, S.merge.pass_d);
            acc_n = E.merge_hits_dev(acc_n, S.merge.acc_q.p, S.merge.acc_t.p, S.merge.acc_s.p, S.merge.acc_d.p, n_pass, S.merge.pass_q.p, S.merge.pass_t.p, S.merge.pass_s.p, S.merge.pass_d.p, /*sorted2=*/true, 0, 1);
            installed = true;
        }
    // installs the accumulated lists and rebuilds the per-query counts (an empty accumulator: empty lists) unless the last merge already did
    if (!installed) E.merge_hits_dev(acc_n, S.merge.acc_q.p, S.merge.acc_t.p, S.merge.acc_s.p, S.merge.acc_d.p, 0, nullptr, nullptr, nullptr, nullptr, true, 0, 1);
    uc_stats &st = E.stats;
    st.n_candidates += PP.n_cand_total;
    st.n_prefilter_hits += E.n_hits;
    st.algorithmic_bytes[UC_ST_UNGAPPED] += cells / 64 + 5ull * PP.n_cand_total;      // a target residue is read once per wave (64 diagonals) + the tile bytes
    st.algorithmic_bytes[UC_ST_SELECT] += 16ull * PP.n_cand_total;
    st.stage_seconds[UC_ST_UNGAPPED] += PP.t_ung;
    st.stage_seconds[UC_ST_SELECT] += PP.t_sel;
    st.prefilter_kernel_ms += PP.gpu_ms;
    release_scratch_for_gapped_stage(E);
}

// Large ranges are processed as several index chunks whose per-query top-M lists are
// merged on the device (lossless, same argument as the multi-GPU shards): the double-hit filter keeps one query's
// (target, diagonal) hashes in 2 x 2^19 LDS bits, which only works while a query has well under ~500 k k-mer hits,
// i.e. up to ~100 M target residues per chunk at default sensitivity (at 760 M residues in one chunk 75 % of the
// hits survived the filter and the key sort took 2/3 of the run).
// (mirror_all — prefilter_cells only: every query lies outside the shard and yields the pair the other way round as well; the lists come
// back ungrouped and are merged by the caller)
static void prefilter_impl(Engine &E, uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend, bool mirror_all) {
    Engine::PressureScope ps(E, 0);
    if (!E.have_db) fail(UC_ERR_ARGS, "no database loaded");
    if (tbegin > tend || tend > E.hdb.n) fail(UC_ERR_ARGS, "prefilter: bad target range");
    if (qend == UINT32_MAX) qend = E.hdb.n;
    if (qbegin > qend || qend > E.hdb.n) fail(UC_ERR_ARGS, "prefilter: bad query range");
    if (E.p.prefilter_mode == 1) {      // rule UC-1/X: no k-mer stage, no chunk index, no mirror
        if (mirror_all) fail(UC_ERR_GENERIC, "prefilter: --prefilter-mode 1 has no mirrored pass");
        prefilter_exhaustive(E, tbegin, tend, qbegin, qend);
        return;
    }
    uint64_t chunk_res = E.prefilter_chunk_residues;
    if (const char *ev = getenv("UC_PREFILTER_CHUNK_RES")) chunk_res = std::max<uint64_t>(1, strtoull(ev, nullptr, 10));
    const char *sym = getenv("UC_PREFILTER_SYMMETRIC");
    const bool symmetric = E.p.mat_symmetric && !(sym && atoi(sym) == 0);
    // The chunk size that keeps a query's hits inside the LDS filter depends on how many k-mer hits a target residue
    // attracts, i.e. on the sensitivity (-s 7.5 gives ~30x the hits of the default 4): prefilter_one measures the density
    // (k-mer hits per query residue) of its first batch and gives up before expanding anything if the chunk is too dense;
    // the range is then re-cut into proportionally smaller chunks (one wasted enumeration pass).
    const double DENSITY_LIMIT = 400.0;   // hits per query residue and chunk (C2 whole DB at -s 4: 124)
    for (int attempt = 0;; attempt++) {
        std::vector<std::pair<uint32_t, uint32_t>> chunks;
        for (uint32_t b = tbegin; b < tend;) {
            uint32_t e = b;
            uint64_t res = 0;
            while (e < tend && (e == b || res + E.h_len[e] <= chunk_res)) res += E.h_len[e++];
            chunks.emplace_back(b, e);
            b = e;
        }
        double density = 0;
        const double limit = attempt < 6 ? DENSITY_LIMIT : 0.0;      // after 6 re-cuts: run with what we have
        const bool triangle = chunks.size() > 1 && tbegin == qbegin && tend == qend && symmetric;
        const bool ok = chunks.size() <= 1 ? prefilter_one(E, tbegin, tend, qbegin, qend, true, limit, &density, mirror_all ? qbegin : UINT32_MAX)
                                           : prefilter_chunks(E, chunks, qbegin, qend, triangle, mirror_all, limit, &density);
        if (ok) {
            E.stats.n_prefilter_hits += E.n_hits;
            if (chunks.size() > 1 || !mirror_all) release_scratch_for_gapped_stage(E);
            return;
        }
        // too dense: smaller chunks, proportionally (and a little more)
        const uint64_t cur = std::min<uint64_t>(chunk_res, std::max<uint64_t>(1, (uint64_t)E.h_poff[chunks[0].second] - E.h_poff[chunks[0].first]));
        chunk_res = std::max<uint64_t>(1u << 16, (uint64_t)((double)cur * DENSITY_LIMIT / density * 0.75));
        logf(3, "unicore-cluster: prefilter: %.0f k-mer hits per query residue in a chunk of %llu residues; re-cutting the targets into chunks of %llu\n",
             density, (unsigned long long)cur, (unsigned long long)chunk_res);
    }
}

void Engine::prefilter(uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend) { prefilter_impl(*this, tbegin, tend, qbegin, qend, false); }

// A rank of a symmetric N-rank pass: the shard's own block (with its inner triangle if it spans several chunks) and one mirrored block per other
// query range; the lists of the blocks (disjoint candidate sets, each truncated to its own top-M) are concatenated and merged once.
void Engine::prefilter_cells(uint32_t tbegin, uint32_t tend, const std::vector<std::pair<uint32_t, uint32_t>> &others) {
    PressureScope ps(*this, 0);
    DevBuf<uint32_t> cq, ct;
    DevBuf<int32_t> cs, cd;
    uint64_t cat_n = 0;
    auto take = [&]() {       // append the engine's current lists (grouped or not) to the accumulator
        if (!n_hits) return;
        const uint64_t tot = cat_n + n_hits;
        cq.grow_preserve(tot, cat_n, stream); ct.grow_preserve(tot, cat_n, stream); cs.grow_preserve(tot, cat_n, stream); cd.grow_preserve(tot, cat_n, stream);
        copy_hits_dev(*this, cq.p + cat_n, ct.p + cat_n, cs.p + cat_n, cd.p + cat_n);
        cat_n = tot;
    };
    const uint64_t before = stats.n_prefilter_hits;
    prefilter_impl(*this, tbegin, tend, tbegin, tend, false);
    take();
    for (const auto &r : others) {
        if (r.first >= r.second) continue;
        if (r.first < tend && r.second > tbegin) fail(UC_ERR_GENERIC, "prefilter_cells: a mirrored query range overlaps the target shard");
        prefilter_impl(*this, tbegin, tend, r.first, r.second, true);
        take();
    }
    const uint64_t kept = import_hits_dev(cat_n, cq.p, ct.p, cs.p, cd.p, 0, 1);
    stats.n_prefilter_hits = before + kept;
    release_scratch_for_gapped_stage(*this);
}

}  // namespace uc
