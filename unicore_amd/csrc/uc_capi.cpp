// uc_capi.cpp — extern "C" boundary (include/unicore_cluster.h).  No exception crosses it: every entry
// point converts failures into the status classes of the header and records uc_last_error().  What a uc_cluster
// run does is not written here: the workflow lives in uc_workflow.cpp.
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>

#include "uc_engine.h"
#include "uc_files.h"
#include "uc_multi.h"
#include "uc_t5.h"
#include "uc_workflow.h"

using namespace uc;

struct uc_comm {
    Comm c;
};
struct uc_t5 {
    T5Model m;
};

namespace {

void require(const void *p, const char *what) {
    if (!p) fail(UC_ERR_ARGS, "%s must not be NULL", what);
}

// ---- the encoder's kernel-level entry points: one call = one device, buffers freed on every exit path
constexpr const char *T5_NO_FALLBACK = "the ProstT5 kernels have no CPU fallback";

struct DevBufs {
    std::vector<void *> p;
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() { for (void *q : p) (void)hipFree(q); }
    template <typename T = void> T *alloc(size_t bytes) {
        void *q = nullptr;
        UC_HIP(hipMalloc(&q, std::max<size_t>(bytes, 16)));
        p.push_back(q);
        return (T *)q;
    }
    template <typename T> T *up(const T *src, size_t n) {
        T *q = alloc<T>(n * sizeof(T));
        UC_HIP(hipMemcpy(q, src, n * sizeof(T), hipMemcpyHostToDevice));
        return q;
    }
    // an output every element of which the kernel must write: filled with 0xff (NaN as f16 / fp32) so that a missed one shows
    template <typename T> T *out(size_t n) {
        T *q = alloc<T>(n * sizeof(T));
        UC_HIP(hipMemset(q, 0xff, n * sizeof(T)));
        return q;
    }
};

void t5_finish() {
    UC_HIP(hipGetLastError());
    UC_HIP(hipDeviceSynchronize());
}

// packed sequence lengths -> token offsets (n + 1); every length >= min_len
std::vector<int32_t> t5_offsets(int32_t n_seqs, const int32_t *seq_len, int32_t min_len, int32_t *max_len) {
    if (n_seqs < 1) fail(UC_ERR_ARGS, "n_seqs must be >= 1");
    require(seq_len, "seq_len");
    std::vector<int32_t> off((size_t)n_seqs + 1, 0);
    int64_t t = 0;
    *max_len = 0;
    for (int32_t i = 0; i < n_seqs; i++) {
        if (seq_len[i] < min_len) fail(UC_ERR_ARGS, "seq_len[%d] = %d < %d", i, seq_len[i], min_len);
        t += seq_len[i];
        if (t > (1 << 28)) fail(UC_ERR_ARGS, "more than 2^28 tokens");
        off[(size_t)i + 1] = (int32_t)t;
        *max_len = std::max(*max_len, seq_len[i]);
    }
    return off;
}

}  // namespace

extern "C" {

const char *uc_last_error(void) { return last_error_cstr(); }
const char *uc_version(void) {
    // says which 3Di matrix a run without --mat3di would use: results with the stand-in are not Foldseek's
    static thread_local std::string v;
    struct stat st;
    const bool real = stat((default_data_dir() + "/mat3di.out").c_str(), &st) == 0;
    v = std::string("unicore-cluster-mi355x 0.2.0 (spec UC-1.1, gfx950; default workflow: linclust pre-step + 3-step cascade; 3Di matrix: ") +
        (real ? "data/mat3di.out" : "MISSING - only the synthetic stand-in is shipped, runs need UC_ALLOW_SYNTHETIC=1 or --mat3di") + ")";
    return v.c_str();
}

uint32_t uc_abi_version(void) { return UC_ABI_VERSION; }
size_t uc_stats_size(void) { return sizeof(uc_stats); }
void uc_set_round_hook(uc_round_hook hook, void *user) { set_round_hook(hook, user); }

int uc_option_arity(const char *flag) { return flag ? option_arity(flag) : -1; }

void uc_release_scratch(void) {
    for (int d = 0; d < 16; d++) {
        free_scratch(ParkedScratch<PrefilterScratch>::take(d));
        free_scratch(ParkedScratch<AlignScratch>::take(d));
    }
}

int uc_check_options(const char *cluster_options) {
    return guard([&] { Params p; parse_cluster_options(cluster_options ? cluster_options : "", p); });
}

int uc_engine_create(const uc_opts *o, uc_engine **out) {
    return guard([&] {
        require(out, "out");
        *out = nullptr;
        Params p = params_from(o);
        if (p.want_bt) p.want_tb = 1;
        auto h = std::make_unique<uc_engine>();
        h->e = std::make_unique<Engine>(p, o ? o->device : -1);
        h->e->emit_bt = p.want_bt != 0;      // the staged API reads them back (uc_engine_backtraces_get)
        *out = h.release();
    });
}

void uc_engine_destroy(uc_engine *e) { delete e; }

int uc_engine_load_db(uc_engine *e, const char *db_prefix) {
    return guard([&] {
        require(e, "engine"); require(db_prefix, "db_prefix");
        Timer tm;
        read_seq_db(db_prefix, e->e->hdb, true);
        e->e->stats.stage_seconds[UC_ST_LOAD] += tm.seconds();
        e->e->upload_db();
    });
}

int uc_engine_set_db(uc_engine *e, uint32_t n, const uint64_t *off, const uint8_t *s3, const uint8_t *sa) {
    return guard([&] {
        require(e, "engine"); require(off, "off");
        if (n >= (1u << 24)) fail(UC_ERR_ARGS, "this build supports < 2^24 sequences");
        HostDb &d = e->e->hdb;
        d = HostDb();
        d.n = n;
        d.off.assign(off, off + n + 1);
        if (d.off[0] != 0) fail(UC_ERR_ARGS, "off[0] must be 0");
        for (uint32_t i = 0; i < n; i++) {
            if (d.off[i + 1] < d.off[i]) fail(UC_ERR_ARGS, "offsets must be non-decreasing");
            if (d.off[i + 1] - d.off[i] > 65535) fail(UC_ERR_ARGS, "sequence %u longer than 65535", i);
        }
        const uint64_t tot = d.off[n];
        if (tot) { require(s3, "s3"); require(sa, "sa"); }
        d.s3.assign(s3, s3 + tot);
        d.sa.assign(sa, sa + tot);
        for (uint64_t k = 0; k < tot; k++)
            if (d.s3[k] > 20 || d.sa[k] > 20) fail(UC_ERR_ARGS, "sequence codes must be in 0..20");
        d.keys.resize(n);
        for (uint32_t i = 0; i < n; i++) d.keys[i] = i;
        e->e->upload_db();
    });
}

uint32_t uc_engine_num_seqs(const uc_engine *e) { return e && e->e ? e->e->hdb.n : 0; }

int uc_engine_prefilter(uc_engine *e, uint32_t tbegin, uint32_t tend) {
    return guard([&] { require(e, "engine"); e->e->prefilter(tbegin, tend); });
}

int uc_engine_prefilter_range(uc_engine *e, uint32_t tbegin, uint32_t tend, uint32_t qbegin, uint32_t qend) {
    return guard([&] { require(e, "engine"); e->e->prefilter(tbegin, tend, qbegin, qend); });
}

int uc_engine_hits_size(const uc_engine *e, uint64_t *n_hits) {
    return guard([&] { require(e, "engine"); require(n_hits, "n_hits"); *n_hits = e->e->n_hits; });
}

int uc_engine_hits_get(const uc_engine *e, uint32_t *counts, uc_hit *hits) {
    return guard([&] {
        require(e, "engine");
        const Engine &E = *e->e;
        if (counts && E.hdb.n) memcpy(counts, E.hit_cnt.data(), (size_t)E.hdb.n * 4);
        if (hits) E.get_hits(hits);
    });
}

int uc_engine_hits_get_range(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint32_t *counts, uc_hit *hits) {
    return guard([&] {
        require(e, "engine");
        const Engine &E = *e->e;
        if (!E.have_db) fail(UC_ERR_ARGS, "hits_get_range: no database loaded");
        if (qbegin > qend || qend > E.hdb.n) fail(UC_ERR_ARGS, "hits_get_range: bad query range");
        if (counts && qend > qbegin) memcpy(counts, E.hit_cnt.data() + qbegin, (size_t)(qend - qbegin) * 4);
        const uint64_t b = E.hit_off[qbegin], k = E.hit_off[qend] - b;
        if (hits && k) E.get_hits_range(b, k, hits);
    });
}

int uc_hits_merge(uint32_t n_seqs, int32_t max_seqs, int n_parts, const uint32_t *const *counts, const uc_hit *const *hits,
                  uint32_t *out_counts, uc_hit *out_hits, uint64_t out_capacity, uint64_t *out_n) {
    return guard([&] {
        require(counts, "counts"); require(hits, "hits"); require(out_counts, "out_counts"); require(out_n, "out_n");
        if (n_parts < 1 || max_seqs < 1) fail(UC_ERR_ARGS, "n_parts and max_seqs must be >= 1");
        std::vector<uint32_t> c;
        std::vector<uc_hit> h;
        merge_hits(n_seqs, max_seqs, n_parts, counts, hits, c, h);
        *out_n = h.size();
        if (h.size() > out_capacity) fail(UC_ERR_ARGS, "uc_hits_merge: output capacity %llu < %zu", (unsigned long long)out_capacity, h.size());
        if (n_seqs) memcpy(out_counts, c.data(), (size_t)n_seqs * 4);
        if (!h.empty()) { require(out_hits, "out_hits"); memcpy(out_hits, h.data(), h.size() * sizeof(uc_hit)); }
    });
}

int uc_engine_hits_set(uc_engine *e, const uint32_t *counts, const uc_hit *hits) {
    return guard([&] { require(e, "engine"); require(counts, "counts"); e->e->set_hits(counts, hits); });
}

int uc_engine_hits_merge(uc_engine *e, int n_parts, const uint32_t *const *counts, const uc_hit *const *hits) {
    return guard([&] {
        require(e, "engine"); require(counts, "counts"); require(hits, "hits");
        std::vector<uint32_t> c;
        std::vector<uc_hit> h;
        merge_hits(e->e->hdb.n, e->e->p.max_seqs, n_parts, counts, hits, c, h);
        e->e->set_hits(c.data(), h.data());
    });
}

int uc_engine_hits_export_dev(const uc_engine *e, uint32_t *d_query, uint32_t *d_target, int32_t *d_score, int32_t *d_diag) {
    return guard([&] {
        require(e, "engine");
        if (e->e->n_hits) { require(d_query, "d_query"); require(d_target, "d_target"); require(d_score, "d_score"); require(d_diag, "d_diag"); }
        e->e->export_hits_dev(d_query, d_target, d_score, d_diag);
    });
}

int uc_engine_hits_import_dev(uc_engine *e, uint64_t n, const uint32_t *d_query, const uint32_t *d_target, const int32_t *d_score,
                              const int32_t *d_diag, uint32_t rank, uint32_t world, uint64_t *n_kept) {
    return guard([&] {
        require(e, "engine");
        if (n) { require(d_query, "d_query"); require(d_target, "d_target"); require(d_score, "d_score"); require(d_diag, "d_diag"); }
        if (world < 1 || rank >= world) fail(UC_ERR_ARGS, "hits_import_dev: rank %u outside world %u", rank, world);
        const uint64_t k = e->e->import_hits_dev(n, d_query, d_target, d_score, d_diag, rank, world);
        if (n_kept) *n_kept = k;
    });
}

int uc_engine_align(uc_engine *e, uint32_t qbegin, uint32_t qend) {
    return guard([&] { require(e, "engine"); e->e->align(qbegin, qend); });
}

int uc_engine_alns_get(const uc_engine *e, uint32_t qbegin, uint32_t qend, uc_aln *out) {
    return guard([&] {
        require(e, "engine");
        const Engine &E = *e->e;
        if (!E.have_db) fail(UC_ERR_ARGS, "alns_get: no database loaded");
        if (qbegin > qend || qend > E.hdb.n) fail(UC_ERR_ARGS, "alns_get: bad query range");
        const uint64_t b = E.hit_off[qbegin], n = E.hit_off[qend] - b;
        if (n) { require(out, "out"); E.get_alns(b, n, out); }
    });
}

static void backtraces_of(const uc_engine *e, uint32_t qbegin, uint32_t qend, std::vector<uint64_t> &off, std::vector<uint32_t> &runs) {
    require(e, "engine");
    const Engine &E = *e->e;
    if (!E.have_db) fail(UC_ERR_ARGS, "backtraces: no database loaded");
    if (qbegin > qend || qend > E.hdb.n) fail(UC_ERR_ARGS, "backtraces: bad query range");
    const uint64_t b = E.hit_off[qbegin], n = E.hit_off[qend] - b;
    off.assign(n + 1, 0);
    E.get_backtraces(b, n, off.data(), runs);
}

int uc_engine_backtraces_size(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint64_t *n_runs) {
    return guard([&] {
        require(n_runs, "n_runs");
        std::vector<uint64_t> off;
        std::vector<uint32_t> runs;
        backtraces_of(e, qbegin, qend, off, runs);
        *n_runs = runs.size();
    });
}

int uc_engine_backtraces_get(const uc_engine *e, uint32_t qbegin, uint32_t qend, uint64_t *run_off, uint32_t *runs_out) {
    return guard([&] {
        require(run_off, "run_off");
        std::vector<uint64_t> off;
        std::vector<uint32_t> runs;
        backtraces_of(e, qbegin, qend, off, runs);
        memcpy(run_off, off.data(), off.size() * 8);
        if (!runs.empty()) { require(runs_out, "runs"); memcpy(runs_out, runs.data(), runs.size() * 4); }
    });
}

int uc_backtrace_render(const uint32_t *runs, uint64_t n_runs, char *out, uint64_t out_capacity, uint64_t *len_out) {
    return guard([&] {
        if (n_runs) require(runs, "runs");
        const std::string s = render_backtrace(runs, n_runs);
        if (len_out) *len_out = s.size();
        if (s.size() + 1 > out_capacity) fail(UC_ERR_ARGS, "uc_backtrace_render: %zu characters do not fit a buffer of %llu", s.size() + 1, (unsigned long long)out_capacity);
        require(out, "out");
        memcpy(out, s.c_str(), s.size() + 1);
    });
}

int uc_format_output_check(const char *list, uint32_t *n_columns) {
    return guard([&] {
        const std::vector<std::string> c = parse_format_output(list ? list : "");
        if (n_columns) *n_columns = (uint32_t)c.size();
    });
}

int uc_engine_tb_emit_pass(uc_engine *e, int route, int band, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *box, const int32_t *known,
                           int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out, int32_t *plain_out,
                           uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint64_t *n_runs) {
    return guard([&] {
        require(e, "engine"); require(run_off, "run_off");
        if (n_runs) *n_runs = 0;
        run_off[0] = 0;
        if (!n) return;
        require(q, "q"); require(t, "t"); require(box, "box");
        if (route != 2) require(known, "known");
        std::vector<SwPassPair> pairs(n);
        for (uint64_t i = 0; i < n; i++) pairs[i] = {q[i], t[i], box[4 * i], box[4 * i + 1], box[4 * i + 2], box[4 * i + 3], known ? known[i] : 0};
        BtPassOut bt;
        e->e->tb_emit_pass(route, band, pairs, {nullptr, nullptr, nullptr, class_out, aln_len_out, idents_out, gaps_out, miss_out}, bt);
        if (n_runs) *n_runs = bt.runs.size();
        if (bt.runs.size() > runs_capacity) fail(UC_ERR_ARGS, "tb_emit_pass: %zu runs, room for %llu", bt.runs.size(), (unsigned long long)runs_capacity);
        memcpy(run_off, bt.run_off.data(), (n + 1) * 8);
        if (!bt.runs.empty()) { require(runs, "runs"); memcpy(runs, bt.runs.data(), bt.runs.size() * 4); }
        if (plain_out) memcpy(plain_out, bt.plain.data(), n * 4);
    });
}

int uc_engine_edges_size(const uc_engine *e, uint64_t *n_edges) {
    return guard([&] { require(e, "engine"); require(n_edges, "n_edges"); *n_edges = e->e->edges_on_host ? e->e->edges.size() / 2 : e->e->n_edges_dev; });
}

int uc_engine_edges_get(const uc_engine *e, uint32_t *edges) {
    return guard([&] {
        require(e, "engine");
        const std::vector<uint32_t> &h = e->e->host_edges();
        if (!h.empty()) { require(edges, "edges"); memcpy(edges, h.data(), h.size() * 4); }
    });
}

int uc_engine_stats(const uc_engine *e, uc_stats *out) {
    return guard([&] { require(e, "engine"); require(out, "out"); *out = e->e->stats; });
}

void uc_engine_reset_stats(uc_engine *e) {
    if (!e || !e->e) return;
    uc_stats &s = e->e->stats;
    const uint64_t ns = s.n_seqs, nr = s.n_residues;
    memset(&s, 0, sizeof s);
    s.n_seqs = ns; s.n_residues = nr;
    for (uint64_t &x : e->e->td_onchip) x = 0;
    for (uint64_t &x : e->e->sw_task_queries) x = 0;
}

int uc_engine_sw_task_queries(const uc_engine *e, uint64_t *out) {
    return guard([&] { require(e, "engine"); require(out, "out"); for (int i = 0; i < 2; i++) out[i] = e->e->sw_task_queries[i]; });
}

int uc_engine_td_onchip(const uc_engine *e, uint64_t *out) {
    return guard([&] { require(e, "engine"); require(out, "out"); for (int i = 0; i < 4; i++) out[i] = e->e->td_onchip[i]; });
}

int uc_engine_linclust_pairs(uc_engine *e, int32_t m, int32_t install, uint32_t *out_pairs, uint64_t cap, uint64_t *n_out) {
    return guard([&] {
        require(e, "engine"); require(n_out, "n_out");
        if (m > 1000) fail(UC_ERR_ARGS, "uc_engine_linclust_pairs: m must be <= 0 (the engine's --kmer-per-seq) or in [1,1000]");
        if (install != 0 && install != 1) fail(UC_ERR_ARGS, "uc_engine_linclust_pairs: install must be 0 or 1");
        if (cap && !install) require(out_pairs, "out_pairs");
        const int mo = m > 0 ? m : 0;
        if (install) { *n_out = e->e->linclust_hits(mo); return; }
        const std::vector<uint32_t> pr = e->e->linclust_pairs(mo);
        *n_out = pr.size() / 2;
        if (!pr.empty() && pr.size() / 2 <= cap) memcpy(out_pairs, pr.data(), pr.size() * 4);
    });
}

int uc_setcover(uint32_t n, const uint32_t *edges, uint64_t n_edges, uint32_t *assign) {
    return guard([&] {
        if (n) require(assign, "assign");
        if (n_edges) require(edges, "edges");
        set_cover(n, edges, n_edges, assign);
    });
}

int uc_engine_setcover(uc_engine *e, const uint32_t *edges, uint64_t n_edges, uint32_t *assign) {
    return guard([&] {
        require(e, "engine");
        const uint32_t n = e->e->hdb.n;
        if (n) require(assign, "assign");
        if (n_edges) require(edges, "edges");
        Timer tc;
        e->e->set_cover_device(n, edges, n_edges, assign);
        e->e->stats.stage_seconds[UC_ST_SETCOVER] += tc.seconds();
    });
}

int uc_cluster_graph(uint32_t n, const uint32_t *edges, uint64_t n_edges, const uint32_t *len, int32_t mode, uint32_t *assign) {
    return guard([&] {
        if (mode != 0 && mode != 2) fail(UC_ERR_ARGS, "uc_cluster_graph: mode %d unsupported (0 = greedy set cover, 2 = greedy incremental)", mode);
        if (n) require(assign, "assign");
        if (n_edges) require(edges, "edges");
        if (n && mode == 2) require(len, "len");
        cluster_graph(n, edges, n_edges, len, mode, assign);
    });
}

int uc_engine_cluster_graph(uc_engine *e, int32_t mode, const uint32_t *edges, uint64_t n_edges, uint32_t *assign) {
    return guard([&] {
        require(e, "engine");
        if (mode != 0 && mode != 2) fail(UC_ERR_ARGS, "uc_engine_cluster_graph: mode %d unsupported (0 = greedy set cover, 2 = greedy incremental)", mode);
        const uint32_t n = e->e->hdb.n;
        if (n) require(assign, "assign");
        if (n_edges) require(edges, "edges");
        Timer tc;
        e->e->cluster_graph_device(mode, n, edges, n_edges, assign);
        e->e->stats.stage_seconds[UC_ST_SETCOVER] += tc.seconds();
    });
}

int uc_engine_reassign(uc_engine *e, const uint32_t *assign_in, uint32_t *assign_out, uint8_t *rejected_out, uint64_t counts[4]) {
    return guard([&] {
        require(e, "engine"); require(counts, "counts");
        if (e->e->hdb.n) { require(assign_in, "assign_in"); require(assign_out, "assign_out"); }
        e->e->reassign(assign_in, assign_out, rejected_out, counts);
    });
}

int uc_write_cluster_db(const char *out_cluster_db, uint32_t n, const uint32_t *assign) {
    return guard([&] {
        require(out_cluster_db, "out_cluster_db");
        std::vector<uint64_t> keys(n);
        for (uint32_t i = 0; i < n; i++) keys[i] = i;
        write_cluster_db(out_cluster_db, keys, assign, n);
    });
}

int uc_engine_ungapped_batch(uc_engine *e, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *diag, int32_t *score_out) {
    return guard([&] {
        require(e, "engine");
        if (n) { require(q, "q"); require(t, "t"); require(diag, "diag"); require(score_out, "score_out"); }
        e->e->ungapped_batch(n, q, t, diag, score_out);
    });
}

int uc_engine_ungapped_select(uc_engine *e, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *diag, int32_t min_score, int32_t *score_out,
                              uint64_t *overlap_out, uint64_t *kept_out) {
    return guard([&] {
        require(e, "engine");
        require(overlap_out, "overlap_out"); require(kept_out, "kept_out");
        if (n) { require(q, "q"); require(t, "t"); require(diag, "diag"); }
        e->e->ungapped_select(n, q, t, diag, min_score, score_out, overlap_out, kept_out);
    });
}

int uc_engine_ungapped_all(uc_engine *e, uint32_t qbegin, uint32_t qend, uint32_t tbegin, uint32_t tend, uint64_t tile_bytes, int32_t *score_out, int32_t *diag_out) {
    return guard([&] {
        require(e, "engine");
        if (qend > qbegin && tend > tbegin) { require(score_out, "score_out"); require(diag_out, "diag_out"); }
        e->e->ungapped_all(qbegin, qend, tbegin, tend, tile_bytes, score_out, diag_out);
    });
}

int uc_engine_sw_batch(uc_engine *e, int mode, uint64_t n, const uint32_t *q, const uint32_t *t, const int32_t *qend_in,
                       const int32_t *tend_in, int32_t *score_out, int32_t *qend_out, int32_t *tend_out) {
    return guard([&] {
        require(e, "engine");
        if (mode < 0 || mode > 2) fail(UC_ERR_ARGS, "sw_batch: mode must be 0, 1 or 2");
        if (!n) return;
        require(q, "q"); require(t, "t"); require(score_out, "score_out");
        if (mode == 2) { require(qend_in, "qend_in"); require(tend_in, "tend_in"); }
        std::vector<PairIn> pairs(n);
        for (uint64_t i = 0; i < n; i++) pairs[i] = {q[i], t[i], mode == 2 ? qend_in[i] : 0, mode == 2 ? tend_in[i] : 0};
        e->e->sw_batch(mode, pairs, score_out, qend_out, tend_out);
    });
}

int uc_engine_sw_pass(uc_engine *e, int table, int mode, int band, int raw, uint64_t n, const uint32_t *q, const uint32_t *t,
                      const int32_t *box, const int32_t *known, int32_t *score_out, int32_t *qend_out, int32_t *tend_out,
                      int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out) {
    return uc_engine_sw_pass2(e, table, mode, band, raw, n, q, t, box, known, score_out, qend_out, tend_out, class_out, aln_len_out, idents_out,
                              gaps_out, miss_out, nullptr, nullptr);
}

int uc_engine_sw_pass2(uc_engine *e, int table, int mode, int band, int raw, uint64_t n, const uint32_t *q, const uint32_t *t,
                       const int32_t *box, const int32_t *known, int32_t *score_out, int32_t *qend_out, int32_t *tend_out,
                       int32_t *class_out, int32_t *aln_len_out, int32_t *idents_out, int32_t *gaps_out, int32_t *miss_out,
                       int32_t *qend2_out, int32_t *tend2_out) {
    return guard([&] {
        require(e, "engine");
        if (!n) return;
        require(q, "q"); require(t, "t");
        if (mode == 2 || mode == 3 || mode == 6 || mode == 7) require(box, "box");
        if (mode == 4 || mode == 6 || mode == 7) require(known, "known");
        std::vector<SwPassPair> pairs(n);
        for (uint64_t i = 0; i < n; i++) {
            SwPassPair &x = pairs[i];
            x.q = q[i]; x.t = t[i];
            x.qs = box ? box[4 * i] : 0; x.qe = box ? box[4 * i + 1] : 0; x.ts = box ? box[4 * i + 2] : 0; x.te = box ? box[4 * i + 3] : 0;
            x.known = known ? known[i] : 0;
        }
        if ((qend2_out || tend2_out) && mode != 4 && mode != 6) fail(UC_ERR_ARGS, "sw_pass: only modes 4 and 6 have a second answer");
        e->e->sw_pass(table, mode, band, raw != 0, pairs,
                      {score_out, qend_out, tend_out, class_out, aln_len_out, idents_out, gaps_out, miss_out, qend2_out, tend2_out});
    });
}

// ---- the three calls of /root/reference/src/modules/cluster.rs:45-76 ----------------------------

int uc_cluster(const char *db, const char *out_cluster_db, const char *tmp, const uc_opts *o, uc_stats *stats_out) {
    return guard([&] {
        require(db, "db"); require(out_cluster_db, "out_cluster_db");
        cluster_workflow(db, out_cluster_db, tmp, o, stats_out);      // uc_workflow.cpp
    });
}

int uc_comm_unique_id(uint8_t id[UC_COMM_ID_BYTES]) {
    return guard([&] { require(id, "id"); comm_unique_id(id); });
}

int uc_comm_create(const uint8_t id[UC_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, uc_comm **out) {
    return guard([&] {
        require(id, "id"); require(out, "out");
        *out = nullptr;
        if (world < 1 || rank < 0 || rank >= world) fail(UC_ERR_ARGS, "uc_comm_create: rank %d outside world %d", rank, world);
        auto h = std::make_unique<uc_comm>();
        if (device < 0) UC_HIP(hipGetDevice(&device));
        comm_init_rank(h->c, id, rank, world, device);
        *out = h.release();
    });
}

void uc_comm_destroy(uc_comm *c) { delete c; }

int uc_comm_info(const uc_comm *c, int32_t *nccl_ranks, int32_t *nccl_rank, int32_t *device) {
    return guard([&] {
        require(c, "comm");
        int n = 0, r = 0, d = 0;
        comm_info(c->c, &n, &r, &d);
        if (nccl_ranks) *nccl_ranks = n;
        if (nccl_rank) *nccl_rank = r;
        if (device) *device = d;
    });
}

int uc_engine_cluster_step(uc_engine *e, uc_comm *comm, int32_t target_shards, uint32_t *assign, uint64_t *n_alignments) {
    return guard([&] {
        require(e, "engine");
        Comm solo;
        Comm &C = comm ? comm->c : solo;
        const uint64_t k = cluster_step(*e->e, C, target_shards, assign);
        if (n_alignments) *n_alignments = k;
    });
}

int uc_search(const char *query_db, const char *target_db, const char *out_aln_db, const char *tmp, const uc_opts *o, uc_stats *stats_out) {
    return guard([&] {
        require(query_db, "query_db"); require(target_db, "target_db"); require(out_aln_db, "out_aln_db");
        Params p = params_from(o, true);
        p.want_tb = 1;
        if (tmp && *tmp) make_dirs(tmp);
        Engine E(p, o ? o->device : -1);
        E.emit_bt = p.want_bt != 0;
        Timer tl;
        HostDb T, Q;
        read_seq_db(target_db, T, false);
        read_seq_db(query_db, Q, false);
        {   // 3Di tracks predicted under different readings of the ProstT5 head (uc_createdb records its reading in <db>_ss.source) are not comparable at the sequence ends
            auto source_of = [](const std::string &db) { std::ifstream f(db + "_ss.source"); std::string l; if (f) std::getline(f, l); return l; };
            const std::string st = source_of(target_db), sq = source_of(query_db);
            if (!st.empty() && !sq.empty() && st != sq)
                logf(2, "unicore-search: WARNING: the 3Di tracks of the two databases were predicted under different ProstT5 head conventions (%s: '%s'; %s: '%s')\n",
                     target_db, st.c_str(), query_db, sq.c_str());
        }
        const uint32_t nt = T.n, nq = Q.n, n = nt + nq;
        if ((uint64_t)nt + nq >= (1u << 24)) fail(UC_ERR_ARGS, "this build supports < 2^24 sequences (query + target)");
        // one loaded set: targets first, then queries; only [0, nt) is indexed, only [nt, n) are queries
        HostDb &C = E.hdb;
        C.n = n;
        C.keys = T.keys; C.keys.insert(C.keys.end(), Q.keys.begin(), Q.keys.end());
        C.off.resize((size_t)n + 1);
        const uint64_t rt = T.residues();
        for (uint32_t i = 0; i <= nt; i++) C.off[i] = T.off[i];
        for (uint32_t i = 0; i <= nq; i++) C.off[nt + i] = rt + Q.off[i];
        C.s3 = T.s3; C.s3.insert(C.s3.end(), Q.s3.begin(), Q.s3.end());
        C.sa = T.sa; C.sa.insert(C.sa.end(), Q.sa.begin(), Q.sa.end());
        E.stats.stage_seconds[UC_ST_LOAD] += tl.seconds();
        E.evalue_residues = rt;
        E.upload_db();
        logf(3, "unicore-search: %u queries vs %u targets (%llu residues) on device %d\n", nq, nt, (unsigned long long)rt, E.device);
        E.prefilter(0, nt, nt, n);
        logf(3, "unicore-search: prefilter kept %llu pairs (k-score %d, max-seqs %d)\n", (unsigned long long)E.n_hits, p.kmer_thr, p.max_seqs);
        E.align(nt, n);
        Timer to;
        std::vector<uc_hit> hits(std::max<uint64_t>(E.n_hits, 1));
        std::vector<uc_aln> alns(std::max<uint64_t>(E.n_hits, 1));
        if (E.n_hits) { E.get_hits(hits.data()); E.get_alns(0, E.n_hits, alns.data()); }
        std::vector<uint64_t> bt_off(E.n_hits + 1, 0);
        std::vector<uint32_t> bt_runs;
        if (p.want_bt && E.n_hits) {
            E.get_backtraces(0, E.n_hits, bt_off.data(), bt_runs);
            logf(3, "unicore-search: backtraces: %llu runs in a device buffer of %llu (%.1f MB)\n", (unsigned long long)bt_runs.size(), (unsigned long long)E.bt_used, E.bt_used * 4 / 1e6);
        }
        std::vector<std::vector<AlnRow>> rows(nq);
        uint64_t n_acc = 0;
        for (uint32_t q = 0; q < nq; q++) {
            const uint32_t qi = nt + q;
            const int lq = (int)C.len(qi);
            std::vector<AlnRow> &rv = rows[q];
            for (uint64_t k = E.hit_off[qi]; k < E.hit_off[qi + 1]; k++) {
                const uc_aln &a = alns[k];
                if (!a.accepted) continue;
                const uint32_t t = hits[k].target;
                AlnRow r;
                r.tkey = T.keys[t];
                r.corrected = a.corrected;
                r.bits = (int32_t)((p.lambda * (double)a.corrected - std::log(p.Kconst)) / std::log(2.0));
                r.evalue = p.Kconst * (double)lq * (double)rt * std::exp(-p.lambda * (double)a.corrected);
                r.fident = a.aln_len > 0 ? (double)a.idents / (double)a.aln_len : 0.0;
                r.qstart = a.qstart; r.qend = a.qend; r.qlen = lq; r.tstart = a.tstart; r.tend = a.tend; r.tlen = (int32_t)T.len(t);
                r.aln_len = a.aln_len; r.idents = a.idents; r.gap_opens = a.gap_opens;
                if (p.want_bt) r.bt = render_backtrace(bt_runs.data() + bt_off[k], bt_off[k + 1] - bt_off[k]);
                rv.push_back(std::move(r));
            }
            std::sort(rv.begin(), rv.end(), [](const AlnRow &x, const AlnRow &y) { return x.corrected != y.corrected ? x.corrected > y.corrected : x.tkey < y.tkey; });
            n_acc += rv.size();
        }
        write_aln_db(out_aln_db, Q.keys, rows);
        E.stats.stage_seconds[UC_ST_OUTPUT] += to.seconds();
        logf(3, "unicore-search: %llu alignments, %llu accepted -> %s\n", (unsigned long long)E.stats.n_gapped_alignments, (unsigned long long)n_acc, out_aln_db);
        E.stats.n_seqs = n;
        if (stats_out) *stats_out = E.stats;
    });
}

int uc_convertalis(const char *query_db, const char *target_db, const char *aln_db, const char *out_m8, const uc_opts *o) {
    return guard([&] {
        require(query_db, "query_db"); require(target_db, "target_db"); require(aln_db, "aln_db"); require(out_m8, "out_m8");
        if (o) g_verbosity = o->verbosity;
        Params p;
        if (o && o->cluster_options) parse_cluster_options(o->cluster_options, p);
        convert_alis(query_db, target_db, aln_db, out_m8, p.format_output);
    });
}

int uc_createtsv(const char *db, const char *cluster_db, const char *out_tsv, const uc_opts *o) {
    return guard([&] {
        require(db, "db"); require(cluster_db, "cluster_db"); require(out_tsv, "out_tsv");
        if (o) g_verbosity = o->verbosity;
        create_tsv(db, cluster_db, out_tsv);
    });
}

int uc_createdb(const char *const *fasta_paths, int n_fasta, const char *out_db, const char *model, const uc_opts *o, uc_t5_stats *stats_out) {
    return guard([&] {
        require(fasta_paths, "fasta_paths"); require(out_db, "out_db"); require(model, "model");
        if (n_fasta < 1) fail(UC_ERR_ARGS, "createdb: no input files");
        std::vector<std::string> fp;
        for (int i = 0; i < n_fasta; i++) { require(fasta_paths[i], "fasta path"); fp.push_back(fasta_paths[i]); }
        // devices: the convention of uc_cluster (plan_devices; more than are visible only with UC_VIRTUAL_GPUS=1: several replicas per device, the
        // single-GPU box's test of this path).  The encoder shards by sequence, "replicas only".
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) fail(UC_ERR_DEVICE, "no HIP device available; the ProstT5 encoder has no CPU fallback");
        const int want = o ? o->num_gpus : 1;
        if (want < 0 || want > 64) fail(UC_ERR_ARGS, "createdb: num_gpus must be in [0,64] (0 = all visible)");
        const std::vector<int> devices = plan_visible_devices(want, o ? o->device : -1, ndev).devices;
        T5Stats st;
        std::vector<T5Stats> per;
        t5_createdb(fp, out_db, model, devices, o ? o->verbosity : 3, &st, &per);
        if (stats_out) {
            stats_out->n_seqs = st.n_seqs; stats_out->n_tokens = st.n_tokens; stats_out->flops = st.flops; stats_out->gpu_ms = st.total_ms;
            stats_out->n_replicas = (uint32_t)per.size(); stats_out->reserved0 = 0;
            stats_out->gpu_ms_sum = 0;
            uint64_t lo = UINT64_MAX, hi = 0;
            for (const T5Stats &x : per) { stats_out->gpu_ms_sum += x.total_ms; lo = std::min<uint64_t>(lo, x.n_tokens); hi = std::max<uint64_t>(hi, x.n_tokens); }
            stats_out->tokens_min_replica = per.empty() ? 0 : lo; stats_out->tokens_max_replica = hi;
        }
    });
}

int uc_t5_load(const char *model, int32_t device, uc_t5 **out) {
    return guard([&] {
        require(model, "model"); require(out, "out");
        *out = nullptr;
        std::string path = model;
        struct stat st;
        if (stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) path += "/prostt5-f16.gguf";
        auto h = std::make_unique<uc_t5>();
        h->m.load(path, device);
        *out = h.release();
    });
}

void uc_t5_free(uc_t5 *m) { delete m; }

int uc_t5_encode(uc_t5 *m, uint32_t n, const uint64_t *off, const char *aa, uint8_t *codes, float *logits) {
    return guard([&] {
        require(m, "model");
        if (!n) return;
        require(off, "off"); require(aa, "aa"); require(codes, "codes");
        std::vector<std::string> seqs(n);
        for (uint32_t i = 0; i < n; i++) {
            if (off[i + 1] < off[i]) fail(UC_ERR_ARGS, "t5_encode: offsets must be non-decreasing");
            seqs[i].assign(aa + off[i], aa + off[i + 1]);
        }
        std::vector<std::vector<uint8_t>> out;
        std::vector<std::vector<float>> lg;
        m->m.encode(seqs, out, logits ? &lg : nullptr);
        for (uint32_t i = 0; i < n; i++) {
            if (!out[i].empty()) memcpy(codes + off[i], out[i].data(), out[i].size());
            if (logits && !lg[i].empty()) memcpy(logits + off[i] * (size_t)m->m.cfg.n_out, lg[i].data(), lg[i].size() * 4);
        }
    });
}

int uc_t5_get_stats(const uc_t5 *m, uc_t5_stats *out) {
    return guard([&] {
        require(m, "model"); require(out, "out");
        out->n_seqs = m->m.stats.n_seqs; out->n_tokens = m->m.stats.n_tokens; out->flops = m->m.stats.flops; out->gpu_ms = m->m.stats.total_ms;
        out->n_replicas = 1; out->reserved0 = 0; out->gpu_ms_sum = m->m.stats.total_ms; out->tokens_min_replica = out->tokens_max_replica = m->m.stats.n_tokens;
    });
}

int uc_t5_gemm_variant(int32_t M, int32_t N, int32_t K, int32_t *variant) {
    return guard([&] {
        require(variant, "variant");
        if (!t5_gemm_admits(0, M, N, K)) fail(UC_ERR_ARGS, "t5 gemm: %d x %d x %d: needs M, N >= 1, N %% 4 == 0, K %% 64 == 0", M, N, K);
        *variant = t5_gemm_pick(M, N, K);
    });
}

int uc_t5_kernel_gemm(int32_t device, int32_t variant, int32_t epi, int32_t M, int32_t N, int32_t K, const uint16_t *A, const uint16_t *W, void *out) {
    return guard([&] {
        require(A, "A"); require(W, "W"); require(out, "out");
        if (epi < 0 || epi > 2) fail(UC_ERR_ARGS, "t5 gemm: epilogue must be 0, 1 or 2");
        if (variant < -1 || variant > 2) fail(UC_ERR_ARGS, "t5 gemm: variant must be -1 (the library's pick), 0, 1 or 2");
        if (!t5_gemm_admits(0, M, N, K)) fail(UC_ERR_ARGS, "t5 gemm: %d x %d x %d: needs M, N >= 1, N %% 4 == 0, K %% 64 == 0", M, N, K);
        const int v = variant < 0 ? t5_gemm_pick(M, N, K) : variant;
        if (!t5_gemm_admits(v, M, N, K)) fail(UC_ERR_ARGS, "t5 gemm: variant %d cannot run %d x %d x %d", v, M, N, K);
        use_device(device, T5_NO_FALLBACK);
        DevBufs b;
        const size_t mn = (size_t)M * N, ob = mn * (epi == 2 ? 4 : 2);
        const uint16_t *dA = b.up(A, (size_t)M * K), *dW = b.up(W, (size_t)N * K);
        void *dO = epi == 2 ? (void *)b.up((const float *)out, mn) : (void *)b.out<uint16_t>(mn);
        t5_gemm_run(v, epi, dA, dW, dO, M, N, K, nullptr);
        t5_finish();
        UC_HIP(hipMemcpy(out, dO, ob, hipMemcpyDeviceToHost));
    });
}

int uc_t5_kernel_rmsnorm(int32_t device, int32_t T, int32_t D, float eps, const float *x, const float *w, uint16_t *y) {
    return guard([&] {
        require(x, "x"); require(w, "w"); require(y, "y");
        if (T < 1 || D < 4 || D % 4) fail(UC_ERR_ARGS, "t5 rmsnorm: needs T >= 1 and D a positive multiple of 4 (T %d, D %d)", T, D);
        use_device(device, T5_NO_FALLBACK);
        DevBufs b;
        const size_t n = (size_t)T * D;
        const float *dx = b.up(x, n), *dw = b.up(w, (size_t)D);
        uint16_t *dy = b.out<uint16_t>(n);
        t5_rmsnorm(dx, dw, dy, T, D, eps, nullptr);
        t5_finish();
        UC_HIP(hipMemcpy(y, dy, n * 2, hipMemcpyDeviceToHost));
    });
}

int uc_t5_kernel_attention(int32_t device, int32_t H, int32_t n_seqs, const int32_t *seq_len, int32_t bias_span, const float *bias,
                           const uint16_t *qkv, uint16_t *out) {
    return guard([&] {
        require(bias, "bias"); require(qkv, "qkv"); require(out, "out");
        if (H < 1 || H > 1024) fail(UC_ERR_ARGS, "t5 attention: H = %d outside 1 .. 1024", H);
        int32_t maxL = 0;
        const std::vector<int32_t> off = t5_offsets(n_seqs, seq_len, 1, &maxL);
        if (bias_span < maxL) fail(UC_ERR_ARGS, "t5 attention: bias_span %d < longest sequence %d", bias_span, maxL);
        if (bias_span > (1 << 24)) fail(UC_ERR_ARGS, "t5 attention: bias_span %d too large", bias_span);
        std::vector<T5AttnTile> tiles;
        t5_attn_tiles(off.data(), (size_t)n_seqs, tiles);
        use_device(device, T5_NO_FALLBACK);
        DevBufs b;
        const size_t T = (size_t)off[(size_t)n_seqs], HD = (size_t)H * 128;
        const uint16_t *dq = b.up(qkv, T * 3 * HD);
        const float *db = b.up(bias, (size_t)H * (2 * (size_t)bias_span - 1));
        const T5AttnTile *dt = b.up(tiles.data(), tiles.size());
        uint16_t *dO = b.out<uint16_t>(T * HD);
        t5_attention(dq, dt, (int)tiles.size(), db, bias_span, H, dO, nullptr);
        t5_finish();
        UC_HIP(hipMemcpy(out, dO, T * HD * 2, hipMemcpyDeviceToHost));
    });
}

int uc_t5_kernel_cnn_head(int32_t device, int32_t n_seqs, const int32_t *seq_len, int32_t D, int32_t C1, int32_t KW, int32_t NO, int32_t eos_in_head,
                          const uint16_t *x, const float *w1, const float *b1, const float *w2, const float *b2, uint8_t *codes, float *logits) {
    return guard([&] {
        require(x, "x"); require(w1, "w1"); require(b1, "b1"); require(w2, "w2"); require(b2, "b2"); require(codes, "codes");
        if (D < 64 || D % 64 || D > 65536) fail(UC_ERR_ARGS, "t5 cnn head: d_model %d is not a multiple of 64 in 64 .. 65536", D);
        if (C1 < 1 || C1 > 4096 || KW < 1 || KW > 31 || !(KW & 1) || NO < 1 || NO > 21)
            fail(UC_ERR_ARGS, "t5 cnn head: C1 %d (1 .. 4096), KW %d (odd, <= 31), NO %d (1 .. 21)", C1, KW, NO);
        int32_t maxL = 0;
        const std::vector<int32_t> off = t5_offsets(n_seqs, seq_len, 2, &maxL);
        const int T = off[(size_t)n_seqs], ldc1 = t5_conv1_rows(C1, KW);
        std::vector<int32_t> seq_of((size_t)T);
        for (int32_t s = 0; s < n_seqs; s++) std::fill(seq_of.begin() + off[(size_t)s], seq_of.begin() + off[(size_t)s + 1], s);
        const std::vector<float> w1r = t5_conv1_rearrange(w1, C1, D, KW);
        use_device(device, T5_NO_FALLBACK);
        DevBufs b;
        const uint16_t *dx = b.up(x, (size_t)T * D);
        const float *dw1f = b.up(w1r.data(), w1r.size());
        void *dw1 = b.alloc(w1r.size() * 2);
        t5_f32_to_f16(dw1f, dw1, w1r.size(), nullptr);                  // as the loader rounds conv1
        const float *db1 = b.up(b1, (size_t)C1), *dw2 = b.up(w2, (size_t)NO * C1 * KW), *db2 = b.up(b2, (size_t)NO);
        const int32_t *dof = b.up(seq_of.data(), seq_of.size()), *doff = b.up(off.data(), off.size());
        void *dy = b.alloc((size_t)T * ldc1 * 2);
        float *dh1 = b.alloc<float>((size_t)T * C1 * 4), *dlg = logits ? b.out<float>((size_t)T * NO) : nullptr;
        uint8_t *dc = b.out<uint8_t>((size_t)T);
        t5_gemm(0, dx, dw1, dy, T, ldc1, D, nullptr);
        t5_cnn_head(dy, ldc1, dof, doff, db1, dw2, db2, dh1, dc, dlg, T, C1, KW, NO, eos_in_head ? 1 : 0, nullptr);
        t5_finish();
        UC_HIP(hipMemcpy(codes, dc, (size_t)T, hipMemcpyDeviceToHost));
        if (logits) UC_HIP(hipMemcpy(logits, dlg, (size_t)T * NO * 4, hipMemcpyDeviceToHost));
    });
}

int uc_t5_bias_table(int32_t H, int32_t buckets, int32_t max_dist, int32_t span, const float *rel_bias, float *out) {
    return guard([&] {
        require(rel_bias, "rel_bias"); require(out, "out");
        if (H < 1 || buckets < 4 || buckets % 2 || max_dist <= buckets / 4 || span < 1 || span > (1 << 24))
            fail(UC_ERR_ARGS, "t5 bias table: H %d >= 1, buckets %d even >= 4, max_dist %d > buckets / 4, span %d in 1 .. 2^24", H, buckets, max_dist, span);
        t5_bias_table(H, buckets, max_dist, span, rel_bias, out);
    });
}

int uc_rmdb(const char *db_prefix) {
    return guard([&] { require(db_prefix, "db_prefix"); remove_db(db_prefix); });
}

}  // extern "C"
