// uc_nj_boot_host.cpp — bootstrap support for the tree builder `nj` (rule UC-N/B): the checks host and device share, the host twins of
// the kernels of uc_nj_boot.hip (draws, replicate counts, batched joins), support counting and the driver behind uc_tree_infer_boot.  The labelled
// Newick writer is the writer of uc_nj_host.cpp with its label argument.  Builds without HIP, like uc_nj_host.cpp.
// The reference ends `unicore tree` in `iqtree -B 1000` (tree.rs:139-161): every internal branch of the tree a user receives carries a support value.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "uc_files.h"
#include "uc_nj.h"

namespace uc {

namespace {

void check_reps(uint64_t n_rep) {
    if (n_rep > NJ_BOOT_MAX_REPS) fail(UC_ERR_ARGS, "nj: %llu bootstrap replicates; 0 .. %u", (unsigned long long)n_rep, NJ_BOOT_MAX_REPS);
}

}  // namespace

void nj_boot_counts_validate(const NjBootCountArgs &a) {
    const NjCountArgs c{a.n, a.w, a.cells, a.threads, a.comp, a.diff};
    nj_counts_validate(c);
    check_reps((uint64_t)a.rep0 + a.n_rep);
}

// a replicate is the alignment of its drawn columns: the codes are gathered row by row and counted as nj_counts_host counts.  Replicates go to
// threads first; what is left of `threads` goes to the rows of one replicate
void nj_boot_counts_host(const NjBootCountArgs &a) {
    const uint64_t n = a.n, w = a.w, words = (w + 7) / 8, tri = n * (n - 1) / 2;
    std::vector<uint8_t> code(n * w);
    for (uint64_t x = 0; x < n * w; x++) code[x] = nj_code(a.cells[x]);
    const uint32_t threads = std::max<uint32_t>(a.threads, 1), outer = std::min<uint32_t>(threads, std::max<uint32_t>(a.n_rep, 1)), inner = std::max<uint32_t>(threads / outer, 1);
    parallel_for(a.n_rep, outer, [&](uint64_t b) {
        const uint64_t key = nj_boot_key(a.seed, a.rep0 + (uint32_t)b);
        std::vector<uint32_t> col(w);
        for (uint64_t t = 0; t < w; t++) col[t] = nj_boot_col(key, t, w);
        std::vector<uint64_t> rows(n * words, 0);
        for (uint64_t i = 0; i < n; i++) {
            uint8_t *o = (uint8_t *)(rows.data() + i * words);
            const uint8_t *c = code.data() + i * w;
            for (uint64_t t = 0; t < w; t++) o[t] = c[col[t]];
        }
        nj_count_codes(rows.data(), n, words, inner, a.comp + b * tri, a.diff + b * tri);
    });
}

void nj_join_batch_validate(const NjJoinBatchArgs &a) {
    check_rows(a.n);
    check_reps(a.n_rep);
    if (!a.n_rep) return;
    need(a.D, "D");
    const uint64_t n = a.n, steps = n > 3 ? n - 3 : 0;
    for (uint64_t b = 0; b < a.n_rep; b++) {
        const NjJoinArgs one{a.n, a.D + b * n * n, a.join_a ? a.join_a + b * steps : nullptr, a.join_b ? a.join_b + b * steps : nullptr, a.len_a ? a.len_a + b * steps : nullptr,
                             a.len_b ? a.len_b + b * steps : nullptr, a.root_node ? a.root_node + b * 3 : nullptr, a.root_len ? a.root_len + b * 3 : nullptr};
        nj_join_validate(one);
    }
}

void nj_join_batch_host(const NjJoinBatchArgs &a) {
    const uint64_t n = a.n, steps = n > 3 ? n - 3 : 0;
    parallel_for(a.n_rep, a.threads, [&](uint64_t b) {
        nj_join_host(NjJoinArgs{a.n, a.D + b * n * n, a.join_a + b * steps, a.join_b + b * steps, a.len_a + b * steps, a.len_b + b * steps, a.root_node + b * 3, a.root_len + b * 3});
    });
}

namespace {

// ---- support: a split is the leaf set of a join's node, kept as a bit set of n bits on the side that does not hold leaf 0
struct Splits {
    uint32_t n = 0, steps = 0;
    uint64_t words = 0;
    std::vector<uint64_t> bits;      // [steps][words]
    const uint64_t *of(uint32_t s) const { return bits.data() + (uint64_t)s * words; }
};

// the joins must describe a forest inside the tree: a step joins two nodes that exist before it and hang from no earlier step
void splits_of(uint32_t n, const uint32_t *ja, const uint32_t *jb, Splits &S, std::vector<uint8_t> &used) {
    const uint32_t steps = n - 3;
    S.n = n; S.steps = steps; S.words = (n + 63) / 64;
    S.bits.assign((uint64_t)steps * S.words, 0);
    used.assign((size_t)n + steps, 0);
    auto add = [&](uint64_t *dst, uint32_t v, uint32_t limit) {
        if (v >= limit || used[v]) fail(UC_ERR_ARGS, "nj: node %u is joined twice or before it exists", v);
        used[v] = 1;
        if (v < n) dst[v / 64] |= 1ull << (v % 64);
        else { const uint64_t *src = S.of(v - n); for (uint64_t x = 0; x < S.words; x++) dst[x] |= src[x]; }
    };
    for (uint32_t s = 0; s < steps; s++) {
        uint64_t *dst = S.bits.data() + (uint64_t)s * S.words;
        add(dst, ja[s], n + s); add(dst, jb[s], n + s);
    }
    const uint64_t tail = n % 64 ? (1ull << (n % 64)) - 1 : ~0ull;
    for (uint32_t s = 0; s < steps; s++) {      // {L, complement} is one split: keep the side without leaf 0
        uint64_t *dst = S.bits.data() + (uint64_t)s * S.words;
        if (!(dst[0] & 1)) continue;
        for (uint64_t x = 0; x < S.words; x++) dst[x] = ~dst[x];
        dst[S.words - 1] &= tail;
    }
}

struct SplitKey {
    const uint64_t *p;
    uint64_t words;
    bool operator==(const SplitKey &o) const { return !memcmp(p, o.p, words * 8); }      // the leaf sets themselves decide
};
struct SplitHash {
    size_t operator()(const SplitKey &k) const {
        uint64_t h = 0;
        for (uint64_t x = 0; x < k.words; x++) h = nj_mix(h ^ k.p[x]);
        return (size_t)h;
    }
};

struct SupportCounter {
    Splits main;
    std::unordered_map<SplitKey, uint32_t, SplitHash> index;
    std::vector<std::atomic<uint32_t>> support;
    SupportCounter(uint32_t n, const uint32_t *ja, const uint32_t *jb) : support(n - 3) {
        std::vector<uint8_t> used;
        splits_of(n, ja, jb, main, used);
        for (uint32_t s = 0; s < main.steps; s++) {
            support[s] = 0;
            if (!index.emplace(SplitKey{main.of(s), main.words}, s).second) fail(UC_ERR_ARGS, "nj: join %u of the main tree repeats a split", s);
        }
    }
    void add(const uint32_t *ja, const uint32_t *jb) {      // one replicate; callable from several threads
        Splits R;
        std::vector<uint8_t> used;
        splits_of(main.n, ja, jb, R, used);
        for (uint32_t s = 0; s < R.steps; s++) {
            const auto it = index.find(SplitKey{R.of(s), R.words});
            if (it != index.end()) support[it->second].fetch_add(1, std::memory_order_relaxed);
        }
    }
};

void support_args(uint32_t n, const uint32_t *ja, const uint32_t *jb, uint32_t n_rep, const uint32_t *rja, const uint32_t *rjb, const uint32_t *support) {
    check_rows(n);
    check_reps(n_rep);
    if (n <= 3) return;
    need(ja, "join_a"); need(jb, "join_b"); need(support, "support");
    if (n_rep) { need(rja, "the replicates' join_a"); need(rjb, "the replicates' join_b"); }
}

}  // namespace

void nj_tree_infer_boot(const char *msa_fasta, const char *out_nwk, const char *model_name, uint32_t n_rep, uint64_t seed, const uc_opts *o, uc_nj_boot_stats *st_out,
                        NjBootRule *rule) {
    check_reps(n_rep);
    uc_nj_boot_stats st;
    memset(&st, 0, sizeof st);
    NjMainTree T;
    uc_nj_stats main_st;
    nj_main_tree(msa_fasta, model_name, o, T, main_st);
    st.n_rows = T.n; st.n_columns = T.w; st.n_replicates = n_rep;
    st.seconds[0] = main_st.seconds[0];
    st.seconds[1] = main_st.seconds[1] + main_st.seconds[2] + main_st.seconds[3];
    Timer t_part;
    auto lap = [&](int phase) { st.seconds[phase] += t_part.seconds(); t_part = Timer(); };
    const uint32_t n = T.n, steps = n > 3 ? n - 3 : 0;
    const uint64_t tri = (uint64_t)n * (n - 1) / 2, nn = (uint64_t)n * n;
    std::vector<uint32_t> support(std::max<uint32_t>(steps, 1), 0);
    std::string boot_trees;
    std::vector<uint64_t> labels;                  // a rule's own; empty: the percentages of support
    std::vector<std::string> tsv_columns;          // a rule's columns of the dump, behind the support
    if (n_rep && (steps || T.dump)) {      // n <= 3 has no internal branch: its replicates are computed for the dump alone
        std::unique_ptr<SupportCounter> counter;
        if (steps && !rule) counter.reset(new SupportCounter(n, T.ja.data(), T.jb.data()));
        if (steps && rule) rule->begin(T, n_rep);
        // a batch holds the counts, D and the join records of its replicates
        const uint64_t per_rep = tri * 8 + nn * 8 + (uint64_t)steps * 24 + 36;
        const uint32_t batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_rep, tree_budget_bytes() / per_rep));
        const size_t rec = std::max<size_t>((size_t)batch * steps, 1);
        std::vector<uint32_t> comp(batch * tri), diff(batch * tri), ja(rec), jb(rec), root((size_t)batch * 3);
        std::vector<double> D(batch * nn), la(rec), lb(rec), rlen((size_t)batch * 3);
        std::vector<const char *> names(n);
        for (uint32_t i = 0; i < n; i++) names[i] = T.names[i].c_str();
        lap(5);
        for (uint32_t b0 = 0; b0 < n_rep; b0 += batch, st.n_batches++) {
            const uint32_t nb = std::min<uint32_t>(batch, n_rep - b0);
            const NjBootCountArgs ca{n, T.w, T.cells.data(), seed, b0, nb, (uint32_t)T.threads, comp.data(), diff.data()};
            if (T.on_host) nj_boot_counts_host(ca); else nj_boot_counts_device(T.device, ca);
            lap(2);
            parallel_for(nb, (uint32_t)T.threads, [&](uint64_t b) { nj_distances_host(comp.data() + b * tri, diff.data() + b * tri, n, T.model, D.data() + b * nn, nullptr); });
            lap(3);
            const NjJoinBatchArgs ja_args{n, nb, D.data(), ja.data(), jb.data(), la.data(), lb.data(), root.data(), rlen.data(), (uint32_t)T.threads};
            if (T.on_host) nj_join_batch_host(ja_args); else nj_join_batch_device(T.device, ja_args);
            lap(4);
            if (steps && rule) rule->batch(T, nb, ja.data(), jb.data());
            else if (steps) parallel_for(nb, (uint32_t)T.threads, [&](uint64_t b) { counter->add(ja.data() + b * steps, jb.data() + b * steps); });
            lap(5);
            if (T.dump)
                for (uint64_t b = 0; b < nb; b++)
                    boot_trees += nj_newick_line(names.data(), n, ja.data() + b * steps, jb.data() + b * steps, la.data() + b * steps, lb.data() + b * steps, root.data() + b * 3,
                                                 rlen.data() + b * 3, nullptr, 0);
            lap(6);
        }
        st.support_min = steps ? n_rep : 0;
        if (steps && rule) rule->finish(support.data(), labels, tsv_columns);
        for (uint32_t s = 0; s < steps; s++) {
            if (!rule) support[s] = counter->support[s];
            st.support_min = std::min<uint64_t>(st.support_min, support[s]);
            st.support_sum += support[s];
        }
        lap(5);
    }
    nj_write_main_tree(out_nwk, T, support.data(), steps ? n_rep : 0, labels.empty() ? nullptr : labels.data());
    if (T.dump && n_rep) {
        std::string txt;
        for (uint32_t s = 0; s < steps; s++) txt += std::to_string(s) + "\t" + std::to_string(support[s]) + (tsv_columns.empty() ? std::string() : tsv_columns[s]) + "\n";
        write_file(std::string(out_nwk) + ".boot.tsv", txt);
        write_file(std::string(out_nwk) + ".boottrees", boot_trees);
    }
    lap(6);
    if (getenv("UC_TIMING"))
        fprintf(stderr, "unicore-cluster[timing]: tree_infer_boot (%s): %u rows x %llu columns, %u replicates in %llu batch(es): read %.3f s, main tree %.3f s, draws + counts %.3f s, "
                "transform %.3f s, joins %.3f s, support %.3f s, write %.3f s\n", T.on_host ? "host" : "device", n, (unsigned long long)T.w, n_rep, (unsigned long long)st.n_batches,
                st.seconds[0], st.seconds[1], st.seconds[2], st.seconds[3], st.seconds[4], st.seconds[5], st.seconds[6]);
    if (st_out) *st_out = st;
}

}  // namespace uc

using namespace uc;

int uc_nj_boot_columns(uint64_t w, uint64_t seed, uint32_t rep, uint32_t *cols) {
    return guard([&] {
        if (w < 1 || w >> 31) fail(UC_ERR_ARGS, "nj: %llu columns; 1 .. 2^31 - 1", (unsigned long long)w);
        check_reps((uint64_t)rep + 1);
        need(cols, "cols");
        const uint64_t key = nj_boot_key(seed, rep);
        for (uint64_t t = 0; t < w; t++) cols[t] = nj_boot_col(key, t, w);
    });
}

int uc_nj_boot_counts(uint32_t n, uint64_t w, const uint8_t *cells, uint64_t seed, uint32_t rep0, uint32_t n_rep, uint32_t threads, uint32_t *comp, uint32_t *diff) {
    return guard([&] {
        const NjBootCountArgs a{n, w, cells, seed, rep0, n_rep, threads, comp, diff};
        nj_boot_counts_validate(a);
        nj_boot_counts_host(a);
    });
}

int uc_nj_boot_counts_dev(int32_t device, uint32_t n, uint64_t w, const uint8_t *cells, uint64_t seed, uint32_t rep0, uint32_t n_rep, uint32_t threads, uint32_t *comp,
                          uint32_t *diff) {
    return guard([&] {
        const NjBootCountArgs a{n, w, cells, seed, rep0, n_rep, threads, comp, diff};
        nj_boot_counts_validate(a);
        if (n_rep) nj_boot_counts_device(device, a);
    });
}

int uc_nj_join_batch(uint32_t n, uint32_t n_rep, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node, double *root_len) {
    return guard([&] {
        const NjJoinBatchArgs a{n, n_rep, D, join_a, join_b, len_a, len_b, root_node, root_len, 1};
        nj_join_batch_validate(a);
        nj_join_batch_host(a);
    });
}

int uc_nj_join_batch_dev(int32_t device, uint32_t n, uint32_t n_rep, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node,
                         double *root_len) {
    return guard([&] {
        const NjJoinBatchArgs a{n, n_rep, D, join_a, join_b, len_a, len_b, root_node, root_len, 1};
        nj_join_batch_validate(a);
        if (n_rep) nj_join_batch_device(device, a);
    });
}

int uc_nj_support(uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a, const uint32_t *rep_join_b, uint32_t *support) {
    return guard([&] {
        support_args(n, join_a, join_b, n_rep, rep_join_a, rep_join_b, support);
        if (n <= 3) return;
        const uint32_t steps = n - 3;
        SupportCounter counter(n, join_a, join_b);
        for (uint64_t b = 0; b < n_rep; b++) counter.add(rep_join_a + b * steps, rep_join_b + b * steps);
        for (uint32_t s = 0; s < steps; s++) support[s] = counter.support[s];
    });
}

int uc_nj_newick_support(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                         const uint32_t *root_node, const double *root_len, const uint32_t *support, uint32_t n_rep, char *buf, uint64_t cap, uint64_t *need_out) {
    return guard([&] {
        const std::string s = nj_newick_line(names, n, join_a, join_b, len_a, len_b, root_node, root_len, support, n_rep);
        if (need_out) *need_out = s.size();
        if (!buf && !cap) return;
        if (!buf || cap < s.size() + 1) fail(UC_ERR_ARGS, "nj: the tree takes %zu bytes and the NUL, the buffer holds %llu", s.size(), (unsigned long long)cap);
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

int uc_nj_boot_geometry(uint32_t *lds_rows) {
    return guard([&] { if (lds_rows) *lds_rows = NJ_LDS_ROWS; });
}

int uc_tree_infer_boot(const char *msa_fasta, const char *out_nwk, const char *model, uint32_t n_rep, uint64_t seed, const uc_opts *o, uc_nj_boot_stats *stats_out) {
    return guard([&] {
        if (!msa_fasta || !out_nwk) fail(UC_ERR_ARGS, "tree_infer_boot: msa_fasta and out_nwk must not be NULL");
        nj_tree_infer_boot(msa_fasta, out_nwk, model, n_rep, seed, o, stats_out, nullptr);
    });
}
