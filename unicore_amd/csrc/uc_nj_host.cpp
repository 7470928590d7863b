// uc_nj_host.cpp — the tree builder `nj` (rule UC-N): the checks host and device share, the host twins of the kernels of uc_nj.hip,
// the distance transform and the Newick writer (host only), the C entry points and the file level (uc_tree_infer).
// The reference hands inference to iqtree, fasttree or raxml-ng (tree.rs:139-161, genetree.rs); `nj` is a builder of this project's own.
// No FMA: uc_nj.h turns contraction off for this file too, and the host build names no -march, so a * b + c is two roundings here as on the device.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "uc_db.h"
#include "uc_files.h"
#include "uc_nj.h"

namespace uc {

namespace {

bool env_is_one(const char *name) { const char *v = getenv(name); return v && !strcmp(v, "1"); }

constexpr uint64_t K7F = 0x7f7f7f7f7f7f7f7full, K80 = 0x8080808080808080ull;

}  // namespace

void nj_counts_validate(const NjCountArgs &a) {
    check_rows(a.n);
    if (a.w < 1 || a.w >> 31) fail(UC_ERR_ARGS, "nj: %llu columns; 1 .. 2^31 - 1", (unsigned long long)a.w);
    need(a.cells, "cells"); need(a.comp, "comp"); need(a.diff, "diff");
}

// eight columns per 64-bit word, as the kernel takes four per dword: codes stay below 0x80, so x + 0x7f sets a byte's top bit iff the byte is not 0
// and never carries into the next byte
void nj_counts_host(const NjCountArgs &a) {
    const uint64_t n = a.n, w = a.w, words = (w + 7) / 8;
    std::vector<uint64_t> code(n * words, 0);
    for (uint64_t i = 0; i < n; i++) {
        uint8_t *o = (uint8_t *)(code.data() + i * words);
        const uint8_t *c = a.cells + i * w;
        for (uint64_t x = 0; x < w; x++) o[x] = nj_code(c[x]);
    }
    nj_count_codes(code.data(), n, words, a.threads, a.comp, a.diff);
}

void nj_count_codes(const uint64_t *code, uint64_t n, uint64_t words, uint32_t threads, uint32_t *comp_out, uint32_t *diff_out) {
    parallel_for(n ? n - 1 : 0, threads, [&](uint64_t i) {      // a ticket is a row and its pairs (i, j > i)
        const uint64_t *x = code + i * words;
        uint64_t k = i * n - i * (i + 1) / 2;
        for (uint64_t j = i + 1; j < n; j++, k++) {
            const uint64_t *y = code + j * words;
            uint64_t comp = 0, diff = 0;
            for (uint64_t t = 0; t < words; t++) {
                const uint64_t m = (x[t] + K7F) & (y[t] + K7F) & K80;
                comp += (uint64_t)__builtin_popcountll(m);
                diff += (uint64_t)__builtin_popcountll(m & ((x[t] ^ y[t]) + K7F));
            }
            comp_out[k] = (uint32_t)comp; diff_out[k] = (uint32_t)diff;
        }
    });
}

void nj_distances_host(const uint32_t *comp, const uint32_t *diff, uint32_t n, uint32_t model, double *D, uint64_t *counts) {
    check_rows(n);
    if (model > 1) fail(UC_ERR_ARGS, "nj: model %u (0 kimura, 1 p)", model);
    need(comp, "comp"); need(diff, "diff"); need(D, "D");
    uint64_t k = 0, none = 0, capped = 0;
    for (uint64_t i = 0; i < n; i++) {
        D[i * n + i] = 0.0;
        for (uint64_t j = i + 1; j < n; j++, k++) {
            if (diff[k] > comp[k]) fail(UC_ERR_ARGS, "nj: pair (%llu, %llu) differs in %u of %u columns", (unsigned long long)i, (unsigned long long)j, diff[k], comp[k]);
            double d = NJ_CAP;
            if (comp[k]) {
                const double p = (double)diff[k] / (double)comp[k];
                if (model == 1) d = p;
                else {
                    const double t = 1.0 - p - 0.2 * p * p;
                    if (t > 0.0) { d = -std::log(t); if (d > NJ_CAP) d = NJ_CAP; }
                }
                if (d == 0.0) d = 0.0;      // -log(1) is -0.0
            } else none++;
            if (d == NJ_CAP) capped++;
            D[i * n + j] = D[j * n + i] = d;
        }
    }
    if (counts) { counts[0] = none; counts[1] = capped; }
}

void nj_join_validate(const NjJoinArgs &a) {
    check_rows(a.n);
    need(a.D, "D"); need(a.root_node, "root_node"); need(a.root_len, "root_len");
    if (a.n > 3) { need(a.join_a, "join_a"); need(a.join_b, "join_b"); need(a.len_a, "len_a"); need(a.len_b, "len_b"); }
    const uint64_t n = a.n;
    for (uint64_t i = 0; i < n; i++) {
        if (a.D[i * n + i] != 0.0 || std::signbit(a.D[i * n + i])) fail(UC_ERR_ARGS, "nj: D(%llu, %llu) is not 0", (unsigned long long)i, (unsigned long long)i);
        for (uint64_t j = i + 1; j < n; j++) {
            const double d = a.D[i * n + j];
            if (!std::isfinite(d) || std::signbit(d)) fail(UC_ERR_ARGS, "nj: D(%llu, %llu) is negative or not finite", (unsigned long long)i, (unsigned long long)j);
            if (memcmp(&d, &a.D[j * n + i], sizeof d) != 0) fail(UC_ERR_ARGS, "nj: D is not symmetric at (%llu, %llu)", (unsigned long long)i, (unsigned long long)j);
        }
    }
}

void nj_join_host(const NjJoinArgs &a) {
    const uint64_t n = a.n;
    if (n == 2) {
        a.root_node[0] = 0; a.root_node[1] = 1; a.root_node[2] = NJ_NO_NODE;
        a.root_len[0] = a.root_len[1] = 0.5 * a.D[1]; a.root_len[2] = 0.0;
        return;
    }
    std::vector<double> d(a.D, a.D + n * n), r(n, 0.0);
    std::vector<uint32_t> node(n);
    std::vector<uint8_t> act(n, 1);
    for (uint32_t i = 0; i < n; i++) node[i] = i;
    uint32_t m = (uint32_t)n;
    for (uint32_t s = 0; m > 3; s++, m--) {
        for (uint64_t i = 0; i < n; i++) {
            if (!act[i]) continue;
            double sum = 0.0;
            for (uint64_t k = 0; k < n; k++) if (act[k] && k != i) sum += d[i * n + k];
            r[i] = sum;
        }
        uint64_t bi = 0, bj = 0;
        double bq = 0.0;
        bool have = false;
        for (uint64_t i = 0; i < n; i++) {
            if (!act[i]) continue;
            for (uint64_t j = i + 1; j < n; j++) {      // ascending (i, j): an equal Q never replaces
                if (!act[j]) continue;
                const double q = nj_q(m, d[i * n + j], r[i], r[j]);
                if (!have || q < bq) { bq = q; bi = i; bj = j; have = true; }
            }
        }
        const double dij = d[bi * n + bj];
        nj_branch(m, dij, r[bi], r[bj], a.len_a[s], a.len_b[s]);
        a.join_a[s] = node[bi]; a.join_b[s] = node[bj];
        for (uint64_t k = 0; k < n; k++) {
            if (!act[k] || k == bi || k == bj) continue;
            d[bi * n + k] = d[k * n + bi] = nj_new(d[bi * n + k], d[bj * n + k], dij);
        }
        node[bi] = (uint32_t)n + s;
        act[bj] = 0;
    }
    uint64_t x[3], c = 0;
    for (uint64_t i = 0; i < n; i++) if (act[i]) x[c++] = i;
    for (int t = 0; t < 3; t++) a.root_node[t] = node[x[t]];
    nj_root3(d[x[0] * n + x[1]], d[x[0] * n + x[2]], d[x[1] * n + x[2]], a.root_len);
}

namespace {

void append_name(std::string &out, const char *name) {
    bool quote = !*name;
    for (const char *p = name; *p; p++) if (strchr("()[]:;,'", *p) || is_space(*p)) quote = true;
    if (!quote) { out += name; return; }
    out += '\'';
    for (const char *p = name; *p; p++) { if (*p == '\'') out += '\''; out += *p; }
    out += '\'';
}
void append_len(std::string &out, double v) {
    char b[400];
    snprintf(b, sizeof b, ":%.6f", v);
    out += b;
}

}  // namespace

std::string nj_newick_line(const char *const *names, uint32_t n, const uint32_t *ja, const uint32_t *jb, const double *la, const double *lb, const uint32_t *root,
                           const double *rlen, const uint32_t *support, uint32_t n_rep, const uint64_t *label_of) {
    check_rows(n);
    need(names, "names"); need(root, "root_node"); need(rlen, "root_len");
    const uint32_t steps = n > 3 ? n - 3 : 0, kids = n == 2 ? 2 : 3;
    if (steps) { need(ja, "join_a"); need(jb, "join_b"); need(la, "len_a"); need(lb, "len_b"); }
    const bool labels = steps && n_rep > 0;      // UC-N/B: the root carries none
    if (labels && !label_of) {
        need(support, "support");
        if (n_rep > NJ_BOOT_MAX_REPS) fail(UC_ERR_ARGS, "nj: %u replicates; 0 .. %u", n_rep, NJ_BOOT_MAX_REPS);
        for (uint32_t s = 0; s < steps; s++) if (support[s] > n_rep) fail(UC_ERR_ARGS, "nj: support %u of %u replicates at join %u", support[s], n_rep, s);
    }
    for (uint32_t i = 0; i < n; i++) need(names[i], "a name");
    // every node hangs from exactly one parent, and a step joins nodes that exist before it
    std::vector<uint8_t> used((size_t)n + steps, 0);
    auto take = [&](uint32_t v, uint32_t limit) {
        if (v >= limit || used[v]) fail(UC_ERR_ARGS, "nj: node %u is joined twice or before it exists", v);
        used[v] = 1;
    };
    for (uint32_t s = 0; s < steps; s++) { take(ja[s], n + s); take(jb[s], n + s); }
    for (uint32_t t = 0; t < kids; t++) take(root[t], n + steps);
    for (size_t v = 0; v < used.size(); v++) if (!used[v]) fail(UC_ERR_ARGS, "nj: node %zu hangs from no join", v);
    std::string out = "(";
    struct Frame { uint32_t v; int st; };
    std::vector<Frame> st;
    for (uint32_t t = 0; t < kids; t++) {
        if (t) out += ',';
        st.push_back(Frame{root[t], 0});
        while (!st.empty()) {
            const Frame f = st.back();
            if (f.v < n) { append_name(out, names[f.v]); st.pop_back(); continue; }
            const uint32_t s = f.v - n;
            if (f.st == 0) { out += '('; st.back().st = 1; st.push_back(Frame{ja[s], 0}); }
            else if (f.st == 1) { append_len(out, la[s]); out += ','; st.back().st = 2; st.push_back(Frame{jb[s], 0}); }
            else {
                append_len(out, lb[s]); out += ')'; st.pop_back();
                if (labels) out += std::to_string(label_of ? label_of[s] : (200ull * support[s] + n_rep) / (2ull * n_rep));      // the percentage, rounded half up
            }
        }
        append_len(out, rlen[t]);
    }
    out += ");\n";
    return out;
}

namespace {

struct Msa { std::vector<std::string> names; std::vector<std::string> rows; };

Msa read_msa(const std::string &path) {
    const std::string text = read_whole_file(path);
    Msa M;
    std::unordered_set<std::string> seen;
    size_t p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        if (text[p] == '>') {
            size_t q = p + 1;
            while (q < e && !is_space(text[q])) q++;
            std::string name = text.substr(p + 1, q - p - 1);
            if (name.empty()) fail(UC_ERR_IO, "%s: a sequence without a name", path.c_str());
            if (!seen.insert(name).second) fail(UC_ERR_IO, "%s: the name %s appears twice", path.c_str(), name.c_str());
            M.names.push_back(std::move(name));
            M.rows.emplace_back();
        } else {
            if (M.rows.empty()) { for (size_t q = p; q < e; q++) if (!is_space(text[q])) fail(UC_ERR_IO, "%s: residues before the first '>'", path.c_str()); }
            else for (size_t q = p; q < e; q++) if (!is_space(text[q])) M.rows.back().push_back(text[q]);
        }
        p = e + 1;
    }
    return M;
}

}  // namespace

void nj_main_tree(const char *msa_fasta, const char *model_name, const uc_opts *o, NjMainTree &T, uc_nj_stats &st) {
    if (o) {
        if (o->struct_size != sizeof(uc_opts)) fail(UC_ERR_ARGS, "uc_opts.struct_size mismatch (%u != %zu)", o->struct_size, sizeof(uc_opts));
        T.device = o->device; T.threads = o->threads > 0 ? o->threads : 1;
    }
    T.model = UC_NJ_MODEL_KIMURA;
    if (model_name && !strcmp(model_name, "p")) T.model = UC_NJ_MODEL_P;
    else if (model_name && strcmp(model_name, "kimura") != 0) fail(UC_ERR_ARGS, "nj: unknown model '%s' (kimura, p)", model_name);
    T.on_host = env_is_one("UC_TREE_HOST"); T.dump = env_is_one("UC_TREE_DUMP");
    memset(&st, 0, sizeof st);
    Timer t_part;
    auto lap = [&](int phase) { st.seconds[phase] += t_part.seconds(); t_part = Timer(); };

    Msa M = read_msa(msa_fasta);
    if (M.rows.size() < NJ_MIN_ROWS || M.rows.size() > NJ_MAX_ROWS)
        fail(UC_ERR_ARGS, "%s: %zu rows; a tree needs %u .. %u", msa_fasta, M.rows.size(), NJ_MIN_ROWS, NJ_MAX_ROWS);
    const uint32_t n = (uint32_t)M.rows.size();
    const uint64_t w = M.rows[0].size();
    for (uint32_t i = 1; i < n; i++)
        if (M.rows[i].size() != w) fail(UC_ERR_ARGS, "%s: row %s has %zu columns, the first row %llu", msa_fasta, M.names[i].c_str(), M.rows[i].size(), (unsigned long long)w);
    T.n = n; T.w = w;
    T.cells.resize((size_t)n * std::max<uint64_t>(w, 1));
    for (uint32_t i = 0; i < n; i++) memcpy(T.cells.data() + (size_t)i * w, M.rows[i].data(), w);
    T.names = std::move(M.names);
    const uint64_t tri = (uint64_t)n * (n - 1) / 2;
    T.comp.resize(tri); T.diff.resize(tri);
    const NjCountArgs ca{n, w, T.cells.data(), (uint32_t)T.threads, T.comp.data(), T.diff.data()};
    nj_counts_validate(ca);
    st.n_rows = n; st.n_columns = w;
    lap(0);
    if (T.on_host) nj_counts_host(ca); else nj_counts_device(T.device, ca);
    lap(1);
    T.D.resize((size_t)n * n);
    uint64_t counts[2];
    nj_distances_host(T.comp.data(), T.diff.data(), n, T.model, T.D.data(), counts);
    st.n_pairs_incomparable = counts[0]; st.n_pairs_capped = counts[1];
    lap(2);
    const uint32_t steps = n > 3 ? n - 3 : 0;
    T.ja.resize(std::max<uint32_t>(steps, 1)); T.jb.resize(std::max<uint32_t>(steps, 1));
    T.la.resize(std::max<uint32_t>(steps, 1)); T.lb.resize(std::max<uint32_t>(steps, 1));
    const NjJoinArgs ja_args{n, T.D.data(), T.ja.data(), T.jb.data(), T.la.data(), T.lb.data(), T.root, T.rlen};
    if (T.on_host) nj_join_host(ja_args); else nj_join_device(T.device, ja_args);      // D comes from nj_distances_host: nothing nj_join_validate could refuse
    for (uint32_t s = 0; s < steps; s++) st.n_lengths_clamped += (T.la[s] == 0.0) + (T.lb[s] == 0.0);
    for (uint32_t t = 0; t < (n == 2 ? 2u : 3u); t++) st.n_lengths_clamped += T.rlen[t] == 0.0;
    lap(3);
}

void nj_write_main_tree(const char *out_nwk, const NjMainTree &T, const uint32_t *support, uint32_t n_rep, const uint64_t *labels) {
    const uint32_t n = T.n;
    std::vector<const char *> names(n);
    for (uint32_t i = 0; i < n; i++) names[i] = T.names[i].c_str();
    write_file(out_nwk, nj_newick_line(names.data(), n, T.ja.data(), T.jb.data(), T.la.data(), T.lb.data(), T.root, T.rlen, support, n_rep, labels));
    if (T.dump) {
        std::string txt;
        char b[128];
        uint64_t k = 0;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = i + 1; j < n; j++, k++) {
                snprintf(b, sizeof b, "%u\t%u\t%u\t%u\t%.17g\n", i, j, T.comp[k], T.diff[k], T.D[(size_t)i * n + j]);
                txt += b;
            }
        write_file(std::string(out_nwk) + ".dist.tsv", txt);
    }
}

namespace {

void tree_infer(const char *msa_fasta, const char *out_nwk, const char *model_name, const uc_opts *o, uc_nj_stats *st_out) {
    NjMainTree T;
    uc_nj_stats st;
    nj_main_tree(msa_fasta, model_name, o, T, st);
    Timer t_write;
    nj_write_main_tree(out_nwk, T, nullptr, 0);
    st.seconds[4] += t_write.seconds();
    if (getenv("UC_TIMING"))
        fprintf(stderr, "unicore-cluster[timing]: tree_infer (%s): %u rows x %llu columns: read %.3f s, counts %.3f s, transform %.3f s, joins %.3f s, write %.3f s\n",
                T.on_host ? "host" : "device", T.n, (unsigned long long)T.w, st.seconds[0], st.seconds[1], st.seconds[2], st.seconds[3], st.seconds[4]);
    if (st_out) *st_out = st;
}

}  // namespace

}  // namespace uc

using namespace uc;

int uc_nj_counts(uint32_t n, uint64_t w, const uint8_t *cells, uint32_t threads, uint32_t *comp, uint32_t *diff) {
    return guard([&] {
        const NjCountArgs a{n, w, cells, threads, comp, diff};
        nj_counts_validate(a);
        nj_counts_host(a);
    });
}

int uc_nj_counts_dev(int32_t device, uint32_t n, uint64_t w, const uint8_t *cells, uint32_t threads, uint32_t *comp, uint32_t *diff) {
    return guard([&] {
        const NjCountArgs a{n, w, cells, threads, comp, diff};
        nj_counts_validate(a);
        nj_counts_device(device, a);
    });
}

int uc_nj_distances(const uint32_t *comp, const uint32_t *diff, uint32_t n, uint32_t model, double *D) {
    return guard([&] { nj_distances_host(comp, diff, n, model, D, nullptr); });
}

int uc_nj_join(uint32_t n, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node, double *root_len) {
    return guard([&] {
        const NjJoinArgs a{n, D, join_a, join_b, len_a, len_b, root_node, root_len};
        nj_join_validate(a);
        nj_join_host(a);
    });
}

int uc_nj_join_dev(int32_t device, uint32_t n, const double *D, uint32_t *join_a, uint32_t *join_b, double *len_a, double *len_b, uint32_t *root_node,
                   double *root_len) {
    return guard([&] {
        const NjJoinArgs a{n, D, join_a, join_b, len_a, len_b, root_node, root_len};
        nj_join_validate(a);
        nj_join_device(device, a);
    });
}

int uc_nj_newick(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                 const uint32_t *root_node, const double *root_len, char *buf, uint64_t cap, uint64_t *need_out) {
    return guard([&] {
        const std::string s = nj_newick_line(names, n, join_a, join_b, len_a, len_b, root_node, root_len, nullptr, 0);
        if (need_out) *need_out = s.size();
        if (!buf && !cap) return;
        if (!buf || cap < s.size() + 1) fail(UC_ERR_ARGS, "nj: the tree takes %zu bytes and the NUL, the buffer holds %llu", s.size(), (unsigned long long)cap);
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

int uc_nj_geometry(uint32_t *tile_rows, uint32_t *chunk_columns) {
    return guard([&] {
        if (tile_rows) *tile_rows = NJ_TILE;
        if (chunk_columns) *chunk_columns = NJ_CHUNK;
    });
}

int uc_tree_infer(const char *msa_fasta, const char *out_nwk, const char *model, const uc_opts *o, uc_nj_stats *stats_out) {
    return guard([&] {
        if (!msa_fasta || !out_nwk) fail(UC_ERR_ARGS, "tree_infer: msa_fasta and out_nwk must not be NULL");
        tree_infer(msa_fasta, out_nwk, model, o, stats_out);
    });
}
