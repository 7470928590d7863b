// uc_msa_host.cpp — `unicore tree --no-inference` (rule UC-T): the checks host and device share, the host twins of the kernels of
// uc_msa.hip, the C entry points and the file level (uc_tree).
//   module body      /root/reference/src/modules/tree.rs:17-137       (run up to `if no_inference { return }`), :299-331 (filter_msa)
//   gene fasta       /root/reference/src/seq/create_gene_specific_fasta.rs:27-88
//   concatenation    /root/reference/src/seq/combine_fasta.rs:27-113
// The reference hands every gene to an external aligner (FoldMason by default); here the aligner is a centre-star MSA on the engine's own 3Di+AA
// gapped stage.  The reference reads its alignments back through hash maps; rows stay in file order here.
#include <dirent.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "uc_engine.h"
#include "uc_files.h"
#include "uc_msa.h"

namespace uc {

namespace {

void need(const void *p, const char *what) { if (!p) fail(UC_ERR_ARGS, "star MSA: %s must not be NULL", what); }

// grp_off: starts at 0, every group 1 .. MSA_MAX_ROWS rows; returns the row count
uint64_t check_groups(uint32_t n_groups, const uint64_t *grp_off) {
    if (!n_groups) return 0;
    need(grp_off, "grp_off");
    if (grp_off[0] != 0) fail(UC_ERR_ARGS, "star MSA: grp_off[0] must be 0");
    for (uint32_t g = 0; g < n_groups; g++) {
        if (grp_off[g + 1] <= grp_off[g]) fail(UC_ERR_ARGS, "star MSA: group %u is empty or grp_off decreases", g);
        if (grp_off[g + 1] - grp_off[g] > MSA_MAX_ROWS) fail(UC_ERR_ARGS, "star MSA: group %u has more than %u rows", g, MSA_MAX_ROWS);
    }
    return grp_off[n_groups];
}

}  // namespace

void msa_center_validate(const MsaCenterArgs &a, std::vector<uint64_t> &tri_off) {
    check_groups(a.n_groups, a.grp_off);
    tri_off.assign((size_t)a.n_groups + 1, 0);
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g];
        tri_off[g + 1] = tri_off[g] + m * (m - 1) / 2;
    }
    if (a.n_groups) need(a.centre, "centre");
    if (tri_off[a.n_groups]) need(a.scores, "scores");
}

void msa_center_host(const MsaCenterArgs &a, const std::vector<uint64_t> &tri_off) {
    std::vector<int64_t> sum;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g];
        const int32_t *t = a.scores + tri_off[g];
        sum.assign(m, 0);
        uint64_t k = 0;
        for (uint64_t i = 0; i < m; i++)
            for (uint64_t j = i + 1; j < m; j++, k++) { sum[i] += t[k]; sum[j] += t[k]; }
        uint64_t best = 0;
        for (uint64_t i = 1; i < m; i++) if (sum[i] > sum[best]) best = i;
        a.centre[g] = (uint32_t)best;
    }
}

void msa_star_validate(const MsaStarArgs &a, MsaStarPlan &plan) {
    if (a.n_tracks != 1 && a.n_tracks != 2) fail(UC_ERR_ARGS, "star MSA: %u tracks (1 or 2)", a.n_tracks);
    const uint64_t n_rows = check_groups(a.n_groups, a.grp_off);
    plan.n_rows = n_rows;
    plan.slot_off.assign((size_t)a.n_groups + 1, 0);
    plan.max_columns = 0;
    if (!a.n_groups) return;
    need(a.centre, "centre"); need(a.res_off, "res_off"); need(a.qs, "qs"); need(a.ts, "ts"); need(a.run_off, "run_off"); need(a.aligned, "aligned");
    need(a.width, "width");
    if (a.res_off[0] != 0 || a.run_off[0] != 0) fail(UC_ERR_ARGS, "star MSA: res_off[0] and run_off[0] must be 0");
    for (uint64_t r = 0; r < n_rows; r++) {
        if (a.res_off[r + 1] < a.res_off[r] || a.res_off[r + 1] - a.res_off[r] > 0x7fffffffull) fail(UC_ERR_ARGS, "star MSA: row %llu has a malformed residue range", (unsigned long long)r);
        if (a.run_off[r + 1] < a.run_off[r]) fail(UC_ERR_ARGS, "star MSA: run_off decreases at row %llu", (unsigned long long)r);
    }
    if (a.res_off[n_rows]) { need(a.res[0], "the residues of track 0"); if (a.n_tracks == 2) need(a.res[1], "the residues of track 1"); }
    if (a.run_off[n_rows]) need(a.runs, "runs");
    uint64_t cols = 0, centre_cols = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b;
        if (a.centre[g] >= m) fail(UC_ERR_ARGS, "star MSA: centre %u of group %u with %llu rows", a.centre[g], g, (unsigned long long)m);
        const uint64_t Lc = a.res_off[b + a.centre[g] + 1] - a.res_off[b + a.centre[g]];
        plan.slot_off[g + 1] = plan.slot_off[g] + Lc + 1;
        cols += Lc; centre_cols += Lc;
        for (uint64_t r = b; r < b + m; r++) {
            if (r == b + a.centre[g] || !a.aligned[r]) continue;
            const uint64_t Lr = a.res_off[r + 1] - a.res_off[r];
            if (a.qs[r] < 0 || a.ts[r] < 0) fail(UC_ERR_ARGS, "star MSA: row %llu starts at a negative position", (unsigned long long)r);
            uint64_t s = (uint64_t)a.qs[r], t = (uint64_t)a.ts[r];
            uint32_t prev = 3;
            for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                const uint32_t w = a.runs[k], op = w & 3u, len = w >> 2;
                if (op == 3u || len == 0) fail(UC_ERR_ARGS, "star MSA: word 0x%x of row %llu is no run", w, (unsigned long long)r);
                if (op == prev) fail(UC_ERR_ARGS, "star MSA: adjacent runs of row %llu share an operation", (unsigned long long)r);
                prev = op;
                if (op != 2u) s += len;
                if (op != 1u) t += len;
                if (op == 2u) cols += len;
            }
            if (s > Lc || t > Lr)      // lengths only grow: the ends bound every intermediate position
                fail(UC_ERR_ARGS, "star MSA: the backtrace of row %llu overruns a sequence (centre %llu of %llu, row %llu of %llu)", (unsigned long long)r,
                     (unsigned long long)s, (unsigned long long)Lc, (unsigned long long)t, (unsigned long long)Lr);
        }
        if (cols >> 31) fail(UC_ERR_ARGS, "star MSA: 2^31 or more columns in one call");
    }
    plan.max_columns = cols;
    if (centre_cols) need(a.col, "col");      // one entry per centre position
}

void msa_star_host(const MsaStarArgs &a, const MsaStarPlan &plan) {
    const uint32_t ng = a.n_groups;
    if (a.need) a.need[0] = a.need[1] = 0;
    if (!ng) return;
    std::vector<uint32_t> ins(plan.slot_off[ng], 0), colx(plan.slot_off[ng], 0);
    uint64_t n_cols = 0, n_cells = 0, co = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, Lc = plan.slot_off[g + 1] - plan.slot_off[g] - 1;
        uint32_t *in = ins.data() + plan.slot_off[g], *cx = colx.data() + plan.slot_off[g];
        for (uint64_t r = b; r < b + m; r++) {
            if (r == b + a.centre[g] || !a.aligned[r]) continue;
            uint64_t s = (uint64_t)a.qs[r];
            for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                const uint32_t w = a.runs[k], len = w >> 2;
                if ((w & 3u) == 2u) in[s] = std::max(in[s], len); else s += len;
            }
        }
        uint32_t cum = 0;
        for (uint64_t s = 0; s <= Lc; s++) { cum += in[s]; cx[s] = (uint32_t)s + cum; }
        a.width[g] = cx[Lc];
        for (uint64_t c = 0; c < Lc; c++) a.col[co + c] = cx[c];
        co += Lc;
        n_cols += a.width[g]; n_cells += m * a.width[g];
    }
    if (a.need) { a.need[0] = n_cols; a.need[1] = n_cells; }
    if (n_cols > a.cnt_capacity || n_cells > a.cells_capacity)
        fail(UC_ERR_ARGS, "star MSA: %llu columns and %llu cell bytes do not fit the capacities %llu and %llu", (unsigned long long)n_cols, (unsigned long long)n_cells,
             (unsigned long long)a.cnt_capacity, (unsigned long long)a.cells_capacity);
    if (n_cols) need(a.cnt, "cnt");
    if (n_cells) { need(a.cells[0], "the cells of track 0"); if (a.n_tracks == 2) need(a.cells[1], "the cells of track 1"); }
    uint64_t wo = 0, cell = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, Lc = plan.slot_off[g + 1] - plan.slot_off[g] - 1, W = a.width[g];
        const uint32_t *in = ins.data() + plan.slot_off[g], *cx = colx.data() + plan.slot_off[g];
        for (uint32_t tr = 0; tr < a.n_tracks; tr++) {
            uint8_t *out = a.cells[tr] + cell;
            const uint8_t *res = a.res[tr];
            memset(out, '-', m * W);
            for (uint64_t r = b; r < b + m; r++) {
                uint8_t *o = out + (r - b) * W;
                const uint8_t *x = res + a.res_off[r];
                if (r == b + a.centre[g]) { for (uint64_t c = 0; c < Lc; c++) o[cx[c]] = x[c]; continue; }
                if (!a.aligned[r]) continue;
                uint64_t s = (uint64_t)a.qs[r], t = (uint64_t)a.ts[r];
                for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                    const uint32_t w = a.runs[k], len = w >> 2, op = w & 3u;
                    if (op == 0u) { for (uint32_t l = 0; l < len; l++) o[cx[s + l]] = x[t + l]; s += len; t += len; }
                    else if (op == 1u) s += len;
                    else { memcpy(o + (cx[s] - in[s]), x + t, len); t += len; }
                }
            }
        }
        for (uint64_t c = 0; c < W; c++) {
            uint32_t n = 0;
            for (uint64_t i = 0; i < m; i++) n += a.cells[0][cell + i * W + c] != (uint8_t)'-';
            a.cnt[wo + c] = n;
        }
        wo += W; cell += m * W;
    }
}

void msa_filter_validate(const MsaFilterArgs &a, MsaFilterPlan &plan) {
    if (a.threshold > 100) fail(UC_ERR_ARGS, "MSA filter: threshold %u outside 0 .. 100", a.threshold);
    check_groups(a.n_groups, a.grp_off);
    plan.col_off.assign((size_t)a.n_groups + 1, 0);
    plan.cell_off.assign((size_t)a.n_groups + 1, 0);
    if (!a.n_groups) return;
    need(a.width, "width"); need(a.fwidth, "fwidth");
    for (uint32_t g = 0; g < a.n_groups; g++) {
        plan.col_off[g + 1] = plan.col_off[g] + a.width[g];
        plan.cell_off[g + 1] = plan.cell_off[g] + (a.grp_off[g + 1] - a.grp_off[g]) * a.width[g];
        if (plan.col_off[g + 1] >> 31) fail(UC_ERR_ARGS, "MSA filter: 2^31 or more columns in one call");
    }
    if (plan.col_off[a.n_groups]) { need(a.keep, "keep"); need(a.cells, "cells"); need(a.fcells, "fcells"); }
}

void msa_filter_host(const MsaFilterArgs &a, const MsaFilterPlan &plan) {
    uint64_t fo = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g], W = a.width[g];
        const uint8_t *in = a.cells + plan.cell_off[g];
        uint8_t *keep = a.keep + plan.col_off[g];
        uint32_t fw = 0;
        for (uint64_t c = 0; c < W; c++) {      // tree.rs:304-318
            uint64_t n = 0;
            for (uint64_t i = 0; i < m; i++) n += in[i * W + c] != (uint8_t)'-';
            keep[c] = n * 100 >= (uint64_t)a.threshold * m;
            fw += keep[c];
        }
        a.fwidth[g] = fw;
        for (uint64_t i = 0; i < m; i++) {
            uint8_t *o = a.fcells + fo + i * fw;
            for (uint64_t c = 0, k = 0; c < W; c++) if (keep[c]) o[k++] = in[i * W + c];
        }
        fo += m * fw;
    }
}

namespace {

MsaStarArgs star_args(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, uint32_t n_tracks, const uint64_t *res_off, const uint8_t *res0,
                      const uint8_t *res1, const int32_t *qs, const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *width,
                      uint32_t *col, uint32_t *cnt, uint64_t cnt_capacity, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out) {
    return MsaStarArgs{n_groups, grp_off, centre, n_tracks, res_off, {res0, res1}, qs, ts, run_off, runs, aligned, width, col, cnt, cnt_capacity, {cells0, cells1},
                       cells_capacity, need_out};
}

// ---- the file level -------------------------------------------------------------------------------------------------------------------
bool env_is_one(const char *name) { const char *v = getenv(name); return v && !strcmp(v, "1"); }

struct Gene {
    std::string name;                    // the file's stem
    std::vector<uint32_t> seq;           // database sequence of every row
    std::vector<std::string> species;    // the row's name
};

// the *.txt files of the profile directory in ascending file-name byte order (tree.rs:63-67)
std::vector<Gene> read_genes(const std::string &dir, const std::unordered_map<std::string_view, uint32_t> &id_of, uint32_t max_rows = MSA_MAX_ROWS) {
    DIR *d = opendir(dir.c_str());
    if (!d) fail(UC_ERR_IO, "cannot open directory %s", dir.c_str());
    std::vector<std::string> files;
    while (const dirent *e = readdir(d)) {
        const std::string f = e->d_name;
        if (f.size() < 5 || f.compare(f.size() - 4, 4, ".txt") != 0) continue;
        struct stat st;
        if (stat((dir + "/" + f).c_str(), &st) == 0 && S_ISREG(st.st_mode)) files.push_back(f);
    }
    closedir(d);
    std::sort(files.begin(), files.end());
    std::vector<Gene> genes;
    for (const std::string &f : files) {
        const std::string path = dir + "/" + f, text = read_whole_file(path);
        Gene G;
        G.name = f.substr(0, f.size() - 4);
        size_t p = 0, line = 0;
        while (p < text.size()) {      // create_gene_specific_fasta.rs:60-76: exactly two fields, the gene must be in the database
            size_t e = text.find('\n', p);
            if (e == std::string::npos) e = text.size();
            line++;
            std::string_view fld[3];
            int k = 0;
            for (size_t q = p; q < e && k < 3;) {
                while (q < e && is_space(text[q])) q++;
                const size_t b = q;
                while (q < e && !is_space(text[q])) q++;
                if (q > b) fld[k++] = std::string_view(text.data() + b, q - b);
            }
            if (k != 2) fail(UC_ERR_IO, "%s: line %zu: Invalid line in gene mapping file (two fields expected)", path.c_str(), line);
            const auto it = id_of.find(fld[0]);
            if (it == id_of.end()) fail(UC_ERR_IO, "%s: line %zu: Sequence %.*s not found in the database", path.c_str(), line, (int)fld[0].size(), fld[0].data());
            G.seq.push_back(it->second);
            G.species.emplace_back(fld[1]);
            p = e + 1;
        }
        if (G.seq.size() > max_rows) fail(UC_ERR_ARGS, "%s: %zu rows; a group holds at most %u", path.c_str(), G.seq.size(), max_rows);
        genes.push_back(std::move(G));
    }
    return genes;
}

void append_fasta(std::string &out, const std::string &name, const uint8_t *seq, size_t n) {
    out += '>'; out += name; out += '\n'; out.append((const char *)seq, n); out += '\n';
}

// refine_iters rounds of UC-T/P (uc_msa_profile_host.cpp, uc_msa_profile.hip) between the star MSA and the filter; 0: the star MSA as it is
// progressive: UC-T/G (uc_msa_progressive_host.cpp, uc_msa_progressive.hip) in the star MSA's place
void tree_files(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, uint32_t refine_iters, const uc_opts *o,
                uc_tree_stats *st_out, uc_tree_refined_stats *rst_out, bool progressive = false, uc_tree_progressive_stats *pst_out = nullptr) {
    uc_tree_progressive_stats pst;
    memset(&pst, 0, sizeof pst);
    if (refine_iters > UC_TREE_MAX_REFINE) fail(UC_ERR_ARGS, "tree: %u refinement rounds; at most %u", refine_iters, (unsigned)UC_TREE_MAX_REFINE);
    uc_tree_refined_stats rst;
    memset(&rst, 0, sizeof rst);
    if (threshold > 100) fail(UC_ERR_ARGS, "tree: threshold %u outside 0 .. 100", threshold);
    int verbosity = 3, device = -1, threads = 1;
    std::string data_dir;
    if (o) {
        if (o->struct_size != sizeof(uc_opts)) fail(UC_ERR_ARGS, "uc_opts.struct_size mismatch (%u != %zu)", o->struct_size, sizeof(uc_opts));
        verbosity = o->verbosity; device = o->device; threads = o->threads > 0 ? o->threads : 1;
        if (o->data_dir) data_dir = o->data_dir;
    }
    // the gapped stage exactly as a `-a` search runs it, with every threshold open; what --aligner-options adds comes last and wins
    Params p;
    p.threads = threads;
    p.verbosity = verbosity == 4 ? 3 : verbosity == 3 ? 2 : verbosity;      // the engine logs on Foldseek's scale (cluster.rs:18)
    parse_cluster_options(std::string("-e 1e30 -c 0 --cov-mode 0 --min-seq-id 0 --rev-correction 0 --max-seqs 65535 ") + (aligner_options ? aligner_options : ""), p);
    p.want_bt = 1; p.want_tb = 1;
    uc_tree_stats st;
    memset(&st, 0, sizeof st);
    const std::string out = out_dir;
    {   // tree.rs:54-57,136: an existing concatenation is kept and nothing is touched
        struct stat sb;
        if (stat((out + "/combined.fasta").c_str(), &sb) == 0) {
            if (verbosity >= 3) { printf("Concatenated alignment file %s/combined.fasta already exists, skipping alignment step\n", out.c_str()); fflush(stdout); }
            if (st_out) *st_out = st;
            if (rst_out) { rst.tree = st; *rst_out = rst; }
            if (pst_out) { pst.tree = st; *pst_out = pst; }
            return;
        }
    }
    g_verbosity = p.verbosity;
    finalize_params(p, data_dir);
    if (refine_iters && (p.gap_ext < 0 || p.gap_open < p.gap_ext)) fail(UC_ERR_ARGS, "tree: gap open %d below gap extension %d; the profile rounds need open >= extension >= 0", p.gap_open, p.gap_ext);
    if (progressive && (p.gap_ext < 0 || p.gap_open < p.gap_ext)) fail(UC_ERR_ARGS, "tree: gap open %d below gap extension %d; the progressive aligner needs open >= extension >= 0", p.gap_open, p.gap_ext);
    Timer t_all, t_part;
    auto lap = [&](int phase) { st.seconds[phase] += t_part.seconds(); t_part = Timer(); };
    make_dirs(out);
    write_file(out + "/tree.chk", "0");      // tree.rs:36

    // ---- the database (codes for the engine, the stored letters for the files) and the gene files: every input is read and checked before the
    // device is asked for
    std::vector<Gene> genes;
    HostDb H;
    read_seq_db(db_prefix, H, true);
    const std::vector<IndexEntry> ia = read_index(std::string(db_prefix) + ".index"), is = read_index(std::string(db_prefix) + "_ss.index");
    const std::string raw_aa = read_whole_file(db_prefix), raw_3di = read_whole_file(std::string(db_prefix) + "_ss");
    {
        std::unordered_map<std::string_view, uint32_t> id_of;
        for (uint32_t i = 0; i < H.n; i++) id_of[H.names[i]] = i;      // a later entry of the same name replaces the earlier one (a HashMap insert)
        genes = read_genes(profile_dir, id_of, progressive ? MSA_PROG_MAX_ROWS : MSA_MAX_ROWS);
    }
    const uint32_t ng_all = (uint32_t)genes.size();
    Engine E(p, device);
    E.emit_bt = true;
    E.hdb = std::move(H);
    const HostDb &D = E.hdb;
    E.upload_db();
    make_dirs(out + "/fasta");
    std::string body, body2;
    for (const Gene &G : genes) {      // create_gene_specific_fasta.rs:50-79
        make_dirs(out + "/fasta/" + G.name);
        body.clear(); body2.clear();
        for (size_t r = 0; r < G.seq.size(); r++) {
            const uint32_t x = G.seq[r];
            append_fasta(body, G.species[r], (const uint8_t *)raw_aa.data() + ia[x].off, D.len(x));
            append_fasta(body2, G.species[r], (const uint8_t *)raw_3di.data() + is[x].off, D.len(x));
        }
        write_file(out + "/fasta/" + G.name + "/aa.fasta", body);
        write_file(out + "/fasta/" + G.name + "/3di.fasta", body2);
    }
    // the groups the MSA runs on: a gene file without a line has no rows to align
    std::vector<uint32_t> live;
    for (uint32_t g = 0; g < ng_all; g++) {
        if (!genes[g].seq.empty()) live.push_back(g);
        else if (verbosity >= 2) fprintf(stderr, "Warning: gene %s has no sequence; it is left out of the concatenated alignment\n", genes[g].name.c_str());
    }
    const uint32_t ng = (uint32_t)live.size();
    std::vector<uint64_t> grp_off((size_t)ng + 1, 0);
    for (uint32_t k = 0; k < ng; k++) grp_off[k + 1] = grp_off[k] + genes[live[k]].seq.size();
    const uint64_t n_rows = grp_off[ng];
    std::vector<uint32_t> row_seq(n_rows);
    for (uint32_t k = 0; k < ng; k++) std::copy(genes[live[k]].seq.begin(), genes[live[k]].seq.end(), row_seq.begin() + grp_off[k]);
    st.n_groups = ng_all; st.n_rows = n_rows;
    const bool on_host = env_is_one("UC_TREE_HOST"), dump = env_is_one("UC_TREE_DUMP");
    const uint64_t budget = tree_budget_bytes();
    lap(0);

    // ---- UC-T/C: all pairs of every group, scores only, batched over whole groups under the byte budget; then the centres
    std::vector<uint32_t> centre(ng, 0);
    std::vector<int32_t> tri_all;      // progressive: every group's triangle, groups back to back
    {
        const uint64_t max_pairs = std::max<uint64_t>(budget / 64, 1);      // a pair of sw_batch: ids, plan and three results on both sides
        std::vector<PairIn> pairs;
        std::vector<int32_t> score;
        std::vector<uint64_t> off;
        for (uint32_t g0 = 0; g0 < ng;) {
            uint32_t g1 = g0;
            uint64_t np = 0;
            while (g1 < ng) {
                const uint64_t m = grp_off[g1 + 1] - grp_off[g1], k = m * (m - 1) / 2;
                if (g1 > g0 && np + k > max_pairs) break;
                np += k; g1++;
            }
            pairs.clear(); pairs.reserve(np);
            off.assign(1, 0);
            for (uint32_t g = g0; g < g1; g++) {
                const uint32_t *s = row_seq.data() + grp_off[g];
                const uint64_t m = grp_off[g + 1] - grp_off[g];
                for (uint64_t i = 0; i < m; i++)
                    for (uint64_t j = i + 1; j < m; j++) pairs.push_back(PairIn{s[i], s[j], 0, 0});
                off.push_back(off.back() + m);
            }
            score.assign(std::max<uint64_t>(np, 1), 0);
            Timer t_dp;
            if (np) E.sw_batch(0, pairs, score.data(), nullptr, nullptr);
            st.seconds[1] += t_dp.seconds();
            st.n_pairs_scored += np;
            if (progressive) tri_all.insert(tri_all.end(), score.begin(), score.begin() + np);
            Timer t_c;
            const MsaCenterArgs ca{g1 - g0, off.data(), score.data(), centre.data() + g0};
            std::vector<uint64_t> tri;
            msa_center_validate(ca, tri);
            if (!progressive) { if (on_host) msa_center_host(ca, tri); else msa_center_device(E.device, ca, tri); }      // progressive: the triangle feeds the guide trees, no centre
            st.seconds[2] += t_c.seconds();
            if (dump)
                for (uint32_t g = g0; g < g1; g++) {
                    const uint64_t m = grp_off[g + 1] - grp_off[g];
                    std::string txt = progressive ? std::string() : "#centre\t" + std::to_string(centre[g]) + "\n";
                    uint64_t k = tri[g - g0];
                    for (uint64_t i = 0; i < m; i++)
                        for (uint64_t j = i + 1; j < m; j++, k++) txt += std::to_string(i) + "\t" + std::to_string(j) + "\t" + std::to_string(score[k]) + "\n";
                    write_file(out + "/fasta/" + genes[live[g]].name + "/pair_scores.tsv", txt);
                }
            g0 = g1;
        }
        t_part = Timer();
    }

    // ---- the centre against every other row of its group with backtraces: one hit list per centre sequence, targets ascending and unique
    std::vector<int32_t> qs(n_rows, 0), ts(n_rows, 0);
    std::vector<uint8_t> aligned(n_rows, 0);
    std::vector<uint64_t> run_off(n_rows + 1, 0);
    std::vector<uint32_t> runs;
    if (!progressive) {
        std::vector<uint64_t> want;      // centre sequence << 32 | member sequence
        for (uint32_t g = 0; g < ng; g++) {
            const uint64_t b = grp_off[g], c = row_seq[b + centre[g]];
            for (uint64_t r = b; r < grp_off[g + 1]; r++) if (r != b + centre[g]) want.push_back(c << 32 | row_seq[r]);
        }
        std::sort(want.begin(), want.end());
        want.erase(std::unique(want.begin(), want.end()), want.end());
        std::vector<uint32_t> counts(D.n, 0);
        std::vector<uc_hit> hits(std::max<size_t>(want.size(), 1));
        for (size_t k = 0; k < want.size(); k++) { counts[want[k] >> 32]++; hits[k] = uc_hit{(uint32_t)want[k], 0, 0}; }
        std::vector<uc_aln> alns(std::max<size_t>(want.size(), 1));
        std::vector<uint64_t> bt_off(want.size() + 1, 0);
        std::vector<uint32_t> bt_runs;
        if (!want.empty()) {
            E.set_hits(counts.data(), hits.data(), false);      // a centre that serves several groups may list more than --max-seqs rows
            E.align(0, D.n);
            E.get_alns(0, want.size(), alns.data());
            E.get_backtraces(0, want.size(), bt_off.data(), bt_runs);
        }
        for (uint32_t g = 0; g < ng; g++) {
            const uint64_t b = grp_off[g], c = row_seq[b + centre[g]];
            for (uint64_t r = b; r < grp_off[g + 1]; r++) {
                run_off[r + 1] = run_off[r];
                if (r == b + centre[g]) { aligned[r] = 1; continue; }
                const size_t k = std::lower_bound(want.begin(), want.end(), c << 32 | row_seq[r]) - want.begin();
                const uc_aln &al = alns[k];
                if (!al.accepted) { st.n_rows_unaligned++; continue; }
                aligned[r] = 1; qs[r] = al.qstart; ts[r] = al.tstart;
                runs.insert(runs.end(), bt_runs.begin() + bt_off[k], bt_runs.begin() + bt_off[k + 1]);
                run_off[r + 1] = runs.size();
            }
        }
    }
    lap(3);

    // ---- UC-T/L, rows, UC-T/F: whole groups per call under the byte budget
    std::vector<uint64_t> res_off(n_rows + 1, 0);
    for (uint64_t r = 0; r < n_rows; r++) res_off[r + 1] = res_off[r] + D.len(row_seq[r]);
    std::vector<uint8_t> res_aa(std::max<uint64_t>(res_off[n_rows], 1)), res_3di(std::max<uint64_t>(res_off[n_rows], 1));
    for (uint64_t r = 0; r < n_rows; r++) {
        memcpy(res_aa.data() + res_off[r], raw_aa.data() + ia[row_seq[r]].off, D.len(row_seq[r]));
        memcpy(res_3di.data() + res_off[r], raw_3di.data() + is[row_seq[r]].off, D.len(row_seq[r]));
    }
    std::vector<uint64_t> bound(ng, 0);      // cell bytes of a group at most: rows x (centre length + every D run)
    for (uint32_t g = 0; g < ng; g++) {
        uint64_t w = D.len(row_seq[grp_off[g] + centre[g]]);
        for (uint64_t k = run_off[grp_off[g]]; k < run_off[grp_off[g + 1]]; k++) if ((runs[k] & 3u) == 2u) w += runs[k] >> 2;
        bound[g] = w;
    }
    // ---- UC-T/G: self scores, guide trees and the merges of all genes together, level by level
    std::vector<uint32_t> pg_width(progressive ? ng : 0);
    std::vector<uint8_t> pg_cells[2];
    std::vector<uint64_t> pg_cell_off((size_t)ng + 1, 0);
    if (progressive && ng) {
        lap(0);      // the guide trees and the merges are booked with layout + render + filter, not with reading
        Timer t_g;
        std::vector<int64_t> self(n_rows);
        msa_self_scores(n_rows, res_off.data(), res_aa.data(), res_3di.data(), p.SA, p.S3, self.data());
        uint64_t nd = 0;
        for (uint32_t g = 0; g < ng; g++) { const uint64_t m = grp_off[g + 1] - grp_off[g]; nd += m * m; }
        std::vector<double> Dm(nd);
        std::vector<uint32_t> merges(std::max<uint64_t>(2 * (n_rows - ng), 1));
        const MsaGuideArgs ga{ng, grp_off.data(), tri_all.data(), self.data(), Dm.data(), merges.data()};
        std::vector<uint64_t> tri;
        msa_guide_validate(ga, tri);
        msa_guide_run(ga, tri, !on_host, E.device);
        pst.seconds[0] = t_g.seconds();
        if (dump) {
            uint64_t d0 = 0;
            char num[64];
            for (uint32_t g = 0; g < ng; g++) {
                const uint64_t m = grp_off[g + 1] - grp_off[g];
                std::string txt;
                for (uint64_t i = 0; i < m; i++)
                    for (uint64_t j = i + 1; j < m; j++) { snprintf(num, sizeof num, "%.17g", Dm[d0 + i * m + j]); txt += "#D\t" + std::to_string(i) + "\t" + std::to_string(j) + "\t" + num + "\n"; }
                const uint32_t *mg = merges.data() + 2 * (grp_off[g] - g);
                for (uint64_t k = 0; k + 1 < m; k++) txt += std::to_string(k) + "\t" + std::to_string(mg[2 * k]) + "\t" + std::to_string(mg[2 * k + 1]) + "\n";
                write_file(out + "/fasta/" + genes[live[g]].name + "/guide.tsv", txt);
                d0 += m * m;
            }
        }
        Timer t_m;
        uint64_t cap = 0;
        for (uint32_t g = 0; g < ng; g++) cap += (grp_off[g + 1] - grp_off[g]) * (res_off[grp_off[g + 1]] - res_off[grp_off[g]]);
        pg_cells[0].resize(std::max<uint64_t>(cap, 1)); pg_cells[1].resize(std::max<uint64_t>(cap, 1));
        MsaProgStats ps{0, 0, 0, 0};
        const MsaProgressiveArgs pa{ng, grp_off.data(), res_off.data(), {res_aa.data(), res_3di.data()}, merges.data(), {p.SA, p.S3}, p.gap_open, p.gap_ext, pg_width.data(),
                                    {pg_cells[0].data(), pg_cells[1].data()}, cap, nullptr, &ps};
        MsaProgressivePlan pp;
        msa_progressive_validate(pa, pp);
        if (on_host) msa_progressive_host(pa, pp, (uint32_t)threads); else msa_progressive_device(E.device, pa, pp);
        pst.seconds[1] = t_m.seconds();
        pst.n_groups_aligned = ng; pst.n_merges = ps.n_merges; pst.n_levels = ps.n_levels; pst.n_launches = ps.n_launches; pst.n_cells = ps.n_cells;
        for (uint32_t g = 0; g < ng; g++) { bound[g] = pg_width[g]; pg_cell_off[g + 1] = pg_cell_off[g] + (grp_off[g + 1] - grp_off[g]) * pg_width[g]; }
        lap(4);
    }
    struct Kept { uint32_t gene; uint32_t fw; std::vector<uint8_t> cells; };      // the filtered amino-acid rows of a group that kept a column
    std::vector<Kept> kept;
    lap(0);
    for (uint32_t g0 = 0; g0 < ng;) {
        uint32_t g1 = g0;
        uint64_t cols = 0, cells = 0;
        while (g1 < ng) {
            const uint64_t m = grp_off[g1 + 1] - grp_off[g1];
            if (g1 > g0 && (cells + m * bound[g1]) * 4 > budget) break;
            cols += bound[g1]; cells += m * bound[g1]; g1++;
        }
        const uint32_t n = g1 - g0;
        const uint64_t r0 = grp_off[g0], r1 = grp_off[g1];
        std::vector<uint64_t> go(n + 1), ro(r1 - r0 + 1), uo(r1 - r0 + 1);
        for (uint32_t k = 0; k <= n; k++) go[k] = grp_off[g0 + k] - r0;
        for (uint64_t r = r0; r <= r1; r++) { ro[r - r0] = res_off[r] - res_off[r0]; uo[r - r0] = run_off[r] - run_off[r0]; }
        std::vector<uint32_t> width(n), col(std::max<uint64_t>(cols, 1)), cnt(std::max<uint64_t>(cols, 1)), fwidth(n);
        std::vector<uint8_t> c_aa(std::max<uint64_t>(cells, 1)), c_3di(std::max<uint64_t>(cells, 1)), keep(std::max<uint64_t>(cols, 1)), f_aa(std::max<uint64_t>(cells, 1));
        const MsaStarArgs sa = star_args(n, go.data(), centre.data() + g0, 2, ro.data(), res_aa.data() + res_off[r0], res_3di.data() + res_off[r0], qs.data() + r0, ts.data() + r0,
                                         uo.data(), runs.data() + run_off[r0], aligned.data() + r0, width.data(), col.data(), cnt.data(), cols, c_aa.data(), c_3di.data(), cells,
                                         nullptr);
        if (progressive) {      // the roots as they are
            for (uint32_t k = 0; k < n; k++) width[k] = pg_width[g0 + k];
            const uint64_t nb = pg_cell_off[g1] - pg_cell_off[g0];
            if (nb) { memcpy(c_aa.data(), pg_cells[0].data() + pg_cell_off[g0], nb); memcpy(c_3di.data(), pg_cells[1].data() + pg_cell_off[g0], nb); }
        } else {
            MsaStarPlan sp;
            msa_star_validate(sa, sp);
            if (on_host) msa_star_host(sa, sp); else msa_star_device(E.device, sa, sp);
        }
        if (refine_iters) {      // ---- UC-T/P: every round realigns the rows against the profile of the others and lays the group out again
            const uint64_t nr = r1 - r0;
            std::vector<uint8_t> p_al(nr), was(nr);
            std::vector<int32_t> p_sc(nr), p_qs(nr), p_ts(nr), p_qe(nr), p_te(nr);
            std::vector<uint64_t> p_uo(nr + 1, 0);
            std::vector<uint32_t> p_runs, nw(n);
            std::vector<std::string> tsv(dump ? n : 0);
            for (uint64_t r = 0; r < nr; r++) was[r] = aligned[r0 + r];      // the centre counts as aligned
            for (uint32_t round = 0; round < refine_iters; round++) {
                Timer t_r;
                uint64_t cap = 0, wsum = 0;
                for (uint32_t k = 0; k < n; k++) { for (uint64_t r = go[k]; r < go[k + 1]; r++) cap += width[k] + (ro[r + 1] - ro[r]); wsum += width[k]; }
                p_runs.resize(std::max<uint64_t>(cap, 1));
                const MsaProfileAlignArgs pa{n, go.data(), width.data(), {c_aa.data(), c_3di.data()}, ro.data(), {res_aa.data() + res_off[r0], res_3di.data() + res_off[r0]},
                                             {p.SA, p.S3}, p.gap_open, p.gap_ext, p_al.data(), p_sc.data(), p_qs.data(), p_ts.data(), p_qe.data(), p_te.data(), p_uo.data(),
                                             p_runs.data(), cap, nullptr};
                MsaProfilePlan pp;
                msa_profile_align_validate(pa, pp);
                if (on_host) msa_profile_align_host(pa, pp, (uint32_t)threads); else msa_profile_align_device(E.device, pa, pp);
                rst.seconds[0] += t_r.seconds();
                Timer t_l;
                uint64_t ccap = 0;
                const MsaProfileLayoutArgs la{n, go.data(), width.data(), {c_aa.data(), c_3di.data()}, ro.data(), {res_aa.data() + res_off[r0], res_3di.data() + res_off[r0]},
                                              p_al.data(), p_qs.data(), p_ts.data(), p_uo.data(), p_runs.data(), nw.data(), {nullptr, nullptr}, 0, nullptr};
                MsaProfileLayoutPlan lp;
                msa_profile_layout_validate(la, lp);
                for (uint32_t k = 0; k < n; k++) ccap += (go[k + 1] - go[k]) * lp.bound[k];
                std::vector<uint8_t> n_aa(std::max<uint64_t>(ccap, 1)), n_3di(std::max<uint64_t>(ccap, 1));
                MsaProfileLayoutArgs lb = la;
                lb.cells[0] = n_aa.data(); lb.cells[1] = n_3di.data(); lb.cells_capacity = ccap;
                if (on_host) msa_profile_layout_host(lb, lp); else msa_profile_layout_device(E.device, lb, lp);
                rst.seconds[1] += t_l.seconds();
                rst.n_rounds = std::max<uint64_t>(rst.n_rounds, round + 1);
                rst.n_tasks += pp.n_tasks; rst.n_cells += pp.n_cells;
                rst.width_before[round] += wsum;
                for (uint32_t k = 0; k < n; k++) {
                    const bool single = go[k + 1] - go[k] == 1;
                    rst.width_after[round] += nw[k];
                    for (uint64_t r = go[k]; r < go[k + 1]; r++) {
                        const uint8_t now = single ? was[r] : p_al[r];
                        rst.n_rows_became_aligned += now && !was[r]; rst.n_rows_became_unaligned += !now && was[r];
                        was[r] = now;
                        if (dump) tsv[k] += std::to_string(round + 1) + "\t" + std::to_string(r - go[k]) + "\t" + std::to_string(p_sc[r]) + "\t" + std::to_string(p_qs[r]) + "\t" +
                                            std::to_string(p_ts[r]) + "\n";
                    }
                }
                width = nw; c_aa.swap(n_aa); c_3di.swap(n_3di);
            }
            for (uint32_t k = 0; k < n; k++) if (dump) write_file(out + "/fasta/" + genes[live[g0 + k]].name + "/refine.tsv", tsv[k]);
            for (uint64_t r = 0; r < nr; r++) rst.tree.n_rows_unaligned += !was[r];
            uint64_t nc = 0, ncell = 0;
            for (uint32_t k = 0; k < n; k++) { nc += width[k]; ncell += (go[k + 1] - go[k]) * width[k]; }
            keep.assign(std::max<uint64_t>(nc, 1), 0); f_aa.assign(std::max<uint64_t>(ncell, 1), 0);
        }
        const MsaFilterArgs fa{n, go.data(), width.data(), c_aa.data(), threshold, keep.data(), fwidth.data(), f_aa.data()};
        MsaFilterPlan fp;
        msa_filter_validate(fa, fp);
        if (on_host) msa_filter_host(fa, fp); else msa_filter_device(E.device, fa, fp);
        lap(4);
        uint64_t fo = 0;
        for (uint32_t k = 0; k < n; k++) {      // <gene>.fa, <gene>_3di.fa, <gene>.fa.filtered: rows in file order
            const Gene &G = genes[live[g0 + k]];
            const uint64_t m = go[k + 1] - go[k], W = width[k], fw = fwidth[k];
            const std::string dir = out + "/fasta/" + G.name + "/";
            std::string a, d, f;
            for (uint64_t i = 0; i < m; i++) {
                append_fasta(a, G.species[i], c_aa.data() + fp.cell_off[k] + i * W, W);
                append_fasta(d, G.species[i], c_3di.data() + fp.cell_off[k] + i * W, W);
                append_fasta(f, G.species[i], f_aa.data() + fo + i * fw, fw);
            }
            write_file(dir + G.name + ".fa", a);
            write_file(dir + G.name + "_3di.fa", d);
            write_file(dir + G.name + ".fa.filtered", f);
            st.n_columns += W; st.n_columns_kept += fw;
            if (fw) kept.push_back(Kept{live[g0 + k], (uint32_t)fw, std::vector<uint8_t>(f_aa.begin() + fo, f_aa.begin() + fo + m * fw)});
            else {
                st.n_groups_dropped++;
                if (verbosity >= 2) fprintf(stderr, "Warning: gene %s keeps no column under threshold %u; it is left out of the concatenated alignment\n", G.name.c_str(), threshold);
            }
            fo += m * fw;
        }
        lap(5);
        g0 = g1;
    }
    for (uint32_t g = 0; g < ng_all; g++) if (genes[g].seq.empty()) st.n_groups_dropped++;

    // ---- combined.fasta and its partitions (combine_fasta.rs:27-113): names by first appearance over the kept groups
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> name_id;
    for (const Kept &K : kept)
        for (const std::string &s : genes[K.gene].species) if (name_id.emplace(s, (uint32_t)names.size()).second) names.push_back(s);
    uint64_t total = 0;
    for (const Kept &K : kept) total += K.fw;
    std::vector<std::string> seqs(names.size(), std::string(total, '-'));
    std::string parts;
    uint64_t at = 0;
    std::vector<uint8_t> seen(names.size());
    for (const Kept &K : kept) {
        const Gene &G = genes[K.gene];
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t i = 0; i < G.species.size(); i++) {      // a name listed twice in one gene file: its first row
            const uint32_t id = name_id[G.species[i]];
            if (seen[id]) continue;
            seen[id] = 1;
            memcpy(&seqs[id][at], K.cells.data() + i * K.fw, K.fw);
        }
        parts += "JTT+F+I+G, " + G.name + "=" + std::to_string(at + 1) + "-" + std::to_string(at + K.fw) + "\n";      // combine_fasta.rs:93
        at += K.fw;
    }
    body.clear();
    for (size_t i = 0; i < names.size(); i++) { body += '>'; body += names[i]; body += '\n'; body += seqs[i]; body += '\n'; }
    write_file(out + "/combined.fasta.partitions", parts);
    write_file(out + "/combined.fasta", body);
    lap(5);
    st.seconds[6] = t_all.seconds();
    if (verbosity >= 3) {
        printf("Aligning genes %u/%u... Done\n", ng, ng_all);
        printf("%llu rows in %u genes, %llu pairs scored, %llu rows unaligned, %llu of %llu columns kept, %llu genes dropped\n", (unsigned long long)n_rows, ng_all,
               (unsigned long long)st.n_pairs_scored, (unsigned long long)st.n_rows_unaligned, (unsigned long long)st.n_columns_kept, (unsigned long long)st.n_columns,
               (unsigned long long)st.n_groups_dropped);
        fflush(stdout);
    }
    if (getenv("UC_TIMING"))
        fprintf(stderr, "unicore-cluster[timing]: tree (%s layout): read %.3f s, all-pairs scores %.3f s, centres %.3f s, centre alignments %.3f s, layout + render + filter %.3f s, "
                        "write %.3f s, total %.3f s\n", on_host ? "host" : "device", st.seconds[0], st.seconds[1], st.seconds[2], st.seconds[3], st.seconds[4], st.seconds[5], st.seconds[6]);
    if (refine_iters) st.n_rows_unaligned = rst.tree.n_rows_unaligned;
    rst.seconds[2] = rst.seconds[0] + rst.seconds[1];
    if (refine_iters && verbosity >= 3) {
        printf("%llu refinement rounds: %llu profile alignments over %llu cells, %llu rows became aligned, %llu unaligned\n", (unsigned long long)rst.n_rounds,
               (unsigned long long)rst.n_tasks, (unsigned long long)rst.n_cells, (unsigned long long)rst.n_rows_became_aligned, (unsigned long long)rst.n_rows_became_unaligned);
        fflush(stdout);
    }
    if (refine_iters && getenv("UC_TIMING"))
        fprintf(stderr, "unicore-cluster[timing]: tree refinement (%s): profile DP + walk %.3f s, layout + compaction %.3f s\n", on_host ? "host" : "device", rst.seconds[0], rst.seconds[1]);
    pst.seconds[2] = pst.seconds[0] + pst.seconds[1];
    pst.width_before = st.n_columns; pst.width_after = st.n_columns_kept;
    if (progressive && verbosity >= 3) {
        printf("progressive MSA: %llu merges in %llu levels, %llu kernel launches, %llu cells\n", (unsigned long long)pst.n_merges, (unsigned long long)pst.n_levels,
               (unsigned long long)pst.n_launches, (unsigned long long)pst.n_cells);
        fflush(stdout);
    }
    if (progressive && getenv("UC_TIMING"))
        fprintf(stderr, "unicore-cluster[timing]: tree progressive (%s): self scores + guide trees %.3f s, merges %.3f s\n", on_host ? "host" : "device", pst.seconds[0], pst.seconds[1]);
    if (st_out) *st_out = st;
    if (rst_out) { rst.tree = st; *rst_out = rst; }
    if (pst_out) { pst.tree = st; *pst_out = pst; }
}

}  // namespace

}  // namespace uc

using namespace uc;

int uc_msa_center(uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, uint32_t *centre) {
    return guard([&] {
        const MsaCenterArgs a{n_groups, grp_off, scores, centre};
        std::vector<uint64_t> tri;
        msa_center_validate(a, tri);
        msa_center_host(a, tri);
    });
}

int uc_msa_center_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, uint32_t *centre) {
    return guard([&] {
        const MsaCenterArgs a{n_groups, grp_off, scores, centre};
        std::vector<uint64_t> tri;
        msa_center_validate(a, tri);
        msa_center_device(device, a, tri);
    });
}

int uc_msa_star(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, uint32_t n_tracks, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1,
                const int32_t *qs, const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *width, uint32_t *col, uint32_t *cnt,
                uint64_t cnt_capacity, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out) {
    return guard([&] {
        const MsaStarArgs a = star_args(n_groups, grp_off, centre, n_tracks, res_off, res0, res1, qs, ts, run_off, runs, aligned, width, col, cnt, cnt_capacity, cells0, cells1,
                                        cells_capacity, need_out);
        MsaStarPlan plan;
        msa_star_validate(a, plan);
        msa_star_host(a, plan);
    });
}

int uc_msa_star_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, uint32_t n_tracks, const uint64_t *res_off, const uint8_t *res0,
                    const uint8_t *res1, const int32_t *qs, const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *width,
                    uint32_t *col, uint32_t *cnt, uint64_t cnt_capacity, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out) {
    return guard([&] {
        const MsaStarArgs a = star_args(n_groups, grp_off, centre, n_tracks, res_off, res0, res1, qs, ts, run_off, runs, aligned, width, col, cnt, cnt_capacity, cells0, cells1,
                                        cells_capacity, need_out);
        MsaStarPlan plan;
        msa_star_validate(a, plan);
        if (plan.max_columns) { if (!cnt) fail(UC_ERR_ARGS, "star MSA: cnt must not be NULL"); if (!cells0 || (n_tracks == 2 && !cells1)) fail(UC_ERR_ARGS, "star MSA: cells must not be NULL"); }
        msa_star_device(device, a, plan);
    });
}

int uc_msa_filter(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells, uint32_t threshold, uint8_t *keep, uint32_t *fwidth,
                  uint8_t *fcells) {
    return guard([&] {
        const MsaFilterArgs a{n_groups, grp_off, width, cells, threshold, keep, fwidth, fcells};
        MsaFilterPlan plan;
        msa_filter_validate(a, plan);
        msa_filter_host(a, plan);
    });
}

int uc_msa_filter_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells, uint32_t threshold, uint8_t *keep,
                      uint32_t *fwidth, uint8_t *fcells) {
    return guard([&] {
        const MsaFilterArgs a{n_groups, grp_off, width, cells, threshold, keep, fwidth, fcells};
        MsaFilterPlan plan;
        msa_filter_validate(a, plan);
        msa_filter_device(device, a, plan);
    });
}

int uc_tree(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, const uc_opts *o, uc_tree_stats *stats_out) {
    return guard([&] {
        if (!db_prefix || !profile_dir || !out_dir) fail(UC_ERR_ARGS, "tree: db_prefix, profile_dir and out_dir must not be NULL");
        tree_files(db_prefix, profile_dir, out_dir, threshold, aligner_options, 0, o, stats_out, nullptr);
    });
}

int uc_tree_refined(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, uint32_t refine_iters,
                    const uc_opts *o, uc_tree_refined_stats *stats_out) {
    return guard([&] {
        if (!db_prefix || !profile_dir || !out_dir) fail(UC_ERR_ARGS, "tree: db_prefix, profile_dir and out_dir must not be NULL");
        tree_files(db_prefix, profile_dir, out_dir, threshold, aligner_options, refine_iters, o, nullptr, stats_out);
    });
}

int uc_tree_progressive(const char *db_prefix, const char *profile_dir, const char *out_dir, uint32_t threshold, const char *aligner_options, const uc_opts *o,
                        uc_tree_progressive_stats *stats_out) {
    return guard([&] {
        if (!db_prefix || !profile_dir || !out_dir) fail(UC_ERR_ARGS, "tree: db_prefix, profile_dir and out_dir must not be NULL");
        tree_files(db_prefix, profile_dir, out_dir, threshold, aligner_options, 0, o, nullptr, nullptr, true, stats_out);
    });
}
