// nj_boot_host_check.cpp — the host side of rule UC-N/B (uc_nj_boot_host.cpp over uc_nj_host.cpp) in a program of its own, for the address and
// undefined-behaviour sanitizers: test_nj_boot.py builds it with -fsanitize=address,undefined together with the two host sources and runs it; nothing
// is preloaded.  The pieces of the library that the sources lean on and that are not under test here (the error text, file reading, the device
// side) are stand-ins below.  `nj_boot_host_check draws W SEED REP COUNT` prints the first COUNT draws of a replicate from uc_nj.h's own function.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "uc_db.h"
#include "uc_nj.h"

namespace uc {
static std::string g_error;
void set_last_error(const std::string &m) { g_error = m; }
std::string read_whole_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) fail(UC_ERR_IO, "cannot read %s", path.c_str());
    std::string s;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, k);
    fclose(f);
    return s;
}
void nj_counts_device(int, const NjCountArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void nj_join_device(int, const NjJoinArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void nj_boot_counts_device(int, const NjBootCountArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void nj_join_batch_device(int, const NjJoinBatchArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
}  // namespace uc

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "nj_boot_host_check: %s (%s)\n", what, uc::g_error.c_str()); exit(1); }
}

static std::string slurp(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return "<missing>";
    std::string s;
    for (int c; (c = fgetc(f)) != EOF;) s += (char)c;
    fclose(f);
    return s;
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "draws")) {
        const uint64_t w = strtoull(argv[2], nullptr, 10), seed = strtoull(argv[3], nullptr, 10), key = uc::nj_boot_key(seed, (uint32_t)strtoul(argv[4], nullptr, 10));
        for (uint64_t t = 0; t < strtoull(argv[5], nullptr, 10); t++) printf("%u\n", uc::nj_boot_col(key, t, w));
        return 0;
    }
    // seven rows on seventeen columns: buffers of exactly the sizes the calls ask for, so that a step past an end is the sanitizer's to find
    const uint32_t n = 7, n_rep = 5, steps = n - 3;
    const uint64_t w = 17, tri = (uint64_t)n * (n - 1) / 2;
    std::vector<uint8_t> cells;
    std::vector<std::string> nm, rows;
    unsigned s = 4242;
    for (uint32_t i = 0; i < n; i++) {
        std::string r;
        for (uint64_t c = 0; c < w; c++) { s = s * 1103515245u + 12345u; r += "ACDEFGHIKLMNPQRSTVWY-Xac"[(s >> 16) % 24]; }
        if (i) for (uint64_t c = 0; c < w; c++) { s = s * 1103515245u + 12345u; if ((s >> 16) % 3) r[c] = rows[(i - 1) / 2][c]; }      // rows that resemble each other
        rows.push_back(r);
        cells.insert(cells.end(), r.begin(), r.end());
        nm.push_back(i == 2 ? "it's" : "leaf" + std::to_string(i));
    }
    std::vector<const char *> names;
    for (const std::string &x : nm) names.push_back(x.c_str());
    // draws stay inside the alignment, and the counts of a replicate are the counts of its gathered columns
    std::vector<uint32_t> cols(w);
    std::vector<uint32_t> comp(n_rep * tri), diff(n_rep * tri), c1(tri), d1(tri);
    check(uc_nj_boot_counts(n, w, cells.data(), 99, 3, n_rep, 4, comp.data(), diff.data()) == UC_OK, "uc_nj_boot_counts");
    for (uint32_t b = 0; b < n_rep; b++) {
        check(uc_nj_boot_columns(w, 99, 3 + b, cols.data()) == UC_OK, "uc_nj_boot_columns");
        std::vector<uint8_t> g(n * w);
        for (uint32_t i = 0; i < n; i++)
            for (uint64_t t = 0; t < w; t++) { check(cols[t] < w, "a draw outside the alignment"); g[i * w + t] = cells[i * w + cols[t]]; }
        check(uc_nj_counts(n, w, g.data(), 1, c1.data(), d1.data()) == UC_OK, "uc_nj_counts");
        check(!memcmp(c1.data(), comp.data() + b * tri, tri * 4) && !memcmp(d1.data(), diff.data() + b * tri, tri * 4), "replicate counts differ from the gathered alignment's");
    }
    // the batch of joins equals the single calls
    std::vector<double> D((size_t)n_rep * n * n), la(n_rep * steps), lb(n_rep * steps), rl(n_rep * 3), la1(steps), lb1(steps);
    std::vector<uint32_t> ja(n_rep * steps), jb(n_rep * steps), rn(n_rep * 3), ja1(steps), jb1(steps);
    for (uint32_t b = 0; b < n_rep; b++) check(uc_nj_distances(comp.data() + b * tri, diff.data() + b * tri, n, UC_NJ_MODEL_KIMURA, D.data() + (size_t)b * n * n) == UC_OK, "uc_nj_distances");
    check(uc_nj_join_batch(n, n_rep, D.data(), ja.data(), jb.data(), la.data(), lb.data(), rn.data(), rl.data()) == UC_OK, "uc_nj_join_batch");
    uint32_t rn1[3];
    double rl1[3];
    for (uint32_t b = 0; b < n_rep; b++) {
        check(uc_nj_join(n, D.data() + (size_t)b * n * n, ja1.data(), jb1.data(), la1.data(), lb1.data(), rn1, rl1) == UC_OK, "uc_nj_join");
        check(!memcmp(ja1.data(), ja.data() + b * steps, steps * 4) && !memcmp(jb1.data(), jb.data() + b * steps, steps * 4) && !memcmp(la1.data(), la.data() + b * steps, steps * 8) &&
                  !memcmp(lb1.data(), lb.data() + b * steps, steps * 8) && !memcmp(rn1, rn.data() + b * 3, 12) && !memcmp(rl1, rl.data() + b * 3, 24),
              "a replicate of the batch differs from the single call");
    }
    // support: a tree supports itself; the labelled line has a label behind every inner `)` and fits the buffer it asked for
    std::vector<uint32_t> support(steps);
    check(uc_nj_support(n, ja.data(), jb.data(), n_rep, ja.data(), jb.data(), support.data()) == UC_OK, "uc_nj_support");
    for (uint32_t x : support) check(x >= 1 && x <= n_rep, "replicate 0 holds its own splits");
    uint64_t need = 0;
    check(uc_nj_newick_support(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), rn.data(), rl.data(), support.data(), n_rep, nullptr, 0, &need) == UC_OK, "newick (size)");
    std::vector<char> buf(need + 1);
    check(uc_nj_newick_support(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), rn.data(), rl.data(), support.data(), n_rep, buf.data(), buf.size(), &need) == UC_OK, "newick");
    check(uc_nj_newick_support(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), rn.data(), rl.data(), support.data(), n_rep, buf.data(), need, nullptr) == UC_ERR_ARGS,
          "a buffer one byte short is refused");
    const std::string line(buf.data());
    check(line.find("'it''s':") != std::string::npos && line.back() == '\n', line.c_str());
    size_t labelled = 0;
    for (size_t p = 0; p + 1 < line.size(); p++) labelled += line[p] == ')' && line[p + 1] >= '0' && line[p + 1] <= '9';
    check(labelled == steps, "one label per join");
    // sixty-five rows: a split of more than one 64-bit word, complemented where it holds leaf 0
    {
        const uint32_t m = 65, st = m - 3;
        std::vector<uint32_t> a(st), b(st), sup(st);
        for (uint32_t k = 0; k < st; k++) { a[k] = k ? m + k - 1 : 0; b[k] = k + 1; }      // a caterpillar from leaf 0
        check(uc_nj_support(m, a.data(), b.data(), 1, a.data(), b.data(), sup.data()) == UC_OK, "uc_nj_support (65)");
        for (uint32_t x : sup) check(x == 1, "the caterpillar supports itself");
        b[0] = 0; a[0] = 1;                                                                   // the same tree, written the other way round
        std::vector<uint32_t> a0(st), b0(st);
        for (uint32_t k = 0; k < st; k++) { a0[k] = k ? m + k - 1 : 0; b0[k] = k + 1; }
        check(uc_nj_support(m, a0.data(), b0.data(), 1, a.data(), b.data(), sup.data()) == UC_OK && sup[0] == 1 && sup[st - 1] == 1, "child order does not matter");
        a[3] = a[2];                                                                          // a node joined twice
        check(uc_nj_support(m, a0.data(), b0.data(), 1, a.data(), b.data(), sup.data()) == UC_ERR_ARGS, "a replicate that is no tree is refused");
    }
    // the driver under UC_TREE_HOST=1 with the dump, two threads and a budget of one replicate per batch
    setenv("UC_TREE_HOST", "1", 1); setenv("UC_TREE_DUMP", "1", 1); setenv("UC_TREE_BUDGET_BYTES", "64", 1);
    char dir[] = "/tmp/nj_boot_host_check_XXXXXX";
    check(mkdtemp(dir) != nullptr, "mkdtemp");
    const std::string fa = std::string(dir) + "/in.fa", out = std::string(dir) + "/o.nwk";
    {
        FILE *f = fopen(fa.c_str(), "wb");
        check(f != nullptr, "the input file");
        for (uint32_t i = 0; i < n; i++) fprintf(f, ">%s\n%s\n", i == 2 ? "its" : nm[i].c_str(), rows[i].c_str());
        fclose(f);
    }
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o; o.threads = 2; o.device = -1;
    uc_nj_boot_stats st;
    check(uc_tree_infer_boot(fa.c_str(), out.c_str(), "kimura", 9, 99, &o, &st) == UC_OK, "uc_tree_infer_boot");
    check(st.n_rows == n && st.n_columns == w && st.n_replicates == 9 && st.n_batches == 9 && st.support_min <= 9 && st.support_sum <= 9 * steps, "the driver's counts");
    const std::string trees = slurp(out + ".boottrees"), tsv = slurp(out + ".boot.tsv");
    size_t lines = 0;
    for (char c : trees) lines += c == '\n';
    check(lines == 9 && tsv.rfind("0\t", 0) == 0 && slurp(out).back() == '\n' && slurp(out + ".dist.tsv") != "<missing>", "the driver's files");
    check(uc_tree_infer_boot(fa.c_str(), out.c_str(), "kimura", 100001, 99, &o, nullptr) == UC_ERR_ARGS, "100,001 replicates are refused");
    for (const char *ext : {"", ".boottrees", ".boot.tsv", ".dist.tsv"}) remove((out + ext).c_str());
    remove(fa.c_str());
    remove(dir);
    puts("nj_boot_host_check: ok");
    return 0;
}
