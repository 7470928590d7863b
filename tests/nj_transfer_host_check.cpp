// nj_transfer_host_check.cpp — the host side of rule UC-N/T (uc_nj_transfer_host.cpp over uc_nj_boot_host.cpp and uc_nj_host.cpp) in a program of its
// own, for the address and undefined-behaviour sanitizers: test_nj_transfer.py builds it with -fsanitize=address,undefined together with the host
// sources and runs it; nothing is preloaded.  The pieces of the library that the sources lean on and that are not under test here (the error text,
// file reading, the device side) are stand-ins below.  Every buffer has exactly the size the call asks for, so that a step past an end is the
// sanitizer's to find.
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
void nj_transfer_device(int, const NjTransferArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
}  // namespace uc

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "nj_transfer_host_check: %s (%s)\n", what, uc::g_error.c_str()); exit(1); }
}

static std::string slurp(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return "<missing>";
    std::string s;
    for (int c; (c = fgetc(f)) != EOF;) s += (char)c;
    fclose(f);
    return s;
}

// a caterpillar over the leaves in `order`: join s joins node m + s - 1 (order[0] for s = 0) with order[s + 1]
static void caterpillar(uint32_t m, const std::vector<uint32_t> &order, uint32_t *a, uint32_t *b) {
    for (uint32_t k = 0; k + 3 < m; k++) { a[k] = k ? m + k - 1 : order[0]; b[k] = order[k + 1]; }
}

int main() {
    // sixty-five and one hundred and thirty leaves: splits of more than one and more than two 64-bit words, the last with a single bit in use
    for (const uint32_t m : {4u, 5u, 64u, 65u, 130u}) {
        const uint32_t st = m - 3, n_rep = 3;
        std::vector<uint32_t> order(m), a(st), b(st), ra((size_t)n_rep * st), rb((size_t)n_rep * st), phi((size_t)n_rep * st), light(st), sup(st);
        for (uint32_t i = 0; i < m; i++) order[i] = i;
        caterpillar(m, order, a.data(), b.data());
        caterpillar(m, order, ra.data(), rb.data());                                         // replicate 0: the tree itself
        order.erase(order.begin() + 1); order.push_back(1);
        caterpillar(m, order, ra.data() + st, rb.data() + st);                               // replicate 1: leaf 1 moves to the far end
        for (uint32_t i = 0; i < m; i++) order[i] = (i * 7 + 3) % m;                         // replicate 2: another order (7 and m share no factor here)
        caterpillar(m, order, ra.data() + 2 * st, rb.data() + 2 * st);
        check(uc_nj_transfer(m, a.data(), b.data(), n_rep, ra.data(), rb.data(), 2, phi.data(), light.data()) == UC_OK, "uc_nj_transfer");
        check(uc_nj_support(m, a.data(), b.data(), n_rep, ra.data(), rb.data(), sup.data()) == UC_OK, "uc_nj_support");
        for (uint32_t s = 0; s < st; s++) {
            const uint32_t below = s + 2;
            check(light[s] == std::min(below, m - below) && light[s] >= 2, "the light side of a caterpillar's join");
            uint32_t zeros = 0;
            for (uint32_t r = 0; r < n_rep; r++) { check(phi[(size_t)r * st + s] <= light[s] - 1, "phi above its cap"); zeros += phi[(size_t)r * st + s] == 0; }
            check(phi[s] == 0 && phi[st + s] <= 1 && zeros == sup[s], "a tree holds its own splits; one moved leaf costs one; zeros are the support");
        }
        // the labelled line: a label behind every inner `)`, and a buffer of exactly the size asked for
        std::vector<uint64_t> phi_sum(st, 0);
        for (uint32_t r = 0; r < n_rep; r++) for (uint32_t s = 0; s < st; s++) phi_sum[s] += phi[(size_t)r * st + s];
        std::vector<std::string> nm;
        std::vector<const char *> names;
        for (uint32_t i = 0; i < m; i++) nm.push_back(i == 2 ? "it's" : "leaf" + std::to_string(i));
        for (const std::string &x : nm) names.push_back(x.c_str());
        std::vector<double> la(st, 0.5), lb(st, 0.25);
        const uint32_t root[3] = {m + st - 1, m - 2, m - 1};
        const double rlen[3] = {1.0, 2.0, 3.0};
        uint64_t need = 0;
        check(uc_nj_newick_transfer(names.data(), m, a.data(), b.data(), la.data(), lb.data(), root, rlen, light.data(), phi_sum.data(), n_rep, nullptr, 0, &need) == UC_OK, "newick (size)");
        std::vector<char> buf(need + 1);
        check(uc_nj_newick_transfer(names.data(), m, a.data(), b.data(), la.data(), lb.data(), root, rlen, light.data(), phi_sum.data(), n_rep, buf.data(), buf.size(), &need) == UC_OK, "newick");
        check(uc_nj_newick_transfer(names.data(), m, a.data(), b.data(), la.data(), lb.data(), root, rlen, light.data(), phi_sum.data(), n_rep, buf.data(), need, nullptr) == UC_ERR_ARGS,
              "a buffer one byte short is refused");
        const std::string line(buf.data());
        size_t labelled = 0;
        for (size_t p = 0; p + 1 < line.size(); p++) labelled += line[p] == ')' && line[p + 1] >= '0' && line[p + 1] <= '9';
        check(labelled == st && line.back() == '\n', "one label per join");
        phi_sum[st - 1] = (uint64_t)n_rep * (light[st - 1] - 1) + 1;
        check(uc_nj_newick_transfer(names.data(), m, a.data(), b.data(), la.data(), lb.data(), root, rlen, light.data(), phi_sum.data(), n_rep, nullptr, 0, &need) == UC_ERR_ARGS,
              "a transfer sum above its denominator is refused");
        if (st > 3) {
            ra[2 * st + 3] = ra[2 * st + 2];                                                 // the last replicate joins a node twice
            check(uc_nj_transfer(m, a.data(), b.data(), n_rep, ra.data(), rb.data(), 2, phi.data(), light.data()) == UC_ERR_ARGS, "a replicate that is no tree is refused");
        }
    }
    uint32_t tile = 0, chunk = 0, host_leaves = 0;
    check(uc_nj_transfer_geometry(&tile, &chunk, &host_leaves) == UC_OK && tile && chunk && host_leaves && uc_nj_transfer_geometry(nullptr, nullptr, nullptr) == UC_OK, "uc_nj_transfer_geometry");
    // the driver in mode tbe under UC_TREE_HOST=1 with the dump, two threads and a budget of one replicate per batch
    const uint32_t n = 7;
    const uint64_t w = 17;
    std::vector<std::string> rows;
    unsigned s = 4242;
    for (uint32_t i = 0; i < n; i++) {
        std::string r;
        for (uint64_t c = 0; c < w; c++) { s = s * 1103515245u + 12345u; r += "ACDEFGHIKLMNPQRSTVWY-Xac"[(s >> 16) % 24]; }
        if (i) for (uint64_t c = 0; c < w; c++) { s = s * 1103515245u + 12345u; if ((s >> 16) % 3) r[c] = rows[(i - 1) / 2][c]; }      // rows that resemble each other
        rows.push_back(r);
    }
    setenv("UC_TREE_HOST", "1", 1); setenv("UC_TREE_DUMP", "1", 1); setenv("UC_TREE_BUDGET_BYTES", "64", 1);
    char dir[] = "/tmp/nj_transfer_host_check_XXXXXX";
    check(mkdtemp(dir) != nullptr, "mkdtemp");
    const std::string fa = std::string(dir) + "/in.fa", out = std::string(dir) + "/o.nwk", old = std::string(dir) + "/old.nwk";
    {
        FILE *f = fopen(fa.c_str(), "wb");
        check(f != nullptr, "the input file");
        for (uint32_t i = 0; i < n; i++) fprintf(f, ">leaf%u\n%s\n", i, rows[i].c_str());
        fclose(f);
    }
    uc_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o; o.threads = 2; o.device = -1;
    uc_nj_boot_stats st, st_old;
    check(uc_tree_infer_support(fa.c_str(), out.c_str(), "kimura", 9, 99, UC_NJ_SUPPORT_TBE, &o, &st) == UC_OK, "uc_tree_infer_support (tbe)");
    check(uc_tree_infer_boot(fa.c_str(), old.c_str(), "kimura", 9, 99, &o, &st_old) == UC_OK, "uc_tree_infer_boot");
    check(st.n_rows == n && st.n_replicates == 9 && st.n_batches == 9 && st.support_min == st_old.support_min && st.support_sum == st_old.support_sum, "support_min / support_sum keep their meaning");
    const std::string tsv = slurp(out + ".boot.tsv");
    size_t tabs = 0, lines = 0;
    for (char c : tsv) { tabs += c == '\t'; lines += c == '\n'; }
    check(lines == n - 3 && tabs == 4 * lines && slurp(out + ".boottrees") == slurp(old + ".boottrees") && slurp(out).back() == '\n', "the driver's files");
    check(uc_tree_infer_support(fa.c_str(), out.c_str(), "kimura", 9, 99, UC_NJ_SUPPORT_FBP, &o, nullptr) == UC_OK && slurp(out) == slurp(old) && slurp(out + ".boot.tsv") == slurp(old + ".boot.tsv"),
          "mode fbp is the old call");
    check(uc_tree_infer_support(fa.c_str(), out.c_str(), "kimura", 9, 99, 2, &o, nullptr) == UC_ERR_ARGS, "an unknown mode is refused");
    check(uc_tree_infer_support(fa.c_str(), out.c_str(), "kimura", 100001, 99, UC_NJ_SUPPORT_TBE, &o, nullptr) == UC_ERR_ARGS, "100,001 replicates are refused");
    for (const std::string &base : {out, old})
        for (const char *ext : {"", ".boottrees", ".boot.tsv", ".dist.tsv"}) remove((base + ext).c_str());
    remove(fa.c_str());
    remove(dir);
    puts("nj_transfer_host_check: ok");
    return 0;
}
