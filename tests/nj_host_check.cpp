// nj_host_check.cpp — the host twins of rule UC-N (uc_nj_host.cpp) in a program of its own, for the address and undefined-behaviour sanitizers:
// test_nj.py builds it with -fsanitize=address,undefined together with uc_nj_host.cpp and runs it; nothing is preloaded.  The pieces of the library
// that uc_nj_host.cpp leans on and that are not under test here (the error text, file reading, the device side) are stand-ins below.
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
std::string read_whole_file(const std::string &path) { fail(UC_ERR_IO, "cannot read %s", path.c_str()); }
void nj_counts_device(int, const NjCountArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void nj_join_device(int, const NjJoinArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
}  // namespace uc

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "nj_host_check: %s (%s)\n", what, uc::g_error.c_str()); exit(1); }
}

static std::string tree_of(const std::vector<std::string> &rows, const std::vector<const char *> &names, uint32_t threads, std::vector<uint32_t> *comp_out) {
    const uint32_t n = (uint32_t)rows.size();
    const uint64_t w = rows[0].size(), tri = (uint64_t)n * (n - 1) / 2;
    std::vector<uint8_t> cells;      // exactly n x w bytes: a read past the last row is the sanitizer's to find
    for (const std::string &r : rows) cells.insert(cells.end(), r.begin(), r.end());
    std::vector<uint32_t> comp(tri), diff(tri);
    check(uc_nj_counts(n, w, cells.data(), threads, comp.data(), diff.data()) == UC_OK, "uc_nj_counts");
    std::vector<double> D((size_t)n * n);
    check(uc_nj_distances(comp.data(), diff.data(), n, UC_NJ_MODEL_KIMURA, D.data()) == UC_OK, "uc_nj_distances");
    const uint32_t steps = n > 3 ? n - 3 : 0;
    std::vector<uint32_t> ja(steps), jb(steps);
    std::vector<double> la(steps), lb(steps);
    uint32_t root[3];
    double rlen[3];
    check(uc_nj_join(n, D.data(), steps ? ja.data() : nullptr, steps ? jb.data() : nullptr, steps ? la.data() : nullptr, steps ? lb.data() : nullptr, root, rlen) == UC_OK, "uc_nj_join");
    uint64_t need = 0;
    check(uc_nj_newick(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), root, rlen, nullptr, 0, &need) == UC_OK, "uc_nj_newick (size)");
    std::vector<char> buf(need + 1);      // exactly what the call asked for
    check(uc_nj_newick(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), root, rlen, buf.data(), buf.size(), &need) == UC_OK, "uc_nj_newick");
    check(uc_nj_newick(names.data(), n, ja.data(), jb.data(), la.data(), lb.data(), root, rlen, buf.data(), need, nullptr) == UC_ERR_ARGS, "a buffer one byte short is refused");
    if (comp_out) *comp_out = comp;
    return std::string(buf.data());
}

int main() {
    // two leaves: p = 1/4, d = -log(1 - 0.25 - 0.0125) = 0.304489..., both leaves at half of it
    std::string t = tree_of({"ACDE", "ACDF"}, {"a", "b c"}, 1, nullptr);
    check(t == "(a:0.152245,'b c':0.152245);\n", t.c_str());
    // three leaves, nine columns (one more than a 64-bit word of the twin's inner loop), a row without any informative cell
    std::vector<uint32_t> comp;
    t = tree_of({"ACDEFGHIK", "---------", "ACDEFGHIL"}, {"x", "it's", "z"}, 2, &comp);
    check(comp == std::vector<uint32_t>({0, 9, 0}), "comp of the all-gap row");
    check(t.find("'it''s':") != std::string::npos && t.back() == '\n', t.c_str());
    // seven leaves on seventeen columns, four threads: every step of the join loop and the trifurcation
    std::vector<std::string> rows;
    std::vector<std::string> nm;
    unsigned s = 12345;
    for (int i = 0; i < 7; i++) {
        std::string r;
        for (int c = 0; c < 17; c++) { s = s * 1103515245u + 12345u; r += "ACDEFGHIKLMNPQRSTVWY-X"[(s >> 16) % 22]; }
        rows.push_back(r);
        nm.push_back("leaf" + std::to_string(i));
    }
    std::vector<const char *> names;
    for (const std::string &x : nm) names.push_back(x.c_str());
    t = tree_of(rows, names, 4, nullptr);
    for (const std::string &x : nm) check(t.find(x + ":") != std::string::npos, "every leaf is in the tree");
    // the refusals leave through the error path
    uint32_t c1, d1;
    check(uc_nj_counts(1, 4, (const uint8_t *)"ACDE", 1, &c1, &d1) == UC_ERR_ARGS, "one row is refused");
    check(uc_nj_counts(2, 0, (const uint8_t *)"", 1, &c1, &d1) == UC_ERR_ARGS, "no column is refused");
    puts("nj_host_check: ok");
    return 0;
}
