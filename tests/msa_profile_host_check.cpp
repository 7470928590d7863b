// msa_profile_host_check.cpp — the host twin of rule UC-T/P (uc_msa_profile_host.cpp) in a program of its own, for the address and
// undefined-behaviour sanitizers: test_msa_profile.py builds it with -fsanitize=address,undefined together with uc_msa_profile_host.cpp and runs
// it; nothing is preloaded.  The pieces of the library the twin leans on and that are not under test here (the error text, the device side) are
// stand-ins below.  Every array is allocated at exactly the size the call is entitled to, so a read or write past it is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "uc_msa.h"

namespace uc {
static std::string g_error;
void set_last_error(const std::string &m) { g_error = m; }
void msa_profile_align_device(int, const MsaProfileAlignArgs &, const MsaProfilePlan &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void msa_profile_layout_device(int, const MsaProfileLayoutArgs &, const MsaProfileLayoutPlan &) { fail(UC_ERR_DEVICE, "no device in this program"); }
}  // namespace uc

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "msa_profile_host_check: %s (%s)\n", what, uc::g_error.c_str()); exit(1); }
}

struct Msa {
    std::vector<uint64_t> grp_off{0}, res_off{0};
    std::vector<uint32_t> width;
    std::vector<uint8_t> cells[2], res[2];
};

static unsigned g_seed = 2024;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1103515245u + 12345u; return (g_seed >> 16) % n; }

// m rows from one ancestor of W columns: substitutions, deleted columns (gaps), inserted residues (in the row only); every `lost`-th row is all gaps
static void add_group(Msa &M, unsigned m, unsigned W, unsigned lost) {
    static const char *LET = "ACDEFGHIKLMNPQRSTVWYX";
    std::string anc[2];
    for (unsigned c = 0; c < W; c++) { anc[0] += LET[rnd(20)]; anc[1] += LET[rnd(20)]; }
    for (unsigned i = 0; i < m; i++) {
        std::string c[2] = {std::string(W, '-'), std::string(W, '-')}, r[2];
        for (unsigned k = 0; k < W; k++) {
            if (rnd(20) == 0) continue;
            for (int t = 0; t < 2; t++) { const char x = rnd(5) == 0 ? LET[rnd(21)] : anc[t][k]; c[t][k] = x; r[t] += x; }
            if (rnd(25) == 0) for (unsigned n = 1 + rnd(3); n; n--) for (int t = 0; t < 2; t++) r[t] += LET[rnd(20)];
        }
        if (lost && i % lost == lost - 1) c[0] = c[1] = std::string(W, '-');
        for (int t = 0; t < 2; t++) { M.cells[t].insert(M.cells[t].end(), c[t].begin(), c[t].end()); M.res[t].insert(M.res[t].end(), r[t].begin(), r[t].end()); }
        M.res_off.push_back(M.res_off.back() + r[0].size());
    }
    M.grp_off.push_back(M.grp_off.back() + m);
    M.width.push_back(W);
}

// one round through the two entry points; returns the new MSA's cell bytes
static uint64_t round_of(Msa &M, const int8_t *S3, const int8_t *SA, int open, int ext) {
    const uint32_t ng = (uint32_t)M.width.size();
    const uint64_t n_rows = M.grp_off[ng];
    std::vector<uint8_t> al(n_rows);
    std::vector<int32_t> sc(n_rows), qs(n_rows), ts(n_rows), qe(n_rows), te(n_rows);
    std::vector<uint64_t> uo(n_rows + 1);
    uint64_t need = 0;
    uint32_t none = 0;
    // first with no room at all: the call reports what it needs
    int rc = uc_msa_profile_align(ng, M.grp_off.data(), M.width.data(), M.cells[0].data(), M.cells[1].data(), M.res_off.data(), M.res[0].data(), M.res[1].data(), S3, SA, open, ext,
                                  al.data(), sc.data(), qs.data(), ts.data(), qe.data(), te.data(), uo.data(), &none, 0, &need, 1);
    check(rc == (need ? UC_ERR_ARGS : UC_OK), "the run count comes back from a call without room");
    std::vector<uint32_t> runs(need);      // exactly that
    rc = uc_msa_profile_align(ng, M.grp_off.data(), M.width.data(), M.cells[0].data(), M.cells[1].data(), M.res_off.data(), M.res[0].data(), M.res[1].data(), S3, SA, open, ext,
                              al.data(), sc.data(), qs.data(), ts.data(), qe.data(), te.data(), uo.data(), runs.data(), need, &need, 3);
    check(rc == UC_OK && uo[n_rows] == need, "uc_msa_profile_align");
    std::vector<uint32_t> nw(ng);
    uint64_t bytes = 0;
    uint8_t dummy = 0;
    rc = uc_msa_profile_layout(ng, M.grp_off.data(), M.width.data(), M.cells[0].data(), M.cells[1].data(), M.res_off.data(), M.res[0].data(), M.res[1].data(), al.data(), qs.data(),
                               ts.data(), uo.data(), runs.data(), nw.data(), &dummy, &dummy, 0, &bytes);
    check(rc == (bytes ? UC_ERR_ARGS : UC_OK), "the cell bytes come back from a call without room");
    std::vector<uint8_t> c0(bytes), c1(bytes);
    rc = uc_msa_profile_layout(ng, M.grp_off.data(), M.width.data(), M.cells[0].data(), M.cells[1].data(), M.res_off.data(), M.res[0].data(), M.res[1].data(), al.data(), qs.data(),
                               ts.data(), uo.data(), runs.data(), nw.data(), c0.data(), c1.data(), bytes, &bytes);
    check(rc == UC_OK, "uc_msa_profile_layout");
    uint64_t sum = 0;
    for (uint32_t g = 0; g < ng; g++) sum += (M.grp_off[g + 1] - M.grp_off[g]) * nw[g];
    check(sum == bytes, "the widths add up to the cell bytes");
    for (uint64_t k = 0; k < bytes; k++) check((c0[k] == '-') == (c1[k] == '-'), "both tracks hold their gaps in the same cells");
    M.width = nw; M.cells[0] = c0; M.cells[1] = c1;
    return bytes;
}

int main() {
    int8_t S3[441], SA[441];
    for (int a = 0; a < 21; a++)
        for (int b = 0; b < 21; b++) {      // asymmetric, entries from -48 to 48
            S3[a * 21 + b] = (int8_t)(a == b ? 6 + a % 5 : (a * 7 + b * 3) % 9 - 6);
            SA[a * 21 + b] = (int8_t)(a == b ? 5 : (a * 5 + b * 11) % 7 - 5);
        }
    S3[1] = 48; S3[21] = -48; SA[2 * 21 + 3] = -48; SA[3 * 21 + 2] = 48;
    Msa M;
    add_group(M, 2, 1, 0); add_group(M, 3, 63, 0); add_group(M, 1, 17, 0); add_group(M, 8, 65, 4); add_group(M, 5, 130, 5); add_group(M, 2, 64, 2);
    for (int r = 0; r < 3; r++) check(round_of(M, S3, SA, 10, 1) > 0, "a round leaves cells");
    Msa N;
    add_group(N, 4, 40, 0);
    check(round_of(N, S3, SA, 3, 3) > 0, "gap open = gap extension");
    // the refusals leave through the error path
    uint8_t al[4];
    int32_t v[4];
    uint64_t uo[5];
    check(uc_msa_profile_align(1, N.grp_off.data(), N.width.data(), N.cells[0].data(), N.cells[1].data(), N.res_off.data(), N.res[0].data(), N.res[1].data(), S3, SA, 1, 2, al, v, v,
                               v, v, v, uo, nullptr, 0, nullptr, 2) == UC_ERR_ARGS, "gap open below gap extension is refused");
    N.cells[1][5] = N.cells[1][5] == '-' ? 'A' : '-';
    check(uc_msa_profile_align(1, N.grp_off.data(), N.width.data(), N.cells[0].data(), N.cells[1].data(), N.res_off.data(), N.res[0].data(), N.res[1].data(), S3, SA, 10, 1, al, v,
                               v, v, v, v, uo, nullptr, 0, nullptr, 2) == UC_ERR_ARGS, "tracks that disagree on a gap are refused");
    N.cells[1][5] = '#'; N.cells[0][5] = '#';
    check(uc_msa_profile_align(1, N.grp_off.data(), N.width.data(), N.cells[0].data(), N.cells[1].data(), N.res_off.data(), N.res[0].data(), N.res[1].data(), S3, SA, 10, 1, al, v,
                               v, v, v, v, uo, nullptr, 0, nullptr, 2) == UC_ERR_ARGS, "a cell that is no letter is refused");
    puts("msa_profile_host_check: ok");
    return 0;
}
