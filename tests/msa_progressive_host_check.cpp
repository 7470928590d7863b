// msa_progressive_host_check.cpp — the host twin of rule UC-T/G (uc_msa_progressive_host.cpp) in a program of its own, for the address and
// undefined-behaviour sanitizers: test_msa_progressive.py builds it with -fsanitize=address,undefined together with uc_msa_progressive_host.cpp and
// runs it; nothing is preloaded.  The pieces of the library the twin leans on and that are not under test here (the error text, the device side, the
// neighbour-joining twin) are stand-ins below.  Every array is allocated at exactly the size the call is entitled to, so a read or write past it is
// the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "uc_msa.h"
#include "uc_nj.h"
#include "unicore_cluster.h"

namespace uc {
static std::string g_error;
void set_last_error(const std::string &m) { g_error = m; }
void msa_merge_device(int, const MsaMergeArgs &, const MsaMergePlan &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void msa_progressive_device(int, const MsaProgressiveArgs &, const MsaProgressivePlan &) { fail(UC_ERR_DEVICE, "no device in this program"); }
void nj_join_validate(const NjJoinArgs &) {}
void nj_join_host(const NjJoinArgs &) { fail(UC_ERR_GENERIC, "the join is not part of this program"); }
void nj_join_device(int, const NjJoinArgs &) { fail(UC_ERR_DEVICE, "no device in this program"); }
}  // namespace uc

static void check(bool ok, const char *what) {
    if (!ok) { fprintf(stderr, "msa_progressive_host_check: %s (%s)\n", what, uc::g_error.c_str()); exit(1); }
}

static unsigned g_seed = 2026;
static unsigned rnd(unsigned n) { g_seed = g_seed * 1103515245u + 12345u; return (g_seed >> 16) % n; }
static const char *LET = "ACDEFGHIKLMNPQRSTVWYX";

int main() {
    std::vector<int8_t> SA(441), S3(441);
    for (int k = 0; k < 441; k++) { SA[k] = (int8_t)((int)rnd(21) - 9 + (k % 22 == 0 ? 6 : 0)); S3[k] = (int8_t)((int)rnd(21) - 9 + (k % 22 == 0 ? 6 : 0)); }
    // ---- groups of 1 .. 9 rows (one row without a residue), caterpillar and balanced merge lists, 1 and 3 threads
    for (unsigned shape = 0; shape < 2; shape++) {
        std::vector<uint64_t> grp_off{0}, res_off{0};
        std::vector<uint8_t> res[2];
        std::vector<uint32_t> merges;
        for (unsigned m = 1; m <= 9; m++) {
            for (unsigned r = 0; r < m; r++) {
                const unsigned L = (m == 5 && r == 2) ? 0 : 1 + rnd(130);
                for (unsigned k = 0; k < L; k++) { res[0].push_back((uint8_t)LET[rnd(21)]); res[1].push_back((uint8_t)LET[rnd(21)]); }
                res_off.push_back(res_off.back() + L);
            }
            grp_off.push_back(grp_off.back() + m);
            if (shape == 0) { for (unsigned k = 0; k + 1 < m; k++) { merges.push_back(k ? m + k - 1 : 0); merges.push_back(k + 1); } }
            else {
                std::vector<uint32_t> cur(m), nxt;
                uint32_t id = m;
                for (unsigned k = 0; k < m; k++) cur[k] = k;
                while (cur.size() > 1) {
                    nxt.clear();
                    for (size_t k = 0; k + 1 < cur.size(); k += 2) { merges.push_back(cur[k]); merges.push_back(cur[k + 1]); nxt.push_back(id++); }
                    if (cur.size() & 1) nxt.push_back(cur.back());
                    cur = nxt;
                }
            }
        }
        const uint32_t ng = (uint32_t)grp_off.size() - 1;
        uint64_t cap = 0;
        for (uint32_t g = 0; g < ng; g++) cap += (grp_off[g + 1] - grp_off[g]) * (res_off[grp_off[g + 1]] - res_off[grp_off[g]]);
        std::vector<uint8_t> first[2];
        for (unsigned threads = 1; threads <= 3; threads += 2) {
            std::vector<uint32_t> width(ng);
            std::vector<uint8_t> c0(cap), c1(cap);
            uint64_t need = 0;
            uc_msa_progressive_stats st;
            check(uc_msa_progressive(ng, grp_off.data(), res_off.data(), res[0].data(), res[1].data(), merges.data(), S3.data(), SA.data(), 9, 2, width.data(), c0.data(), c1.data(), cap,
                                     &need, &st, threads) == UC_OK, "uc_msa_progressive");
            check(need <= cap && st.n_merges == grp_off[ng] - ng, "the progressive call's counts");
            uint64_t o = 0;
            for (uint32_t g = 0; g < ng; g++)      // every row without its gaps is the row's residues
                for (uint64_t r = grp_off[g]; r < grp_off[g + 1]; r++, o += width[g]) {
                    std::string a, b;
                    for (uint32_t c = 0; c < width[g]; c++) { if (c0[o + c] != '-') a += (char)c0[o + c]; if (c1[o + c] != '-') b += (char)c1[o + c]; check((c0[o + c] == '-') == (c1[o + c] == '-'), "gaps"); }
                    check(a == std::string(res[0].begin() + res_off[r], res[0].begin() + res_off[r + 1]) && b == std::string(res[1].begin() + res_off[r], res[1].begin() + res_off[r + 1]), "a row's residues");
                }
            c0.resize(need); c1.resize(need);
            if (threads == 1) { first[0] = c0; first[1] = c1; } else check(first[0] == c0 && first[1] == c1, "the thread count changes the answer");
        }
        // exact capacity is enough; one byte less is refused
        std::vector<uint32_t> width(ng);
        std::vector<uint8_t> c0(first[0].size() - 1), c1(first[0].size() - 1);
        check(uc_msa_progressive(ng, grp_off.data(), res_off.data(), res[0].data(), res[1].data(), merges.data(), S3.data(), SA.data(), 9, 2, width.data(), c0.data(), c1.data(),
                                 c0.size(), nullptr, nullptr, 1) == UC_ERR_ARGS, "a capacity one byte short");
    }
    // ---- merges at the widths around the chunk, nodes with gaps, a side of width 0; arrays at the documented bounds
    {
        const unsigned Ws[] = {0, 1, 63, 64, 65, 129};
        std::vector<uint32_t> ma, mb, Wa, Wb;
        std::vector<uint8_t> a[2], b[2];
        auto node = [&](unsigned m, unsigned W, std::vector<uint8_t> out[2]) {
            for (unsigned r = 0; r < m; r++)
                for (unsigned c = 0; c < W; c++) {
                    const bool gap = m > 1 && r != c % m && rnd(3) == 0;
                    out[0].push_back(gap ? (uint8_t)'-' : (uint8_t)LET[rnd(21)]); out[1].push_back(gap ? (uint8_t)'-' : (uint8_t)LET[rnd(21)]);
                }
        };
        uint64_t rcap = 0, ccap = 0;
        for (unsigned x : Ws)
            for (unsigned y : Ws) {
                const unsigned m1 = 1 + rnd(3), m2 = 1 + rnd(3);
                ma.push_back(m1); mb.push_back(m2); Wa.push_back(x); Wb.push_back(y);
                node(m1, x, a); node(m2, y, b);
                rcap += x + y; ccap += (uint64_t)(m1 + m2) * (x + y);
            }
        const uint32_t n = (uint32_t)ma.size();
        std::vector<int32_t> score(n), is(n), js(n), ie(n), je(n);
        std::vector<uint64_t> run_off(n + 1);
        std::vector<uint32_t> runs(rcap), width(n);
        std::vector<uint8_t> c0(ccap), c1(ccap);
        uint64_t need[2];
        for (int open = 0; open <= 11; open += 11)
            check(uc_msa_merge(n, ma.data(), mb.data(), Wa.data(), Wb.data(), a[0].data(), a[1].data(), b[0].data(), b[1].data(), S3.data(), SA.data(), open, 0, score.data(), is.data(),
                               js.data(), ie.data(), je.data(), run_off.data(), runs.data(), rcap, width.data(), c0.data(), c1.data(), ccap, need, 2) == UC_OK, "uc_msa_merge");
        check(need[0] <= rcap && need[1] <= ccap, "the merge call's needs");
    }
    // ---- self scores and the guide of groups that need no join
    {
        const uint64_t res_off[] = {0, 3, 3, 7};
        const uint8_t r0[] = "ACDEFGH", r1[] = "HGFEDCA";
        int64_t self[3];
        check(uc_msa_self_scores(3, res_off, r0, r1, S3.data(), SA.data(), self) == UC_OK && self[1] == 0, "uc_msa_self_scores");
        const uint64_t grp_off[] = {0, 1, 3};
        const int32_t tri[] = {5};
        double D[5];
        uint32_t mg[2];
        check(uc_msa_guide(2, grp_off, tri, self, D, mg) == UC_OK && mg[0] == 0 && mg[1] == 1 && D[2] == 1.0 && D[3] == 1.0, "uc_msa_guide");
    }
    printf("msa_progressive_host_check: ok\n");
    return 0;
}
