// uc_msa_progressive_host.cpp — rule UC-T/G, the progressive MSA of `unicore tree -a progressive`: the checks host and device share, the
// host twins of the kernels of uc_msa_progressive.hip and the C entry points.  Builds without HIP (the _dev entry points call the device side).
//   guide     D(i, j) = 1 - S(i, j) / min(self(i), self(j)) (1 where the minimum is <= 0, clamped at 0), rule UC-N/J over D, the merge list from the joins
//   merge     cnt[column][letter] per side and track; s(i, j) = floor(sum_t sum_x sum_y cntA_t[i][x] cntB_t[j][y] S_t[x][y] / (ma mb)); the overlap DP
//             H / E / F without a floor; the end cell on the last row or column by (largest H, smallest j, smallest i); one walk with E6's preferences;
//             the merged node: leading overhang, the path, trailing overhang
//   MSA       the merges of a group level by level; the root's rows back in file order
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "uc_files.h"
#include "uc_msa.h"
#include "uc_nj.h"

namespace uc {

namespace {

constexpr uint32_t A = MSA_PROFILE_A;

void pg_need(const void *p, const char *what) { if (!p) fail(UC_ERR_ARGS, "progressive MSA: %s must not be NULL", what); }

uint64_t check_groups(uint32_t n_groups, const uint64_t *grp_off) {
    if (!n_groups) return 0;
    pg_need(grp_off, "grp_off");
    if (grp_off[0] != 0) fail(UC_ERR_ARGS, "progressive MSA: grp_off[0] must be 0");
    for (uint32_t g = 0; g < n_groups; g++) {
        if (grp_off[g + 1] <= grp_off[g]) fail(UC_ERR_ARGS, "progressive MSA: group %u is empty or grp_off decreases", g);
        if (grp_off[g + 1] - grp_off[g] > MSA_PROG_MAX_ROWS) fail(UC_ERR_ARGS, "progressive MSA: group %u has more than %u rows", g, MSA_PROG_MAX_ROWS);
    }
    return grp_off[n_groups];
}

void check_gaps(int32_t open, int32_t ext) {
    if (ext < 0 || open < ext) fail(UC_ERR_ARGS, "progressive MSA: gap open %d below gap extension %d, or a negative extension", open, ext);
}

void check_matrix(const int8_t *S, const char *what) {
    pg_need(S, what);
    for (uint32_t k = 0; k < A * A; k++) if (S[k] < -48 || S[k] > 48) fail(UC_ERR_ARGS, "progressive MSA: %s holds %d, outside -48 .. 48", what, (int)S[k]);
}

// over up to `threads` host threads, an item to the thread that draws its ticket
template <class F>
void over(uint32_t threads, uint64_t count, F &&fn) {
    const uint32_t nt = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(threads, 1), std::max<uint64_t>(count, 1));
    std::atomic<uint64_t> ticket{0};
    std::vector<std::string> err(nt);
    std::vector<int> code(nt, 0);
    auto work = [&](uint32_t t) {
        try { for (uint64_t k = ticket++; k < count; k = ticket++) fn(k); }
        catch (const Error &e) { code[t] = e.code; err[t] = e.what(); }
        catch (const std::exception &e) { code[t] = UC_ERR_GENERIC; err[t] = e.what(); }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &t : pool) t.join();
    for (uint32_t t = 0; t < nt; t++) if (code[t]) fail(code[t], "%s", err[t].c_str());
}

struct MergeOut {
    int32_t score = 0, is = 0, js = 0, ie = 0, je = 0;
    uint32_t width = 0;
    std::vector<uint32_t> runs;
    std::vector<uint8_t> cells[2];      // (ma + mb) x width
};

// cnt[(track * W + column) * 21 + letter]
void counts(uint32_t m, uint64_t W, const uint8_t *const cells[2], std::vector<int32_t> &cnt) {
    cnt.assign(2 * W * A, 0);
    for (uint32_t tr = 0; tr < 2; tr++)
        for (uint64_t i = 0; i < m; i++)
            for (uint64_t c = 0; c < W; c++) {
                const uint8_t ch = cells[tr][i * W + c];
                if (ch != (uint8_t)'-') cnt[(tr * W + c) * A + msa_letter_code(ch)]++;
            }
}

void merge_one(uint32_t ma, uint32_t mb, uint64_t Wa, uint64_t Wb, const uint8_t *const a[2], const uint8_t *const b[2], const int8_t *const S[2], int32_t open, int32_t ext,
               MergeOut &o) {
    o = MergeOut();
    if (Wa && Wb) {
        std::vector<int32_t> cA, cB, Q(Wb * 2 * A);
        counts(ma, Wa, a, cA); counts(mb, Wb, b, cB);
        for (uint32_t tr = 0; tr < 2; tr++)      // Q[j][track][x] = sum_y cntB[j][y] S[x][y]
            for (uint64_t j = 0; j < Wb; j++)
                for (uint32_t x = 0; x < A; x++) {
                    int32_t acc = 0;
                    for (uint32_t y = 0; y < A; y++) acc += cB[(tr * Wb + j) * A + y] * (int32_t)S[tr][x * A + y];
                    Q[(j * 2 + tr) * A + x] = acc;
                }
        const int32_t div = (int32_t)(ma * mb);
        std::vector<int32_t> H(Wb + 1, 0), F(Wb + 1, MSA_PROG_NEG);
        std::vector<uint8_t> dec(Wa * Wb);
        int32_t best = 0;
        uint64_t bi = Wa, bj = 0;      // the corner (Wa, 0); (0, Wb) ties with it and loses by its j
        for (uint64_t i = 1; i <= Wa; i++) {
            int32_t hleft = 0, e = MSA_PROG_NEG, hdiag = 0;
            const int32_t *ca0 = cA.data() + (i - 1) * A, *ca1 = cA.data() + (Wa + i - 1) * A;
            for (uint64_t j = 1; j <= Wb; j++) {
                const int32_t *q = Q.data() + (j - 1) * 2 * A;
                int32_t raw = 0;
                for (uint32_t x = 0; x < A; x++) raw += ca0[x] * q[x] + ca1[x] * q[A + x];
                const int32_t s = msa_floor_div(raw, div);
                const int32_t upH = H[j], upF = F[j];
                const int32_t fn = std::max(upF - ext, upH - open), en = std::max(e - ext, hleft - open), d = hdiag + s;
                const int32_t h = std::max(d, std::max(en, fn));
                dec[(i - 1) * Wb + (j - 1)] = (uint8_t)((h == d ? 1 : h == fn ? 2 : 3) | (fn == upH - open ? 4 : 0) | (en == hleft - open ? 8 : 0));
                hdiag = upH; H[j] = h; F[j] = fn; hleft = h; e = en;
                if ((i == Wa || j == Wb) && (h > best || (h == best && (j < bj || (j == bj && i < bi))))) { best = h; bi = i; bj = j; }
            }
        }
        o.score = best; o.ie = (int32_t)bi; o.je = (int32_t)bj;
        uint64_t i = bi, j = bj;
        uint32_t state = 0, op = 3, len = 0;
        std::vector<uint32_t> rev;
        auto emit = [&](uint32_t x) { if (x == op) { len++; return; } if (len) rev.push_back(len << 2 | op); op = x; len = 1; };
        while (i > 0 && j > 0) {
            const uint8_t d = dec[(i - 1) * Wb + (j - 1)];
            if (state == 0) {
                const uint32_t k = d & 3u;
                if (k == 1) { emit(0); i--; j--; } else state = k == 2 ? 1 : 2;
            } else if (state == 1) { emit(1); if (d & 4u) state = 0; i--; }
            else { emit(2); if (d & 8u) state = 0; j--; }
        }
        if (len) rev.push_back(len << 2 | op);
        o.is = (int32_t)i; o.js = (int32_t)j;
        o.runs.assign(rev.rbegin(), rev.rend());
    }
    uint64_t path = 0;
    for (uint32_t w : o.runs) path += w >> 2;
    const uint64_t W = (uint64_t)o.is + o.js + path + (Wa - o.ie) + (Wb - o.je);
    o.width = (uint32_t)W;
    for (uint32_t tr = 0; tr < 2; tr++) {
        o.cells[tr].assign((uint64_t)(ma + mb) * W, (uint8_t)'-');
        uint8_t *out = o.cells[tr].data();
        // a's column x / b's column y into merged column c
        auto col_a = [&](uint64_t c, uint64_t x) { for (uint32_t r = 0; r < ma; r++) out[r * W + c] = a[tr][r * Wa + x]; };
        auto col_b = [&](uint64_t c, uint64_t y) { for (uint32_t r = 0; r < mb; r++) out[(ma + r) * W + c] = b[tr][r * Wb + y]; };
        uint64_t c = 0, x = 0, y = 0;
        for (; x < (uint64_t)o.is; x++) col_a(c++, x);
        for (; y < (uint64_t)o.js; y++) col_b(c++, y);
        for (uint32_t w : o.runs)
            for (uint32_t l = 0; l < w >> 2; l++) {
                const uint32_t k = w & 3u;
                if (k != 2u) col_a(c, x++);
                if (k != 1u) col_b(c, y++);
                c++;
            }
        for (; x < Wa; x++) col_a(c++, x);
        for (; y < Wb; y++) col_b(c++, y);
    }
}

}  // namespace

void msa_merge_check_widths(uint64_t Wa, uint64_t Wb, int32_t gap_open, const char *what, uint64_t k) {
    if (Wa * Wb >> 31) fail(UC_ERR_ARGS, "progressive MSA: %s %llu needs %llu x %llu cells, 2^31 or more", what, (unsigned long long)k, (unsigned long long)Wa, (unsigned long long)Wb);
    if ((Wa + Wb) * (uint64_t)std::max(gap_open, 96) >> 27)
        fail(UC_ERR_ARGS, "progressive MSA: %s %llu: (%llu + %llu) columns x max(gap open %d, 96) reach 2^27", what, (unsigned long long)k, (unsigned long long)Wa,
             (unsigned long long)Wb, gap_open);
    // the score and decision bytes of a task are laid out by chunk of a's columns and anti-diagonal
    if ((Wa + MSA_PROG_CHUNK - 1) / MSA_PROG_CHUNK * (Wb + MSA_PROG_CHUNK - 1) * MSA_PROG_CHUNK >> 31)
        fail(UC_ERR_ARGS, "progressive MSA: %s %llu of %llu x %llu columns needs 2^31 or more decision bytes", what, (unsigned long long)k, (unsigned long long)Wa, (unsigned long long)Wb);
}

void msa_self_scores(uint64_t n_rows, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *SA, const int8_t *S3, int64_t *self) {
    if (!n_rows) return;
    pg_need(res_off, "res_off"); pg_need(self, "self"); check_matrix(SA, "the amino-acid matrix"); check_matrix(S3, "the 3Di matrix");
    if (res_off[0] != 0) fail(UC_ERR_ARGS, "progressive MSA: res_off[0] must be 0");
    for (uint64_t r = 0; r < n_rows; r++) if (res_off[r + 1] < res_off[r]) fail(UC_ERR_ARGS, "progressive MSA: row %llu has a malformed residue range", (unsigned long long)r);
    if (res_off[n_rows]) { pg_need(res0, "the residues of track 0"); pg_need(res1, "the residues of track 1"); }
    for (uint64_t r = 0; r < n_rows; r++) {
        int64_t s = 0;
        for (uint64_t k = res_off[r]; k < res_off[r + 1]; k++) { const uint32_t x = msa_letter_code(res0[k]), y = msa_letter_code(res1[k]); s += SA[x * A + x] + S3[y * A + y]; }
        self[r] = s;
    }
}

void msa_guide_validate(const MsaGuideArgs &a, std::vector<uint64_t> &tri_off) {
    const uint64_t n_rows = check_groups(a.n_groups, a.grp_off);
    tri_off.assign((size_t)a.n_groups + 1, 0);
    for (uint32_t g = 0; g < a.n_groups; g++) { const uint64_t m = a.grp_off[g + 1] - a.grp_off[g]; tri_off[g + 1] = tri_off[g] + m * (m - 1) / 2; }
    if (!a.n_groups) return;
    pg_need(a.self, "self"); pg_need(a.D, "D");
    if (tri_off[a.n_groups]) pg_need(a.scores, "scores");
    if (n_rows > a.n_groups) pg_need(a.merges, "merges");
}

void msa_guide_run(const MsaGuideArgs &a, const std::vector<uint64_t> &tri_off, bool on_device, int device) {
    uint64_t d_off = 0;
    std::vector<uint32_t> ja, jb;
    std::vector<double> la, lb;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b;
        double *D = a.D + d_off;
        d_off += m * m;
        const int32_t *t = a.scores + tri_off[g];
        uint64_t k = 0;
        for (uint64_t i = 0; i < m; i++) {
            D[i * m + i] = 0.0;
            for (uint64_t j = i + 1; j < m; j++, k++) {
                const int64_t den = std::min(a.self[b + i], a.self[b + j]);
                double d = 1.0;
                if (den > 0) { d = 1.0 - (double)t[k] / (double)den; if (d < 0.0) d = 0.0; }
                D[i * m + j] = D[j * m + i] = d;
            }
        }
        uint32_t *mg = a.merges + 2 * (b - g);
        if (m == 1) continue;
        if (m == 2) { mg[0] = 0; mg[1] = 1; continue; }
        const uint64_t steps = m - 3;
        ja.assign(std::max<uint64_t>(steps, 1), 0); jb.assign(std::max<uint64_t>(steps, 1), 0); la.assign(std::max<uint64_t>(steps, 1), 0); lb.assign(std::max<uint64_t>(steps, 1), 0);
        uint32_t root[3];
        double root_len[3];
        const NjJoinArgs ja_{(uint32_t)m, D, ja.data(), jb.data(), la.data(), lb.data(), root, root_len};
        nj_join_validate(ja_);
        if (on_device && m >= MSA_GUIDE_DEV_ROWS) nj_join_device(device, ja_); else nj_join_host(ja_);
        for (uint64_t s = 0; s < steps; s++) { mg[2 * s] = ja[s]; mg[2 * s + 1] = jb[s]; }
        mg[2 * steps] = root[0]; mg[2 * steps + 1] = root[1];
        mg[2 * steps + 2] = (uint32_t)(m + steps); mg[2 * steps + 3] = root[2];
    }
}

void msa_merge_validate(const MsaMergeArgs &a, MsaMergePlan &plan) {
    check_gaps(a.gap_open, a.gap_ext);
    plan.a_off.assign((size_t)a.n_tasks + 1, 0); plan.b_off.assign((size_t)a.n_tasks + 1, 0);
    plan.n_cells = 0;
    if (!a.n_tasks) return;
    pg_need(a.ma, "ma"); pg_need(a.mb, "mb"); pg_need(a.Wa, "Wa"); pg_need(a.Wb, "Wb");
    check_matrix(a.S[0], "the amino-acid matrix"); check_matrix(a.S[1], "the 3Di matrix");
    pg_need(a.score, "score"); pg_need(a.is, "is"); pg_need(a.js, "js"); pg_need(a.ie, "ie"); pg_need(a.je, "je"); pg_need(a.run_off, "run_off"); pg_need(a.width, "width");
    for (uint32_t k = 0; k < a.n_tasks; k++) {
        if (!a.ma[k] || !a.mb[k] || (uint64_t)a.ma[k] + a.mb[k] > MSA_PROG_MAX_ROWS)
            fail(UC_ERR_ARGS, "progressive MSA: task %u joins %u and %u rows (1 at least each, %u at most together)", k, a.ma[k], a.mb[k], MSA_PROG_MAX_ROWS);
        msa_merge_check_widths(a.Wa[k], a.Wb[k], a.gap_open, "task", k);
        plan.a_off[k + 1] = plan.a_off[k] + (uint64_t)a.ma[k] * a.Wa[k];
        plan.b_off[k + 1] = plan.b_off[k] + (uint64_t)a.mb[k] * a.Wb[k];
        plan.n_cells += (uint64_t)a.Wa[k] * a.Wb[k];
    }
    if (plan.a_off[a.n_tasks]) { pg_need(a.a[0], "a's cells of track 0"); pg_need(a.a[1], "a's cells of track 1"); }
    if (plan.b_off[a.n_tasks]) { pg_need(a.b[0], "b's cells of track 0"); pg_need(a.b[1], "b's cells of track 1"); }
    auto is_letter = [](uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    for (uint32_t side = 0; side < 2; side++) {
        const uint8_t *const *c = side ? a.b : a.a;
        const uint64_t n = side ? plan.b_off[a.n_tasks] : plan.a_off[a.n_tasks];
        for (uint64_t k = 0; k < n; k++) {
            const bool g0 = c[0][k] == (uint8_t)'-', g1 = c[1][k] == (uint8_t)'-';
            if ((!g0 && !is_letter(c[0][k])) || (!g1 && !is_letter(c[1][k]))) fail(UC_ERR_ARGS, "progressive MSA: cell %llu of side %c is neither a letter nor '-'", (unsigned long long)k, side ? 'b' : 'a');
            if (g0 != g1) fail(UC_ERR_ARGS, "progressive MSA: the tracks of side %c disagree on the gap in cell %llu", side ? 'b' : 'a', (unsigned long long)k);
        }
    }
}

void msa_merge_host(const MsaMergeArgs &a, const MsaMergePlan &plan, uint32_t threads) {
    if (a.need) a.need[0] = a.need[1] = 0;
    if (!a.n_tasks) return;
    std::vector<MergeOut> out(a.n_tasks);
    over(threads, a.n_tasks, [&](uint64_t k) {
        const uint8_t *pa[2] = {a.a[0] + plan.a_off[k], a.a[1] + plan.a_off[k]}, *pb[2] = {a.b[0] + plan.b_off[k], a.b[1] + plan.b_off[k]};
        merge_one(a.ma[k], a.mb[k], a.Wa[k], a.Wb[k], pa, pb, a.S, a.gap_open, a.gap_ext, out[k]);
    });
    uint64_t nr = 0, nc = 0;
    a.run_off[0] = 0;
    for (uint32_t k = 0; k < a.n_tasks; k++) {
        const MergeOut &o = out[k];
        a.score[k] = o.score; a.is[k] = o.is; a.js[k] = o.js; a.ie[k] = o.ie; a.je[k] = o.je; a.width[k] = o.width;
        nr += o.runs.size(); nc += o.cells[0].size();
        a.run_off[k + 1] = nr;
    }
    if (a.need) { a.need[0] = nr; a.need[1] = nc; }
    if (nr > a.runs_capacity || nc > a.cells_capacity)
        fail(UC_ERR_ARGS, "progressive MSA: %llu runs and %llu cell bytes do not fit the capacities %llu and %llu", (unsigned long long)nr, (unsigned long long)nc,
             (unsigned long long)a.runs_capacity, (unsigned long long)a.cells_capacity);
    if (nr) pg_need(a.runs, "runs");
    if (nc) { pg_need(a.cells[0], "the cells of track 0"); pg_need(a.cells[1], "the cells of track 1"); }
    nc = 0;
    for (uint32_t k = 0; k < a.n_tasks; k++) {
        const MergeOut &o = out[k];
        if (!o.runs.empty()) memcpy(a.runs + a.run_off[k], o.runs.data(), o.runs.size() * 4);
        for (uint32_t tr = 0; tr < 2; tr++) if (!o.cells[tr].empty()) memcpy(a.cells[tr] + nc, o.cells[tr].data(), o.cells[tr].size());
        nc += o.cells[0].size();
    }
}

void msa_progressive_validate(const MsaProgressiveArgs &a, MsaProgressivePlan &plan) {
    check_gaps(a.gap_open, a.gap_ext);
    const uint64_t n_rows = check_groups(a.n_groups, a.grp_off);
    plan.n_rows = n_rows;
    plan.levels.clear();
    plan.node_off.assign((size_t)a.n_groups + 1, 0);
    plan.rows.clear();
    if (!a.n_groups) return;
    pg_need(a.res_off, "res_off"); pg_need(a.width, "width");
    check_matrix(a.S[0], "the amino-acid matrix"); check_matrix(a.S[1], "the 3Di matrix");
    if (a.res_off[0] != 0) fail(UC_ERR_ARGS, "progressive MSA: res_off[0] must be 0");
    for (uint64_t r = 0; r < n_rows; r++)
        if (a.res_off[r + 1] < a.res_off[r] || a.res_off[r + 1] - a.res_off[r] > 0x7fffffffull) fail(UC_ERR_ARGS, "progressive MSA: row %llu has a malformed residue range", (unsigned long long)r);
    if (a.res_off[n_rows]) { pg_need(a.res[0], "the residues of track 0"); pg_need(a.res[1], "the residues of track 1"); }
    if (n_rows > a.n_groups) pg_need(a.merges, "merges");
    for (uint32_t g = 0; g < a.n_groups; g++) plan.node_off[g + 1] = plan.node_off[g] + 2 * (a.grp_off[g + 1] - a.grp_off[g]) - 1;
    plan.rows.assign(plan.node_off[a.n_groups], 0);
    std::vector<uint32_t> level;
    std::vector<uint8_t> used;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, n0 = plan.node_off[g];
        const uint32_t *mg = a.merges + 2 * (b - g);
        level.assign(2 * m - 1, 0); used.assign(2 * m - 1, 0);
        for (uint64_t r = 0; r < m; r++) plan.rows[n0 + r] = 1;
        for (uint64_t k = 0; k + 1 < m; k++) {      // a tree over the group: every child exists already and is used once
            const uint32_t x = mg[2 * k], y = mg[2 * k + 1];
            if (x >= m + k || y >= m + k || x == y || used[x] || used[y]) fail(UC_ERR_ARGS, "progressive MSA: merge %llu of group %u (%u, %u) is not part of a tree over the group", (unsigned long long)k, g, x, y);
            used[x] = used[y] = 1;
            const uint64_t node = m + k;
            plan.rows[n0 + node] = plan.rows[n0 + x] + plan.rows[n0 + y];
            level[node] = std::max(level[x], level[y]) + 1;
            if (plan.levels.size() < level[node]) plan.levels.resize(level[node]);
            plan.levels[level[node] - 1].push_back(MsaProgMerge{g, x, y, (uint32_t)node});
        }
    }
}

void msa_progressive_host(const MsaProgressiveArgs &a, const MsaProgressivePlan &plan, uint32_t threads) {
    if (a.need) a.need[0] = 0;
    if (a.stats) *a.stats = MsaProgStats{0, 0, 0, 0};
    if (!a.n_groups) return;
    struct Node { uint32_t m = 0; uint64_t W = 0; std::vector<uint8_t> cells[2]; std::vector<uint32_t> order; };
    std::vector<Node> nodes(plan.node_off[a.n_groups]);
    for (uint32_t g = 0; g < a.n_groups; g++)
        for (uint64_t r = a.grp_off[g]; r < a.grp_off[g + 1]; r++) {
            Node &N = nodes[plan.node_off[g] + (r - a.grp_off[g])];
            N.m = 1; N.W = a.res_off[r + 1] - a.res_off[r]; N.order.assign(1, (uint32_t)(r - a.grp_off[g]));
            for (uint32_t tr = 0; tr < 2; tr++) N.cells[tr].assign(a.res[tr] + a.res_off[r], a.res[tr] + a.res_off[r] + N.W);
        }
    MsaProgStats st{0, plan.levels.size(), 0, 0};
    for (const std::vector<MsaProgMerge> &lv : plan.levels) {
        // UC-T/G/M's limits on the widths the two sides have, before the level runs
        for (const MsaProgMerge &M : lv) msa_merge_check_widths(nodes[plan.node_off[M.group] + M.a].W, nodes[plan.node_off[M.group] + M.b].W, a.gap_open, "a merge of group", M.group);
        over(threads, lv.size(), [&](uint64_t k) {
            const MsaProgMerge &M = lv[k];
            Node &X = nodes[plan.node_off[M.group] + M.a], &Y = nodes[plan.node_off[M.group] + M.b], &N = nodes[plan.node_off[M.group] + M.node];
            const uint8_t *pa[2] = {X.cells[0].data(), X.cells[1].data()}, *pb[2] = {Y.cells[0].data(), Y.cells[1].data()};
            MergeOut o;
            merge_one(X.m, Y.m, X.W, Y.W, pa, pb, a.S, a.gap_open, a.gap_ext, o);
            N.m = X.m + Y.m; N.W = o.width;
            N.cells[0].swap(o.cells[0]); N.cells[1].swap(o.cells[1]);
            N.order = X.order; N.order.insert(N.order.end(), Y.order.begin(), Y.order.end());
            for (uint32_t tr = 0; tr < 2; tr++) { std::vector<uint8_t>().swap(X.cells[tr]); std::vector<uint8_t>().swap(Y.cells[tr]); }
        });
        for (const MsaProgMerge &M : lv) { st.n_merges++; st.n_cells += nodes[plan.node_off[M.group] + M.a].W * nodes[plan.node_off[M.group] + M.b].W; }
    }
    uint64_t out = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) { const Node &R = nodes[plan.node_off[g + 1] - 1]; a.width[g] = (uint32_t)R.W; out += (uint64_t)R.m * R.W; }
    if (a.need) a.need[0] = out;
    if (out > a.cells_capacity) fail(UC_ERR_ARGS, "progressive MSA: %llu cell bytes do not fit the capacity %llu", (unsigned long long)out, (unsigned long long)a.cells_capacity);
    if (out) { pg_need(a.cells[0], "the cells of track 0"); pg_need(a.cells[1], "the cells of track 1"); }
    out = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const Node &R = nodes[plan.node_off[g + 1] - 1];
        for (uint32_t tr = 0; tr < 2; tr++)
            for (uint32_t r = 0; r < R.m; r++) if (R.W) memcpy(a.cells[tr] + out + (uint64_t)R.order[r] * R.W, R.cells[tr].data() + (uint64_t)r * R.W, R.W);
        out += (uint64_t)R.m * R.W;
    }
    if (a.stats) *a.stats = st;
}

}  // namespace uc

using namespace uc;

int uc_msa_self_scores(uint64_t n_rows, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int64_t *self) {
    return guard([&] { msa_self_scores(n_rows, res_off, res0, res1, SA, S3, self); });
}

int uc_msa_guide(uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, const int64_t *self, double *D, uint32_t *merges) {
    return guard([&] {
        const MsaGuideArgs a{n_groups, grp_off, scores, self, D, merges};
        std::vector<uint64_t> tri;
        msa_guide_validate(a, tri);
        msa_guide_run(a, tri, false, -1);
    });
}

int uc_msa_guide_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const int32_t *scores, const int64_t *self, double *D, uint32_t *merges) {
    return guard([&] {
        const MsaGuideArgs a{n_groups, grp_off, scores, self, D, merges};
        std::vector<uint64_t> tri;
        msa_guide_validate(a, tri);
        msa_guide_run(a, tri, true, device);
    });
}

namespace {
MsaMergeArgs merge_args(uint32_t n_tasks, const uint32_t *ma, const uint32_t *mb, const uint32_t *Wa, const uint32_t *Wb, const uint8_t *a0, const uint8_t *a1, const uint8_t *b0,
                        const uint8_t *b1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, int32_t *score, int32_t *is, int32_t *js, int32_t *ie, int32_t *je,
                        uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out) {
    return MsaMergeArgs{n_tasks, ma, mb, Wa, Wb, {a0, a1}, {b0, b1}, {SA, S3}, gap_open, gap_ext, score, is, js, ie, je, run_off, runs, runs_capacity, width, {cells0, cells1},
                        cells_capacity, need_out};
}
}  // namespace

int uc_msa_merge(uint32_t n_tasks, const uint32_t *ma, const uint32_t *mb, const uint32_t *Wa, const uint32_t *Wb, const uint8_t *a0, const uint8_t *a1, const uint8_t *b0,
                 const uint8_t *b1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, int32_t *score, int32_t *is, int32_t *js, int32_t *ie, int32_t *je,
                 uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out,
                 uint32_t threads) {
    return guard([&] {
        const MsaMergeArgs a = merge_args(n_tasks, ma, mb, Wa, Wb, a0, a1, b0, b1, S3, SA, gap_open, gap_ext, score, is, js, ie, je, run_off, runs, runs_capacity, width, cells0, cells1,
                                          cells_capacity, need_out);
        MsaMergePlan plan;
        msa_merge_validate(a, plan);
        msa_merge_host(a, plan, threads);
    });
}

int uc_msa_merge_dev(int32_t device, uint32_t n_tasks, const uint32_t *ma, const uint32_t *mb, const uint32_t *Wa, const uint32_t *Wb, const uint8_t *a0, const uint8_t *a1,
                     const uint8_t *b0, const uint8_t *b1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, int32_t *score, int32_t *is, int32_t *js, int32_t *ie,
                     int32_t *je, uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                     uint64_t *need_out) {
    return guard([&] {
        const MsaMergeArgs a = merge_args(n_tasks, ma, mb, Wa, Wb, a0, a1, b0, b1, S3, SA, gap_open, gap_ext, score, is, js, ie, je, run_off, runs, runs_capacity, width, cells0, cells1,
                                          cells_capacity, need_out);
        MsaMergePlan plan;
        msa_merge_validate(a, plan);
        msa_merge_device(device, a, plan);
    });
}

int uc_msa_progressive(uint32_t n_groups, const uint64_t *grp_off, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint32_t *merges, const int8_t *S3,
                       const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out,
                       uc_msa_progressive_stats *stats_out, uint32_t threads) {
    return guard([&] {
        MsaProgStats st{0, 0, 0, 0};
        const MsaProgressiveArgs a{n_groups, grp_off, res_off, {res0, res1}, merges, {SA, S3}, gap_open, gap_ext, width, {cells0, cells1}, cells_capacity, need_out, &st};
        MsaProgressivePlan plan;
        msa_progressive_validate(a, plan);
        msa_progressive_host(a, plan, threads);
        if (stats_out) *stats_out = uc_msa_progressive_stats{st.n_merges, st.n_levels, st.n_launches, st.n_cells};
    });
}

int uc_msa_progressive_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint32_t *merges,
                           const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint32_t *width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                           uint64_t *need_out, uc_msa_progressive_stats *stats_out) {
    return guard([&] {
        MsaProgStats st{0, 0, 0, 0};
        const MsaProgressiveArgs a{n_groups, grp_off, res_off, {res0, res1}, merges, {SA, S3}, gap_open, gap_ext, width, {cells0, cells1}, cells_capacity, need_out, &st};
        MsaProgressivePlan plan;
        msa_progressive_validate(a, plan);
        msa_progressive_device(device, a, plan);
        if (stats_out) *stats_out = uc_msa_progressive_stats{st.n_merges, st.n_levels, st.n_launches, st.n_cells};
    });
}

int uc_msa_progressive_geometry(uint32_t *chunk, uint32_t *cap, uint32_t *task_bytes_per_cell) {
    return guard([&] {
        if (!chunk || !cap || !task_bytes_per_cell) fail(UC_ERR_ARGS, "progressive MSA: the geometry's outputs must not be NULL");
        *chunk = MSA_PROG_CHUNK; *cap = 0; *task_bytes_per_cell = 2;      // one score byte and one decision byte
    });
}
