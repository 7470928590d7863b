// uc_msa_profile_host.cpp — rule UC-T/P, one profile refinement round of the star MSA: the checks host and device share, the host
// twins of the kernels of uc_msa_profile.hip and the C entry points.  Builds without HIP (tests/msa_profile_host_check.cpp links this file alone).
//   profile   num[track][c][x] = sum over the rows with a letter b in column c of S[b][x]; row r sees P_r[c][x] = floor((num - S[own][x]) / (m - 1))
//   DP        E5's H / E / F over columns x residues with the cell score P0_r[c][a_j] + P1_r[c][d_j]; one decision byte per cell; the end cell by
//             (largest score, smallest residue, smallest column); one walk with E6's preferences
//   layout    UC-T/L with a virtual centre of the MSA's width, then the columns without an amino acid are dropped
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "uc_files.h"
#include "uc_msa.h"

namespace uc {

namespace {

void need(const void *p, const char *what) { if (!p) fail(UC_ERR_ARGS, "profile MSA: %s must not be NULL", what); }

// grp_off, width and res_off of either call; fills cell_off and returns the row count
uint64_t check_shape(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint64_t *res_off, std::vector<uint64_t> &cell_off) {
    cell_off.assign((size_t)n_groups + 1, 0);
    if (!n_groups) return 0;
    need(grp_off, "grp_off"); need(width, "width"); need(res_off, "res_off");
    if (grp_off[0] != 0) fail(UC_ERR_ARGS, "profile MSA: grp_off[0] must be 0");
    for (uint32_t g = 0; g < n_groups; g++) {
        if (grp_off[g + 1] <= grp_off[g]) fail(UC_ERR_ARGS, "profile MSA: group %u is empty or grp_off decreases", g);
        const uint64_t m = grp_off[g + 1] - grp_off[g];
        if (m > MSA_PROFILE_MAX_ROWS) fail(UC_ERR_ARGS, "profile MSA: group %u has more than %u rows", g, MSA_PROFILE_MAX_ROWS);
        if (width[g] >> 31) fail(UC_ERR_ARGS, "profile MSA: group %u is 2^31 or more columns wide", g);
        cell_off[g + 1] = cell_off[g] + m * width[g];
    }
    const uint64_t n_rows = grp_off[n_groups];
    if (res_off[0] != 0) fail(UC_ERR_ARGS, "profile MSA: res_off[0] must be 0");
    for (uint64_t r = 0; r < n_rows; r++)
        if (res_off[r + 1] < res_off[r] || res_off[r + 1] - res_off[r] > 0x7fffffffull) fail(UC_ERR_ARGS, "profile MSA: row %llu has a malformed residue range", (unsigned long long)r);
    return n_rows;
}

bool is_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

}  // namespace

void msa_profile_align_validate(const MsaProfileAlignArgs &a, MsaProfilePlan &plan) {
    if (a.gap_ext < 0 || a.gap_open < a.gap_ext) fail(UC_ERR_ARGS, "profile MSA: gap open %d below gap extension %d, or a negative extension", a.gap_open, a.gap_ext);
    if (a.gap_open > (1 << 20)) fail(UC_ERR_ARGS, "profile MSA: gap open %d beyond 2^20", a.gap_open);
    const uint64_t n_rows = check_shape(a.n_groups, a.grp_off, a.width, a.res_off, plan.cell_off);
    plan.n_rows = n_rows;
    plan.col_off.assign((size_t)a.n_groups + 1, 0);
    plan.row_group.assign(n_rows, 0);
    plan.n_tasks = plan.n_cells = 0;
    if (!a.n_groups) return;
    need(a.S[0], "the amino-acid matrix"); need(a.S[1], "the 3Di matrix");
    need(a.aligned, "aligned"); need(a.score, "score"); need(a.qs, "qs"); need(a.ts, "ts"); need(a.qe, "qe"); need(a.te, "te"); need(a.run_off, "run_off");
    if (plan.cell_off[a.n_groups]) { need(a.cells[0], "the cells of track 0"); need(a.cells[1], "the cells of track 1"); }
    if (a.res_off[n_rows]) { need(a.res[0], "the residues of track 0"); need(a.res[1], "the residues of track 1"); }
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g];
        plan.col_off[g + 1] = plan.col_off[g] + W;
        const uint8_t *c0 = a.cells[0] + plan.cell_off[g], *c1 = a.cells[1] + plan.cell_off[g];
        for (uint64_t k = 0; k < m * W; k++) {
            const bool g0 = c0[k] == (uint8_t)'-', g1 = c1[k] == (uint8_t)'-';
            if ((!g0 && !is_letter(c0[k])) || (!g1 && !is_letter(c1[k])))
                fail(UC_ERR_ARGS, "profile MSA: cell %llu of group %u is neither a letter nor '-'", (unsigned long long)k, g);
            if (g0 != g1) fail(UC_ERR_ARGS, "profile MSA: the tracks of group %u disagree on the gap in cell %llu", g, (unsigned long long)k);
        }
        for (uint64_t r = b; r < b + m; r++) {
            plan.row_group[r] = g;
            const uint64_t L = a.res_off[r + 1] - a.res_off[r];
            if (W * L >> 31) fail(UC_ERR_ARGS, "profile MSA: row %llu needs %llu x %llu cells, 2^31 or more", (unsigned long long)r, (unsigned long long)W, (unsigned long long)L);
            // the decision bytes of a task are laid out by chunk of columns and anti-diagonal: ceil(W / chunk) x (L + chunk - 1) x chunk of them
            if ((W + MSA_PROFILE_CHUNK - 1) / MSA_PROFILE_CHUNK * (L + MSA_PROFILE_CHUNK - 1) * MSA_PROFILE_CHUNK >> 31)
                fail(UC_ERR_ARGS, "profile MSA: row %llu of %llu residues against %llu columns needs 2^31 or more decision bytes", (unsigned long long)r, (unsigned long long)L,
                     (unsigned long long)W);
            if (m > 1 && W && L) { plan.n_tasks++; plan.n_cells += W * L; }
        }
    }
}

namespace {

// the numerators of one group: num[(track * W + c) * 21 + x]
void numerators(const MsaProfileAlignArgs &a, const MsaProfilePlan &plan, uint32_t g, std::vector<int32_t> &num) {
    const uint64_t m = a.grp_off[g + 1] - a.grp_off[g], W = a.width[g];
    num.assign(2 * W * MSA_PROFILE_A, 0);
    for (uint32_t tr = 0; tr < 2; tr++) {
        const uint8_t *cells = a.cells[tr] + plan.cell_off[g];
        for (uint64_t i = 0; i < m; i++)
            for (uint64_t c = 0; c < W; c++) {
                const uint8_t ch = cells[i * W + c];
                if (ch == (uint8_t)'-') continue;
                const int8_t *row = a.S[tr] + msa_letter_code(ch) * MSA_PROFILE_A;
                int32_t *n = num.data() + (tr * W + c) * MSA_PROFILE_A;
                for (uint32_t x = 0; x < MSA_PROFILE_A; x++) n[x] += row[x];
            }
    }
}

struct TaskScratch { std::vector<int8_t> P; std::vector<int32_t> H, F; std::vector<uint8_t> dec; std::vector<uint32_t> rev; };

// one task; appends the row's runs to `runs`
void align_row(const MsaProfileAlignArgs &a, const MsaProfilePlan &plan, uint32_t g, uint64_t r, const std::vector<int32_t> &num, TaskScratch &S, std::vector<uint32_t> &runs) {
    const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g], L = a.res_off[r + 1] - a.res_off[r];
    const int32_t open = a.gap_open, ext = a.gap_ext, div = (int32_t)(m - 1);
    S.P.resize(2 * W * MSA_PROFILE_A);
    for (uint32_t tr = 0; tr < 2; tr++) {
        const uint8_t *own = a.cells[tr] + plan.cell_off[g] + (r - b) * W;
        for (uint64_t c = 0; c < W; c++) {
            const int8_t *sub = own[c] == (uint8_t)'-' ? nullptr : a.S[tr] + msa_letter_code(own[c]) * MSA_PROFILE_A;
            for (uint32_t x = 0; x < MSA_PROFILE_A; x++)
                S.P[(tr * W + c) * MSA_PROFILE_A + x] = (int8_t)msa_floor_div(num[(tr * W + c) * MSA_PROFILE_A + x] - (sub ? sub[x] : 0), div);
        }
    }
    const uint8_t *t0 = a.res[0] + a.res_off[r], *t1 = a.res[1] + a.res_off[r];
    S.H.assign(L + 1, 0); S.F.assign(L + 1, MSA_PROFILE_NEG);
    S.dec.resize(W * L);
    int32_t best = 0;
    uint64_t bi = 0, bj = 0;
    for (uint64_t i = 0; i < W; i++) {
        const int8_t *p0 = S.P.data() + i * MSA_PROFILE_A, *p1 = S.P.data() + (W + i) * MSA_PROFILE_A;
        int32_t hleft = 0, e = MSA_PROFILE_NEG, hdiag = 0;
        for (uint64_t j = 0; j < L; j++) {
            const int32_t upH = S.H[j + 1], upF = S.F[j + 1];
            const int32_t fn = std::max(upF - ext, upH - open), en = std::max(e - ext, hleft - open);
            const int32_t d = hdiag + p0[msa_letter_code(t0[j])] + p1[msa_letter_code(t1[j])];
            const int32_t h = std::max(std::max(0, d), std::max(en, fn));
            S.dec[i * L + j] = (uint8_t)((h == 0 ? 0 : h == d ? 1 : h == fn ? 2 : 3) | (fn == upH - open ? 4 : 0) | (en == hleft - open ? 8 : 0));
            hdiag = upH; S.H[j + 1] = h; S.F[j + 1] = fn; hleft = h; e = en;
            if (h > best || (h == best && best > 0 && j < bj)) { best = h; bi = i; bj = j; }
        }
    }
    a.score[r] = best;
    if (best <= 0) return;
    a.aligned[r] = 1; a.qe[r] = (int32_t)bi; a.te[r] = (int32_t)bj;
    int64_t i = (int64_t)bi, j = (int64_t)bj;
    uint32_t state = 0, op = 3, len = 0;
    S.rev.clear();
    auto emit = [&](uint32_t o) { if (o == op) { len++; return; } if (len) S.rev.push_back(len << 2 | op); op = o; len = 1; };
    while (i >= 0 && j >= 0) {
        const uint8_t d = S.dec[(uint64_t)i * L + (uint64_t)j];
        if (state == 0) {
            const uint32_t k = d & 3u;
            if (k == 0) break;
            if (k == 1) { emit(0); i--; j--; } else state = k == 2 ? 1 : 2;
        } else if (state == 1) { emit(1); if (d & 4u) state = 0; i--; }
        else { emit(2); if (d & 8u) state = 0; j--; }
    }
    if (len) S.rev.push_back(len << 2 | op);
    a.qs[r] = (int32_t)(i + 1); a.ts[r] = (int32_t)(j + 1);
    runs.insert(runs.end(), S.rev.rbegin(), S.rev.rend());
}

}  // namespace

void msa_profile_align_host(const MsaProfileAlignArgs &a, const MsaProfilePlan &plan, uint32_t threads) {
    if (a.need) a.need[0] = 0;
    if (!a.n_groups) return;
    const uint64_t n_rows = plan.n_rows;
    // the numerators of every group, then the rows: both over up to `threads` host threads, an item to the thread that draws its ticket; a row's runs
    // stay with the row until they are laid end to end, so the answer does not depend on the thread count
    std::vector<std::vector<int32_t>> num(a.n_groups);
    std::vector<std::vector<uint32_t>> row_runs(n_rows);
    auto over = [&](uint64_t count, auto &&fn) {
        const uint32_t nt = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(threads, 1), std::max<uint64_t>(count, 1));
        std::atomic<uint64_t> ticket{0};
        std::vector<std::string> err(nt);
        std::vector<int> code(nt, 0);
        auto work = [&](uint32_t t) {
            try {
                TaskScratch S;
                for (uint64_t k = ticket++; k < count; k = ticket++) fn(k, S);
            } catch (const Error &e) { code[t] = e.code; err[t] = e.what(); }
            catch (const std::exception &e) { code[t] = UC_ERR_GENERIC; err[t] = e.what(); }
        };
        std::vector<std::thread> pool;
        for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work, t);
        work(0);
        for (std::thread &t : pool) t.join();
        for (uint32_t t = 0; t < nt; t++) if (code[t]) fail(code[t], "%s", err[t].c_str());
    };
    over(a.n_groups, [&](uint64_t g, TaskScratch &) {
        if (a.grp_off[g + 1] - a.grp_off[g] > 1 && a.width[g]) numerators(a, plan, (uint32_t)g, num[g]);
    });
    over(n_rows, [&](uint64_t r, TaskScratch &S) {
        const uint32_t g = plan.row_group[r];
        a.aligned[r] = 0; a.score[r] = a.qs[r] = a.ts[r] = a.qe[r] = a.te[r] = 0;
        if (a.grp_off[g + 1] - a.grp_off[g] > 1 && a.width[g] && a.res_off[r + 1] > a.res_off[r]) align_row(a, plan, g, r, num[g], S, row_runs[r]);
    });
    a.run_off[0] = 0;
    for (uint64_t r = 0; r < n_rows; r++) a.run_off[r + 1] = a.run_off[r] + row_runs[r].size();
    const uint64_t total = a.run_off[n_rows];
    if (a.need) a.need[0] = total;
    if (total > a.runs_capacity) fail(UC_ERR_ARGS, "profile MSA: %llu runs do not fit the capacity %llu", (unsigned long long)total, (unsigned long long)a.runs_capacity);
    if (total) need(a.runs, "runs");
    for (uint64_t r = 0; r < n_rows; r++) if (!row_runs[r].empty()) memcpy(a.runs + a.run_off[r], row_runs[r].data(), row_runs[r].size() * 4);
}

void msa_profile_layout_validate(const MsaProfileLayoutArgs &a, MsaProfileLayoutPlan &plan) {
    const uint64_t n_rows = check_shape(a.n_groups, a.grp_off, a.width, a.res_off, plan.cell_off);
    plan.n_rows = n_rows;
    plan.bound.assign(a.n_groups, 0);
    if (!a.n_groups) return;
    need(a.aligned, "aligned"); need(a.qs, "qs"); need(a.ts, "ts"); need(a.run_off, "run_off"); need(a.new_width, "new_width");
    if (a.run_off[0] != 0) fail(UC_ERR_ARGS, "profile MSA: run_off[0] must be 0");
    for (uint64_t r = 0; r < n_rows; r++) if (a.run_off[r + 1] < a.run_off[r]) fail(UC_ERR_ARGS, "profile MSA: run_off decreases at row %llu", (unsigned long long)r);
    if (a.run_off[n_rows]) need(a.runs, "runs");
    if (a.res_off[n_rows]) { need(a.res[0], "the residues of track 0"); need(a.res[1], "the residues of track 1"); }
    uint64_t cols = 0;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g];
        uint64_t w = W;
        if (m == 1) { if (W) { need(a.cells_in[0], "the cells of track 0"); need(a.cells_in[1], "the cells of track 1"); } }
        else
            for (uint64_t r = b; r < b + m; r++) {
                if (!a.aligned[r]) continue;
                const uint64_t Lr = a.res_off[r + 1] - a.res_off[r];
                if (a.qs[r] < 0 || a.ts[r] < 0) fail(UC_ERR_ARGS, "profile MSA: row %llu starts at a negative position", (unsigned long long)r);
                uint64_t s = (uint64_t)a.qs[r], t = (uint64_t)a.ts[r];
                uint32_t prev = 3;
                for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                    const uint32_t x = a.runs[k], op = x & 3u, len = x >> 2;
                    if (op == 3u || len == 0) fail(UC_ERR_ARGS, "profile MSA: word 0x%x of row %llu is no run", x, (unsigned long long)r);
                    if (op == prev) fail(UC_ERR_ARGS, "profile MSA: adjacent runs of row %llu share an operation", (unsigned long long)r);
                    prev = op;
                    if (op != 2u) s += len;
                    if (op != 1u) t += len;
                    if (op == 2u) w += len;
                }
                if (s > W || t > Lr) fail(UC_ERR_ARGS, "profile MSA: the runs of row %llu overrun the columns or the row", (unsigned long long)r);
            }
        plan.bound[g] = w;
        cols += w;
        if (cols >> 31) fail(UC_ERR_ARGS, "profile MSA: 2^31 or more columns in one call");
    }
}

void msa_profile_layout_host(const MsaProfileLayoutArgs &a, const MsaProfileLayoutPlan &plan) {
    if (a.need) a.need[0] = 0;
    uint64_t out = 0;
    std::vector<uint32_t> ins, cx;
    std::vector<uint8_t> grid[2], keep;
    for (uint32_t g = 0; g < a.n_groups; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g];
        if (m == 1) {      // left as it is
            a.new_width[g] = (uint32_t)W;
            if (out + W <= a.cells_capacity && W)
                for (uint32_t tr = 0; tr < 2; tr++) { need(a.cells[tr], "cells"); memcpy(a.cells[tr] + out, a.cells_in[tr] + plan.cell_off[g], W); }
            out += W;
            continue;
        }
        ins.assign(W + 1, 0); cx.assign(W + 1, 0);
        for (uint64_t r = b; r < b + m; r++) {
            if (!a.aligned[r]) continue;
            uint64_t s = (uint64_t)a.qs[r];
            for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                const uint32_t x = a.runs[k], len = x >> 2;
                if ((x & 3u) == 2u) ins[s] = std::max(ins[s], len); else s += len;
            }
        }
        uint32_t cum = 0;
        for (uint64_t s = 0; s <= W; s++) { cum += ins[s]; cx[s] = (uint32_t)s + cum; }
        const uint64_t W2 = cx[W];
        for (uint32_t tr = 0; tr < 2; tr++) {
            grid[tr].assign(m * W2, (uint8_t)'-');
            for (uint64_t r = b; r < b + m; r++) {
                if (!a.aligned[r]) continue;
                uint8_t *o = grid[tr].data() + (r - b) * W2;
                const uint8_t *x = a.res[tr] + a.res_off[r];
                uint64_t s = (uint64_t)a.qs[r], t = (uint64_t)a.ts[r];
                for (uint64_t k = a.run_off[r]; k < a.run_off[r + 1]; k++) {
                    const uint32_t w = a.runs[k], len = w >> 2, op = w & 3u;
                    if (op == 0u) { for (uint32_t l = 0; l < len; l++) o[cx[s + l]] = x[t + l]; s += len; t += len; }
                    else if (op == 1u) s += len;
                    else { memcpy(o + (cx[s] - ins[s]), x + t, len); t += len; }
                }
            }
        }
        keep.assign(W2, 0);
        uint64_t W3 = 0;
        for (uint64_t c = 0; c < W2; c++) {
            for (uint64_t i = 0; i < m && !keep[c]; i++) keep[c] = grid[0][i * W2 + c] != (uint8_t)'-';
            W3 += keep[c];
        }
        a.new_width[g] = (uint32_t)W3;
        if (out + m * W3 <= a.cells_capacity && W3 > 0)
            for (uint32_t tr = 0; tr < 2; tr++) {
                need(a.cells[tr], "cells");
                uint8_t *o = a.cells[tr] + out;
                for (uint64_t i = 0; i < m; i++)
                    for (uint64_t c = 0; c < W2; c++) if (keep[c]) *o++ = grid[tr][i * W2 + c];
            }
        out += m * W3;
    }
    if (a.need) a.need[0] = out;
    if (out > a.cells_capacity) fail(UC_ERR_ARGS, "profile MSA: %llu cell bytes do not fit the capacity %llu", (unsigned long long)out, (unsigned long long)a.cells_capacity);
}

}  // namespace uc

using namespace uc;

namespace {
MsaProfileAlignArgs align_args(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0, const uint8_t *cells1, const uint64_t *res_off,
                               const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint8_t *aligned, int32_t *score,
                               int32_t *qs, int32_t *ts, int32_t *qe, int32_t *te, uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity, uint64_t *need_out) {
    return MsaProfileAlignArgs{n_groups, grp_off, width, {cells0, cells1}, res_off, {res0, res1}, {SA, S3}, gap_open, gap_ext, aligned, score, qs, ts, qe, te, run_off, runs,
                               runs_capacity, need_out};
}
MsaProfileLayoutArgs layout_args(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0_in, const uint8_t *cells1_in, const uint64_t *res_off,
                                 const uint8_t *res0, const uint8_t *res1, const uint8_t *aligned, const int32_t *qs, const int32_t *ts, const uint64_t *run_off,
                                 const uint32_t *runs, uint32_t *new_width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity, uint64_t *need_out) {
    return MsaProfileLayoutArgs{n_groups, grp_off, width, {cells0_in, cells1_in}, res_off, {res0, res1}, aligned, qs, ts, run_off, runs, new_width, {cells0, cells1},
                                cells_capacity, need_out};
}
}  // namespace

int uc_msa_profile_align(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0, const uint8_t *cells1, const uint64_t *res_off,
                         const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int32_t gap_open, int32_t gap_ext, uint8_t *aligned,
                         int32_t *score, int32_t *qs, int32_t *ts, int32_t *qe, int32_t *te, uint64_t *run_off, uint32_t *runs, uint64_t runs_capacity,
                         uint64_t *need_out, uint32_t threads) {
    return guard([&] {
        const MsaProfileAlignArgs a = align_args(n_groups, grp_off, width, cells0, cells1, res_off, res0, res1, S3, SA, gap_open, gap_ext, aligned, score, qs, ts, qe, te, run_off,
                                                 runs, runs_capacity, need_out);
        MsaProfilePlan plan;
        msa_profile_align_validate(a, plan);
        msa_profile_align_host(a, plan, threads);
    });
}

int uc_msa_profile_align_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0, const uint8_t *cells1,
                             const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *S3, const int8_t *SA, int32_t gap_open,
                             int32_t gap_ext, uint8_t *aligned, int32_t *score, int32_t *qs, int32_t *ts, int32_t *qe, int32_t *te, uint64_t *run_off,
                             uint32_t *runs, uint64_t runs_capacity, uint64_t *need_out) {
    return guard([&] {
        const MsaProfileAlignArgs a = align_args(n_groups, grp_off, width, cells0, cells1, res_off, res0, res1, S3, SA, gap_open, gap_ext, aligned, score, qs, ts, qe, te, run_off,
                                                 runs, runs_capacity, need_out);
        MsaProfilePlan plan;
        msa_profile_align_validate(a, plan);
        msa_profile_align_device(device, a, plan);
    });
}

int uc_msa_profile_layout(uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0_in, const uint8_t *cells1_in,
                          const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint8_t *aligned, const int32_t *qs, const int32_t *ts,
                          const uint64_t *run_off, const uint32_t *runs, uint32_t *new_width, uint8_t *cells0, uint8_t *cells1, uint64_t cells_capacity,
                          uint64_t *need_out) {
    return guard([&] {
        const MsaProfileLayoutArgs a = layout_args(n_groups, grp_off, width, cells0_in, cells1_in, res_off, res0, res1, aligned, qs, ts, run_off, runs, new_width, cells0, cells1,
                                                   cells_capacity, need_out);
        MsaProfileLayoutPlan plan;
        msa_profile_layout_validate(a, plan);
        msa_profile_layout_host(a, plan);
    });
}

int uc_msa_profile_layout_dev(int32_t device, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *width, const uint8_t *cells0_in,
                              const uint8_t *cells1_in, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const uint8_t *aligned, const int32_t *qs,
                              const int32_t *ts, const uint64_t *run_off, const uint32_t *runs, uint32_t *new_width, uint8_t *cells0, uint8_t *cells1,
                              uint64_t cells_capacity, uint64_t *need_out) {
    return guard([&] {
        const MsaProfileLayoutArgs a = layout_args(n_groups, grp_off, width, cells0_in, cells1_in, res_off, res0, res1, aligned, qs, ts, run_off, runs, new_width, cells0, cells1,
                                                   cells_capacity, need_out);
        MsaProfileLayoutPlan plan;
        msa_profile_layout_validate(a, plan);
        msa_profile_layout_device(device, a, plan);
    });
}

int uc_msa_profile_geometry(uint32_t *chunk, uint32_t *cap, uint32_t *task_bytes_per_cell) {
    return guard([&] {
        if (!chunk || !cap || !task_bytes_per_cell) fail(UC_ERR_ARGS, "profile MSA: the geometry's outputs must not be NULL");
        *chunk = MSA_PROFILE_CHUNK; *cap = 0; *task_bytes_per_cell = 1;
    });
}
