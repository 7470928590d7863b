// uc_msa_profile.hip — the device side of rule UC-T/P (`unicore tree -a profile`): one profile refinement round of the star MSA.
// Every launch serves all groups (numerators) or all tasks of a batch (DP, walk); a task is one row of a group with two rows or more.
//   numerators  one thread per (track, column, letter x): num = sum over the rows with a letter b in the column of S[b][x]; shared by the group's rows
//   DP          one wave (a 64-thread block) per task.  Lane l holds column c0 + l of a chunk of 64 columns and walks down the row's residues one
//               anti-diagonal per step: at step t it computes cell (c0 + l, t - l).  The row's own profile of the chunk is formed while it is staged in
//               LDS (the own cell's matrix row subtracted, floor division by m - 1, bytes laid out [track][letter][lane]); H, E, F stay in registers,
//               the upper neighbour's H and F arrive by DPP wave_shr:1, the row's letters move down the lanes the same way; the last lane of a chunk
//               leaves H and F of its column in a per-task boundary row that lane 0 of the next chunk reads (two rows, alternating).  One decision
//               byte per cell (bits 0-1: H is 0 / diagonal / F / E, in E6's order of preference; bit 2: F opened here; bit 3: E opened here) goes to the
//               batch's buffer, laid out [chunk][step][lane] so that a step is one 64-byte store.  Every lane keeps (best score, smallest residue,
//               smallest column) of its columns; a butterfly over the lanes takes the same key, so the end cell does not depend on scheduling.
//   walk        one thread per task reads the decision bytes backwards from the end cell and writes the runs from the end of the task's run buffer
//   layout      UC-T/L with a virtual centre: the star MSA's own kernels (msa_star_device of uc_msa.hip) over the group plus one row of `-` as the
//               centre; then the columns whose count is 0 are dropped here (flags, exclusive scan, compaction), and the virtual row with them
// Vector stores only, no atomics.  Scratch is hipMalloc'ed and freed inside the call, as in uc_msa.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_engine.h"
#include "uc_msa.h"

namespace uc {

namespace {

constexpr int MP_WAVE = 64;
static_assert(MSA_PROFILE_CHUNK == MP_WAVE, "one column per lane");
constexpr uint32_t MP_A = MSA_PROFILE_A;
constexpr uint8_t MP_GAP = 255;      // the code of `-`
constexpr const char *MP_NO_FALLBACK = "the device side of the profile MSA has no CPU fallback (the host twins are separate entry points)";

struct MpTask {
    uint64_t dec_off;      // into the batch's decision bytes
    uint64_t own_off;      // the row's own cells
    uint64_t num_col;      // the group's first column in num
    uint64_t res_off;      // the row's residues
    uint64_t bnd_off;      // 4 L ints: two boundary rows of H and F
    uint64_t run_off;      // W + L words
    uint32_t W, L, div, pad;
};

__device__ __forceinline__ uint32_t mp_seg(const uint64_t *off, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

// num[(track * n_cols + column) * 21 + x]
__global__ void __launch_bounds__(256) mp_num_kernel(uint64_t n_cols, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *col_off, const uint64_t *cell_off,
                                                     const uint8_t *code0, const uint8_t *code1, const int8_t *S, int32_t *num) {
    __shared__ int8_t s_S[2 * MP_A * MP_A];
    for (uint32_t k = threadIdx.x; k < 2 * MP_A * MP_A; k += 256) s_S[k] = S[k];
    __syncthreads();
    const uint64_t n_items = 2 * n_cols * MP_A;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_items; k += (uint64_t)gridDim.x * 256) {
        const uint32_t x = (uint32_t)(k % MP_A), tr = (uint32_t)(k / (n_cols * MP_A));
        const uint64_t col = (k / MP_A) % n_cols;
        const uint32_t g = mp_seg(col_off, n_groups, col);
        const uint64_t m = grp_off[g + 1] - grp_off[g], W = col_off[g + 1] - col_off[g];
        const uint8_t *p = (tr ? code1 : code0) + cell_off[g] + (col - col_off[g]);
        const int8_t *Sx = s_S + tr * MP_A * MP_A + x;
        int32_t acc = 0;
        for (uint64_t i = 0; i < m; i++) {
            const uint8_t b = p[i * W];
            if (b != MP_GAP) acc += Sx[b * MP_A];
        }
        num[k] = acc;
    }
}

__device__ __forceinline__ int mp_from_prev_lane(int v, int lane0) { return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false); }      // wave_shr:1

// out[3 task .. ]: score, end column, end residue
__global__ void __launch_bounds__(MP_WAVE) mp_dp_kernel(uint32_t n_tasks, const MpTask *tasks, uint64_t n_cols, const int32_t *num, const uint8_t *code0, const uint8_t *code1,
                                                        const int8_t *S, const uint16_t *res, int open, int ext, uint8_t *dec, int32_t *bnd, int32_t *out) {
    __shared__ int8_t s_S[2 * MP_A * MP_A];
    __shared__ int8_t s_P[2][MP_A][MP_WAVE];
    const uint32_t task = blockIdx.x;
    if (task >= n_tasks) return;
    const int lane = (int)threadIdx.x;
    for (uint32_t k = threadIdx.x; k < 2 * MP_A * MP_A; k += MP_WAVE) s_S[k] = S[k];
    const MpTask T = tasks[task];
    const int W = (int)T.W, L = (int)T.L, div = (int)T.div;
    const uint16_t *t = res + T.res_off;
    uint8_t *d = dec + T.dec_off;
    int best = 0, bi = 0, bj = 0;
    const int n_chunks = (W + MP_WAVE - 1) / MP_WAVE;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int c0 = ch * MP_WAVE, nl = min(MP_WAVE, W - c0);
        __syncthreads();      // the last chunk's lookups are over (and s_S is there)
        for (int tr = 0; tr < 2; tr++) {
            const uint8_t *own = (tr ? code1 : code0) + T.own_off + c0;
            const int32_t *nm = num + ((uint64_t)tr * n_cols + T.num_col + c0) * MP_A;
            for (int e = lane; e < nl * (int)MP_A; e += MP_WAVE) {
                const int c = e / (int)MP_A, x = e - c * (int)MP_A;
                const uint8_t o = own[c];
                const int n = nm[e] - (o != MP_GAP ? (int)s_S[(tr * MP_A + o) * MP_A + x] : 0);
                const int q = n / div;
                s_P[tr][x][c] = (int8_t)((n % div != 0 && n < 0) ? q - 1 : q);
            }
        }
        __syncthreads();
        const int32_t *b_in = bnd + T.bnd_off + (uint64_t)(ch & 1) * 2 * L;
        int32_t *b_out = bnd + T.bnd_off + (uint64_t)((ch + 1) & 1) * 2 * L;
        const bool has_in = ch > 0, has_out = ch + 1 < n_chunks, mine = lane < nl;
        int H = 0, E = MSA_PROFILE_NEG, F = MSA_PROFILE_NEG, diag = 0, let = 0;
        int nxt_let = 0, nxt_h = 0, nxt_f = MSA_PROFILE_NEG;
        uint8_t *dc = d + (uint64_t)ch * (uint64_t)(L + MP_WAVE - 1) * MP_WAVE + lane;
        const int steps = L + MP_WAVE - 1;
        for (int s = 0; s < steps; s++) {
            const int k = s & (MP_WAVE - 1);
            if (k == 0) {      // the next 64 residues (and boundary cells), one per lane
                const int idx = s + lane;
                nxt_let = idx < L ? (int)t[idx] : 0;
                if (has_in) { nxt_h = idx < L ? b_in[idx] : 0; nxt_f = idx < L ? b_in[L + idx] : MSA_PROFILE_NEG; }
            }
            const int in_let = __builtin_amdgcn_readlane(nxt_let, k);
            const int in_h = has_in ? __builtin_amdgcn_readlane(nxt_h, k) : 0;
            const int in_f = has_in ? __builtin_amdgcn_readlane(nxt_f, k) : MSA_PROFILE_NEG;
            let = mp_from_prev_lane(let, in_let);
            const int upH = mp_from_prev_lane(H, in_h), upF = mp_from_prev_lane(F, in_f);
            const int j = s - lane;
            const bool valid = mine && j >= 0 && j < L;
            const int a0 = let & 0xff, a1 = (let >> 8) & 0xff;      // both below 21: codes, and 0 where no residue has arrived
            const int sc = (int)s_P[0][a0][lane] + (int)s_P[1][a1][lane];
            int fn = max(upF - ext, upH - open), en = max(E - ext, H - open);
            const int dg = diag + sc;
            int h = max(max(0, dg), max(en, fn));
            const uint32_t bits = (h == 0 ? 0u : h == dg ? 1u : h == fn ? 2u : 3u) | (fn == upH - open ? 4u : 0u) | (en == H - open ? 8u : 0u);
            dc[(uint64_t)s * MP_WAVE] = (uint8_t)bits;      // cells outside the matrix land in the buffer's slack and are never read
            if (!valid) { h = 0; en = MSA_PROFILE_NEG; fn = MSA_PROFILE_NEG; }
            if (valid && (h > best || (h == best && best > 0 && j < bj))) { best = h; bi = c0 + lane; bj = j; }
            diag = upH; H = h; E = en; F = fn;
            if (has_out && lane == MP_WAVE - 1 && valid) { b_out[j] = h; b_out[L + j] = fn; }
        }
    }
    for (int o = 1; o < MP_WAVE; o <<= 1) {
        const int s2 = __shfl_xor(best, o, MP_WAVE), i2 = __shfl_xor(bi, o, MP_WAVE), j2 = __shfl_xor(bj, o, MP_WAVE);
        if (s2 > best || (s2 == best && (j2 < bj || (j2 == bj && i2 < bi)))) { best = s2; bi = i2; bj = j2; }
    }
    if (lane == 0) { out[3 * (uint64_t)task] = best; out[3 * (uint64_t)task + 1] = bi; out[3 * (uint64_t)task + 2] = bj; }
}

// walk[3 task ..]: first column, first residue, run count; the runs end at the end of the task's buffer
__global__ void __launch_bounds__(256) mp_walk_kernel(uint32_t n_tasks, const MpTask *tasks, const int32_t *out, const uint8_t *dec, uint32_t *runbuf, int32_t *walk) {
    for (uint32_t task = blockIdx.x * 256 + threadIdx.x; task < n_tasks; task += gridDim.x * 256) {
        const MpTask T = tasks[task];
        const uint8_t *d = dec + T.dec_off;
        const uint64_t stride = (uint64_t)(T.L + MP_WAVE - 1) * MP_WAVE;
        uint32_t *end = runbuf + T.run_off + T.W + T.L, *p = end;
        int i = out[3 * (uint64_t)task + 1], j = out[3 * (uint64_t)task + 2];
        uint32_t state = 0, op = 3, len = 0;
        if (out[3 * (uint64_t)task] > 0)
            while (i >= 0 && j >= 0) {
                const uint32_t l = (uint32_t)i & (MP_WAVE - 1);
                const uint32_t b = d[(uint64_t)(i >> 6) * stride + (uint64_t)(j + l) * MP_WAVE + l];
                uint32_t o;
                if (state == 0) {
                    const uint32_t k = b & 3u;
                    if (k == 0) break;
                    if (k != 1) { state = k == 2 ? 1 : 2; continue; }
                    o = 0; i--; j--;
                } else if (state == 1) { o = 1; if (b & 4u) state = 0; i--; }
                else { o = 2; if (b & 8u) state = 0; j--; }
                if (o == op) len++;
                else { if (len) *--p = len << 2 | op; op = o; len = 1; }
            }
        if (len) *--p = len << 2 | op;
        walk[3 * (uint64_t)task] = i + 1; walk[3 * (uint64_t)task + 1] = j + 1; walk[3 * (uint64_t)task + 2] = (int32_t)(end - p);
    }
}

// ---- the drop of the empty columns: n_cols + 1 flags, the last one 0
__global__ void __launch_bounds__(256) mp_flag_kernel(uint64_t n_cols, const uint32_t *cnt, uint32_t *flag) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x <= n_cols; x += (uint64_t)gridDim.x * 256) flag[x] = x < n_cols && cnt[x] ? 1u : 0u;
}
// in: group g holds (m_g + 1) x width rows (the last one the virtual centre); out: m_g x new width at out_off[g]
__global__ void __launch_bounds__(256) mp_compact_kernel(uint64_t n_cells, uint32_t n_groups, const uint64_t *wcol_off, const uint64_t *cell_off, const uint64_t *out_off,
                                                         const uint32_t *flag, const uint32_t *pos, const uint8_t *in0, const uint8_t *in1, uint8_t *out0, uint8_t *out1) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n_cells; x += (uint64_t)gridDim.x * 256) {
        const uint32_t g = mp_seg(cell_off, n_groups, x);
        const uint64_t W = wcol_off[g + 1] - wcol_off[g], rem = x - cell_off[g], i = rem / W, c = rem % W, col = wcol_off[g] + c;
        const uint64_t m = (cell_off[g + 1] - cell_off[g]) / W - 1;
        if (i < m && flag[col]) {
            const uint64_t o = out_off[g] + i * (pos[wcol_off[g + 1]] - pos[wcol_off[g]]) + (pos[col] - pos[wcol_off[g]]);
            out0[o] = in0[x]; out1[o] = in1[x];
        }
    }
}

template <typename T>
void up(DevBuf<T> &d, const T *src, size_t n) {
    d.reserve_exact(std::max<size_t>(n, 1));
    if (n) UC_HIP(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
}

}  // namespace

void msa_profile_align_device(int device, const MsaProfileAlignArgs &a, const MsaProfilePlan &plan) {
    use_device(device, MP_NO_FALLBACK);
    if (a.need) a.need[0] = 0;
    const uint32_t ng = a.n_groups;
    if (!ng) return;
    const uint64_t n_rows = plan.n_rows;
    for (uint64_t r = 0; r < n_rows; r++) { a.aligned[r] = 0; a.score[r] = a.qs[r] = a.ts[r] = a.qe[r] = a.te[r] = 0; }
    std::fill(a.run_off, a.run_off + n_rows + 1, 0);
    if (!plan.n_tasks) return;
    const uint64_t n_cells = plan.cell_off[ng], n_cols = plan.col_off[ng], n_res = a.res_off[n_rows];
    // codes: the loader's mapping, 255 for a gap; the two letters of a residue in one 16-bit word
    std::vector<uint8_t> code[2];
    for (uint32_t tr = 0; tr < 2; tr++) {
        code[tr].resize(n_cells);
        for (uint64_t k = 0; k < n_cells; k++) code[tr][k] = a.cells[tr][k] == (uint8_t)'-' ? MP_GAP : (uint8_t)msa_letter_code(a.cells[tr][k]);
    }
    std::vector<uint16_t> res(n_res);
    for (uint64_t k = 0; k < n_res; k++) res[k] = (uint16_t)(msa_letter_code(a.res[0][k]) | msa_letter_code(a.res[1][k]) << 8);
    std::vector<int8_t> S(2 * MP_A * MP_A);
    memcpy(S.data(), a.S[0], MP_A * MP_A); memcpy(S.data() + MP_A * MP_A, a.S[1], MP_A * MP_A);
    hipStream_t s = nullptr;
    DevBuf<uint64_t> d_grp, d_col, d_cell;
    DevBuf<uint8_t> d_c0, d_c1, d_dec;
    DevBuf<uint16_t> d_res;
    DevBuf<int8_t> d_S;
    DevBuf<int32_t> d_num, d_bnd, d_out, d_walk;
    DevBuf<uint32_t> d_runs;
    DevBuf<MpTask> d_tasks;
    up(d_grp, a.grp_off, (size_t)ng + 1); up(d_col, plan.col_off.data(), (size_t)ng + 1); up(d_cell, plan.cell_off.data(), (size_t)ng + 1);
    up(d_c0, code[0].data(), n_cells); up(d_c1, code[1].data(), n_cells); up(d_res, res.data(), n_res); up(d_S, S.data(), S.size());
    d_num.reserve_exact(2 * n_cols * MP_A);
    hipLaunchKernelGGL(mp_num_kernel, grid_for(2 * n_cols * MP_A), dim3(256), 0, s, n_cols, ng, (const uint64_t *)d_grp.p, (const uint64_t *)d_col.p, (const uint64_t *)d_cell.p,
                       (const uint8_t *)d_c0.p, (const uint8_t *)d_c1.p, (const int8_t *)d_S.p, d_num.p);
    UC_HIP(hipGetLastError());

    // batches of tasks whose decision bytes fit the budget (one task at least)
    const uint64_t budget = tree_budget_bytes();
    const bool timing = getenv("UC_TIMING") != nullptr;
    double dp_ms = 0;
    std::vector<MpTask> tasks;
    std::vector<uint64_t> task_row;
    std::vector<int32_t> out, walk;
    std::vector<uint32_t> runbuf, runs;
    uint64_t r = 0;
    while (r < n_rows) {
        tasks.clear(); task_row.clear();
        uint64_t dec_bytes = 0, bnd_ints = 0, run_words = 0;
        for (; r < n_rows; r++) {
            const uint32_t g = plan.row_group[r];
            const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g], L = a.res_off[r + 1] - a.res_off[r];
            if (m < 2 || !W || !L) continue;
            const uint64_t bytes = (W + MP_WAVE - 1) / MP_WAVE * (L + MP_WAVE - 1) * MP_WAVE;
            if (!tasks.empty() && (dec_bytes + bytes > budget || tasks.size() >= (1u << 30))) break;
            tasks.push_back(MpTask{dec_bytes, plan.cell_off[g] + (r - b) * W, plan.col_off[g], a.res_off[r], bnd_ints, run_words, (uint32_t)W, (uint32_t)L, (uint32_t)(m - 1), 0});
            task_row.push_back(r);
            dec_bytes += bytes; bnd_ints += 4 * L; run_words += W + L;
        }
        if (tasks.empty()) break;
        const uint32_t nt = (uint32_t)tasks.size();
        up(d_tasks, tasks.data(), nt);
        d_dec.reserve(dec_bytes); d_bnd.reserve(bnd_ints); d_runs.reserve(run_words); d_out.reserve((size_t)nt * 3); d_walk.reserve((size_t)nt * 3);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timing) { UC_HIP(hipEventCreate(&e0)); UC_HIP(hipEventCreate(&e1)); UC_HIP(hipEventRecord(e0, s)); }
        hipLaunchKernelGGL(mp_dp_kernel, dim3(nt), dim3(MP_WAVE), 0, s, nt, (const MpTask *)d_tasks.p, n_cols, (const int32_t *)d_num.p, (const uint8_t *)d_c0.p,
                           (const uint8_t *)d_c1.p, (const int8_t *)d_S.p, (const uint16_t *)d_res.p, (int)a.gap_open, (int)a.gap_ext, d_dec.p, d_bnd.p, d_out.p);
        if (timing) UC_HIP(hipEventRecord(e1, s));
        hipLaunchKernelGGL(mp_walk_kernel, grid_for(nt), dim3(256), 0, s, nt, (const MpTask *)d_tasks.p, (const int32_t *)d_out.p, (const uint8_t *)d_dec.p, d_runs.p, d_walk.p);
        UC_HIP(hipGetLastError());
        UC_HIP(hipStreamSynchronize(s));
        if (timing) { float ms = 0; UC_HIP(hipEventElapsedTime(&ms, e0, e1)); dp_ms += ms; UC_HIP(hipEventDestroy(e0)); UC_HIP(hipEventDestroy(e1)); }
        out.resize((size_t)nt * 3); walk.resize((size_t)nt * 3); runbuf.resize(run_words);
        UC_HIP(hipMemcpy(out.data(), d_out.p, (size_t)nt * 12, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(walk.data(), d_walk.p, (size_t)nt * 12, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(runbuf.data(), d_runs.p, run_words * 4, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < nt; k++) {
            const uint64_t row = task_row[k];
            a.score[row] = out[3 * (size_t)k];
            if (out[3 * (size_t)k] <= 0) continue;
            a.aligned[row] = 1; a.qe[row] = out[3 * (size_t)k + 1]; a.te[row] = out[3 * (size_t)k + 2];
            a.qs[row] = walk[3 * (size_t)k]; a.ts[row] = walk[3 * (size_t)k + 1];
            const uint64_t n = (uint64_t)walk[3 * (size_t)k + 2], end = tasks[k].run_off + tasks[k].W + tasks[k].L;
            if (n > (uint64_t)tasks[k].W + tasks[k].L) fail(UC_ERR_GENERIC, "profile MSA: the walk of row %llu reports %llu runs", (unsigned long long)row, (unsigned long long)n);
            runs.insert(runs.end(), runbuf.begin() + (end - n), runbuf.begin() + end);
            a.run_off[row + 1] = n;
        }
    }
    for (uint64_t k = 0; k < n_rows; k++) a.run_off[k + 1] += a.run_off[k];
    if (timing) fprintf(stderr, "unicore-cluster[timing]: profile MSA: %llu tasks, %llu cells, DP kernel %.3f ms\n", (unsigned long long)plan.n_tasks, (unsigned long long)plan.n_cells, dp_ms);
    if (a.need) a.need[0] = runs.size();
    if (runs.size() > a.runs_capacity) fail(UC_ERR_ARGS, "profile MSA: %llu runs do not fit the capacity %llu", (unsigned long long)runs.size(), (unsigned long long)a.runs_capacity);
    if (!runs.empty()) {
        if (!a.runs) fail(UC_ERR_ARGS, "profile MSA: runs must not be NULL");
        memcpy(a.runs, runs.data(), runs.size() * 4);
    }
}

void msa_profile_layout_device(int device, const MsaProfileLayoutArgs &a, const MsaProfileLayoutPlan &plan) {
    use_device(device, MP_NO_FALLBACK);
    if (a.need) a.need[0] = 0;
    const uint32_t ng = a.n_groups;
    if (!ng) return;
    // the star call: every group of two rows or more, with one more row of `-` as long as the MSA is wide as its centre
    std::vector<uint32_t> sub;      // the groups of the star call
    std::vector<uint64_t> go(1, 0), ro(1, 0), uo(1, 0);
    std::vector<uint32_t> centre, runs;
    std::vector<int32_t> qs, ts;
    std::vector<uint8_t> al, res[2];
    uint64_t cols = 0, cells = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t b = a.grp_off[g], m = a.grp_off[g + 1] - b, W = a.width[g];
        if (m == 1) continue;
        sub.push_back(g);
        for (uint64_t r = b; r < b + m; r++) {
            const uint64_t L = a.res_off[r + 1] - a.res_off[r];
            for (uint32_t tr = 0; tr < 2; tr++) res[tr].insert(res[tr].end(), a.res[tr] + a.res_off[r], a.res[tr] + a.res_off[r] + L);
            ro.push_back(ro.back() + L);
            qs.push_back(a.qs[r]); ts.push_back(a.ts[r]); al.push_back(a.aligned[r]);
            if (a.aligned[r]) runs.insert(runs.end(), a.runs + a.run_off[r], a.runs + a.run_off[r + 1]);
            uo.push_back(runs.size());
        }
        for (uint32_t tr = 0; tr < 2; tr++) res[tr].insert(res[tr].end(), W, (uint8_t)'-');
        ro.push_back(ro.back() + W); uo.push_back(runs.size());
        qs.push_back(0); ts.push_back(0); al.push_back(1);
        centre.push_back((uint32_t)m);
        go.push_back(go.back() + m + 1);
        cols += plan.bound[g]; cells += (m + 1) * plan.bound[g];
    }
    const uint32_t ns = (uint32_t)sub.size();
    std::vector<uint32_t> width(std::max<uint32_t>(ns, 1)), col(std::max<uint64_t>(cols, 1)), cnt(std::max<uint64_t>(cols, 1));
    std::vector<uint8_t> c0(std::max<uint64_t>(cells, 1)), c1(std::max<uint64_t>(cells, 1));
    if (ns) {
        const MsaStarArgs sa{ns, go.data(), centre.data(), 2, ro.data(), {res[0].data(), res[1].data()}, qs.data(), ts.data(), uo.data(), runs.data(), al.data(), width.data(),
                             col.data(), cnt.data(), cols, {c0.data(), c1.data()}, cells, nullptr};
        MsaStarPlan sp;
        msa_star_validate(sa, sp);
        msa_star_device(device, sa, sp);
    }
    // the new widths from the counts, and where every group's rows go
    std::vector<uint64_t> wcol((size_t)ns + 1, 0), cell((size_t)ns + 1, 0), out_off(std::max<uint32_t>(ns, 1), 0);
    uint64_t out = 0;
    for (uint32_t g = 0, k = 0; g < ng; g++) {
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g];
        if (m == 1) { a.new_width[g] = a.width[g]; out += a.width[g]; continue; }
        wcol[k + 1] = wcol[k] + width[k]; cell[k + 1] = cell[k] + (m + 1) * width[k];
        uint32_t nw = 0;
        for (uint64_t c = wcol[k]; c < wcol[k + 1]; c++) nw += cnt[c] != 0;
        a.new_width[g] = nw; out_off[k] = out; out += m * nw; k++;
    }
    if (a.need) a.need[0] = out;
    if (out > a.cells_capacity) fail(UC_ERR_ARGS, "profile MSA: %llu cell bytes do not fit the capacity %llu", (unsigned long long)out, (unsigned long long)a.cells_capacity);
    if (!out) return;
    if (!a.cells[0] || !a.cells[1]) fail(UC_ERR_ARGS, "profile MSA: cells must not be NULL");
    const uint64_t n_cols = wcol[ns], n_cells = cell[ns];
    if (n_cells) {
        hipStream_t s = nullptr;
        DevBuf<char> tmp;
        DevBuf<uint64_t> d_wcol, d_cell, d_out_off;
        DevBuf<uint32_t> d_cnt, d_flag, d_pos;
        DevBuf<uint8_t> d_i0, d_i1, d_o0, d_o1;
        up(d_wcol, wcol.data(), (size_t)ns + 1); up(d_cell, cell.data(), (size_t)ns + 1); up(d_out_off, out_off.data(), ns);
        up(d_cnt, cnt.data(), n_cols); up(d_i0, c0.data(), n_cells); up(d_i1, c1.data(), n_cells);
        d_flag.reserve_exact(n_cols + 1); d_pos.reserve_exact(n_cols + 1); d_o0.reserve_exact(out); d_o1.reserve_exact(out);
        hipLaunchKernelGGL(mp_flag_kernel, grid_for(n_cols + 1), dim3(256), 0, s, n_cols, (const uint32_t *)d_cnt.p, d_flag.p);
        rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_flag.p, d_pos.p, 0u, (size_t)n_cols + 1, rocprim::plus<uint32_t>(), s); });
        hipLaunchKernelGGL(mp_compact_kernel, grid_for(n_cells), dim3(256), 0, s, n_cells, ns, (const uint64_t *)d_wcol.p, (const uint64_t *)d_cell.p, (const uint64_t *)d_out_off.p,
                           (const uint32_t *)d_flag.p, (const uint32_t *)d_pos.p, (const uint8_t *)d_i0.p, (const uint8_t *)d_i1.p, d_o0.p, d_o1.p);
        UC_HIP(hipGetLastError());
        UC_HIP(hipStreamSynchronize(s));
        UC_HIP(hipMemcpy(a.cells[0], d_o0.p, out, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.cells[1], d_o1.p, out, hipMemcpyDeviceToHost));
    }
    uint64_t o = 0;
    for (uint32_t g = 0; g < ng; g++) {      // the groups of one row keep their cells
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g];
        if (m == 1 && a.width[g])
            for (uint32_t tr = 0; tr < 2; tr++) memcpy(a.cells[tr] + o, a.cells_in[tr] + plan.cell_off[g], a.width[g]);
        o += m * a.new_width[g];
    }
}

}  // namespace uc
