// uc_msa_progressive.hip — the device side of rule UC-T/G (`unicore tree -a progressive`): profile-profile merges along guide trees.
// A level is every merge whose two children exist; one set of launches serves a batch of a level's tasks of all groups (whole tasks under the byte
// budget, one task at least).  Node cells (letters and `-`, both tracks) stay on the device from the leaves to the root; widths and bounds are all
// that visits the host between levels.  A level's buffer is sized by the sum of (ma + mb) (Wa + Wb); the merged sizes go through one exclusive scan
// per batch (rocPRIM), so the level's nodes lie back to back, each with its merged width as row stride.
//   count    one thread per (task, side column, track, letter): cnt = the side's rows with the letter in the column, u16
//   score    an int32 GEMM per task with K = 2 x 21: cntA (Wa x 42) against Q[j][x] = sum_y cntB[j][y] S[x][y].  A block of 256 threads takes a tile of
//            64 x 64 cells: cntA's and cntB's rows are staged in LDS, Q is formed there, every thread holds 4 x 4 accumulators (plain VALU multiply-adds),
//            applies the floor division by ma mb and writes one signed byte per cell in the DP's own [chunk][step][lane] order
//   DP       one wave (a 64-thread block) per task.  Lane l holds a's column c0 + l of a chunk of 64 and walks along b's columns one anti-diagonal per
//            step: at step t it computes cell (c0 + l, t - l), reading its score byte from the step's 64-byte line.  H, E, F stay in registers, the upper
//            neighbour's H and F arrive by DPP wave_shr:1; the last lane of a chunk leaves H and F in a per-task boundary row that lane 0 of the next
//            chunk reads (two rows, alternating), so widths have no cap.  Borders are 0 (overlap alignment) and H has no floor.  One decision byte per
//            cell (bits 0-1: 1 diagonal / 2 F / 3 E; bit 2: F opened here; bit 3: E opened here), laid out as the scores.  Every lane keeps the best
//            (H, smallest j, smallest i) of its cells on the last row or column; a butterfly takes the same key
//   walk     one thread per task reads the decision bytes backwards from the end cell, writes the runs from the end of the task's run buffer, and the
//            merged width and the merged node's size for the scan
//   render   one wave per merged row: leading overhang, the run list, trailing overhang, both tracks; the other side's columns are `-`
// Vector stores only, no atomics.  Scratch is hipMalloc'ed and freed inside the call, as in uc_msa.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>

#include <rocprim/rocprim.hpp>

#include "uc_engine.h"
#include "uc_msa.h"

namespace uc {

namespace {

constexpr int PG_WAVE = 64;
static_assert(MSA_PROG_CHUNK == PG_WAVE, "one column per lane");
constexpr uint32_t PG_A = MSA_PROFILE_A;
constexpr uint32_t PG_K = 2 * PG_A;
constexpr int PG_TILE = 64;
constexpr const char *PG_NO_FALLBACK = "the device side of the progressive MSA has no CPU fallback (the host twins are separate entry points)";

struct PgTask {
    const uint8_t *a[2], *b[2];      // the sides' cells, m x W row-major
    uint64_t cnt_off;                // 42 (Wa + Wb) counts: a's [track][column][letter], then b's
    uint64_t cell_off;               // into the score and the decision bytes: ceil(Wa / 64) x (Wb + 63) x 64 each
    uint64_t bnd_off;                // 4 Wb ints: two boundary rows of H and F
    uint64_t run_off;                // Wa + Wb words
    uint32_t ma, mb, Wa, Wb;
};

__device__ __forceinline__ uint32_t pg_seg(const uint64_t *off, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

// the loader's mapping (msa_letter_code), by arithmetic
__device__ __forceinline__ uint32_t pg_code(uint32_t c) {
    if (c >= 'a' && c <= 'z') c -= 32;
    if (c < 'A' || c > 'Z') return 20u;
    const uint32_t k = c - 'A';
    // A C D E F G H I K L M N P Q R S T V W Y -> 0 .. 19; B J O U X Z -> 20
    const uint32_t bad = (1u << 1) | (1u << 9) | (1u << 14) | (1u << 20) | (1u << 23) | (1u << 25);
    if (bad >> k & 1u) return 20u;
    return k - __popc(bad & ((1u << k) - 1u));
}

// col_off [n_tasks + 1]: the tasks' side columns (Wa + Wb each) back to back
__global__ void __launch_bounds__(256) pg_count_kernel(uint32_t n_tasks, const PgTask *tasks, const uint64_t *col_off, uint16_t *cnt) {
    const uint64_t n_items = col_off[n_tasks] * PG_K;
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_items; k += (uint64_t)gridDim.x * 256) {
        const uint64_t col = k / PG_K;
        const uint32_t rem = (uint32_t)(k % PG_K), tr = rem / PG_A, x = rem % PG_A;
        const uint32_t t = pg_seg(col_off, n_tasks, col);
        const PgTask T = tasks[t];
        uint32_t c = (uint32_t)(col - col_off[t]);
        const bool side_b = c >= T.Wa;
        if (side_b) c -= T.Wa;
        const uint32_t m = side_b ? T.mb : T.ma, W = side_b ? T.Wb : T.Wa;
        const uint8_t *p = (side_b ? T.b[tr] : T.a[tr]) + c;
        uint32_t n = 0;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t ch = p[(uint64_t)i * W];
            n += ch != (uint32_t)'-' && pg_code(ch) == x;
        }
        cnt[T.cnt_off + (side_b ? (uint64_t)PG_K * T.Wa : 0) + ((uint64_t)tr * W + c) * PG_A + x] = (uint16_t)n;
    }
}

// tile_off [n_tasks + 1]: the tasks' 64 x 64 tiles back to back, a task's tiles row-major over (chunk of a's columns, block of b's columns)
__global__ void __launch_bounds__(256) pg_score_kernel(uint32_t n_tasks, const PgTask *tasks, const uint64_t *tile_off, const uint16_t *cnt, const int8_t *S, int8_t *sc) {
    __shared__ int8_t s_S[2 * PG_A * PG_A];
    __shared__ int32_t s_A[PG_TILE][PG_K + 1];
    __shared__ int32_t s_Q[PG_TILE][PG_K + 1];
    __shared__ uint16_t s_B[PG_TILE][PG_K];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < 2 * PG_A * PG_A; k += 256) s_S[k] = S[k];
    const uint64_t n_tiles = tile_off[n_tasks];
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t t = pg_seg(tile_off, n_tasks, tile);
        const PgTask T = tasks[t];
        const uint32_t Wa = T.Wa, Wb = T.Wb, ntj = (Wb + PG_TILE - 1) / PG_TILE;
        const uint32_t local = (uint32_t)(tile - tile_off[t]), ti = local / ntj, tj = local % ntj;
        const uint32_t i0 = ti * PG_TILE, j0 = tj * PG_TILE, ni = min((uint32_t)PG_TILE, Wa - i0), nj = min((uint32_t)PG_TILE, Wb - j0);
        const uint16_t *cA = cnt + T.cnt_off, *cB = cA + (uint64_t)PG_K * Wa;
        __syncthreads();      // the last tile's reads are over (and s_S is there)
        for (uint32_t e = tid; e < PG_TILE * PG_K; e += 256) {
            const uint32_t r = e / PG_K, k = e % PG_K, tr = k / PG_A, x = k % PG_A;
            s_A[r][k] = r < ni ? (int32_t)cA[((uint64_t)tr * Wa + i0 + r) * PG_A + x] : 0;
            s_B[r][k] = r < nj ? cB[((uint64_t)tr * Wb + j0 + r) * PG_A + x] : (uint16_t)0;
        }
        __syncthreads();
        for (uint32_t e = tid; e < PG_TILE * PG_K; e += 256) {
            const uint32_t r = e / PG_K, k = e % PG_K, tr = k / PG_A, x = k % PG_A;
            const int8_t *Sx = s_S + (tr * PG_A + x) * PG_A;
            int32_t acc = 0;
            for (uint32_t y = 0; y < PG_A; y++) acc += (int32_t)s_B[r][tr * PG_A + y] * (int32_t)Sx[y];
            s_Q[r][k] = acc;
        }
        __syncthreads();
        const uint32_t ty = tid >> 4, tx = tid & 15;
        int32_t acc[4][4] = {};
        for (uint32_t k = 0; k < PG_K; k++) {
            int32_t av[4], qv[4];
            for (int r = 0; r < 4; r++) { av[r] = s_A[ty + 16 * r][k]; qv[r] = s_Q[tx + 16 * r][k]; }
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) acc[r][c] += av[r] * qv[c];
        }
        const int32_t div = (int32_t)(T.ma * T.mb);
        int8_t *out = sc + T.cell_off + (uint64_t)ti * (uint64_t)(Wb + PG_WAVE - 1) * PG_WAVE;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                const uint32_t l = ty + 16 * r, jl = tx + 16 * c;
                if (l < ni && jl < nj) {
                    const int32_t n = acc[r][c], q = n / div;
                    out[(uint64_t)(j0 + jl + l) * PG_WAVE + l] = (int8_t)((n % div != 0 && n < 0) ? q - 1 : q);
                }
            }
    }
}

__device__ __forceinline__ int pg_from_prev_lane(int v, int lane0) { return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false); }      // wave_shr:1

// out[3 task ..]: score, ie, je (1-based: the columns of a / of b up to the end cell)
__global__ void __launch_bounds__(PG_WAVE) pg_dp_kernel(uint32_t n_tasks, const PgTask *tasks, const int8_t *sc, int open, int ext, uint8_t *dec, int32_t *bnd, int32_t *out) {
    const uint32_t task = blockIdx.x;
    if (task >= n_tasks) return;
    const int lane = (int)threadIdx.x;
    const PgTask T = tasks[task];
    const int Wa = (int)T.Wa, Wb = (int)T.Wb;
    if (!Wa || !Wb) {      // no DP: the other side's columns
        if (lane == 0) { out[3 * (uint64_t)task] = 0; out[3 * (uint64_t)task + 1] = 0; out[3 * (uint64_t)task + 2] = 0; }
        return;
    }
    const int8_t *sp0 = sc + T.cell_off;
    uint8_t *d = dec + T.cell_off;
    int best = 0, bi = Wa, bj = 0;      // the corner (Wa, 0); (0, Wb) ties with it and loses by its j
    const int n_chunks = (Wa + PG_WAVE - 1) / PG_WAVE;
    const uint64_t stride = (uint64_t)(Wb + PG_WAVE - 1) * PG_WAVE;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int c0 = ch * PG_WAVE, nl = min(PG_WAVE, Wa - c0);
        __syncthreads();      // the last chunk's boundary row is written
        const int32_t *b_in = bnd + T.bnd_off + (uint64_t)(ch & 1) * 2 * Wb;
        int32_t *b_out = bnd + T.bnd_off + (uint64_t)((ch + 1) & 1) * 2 * Wb;
        const bool has_in = ch > 0, has_out = ch + 1 < n_chunks, mine = lane < nl, last_col = c0 + lane == Wa - 1;
        int H = 0, E = MSA_PROG_NEG, F = MSA_PROG_NEG, diag = 0;
        int nxt_h = 0, nxt_f = MSA_PROG_NEG;
        const int8_t *sp = sp0 + (uint64_t)ch * stride + lane;
        uint8_t *dc = d + (uint64_t)ch * stride + lane;
        const int steps = Wb + PG_WAVE - 1;
        for (int s = 0; s < steps; s++) {
            const int k = s & (PG_WAVE - 1);
            if (k == 0 && has_in) {      // the next 64 boundary cells, one per lane
                const int idx = s + lane;
                nxt_h = idx < Wb ? b_in[idx] : 0; nxt_f = idx < Wb ? b_in[Wb + idx] : MSA_PROG_NEG;
            }
            const int in_h = has_in ? __builtin_amdgcn_readlane(nxt_h, k) : 0;
            const int in_f = has_in ? __builtin_amdgcn_readlane(nxt_f, k) : MSA_PROG_NEG;
            const int upH = pg_from_prev_lane(H, in_h), upF = pg_from_prev_lane(F, in_f);
            const int j = s - lane;
            const bool valid = mine && j >= 0 && j < Wb;
            const int cs = (int)sp[(uint64_t)s * PG_WAVE];      // cells outside the matrix read the buffer's slack and are never used
            int fn = max(upF - ext, upH - open), en = max(E - ext, H - open);
            const int dg = diag + cs;
            int h = max(dg, max(en, fn));
            const uint32_t bits = (h == dg ? 1u : h == fn ? 2u : 3u) | (fn == upH - open ? 4u : 0u) | (en == H - open ? 8u : 0u);
            dc[(uint64_t)s * PG_WAVE] = (uint8_t)bits;
            if (!valid) { h = 0; en = MSA_PROG_NEG; fn = MSA_PROG_NEG; }
            if (valid && (last_col || j == Wb - 1)) {
                const int j1 = j + 1, i1 = c0 + lane + 1;
                if (h > best || (h == best && (j1 < bj || (j1 == bj && i1 < bi)))) { best = h; bi = i1; bj = j1; }
            }
            diag = upH; H = h; E = en; F = fn;
            if (has_out && lane == PG_WAVE - 1 && valid) { b_out[j] = h; b_out[Wb + j] = fn; }
        }
    }
    for (int o = 1; o < PG_WAVE; o <<= 1) {
        const int s2 = __shfl_xor(best, o, PG_WAVE), i2 = __shfl_xor(bi, o, PG_WAVE), j2 = __shfl_xor(bj, o, PG_WAVE);
        if (s2 > best || (s2 == best && (j2 < bj || (j2 == bj && i2 < bi)))) { best = s2; bi = i2; bj = j2; }
    }
    if (lane == 0) { out[3 * (uint64_t)task] = best; out[3 * (uint64_t)task + 1] = bi; out[3 * (uint64_t)task + 2] = bj; }
}

// walk[4 task ..]: is, js, run count, merged width; size[task] = the merged node's bytes per track; the runs end at the end of the task's buffer
__global__ void __launch_bounds__(256) pg_walk_kernel(uint32_t n_tasks, const PgTask *tasks, const int32_t *out, const uint8_t *dec, uint32_t *runbuf, int32_t *walk,
                                                      uint64_t *size) {
    for (uint32_t task = blockIdx.x * 256 + threadIdx.x; task < n_tasks; task += gridDim.x * 256) {
        const PgTask T = tasks[task];
        const uint8_t *d = dec + T.cell_off;
        const uint64_t stride = (uint64_t)(T.Wb + PG_WAVE - 1) * PG_WAVE;
        uint32_t *end = runbuf + T.run_off + T.Wa + T.Wb, *p = end;
        const int ie = out[3 * (uint64_t)task + 1], je = out[3 * (uint64_t)task + 2];
        int i = ie, j = je;
        uint32_t state = 0, op = 3, len = 0, path = 0;
        while (i > 0 && j > 0) {
            const uint32_t c = (uint32_t)(i - 1), l = c & (PG_WAVE - 1);
            const uint32_t b = d[(uint64_t)(c >> 6) * stride + (uint64_t)((uint32_t)(j - 1) + l) * PG_WAVE + l];
            uint32_t o;
            if (state == 0) {
                const uint32_t k = b & 3u;
                if (k != 1) { state = k == 2 ? 1 : 2; continue; }
                o = 0; i--; j--;
            } else if (state == 1) { o = 1; if (b & 4u) state = 0; i--; }
            else { o = 2; if (b & 8u) state = 0; j--; }
            path++;
            if (o == op) len++;
            else { if (len) *--p = len << 2 | op; op = o; len = 1; }
        }
        if (len) *--p = len << 2 | op;
        walk[4 * (uint64_t)task] = i; walk[4 * (uint64_t)task + 1] = j; walk[4 * (uint64_t)task + 2] = (int32_t)(end - p);
        const uint32_t W = (uint32_t)i + (uint32_t)j + path + (T.Wa - (uint32_t)ie) + (T.Wb - (uint32_t)je);
        walk[4 * (uint64_t)task + 3] = (int32_t)W;
        size[task] = (uint64_t)(T.ma + T.mb) * W;
    }
}

// row_off [n_tasks + 1]: the tasks' merged rows (ma + mb each) back to back; o_off [n_tasks]: where a task's node starts in o0 / o1 (the scan of size)
__global__ void __launch_bounds__(PG_WAVE) pg_render_kernel(uint32_t n_tasks, const PgTask *tasks, const uint64_t *row_off, const int32_t *out, const int32_t *walk,
                                                            const uint32_t *runbuf, const uint64_t *o_off, uint8_t *o0, uint8_t *o1) {
    const uint32_t lane = threadIdx.x;
    const uint64_t n_rows = row_off[n_tasks];
    for (uint64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint32_t t = pg_seg(row_off, n_tasks, row);
        const PgTask T = tasks[t];
        uint32_t r = (uint32_t)(row - row_off[t]);
        const uint32_t is = (uint32_t)walk[4 * (uint64_t)t], js = (uint32_t)walk[4 * (uint64_t)t + 1], nr = (uint32_t)walk[4 * (uint64_t)t + 2], W = (uint32_t)walk[4 * (uint64_t)t + 3];
        const uint32_t ie = (uint32_t)out[3 * (uint64_t)t + 1], je = (uint32_t)out[3 * (uint64_t)t + 2];
        const bool side_b = r >= T.ma;
        uint8_t *d0 = o0 + o_off[t] + (uint64_t)r * W, *d1 = o1 + o_off[t] + (uint64_t)r * W;
        if (side_b) r -= T.ma;
        const uint8_t *s0 = side_b ? T.b[0] + (uint64_t)r * T.Wb : T.a[0] + (uint64_t)r * T.Wa, *s1 = side_b ? T.b[1] + (uint64_t)r * T.Wb : T.a[1] + (uint64_t)r * T.Wa;
        uint32_t pos = 0;
        // `len` merged columns from pos: this row's cells from `from` on where its side has them, `-` otherwise
        auto put = [&](uint32_t len, bool has, uint32_t from) {
            for (uint32_t c = lane; c < len; c += PG_WAVE) {
                d0[pos + c] = has ? s0[from + c] : (uint8_t)'-';
                d1[pos + c] = has ? s1[from + c] : (uint8_t)'-';
            }
            pos += len;
        };
        put(is, !side_b, 0);
        put(js, side_b, 0);
        uint32_t x = is, y = js;
        const uint32_t *runs = runbuf + T.run_off + T.Wa + T.Wb - nr;
        for (uint32_t k = 0; k < nr; k++) {
            const uint32_t w = runs[k], len = w >> 2, op = w & 3u;
            put(len, side_b ? op != 1u : op != 2u, side_b ? y : x);
            if (op != 2u) x += len;
            if (op != 1u) y += len;
        }
        put(T.Wa - ie, !side_b, ie);
        put(T.Wb - je, side_b, je);
    }
}

template <typename T>
void up(DevBuf<T> &d, const T *src, size_t n) {
    d.reserve_exact(std::max<size_t>(n, 1));
    if (n) UC_HIP(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
}

struct PgResult { int32_t score, is, js, ie, je; uint32_t n_runs, width; uint64_t off; };      // off: where the node starts in the level's buffer, per track

// the events around the score and the DP kernel of one batch
struct PgEvents {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    explicit PgEvents(bool on) { if (on) for (hipEvent_t &x : e) UC_HIP(hipEventCreate(&x)); }
    ~PgEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    PgEvents(const PgEvents &) = delete;
    PgEvents &operator=(const PgEvents &) = delete;
};

uint64_t task_bytes(uint64_t Wa, uint64_t Wb) { return (Wa + PG_WAVE - 1) / PG_WAVE * (Wb + PG_WAVE - 1) * PG_WAVE; }

// the tasks of one level, in batches under the budget.  tasks hold device pointers; cnt_off .. run_off are filled in here.  The merged nodes go to
// o0 / o1 (one per track; the sum of (ma + mb) (Wa + Wb) bytes each always suffices) back to back in task order.  runs (nullable) receives every task's
// runs.  The budget counts the score and decision bytes, which are all that grows with Wa x Wb; counts, boundary rows and run buffers grow with
// Wa + Wb and stay a small part of it.
struct PgRunner {
    hipStream_t s = nullptr;
    DevBuf<int8_t> d_S, d_sc;
    DevBuf<uint8_t> d_dec;
    DevBuf<uint16_t> d_cnt;
    DevBuf<int32_t> d_bnd, d_out, d_walk;
    DevBuf<uint32_t> d_runs;
    DevBuf<uint64_t> d_col, d_tile, d_row, d_size, d_ooff;
    DevBuf<char> d_tmp;
    DevBuf<PgTask> d_tasks;
    int open = 0, ext = 0;
    uint64_t budget = 0;
    MsaProgStats st{0, 0, 0, 0};
    double score_ms = 0, dp_ms = 0;
    bool timing = false;

    void init(const int8_t *const S[2], int32_t gap_open, int32_t gap_ext) {
        std::vector<int8_t> m(2 * PG_A * PG_A);
        memcpy(m.data(), S[0], PG_A * PG_A); memcpy(m.data() + PG_A * PG_A, S[1], PG_A * PG_A);
        up(d_S, m.data(), m.size());
        open = gap_open; ext = gap_ext; budget = tree_budget_bytes(); timing = getenv("UC_TIMING") != nullptr;
    }

    void level(std::vector<PgTask> &tasks, std::vector<PgResult> &res, std::vector<std::vector<uint32_t>> *runs, uint8_t *o0, uint8_t *o1) {
        const size_t n = tasks.size();
        uint64_t used = 0;      // of o0 / o1, by the batches so far
        res.assign(n, PgResult{0, 0, 0, 0, 0, 0, 0, 0});
        if (runs) runs->assign(n, std::vector<uint32_t>());
        std::vector<uint64_t> col, tile, row;
        std::vector<int32_t> out, walk;
        std::vector<uint32_t> runbuf;
        for (size_t k0 = 0; k0 < n;) {
            size_t k1 = k0;
            uint64_t bytes = 0, cnts = 0, bnds = 0, words = 0;
            col.assign(1, 0); tile.assign(1, 0); row.assign(1, 0);
            for (; k1 < n; k1++) {
                PgTask &T = tasks[k1];
                const uint64_t b = T.Wa && T.Wb ? task_bytes(T.Wa, T.Wb) : 0;
                if (k1 > k0 && (2 * (bytes + b) > budget || k1 - k0 >= (1u << 30))) break;
                T.cnt_off = cnts; T.cell_off = bytes; T.bnd_off = bnds; T.run_off = words;
                bytes += b; cnts += (uint64_t)PG_K * ((uint64_t)T.Wa + T.Wb); bnds += 4 * (uint64_t)T.Wb; words += (uint64_t)T.Wa + T.Wb;
                col.push_back(col.back() + (T.Wa && T.Wb ? (uint64_t)T.Wa + T.Wb : 0));
                tile.push_back(tile.back() + (uint64_t)((T.Wa + PG_TILE - 1) / PG_TILE) * ((T.Wb + PG_TILE - 1) / PG_TILE));
                row.push_back(row.back() + T.ma + T.mb);
                st.n_cells += (uint64_t)T.Wa * T.Wb;
            }
            const uint32_t nt = (uint32_t)(k1 - k0);
            up(d_tasks, tasks.data() + k0, nt); up(d_col, col.data(), col.size()); up(d_tile, tile.data(), tile.size()); up(d_row, row.data(), row.size());
            d_sc.reserve(std::max<uint64_t>(bytes, 1)); d_dec.reserve(std::max<uint64_t>(bytes, 1)); d_cnt.reserve(std::max<uint64_t>(cnts, 1)); d_bnd.reserve(std::max<uint64_t>(bnds, 1));
            d_runs.reserve(std::max<uint64_t>(words, 1)); d_out.reserve((size_t)nt * 3); d_walk.reserve((size_t)nt * 4);
            d_size.reserve(nt); d_ooff.reserve(nt);
            PgEvents ev(timing);
            hipEvent_t e0 = ev.e[0], e1 = ev.e[1], e2 = ev.e[2];
            hipLaunchKernelGGL(pg_count_kernel, grid_for(col.back() * PG_K), dim3(256), 0, s, nt, (const PgTask *)d_tasks.p, (const uint64_t *)d_col.p, d_cnt.p);
            if (timing) UC_HIP(hipEventRecord(e0, s));
            hipLaunchKernelGGL(pg_score_kernel, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tile.back(), 1u << 20))), dim3(256), 0, s, nt, (const PgTask *)d_tasks.p,
                               (const uint64_t *)d_tile.p, (const uint16_t *)d_cnt.p, (const int8_t *)d_S.p, d_sc.p);
            if (timing) UC_HIP(hipEventRecord(e1, s));
            hipLaunchKernelGGL(pg_dp_kernel, dim3(nt), dim3(PG_WAVE), 0, s, nt, (const PgTask *)d_tasks.p, (const int8_t *)d_sc.p, open, ext, d_dec.p, d_bnd.p, d_out.p);
            if (timing) UC_HIP(hipEventRecord(e2, s));
            hipLaunchKernelGGL(pg_walk_kernel, grid_for(nt), dim3(256), 0, s, nt, (const PgTask *)d_tasks.p, (const int32_t *)d_out.p, (const uint8_t *)d_dec.p, d_runs.p, d_walk.p,
                               d_size.p);
            rocprim_call(d_tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_size.p, d_ooff.p, used, (size_t)nt, rocprim::plus<uint64_t>(), s); });
            hipLaunchKernelGGL(pg_render_kernel, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(row.back(), 1u << 20))), dim3(PG_WAVE), 0, s, nt, (const PgTask *)d_tasks.p,
                               (const uint64_t *)d_row.p, (const int32_t *)d_out.p, (const int32_t *)d_walk.p, (const uint32_t *)d_runs.p, (const uint64_t *)d_ooff.p, o0, o1);
            UC_HIP(hipGetLastError());
            UC_HIP(hipStreamSynchronize(s));
            st.n_launches += 5;
            if (timing) {
                float ms = 0;
                UC_HIP(hipEventElapsedTime(&ms, e0, e1)); score_ms += ms;
                UC_HIP(hipEventElapsedTime(&ms, e1, e2)); dp_ms += ms;
            }
            out.resize((size_t)nt * 3); walk.resize((size_t)nt * 4);
            UC_HIP(hipMemcpy(out.data(), d_out.p, (size_t)nt * 12, hipMemcpyDeviceToHost));
            UC_HIP(hipMemcpy(walk.data(), d_walk.p, (size_t)nt * 16, hipMemcpyDeviceToHost));
            if (runs && words) { runbuf.resize(words); UC_HIP(hipMemcpy(runbuf.data(), d_runs.p, words * 4, hipMemcpyDeviceToHost)); }
            for (uint32_t k = 0; k < nt; k++) {
                const PgTask &T = tasks[k0 + k];
                PgResult &R = res[k0 + k];
                R = PgResult{out[3 * (size_t)k], walk[4 * (size_t)k], walk[4 * (size_t)k + 1], out[3 * (size_t)k + 1], out[3 * (size_t)k + 2], (uint32_t)walk[4 * (size_t)k + 2],
                             (uint32_t)walk[4 * (size_t)k + 3], used};
                if (R.n_runs > (uint64_t)T.Wa + T.Wb || R.width > (uint64_t)T.Wa + T.Wb)
                    fail(UC_ERR_GENERIC, "progressive MSA: the walk of a task reports %u runs and width %u for %u + %u columns", R.n_runs, R.width, T.Wa, T.Wb);
                used += (uint64_t)(T.ma + T.mb) * R.width;      // the scan's own sum, from the widths
                if (runs) { const uint64_t end = T.run_off + T.Wa + T.Wb; (*runs)[k0 + k].assign(runbuf.begin() + (end - R.n_runs), runbuf.begin() + end); }
            }
            st.n_merges += nt;
            k0 = k1;
        }
    }

    void report(const char *what) const {
        if (timing) fprintf(stderr, "unicore-cluster[timing]: progressive MSA (%s): %llu merges, %llu cells, %llu launches, score kernel %.3f ms, DP kernel %.3f ms\n", what,
                            (unsigned long long)st.n_merges, (unsigned long long)st.n_cells, (unsigned long long)st.n_launches, score_ms, dp_ms);
    }
};

}  // namespace

void msa_merge_device(int device, const MsaMergeArgs &a, const MsaMergePlan &plan) {
    use_device(device, PG_NO_FALLBACK);
    if (a.need) a.need[0] = a.need[1] = 0;
    const uint32_t n = a.n_tasks;
    if (!n) return;
    const uint64_t na = plan.a_off[n], nb = plan.b_off[n];
    DevBuf<uint8_t> d_a0, d_a1, d_b0, d_b1, d_o;
    up(d_a0, a.a[0], na); up(d_a1, a.a[1], na); up(d_b0, a.b[0], nb); up(d_b1, a.b[1], nb);
    std::vector<uint64_t> o_off((size_t)n + 1, 0);
    for (uint32_t k = 0; k < n; k++) o_off[k + 1] = o_off[k] + (uint64_t)(a.ma[k] + a.mb[k]) * ((uint64_t)a.Wa[k] + a.Wb[k]);
    d_o.reserve_exact(std::max<uint64_t>(2 * o_off[n], 1));
    std::vector<PgTask> tasks(n);
    for (uint32_t k = 0; k < n; k++)
        tasks[k] = PgTask{{d_a0.p + plan.a_off[k], d_a1.p + plan.a_off[k]}, {d_b0.p + plan.b_off[k], d_b1.p + plan.b_off[k]}, 0, 0, 0, 0,
                          a.ma[k], a.mb[k], a.Wa[k], a.Wb[k]};
    PgRunner R;
    R.init(a.S, a.gap_open, a.gap_ext);
    std::vector<PgResult> res;
    std::vector<std::vector<uint32_t>> runs;
    R.level(tasks, res, &runs, d_o.p, d_o.p + o_off[n]);
    R.report("merges");
    uint64_t nr = 0, nc = 0;
    a.run_off[0] = 0;
    for (uint32_t k = 0; k < n; k++) {
        a.score[k] = res[k].score; a.is[k] = res[k].is; a.js[k] = res[k].js; a.ie[k] = res[k].ie; a.je[k] = res[k].je; a.width[k] = res[k].width;
        nr += runs[k].size(); nc += (uint64_t)(a.ma[k] + a.mb[k]) * res[k].width;
        a.run_off[k + 1] = nr;
    }
    if (a.need) { a.need[0] = nr; a.need[1] = nc; }
    if (nr > a.runs_capacity || nc > a.cells_capacity)
        fail(UC_ERR_ARGS, "progressive MSA: %llu runs and %llu cell bytes do not fit the capacities %llu and %llu", (unsigned long long)nr, (unsigned long long)nc,
             (unsigned long long)a.runs_capacity, (unsigned long long)a.cells_capacity);
    if (nr && !a.runs) fail(UC_ERR_ARGS, "progressive MSA: runs must not be NULL");
    if (nc && (!a.cells[0] || !a.cells[1])) fail(UC_ERR_ARGS, "progressive MSA: cells must not be NULL");
    for (uint32_t k = 0; k < n; k++) if (!runs[k].empty()) memcpy(a.runs + a.run_off[k], runs[k].data(), runs[k].size() * 4);
    if (nc) {      // the nodes lie on the device as the call returns them: back to back in task order
        UC_HIP(hipMemcpy(a.cells[0], d_o.p, nc, hipMemcpyDeviceToHost));
        UC_HIP(hipMemcpy(a.cells[1], d_o.p + o_off[n], nc, hipMemcpyDeviceToHost));
    }
}

void msa_progressive_device(int device, const MsaProgressiveArgs &a, const MsaProgressivePlan &plan) {
    use_device(device, PG_NO_FALLBACK);
    if (a.need) a.need[0] = 0;
    if (a.stats) *a.stats = MsaProgStats{0, 0, 0, 0};
    const uint32_t ng = a.n_groups;
    if (!ng) return;
    const uint64_t n_res = a.res_off[plan.n_rows], n_nodes = plan.node_off[ng];
    DevBuf<uint8_t> d_r0, d_r1;
    up(d_r0, a.res[0], n_res); up(d_r1, a.res[1], n_res);
    struct Node { const uint8_t *c[2] = {nullptr, nullptr}; uint32_t W = 0; int32_t buf = -1; };      // buf: the level buffer that holds it
    std::vector<Node> nodes(n_nodes);
    std::vector<std::vector<uint32_t>> order(n_nodes);      // the group-local rows of a node, top to bottom
    for (uint32_t g = 0; g < ng; g++)
        for (uint64_t r = a.grp_off[g]; r < a.grp_off[g + 1]; r++) {
            const uint64_t x = plan.node_off[g] + (r - a.grp_off[g]);
            nodes[x].c[0] = d_r0.p + a.res_off[r]; nodes[x].c[1] = d_r1.p + a.res_off[r]; nodes[x].W = (uint32_t)(a.res_off[r + 1] - a.res_off[r]);
            order[x].assign(1, (uint32_t)(r - a.grp_off[g]));
        }
    PgRunner R;
    R.init(a.S, a.gap_open, a.gap_ext);
    std::vector<std::unique_ptr<DevBuf<uint8_t>>> bufs(plan.levels.size());      // one per level; freed when its last node is consumed
    std::vector<uint64_t> live(plan.levels.size(), 0);
    std::vector<PgTask> tasks;
    std::vector<PgResult> res;
    for (size_t lv = 0; lv < plan.levels.size(); lv++) {
        const std::vector<MsaProgMerge> &L = plan.levels[lv];
        std::vector<uint64_t> o_off(L.size() + 1, 0);
        for (size_t k = 0; k < L.size(); k++) {
            const uint64_t n0 = plan.node_off[L[k].group];
            o_off[k + 1] = o_off[k] + (uint64_t)plan.rows[n0 + L[k].node] * ((uint64_t)nodes[n0 + L[k].a].W + nodes[n0 + L[k].b].W);
        }
        bufs[lv].reset(new DevBuf<uint8_t>());
        bufs[lv]->reserve_exact(std::max<uint64_t>(2 * o_off[L.size()], 1));
        uint8_t *base = bufs[lv]->p;
        tasks.resize(L.size());
        for (size_t k = 0; k < L.size(); k++) {
            const uint64_t n0 = plan.node_off[L[k].group];
            const Node &X = nodes[n0 + L[k].a], &Y = nodes[n0 + L[k].b];
            msa_merge_check_widths(X.W, Y.W, a.gap_open, "a merge of group", L[k].group);      // UC-T/G/M's limits on the widths the two sides have, before the level runs
            tasks[k] = PgTask{{X.c[0], X.c[1]}, {Y.c[0], Y.c[1]}, 0, 0, 0, 0, plan.rows[n0 + L[k].a], plan.rows[n0 + L[k].b], X.W, Y.W};
        }
        R.level(tasks, res, nullptr, base, base + o_off[L.size()]);
        for (size_t k = 0; k < L.size(); k++) {
            const uint64_t n0 = plan.node_off[L[k].group];
            Node &N = nodes[n0 + L[k].node];
            N.c[0] = base + res[k].off; N.c[1] = base + o_off[L.size()] + res[k].off; N.W = res[k].width; N.buf = (int32_t)lv;
            order[n0 + L[k].node] = std::move(order[n0 + L[k].a]);
            order[n0 + L[k].node].insert(order[n0 + L[k].node].end(), order[n0 + L[k].b].begin(), order[n0 + L[k].b].end());
            std::vector<uint32_t>().swap(order[n0 + L[k].b]);
            live[lv]++;
            for (const uint32_t child : {L[k].a, L[k].b}) {
                const int32_t b = nodes[n0 + child].buf;
                if (b >= 0 && --live[b] == 0) bufs[b].reset();
            }
        }
    }
    R.st.n_levels = plan.levels.size();
    R.report("levels");
    uint64_t out = 0;
    for (uint32_t g = 0; g < ng; g++) { const Node &N = nodes[plan.node_off[g + 1] - 1]; a.width[g] = N.W; out += (a.grp_off[g + 1] - a.grp_off[g]) * N.W; }
    if (a.need) a.need[0] = out;
    if (a.stats) *a.stats = R.st;
    if (out > a.cells_capacity) fail(UC_ERR_ARGS, "progressive MSA: %llu cell bytes do not fit the capacity %llu", (unsigned long long)out, (unsigned long long)a.cells_capacity);
    if (out && (!a.cells[0] || !a.cells[1])) fail(UC_ERR_ARGS, "progressive MSA: cells must not be NULL");
    // the roots come back as they lie on the device; their rows go back into file order here
    std::vector<uint8_t> tmp;
    out = 0;
    for (uint32_t g = 0; g < ng; g++) {
        const uint64_t m = a.grp_off[g + 1] - a.grp_off[g], x = plan.node_off[g + 1] - 1;
        const Node &N = nodes[x];
        const uint64_t W = N.W;
        if (W)
            for (uint32_t tr = 0; tr < 2; tr++) {
                tmp.resize(m * W);
                UC_HIP(hipMemcpy(tmp.data(), N.c[tr], m * W, hipMemcpyDeviceToHost));
                for (uint64_t r = 0; r < m; r++) memcpy(a.cells[tr] + out + (uint64_t)order[x][r] * W, tmp.data() + r * W, W);
            }
        out += m * W;
    }
}

}  // namespace uc
