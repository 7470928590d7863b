// uc_msa.hip — the device side of `unicore tree --no-inference` (rule UC-T): everything between the pair scores / backtraces of the
// gapped stage and the bytes of the alignment files.  Every kernel is segmented: one launch serves all groups of the call.
//   centre    one wave per row sums the row's pair scores (64 bit) out of the group's packed triangle; one block per group takes the
//             largest sum, earliest row (UC-T/C)
//   slot max  one thread per aligned row walks its runs and raises ins[slot] to the length of each D run (atomicMax: order-free)
//   scan      one inclusive scan of ins over all groups; col[c] = c + the scan inside the group, width = the value at slot Lc (UC-T/L)
//   render    one wave per row walks the row's runs; once a run's offsets are known the lanes copy its residues, both tracks
//   counts    one thread per column counts the rows whose track-0 cell is not '-'
//   filter    keep flags, their exclusive scan, compaction of the kept columns (UC-T/F)
// Maxima and counts do not depend on the order of execution, so the outputs are the host twins' byte for byte (uc_msa_host.cpp).
// Scratch is hipMalloc'ed and freed inside the call, as in uc_profile.hip: group sizes are tiny next to the DP that feeds this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "uc_engine.h"
#include "uc_msa.h"

namespace uc {

namespace {

constexpr int MSA_WAVE = 64;      // gfx950

// the segment of x: the last g in [0, n) with off[g] <= x (x < off[n]; empty segments are stepped over)
__device__ __forceinline__ uint32_t msa_seg(const uint64_t *off, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;      // first g in [0, n] with off[g] > x, minus one
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

__global__ void __launch_bounds__(256) msa_rowsum_kernel(uint64_t n_rows, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *tri_off, const int32_t *scores,
                                                         long long *sum) {
    const uint32_t lane = threadIdx.x & (MSA_WAVE - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (256 / MSA_WAVE);
    for (uint64_t r = (uint64_t)blockIdx.x * (256 / MSA_WAVE) + threadIdx.x / MSA_WAVE; r < n_rows; r += waves) {
        const uint32_t g = msa_seg(grp_off, n_groups, r);
        const uint64_t m = grp_off[g + 1] - grp_off[g], i = r - grp_off[g];
        const int32_t *tri = scores + tri_off[g];
        long long acc = 0;
        for (uint64_t j = lane; j < m; j += MSA_WAVE) {
            if (j == i) continue;
            const uint64_t a = i < j ? i : j, b = i < j ? j : i;
            acc += tri[a * m - a * (a + 1) / 2 + (b - a - 1)];
        }
        for (int d = MSA_WAVE / 2; d > 0; d >>= 1) acc += __shfl_down(acc, d, MSA_WAVE);
        if (lane == 0) sum[r] = acc;
    }
}
// largest sum, earliest row
__global__ void __launch_bounds__(256) msa_argmax_kernel(uint32_t n_groups, const uint64_t *grp_off, const long long *sum, uint32_t *centre) {
    __shared__ long long s_sum[256];
    __shared__ uint32_t s_row[256];
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint64_t b = grp_off[g];
        const uint32_t m = (uint32_t)(grp_off[g + 1] - b);
        long long best = 0;
        uint32_t row = 0xffffffffu;
        for (uint32_t i = threadIdx.x; i < m; i += 256) {      // ascending rows: a later row replaces only with a larger sum
            const long long v = sum[b + i];
            if (row == 0xffffffffu || v > best) { best = v; row = i; }
        }
        s_sum[threadIdx.x] = best; s_row[threadIdx.x] = row;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if ((int)threadIdx.x < d) {
                const long long v = s_sum[threadIdx.x + d];
                const uint32_t r2 = s_row[threadIdx.x + d], r1 = s_row[threadIdx.x];
                if (r2 != 0xffffffffu && (r1 == 0xffffffffu || v > s_sum[threadIdx.x] || (v == s_sum[threadIdx.x] && r2 < r1))) { s_sum[threadIdx.x] = v; s_row[threadIdx.x] = r2; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) centre[g] = s_row[0];
        __syncthreads();
    }
}

// the validation (msa_star_validate) has walked every aligned row: its slots stay inside 0 .. Lc
__global__ void __launch_bounds__(256) msa_slotmax_kernel(uint64_t n_rows, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, const uint64_t *slot_off,
                                                          const int32_t *qs, const uint64_t *run_off, const uint32_t *runs, const uint8_t *aligned, uint32_t *ins) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256) {
        const uint32_t g = msa_seg(grp_off, n_groups, r);
        if (r - grp_off[g] == centre[g] || !aligned[r]) continue;
        uint32_t *in = ins + slot_off[g];
        uint32_t s = (uint32_t)qs[r];
        for (uint64_t k = run_off[r]; k < run_off[r + 1]; k++) {
            const uint32_t w = runs[k], len = w >> 2;
            if ((w & 3u) == 2u) atomicMax(&in[s], len);
            else s += len;
        }
    }
}
// scan = inclusive scan of ins over all slots of the call; colx[slot s of g] = s + (scan inside g); the value at slot Lc is the width
__global__ void __launch_bounds__(256) msa_col_kernel(uint64_t n_slots, uint32_t n_groups, const uint64_t *slot_off, const uint32_t *scan, uint32_t *colx, uint32_t *width) {
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < n_slots; k += (uint64_t)gridDim.x * 256) {
        const uint32_t g = msa_seg(slot_off, n_groups, k);
        const uint64_t b = slot_off[g];
        const uint32_t base = b ? scan[b - 1] : 0u, s = (uint32_t)(k - b);
        const uint32_t c = s + (scan[k] - base);
        colx[k] = c;
        if (k + 1 == slot_off[g + 1]) width[g] = c;
    }
}
// cells are '-' before; one wave per row
__global__ void __launch_bounds__(256) msa_render_kernel(uint64_t n_rows, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *centre, const uint64_t *slot_off,
                                                         const uint32_t *ins, const uint32_t *colx, const uint32_t *width, const uint64_t *cell_off, const uint64_t *res_off,
                                                         const uint8_t *res0, const uint8_t *res1, const int32_t *qs, const int32_t *ts, const uint64_t *run_off,
                                                         const uint32_t *runs, const uint8_t *aligned, uint8_t *cells0, uint8_t *cells1) {
    const uint32_t lane = threadIdx.x & (MSA_WAVE - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (256 / MSA_WAVE);
    for (uint64_t r = (uint64_t)blockIdx.x * (256 / MSA_WAVE) + threadIdx.x / MSA_WAVE; r < n_rows; r += waves) {
        const uint32_t g = msa_seg(grp_off, n_groups, r);
        const uint64_t i = r - grp_off[g], o = cell_off[g] + i * width[g], ro = res_off[r];
        const uint32_t *cx = colx + slot_off[g], *in = ins + slot_off[g];
        if (i == centre[g]) {
            const uint32_t Lc = (uint32_t)(slot_off[g + 1] - slot_off[g] - 1);
            for (uint32_t c = lane; c < Lc; c += MSA_WAVE) {
                cells0[o + cx[c]] = res0[ro + c];
                if (cells1) cells1[o + cx[c]] = res1[ro + c];
            }
            continue;
        }
        if (!aligned[r]) continue;
        uint32_t s = (uint32_t)qs[r], t = (uint32_t)ts[r];
        for (uint64_t k = run_off[r]; k < run_off[r + 1]; k++) {      // uniform over the wave
            const uint32_t w = runs[k], len = w >> 2, op = w & 3u;
            if (op == 0u) {
                for (uint32_t l = lane; l < len; l += MSA_WAVE) {
                    cells0[o + cx[s + l]] = res0[ro + t + l];
                    if (cells1) cells1[o + cx[s + l]] = res1[ro + t + l];
                }
                s += len; t += len;
            } else if (op == 1u) {
                s += len;
            } else {
                const uint32_t start = cx[s] - in[s];      // len <= ins[s]: left-justified in the slot's block
                for (uint32_t l = lane; l < len; l += MSA_WAVE) {
                    cells0[o + start + l] = res0[ro + t + l];
                    if (cells1) cells1[o + start + l] = res1[ro + t + l];
                }
                t += len;
            }
        }
    }
}
__global__ void __launch_bounds__(256) msa_count_kernel(uint64_t n_cols, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *wcol_off, const uint64_t *cell_off,
                                                        const uint8_t *cells, uint32_t *cnt) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n_cols; x += (uint64_t)gridDim.x * 256) {
        const uint32_t g = msa_seg(wcol_off, n_groups, x);
        const uint64_t W = wcol_off[g + 1] - wcol_off[g], m = grp_off[g + 1] - grp_off[g];
        const uint8_t *p = cells + cell_off[g] + (x - wcol_off[g]);
        uint32_t c = 0;
        for (uint64_t i = 0; i < m; i++) c += p[i * W] != (uint8_t)'-';
        cnt[x] = c;
    }
}
// n_cols + 1 flags, the last one 0: the exclusive scan then ends with the total
__global__ void __launch_bounds__(256) msa_keep_kernel(uint64_t n_cols, uint32_t n_groups, const uint64_t *grp_off, const uint64_t *wcol_off, const uint32_t *cnt,
                                                       uint32_t threshold, uint8_t *keep, uint32_t *flag) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x <= n_cols; x += (uint64_t)gridDim.x * 256) {
        uint32_t f = 0;
        if (x < n_cols) {
            const uint32_t g = msa_seg(wcol_off, n_groups, x);
            const uint64_t m = grp_off[g + 1] - grp_off[g];
            f = (uint64_t)cnt[x] * 100 >= (uint64_t)threshold * m ? 1u : 0u;
            keep[x] = (uint8_t)f;
        }
        flag[x] = f;
    }
}
__global__ void __launch_bounds__(256) msa_fwidth_kernel(uint32_t n_groups, const uint64_t *wcol_off, const uint32_t *pos, uint32_t *fwidth) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * 256) fwidth[g] = pos[wcol_off[g + 1]] - pos[wcol_off[g]];
}
__global__ void __launch_bounds__(256) msa_compact_kernel(uint64_t n_cells, uint32_t n_groups, const uint64_t *wcol_off, const uint64_t *cell_off, const uint64_t *fcell_off,
                                                          const uint32_t *fwidth, const uint8_t *keep, const uint32_t *pos, const uint8_t *cells, uint8_t *fcells) {
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n_cells; x += (uint64_t)gridDim.x * 256) {
        const uint32_t g = msa_seg(cell_off, n_groups, x);
        const uint64_t W = wcol_off[g + 1] - wcol_off[g], rem = x - cell_off[g], i = rem / W, c = rem % W, col = wcol_off[g] + c;
        if (keep[col]) fcells[fcell_off[g] + i * fwidth[g] + (pos[col] - pos[wcol_off[g]])] = cells[x];
    }
}

constexpr const char *MSA_NO_FALLBACK = "the device side of the star MSA has no CPU fallback (the host twins are separate entry points)";

template <typename T>
void up(DevBuf<T> &d, const T *src, size_t n) {
    d.reserve_exact(std::max<size_t>(n, 1));
    if (n) UC_HIP(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
}
dim3 wave_grid(uint64_t n_rows) { return grid_for(n_rows * MSA_WAVE); }

// the counts of track-0 cells per column on the null stream (shared by star and filter)
void launch_count(uint64_t n_cols, uint32_t ng, const uint64_t *d_grp, const uint64_t *d_wcol, const uint64_t *d_cell, const uint8_t *d_cells, uint32_t *d_cnt) {
    hipLaunchKernelGGL(msa_count_kernel, grid_for(n_cols), dim3(256), 0, nullptr, n_cols, ng, d_grp, d_wcol, d_cell, d_cells, d_cnt);
}

}  // namespace

void msa_center_device(int device, const MsaCenterArgs &a, const std::vector<uint64_t> &tri_off) {
    use_device(device, MSA_NO_FALLBACK);
    const uint32_t ng = a.n_groups;
    if (!ng) return;
    const uint64_t n_rows = a.grp_off[ng], n_sc = tri_off[ng];
    DevBuf<uint64_t> d_grp, d_tri;
    DevBuf<int32_t> d_sc;
    DevBuf<long long> d_sum;
    DevBuf<uint32_t> d_centre;
    up(d_grp, a.grp_off, (size_t)ng + 1); up(d_tri, tri_off.data(), (size_t)ng + 1); up(d_sc, a.scores, n_sc);
    d_sum.reserve_exact(n_rows); d_centre.reserve_exact(ng);
    hipLaunchKernelGGL(msa_rowsum_kernel, wave_grid(n_rows), dim3(256), 0, nullptr, n_rows, ng, (const uint64_t *)d_grp.p, (const uint64_t *)d_tri.p,
                       (const int32_t *)d_sc.p, d_sum.p);
    hipLaunchKernelGGL(msa_argmax_kernel, dim3(std::min<uint32_t>(ng, 4096)), dim3(256), 0, nullptr, ng, (const uint64_t *)d_grp.p, (const long long *)d_sum.p, d_centre.p);
    UC_HIP(hipGetLastError());
    UC_HIP(hipDeviceSynchronize());
    UC_HIP(hipMemcpy(a.centre, d_centre.p, (size_t)ng * 4, hipMemcpyDeviceToHost));
}

void msa_star_device(int device, const MsaStarArgs &a, const MsaStarPlan &plan) {
    use_device(device, MSA_NO_FALLBACK);
    const uint32_t ng = a.n_groups;
    if (a.need) a.need[0] = a.need[1] = 0;
    if (!ng) return;
    const uint64_t n_rows = plan.n_rows, n_slots = plan.slot_off[ng], n_res = a.res_off[n_rows], n_runs = a.run_off[n_rows];
    hipStream_t s = nullptr;
    DevBuf<char> tmp;
    DevBuf<uint64_t> d_grp, d_slot, d_resoff, d_runoff, d_wcol, d_cell;
    DevBuf<uint32_t> d_centre, d_runs, d_ins, d_scan, d_colx, d_width, d_cnt;
    DevBuf<int32_t> d_qs, d_ts;
    DevBuf<uint8_t> d_al, d_res0, d_res1, d_c0, d_c1;
    up(d_grp, a.grp_off, (size_t)ng + 1); up(d_slot, plan.slot_off.data(), (size_t)ng + 1); up(d_centre, a.centre, ng);
    up(d_resoff, a.res_off, n_rows + 1); up(d_runoff, a.run_off, n_rows + 1); up(d_runs, a.runs, n_runs);
    up(d_qs, a.qs, n_rows); up(d_ts, a.ts, n_rows); up(d_al, a.aligned, n_rows);
    up(d_res0, a.res[0], n_res);
    if (a.n_tracks == 2) up(d_res1, a.res[1], n_res);

    // ---- layout
    d_ins.reserve_exact(n_slots); d_scan.reserve_exact(n_slots); d_colx.reserve_exact(n_slots); d_width.reserve_exact(ng);
    UC_HIP(hipMemsetAsync(d_ins.p, 0, n_slots * 4, s));
    hipLaunchKernelGGL(msa_slotmax_kernel, grid_for(n_rows), dim3(256), 0, s, n_rows, ng, (const uint64_t *)d_grp.p, (const uint32_t *)d_centre.p, (const uint64_t *)d_slot.p,
                       (const int32_t *)d_qs.p, (const uint64_t *)d_runoff.p, (const uint32_t *)d_runs.p, (const uint8_t *)d_al.p, d_ins.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, d_ins.p, d_scan.p, (size_t)n_slots, rocprim::plus<uint32_t>(), s); });
    hipLaunchKernelGGL(msa_col_kernel, grid_for(n_slots), dim3(256), 0, s, n_slots, ng, (const uint64_t *)d_slot.p, (const uint32_t *)d_scan.p, d_colx.p, d_width.p);
    UC_HIP(hipGetLastError());
    UC_HIP(hipMemcpy(a.width, d_width.p, (size_t)ng * 4, hipMemcpyDeviceToHost));      // the widths size everything that follows
    std::vector<uint64_t> wcol((size_t)ng + 1, 0), cell((size_t)ng + 1, 0);
    for (uint32_t g = 0; g < ng; g++) {
        wcol[g + 1] = wcol[g] + a.width[g];
        cell[g + 1] = cell[g] + (a.grp_off[g + 1] - a.grp_off[g]) * a.width[g];
    }
    const uint64_t n_cols = wcol[ng], n_cells = cell[ng];
    if (a.need) { a.need[0] = n_cols; a.need[1] = n_cells; }
    if (n_cols > plan.max_columns) fail(UC_ERR_GENERIC, "star MSA: %llu columns from a bound of %llu", (unsigned long long)n_cols, (unsigned long long)plan.max_columns);
    if (n_cols > a.cnt_capacity || n_cells > a.cells_capacity)
        fail(UC_ERR_ARGS, "star MSA: %llu columns and %llu cell bytes do not fit the capacities %llu and %llu", (unsigned long long)n_cols, (unsigned long long)n_cells,
             (unsigned long long)a.cnt_capacity, (unsigned long long)a.cells_capacity);
    {   // col: the slots of every group without the last one
        std::vector<uint32_t> colx(n_slots);
        UC_HIP(hipMemcpy(colx.data(), d_colx.p, n_slots * 4, hipMemcpyDeviceToHost));
        uint64_t o = 0;
        for (uint32_t g = 0; g < ng; g++) {
            const uint64_t Lc = plan.slot_off[g + 1] - plan.slot_off[g] - 1;
            if (Lc) memcpy(a.col + o, colx.data() + plan.slot_off[g], Lc * 4);
            o += Lc;
        }
    }
    if (!n_cells && !n_cols) return;

    // ---- rows
    up(d_wcol, wcol.data(), (size_t)ng + 1); up(d_cell, cell.data(), (size_t)ng + 1);
    d_c0.reserve_exact(std::max<uint64_t>(n_cells, 1)); d_cnt.reserve_exact(std::max<uint64_t>(n_cols, 1));
    UC_HIP(hipMemsetAsync(d_c0.p, '-', std::max<uint64_t>(n_cells, 1), s));
    if (a.n_tracks == 2) { d_c1.reserve_exact(std::max<uint64_t>(n_cells, 1)); UC_HIP(hipMemsetAsync(d_c1.p, '-', std::max<uint64_t>(n_cells, 1), s)); }
    hipLaunchKernelGGL(msa_render_kernel, wave_grid(n_rows), dim3(256), 0, s, n_rows, ng, (const uint64_t *)d_grp.p, (const uint32_t *)d_centre.p, (const uint64_t *)d_slot.p,
                       (const uint32_t *)d_ins.p, (const uint32_t *)d_colx.p, (const uint32_t *)d_width.p, (const uint64_t *)d_cell.p, (const uint64_t *)d_resoff.p,
                       (const uint8_t *)d_res0.p, (const uint8_t *)(a.n_tracks == 2 ? d_res1.p : nullptr), (const int32_t *)d_qs.p, (const int32_t *)d_ts.p,
                       (const uint64_t *)d_runoff.p, (const uint32_t *)d_runs.p, (const uint8_t *)d_al.p, d_c0.p, a.n_tracks == 2 ? d_c1.p : (uint8_t *)nullptr);
    if (n_cols) launch_count(n_cols, ng, d_grp.p, d_wcol.p, d_cell.p, d_c0.p, d_cnt.p);
    UC_HIP(hipGetLastError());
    UC_HIP(hipStreamSynchronize(s));
    if (n_cols) UC_HIP(hipMemcpy(a.cnt, d_cnt.p, n_cols * 4, hipMemcpyDeviceToHost));
    if (n_cells) {
        UC_HIP(hipMemcpy(a.cells[0], d_c0.p, n_cells, hipMemcpyDeviceToHost));
        if (a.n_tracks == 2) UC_HIP(hipMemcpy(a.cells[1], d_c1.p, n_cells, hipMemcpyDeviceToHost));
    }
}

void msa_filter_device(int device, const MsaFilterArgs &a, const MsaFilterPlan &plan) {
    use_device(device, MSA_NO_FALLBACK);
    const uint32_t ng = a.n_groups;
    if (!ng) return;
    const uint64_t n_cols = plan.col_off[ng], n_cells = plan.cell_off[ng];
    if (!n_cols) { memset(a.fwidth, 0, (size_t)ng * 4); return; }
    hipStream_t s = nullptr;
    DevBuf<char> tmp;
    DevBuf<uint64_t> d_grp, d_wcol, d_cell, d_fcell;
    DevBuf<uint32_t> d_cnt, d_flag, d_pos, d_fwidth;
    DevBuf<uint8_t> d_cells, d_keep, d_fcells;
    up(d_grp, a.grp_off, (size_t)ng + 1); up(d_wcol, plan.col_off.data(), (size_t)ng + 1); up(d_cell, plan.cell_off.data(), (size_t)ng + 1);
    up(d_cells, a.cells, n_cells);
    d_cnt.reserve_exact(n_cols); d_keep.reserve_exact(n_cols); d_flag.reserve_exact(n_cols + 1); d_pos.reserve_exact(n_cols + 1); d_fwidth.reserve_exact(ng);
    launch_count(n_cols, ng, d_grp.p, d_wcol.p, d_cell.p, d_cells.p, d_cnt.p);
    hipLaunchKernelGGL(msa_keep_kernel, grid_for(n_cols + 1), dim3(256), 0, s, n_cols, ng, (const uint64_t *)d_grp.p, (const uint64_t *)d_wcol.p, (const uint32_t *)d_cnt.p,
                       a.threshold, d_keep.p, d_flag.p);
    rocprim_call(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, d_flag.p, d_pos.p, 0u, (size_t)n_cols + 1, rocprim::plus<uint32_t>(), s); });
    hipLaunchKernelGGL(msa_fwidth_kernel, grid_for(ng), dim3(256), 0, s, ng, (const uint64_t *)d_wcol.p, (const uint32_t *)d_pos.p, d_fwidth.p);
    UC_HIP(hipGetLastError());
    UC_HIP(hipMemcpy(a.fwidth, d_fwidth.p, (size_t)ng * 4, hipMemcpyDeviceToHost));
    UC_HIP(hipMemcpy(a.keep, d_keep.p, n_cols, hipMemcpyDeviceToHost));
    std::vector<uint64_t> fcell((size_t)ng + 1, 0);
    for (uint32_t g = 0; g < ng; g++) {
        if (a.fwidth[g] > a.width[g]) fail(UC_ERR_GENERIC, "MSA filter: group %u keeps %u of %u columns", g, a.fwidth[g], a.width[g]);
        fcell[g + 1] = fcell[g] + (a.grp_off[g + 1] - a.grp_off[g]) * a.fwidth[g];
    }
    const uint64_t n_f = fcell[ng];
    if (!n_f || !n_cells) return;
    up(d_fcell, fcell.data(), (size_t)ng + 1);
    d_fcells.reserve_exact(n_f);
    hipLaunchKernelGGL(msa_compact_kernel, grid_for(n_cells), dim3(256), 0, s, n_cells, ng, (const uint64_t *)d_wcol.p, (const uint64_t *)d_cell.p, (const uint64_t *)d_fcell.p,
                       (const uint32_t *)d_fwidth.p, (const uint8_t *)d_keep.p, (const uint32_t *)d_pos.p, (const uint8_t *)d_cells.p, d_fcells.p);
    UC_HIP(hipGetLastError());
    UC_HIP(hipStreamSynchronize(s));
    UC_HIP(hipMemcpy(a.fcells, d_fcells.p, n_f, hipMemcpyDeviceToHost));
}

}  // namespace uc
