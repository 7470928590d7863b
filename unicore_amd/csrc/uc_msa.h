// uc_msa.h — the star MSA of `unicore tree --no-inference` (rule UC-T): argument blocks, the checks both sides share, the host
// twins (uc_msa_host.cpp) and the device side (uc_msa.hip).  Host and device take the same arrays and give the same outputs.
#pragma once
#include <cstdint>
#include <vector>

#include "uc_common.h"

namespace uc {

constexpr uint32_t MSA_MAX_ROWS = 65535;      // rows of one group (the engine's --max-seqs limit: the centre's hit list holds the group)

// ---- UC-T/C: the centre of every group from its packed upper triangle of pair scores
struct MsaCenterArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;      // n_groups + 1, rows
    const int32_t *scores;        // group g: m (m - 1) / 2 scores, (i, j) with i < j at i m - i (i + 1) / 2 + (j - i - 1), groups back to back
    uint32_t *centre;             // n_groups, group-local row
};
// tri_off [n_groups + 1]: where every group's triangle starts (UC_ERR_ARGS on a malformed grp_off, an empty group, a group beyond MSA_MAX_ROWS)
void msa_center_validate(const MsaCenterArgs &a, std::vector<uint64_t> &tri_off);
void msa_center_host(const MsaCenterArgs &a, const std::vector<uint64_t> &tri_off);
void msa_center_device(int device, const MsaCenterArgs &a, const std::vector<uint64_t> &tri_off);

// ---- UC-T/L + rows: layout and rendering
struct MsaStarArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const uint32_t *centre;
    uint32_t n_tracks;            // 1 or 2; track 0 is the one the column counts are taken from (the amino acids)
    const uint64_t *res_off;      // n_rows + 1 into res[*]
    const uint8_t *res[2];
    const int32_t *qs, *ts;       // per row: start of the box in the centre / in the row
    const uint64_t *run_off;      // n_rows + 1 into runs
    const uint32_t *runs;         // length << 2 | op (0 M, 1 I, 2 D)
    const uint8_t *aligned;       // per row; the centre's own entry is not read
    uint32_t *width;              // n_groups
    uint32_t *col;                // sum of the centre lengths, groups back to back
    uint32_t *cnt;                // sum of the widths
    uint64_t cnt_capacity;
    uint8_t *cells[2];            // group g: m_g x width[g] bytes, row-major, groups back to back
    uint64_t cells_capacity;
    uint64_t *need;               // nullable, 2: columns and cell bytes (per track) the call needs
};
struct MsaStarPlan {
    uint64_t n_rows = 0;
    std::vector<uint64_t> slot_off;      // n_groups + 1: a group has centre length + 1 insert slots
    uint64_t max_columns = 0;            // bound on the sum of the widths: centre lengths + every D run
};
void msa_star_validate(const MsaStarArgs &a, MsaStarPlan &plan);
void msa_star_host(const MsaStarArgs &a, const MsaStarPlan &plan);
void msa_star_device(int device, const MsaStarArgs &a, const MsaStarPlan &plan);

// ---- UC-T/F: the column filter
struct MsaFilterArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const uint32_t *width;
    const uint8_t *cells;         // one track, laid out as MsaStarArgs::cells
    uint32_t threshold;           // 0 .. 100
    uint8_t *keep;                // sum of the widths
    uint32_t *fwidth;             // n_groups
    uint8_t *fcells;              // group g: m_g x fwidth[g]; the capacity of `cells` always suffices
};
struct MsaFilterPlan { std::vector<uint64_t> col_off, cell_off; };      // n_groups + 1 each
void msa_filter_validate(const MsaFilterArgs &a, MsaFilterPlan &plan);
void msa_filter_host(const MsaFilterArgs &a, const MsaFilterPlan &plan);
void msa_filter_device(int device, const MsaFilterArgs &a, const MsaFilterPlan &plan);

// ---- UC-T/P: one refinement round (uc_msa_profile_host.cpp, uc_msa_profile.hip).  Track 0 = amino acids, track 1 = 3Di.
constexpr uint32_t MSA_PROFILE_MAX_ROWS = MSA_MAX_ROWS - 1;      // the device layout adds the virtual centre as one more row of a star call
constexpr uint32_t MSA_PROFILE_CHUNK = 64;                       // columns a wave holds at a time: one per lane
constexpr int32_t MSA_PROFILE_NEG = -(1 << 28);                  // E and F on the borders
constexpr uint32_t MSA_PROFILE_A = 21;

// the loader's mapping (letter_code of uc_options.cpp) without the library behind it: the host twin builds alone
inline uint32_t msa_letter_code(uint8_t c) {
    static const int8_t T[26] = {0, 20, 1, 2, 3, 4, 5, 6, 7, 20, 8, 9, 10, 11, 20, 12, 13, 14, 15, 16, 20, 17, 18, 20, 19, 20};
    if (c >= 'a' && c <= 'z') c -= 32;
    return c >= 'A' && c <= 'Z' ? (uint32_t)T[c - 'A'] : 20u;
}
// floor(n / d) for d > 0
inline int32_t msa_floor_div(int32_t n, int32_t d) { const int32_t q = n / d; return (n % d != 0 && n < 0) ? q - 1 : q; }

struct MsaProfileAlignArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const uint32_t *width;        // n_groups: the current MSA
    const uint8_t *cells[2];      // as MsaStarArgs::cells
    const uint64_t *res_off;      // n_rows + 1
    const uint8_t *res[2];        // the full rows as letters
    const int8_t *S[2];           // [0] SA, [1] S3: 21 x 21, [column letter][row letter]
    int32_t gap_open, gap_ext;
    uint8_t *aligned;             // per row
    int32_t *score, *qs, *ts, *qe, *te;
    uint64_t *run_off;            // n_rows + 1
    uint32_t *runs;
    uint64_t runs_capacity;
    uint64_t *need;               // nullable, 1: the runs of the call
};
struct MsaProfilePlan {
    uint64_t n_rows = 0;
    std::vector<uint64_t> cell_off, col_off;      // n_groups + 1: where a group's cells / columns start
    std::vector<uint32_t> row_group;              // n_rows
    uint64_t n_tasks = 0, n_cells = 0;            // rows of groups with two rows or more that have a residue and a column; width x length over them
};
void msa_profile_align_validate(const MsaProfileAlignArgs &a, MsaProfilePlan &plan);
void msa_profile_align_host(const MsaProfileAlignArgs &a, const MsaProfilePlan &plan, uint32_t threads);      // the same answer for every thread count
void msa_profile_align_device(int device, const MsaProfileAlignArgs &a, const MsaProfilePlan &plan);

struct MsaProfileLayoutArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const uint32_t *width;
    const uint8_t *cells_in[2];   // read for the groups of one row only
    const uint64_t *res_off;
    const uint8_t *res[2];
    const uint8_t *aligned;
    const int32_t *qs, *ts;
    const uint64_t *run_off;
    const uint32_t *runs;
    uint32_t *new_width;
    uint8_t *cells[2];
    uint64_t cells_capacity;      // per track
    uint64_t *need;               // nullable, 1: cell bytes per track
};
struct MsaProfileLayoutPlan {
    uint64_t n_rows = 0;
    std::vector<uint64_t> cell_off;               // of cells_in
    std::vector<uint64_t> bound;                  // n_groups: columns at most, width + every D run (a group of one row: its width)
};
void msa_profile_layout_validate(const MsaProfileLayoutArgs &a, MsaProfileLayoutPlan &plan);
void msa_profile_layout_host(const MsaProfileLayoutArgs &a, const MsaProfileLayoutPlan &plan);
void msa_profile_layout_device(int device, const MsaProfileLayoutArgs &a, const MsaProfileLayoutPlan &plan);

// ---- UC-T/G: the progressive MSA (uc_msa_progressive_host.cpp, uc_msa_progressive.hip).  Track 0 = amino acids, track 1 = 3Di; side a gives the column letter.
constexpr uint32_t MSA_PROG_MAX_ROWS = 8192;                  // ma mb 96 < 2^31 for ma + mb <= 8192
constexpr uint32_t MSA_PROG_CHUNK = 64;                       // a's columns a wave holds at a time: one per lane
constexpr int32_t MSA_PROG_NEG = MSA_PROFILE_NEG;
constexpr uint32_t MSA_PROG_NO_NODE = 0xffffffffu;

struct MsaProgStats { uint64_t n_merges, n_levels, n_launches, n_cells; };

// the guide tree: D (n_groups blocks of m x m doubles) and the merge list (group g: m_g - 1 pairs at 2 (grp_off[g] - g)) from the packed triangles and self scores
struct MsaGuideArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const int32_t *scores;        // as MsaCenterArgs::scores
    const int64_t *self;          // per row
    double *D;                    // group g: m_g x m_g at the sum of the squares before it
    uint32_t *merges;             // 2 (n_rows - n_groups)
};
void msa_guide_validate(const MsaGuideArgs &a, std::vector<uint64_t> &tri_off);
// device < -1: the host join for every group; otherwise the device join (bit-identical) for the groups of MSA_GUIDE_DEV_ROWS rows or more
constexpr uint32_t MSA_GUIDE_DEV_ROWS = 256;
void msa_guide_run(const MsaGuideArgs &a, const std::vector<uint64_t> &tri_off, bool on_device, int device);
void msa_self_scores(uint64_t n_rows, const uint64_t *res_off, const uint8_t *res0, const uint8_t *res1, const int8_t *SA, const int8_t *S3, int64_t *self);

// a batch of independent merges: task k joins a (ma x Wa) and b (mb x Wb); the sides' cells lie task after task, m x W bytes each, row-major
struct MsaMergeArgs {
    uint32_t n_tasks;
    const uint32_t *ma, *mb, *Wa, *Wb;
    const uint8_t *a[2], *b[2];
    const int8_t *S[2];           // [0] SA, [1] S3
    int32_t gap_open, gap_ext;
    int32_t *score, *is, *js, *ie, *je;      // per task
    uint64_t *run_off;            // n_tasks + 1
    uint32_t *runs;
    uint64_t runs_capacity;
    uint32_t *width;              // per task: the merged width
    uint8_t *cells[2];            // task k: (ma + mb) x width[k], tasks back to back
    uint64_t cells_capacity;      // per track
    uint64_t *need;               // nullable, 2: runs and cell bytes per track
};
struct MsaMergePlan {
    std::vector<uint64_t> a_off, b_off;      // n_tasks + 1
    uint64_t n_cells = 0;                    // DP cells
};
void msa_merge_validate(const MsaMergeArgs &a, MsaMergePlan &plan);
void msa_merge_host(const MsaMergeArgs &a, const MsaMergePlan &plan, uint32_t threads);      // the same answer for every thread count
void msa_merge_device(int device, const MsaMergeArgs &a, const MsaMergePlan &plan);
// the limits of one merge, shared by both calls (UC_ERR_ARGS)
void msa_merge_check_widths(uint64_t Wa, uint64_t Wb, int32_t gap_open, const char *what, uint64_t k);

struct MsaProgressiveArgs {
    uint32_t n_groups;
    const uint64_t *grp_off;
    const uint64_t *res_off;      // n_rows + 1
    const uint8_t *res[2];
    const uint32_t *merges;       // as MsaGuideArgs::merges
    const int8_t *S[2];
    int32_t gap_open, gap_ext;
    uint32_t *width;              // n_groups
    uint8_t *cells[2];            // group g: m_g x width[g], rows in file order
    uint64_t cells_capacity;
    uint64_t *need;               // nullable, 1
    MsaProgStats *stats;          // nullable
};
struct MsaProgMerge { uint32_t group, a, b, node; };      // group-local node ids
struct MsaProgressivePlan {
    uint64_t n_rows = 0;
    std::vector<std::vector<MsaProgMerge>> levels;       // every merge whose children exist after the levels before it
    std::vector<uint64_t> node_off;                      // n_groups + 1: group g has 2 m_g - 1 nodes
    std::vector<uint32_t> rows;                          // per node: its row count
};
void msa_progressive_validate(const MsaProgressiveArgs &a, MsaProgressivePlan &plan);
void msa_progressive_host(const MsaProgressiveArgs &a, const MsaProgressivePlan &plan, uint32_t threads);
void msa_progressive_device(int device, const MsaProgressiveArgs &a, const MsaProgressivePlan &plan);

}  // namespace uc
