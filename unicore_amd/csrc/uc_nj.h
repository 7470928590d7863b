// uc_nj.h — the built-in tree builder `nj` of `unicore tree` / `unicore gene-tree` (rule UC-N): argument blocks, the checks both
// sides share, the host twins (uc_nj_host.cpp) and the device side (uc_nj.hip, uc_nj_join.hip).  Host and device take the same arrays and give the same outputs:
// integers as integers, fp64 values by their bits.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "uc_common.h"

// UC-N/J rounds every operation on its own: no fused multiply-add may be formed from the expressions below.  The device compiler contracts by
// default, so the pragma is what keeps a * b + c two roundings there; the host build names no -march and so has no FMA instruction to form.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // __umul64hi of the draws
#define UC_NJ_HD __host__ __device__
#else
#define UC_NJ_HD
#endif

namespace uc {

constexpr uint32_t NJ_MIN_ROWS = 2, NJ_MAX_ROWS = 16384;      // D is 2 GiB at the top
constexpr uint32_t NJ_TILE = 64;                               // rows of a pair tile of the count kernel (a tile is NJ_TILE x NJ_TILE pairs)
constexpr uint32_t NJ_CHUNK = 256;                             // columns of both row tiles staged through LDS at a time
constexpr double NJ_CAP = 5.0;                                 // the largest distance (UC-N/D)
constexpr uint32_t NJ_NO_NODE = 0xffffffffu;                   // root_node[2] of a two-leaf tree
constexpr const char *NJ_NO_FALLBACK = "the device side of nj has no CPU fallback (the host twins are separate entry points)";      // use_device's sentence

// ---- what every validate of the host files starts with, and their thread pool
inline void need(const void *p, const char *what) { if (!p) fail(UC_ERR_ARGS, "nj: %s must not be NULL", what); }
inline void check_rows(uint32_t n) {
    if (n < NJ_MIN_ROWS || n > NJ_MAX_ROWS) fail(UC_ERR_ARGS, "nj: %u rows; a tree needs %u .. %u", n, NJ_MIN_ROWS, NJ_MAX_ROWS);
}
// items 0 .. count - 1 over up to `threads` host threads (the caller is one of them); an item goes to the thread that draws its ticket
inline void parallel_for(uint64_t count, uint32_t threads, const std::function<void(uint64_t)> &fn) {
    std::atomic<uint64_t> next{0};
    auto work = [&] { for (uint64_t i; (i = next.fetch_add(1)) < count;) fn(i); };
    const uint32_t nt = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(threads, count));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
}

// ---- UC-N/D: comp / diff of every row pair
struct NjCountArgs {
    uint32_t n;                   // rows
    uint64_t w;                   // columns of every row
    const uint8_t *cells;         // n x w bytes, row-major
    uint32_t threads;             // host twin only (0 = 1)
    uint32_t *comp, *diff;        // n (n - 1) / 2 each: (i, j) with i < j at i n - i (i + 1) / 2 + (j - i - 1), as MsaCenterArgs::scores
};
void nj_counts_validate(const NjCountArgs &a);
void nj_counts_host(const NjCountArgs &a);
void nj_counts_device(int device, const NjCountArgs &a);

// the code of a cell: 0 = uninformative, 1 .. 26 = the letters without X, case folded
UC_NJ_HD inline uint8_t nj_code(uint8_t c) {
    const uint8_t u = (uint8_t)(c | 0x20);
    return (u >= 'a' && u <= 'z' && u != 'x') ? (uint8_t)(u - 'a' + 1) : (uint8_t)0;
}

// model: 0 kimura, 1 p; D is n x n, symmetric, zero on the diagonal.  counts (nullable, 2): pairs without a comparable column, pairs at the cap
void nj_distances_host(const uint32_t *comp, const uint32_t *diff, uint32_t n, uint32_t model, double *D, uint64_t *counts);

// ---- UC-N/J: the joins
struct NjJoinArgs {
    uint32_t n;
    const double *D;              // n x n, not modified
    uint32_t *join_a, *join_b;    // n - 3 (n > 3): the nodes in slot i and slot j of every step
    double *len_a, *len_b;        // n - 3
    uint32_t *root_node;          // 3 (n == 2: two, the third is NJ_NO_NODE)
    double *root_len;             // 3
};
// the arithmetic of a step, written once for both sides; m = the active slots of the step
UC_NJ_HD inline double nj_pos(double v) { return v > 0.0 ? v : 0.0; }
UC_NJ_HD inline double nj_q(uint32_t m, double dij, double ri, double rj) { return (((double)(m - 2) * dij) - ri) - rj; }
UC_NJ_HD inline void nj_branch(uint32_t m, double dij, double ri, double rj, double &li, double &lj) {
    li = 0.5 * dij + (ri - rj) / (2.0 * (double)(m - 2));
    lj = dij - li;
    if (!(li > 0.0)) { li = 0.0; lj = nj_pos(dij); }      // a reduced distance of a matrix that is no tree metric can be negative itself
    else if (!(lj > 0.0)) { lj = 0.0; li = nj_pos(dij); }
}
UC_NJ_HD inline double nj_new(double dik, double djk, double dij) { return 0.5 * ((dik + djk) - dij); }
UC_NJ_HD inline void nj_root3(double dab, double dac, double dbc, double *len) {
    len[0] = nj_pos(0.5 * ((dab + dac) - dbc));
    len[1] = nj_pos(0.5 * ((dab + dbc) - dac));
    len[2] = nj_pos(0.5 * ((dac + dbc) - dab));
}
// finite, >= 0 (no -0.0), symmetric, zero diagonal: the device reads rows as columns
void nj_join_validate(const NjJoinArgs &a);
void nj_join_host(const NjJoinArgs &a);
void nj_join_device(int device, const NjJoinArgs &a);

// ---- the pieces of uc_nj_host.cpp that the bootstrap (uc_nj_boot_host.cpp) builds on
// comp / diff of every row pair over n rows of `words` 64-bit words of codes (eight columns a word, padding 0), spread over `threads`
void nj_count_codes(const uint64_t *code, uint64_t n, uint64_t words, uint32_t threads, uint32_t *comp, uint32_t *diff);
// the Newick line; support (nullable) [n - 3] with n_rep > 0 labels node n + s with the percentage (200 support[s] + n_rep) div (2 n_rep); labels
// (nullable) [n - 3] with n_rep > 0 are written as they are instead (UC-N/T works its percentages out itself) and support is not read
std::string nj_newick_line(const char *const *names, uint32_t n, const uint32_t *ja, const uint32_t *jb, const double *la, const double *lb, const uint32_t *root,
                           const double *rlen, const uint32_t *support, uint32_t n_rep, const uint64_t *labels = nullptr);
// the tree of the alignment itself, as uc_tree_infer computes it (phases 0 .. 3 of st.seconds), and the files uc_tree_infer writes for it
struct NjMainTree {
    std::vector<std::string> names;
    uint32_t n = 0, model = 0;
    uint64_t w = 0;
    int device = -1, threads = 1;
    bool on_host = false, dump = false;
    std::vector<uint8_t> cells;                      // n x w
    std::vector<uint32_t> comp, diff, ja, jb;
    std::vector<double> D, la, lb;
    uint32_t root[3];
    double rlen[3];
};
void nj_main_tree(const char *msa_fasta, const char *model_name, const uc_opts *o, NjMainTree &T, uc_nj_stats &st);
void nj_write_main_tree(const char *out_nwk, const NjMainTree &T, const uint32_t *support, uint32_t n_rep, const uint64_t *labels = nullptr);

// ---- UC-N/B: bootstrap support.  Draws: SplitMix64's finaliser over (seed, replicate, draw); a draw depends on nothing else
constexpr uint32_t NJ_BOOT_MAX_REPS = 100000;
constexpr uint32_t NJ_LDS_ROWS = 128;                          // the largest n whose join loop runs in LDS: n (n | 1) doubles and the vectors fit 160 KiB
constexpr uint64_t NJ_GOLDEN = 0x9E3779B97F4A7C15ull;
UC_NJ_HD inline uint64_t nj_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
UC_NJ_HD inline uint64_t nj_boot_key(uint64_t seed, uint32_t rep) { return nj_mix(seed + NJ_GOLDEN * ((uint64_t)rep + 1)); }
UC_NJ_HD inline uint64_t nj_boot_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
UC_NJ_HD inline uint32_t nj_boot_col(uint64_t key, uint64_t t, uint64_t w) { return (uint32_t)nj_boot_mulhi(nj_mix(key + NJ_GOLDEN * (t + 1)), w); }

struct NjBootCountArgs {
    uint32_t n;
    uint64_t w;
    const uint8_t *cells;         // n x w bytes, row-major
    uint64_t seed;
    uint32_t rep0, n_rep;         // replicates rep0 .. rep0 + n_rep - 1
    uint32_t threads;             // host twin only (0 = 1)
    uint32_t *comp, *diff;        // [n_rep][n (n - 1) / 2]
};
void nj_boot_counts_validate(const NjBootCountArgs &a);
void nj_boot_counts_host(const NjBootCountArgs &a);
void nj_boot_counts_device(int device, const NjBootCountArgs &a);

struct NjJoinBatchArgs {
    uint32_t n, n_rep;
    const double *D;              // [n_rep][n][n], not modified
    uint32_t *join_a, *join_b;    // [n_rep][n - 3]
    double *len_a, *len_b;        // [n_rep][n - 3]
    uint32_t *root_node;          // [n_rep][3]
    double *root_len;             // [n_rep][3]
    uint32_t threads;             // host twin only (0 = 1)
};
void nj_join_batch_validate(const NjJoinBatchArgs &a);
void nj_join_batch_host(const NjJoinBatchArgs &a);
void nj_join_batch_device(int device, const NjJoinBatchArgs &a);

// the bootstrap driver behind uc_tree_infer_boot.  rule == nullptr is that entry point, bit for bit and call for call; a rule (UC-N/T's lives in
// uc_nj_transfer_host.cpp, which uc_nj_boot_host.cpp names nowhere: it links without it) takes the place of the split count: it sees the main tree once,
// then every batch's join records (its time is phase [5]), and at the end gives the count of replicates that hold each split, the labels and the dump's columns
struct NjBootRule {
    virtual ~NjBootRule() = default;
    virtual void begin(const NjMainTree &T, uint32_t n_rep) = 0;                                                     // n > 3 and n_rep > 0
    virtual void batch(const NjMainTree &T, uint32_t nb, const uint32_t *ja, const uint32_t *jb) = 0;               // [nb][n - 3] each
    virtual void finish(uint32_t *support, std::vector<uint64_t> &labels, std::vector<std::string> &tsv_columns) = 0;   // [n - 3] each
};
void nj_tree_infer_boot(const char *msa_fasta, const char *out_nwk, const char *model_name, uint32_t n_rep, uint64_t seed, const uc_opts *o, uc_nj_boot_stats *st_out,
                        NjBootRule *rule);

// ---- UC-N/T: transfer bootstrap support (uc_nj_transfer_host.cpp, uc_nj_transfer.hip)
constexpr uint32_t NJ_T_TILE = 64;                             // splits of a tile of the comparison kernel, both ways
constexpr uint32_t NJ_T_CHUNK = 16;                            // 32-bit words of both tiles staged through LDS at a time
constexpr uint32_t NJ_T_HOST_LEAVES = 128;                     // up to here the driver runs the twin: the device call's allocations and transfers take
                                                               // longer than the twin's comparison (profiles/nj_transfer); the _dev entry point never does
struct NjTransferArgs {
    uint32_t n;
    const uint32_t *join_a, *join_b;          // the main tree, n - 3
    uint32_t n_rep;
    const uint32_t *rep_join_a, *rep_join_b;  // [n_rep][n - 3]
    uint32_t threads;                         // host twin only (0 = 1)
    uint32_t *phi;                            // [n_rep][n - 3]
    uint32_t *light;                          // n - 3
};
// the limits, the pointers and that every tree's records form a tree; fills light.  n <= 3 checks the limits alone
void nj_transfer_validate(const NjTransferArgs &a);
void nj_transfer_host(const NjTransferArgs &a);              // after nj_transfer_validate: a.light is read
void nj_transfer_device(int device, const NjTransferArgs &a);
std::string nj_newick_transfer_line(const char *const *names, uint32_t n, const uint32_t *ja, const uint32_t *jb, const double *la, const double *lb, const uint32_t *root,
                                    const double *rlen, const uint32_t *light, const uint64_t *phi_sum, uint32_t n_rep);

}  // namespace uc
