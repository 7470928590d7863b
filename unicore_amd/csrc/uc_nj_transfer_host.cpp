// uc_nj_transfer_host.cpp — transfer bootstrap support for the tree builder `nj` (rule UC-N/T; TBE of Lemoine et al., Nature 2018):
// the checks host and device share, the host twin of the kernels of uc_nj_transfer.hip, the labelled Newick line and the rule that rides on the
// bootstrap driver of uc_nj_boot_host.cpp behind uc_tree_infer_support.  Integers throughout: host, device and the Python reference agree bit for bit.
// Builds without HIP, like uc_nj_host.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "uc_files.h"
#include "uc_nj.h"

namespace uc {

namespace {

// the joins must describe a forest inside the tree: a step joins two nodes that exist before it and hang from no earlier step.  size (nullable)
// [n - 3] receives |L_s|; used and below are the caller's, so that a thousand replicates allocate once
void check_tree(uint32_t n, const uint32_t *ja, const uint32_t *jb, std::vector<uint8_t> &used, std::vector<uint32_t> &below, uint32_t *size) {
    const uint32_t steps = n - 3;
    used.assign((size_t)n + steps, 0);
    below.assign((size_t)n + steps, 1);
    for (uint32_t s = 0; s < steps; s++) {
        for (const uint32_t v : {ja[s], jb[s]}) {
            if (v >= n + s || used[v]) fail(UC_ERR_ARGS, "nj: node %u is joined twice or before it exists", v);
            used[v] = 1;
        }
        below[n + s] = below[ja[s]] + below[jb[s]];
        if (size) size[s] = below[n + s];
    }
}

// rows [n - 3][words] of 64-bit words: row(n + s) = row(a) | row(b), a leaf is its bit
void bit_sets(uint32_t n, const uint32_t *ja, const uint32_t *jb, uint64_t words, uint64_t *rows) {
    const uint32_t steps = n - 3;
    std::fill(rows, rows + (uint64_t)steps * words, 0);
    for (uint32_t s = 0; s < steps; s++) {
        uint64_t *dst = rows + (uint64_t)s * words;
        for (const uint32_t v : {ja[s], jb[s]}) {
            if (v < n) dst[v / 64] |= 1ull << (v % 64);
            else { const uint64_t *src = rows + (uint64_t)(v - n) * words; for (uint64_t x = 0; x < words; x++) dst[x] |= src[x]; }
        }
    }
}

}  // namespace

void nj_transfer_validate(const NjTransferArgs &a) {
    if (a.n < NJ_MIN_ROWS || a.n > NJ_MAX_ROWS) fail(UC_ERR_ARGS, "nj: %u rows; a tree needs %u .. %u", a.n, NJ_MIN_ROWS, NJ_MAX_ROWS);
    if (a.n_rep > NJ_BOOT_MAX_REPS) fail(UC_ERR_ARGS, "nj: %u bootstrap replicates; 0 .. %u", a.n_rep, NJ_BOOT_MAX_REPS);
    if (a.n <= 3) return;
    need(a.join_a, "join_a"); need(a.join_b, "join_b"); need(a.light, "light");
    if (a.n_rep) { need(a.rep_join_a, "the replicates' join_a"); need(a.rep_join_b, "the replicates' join_b"); need(a.phi, "phi"); }
    const uint32_t steps = a.n - 3;
    std::vector<uint8_t> used;
    std::vector<uint32_t> below;
    check_tree(a.n, a.join_a, a.join_b, used, below, a.light);
    for (uint32_t s = 0; s < steps; s++) a.light[s] = std::min(a.light[s], a.n - a.light[s]);      // >= 2: two nodes join, three are left at the root
    for (uint64_t b = 0; b < a.n_rep; b++) check_tree(a.n, a.rep_join_a + b * steps, a.rep_join_b + b * steps, used, below, nullptr);
}

void nj_transfer_host(const NjTransferArgs &a) {
    if (a.n <= 3 || !a.n_rep) return;
    const uint32_t n = a.n, steps = n - 3;
    const uint64_t words = (n + 63) / 64;
    std::vector<uint64_t> main_rows((uint64_t)steps * words);
    bit_sets(n, a.join_a, a.join_b, words, main_rows.data());
    parallel_for(a.n_rep, std::max<uint32_t>(a.threads, 1), [&](uint64_t b) {
        std::vector<uint64_t> rows((uint64_t)steps * words);
        bit_sets(n, a.rep_join_a + b * steps, a.rep_join_b + b * steps, words, rows.data());
        uint32_t *phi = a.phi + b * steps;
        for (uint32_t s = 0; s < steps; s++) {
            const uint64_t *x = main_rows.data() + (uint64_t)s * words;
            uint32_t best = a.light[s] - 1;      // the cap: what the replicate's terminal branches would give
            for (uint32_t r = 0; r < steps; r++) {
                const uint64_t *y = rows.data() + (uint64_t)r * words;
                uint32_t h = 0;
                for (uint64_t k = 0; k < words; k++) h += (uint32_t)__builtin_popcountll(x[k] ^ y[k]);
                best = std::min(best, std::min(h, n - h));
            }
            phi[s] = best;
        }
    });
}

std::string nj_newick_transfer_line(const char *const *names, uint32_t n, const uint32_t *ja, const uint32_t *jb, const double *la, const double *lb, const uint32_t *root,
                                    const double *rlen, const uint32_t *light, const uint64_t *phi_sum, uint32_t n_rep) {
    const uint32_t steps = n > 3 && n <= NJ_MAX_ROWS ? n - 3 : 0;
    if (!steps || !n_rep) return nj_newick_line(names, n, ja, jb, la, lb, root, rlen, nullptr, 0);
    if (n_rep > NJ_BOOT_MAX_REPS) fail(UC_ERR_ARGS, "nj: %u replicates; 0 .. %u", n_rep, NJ_BOOT_MAX_REPS);
    need(light, "light"); need(phi_sum, "phi_sum");
    std::vector<uint64_t> labels(steps);
    for (uint32_t s = 0; s < steps; s++) {
        if (light[s] < 2 || light[s] > n / 2) fail(UC_ERR_ARGS, "nj: a light side of %u leaves at join %u of a tree on %u", light[s], s, n);
        const uint64_t den = (uint64_t)n_rep * (light[s] - 1);
        if (phi_sum[s] > den) fail(UC_ERR_ARGS, "nj: a transfer sum of %llu at join %u; %u replicates at a light side of %u give %llu at most", (unsigned long long)phi_sum[s], s, n_rep,
                                   light[s], (unsigned long long)den);
        labels[s] = (200 * (den - phi_sum[s]) + den) / (2 * den);      // the percentage of 1 - phi_sum / den, rounded half up
    }
    return nj_newick_line(names, n, ja, jb, la, lb, root, rlen, nullptr, n_rep, labels.data());
}

namespace {

// UC-N/T on the bootstrap driver: phi of every batch, summed per join; the zeros are the replicates that hold the split (UC-N/B's support)
struct TransferRule : NjBootRule {
    uint32_t n = 0, steps = 0, n_rep = 0;
    std::vector<uint32_t> light, zeros, phi;
    std::vector<uint64_t> phi_sum;
    void begin(const NjMainTree &T, uint32_t reps) override {
        n = T.n; steps = n - 3; n_rep = reps;
        light.assign(steps, 0); zeros.assign(steps, 0); phi_sum.assign(steps, 0);
    }
    void batch(const NjMainTree &T, uint32_t nb, const uint32_t *ja, const uint32_t *jb) override {
        phi.resize((size_t)nb * steps);
        const NjTransferArgs a{n, T.ja.data(), T.jb.data(), nb, ja, jb, (uint32_t)T.threads, phi.data(), light.data()};
        nj_transfer_validate(a);
        if (T.on_host || n <= NJ_T_HOST_LEAVES) nj_transfer_host(a); else nj_transfer_device(T.device, a);      // the same integers either way
        for (uint32_t b = 0; b < nb; b++)
            for (uint32_t s = 0; s < steps; s++) { const uint32_t v = phi[(size_t)b * steps + s]; phi_sum[s] += v; zeros[s] += v == 0; }
    }
    void finish(uint32_t *support, std::vector<uint64_t> &labels, std::vector<std::string> &tsv_columns) override {
        labels.resize(steps); tsv_columns.resize(steps);
        for (uint32_t s = 0; s < steps; s++) {
            support[s] = zeros[s];
            const uint64_t den = (uint64_t)n_rep * (light[s] - 1);
            if (phi_sum[s] > den) fail(UC_ERR_GENERIC, "nj: a transfer sum of %llu at join %u is above %llu", (unsigned long long)phi_sum[s], s, (unsigned long long)den);
            labels[s] = (200 * (den - phi_sum[s]) + den) / (2 * den);
            tsv_columns[s] = "\t" + std::to_string(light[s]) + "\t" + std::to_string(phi_sum[s]) + "\t" + std::to_string(labels[s]);
        }
    }
};

}  // namespace

}  // namespace uc

using namespace uc;

int uc_nj_transfer(uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a, const uint32_t *rep_join_b, uint32_t threads,
                   uint32_t *phi, uint32_t *light) {
    return guard([&] {
        const NjTransferArgs a{n, join_a, join_b, n_rep, rep_join_a, rep_join_b, threads, phi, light};
        nj_transfer_validate(a);
        nj_transfer_host(a);
    });
}

int uc_nj_transfer_dev(int32_t device, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, uint32_t n_rep, const uint32_t *rep_join_a, const uint32_t *rep_join_b,
                       uint32_t threads, uint32_t *phi, uint32_t *light) {
    return guard([&] {
        const NjTransferArgs a{n, join_a, join_b, n_rep, rep_join_a, rep_join_b, threads, phi, light};
        nj_transfer_validate(a);
        if (n > 3 && n_rep) nj_transfer_device(device, a);
    });
}

int uc_nj_newick_transfer(const char *const *names, uint32_t n, const uint32_t *join_a, const uint32_t *join_b, const double *len_a, const double *len_b,
                          const uint32_t *root_node, const double *root_len, const uint32_t *light, const uint64_t *phi_sum, uint32_t n_rep, char *buf, uint64_t cap,
                          uint64_t *need_out) {
    return guard([&] {
        const std::string s = nj_newick_transfer_line(names, n, join_a, join_b, len_a, len_b, root_node, root_len, light, phi_sum, n_rep);
        if (need_out) *need_out = s.size();
        if (!buf && !cap) return;
        if (!buf || cap < s.size() + 1) fail(UC_ERR_ARGS, "nj: the tree takes %zu bytes and the NUL, the buffer holds %llu", s.size(), (unsigned long long)cap);
        memcpy(buf, s.c_str(), s.size() + 1);
    });
}

int uc_nj_transfer_geometry(uint32_t *tile_splits, uint32_t *chunk_words, uint32_t *host_leaves) {
    return guard([&] {
        if (tile_splits) *tile_splits = NJ_T_TILE;
        if (chunk_words) *chunk_words = NJ_T_CHUNK;
        if (host_leaves) *host_leaves = NJ_T_HOST_LEAVES;
    });
}

int uc_tree_infer_support(const char *msa_fasta, const char *out_nwk, const char *model, uint32_t n_rep, uint64_t seed, uint32_t support_mode, const uc_opts *o,
                          uc_nj_boot_stats *stats_out) {
    return guard([&] {
        if (!msa_fasta || !out_nwk) fail(UC_ERR_ARGS, "tree_infer_support: msa_fasta and out_nwk must not be NULL");
        if (support_mode != UC_NJ_SUPPORT_FBP && support_mode != UC_NJ_SUPPORT_TBE) fail(UC_ERR_ARGS, "nj: unknown support mode %u (0 fbp, 1 tbe)", support_mode);
        TransferRule rule;
        nj_tree_infer_boot(msa_fasta, out_nwk, model, n_rep, seed, o, stats_out, support_mode == UC_NJ_SUPPORT_TBE ? &rule : nullptr);
    });
}
