// workflow_host_check.cpp — the host pieces of the cluster workflow (unicore_amd/csrc/uc_workflow_host.cpp) on their own: built with
// -fsanitize=address,undefined and run as a child process by tests/test_host.py.  No HIP, no Python; exit status 0 = every check held.
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "uc_workflow.h"

using namespace uc;

static int g_failed = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

typedef std::vector<uint32_t> V;

static uint32_t rnd(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

// assign maps every sequence to a member of cur; sa maps every position of cur to a position that maps to itself
static void check_merge(uint32_t n, const V &cur, const V &sa, uint64_t seed) {
    V pos(n, 0xffffffffu);
    for (uint32_t i = 0; i < cur.size(); i++) pos[cur[i]] = i;
    V assign(n);
    for (uint32_t x = 0; x < n; x++) assign[x] = pos[x] != 0xffffffffu ? x : cur[rnd(seed) % cur.size()];
    // the restatement: assign'[x] = cur[sa[pos[assign[x]]]], next = {cur[i] : sa[i] == i}
    V want(n), want_next;
    for (uint32_t x = 0; x < n; x++) want[x] = cur[sa[pos[assign[x]]]];
    for (uint32_t i = 0; i < cur.size(); i++) if (sa[i] == i) want_next.push_back(cur[i]);
    V posmap(n, 0);
    const V next = merge_round(assign, cur, sa, posmap);
    CHECK(assign == want);
    CHECK(next == want_next);
    for (uint32_t r : next) CHECK(assign[r] == r);                 // every representative maps to itself
    for (uint32_t x = 0; x < n; x++) CHECK(assign[assign[x]] == assign[x]);
}

static void test_merge_round() {
    for (uint32_t n : {1u, 2u, 7u, 1000u}) {
        uint64_t seed = 0x5EED0000u + n;
        V everything(n), subset;
        std::iota(everything.begin(), everything.end(), 0u);
        for (uint32_t x = 0; x < n; x++) if (x == n - 1 || x % 3 == 1) subset.push_back(x);      // strict for n > 1, never empty
        for (const V &cur : {everything, subset}) {
            const uint32_t m = (uint32_t)cur.size();
            V identity(m), to_zero(m, 0), random_sa(m), centres;
            std::iota(identity.begin(), identity.end(), 0u);
            for (uint32_t i = 0; i < m; i++) if (i == m - 1 || rnd(seed) % 4 == 0) centres.push_back(i);      // a random star forest
            for (uint32_t i = 0; i < m; i++) random_sa[i] = centres[rnd(seed) % centres.size()];
            for (uint32_t c : centres) random_sa[c] = c;
            check_merge(n, cur, identity, seed);
            check_merge(n, cur, to_zero, seed);
            check_merge(n, cur, random_sa, seed);
        }
    }
}

static void test_sub_db() {
    HostDb full;
    const uint32_t len[5] = {3, 0, 5, 1, 4};
    full.n = 5;
    full.off.push_back(0);
    for (uint32_t i = 0; i < 5; i++) {
        full.keys.push_back(100 + 7 * i);
        for (uint32_t j = 0; j < len[i]; j++) { full.s3.push_back((uint8_t)(i * 4 + j)); full.sa.push_back((uint8_t)(20 - i - j)); }
        full.off.push_back(full.s3.size());
    }
    for (const V &cur : {V{4, 1, 2}, V{1}, V{}, V{0, 1, 2, 3, 4}}) {
        const HostDb sub = sub_db(full, cur);
        CHECK(sub.n == cur.size());
        CHECK(sub.off.size() == cur.size() + 1 && sub.off[0] == 0);
        CHECK(sub.keys.size() == cur.size());
        CHECK(sub.s3.size() == sub.residues() && sub.sa.size() == sub.residues());
        for (uint32_t i = 0; i < sub.n; i++) {
            CHECK(sub.keys[i] == full.keys[cur[i]]);
            CHECK(sub.len(i) == len[cur[i]]);
            for (uint32_t j = 0; j < sub.len(i); j++) {
                CHECK(sub.s3[sub.off[i] + j] == full.s3[full.off[cur[i]] + j]);
                CHECK(sub.sa[sub.off[i] + j] == full.sa[full.off[cur[i]] + j]);
            }
        }
    }
    CHECK(sub_db(full, {4, 1, 2}).residues() == 9);
    CHECK(sub_db(full, {}).residues() == 0);
}

static void test_plan_devices() {
    DevicePlan d = plan_devices(0, -1, 3, 8, false);
    CHECK(d.world == 8 && !d.virtual_gpus && d.devices == (std::vector<int>{0, 1, 2, 3, 4, 5, 6, 7}));
    d = plan_devices(1, -1, 3, 8, false);
    CHECK(d.world == 1 && !d.virtual_gpus && d.devices == std::vector<int>{3});
    d = plan_devices(1, 5, 3, 8, false);
    CHECK(d.world == 1 && !d.virtual_gpus && d.devices == std::vector<int>{5});
    d = plan_devices(4, -1, 0, 2, true);
    CHECK(d.world == 4 && d.virtual_gpus && d.devices == (std::vector<int>{0, 1, 0, 1}));
    d = plan_devices(2, -1, 0, 2, true);
    CHECK(d.world == 2 && !d.virtual_gpus && d.devices == (std::vector<int>{0, 1}));
    bool threw = false;
    try {
        plan_devices(4, -1, 0, 2, false);
    } catch (const Error &e) {
        threw = true;
        CHECK(e.code == UC_ERR_DEVICE);
        CHECK(std::string(e.what()) == "4 GPUs requested but only 2 visible");
    }
    CHECK(threw);
}

static void test_merge_stats() {
    uc_stats d, s;
    memset(&d, 0, sizeof d);
    memset(&s, 0, sizeof s);
    d.n_index_entries = 1; s.n_index_entries = 10; d.n_sim_kmers = 2; s.n_sim_kmers = 20; d.n_kmer_hits = 3; s.n_kmer_hits = 30;
    d.n_candidates = 4; s.n_candidates = 40; d.n_prefilter_hits = 5; s.n_prefilter_hits = 50; d.n_gapped_alignments = 6; s.n_gapped_alignments = 60;
    d.n_start_alignments = 7; s.n_start_alignments = 70; d.n_pk_reruns = 8; s.n_pk_reruns = 80;
    d.cells_fwd = 9; s.cells_fwd = 90; d.cells_rev = 1; s.cells_rev = 11; d.cells_start = 2; s.cells_start = 12; d.cells_tb = 3; s.cells_tb = 13;
    d.sw_kernel_launches = 4; s.sw_kernel_launches = 14; d.sw_algorithmic_bytes = 5; s.sw_algorithmic_bytes = 15;
    d.n_filtered_hits = 6; s.n_filtered_hits = 16; d.n_sw_runs = 7; s.n_sw_runs = 17; d.cells_run = 8; s.cells_run = 18; d.exchange_bytes = 9; s.exchange_bytes = 19;
    d.n_edges = 123; s.n_edges = 456; d.n_clusters = 5; s.n_clusters = 6;      // rank 0's: not merged
    for (int k = 0; k < UC_NSTAGE; k++) { d.algorithmic_bytes[k] = 100 + k; s.algorithmic_bytes[k] = 1000 + k; d.stage_seconds[k] = k % 2 ? 1.0 : 3.0; s.stage_seconds[k] = 2.0; }
    for (int k = 0; k < UC_NPHASE; k++) { d.phase_seconds[k] = k % 2 ? 0.5 : 2.5; s.phase_seconds[k] = 1.5; }
    d.sw_kernel_ms = 1; s.sw_kernel_ms = 2; d.prefilter_kernel_ms = 4; s.prefilter_kernel_ms = 3; d.exchange_seconds = 0.25; s.exchange_seconds = 0.75;
    for (int k = 0; k < 4; k++) { d.exchange2_seconds[k] = 10 + k; s.exchange2_seconds[k] = 20 + k; }
    merge_stats(d, s);
    CHECK(d.n_index_entries == 11 && d.n_sim_kmers == 22 && d.n_kmer_hits == 33 && d.n_candidates == 44 && d.n_prefilter_hits == 55);
    CHECK(d.n_gapped_alignments == 66 && d.n_start_alignments == 77 && d.n_pk_reruns == 88);
    CHECK(d.cells_fwd == 99 && d.cells_rev == 12 && d.cells_start == 14 && d.cells_tb == 16);
    CHECK(d.sw_kernel_launches == 18 && d.sw_algorithmic_bytes == 20 && d.n_filtered_hits == 22 && d.n_sw_runs == 24 && d.cells_run == 26 && d.exchange_bytes == 28);
    CHECK(d.n_edges == 123 && d.n_clusters == 5);
    for (int k = 0; k < UC_NSTAGE; k++) {
        const bool excluded = k == UC_ST_SETCOVER || k == UC_ST_OUTPUT || k == UC_ST_LOAD;
        CHECK(d.algorithmic_bytes[k] == (excluded ? 100u + k : 1100u + 2 * k));
        CHECK(d.stage_seconds[k] == (k % 2 ? 2.0 : 3.0));
    }
    for (int k = 0; k < UC_NPHASE; k++) CHECK(d.phase_seconds[k] == (k % 2 ? 1.5 : 2.5));
    CHECK(d.sw_kernel_ms == 2 && d.prefilter_kernel_ms == 4 && d.exchange_seconds == 0.75);
    for (int k = 0; k < 4; k++) CHECK(d.exchange2_seconds[k] == 20 + k);      // phase 3: s was the slower rank (1.5 > 0.5), its split is kept
    uc_stats e = d;
    s.phase_seconds[3] = 0.1;
    for (int k = 0; k < 4; k++) s.exchange2_seconds[k] = 30 + k;
    merge_stats(e, s);
    for (int k = 0; k < 4; k++) CHECK(e.exchange2_seconds[k] == 20 + k);      // ... and a faster rank's is not
}

int main() {
    test_merge_round();
    test_sub_db();
    test_plan_devices();
    test_merge_stats();
    if (g_failed) { fprintf(stderr, "workflow_host_check: %d check(s) failed\n", g_failed); return 1; }
    printf("workflow_host_check: ok\n");
    return 0;
}
