// uc_workflow_host.cpp — the pieces of the cluster workflow (uc_workflow.h) that are plain host code: no HIP call, so that they can be built and
// run under a sanitizer on their own.
#include <algorithm>
#include <cstring>

#include "uc_workflow.h"

namespace uc {

DevicePlan plan_devices(int want, int device, int current_device, int ndev, bool allow_virtual) {
    DevicePlan d;
    d.world = want == 0 ? ndev : want;
    if (d.world == 1) {
        d.devices.push_back(device < 0 ? current_device : device);
        return d;
    }
    if (d.world > ndev) {
        if (!allow_virtual) fail(UC_ERR_DEVICE, "%d GPUs requested but only %d visible", d.world, ndev);
        d.virtual_gpus = true;
    }
    for (int r = 0; r < d.world; r++) d.devices.push_back(r % ndev);
    return d;
}

HostDb sub_db(const HostDb &full, const std::vector<uint32_t> &cur) {
    HostDb sub;
    sub.n = (uint32_t)cur.size();
    sub.off.resize((size_t)sub.n + 1);
    uint64_t tot = 0;
    for (uint32_t i = 0; i < sub.n; i++) { sub.off[i] = tot; tot += full.len(cur[i]); }
    sub.off[sub.n] = tot;
    sub.s3.resize(tot); sub.sa.resize(tot); sub.keys.resize(sub.n);
    for (uint32_t i = 0; i < sub.n; i++) {
        if (full.len(cur[i])) {
            memcpy(sub.s3.data() + sub.off[i], full.s3.data() + full.off[cur[i]], full.len(cur[i]));
            memcpy(sub.sa.data() + sub.off[i], full.sa.data() + full.off[cur[i]], full.len(cur[i]));
        }
        sub.keys[i] = full.keys[cur[i]];
    }
    return sub;
}

std::vector<uint32_t> merge_round(std::vector<uint32_t> &assign, const std::vector<uint32_t> &cur, const std::vector<uint32_t> &sa, std::vector<uint32_t> &posmap) {
    for (uint32_t i = 0; i < cur.size(); i++) posmap[cur[i]] = i;
    for (uint32_t &a : assign) a = cur[sa[posmap[a]]];
    std::vector<uint32_t> next;
    for (uint32_t i = 0; i < cur.size(); i++) if (sa[i] == i) next.push_back(cur[i]);
    return next;
}

void merge_stats(uc_stats &d, const uc_stats &s) {
    d.n_index_entries += s.n_index_entries; d.n_sim_kmers += s.n_sim_kmers; d.n_kmer_hits += s.n_kmer_hits;
    d.n_candidates += s.n_candidates; d.n_prefilter_hits += s.n_prefilter_hits; d.n_gapped_alignments += s.n_gapped_alignments;
    d.n_start_alignments += s.n_start_alignments; d.n_pk_reruns += s.n_pk_reruns;
    d.cells_fwd += s.cells_fwd; d.cells_rev += s.cells_rev; d.cells_start += s.cells_start; d.cells_tb += s.cells_tb;
    d.sw_kernel_launches += s.sw_kernel_launches; d.sw_algorithmic_bytes += s.sw_algorithmic_bytes;
    d.n_filtered_hits += s.n_filtered_hits; d.n_sw_runs += s.n_sw_runs; d.cells_run += s.cells_run; d.exchange_bytes += s.exchange_bytes;
    for (int k = 0; k < UC_NSTAGE; k++) {
        if (k != UC_ST_SETCOVER && k != UC_ST_OUTPUT && k != UC_ST_LOAD) d.algorithmic_bytes[k] += s.algorithmic_bytes[k];
        d.stage_seconds[k] = std::max(d.stage_seconds[k], s.stage_seconds[k]);
    }
    d.sw_kernel_ms = std::max(d.sw_kernel_ms, s.sw_kernel_ms);
    d.prefilter_kernel_ms = std::max(d.prefilter_kernel_ms, s.prefilter_kernel_ms);
    d.exchange_seconds = std::max(d.exchange_seconds, s.exchange_seconds);
    if (s.phase_seconds[3] > d.phase_seconds[3]) memcpy(d.exchange2_seconds, s.exchange2_seconds, sizeof d.exchange2_seconds);   // the split of the slowest rank's phase 3
    for (int k = 0; k < UC_NPHASE; k++) d.phase_seconds[k] = std::max(d.phase_seconds[k], s.phase_seconds[k]);
}

}  // namespace uc
