// uc_workflow.h — what a `unicore cluster` run does (spec UC-1 E8): the linear-time pre-step, the cascade rounds on the representatives, the
// merge of the rounds' clusterings and the optional reassignment, on one rank or on one host thread per GPU.  uc_workflow.cpp drives the
// engines; the pieces that touch no device live in uc_workflow_host.cpp and link without the HIP runtime (tests/workflow_host_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "uc_common.h"
#include "uc_db.h"

namespace uc {

// the body of uc_cluster: <db> -> cluster DB <out>; stats_out may be null
void cluster_workflow(const char *db, const char *out, const char *tmp, const uc_opts *o, uc_stats *stats_out);
// workflow observer (uc_set_round_hook): read once per round by rank 0's thread, after the round's align and before its edges are gathered
void set_round_hook(uc_round_hook hook, void *user);

// The convention of uc_opts.num_gpus / device: want 0 = every visible device, 1 = `device` (negative: the current one), N = devices 0..N-1.  More
// ranks than devices are an error (UC_ERR_DEVICE) unless allow_virtual: then several ranks share a device (r % ndev), which only exists to
// exercise the N > 1 paths on a single-GPU box; RCCL refuses two ranks on one device, so such ranks exchange with plain device copies.
struct DevicePlan {
    int world = 1;
    std::vector<int> devices;      // one per rank
    bool virtual_gpus = false;
};
DevicePlan plan_devices(int want, int device, int current_device, int ndev, bool allow_virtual);
// ... with the calling thread's current device and the permission of UC_VIRTUAL_GPUS=1
DevicePlan plan_visible_devices(int want, int device, int ndev);

// the sub-database of the current representatives (createsubdb)
HostDb sub_db(const HostDb &full, const std::vector<uint32_t> &cur);
// mergeclusters: sa is the round's assignment over the positions of cur; the representative of a sequence becomes the representative of its
// representative.  posmap is scratch (one entry per sequence).  Returns the representatives of the next round.
std::vector<uint32_t> merge_round(std::vector<uint32_t> &assign, const std::vector<uint32_t> &cur, const std::vector<uint32_t> &sa, std::vector<uint32_t> &posmap);
// counters add up over the ranks of a run; times are the slowest rank's (the ranks run side by side)
void merge_stats(uc_stats &d, const uc_stats &s);

}  // namespace uc
