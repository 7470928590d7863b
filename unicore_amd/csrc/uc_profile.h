// uc_profile.h — the counting core of `unicore profile` (rule UC-P): one argument block, a host counter and a device counter
// that give the same outputs.
#pragma once
#include <cstdint>

#include "uc_common.h"

namespace uc {

constexpr uint32_t PROFILE_ID_LIMIT = 1u << 24;      // groups, genes, species: the project's sequence limit; the sort key is group << 24 | species

struct ProfileArgs {
    uint64_t n_rows;
    const uint32_t *group, *gene;
    uint32_t n_groups, n_genes;
    const uint64_t *sp_off;
    const uint32_t *sp;
    uint32_t n_species, threshold;
    uint32_t *single, *multiple;
    uint8_t *core;
    uint64_t *core_off;
    uint32_t *core_gene, *core_species, *full;
};

// the limits and the shape of the inputs (UC_ERR_ARGS); returns the number of (row, species) pairs
uint64_t profile_validate(const ProfileArgs &a);
void profile_count_host(const ProfileArgs &a, uint64_t n_pairs);
// uc_profile.hip; device = -1: the current one.  ms (nullable, 6): expand, sort, runs, groups, emit, total of the device work (HIP events)
void profile_count_device(int device, const ProfileArgs &a, uint64_t n_pairs, float *ms);

}  // namespace uc
