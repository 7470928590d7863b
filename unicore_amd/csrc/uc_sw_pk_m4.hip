// uc_sw_pk_m4.hip — instantiates the packed 16-bit gapped DP kernel classes for MODE 4 (known-score exact re-run of
// MODE 0, uc_sw_pk_impl.hpp).
#include "uc_sw_pk_impl.hpp"
namespace uc {
int launch_sw_pk_class_m4(int G, int R, const SwArgs &a, uint32_t n_tasks, hipStream_t s, int kmax, uint32_t tcap) {
    return launch_sw_pk_class_mode<4>(G, R, a, n_tasks, s, kmax, tcap);
}
void preload_sw_pk_m4() { preload_sw_pk_mode<4>(); }
}  // namespace uc
