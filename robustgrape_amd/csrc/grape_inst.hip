// grape_inst.hip -- the small-d engine's kernels and launch sequences for ONE
// compile-time dimension (-DGRAPE_INST_DIM=D); the build compiles one object per
// D in parallel.  The explicit instantiations below are the only definitions of the launch sequences: the
// host units see their declarations (grape_launch_api.hpp) and link against these.
#include "grape_launch.hpp"

#ifndef GRAPE_INST_DIM
#error "compile with -DGRAPE_INST_DIM=<d>"
#endif

namespace grape_host {
template hipError_t launch_pipeline<GRAPE_INST_DIM>(const DevProblem &, const DevBatch &, const grape::FactorTab &,
                                                    hipStream_t, const KMark &);
template hipError_t launch_sector_stage<GRAPE_INST_DIM>(int, const DevProblem &, const DevBatch &,
                                                        const grape::FactorTab &, hipStream_t, const KMark &);
template hipError_t launch_sector_reduce<GRAPE_INST_DIM>(const DevProblem &, const DevBatch &, const grape::SecParts &,
                                                         int, hipStream_t, const KMark &);
template hipError_t launch_expm_raw<GRAPE_INST_DIM>(const cd *, cd *, int, int *, int *, int *, int *, hipStream_t);
template hipError_t set_lds_limits<GRAPE_INST_DIM>();
template hipError_t launch_expm_variants<GRAPE_INST_DIM>(const DevProblem &, const DevBatch &, const grape::FactorTab &,
                                                         hipStream_t);
template hipError_t launch_expm_table<GRAPE_INST_DIM>(const DevProblem &, const DevBatch &, hipStream_t);
#if GRAPE_INST_DIM == 3 || GRAPE_INST_DIM == 4
// the pair scans of the Rydberg layout (class A of 4 or 3 levels beside the 2-level class), in the unit of D0
#define GRAPE_SCAN_PAIR(W)                                                                                      \
    template hipError_t launch_scan_pair<GRAPE_INST_DIM, 2, W>(const DevProblem &, const DevBatch &, const DevProblem &, \
                                                               const DevBatch &, hipStream_t);
GRAPE_SCAN_PAIR(kScanLatency)
GRAPE_SCAN_PAIR(kScanTiny)
#endif
}  // namespace grape_host
