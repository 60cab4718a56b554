// grape_prod_inst.hip -- the product-coefficient kernels (grape_prod.hpp) and their launchers for ONE
// compile-time dimension (-DGRAPE_INST_DIM=D), one object per D beside grape_inst.hip's: the launch
// sequences of grape_launch.hpp call the launchers instantiated here.
#include "grape_prod.hpp"

#ifndef GRAPE_INST_DIM
#error "compile with -DGRAPE_INST_DIM=<d>"
#endif

namespace grape_host {
template hipError_t launch_expm_prod<GRAPE_INST_DIM>(bool, const DevProblem &, const DevBatch &,
                                                     const grape::FactorTab &, hipStream_t);
template hipError_t launch_expm_grad_prod<GRAPE_INST_DIM>(const DevProblem &, const DevBatch &,
                                                          const grape::FactorTab &, hipStream_t);
}  // namespace grape_host
