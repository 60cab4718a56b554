// grape_pade_degree.hpp -- the small engine's degree choice (Julia LinearAlgebra.exp!): Pade degree m and squaring
// count s of an item from its 1-norm.  No device memory and no group state, so the same lines compile for the
// host: tests/c/pade_degree_check.cpp checks them there (the pattern of grape_tiled_ctl.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace grape {

// Degree choice of exp! for a 1-norm: returns m, writes s (squarings).  Julia's thresholds and
// s = ceil(log2(nA / 5.4)), unchanged for every finite norm (DBL_MAX: s = 1022).  Total: a norm that is not
// finite (an infinite or NaN control) gets m = 13 and s = 0 -- before, the conversion of ceil(+inf) to int
// saturated and expm_high ran about 2^31 squarings -- so that item's own result comes back non-finite and the
// kernel ends at once.
__host__ __device__ __forceinline__ int pade_degree(double nA, int &s) {
    s = 0;
    if (nA <= 2.1) {
        if (nA > 0.95) return 9;
        if (nA > 0.25) return 7;
        if (nA > 0.015) return 5;
        return 3;
    }
    if (!(nA <= 1.7976931348623157e308)) return 13;  // +inf, NaN
    const double l = log2(nA / 5.4);
    if (l > 0.0) s = (int)ceil(l);
    return 13;
}

}  // namespace grape
