// grape_tiled_ctl.hpp -- the tiled engine's scalar rules (grape_tiled.hip k_tctl): Taylor degree, Julia's Pade
// histogram slot and the control word of an item from its 1-norm.  No MFMA builtin and no device memory, so the
// same lines compile for the host: tests/c/tiled_ctl_check.cpp checks them there.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace grape_tiled {

// The dense engine's Taylor degree rule (grape_dense.hpp taylor_degree: the lowest of 8 / 12 / 16 / 20 whose
// remainder bound is at most 2^-53 at that 1-norm) as the index `top` of the highest Paterson-Stockmeyer
// block below the initial one: degree = 4 (top + 2).
__host__ __device__ __forceinline__ int taylor_top(double nA) {
    if (nA <= 0.069) return 0;
    if (nA <= 0.335) return 1;
    if (nA <= 0.826) return 2;
    return 3;
}
// Julia's Pade degree for |A|_1 as a histogram slot (m = 3, 5, 7, 9, 13): the stats of grape_expm_batch
__host__ __device__ __forceinline__ int julia_m_index(double nA) {
    if (nA <= 0.015) return 0;
    if (nA <= 0.25) return 1;
    if (nA <= 0.95) return 2;
    if (nA <= 2.1) return 3;
    return 4;
}
// ctl word of an item: Taylor block index | squaring count << 2.  s is the smallest count that brings
// |A / 2^s|_1 to at most 0.95, the end of the solve-free regime: with nA = m 2^e, 0.5 <= m < 1, that is e, or
// e + 1 where m itself is above 0.95 (exact, no search; at most 1 025 for a finite double).  Total: a norm that
// is not finite (an infinite or NaN control) gets s = 0 and the highest degree, so that item's own result comes
// back non-finite and the pass's largest squaring count is left alone.
__host__ __device__ __forceinline__ int make_ctl(double nA) {
    if (!(fabs(nA) <= 1.7976931348623157e308)) return 3;
    int s = 0;
    if (nA > 0.95) {
        int e;
        const double m = frexp(nA, &e);
        s = e + (m > 0.95 ? 1 : 0);
    }
    return taylor_top(ldexp(nA, -s)) | (s << 2);
}

}  // namespace grape_tiled
