// grape_plan_setup.hpp -- host-side pieces of plan construction (grape_engine.hip): the propagator
// variant list, the owner of a plan's device allocations, and the operator / projector tile layouts.
// Host code only: no kernel and no launch.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "grape_kernels.hpp"

namespace grape_setup {

using grape::cd;

// Propagator variants of one step (the closure call sites of UnitaryCalculations.jl:45-95):
//   0 nominal | dx: x_p + eps (np) | dxa: x_add_q + eps (nxa) | ne > 0: dx2: x_p + eps2, then
//   x_add_q + eps2 | per error e: err(eps), err2(eps2), mix_p (x_p + eps2, err eps2), then mix_q
//   (x_add_q + eps2, err eps2)
// nxa: na only if H0 reads x_add, otherwise exp(A(x_add + eps)) == exp(A) bit for bit and the
// reference's difference is 0 (the analysis entry points and the host-table layout keep every x_add
// site).  The eps2 variants only feed the mixed stencils: skipped when ne == 0 (dead work).
// with_grad_variants = false drops dx / dxa too (dense engine without error sources: k_dgrad
// exponentiates its variants in place).  "u" indexes the np + nxa gradient parameters, controls then
// x_add: off_dx + u, off_dx2 + u and off_err + e * err_stride + 2 + u are the variants of parameter u.
struct Variants {
    std::vector<grape::VSpec> vs;
    int off_dx, off_dxa, off_dx2, off_err, err_stride;
};
inline Variants build_variants(int np, int nxa, int ne, double eps, double eps2, bool with_grad_variants) {
    Variants V;
    auto addv = [&](int var, int idx, double delta, int err, double errval) {
        grape::VSpec v;
        v.pert.var = var;
        v.pert.index = idx;
        v.pert.delta = delta;
        v.err = err;
        v.errval = errval;
        V.vs.push_back(v);
    };
    auto params = [&](double delta, int err, double errval) {  // controls, then x_add
        for (int q = 0; q < np; ++q) addv(1, q, delta, err, errval);
        for (int q = 0; q < nxa; ++q) addv(2, q, delta, err, errval);
    };
    addv(-1, 0, 0.0, -1, 0.0);
    V.off_dx = (int)V.vs.size();
    V.off_dxa = V.off_dx + (with_grad_variants ? np : 0);
    if (with_grad_variants) params(eps, -1, 0.0);
    V.off_dx2 = (int)V.vs.size();
    if (ne > 0) params(eps2, -1, 0.0);
    V.off_err = (int)V.vs.size();
    V.err_stride = 2 + np + nxa;
    for (int e = 0; e < ne; ++e) {
        addv(-1, 0, 0.0, e, eps);
        addv(-1, 0, 0.0, e, eps2);
        params(eps2, e, eps2);
    }
    return V;
}

// The one owner of a set of device allocations: alloc() hands out a buffer and remembers it,
// release_all() -- at the latest the destructor, so a local pool is scoped scratch -- frees every one.
// n == 0 allocates one element (a valid pointer for empty tables).
struct DevicePool {
    std::vector<void *> owned;
    DevicePool() = default;
    DevicePool(const DevicePool &) = delete;
    DevicePool &operator=(const DevicePool &) = delete;
    ~DevicePool() { release_all(); }
    template <class T>
    hipError_t alloc(T **out, size_t n) {
        *out = nullptr;
        if (n == 0) n = 1;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(out), n * sizeof(T));
        if (e == hipSuccess) owned.push_back(*out);
        return e;
    }
    void release_all() {
        for (void *b : owned) (void)hipFree(b);
        owned.clear();
    }
};

// Operator basis: column-major interleaved d x d matrices -> row-major cd tiles (row builds) and
// column-major ones (the exp kernels build columns; col may be null).  With sidx ([nsec][S]: the level
// in slot a of sector w, or -1 for padding) the S x S blocks of every sector, [w][o][S][S]; sidx
// null: the whole matrices (nsec = 1, S = D).
inline void to_tiles(const double *ops, int n_ops, int D, const int *sidx, int nsec, int S, cd *row, cd *col) {
    const size_t T = (size_t)D * D, TS = (size_t)S * S;
    for (int w = 0; w < nsec; ++w)
        for (int o = 0; o < n_ops; ++o)
            for (int a = 0; a < S; ++a)
                for (int c = 0; c < S; ++c) {
                    const int gi = sidx ? sidx[(size_t)w * S + a] : a, gj = sidx ? sidx[(size_t)w * S + c] : c;
                    cd v{0.0, 0.0};
                    if (gi >= 0 && gj >= 0) {
                        const double *sv = ops + 2 * ((size_t)o * T + gi + (size_t)gj * D);
                        v = cd{sv[0], sv[1]};
                    }
                    const size_t base = ((size_t)w * n_ops + o) * TS;
                    row[base + (size_t)a * S + c] = v;
                    if (col) col[base + (size_t)c * S + a] = v;
                }
}

// a diagonal projector as the heads' tiles: A = diag(w), B = diag(w != 0)
inline void diag_projector_tiles(const double *W, int D, std::vector<cd> &A, std::vector<cd> &B) {
    A.assign((size_t)D * D, cd{0.0, 0.0});
    B.assign((size_t)D * D, cd{0.0, 0.0});
    for (int i = 0; i < D; ++i) {
        A[(size_t)i * D + i] = cd{W[i], 0.0};
        B[(size_t)i * D + i] = cd{W[i] != 0.0 ? 1.0 : 0.0, 0.0};
    }
}

}  // namespace grape_setup
