// grape_analysis.hip -- the single-evaluation analysis entry points of the C ABI and their workspace (ud_*):
// unitary derivatives, interaction-picture error operators, expectation values, and grape_expm_batch*.
// (The general-H0 call path, grape_call.hip enqueue_general, runs on the same workspace.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "grape_plan.hpp"

using namespace grape_eng;

namespace grape_eng {

// every closure call site of UnitaryCalculations.jl:45-95 as a propagator variant, in the
// layout of grape_unitary::UProblem (= the host-table layout of grape_fidelity_grad_tables
// with every x_add site present), and the assembly's slots per step
static grape_setup::Variants ud_variants(const DevProblem &P0) {
    return grape_setup::build_variants(P0.np, P0.na, P0.ne, P0.eps, P0.eps2, true);
}
static int ud_nslots(const DevProblem &P0) { return P0.np + P0.na + P0.ne + P0.ne * (P0.np + P0.na); }

// workspace of the single-evaluation analysis entry points (unitary derivatives,
// interaction-picture error operators, expectation values), allocated on first use
int ud_alloc(grape_plan *p) {
    if (p->ud_vs) return GRAPE_OK;
    const DevProblem &P = p->P;
    const size_t T = (size_t)P.D * P.D, Nt = P.Nt, np = P.np, na = P.na, ne = P.ne;
    const size_t nv = ud_variants(P).vs.size(), nslots = ud_nslots(P);
    const size_t nout = T * (np * Nt + na + ne + np * Nt * ne + na * ne + Nt * ne);
    bool ok = p->mem.alloc(&p->ud_vs, nv) == hipSuccess && p->mem.alloc(&p->ud_E, Nt * nv * T) == hipSuccess &&
                    p->mem.alloc(&p->ud_ovf, Nt * nv) == hipSuccess && p->mem.alloc(&p->ud_C, Nt * T) == hipSuccess &&
                    p->mem.alloc(&p->ud_V, Nt * nslots * T) == hipSuccess &&
                    p->mem.alloc(&p->ud_S, Nt * std::max<size_t>(ne, 1) * T) == hipSuccess && p->mem.alloc(&p->ud_out, nout) == hipSuccess;
    if (ok && P.D > grape_unitary::kMaxD) ok = p->mem.alloc(&p->ud_gscr, grape_unitary::scratch_elems(P.D)) == hipSuccess;
    if (ok && (p->dense || P.D > GRAPE_MAX_SMALL_DIM))
        ok = p->mem.alloc(&p->ud_Eimg, Nt * nv * grape_dense::kImgDoubles) == hipSuccess;
    if (ok && p->tables && P.D > GRAPE_MAX_SMALL_DIM)
        ok = p->mem.alloc(&p->ud_Aimg, Nt * nv * grape_dense::kImgDoubles) == hipSuccess;
    return ok ? GRAPE_OK : fail(GRAPE_ERR_ALLOC, "device allocation failed (single-evaluation workspace)");
}

// Propagator table E[k][v] of ONE x into the ud workspace, for the variant list already in
// ud_vs (nv entries): from the operator basis (d_Htab == nullptr), or -- closure fallback --
// from the device copy of the host-evaluated H table [Nt][nv][D][D] column-major, whose
// variant layout is ud_vs's.  d_x: the evaluation's controls on the device.
int ud_propagators_dev(grape_plan *p, const double *d_x, int nv, const cd *d_Htab) {
    const DevProblem &P0 = p->P;
    hipStream_t st = p->stream;
    HIPCHECK(hipMemsetAsync(p->d_ctrl, 0, 2 * sizeof(int), st));
    DevProblem Pu = P0;
    Pu.nv = nv;
    Pu.vs = p->ud_vs;
    DevBatch Bu{};
    Bu.nb = 1;
    Bu.x = d_x;
    Bu.E = p->ud_E;
    Bu.overflow = p->ud_ovf;
    Bu.overflow_count = p->d_ctrl;
    Bu.status = p->d_ctrl + 2;
    if (p->dense) {  // 12 < d <= 64: k_dexp over the variant list, images -> row-major tiles
        grape_dense::DenseProblem DPu = p->DP;
        DPu.P.nv = nv;
        DPu.P.vs = p->ud_vs;
        grape_dense::DenseBatch DB{};
        DB.nb = 1;
        DB.x = d_x;
        DB.E = p->ud_Eimg;
        DB.status = p->d_ctrl + 2;
        HIPCHECK(grape_dense::launch_variant_table(DPu, DB, p->ud_E, st, p->pivot));
    } else if (d_Htab && P0.D > GRAPE_MAX_SMALL_DIM) {  // closures above the small engine
        HIPCHECK(grape_dense::launch_table_variants(d_Htab, P0.D, P0.Nt * nv, P0.dt, p->ud_Aimg, p->ud_Eimg, p->ud_E,
                                                   p->d_ctrl + 2, st, p->pivot));
    } else if (d_Htab) {
        Bu.Htab = d_Htab;
        HIPCHECK(dispatch_expm_table(P0.D, Pu, Bu, st));
    } else {
        HIPCHECK(dispatch_expm_variants(P0.D, Pu, Bu, p->FT, st));
    }
    return GRAPE_OK;
}

// The same for a host x (and host H table): uploads the variant list, x and the table first.
static int ud_propagators(grape_plan *p, const double *x, const std::vector<grape::VSpec> &vs, const double *Htab) {
    const DevProblem &P0 = p->P;
    const int nv = (int)vs.size();
    hipStream_t st = p->stream;
    const size_t T = (size_t)P0.D * P0.D;
    p->ud_vs_host = vs;  // the async copy reads this plan-owned copy
    HIPCHECK(hipMemcpyAsync(p->ud_vs, p->ud_vs_host.data(), vs.size() * sizeof(grape::VSpec), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(p->d_x, x, (size_t)P0.nx * sizeof(double), hipMemcpyHostToDevice, st));
    if (Htab) HIPCHECK(hipMemcpyAsync(p->d_Htab, Htab, (size_t)P0.Nt * nv * T * sizeof(cd), hipMemcpyHostToDevice, st));
    return ud_propagators_dev(p, p->d_x, nv, Htab ? p->d_Htab : nullptr);
}

// nominal propagators E_k and the chain C_k of one x into the ud workspace (H0tab: the
// closure fallback's host-evaluated H0(k, x_k, x_add), [Nt][D][D] column-major)
static int ud_chain(grape_plan *p, const double *x, const double *H0tab) {
    const DevProblem &P0 = p->P;
    grape::VSpec nominal{};
    nominal.pert.var = -1;
    nominal.err = -1;
    if (int rc = ud_propagators(p, x, std::vector<grape::VSpec>{nominal}, H0tab)) return rc;
    grape_unitary::UProblem UP{};
    UP.D = P0.D;
    UP.Nt = P0.Nt;
    UP.nv = 1;
    UP.gscr = p->ud_gscr;
    HIPCHECK(grape_unitary::launch_chain(UP, p->ud_E, p->ud_C, p->stream));
    return GRAPE_OK;
}

// interaction-picture error operators of one x into ud_out (d, d, Nt, ne) column-major;
// closure fallback when H0tab / Oerr are given (host arrays)
static int ud_interaction(grape_plan *p, const double *x, const double *H0tab, const double *Oerr) {
    if (int rc = ud_alloc(p)) return rc;
    if (int rc = ud_chain(p, x, H0tab)) return rc;
    const cd *Ci = nullptr;
    if (p->general_h0) {  // cum_evo_inv = inv(cum_evo) (UnitaryCalculations.jl:194)
        grape_unitary::UProblem UP{};
        UP.D = p->P.D;
        UP.Nt = p->P.Nt;
        UP.gscr = p->ud_gscr;
        HIPCHECK(grape_unitary::launch_inverse(UP, p->ud_C, p->ud_Ci, p->d_ctrl + 2, p->stream));
        Ci = p->ud_Ci;
    }
    if (Oerr) {
        cd *dO = p->ud_V;  // Nt * nslots >= Nt * ne tiles
        const size_t n = (size_t)p->P.D * p->P.D * p->P.Nt * p->P.ne;
        HIPCHECK(hipMemcpyAsync(dO, Oerr, n * sizeof(cd), hipMemcpyHostToDevice, p->stream));
        HIPCHECK(grape_unitary::launch_interaction_table(p->P, dO, p->ud_C, Ci, p->ud_out, p->ud_gscr, p->stream));
    } else {
        HIPCHECK(grape_unitary::launch_interaction(p->P, p->d_x, p->ud_C, Ci, p->ud_out, p->ud_gscr, p->FT.err, p->stream));
    }
    return GRAPE_OK;
}

static int analysis_check(grape_plan *p, bool tables_call, const char *what) {
    if (p->tiled)  // (no dense kernel at the wrong size: the analysis kernels stop at GRAPE_MAX_DENSE_DIM)
        return fail(GRAPE_ERR_UNSUPPORTED, std::string(what) + ": not served by the tiled engine (ndim > GRAPE_MAX_DENSE_DIM)");
    if (p->tables && !tables_call)
        return fail(GRAPE_ERR_INVALID, std::string(what) + ": host-table plan: use the _tables entry point");
    if (!p->tables && tables_call)
        return fail(GRAPE_ERR_INVALID, std::string(what) + ": plan was not created with GRAPE_DESC_HOST_TABLES");
    return GRAPE_OK;
}

static int interaction_to(grape_plan *p, const double *x, const double *H0tab, const double *Oerr, double *O,
                          hipMemcpyKind kind) {
    if (p->P.ne == 0) return GRAPE_OK;
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = ud_interaction(p, x, H0tab, Oerr)) return rc;
    const size_t n = (size_t)p->P.D * p->P.D * p->P.Nt * p->P.ne;
    HIPCHECK(hipMemcpyAsync(O, p->ud_out, n * sizeof(cd), kind, p->stream));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return grape_plan_synchronize(p);
}

}  // namespace grape_eng

extern "C" {

int grape_interaction_error_operators(grape_plan *p, const double *x, double *O) {
    if (!p || !x || !O) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, false, "interaction error operators")) return rc;
    return interaction_to(p, x, nullptr, nullptr, O, hipMemcpyDeviceToHost);
}

int grape_interaction_error_operators_device(grape_plan *p, const double *x, double *d_O) {
    if (!p || !x || !d_O) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, false, "interaction error operators")) return rc;
    return interaction_to(p, x, nullptr, nullptr, d_O, hipMemcpyDeviceToDevice);
}

int grape_interaction_error_operators_tables(grape_plan *p, const double *x, const double *H0, const double *Oerr,
                                             double *O, int O_on_device) {
    if (!p || !x || !O || (p->P.ne > 0 && (!H0 || !Oerr))) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, true, "interaction error operators")) return rc;
    return interaction_to(p, x, H0, Oerr, O, O_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
}

}  // extern "C"

namespace grape_eng {

static int expectation_to(grape_plan *p, const double *x, const double *H0tab, const double *Oerr, double *ev) {
    if (p->P.ne == 0) return GRAPE_OK;
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = ud_interaction(p, x, H0tab, Oerr)) return rc;
    double *dev = reinterpret_cast<double *>(p->ud_S);  // (Nt, ne) column-major: Nt * ne tiles of room
    HIPCHECK(grape_unitary::launch_expectation(p->P, p->ud_out, dev, p->stream));
    HIPCHECK(hipMemcpyAsync(ev, dev, (size_t)p->P.Nt * p->P.ne * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return grape_plan_synchronize(p);
}

}  // namespace grape_eng

extern "C" {

int grape_expectation_values(grape_plan *p, const double *x, double *ev) {
    if (!p || !x || !ev) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, false, "expectation values")) return rc;
    return expectation_to(p, x, nullptr, nullptr, ev);
}

int grape_expectation_values_tables(grape_plan *p, const double *x, const double *H0, const double *Oerr,
                                    double *ev) {
    if (!p || !x || !ev || (p->P.ne > 0 && (!H0 || !Oerr))) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, true, "expectation values")) return rc;
    return expectation_to(p, x, H0, Oerr, ev);
}

}  // extern "C"

namespace grape_eng {

// The assembly problem and buffers of the ud workspace (outputs packed in ud_out:
// U_dx | U_dx_add | U_derr | U_derr_dx | U_derr_dx_add); returns the variant list.
std::vector<grape::VSpec> ud_setup(grape_plan *p, grape_unitary::UProblem &UP, grape_unitary::UBuffers &UB) {
    const DevProblem &P0 = p->P;
    const int D = P0.D, Nt = P0.Nt, np = P0.np, na = P0.na, ne = P0.ne;
    const size_t T = (size_t)D * D;
    UP = grape_unitary::UProblem{};
    grape_setup::Variants V = ud_variants(P0);
    UP.off_x2 = V.off_dx2;
    UP.off_err = V.off_err;
    UP.D = D;
    UP.Nt = Nt;
    UP.np = np;
    UP.na = na;
    UP.ne = ne;
    UP.nv = (int)V.vs.size();
    UP.nslots = ud_nslots(P0);
    UP.inv_eps = P0.inv_eps;
    UP.inv_eps2sq = 1.0 / (P0.eps2 * P0.eps2);
    UP.gscr = p->ud_gscr;
    const size_t n_dx = T * np * Nt, n_dxa = T * na, n_e = T * ne, n_edx = T * np * Nt * ne;
    UB = grape_unitary::UBuffers{};
    UB.E = p->ud_E;
    UB.C = p->ud_C;
    UB.Ci = p->general_h0 ? p->ud_Ci : nullptr;
    UB.status = p->d_ctrl + 2;
    UB.V = p->ud_V;
    UB.S = p->ud_S;
    UB.Udx = p->ud_out;
    UB.Udxa = UB.Udx + n_dx;
    UB.Ue = UB.Udxa + n_dxa;
    UB.Uedx = UB.Ue + n_e;
    UB.Uedxa = UB.Uedx + n_edx;
    return std::move(V.vs);
}

static int unitary_derivs(grape_plan *p, const double *x, const double *Htab, double *U, double *U_dx,
                          double *U_dx_add, double *U_derr, double *U_derr_dx, double *U_derr_dx_add) {
    HIPCHECK(hipSetDevice(p->device));
    const DevProblem &P0 = p->P;
    const int D = P0.D, Nt = P0.Nt, np = P0.np, na = P0.na, ne = P0.ne;
    const size_t T = (size_t)D * D;
    if (int rc = ud_alloc(p)) return rc;
    grape_unitary::UProblem UP;
    grape_unitary::UBuffers UB;
    const std::vector<grape::VSpec> vs = ud_setup(p, UP, UB);
    const size_t n_dx = T * np * Nt, n_dxa = T * na, n_e = T * ne, n_edx = T * np * Nt * ne, n_edxa = T * na * ne;
    if (int rc = ud_propagators(p, x, vs, Htab)) return rc;
    hipStream_t st = p->stream;
    HIPCHECK(grape_unitary::launch_assembly(UP, UB, st));
    std::vector<cd> Ulast(T);
    HIPCHECK(hipMemcpyAsync(Ulast.data(), p->ud_C + (size_t)(Nt - 1) * T, T * sizeof(cd), hipMemcpyDeviceToHost, st));
    auto out = [&](double *dst, const cd *src, size_t n) -> hipError_t {
        if (!dst || n == 0) return hipSuccess;
        return hipMemcpyAsync(dst, src, n * sizeof(cd), hipMemcpyDeviceToHost, st);
    };
    HIPCHECK(out(U_dx, UB.Udx, n_dx));
    HIPCHECK(out(U_dx_add, UB.Udxa, n_dxa));
    HIPCHECK(out(U_derr, UB.Ue, n_e));
    HIPCHECK(out(U_derr_dx, UB.Uedx, n_edx));
    HIPCHECK(out(U_derr_dx_add, UB.Uedxa, n_edxa));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    const int rc = grape_plan_synchronize(p);
    if (rc) return rc;
    if (U)  // C_N is stored row-major; the reference's layout is column-major
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                U[2 * ((size_t)i + (size_t)j * D)] = Ulast[(size_t)i * D + j].re;
                U[2 * ((size_t)i + (size_t)j * D) + 1] = Ulast[(size_t)i * D + j].im;
            }
    return GRAPE_OK;
}

}  // namespace grape_eng

extern "C" {

int grape_unitary_derivs(grape_plan *p, const double *x, double *U, double *U_dx, double *U_dx_add, double *U_derr,
                         double *U_derr_dx, double *U_derr_dx_add) {
    if (!p || !x) return fail(GRAPE_ERR_INVALID, "null argument");
    if (int rc = analysis_check(p, p->tables, "grape_unitary_derivs")) return rc;
    if (p->tables) return fail(GRAPE_ERR_INVALID, "grape_unitary_derivs: host-table plan: use grape_unitary_derivs_tables");
    return unitary_derivs(p, x, nullptr, U, U_dx, U_dx_add, U_derr, U_derr_dx, U_derr_dx_add);
}

int grape_unitary_derivs_tables(grape_plan *p, const double *x, const double *H, double *U, double *U_dx,
                                double *U_dx_add, double *U_derr, double *U_derr_dx, double *U_derr_dx_add) {
    if (!p || !x || !H) return fail(GRAPE_ERR_INVALID, "null argument");
    if (!p->tables) return fail(GRAPE_ERR_INVALID, "plan was not created with GRAPE_DESC_HOST_TABLES");
    return unitary_derivs(p, x, H, U, U_dx, U_dx_add, U_derr, U_derr_dx, U_derr_dx_add);
}

}  // extern "C"

namespace grape_eng {

static int dense_expm_batch(int device, int ndim, int n, const double *A, double *E, int *stats, bool pivot) {
    const size_t IMG = grape_dense::kImgDoubles;
    std::vector<double> h((size_t)n * IMG);
    for (int i = 0; i < n; ++i) to_dense_image(A + 2 * (size_t)i * ndim * ndim, ndim, h.data() + i * IMG);
    DevicePool mem;
    double *dA = nullptr, *dE = nullptr;
    int *dctrl = nullptr;
    if (mem.alloc(&dA, n * IMG) || mem.alloc(&dE, n * IMG) || mem.alloc(&dctrl, 8))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed");
    int ctrl[8] = {0};
    if (grape_dense::set_lds_limits() != hipSuccess ||
        hipMemcpy(dA, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dctrl, 0, 8 * sizeof(int)) != hipSuccess ||
        grape_dense::launch_expm_raw(dA, dE, n, dctrl + 1, dctrl + 2, nullptr, pivot) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h.data(), dE, h.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ctrl, dctrl, 8 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(GRAPE_ERR_HIP, std::string("dense expm batch failed: ") + hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < n; ++i) from_dense_image(h.data() + i * IMG, ndim, E + 2 * (size_t)i * ndim * ndim);
    if (stats)
        for (int k = 0; k < 5; ++k) stats[k] = ctrl[2 + k];
    if (ctrl[1] & 1) return fail(GRAPE_ERR_SINGULAR, "singular Pade denominator");
    return GRAPE_OK;
}

// 64 < ndim <= 128: the tiled engine's solve-free exponential, in slabs of a byte budget
static int tiled_expm_batch(int ndim, int n, const double *A, double *E, int *stats) {
    const size_t IMG = grape_tiled::image_doubles(ndim);
    std::vector<double> h((size_t)n * IMG);
    for (int i = 0; i < n; ++i) to_tiled_image(A + 2 * (size_t)i * ndim * ndim, ndim, h.data() + i * IMG);
    DevicePool mem;
    double *dA = nullptr, *dE = nullptr;
    int *dctl = nullptr, *dwords = nullptr, *h_smax = nullptr;
    grape_tiled::ExpSlab X{};
    const size_t slab = std::min<size_t>((size_t)n, std::max<size_t>(1, ((size_t)1 << 30) / (6 * IMG * sizeof(double))));
    if (mem.alloc(&dA, n * IMG) || mem.alloc(&dE, n * IMG) || mem.alloc(&dctl, (size_t)n) || mem.alloc(&dwords, (size_t)8) ||
        alloc_exp_slab(mem, slab, IMG, X, nullptr, 0))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed");
    if (hipHostMalloc(reinterpret_cast<void **>(&h_smax), sizeof(int), hipHostMallocDefault) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "pinned allocation failed");
    int words[8] = {0};
    const bool ok = hipMemcpy(dA, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemset(dwords, 0, 8 * sizeof(int)) == hipSuccess &&
                    grape_tiled::launch_expm_raw(ndim, dA, dE, n, X, dctl, dwords, h_smax, dwords + 2, nullptr) == hipSuccess &&
                    hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(h.data(), dE, h.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(words, dwords, 8 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipHostFree(h_smax);
    if (!ok) return fail(GRAPE_ERR_HIP, std::string("tiled expm batch failed: ") + hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < n; ++i) from_tiled_image(h.data() + i * IMG, ndim, E + 2 * (size_t)i * ndim * ndim);
    if (stats)
        for (int k = 0; k < 5; ++k) stats[k] = words[2 + k];
    return GRAPE_OK;
}

static int expm_batch(int device, int ndim, int n, const double *A, double *E, int *stats, bool pivot) {
    const int dmax = pivot ? GRAPE_MAX_DENSE_DIM : GRAPE_MAX_TILED_DIM;  // (the pivoted exponential stays the dense engine's)
    if (ndim < 2 || ndim > dmax)
        return fail(GRAPE_ERR_UNSUPPORTED, pivot ? "ndim outside [2, GRAPE_MAX_DENSE_DIM]" : "ndim outside [2, GRAPE_MAX_TILED_DIM]");
    if (n < 0 || (n > 0 && (!A || !E))) return fail(GRAPE_ERR_INVALID, "bad argument");
    if (n == 0) return GRAPE_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GRAPE_ERR_NO_DEVICE, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    if (ndim > GRAPE_MAX_DENSE_DIM) return tiled_expm_batch(ndim, n, A, E, stats);
    if (ndim > GRAPE_MAX_SMALL_DIM) return dense_expm_batch(device, ndim, n, A, E, stats, pivot);
    const size_t T = (size_t)ndim * ndim;
    DevicePool mem;
    cd *dA = nullptr, *dE = nullptr;
    int *dovf = nullptr, *dctrl = nullptr;
    if (mem.alloc(&dA, n * T) || mem.alloc(&dE, n * T) || mem.alloc(&dovf, (size_t)n) || mem.alloc(&dctrl, 8))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed");
    int ctrl[8] = {0};
    if (hipMemcpy(dA, A, n * T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dctrl, 0, 8 * sizeof(int)) != hipSuccess ||
        dispatch_expm_raw(ndim, dA, dE, n, dovf, dctrl, dctrl + 1, dctrl + 2, nullptr) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(E, dE, n * T * sizeof(cd), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ctrl, dctrl, 8 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(GRAPE_ERR_HIP, std::string("expm batch failed: ") + hipGetErrorString(hipGetLastError()));
    if (stats)
        for (int k = 0; k < 5; ++k) stats[k] = ctrl[2 + k];
    if (ctrl[1] & 1) return fail(GRAPE_ERR_SINGULAR, "singular Pade denominator");
    return GRAPE_OK;
}

}  // namespace grape_eng

extern "C" {

int grape_expm_batch(int device, int ndim, int n, const double *A, double *E, int *stats) {
    return expm_batch(device, ndim, n, A, E, stats, false);
}

int grape_expm_batch_general(int device, int ndim, int n, const double *A, double *E, int *stats) {
    return expm_batch(device, ndim, n, A, E, stats, true);
}

}  // extern "C"
