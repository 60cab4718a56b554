// grape_plan.hpp -- what the host units of the C ABI share: struct grape_plan, the error helpers, the
// tuning constants and their -D knobs, the owner of a plan's device allocations (DevicePool), and the
// declaration of every function that crosses a unit boundary (namespace grape_eng).  It includes the plain
// types (grape_types.hpp) and the engines' API headers only: no kernel header and no launch body, so none of
// these units can instantiate a kernel (tests/test_capi_cpu.py follows the includes).  The units:
// grape_engine.hip (errors, ids, fault handler, per-dimension dispatch, plan lifetime and getters),
// grape_descriptor.hip (pure host logic on the descriptor), grape_plan_build.hip (plan construction),
// grape_call.hip (the call path), grape_analysis.hip (the single-evaluation analysis entry points).
// Private to those units (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "grape.h"
#include "grape_launch_api.hpp"
#include "grape_walk_api.hpp"
#include "grape_projector_api.hpp"
#include "grape_dense_api.hpp"
#include "grape_tiled_api.hpp"
#include "grape_unitary_api.hpp"
#include "grape_eval1_api.hpp"
#include "grape_plan_setup.hpp"
#include "grape_descriptor.hpp"

using grape::DevBatch;
using grape::DevProblem;
using grape::Term;
using grape_host::KMark;

#define HIPCHECK(expr)                                                                  \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(GRAPE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace grape_eng {

constexpr int kScanWide = grape_host::kScanWide, kScanNarrow = grape_host::kScanNarrow,
              kScanTiny = grape_host::kScanTiny, kScanLatency = grape_host::kScanLatency;
// calls of at most this many evaluations run the two sector classes on two streams (enqueue)
#ifndef GRAPE_FORK_MAX_BATCH
#define GRAPE_FORK_MAX_BATCH 4096
#endif
constexpr int kForkMaxBatch = GRAPE_FORK_MAX_BATCH;
// throughput passes of the Rydberg layout: both walk classes' one-wave scans in one launch
// (grape_launch_api.hpp launch_scan_pair)
// chunks of a phase-covariant throughput walk class: (64 / S) / this per scan wave.  2: C2
// 26.4 -> 29.0 M evals/s (4: 27.7 M; one GPU call, gpurun_out A/B r5chunk)
#ifndef GRAPE_GAUGE_CHUNK_DIV
#define GRAPE_GAUGE_CHUNK_DIV 2
#endif
// chunks per evaluation of the lab-frame error walks on throughput passes (0: the walks' formula, 8 and 16 at
// C3).  C3 (A/B in one GPU call, profiles/r06/c3): 4-level class 8 -> 6 chunks 2.64 -> 2.68 M evals/s (12:
// 2.49 M), 2-level class 16 -> 8 chunks 2.64 -> 2.69 M -- fewer lanes, whole waves per SIMD round, and
// shorter error scans
#ifndef GRAPE_LAB_CHUNKS4  // classes of 4 levels
#define GRAPE_LAB_CHUNKS4 6
#endif
#ifndef GRAPE_LAB_CHUNKS2  // ... of fewer levels
#define GRAPE_LAB_CHUNKS2 8
#endif
// Pair kernels (both sector classes of a stage in one launch) for calls of at most this many evaluations
// (fewer sub-evaluations than CUs: latency-bound; grape_walk_api.hpp launch_pair)
constexpr int kPairMaxBatch = 64;
// One workgroup per evaluation (grape_eval1.hip) for every call of an eligible plan (the Rydberg
// layout with phase-covariant classes) whose max_batch is at most this: a plan-level choice, so that a
// single evaluation and the same evaluation inside a batch stay bit-identical on every plan
// (GRAPE_OPT_NO_EVAL1 turns it off).  Round 6: 2 048 (was 256) -- C2 passes of 1 024 / 2 048 evaluations
// measured 15.8 / 17.1 M evals/s this way against 5.3 / 15.6 M through the merged walks, 4 096 17.8 M
// against 24.3 M; the optimiser's 1 024-restart plan (c4opt) 2.3 -> 3.5 M evals/s (profiles/r06/lat2)
#ifndef GRAPE_EVAL1_MAX_BATCH
#define GRAPE_EVAL1_MAX_BATCH 2048
#endif
constexpr int kEval1MaxBatch = GRAPE_EVAL1_MAX_BATCH;
constexpr int kCtrlInts = 8;  // [0..1] single-eval counters, [2] status, [4..5] pipeline overflow counters

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

}  // namespace grape_eng

struct grape_plan {
    int device = 0;
    hipStream_t stream = nullptr;      // where work is enqueued (own_stream or the caller's)
    hipStream_t own_stream = nullptr;
    hipStream_t cur_stream = nullptr;  // stream of the launch being enqueued (profiling marks)
    int *h_status = nullptr;           // pinned copy of the device status word
    DevProblem P{};
    int max_batch = 0;
    grape_eng::DevicePool mem;  // owns every device buffer of the plan; the named pointers below are views
    cd *d_ops = nullptr;
    cd *d_opsT = nullptr;
    Term *d_h0 = nullptr, *d_tgt = nullptr, *d_err = nullptr;
    int *d_err_off = nullptr;
    // product coefficients (grape.h GRAPE_OP_FACTOR): the factor slots of the H0 and error terms, an argument
    // of the product kernels (grape_prod.hpp); FT.h0 is null for a plan without factor terms
    grape::FactorTab FT{};
    Term *d_fac_h0 = nullptr, *d_fac_err = nullptr;
    double *d_W = nullptr;
    cd *d_E = nullptr, *d_Q = nullptr, *d_Mc = nullptr, *d_Carry = nullptr, *d_Ub = nullptr, *d_Me = nullptr;
    grape::VSpec *d_vs = nullptr;
    int *d_ovf2 = nullptr;
    cd *d_ovf2_slots = nullptr;
    double *d_Fd2 = nullptr, *d_Fd2dx = nullptr, *d_part_err = nullptr;
    cd *d_Zl = nullptr;
    double *d_x = nullptr, *d_F = nullptr, *d_Fdx = nullptr, *d_part = nullptr, *d_tgt_part = nullptr;
    int *d_ovf = nullptr, *d_ctrl = nullptr;  // ctrl: [0], [1] overflow counts, [2] status
    // closure mode (GRAPE_DESC_HOST_TABLES): host-evaluated H and target tables
    bool tables = false;
    cd *d_Htab = nullptr, *d_U0tab = nullptr;
    cd *d_sink = nullptr;                      // DevBatch::sink
    // general projector (FidelityCalculations.jl:47-51): P0 P, P, P0 row-major; head scratch
    cd *d_PA = nullptr, *d_PB = nullptr, *d_P0g = nullptr, *d_gpscr = nullptr;
    // sectors (grape.h grape_plan_sectors): per evaluation the fidelity path runs the sector
    // problems of ncls classes (Ps[c]: nsec sectors of S levels each, workspace sb[c]), then
    // the sector head over the assembled U (SH)
    struct SecBuf {
        cd *E = nullptr, *Q = nullptr, *Mc = nullptr, *Carry = nullptr, *Ub = nullptr, *slots = nullptr,
           *ops = nullptr, *opsT = nullptr, *Msec = nullptr, *Tc = nullptr, *wscr = nullptr, *Ew = nullptr,
           *gEt = nullptr;
        int *ovf = nullptr, *ovf2 = nullptr, *sidx = nullptr, *gauge_n = nullptr;
        double *part = nullptr;
        // error sources: local-frame images, per-chunk triples, Tot / M_e blocks, F_d2err_dx terms
        cd *Zl = nullptr, *Me = nullptr, *TotS = nullptr, *MsecE = nullptr, *Wc = nullptr;
        double *part_err = nullptr;
    };
    int ncls = 0;
    DevProblem Ps[2]{};
    SecBuf sb[2];
    int *d_fixed = nullptr;
    grape_proj::SectorHead SH{};
    // one workgroup per evaluation (grape_eval1.hip): eligible plan, its E~ tables, class A's index
    bool e1 = false;
    // throughput passes: both walk classes in one lane (grape_walk.hpp k_walk_fwd_m / k_walk_grad_m);
    // merge_pa: the index of the class of 3 or 4 levels
    bool merged = false;
    int merge_pa = 0;
    // the wide pass (enqueue_wide): W = max_batch x nchunks evaluations per pass of a rank-one merged plan, or 0
    int wide = 0;
    int wide_lev[2][2] = {{0, 0}, {0, 0}};  // the head's level of sector w's weighted slot, per class (k_wide_head)
    cd *d_e1_Et = nullptr, *d_e1_scr = nullptr;
    unsigned char *d_e1_tab = nullptr;  // the kernel's table blob (grape_eval1 tab_build)
    int e1_pa = 0;
    // GRAPE_EVAL1_TRACE=1: workgroup 0's phase clocks of every host-array call, averaged and printed
    // to stderr when the plan is destroyed (mapped pinned buffer; a tuning aid)
    long long *e1_trace = nullptr, *e1_trace_d = nullptr;
    double e1_phase[16] = {0};
    long e1_calls = 0;
    // symmetry-adapted sectors (grape_symmetry.hpp): the head's rotated operators, projector, weights
    bool symmetry = false;
    cd *d_ops_sym = nullptr, *d_opsT_sym = nullptr, *d_PA_sym = nullptr, *d_PB_sym = nullptr;
    double *d_W_sym = nullptr;
    // small calls with two sector classes: the second class runs on an auxiliary stream beside the
    // first (fork / join events; the classes are independent until the sector heads)
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool capturing = false;  // graph_capture in progress: calls captured into graphs never fork (the
                             // captured fork was removed in round 5)
    // dense engine (GRAPE_MAX_SMALL_DIM < d <= GRAPE_MAX_DENSE_DIM)
    bool dense = false;
    grape_dense::DenseProblem DP{};
    double *dn_opimg = nullptr, *dn_W = nullptr, *dn_E = nullptr, *dn_Q = nullptr, *dn_Carry = nullptr,
           *dn_M = nullptr, *dn_Mc = nullptr, *dn_Z = nullptr, *dn_Ub = nullptr, *dn_Zl = nullptr, *dn_Vc = nullptr,
           *dn_Sx = nullptr, *dn_Tot = nullptr, *dn_Me = nullptr, *dn_Mp = nullptr, *dn_B0 = nullptr,
           *dn_Fadd = nullptr, *dn_Fd2add = nullptr;
    // tiled engine (GRAPE_MAX_DENSE_DIM < d <= GRAPE_MAX_TILED_DIM): the problem and the workspace of one pass
    // of max_batch evaluations (max_batch: the caller's, cut to what the plan's byte budget holds)
    bool tiled = false;
    grape_tiled::TiledProblem TP{};
    grape_tiled::TiledBatch TB{};
    int *tl_h_smax = nullptr;  // pinned: the pass's largest squaring count
    // grape_unitary_derivs workspace (allocated on first use)
    grape::VSpec *ud_vs = nullptr;
    cd *ud_E = nullptr, *ud_C = nullptr, *ud_V = nullptr, *ud_S = nullptr, *ud_out = nullptr;
    int *ud_ovf = nullptr;
    cd *ud_gscr = nullptr;     // d > 12: tile scratch of the grape_unitary kernels
    // general (non-Hermitian) H0, e.g. a -i Gamma/2 decay term: the chain is inverted by LU
    // (UnitaryCalculations.jl:47) and the fidelity path runs from the materialised derivatives
    // (grape_unitary.hip k_u_fid_head / k_u_fid_contract), one evaluation at a time
    bool general_h0 = false;
    // 12 < d <= 64 created with GRAPE_OPT_GENERAL_H0: every exponential through the dense engine's
    // pivoted kernels (k_dexp<true> / k_dexp_raw<true>), valid for any generator
    bool pivot = false;
    cd *ud_Ci = nullptr, *d_G = nullptr;
    cd *d_fscr = nullptr;        // d > 12: the fidelity head's tiles (global scratch)
    double *ud_Aimg = nullptr;   // closures at d > 12: the tabulated generators as padded images
    std::vector<grape::VSpec> ud_vs_host;  // the variant list in ud_vs (general H0 batches)
    double *ud_Eimg = nullptr; // dense engine: the variant table as register-file images
    // small host-array calls (the reference's one-x-per-call pattern): the whole call --
    // H2D copy, every launch, D2H copies -- replayed as one captured HIP graph per batch size
    struct GraphEntry {
        int nb;
        hipGraphExec_t exec;
    };
    std::vector<GraphEntry> graphs;
    double *h_x = nullptr, *h_F = nullptr, *h_Fd2 = nullptr, *h_Fd2dx = nullptr;  // pinned
    double *hd_x = nullptr, *hd_F = nullptr;  // ... h_x and h_F as the device sees them (eval1 calls)
    // graph path: F ([kGraphBatch]) and F_dx ([nb][nx]) of a call side by side in one device block
    // (h_F is its pinned image), so one D2H copy returns both
    double *d_gout = nullptr;
    // time-sharded evaluations (grape_slice_*): column-major U_slice / M' staging (2 d x d)
    cd *d_slice = nullptr;
    bool uses_tstep = false;  // some H0 term reads the step index (slices would need its offset)
    // optional per-kernel timing with HIP events on the plan's stream
    bool profiling = false;
    struct Pending {
        int kernel;
        hipEvent_t a, b;
    };
    std::vector<hipEvent_t> ev_pool;
    std::vector<Pending> pending;
    double kernel_ms[GRAPE_NUM_KERNELS] = {0};
    long long kernel_launches[GRAPE_NUM_KERNELS] = {0};
    hipEvent_t get_event() {
        hipEvent_t e = nullptr;
        if (!ev_pool.empty()) {
            e = ev_pool.back();
            ev_pool.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    }
};

namespace grape_eng {

// What the phases of a small-engine / general-path plan share.
struct PlanBuild {
    const grape_desc *desc;
    grape_plan *p;
    const Route &rt;
    const ProjectorSetup &ps;
    int n_err_terms;
    int ncu = 256;          // compute units of the plan's device
    int scan_override = 0;  // plan option: 1, 4, 8 or 16 waves (0: by batch size)
    int n_ops = 0;
    std::vector<grape::VSpec> vs;
    // the sector path's view: rotated operators and projector when the symmetry-adapted sectors are on
    SymSetup sym;
    grape_desc sdesc{};
    SectorSetup ss;
    const ProjectorSetup &sps() const { return sym.on ? sym.ps : ps; }
};

// grape_engine.hip
hipError_t dispatch_pipeline(int D, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st,
                             const KMark &mk);
hipError_t dispatch_sector_stage(int S, int stage, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                                 hipStream_t st, const KMark &mk);
hipError_t dispatch_sector_reduce(int S, const DevProblem &P, const DevBatch &B, const grape::SecParts &sp, int nev,
                                  hipStream_t st, const KMark &mk);
hipError_t dispatch_expm_raw(int D, const cd *A, cd *E, int n, int *ovf, int *ovfc, int *status,
                             int *mstats, hipStream_t st);
hipError_t dispatch_expm_variants(int D, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                                  hipStream_t st);
hipError_t dispatch_expm_table(int D, const DevProblem &P, const DevBatch &B, hipStream_t st);
hipError_t dispatch_lds_limits(int D);

// grape_plan_build.hip
void to_dense_image(const double *src, int d, double *img);
void from_dense_image(const double *img, int d, double *dst);
void to_tiled_image(const double *src, int d, double *img);
void from_tiled_image(const double *img, int d, double *dst);
hipError_t alloc_exp_slab(DevicePool &mem, size_t items, size_t img, grape_tiled::ExpSlab &X,
                          double **extra, size_t n_extra);
int create_dense(const grape_desc *desc, grape_plan *p, bool xadd_dep, const ProjectorSetup &ps, int n_err_terms);
int create_tiled(const grape_desc *desc, grape_plan *p, const ProjectorSetup &ps);
int upload_factors(grape_plan *p, const FactorSplit &fs);
int open_plan(grape_plan *p, const grape_desc *desc, int device, const Route &rt);
int create_small(PlanBuild &b);
void walk_pair_order(const grape_plan *p, int *pa, int *pb);

// grape_call.hip
grape_eval1::Args eval1_args(const grape_plan *p, const double *x, double *F, double *Fdx);

// grape_analysis.hip
std::vector<grape::VSpec> ud_setup(grape_plan *p, grape_unitary::UProblem &UP, grape_unitary::UBuffers &UB);
int ud_alloc(grape_plan *p);
int ud_propagators_dev(grape_plan *p, const double *d_x, int nv, const cd *d_Htab);

}  // namespace grape_eng
