// grape_engine.hip -- C ABI (include/grape.h) over the gfx950 GRAPE kernels.
//
// A plan owns: the device copy of the operator basis (row-major tiles), the
// term tables, and a workspace for `max_batch` evaluations laid out in HBM as
//   E  [b][k][v][D][D]   propagators of every FD variant   (c128)
//   Q  [b][k][D][D]      chunk-local prefix products
//   Mc [b][c][D][D]      per-chunk gradient kernels
// (288 GB per MI355X; at d=9, N_t=512 one evaluation needs 2.0 MB).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <cstdlib>
#include <csignal>
#include <cstdint>
#include <dlfcn.h>
#include <execinfo.h>
#include <link.h>
#include <ucontext.h>
#include <unistd.h>
#include <vector>

#include "grape.h"
#include "grape_launch.hpp"
#include "grape_dense_api.hpp"
#include "grape_tiled_api.hpp"
#include "grape_unitary_api.hpp"
#include "grape_symmetry.hpp"
#include "grape_eval1_api.hpp"
#include "grape_plan_setup.hpp"

// instantiated in grape_inst.hip (one translation unit per dimension)
namespace grape_host {
#define GRAPE_EXTERN_DIM(d) GRAPE_DECLARE_DIM(d, extern)
GRAPE_DIMS(GRAPE_EXTERN_DIM)
#undef GRAPE_EXTERN_DIM
GRAPE_DECLARE_SCAN_PAIR(extern)
}  // namespace grape_host

using grape::cd;
using grape::DevBatch;
using grape::DevProblem;
using grape::Term;

static_assert(sizeof(Term) == sizeof(grape_term), "grape_term layout");

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHECK(expr)                                                                  \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(GRAPE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr int kScanWide = grape_host::kScanWide, kScanNarrow = grape_host::kScanNarrow,
              kScanTiny = grape_host::kScanTiny, kScanLatency = grape_host::kScanLatency;
// calls of at most this many evaluations run the two sector classes on two streams (enqueue)
#ifndef GRAPE_FORK_MAX_BATCH
#define GRAPE_FORK_MAX_BATCH 4096
#endif
constexpr int kForkMaxBatch = GRAPE_FORK_MAX_BATCH;
// throughput passes of the Rydberg layout: both walk classes' one-wave scans in one launch
// (grape_launch.hpp launch_scan_pair)
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
// Chunk count of the 3-level phase-covariant class on throughput passes (the merged walks' chunking,
// grape_walk.hpp k_walk_fwd_m / k_walk_grad_m).  A walk's time is (rounds of resident waves) x (steps
// per lane): every lane of a pass walks L steps, so a chunk count that leaves the last round of waves
// partly empty wastes that round's SIMD time -- C2's 10 chunks at 32 768 evaluations per pass were
// 5 120 gradient waves, 2.5 rounds at 2 waves per SIMD.  The model, in microseconds per C2 unit from
// the round-5 profile (profiles/r05/final_c2b): 2.72 x rounds(grad, 2 waves/SIMD) x L + 5.7 x chunks
// (k_scan_seq), minimised over [nc/2, 2 nc]; the forward walk measured the same at 8, 10, 12 and 16
// chunks (0.185-0.187 ms per pass), so it has no term.  C2: 8 chunks, 48.5-48.9 -> 50.7 M evals/s
// (12: 49.7 M, 16: 48.9 M; profiles/r05/ab_nchunks).  GRAPE_GAUGE_NCHUNKS=n (environment) forces n.
static int merged_chunk_count(long MB, int Nt, int nc, int ncu) {
    if (const char *e = getenv("GRAPE_GAUGE_NCHUNKS")) {
        const int n = atoi(e);
        if (n > 0) return std::min(n, Nt);
    }
    const double simds = 4.0 * ncu;
    double best = 1e300;
    int pick = nc;
    for (int n = std::max(1, nc / 2); n <= std::min(2 * nc, Nt); ++n) {
        const int L = (Nt + n - 1) / n, nch = (Nt + L - 1) / L;
        const double waves = std::ceil((double)MB * nch / 64.0);
        const double cost = 2.72 * std::ceil(waves / (2.0 * simds)) * L + 5.7 * nch;
        if (cost < best - 1e-9) {
            best = cost;
            pick = nch;
        }
    }
    return pick;
}
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
using grape_host::KMark;
using grape_host::launch_pipeline;
using grape_host::launch_expm_raw;
using grape_host::set_lds_limits;

// f(std::integral_constant<int, D>) for the instantiated dimension D (GRAPE_DIMS)
template <class F>
hipError_t dispatch_dim(int D, F &&f) {
    switch (D) {
#define CASE(d) \
    case d: return f(std::integral_constant<int, d>{});
        GRAPE_DIMS(CASE)
#undef CASE
    }
    return hipErrorInvalidValue;
}
hipError_t dispatch_pipeline(int D, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F, hipStream_t st,
                             const KMark &mk) {
    return dispatch_dim(D, [&](auto d) { return launch_pipeline<decltype(d)::value>(P, B, F, st, mk); });
}
hipError_t dispatch_sector_stage(int S, int stage, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                                 hipStream_t st, const KMark &mk) {
    return dispatch_dim(S, [&](auto d) { return grape_host::launch_sector_stage<decltype(d)::value>(stage, P, B, F, st, mk); });
}
hipError_t dispatch_sector_reduce(int S, const DevProblem &P, const DevBatch &B, const grape::SecParts &sp, int nev,
                                  hipStream_t st, const KMark &mk) {
    return dispatch_dim(S, [&](auto d) { return grape_host::launch_sector_reduce<decltype(d)::value>(P, B, sp, nev, st, mk); });
}
hipError_t dispatch_expm_raw(int D, const cd *A, cd *E, int n, int *ovf, int *ovfc, int *status,
                             int *mstats, hipStream_t st) {
    return dispatch_dim(D, [&](auto d) { return launch_expm_raw<decltype(d)::value>(A, E, n, ovf, ovfc, status, mstats, st); });
}
hipError_t dispatch_expm_variants(int D, const DevProblem &P, const DevBatch &B, const grape::FactorTab &F,
                                  hipStream_t st) {
    return dispatch_dim(D, [&](auto d) { return grape_host::launch_expm_variants<decltype(d)::value>(P, B, F, st); });
}
hipError_t dispatch_expm_table(int D, const DevProblem &P, const DevBatch &B, hipStream_t st) {
    return dispatch_dim(D, [&](auto d) { return grape_host::launch_expm_table<decltype(d)::value>(P, B, st); });
}
hipError_t dispatch_lds_limits(int D) {
    return dispatch_dim(D, [&](auto d) { return set_lds_limits<decltype(d)::value>(); });
}

}  // namespace

struct grape_plan {
    int device = 0;
    hipStream_t stream = nullptr;      // where work is enqueued (own_stream or the caller's)
    hipStream_t own_stream = nullptr;
    hipStream_t cur_stream = nullptr;  // stream of the launch being enqueued (profiling marks)
    int *h_status = nullptr;           // pinned copy of the device status word
    DevProblem P{};
    int max_batch = 0;
    grape_setup::DevicePool mem;  // owns every device buffer of the plan; the named pointers below are views
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
    // pivoted kernels (k_dexp_piv / k_dexp_raw_piv), valid for any generator
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

static grape_eval1::Args eval1_args(const grape_plan *p, const double *x, double *F, double *Fdx);

static void free_plan(grape_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->e1_trace) {
        if (p->e1_calls > 0) {
            std::fprintf(stderr, "[grape eval1 trace] %ld calls, mean clocks per phase:", p->e1_calls);
            for (int i = 0; i < 9; ++i) std::fprintf(stderr, " %.0f", p->e1_phase[i] / p->e1_calls);
            std::fprintf(stderr, " (x+tables, totals, wave scan, sync, carry, head, grad, sync, store);"
                                 " clocks per us %.1f; head wave: sums %.0f, reduce+F %.0f, M blocks %.0f,"
                                 " x_add %.0f; phase A: head wave %.0f, class B %.0f\n", p->e1_phase[9] / p->e1_calls,
                                 p->e1_phase[10] / p->e1_calls, p->e1_phase[11] / p->e1_calls,
                                 p->e1_phase[12] / p->e1_calls, p->e1_phase[13] / p->e1_calls,
                                 p->e1_phase[14] / p->e1_calls, p->e1_phase[15] / p->e1_calls);
        }
        (void)hipHostFree(p->e1_trace);
    }
    p->mem.release_all();
    for (auto &e : p->ev_pool) (void)hipEventDestroy(e);
    for (auto &pe : p->pending) {
        (void)hipEventDestroy(pe.a);
        (void)hipEventDestroy(pe.b);
    }
    for (auto &g : p->graphs) (void)hipGraphExecDestroy(g.exec);
    for (double *h : {p->h_x, p->h_F, p->h_Fd2, p->h_Fd2dx})
        if (h) (void)hipHostFree(h);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    if (p->aux_stream) (void)hipStreamDestroy(p->aux_stream);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    if (p->h_status) (void)hipHostFree(p->h_status);
    if (p->tl_h_smax) (void)hipHostFree(p->tl_h_smax);
    delete p;
}

static int validate_terms(const grape_term *t, int n, int n_ops, int np, int na, bool target, const char *what) {
    int nfac = 0;  // factor terms on the current operator term
    for (int k = 0; k < n; ++k) {
        const bool factor = t[k].op == GRAPE_OP_FACTOR;
        if (factor) {  // product coefficients: a real scalar on the closest preceding operator term of this list
            if (target) return fail(GRAPE_ERR_INVALID, std::string(what) + ": factor terms are not allowed in target terms");
            if (k == 0)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term must follow an operator term of its list");
            if (++nfac > GRAPE_MAX_FACTORS)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": more than GRAPE_MAX_FACTORS factor terms on one operator term");
            if (t[k].func < GRAPE_FN_ONE || t[k].func > GRAPE_FN_SIN)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term's func must be ONE, LINEAR, COS or SIN");
            if (t[k].scale_im != 0.0)
                return fail(GRAPE_ERR_INVALID, std::string(what) + ": a factor term's scale must be real (scale_im = 0)");
        } else {
            nfac = 0;
        }
        if (!factor && (t[k].op < 0 || t[k].op >= n_ops)) return fail(GRAPE_ERR_INVALID, std::string(what) + ": op out of range");
        if (t[k].var < 0 || t[k].var > 3) return fail(GRAPE_ERR_INVALID, std::string(what) + ": bad var");
        if (t[k].func < 0 || t[k].func > 4) return fail(GRAPE_ERR_INVALID, std::string(what) + ": bad func");
        if (t[k].var == 1 && (t[k].index < 0 || t[k].index >= np))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": control index out of range");
        if (t[k].var == 2 && (t[k].index < 0 || t[k].index >= na))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": x_add index out of range");
        if (target && (t[k].var == 1 || t[k].var == 3))
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": target terms may only use x_add");
        if (!target && t[k].func == 4)
            return fail(GRAPE_ERR_INVALID, std::string(what) + ": cis coefficients only in target terms");
    }
    return GRAPE_OK;
}

// Product coefficients (grape.h GRAPE_OP_FACTOR).  A validated descriptor split once into the plain
// descriptor every other piece of host logic sees -- operator terms only, err_term_offsets re-based, so
// that nothing ever indexes ops[-1] -- and the factor slots of its H0 and error terms
// (grape_kernels.hpp FactorTab: kMaxFactors slots per operator term, op = 1 live, 0 empty).  A descriptor
// without factor terms is passed through untouched (plain = *desc, the caller's own pointers).
struct FactorSplit {
    bool any = false;
    bool reads_xadd = false, reads_tstep = false;  // some factor reads x_add / the step index
    grape_desc plain{};
    std::vector<grape_term> h0, err, fac_h0, fac_err;
    std::vector<int32_t> err_off;
};
static void split_list(const grape_term *t, int n, std::vector<grape_term> &ops, std::vector<grape_term> &fac,
                       FactorSplit &fs) {
    int slot = 0;
    for (int k = 0; k < n; ++k) {
        if (t[k].op != GRAPE_OP_FACTOR) {
            ops.push_back(t[k]);
            grape_term empty{};  // op = 0: an empty slot
            fac.insert(fac.end(), (size_t)GRAPE_MAX_FACTORS, empty);
            slot = 0;
        } else if (!ops.empty() && slot < GRAPE_MAX_FACTORS) {
            grape_term f = t[k];
            f.op = 1;
            fac[fac.size() - (size_t)GRAPE_MAX_FACTORS + (size_t)slot++] = f;
            fs.any = true;
            fs.reads_xadd = fs.reads_xadd || f.var == GRAPE_VAR_XADD;
            fs.reads_tstep = fs.reads_tstep || f.var == GRAPE_VAR_TSTEP;
        }
    }
}
static void split_factors(const grape_desc *desc, FactorSplit &fs) {
    fs.plain = *desc;
    if ((desc->reserved[0] & GRAPE_DESC_HOST_TABLES) || !desc->h0_terms) return;
    split_list(desc->h0_terms, desc->n_h0_terms, fs.h0, fs.fac_h0, fs);
    if (desc->nerr > 0 && desc->err_term_offsets && desc->err_terms) {
        fs.err_off.push_back(0);
        for (int e = 0; e < desc->nerr; ++e) {
            const int a = desc->err_term_offsets[e], b = desc->err_term_offsets[e + 1];
            split_list(desc->err_terms + a, b - a, fs.err, fs.fac_err, fs);
            fs.err_off.push_back((int32_t)fs.err.size());
        }
    }
    if (!fs.any) return;  // the caller's descriptor as it is
    fs.plain.h0_terms = fs.h0.data();
    fs.plain.n_h0_terms = (int32_t)fs.h0.size();
    if (!fs.err_off.empty()) {
        fs.plain.err_terms = fs.err.data();
        fs.plain.err_term_offsets = fs.err_off.data();
    }
    // the stored pipeline only: no lane matrices, chains, chunk walks (so no gauge search, pair, merged or
    // wide passes) and no one-workgroup kernel -- those build generators from the plain term lists
    fs.plain.reserved[1] |= GRAPE_OPT_NO_LANE | GRAPE_OPT_NO_CHAIN | GRAPE_OPT_NO_WALK | GRAPE_OPT_NO_GAUGE |
                            GRAPE_OPT_NO_PAIR | GRAPE_OPT_NO_MERGE | GRAPE_OPT_NO_RANK1 | GRAPE_OPT_NO_WIDE |
                            GRAPE_OPT_NO_EVAL1 | GRAPE_OPT_NO_TWIN;
}

// The fused engines take C_k^-1 = C_k^dagger for the chain C_k of the NOMINAL propagators
// exp(-i dt H0) and skip balancing (a permutation only for Hermitian H): both need a
// Hermitian H0.  A term c(x) * OP keeps H0 Hermitian for every x when its function is
// real-valued and scale * OP is Hermitian; anything else (e.g. a -i Gamma/2 decay term in
// H0) selects the general-H0 path (LU inverse of the chain, grape_unitary.hip) on the small
// engine and is refused by the dense one.  Error generators need no such property:
// their propagators only enter through differences dE (UnitaryCalculations.jl:68-83) that
// the nominal chain transports, so a non-Hermitian Herror (a decay-rate error) is served.
// 0: every term keeps H Hermitian; 1: a complex-valued coefficient; 2: scale * operator not Hermitian
static int hermitian_terms(const grape_desc *desc, const grape_term *t, int n) {
    const int D = desc->ndim;
    for (int k = 0; k < n; ++k) {
        if (t[k].func == GRAPE_FN_CIS) return 1;
        const double *op = desc->ops + 2 * (size_t)t[k].op * D * D;
        const double sr = t[k].scale_re, si = t[k].scale_im;
        double mx = 0.0, dev = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                const double *a = op + 2 * ((size_t)i + (size_t)j * D), *b = op + 2 * ((size_t)j + (size_t)i * D);
                // (s a)_ij - conj((s a)_ji)
                const double re = (sr * a[0] - si * a[1]) - (sr * b[0] - si * b[1]);
                const double im = (sr * a[1] + si * a[0]) + (sr * b[1] + si * b[0]);
                mx = std::max(mx, std::hypot(sr * a[0] - si * a[1], sr * a[1] + si * a[0]));
                dev = std::max(dev, std::hypot(re, im));
            }
        if (dev > 1e-12 * std::max(mx, 1e-300)) return 2;
    }
    return 0;
}
// The SUM of a term list Hermitian for every argument (round 6): terms with complex coefficients (each
// scale * operator non-Hermitian, e.g. e^{i a} U + e^{-i a} U^dag) whose sum is Hermitian, as the reference
// accepts any closure with a Hermitian value (UnitaryCalculations.jl:45-47).  Checked at seven probe
// arguments (controls, x_add and the step index drawn from a fixed generator): the coefficients are
// analytic in their argument, so a sum Hermitian at generic points is Hermitian everywhere.
static std::complex<double> term_value(const grape_term &t, const double *x, const double *xa, int nt1) {
    double v = 1.0;
    if (t.var == 1) v = x[t.index];
    else if (t.var == 2) v = xa[t.index];
    else if (t.var == 3) v = (double)nt1;
    const double arg = t.a * v + t.b;
    std::complex<double> f(1.0, 0.0);
    if (t.func == 1) f = arg;
    else if (t.func == 2) f = std::cos(arg);
    else if (t.func == 3) f = std::sin(arg);
    else if (t.func == 4) f = std::complex<double>(std::cos(arg), std::sin(arg));
    return std::complex<double>(t.scale_re, t.scale_im) * f;
}
static bool hermitian_sum(const grape_desc *desc, const grape_term *t, int n) {
    const int D = desc->ndim;
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {  // splitmix64 -> [-3, 3)
        st += 0x9e3779b97f4a7c15ull;
        uint64_t z = st;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return 6.0 * ((double)(z >> 11) * (1.0 / 9007199254740992.0)) - 3.0;
    };
    std::vector<double> x(std::max(1, desc->nparam)), xa(std::max(1, desc->nadd));
    std::vector<std::complex<double>> H((size_t)D * D);
    for (int probe = 0; probe < 7; ++probe) {
        for (double &v : x) v = rnd();
        for (double &v : xa) v = rnd();
        const int nt1 = 1 + (int)((unsigned)(probe * 7919) % (unsigned)std::max(1, desc->ntimes));
        std::fill(H.begin(), H.end(), std::complex<double>(0.0, 0.0));
        for (int k = 0; k < n; ++k) {
            const std::complex<double> c = term_value(t[k], x.data(), xa.data(), nt1);
            const double *op = desc->ops + 2 * (size_t)t[k].op * D * D;
            for (size_t e = 0; e < (size_t)D * D; ++e) H[e] += c * std::complex<double>(op[2 * e], op[2 * e + 1]);
        }
        double mx = 0.0, dev = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                mx = std::max(mx, std::abs(H[i + (size_t)j * D]));
                dev = std::max(dev, std::abs(H[i + (size_t)j * D] - std::conj(H[j + (size_t)i * D])));
            }
        if (dev > 1e-12 * std::max(mx, 1e-300)) return false;
    }
    return true;
}
static int check_hermitian_terms(const grape_desc *desc, const grape_term *t, int n, const char *what) {
    const int h = hermitian_terms(desc, t, n);
    if (h && desc->ndim > GRAPE_MAX_SMALL_DIM && hermitian_sum(desc, t, n)) return GRAPE_OK;  // dense: the sum
    if (h == 1) return fail(GRAPE_ERR_UNSUPPORTED, std::string(what) + ": complex-valued coefficient (H must be Hermitian)");
    if (h == 2)
        return fail(GRAPE_ERR_UNSUPPORTED,
                    std::string(what) + ": scale * operator is not Hermitian (non-unitary propagators are not supported)");
    return GRAPE_OK;
}

// ---------------------------------------------------------------------------
// dense engine plan (GRAPE_MAX_SMALL_DIM < d <= GRAPE_MAX_DENSE_DIM)
// ---------------------------------------------------------------------------
// column-major interleaved d x d complex <-> zero-padded 64 x 64 register-file image:
// f(o, e) for every image slot o (re at o, im at 64 * 64 + o) and its element's offset e (-1: padding)
template <class F>
static void dense_image_slots(int d, F &&f) {
    for (int w = 0; w < 4; ++w)
        for (int t = 0; t < 4; ++t)
            for (int r = 0; r < 4; ++r)
                for (int l = 0; l < 64; ++l) {
                    const int row = 16 * t + (l >> 4) + 4 * r, col = 16 * w + (l & 15);
                    f(((w * 4 + t) * 4 + r) * 64 + l, row < d && col < d ? 2 * ((long)row + (long)col * d) : -1L);
                }
}
static void to_dense_image(const double *src, int d, double *img) {
    dense_image_slots(d, [&](int o, long e) {
        img[o] = e >= 0 ? src[e] : 0.0;
        img[64 * 64 + o] = e >= 0 ? src[e + 1] : 0.0;
    });
}
static void from_dense_image(const double *img, int d, double *dst) {
    dense_image_slots(d, [&](int o, long e) {
        if (e >= 0) dst[e] = img[o], dst[e + 1] = img[64 * 64 + o];
    });
}

// The projector (FidelityCalculations.jl:47-51): the full matrix P0 when given, else its
// diagonal.  A real diagonal P0 is served by the engines' specialised kernels (weights W);
// anything else sets gen_proj and keeps A = P0 P, B = P (P = P0 with nonzeros set to 1)
// and P0 itself, row-major, for the general heads (grape_projector.hip).
struct ProjectorSetup {
    std::vector<double> W;
    std::vector<cd> A, B, P0;
    bool general = false;
    double trP = 0.0;
    void set_general(int D, const std::vector<cd> &pattern) {  // B = the pattern P, A = P0 P
        std::fill(W.begin(), W.end(), 0.0);  // the specialised results are all overwritten
        B = pattern;
        A.assign((size_t)D * D, cd{0.0, 0.0});
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                for (int l = 0; l < D; ++l) {
                    const cd a = P0[(size_t)i * D + l], b = B[(size_t)l * D + j];
                    A[(size_t)i * D + j].re += a.re * b.re - a.im * b.im;
                    A[(size_t)i * D + j].im += a.re * b.im + a.im * b.re;
                }
    }
};
// P0 and its pattern P = P0 .!= 0 as column-major interleaved matrices
static void projector_matrices(const grape_desc *desc, std::vector<double> &P0, std::vector<double> &Pp) {
    const int D = desc->ndim;
    P0.assign(2 * (size_t)D * D, 0.0);
    Pp.assign(P0.size(), 0.0);
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i) {
            const size_t t = 2 * (i + (size_t)j * D);
            if (desc->projector) {
                P0[t] = desc->projector[t];
                P0[t + 1] = desc->projector[t + 1];
            } else if (i == j) {
                P0[t] = desc->projector_diag[i];
            }
            Pp[t] = (P0[t] != 0.0 || P0[t + 1] != 0.0) ? 1.0 : 0.0;
        }
}
// ... the setup from them (the caller's, or rotated ones: the symmetry-adapted sectors, whose pattern
// is the rotated P, not the pattern of the rotated P0)
static ProjectorSetup projector_from(const double *P0, const double *Pp, int D) {
    ProjectorSetup ps;
    ps.W.assign(D, 0.0);
    ps.P0.resize((size_t)D * D);
    std::vector<cd> B((size_t)D * D);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {  // row-major tiles
            const size_t t = 2 * (i + (size_t)j * D);
            ps.P0[(size_t)i * D + j] = cd{P0[t], P0[t + 1]};
            B[(size_t)i * D + j] = cd{Pp[t], Pp[t + 1]};
            if (i == j) {
                ps.trP += P0[t];
                ps.W[i] = P0[t];
                // the diagonal specialisation needs P = diag(P0 != 0) exactly
                const double pat = P0[t] != 0.0 ? 1.0 : 0.0;
                if (P0[t + 1] != 0.0 || Pp[t + 1] != 0.0 || std::fabs(Pp[t] - pat) > 1e-14) ps.general = true;
            } else if (P0[t] != 0.0 || P0[t + 1] != 0.0 || Pp[t] != 0.0 || Pp[t + 1] != 0.0) {
                ps.general = true;
            }
        }
    if (ps.general) ps.set_general(D, B);
    return ps;
}
static ProjectorSetup setup_projector(const grape_desc *desc) {
    std::vector<double> P0, Pp;
    projector_matrices(desc, P0, Pp);
    return projector_from(P0.data(), Pp.data(), desc->ndim);
}

// uploads the general-projector matrices and sets P.gen_proj / PA / PB / P0g
static int upload_projector(grape_plan *p, const ProjectorSetup &ps, DevProblem &P, size_t scratch_blocks) {
    P.gen_proj = ps.general ? 1 : 0;
    if (!ps.general) return GRAPE_OK;
    const size_t T = ps.A.size();
    if (p->mem.alloc(&p->d_PA, T) != hipSuccess || p->mem.alloc(&p->d_PB, T) != hipSuccess || p->mem.alloc(&p->d_P0g, T) != hipSuccess ||
        p->mem.alloc(&p->d_gpscr, scratch_blocks * grape_proj::kScratchSlots * T) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (general projector)");
    if (hipMemcpy(p->d_PA, ps.A.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_PB, ps.B.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->d_P0g, ps.P0.data(), T * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (general projector)");
    P.PA = p->d_PA;
    P.PB = p->d_PB;
    P.P0g = p->d_P0g;
    return GRAPE_OK;
}

// (SectorClass, SectorSetup, pack_sectors, sector_cost and find_sectors -- the layout rule -- live in
// grape_plan_setup.hpp, where tests/c/sectors_check.cpp runs them on the host.)
using grape_setup::SectorClass;
using grape_setup::SectorSetup;
using grape_setup::find_sectors;
using grape_setup::pack_sectors;
using grape_setup::sector_cost;

// Levels that cannot reach F or a derivative of it when no operator couples them to another level (find_sectors):
// diagonal projector (in the sector path's basis) without weight on the level, and every target operator free of
// entries beside the diagonal in the level's row and column.
static std::vector<char> idle_levels(const grape_desc *desc, const grape_desc &sdesc, const ProjectorSetup &sps) {
    const int D = desc->ndim;
    std::vector<char> idle(D, 0);
    if (sps.general || !desc->target_terms) return idle;
    for (int g = 0; g < D; ++g) idle[g] = sps.W[g] == 0.0;
    for (int k = 0; k < desc->n_target_terms; ++k) {
        const double *op = sdesc.ops + 2 * (size_t)desc->target_terms[k].op * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                if (i != j && (op[2 * (i + (size_t)j * D)] != 0.0 || op[2 * (i + (size_t)j * D) + 1] != 0.0))
                    idle[i] = idle[j] = 0;
    }
    return idle;
}

// Phase covariance of a sector class (grape_walk.hpp GAUGE): does every sector block obey
// H_w(x) = D(a x) H_w(0) D(a x)^dag, D(t) = diag(e^{i t N_j}), for the one control x?  Needs np = 1,
// H0 and every error source's terms free of x_add and of the step index (error sources are accepted:
// their terms must be covariant with the same charges, k_walk_img_gauge), and every term that reads x
// a cos / sin / cis of a x + b with one common a.  The charges come from the ratios of the blocks'
// entries at a small x to their values at x = 0 (N_j - N_k = n_jk, integer), propagated over each
// sector's coupling graph; the identity is then checked entry by entry at seven x values (a
// rotated basis -- the symmetry-adapted sectors -- is covered: the blocks are the rotated ones).
// On success N holds [nsec][S] charges >= 0 (0 on padding slots) and a the common factor.
static bool find_gauge(const grape_desc *desc, const grape_desc &sdesc, const SectorClass &sc, double &a,
                       std::vector<int> &N) {
    constexpr int kMaxCharge = 8;
    const int D = desc->ndim, S = sc.S, NE = desc->nerr;
    const size_t T = (size_t)D * D;
    if (desc->nparam != 1) return false;
    // the term lists: H0's, then every error source's (UnitaryCalculations.jl:67-97 adds
    // errval * Herror_e to H0: both must be covariant with the same charges)
    std::vector<std::pair<const grape_term *, int>> lists{{desc->h0_terms, desc->n_h0_terms}};
    for (int e = 0; e < NE; ++e)
        lists.push_back({desc->err_terms + desc->err_term_offsets[e],
                         desc->err_term_offsets[e + 1] - desc->err_term_offsets[e]});
    bool have_a = false;
    a = 1.0;
    for (const auto &l : lists)
        for (int t = 0; t < l.second; ++t) {
            const grape_term &tm = l.first[t];
            if (tm.var == 2 || tm.var == 3) return false;  // x_add or the step index
            if (tm.var != 1) continue;
            if (tm.func != 2 && tm.func != 3 && tm.func != 4) return false;  // x must enter as a phase
            if (!(tm.a != 0.0) || (have_a && tm.a != a)) return false;
            a = tm.a;
            have_a = true;
        }
    auto block = [&](int w, int li, double x, std::vector<std::complex<double>> &H) {
        H.assign((size_t)S * S, 0.0);
        for (int t = 0; t < lists[li].second; ++t) {
            const grape_term &tm = lists[li].first[t];
            const std::complex<double> c = term_value(tm, &x, nullptr, 0);  // (no x_add, no step index: checked above)
            for (int r = 0; r < S; ++r)
                for (int q = 0; q < S; ++q) {
                    const int gi = sc.sidx[(size_t)w * S + r], gj = sc.sidx[(size_t)w * S + q];
                    if (gi < 0 || gj < 0) continue;
                    const double *v = sdesc.ops + 2 * ((size_t)tm.op * T + gi + (size_t)gj * D);
                    H[(size_t)r * S + q] += c * std::complex<double>(v[0], v[1]);
                }
        }
    };
    N.assign((size_t)sc.nsec * S, 0);
    const double xs = 0.01 / std::fabs(a);
    const double probe[7] = {0.37, -1.3, 2.9, 7.77, -31.4, 0.001, 123.456};
    const int NL = (int)lists.size();
    std::vector<std::vector<std::complex<double>>> H0(NL), Hs(NL);
    std::vector<std::complex<double>> Hx;
    std::vector<double> tol(NL);
    for (int w = 0; w < sc.nsec; ++w) {
        // charge differences n_rq = N_r - N_q from every block's entries (H0's and the errors')
        std::vector<int> n((size_t)S * S, 0);
        std::vector<char> cpl((size_t)S * S, 0);
        for (int li = 0; li < NL; ++li) {
            block(w, li, 0.0, H0[li]);
            block(w, li, xs, Hs[li]);
            double hmax = 0.0;
            for (const auto &h : H0[li]) hmax = std::max(hmax, std::abs(h));
            for (const auto &h : Hs[li]) hmax = std::max(hmax, std::abs(h));
            tol[li] = 1e-13 * std::max(hmax, 1e-300);
            for (int r = 0; r < S; ++r)
                for (int q = 0; q < S; ++q) {
                    const std::complex<double> h0 = H0[li][(size_t)r * S + q], h1 = Hs[li][(size_t)r * S + q];
                    if (std::abs(h0) <= tol[li]) {
                        if (std::abs(h1) > tol[li]) return false;  // vanishes at x = 0 only: not a phase
                        continue;
                    }
                    const double m = std::arg(h1 / h0) / (a * xs);
                    const int nn = (int)std::lround(m);
                    if (std::fabs(m - nn) > 1e-6 || std::abs(nn) > kMaxCharge || (r == q && nn != 0)) return false;
                    if (cpl[(size_t)r * S + q] && n[(size_t)r * S + q] != nn) return false;
                    cpl[(size_t)r * S + q] = 1;
                    n[(size_t)r * S + q] = nn;
                }
        }
        std::vector<int> Nw(S, 0);  // charges by breadth-first search over the couplings
        std::vector<char> seen(S, 0);
        for (int s0 = 0; s0 < S; ++s0) {
            if (seen[s0]) continue;
            seen[s0] = 1;
            std::vector<int> stack{s0};
            while (!stack.empty()) {
                const int r = stack.back();
                stack.pop_back();
                for (int q = 0; q < S; ++q) {
                    if (!cpl[(size_t)r * S + q]) continue;
                    const int want = Nw[r] - n[(size_t)r * S + q];  // n_rq = N_r - N_q
                    if (!seen[q]) {
                        seen[q] = 1;
                        Nw[q] = want;
                        stack.push_back(q);
                    } else if (Nw[q] != want) {
                        return false;
                    }
                }
            }
        }
        const int lo = *std::min_element(Nw.begin(), Nw.end());
        for (int r = 0; r < S; ++r) {
            Nw[r] -= lo;
            if (Nw[r] > kMaxCharge) return false;
            N[(size_t)w * S + r] = Nw[r];
        }
        for (int li = 0; li < NL; ++li)
            for (double x : probe) {  // the identity itself, entry by entry, every block
                block(w, li, x, Hx);
                double hm = tol[li] * 1e13;
                for (const auto &h : Hx) hm = std::max(hm, std::abs(h));
                for (int r = 0; r < S; ++r)
                    for (int q = 0; q < S; ++q) {
                        const std::complex<double> ph = std::polar(1.0, a * x * (Nw[r] - Nw[q]));
                        if (std::abs(Hx[(size_t)r * S + q] - ph * H0[li][(size_t)r * S + q]) > 1e-12 * std::max(hm, 1e-300))
                            return false;
                    }
            }
    }
    return true;
}

// Symmetry-adapted sectors (grape_symmetry.hpp): the sector path's view of the problem in the basis
// V that splits the sparsity components further -- every operator V^dag O V (grape_desc layout;
// H0's and the error sources' operators with their off-block residue set to exact zeros, the others
// with rounding residue below 1e-15 of their largest entry snapped to 0), and the head's projector:
// P0' = V^dag P0 V with the pattern P' = V^dag P V of the ORIGINAL P0 (P = P0 .!= 0,
// FidelityCalculations.jl:47-51 -- the pattern of P0' is not P' in general).  On only when the
// rotated sectors cost less work (sum nsec S^3) than the permutation sectors.
struct SymSetup {
    bool on = false;
    grape_sym::Split split;
    std::vector<double> ops;  // n_ops * d * d complex, column-major interleaved
    ProjectorSetup ps;        // the rotated projector (A = P0' P', B = P' when not diagonal)
    grape_desc view(const grape_desc *d) const {
        grape_desc v = *d;
        v.ops = ops.data();
        return v;
    }
};
static std::vector<const double *> used_operators(const grape_desc *desc) {
    std::vector<const double *> u;
    const int D = desc->ndim;
    for (int t = 0; t < desc->n_h0_terms; ++t) u.push_back(desc->ops + 2 * (size_t)desc->h0_terms[t].op * D * D);
    const int ne = desc->nerr > 0 ? desc->err_term_offsets[desc->nerr] : 0;
    for (int t = 0; t < ne; ++t) u.push_back(desc->ops + 2 * (size_t)desc->err_terms[t].op * D * D);
    return u;
}
static void snap_residue(double *m, int D, double rel) {  // m: D x D interleaved
    double big = 0.0;
    for (int t = 0; t < 2 * D * D; ++t) big = std::max(big, std::fabs(m[t]));
    for (int t = 0; t < 2 * D * D; ++t)
        if (std::fabs(m[t]) <= rel * big) m[t] = 0.0;
}
static SymSetup symmetry_setup(const grape_desc *desc) {
    SymSetup sy;
    const int D = desc->ndim;
    if (D > GRAPE_MAX_SMALL_DIM || (desc->reserved[1] & (GRAPE_OPT_NO_SYMMETRY | GRAPE_OPT_NO_SECTORS))) return sy;
    sy.split = grape_sym::symmetry_split(D, used_operators(desc));
    if (!sy.split.rotated) return sy;
    const size_t T2 = 2 * (size_t)D * D;
    sy.ops.assign((size_t)desc->n_ops * T2, 0.0);
    std::vector<char> used(desc->n_ops, 0);
    for (int t = 0; t < desc->n_h0_terms; ++t) used[desc->h0_terms[t].op] = 1;
    const int ne = desc->nerr > 0 ? desc->err_term_offsets[desc->nerr] : 0;
    for (int t = 0; t < ne; ++t) used[desc->err_terms[t].op] = 1;
    for (int o = 0; o < desc->n_ops; ++o) {
        double *r = sy.ops.data() + (size_t)o * T2;
        grape_sym::rotate(sy.split, desc->ops + (size_t)o * T2, r);
        if (used[o])  // off the invariant blocks: zero by construction (checked in symmetry_split)
            for (int j = 0; j < D; ++j)
                for (int i = 0; i < D; ++i)
                    if (sy.split.block[i] != sy.split.block[j]) r[2 * (i + (size_t)j * D)] = r[2 * (i + (size_t)j * D) + 1] = 0.0;
        snap_residue(r, D, 1e-15);
    }
    // the projector P0 and its pattern P in the rotated basis
    std::vector<double> P0, Pp, P0r(T2), Ppr(T2);
    projector_matrices(desc, P0, Pp);
    grape_sym::rotate(sy.split, P0.data(), P0r.data());
    grape_sym::rotate(sy.split, Pp.data(), Ppr.data());
    snap_residue(P0r.data(), D, 1e-15);
    snap_residue(Ppr.data(), D, 1e-15);
    sy.ps = projector_from(P0r.data(), Ppr.data(), D);
    // worth it only when the rotated sectors are cheaper than the permutation ones
    const grape_desc rv = sy.view(desc);
    const SectorSetup rot = find_sectors(&rv, false), perm = find_sectors(desc, false);
    if (rot.cls.empty()) return sy;
    long crot = 0, cperm = 0;
    for (const SectorClass &c : rot.cls) crot += sector_cost(c);
    for (const SectorClass &c : perm.cls) cperm += sector_cost(c);
    if (perm.cls.empty()) cperm = (long)D * D * D;
    sy.on = crot < cperm;
    return sy;
}

extern "C" int grape_symmetry_basis(const grape_desc *desc, double *V, int *block) {
    if (!desc || !V || desc->ndim < 1 || desc->ndim > GRAPE_MAX_SMALL_DIM || !desc->ops || desc->n_ops < 1)
        return fail(GRAPE_ERR_INVALID, "grape_symmetry_basis: operator-basis descriptor with 1 <= ndim <= 12");
    const int D = desc->ndim;
    for (int t = 0; t < desc->n_h0_terms; ++t)
        if (desc->h0_terms[t].op != GRAPE_OP_FACTOR && (desc->h0_terms[t].op < 0 || desc->h0_terms[t].op >= desc->n_ops))
            return fail(GRAPE_ERR_INVALID, "bad op index");
    FactorSplit fs;  // factor terms carry no operator: the operator terms alone span the algebra
    split_factors(desc, fs);
    desc = &fs.plain;
    const grape_sym::Split sp = grape_sym::symmetry_split(D, used_operators(desc));
    for (size_t t = 0; t < sp.V.size(); ++t) {
        V[2 * t] = sp.V[t].real();
        V[2 * t + 1] = sp.V[t].imag();
    }
    if (block)
        for (int i = 0; i < D; ++i) block[i] = sp.block[i];
    return sp.rotated ? 1 : 0;
}

// the scalars of a plan's problem that come straight from the descriptor (every engine)
static void fill_problem_scalars(const grape_desc *desc, double trP, DevProblem &P) {
    P.D = desc->ndim;
    P.opts = desc->reserved[1];
    P.Nt = desc->ntimes;
    P.np = desc->nparam;
    P.na = desc->nadd;
    P.ne = desc->nerr;
    P.nx = desc->nparam * desc->ntimes + desc->nadd;
    P.n_h0 = desc->n_h0_terms;
    P.n_tgt = desc->n_target_terms;
    P.dt = desc->t0 / desc->ntimes;
    P.eps = desc->eps;
    P.eps2 = desc->eps2;
    P.inv_eps = 1.0 / desc->eps;
    P.inv_eps2sq = 1.0 / (desc->eps2 * desc->eps2);
    P.DD = trP * (trP + 1.0);
    P.Dtr = trP;
}

// the variant list of P's scalars (grape_plan_setup.hpp build_variants) and its layout into P
static std::vector<grape::VSpec> set_variants(DevProblem &P, int nxa, bool with_grad_variants) {
    grape_setup::Variants V = grape_setup::build_variants(P.np, nxa, P.ne, P.eps, P.eps2, with_grad_variants);
    P.off_dx = V.off_dx;
    P.off_dxa = V.off_dxa;
    P.off_dx2 = V.off_dx2;
    P.off_err = V.off_err;
    P.err_stride = V.err_stride;
    return std::move(V.vs);
}

// Device copies of the term lists, the error offsets and the variant list, and their pointers in P
// (d_err / d_err_off: plans with error sources; host-table plans upload no terms).  sfx / err_sfx name
// the engine in the messages.
static int upload_terms(grape_plan *p, const grape_desc *desc, int n_err_terms, const std::vector<grape::VSpec> &vs,
                        DevProblem &P, const char *sfx, const char *err_sfx) {
    const int ne = desc->nerr;
    bool ok = p->mem.alloc(&p->d_h0, std::max(desc->n_h0_terms, 0)) == hipSuccess &&
              p->mem.alloc(&p->d_tgt, std::max(desc->n_target_terms, 0)) == hipSuccess &&
              p->mem.alloc(&p->d_vs, vs.size()) == hipSuccess;
    if (ok && ne > 0)
        ok = p->mem.alloc(&p->d_err, (size_t)n_err_terms) == hipSuccess &&
             p->mem.alloc(&p->d_err_off, (size_t)ne + 1) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, std::string("device allocation failed") + sfx);
    if (hipMemcpy(p->d_vs, vs.data(), vs.size() * sizeof(grape::VSpec), hipMemcpyHostToDevice) != hipSuccess ||
        (!p->tables &&
         (hipMemcpy(p->d_h0, desc->h0_terms, desc->n_h0_terms * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->d_tgt, desc->target_terms, desc->n_target_terms * sizeof(Term), hipMemcpyHostToDevice) !=
              hipSuccess)))
        return fail(GRAPE_ERR_HIP, std::string("upload failed") + sfx);
    if (ne > 0 && !p->tables &&
        (hipMemcpy(p->d_err, desc->err_terms, n_err_terms * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(p->d_err_off, desc->err_term_offsets, ((size_t)ne + 1) * sizeof(int), hipMemcpyHostToDevice) !=
             hipSuccess))
        return fail(GRAPE_ERR_HIP, std::string("upload failed") + err_sfx);
    P.h0 = p->d_h0;
    P.tgt = p->d_tgt;
    P.vs = p->d_vs;
    P.err = p->d_err;
    P.err_off = p->d_err_off;
    return GRAPE_OK;
}

static int create_dense(const grape_desc *desc, grape_plan *p, bool xadd_dep, const ProjectorSetup &ps, int n_err_terms) {
    const int D = desc->ndim, ne = desc->nerr;
    // H0 (or Herror) reading x_add: without error sources k_dgrad adds each step's x_add variant (DP.nva);
    // with error sources (round 6) the variant table carries the x_add variants too (the small engine's
    // layout: nvg = np + na gradient parameters per step), k_dlocal / k_derr_grad write their per-step x_add
    // terms and k_dadd / k_dadd_err sum them onto the target's parts (UnitaryCalculations.jl:57-64, 87-95)
    // Hermitian H0: checked for every engine in choose_route (the dense no-interchange
    // solve relies on it too, grape_dense.hpp).  The error variants exponentiate
    // H0 + err Herror (err <= eps2): Hermitian error terms keep them inside that proof.
    for (int e = 0; e < ne; ++e)  // (each source on its own: its terms' sum must be Hermitian)
        if (int rc = check_hermitian_terms(desc, desc->err_terms + desc->err_term_offsets[e],
                                           desc->err_term_offsets[e + 1] - desc->err_term_offsets[e],
                                           "error source (dense engine)"))
            return rc;
    if (grape_dense::set_lds_limits() != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit (dense)");
    p->dense = true;
    grape_dense::DenseProblem &DP = p->DP;
    DevProblem &P = DP.P;
    fill_problem_scalars(desc, ps.trP, P);
    // propagator variants (the small engine's layout, grape_plan_setup.hpp build_variants): nominal alone
    // without error sources (k_dgrad exponentiates its variants in place)
    const int nva = xadd_dep ? desc->nadd : 0, nvg = desc->nparam + nva;
    const std::vector<grape::VSpec> vs = set_variants(P, nva, ne > 0);
    P.nv = (int)vs.size();
    P.nvg = ne > 0 ? nvg : P.np;
    DP.nz = P.nvg * (1 + ne) + ne;
    P.nz = DP.nz;
    DP.nva = xadd_dep ? P.na : 0;
    // scan chunking: ~sqrt(N_t) chunks balances the chunk chains against the carry chain
    int nc = (int)std::ceil(std::sqrt((double)P.Nt));
    DP.Lc = (P.Nt + nc - 1) / nc;
    DP.Nc = (P.Nt + DP.Lc - 1) / DP.Lc;
    const size_t IMG = grape_dense::kImgDoubles, MB = p->max_batch, NE = ne;
    std::vector<double> img((size_t)desc->n_ops * IMG), W(64, 0.0);
    for (int o = 0; o < desc->n_ops; ++o) to_dense_image(desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    for (int i = 0; i < D; ++i) W[i] = ps.W[i];
    bool ok = p->mem.alloc(&p->dn_opimg, img.size()) == hipSuccess && p->mem.alloc(&p->dn_W, (size_t)64) == hipSuccess &&
              p->mem.alloc(&p->dn_E, MB * P.Nt * P.nv * IMG) == hipSuccess && p->mem.alloc(&p->dn_Q, MB * P.Nt * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Carry, MB * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->dn_M, MB * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Mc, MB * DP.Nc * IMG) == hipSuccess &&
              p->mem.alloc(&p->dn_Z, ne ? 1 : MB * P.Nt * IMG) == hipSuccess &&
              p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_F, MB) == hipSuccess && p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess;
    if (ok && DP.nva > 0) ok = p->mem.alloc(&p->dn_Fadd, MB * P.Nt * DP.nva) == hipSuccess;
    if (ok && DP.nva > 0 && ne > 0) ok = p->mem.alloc(&p->dn_Fd2add, MB * NE * P.Nt * DP.nva) == hipSuccess;
    if (ok && ne > 0)
        ok = p->mem.alloc(&p->dn_Ub, MB * IMG) == hipSuccess && p->mem.alloc(&p->dn_Zl, MB * P.Nt * DP.nz * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Vc, MB * NE * DP.Nc * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Sx, MB * NE * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->dn_Tot, MB * NE * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_Me, MB * NE * IMG) == hipSuccess && p->mem.alloc(&p->dn_Mp, MB * NE * DP.Nc * IMG) == hipSuccess &&
             p->mem.alloc(&p->dn_B0, MB * NE * DP.Nc * IMG) == hipSuccess && p->mem.alloc(&p->d_Fd2, MB * NE) == hipSuccess &&
             p->mem.alloc(&p->d_Fd2dx, MB * NE * P.nx) == hipSuccess;
    if (ok && ps.general && ne == 0) ok = p->mem.alloc(&p->dn_Ub, MB * IMG) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense)");
    {  // row-major operator basis: the general-projector heads and the analysis kernels
        std::vector<cd> ops((size_t)desc->n_ops * D * D);
        grape_setup::to_tiles(desc->ops, desc->n_ops, D, nullptr, 1, D, ops.data(), nullptr);
        if (p->mem.alloc(&p->d_ops, ops.size()) != hipSuccess ||
            hipMemcpy(p->d_ops, ops.data(), ops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense, general projector)");
        P.ops = p->d_ops;
    }
    if (int rc = upload_projector(p, ps, P, MB * std::max<size_t>(NE, 1))) return rc;
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->dn_opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->dn_W, W.data(), 64 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (dense)");
    if (int rc = upload_terms(p, desc, n_err_terms, vs, P, " (dense)", " (dense error terms)")) return rc;
    DP.opimg = p->dn_opimg;
    DP.W = p->dn_W;
    P.W = p->dn_W;  // zero-padded to 64; the analysis kernels (expectation values) read W[0..D)
    p->P = P;  // the C ABI reads nx / np / ne from the plan's problem for every engine
    return GRAPE_OK;
}

// ---------------------------------------------------------------------------
// tiled engine plan (GRAPE_MAX_DENSE_DIM < d <= GRAPE_MAX_TILED_DIM; grape_tiled.hip)
// ---------------------------------------------------------------------------
// column-major interleaved d x d complex <-> zero-padded row-major planes (re, then im) of P x P
static void to_tiled_image(const double *src, int d, double *img) {
    const int P = grape_tiled::padded_dim(d);
    const size_t plane = (size_t)P * P;
    std::fill(img, img + 2 * plane, 0.0);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            img[(size_t)i * P + j] = src[2 * ((size_t)i + (size_t)j * d)];
            img[plane + (size_t)i * P + j] = src[2 * ((size_t)i + (size_t)j * d) + 1];
        }
}
static void from_tiled_image(const double *img, int d, double *dst) {
    const int P = grape_tiled::padded_dim(d);
    const size_t plane = (size_t)P * P;
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            dst[2 * ((size_t)i + (size_t)j * d)] = img[(size_t)i * P + j];
            dst[2 * ((size_t)i + (size_t)j * d) + 1] = img[plane + (size_t)i * P + j];
        }
}

// A tiled plan's workspace is sized by bytes, not by max_batch x everything: a quarter of the budget (at most
// kTiledSlabItems items) holds the slab of the exponential and of the gradient's eps-variants, the rest the
// evaluations of one pass (E and Q: 2 N_t images each, 512 MB at P = 128, N_t = 1 024).  A call of more
// evaluations than fit runs as several passes with identical arithmetic.
constexpr size_t kTiledBudgetBytes = (size_t)6 << 30;
constexpr size_t kTiledSlabItems = 1024;
constexpr size_t kTiledSlabImages = 9;  // A, A^2, A^3, A^4, two Horner buffers, E', Q_{k-1} M'_c, Y^dag

// slab of the exponential: `items` images in each of the six buffers, from one allocation
static hipError_t alloc_exp_slab(grape_setup::DevicePool &mem, size_t items, size_t img, grape_tiled::ExpSlab &X,
                                 double **extra, size_t n_extra) {
    double *base = nullptr;
    const hipError_t e = mem.alloc(&base, (6 + n_extra) * items * img);
    if (e != hipSuccess) return e;
    X.slab = (int)items;
    double **slots[6] = {&X.A, &X.A2, &X.A3, &X.A4, &X.B0, &X.B1};
    for (int i = 0; i < 6; ++i) *slots[i] = base + (size_t)i * items * img;
    for (size_t i = 0; i < n_extra; ++i) extra[i] = base + (6 + i) * items * img;
    return hipSuccess;
}

static int create_tiled(const grape_desc *desc, grape_plan *p, const ProjectorSetup &ps) {
    const int D = desc->ndim;
    p->tiled = true;
    grape_tiled::TiledProblem &TP = p->TP;
    DevProblem &P = TP.P;
    fill_problem_scalars(desc, ps.trP, P);
    const std::vector<grape::VSpec> vs = set_variants(P, 0, false);  // nominal only: the eps-variants are never kept
    P.nv = 1;
    P.nvg = P.np;
    TP.Pd = grape_tiled::padded_dim(D);
    // scan chunking: ~sqrt(N_t) chunks, as the dense engine
    const int nc = (int)std::ceil(std::sqrt((double)P.Nt));
    TP.Lc = (P.Nt + nc - 1) / nc;
    TP.Nc = (P.Nt + TP.Lc - 1) / TP.Lc;
    const size_t IMG = grape_tiled::image_doubles(D), imgB = IMG * sizeof(double);
    const size_t Nt = P.Nt, Nc = TP.Nc, nh = 1 + (size_t)P.na;
    const size_t eval_imgs = 2 * Nt + 3 * Nc + 4 + 2 * nh;
    size_t slab = std::min<size_t>(kTiledSlabItems, std::max<size_t>(1, kTiledBudgetBytes / 4 / (kTiledSlabImages * imgB)));
    slab = std::min(slab, (size_t)p->max_batch * Nt);
    const size_t slabB = slab * kTiledSlabImages * imgB;
    const size_t fit = kTiledBudgetBytes > slabB ? (kTiledBudgetBytes - slabB) / (eval_imgs * imgB) : 0;
    if (fit < 1)
        return fail(GRAPE_ERR_ALLOC, "tiled engine: one evaluation needs " + std::to_string(eval_imgs * imgB + slabB) +
                                         " bytes of workspace, the plan's budget is " + std::to_string(kTiledBudgetBytes));
    p->max_batch = (int)std::min<size_t>(p->max_batch, fit);
    const size_t MB = p->max_batch;
    grape_tiled::TiledBatch &B = p->TB;
    double *opimg = nullptr, *W = nullptr, *extra[3] = {nullptr, nullptr, nullptr};
    bool ok = p->mem.alloc(&opimg, (size_t)desc->n_ops * IMG) == hipSuccess && p->mem.alloc(&W, (size_t)TP.Pd) == hipSuccess &&
              p->mem.alloc(&B.E, MB * Nt * IMG) == hipSuccess && p->mem.alloc(&B.Q, MB * Nt * IMG) == hipSuccess &&
              p->mem.alloc(&B.Carry, MB * Nc * IMG) == hipSuccess && p->mem.alloc(&B.Tm, MB * Nc * IMG) == hipSuccess &&
              p->mem.alloc(&B.Mc, MB * Nc * IMG) == hipSuccess && p->mem.alloc(&B.U, MB * IMG) == hipSuccess &&
              p->mem.alloc(&B.M, MB * IMG) == hipSuccess && p->mem.alloc(&B.WK, MB * IMG) == hipSuccess &&
              p->mem.alloc(&B.T, MB * IMG) == hipSuccess && p->mem.alloc(&B.U0, MB * nh * IMG) == hipSuccess &&
              p->mem.alloc(&B.K, MB * nh * IMG) == hipSuccess && p->mem.alloc(&B.tau, 2 * MB) == hipSuccess &&
              p->mem.alloc(&B.ctl, MB * Nt) == hipSuccess && p->mem.alloc(&B.smax, (size_t)1) == hipSuccess &&
              alloc_exp_slab(p->mem, slab, IMG, B.X, extra, 3) == hipSuccess &&
              p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess && p->mem.alloc(&p->d_F, MB) == hipSuccess &&
              p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess && p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed (tiled)");
    B.Ev = extra[0];
    B.Ts = extra[1];
    B.Yd = extra[2];
    if (hipHostMalloc(reinterpret_cast<void **>(&p->tl_h_smax), sizeof(int), hipHostMallocDefault) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "pinned allocation failed (tiled)");
    B.h_smax = p->tl_h_smax;
    std::vector<double> img((size_t)desc->n_ops * IMG), Wp(TP.Pd, 0.0);
    for (int o = 0; o < desc->n_ops; ++o) to_tiled_image(desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    for (int i = 0; i < D; ++i) Wp[i] = ps.W[i];
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess ||
        hipMemcpy(opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(W, Wp.data(), Wp.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (tiled)");
    if (int rc = upload_terms(p, desc, 0, vs, P, " (tiled)", " (tiled)")) return rc;
    TP.opimg = opimg;
    TP.W = W;
    P.W = W;
    p->P = P;  // the C ABI reads nx / np / ne from the plan's problem for every engine
    return GRAPE_OK;
}

// ---------------------------------------------------------------------------
// plan creation, phase by phase (grape_plan_create calls them top to bottom; each returns a GRAPE_*
// code with the message set, and the caller frees the plan on any failure)
// ---------------------------------------------------------------------------
// Everything checkable without a device, in this order (a machine without one sees these codes
// before GRAPE_ERR_NO_DEVICE).
static int validate_desc(const grape_desc *desc, int *n_err_terms) {
    const int D = desc->ndim;
    const bool tables = (desc->reserved[0] & GRAPE_DESC_HOST_TABLES) != 0;
    if (D < 2 || desc->ntimes < 1 || desc->nparam < 1 || desc->nadd < 0 || desc->nerr < 0 ||
        (!tables && desc->n_ops < 1))
        return fail(GRAPE_ERR_INVALID, "bad dimensions in descriptor");
    if (D > GRAPE_MAX_TILED_DIM) return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_TILED_DIM");
    if (D > GRAPE_MAX_DENSE_DIM) {  // the tiled engine: what it does not serve is refused here, before any device work
        if (tables)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: closures (host tables) are served up to "
                                               "GRAPE_MAX_DENSE_DIM levels");
        if (desc->nerr > 0)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: error sources are served up to "
                                               "GRAPE_MAX_DENSE_DIM levels");
        if (desc->reserved[1] & GRAPE_OPT_GENERAL_H0)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: GRAPE_OPT_GENERAL_H0 is served up to "
                                               "GRAPE_MAX_DENSE_DIM levels (the tiled engine needs a Hermitian H0)");
        if (desc->n_h0_terms > grape_tiled::kMaxTerms || desc->n_target_terms > grape_tiled::kMaxTerms)
            return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: more than 256 H0 or target terms");
    }
    if (tables) {  // above GRAPE_MAX_SMALL_DIM: the general path with the dense exponential of the tables
        if (!desc->projector_diag && !desc->projector) return fail(GRAPE_ERR_INVALID, "missing projector");
    } else {
        if (desc->nerr > 0 && !desc->err_term_offsets) return fail(GRAPE_ERR_INVALID, "missing err_term_offsets");
        if (!desc->ops || !desc->h0_terms || desc->n_h0_terms < 1 || (!desc->projector_diag && !desc->projector) ||
            !desc->target_terms || desc->n_target_terms < 1)
            return fail(GRAPE_ERR_INVALID, "missing operator basis / terms / projector");
    }
    if (!(desc->t0 > 0) || !(desc->eps > 0)) return fail(GRAPE_ERR_INVALID, "t0 and eps must be positive");
    int rc;
    if (!tables && (rc = validate_terms(desc->h0_terms, desc->n_h0_terms, desc->n_ops, desc->nparam, desc->nadd, false, "H0")))
        return rc;
    if (!tables && (rc = validate_terms(desc->target_terms, desc->n_target_terms, desc->n_ops, desc->nparam, desc->nadd, true,
                             "target")))
        return rc;
    *n_err_terms = 0;
    if (desc->nerr > 0 && !tables) {
        for (int e = 0; e < desc->nerr; ++e)
            if (desc->err_term_offsets[e + 1] <= desc->err_term_offsets[e])
                return fail(GRAPE_ERR_INVALID, "each error source needs at least one term");
        if (desc->err_term_offsets[0] != 0) return fail(GRAPE_ERR_INVALID, "err_term_offsets[0] must be 0");
        *n_err_terms = desc->err_term_offsets[desc->nerr];
        for (int e = 0; e < desc->nerr; ++e)  // per source: a factor term never starts a source's range
            if ((rc = validate_terms(desc->err_terms + desc->err_term_offsets[e],
                                     desc->err_term_offsets[e + 1] - desc->err_term_offsets[e], desc->n_ops, desc->nparam,
                                     desc->nadd, false, "error source")))
                return rc;
    }
    if (!tables && D > GRAPE_MAX_SMALL_DIM) {  // product coefficients: the small engine's stored pipeline only
        bool any = false;
        for (int k = 0; k < desc->n_h0_terms; ++k) any = any || desc->h0_terms[k].op == GRAPE_OP_FACTOR;
        for (int k = 0; k < *n_err_terms; ++k) any = any || desc->err_terms[k].op == GRAPE_OP_FACTOR;
        if (any)
            return fail(GRAPE_ERR_UNSUPPORTED, "product coefficients (factor terms) are served up to GRAPE_MAX_SMALL_DIM "
                                               "levels; the dense and tiled engines do not take them");
    }
    return GRAPE_OK;
}

// the factor slots on the plan's device
static int upload_factors(grape_plan *p, const FactorSplit &fs) {
    if (!fs.any) return GRAPE_OK;
    if (p->mem.alloc(&p->d_fac_h0, fs.fac_h0.size()) != hipSuccess || p->mem.alloc(&p->d_fac_err, fs.fac_err.size()) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (product factors)");
    if (hipMemcpy(p->d_fac_h0, fs.fac_h0.data(), fs.fac_h0.size() * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess ||
        (!fs.fac_err.empty() &&
         hipMemcpy(p->d_fac_err, fs.fac_err.data(), fs.fac_err.size() * sizeof(Term), hipMemcpyHostToDevice) != hipSuccess))
        return fail(GRAPE_ERR_HIP, "upload failed (product factors)");
    p->FT.h0 = p->d_fac_h0;
    p->FT.err = p->d_fac_err;
    return GRAPE_OK;
}

// Which engine serves the descriptor (pure host logic).
struct Route {
    bool tables = false;      // GRAPE_DESC_HOST_TABLES: host-evaluated H and target tables
    bool general_h0 = false;  // the general path (materialised derivatives, LU inverse of the chain)
    bool pivot = false;       // ... over the dense engine's pivoted exponential (12 < d <= 64)
    bool xadd_dep = false;    // H0 or an error source reads x_add: x_add variants exist
    bool err_herm = true;     // Hermitian error generators
};
static int choose_route(const grape_desc *desc, int n_err_terms, Route &rt) {
    const int D = desc->ndim;
    rt.tables = (desc->reserved[0] & GRAPE_DESC_HOST_TABLES) != 0;
    rt.general_h0 = (desc->reserved[1] & GRAPE_OPT_GENERAL_H0) != 0;
    if (!rt.tables && !rt.general_h0)
        if (int rc = check_hermitian_terms(desc, desc->h0_terms, desc->n_h0_terms, "H0")) {
            if (rc != GRAPE_ERR_UNSUPPORTED || D > GRAPE_MAX_SMALL_DIM) return rc;
            rt.general_h0 = true;  // non-Hermitian H0: the general path serves it
        }
    // 12 < d <= 64 with the option: the general path over the dense engine's pivoted exponential
    // (operator bases: setup_pivot_dense, after the general-path problem; host tables:
    // launch_table_variants).  Without the option nothing changes: a non-Hermitian H0 or error source
    // is refused above.
    rt.pivot = rt.general_h0 && D > GRAPE_MAX_SMALL_DIM;
    if (D > GRAPE_MAX_DENSE_DIM) {  // the tiled engine (validate_desc refused closures, error sources, the general option)
        for (int k = 0; k < desc->n_h0_terms; ++k)
            if (desc->h0_terms[k].var == GRAPE_VAR_XADD)
                return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: H0 terms that read x_add are served up "
                                                   "to GRAPE_MAX_DENSE_DIM levels");
        if (desc->projector) {
            const size_t n = (size_t)D;
            for (size_t j = 0; j < n; ++j)
                for (size_t i = 0; i < n; ++i) {
                    const double *e = desc->projector + 2 * (i + j * n);
                    if ((i != j && (e[0] != 0.0 || e[1] != 0.0)) || (i == j && e[1] != 0.0))
                        return fail(GRAPE_ERR_UNSUPPORTED, "ndim > GRAPE_MAX_DENSE_DIM: a non-diagonal projector is "
                                                           "served up to GRAPE_MAX_DENSE_DIM levels");
                }
        }
    }
    // closures above the small engine: host tables through the general path (materialised
    // derivatives), each tabulated generator exponentiated by the dense engine (grape_dense.hip
    // launch_table_variants; the host checks that the tables are Hermitian)
    if (rt.tables && D > GRAPE_MAX_SMALL_DIM) rt.general_h0 = true;
    // host tables: H0 / Herror are opaque closures that may read x_add, so every x_add call
    // site of the reference is tabulated (UnitaryCalculations.jl:57-64, 87-95)
    rt.xadd_dep = rt.tables && desc->nadd > 0;
    for (int k = 0; k < (rt.tables ? 0 : desc->n_h0_terms); ++k)
        if (desc->h0_terms[k].var == 2) rt.xadd_dep = true;
    for (int k = 0; k < n_err_terms; ++k)
        if (desc->err_terms[k].var == 2) rt.xadd_dep = true;
    // Hermitian error generators (the image walk's exponential is skew-Hermitian, grape_walk.hpp)
    rt.err_herm = rt.tables || hermitian_terms(desc, desc->err_terms, n_err_terms) == 0;
    return GRAPE_OK;
}

// the plan's device, stream and pinned status word
static int open_plan(grape_plan *p, const grape_desc *desc, int device, const Route &rt) {
    for (int k = 0; k < (rt.tables ? 0 : desc->n_h0_terms); ++k)
        if (desc->h0_terms[k].var == GRAPE_VAR_TSTEP) p->uses_tstep = true;
    p->device = device;
    p->max_batch = desc->max_batch > 0 ? desc->max_batch : 256;
    p->pivot = rt.pivot;
    if (hipSetDevice(device) != hipSuccess) return fail(GRAPE_ERR_HIP, "hipSetDevice failed");
    if (hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "hipStreamCreate failed");
    p->stream = p->own_stream;
    if (hipHostMalloc(reinterpret_cast<void **>(&p->h_status), sizeof(int), hipHostMallocDefault) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "pinned allocation failed");
    *p->h_status = 0;
    return GRAPE_OK;
}

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

// The whole-matrix problem P: scalars, variant layout, scan chunking; then the sector layout (host).
static int setup_problem(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    const int D = desc->ndim;
    if (D <= GRAPE_MAX_SMALL_DIM && dispatch_lds_limits(D) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "cannot raise LDS limit");
    DevProblem &P = p->P;
    p->tables = b.rt.tables;
    p->general_h0 = b.rt.general_h0;
    b.n_ops = b.rt.tables ? 0 : desc->n_ops;
    fill_problem_scalars(desc, b.ps.trP, P);
    P.xadd_dep = b.rt.xadd_dep ? 1 : 0;
    // propagator variants of one step (grape_plan_setup.hpp build_variants), with the x_add variants
    // only if H0 reads x_add
    const int nad = b.rt.xadd_dep ? desc->nadd : 0;
    b.vs = set_variants(P, nad, true);
    // E stores every variant for the error-source pipeline; without error sources
    // only the nominal propagators are stored (k_expm_grad consumes the rest in place)
    // host tables: every variant's propagator is stored (k_grad reads them back)
    P.nv = (desc->nerr > 0 || b.rt.tables) ? (int)b.vs.size() : 1;
    P.nvg = desc->nparam + nad;
    P.nz = P.nvg * (1 + desc->nerr) + desc->nerr;
    // scan width: narrow once a launch can hold two evaluations per CU
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) == hipSuccess && prop.multiProcessorCount > 0)
        b.ncu = prop.multiProcessorCount;
    b.scan_override = desc->reserved[2];
    P.scan_waves = p->max_batch >= 2 * b.ncu ? kScanNarrow : kScanWide;
    if (b.scan_override == kScanNarrow || b.scan_override == kScanWide) P.scan_waves = b.scan_override;
    const int nc0 = std::min(P.scan_waves * (64 / D), P.Nt);
    P.L = (P.Nt + nc0 - 1) / nc0;
    P.nchunks = (P.Nt + P.L - 1) / P.L;
    P.sectors = 0;
    P.nsec = 1;
    P.sec_ops = 0;
    // symmetry-adapted sectors: the sector path (operators, head) in the rotated basis when that
    // splits the sectors further; the whole-matrix problem P keeps the caller's basis
    if (!b.rt.general_h0 && !b.rt.tables) b.sym = symmetry_setup(desc);
    b.sdesc = b.sym.on ? b.sym.view(desc) : *desc;
    if (!b.rt.general_h0) {
        const std::vector<char> idle = b.rt.tables ? std::vector<char>() : idle_levels(desc, b.sdesc, b.sps());
        b.ss = find_sectors(&b.sdesc, b.rt.tables, b.rt.tables ? nullptr : &idle);
    }
    p->symmetry = b.sym.on;
    return GRAPE_OK;
}

// The whole-matrix workspace (no rows when sectors or the general-H0 path run), the per-call buffers
// every path uses, and the uploads of operators, terms, weights and projector.
static int alloc_whole_matrix(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    DevProblem &P = p->P;
    const bool tables = b.rt.tables;
    const int D = P.D;
    const size_t FR = (!b.ss.cls.empty() || b.rt.general_h0) ? 0 : (size_t)p->max_batch;
    const size_t MB = p->max_batch, T = (size_t)D * D;
    std::vector<cd> ops((size_t)b.n_ops * T), opsT(ops.size());
    grape_setup::to_tiles(desc->ops, b.n_ops, D, nullptr, 1, D, ops.data(), opsT.data());
    bool ok = p->mem.alloc(&p->d_ops, ops.size()) == hipSuccess && p->mem.alloc(&p->d_opsT, opsT.size()) == hipSuccess &&
              p->mem.alloc(&p->d_W, (size_t)D) == hipSuccess &&
              p->mem.alloc(&p->d_E, FR * P.Nt * P.nv * T) == hipSuccess && p->mem.alloc(&p->d_Q, FR * P.Nt * T) == hipSuccess &&
              p->mem.alloc(&p->d_Mc, FR * P.nchunks * T) == hipSuccess && p->mem.alloc(&p->d_x, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_F, MB) == hipSuccess && p->mem.alloc(&p->d_Fdx, MB * P.nx) == hipSuccess &&
              p->mem.alloc(&p->d_part, MB * P.Nt * std::max(P.na, 1)) == hipSuccess &&
              p->mem.alloc(&p->d_tgt_part, MB * std::max(P.na, 1)) == hipSuccess &&
              p->mem.alloc(&p->d_ovf, FR * P.Nt * P.nv) == hipSuccess && p->mem.alloc(&p->d_ctrl, kCtrlInts) == hipSuccess &&
              p->mem.alloc(&p->d_sink, T) == hipSuccess;
    if (ok && P.ne == 0)
        ok = p->mem.alloc(&p->d_ovf2, FR * P.Nt * P.nvg) == hipSuccess &&
             p->mem.alloc(&p->d_ovf2_slots, FR * P.Nt * P.nvg * T) == hipSuccess;
    if (ok && (P.ne > 0 || b.ps.general))  // carries and U: the error path and the general-projector heads
        ok = p->mem.alloc(&p->d_Carry, FR * P.nchunks * T) == hipSuccess && p->mem.alloc(&p->d_Ub, FR * T) == hipSuccess;
    if (ok && P.ne > 0)
        ok = p->mem.alloc(&p->d_Me, FR * P.ne * P.nchunks * 3 * T) == hipSuccess &&
             p->mem.alloc(&p->d_Fd2, MB * P.ne) == hipSuccess && p->mem.alloc(&p->d_Fd2dx, MB * P.ne * P.nx) == hipSuccess &&
             p->mem.alloc(&p->d_Zl, FR * P.Nt * P.nz * T) == hipSuccess;
    if (ok && P.ne > 0 && P.xadd_dep)
        ok = p->mem.alloc(&p->d_part_err, MB * P.ne * P.Nt * P.na) == hipSuccess;
    if (ok && tables)
        ok = p->mem.alloc(&p->d_Htab, MB * P.Nt * P.nv * T) == hipSuccess &&
             p->mem.alloc(&p->d_U0tab, MB * (1 + P.na) * T) == hipSuccess;
    if (!ok) return fail(GRAPE_ERR_ALLOC, "device allocation failed");
    if (hipMemset(p->d_ctrl, 0, kCtrlInts * sizeof(int)) != hipSuccess) return fail(GRAPE_ERR_HIP, "memset failed");
    if (int rc = upload_terms(p, desc, b.n_err_terms, b.vs, P, "", "")) return rc;
    if ((!tables &&
         (hipMemcpy(p->d_ops, ops.data(), ops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->d_opsT, opsT.data(), opsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemcpy(p->d_W, b.ps.W.data(), D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed");
    if (int rc = upload_projector(p, b.ps, P, MB * std::max(P.ne, 1))) return rc;
    P.ops = p->d_ops;
    P.opsT = p->d_opsT;
    P.W = p->d_W;
    return GRAPE_OK;
}

// a diagonal projector's tiles A = diag(w), B = diag(w != 0) (or the given general ones) on the device
static hipError_t upload_projector_tiles(grape_plan *p, const std::vector<cd> &A, const std::vector<cd> &B, cd **dA, cd **dB) {
    hipError_t e = p->mem.alloc(dA, A.size());
    if (e == hipSuccess) e = p->mem.alloc(dB, B.size());
    if (e == hipSuccess) e = hipMemcpy(*dA, A.data(), A.size() * sizeof(cd), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*dB, B.data(), B.size() * sizeof(cd), hipMemcpyHostToDevice);
    return e;
}

// General H0: the fidelity heads need P0 P and P as tiles; the chain's inverses and the head's scratch.
static int setup_general_h0(PlanBuild &b) {
    if (!b.rt.general_h0) return GRAPE_OK;
    grape_plan *p = b.p;
    DevProblem &P = p->P;
    const size_t T = (size_t)P.D * P.D;
    if (!b.ps.general) {
        std::vector<cd> A, Bm;
        grape_setup::diag_projector_tiles(b.ps.W.data(), P.D, A, Bm);
        if (upload_projector_tiles(p, A, Bm, &p->d_PA, &p->d_PB) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (general H0)");
        P.PA = p->d_PA;
        P.PB = p->d_PB;
    }
    if (p->mem.alloc(&p->ud_Ci, (size_t)P.Nt * T) != hipSuccess || p->mem.alloc(&p->d_G, (1 + (size_t)P.ne) * T) != hipSuccess ||
        (P.D > grape_unitary::kMaxD && p->mem.alloc(&p->d_fscr, (size_t)grape_unitary::kFidTiles * T) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (general H0)");
    return GRAPE_OK;
}

// The head over the assembled U (SH): its projector tiles, weights and operators (the rotated ones
// with symmetry-adapted sectors), the fixed levels, and the choice of the diagonal head.
static int setup_sector_head(PlanBuild &b) {
    const grape_desc *desc = b.desc;
    grape_plan *p = b.p;
    const DevProblem &P = p->P;
    const ProjectorSetup &sps = b.sps();
    const SectorSetup &ss = b.ss;
    const bool sym = b.sym.on;
    const int D = P.D;
    std::vector<cd> A, Bm;
    grape_setup::diag_projector_tiles(sps.W.data(), D, A, Bm);
    if (sym && sps.general) {
        A = sps.A;
        Bm = sps.B;
    }
    if (sym) {  // the head's own rotated projector tiles, weights and operators
        std::vector<cd> rops((size_t)b.n_ops * D * D), ropsT(rops.size());
        grape_setup::to_tiles(b.sym.ops.data(), b.n_ops, D, nullptr, 1, D, rops.data(), ropsT.data());
        if (upload_projector_tiles(p, A, Bm, &p->d_PA_sym, &p->d_PB_sym) != hipSuccess ||
            p->mem.alloc(&p->d_W_sym, (size_t)D) != hipSuccess || p->mem.alloc(&p->d_ops_sym, rops.size()) != hipSuccess ||
            p->mem.alloc(&p->d_opsT_sym, ropsT.size()) != hipSuccess ||
            hipMemcpy(p->d_W_sym, sps.W.data(), D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->d_ops_sym, rops.data(), rops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->d_opsT_sym, ropsT.data(), ropsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (symmetry sectors)");
    } else if (!b.ps.general && upload_projector_tiles(p, A, Bm, &p->d_PA, &p->d_PB) != hipSuccess) {
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    }
    if (p->mem.alloc(&p->d_fixed, ss.fixed.size()) != hipSuccess ||
        (!ss.fixed.empty() && hipMemcpy(p->d_fixed, ss.fixed.data(), ss.fixed.size() * sizeof(int),
                                        hipMemcpyHostToDevice) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    grape_proj::SectorHead &H = p->SH;
    H.P = P;
    H.P.PA = sym ? p->d_PA_sym : p->d_PA;
    H.P.PB = sym ? p->d_PB_sym : p->d_PB;
    if (sym) {
        H.P.W = p->d_W_sym;
        H.P.ops = p->d_ops_sym;
        H.P.opsT = p->d_opsT_sym;
    }
    H.ncls = (int)ss.cls.size();
    H.fixed = p->d_fixed;
    H.nfixed = (int)ss.fixed.size();
    // diagonal projector and target, classes of <= 4 levels: the one-thread-per-evaluation head
    // (grape_projector.hip k_sec_head_diag)
    H.diag = !sps.general && !b.rt.tables && !(P.opts & GRAPE_OPT_GENERAL_HEAD);
    int rows = 0;  // the row-parallel head's lanes per evaluation (grape_projector.hip diag_group)
    for (const SectorClass &sc : ss.cls) {
        H.diag = H.diag && sc.S <= 4;
        rows += sc.nsec * sc.S;
    }
    H.diag = H.diag && rows <= 32;
    for (int k = 0; H.diag && k < desc->n_target_terms; ++k) {
        const double *op = b.sdesc.ops + 2 * (size_t)desc->target_terms[k].op * D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j)
                if (i != j && (op[2 * (i + (size_t)j * D)] != 0.0 || op[2 * (i + (size_t)j * D) + 1] != 0.0))
                    H.diag = 0;
    }
    return GRAPE_OK;
}

// Every decision about one sector class, into Ps (pure host logic; gauge_n: the class's charges, for
// alloc_class to upload; sops: the class's operator tiles [w][o][S][S]).
static void decide_class(const PlanBuild &b, const SectorClass &sc, const std::vector<cd> &sops, DevProblem &Ps,
                         std::vector<int> &gauge_n) {
    const grape_desc *desc = b.desc;
    const DevProblem &P = b.p->P;
    const int S = sc.S, ncu = b.ncu, scan_override = b.scan_override;
    const size_t TS = (size_t)S * S, MB = b.p->max_batch, R = MB * sc.nsec;  // workspace rows: sub-evaluations
    Ps = P;
    Ps.D = S;
    Ps.sectors = 1;
    Ps.nsec = sc.nsec;
    Ps.sec_ops = (size_t)b.n_ops * TS;
    Ps.gen_proj = 0;
    Ps.scan_waves = (long)R >= 8L * ncu ? kScanTiny : (long)R >= 2L * ncu ? kScanNarrow : kScanWide;
    if (scan_override == kScanTiny || scan_override == kScanNarrow || scan_override == kScanWide)
        Ps.scan_waves = scan_override;
    // chunk walks (grape_walk.hpp): classes of <= kWalkMaxD levels; with error sources the
    // image walk (k_walk_img), for any number of gradient parameters per step
    // (its exponential keeps A skew-Hermitian in compressed form: Hermitian error generators only;
    // a decay-rate error, -i e/2 |r><r|, keeps the stored-variant kernels)
    Ps.walk = (S <= grape::kWalkMaxD && (P.ne == 0 || b.rt.err_herm) && P.np <= grape::kWalkMaxNpA &&
               P.na <= grape::kWalkMaxNpA && !(P.opts & GRAPE_OPT_NO_WALK)) ? 1 : 0;
    // phase-covariant classes (grape_walk.hpp GAUGE): one exponential per walk lane
    // (with error sources: the phase-covariant image walk, one gradient parameter per step)
    double gauge_a = 1.0;
    Ps.gauge = (Ps.walk && (P.ne == 0 || (P.nvg == 1 && P.ne <= grape::kGaugeMaxE)) &&
                !(P.opts & GRAPE_OPT_NO_GAUGE) && find_gauge(desc, b.sdesc, sc, gauge_a, gauge_n)) ? 1 : 0;
    Ps.gauge_a = gauge_a;
    Ps.gauge_n = nullptr;
    Ps.gauge_ladder = Ps.gauge;
    for (size_t i = 0; Ps.gauge && i < gauge_n.size(); ++i)
        if (gauge_n[i] != (int)(i % (size_t)S)) Ps.gauge_ladder = 0;
    // error sources on a phase-covariant class: the lab-frame walks (no images, grape_walk.hpp,
    // GRAPE_WALK_ERR_LAB) when the base table's lanes fit one workgroup
    Ps.gauge_lab = (GRAPE_WALK_ERR_LAB && Ps.gauge && P.ne > 0 &&
                    sc.nsec * (1 + 2 * P.ne) <= grape::kLabBaseMaxLanes) ? 1 : 0;
    Ps.gauge_Et = nullptr;
    // the forward walk hands its propagators to the gradient walk (HBM, lane-minor) where the
    // exponential is the expensive part: the 4-level class (grape_walk.hpp; measured C2 6.04 ->
    // 6.52 M evals/s; for the 2-level class it lost, 0.72 -> 1.01 ms per pass)
    Ps.walk_store_e = Ps.walk && !Ps.gauge && P.ne == 0 && S >= grape::kWalkStoreMinD &&
                      !(P.opts & GRAPE_OPT_WALK_RECOMPUTE) ? 1 : 0;
    // latency-bound walk classes (fewer sub-evaluations than CUs, or the option): 16-wave scans,
    // half-length walks (grape_launch.hpp kScanLatency)
    // (not the error walks: the longer error scans cost more than the shorter walks save)
    if (Ps.walk && P.ne == 0 &&
        (scan_override == kScanLatency || (scan_override == 0 && (long)R < (long)ncu)))
        Ps.scan_waves = kScanLatency;
    // phase-covariant throughput classes: a step costs a few products instead of an
    // exponential, so longer chunks (fewer per-lane prologues and a shorter scan) can pay
    const int cdiv = (Ps.gauge && Ps.scan_waves == kScanTiny) ? GRAPE_GAUGE_CHUNK_DIV : 1;
    int ncs = std::max(1, std::min(Ps.scan_waves * (64 / S) / cdiv, P.Nt));
    if (Ps.gauge && Ps.scan_waves == kScanTiny && S == 3 && P.ne == 0)
        ncs = merged_chunk_count((long)MB, P.Nt, ncs, ncu);
    // the lab-frame error walks' throughput chunking (A/B knobs; 0: the formula above)
    if (Ps.gauge_lab && Ps.scan_waves == kScanTiny) {
        const int lc = S >= 4 ? GRAPE_LAB_CHUNKS4 : GRAPE_LAB_CHUNKS2;
        if (lc > 0) ncs = std::max(1, std::min(lc, P.Nt));
    }
    Ps.L = (P.Nt + ncs - 1) / ncs;
    Ps.nchunks = (P.Nt + Ps.L - 1) / Ps.L;
    // twin sectors (grape_walk.hpp TWIN): two walk sectors whose blocks of every operator H0
    // and the error sources use are identical, with the same padding -- one exponential
    // per step serves both (the 2-level Rydberg sectors at equal Rabi frequencies)
    Ps.twin = 0;
    // (S == 2 only: launch<2> is the one launcher that runs a class with two sectors per lane)
    if (Ps.walk && P.ne == 0 && sc.nsec == 2 && S == 2 && !Ps.walk_store_e && !(P.opts & GRAPE_OPT_NO_TWIN)) {
        bool same = true;
        for (int a = 0; a < S; ++a) same = same && ((sc.sidx[a] < 0) == (sc.sidx[S + a] < 0));
        std::vector<char> used(b.n_ops, 0);
        for (int t = 0; t < desc->n_h0_terms; ++t) used[desc->h0_terms[t].op] = 1;
        for (int o = 0; same && o < b.n_ops; ++o)
            if (used[o])
                same = std::memcmp(&sops[(size_t)o * TS], &sops[((size_t)b.n_ops + o) * TS], TS * sizeof(cd)) == 0;
        Ps.twin = same ? 1 : 0;
    }
}

// The workspace of one sector class (sb[cl]) as decide_class sized it, and the uploads of its
// charges, operator tiles and level indices.
static int alloc_class(PlanBuild &b, int cl, const std::vector<int> &gauge_n, const std::vector<cd> &sops,
                       const std::vector<cd> &sopsT) {
    grape_plan *p = b.p;
    const DevProblem &P = p->P;
    DevProblem &Ps = p->Ps[cl];
    const SectorClass &sc = b.ss.cls[cl];
    grape_plan::SecBuf &sb = p->sb[cl];
    const size_t TS = (size_t)sc.S * sc.S, MB = p->max_batch, R = MB * sc.nsec, nvg = P.nvg;
    if (Ps.gauge) {
        if (p->mem.alloc(&sb.gauge_n, gauge_n.size()) != hipSuccess) return fail(GRAPE_ERR_ALLOC, "device allocation failed (gauge)");
        if (hipMemcpy(sb.gauge_n, gauge_n.data(), gauge_n.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GRAPE_ERR_HIP, "upload failed (gauge)");
        Ps.gauge_n = sb.gauge_n;
    }
    const size_t ne = (size_t)P.ne, R2 = (P.ne > 0 || Ps.walk) ? 0 : R;  // k_expm_grad parking: no error sources only
    const size_t RE = Ps.walk ? 0 : R;  // the walks store no E / Q
    const size_t lanes_pad = (MB * Ps.nchunks + grape::kWalkBlockA - 1) / grape::kWalkBlockA * grape::kWalkBlockA;
    // stored propagators: D*D elements + the diagonal shift per (step, sector) (grape_walk.hpp kEwStride)
    if (Ps.walk_store_e && p->mem.alloc(&sb.Ew, (size_t)sc.nsec * Ps.L * (TS + 1) * lanes_pad) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sector walks)");
    if (Ps.walk && (p->mem.alloc(&sb.Tc, R * Ps.nchunks * TS) != hipSuccess ||
                    p->mem.alloc(&sb.wscr, 2 * (size_t)sc.nsec * lanes_pad * TS) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sector walks)");
    if (p->mem.alloc(&sb.E, RE * P.Nt * P.nv * TS) != hipSuccess || p->mem.alloc(&sb.Q, RE * P.Nt * TS) != hipSuccess ||
        p->mem.alloc(&sb.Mc, R * Ps.nchunks * TS) != hipSuccess || p->mem.alloc(&sb.Carry, R * Ps.nchunks * TS) != hipSuccess ||
        p->mem.alloc(&sb.Ub, R * TS) != hipSuccess || p->mem.alloc(&sb.Msec, R * TS) != hipSuccess ||
        p->mem.alloc(&sb.slots, R2 * P.Nt * nvg * TS) != hipSuccess || p->mem.alloc(&sb.ovf, RE * P.Nt * P.nv) != hipSuccess ||
        p->mem.alloc(&sb.ovf2, R2 * P.Nt * nvg) != hipSuccess || p->mem.alloc(&sb.part, R * P.Nt * nvg) != hipSuccess ||
        p->mem.alloc(&sb.sidx, sc.sidx.size()) != hipSuccess || p->mem.alloc(&sb.ops, sops.size()) != hipSuccess ||
        p->mem.alloc(&sb.opsT, sopsT.size()) != hipSuccess ||
        // (the image walk's images are lane-minor over its padded launch width: grape_walk.hpp img_index)
        p->mem.alloc(&sb.Zl, (Ps.walk ? (size_t)sc.nsec * Ps.L * lanes_pad : R * P.Nt) * (ne && !Ps.gauge_lab ? P.nz : 0) * TS) != hipSuccess ||
        p->mem.alloc(&sb.Wc, (Ps.walk ? R * ne * Ps.nchunks : 0) * TS) != hipSuccess ||
        p->mem.alloc(&sb.Me, R * ne * Ps.nchunks * 3 * TS) != hipSuccess || p->mem.alloc(&sb.TotS, R * ne * TS) != hipSuccess ||
        p->mem.alloc(&sb.MsecE, R * ne * TS) != hipSuccess || p->mem.alloc(&sb.part_err, R * ne * P.Nt * nvg) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (sectors)");
    if (hipMemcpy(sb.ops, sops.data(), sops.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sb.opsT, sopsT.data(), sopsT.size() * sizeof(cd), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sb.sidx, sc.sidx.data(), sc.sidx.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "upload failed (sectors)");
    Ps.ops = sb.ops;
    Ps.opsT = sb.opsT;
    return GRAPE_OK;
}

// E~ of every sector of a phase-covariant class, once per plan, into sb[cl].gEt: the merged walks' table
// (grape_walk.hpp gauge_prop_lds: the walks' own exponential, so the same bits as a per-workgroup
// copy) or, err: the lab-frame error walks' base table (1 + 2 ne matrices per sector).
static int fill_gauge_table(grape_plan *p, int cl, bool err) {
    DevProblem &Pc = p->Ps[cl];
    const size_t nbm = (size_t)Pc.nsec * (err ? 1 + 2 * Pc.ne : 1), TS = (size_t)Pc.D * Pc.D;
    grape_setup::DevicePool tmp;  // the fill's scratch
    cd *scr = nullptr, *&gEt = p->sb[cl].gEt;
    if (p->mem.alloc(&gEt, nbm * TS) != hipSuccess || tmp.alloc(&scr, nbm * 2 * TS) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, err ? "device allocation failed (gauge error base)" : "device allocation failed (gauge base)");
    const hipError_t e = err ? grape_walk::fill_gauge_err_base(Pc, Pc.nsec, scr, gEt, p->stream)
                             : grape_walk::fill_gauge_base(Pc, Pc.nsec, scr, gEt, p->stream);
    const hipError_t es = hipStreamSynchronize(p->stream);
    if (e != hipSuccess || es != hipSuccess)
        return fail(GRAPE_ERR_HIP, err ? "gauge error base fill failed" : "gauge base fill failed");
    Pc.gauge_Et = gEt;
    return GRAPE_OK;
}

// The two walk classes of the Rydberg layout in the pair kernels' order: pa the 4- (or 3-) level
// class, pb the 2-level one.
static void walk_pair_order(const grape_plan *p, int *pa, int *pb) {
    *pa = 0;
    *pb = 1;
    if (p->ncls == 2 && grape_walk::pair_ok(p->Ps[1], p->Ps[0])) std::swap(*pa, *pb);
}

// throughput passes of the Rydberg layout with phase-covariant classes: class B (2 levels)
// takes class A's chunking (fewer, longer chunks: its buffers, sized for its own count,
// suffice) so that one lane can walk both (merged walks; GRAPE_OPT_NO_MERGE launches the
// same chunking per class)
static int setup_merge(PlanBuild &b) {
    grape_plan *p = b.p;
    if (p->ncls != 2) return GRAPE_OK;
    const DevProblem &P = p->P;
    int pa, pb;
    walk_pair_order(p, &pa, &pb);
    DevProblem &A = p->Ps[pa], &Bq = p->Ps[pb];
    if (!(grape_walk::pair_ok(A, Bq) && A.D == 3 && A.gauge && Bq.gauge && A.gauge_a == Bq.gauge_a &&
          A.scan_waves == kScanTiny && Bq.scan_waves == kScanTiny && A.nchunks <= Bq.nchunks && P.np == 1 && P.na <= 1))
        return GRAPE_OK;
    Bq.L = A.L;
    Bq.nchunks = A.nchunks;
    p->merged = !(P.opts & GRAPE_OPT_NO_MERGE) && grape_walk::merged_ok(A, Bq);
    p->merge_pa = pa;
    for (int cl = 0; p->merged && cl < 2; ++cl)  // E~ of both classes for the merged walks' scalar loads
        if (int rc = fill_gauge_table(p, cl, false)) return rc;
    // The rank-one gradient walk (grape_walk.hpp merged_step_grad_r1, GRAPE_OPT_NO_RANK1): the diagonal head
    // writes row r of a sector's M block with the factor W[g_r] (grape_projector.hip diag_row, pass 1), so a
    // sector with exactly one weighted level (the head's W and level order: the rotated ones with
    // symmetry-adapted sectors) has M = e_c m^T.  Every sector of both classes must be such, and summed twins
    // must hold that level at one in-sector index; anything else keeps the matrix walk.
    const std::vector<double> &W = b.sps().W;
    bool r1 = p->merged && p->SH.diag && !(P.opts & GRAPE_OPT_NO_RANK1);
    for (int cl = 0; cl < 2; ++cl) {
        const SectorClass &sc = b.ss.cls[cl];
        DevProblem &Pc = p->Ps[cl];
        Pc.rank1 = Pc.rank1_c[0] = Pc.rank1_c[1] = 0;
        r1 = r1 && sc.nsec <= 2;
        for (int w = 0; r1 && w < sc.nsec; ++w) {
            int n = 0;
            for (int r = 0; r < sc.S; ++r) {
                const int g = sc.sidx[(size_t)w * sc.S + r];
                if (g >= 0 && W[g] != 0.0) {
                    Pc.rank1_c[w] = r;
                    ++n;
                }
            }
            r1 = r1 && n == 1;
        }
        if (Pc.twin && grape_walk::merged_twin_sum()) r1 = r1 && Pc.rank1_c[0] == Pc.rank1_c[1];
    }
    A.rank1 = Bq.rank1 = r1 ? 1 : 0;
    // the wide pass: its U blocks and alphas take the chunk totals' and carries' buffers (alloc_class: at least
    // max_batch x nchunks tiles per sector of either class, class B's sized for its own, larger, chunk count)
    const long wide = (long)p->max_batch * A.nchunks;
    if (r1 && !(P.opts & GRAPE_OPT_NO_WIDE) && grape_walk::wide_ok(A, Bq) && wide * 2 <= (long)INT_MAX) p->wide = (int)wide;
    return GRAPE_OK;
}

// latency-bound calls of the Rydberg layout with phase-covariant classes: one workgroup per
// evaluation (grape_eval1.hip), with E~ of each class computed here once
static int setup_eval1(grape_plan *p) {
    const grape_proj::SectorHead &H = p->SH;
    if (p->ncls != 2 || (long)p->max_batch > kEval1MaxBatch || (p->P.opts & GRAPE_OPT_NO_EVAL1)) return GRAPE_OK;
    int pa, pb;
    walk_pair_order(p, &pa, &pb);
    const DevProblem &A = p->Ps[pa], &Bq = p->Ps[pb];
    if (!grape_walk::pair_ok(A, Bq) || !grape_eval1::eligible(A, Bq, H)) return GRAPE_OK;
    if (p->mem.alloc(&p->d_e1_Et, (size_t)A.D * A.D + 8) != hipSuccess ||
        p->mem.alloc(&p->d_e1_scr, (size_t)2 * 2 * 16) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (eval1)");
    const hipError_t e = grape_eval1::prepare(A, Bq, p->d_e1_Et, p->d_e1_Et + (size_t)A.D * A.D, p->d_e1_scr, p->stream);
    if (e != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "eval1 preparation failed");
    p->e1 = true;
    p->e1_pa = pa;
    const size_t tb = grape_eval1::tab_bytes(A, Bq, H);
    if (p->mem.alloc(&p->d_e1_tab, std::max<size_t>(tb, 16)) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (eval1)");
    if (grape_eval1::tab_build(eval1_args(p, nullptr, nullptr, nullptr), p->d_e1_tab, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess)
        return fail(GRAPE_ERR_HIP, "eval1 table build failed");
    const char *tr = std::getenv("GRAPE_EVAL1_TRACE");
    if (tr && tr[0] == '1' &&
        (hipHostMalloc(reinterpret_cast<void **>(&p->e1_trace), 32 * sizeof(long long), hipHostMallocDefault) != hipSuccess ||
         hipHostGetDevicePointer(reinterpret_cast<void **>(&p->e1_trace_d), p->e1_trace, 0) != hipSuccess))
        return fail(GRAPE_ERR_ALLOC, "eval1 trace buffer");
    return GRAPE_OK;
}

// The sector problems of every class and the head over the assembled U; then the merged walks, the
// one-workgroup kernel and the auxiliary stream of two-class plans.
static int setup_sectors(PlanBuild &b) {
    if (b.ss.cls.empty()) return GRAPE_OK;
    grape_plan *p = b.p;
    if (int rc = setup_sector_head(b)) return rc;
    grape_proj::SectorHead &H = p->SH;
    for (int cl = 0; cl < (int)b.ss.cls.size(); ++cl) {
        const SectorClass &sc = b.ss.cls[cl];
        if (dispatch_lds_limits(sc.S) != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit");
        std::vector<cd> sops((size_t)sc.nsec * b.n_ops * sc.S * sc.S), sopsT(sops.size());  // (rotated) operator blocks
        grape_setup::to_tiles(b.sdesc.ops, b.n_ops, p->P.D, sc.sidx.data(), sc.nsec, sc.S, sops.data(), sopsT.data());
        std::vector<int> gauge_n;
        decide_class(b, sc, sops, p->Ps[cl], gauge_n);
        if (int rc = alloc_class(b, cl, gauge_n, sops, sopsT)) return rc;
        // the lab-frame error walks' base table, once per plan
        if (p->Ps[cl].gauge_lab)
            if (int rc = fill_gauge_table(p, cl, true)) return rc;
        const grape_plan::SecBuf &sb = p->sb[cl];
        H.S[cl] = sc.S;
        H.nsec[cl] = sc.nsec;
        H.sidx[cl] = sb.sidx;
        H.Ub[cl] = sb.Ub;
        H.Msec[cl] = sb.Msec;
        H.TotS[cl] = sb.TotS;
        H.MsecE[cl] = sb.MsecE;
    }
    p->ncls = (int)b.ss.cls.size();
    if (int rc = setup_merge(b)) return rc;
    if (int rc = setup_eval1(p)) return rc;
    if (p->e1) p->wide = 0;  // (one workgroup per evaluation serves every call of such a plan)
    if (p->ncls == 2 && (hipStreamCreateWithFlags(&p->aux_stream, hipStreamNonBlocking) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess))
        return fail(GRAPE_ERR_HIP, "cannot create the auxiliary stream");
    return GRAPE_OK;
}

// 12 < d <= 64 with GRAPE_OPT_GENERAL_H0, operator basis: the operator images and the problem
// ud_propagators_dev's dense branch exponentiates from (k_dexp_piv over the variant list): the terms,
// scalars and x layout are the general path's
static int setup_pivot_dense(PlanBuild &b) {
    if (!b.rt.pivot || b.rt.tables) return GRAPE_OK;
    grape_plan *p = b.p;
    const int D = p->P.D;
    if (grape_dense::set_lds_limits() != hipSuccess) return fail(GRAPE_ERR_HIP, "cannot raise LDS limit (dense)");
    const size_t IMG = grape_dense::kImgDoubles;
    std::vector<double> img((size_t)b.n_ops * IMG);
    for (int o = 0; o < b.n_ops; ++o) to_dense_image(b.desc->ops + 2 * (size_t)o * D * D, D, img.data() + o * IMG);
    if (p->mem.alloc(&p->dn_opimg, img.size()) != hipSuccess ||
        hipMemcpy(p->dn_opimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (dense operator images)");
    p->DP = grape_dense::DenseProblem{};
    p->DP.P = p->P;
    p->DP.opimg = p->dn_opimg;
    p->dense = true;
    return GRAPE_OK;
}

static int create_small(PlanBuild &b) {
    if (int rc = setup_problem(b)) return rc;
    if (int rc = alloc_whole_matrix(b)) return rc;
    if (int rc = setup_general_h0(b)) return rc;
    if (int rc = setup_sectors(b)) return rc;
    return setup_pivot_dense(b);
}

// A fatal signal raised by code inside the library names its native frames on stderr before the
// previous handler (Python's faulthandler, or the default action) runs.  Opt-in: the Python binding
// installs it (grape_install_fault_handler, _capi.lib(); GRAPE_NO_SIGNAL_HANDLER=1 skips that), never
// a load-time constructor -- a host such as Julia uses SIGSEGV itself (GC safepoints, stack probes),
// so the library leaves every process's handlers alone unless asked.  A signal whose faulting PC lies
// outside libgrape's own text goes straight to the displaced handler (called in place, or, for the
// default action, reinstated so that the instruction faults again into it); only a fault inside the
// library prints the frames first.  backtrace() is called once at install time so that the unwinder
// is resolved before any signal (it is not async-signal-safe on its first call).
namespace {
struct sigaction g_prev_sig[2];
const int kFatalSigs[2] = {SIGSEGV, SIGBUS};
uintptr_t g_text_lo = 0, g_text_hi = 0;  // libgrape's executable segments (host code)
bool g_handler_installed = false;

int find_text(struct dl_phdr_info *info, size_t, void *base) {
    if (info->dlpi_addr != (uintptr_t)base) return 0;
    for (int i = 0; i < info->dlpi_phnum; ++i) {
        const ElfW(Phdr) &ph = info->dlpi_phdr[i];
        if (ph.p_type != PT_LOAD || !(ph.p_flags & PF_X)) continue;
        const uintptr_t lo = info->dlpi_addr + ph.p_vaddr, hi = lo + ph.p_memsz;
        if (!g_text_lo || lo < g_text_lo) g_text_lo = lo;
        if (hi > g_text_hi) g_text_hi = hi;
    }
    return 1;
}

void chain_previous(int sig, siginfo_t *si, void *uc) {
    for (int i = 0; i < 2; ++i) {
        if (kFatalSigs[i] != sig) continue;
        const struct sigaction &prev = g_prev_sig[i];
        if ((prev.sa_flags & SA_SIGINFO) && prev.sa_sigaction) {
            prev.sa_sigaction(sig, si, uc);
        } else if (prev.sa_handler != SIG_DFL && prev.sa_handler != SIG_IGN) {
            prev.sa_handler(sig);
        } else {
            sigaction(sig, &prev, nullptr);  // returning re-raises the fault into the default action
        }
    }
}

void grape_fatal_signal(int sig, siginfo_t *si, void *uc) {
    uintptr_t pc = 0;
#if defined(__x86_64__)
    if (uc) pc = (uintptr_t) static_cast<ucontext_t *>(uc)->uc_mcontext.gregs[REG_RIP];
#endif
    if (pc >= g_text_lo && pc < g_text_hi) {
        static const char head[] = "\n[libgrape] fatal signal inside libgrape; native frames (innermost first):\n";
        (void)!write(2, head, sizeof head - 1);
        void *frames[64];
        const int n = backtrace(frames, 64);
        backtrace_symbols_fd(frames, n, 2);
    }
    chain_previous(sig, si, uc);
}
}  // namespace

extern "C" int grape_install_fault_handler(void) {
    if (g_handler_installed) return 1;
    Dl_info di;
    if (!dladdr(reinterpret_cast<void *>(&grape_install_fault_handler), &di) || !di.dli_fbase) return 0;
    dl_iterate_phdr(find_text, di.dli_fbase);
    if (!g_text_hi) return 0;
    void *warm[2];
    (void)backtrace(warm, 2);
    struct sigaction sa {};
    sa.sa_sigaction = grape_fatal_signal;
    sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigemptyset(&sa.sa_mask);
    for (int i = 0; i < 2; ++i) sigaction(kFatalSigs[i], &sa, &g_prev_sig[i]);
    g_handler_installed = true;
    return 1;
}

#ifndef GRAPE_BUILD_ID
#define GRAPE_BUILD_ID "unversioned"
#endif

extern "C" {

int grape_abi_version(void) { return GRAPE_ABI_VERSION; }

const char *grape_build_id(void) { return GRAPE_BUILD_ID; }

const char *grape_last_error(void) { return g_err.c_str(); }

int grape_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int grape_plan_create(const grape_desc *full, int device, grape_plan **out) {
    if (!full || !out) return fail(GRAPE_ERR_INVALID, "null argument");
    *out = nullptr;
    int n_err_terms = 0;
    Route rt;
    if (int rc = validate_desc(full, &n_err_terms)) return rc;
    // product coefficients: everything below sees the plain descriptor (operator terms only)
    FactorSplit fs;
    split_factors(full, fs);
    const grape_desc *desc = &fs.plain;
    if (fs.any) n_err_terms = (int)fs.err.size();
    if (int rc = choose_route(desc, n_err_terms, rt)) return rc;
    if (fs.reads_xadd) rt.xadd_dep = true;  // a factor on x_add: the x_add variants exist
    const ProjectorSetup ps = setup_projector(desc);
    if (!(ps.trP > 0)) return fail(GRAPE_ERR_INVALID, "projector trace must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(GRAPE_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= ndev) return fail(GRAPE_ERR_NO_DEVICE, "device index out of range");

    grape_plan *p = new grape_plan();
    int rc = open_plan(p, desc, device, rt);
    if (fs.reads_tstep) p->uses_tstep = true;
    if (!rc && desc->ndim > GRAPE_MAX_DENSE_DIM) {
        rc = create_tiled(desc, p, ps);
    } else if (!rc && desc->ndim > GRAPE_MAX_SMALL_DIM && !rt.tables && !rt.pivot) {
        rc = create_dense(desc, p, rt.xadd_dep, ps, n_err_terms);
    } else if (!rc) {
        PlanBuild b{desc, p, rt, ps, n_err_terms};
        rc = create_small(b);
        if (!rc) rc = upload_factors(p, fs);
    }
    if (rc) {  // (the message is set; the plan's pool returns whatever was allocated so far)
        free_plan(p);
        return rc;
    }
    *out = p;
    return GRAPE_OK;
}

int grape_plan_sectors(grape_plan *p, int *sector_dims, int *nsectors, int max_classes) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    const int n = p->ncls > 0 ? p->ncls : 1;
    for (int c = 0; c < n && c < max_classes; ++c) {
        if (sector_dims) sector_dims[c] = p->ncls ? p->Ps[c].D : (p->dense ? p->DP.P.D : p->P.D);
        if (nsectors) nsectors[c] = p->ncls ? p->Ps[c].nsec : 1;
    }
    return n;
}

int grape_plan_sector_info(grape_plan *p, int *twin, int *symmetric, int max_classes) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    const int n = p->ncls > 0 ? p->ncls : 1;
    for (int c = 0; c < n && c < max_classes; ++c)
        if (twin) twin[c] = p->ncls ? p->Ps[c].twin : 0;
    if (symmetric) *symmetric = p->symmetry ? 1 : 0;
    return n;
}

int grape_plan_gauge_info(grape_plan *p, int *gauge, int max_classes) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    const int n = p->ncls > 0 ? p->ncls : 1;
    for (int c = 0; c < n && c < max_classes; ++c)
        if (gauge) gauge[c] = p->ncls ? (p->Ps[c].gauge ? (p->Ps[c].gauge_ladder ? 2 : 1) : 0) : 0;
    return n;
}

int grape_plan_eval1(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    return p->e1 ? 1 : 0;
}

int grape_plan_rank1(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    return p->merged && p->Ps[0].rank1 && p->Ps[1].rank1 ? 1 : 0;
}

int grape_plan_wide(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    return p->wide;
}

void grape_plan_destroy(grape_plan *plan) { free_plan(plan); }

void *grape_plan_stream(grape_plan *plan) { return plan ? (void *)plan->stream : nullptr; }

int grape_plan_set_stream(grape_plan *plan, void *stream) {
    if (!plan) return fail(GRAPE_ERR_INVALID, "null plan");
    plan->stream = stream ? static_cast<hipStream_t>(stream) : plan->own_stream;
    return GRAPE_OK;
}

// every closure call site of UnitaryCalculations.jl:45-95 as a propagator variant, in the
// layout of grape_unitary::UProblem (= the host-table layout of grape_fidelity_grad_tables
// with every x_add site present), and the assembly's slots per step
static grape_setup::Variants ud_variants(const DevProblem &P0) {
    return grape_setup::build_variants(P0.np, P0.na, P0.ne, P0.eps, P0.eps2, true);
}
static int ud_nslots(const DevProblem &P0) { return P0.np + P0.na + P0.ne + P0.ne * (P0.np + P0.na); }
static std::vector<grape::VSpec> ud_setup(grape_plan *p, grape_unitary::UProblem &UP, grape_unitary::UBuffers &UB);
static int ud_alloc(grape_plan *p);
static int ud_propagators_dev(grape_plan *p, const double *d_x, int nv, const cd *d_Htab);
static int enqueue_general(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                           double *d_Fd2dx, const KMark &mk);

// the dense engine's view of one launch (plan workspaces + the call's inputs and outputs)
static grape_dense::DenseBatch dense_batch(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx,
                                           double *d_Fd2, double *d_Fd2dx) {
    grape_dense::DenseBatch DB{};
    DB.nb = nb;
    DB.x = d_x;
    DB.E = p->dn_E;
    DB.Q = p->dn_Q;
    DB.Carry = p->dn_Carry;
    DB.M = p->dn_M;
    DB.Mc = p->dn_Mc;
    DB.Z = p->dn_Z;
    DB.Ub = p->dn_Ub;
    DB.Zl = p->dn_Zl;
    DB.Vc = p->dn_Vc;
    DB.Sx = p->dn_Sx;
    DB.Tot = p->dn_Tot;
    DB.Me = p->dn_Me;
    DB.Mp = p->dn_Mp;
    DB.B0 = p->dn_B0;
    DB.Fd2 = d_Fd2;
    DB.Fd2dx = d_Fd2dx;
    DB.F = d_F;
    DB.Fdx = d_Fdx;
    DB.Fadd = p->dn_Fadd;
    DB.Fd2add = p->dn_Fd2add;
    DB.status = p->d_ctrl + 2;
    DB.mstats = nullptr;
    DB.gp_scr = p->d_gpscr;
    return DB;
}

static grape_eval1::Args eval1_args(const grape_plan *p, const double *x, double *F, double *Fdx) {
    grape_eval1::Args A{};
    A.PA = p->Ps[p->e1_pa];
    A.PB = p->Ps[1 - p->e1_pa];
    A.H = p->SH;
    A.EtA = p->d_e1_Et;
    A.EtB = p->d_e1_Et + (size_t)A.PA.D * A.PA.D;
    A.x = x;
    A.F = F;
    A.Fdx = Fdx;
    A.a_first = p->e1_pa == 0 ? 1 : 0;
    A.trace = p->e1_trace_d;
    A.tab = p->d_e1_tab;
    return A;
}

// One launch sequence of `nb` evaluations on the plan's stream over workspace rows
// [0, nb).  The caller copies the status word afterwards.
static KMark profiling_mark(grape_plan *p) {  // per-kernel event pairs on the stream being enqueued (profiling on)
    KMark mk;
    if (p->profiling) {
        mk.ctx = p;
        mk.fn = [](void *ctx, int k, int phase) {
            grape_plan *pl = static_cast<grape_plan *>(ctx);
            hipEvent_t e = pl->get_event();
            if (!e) return;
            (void)hipEventRecord(e, pl->cur_stream);
            if (phase == 0) {
                pl->pending.push_back({k, e, nullptr});
            } else {
                pl->pending.back().b = e;
            }
        };
    }
    return mk;
}

// One wide pass (grape_walk_api.hpp launch_merged_wide) of nb == p->wide evaluations on the caller's buffers:
// the forward state walk, the head (alpha per sector instead of the M blocks), the time-reversed gradient walk.
// The U blocks and the alphas live in the chunk totals' and the carries' buffers, which hold exactly
// max_batch x nchunks tiles per sector and are idle here (no chunks); later chunked passes follow in stream order.
static int enqueue_wide(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx) {
    hipStream_t st = p->stream;
    p->cur_stream = st;
    const KMark mk = profiling_mark(p);
    const int ma = p->merge_pa, mb = 1 - ma;
    DevProblem Pw[2] = {p->Ps[ma], p->Ps[mb]};
    DevBatch Bw[2]{};
    grape_proj::SectorHead H = p->SH;
    for (int i = 0; i < 2; ++i) {
        const int cl = i == 0 ? ma : mb;
        const grape_plan::SecBuf &sb = p->sb[cl];
        Pw[i].nchunks = 1;
        Pw[i].L = Pw[i].Nt;
        Bw[i].nb = nb * Pw[i].nsec;
        Bw[i].x = d_x;
        Bw[i].F = d_F;
        Bw[i].Fdx = d_Fdx;
        Bw[i].Ub = sb.Tc;
        Bw[i].Msec = sb.Carry;
        Bw[i].status = p->d_ctrl + 2;
        Bw[i].sink = p->d_sink;
        H.Ub[cl] = sb.Tc;
        H.Msec[cl] = sb.Carry;
    }
    H.alpha = 1;
    H.x = d_x;
    H.F = d_F;
    H.Fdx = d_Fdx;
    H.tgt_part = p->d_tgt_part;
    mk(GRAPE_KERNEL_WALK_FWD, 0);
    HIPCHECK(grape_walk::launch_merged_wide(0, Pw[0], Bw[0], Pw[1], Bw[1], st));
    mk(GRAPE_KERNEL_WALK_FWD, 1);
    mk(GRAPE_KERNEL_SCAN, 0);
    HIPCHECK(grape_proj::launch_sector_head(H, nb, st));
    mk(GRAPE_KERNEL_SCAN, 1);
    mk(GRAPE_KERNEL_WALK_GRAD, 0);
    HIPCHECK(grape_walk::launch_merged_wide(1, Pw[0], Bw[0], Pw[1], Bw[1], st));
    mk(GRAPE_KERNEL_WALK_GRAD, 1);
    return GRAPE_OK;
}

static int enqueue(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                   double *d_Fd2dx) {
    hipStream_t st = p->stream;
    p->cur_stream = st;
    const KMark mk = profiling_mark(p);
    if (p->tiled) {  // one pass of nb <= max_batch evaluations in the plan's workspace (grape_tiled.hip)
        grape_tiled::TiledBatch TB = p->TB;
        TB.nb = nb;
        TB.x = d_x;
        TB.F = d_F;
        TB.Fdx = d_Fdx;
        HIPCHECK(grape_tiled::launch_pipeline(p->TP, TB, st, mk));
        return GRAPE_OK;
    }
    if (p->general_h0) return enqueue_general(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx, mk);
    if (p->dense) {
        const grape_dense::DenseBatch DB = dense_batch(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx);
        HIPCHECK(grape_dense::launch_pipeline(p->DP, DB, st, mk));
        return GRAPE_OK;
    }
    if (p->e1) {  // one workgroup per evaluation (grape_eval1.hip)
        mk(GRAPE_KERNEL_EVAL1, 0);
        HIPCHECK(grape_eval1::launch(eval1_args(p, d_x, d_F, d_Fdx), nb, st));
        mk(GRAPE_KERNEL_EVAL1, 1);
        return GRAPE_OK;
    }
    if (p->ncls) {  // sectors: stage 0 of every class, the head, stage 1 of every class, the sum
        DevBatch Bc[2]{};
        grape::SecParts sp{};
        for (int cl = 0; cl < p->ncls; ++cl) {
            const grape_plan::SecBuf &sb = p->sb[cl];
            DevBatch &B = Bc[cl];
            B.nb = nb * p->Ps[cl].nsec;
            B.x = d_x;
            B.F = d_F;
            B.Fdx = d_Fdx;
            B.E = sb.E;
            B.Q = sb.Q;
            B.Mc = sb.Mc;
            B.Carry = sb.Carry;
            B.Ub = sb.Ub;
            B.Msec = sb.Msec;
            B.part_add = p->d_part;
            B.tgt_part = p->d_tgt_part;
            B.overflow = sb.ovf;
            B.ovf2 = sb.ovf2;
            B.ovf2_slots = sb.slots;
            B.sec_part = sb.part;
            B.Fd2 = d_Fd2;
            B.Fd2dx = d_Fd2dx;
            B.part_err_add = p->d_part_err;
            if (p->P.ne > 0) {
                B.Zl = sb.Zl;
                B.Wc = p->Ps[cl].walk ? sb.Wc : nullptr;
                B.Me = sb.Me;
                B.TotS = sb.TotS;
                B.MsecE = sb.MsecE;
                B.sec_part_err = sb.part_err;
            }
            B.overflow_count = p->d_ctrl + 4 + 2 * cl;  // ctrl [4..7]: two counters per class
            B.ovf2_count = p->d_ctrl + 5 + 2 * cl;
            B.status = p->d_ctrl + 2;
            B.sink = p->d_sink;
            B.Tc = sb.Tc;  // chunk walks (null otherwise)
            B.wscr = sb.wscr;
            B.Ew = sb.Ew;
            sp.part[cl] = sb.part;
            sp.nsec[cl] = p->Ps[cl].walk ? grape_walk::grad_parts(p->Ps[cl]) : p->Ps[cl].nsec;
            if (p->merged && cl != p->merge_pa) sp.nsec[cl] = 0;  // (the merged walk's one part is class A's)
            sp.lane_major[cl] = p->Ps[cl].walk;  // k_walk_grad's / k_walk_img_sum's layout
            sp.part_err[cl] = sb.part_err;
            sp.lane_major_err[cl] = p->Ps[cl].walk;  // k_walk_err_grad's layout
        }
        bool parks = false;  // the chunk walks never park a step for k_expm_high: no counters to clear
        for (int cl = 0; cl < p->ncls; ++cl) parks = parks || !p->Ps[cl].walk;
        if (parks) HIPCHECK(hipMemsetAsync(p->d_ctrl + 4, 0, 4 * sizeof(int), st));
        // Small calls (latency-bound: the optimiser's line-search rounds, single evaluations) run
        // the second sector class on the auxiliary stream beside the first; large ones keep one
        // stream (no gain there, DESIGN 4.1, and per-kernel event times stay per kernel).
        const bool fork = p->aux_stream && !p->capturing && nb <= kForkMaxBatch &&
                          !(p->P.opts & GRAPE_OPT_NO_FORK);
        // Latency-bound calls of the Rydberg layout: both classes' walks (and scans) in ONE launch per
        // stage (grape_walk_api.hpp launch_pair) -- neither a graph branch nor a second stream overlaps
        // them inside a captured graph on this runtime.  pa: the 4- (or 3-) level class, pb: the 2-level one.
        int pa, pb;
        walk_pair_order(p, &pa, &pb);
        // (small calls only: a pair kernel runs the 2-level class at the 4-level class's occupancy)
        const bool pair = p->ncls == 2 && nb <= kPairMaxBatch && !(p->P.opts & GRAPE_OPT_NO_PAIR) &&
                          p->Ps[0].scan_waves == kScanLatency &&
                          p->Ps[1].scan_waves == kScanLatency && grape_walk::pair_ok(p->Ps[pa], p->Ps[pb]);
        auto stage = [&](int s) -> hipError_t {  // stage s of every class (class 1 forked when `fork`)
            if (p->merged && s < 2) {  // both classes in one lane (throughput passes)
                const int ma = p->merge_pa, mb = 1 - ma;
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 0);
                hipError_t e = grape_walk::launch_merged(s, p->Ps[ma], Bc[ma], p->Ps[mb], Bc[mb], st);
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 1);
                if (e == hipSuccess && s == 0) {  // the merged walks' sequential scan (lane-minor totals)
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = grape_walk::launch_merged(2, p->Ps[ma], Bc[ma], p->Ps[mb], Bc[mb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                }
                return e;
            }
            if (pair && s < 2) {
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 0);
                hipError_t e = grape_walk::launch_pair(s, p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st);
                mk(s == 0 ? GRAPE_KERNEL_WALK_FWD : GRAPE_KERNEL_WALK_GRAD, 1);
                if (e == hipSuccess && s == 0) {
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = p->Ps[pa].D == 4 ? grape_host::launch_scan_pair<4, 2>(p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st)
                                         : grape_host::launch_scan_pair<3, 2>(p->Ps[pa], Bc[pa], p->Ps[pb], Bc[pb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                }
                return e;
            }
            if (s == 0 && !fork && !pair) {  // both walk classes' one-wave scans in one launch
                const int ca = p->Ps[0].D == 2 ? 1 : 0, cb = 1 - ca;
                const DevProblem &Pa = p->Ps[ca], &Pb = p->Ps[cb];
                if (p->ncls == 2 && Pa.walk && Pb.walk && (Pa.D == 3 || Pa.D == 4) && Pb.D == 2 &&
                    Pa.scan_waves == kScanTiny && Pb.scan_waves == kScanTiny) {
                    mk(GRAPE_KERNEL_WALK_FWD, 0);
                    hipError_t e = Pa.D == 4 ? grape_walk::launch<4>(0, Pa, Bc[ca], st) : grape_walk::launch<3>(0, Pa, Bc[ca], st);
                    if (e == hipSuccess) e = grape_walk::launch<2>(0, Pb, Bc[cb], st);
                    mk(GRAPE_KERNEL_WALK_FWD, 1);
                    if (e != hipSuccess) return e;
                    mk(GRAPE_KERNEL_SCAN, 0);
                    e = Pa.D == 4 ? grape_host::launch_scan_pair<4, 2, kScanTiny>(Pa, Bc[ca], Pb, Bc[cb], st)
                                  : grape_host::launch_scan_pair<3, 2, kScanTiny>(Pa, Bc[ca], Pb, Bc[cb], st);
                    mk(GRAPE_KERNEL_SCAN, 1);
                    return e;
                }
            }
            if (!fork || pair) {
                for (int cl = 0; cl < p->ncls; ++cl) {
                    const hipError_t e = dispatch_sector_stage(p->Ps[cl].D, s, p->Ps[cl], Bc[cl], p->FT, st, mk);
                    if (e != hipSuccess) return e;
                }
                return hipSuccess;
            }
            hipEvent_t evf = p->ev_fork, evj = p->ev_join;
            hipError_t e = hipEventRecord(evf, st);
            if (e == hipSuccess) e = hipStreamWaitEvent(p->aux_stream, evf, 0);
            if (e == hipSuccess) e = dispatch_sector_stage(p->Ps[0].D, s, p->Ps[0], Bc[0], p->FT, st, mk);
            p->cur_stream = p->aux_stream;
            if (e == hipSuccess) e = dispatch_sector_stage(p->Ps[1].D, s, p->Ps[1], Bc[1], p->FT, p->aux_stream, mk);
            p->cur_stream = st;
            if (e == hipSuccess) e = hipEventRecord(evj, p->aux_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(st, evj, 0);
            return e;
        };
        HIPCHECK(stage(0));
        grape_proj::SectorHead H = p->SH;
        H.x = d_x;
        H.F = d_F;
        H.Fdx = d_Fdx;
        H.tgt_part = p->d_tgt_part;
        H.Fd2 = d_Fd2;
        H.Fd2dx = d_Fd2dx;
        mk(GRAPE_KERNEL_SCAN, 0);
        HIPCHECK(grape_proj::launch_sector_head(H, nb, st));
        mk(GRAPE_KERNEL_SCAN, 1);
        HIPCHECK(stage(1));
        if (p->P.ne > 0) {  // the sector error head, then the F_d2err_dx walks of every class
            mk(GRAPE_KERNEL_ERR_SCAN, 0);
            HIPCHECK(grape_proj::launch_sector_err_head(H, nb, st));
            mk(GRAPE_KERNEL_ERR_SCAN, 1);
            HIPCHECK(stage(2));
        }
        // (the merged gradient walk wrote F_dx itself; without x_add-dependent H0 nothing is left to sum)
        if (!(p->merged && !(p->P.xadd_dep && p->P.na > 0)))
            HIPCHECK(dispatch_sector_reduce(p->Ps[0].D, p->Ps[0], Bc[0], sp, nb, st, mk));
        return GRAPE_OK;
    }
    const DevProblem &P = p->P;
    DevBatch B{};
    B.Fd2 = d_Fd2;
    B.Fd2dx = d_Fd2dx;
    B.nb = nb;
    B.x = d_x;
    B.F = d_F;
    B.Fdx = d_Fdx;
    B.E = p->d_E;
    B.Q = p->d_Q;
    B.Mc = p->d_Mc;
    B.part_add = p->d_part;
    B.tgt_part = p->d_tgt_part;
    B.overflow = p->d_ovf;
    B.Carry = p->d_Carry;  // allocated for the error path and the general-projector heads
    B.Ub = p->d_Ub;
    B.gp_scr = p->d_gpscr;
    if (P.ne == 0) {
        B.ovf2 = p->d_ovf2;
        B.ovf2_slots = p->d_ovf2_slots;
    } else {
        B.Me = p->d_Me;
        B.part_err_add = p->d_part_err;
        B.Zl = p->d_Zl;
    }
    // ctrl: [2] status (sticky until grape_plan_synchronize reports it),
    // [4] k_expm overflow count, [5] k_expm_grad overflow count
    int *cnt = p->d_ctrl + 4;
    B.overflow_count = cnt;
    B.ovf2_count = cnt + 1;
    B.status = p->d_ctrl + 2;
    B.sink = p->d_sink;
    HIPCHECK(hipMemsetAsync(cnt, 0, 2 * sizeof(int), st));
    if (p->tables) {
        B.Htab = p->d_Htab;
        B.U0tab = p->d_U0tab;
    }
    HIPCHECK(dispatch_pipeline(P.D, P, B, p->FT, st, mk));
    return GRAPE_OK;
}

// General H0 (p->general_h0): every evaluation of the launch through the materialised
// derivatives -- its propagator table, the chain and its LU inverses, the assembly
// (UnitaryCalculations.jl:44-155) -- then F, F_dx, F_d2err, F_d2err_dx from them
// (FidelityCalculations.jl:19-119), on the plan's stream, one evaluation after another in
// the single-evaluation workspace.
static int enqueue_general(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                           double *d_Fd2dx, const KMark &mk) {
    if (int rc = ud_alloc(p)) return rc;
    const DevProblem &P = p->P;
    const size_t T = (size_t)P.D * P.D, nx = P.nx;
    hipStream_t st = p->stream;
    grape_unitary::UProblem UP;
    grape_unitary::UBuffers UB;
    const std::vector<grape::VSpec> vs = ud_setup(p, UP, UB);
    p->ud_vs_host = vs;  // the async copy reads this plan-owned copy
    HIPCHECK(hipMemcpyAsync(p->ud_vs, p->ud_vs_host.data(), vs.size() * sizeof(grape::VSpec), hipMemcpyHostToDevice, st));
    grape_unitary::FidArgs FA{};
    FA.P = P;
    FA.U = p->ud_C + (size_t)(P.Nt - 1) * T;
    FA.Udx = UB.Udx;
    FA.Udxa = UB.Udxa;
    FA.Ue = UB.Ue;
    FA.Uedx = UB.Uedx;
    FA.Uedxa = UB.Uedxa;
    FA.G = p->d_G;
    FA.scr = p->d_fscr;
    for (int b = 0; b < nb; ++b) {
        const double *xb = d_x + (size_t)b * nx;
        mk(GRAPE_KERNEL_EXPM, 0);
        if (int rc = ud_propagators_dev(p, xb, UP.nv,
                                        p->tables ? p->d_Htab + (size_t)b * P.Nt * UP.nv * T : nullptr)) return rc;
        mk(GRAPE_KERNEL_EXPM, 1);
        mk(GRAPE_KERNEL_GRAD, 0);
        HIPCHECK(grape_unitary::launch_assembly(UP, UB, st));
        FA.x = xb;
        FA.U0tab = p->tables ? p->d_U0tab + (size_t)b * (1 + P.na) * T : nullptr;
        FA.F = d_F + b;
        FA.Fdx = d_Fdx + (size_t)b * nx;
        FA.Fd2 = P.ne ? d_Fd2 + (size_t)b * P.ne : nullptr;
        FA.Fd2dx = P.ne ? d_Fd2dx + (size_t)b * P.ne * nx : nullptr;
        HIPCHECK(grape_unitary::launch_fidelity(FA, st));
        mk(GRAPE_KERNEL_GRAD, 1);
    }
    return GRAPE_OK;
}

// Enqueue one call's batch, then copy the status word to pinned memory on the plan's stream.
// (Sector plans whose every class walks set no status bit -- no Pade solve, no parked step, no
// LU -- and skip that copy.)
static bool status_free(const grape_plan *p) {
    if (!p->ncls || p->general_h0 || p->dense || p->tables) return false;
    for (int cl = 0; cl < p->ncls; ++cl)
        if (!p->Ps[cl].walk) return false;
    return true;
}
static int enqueue_call(grape_plan *p, int nb, const double *d_x, double *d_F, double *d_Fdx, double *d_Fd2,
                        double *d_Fd2dx) {
    if (int rc = enqueue(p, nb, d_x, d_F, d_Fdx, d_Fd2, d_Fd2dx)) return rc;
    if (!status_free(p))
        HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return GRAPE_OK;
}

static void resolve_events(grape_plan *p) {
    for (auto &pe : p->pending) {
        float ms = 0.f;
        if (pe.a && pe.b && hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            p->kernel_ms[pe.kernel] += ms;
            p->kernel_launches[pe.kernel] += 1;
        }
        if (pe.a) p->ev_pool.push_back(pe.a);
        if (pe.b) p->ev_pool.push_back(pe.b);
    }
    p->pending.clear();
}

int grape_fidelity_grad_device_async(grape_plan *p, int nbatch, const double *d_x, double *d_F, double *d_F_dx,
                                     double *d_F_d2err, double *d_F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!d_x || !d_F || !d_F_dx))) return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p->tables) return fail(GRAPE_ERR_INVALID, "host-table plan: use grape_fidelity_grad_tables");
    if (p->P.ne > 0 && nbatch > 0 && (!d_F_d2err || !d_F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    HIPCHECK(hipSetDevice(p->device));
    // Device-resident batches of a rank-one merged plan: while at least W = max_batch x nchunks evaluations remain,
    // one wide pass of W (one lane per evaluation, no chunks: enqueue_wide); the rest through the chunked passes.
    // The path is chosen by count alone, so a repeated call repeats its bits.
    int b0 = 0;
    for (; p->wide > 0 && nbatch - b0 >= p->wide; b0 += p->wide)
        if (int rc = enqueue_wide(p, p->wide, d_x + (size_t)b0 * p->P.nx, d_F + b0, d_F_dx + (size_t)b0 * p->P.nx)) return rc;
    for (; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        int rc = enqueue_call(p, nb, d_x + (size_t)b0 * p->P.nx, d_F + b0, d_F_dx + (size_t)b0 * p->P.nx,
                              p->P.ne ? d_F_d2err + (size_t)b0 * p->P.ne : nullptr,
                              p->P.ne ? d_F_d2err_dx + (size_t)b0 * p->P.ne * p->P.nx : nullptr);
        if (rc) return rc;
    }
    return GRAPE_OK;
}

int grape_plan_synchronize(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    HIPCHECK(hipSetDevice(p->device));
    HIPCHECK(hipStreamSynchronize(p->stream));
    resolve_events(p);
    const int st = *p->h_status;
    if (st & 3) {
        *p->h_status = 0;
        HIPCHECK(hipMemset(p->d_ctrl + 2, 0, sizeof(int)));
        return fail(GRAPE_ERR_SINGULAR, (st & 2) ? "singular propagator chain C_k (Julia inv would throw SingularException)"
                                                 : "singular Pade denominator (Julia gesv! would throw SingularException)");
    }
    return GRAPE_OK;
}

// Host-array calls of at most kGraphBatch evaluations are latency-bound (a 1-evaluation C2
// call is ~10 dependent launches and copies of a few KB): they are captured once per batch size
// into a HIP graph -- pinned staging copies in, the pipeline, status and results out -- and
// replayed with one launch.  GRAPE_NO_GRAPH=1 (or profiling) takes the stream path.
constexpr int kGraphBatch = 64, kGraphCache = 8;

// offsets (doubles) of the outputs of a graph-path call of nb evaluations in p->d_gout / p->h_F:
// F [B], F_dx [nb][nx], F_d2err [nb][ne], F_d2err_dx [nb][ne][nx] (B = the graph path's batch capacity);
// used = the extent one D2H copy returns
struct GraphOut {
    size_t fdx, fd2, fd2dx, used, capacity;
};
static GraphOut graph_out(const grape_plan *p, int nb) {
    const size_t nx = p->P.nx, ne = p->P.ne, B = std::min(kGraphBatch, p->max_batch);
    GraphOut o;
    o.fdx = B;
    o.fd2 = B * (1 + nx);
    o.fd2dx = o.fd2 + B * ne;
    o.used = ne ? o.fd2dx + (size_t)nb * ne * nx : o.fdx + (size_t)nb * nx;
    o.capacity = o.fd2dx + B * ne * nx;
    return o;
}

static int graph_capture(grape_plan *p, int nb, hipGraphExec_t *out) {
    const int nx = p->P.nx, ne = p->P.ne;
    hipStream_t st = p->stream;
    HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    auto body = [&]() -> int {
        HIPCHECK(hipMemcpyAsync(p->d_x, p->h_x, (size_t)nb * nx * sizeof(double), hipMemcpyHostToDevice, st));
        // every output in one device block [F | F_dx | F_d2err | F_d2err_dx] (graph_out), returned by ONE
        // D2H copy into its pinned image (round 6: one copy instead of three with error sources, ~9 us
        // of a 0.09-ms single evaluation)
        const GraphOut o = graph_out(p, nb);
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_gout, p->d_gout + o.fdx, p->d_gout + o.fd2, p->d_gout + o.fd2dx))
            return rc;
        HIPCHECK(hipMemcpyAsync(p->h_F, p->d_gout, o.used * sizeof(double), hipMemcpyDeviceToHost, st));
        return GRAPE_OK;
    };
    p->capturing = true;
    const int rc = body();
    p->capturing = false;
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess) return fail(GRAPE_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) return fail(GRAPE_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(ei));
    if ((int)p->graphs.size() >= kGraphCache) {
        (void)hipGraphExecDestroy(p->graphs.front().exec);
        p->graphs.erase(p->graphs.begin());
    }
    p->graphs.push_back({nb, ex});
    *out = ex;
    return GRAPE_OK;
}

static bool graph_path(const grape_plan *p, int nbatch) {
    const bool disabled = (p->P.opts & GRAPE_OPT_NO_GRAPH) != 0;
    return !disabled && !p->profiling && !p->tables && !p->general_h0 && !p->tiled && nbatch > 0 && nbatch <= kGraphBatch &&
           nbatch <= p->max_batch;
}

static int fidelity_grad_graph(grape_plan *p, int nb, const double *x, double *F, double *F_dx, double *F_d2err,
                               double *F_d2err_dx) {
    const size_t nx = p->P.nx, ne = p->P.ne, B = std::min(kGraphBatch, p->max_batch);
    if (!p->h_x) {
        auto pin = [](double **h, size_t n) {
            return hipHostMalloc(reinterpret_cast<void **>(h), std::max<size_t>(n, 1) * sizeof(double),
                                 hipHostMallocDefault) == hipSuccess;
        };
        const size_t cap = graph_out(p, 1).capacity;
        if (!pin(&p->h_x, B * nx) || !pin(&p->h_F, cap))
            return fail(GRAPE_ERR_ALLOC, "pinned allocation failed (graph path)");
        if (p->mem.alloc(&p->d_gout, cap) != hipSuccess)
            return fail(GRAPE_ERR_ALLOC, "device allocation failed (graph path)");
    }
    if (p->e1) {
        // one workgroup per evaluation: a single launch that reads x from and writes F, F_dx to the
        // mapped pinned buffers -- no staging copies, no graph
        if (!p->hd_x && (hipHostGetDevicePointer(reinterpret_cast<void **>(&p->hd_x), p->h_x, 0) != hipSuccess ||
                         hipHostGetDevicePointer(reinterpret_cast<void **>(&p->hd_F), p->h_F, 0) != hipSuccess))
            return fail(GRAPE_ERR_HIP, "pinned buffers are not mapped (eval1)");
        std::memcpy(p->h_x, x, (size_t)nb * nx * sizeof(double));
        if (int rc = enqueue_call(p, nb, p->hd_x, p->hd_F, p->hd_F + B, nullptr, nullptr)) return rc;
        if (int rc = grape_plan_synchronize(p)) return rc;
        std::memcpy(F, p->h_F, (size_t)nb * sizeof(double));
        std::memcpy(F_dx, p->h_F + B, (size_t)nb * nx * sizeof(double));
        if (p->e1_trace) {
            const long long *tr = p->e1_trace;
            for (int i = 0; i < 9; ++i) p->e1_phase[i] += (double)(tr[i + 1] - tr[i]);
            const double us = (double)(tr[15] - tr[14]) / 100.0;  // (wall clock: 100 MHz)
            if (us > 0) p->e1_phase[9] += (double)(tr[9] - tr[0]) / us;
            for (int i = 0; i < 4; ++i) p->e1_phase[10 + i] += (double)(tr[17 + i] - tr[16 + i]);
            p->e1_phase[14] += (double)(tr[21] - tr[1]);
            p->e1_phase[15] += (double)(tr[22] - tr[1]);
            p->e1_calls += 1;
        }
        return GRAPE_OK;
    }
    hipGraphExec_t ex = nullptr;
    for (auto &g : p->graphs)
        if (g.nb == nb) ex = g.exec;
    if (!ex)
        if (int rc = graph_capture(p, nb, &ex)) return rc;
    std::memcpy(p->h_x, x, (size_t)nb * nx * sizeof(double));
    HIPCHECK(hipGraphLaunch(ex, p->stream));
    if (int rc = grape_plan_synchronize(p)) return rc;
    const GraphOut o = graph_out(p, nb);
    std::memcpy(F, p->h_F, (size_t)nb * sizeof(double));
    std::memcpy(F_dx, p->h_F + o.fdx, (size_t)nb * nx * sizeof(double));
    if (ne > 0) {
        std::memcpy(F_d2err, p->h_F + o.fd2, (size_t)nb * ne * sizeof(double));
        std::memcpy(F_d2err_dx, p->h_F + o.fd2dx, (size_t)nb * ne * nx * sizeof(double));
    }
    return GRAPE_OK;
}

// the results of workspace rows [0, nb) into the caller's host arrays at evaluation b0; synchronises
static int results_to_host(grape_plan *p, int b0, int nb, double *F, double *F_dx, double *F_d2err, double *F_d2err_dx) {
    const size_t nx = p->P.nx, ne = p->P.ne;
    HIPCHECK(hipMemcpyAsync(F + b0, p->d_F, nb * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (ne > 0) {
        HIPCHECK(hipMemcpyAsync(F_d2err + b0 * ne, p->d_Fd2, nb * ne * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIPCHECK(hipMemcpyAsync(F_d2err_dx + b0 * ne * nx, p->d_Fd2dx, nb * ne * nx * sizeof(double),
                                hipMemcpyDeviceToHost, p->stream));
    }
    HIPCHECK(hipMemcpyAsync(F_dx + b0 * nx, p->d_Fdx, nb * nx * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    return grape_plan_synchronize(p);
}

int grape_fidelity_grad(grape_plan *p, int nbatch, const double *x, double *F, double *F_dx, double *F_d2err,
                        double *F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!x || !F || !F_dx))) return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p->tables) return fail(GRAPE_ERR_INVALID, "host-table plan: use grape_fidelity_grad_tables");
    if (p->P.ne > 0 && nbatch > 0 && (!F_d2err || !F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    HIPCHECK(hipSetDevice(p->device));
    if (graph_path(p, nbatch)) return fidelity_grad_graph(p, nbatch, x, F, F_dx, F_d2err, F_d2err_dx);
    const int nx = p->P.nx;
    for (int b0 = 0; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        HIPCHECK(hipMemcpyAsync(p->d_x, x + (size_t)b0 * nx, (size_t)nb * nx * sizeof(double),
                                hipMemcpyHostToDevice, p->stream));
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_F, p->d_Fdx, p->d_Fd2, p->d_Fd2dx)) return rc;
        if (int rc = results_to_host(p, b0, nb, F, F_dx, F_d2err, F_d2err_dx)) return rc;
    }
    return GRAPE_OK;
}

// Time sharding of one evaluation: see include/grape.h.
static int slice_check(grape_plan *p) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    if (p->tiled) return fail(GRAPE_ERR_UNSUPPORTED, "time slices: not served by the tiled engine (ndim > GRAPE_MAX_DENSE_DIM)");
    if (!p->dense || p->general_h0 || p->tables || p->P.ne > 0 || p->P.na > 0 || p->P.gen_proj || p->uses_tstep)
        return fail(GRAPE_ERR_UNSUPPORTED, "time slices: dense-engine operator-basis plans without error sources, "
                                           "x_add, a general projector or step-index terms");
    const size_t T = (size_t)p->P.D * p->P.D;
    if (!p->dn_Ub && p->mem.alloc(&p->dn_Ub, (size_t)p->max_batch * grape_dense::kImgDoubles) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (time slices)");
    if (!p->d_slice && p->mem.alloc(&p->d_slice, 2 * T) != hipSuccess)
        return fail(GRAPE_ERR_ALLOC, "device allocation failed (time slices)");
    return GRAPE_OK;
}

int grape_slice_forward(grape_plan *p, const double *x, double *U_slice) {
    if (!p || !x || !U_slice) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const size_t T = (size_t)p->P.D * p->P.D;
    hipStream_t st = p->stream;
    HIPCHECK(hipMemcpyAsync(p->d_x, x, (size_t)p->P.nx * sizeof(double), hipMemcpyHostToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_forward(p->DP, DB, p->d_slice, st));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(U_slice, p->d_slice, T * sizeof(cd), hipMemcpyDeviceToHost, st));
    return grape_plan_synchronize(p);
}

int grape_slice_gradient(grape_plan *p, const double *M_prime, double *F_dx) {
    if (!p || !M_prime || !F_dx) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const size_t T = (size_t)p->P.D * p->P.D;
    hipStream_t st = p->stream;
    HIPCHECK(hipMemcpyAsync(p->d_slice + T, M_prime, T * sizeof(cd), hipMemcpyHostToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_gradient(p->DP, DB, p->d_slice + T, st));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(F_dx, p->d_Fdx, (size_t)p->P.np * p->P.Nt * sizeof(double), hipMemcpyDeviceToHost, st));
    return grape_plan_synchronize(p);
}

int grape_slice_forward_device(grape_plan *p, const double *d_x, double *d_U_slice) {
    if (!p || !d_x || !d_U_slice) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    hipStream_t st = p->stream;
    // the slice's controls stay in the plan for grape_slice_gradient_device (as the host entry)
    HIPCHECK(hipMemcpyAsync(p->d_x, d_x, (size_t)p->P.nx * sizeof(double), hipMemcpyDeviceToDevice, st));
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, p->d_Fdx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_forward(p->DP, DB, reinterpret_cast<cd *>(d_U_slice), st));
    // the Pade status for the caller's grape_plan_synchronize (as the host entries report it)
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    return GRAPE_OK;
}

int grape_slice_gradient_device(grape_plan *p, const double *d_M_prime, double *d_F_dx) {
    if (!p || !d_M_prime || !d_F_dx) return fail(GRAPE_ERR_INVALID, "bad argument");
    HIPCHECK(hipSetDevice(p->device));
    if (int rc = slice_check(p)) return rc;
    const grape_dense::DenseBatch DB = dense_batch(p, 1, p->d_x, p->d_F, d_F_dx, nullptr, nullptr);
    HIPCHECK(grape_dense::launch_slice_gradient(p->DP, DB, reinterpret_cast<const cd *>(d_M_prime), p->stream));
    HIPCHECK(hipMemcpyAsync(p->h_status, p->d_ctrl + 2, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    return GRAPE_OK;
}

int grape_fidelity_grad_tables(grape_plan *p, int nbatch, const double *x, const double *H, const double *U0,
                               double *F, double *F_dx, double *F_d2err, double *F_d2err_dx) {
    if (!p || nbatch < 0 || (nbatch > 0 && (!x || !H || !U0 || !F || !F_dx)))
        return fail(GRAPE_ERR_INVALID, "bad argument");
    if (p && p->P.ne > 0 && nbatch > 0 && (!F_d2err || !F_d2err_dx))
        return fail(GRAPE_ERR_INVALID, "error sources need F_d2err and F_d2err_dx outputs");
    if (!p->tables) return fail(GRAPE_ERR_INVALID, "plan was not created with GRAPE_DESC_HOST_TABLES");
    HIPCHECK(hipSetDevice(p->device));
    const DevProblem &P = p->P;
    const size_t nx = P.nx, T = (size_t)P.D * P.D, hsz = (size_t)P.Nt * P.nv * T, usz = (1 + (size_t)P.na) * T;
    for (int b0 = 0; b0 < nbatch; b0 += p->max_batch) {
        const int nb = std::min(p->max_batch, nbatch - b0);
        HIPCHECK(hipMemcpyAsync(p->d_x, x + b0 * nx, nb * nx * sizeof(double), hipMemcpyHostToDevice, p->stream));
        HIPCHECK(hipMemcpyAsync(p->d_Htab, H + 2 * b0 * hsz, nb * hsz * sizeof(cd), hipMemcpyHostToDevice,
                                p->stream));
        HIPCHECK(hipMemcpyAsync(p->d_U0tab, U0 + 2 * b0 * usz, nb * usz * sizeof(cd), hipMemcpyHostToDevice,
                                p->stream));
        if (int rc = enqueue_call(p, nb, p->d_x, p->d_F, p->d_Fdx, p->d_Fd2, p->d_Fd2dx)) return rc;
        if (int rc = results_to_host(p, b0, nb, F, F_dx, F_d2err, F_d2err_dx)) return rc;
    }
    return GRAPE_OK;
}

int grape_plan_set_profiling(grape_plan *p, int enable) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    p->profiling = enable != 0;
    return GRAPE_OK;
}

int grape_plan_kernel_times(grape_plan *p, double *total_ms, long long *launches, int reset) {
    if (!p) return fail(GRAPE_ERR_INVALID, "null plan");
    for (int k = 0; k < GRAPE_NUM_KERNELS; ++k) {
        if (total_ms) total_ms[k] = p->kernel_ms[k];
        if (launches) launches[k] = p->kernel_launches[k];
        if (reset) {
            p->kernel_ms[k] = 0.0;
            p->kernel_launches[k] = 0;
        }
    }
    return GRAPE_OK;
}

// workspace of the single-evaluation analysis entry points (unitary derivatives,
// interaction-picture error operators, expectation values), allocated on first use
static int ud_alloc(grape_plan *p) {
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
static int ud_propagators_dev(grape_plan *p, const double *d_x, int nv, const cd *d_Htab) {
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

// The assembly problem and buffers of the ud workspace (outputs packed in ud_out:
// U_dx | U_dx_add | U_derr | U_derr_dx | U_derr_dx_add); returns the variant list.
static std::vector<grape::VSpec> ud_setup(grape_plan *p, grape_unitary::UProblem &UP, grape_unitary::UBuffers &UB) {
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

static int dense_expm_batch(int device, int ndim, int n, const double *A, double *E, int *stats, bool pivot) {
    const size_t IMG = grape_dense::kImgDoubles;
    std::vector<double> h((size_t)n * IMG);
    for (int i = 0; i < n; ++i) to_dense_image(A + 2 * (size_t)i * ndim * ndim, ndim, h.data() + i * IMG);
    grape_setup::DevicePool mem;
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
    grape_setup::DevicePool mem;
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
    grape_setup::DevicePool mem;
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

int grape_expm_batch(int device, int ndim, int n, const double *A, double *E, int *stats) {
    return expm_batch(device, ndim, n, A, E, stats, false);
}

int grape_expm_batch_general(int device, int ndim, int n, const double *A, double *E, int *stats) {
    return expm_batch(device, ndim, n, A, E, stats, true);
}

}  // extern "C"
