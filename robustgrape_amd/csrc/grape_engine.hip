// grape_engine.hip -- C ABI (include/grape.h) over the gfx950 GRAPE kernels.
//
// A plan owns: the device copy of the operator basis (row-major tiles), the
// term tables, and a workspace for `max_batch` evaluations laid out in HBM as
//   E  [b][k][v][D][D]   propagators of every FD variant   (c128)
//   Q  [b][k][D][D]      chunk-local prefix products
//   Mc [b][c][D][D]      per-chunk gradient kernels
// (288 GB per MI355X; at d=9, N_t=512 one evaluation needs 2.0 MB).
//
// The ABI's host code is five units around grape_plan.hpp.  This one: the error message, the ids, the fault
// handler, the per-dimension dispatch, plan creation's top level, destruction and the getters.  The others:
// grape_descriptor.hip, grape_plan_build.hip, grape_call.hip, grape_analysis.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <type_traits>
#include <csignal>
#include <cstdint>
#include <dlfcn.h>
#include <execinfo.h>
#include <link.h>
#include <ucontext.h>
#include <unistd.h>

#include "grape_plan.hpp"

static_assert(sizeof(Term) == sizeof(grape_term), "grape_term layout");

namespace {

thread_local std::string g_err;

}  // namespace

namespace grape_eng {

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

using grape_host::launch_pipeline;
using grape_host::launch_expm_raw;
using grape_host::set_lds_limits;

// f(std::integral_constant<int, D>) for the dimension D (GRAPE_DIMS); the launch sequences called through it
// are declared in grape_launch_api.hpp and instantiated in grape_inst.hip (one translation unit per dimension)
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

}  // namespace grape_eng
using namespace grape_eng;

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

}  // extern "C"
