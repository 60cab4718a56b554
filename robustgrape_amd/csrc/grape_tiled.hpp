// grape_tiled.hpp -- CDNA4 (gfx950) building blocks of the TILED engine
// (GRAPE_MAX_DENSE_DIM < d <= GRAPE_MAX_TILED_DIM).
//
// Above 64 levels a complex FP64 matrix no longer fits the registers and LDS of one workgroup
// (128 x 128: 256 KB), so the matrices live in HBM / L2 and every product streams tiles through LDS.
//
// Images: d is padded to P = 16 ceil(d / 16) (80, 96, 112 or 128); a matrix is two row-major P x P
// double planes (re, then im) whose padding is zero.  Every kernel preserves that: products of
// zero-padded operands are zero-padded, and the identity of an epilogue is added on the first d
// diagonal entries only, so the padded block of a propagator is zero (as in the dense images).
//
// Product C = op(L) op(R) (op: plain, or conjugate-transposed) on v_mfma_f64_16x16x4_f64 with the
// fragment layouts of grape_dense.hpp (scripts/probes/mfma_probe.hip):
//   A fragment (16 x 4):  lane l holds A[l & 15][l >> 4]
//   B fragment (4 x 16):  lane l holds B[l >> 4][l & 15]
//   C tile (16 x 16):     lane l, element r holds C[(l >> 4) + 4r][l & 15]
// A workgroup of 4 waves owns one 64 x 64 output tile (or the remainder tile: P - 64 rows / columns,
// a multiple of 16); wave w owns rows 16w .. 16w + 15 of it, four C tiles, as four real MFMA
// streams per complex product (no Gauss form: the 4-multiplication product keeps re and im
// independent, and the tiled engine's kernels are bound by the MFMA pipe either way).  Both operands
// are staged through LDS in K-slabs of 16: 64 x 16 of op(L), 16 x 64 of op(R), re and im, 40 KB with
// the padding below (three workgroups per CU).  The next slab's global loads are issued into registers
// before the current slab's MFMAs, so HBM / L2 latency overlaps the MFMA stream.
//
// LDS layouts, chosen per operand form so that the global reads follow the images' rows:
//   XM  [x][k], leading dimension 17: L plain, R conjugate-transposed (global rows run along k)
//   KM  [k][x], leading dimension 80: L conjugate-transposed, R plain (global rows run along x)
// Fragment reads take x = 16 a + (l & 15), k = 4 s + (l >> 4).  The re and im planes lie 10 240 B apart, so the
// compiler pairs each fragment's two reads into one ds_read2st64_b64 (and the staging stores into
// ds_write2st64_b64; checked in the ISA): four 16-lane groups over 32 banks, the second access model of
// scripts/probes/lds_banks.py.  There a group reads 16 x at one k: XM dword 34 x + 2 k is 2 x + const mod 32, KM
// is contiguous -- 16 distinct bank pairs, no conflict, for reads and staging stores alike.  (As plain
// ds_read_b64, two 32-lane groups over 64 banks, KM stays conflict free and XM would pay one extra cycle per
// half-wave: x = 15 at the second k wraps onto x = 0 at the first.)  Measured: 46-52 TFLOP/s credited at
// P = 128.
#pragma once
#include <hip/hip_runtime.h>

#include "grape_kernels.hpp"
#include "grape_tiled_ctl.hpp"

namespace grape_tiled {

using grape::cd;
using grape::Term;
typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int TILE = 64;        // output tile of a workgroup
constexpr int KSLAB = 16;       // K extent of one staged slab
constexpr int LDX = 17;         // XM leading dimension
constexpr int LDK = 80;         // KM leading dimension
constexpr int SLAB = KSLAB * LDK;  // doubles per staged plane (XM needs 64 * 17 = 1 088 of them)
constexpr int NTHREADS = 256;   // 4 waves
static_assert(TILE * LDX <= SLAB, "XM plane must fit the staged plane");

struct Geo {
    int P;  // padded dimension
    int d;  // levels
};

// One product's operands: C = op(L) op(R) [+ c0 I + c1 X1 + c2 X2 + c3 X3 when X1 is set]
struct Ops {
    const double *L = nullptr, *R = nullptr;
    double *C = nullptr;
    const double *X1 = nullptr, *X2 = nullptr, *X3 = nullptr;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
};

__device__ __forceinline__ v4d mfma(double a, double b, v4d c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// element (x, k) of a staged plane
template <bool XM>
__device__ __forceinline__ int sidx(int x, int k) {
    return XM ? x * LDX + k : k * LDK + x;
}

// One slab of one operand: 64 (x) by 16 (k) elements, 4 per thread and plane.  XM: element e = t + 256 q
// is (x, k) = (e >> 4, e & 15) and lives at row x0 + x, column k0 + k of the image; KM: (x, k) =
// (e & 63, e >> 6) at row k0 + k, column x0 + x.  Rows / columns at or beyond `ext` (the remainder tile)
// read as zero and are never addressed.
template <bool XM>
__device__ __forceinline__ void slab_load(const double *img, int P, int x0, int k0, int ext, double (&re)[4],
                                          double (&im)[4]) {
    const int t = threadIdx.x;
    const size_t plane = (size_t)P * P;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + NTHREADS * q;
        const int x = XM ? e >> 4 : e & 63, k = XM ? e & 15 : e >> 6;
        const bool in = x < ext;
        const size_t a = XM ? (size_t)(x0 + x) * P + (k0 + k) : (size_t)(k0 + k) * P + (x0 + x);
        re[q] = in ? img[a] : 0.0;
        im[q] = in ? img[plane + a] : 0.0;
    }
}
template <bool XM, bool CONJ>
__device__ __forceinline__ void slab_store(double *sre, double *sim, const double (&re)[4], const double (&im)[4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + NTHREADS * q;
        const int x = XM ? e >> 4 : e & 63, k = XM ? e & 15 : e >> 6;
        sre[sidx<XM>(x, k)] = re[q];
        sim[sidx<XM>(x, k)] = CONJ ? -im[q] : im[q];
    }
}

// The workgroup's tile (tile = 2 ti + tj of the 2 x 2 tiling of a P x P image, 64 < P <= 128) of
// C = op(L) op(R) with the epilogue of `o`.  lds: 4 * SLAB doubles.  Every thread of the workgroup calls it.
template <bool LCT, bool RCT>
__device__ __forceinline__ void tile_product(const Geo &g, const Ops &o, int tile, double *lds) {
    constexpr bool LXM = !LCT, RXM = RCT;
    const int P = g.P;
    const int i0 = TILE * (tile >> 1), j0 = TILE * (tile & 1);
    const int mh = min(TILE, P - i0), mw = min(TILE, P - j0);  // multiples of 16
    const int l = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double *Lr = lds, *Li = lds + SLAB, *Rr = lds + 2 * SLAB, *Ri = lds + 3 * SLAB;
    v4d cr[4], ci[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) cr[ct] = ci[ct] = v4d{0.0, 0.0, 0.0, 0.0};
    double lre[4], lim[4], rre[4], rim[4];
    slab_load<LXM>(o.L, P, i0, 0, mh, lre, lim);
    slab_load<RXM>(o.R, P, j0, 0, mw, rre, rim);
    const bool active = 16 * w < mh;  // wave-uniform
    const int arow = 16 * w + (l & 15), kq = l >> 4;
    for (int k0 = 0; k0 < P; k0 += KSLAB) {
        __syncthreads();  // the previous slab's fragments are consumed
        slab_store<LXM, LCT>(Lr, Li, lre, lim);
        slab_store<RXM, RCT>(Rr, Ri, rre, rim);
        __syncthreads();
        if (k0 + KSLAB < P) {  // next slab into registers while this one multiplies
            slab_load<LXM>(o.L, P, i0, k0 + KSLAB, mh, lre, lim);
            slab_load<RXM>(o.R, P, j0, k0 + KSLAB, mw, rre, rim);
        }
        if (active) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = 4 * s + kq;
                const double ar = Lr[sidx<LXM>(arow, k)], ai = Li[sidx<LXM>(arow, k)];
                const double nai = -ai;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (16 * ct < mw) {
                        const int c = 16 * ct + (l & 15);
                        const double br = Rr[sidx<RXM>(c, k)], bi = Ri[sidx<RXM>(c, k)];
                        cr[ct] = mfma(ar, br, cr[ct]);
                        cr[ct] = mfma(nai, bi, cr[ct]);
                        ci[ct] = mfma(ar, bi, ci[ct]);
                        ci[ct] = mfma(ai, br, ci[ct]);
                    }
                }
            }
        }
    }
    if (!active) return;
    const size_t plane = (size_t)P * P;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        if (16 * ct >= mw) continue;
        const int col = j0 + 16 * ct + (l & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + 16 * w + kq + 4 * r;
            const size_t a = (size_t)row * P + col;
            double vr = cr[ct][r], vi = ci[ct][r];
            if (o.X1) {  // B_j + A^4 x: the block first (c0 I + c1 A + c2 A^2 + c3 A^3), then the product
                double br = (row == col && row < g.d) ? o.c0 : 0.0, bi = 0.0;
                br = fma(o.c1, o.X1[a], br);
                bi = fma(o.c1, o.X1[plane + a], bi);
                br = fma(o.c2, o.X2[a], br);
                bi = fma(o.c2, o.X2[plane + a], bi);
                br = fma(o.c3, o.X3[a], br);
                bi = fma(o.c3, o.X3[plane + a], bi);
                vr = br + vr;
                vi = bi + vi;
            }
            o.C[a] = vr;
            o.C[plane + a] = vi;
        }
    }
}

// 1 / k!
__constant__ const double kInvFact[21] = {1.0, 1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040,
                                          1.0 / 40320, 1.0 / 362880, 1.0 / 3628800, 1.0 / 39916800,
                                          1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0,
                                          1.0 / 1307674368000.0, 1.0 / 20922789888000.0,
                                          1.0 / 355687428096000.0, 1.0 / 6402373705728000.0,
                                          1.0 / 121645100408832000.0, 1.0 / 2432902008176640000.0};

// (taylor_top, julia_m_index, make_ctl: grape_tiled_ctl.hpp, host-testable)

// Workgroup sum / max in a fixed order (deterministic); red: NTHREADS doubles of LDS
__device__ __forceinline__ double wg_sum(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double wg_max(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    return red[0];
}

}  // namespace grape_tiled
