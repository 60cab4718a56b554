// grape_fd_weight.hpp -- the finite-difference weights rho(m) = e^{i m phi} - 1 of the phase-covariant walks
// (grape_walk_gauge.hpp: (E'_k - E_k)_rj = E_rj rho(N_r - N_j), phi = a ((x_k + eps) - x_k)), on plain doubles so
// that a host compiler builds the same source (tests/c/fd_weight_check.cpp, as grape_cis.hpp).
//
// Per step (every walk but the wide gradient walk): q = cis_m1(phi), rho(m) by the recurrence rho_next.
//
// Base plus first-order term (the wide gradient walk).  phi is a eps up to the rounding of x_k + eps: the same
// number in every lane and step to about eleven digits.  So once per kernel, with phi0 = fl(a eps), the same
// cis_m1 and the same recurrence give rho0(m) (fd_base), and a step takes
//   dh = h - eps  (h = (x_k + eps) - x_k; exact, as h is, wherever the fast form is taken: |dh| <= eps / 2),
//   rho(m) = rho0(m) + dh ga(m),   ga(m) = a g(m),  g(m) = i m (1 + rho0(m)) = d rho / d phi at phi0:
// two FMAs per weight, the step's phase being phi0 + dphi with dphi = a dh.  Whenever h == eps, dh is exactly 0 and
// the weights are the per-step form's bit for bit (there phi = fl(a eps) = phi0; a dphi taken as fma(a, h, -phi0)
// would carry the rounding error of a eps, up to half a unit of phi0's last place, into every weight).  For
// h != eps the phase phi0 + a dh differs from the per-step form's fl(a h) by roundings of a eps and a h alone.
// What the first-order form drops: with y = m dphi, e^{i m phi} - 1 = rho0 + (1 + rho0)(e^{i y} - 1) and
// |e^{i y} - 1 - i y| <= y^2 / 2, |1 + rho0| = 1, so the dropped term is at most (m dphi)^2 / 2.
// Guard (fd_threshold): the fast form is taken only for |dphi| <= T, i.e. |dh| <= T / |a| (fd_threshold_h),
//   T = min(|phi0| / 2, sqrt(2^-55 |phi0|) / m_max),   and only if m_max |phi0| <= 1/2.
// Then |phi| >= |phi0| / 2 and m |phi| <= 3/4, so |rho(m)| = 2 |sin(m phi / 2)| >= 0.976 m |phi| >= 0.488 |phi0|,
// and (m dphi)^2 / 2 <= 2^-56 |phi0| < 2^-54 |rho(m)|: below half a unit of the last place of |rho(m)|, which
// is at least 2^-53 |rho(m)|.  Everything else (x + eps rounding to x or to x + 2 eps at huge |x|, a NaN, a phase
// step too large for the bound) takes cis_m1 and the recurrence.
#pragma once

#include <hip/hip_runtime.h>

namespace grape_fd {

struct Z {
    double re, im;
};

__host__ __device__ __forceinline__ double sin_small(double t) {  // sin t, |t| <= 0.05: Taylor to t^9
    const double t2 = t * t;
    return t * fma(t2, fma(t2, fma(t2, fma(t2, 1.0 / 362880.0, -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0), 1.0);
}
// e^{i phi} - 1 without cancellation: (-2 sin^2(phi / 2), sin phi); Taylor for the FD-sized
// phases (|phi| <= 0.05: truncation below 1e-22 relative), the library otherwise
__host__ __device__ __forceinline__ Z cis_m1(double phi) {
    if (fabs(phi) <= 0.05) {
        const double sh = sin_small(0.5 * phi);
        return Z{-2.0 * sh * sh, sin_small(phi)};
    }
    const double sh = sin(0.5 * phi);
    return Z{-2.0 * sh * sh, sin(phi)};
}
// rho(m + 1) = rho(m) + q + q rho(m) from rho(1) = q (the operations of gauge_fd_weights_dn and ladder_rho)
__host__ __device__ __forceinline__ Z rho_next(Z q, Z z) {
    return Z{(z.re + q.re) + fma(q.re, z.re, -(q.im * z.im)), (z.im + q.im) + fma(q.re, z.im, q.im * z.re)};
}
__host__ __device__ __forceinline__ Z rho_pow(Z q, int m) {  // rho(m), m >= 1
    Z z = q;
    for (int i = 1; i < m; ++i) z = rho_next(q, z);
    return z;
}

// One weight's base: rho0 = e^{i dn phi0} - 1 for the signed charge difference dn (conjugated for dn < 0, exactly
// zero for dn = 0, as gauge_fd_weights_dn forms it) and g = i dn (1 + rho0)
struct Base {
    Z rho0, g;
};
__host__ __device__ __forceinline__ Base fd_base_signed(Z r, int dn) {  // r = rho0 itself (zero for dn = 0)
    return Base{r, Z{-(double)dn * r.im, (double)dn * (1.0 + r.re)}};
}
__host__ __device__ __forceinline__ Base fd_base_from(Z rho_abs, int dn) {  // rho_abs = rho(|dn|) (unused for dn = 0)
    if (dn == 0) return Base{Z{0.0, 0.0}, Z{0.0, 0.0}};
    return fd_base_signed(Z{rho_abs.re, dn < 0 ? -rho_abs.im : rho_abs.im}, dn);
}
__host__ __device__ __forceinline__ Base fd_base(double phi0, int dn) {
    return fd_base_from(rho_pow(cis_m1(phi0), dn < 0 ? -dn : dn), dn);
}
// the guard's bound on |dphi| (negative: never the fast form), and the same bound on |dh| = |dphi| / |a|
__host__ __device__ __forceinline__ double fd_threshold(double phi0, int m_max) {
    const double p = fabs(phi0);
    if (!(m_max >= 1) || !(p > 0.0) || !((double)m_max * p <= 0.5)) return -1.0;
    return fmin(0.5 * p, sqrt(0x1p-55 * p) / (double)m_max);
}
__host__ __device__ __forceinline__ double fd_threshold_h(double a, double eps, int m_max) {
    const double t = fd_threshold(a * eps, m_max);
    return t < 0.0 ? -1.0 : t / fabs(a);  // (phi0 != 0 here, so a != 0)
}
// ga = a g: the base's derivative with respect to h
__host__ __device__ __forceinline__ Base fd_base_h(Base b, double a) { return Base{b.rho0, Z{a * b.g.re, a * b.g.im}}; }
// rho0 + d g (d = dphi with fd_base's g, d = dh with fd_base_h's)
__host__ __device__ __forceinline__ Z fd_step(const Base &b, double d) {
    return Z{fma(d, b.g.re, b.rho0.re), fma(d, b.g.im, b.rho0.im)};
}

}  // namespace grape_fd
