"""The wide walks' step frame as a numpy model (csrc/grape_walk_merged.hpp wide_step_frame, wide_step_grad_frame;
DESIGN.md 4.2.4): the lab-frame recurrences the wide pass ran first and the step-frame recurrences it runs for
ladder charges, side by side.

One sector of S levels with ladder charges N_j = j: D_k = diag(p_k^j), p_k = e^{i a x_k}, E_k = D_k E~ D_k^dag with
E~ = exp(-i dt H) of a random Hermitian H.

  forward    lab    psi_k = E_k psi_{k-1}, psi_0 = e_c
             frame  chi_k = E~ diag(dl^j) chi_{k-1}, dl = e^{i a (x_{k-1} - x_k)}, x_0 = 0; psi_k = D_k chi_k
  gradient   lab    k = N .. 1:  psi_{k-1} = E_k^dag psi_k,  v_rj = conj(phi_k,r) (E_k)_rj,
                    z_rj = v_rj psi_{k-1},j,  T_m = sum_{r-j=m} z_rj + conj(sum_{r-j=-m} z_rj),
                    phi_{k-1},j = conj(sum_r v_rj);  phi_N = conj(alpha) e_c
             frame  (chi, eta) start as (psi_N, phi_N) with x_{N+1} = 0; per step dl = e^{i a (x_{k+1} - x_k)},
                    chi <- diag(dl^j) chi, eta <- diag(dl^j) eta (now D_k^dag psi_k, D_k^dag phi_k), then the lab
                    step with E~ for E_k: chi' = E~^dag chi = D_k^dag psi_{k-1}, the same z_rj entry by entry

Every per-step vector agrees to 1e-13 of its maximum, and every z_rj and T_m entry by entry.  The phases of the
model's dl come from the controls' difference, as the kernels take them.
"""
import numpy as np
import pytest

TOL = 1e-13
SIZES = (2, 3)
AS = (1.0, -2.5)
NTS = (1, 2, 17)


def _setup(S, a, nt, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(S, S)) + 1j * rng.normal(size=(S, S))
    H = (A + A.conj().T) / 2
    w, V = np.linalg.eigh(H)
    Et = (V * np.exp(-1j * 0.37 * w)) @ V.conj().T  # E~ = exp(-i dt H)
    x = rng.uniform(-7.0, 7.0, size=nt)
    c = int(rng.integers(S))
    alpha = complex(rng.normal(), rng.normal())
    return Et, x, c, alpha


def _D(a, xk, S):
    return np.exp(1j * a * xk * np.arange(S))


def _close(u, v, what):
    scale = max(float(np.max(np.abs(v))), 1e-300)
    err = float(np.max(np.abs(np.asarray(u) - np.asarray(v))))
    assert err <= TOL * scale, (what, err, scale)


def _grad_step(E, psi, phi):
    """one time-reversed step with propagator E: (psi_{k-1}, phi_{k-1}, z, T)"""
    S = len(psi)
    pm = E.conj().T @ psi
    v = phi.conj()[:, None] * E
    z = v * pm[None, :]
    T = np.zeros(S, complex)
    for r in range(S):
        for j in range(S):
            if r > j:
                T[r - j] += z[r, j]
            elif r < j:
                T[j - r] += np.conj(z[r, j])
    return pm, np.conj(v.sum(axis=0)), z, T


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("S", SIZES)
def test_forward_walk_in_the_step_frame(S, a, nt):
    Et, x, c, _ = _setup(S, a, nt, 100 * S + nt)
    psi = np.zeros(S, complex)
    psi[c] = 1.0
    chi, xprev = psi.copy(), 0.0
    for k in range(nt):
        d = _D(a, x[k], S)
        psi = (d[:, None] * Et * d.conj()[None, :]) @ psi
        chi = Et @ (np.exp(1j * a * (xprev - x[k]) * np.arange(S)) * chi)
        xprev = x[k]
        _close(d * chi, psi, ("psi", k))
    _close(_D(a, xprev, S) * chi, psi, "psi_N")  # the closing re-framing: the phase of a x_N


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("S", SIZES)
def test_gradient_walk_in_the_step_frame(S, a, nt):
    Et, x, c, alpha = _setup(S, a, nt, 200 * S + nt)
    psi = np.zeros(S, complex)
    psi[c] = 1.0
    for k in range(nt):
        d = _D(a, x[k], S)
        psi = (d[:, None] * Et * d.conj()[None, :]) @ psi
    phi = np.zeros(S, complex)
    phi[c] = np.conj(alpha)
    chi, eta, xlast = psi.copy(), phi.copy(), 0.0  # the lab frame: x "of the step before" is 0
    for k in range(nt - 1, -1, -1):
        d = _D(a, x[k], S)
        dl = np.exp(1j * a * (xlast - x[k]) * np.arange(S))
        xlast = x[k]
        chi, eta = dl * chi, dl * eta
        _close(d * chi, psi, ("chi re-framed", k))
        _close(d * eta, phi, ("eta re-framed", k))
        psi, phi, z0, T0 = _grad_step(d[:, None] * Et * d.conj()[None, :], psi, phi)
        chi, eta, z1, T1 = _grad_step(Et, chi, eta)
        _close(d * chi, psi, ("psi_{k-1}", k))
        _close(d * eta, phi, ("phi_{k-1}", k))
        scale = max(float(np.max(np.abs(z0))), 1e-300)
        assert np.all(np.abs(z1 - z0) <= TOL * scale), ("z entry by entry", k, float(np.max(np.abs(z1 - z0))), scale)
        assert np.all(np.abs(T1 - T0) <= TOL * scale), ("T_m entry by entry", k, float(np.max(np.abs(T1 - T0))), scale)


def test_the_model_tells_a_wrong_frame():
    """the checks above have teeth: dl conjugated, or eta left in the old frame, is seen at the first seam"""
    S, a, nt = 3, -2.5, 2
    Et, x, c, alpha = _setup(S, a, nt, 7)
    d1, d0 = _D(a, x[1], S), _D(a, x[0], S)
    psi = np.zeros(S, complex)
    psi[c] = 1.0
    psi = (d1[:, None] * Et * d1.conj()[None, :]) @ ((d0[:, None] * Et * d0.conj()[None, :]) @ psi)
    phi = np.conj(alpha) * np.array([0.3 - 0.4j, 1.0, -0.7 + 0.2j])  # (a phi with every level: as after one step)
    _, _, z0, _ = _grad_step(d1[:, None] * Et * d1.conj()[None, :], psi, phi)
    good = np.exp(1j * a * (0.0 - x[1]) * np.arange(S))
    for dchi, deta in ((good.conj(), good.conj()), (good, np.ones(S))):
        _, _, z1, _ = _grad_step(Et, dchi * psi, deta * phi)
        assert float(np.max(np.abs(z1 - z0))) > 1e-3 * float(np.max(np.abs(z0)))
    _, _, z1, _ = _grad_step(Et, good * psi, good * phi)
    assert float(np.max(np.abs(z1 - z0))) <= TOL * float(np.max(np.abs(z0)))
