"""Numpy restatement of the sector spectral functions (pymes_amd/solver/ueg_eom.py, SectorSpectralFunction): the Arnoldi
process with two rounds of classical Gram-Schmidt from the singles unit vector, the diagonal resolvent element from the Hessenberg
matrix alone, its residual estimate, and the poles and residues of the Ritz decomposition.

With s = +1 for IP and -1 for EA, G(z) = N_p [(z + s H)^-1]_11, approximated in K_m(H, e_1) by [(z + s H_m)^-1]_11 because
v_1 = e_1; the residual of x_m = V_m y, (z + s H_m) y = e_1, is -s h_{m+1,m} y_m v_{m+1}.  What the CPU tests check of it
(tests/test_sector_gf_reference.py) and what the HIP path is compared with on the GPU."""
import numpy as np

SIGN = {"ip": 1.0, "ea": -1.0}


def cgs2_step(V, w, breakdown=0.0):
    """One step as pymes_sector_arnoldi_step takes it: V [j+1, len] orthonormal rows, w = H v_j.  Returns (the column h + h' of
    j + 1 elements, |w''|, w'' / |w''|), or (column, 0.0, zeros) on breakdown (not |w''| > breakdown |w|)."""
    h1 = V @ w
    w1 = w - V.T @ h1
    h2 = V @ w1
    w2 = w1 - V.T @ h2
    nrm = np.linalg.norm(w2)
    if not nrm > breakdown * np.linalg.norm(w):
        return h1 + h2, 0.0, np.zeros_like(w)
    return h1 + h2, nrm, w2 / nrm


def arnoldi(H, m, breakdown=1e-10, start=0):
    """(V [k+1, n], Hbar [k+1, k], k, broke): at most m steps from the unit vector ``start``; on breakdown at step j the space is
    invariant, k = j + 1, Hbar[k, k-1] = 0 exactly and the row k of V is zero."""
    n = H.shape[0]
    V, Hb = np.zeros((m + 1, n)), np.zeros((m + 1, m))
    V[0, start] = 1.0
    for j in range(m):
        col, nrm, v = cgs2_step(V[:j + 1], H @ V[j], breakdown)
        Hb[:j + 1, j], Hb[j + 1, j], V[j + 1] = col, nrm, v
        if nrm == 0.0:
            return V[:j + 2], Hb[:j + 2, :j + 1], j + 1, True
    return V, Hb, m, False


def shifted_solutions(Hbar, kind, z):
    """y(z) [len(z), k] of (z + s H_k) y = e_1 for every shift, and the residual estimates h_{k+1,k} |y_k|."""
    k = Hbar.shape[1]
    Hk, s = Hbar[:k], SIGN[kind]
    e1 = np.zeros(k)
    e1[0] = 1.0
    Y = np.array([np.linalg.solve(zz * np.eye(k) + s * Hk, e1) for zz in np.atleast_1d(z)])
    return Y, abs(Hbar[k, k - 1]) * np.abs(Y[:, -1])


def greens_function(Hbar, kind, z, norm=1.0):
    """(G(z), residual estimates) from the Hessenberg matrix alone."""
    Y, res = shifted_solutions(Hbar, kind, z)
    return norm * Y[:, 0], res


def exact_resolvent(H, kind, z, start=0):
    """[(z + s H)^-1]_{start,start} by a dense solve per shift."""
    n, s = H.shape[0], SIGN[kind]
    e = np.zeros(n)
    e[start] = 1.0
    return np.array([np.linalg.solve(zz * np.eye(n) + s * H, e)[start] for zz in np.atleast_1d(z)])


def resolvent_norm(H, kind, z):
    """||(z + s H)^-1||_2 = 1 / the smallest singular value."""
    n, s = H.shape[0], SIGN[kind]
    return 1.0 / np.linalg.svd(z * np.eye(n) + s * H, compute_uv=False).min()


def true_residual(H, kind, z, V, y, start=0):
    """|e - (z + s H) V_k^T y|."""
    k = len(y)
    x = V[:k].T @ y
    e = np.zeros(H.shape[0], dtype=complex)
    e[start] = 1.0
    return np.linalg.norm(e - (z * x + SIGN[kind] * (H @ x)))


def poles(Hbar, kind, norm=1.0):
    """(pole energies -s theta_j, strengths Z_j = N_p S_1j (S^-1)_j1, residuals h_{k+1,k} |S_kj| / |S_:j|, theta) of the Ritz
    decomposition H_k = S theta S^-1, all complex."""
    k = Hbar.shape[1]
    theta, S = np.linalg.eig(Hbar[:k])
    rho = S[0, :] * np.linalg.inv(S)[:, 0]
    res = abs(Hbar[k, k - 1]) * np.abs(S[-1, :]) / np.linalg.norm(S, axis=0)
    return -SIGN[kind] * theta.astype(complex), norm * rho.astype(complex), res, theta


def quasiparticle(energies, strengths, residuals, r_epsilon):
    """The real pole of largest |Z_j| among those whose residual lies below r_epsilon: (energy, Z), NaN where there is none."""
    ok = (residuals < r_epsilon) & (np.abs(energies.imag) <= 1e-12 * np.maximum(1.0, np.abs(energies.real)))
    if not ok.any():
        return np.nan, np.nan
    j = np.flatnonzero(ok)[np.argmax(np.abs(strengths[ok]))]
    return float(energies[j].real), float(strengths[j].real)
