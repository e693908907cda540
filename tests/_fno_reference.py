"""numpy restatement of the frozen-natural-orbital definitions (pymes_amd/solver/fno.py, include/pymes_amd.h): the MP2
virtual density and energy over an occupied window, the natural orbitals with the sign rule, the semicanonical kept
virtuals and the transformed integrals of the new space."""
import numpy as np


def mp2_amplitudes(no, f, V, n_frozen=0):
    """t[a,b,i,j] = V_ijab / (eps_i + eps_j - eps_a - eps_b) over occupied [n_frozen, no) and all virtuals."""
    eps = np.diag(f)
    eo, ev = eps[n_frozen:no], eps[no:]
    Vijab = V[n_frozen:no, n_frozen:no, no:, no:]
    d = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    return (Vijab / d).transpose(2, 3, 0, 1), Vijab


def mp2_density(no, f, V, n_frozen=0):
    """(D_ab = 2 sum_cij (2 t_acij - t_caij) t_bcij, E_MP2 = sum (2 t_abij - t_baij) V_ijab)."""
    t, Vijab = mp2_amplitudes(no, f, V, n_frozen)
    tt = 2.0 * t - t.transpose(1, 0, 2, 3)
    D = 2.0 * np.einsum("acij,bcij->ab", tt, t, optimize=True)
    e = float(np.einsum("abij,ijab->", tt, Vijab, optimize=True))
    return D, e


def mp2_density_ijab(Vijab, eps_o, eps_v, n_frozen=0):
    """``mp2_density`` from V_ijab [no,no,v,v] and the orbital energies alone (no n^4 V_pqrs): the same D and E_MP2 over
    occupied [n_frozen, no) and all virtuals."""
    eo, ev = np.asarray(eps_o)[n_frozen:], np.asarray(eps_v)
    V = np.asarray(Vijab)[n_frozen:, n_frozen:]
    d = eo[:, None, None, None] + eo[None, :, None, None] - ev[None, None, :, None] - ev[None, None, None, :]
    t = (V / d).transpose(2, 3, 0, 1)
    tt = 2.0 * t - t.transpose(1, 0, 2, 3)
    D = 2.0 * np.einsum("acij,bcij->ab", tt, t, optimize=True)
    e = float(np.einsum("abij,ijab->", tt, V, optimize=True))
    return D, e


def sign_rule(M):
    M = M.copy()
    for k in range(M.shape[1]):
        if M[np.argmax(np.abs(M[:, k])), k] < 0:
            M[:, k] *= -1.0
    return M


def fno_space(no, f, V, n_frozen=0, nv_keep=None):
    """(U [n, n'] with occupied [n_frozen, no) unrotated and the kept semicanonical natural virtuals, occupations,
    E_MP2 full, D)."""
    n = f.shape[0]
    nv = n - no
    D, e = mp2_density(no, f, V, n_frozen)
    occ, vec = np.linalg.eigh(D)
    order = np.argsort(-occ, kind="stable")
    occ, vec = occ[order], sign_rule(vec[:, order])
    k = nv if nv_keep is None else nv_keep
    if nv_keep is None:
        Cm = np.eye(nv)
    else:
        N = vec[:, :k]
        F = N.T @ f[no:, no:] @ N
        w, W = np.linalg.eigh(0.5 * (F + F.T))
        Cm = sign_rule(N @ W)
    U = np.zeros((n, no - n_frozen + k))
    U[n_frozen:no, :no - n_frozen] = np.eye(no - n_frozen)
    U[no:, no - n_frozen:] = Cm
    return U, occ, e, D


def transform(V, U):
    return np.einsum("pqrs,pw,qx,ry,sz->wxyz", V, U, U, U, U, optimize=True)
