"""numpy reference of the left EOM-CCSD eigenvectors, the two transition densities and the strengths.  TEST INFRASTRUCTURE ONLY.

Built from the oracles as ``_lambda_reference.py`` is: the dense right / left sigma come from ``dense_operators``, the densities
are derivatives with respect to the Fock matrix of expressions in ``oracle/cc_oracle.py``'s residuals and ``oracle/eom_oracle.py``'s
sigma, evaluated with unit matrices as Fock matrix and V = 0 (everything is linear in f).

For root k (vectors as in _lambda_reference: pairs (x1 [v,o], x2 [v,v,o,o]), plain inner product):
  gammaL_k[p,q] = d/df_pq ( <l1_k, R1(f)> + <l2_k, R2(f)> )
  gammaR_k[p,q] = d/df_pq ( 2 sum f~_ov[i,a] r1_k[a,i] + <lambda, A(f) r_k> + 2 sum lambda2[a,b,i,j] r1_k[a,i] R1(f)[b,j]
                            - <lambda, r_k> ( <lambda1, R1(f)> + <lambda2, R2(f)> ) )
  S_k(O) = (sum gammaL_k O) (sum gammaR_k O),   r0_k = -<lambda, r_k>,   <l_j, r_k> = delta_jk.
"""
import functools

import numpy as np
import scipy.linalg

from oracle import cc_oracle as cc
from oracle import eom_oracle as eo
from tests import _lambda_reference as R


def dot(x, y):
    return float((x[0] * y[0]).sum() + (x[1] * y[1]).sum())


# ---- the definitions ---------------------------------------------------------------------------------------------------------------
def transition_densities_definition(no, t1, t2, lam, ls, rs):
    """(gammaL [k,n,n], gammaR [k,n,n]) by the definition: one evaluation of R1(f), R2(f), A(f) r_k per unit matrix."""
    nv = t1.shape[0]
    n, k = no + nv, len(ls)
    Vb = cc.split_blocks(no, np.zeros((n, n, n, n)))
    Vd = cc.dressed_V(t1, Vb)
    ein = functools.partial(np.einsum, optimize=True)
    gl, gr = np.zeros((k, n, n)), np.zeros((k, n, n))
    for p in range(n):
        for q in range(n):
            e = np.zeros((n, n))
            e[p, q] = 1.0
            fd = cc.dressed_fock(no, e, t1, Vb)
            r1 = cc.singles_residual(no, fd, t1, t2, Vb)
            r2 = cc.ccsd_doubles_residual(no, fd, t2, Vd, ein=ein)
            lag = dot(lam, (r1, r2))
            for z in range(k):
                gl[z, p, q] = dot(ls[z], (r1, r2))
                u1, u2 = rs[z]
                s = (eo.sigma_singles(no, fd, Vd, u1, u2, t2), eo.sigma_doubles(no, fd, Vd, u1, u2, t2))
                gr[z, p, q] = (2.0 * (fd[:no, no:] * u1.T).sum() + dot(lam, s)
                               + 2.0 * np.einsum("abij,ai,bj->", lam[1], u1, r1) - dot(lam, rs[z]) * lag)
    return gl, gr


# ---- the same written out: the coefficients C of the T1-dressed Fock matrix, then the dressing undone ------------------------------
def _lagrange_coefficients(no, t2, l1, l2):
    """C[p,q] = d/df~_pq ( <l1, R1> + <l2, R2> ): the blocks of ``density_terms`` without the energy's 2 t1."""
    n = no + l1.shape[0]
    c = np.zeros((n, n))
    c[no:, :no] = l1
    c[:no, :no] = -2.0 * np.einsum("abij,abkj->ki", l2, t2)
    c[no:, no:] = 2.0 * np.einsum("abij,cbij->ac", l2, t2)
    c[:no, no:] = np.einsum("ai,abij->jb", l1, 2.0 * t2 - t2.transpose(0, 1, 3, 2))
    return c


def _undress(no, c, t1):
    """d/df from d/df~: f~_oo = f_oo + f_ov t1, f~_vv = f_vv - t1 f_ov, f~_vo = f_vo + f_vv t1 - t1 f_oo - t1 f_ov t1."""
    g = np.zeros_like(c)
    coo, cov, cvo, cvv = c[:no, :no], c[:no, no:], c[no:, :no], c[no:, no:]
    g[no:, :no] = cvo
    g[:no, :no] = coo - t1.T @ cvo
    g[no:, no:] = cvv + cvo @ t1.T
    g[:no, no:] = cov + g[:no, :no] @ t1.T - t1.T @ cvv
    return g


def left_density_terms(no, t1, t2, l1, l2):
    return _undress(no, _lagrange_coefficients(no, t2, l1, l2), t1)


def right_density_terms(no, t1, t2, lam1, lam2, r1, r2):
    """The four terms of gammaR as contractions (the ones the device kernel assembles)."""
    s = float((lam1 * r1).sum() + (lam2 * r2).sum())
    yoo = np.einsum("abij,abkj->ki", lam2, t2)
    yvv = np.einsum("abij,cbij->ac", lam2, t2)
    leff = 2.0 * np.einsum("abij,ai->bj", lam2, r1)                      # term 3: R1(f) against 2 lambda2 . r1
    c = _lagrange_coefficients(no, t2, leff, np.zeros_like(t2)) - s * _lagrange_coefficients(no, t2, lam1, lam2)
    # <lambda, A(f) r> (the rows with an f operand of eom_oracle's tables; the permuted doubles rows see 2 lambda2)
    c[:no, :no] += -np.einsum("aj,ai->ji", r1, lam1) - 2.0 * np.einsum("abij,abkj->ki", lam2, r2)
    c[no:, no:] += np.einsum("ai,bi->ab", lam1, r1) + 2.0 * np.einsum("abij,cbij->ac", lam2, r2)
    c[:no, no:] += (2.0 * r1.T + np.einsum("ai,abij->jb", lam1, 2.0 * r2 - r2.transpose(0, 1, 3, 2))
                    - 2.0 * yoo @ r1.T - 2.0 * r1.T @ yvv)
    return _undress(no, c, t1)


def transition_density_terms(no, t1, t2, lam, ls, rs):
    gl = np.stack([left_density_terms(no, t1, t2, *l) for l in ls])
    gr = np.stack([right_density_terms(no, t1, t2, lam[0], lam[1], *r) for r in rs])
    return gl, gr


# ---- the dense eigenproblem ------------------------------------------------------------------------------------------------------
def dense_eom(no, fd, Vd, t2, nroots):
    """(w [k], rs, ls, complex) of the k lowest roots of scipy.linalg.eig(B^T A B, B^T B, left=True), biorthonormalised by the
    inverse of G_jk = <l_j, r_k>.  ``complex``: the largest imaginary part among the roots taken."""
    co, BA, _ = R.dense_operators(no, fd, Vd, t2)
    G = co.B.T @ co.B
    w, vl, vr = scipy.linalg.eig(BA, G, left=True)
    pick = np.argsort(w.real)[:nroots]
    imag = float(np.abs(w[pick].imag).max())
    rs = [co.split(co.B @ vr[:, p].real) for p in pick]
    rs = [(r[0] / np.sqrt(dot(r, r)), r[1] / np.sqrt(dot(r, r))) for r in rs]          # unit norm; the sign stays arbitrary
    # a left eigenvector y of the pencil (y^T BA = w y^T G) is the coordinate vector of the left vector itself
    ls = [co.split(co.B @ vl[:, p].real) for p in pick]
    if imag == 0.0:                # (a complex pair has no real vectors to normalise: the caller refuses such a root)
        ls = biorthonormalise(ls, rs)
    return w[pick].real.copy(), rs, ls, imag


def biorthonormalise(ls, rs):
    g = np.array([[dot(l, r) for r in rs] for l in ls])
    gi = np.linalg.inv(g)
    return [(sum(gi[j, m] * ls[m][0] for m in range(len(ls))), sum(gi[j, m] * ls[m][1] for m in range(len(ls))))
            for j in range(len(ls))]


def strengths(gl, gr, O):
    return np.array([(gl[z] * O).sum() * (gr[z] * O).sum() for z in range(gl.shape[0])])


def nonhermitian_variant(f, V, seed):
    """The mild non-hermitian variant of an 8-fold problem: V + W + W^T(1,0,3,2), W = 0.002 N(0,1); f + 0.005 N(0,1)."""
    rng = np.random.default_rng(seed + 1000)
    n = f.shape[0]
    W = 0.002 * rng.standard_normal((n, n, n, n))
    V = V + W + W.transpose(1, 0, 3, 2)
    return f + 0.005 * rng.standard_normal((n, n)), V


def problem(no, nv, seed, hermitian=True, scale=0.02):
    f, V = R.random_problem(no, nv, seed, eight=True, scale=scale)
    return (f, V) if hermitian else nonhermitian_variant(f, V, seed)


@functools.lru_cache(maxsize=None)
def reference_transitions(no, nv, seed, hermitian=True, nroots=3, scale=0.02):
    """Everything of one test problem, dense: a dictionary with f, V, the converged state, lambda, w, rs, ls, the densities."""
    f, V = problem(no, nv, seed, hermitian, scale)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V)
    t2 = 0.5 * R.symd(t2)          # (the oracle's iteration leaves an exchange-antisymmetric part of 1e-7 that the solution does not have)
    lam = R.solve_lambda(no, fd, Vd, t2)
    w, rs, ls, imag = dense_eom(no, fd, Vd, t2, nroots)
    gl, gr = transition_density_terms(no, t1, t2, lam, ls, rs)
    return dict(f=f, V=V, t1=t1, t2=t2, fd=fd, Vd=Vd, lam=lam, w=w, rs=rs, ls=ls, imag=imag, gl=gl, gr=gr)


def seeded_operator(n, seed=21):
    O = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (O + O.T)


# ---- exact two-electron calculation: singlet FCI in the symmetric coefficients C_pq -----------------------------------------------
def two_electron_fci(f, V, O):
    """(gaps of the excited singlets above the ground state [m], <0|O|k>^2 [m]) for no = 1: h = f - (2 V_piqi - V_piiq)."""
    n = f.shape[0]
    h = f - (2.0 * V[:, 0, :, 0] - V[:, 0, 0, :])
    basis = []
    for p in range(n):
        for q in range(p, n):
            c = np.zeros((n, n))
            c[p, q] = c[q, p] = 1.0
            basis.append(c / np.linalg.norm(c))
    op = lambda m, c: m @ c + c @ m.T
    H = np.array([[(b * (op(h, c) + np.einsum("pqrs,rs->pq", V, c))).sum() for c in basis] for b in basis])
    e, x = np.linalg.eigh(0.5 * (H + H.T))
    assert np.abs(H - H.T).max() < 1e-12
    cs = [sum(x[m, z] * basis[m] for m in range(len(basis))) for z in range(len(e))]
    mom = np.array([(cs[0] * op(O, c)).sum() for c in cs[1:]])
    return e[1:] - e[0], mom ** 2


# ---- the densities by definition at (6,17), recorded (python -m tests._transition_reference rewrites the file) --------------------
def density_inputs(no, nv, seed, k=3):
    """Random (t1, t2, lambda, ls, rs) with exchange-symmetric doubles; they need not solve anything."""
    rng = np.random.default_rng(seed)
    s1 = lambda: 0.1 * rng.standard_normal((nv, no))
    s2 = lambda: R.symd(0.05 * rng.standard_normal((nv, nv, no, no)))
    t1, t2 = s1(), s2()
    lam = (s1(), s2())
    ls = [(s1(), s2()) for _ in range(k)]
    rs = [(s1(), s2()) for _ in range(k)]
    return t1, t2, lam, ls, rs


GOLDEN_TDM1 = ("tdm1_6_17.npz", 6, 17, 9)          # file, no, nv, seed


if __name__ == "__main__":
    import os
    name, no, nv, seed = GOLDEN_TDM1
    gl, gr = transition_densities_definition(no, *density_inputs(no, nv, seed))
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), left=gl, right=gr)
