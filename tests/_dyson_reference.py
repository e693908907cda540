"""numpy reference of the left IP / EA-EOM-CCSD vectors, the Dyson amplitudes and the pole strengths (DESIGN.md 8f;
include/pymes_amd.h, pymes_ipea_sigma_apply_left / pymes_ipea_dyson).  TEST INFRASTRUCTURE ONLY.

Definitions.  H is the IP / EA operator of ``_ipea_reference`` on the compact vectors (r1, r2) (IP r1[i], r2[i,j,b]; EA r1[a],
r2[a,b,j]), <x, y> the plain sum over both arrays.

D1  left vectors: H^T l_k = w_k l_k, <l_j, r_k> = delta_jk against unit-norm right vectors.
D2  Dyson amplitudes, from the EE transition densities (``_transition_reference.transition_densities_definition``) of the problem
    with one more orbital x that interacts with nothing, T and Lambda zero in x:
      b_p = the restriction of d(R1, R2)/df_xp (IP) or d(R1, R2)/df_px (EA) to the sector, ONE copy, as sigma is restricted:
            [x,b,i,j] -> [i,j,b] (IP), [a,b,x,j] -> [a,b,j] (EA)
      e_q = ONE HALF of r -> gammaR[q,x] (IP) / gammaR[x,q] (EA) on the embedded exchange-symmetric vector of r
      psiL_k(p) = <l_k, b_p>,   psiR_k(q) = <e_q, r_k>         (p, q over the n orbitals, occupied first)
D3  Z_k[q,p] = psiR_k(q) psiL_k(p),  P_k = sum_p psiR_k(p) psiL_k(p),
    A_pq(w) = (1/pi) sum_k Z_k[p,q] eta / ((w - eps_k)^2 + eta^2),  eps_k = -w_k (IP), +w_k (EA)
D4  sum_c e_q[c] b_p[c] = rdm1[q,p] / 2 (IP),  delta_qp - rdm1[p,q] / 2 (EA)      (identities in t1, t2, lambda1, lambda2)

Written out (``dyson_terms``; t = T2, Yoo[k,i] = sum lam2[a,b,i,j] t[a,b,k,j], Yvv[a,c] = sum lam2[a,b,i,j] t[c,b,i,j]):
  IP  psiL(i) = l1[i]                             psiL(a) = sum_i l1[i] t1[a,i] + sum l2[i,j,b] t[a,b,i,j]
      psiR(a) = sum_i lam1[a,i] r1[i] / 2 + sum lam2[a,b,i,j] r2[i,j,b]
      psiR(j) = r1[j] + sum lam1[a,i] (2 r2[j,i,a] - r2[i,j,a]) / 2 - sum_i Yoo[j,i] r1[i] - sum_a t1[a,j] psiR(a)
  EA  psiL(a) = l1[a]                             psiL(k) = -sum_a t1[a,k] l1[a] - sum l2[a,b,j] t[a,b,k,j]
      psiR(i) = -sum_a r1[a] lam1[a,i] / 2 - sum lam2[a,b,i,j] r2[a,b,j]
      psiR(b) = r1[b] + sum lam1[a,i] (2 r2[b,a,i] - r2[a,b,i]) / 2 - sum_a r1[a] Yvv[a,b] + sum_i psiR(i) t1[b,i]
so b_i = the unit single and b_a = (t1[a,:], t[a,b,i,j]) for IP; b_a = the unit single and b_k = -(t1[:,k], t[a,b,k,j]) for EA.
"""
import functools

import numpy as np
import scipy.linalg

from oracle import cc_oracle as cc
from oracle import eom_oracle as eo
from tests import _ipea_reference as IR
from tests import _lambda_reference as LR


def dot(x, y):
    return float((x[0] * y[0]).sum() + (x[1] * y[1]).sum())


def flat(x):
    return np.concatenate([x[0].ravel(), x[1].ravel()])


def split(kind, no, nv, y):
    s1, s2 = IR.shapes(kind, no, nv)
    n1 = int(np.prod(s1))
    return y[:n1].reshape(s1).copy(), y[n1:].reshape(s2).copy()


# ---- D2 by the definition: only the x row and the x column of the augmented densities ---------------------------------------------
def _augmented(kind, no, t1, t2, lam):
    """(no', x, index of orbital p in the augmented basis, padded t1, t2, lambda)."""
    nv = t1.shape[0]
    if kind == "ip":                  # x: one more virtual, the last
        pad1 = lambda a: np.concatenate([a, np.zeros((1, no))], axis=0)
        pad2 = lambda a: np.pad(a, ((0, 1), (0, 1), (0, 0), (0, 0)))
        return no, no + nv, (lambda p: p), pad1(t1), pad2(t2), (pad1(lam[0]), pad2(lam[1]))
    pad1 = lambda a: np.concatenate([np.zeros((nv, 1)), a], axis=1)
    pad2 = lambda a: np.pad(a, ((0, 0), (0, 0), (1, 0), (1, 0)))
    return no + 1, 0, (lambda p: p + 1), pad1(t1), pad2(t2), (pad1(lam[0]), pad2(lam[1]))


def embed(kind, no, nv, r1, r2):
    """The exchange-symmetric EE vector of (r1, r2) in the augmented problem (``_ipea_reference.sigma_embedded``)."""
    if kind == "ip":
        u1, u2 = np.zeros((nv + 1, no)), np.zeros((nv + 1, nv + 1, no, no))
        u1[nv] = r1
        u2[nv, :nv] = r2.transpose(2, 0, 1)
        u2[:nv, nv] = r2.transpose(2, 1, 0)
        return u1, u2
    u1, u2 = np.zeros((nv, no + 1)), np.zeros((nv, nv, no + 1, no + 1))
    u1[:, 0] = r1
    u2[:, :, 0, 1:] = r2
    u2[:, :, 1:, 0] = r2.transpose(1, 0, 2)
    return u1, u2


def restrict(kind, no, nv, x1, x2):
    """One copy of the sector: [x,b,i,j] -> [i,j,b] (IP), [a,b,x,j] -> [a,b,j] (EA)."""
    if kind == "ip":
        return x1[nv].copy(), x2[nv, :nv].transpose(1, 2, 0).copy()
    return x1[:, 0].copy(), x2[:, :, 0, 1:].copy()


def dyson_definition(kind, no, t1, t2, lam, ls, rs):
    """(psiL [k,n], psiR [k,n]) by D2: n residual evaluations for b, n functionals for e."""
    nv = t1.shape[0]
    n, k = no + nv, len(ls)
    no2, x, at, T1, T2, LAM = _augmented(kind, no, t1, t2, lam)
    m = n + 1
    Vb = cc.split_blocks(no2, np.zeros((m, m, m, m)))
    Vd = cc.dressed_V(T1, Vb)
    ein = functools.partial(np.einsum, optimize=True)
    us = [embed(kind, no, nv, *r) for r in rs]

    def residuals(p, q):
        e = np.zeros((m, m))
        e[p, q] = 1.0
        fd = cc.dressed_fock(no2, e, T1, Vb)
        return fd, cc.singles_residual(no2, fd, T1, T2, Vb), cc.ccsd_doubles_residual(no2, fd, T2, Vd, ein=ein)

    psiL, psiR = np.zeros((k, n)), np.zeros((k, n))
    for p in range(n):
        _, r1, r2 = residuals(*((x, at(p)) if kind == "ip" else (at(p), x)))
        b = restrict(kind, no, nv, r1, r2)
        for z in range(k):
            psiL[z, p] = dot(ls[z], b)
        fd, r1, r2 = residuals(*((at(p), x) if kind == "ip" else (x, at(p))))
        lag = dot(LAM, (r1, r2))
        for z in range(k):
            u1, u2 = us[z]
            s = (eo.sigma_singles(no2, fd, Vd, u1, u2, T2), eo.sigma_doubles(no2, fd, Vd, u1, u2, T2))
            gr = (2.0 * (fd[:no2, no2:] * u1.T).sum() + dot(LAM, s) + 2.0 * np.einsum("abij,ai,bj->", LAM[1], u1, r1)
                  - dot(LAM, us[z]) * lag)
            psiR[z, p] = 0.5 * gr
    return psiL, psiR


# ---- the same written out (what the device assembles) -------------------------------------------------------------------------------
def dyson_terms(kind, no, t1, t2, lam1, lam2, l, r):
    """(psiL [n], psiR [n]) of one pair of vectors l = (l1, l2), r = (r1, r2)."""
    nv = t1.shape[0]
    l1, l2 = l
    r1, r2 = r
    pl, pr = np.zeros(no + nv), np.zeros(no + nv)
    if kind == "ip":
        yoo = np.einsum("abij,abkj->ki", lam2, t2)
        pl[:no] = l1
        pl[no:] = t1 @ l1 + np.einsum("ijb,abij->a", l2, t2)
        pv = 0.5 * lam1 @ r1 + np.einsum("abij,ijb->a", lam2, r2)
        pr[no:] = pv
        pr[:no] = r1 + 0.5 * np.einsum("ai,jia->j", lam1, 2.0 * r2 - r2.transpose(1, 0, 2)) - yoo @ r1 - t1.T @ pv
        return pl, pr
    yvv = np.einsum("abij,cbij->ac", lam2, t2)
    pl[no:] = l1
    pl[:no] = -t1.T @ l1 - np.einsum("abj,abkj->k", l2, t2)
    po = -0.5 * r1 @ lam1 - np.einsum("abij,abj->i", lam2, r2)
    pr[:no] = po
    pr[no:] = r1 + 0.5 * np.einsum("ai,bai->b", lam1, 2.0 * r2 - r2.transpose(1, 0, 2)) - r1 @ yvv + t1 @ po
    return pl, pr


def dyson_matrices(kind, no, t1, t2, lam1, lam2):
    """(B [dim,n], E [dim,n]): the vectors b_p and the functionals e_q as columns, from the written-out terms."""
    nv = t1.shape[0]
    dim, n = IR.dim(kind, no, nv), no + nv
    B, E = np.zeros((dim, n)), np.zeros((dim, n))
    for c in range(dim):
        u = np.zeros(dim)
        u[c] = 1.0
        x = split(kind, no, nv, u)
        B[c], E[c] = dyson_terms(kind, no, t1, t2, lam1, lam2, x, x)
    return B, E


def sum_rule(kind, no, t1, t2, lam1, lam2):
    """D4's right-hand side [q,p]."""
    g = LR.rdm1(no, t1, t2, lam1, lam2)
    return 0.5 * g if kind == "ip" else np.eye(g.shape[0]) - 0.5 * g.T


# ---- D3 ---------------------------------------------------------------------------------------------------------------------------
def residues(psiL, psiR):
    return np.einsum("kq,kp->kqp", psiR, psiL)


def pole_strengths(psiL, psiR):
    return (psiL * psiR).sum(axis=1)


def spectral_function(kind, w, psiL, psiR, omegas, eta):
    eps = -np.asarray(w) if kind == "ip" else np.asarray(w)
    lor = eta / ((np.asarray(omegas)[:, None] - eps[None, :]) ** 2 + eta ** 2) / np.pi
    return np.einsum("wk,kpq->wpq", lor, residues(psiL, psiR))


# ---- the adjoint of the term tables -------------------------------------------------------------------------------------------------
def _adjoint(tab):
    out = []
    for c, spec, names in tab:
        ins, res = spec.split("->")
        ins = ins.split(",")
        k = [i for i, nm in enumerate(names) if nm in ("r1", "r2")]
        assert len(k) == 1, "every row is linear in exactly one of r1 / r2"
        target = ins[k[0]]
        ins[k[0]] = res
        out.append((c, ",".join(ins) + "->" + target, names, k[0]))
    return tuple(out)


LEFT_TABLES = {kind: tuple(_adjoint(tab) for tab in IR.TABLES[kind]) for kind in IR.TABLES}


def left_sigma_terms(kind, no, f, Vd, t2, l1, l2):
    """H^T l term by term: each row of ``_ipea_reference.TABLES`` with the trial vector's slot and the output exchanged."""
    env = dict(Vd)
    env.update(foo=f[:no, :no], fov=f[:no, no:], fvv=f[no:, no:], t=t2)
    o1, o2 = np.zeros_like(l1), np.zeros_like(l2)
    for tab, left in zip(LEFT_TABLES[kind], (l1, l2)):
        for c, spec, names, k in tab:
            ops = [left if i == k else env[nm] for i, nm in enumerate(names)]
            out = c * np.einsum(spec, *ops, optimize=True)
            if names[k] == "r1":
                o1 += out
            else:
                o2 += out
    return o1, o2


# ---- the dense eigenproblem ---------------------------------------------------------------------------------------------------------
def dense_ipea(kind, no, fd, Vd, t2, nroots=None):
    """(w, rs, ls, largest imaginary part): the ``nroots`` lowest roots (all: None) of scipy.linalg.eig(H, left=True), right
    vectors of unit norm, left vectors biorthonormalised by the inverse Gram matrix; vectors as pairs."""
    nv = fd.shape[0] - no
    H = IR.dense(kind, no, fd, Vd, t2)
    w, vl, vr = scipy.linalg.eig(H, left=True)
    pick = np.argsort(w.real, kind="stable")[:nroots]
    imag = float(np.abs(w[pick].imag).max())
    R = vr[:, pick].real
    R = R / np.linalg.norm(R, axis=0)[None, :]
    L = vl[:, pick].real
    if imag == 0.0:
        L = L @ np.linalg.inv(L.T @ R).T                    # l_j <- sum_m (G^-1)_jm l_m, G_jk = <l_j, r_k>
    sp = lambda M: [split(kind, no, nv, M[:, z]) for z in range(M.shape[1])]
    return w[pick].real.copy(), sp(R), sp(L), imag


@functools.lru_cache(maxsize=None)
def reference_case(kind, no, nv, seed, eight=True, nroots=None, scale=0.02):
    """Everything of one test problem, dense: f, V, the converged state, lambda, w, rs, ls, psiL, psiR."""
    f, V = LR.random_problem(no, nv, seed, eight=eight, scale=scale)
    t1, t2, fd, Vd, _ = LR.converged_state(no, f, V)
    t2 = 0.5 * LR.symd(t2)
    Vd = {k: (v if v is not None else cc.split_blocks(no, V)[k]) for k, v in Vd.items()}
    lam = LR.solve_lambda(no, fd, Vd, t2)
    w, rs, ls, imag = dense_ipea(kind, no, fd, Vd, t2, nroots)
    amps = [dyson_terms(kind, no, t1, t2, lam[0], lam[1], l, r) for l, r in zip(ls, rs)]
    return dict(f=f, V=V, t1=t1, t2=t2, fd=fd, Vd=Vd, lam=lam, w=w, rs=rs, ls=ls, imag=imag,
                psiL=np.stack([a[0] for a in amps]), psiR=np.stack([a[1] for a in amps]))


# ---- exact two-electron calculation -------------------------------------------------------------------------------------------------
def two_electron_dyson(f, V):
    """For no = 1: (IP roots eps_k(h) - E0 ascending [n], d [n,n]) with d[k] = C0 phi_k, C0 the normalised symmetric coefficient
    matrix of the singlet FCI ground state and (eps_k, phi_k) the one-electron states of h = f - (2 V_p0q0 - V_p00q); the exact
    residue matrix of root k is d[k] d[k]^T (per spin; their sum is C0 C0^T, of trace 1)."""
    n = f.shape[0]
    h = f - (2.0 * V[:, 0, :, 0] - V[:, 0, 0, :])
    basis = []
    for p in range(n):
        for q in range(p, n):
            c = np.zeros((n, n))
            c[p, q] = c[q, p] = 1.0
            basis.append(c / np.linalg.norm(c))
    op = lambda m, c: m @ c + c @ m.T
    Hm = np.array([[(b * (op(h, c) + np.einsum("pqrs,rs->pq", V, c))).sum() for c in basis] for b in basis])
    assert np.abs(Hm - Hm.T).max() < 1e-12 and np.abs(h - h.T).max() < 1e-12
    e, xs = np.linalg.eigh(0.5 * (Hm + Hm.T))
    C0 = sum(xs[m, 0] * basis[m] for m in range(len(basis)))
    eps, phi = np.linalg.eigh(h)
    order = np.argsort(eps - e[0], kind="stable")
    return (eps - e[0])[order], np.stack([C0 @ phi[:, k] for k in order])


# ---- D2 by the definition at the larger shapes of the GPU test: seconds each, so the results are recorded
# (python -m tests._dyson_reference rewrites tests/golden/dyson_definition.npz) ---------------------------------------------------------
def definition_inputs(kind, no, nv, k=3):
    """Random (t1, t2, lambda, ls, rs): exchange-symmetric T2 and Lambda2, compact vectors; they need not solve anything."""
    t1, t2, l1, l2 = LR.density_inputs(no, nv, 9)
    rng = np.random.default_rng(21 + (kind == "ea"))
    s1, s2 = IR.shapes(kind, no, nv)
    vec = lambda: (rng.standard_normal(s1), rng.standard_normal(s2))
    return t1, t2, (l1, l2), [vec() for _ in range(k)], [vec() for _ in range(k)]


GOLDEN_DYSON = ("dyson_definition.npz", ((5, 19), (20, 10)))          # file, shapes (both kinds)


if __name__ == "__main__":
    import os
    name, shapes = GOLDEN_DYSON
    out = {}
    for kind in ("ip", "ea"):
        for no, nv in shapes:
            pl, pr = dyson_definition(kind, no, *definition_inputs(kind, no, nv))
            out["%s_%d_%d_left" % (kind, no, nv)], out["%s_%d_%d_right" % (kind, no, nv)] = pl, pr
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), **out)
