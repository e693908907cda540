"""numpy reference of the EOM-CCSD linear response function.  TEST INFRASTRUCTURE ONLY.

Built on ``_lambda_reference`` (dense sigma in symmetric coordinates) and ``_transition_reference`` (transition densities, the
two-electron FCI): the property vectors xi(O), eta(O) by their definitions and written out (include/pymes_amd.h,
pymes_response_vectors), the dense resolvent, the sum over all states of the dense eigenproblem, and the exact two-electron value.

  xi(O) = (R1(O), R2(O)): the CCSD residuals at (t1, t2) with f = O and V = 0
  <eta(O), r> = sum gammaR(r) O for every symmetric r (gammaR of _transition_reference, linear in r and in f)
  x^O(z) = (z - A)^-1 xi(O),   <<X;Y>>_z = <eta(X), x^Y(z)> + <eta(Y), x^X(-z)>
"""
import functools

import numpy as np
import scipy.linalg

from oracle import cc_oracle as cc
from oracle import eom_oracle as eo
from tests import _lambda_reference as R
from tests import _transition_reference as T

dot = T.dot


# ---- the definitions ---------------------------------------------------------------------------------------------------------------
def _zero_blocks(no, nv, t1):
    n = no + nv
    Vb = cc.split_blocks(no, np.zeros((n, n, n, n)))
    return Vb, cc.dressed_V(t1, Vb)


def xi_definition(no, t1, t2, O):
    """(R1(O), R2(O)) from the oracle's residuals with f = O and all integrals zero."""
    Vb, Vd = _zero_blocks(no, t1.shape[0], t1)
    fd = cc.dressed_fock(no, O, t1, Vb)
    ein = functools.partial(np.einsum, optimize=True)
    return cc.singles_residual(no, fd, t1, t2, Vb), cc.ccsd_doubles_residual(no, fd, t2, Vd, ein=ein)


def eta_definition(no, t1, t2, lam, O):
    """The symmetric vector with <eta, r> = sum gammaR(r) O: gammaR's defining expression (``transition_densities_definition``)
    evaluated at f = O for every symmetric coordinate vector r."""
    nv = t1.shape[0]
    Vb, Vd = _zero_blocks(no, nv, t1)
    fd = cc.dressed_fock(no, O, t1, Vb)
    r1, r2 = xi_definition(no, t1, t2, O)
    lag = dot(lam, (r1, r2))
    co = R.SymmetricCoordinates(no, nv)
    val = np.zeros(co.dim)
    for k in range(co.dim):
        x = np.zeros(co.dim)
        x[k] = 1.0
        u1, u2 = co.unpack(x)
        s = (eo.sigma_singles(no, fd, Vd, u1, u2, t2), eo.sigma_doubles(no, fd, Vd, u1, u2, t2))
        val[k] = (2.0 * (fd[:no, no:] * u1.T).sum() + dot(lam, s) + 2.0 * np.einsum("abij,ai,bj->", lam[1], u1, r1)
                  - dot(lam, (u1, u2)) * lag)
    return co.split(co.B @ np.linalg.solve(co.B.T @ co.B, val))


# ---- the same written out ------------------------------------------------------------------------------------------------------------
def dress_operator(no, O, t1):
    """(O~_oo [j,i], O~_ov [j,b], O~_vo [a,i], O~_vv [a,b]): ``_undress`` of _transition_reference read backwards."""
    oo, ov, vo, vv = O[:no, :no], O[:no, no:], O[no:, :no], O[no:, no:]
    doo = oo + ov @ t1
    return doo, ov.copy(), vo + vv @ t1 - t1 @ doo, vv - t1 @ ov


def xi_terms(no, t1, t2, O):
    oo, ov, vo, vv = dress_operator(no, O, t1)
    x1 = vo + np.einsum("abij,jb->ai", 2.0 * t2 - t2.transpose(0, 1, 3, 2), ov)
    S = np.einsum("ac,cbij->abij", vv, t2) - np.einsum("ki,abkj->abij", oo, t2)
    return x1, R.symd(S)


def eta_terms(no, t1, t2, lam, O):
    l1, l2 = lam
    oo, ov, vo, vv = dress_operator(no, O, t1)
    x1, x2 = xi_terms(no, t1, t2, O)
    g0 = dot(lam, (x1, x2))
    yoo = np.einsum("abij,abkj->ki", l2, t2)
    yvv = np.einsum("abij,cbij->ac", l2, t2)
    e1 = (2.0 * ov.T + 2.0 * np.einsum("caki,ai->ck", l2, x1) - np.einsum("ci,ki->ck", l1, oo) + np.einsum("ac,ak->ck", vv, l1)
          - 2.0 * np.einsum("jk,jc->ck", yoo, ov) - 2.0 * np.einsum("cb,kb->ck", yvv, ov) - g0 * l1)
    E = (-2.0 * np.einsum("abkj,ik->abij", l2, oo) + 2.0 * np.einsum("ca,cbij->abij", vv, l2) + 2.0 * np.einsum("ai,jb->abij", l1, ov)
         - np.einsum("aj,ib->abij", l1, ov))
    return e1, 0.5 * R.symd(E) - g0 * l2


# ---- the response function, dense --------------------------------------------------------------------------------------------------
class DenseResponse:
    """Everything of one problem in symmetric coordinates: the pencil (B^T A B, G = B^T B) and the property vectors of the
    operators (written-out formulas)."""

    def __init__(self, no, t1, t2, fd, Vd, lam, operators):
        self.no, self.t1, self.t2, self.lam, self.ops = no, t1, t2, lam, [np.asarray(O) for O in operators]
        self.co, self.BA, _ = R.dense_operators(no, fd, Vd, t2)
        self.G = self.co.B.T @ self.co.B
        self.xi = [xi_terms(no, t1, t2, O) for O in self.ops]
        self.eta = [eta_terms(no, t1, t2, lam, O) for O in self.ops]

    def coords(self, vec):
        return self.co.B.T @ self.co.full(*vec)

    def solve(self, z, vec):
        """x = B (z G - B^T A B)^-1 B^T vec as a (singles, doubles) pair (complex for a complex z)."""
        y = np.linalg.solve(z * self.G - self.BA, self.coords(vec).astype(type(z * 1.0)))
        return self.co.split(self.co.B @ y)

    def response(self, z):
        """<<X;Y>>_z [m,m] from the dense resolvent."""
        m = len(self.ops)
        xp = [self.solve(z, v) for v in self.xi]
        xm = [self.solve(-z, v) for v in self.xi]
        cd = lambda a, b: (a[0] * b[0]).sum() + (a[1] * b[1]).sum()
        return np.array([[cd(self.eta[X], xp[Y]) + cd(self.eta[Y], xm[X]) for Y in range(m)] for X in range(m)])

    def states(self):
        """(w [dim], <0|O|k> [m,dim], <k|O|0> [m,dim]) of ALL states of the dense eigenproblem, the moments from the transition
        densities of ``_transition_reference`` (written out independently of xi and eta), and the largest imaginary part met.
        Complex-conjugate pairs are kept as they are: the densities are linear in the vectors, so they are taken of the real
        and the imaginary parts, and the sum over states stays exact (no conjugation anywhere: the products are bilinear)."""
        w, vr = scipy.linalg.eig(self.BA, self.G)
        imag = float(max(np.abs(w.imag).max(), np.abs(vr.imag).max()))
        # the left vectors biorthonormal to ALL right ones: the rows y_k of (G Vr)^-1 have y_k^T B^T A B = w_k y_k^T G, and the
        # left vector is B y_k itself (degenerate roots need no care: any basis of their space serves the sum)
        yl = np.linalg.inv(self.G @ vr)
        dim = len(w)
        right, left = np.zeros((len(self.ops), dim), dtype=complex), np.zeros((len(self.ops), dim), dtype=complex)
        for part, unit in ((np.real, 1.0), (np.imag, 1.0j)):
            rs = [self.co.split(self.co.B @ part(vr[:, k])) for k in range(dim)]
            ls = [self.co.split(self.co.B @ part(yl[k])) for k in range(dim)]
            gl, gr = T.transition_density_terms(self.no, self.t1, self.t2, self.lam, ls, rs)
            right += unit * np.array([[(gr[k] * O).sum() for k in range(dim)] for O in self.ops])
            left += unit * np.array([[(gl[k] * O).sum() for k in range(dim)] for O in self.ops])
        return w, right, left, imag

    def sum_over_states(self, z, states=None):
        w, right, left, _ = states or self.states()
        return (np.einsum("xk,yk,k->xy", right, left, 1.0 / (z - w)) - np.einsum("yk,xk,k->xy", right, left, 1.0 / (z + w)))

    def resolvent_norm(self, z):
        """|(z - A)^-1|_2 on the symmetric subspace, from the dense matrix in an orthonormalised symmetric basis."""
        Q, _ = np.linalg.qr(self.co.B)
        A = Q.T @ (self.co.B @ np.linalg.solve(self.G, self.BA) @ np.linalg.solve(self.G, self.co.B.T @ Q))
        return float(np.linalg.norm(np.linalg.inv(z * np.eye(A.shape[0]) - A), 2))


def norm(vec):
    return float(np.sqrt(dot(vec, vec)))


@functools.lru_cache(maxsize=None)
def reference_problem(no, nv, seed, hermitian=True, nops=2, scale=0.02, symmetric_ops=False):
    """A converged 8-fold (or mildly non-hermitian) problem with Lambda, ``nops`` seeded operators (non-symmetric unless
    ``symmetric_ops``) and its ``DenseResponse``; w1: the lowest excitation energy."""
    f, V = T.problem(no, nv, seed, hermitian, scale)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V)
    t2 = 0.5 * R.symd(t2)
    lam = R.solve_lambda(no, fd, Vd, t2)
    rng = np.random.default_rng(seed + 77)
    ops = rng.standard_normal((nops, no + nv, no + nv))
    if symmetric_ops:
        ops = 0.5 * (ops + ops.transpose(0, 2, 1))
    dense = DenseResponse(no, t1, t2, fd, Vd, lam, ops)
    w = scipy.linalg.eigvals(dense.BA, dense.G)
    return dict(f=f, V=V, t1=t1, t2=t2, fd=fd, Vd=Vd, lam=lam, ops=ops, dense=dense, w1=float(np.sort(w.real)[0]))


def frequencies(w1):
    """The three test frequencies of the issue: 0, 0.4 w1 and 1.3 w1 + 0.05i."""
    return [0.0, 0.4 * w1, 1.3 * w1 + 0.05j]


def two_electron_polarizability(f, V, O, z):
    """-<<O;O>>_z of the exact singlet states of two electrons (``two_electron_fci``)."""
    gaps, mom = T.two_electron_fci(f, V, O)
    return -(mom * (1.0 / (z - gaps) - 1.0 / (z + gaps))).sum()
