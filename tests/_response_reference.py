"""numpy reference of the EOM-CCSD linear response function.  TEST INFRASTRUCTURE ONLY.

Built on ``_lambda_reference`` (dense sigma in symmetric coordinates) and ``_transition_reference`` (transition densities, the
two-electron FCI): the property vectors xi(O), eta(O) by their definitions and written out (include/pymes_amd.h,
pymes_response_vectors), the dense resolvent, the sum over all states of the dense eigenproblem, and the exact two-electron value.

  xi(O) = (R1(O), R2(O)): the CCSD residuals at (t1, t2) with f = O and V = 0
  <eta(O), r> = sum gammaR(r) O for every symmetric r (gammaR of _transition_reference, linear in r and in f)
  x^O(z) = (z - A)^-1 xi(O),   <<X;Y>>_z = <eta(X), x^Y(z)> + <eta(Y), x^X(-z)>

and the two passes of the linear solver's sweep over flat vectors by their contract in include/pymes_amd.h (``sweep_dots_reference``,
``sweep_update_reference``: complex128, exactly rounded sums, with the magnitude of every expression for a forward error bound) and
the solver's loop written with nothing but those two (``orthomin_reference``).
"""
import functools
import math

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


# ---- the solver's sweep: dots and the fused update over flat vectors (include/pymes_amd.h, pymes_response_dots / _update) --------------
HIST = 32                   # PYMES_RESPONSE_HIST
DOTS = 2 * (HIST + 2)       # PYMES_RESPONSE_DOTS


class SweepSystem:
    """One system of a sweep on the host: flat vectors x, r, p, ap (real or complex; p, ap None: no step), the stored directions
    hp, hq (lists), the coefficients g, alpha, the shift z and the scale inv."""

    def __init__(self, x=None, r=None, p=None, ap=None, hp=(), hq=(), g=(), alpha=0.0, z=0.0, inv=1.0):
        self.x, self.r, self.p, self.ap = x, r, p, ap
        self.hp, self.hq, self.g = list(hp), list(hq), list(g)
        self.alpha, self.z, self.inv = complex(alpha), complex(z), float(inv)

    @property
    def nh(self):
        return len(self.hq)


def active_mask(length, n1, off2):
    e = np.arange(length)
    return (e < n1) | (e >= off2)


def _c(v):
    return np.asarray(v).astype(np.complex128)


def mag(v):
    """|Re| + |Im|, element by element (of a number: the same)."""
    v = np.asarray(v)
    return np.abs(v.real) + np.abs(v.imag)


def fsum(*terms):
    return math.fsum(np.concatenate([np.ravel(t) for t in terms]).tolist())


def _inner(u, v):
    """(Re, Im) of sum conj(u) v, every real product a term of its own in an exactly rounded sum."""
    return fsum(u.real * v.real, u.imag * v.imag), fsum(u.real * v.imag, -(u.imag * v.real))


def sweep_dots_reference(system, n1, off2):
    """(row, magnitudes) [PYMES_RESPONSE_DOTS] each: <hq_j, q> for j < nh, <q, q> (its second double 0), <q, r> with
    q = z p - ap, summed over the active elements; magnitudes: the same sums with every product replaced by the product of the
    factors' |Re| + |Im|, mag(q) = mag(z) mag(p) + mag(ap)."""
    S = system
    act = active_mask(len(S.p), n1, off2)
    p, ap, r = _c(S.p)[act], _c(S.ap)[act], _c(S.r)[act]
    q, mq = S.z * p - ap, mag(S.z) * mag(p) + mag(ap)
    row, mags = np.zeros(DOTS), np.zeros(DOTS)
    for j in range(S.nh):
        hq = _c(S.hq[j])[act]
        row[2 * j], row[2 * j + 1] = _inner(hq, q)
        mags[2 * j] = mags[2 * j + 1] = fsum(mag(hq) * mq)
    nh = S.nh
    row[2 * nh] = fsum(q.real * q.real, q.imag * q.imag)
    mags[2 * nh] = fsum(mq * mq)
    row[2 * nh + 2], row[2 * nh + 3] = _inner(q, r)
    mags[2 * nh + 2] = mags[2 * nh + 3] = fsum(mq * mag(r))
    return row, mags


def sweep_update_reference(system, d, floor, n1, off2):
    """(new, magnitudes, |r|^2, its magnitude sum, floored): ``new`` and ``magnitudes`` are dictionaries of the flat complex
    vectors x, r, p, ap, pn after the update (p, ap None without a step; the pad of pn zero, of the others as given) and of the
    element-wise magnitudes of their expressions (absolute values, every subtraction an addition); ``floored``: the elements
    whose |z - d| was below the floor."""
    S = system
    length = len(S.r)
    act = active_mask(length, n1, off2)
    x, r = _c(S.x).copy(), _c(S.r).copy()
    mx, mr = mag(x), mag(r)
    new, mags = dict(p=None, ap=None), dict(p=None, ap=None)
    if S.p is not None:
        p, ap = _c(S.p).copy(), _c(S.ap).copy()
        q, mq = S.z * p - ap, mag(S.z) * mag(p) + mag(ap)
        mp = mag(p)
        for j in range(S.nh):
            p = p - S.g[j] * _c(S.hp[j])
            q = q - S.g[j] * _c(S.hq[j])
            mp = mp + mag(S.g[j]) * mag(S.hp[j])
            mq = mq + mag(S.g[j]) * mag(S.hq[j])
        p, q, mp, mq = p * S.inv, q * S.inv, mp * abs(S.inv), mq * abs(S.inv)
        x[act] = (x + S.alpha * p)[act]
        r[act] = (r - S.alpha * q)[act]
        mx, mr = mx + mag(S.alpha) * mp, mr + mag(S.alpha) * mq
        new["p"], new["ap"], mags["p"], mags["ap"] = p, q, mp, mq
    w = S.z - np.asarray(d, dtype=np.float64)[act]
    re, im = w.real.copy(), w.imag
    low = np.abs(w) < floor
    re[low] = np.copysign(floor, re[low])
    den = re * re + im * im
    pn, mpn = np.zeros(length, dtype=np.complex128), np.zeros(length)
    pn[act] = r[act] * (re - 1j * im) / den
    mpn[act] = mr[act] * (np.abs(re) + np.abs(im)) / den
    new.update(x=x, r=r, pn=pn)
    mags.update(x=mx, r=mr, pn=mpn)
    ra = r[act]
    floored = np.zeros(length, dtype=bool)
    floored[act] = low
    return new, mags, fsum(ra.real * ra.real, ra.imag * ra.imag), fsum(mr[act] * mr[act]), floored


def orthomin_reference(A, d, xi, z, history, floor, r_epsilon, max_iter):
    """The loop of ``EOM_CCSD_Response._sweep`` for one system (z - A) x = xi with a dense A and the two references above (no
    pad): (x, sweeps, |xi - (z - A) x| / |xi| measured afresh).  A break-down or max_iter sweeps end the loop as they are: the
    residual returned tells."""
    n = len(xi)
    S = SweepSystem(x=np.zeros(n, dtype=np.complex128), r=_c(xi), z=z)
    new, _, nrm, _, _ = sweep_update_reference(S, d, floor, n, n)                   # p_0 = r_0 / (z - d), |xi|^2
    norm0, pn = np.sqrt(nrm), new["pn"]
    sweeps = 0
    while sweeps < max_iter and norm0 > 0.0:
        S.p = pn
        S.ap = A @ S.p
        row, _ = sweep_dots_reference(S, n, n)
        nh = S.nh
        g = row[0:2 * nh:2] + 1j * row[1:2 * nh:2]
        qq, qr = row[2 * nh], complex(row[2 * nh + 2], row[2 * nh + 3])
        left = qq - float((np.abs(g) ** 2).sum())
        if not np.isfinite(left) or left <= 1e-12 * max(qq, 1e-300):
            break
        S.g, S.inv = list(g), 1.0 / np.sqrt(left)
        S.alpha = qr * S.inv
        new, _, nrm, _, _ = sweep_update_reference(S, d, floor, n, n)
        S.x, S.r, pn = new["x"], new["r"], new["pn"]
        S.hp.append(new["p"])
        S.hq.append(new["ap"])
        if len(S.hp) > history:
            S.hp.pop(0)
            S.hq.pop(0)
        S.p = S.ap = None
        sweeps += 1
        if not np.isfinite(nrm) or np.sqrt(nrm) <= r_epsilon * norm0:
            break
    res = _c(xi) - (z * S.x - A @ S.x)
    return S.x, sweeps, float(np.linalg.norm(res) / norm0) if norm0 > 0.0 else 0.0
