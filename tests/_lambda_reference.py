"""numpy reference of the CCSD Lambda equations and the one-particle response density.  TEST INFRASTRUCTURE ONLY.

Everything is derived from the two oracles: the left sigma is the adjoint of ``oracle/eom_oracle.py``'s term tables (each row is
linear in exactly one of u1 / u2, so its adjoint swaps that operand with the output), Lambda is a dense solve on the
exchange-symmetric subspace, and the density is the derivative of the Lagrangian with ``oracle/cc_oracle.py``'s residuals.

Conventions: vectors are pairs (x1 [v,o], x2 [v,v,o,o]) with x2_abij = x2_baji; the inner product is the plain sum over all
elements of both arrays.
"""
import functools

import numpy as np

from oracle import cc_oracle as cc
from oracle import eom_oracle as eo


def symd(x):
    return x + x.transpose(1, 0, 3, 2)


def _adjoint(terms):
    """(coefficient, subscripts with the trial vector's slot and the output swapped, operand names, slot of the left vector,
    "u1" / "u2": which part of the result the row adds to)."""
    out = []
    for c, spec, names in terms:
        ins, res = spec.split("->")
        ins = ins.split(",")
        k = [i for i, nm in enumerate(names) if nm in ("u1", "u2")]
        assert len(k) == 1, "every row is linear in exactly one of u1 / u2"
        k = k[0]
        target = ins[k]
        ins[k] = res
        out.append((c, ",".join(ins) + "->" + target, names, k, names[k]))
    return tuple(out)


LEFT_SINGLES_TERMS = _adjoint(eo.SINGLES_TERMS)         # left vector: l1
LEFT_DOUBLES_TERMS_P = _adjoint(eo.DOUBLES_TERMS_P)     # left vector: l2 + l2^T(1,0,3,2)
LEFT_DOUBLES_TERMS_N = _adjoint(eo.DOUBLES_TERMS_N)     # left vector: l2


def left_sigma(no, f, Vd, l1, l2, t2):
    """(A^T l)_1 [v,o], (A^T l)_2 [v,v,o,o] for the EE sigma A of eom_oracle (update_singles / update_doubles)."""
    env = eo._env(no, f, Vd, t2, None, None)
    o1, o2 = np.zeros_like(l1), np.zeros_like(l2)
    for terms, left in ((LEFT_SINGLES_TERMS, l1), (LEFT_DOUBLES_TERMS_P, symd(l2)), (LEFT_DOUBLES_TERMS_N, l2)):
        for c, spec, names, k, target in terms:
            ops = [left if i == k else env[nm] for i, nm in enumerate(names)]
            r = c * np.einsum(spec, *ops, optimize=True)
            if target == "u1":
                o1 += r
            else:
                o2 += r
    return o1, 0.5 * symd(o2)


def eta(no, f, Vd):
    """eta1[a,i] = 2 f_ov[i,a], eta2[a,b,i,j] = 2 V_ijab[i,j,a,b] - V_ijab[i,j,b,a]."""
    Vijab = Vd["ijab"]
    return 2.0 * f[:no, no:].T.copy(), 2.0 * Vijab.transpose(2, 3, 0, 1) - Vijab.transpose(3, 2, 0, 1)


class SymmetricCoordinates:
    """Independent coordinates of the exchange-symmetric vectors: the singles and the pairs (ai) <= (bj) of the doubles."""

    def __init__(self, no, nv):
        self.no, self.nv, self.n1 = no, nv, no * nv
        n1 = self.n1
        self.pairs = [(p, q) for p in range(n1) for q in range(p, n1)]
        self.dim = n1 + len(self.pairs)
        self.B = np.zeros((n1 + n1 * n1, self.dim))           # coordinates -> full arrays
        for k in range(self.dim):
            x = np.zeros(self.dim)
            x[k] = 1.0
            self.B[:, k] = self.full(*self.unpack(x))

    def unpack(self, x):
        n1, no, nv = self.n1, self.no, self.nv
        M = np.zeros((n1, n1))
        for k, (p, q) in enumerate(self.pairs):
            M[p, q] = M[q, p] = x[n1 + k]
        return x[:n1].reshape(nv, no).copy(), M.reshape(nv, no, nv, no).transpose(0, 2, 1, 3).copy()

    def full(self, s1, s2):
        return np.concatenate([s1.ravel(), s2.transpose(0, 2, 1, 3).reshape(self.n1 * self.n1)])

    def split(self, y):
        n1, no, nv = self.n1, self.no, self.nv
        return y[:n1].reshape(nv, no).copy(), y[n1:].reshape(nv, no, nv, no).transpose(0, 2, 1, 3).copy()


def dense_operators(no, f, Vd, t2):
    """(coordinates, B^T A B, B^T A^T B): the right and the left sigma as matrices between symmetric coordinates and the
    plain inner product with symmetric vectors, column by column (tiny sizes only)."""
    nv = f.shape[0] - no
    co = SymmetricCoordinates(no, nv)
    AF, LF = np.zeros((co.B.shape[0], co.dim)), np.zeros((co.B.shape[0], co.dim))
    for k in range(co.dim):
        x = np.zeros(co.dim)
        x[k] = 1.0
        u1, u2 = co.unpack(x)
        AF[:, k] = co.full(eo.sigma_singles(no, f, Vd, u1, u2, t2), eo.sigma_doubles(no, f, Vd, u1, u2, t2))
        LF[:, k] = co.full(*left_sigma(no, f, Vd, u1, u2, t2))
    return co, co.B.T @ AF, co.B.T @ LF


def solve_lambda(no, f, Vd, t2):
    """(lambda1, lambda2) with A^T lambda + eta = 0 on the symmetric subspace: <lambda, A u> + <eta, u> = 0 for all symmetric u."""
    co, BA, _ = dense_operators(no, f, Vd, t2)
    e1, e2 = eta(no, f, Vd)
    y = np.linalg.solve(BA.T, -(co.B.T @ co.full(e1, e2)))
    return co.split(co.B @ y)


def lagrangian_density(no, t1, t2, l1, l2):
    """gamma_pq = dL/df_pq of L(f) = E(f) + <l1, R1(f)> + <l2, R2(f)>, by evaluating L with the unit matrix e_pq as Fock
    matrix and V = 0 (L is linear in f)."""
    nv = t1.shape[0]
    n = no + nv
    Vb = cc.split_blocks(no, np.zeros((n, n, n, n)))
    Vd = cc.dressed_V(t1, Vb)                  # (zero; it does not depend on the Fock matrix)
    ein = functools.partial(np.einsum, optimize=True)
    g = np.zeros((n, n))
    for p in range(n):
        for q in range(n):
            e = np.zeros((n, n))
            e[p, q] = 1.0
            fd = cc.dressed_fock(no, e, t1, Vb)
            r1 = cc.singles_residual(no, fd, t1, t2, Vb)
            r2 = cc.ccsd_doubles_residual(no, fd, t2, Vd, ein=ein)
            g[p, q] = sum(cc.ccsd_energy(e[:no, no:], t1, t2, Vb["ijab"])) + (l1 * r1).sum() + (l2 * r2).sum()
    return g


def density_terms(no, t1, t2, l1, l2):
    """The same gamma written out (the contractions the device kernel assembles); pinned against lagrangian_density."""
    nv = t1.shape[0]
    n = no + nv
    gvv = 2.0 * np.einsum("abij,cbij->ac", l2, t2)                       # coefficient of the dressed f_vv[a,c]
    goo = -2.0 * np.einsum("abij,abkj->ki", l2, t2)                      # ... of the dressed f_oo[k,i]
    gov = np.einsum("ai,abij->jb", l1, 2.0 * t2 - t2.transpose(0, 1, 3, 2))
    g = np.zeros((n, n))
    g[no:, :no] = l1
    g[:no, :no] = goo - t1.T @ l1
    g[no:, no:] = gvv + l1 @ t1.T
    g[:no, no:] = gov + 2.0 * t1.T - t1.T @ l1 @ t1.T + goo @ t1.T - t1.T @ gvv
    return g


def rdm1(no, t1, t2, l1, l2):
    """The response density plus 2 on the occupied diagonal: its trace is the electron count."""
    g = lagrangian_density(no, t1, t2, l1, l2)
    g[np.arange(no), np.arange(no)] += 2.0
    return g


# ---- shared set-ups of the tests -----------------------------------------------------------------------------------------------
def sym8(V):
    V = V + V.transpose(1, 0, 3, 2)
    V = V + V.transpose(2, 3, 0, 1)
    V = V + V.transpose(2, 1, 0, 3)
    return V + V.transpose(0, 3, 2, 1)


def random_problem(no, nv, seed, eight=True, scale=0.02, gap=3.0):
    """(f, V): random integrals of the given scale (8-fold symmetric, or with V_pqrs = V_qpsr only) and a Fock matrix with
    the given gap between the occupied and the virtual diagonal."""
    rng = np.random.default_rng(seed)
    n = no + nv
    V = rng.standard_normal((n, n, n, n)) * scale
    V = sym8(V) if eight else V + V.transpose(1, 0, 3, 2)
    f = np.diag(np.concatenate([-gap + 1.0 - rng.random(no), 1.0 + rng.random(nv)])) + 0.05 * rng.standard_normal((n, n))
    if eight:
        f = 0.5 * (f + f.T)
    return f, V


def converged_state(no, f, V, delta_e=1e-15):
    """(t1, t2, dressed Fock, dressed blocks) of the oracle's CCSD solution."""
    r = cc.ccsd_solve(no, f, V, delta_e=delta_e, max_iter=300)
    Vb = cc.split_blocks(no, V)
    return r["t1"], r["t2"], cc.dressed_fock(no, f, r["t1"], Vb), cc.dressed_V(r["t1"], Vb), r["e"]


# ---- the density by definition at (6,17): n^2 = 529 evaluations of the Lagrangian take ten seconds, so the result is recorded
# (python -m tests._lambda_reference rewrites tests/golden/lambda_rdm1_6_17.npz) ------------------------------------------------------
def density_inputs(no, nv, seed):
    """Random (t1, t2, l1, l2) with exchange-symmetric doubles; they need not solve anything: the density is a formula."""
    rng = np.random.default_rng(seed)
    t1, l1 = 0.1 * rng.standard_normal((nv, no)), 0.1 * rng.standard_normal((nv, no))
    t2, l2 = symd(0.05 * rng.standard_normal((nv, nv, no, no))), symd(0.05 * rng.standard_normal((nv, nv, no, no)))
    return t1, t2, l1, l2


GOLDEN_RDM1 = ("lambda_rdm1_6_17.npz", 6, 17, 7)          # file, no, nv, seed


if __name__ == "__main__":
    import os
    name, no, nv, seed = GOLDEN_RDM1
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), rdm1=rdm1(no, *density_inputs(no, nv, seed)))
