"""CPU: the numpy reference of the CCSD Lambda equations and of the one-particle response density (tests/_lambda_reference.py)
against the two oracles it is derived from: the adjoint identity, the spectrum, and the derivative of the CCSD energy with
respect to the Fock matrix by finite differences of the oracle's own solver."""
import functools

import numpy as np
import pytest

from oracle import cc_oracle as cc
from oracle import eom_oracle as eo
from tests import _lambda_reference as R


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5)])
def test_adjoint_identity(no, nv):
    """<l, A u> = <A^T l, u> for symmetric u, l and integrals / amplitudes without the (pq <-> rs) symmetry."""
    rng = np.random.default_rng(5)
    n = no + nv
    V = rng.standard_normal((n, n, n, n))
    V = V + V.transpose(1, 0, 3, 2)
    f = rng.standard_normal((n, n))
    Vb = cc.split_blocks(no, V)
    t2 = R.symd(rng.standard_normal((nv, nv, no, no)))
    u1, u2 = rng.standard_normal((nv, no)), R.symd(rng.standard_normal((nv, nv, no, no)))
    l1, l2 = rng.standard_normal((nv, no)), R.symd(rng.standard_normal((nv, nv, no, no)))
    s1, s2 = eo.sigma_singles(no, f, Vb, u1, u2, t2), eo.sigma_doubles(no, f, Vb, u1, u2, t2)
    o1, o2 = R.left_sigma(no, f, Vb, l1, l2, t2)
    a, b = (l1 * s1).sum() + (l2 * s2).sum(), (o1 * u1).sum() + (o2 * u2).sum()
    print("adjoint identity (%d,%d): %.16e %.16e relative %.2e" % (no, nv, a, b, abs(a - b) / abs(a)))
    assert abs(a - b) <= 1e-12 * abs(a)
    assert np.array_equal(o2, o2.transpose(1, 0, 3, 2))


def test_left_and_right_spectra_agree():
    no, nv = 2, 3
    f, V = R.random_problem(no, nv, seed=3, eight=False)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    co, BA, BL = R.dense_operators(no, fd, Vd, t2)
    G = co.B.T @ co.B
    wr = np.sort_complex(np.linalg.eigvals(np.linalg.solve(G, BA)))
    wl = np.sort_complex(np.linalg.eigvals(np.linalg.solve(G, BL)))
    print("largest spectral difference %.2e" % np.abs(wr - wl).max())
    assert np.abs(wr - wl).max() < 1e-9


@functools.lru_cache(maxsize=None)
def _density_case(no, nv):
    """8-fold-symmetric integrals, symmetric O: (gamma by the Lagrangian, gamma written out, O, finite difference)."""
    f, V = R.random_problem(no, nv, seed=3, eight=True)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V)
    l1, l2 = R.solve_lambda(no, fd, Vd, t2)
    g = R.lagrangian_density(no, t1, t2, l1, l2)
    O = np.random.default_rng(11).standard_normal(f.shape)
    O = 0.5 * (O + O.T)
    h = 1e-4
    ep = cc.ccsd_solve(no, f + h * O, V, delta_e=1e-15, max_iter=300)["e"]
    em = cc.ccsd_solve(no, f - h * O, V, delta_e=1e-15, max_iter=300)["e"]
    return g, R.density_terms(no, t1, t2, l1, l2), O, (ep - em) / (2.0 * h), (f, V, t1, t2, fd, Vd, l1, l2)


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4)])
def test_density_is_the_energy_derivative(no, nv):
    g, _, O, fd, _ = _density_case(no, nv)
    val = (g * O).sum()
    print("(%d,%d) finite difference %.12e  sum gamma O %.12e  difference %.2e" % (no, nv, fd, val, abs(fd - val)))
    assert abs(fd - val) < 1e-6


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4)])
def test_lambda_solves_its_equation_and_traces(no, nv):
    g, gt, _, _, (f, V, t1, t2, fd, Vd, l1, l2) = _density_case(no, nv)
    o1, o2 = R.left_sigma(no, fd, Vd, l1, l2, t2)
    e1, e2 = R.eta(no, fd, Vd)
    assert max(np.abs(o1 + e1).max(), np.abs(o2 + e2).max()) < 1e-12
    assert abs(np.trace(g)) < 1e-12
    assert np.abs(g - gt).max() < 1e-13                   # the contractions the device kernel assembles
    assert abs(np.trace(R.rdm1(no, t1, t2, l1, l2)) - 2 * no) < 1e-12
