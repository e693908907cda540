"""CPU: the numpy references of Lambda-CCSD(T) (tests/_lambda_triples_reference.py) against each other: the closed-shell
loop against the spin-orbital expression on integrals without V_pqrs = V_rspq, the Hermitian limit against (T), the
multiplicity sum against the full sum, and the normalisation of the library's Lambda pinned by converged CCSD states."""
import numpy as np
import pytest

from tests import _lambda_reference as LR
from tests import _lambda_triples_reference as LT
from tests import _triples_reference as R


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4)])
@pytest.mark.parametrize("with_l1", [True, False])
def test_spatial_equals_spin_orbital_non_hermitian(no, nv, with_l1):
    f, V, eps, T, lam1, lam2 = LT.problem(no, nv, seed=10 * no + nv)
    assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-3
    lam1 = lam1 if with_l1 else None
    e, scale = LT.energy(no, V, eps, T, lam1, lam2)
    ref = LT.spin_orbital_energy(no, V, eps, T, lam1, lam2)
    assert scale > 1e-8
    assert abs(e - ref) <= 1e-12 * scale, (e, ref, scale)


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4), (4, 6)])
def test_hermitian_limit_is_plain_triples(no, nv):
    V = R.four_fold_V(no + nv, seed=no + nv)
    eps = LT.gapped_eps(no, nv, seed=5)
    t1, T = R.random_amplitudes(no, nv, seed=7)
    lam1, lam2 = LT.library_normalisation(t1, T)
    e, _ = LT.energy(no, V, eps, T, lam1, lam2)
    ref = R.energy(no, V, eps, t1, T)
    assert abs(e - ref) <= 1e-13 * abs(ref), (e, ref)


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4)])
def test_multiplicity_sum_equals_full_sum(no, nv):
    f, V, eps, T, lam1, lam2 = LT.problem(no, nv, seed=3 * no + nv)
    e, scale = LT.energy(no, V, eps, T, lam1, lam2)
    full = LT.full_sum(no, V, eps, T, lam1, lam2)
    assert abs(e - full) <= 1e-12 * scale, (e, full, scale)


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 4)])
def test_library_lambda_normalisation(no, nv):
    """Converged CCSD and its Lambda for weak 8-fold symmetric integrals: lam2 is 2T - T^x to a few per cent, so E_Lambda(T) / E(T)
    must be close to 1 (1.0068 and 0.9968 at these two sizes).  A wrong sign or a factor 2/3, 3/2 or 2 in the conversion of
    the library's Lambda falls far outside the band."""
    f, V = LR.random_problem(no, nv, 3, scale=0.02)
    f = np.diag(np.diag(f))
    t1, t2, fd, Vd, _ = LR.converged_state(no, f, V)
    lam1, lam2 = LR.solve_lambda(no, fd, Vd, t2)
    eps = np.diag(f).copy()
    e_t = R.energy(no, V, eps, t1, t2)
    e_l, _ = LT.energy(no, V, eps, t2, lam1, lam2)
    assert abs(e_t) > 1e-12
    assert 0.97 <= e_l / e_t <= 1.03, (e_l, e_t, e_l / e_t)
