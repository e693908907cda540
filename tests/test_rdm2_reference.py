"""CPU: the numpy reference of the CCSD two-particle response density (tests/_rdm2_reference.py) against its definition, the
Lagrangian it is the derivative of, the CCSD energy and the trace identities of the full two-particle density matrix."""
import functools

import numpy as np
import pytest

from oracle import cc_oracle as cc
from pymes_amd.solver.lambda_ccsd import RDM2_IMAGE, RDM2_NAMES, RDM2_STORED, full_rdm2
from tests import _lambda_reference as LR
from tests import _rdm2_reference as R


@functools.lru_cache(maxsize=None)
def _by_definition(no, nv):
    """(inputs, Gamma [n,n,n,n] by definition): (3,5) from the golden file, (2,3) evaluated here (625 Lagrangians)."""
    if (no, nv) == R.GOLDEN_RDM2[1:3]:
        _, _, inp, G = R.golden_rdm2()
        return inp, G
    inp = LR.density_inputs(no, nv, 5)
    return inp, R.lagrangian_density2(no, *inp)


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5)])
def test_terms_are_the_derivative_of_the_lagrangian(no, nv):
    inp, G = _by_definition(no, nv)
    assert np.abs(inp[0]).max() > 0.01                        # t1 != 0: the back-transformation and the Fock part are exercised
    blocks = R.rdm2_terms(no, *inp)
    ref = cc.split_blocks(no, G)
    assert set(blocks) == set(cc.BLOCK_NAMES) == set(RDM2_NAMES)
    for nm in cc.BLOCK_NAMES:
        assert blocks[nm].shape == ref[nm].shape
        assert np.abs(blocks[nm] - ref[nm]).max() < 1e-13, nm
        assert np.abs(ref[nm]).max() > 1e-4, nm               # no block is trivially zero
    # the projection: a block and its image under (pq,rs) -> (qp,sr) are the same data; nothing is hermitian
    assert np.abs(G - G.transpose(1, 0, 3, 2)).max() < 1e-15
    assert np.abs(G - G.transpose(2, 3, 0, 1)).max() > 1e-3
    for image, stored in RDM2_IMAGE.items():
        assert np.array_equal(blocks[image], blocks[stored].transpose(1, 0, 3, 2))
    assert len(RDM2_STORED) == 10 and set(RDM2_STORED) | set(RDM2_IMAGE) == set(RDM2_NAMES)


def test_golden_file_is_the_definition_on_a_sample():
    """The recorded (3,5) density: a handful of its entries evaluated afresh from the Lagrangian."""
    no, nv, inp, G = R.golden_rdm2()
    n = no + nv
    rng = np.random.default_rng(0)
    f0, e = np.zeros((n, n)), np.zeros((n, n, n, n))
    for idx in rng.integers(0, n, size=(12, 4)):
        p, q, r, s = (int(x) for x in idx)
        e[...] = 0.0
        e[p, q, r, s] = 1.0
        a = R.lagrangian(no, f0, e, *inp)
        e[...] = 0.0
        e[q, p, s, r] = 1.0
        b = R.lagrangian(no, f0, e, *inp)
        assert abs(0.5 * (a + b) - G[p, q, r, s]) < 1e-14


@pytest.mark.parametrize("eight", [False, True])
def test_densities_reproduce_the_lagrangian(eight):
    """L(f, V) = sum gamma f + sum Gamma V for any V with V_pqrs = V_qpsr, at inputs that solve nothing."""
    no, nv = 3, 5
    inp = LR.density_inputs(no, nv, 23)
    f, V = LR.random_problem(no, nv, 4, eight=eight)
    if not eight:
        f = f + 0.1 * np.random.default_rng(2).standard_normal(f.shape)            # (not symmetric either)
        assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-3
    gamma = LR.density_terms(no, *inp)
    G = R.assemble(no, R.rdm2_terms(no, *inp))
    want = R.lagrangian(no, f, V, *inp)
    got = (gamma * f).sum() + (G * V).sum()
    assert abs(got - want) < 1e-13 * max(1.0, (np.abs(gamma) * np.abs(f)).sum() + (np.abs(G) * np.abs(V)).sum())
    # the two halves separately: L is linear and homogeneous
    assert abs((G * V).sum() - R.lagrangian(no, np.zeros_like(f), V, *inp)) < 1e-13
    assert abs((gamma * f).sum() - R.lagrangian(no, f, np.zeros_like(V), *inp)) < 1e-13


@functools.lru_cache(maxsize=None)
def _converged(eight):
    no, nv = 3, 5
    f, V = LR.random_problem(no, nv, 1, eight=eight)
    t1, t2, fd, Vd, e = LR.converged_state(no, f, V)
    l1, l2 = LR.solve_lambda(no, fd, Vd, t2)
    return no, f, V, (t1, t2, l1, l2), e


@pytest.mark.parametrize("eight", [True, False])
def test_density_energy_is_the_ccsd_energy(eight):
    """At R = 0 the Lagrangian is the energy, whatever the symmetry of V: "density e" = sum gamma f + sum Gamma V equals the
    oracle's CCSD correlation energy within the bound the project uses for converged quantities."""
    no, f, V, inp, e = _converged(eight)
    gamma = LR.density_terms(no, *inp)
    Gb = R.rdm2_terms(no, *inp)
    de = (gamma * f).sum() + R.contract_blocks(Gb, cc.split_blocks(no, V))
    assert abs(de - e) < 1e-9
    # ... and the full two-particle density matrix gives the same energy through E = sum h D1 + 1/2 sum V D
    h = f - 2.0 * np.einsum("piqi->pq", V[:, :no, :, :no]) + np.einsum("piiq->pq", V[:, :no, :no, :])
    D1 = gamma.copy()
    D1[np.arange(no), np.arange(no)] += 2.0
    D = full_rdm2(no, gamma, Gb)
    e_hf = 2.0 * np.trace(h[:no, :no]) + 2.0 * np.einsum("ijij->", V[:no, :no, :no, :no]) - np.einsum("ijji->", V[:no, :no, :no, :no])
    assert abs((h * D1).sum() + 0.5 * (V * D).sum() - e_hf - e) < 1e-9


def test_full_rdm2_energy_identity_for_arbitrary_inputs():
    """E = sum h D1 + 1/2 sum V D with f = h + sum_i (2 V_piqi - V_piiq) is E_HF + L(f, V) identically in (t, lambda): the
    coefficients of full_rdm2 are pinned by it (V_pqrs = V_qpsr only)."""
    no, nv = 3, 5
    inp = LR.density_inputs(no, nv, 31)
    f, V = LR.random_problem(no, nv, 8, eight=False)
    gamma = LR.density_terms(no, *inp)
    Gb = R.rdm2_terms(no, *inp)
    h = f - 2.0 * np.einsum("piqi->pq", V[:, :no, :, :no]) + np.einsum("piiq->pq", V[:, :no, :no, :])
    D1 = gamma.copy()
    D1[np.arange(no), np.arange(no)] += 2.0
    D = full_rdm2(no, gamma, Gb)
    e_hf = 2.0 * np.trace(h[:no, :no]) + 2.0 * np.einsum("ijij->", V[:no, :no, :no, :no]) - np.einsum("ijji->", V[:no, :no, :no, :no])
    assert abs((h * D1).sum() + 0.5 * (V * D).sum() - e_hf - R.lagrangian(no, f, V, *inp)) < 1e-12
    with pytest.raises(ValueError, match="all sixteen blocks"):
        full_rdm2(no, gamma, {nm: Gb[nm] for nm in RDM2_STORED})


def test_trace_identities_of_the_full_density():
    """Number conservation: sum_pq D_pqpq = N (N - 1) and sum_q (D_pqrq + D_rqpq) / 2 = (N - 1) (D1_pr + D1_rp) / 2.  Both were
    checked on this reference for arbitrary (t, lambda) before being asserted: the package's functional satisfies
    them to rounding, and the partial trace even without the symmetrisation."""
    no, nv = 3, 5
    N = 2 * no
    for inp in (LR.density_inputs(no, nv, 11), _converged(True)[3]):
        gamma = LR.density_terms(no, *inp)
        D1 = gamma.copy()
        D1[np.arange(no), np.arange(no)] += 2.0
        D = full_rdm2(no, gamma, R.rdm2_terms(no, *inp))
        assert abs(np.trace(D1) - N) < 1e-10
        assert abs(np.einsum("pqpq->", D) - N * (N - 1)) < 1e-10
        part = 0.5 * (np.einsum("pqrq->pr", D) + np.einsum("rqpq->pr", D))
        assert np.abs(part - (N - 1) * 0.5 * (D1 + D1.T)).max() < 1e-10
        assert np.abs(np.einsum("pqrq->pr", D) - (N - 1) * D1).max() < 1e-10
