"""CPU: the numpy reference of the transition densities (tests/_transition_reference.py): the definitions D1-D3 against an exact
two-electron calculation, and the written-out contractions (what the device kernel assembles) against the definitions."""
import numpy as np
import pytest

from tests import _lambda_reference as R
from tests import _transition_reference as X


def test_two_electron_anchor():
    """(no, nv) = (1, 4): CCSD and EOM-CCSD are exact for two electrons, so w_k and S_k of the three lowest roots equal the
    FCI gaps and <0|O|k>^2.  Measured: 2e-14 on the energies, 3e-13 on the strengths."""
    no, nv = 1, 4
    ref = X.reference_transitions(no, nv, 3, True, 3, 0.05)
    O = X.seeded_operator(no + nv)
    gaps, mom2 = X.two_electron_fci(ref["f"], ref["V"], O)
    gl, gr = X.transition_densities_definition(no, ref["t1"], ref["t2"], ref["lam"], ref["ls"], ref["rs"])
    s = X.strengths(gl, gr, O)
    for k in range(3):
        print("root %d  w %.14f  FCI %.14f  S %.14f  FCI %.14f" % (k, ref["w"][k], gaps[k], s[k], mom2[k]))
    assert ref["imag"] == 0.0
    assert np.abs(ref["w"] - gaps[:3]).max() < 1e-10
    assert np.abs(s - mom2[:3]).max() < 1e-10


def test_two_electron_anchor_tells_the_coefficient_of_term_3():
    """With 1 instead of 2 in front of lambda2 r1 R1(f) the first strength moves in the second digit."""
    no, nv = 1, 4
    ref = X.reference_transitions(no, nv, 3, True, 3, 0.05)
    O = X.seeded_operator(no + nv)
    _, mom2 = X.two_electron_fci(ref["f"], ref["V"], O)
    lam, t1, t2 = ref["lam"], ref["t1"], ref["t2"]
    r1, r2 = ref["rs"][0]
    half = X._undress(no, X._lagrange_coefficients(no, t2, np.einsum("abij,ai->bj", lam[1], r1), np.zeros_like(t2)), t1)
    wrong = (ref["gl"][0] * O).sum() * ((ref["gr"][0] - half) * O).sum()
    assert abs(wrong - mom2[0]) > 1e-3


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_written_out_densities_equal_the_definitions(no, nv, seed, hermitian):
    ref = X.reference_transitions(no, nv, seed, hermitian)
    gl, gr = X.transition_densities_definition(no, ref["t1"], ref["t2"], ref["lam"], ref["ls"], ref["rs"])
    dl, dr = np.abs(gl - ref["gl"]).max(), np.abs(gr - ref["gr"]).max()
    print("(%d,%d) hermitian %s: |gammaL - definition| %.2e  |gammaR - definition| %.2e" % (no, nv, hermitian, dl, dr))
    assert dl < 1e-12 and dr < 1e-12


@pytest.mark.parametrize("no,nv,seed", [(2, 3, 5), (3, 5, 6)])
def test_written_out_densities_for_vectors_that_solve_nothing(no, nv, seed):
    t1, t2, lam, ls, rs = X.density_inputs(no, nv, seed)
    gl, gr = X.transition_densities_definition(no, t1, t2, lam, ls, rs)
    tl, tr = X.transition_density_terms(no, t1, t2, lam, ls, rs)
    assert np.abs(gl - tl).max() < 1e-12 and np.abs(gr - tr).max() < 1e-12


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_dense_vectors_solve_their_equations(no, nv, seed, hermitian):
    """The dense reference: real, separated roots; A r = w r, A^T l = w l, <l_j, r_k> = delta_jk; for the non-hermitian variant
    the left vector of root 0 is not the right one."""
    from oracle import eom_oracle as eo
    ref = X.reference_transitions(no, nv, seed, hermitian)
    w, fd, Vd, t2 = ref["w"], ref["fd"], ref["Vd"], ref["t2"]
    assert ref["imag"] == 0.0 and np.diff(w).min() > 0.05
    for k in range(3):
        r, l = ref["rs"][k], ref["ls"][k]
        s = (eo.sigma_singles(no, fd, Vd, r[0], r[1], t2), eo.sigma_doubles(no, fd, Vd, r[0], r[1], t2))
        o = R.left_sigma(no, fd, Vd, l[0], l[1], t2)
        assert max(np.abs(s[0] - w[k] * r[0]).max(), np.abs(s[1] - w[k] * r[1]).max()) < 1e-11
        assert max(np.abs(o[0] - w[k] * l[0]).max(), np.abs(o[1] - w[k] * l[1]).max()) < 1e-11 * max(1.0, np.abs(l[1]).max())
    g = np.array([[X.dot(l, r) for r in ref["rs"]] for l in ref["ls"]])
    assert np.abs(g - np.eye(3)).max() < 1e-12
    if not hermitian:
        l, r = ref["ls"][0], ref["rs"][0]
        cos = X.dot(l, r) / np.sqrt(X.dot(l, l) * X.dot(r, r))
        print("(%d,%d) cosine between the left and the right vector of root 0: %.3f" % (no, nv, cos))
        assert cos < 0.999


def test_complex_pairs_without_the_eightfold_symmetry():
    """random_problem(..., eight=False) has complex-conjugate pairs among its lowest roots: the case the solver refuses."""
    no, nv = 2, 3
    f, V = R.random_problem(no, nv, seed=11, eight=False)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    _, _, _, imag = X.dense_eom(no, fd, Vd, t2, 4)
    print("largest imaginary part among the four lowest roots: %.3e" % imag)
    assert imag > 1e-6
