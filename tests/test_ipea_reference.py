"""CPU: the numpy references of the IP- and EA-EOM-CCSD operators (tests/_ipea_reference.py, the GPU tests' oracle): the term
tables against the definition by the non-interacting orbital, the two closed-form limits, Koopmans at t = 0."""
import numpy as np
import pytest

from oracle.cases import random_case, synthetic_case
from oracle import cc_oracle as cc
from tests import _ipea_reference as R


def _random_inputs(kind, no, nv, seed):
    rng = np.random.default_rng(seed)
    f, V, _, t2 = random_case(no, nv, seed=seed)
    V = R.symmetrise(V)                                   # V_pqrs = V_qpsr is all that is left
    f = f + 0.03 * rng.standard_normal(f.shape)           # a non-symmetric, dressed-like Fock matrix
    s1, s2 = R.shapes(kind, no, nv)
    return f, V, t2, rng.standard_normal(s1), rng.standard_normal(s2)


@pytest.mark.parametrize("kind,eps_x", [("ip", 0.37), ("ip", -1.9), ("ea", -0.41), ("ea", 2.2)])
@pytest.mark.parametrize("no,nv", [(3, 5), (4, 3), (2, 7)])
def test_term_tables_equal_the_embedding(kind, eps_x, no, nv):
    f, V, t2, r1, r2 = _random_inputs(kind, no, nv, seed=7)
    assert np.abs(t2 - t2.transpose(1, 0, 3, 2)).max() < 1e-15
    a1, a2, leak = R.sigma_embedded(kind, no, f, V, t2, r1, r2, eps_x)
    b1, b2 = R.sigma_terms(kind, no, f, cc.split_blocks(no, V), t2, r1, r2)
    print(kind, no, nv, eps_x, "leak", leak, "dev", np.abs(a1 - b1).max(), np.abs(a2 - b2).max())
    assert leak < 1e-13                                   # the sector is closed, its doubles exchange-symmetric
    assert np.abs(a1 - b1).max() < 1e-13 and np.abs(a2 - b2).max() < 1e-13


@pytest.mark.parametrize("kind", ["ip", "ea"])
def test_the_operator_does_not_depend_on_eps_x(kind):
    f, V, t2, r1, r2 = _random_inputs(kind, 3, 5, seed=5)
    a = R.sigma_embedded(kind, 3, f, V, t2, r1, r2, 0.37)
    b = R.sigma_embedded(kind, 3, f, V, t2, r1, r2, -1.9)
    assert np.abs(a[0] - b[0]).max() < 1e-13 and np.abs(a[1] - b[1]).max() < 1e-13


def test_block_lists():
    assert "abcd" not in R.BLOCKS["ip"] and "abic" not in R.BLOCKS["ip"]
    assert {"abcd", "abic", "iabc"} <= set(R.BLOCKS["ea"])
    assert len(R.IP_SINGLES) == len(R.EA_SINGLES) == 7 and len(R.IP_DOUBLES) == len(R.EA_DOUBLES) == 32


@pytest.mark.parametrize("nv,seed", [(6, 3), (9, 4)])
def test_two_electrons_ip_spectrum_is_exact(nv, seed):
    """One occupied orbital: CCSD is exact, the N-1 states are one-electron states, so the WHOLE spectrum of the IP operator
    is eig(h) - (E_HF + E_CCSD)."""
    no = 1
    f, V, _, _ = synthetic_case(no, nv, seed=seed, scale=0.6)
    h, _ = R.fock_and_core(no, f, V)
    r, fd, Vd = R.converged_case(no, f, V)
    w = np.linalg.eigvals(R.dense("ip", no, fd, Vd, r["t2"]))
    exact = np.sort(np.linalg.eigvalsh(h)) - (R.hf_energy(no, h, f) + r["e"])
    dev = np.abs(np.sort(w.real) - exact).max()
    print("IP, two electrons", nv, "max deviation", dev, "max |imag|", np.abs(w.imag).max())
    assert len(w) == 1 + nv and np.abs(w.imag).max() < 1e-11 and dev < 1e-11


@pytest.mark.parametrize("no,seed", [(5, 3), (7, 4)])
def test_two_holes_ea_spectrum_is_exact(no, seed):
    """One virtual orbital: the N+1 states are one-hole states of the completely filled determinant, so the WHOLE spectrum of
    the EA operator is (E_full - eig(f_full)) - (E_HF + E_CCSD)."""
    nv = 1
    f, V, _, _ = synthetic_case(no, nv, seed=seed, scale=0.6)
    h, f_full = R.fock_and_core(no, f, V)
    r, fd, Vd = R.converged_case(no, f, V)
    w = np.linalg.eigvals(R.dense("ea", no, fd, Vd, r["t2"]))
    exact = np.sort(R.full_energy(h, f_full) - np.linalg.eigvalsh(f_full)) - (R.hf_energy(no, h, f) + r["e"])
    dev = np.abs(np.sort(w.real) - exact).max()
    print("EA, two holes", no, "max deviation", dev, "max |imag|", np.abs(w.imag).max())
    assert len(w) == 1 + no and np.abs(w.imag).max() < 1e-11 and dev < 1e-11


@pytest.mark.parametrize("kind", ["ip", "ea"])
def test_koopmans_at_zero_amplitudes(kind):
    no, nv = 3, 4
    f, V, _, eps = synthetic_case(no, nv, seed=2)
    Vd = cc.split_blocks(no, V)
    t2 = np.zeros((nv, nv, no, no))
    s1, s2 = R.shapes(kind, no, nv)
    for p in range(s1[0]):
        r1 = np.zeros(s1)
        r1[p] = 1.0
        a, _ = R.sigma_terms(kind, no, f, Vd, t2, r1, np.zeros(s2))
        want = -f[:no, p] if kind == "ip" else f[no:, no + p]
        assert np.abs(a - want).max() < 1e-14
    d1, d2 = R.diagonals(kind, no, f, Vd, t2)
    assert np.abs(d1 - (-eps[:no] if kind == "ip" else eps[no:])).max() < 1e-14
    H = R.dense(kind, no, f, Vd, t2)
    n1 = s1[0]
    assert np.abs(H.diagonal()[:n1] - d1).max() < 1e-14


@pytest.mark.parametrize("kind", ["ip", "ea"])
def test_diagonals_are_the_dressed_one_body_part(kind):
    """d1 is the exact diagonal of the singles block; d2 differs from the exact diagonal only by two-body slices."""
    no, nv = 3, 4
    f, V, _, _ = synthetic_case(no, nv, seed=5)
    r, fd, Vd = R.converged_case(no, f, V, delta_e=1e-12)
    d1, d2 = R.diagonals(kind, no, fd, Vd, r["t2"])
    H = R.dense(kind, no, fd, Vd, r["t2"])
    n1 = d1.size
    assert np.abs(H.diagonal()[:n1] - d1).max() < 1e-13
    assert np.abs(H.diagonal()[n1:] - d2.ravel()).max() < 0.5          # same scale: a usable preconditioner
