"""Frozen natural orbitals (pymes_amd/solver/fno.py) on the host: the sign rule, the truncation rules, the argument checks of
``truncate`` and ``CCSD.solve``, and pymes_derive_context on the host simulator (all 16 blocks against numpy, refusals)."""
import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.integral.partition import BLOCK_NAMES, part_2_body_int
from pymes_amd.solver import fno
from pymes_amd.solver.ccsd import CCSD
from tests import _fno_reference as ref


def test_sign_rule_makes_largest_component_positive():
    M = np.array([[0.1, -0.9, 0.5], [-0.8, 0.2, -0.5], [0.3, 0.1, 0.0]])
    S = fno.sign_fix(M)
    assert np.array_equal(S[:, 0], -M[:, 0])
    assert np.array_equal(S[:, 1], -M[:, 1])
    assert np.array_equal(S[:, 2], M[:, 2])          # a tie: the first component of largest magnitude decides
    assert np.array_equal(fno.sign_fix(-M), S)
    assert np.array_equal(S, ref.sign_rule(M))


def test_natural_orbitals_sorted_and_signed():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((7, 7))
    D = A @ A.T
    occ, N = fno.natural_orbitals(D)
    assert np.all(np.diff(occ) <= 0)
    assert np.allclose(D @ N, N * occ, atol=1e-12)
    for k in range(7):
        assert N[np.argmax(np.abs(N[:, k])), k] > 0


def test_truncation_rules():
    occ = np.array([1.0e-1, 2.0e-2, 5.0e-3, 5.0e-3, 1.0e-4])
    assert fno.n_kept(occ) == 5
    assert fno.n_kept(occ, nv_keep=2) == 2
    assert fno.n_kept(occ, occ_threshold=5.0e-3) == 4          # ">=": equal occupations are kept
    assert fno.n_kept(occ, occ_threshold=6.0e-3) == 2
    with pytest.raises(ValueError, match="keeps no virtual"):
        fno.n_kept(occ, occ_threshold=1.0)


def test_semicanonical_diagonalises_the_kept_block():
    rng = np.random.default_rng(1)
    f_vv = np.diag(np.sort(rng.random(6)) + 1.0)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    N = Q[:, :4]
    Cm, e = fno.semicanonical(N, f_vv)
    assert np.all(np.diff(e) >= 0)
    F = Cm.T @ f_vv @ Cm
    assert np.abs(F - np.diag(e)).max() < 1e-12
    assert np.abs(Cm.T @ Cm - np.eye(4)).max() < 1e-12


@pytest.mark.parametrize("kw, match", [
    (dict(n_frozen=3), r"n_frozen = 3 must lie in \[0, no\)"),
    (dict(n_frozen=-1), r"n_frozen = -1 must lie in \[0, no\)"),
    (dict(nv_keep=0), r"nv_keep = 0 must lie in \[1, nv\]"),
    (dict(nv_keep=9), r"nv_keep = 9 must lie in \[1, nv\]"),
    (dict(nv_keep=2, occ_threshold=1e-3), "at most one of occ_threshold and nv_keep"),
])
def test_truncate_argument_checks(kw, match):
    no, nv = 3, 8
    f, V, _, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    with pytest.raises(ValueError, match=match):
        fno.truncate(no, f, V, **kw)


def test_truncate_refuses_non_canonical_fock_and_tc_factors():
    no, nv = 3, 8
    f, V, _, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    g = f.copy()
    g[no, no + 1] = g[no + 1, no] = 1e-3
    with pytest.raises(ValueError, match="canonical"):
        fno.truncate(no, g, V, nv_keep=4)
    B = np.random.default_rng(0).standard_normal((6, no + nv, no + nv))
    with pytest.raises(ValueError, match="Hermitian"):
        fno.truncate(no, f, ("factors", B), nv_keep=4)
    with pytest.raises(ValueError, match="shard= is supported with the \\('factors', B\\) source only"):
        fno.truncate(no, f, V, nv_keep=4, shard=(0, 2))


def test_ccsd_solve_refuses_fno_with_sharded_integrals_and_factors():
    no, nv = 3, 8
    f, V, _, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    with pytest.raises(ValueError, match="shard_integrals=True with frozen_core"):
        CCSD(no, shard_integrals=True).solve(f, V, fno_nv=4)
    with pytest.raises(ValueError, match="for factors call fno.truncate"):
        CCSD(no).solve(f, ("factors", np.zeros((2, no + nv, no + nv))), frozen_core=1)


def test_derive_context_blocks_match_numpy(hostsim_lib):
    no, nv, nf, k = 4, 9, 1, 6
    f, V, _, _ = synthetic_case(no, nv, seed=1, scale=0.3)
    ints = DeviceIntegrals.from_V_pqrs(no, V, lib=hostsim_lib)
    try:
        Q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((nv, nv)))
        Cm = Q[:, :k]
        new = fno.derive_context(ints, nf, Cm)
        try:
            assert (new.no, new.nv) == (no - nf, k)
            U = np.zeros((no + nv, no - nf + k))
            U[nf:no, :no - nf] = np.eye(no - nf)
            U[no:, no - nf:] = Cm
            want = part_2_body_int(no - nf, ref.transform(V, U))
            for nm in BLOCK_NAMES:
                got = new.block(nm).get()
                assert np.abs(got - want[nm]).max() <= 1e-12 * np.abs(want[nm]).max(initial=1.0), nm
        finally:
            new.ctx.close()
    finally:
        ints.ctx.close()


def test_derive_context_refusals(hostsim_lib):
    no, nv = 3, 6
    f, V, _, _ = synthetic_case(no, nv, seed=2, scale=0.3)
    lib = hostsim_lib
    src = Context(no, nv, lib=lib)
    src.set_V_pqrs(V)
    I = np.eye(nv)
    opened = [src]

    def ctx(o, v, **kw):
        c = Context(o, v, lib=lib, **kw)
        opened.append(c)
        return c

    def call(s, d, nf, Cm, nvd):
        Cm = np.ascontiguousarray(Cm)
        lib.call("pymes_derive_context", s.handle, d.handle, nf, _lib.host_ptr(Cm), nvd)

    try:
        cases = [
            (lambda: call(src, src, 0, I, nv), "same context"),
            (lambda: call(src, ctx(no, nv), no, I, nv), r"n_frozen = 3 outside \[0, no\)"),
            (lambda: call(src, ctx(no, nv), -1, I, nv), r"n_frozen = -1 outside"),
            (lambda: call(src, ctx(no, 1), 0, I, 0), r"nv_dst = 0 outside \[1, nv\]"),
            (lambda: call(src, ctx(no, nv), 0, I, nv + 1), r"nv_dst = 7 outside \[1, nv\]"),
            (lambda: call(src, ctx(no - 1, nv), 0, I, nv), "expected"),
        ]
        full = ctx(no, nv)
        full.set_V_pqrs(V)
        cases.append((lambda: call(src, full, 0, I, nv), "not empty"))
        partial = ctx(no, nv)
        partial.set_V_block("ijab", V[:no, :no, no:, no:])
        cases.append((lambda: call(partial, ctx(no, nv), 0, I, nv), "lacks the integral block"))
        shard_src = ctx(no, nv, shard=(0, 2))
        shard_src.set_V_pqrs(V)
        cases.append((lambda: call(shard_src, ctx(no, nv), 0, I, nv), "source context shards its integrals"))
        cases.append((lambda: call(src, ctx(no, nv, shard=(0, 2)), 0, I, nv), "destination context shards"))
        Vtc = V.copy()
        Vtc[no:, no:, :no, no:] += 1e-3 * np.random.default_rng(0).standard_normal((nv, nv, no, nv))   # abic only: V_pqrs != V_rspq
        tc = ctx(no, nv)
        tc.set_V_pqrs(Vtc)
        cases.append((lambda: call(tc, ctx(no, nv), 0, I, nv), "Hermitian"))
        for fn, match in cases:
            with pytest.raises(_lib.PymesError, match=match):
                fn()
        with pytest.raises(ValueError, match="sharded context"):
            fno.truncate(no, f, DeviceIntegrals(shard_src), nv_keep=3)
    finally:
        for c in opened:
            c.close()


@pytest.mark.parametrize("nf", [0, 1, 2])
def test_density_from_vijab_states_the_same_definition(nf):
    """The reference the multi-tile GPU test uses (V_ijab and orbital energies alone) against the one from the full V_pqrs."""
    no, nv = 5, 11
    f, V, _, _ = synthetic_case(no, nv, seed=3, scale=0.3)
    D, e = ref.mp2_density(no, f, V, nf)
    D2, e2 = ref.mp2_density_ijab(V[:no, :no, no:, no:], np.diag(f)[:no], np.diag(f)[no:], nf)
    assert np.abs(D2 - D).max() <= 1e-14 * np.abs(D).max() and abs(e2 - e) <= 1e-14 * abs(e)
