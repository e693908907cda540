"""CPU: the numpy restatement of the sector spectral functions (tests/_sector_gf_reference.py) on the block matrices of
tests/_sector_ipea_reference.matrix: the exact error bound of the Krylov resolvent, the residual estimate against the true
residual, orthogonality of the CGS2 basis, breakdown at the Krylov dimension, the sum rules of the pole strengths, and the refusal
of the host simulator, which has no Arnoldi kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

from pymes_amd.solver import subspace
from pymes_amd.solver.sectors import QuasiparticleTables
from tests import _sector_gf_reference as gf
from tests import _sector_ipea_reference as sq
from tests.test_sector_ipea_reference import all_targets, block_of, host_case
from tests.test_sector_reference import symmetric_amplitudes

KINDS = ("ip", "ea")
CASES = [(14, 2, "coulomb"), (14, 2, "tc"), (14, 3, "coulomb"), (14, 3, "tc"), (54, 5, "coulomb"), "twist"]
ETAS = (0.1, 0.02)
SIGMA_BOUND = 1e-11          # the project's bound on a sigma vector, per unit of its largest element
BREAKDOWN = 1e-10


@functools.lru_cache(maxsize=None)
def block_matrix(label, kind, which):
    """The block of the lowest (which = 0) or highest (-1) admissible target on the positions inside the space."""
    tab, tt, V, eps, ints, lists = host_case(label)
    p = all_targets(tab, kind)[which]
    qt = QuasiparticleTables(tt, kind, p)
    H = sq.matrix(qt, eps, block_of(tab, tt, V, ints, lists, qt), 0.1 * symmetric_amplitudes(tab, 5))
    keep = np.concatenate([[0], 1 + np.flatnonzero(qt.inside)])
    return p, np.ascontiguousarray(H[np.ix_(keep, keep)])


def frequencies(H, kind, n=41):
    """n frequencies across the spectrum of the block, in the energy convention of the poles (-w for IP, +w for EA)."""
    e = -gf.SIGN[kind] * np.linalg.eigvals(H).real
    pad = 0.1 * max(e.max() - e.min(), 1.0)
    return np.linspace(e.min() - pad, e.max() + pad, n)


def dims(dim):
    return sorted({min(m, dim + 1) for m in (dim + 1, 20, 60, 150)})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("label", CASES, ids=str)
def test_krylov_resolvent_within_its_exact_error_bound(label, kind):
    """x - x_m = (z + s H)^-1 r_m, so |G_m(z) - G(z)| <= ||(z + s H)^-1||_2 (|r_m| + 1e-11) per unit N_p, with the norm from
    numpy's SVD and r_m the true residual of V_m y; the residual estimate h_{m+1,m} |y_m| against the true residual within
    1e-12 max(1, |z| + ||H||); the basis orthonormal to subspace.ORTH_TOL; m = dim + 1 breaks down at the Krylov dimension and
    gives the exact resolvent; sum_j rho_j = 1 and sum_j rho_j theta_j = H_11 to 1e-12 ||H||."""
    for which in (0, -1):
        p, H = block_matrix(label, kind, which)
        dim, nrm_h = H.shape[0], np.linalg.norm(H, 2)
        omegas = frequencies(H, kind)
        V, Hb, k_all, broke = gf.arnoldi(H, dim + 1, BREAKDOWN)
        assert broke and k_all <= dim and Hb[k_all, k_all - 1] == 0.0 and not V[k_all].any()
        orth = np.abs(V[:k_all] @ V[:k_all].T - np.eye(k_all)).max()
        assert orth <= subspace.ORTH_TOL
        worst = dict(ratio_cut=0.0, ratio_full=0.0, est=0.0, sum0=0.0, sum1=0.0)
        for eta in ETAS:
            z = omegas + 1j * eta
            exact = gf.exact_resolvent(H, kind, z)
            rnorm = np.array([gf.resolvent_norm(H, kind, zz) for zz in z])
            for m in dims(dim):
                k = min(m, k_all)
                Hm = Hb[:k + 1, :k]
                Y, est = gf.shifted_solutions(Hm, kind, z)
                true = np.array([gf.true_residual(H, kind, zz, V, y) for zz, y in zip(z, Y)])
                bound = rnorm * (true + SIGMA_BOUND)
                err = np.abs(Y[:, 0] - exact)
                key = "ratio_full" if k == k_all else "ratio_cut"
                worst[key] = max(worst[key], (err / bound).max())
                worst["est"] = max(worst["est"], np.abs(est - true).max())
                assert (err <= bound).all(), (label, kind, p, m, eta, (err / bound).max())
                assert (np.abs(est - true) <= 1e-12 * np.maximum(1.0, np.abs(z) + nrm_h)).all()
                if k == k_all:
                    assert (est == 0.0).all()                  # breakdown: the space is invariant, the result exact
        for m in dims(dim):
            k = min(m, k_all)
            e, rho, res, theta = gf.poles(Hb[:k + 1, :k], kind)
            worst["sum0"] = max(worst["sum0"], abs(rho.sum() - 1.0))
            worst["sum1"] = max(worst["sum1"], abs((rho * theta).sum() - H[0, 0]))
            assert abs(rho.sum() - 1.0) <= 1e-12 * max(nrm_h, 1.0)
            assert abs((rho * theta).sum() - H[0, 0]) <= 1e-12 * max(nrm_h, 1.0)
            assert np.allclose(e, -gf.SIGN[kind] * theta)
        print(f"{label} {kind} target {p} (dim {dim}, Krylov dimension {k_all}): error / bound {worst['ratio_cut']:.2e} (truncated) "
              f"{worst['ratio_full']:.2e} (full), |estimate - true residual| {worst['est']:.1e}, max|V V^T - 1| {orth:.1e}, "
              f"sum rules {worst['sum0']:.1e} {worst['sum1']:.1e}, ||H|| {nrm_h:.2f}")


def test_one_step_as_the_device_entry_takes_it():
    """cgs2_step on a seeded orthonormal basis: the column, the norm and the new row satisfy w = V^T h + |w''| v; a combination
    of the rows breaks down."""
    rng = np.random.default_rng(4)
    V = np.linalg.qr(rng.standard_normal((257, 12)))[0].T
    w = rng.standard_normal(257)
    h, nrm, v = gf.cgs2_step(V, w)
    assert np.abs(V.T @ h + nrm * v - w).max() <= 1e-13 * np.linalg.norm(w)
    assert np.abs(V @ v).max() <= subspace.ORTH_TOL and abs(np.linalg.norm(v) - 1.0) <= 1e-14
    h, nrm, v = gf.cgs2_step(V, V.T @ rng.standard_normal(12), 1e-10)
    assert nrm == 0.0 and not v.any()


def test_quasiparticle_pole_selection():
    e = np.array([-1.0, -0.5 + 0.1j, -0.2, 0.3], dtype=complex)
    Z = np.array([0.1, 0.9, 0.5, 0.7], dtype=complex)
    res = np.array([1e-9, 1e-9, 1e-9, 1e-3])
    assert gf.quasiparticle(e, Z, res, 1e-6) == (-0.2, 0.5)
    assert all(np.isnan(gf.quasiparticle(e, Z, np.ones(4), 1e-6)))


def test_the_host_simulator_refuses_the_arnoldi_step_by_name(hostsim_lib):
    from pymes_amd._lib import PymesError
    from pymes_amd.device import Context
    ctx = Context(1, 1, lib=hostsim_lib)
    try:
        x = ctx.zeros((128,))
        p, size = C.c_void_p(x.ptr), C.c_int64(128)
        with pytest.raises(PymesError, match="sector_arnoldi_step: not available in this backend"):
            ctx.lib.call("pymes_sector_arnoldi_step", ctx.handle, p, 32, 32, 0, p, 1, 1e-10, p, C.byref(size), p)
        with pytest.raises(PymesError, match="sector_arnoldi_step: not available in this backend"):
            ctx.lib.call("pymes_sector_arnoldi_step", ctx.handle, None, 32, 32, 0, None, 1, 1e-10, None, C.byref(size), None)
    finally:
        ctx.close()


def test_header_and_signatures_name_the_new_entry():
    import os
    from pymes_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pymes_amd.h")).read()
    assert "pymes_sector_arnoldi_step" in _lib.SIGNATURES and "int pymes_sector_arnoldi_step(" in header
    assert "#define PYMES_SECTOR_ARNOLDI_MAX 512" in header
