"""GPU: the sector spectral functions (pymes_amd/solver/ueg_eom.py, SectorSpectralFunction; csrc/kernels_sector.hip,
pymes_sector_arnoldi_step): the step entry alone against numpy CGS2, the Arnoldi relation on the device, G against the
numpy resolvent of the block inside its exact error bound, poles against the sector IP / EA roots and numpy's residues, the
normalisation against n(k) and the dense Y_oo / Y_vv, SectorCCD.solve(spectral=...), and the refusals."""
import ctypes as C

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.solver import subspace
from pymes_amd.solver.sectors import QuasiparticleTables
from tests import _sector_gf_reference as gf
from tests import _sector_ipea_reference as sq
from tests.test_gpu_sector_cc import quiet
from tests.test_gpu_sector_ipea import (bits, block_spectrum, converged, ctx, hamiltonians, ladders_for,  # noqa: F401 (fixtures)
                                        reference_blocks)
from tests.test_gpu_sector_lambda import symmetric
from tests.test_sector_ipea_reference import all_targets, some_targets

pytestmark = pytest.mark.gpu
KINDS = ("ip", "ea")
SIGMA_BOUND = 1e-11


def record(line):
    """The observed differences: `pytest -s` prints them, and profiles/sector_gf/gpu_test_errors.txt keeps one such run."""
    print(line)


# ---- the step entry alone ------------------------------------------------------------------------------------------------
def run_step(ctx, V, w, pitch, rows, breakdown=1e-10, status=0, extra_ldh=0):
    """One pymes_sector_arnoldi_step on a basis of ``rows`` allocated rows ``pitch`` apart, everything the call must not touch
    filled with NaN (the pad of every row, the rows behind j + 1, the rest of the Hessenberg matrix, the workspace).  Returns
    (basis [rows, pitch], hess [j+2, ldh], status) as the device left them."""
    from pymes_amd.solver.ueg_eom import arnoldi_step, arnoldi_workspace
    j, length = V.shape[0] - 1, V.shape[1]
    host = np.full((rows, pitch), np.nan)
    host[:j + 1, :length], host[j + 1, :length] = V, w
    ldh = j + 1 + extra_ldh
    basis, hess = ctx.array(host.ravel()), ctx.array(np.full((j + 2) * ldh, np.nan))
    flag = ctx.array(np.array([status], dtype=np.int64).view(np.float64))
    ws = ctx.array(np.full(arnoldi_workspace(ctx, length, j), np.nan))
    try:
        arnoldi_step(ctx, basis, pitch, length, j, hess, ldh, breakdown, ws, flag)
        return basis.get().reshape(rows, pitch), hess.get().reshape(j + 2, ldh), int(flag.get().view(np.int64)[0])
    finally:
        for arr in (basis, hess, flag, ws):
            arr.free()


def untouched(got, V, w, j, length):
    """Everything but the valid part of row j + 1 is bit-identical to what went in (NaN pads included)."""
    want = np.full(got.shape, np.nan)
    want[:j + 1, :length] = V
    mask = np.ones(got.shape, dtype=bool)
    mask[j + 1, :length] = False
    return np.array_equal(bits(got[mask]), bits(want[mask]))


# 33 ... 4099: one to 17 chunks of 256 (odd, one past a chunk, not a multiple); 262221: the 1024-wide chunks taken from
# len = 262144 (two values of j there: the transfers of such a basis are what takes the time)
@pytest.mark.parametrize("length", [33, 257, 1000, 4099, 262221])
def test_step_against_numpy_cgs2(ctx, length):
    """Bases from numpy's QR of seeded matrices, pitch = len rounded up to 32 plus 32 with the pad filled with NaN: the Hessenberg
    column to 1e-13 |w|, max|V v_new| <= subspace.ORTH_TOL, ||v_new| - 1| <= 1e-14, the pad and every other row bit-identical,
    identical bits on a repeated call and with another pitch, another ldh and more allocated rows.  (j + 2 <= len: a basis
    cannot hold more orthonormal rows than its length.)"""
    rng = np.random.default_rng(length)
    pitch = -(-length // 32) * 32 + 32
    for j in ((1, 33) if length > 100000 else (0, 1, 31, 32, 33, 100)):
        if j + 2 > length:
            continue
        V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((length, j + 1)))[0].T)
        w = rng.standard_normal(length) * 3.0
        col, nrm, v = gf.cgs2_step(V, w)
        got, hess, flag = run_step(ctx, V, w, pitch, j + 2)
        wn = np.linalg.norm(w)
        new = got[j + 1, :length]
        e_col = max(np.abs(hess[:j + 1, j] - col).max(), abs(hess[j + 1, j] - nrm))
        e_orth, e_norm = np.abs(V @ new).max(), abs(np.linalg.norm(new) - 1.0)
        record(f"step len {length} j {j}: |column - numpy| = {e_col:.2e} (|w| = {wn:.2f}), max|V v| = {e_orth:.2e}, "
               f"||v| - 1| = {e_norm:.2e}, |v - numpy| = {np.abs(new - v).max():.2e}")
        assert np.all(np.isfinite(new)) and np.all(np.isfinite(hess[:, j]))
        assert e_col <= 1e-13 * wn
        assert e_orth <= subspace.ORTH_TOL
        assert e_norm <= 1e-14
        assert flag == 0
        assert untouched(got, V, w, j, length)
        assert np.isnan(hess[:, :j]).all()                                # the other columns are not written
        again, hess2, _ = run_step(ctx, V, w, pitch, j + 2)
        wide, hess3, _ = run_step(ctx, V, w, pitch + 64, j + 5, extra_ldh=3)
        assert untouched(wide, V, w, j, length)
        for other, h in ((again, hess2), (wide, hess3)):
            assert np.array_equal(bits(other[j + 1, :length]), bits(new))
            assert np.array_equal(bits(h[:, j]), bits(hess[:, j]))


@pytest.mark.parametrize("length", [33, 1000, 262221])
def test_step_breakdown(ctx, length):
    """w a combination of the rows (and the full space at len = 33, j = 32): an exact 0.0 in hess[j+1, j], a +0.0 row, status
    j + 1; a later breakdown does not overwrite the first, and a step without one leaves the status alone."""
    rng = np.random.default_rng(7 + length)
    pitch = -(-length // 32) * 32 + 32
    for j in {33: (5, 32), 1000: (5, 40)}.get(length, (5,)):
        V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((length, j + 1)))[0].T)
        w = V.T @ rng.standard_normal(j + 1)
        got, hess, flag = run_step(ctx, V, w, pitch, j + 2)
        assert bits(hess[j + 1:j + 2, j])[0] == 0
        assert np.array_equal(bits(got[j + 1, :length]), np.zeros(length, dtype=np.int64))           # +0.0, not -0.0
        assert flag == j + 1
        assert np.abs(hess[:j + 1, j] - V @ w).max() <= 1e-13 * np.linalg.norm(w)
        assert untouched(got, V, w, j, length)
        assert run_step(ctx, V, w, pitch, j + 2, status=3)[2] == 3
        assert run_step(ctx, V, rng.standard_normal(length), pitch, j + 2, status=3)[2] == 3
        zero = run_step(ctx, V, np.zeros(length), pitch, j + 2)                                      # H v = 0: nothing new either
        assert zero[2] == j + 1 and bits(zero[1][j + 1:j + 2, j])[0] == 0
        assert np.array_equal(bits(zero[0][j + 1, :length]), np.zeros(length, dtype=np.int64))


def test_step_refusals(ctx):
    """Every refusal of the entry by its message; nothing is launched."""
    from pymes_amd.solver.ueg_eom import ARNOLDI_MAX, arnoldi_workspace
    x = ctx.zeros((4096,))
    p = C.c_void_p(x.ptr)
    need = arnoldi_workspace(ctx, 64, 3)
    assert need > 0 and arnoldi_workspace(ctx, 64, 4) > need
    call = lambda *a: ctx.lib.call("pymes_sector_arnoldi_step", ctx.handle, *a)
    size = lambda n: C.byref(C.c_int64(n))
    try:
        for args, message in (((None, 64, 64, 3, p, 4, 1e-10, p, size(need), p), "null pointer: basis"),
                              ((p, 64, 64, 3, None, 4, 1e-10, p, size(need), p), "null pointer: hess"),
                              ((p, 64, 64, 3, p, 4, 1e-10, p, size(need), None), "null pointer: status"),
                              ((p, 64, 64, 3, p, 4, 1e-10, p, None, p), "null pointer: ws_doubles"),
                              ((p, 64, 64, -1, p, 4, 1e-10, p, size(need), p), r"j must lie in \[0, 512\)"),
                              ((p, 64, 64, ARNOLDI_MAX, p, 4, 1e-10, p, size(1 << 20), p), r"j must lie in \[0, 512\)"),
                              ((p, 64, 0, 3, p, 4, 1e-10, p, size(need), p), "bad vector length"),
                              ((p, 32, 64, 3, p, 4, 1e-10, p, size(need), p), "pitch must be a multiple of 32 doubles and at least len"),
                              ((p, 72, 64, 3, p, 4, 1e-10, p, size(need), p), "pitch must be a multiple of 32 doubles and at least len"),
                              ((p, 64, 64, 3, p, 3, 1e-10, p, size(need), p), "ldh is too small for column j"),
                              ((p, 64, 64, 3, p, 4, -1.0, p, size(need), p), "breakdown threshold must be finite and not negative"),
                              ((p, 64, 64, 3, p, 4, np.nan, p, size(need), p), "breakdown threshold must be finite and not negative"),
                              ((p, 64, 64, 3, p, 4, 1e-10, p, size(need - 1), p), r"workspace is too small \(%d doubles are needed\)" % need)):
            with pytest.raises(_lib.PymesError, match="sector_arnoldi_step: .*" + message if "null pointer" not in message else message):
                call(*args)
        ctx.graph_begin()
        try:
            with pytest.raises(_lib.PymesError, match="sector_arnoldi_step while a launch graph is being recorded"):
                call(p, 64, 64, 3, p, 4, 1e-10, p, size(need), p)
        finally:
            ctx.graph_abort()
        assert not x.get().any()
    finally:
        x.free()


# ---- the Arnoldi relation on the device -------------------------------------------------------------------------------------
def flat_to_block(lay, qt, x):
    """(singles element, doubles [shape]) of a flat host vector."""
    return x[0], x[lay.off2:lay.off2 + qt.npos].reshape(qt.shape)


@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("case,kind", [((14, 5), "ea"), ((54, 5), "ip")], ids=str)
def test_arnoldi_relation_on_the_device(ctx, hamiltonians, case, kind, mode):
    """m = 20: H V_m = V_{m+1} Hbar_m with H v_j from the numpy restatement, within 1e-11 max|sigma|; the basis orthonormal to
    subspace.ORTH_TOL.  (14,5) EA has vectors of 350 + 32 elements (two chunks), (54,5) IP of 729 + 32 (three)."""
    from pymes_amd.solver.ueg_eom import SectorSpectralFunction
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians(case, mode)
    T = symmetric(tab, 11, 0.1)
    p = some_targets(tt, kind)[0]
    ladders = ladders_for(ctx, m, tt, mode, [p]) if kind == "ea" else None
    blk = reference_blocks(tab, tt, hi, lists, ladders, [p])
    res = quiet(SectorSpectralFunction(tab.no, max_dim=20, r_epsilon=0.0).solve, eps, ints, tints, T, np.ones(tab.n), [0.0], 0.1,
                keep_basis=True, ladders=ladders, **{kind: [p]})
    kept = res[kind + " basis"]
    try:
        qt = QuasiparticleTables(tt, kind, p)
        Hbar, rows = kept.hessenberg(p), np.array([r.get() for r in kept.rows(p)])
        lay = subspace.FlatLayout(ctx, (1,), qt.shape)
        assert Hbar.shape == (21, 20) and res[kind + " krylov dim"][0] == 20 and not res[kind + " breakdown"][0]
        r1 = rows[:20, 0].copy()
        R = np.array([flat_to_block(lay, qt, x)[1] for x in rows[:20]])
        s1, S, _ = sq.sigma(qt, eps, blk, T, r1, R)
        HV = np.zeros((20, rows.shape[1]))
        HV[:, 0], HV[:, lay.off2:] = s1, S.reshape(20, -1)
        scale = max(np.abs(S).max(), np.abs(s1).max())
        err = np.abs(HV - Hbar.T @ rows).max()
        orth = np.abs(rows @ rows.T - np.eye(21)).max()
        record(f"relation {case} {mode} {kind} target {p} (dim {qt.dim}): max|H V - V Hbar| = {err:.2e}, max|sigma| = {scale:.2e}, "
               f"max|V V^T - 1| = {orth:.2e}")
        assert err <= SIGMA_BOUND * scale
        assert orth <= subspace.ORTH_TOL
    finally:
        kept.close()


# ---- G against the numpy resolvent -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("case", [(14, 2), (14, 5), (54, 5), "twist"], ids=str)
def test_greens_function_against_the_numpy_resolvent(ctx, hamiltonians, case, mode, kind):
    """|G - N_p [(z + s H)^-1]_11| <= N_p ||(z + s H)^-1||_2 (|r| + 1e-11), r the residual of ``solution(target, z)`` taken fresh
    under the numpy restatement's block matrix and the norm from numpy's SVD; the reported residual within 1e-11 (|z| + max|H|)
    of the fresh one; m in {dim + 1, 20, 60}, eta in {0.1, 0.02}, five frequencies across the spectrum; an exact +0.0 at the
    positions outside the space and in the pad of every basis row."""
    from pymes_amd.solver.ueg_eom import SectorSpectralFunction
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians(case, mode)
    T = symmetric(tab, 11, 0.1)
    targets = some_targets(tt, kind)
    ladders = ladders_for(ctx, m, tt, mode, targets) if kind == "ea" else None
    blk = reference_blocks(tab, tt, hi, lists, ladders, targets)
    nk = np.random.default_rng(2).uniform(0.2, 1.8, tab.n)
    s = gf.SIGN[kind]
    for p in targets:
        qt = QuasiparticleTables(tt, kind, p)
        lay = subspace.FlatLayout(ctx, (1,), qt.shape)
        keep = np.concatenate([[0], 1 + np.flatnonzero(qt.inside)])
        flat_keep = np.concatenate([[0], lay.off2 + np.flatnonzero(qt.inside)])
        H = sq.matrix(qt, eps, blk, T)[np.ix_(keep, keep)]
        dim, hmax = qt.dim, np.abs(H).max()
        assert dim == len(keep)
        ev = -s * np.linalg.eigvals(H).real
        omegas = np.linspace(ev.min() - 0.1, ev.max() + 0.1, 5)
        norm = 0.5 * nk[p] if kind == "ip" else 1.0 - 0.5 * nk[p]
        worst = dict(ratio=0.0, res=0.0)
        for eta in (0.1, 0.02):
            z = omegas + 1j * eta
            exact = norm * gf.exact_resolvent(H, kind, z)
            rnorm = np.array([gf.resolvent_norm(H, kind, zz) for zz in z])
            for mm in sorted({min(mm, dim + 1) for mm in (dim + 1, 20, 60)}):
                res = quiet(SectorSpectralFunction(tab.no, max_dim=mm, r_epsilon=0.0).solve, eps, ints, tints, T, nk, omegas, eta,
                            keep_basis=True, ladders=ladders, **{kind: [p]})
                kept = res[kind + " basis"]
                try:
                    k = int(res[kind + " krylov dim"][0])
                    assert k == min(mm, dim) or res[kind + " breakdown"][0]
                    assert res[kind + " norm"][0] == norm
                    assert np.array_equal(res[kind + " A"], -res[kind + " G"].imag / np.pi) and np.array_equal(res["A"], res[kind + " A"])
                    for n, zz in enumerate(z):
                        re, im = kept.solution(p, zz)
                        x = (re.get() + 1j * im.get())[flat_keep]
                        re.free()
                        im.free()
                        e1 = np.zeros(dim, dtype=complex)
                        e1[0] = 1.0
                        fresh = np.linalg.norm(e1 - (zz * x + s * (H @ x)))
                        bound = norm * rnorm[n] * (fresh + SIGMA_BOUND)
                        err = abs(res[kind + " G"][0, n] - exact[n])
                        worst["ratio"] = max(worst["ratio"], err / bound)
                        worst["res"] = max(worst["res"], abs(res[kind + " residuals"][0, n] - fresh))
                        assert err <= bound, (p, mm, eta, zz, err, bound)
                        assert abs(res[kind + " residuals"][0, n] - fresh) <= SIGMA_BOUND * (abs(zz) + hmax)
                    rows = np.array([r.get() for r in kept.rows(p)])
                    outside = np.ones(rows.shape[1], dtype=bool)
                    outside[flat_keep] = False
                    assert np.array_equal(bits(rows[:, outside]), np.zeros((rows.shape[0], outside.sum()), dtype=np.int64))
                finally:
                    kept.close()
        record(f"G {case} {mode} {kind} target {p} (dim {dim}): error / bound at most {worst['ratio']:.2e}, |reported - fresh residual| "
               f"at most {worst['res']:.2e}, max|H| = {hmax:.2f}")


# ---- poles and normalisation on converged amplitudes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def densities(ctx, converged):
    """n(k) of the converged amplitudes of the IP / EA tests and their Lambda, once per (cutoff, mode)."""
    from pymes_amd.solver.ueg_cc import SectorLambda, sector_density
    cache = {}

    def get(cutoff, mode):
        if (cutoff, mode) not in cache:
            m, tab, tt, eps, ints, tints, amps, hi, lists = converged(cutoff, mode)
            lam = quiet(SectorLambda(tab.no, 1e-11).solve, eps, ints, amps)
            assert lam["converged"]
            dens = sector_density(eps, ints, amps, lam["lambda2"])
            cache[cutoff, mode] = (dens, dens.momentum_distribution(), lam["lambda2"])
        return cache[cutoff, mode]
    return get


def numpy_poles(H, kind):
    """numpy's poles of [(z + s H)^-1]_11: (energies -s w_j, residues with those of eigenvalues within 1e-8 summed, singles weights
    |S_1j|^2 / |S_:j|^2 of the right eigenvectors), from eig(H); and the summed residues from eig(H^T)."""
    w, S = np.linalg.eig(H)
    e = -gf.SIGN[kind] * w
    near = np.abs(e[:, None] - e[None, :]) <= 1e-8
    rho = near @ (S[0, :] * np.linalg.inv(S)[:, 0])
    wt, L = np.linalg.eig(H.T)
    et = -gf.SIGN[kind] * wt
    rho_t = (np.abs(e[:, None] - et[None, :]) <= 1e-8) @ (L[0, :] * np.linalg.inv(L)[:, 0])
    return e, rho, np.abs(S[0, :]) ** 2 / (np.abs(S) ** 2).sum(axis=0), rho_t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("cutoff", [2, 3])
def test_poles_against_the_sector_roots_and_numpy_residues(ctx, converged, densities, cutoff, mode, kind):
    """"qp e" equals the SectorIP_EOM_CCD / SectorEA_EOM_CCD root of largest singles weight within the sum of the two Bauer-Fike
    bounds; "qp z" equals numpy's residue of that eigenvalue (residues of eigenvalues within 1e-8 summed) within 100 x the spread
    of numpy against itself (eig(H) against eig(H^T)) plus 1e-12; sum_j Z_j = N_p to 1e-12.

    The Davidson is asked for every root of the block, because the root of largest singles weight need not be among the lowest:
    the k = 0 hole of N = 14 at 19 and 27 plane waves has two poles, Z = 0.52 at -0.87 and 0.48 at -0.11, and the first is the
    upper root of the IP block.  The first statement also needs the pole of largest |Z_j| = |S_1j (S^-1)_j1| and the root of
    largest singles weight r1^2 / |r|^2 to be the same eigenvalue; H-bar is not Hermitian, so these are two numbers.  numpy's
    eigenvectors of the block say whether they are (for every target here they are); if not, "qp e" is held against numpy's
    eigenvalue of largest residue alone, which is asserted for every target, and the root must be one of the poles."""
    from pymes_amd.solver.ueg_eom import SectorEA_EOM_CCD, SectorIP_EOM_CCD, SectorSpectralFunction
    m, tab, tt, eps, ints, tints, amps, hi, lists = converged(cutoff, mode)
    dens, nk, _ = densities(cutoff, mode)
    T = amps.get()
    targets = some_targets(tt, kind)
    ladders = ladders_for(ctx, m, tt, mode, targets) if kind == "ea" else None
    blk = reference_blocks(tab, tt, hi, lists, ladders, targets)
    s = gf.SIGN[kind]
    res = quiet(SectorSpectralFunction(tab.no, max_dim=256, r_epsilon=1e-8).solve, eps, ints, tints, amps, dens, [0.0], 0.1,
                ladders=ladders, **{kind: targets})
    cls = SectorIP_EOM_CCD if kind == "ip" else SectorEA_EOM_CCD
    for n, p in enumerate(targets):
        qt = QuasiparticleTables(tt, kind, p)
        keep = np.concatenate([[0], 1 + np.flatnonzero(qt.inside)])
        H = sq.matrix(qt, eps, blk, T)[np.ix_(keep, keep)]
        kappa = float(np.linalg.cond(np.linalg.eig(H)[1]))
        norm = 0.5 * nk[p] if kind == "ip" else 1.0 - 0.5 * nk[p]
        assert res[kind + " converged"][n] and abs(res[kind + " norm"][n] - norm) == 0.0
        Z, e, pres = res[kind + " pole strengths"][n], res[kind + " poles"][n], res[kind + " pole residuals"][n]
        assert abs(Z.sum() - norm) <= 1e-12
        qe, qz = res[kind + " qp e"][n], res[kind + " qp z"][n]
        assert np.isfinite(qe) and np.isfinite(qz)
        mine = pres[np.argmin(np.abs(e - qe))]
        e_np, rho, weight, rho_t = numpy_poles(H, kind)
        real = np.abs(e_np.imag) <= 1e-12
        jz = np.flatnonzero(real)[np.argmax(np.abs(rho[real]))]
        same = abs(e_np[np.argmax(weight)] - e_np[jz]) <= 1e-8
        spread = abs(rho[jz] - rho_t[jz])
        # (every root of the block, so that the one of largest singles weight is among them: the blocks have at most 29 elements)
        dav = quiet(cls(tab.no, n_roots=qt.dim, r_epsilon=1e-8).solve, eps, ints, tints, amps, [p], ladders=ladders)
        best = int(np.argmax(dav["singles weight"][0]))
        root, rres = -s * dav[kind + " e"][0, best], dav["residuals"][0, best]
        own = kappa * max(mine, 1e-13) * max(1.0, abs(qe)) + 1e-12
        bound = kappa * (max(mine, 1e-13) + max(rres, 1e-13)) * max(1.0, abs(root)) + 1e-12
        record(f"poles c{cutoff} {mode} {kind} target {p} (dim {qt.dim}, Krylov dimension {res[kind + ' krylov dim'][n]}): qp e {qe:.10f}, "
               f"numpy {e_np[jz].real:.10f}, root {root:.10f} (singles weight {dav['singles weight'][0, best]:.4f}, "
               f"{'the same pole' if same else 'ANOTHER pole by numpy'}), diff {abs(qe - root):.2e}, bound {bound:.2e}; "
               f"qp z {qz:.10f}, numpy {norm * rho[jz].real:.10f}, diff {abs(qz - norm * rho[jz].real):.2e}, numpy against itself "
               f"{norm * spread:.2e}; |sum Z - N_p| {abs(Z.sum() - norm):.1e}, N_p {norm:.6f}")
        assert abs(qe - e_np[jz].real) <= own
        assert abs(qz - norm * rho[jz].real) <= 100 * norm * spread + 1e-12
        if same:
            assert abs(qe - root) <= bound
        else:
            near = int(np.argmin(np.abs(e - root)))
            assert abs(e[near] - root) <= kappa * (max(pres[near], 1e-13) + max(rres, 1e-13)) * max(1.0, abs(root)) + 1e-12


@pytest.mark.parametrize("mode", ["coulomb", "tc"])
def test_norm_is_one_minus_the_dense_y(ctx, converged, densities, mode):
    """CCD at (14,3): N_p = 1 - Yoo[p,p] (IP) and 1 - Yvv[p,p] (EA) of DESIGN 8f, Yoo[k,i] = lam2[a,b,i,j] t[a,b,k,j] and Yvv[a,c]
    = lam2[a,b,i,j] t[c,b,i,j] from the to_dense() amplitudes by einsum, to 1e-12 (identity D4: 1 - Yoo[p,p] = n(k_p) / 2)."""
    from pymes_amd.solver.ueg_eom import SectorSpectralFunction
    m, tab, tt, eps, ints, tints, amps, hi, lists = converged(3, mode)
    dens, nk, lam2 = densities(3, mode)
    t, lam = amps.to_dense(), lam2.to_dense()
    yoo, yvv = np.einsum("abij,abkj->ki", lam, t), np.einsum("abij,cbij->ac", lam, t)
    ip_t, ea_t = all_targets(tab, "ip"), some_targets(tt, "ea")
    ladders = ladders_for(ctx, m, tt, mode, ea_t)
    res = quiet(SectorSpectralFunction(tab.no, max_dim=4).solve, eps, ints, tints, amps, dens, [0.0], 0.1, ip=ip_t, ea=ea_t,
                ladders=ladders)
    e_ip = np.abs(res["ip norm"] - (1.0 - np.diag(yoo)[ip_t])).max()
    e_ea = np.abs(res["ea norm"] - (1.0 - np.diag(yvv)[np.array(ea_t) - tab.no])).max()
    record(f"norm c3 {mode}: |N_p - (1 - Yoo)| = {e_ip:.2e}, |N_p - (1 - Yvv)| = {e_ea:.2e}, N_p in [{res['ip norm'].min():.6f}, "
           f"{res['ip norm'].max():.6f}] (IP), [{res['ea norm'].min():.6f}, {res['ea norm'].max():.6f}] (EA)")
    assert e_ip <= 1e-12 and e_ea <= 1e-12
    assert np.array_equal(res["ip norm"], 0.5 * nk[ip_t]) and np.array_equal(res["ea norm"], 1.0 - 0.5 * nk[ea_t])
    assert res["A"].shape == (len(ip_t) + len(ea_t), 1) and np.array_equal(res["targets"], ip_t + ea_t)


# ---- the dense library -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["coulomb", "tc"])
def test_pole_strength_against_the_dense_library(ctx, converged, densities, mode, kind):
    """(14,3): "pole strengths" of root 0 of the dense IP_EOM_CCSD_Dyson / EA_EOM_CCSD_Dyson (t1 = 0) on the dense integrals and
    to_dense() amplitudes against "qp z" of the winning target -- the one whose quasi-particle pole is the lowest root over all
    targets -- within the first-order bound in the two routes' residuals, 4 kappa^2 (res_sector + res_dense) / gap + 1e-10: kappa
    the condition number of the block's eigenvector matrix, gap the distance to the nearest other eigenvalue the singles vector
    reaches, both from numpy.  The dense solver starts from one unit single, so it stays inside one momentum block of the
    degenerate shell; the strength is the same for every orbital of a shell."""
    from oracle import cc_oracle as oc
    from pymes_amd.solver import eom_dyson
    from pymes_amd.solver.ueg_eom import SectorSpectralFunction
    m, tab, tt, eps, ints, tints, amps, hi, lists = converged(3, mode)
    dens, nk, _ = densities(3, mode)
    s, targets = gf.SIGN[kind], all_targets(tab, kind)
    ladders = ladders_for(ctx, m, tt, mode, targets) if kind == "ea" else None
    res = quiet(SectorSpectralFunction(tab.no, max_dim=256, r_epsilon=1e-9).solve, eps, ints, tints, amps, dens, [0.0], 0.1,
                ladders=ladders, **{kind: targets})
    roots = -s * res[kind + " qp e"]                                       # E(N -+ 1) - E(N) of every quasi-particle pole
    assert np.all(np.isfinite(roots))
    win = int(np.argmin(roots))
    p = targets[win]
    e, pres = res[kind + " poles"][win], res[kind + " pole residuals"][win]
    mine = pres[np.argmin(np.abs(e - res[kind + " qp e"][win]))]
    dense = lambda **flags: quiet(m.eval_2b_integrals, sp=0, on_device=True, ctx=ctx, **flags).get()
    V = dense(correlator=m.trunc, is_only_2b=True) + dense(correlator=m.trunc, is_effect_2b=True) if mode == "tc" else dense()
    solver = getattr(eom_dyson, "IP_EOM_CCSD_Dyson" if kind == "ip" else "EA_EOM_CCSD_Dyson")(tab.no, n_roots=1, r_epsilon=1e-9)
    out = quiet(solver.solve, np.diag(eps), oc.split_blocks(tab.no, 0.5 * (V + V.transpose(1, 0, 3, 2))), amps.to_dense(),
                np.zeros((tab.nv, tab.no)))
    theirs = max(float(out["right residual"][0]), float(out["left residual"][0]))
    blk = reference_blocks(tab, tt, hi, lists, ladders, [p])
    w, vr, kappa, reach = block_spectrum(QuasiparticleTables(tt, kind, p), eps, blk, amps.get())
    others = w[reach & (np.abs(w - roots[win]) > 1e-8)]
    gap = np.abs(others - roots[win]).min()
    bound = 4.0 * kappa ** 2 * (mine + theirs) / gap + 1e-10
    diff = abs(out["pole strengths"][0] - res[kind + " qp z"][win])
    record(f"dense c3 {mode} {kind}: winning target {p}, root {roots[win]:.10f}, dense {out['e'][0]:.10f}; qp z {res[kind + ' qp z'][win]:.10f}, "
           f"dense pole strength {out['pole strengths'][0]:.10f}, diff {diff:.2e}, bound {bound:.2e} (kappa {kappa:.2f}, gap {gap:.3f}, "
           f"residuals {mine:.1e} sector, {theirs:.1e} dense)")
    assert abs(out["e"][0] - roots[win]) <= kappa * (max(mine, 1e-13) + theirs) * max(1.0, abs(roots[win])) + 1e-12
    assert diff <= bound


# ---- SectorCCD.solve(spectral=...) ------------------------------------------------------------------------------------------
def test_solve_with_spectral(ctx, converged, monkeypatch):
    """The new keys equal the stand-alone call on the amplitudes and the density the solve returns, to the bit; every old key is
    bit-equal to a solve without ``spectral``; with density=True Lambda is solved once."""
    from pymes_amd.solver import ueg_cc
    from pymes_amd.solver.ueg_cc import SectorCCD, SectorSpectralFunction
    m, tab, tt, eps, ints, tints, _, _, _ = converged(2, "tc")
    ip_t, ea_t = [0, tab.no - 1], [tab.no, tab.n - 1]
    ladders = ladders_for(ctx, m, tt, "tc", ea_t)
    omegas = np.linspace(-2.0, 3.0, 7)
    spec = dict(tints=tints, omegas=omegas, eta=0.1, ip=ip_t, ea=ea_t, ladders=ladders, max_dim=12)
    solves = []
    real = ueg_cc.SectorLambda.solve
    monkeypatch.setattr(ueg_cc.SectorLambda, "solve", lambda self, *a, **k: (solves.append(1), real(self, *a, **k))[1])
    plain = quiet(SectorCCD(tab.no, delta_e=1e-9).solve, eps, ints, density=True)
    assert len(solves) == 1
    out = quiet(SectorCCD(tab.no, delta_e=1e-9).solve, eps, ints, density=True, spectral=spec)
    assert len(solves) == 2                                              # once, shared with density=True
    only = quiet(SectorCCD(tab.no, delta_e=1e-9).solve, eps, ints, spectral=spec)
    assert len(solves) == 3 and "n(k)" not in only and "lambda2" in only
    for key, val in plain.items():
        if isinstance(val, (float, np.floating, np.ndarray)):
            assert np.array_equal(bits(np.asarray(val, dtype=np.float64)), bits(np.asarray(out[key], dtype=np.float64))), key
    assert np.array_equal(bits(plain["t2 amp"].get()), bits(out["t2 amp"].get()))
    assert np.array_equal(bits(plain["lambda2"].get()), bits(out["lambda2"].get()))
    alone = quiet(SectorSpectralFunction(tab.no, max_dim=12).solve, eps, ints, tints, out["t2 amp"], out["density"], omegas, 0.1,
                  ip=ip_t, ea=ea_t, ladders=ladders)
    for key, val in alone.items():
        assert key in out, key
        if isinstance(val, list):
            assert all(np.array_equal(a, b) for a, b in zip(val, out[key])), key
        else:
            assert np.array_equal(val, out[key], equal_nan=True) and np.array_equal(val, only[key], equal_nan=True), key
    assert out["ip G"].shape == (2, 7) and out["ea A"].shape == (2, 7) and out["A"].shape == (4, 7)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_driver_refusals(ctx, hamiltonians):
    from pymes_amd.device import Context
    from pymes_amd.solver.ueg_cc import SectorCCD, sector_density
    from pymes_amd.solver.ueg_eom import ARNOLDI_MAX, SectorSpectralFunction
    from tests.test_gpu_sector_cc import model
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians((14, 2), "tc")
    T, nk = symmetric(tab, 1, 0.1), np.ones(tab.n)
    with pytest.raises(ValueError, match=r"SectorSpectralFunction: max_dim must lie in \[1, %d\]" % ARNOLDI_MAX):
        SectorSpectralFunction(tab.no, max_dim=ARNOLDI_MAX + 1)
    with pytest.raises(ValueError, match=r"SectorSpectralFunction: max_dim must lie in \[1, %d\]" % ARNOLDI_MAX):
        SectorSpectralFunction(tab.no, max_dim=0)
    with pytest.raises(ValueError, match="check_every must be at least 1"):
        SectorSpectralFunction(tab.no, check_every=0)
    solver = SectorSpectralFunction(tab.no)
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: give the targets ip= and / or ea="):
        solver.solve(eps, ints, tints, T, nk, [0.0], 0.1)
    for eta in (0.0, -0.1, np.nan):
        with pytest.raises(ValueError, match="SectorSpectralFunction.solve: eta must be positive"):
            solver.solve(eps, ints, tints, T, nk, [0.0], eta, ip=[0])
    with pytest.raises(ValueError, match=r"n\(k\) must hold one number per orbital \(%d\)" % tab.n):
        solver.solve(eps, ints, tints, T, nk[:-1], [0.0], 0.1, ip=[0])
    other = model(14, 3)
    oints = quiet(other.eval_2b_sectors, other.sector_tables(), ctx=ctx)
    okin = np.array([b.kinetic for b in other.basis_fns[::2]])
    otab = oints.tables
    foreign = sector_density(oints.hf_orbital_energies(okin), oints, symmetric(otab, 1, 0.1), symmetric(otab, 2, 0.1))
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: the density belongs to other tables or another context"):
        solver.solve(eps, ints, tints, T, foreign, [0.0], 0.1, ip=[0])
    ctx2 = Context(1, 1, lib=ctx.lib)
    try:
        ints2 = quiet(m.eval_2b_sectors, tab, ctx=ctx2)
        elsewhere = sector_density(eps, ints2, T, T)
        with pytest.raises(ValueError, match="the density belongs to other tables or another context"):
            solver.solve(eps, ints, tints, T, elsewhere, [0.0], 0.1, ip=[0])
    finally:
        ctx2.close()
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: the tables of the integrals"):
        SectorSpectralFunction(6).solve(eps, ints, tints, T, nk, [0.0], 0.1, ip=[0])
    # what SectorIPEASigma refuses, under this solver's name or its own
    one_sided = quiet(m.eval_2b_triples, tt, ctx=ctx)
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: the triples integrals lack the right-hand families"):
        solver.solve(eps, ints, one_sided, T, nk, [0.0], 0.1, ip=[0])
    with pytest.raises(TypeError, match="SectorSpectralFunction.solve: ints must be SectorIntegrals"):
        solver.solve(eps, np.zeros((19,) * 4), tints, T, nk, [0.0], 0.1, ip=[0])
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: the Fock matrix must be diagonal"):
        solver.solve(np.diag(eps) + 1e-3, ints, tints, T, nk, [0.0], 0.1, ip=[0])
    with pytest.raises(ValueError, match="SectorSpectralFunction.solve: the amplitudes are not exchange-symmetric"):
        solver.solve(eps, ints, tints, np.random.default_rng(0).standard_normal(tab.nnz), nk, [0.0], 0.1, ip=[0])
    with pytest.raises(ValueError, match="the IP target 7 is not an occupied orbital"):
        solver.solve(eps, ints, tints, T, nk, [0.0], 0.1, ip=[7])
    with pytest.raises(ValueError, match="the EA target 6 is not a virtual orbital"):
        solver.solve(eps, ints, tints, T, nk, [0.0], 0.1, ea=[6])
    m5, tab5, tt5, ints5, tints5, eps5, _, _ = hamiltonians((14, 5), "coulomb")
    with pytest.raises(ValueError, match="reads V_abcd at pair momenta.*eval_2b_ladder"):
        solver.solve(eps5, ints5, tints5, symmetric(tab5, 1, 0.1), np.ones(tab5.n), [0.0], 0.1, ea=[7])
    with pytest.raises(ValueError, match="SectorCCD.solve: spectral must be a dictionary with 'tints'"):
        SectorCCD(tab.no).solve(eps, ints, spectral=dict(omegas=[0.0], eta=0.1, ip=[0]))
    with pytest.raises(ValueError, match="SectorCCD.solve: spectral must be a dictionary with 'tints', 'omegas', 'eta'"):
        SectorCCD(tab.no).solve(eps, ints, spectral=dict(tints=tints, ip=[0]))
    ctx.graph_begin()
    try:
        with pytest.raises(RuntimeError, match="the context is recording a launch graph"):
            solver.solve(eps, ints, tints, T, nk, [0.0], 0.1, ip=[0])
    finally:
        ctx.graph_abort()
