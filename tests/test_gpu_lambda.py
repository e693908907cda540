"""GPU: the adjoint of the EE-EOM-CCSD sigma build, the CCSD Lambda equations and the one-particle density
(pymes_amd/solver/lambda_ccsd.py; csrc/eom.cpp, EomSigma::apply_left / lambda_step, lambda_rdm1; include/pymes_amd.h).  The left
apply against the adjoint term tables (tests/_lambda_reference.py) and against the device's own right apply, the Lambda solve
against a dense solve, one Lambda step from a random lambda against the same tables, the density against its definition and against a finite difference of the device CCSD energy, the
combinations of CCSD.solve, refusals and housekeeping."""
import contextlib
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import synthetic_case
from pymes_amd import _lib
from tests import _eom_branch_cases as BC
from tests import _lambda_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _vectors(no, nv, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, no)), R.symd(rng.standard_normal((nv, nv, no, no)))


@functools.lru_cache(maxsize=None)
def _apply_case(no, nv, hermitian):
    """(f, blocks, t2, l1, l2, the reference's A^T l): integrals with V_pqrs = V_qpsr only (the adjoint of the particle
    ladder is not the ladder) or 8-fold symmetric ones (it is, and runs pair-packed); a non-symmetric Fock matrix."""
    rng = np.random.default_rng(10 * no + nv)
    n = no + nv
    V = 0.1 * rng.standard_normal((n, n, n, n))
    V = R.sym8(V) / 4.0 if hermitian else V + V.transpose(1, 0, 3, 2)
    f = np.diag(np.concatenate([-1.0 - rng.random(no), 1.0 + rng.random(nv)])) + 0.05 * rng.standard_normal((n, n))
    t2 = 0.1 * R.symd(rng.standard_normal((nv, nv, no, no)))
    l1, l2 = _vectors(no, nv, seed=3)
    Vb = oc.split_blocks(no, V)
    return f, Vb, t2, l1, l2, R.left_sigma(no, f, Vb, l1, l2, t2)


# ---- 1. the left apply against the adjoint term tables -----------------------------------------------------------------------------
@pytest.mark.parametrize("hermitian", [False, True], ids=["exchange-only", "hermitian"])
@pytest.mark.parametrize("no,nv", [(3, 5), (4, 12), (6, 17)])
def test_left_apply_against_the_reference(gpu_lib, no, nv, hermitian):
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    f, Vb, t2, l1, l2, (r1, r2) = _apply_case(no, nv, hermitian)
    if not hermitian:
        assert np.abs(Vb["abcd"] - Vb["abcd"].transpose(2, 3, 0, 1)).max() > 1e-3
    o1, o2 = quiet(Lambda_CCSD(no).apply_left, f, Vb, t2, l1, l2)
    scale = max(np.abs(r1).max(), np.abs(r2).max())
    err = max(np.abs(o1 - r1).max(), np.abs(o2 - r2).max())
    print(no, nv, "hermitian" if hermitian else "exchange-only", "max error / max |ref| = %.2e" % (err / scale))
    assert err <= 1e-10 * scale
    assert np.array_equal(o2, o2.transpose(1, 0, 3, 2))          # the result is on the symmetric subspace, exactly


# ---- 2. against the device's own right apply; the right apply is not disturbed -----------------------------------------------------
def test_adjoint_identity_on_the_device_12_48(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    no, nv = 12, 48
    n = no + nv
    rng = np.random.default_rng(8)
    V = 0.05 * rng.standard_normal((n, n, n, n))
    V += V.transpose(1, 0, 3, 2).copy()                            # V_pqrs = V_qpsr only
    f = np.diag(np.concatenate([-1.0 - rng.random(no), 1.0 + rng.random(nv)])) + 0.02 * rng.standard_normal((n, n))
    t2 = 0.02 * R.symd(rng.standard_normal((nv, nv, no, no)))
    (u1, u2), (l1, l2) = _vectors(no, nv, 1), _vectors(no, nv, 2)
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        ctx = ints.ctx
        sig = LeftSigma(ctx, f, ctx.array(t2))
        s1, s2 = [x.get() for x in sig.apply(ctx.array(u1), ctx.array(u2))]
        o1, o2 = [x.get() for x in sig.apply_left(ctx.array(l1), ctx.array(l2))]
        a, b = (l1 * s1).sum() + (l2 * s2).sum(), (o1 * u1).sum() + (o2 * u2).sum()
        print("<l, A u> = %.15e  <A^T l, u> = %.15e  relative %.2e" % (a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-11 * abs(a)
        sig.close()
    finally:
        ints.ctx.close()


def test_right_apply_is_bit_identical_after_a_left_apply(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    no, nv = 4, 12
    f, Vb, t2, l1, l2, _ = _apply_case(no, nv, True)
    u1, u2 = _vectors(no, nv, 5)
    ctx = Context(no, nv)
    try:
        for name in LeftSigma.BLOCKS:
            ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        sig = LeftSigma(ctx, f, ctx.array(t2))
        du1, du2 = ctx.array(u1), ctx.array(u2)
        before = [x.get() for x in sig.apply(du1, du2)]
        left = [x.get() for x in sig.apply_left(ctx.array(l1), ctx.array(l2))]
        after = [x.get() for x in sig.apply(du1, du2)]
        again = [x.get() for x in sig.apply_left(ctx.array(l1), ctx.array(l2))]
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.array_equal(left[0], again[0]) and np.array_equal(left[1], again[1])
        sig.close()
    finally:
        ctx.close()


# ---- 3. the Lambda solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eight", [False, True], ids=["exchange-only", "hermitian"])
def test_lambda_against_the_dense_solve_3_5(gpu_lib, eight):
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    no, nv = 3, 5
    f, V = R.random_problem(no, nv, seed=4, eight=eight)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    ref1, ref2 = R.solve_lambda(no, fd, Vd, t2)
    s = Lambda_CCSD(no, r_epsilon=1e-10)          # (the residual norm bounds the error only up to 1 / the smallest eigenvalue)
    out = quiet(s.solve, fd, Vd, t2)
    err = max(np.abs(out["lambda1"] - ref1).max(), np.abs(out["lambda2"] - ref2).max())
    print("iterations", out["iterations"], "residual norm %.2e" % out["residual norm"], "max |lambda - dense| = %.2e" % err)
    assert out["converged"] and out["residual norm"] < 1e-10
    assert err < 1e-8
    o1, o2 = R.left_sigma(no, fd, Vd, out["lambda1"], out["lambda2"], t2)      # the reported norm is that of the returned vector
    e1, e2 = R.eta(no, fd, Vd)
    assert abs(np.sqrt(((o1 + e1) ** 2).sum() + ((o2 + e2) ** 2).sum()) - out["residual norm"]) < 1e-12


def test_unconverged_solve_returns_the_vector_its_norm_belongs_to(gpu_lib):
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    no, nv = 3, 5
    f, V = R.random_problem(no, nv, seed=4, eight=True)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    s = Lambda_CCSD(no, r_epsilon=1e-10, max_iter=4)
    out = quiet(s.solve, fd, Vd, t2)
    assert not out["converged"] and out["iterations"] == 4 and out["residual norm"] > 1e-10
    o1, o2 = R.left_sigma(no, fd, Vd, out["lambda1"], out["lambda2"], t2)
    e1, e2 = R.eta(no, fd, Vd)
    norm = np.sqrt(((o1 + e1) ** 2).sum() + ((o2 + e2) ** 2).sum())
    print("reported %.6e  recomputed %.6e" % (out["residual norm"], norm))
    assert abs(norm - out["residual norm"]) < 1e-12


STEP_SHIFT = 0.25


@functools.lru_cache(maxsize=None)
def _step_case(no, nv, packed):
    """(f, blocks, t2, lam1, lam2, res1, res2, A^T lam) for one Lambda step from a random exchange-symmetric lambda: 8-fold
    symmetric integrals, a non-symmetric Fock matrix and, unless ``packed``, noise without V_abcd = V_badc on the abcd block only
    (tests/_eom_branch_cases.branch_case), so that the ladder adjoint is the plain product."""
    f, Vb, t2 = BC.branch_case(no, nv, 11, () if packed else ("abcd",))
    l1, l2 = _vectors(no, nv, seed=6)
    s1, s2 = R.left_sigma(no, f, Vb, l1, l2, t2)
    n1, n2 = R.eta(no, f, Vb)
    return f, Vb, t2, l1, l2, s1 + n1, s2 + n2, max(np.abs(s1).max(), np.abs(s2).max())


@pytest.mark.parametrize("packed", [True, False], ids=["packed-ladder", "abcd-broken"])
@pytest.mark.parametrize("no,nv", [(1, 3), (3, 1), (2, 2), (3, 5), (6, 17)])
def test_lambda_step_from_a_random_lambda_against_the_reference(gpu_lib, no, nv, packed):
    """lambda_step feeds a stack of one into the UPDATE form of the assembly: out = lam - res / d, err = -res / d and |res| for
    res = eta + A^T lam against tests/_lambda_reference.py at the bound of test_left_apply_against_the_reference, 1e-10 of the
    largest element of A^T lam.  (1,3): no antisymmetric ladder half (o (o - 1) / 2 = 0); (3,1): v (v - 1) / 2 = 0, and a
    one-element abcd block cannot lose its symmetry; (2,2): the smallest shape with both halves; (6,17): o (o + 1) / 2 = 21 is
    odd, the pad column of the packed operand is live."""
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    f, Vb, t2, l1, l2, r1, r2, scale = _step_case(no, nv, packed)
    eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
    d1 = eps_v[:, None] - eps_o[None, :] - STEP_SHIFT
    d2 = (eps_v[:, None, None, None] + eps_v[None, :, None, None] - eps_o[None, None, :, None] - eps_o[None, None, None, :]
          - STEP_SHIFT)
    ctx = Context(no, nv)
    try:
        for name in LeftSigma.BLOCKS:
            ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        sig = LeftSigma(ctx, f, ctx.array(t2))
        assert sig.v_sym == BC.expected_flags(no, Vb, t2)[0] == (packed or nv == 1)
        a1, a2 = ctx.array(l1), ctx.array(l2)
        o1, e1 = [ctx.array(np.full(l1.shape, np.nan)) for _ in range(2)]
        o2, e2 = [ctx.array(np.full(l2.shape, np.nan)) for _ in range(2)]
        norm = sig.lambda_step((a1, a2), eps_o, eps_v, STEP_SHIFT, (o1, o2), (e1, e2))
        got = [x.get() for x in (o1, o2, e1, e2)]
        sig.close()
    finally:
        ctx.close()
    want = (l1 - r1 / d1, l2 - r2 / d2, -r1 / d1, -r2 / d2)
    errs = [np.abs(g - w).max() for g, w in zip(got, want)]
    nerr = abs(norm - np.sqrt((r1 ** 2).sum() + (r2 ** 2).sum()))
    print(no, nv, "packed" if packed else "abcd broken", "out1 %.2e out2 %.2e err1 %.2e err2 %.2e norm %.2e, all / max |A^T lam|" % tuple(
        x / scale for x in errs + [nerr]))
    assert all(np.all(np.isfinite(g)) for g in got)
    assert max(errs) <= 1e-10 * scale and nerr <= 1e-10 * scale


@functools.lru_cache(maxsize=None)
def _water_sized_state():
    """A converged device CCSD state at (5,19), synthetic 8-fold integrals; dressed Fock matrix and blocks by the oracle."""
    from pymes_amd.model import synthetic
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 5, 19
    B, eps = synthetic.factors(no, nv, seed=2)
    f, V = np.diag(eps), synthetic.dense_eri(B)
    res = quiet(CCSD(no, delta_e=1e-13).solve, f, V, max_iter=200)
    Vb = oc.split_blocks(no, V)
    return no, f, V, res, oc.dressed_fock(no, f, res["t1"], Vb), oc.dressed_V(res["t1"], Vb)


def test_lambda_converges_5_19_and_two_solves_give_identical_bits(gpu_lib):
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    no, f, V, res, fd, Vd = _water_sized_state()
    runs = []
    for _ in range(2):
        s = Lambda_CCSD(no)
        out = quiet(s.solve, fd, Vd, res["t2"])
        runs.append((out, np.array(s.history), s.rdm1(res["t1"])))
    out = runs[0][0]
    print("iterations", out["iterations"], "residual norm %.2e" % out["residual norm"])
    assert out["converged"] and out["residual norm"] < 1e-8 and out["iterations"] < 100
    assert np.array_equal(runs[0][1], runs[1][1])
    for key in ("lambda1", "lambda2"):
        assert np.array_equal(runs[0][0][key], runs[1][0][key])
    assert np.array_equal(runs[0][2], runs[1][2])


# ---- 4. the density --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(3, 5), (6, 17)])
def test_density_against_the_definition(gpu_lib, no, nv):
    """gamma = dL/df by the reference (n^2 evaluations of the Lagrangian with the oracle's residuals; at (6,17) recorded in
    tests/golden by ``python -m tests._lambda_reference``)."""
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import device_rdm1
    name, gno, gnv, seed = R.GOLDEN_RDM1
    t1, t2, l1, l2 = R.density_inputs(no, nv, seed)
    ref = np.load(os.path.join(GOLD, name))["rdm1"] if (no, nv) == (gno, gnv) else R.rdm1(no, t1, t2, l1, l2)
    ctx = Context(no, nv)
    try:
        g = device_rdm1(ctx, ctx.array(t1), ctx.array(t2), ctx.array(l1), ctx.array(l2))
        g0 = device_rdm1(ctx, ctx.array(t1), ctx.array(t2), ctx.array(l1), ctx.array(l2), ref=0.0)
    finally:
        ctx.close()
    err = np.abs(g - ref).max()
    print(no, nv, "max |gamma - reference| = %.2e" % err, "trace - 2 no = %.2e" % (np.trace(g) - 2 * no))
    assert err < 1e-10
    assert abs(np.trace(g) - 2 * no) < 1e-12 and abs(np.trace(g0)) < 1e-12
    assert np.abs(g - g.T).max() > 1e-3               # not symmetric, and not symmetrised


def test_ccsd_density_against_the_energy_derivative_4_12(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 4, 12
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    O = np.random.default_rng(5).standard_normal(f.shape)
    O = 0.5 * (O + O.T)
    h = 1e-4
    cc = CCSD(no, delta_e=1e-13)
    res = quiet(cc.solve, f, V, max_iter=300, density=True)
    for key in ("lambda1", "lambda2", "rdm1", "natural occupations"):
        assert key in res
    assert cc.lambda_solver.converged
    val = cc.lambda_solver.expectation(O)
    ep = quiet(cc.solve, f + h * O, V, max_iter=300)["ccsd e"]
    em = quiet(cc.solve, f - h * O, V, max_iter=300)["ccsd e"]
    fd = (ep - em) / (2.0 * h)
    print("finite difference %.12e  sum gamma O %.12e  difference %.2e" % (fd, val, abs(fd - val)))
    assert abs(fd - val) < 1e-6
    assert res["rdm1"].shape == (no + nv, no + nv) and abs(np.trace(res["rdm1"]) - 2 * no) < 1e-10
    occ = res["natural occupations"]
    assert occ.shape == (no + nv,) and np.all(np.diff(occ) <= 0) and abs(occ.sum() - 2 * no) < 1e-10
    assert "rdm1" not in quiet(cc.solve, f, V, max_iter=300)


# ---- 5. combinations and refusals ------------------------------------------------------------------------------------------------------
def test_ccsd_solve_density_with_truncation_triples_and_roots(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    no, f, V, _, _, _ = _water_sized_state()
    nv = f.shape[0] - no
    cc = CCSD(no, delta_e=1e-10)
    res = quiet(cc.solve, f, V, max_iter=200, density=True, frozen_core=1, fno_nv=nv - 4, triples=True, ip_roots=1, ea_roots=1,
                lambda_r_epsilon=1e-7)
    m = (no - 1) + (nv - 4)
    assert res["fno nv"] == nv - 4 and "(t) e" in res and len(res["ip e"]) == 1 and len(res["ea e"]) == 1
    assert res["rdm1"].shape == (m, m) and res["lambda1"].shape == (nv - 4, no - 1)
    assert res["lambda2"].shape == (nv - 4, nv - 4, no - 1, no - 1) and res["natural occupations"].shape == (m,)
    assert abs(np.trace(res["rdm1"]) - 2 * (no - 1)) < 1e-10
    assert cc.lambda_solver.r_epsilon == 1e-7 and cc.lambda_solver.residual_norm < 1e-7


def test_refusals_by_name(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.model import synthetic
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    no, nv = 4, 12
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, density=True)
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(no, shard_integrals=True).solve(f, V, density=True)
    B, eps = synthetic.factors(no, nv, seed=1)
    shard = DeviceIntegrals.from_factors(no, B, shard=(0, 2))
    try:
        before = _live()
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            quiet(CCSD(no).solve, np.diag(eps), shard, density=True)
        assert _live() == before
        cc = CCSD(no)
        t1 = np.zeros((nv, no))
        dressed = quiet(cc.get_T1_dressed_V, t1, shard, ("ijab", "iabj", "iajb", "ijka", "ijak", "iabc", "iajk", "klij"))
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            quiet(Lambda_CCSD(no).solve, np.diag(eps), dressed, np.zeros((nv, nv, no, no)))
    finally:
        shard.ctx.close()


# ---- 6. housekeeping ---------------------------------------------------------------------------------------------------------------------
def test_handle_refusals_and_allocations(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD, LeftSigma
    E = _lib.PymesError
    no, nv = 3, 5
    f, Vb, t2, l1, l2, _ = _apply_case(no, nv, False)
    before = _live()
    ctx = Context(no, nv)
    try:
        for name in LeftSigma.BLOCKS:
            if name != "iabc":
                ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        d2 = ctx.array(t2)
        held = _live()
        with pytest.raises(E, match="'iabc'"):
            LeftSigma(ctx, f, d2)
        ctx.trim()                       # (the hoist of the right build had begun: its buffers are in the context's pool)
        assert _live() == held
        ctx.set_V_block("iabc", np.ascontiguousarray(Vb["iabc"]))
        sig = LeftSigma(ctx, f, d2)
        a1, a2 = ctx.array(l1), ctx.array(l2)
        o1, o2 = ctx.empty(a1.shape), ctx.empty(a2.shape)
        e1, e2 = ctx.empty(a1.shape), ctx.empty(a2.shape)
        eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
        first = [x.get() for x in sig.apply_left(a1, a2)]
        bad = ctx.array(l2 + 1e-3 * np.random.default_rng(0).standard_normal(l2.shape))
        held = _live()
        with pytest.raises(E, match="exchange symmetry"):
            sig.apply_left_many([a1], [bad], out1=[o1], out2=[o2])
        with pytest.raises(E, match="exchange symmetry"):
            sig.lambda_step((a1, bad), eps_o, eps_v, 0.0, (o1, o2), (e1, e2))
        with pytest.raises(E, match="aliases"):
            sig.apply_left_many([a1], [a2], out1=[a1], out2=[o2])
        assert _live() == held
        assert ctx.graphs_supported()
        ctx.graph_begin()
        try:
            held = _live()
            with pytest.raises(E, match="launch graph"):
                sig.apply_left_many([a1], [a2], out1=[o1], out2=[o2])
            with pytest.raises(E, match="launch graph"):
                sig.lambda_step((a1, a2), eps_o, eps_v, 0.0, (o1, o2), (e1, e2))
            assert _live() == held
        finally:
            ctx.graph_abort()
        again = [x.get() for x in sig.apply_left(a1, a2)]
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        # one Lambda step against its definition: out = lam - (eta + A^T lam) / d, err = out - lam, the norm of eta + A^T lam
        norm = sig.lambda_step((a1, a2), eps_o, eps_v, 0.25, (o1, o2), (e1, e2))
        r1, r2 = R.left_sigma(no, f, Vb, l1, l2, t2)
        n1, n2 = R.eta(no, f, Vb)
        r1, r2 = r1 + n1, r2 + n2
        d1 = eps_v[:, None] - eps_o[None, :] - 0.25
        d2_ = (eps_v[:, None, None, None] + eps_v[None, :, None, None] - eps_o[None, None, :, None] - eps_o[None, None, None, :]
               - 0.25)
        scale = max(np.abs(r1).max(), np.abs(r2).max())
        assert abs(norm - np.sqrt((r1 ** 2).sum() + (r2 ** 2).sum())) < 1e-10 * scale
        assert np.abs(e1.get() + r1 / d1).max() < 1e-10 * scale and np.abs(e2.get() + r2 / d2_).max() < 1e-10 * scale
        assert np.abs(o1.get() - (l1 - r1 / d1)).max() < 1e-10 * scale and np.abs(o2.get() - (l2 - r2 / d2_)).max() < 1e-10 * scale
        sig.close()
        with pytest.raises(E, match="destroyed"):
            sig.apply_left(a1, a2)
        sig = LeftSigma(ctx, f, d2)
    finally:
        ctx.close()
    with pytest.raises(E, match="destroyed"):
        sig.apply_left(a1, a2)
    sig.close()
    del a1, a2, o1, o2, e1, e2, bad, d2
    assert _live() == before
    with pytest.raises(KeyError, match="iabc"):
        quiet(Lambda_CCSD(no).solve, f, {k: v for k, v in Vb.items() if k != "iabc"}, t2)
    assert _live() == before
