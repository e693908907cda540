"""GPU: left EOM-CCSD eigenvectors, transition densities and strengths (pymes_amd/solver/eom_transitions.py; csrc/eom.cpp,
EomSigma::left_build, transition_densities; include/pymes_amd.h, pymes_tdm1).  The stacked left apply against the single one
(the same build as a stack of one, called once per vector), the density kernel against the definitions, the solver against the dense eigenproblem (tests/_transition_reference.py), the
normalisation, the opt-in of CCSD.solve, refusals."""
import contextlib
import ctypes as C
import gc
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import synthetic_case
from pymes_amd import _lib
from tests import _lambda_reference as R
from tests import _transition_reference as X

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    gc.collect()
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _vectors(no, nv, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, no)), R.symd(rng.standard_normal((nv, nv, no, no)))


# ---- 1. the stacked left apply ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(3, 5), (6, 17), (12, 48)])
def test_stacked_left_apply_equals_the_single_one(gpu_lib, no, nv):
    """k = 3 vectors in one call against three k = 1 calls on the same handle: 1e-13 of the largest element per vector; fewer
    GEMM launches than three single builds by at least eight (the (ov)^3 products, the ladder halves and the o v^3 product
    run once); at (12,48) the adjoint identity per vector within the bound of test_adjoint_identity_on_the_device_12_48."""
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    n = no + nv
    rng = np.random.default_rng(100 * no + nv)
    V = 0.05 * rng.standard_normal((n, n, n, n))
    V += V.transpose(1, 0, 3, 2).copy()                            # V_pqrs = V_qpsr only
    f = np.diag(np.concatenate([-1.0 - rng.random(no), 1.0 + rng.random(nv)])) + 0.02 * rng.standard_normal((n, n))
    t2 = 0.02 * R.symd(rng.standard_normal((nv, nv, no, no)))
    ls = [_vectors(no, nv, 20 + z) for z in range(3)]
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        ctx = ints.ctx
        sig = LeftSigma(ctx, f, ctx.array(t2))
        d1, d2 = [ctx.array(l[0]) for l in ls], [ctx.array(l[1]) for l in ls]
        sig.apply_left(d1[0], d2[0], True)                         # (first use: eta1 and the packed V+ / V- are built once)
        ctx.stats(reset=True)
        single = [[x.get() for x in sig.apply_left(d1[0], d2[0], True)]]
        c1 = ctx.stats(reset=True)["gemm_calls"]
        single += [[x.get() for x in sig.apply_left(d1[z], d2[z], True)] for z in (1, 2)]
        ctx.stats(reset=True)
        stacked = [[x.get() for x in pair] for pair in sig.apply_left_many(d1, d2, [True] * 3)]
        c3 = ctx.stats(reset=True)["gemm_calls"]
        print("(%d,%d) GEMM calls: k = 1 %d, k = 3 %d (bound %d)" % (no, nv, c1, c3, 3 * c1 - 8))
        assert c3 <= 3 * c1 - 8
        for z in range(3):
            scale = max(np.abs(single[z][0]).max(), np.abs(single[z][1]).max())
            err = max(np.abs(single[z][0] - stacked[z][0]).max(), np.abs(single[z][1] - stacked[z][1]).max())
            print("   vector %d: max |stacked - single| / max |single| = %.2e" % (z, err / scale))
            assert err <= 1e-13 * scale
            assert np.array_equal(stacked[z][1], stacked[z][1].transpose(1, 0, 3, 2))
        if (no, nv) == (12, 48):
            u1, u2 = _vectors(no, nv, 1)
            s1, s2 = [x.get() for x in sig.apply(ctx.array(u1), ctx.array(u2))]
            for z in range(3):
                a = (ls[z][0] * s1).sum() + (ls[z][1] * s2).sum()
                b = (stacked[z][0] * u1).sum() + (stacked[z][1] * u2).sum()
                print("   vector %d: <l, A u> = %.15e  <A^T l, u> = %.15e  relative %.2e" % (z, a, b, abs(a - b) / abs(a)))
                assert abs(a - b) <= 1e-11 * abs(a)
        sig.close()
    finally:
        ints.ctx.close()


# ---- 2. the density kernel against the definitions -----------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5), (6, 17)])
def test_tdm1_against_the_definitions(gpu_lib, no, nv):
    """gammaL, gammaR by D1 / D2 evaluated with the oracles (at (6,17) recorded in tests/golden by ``python -m
    tests._transition_reference``); random vectors that solve nothing; the tolerance of test_density_against_the_definition."""
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_transitions import device_tdm1
    name, gno, gnv, seed = X.GOLDEN_TDM1
    t1, t2, lam, ls, rs = X.density_inputs(no, nv, seed)
    if (no, nv) == (gno, gnv):
        gold = np.load(os.path.join(GOLD, name))
        ref_l, ref_r = gold["left"], gold["right"]
    else:
        ref_l, ref_r = X.transition_densities_definition(no, t1, t2, lam, ls, rs)
    ctx = Context(no, nv)
    try:
        up = ctx.array
        args = (up(t1), up(t2), up(lam[0]), up(lam[1]), [up(l[0]) for l in ls], [up(l[1]) for l in ls], [up(r[0]) for r in rs],
                [up(r[1]) for r in rs])
        gl, gr, r0 = device_tdm1(ctx, *args)
        gl2, gr2, r02 = device_tdm1(ctx, *args)
    finally:
        ctx.close()
    el, er = np.abs(gl - ref_l).max(), np.abs(gr - ref_r).max()
    e0 = np.abs(r0 + np.array([X.dot(lam, r) for r in rs])).max()
    print(no, nv, "max |gammaL - definition| = %.2e  max |gammaR - definition| = %.2e  max |r0 + <lambda, r>| = %.2e" % (el, er, e0))
    assert el < 1e-10 and er < 1e-10 and e0 < 1e-12
    assert np.array_equal(gl, gl2) and np.array_equal(gr, gr2) and np.array_equal(r0, r02)
    assert np.abs(gl[0] - gl[1]).max() > 1e-3 and np.abs(gr[0] - gr[1]).max() > 1e-3


# ---- 3. the solver against the dense eigenproblem ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hermitian", [True, False], ids=["8-fold", "non-hermitian"])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_solver_against_the_dense_reference(gpu_lib, no, nv, seed, hermitian):
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    ref = X.reference_transitions(no, nv, seed, hermitian)
    fd, Vd, t1, t2 = ref["fd"], ref["Vd"], ref["t1"], ref["t2"]
    eps = 1e-10
    s = EOM_CCSD_Transitions(no, n_excit=3, r_epsilon=eps)
    out = quiet(s.solve, fd, Vd, t2, t1)
    O = X.seeded_operator(no + nv)
    dw = np.abs(out["e"] - ref["w"]).max()
    # both sets of right vectors have unit norm; an eigenvector's sign is arbitrary, and gammaL, gammaR both follow it
    sgn = np.array([np.sign(X.dot((out["r1"][k], out["r2"][k]), ref["rs"][k])) for k in range(3)])[:, None, None]
    dl, dr = np.abs(sgn * out["tdm left"] - ref["gl"]).max(), np.abs(sgn * out["tdm right"] - ref["gr"]).max()
    ds = np.abs(s.strengths(O) - X.strengths(ref["gl"], ref["gr"], O)).max()
    print("(%d,%d) %s: |w - dense| %.2e  |gammaL - dense| %.2e  |gammaR - dense| %.2e  |S - dense| %.2e  biorthogonality %.2e  "
          "passes %s" % (no, nv, "8-fold" if hermitian else "non-hermitian", dw, dl, dr, ds, out["biorthogonality"],
                         out["iterations"]))
    assert out["converged"]
    assert dw < 1e-9
    assert dl < 1e-7 and dr < 1e-7 and ds < 1e-7
    assert out["biorthogonality"] < 1e-9
    assert np.abs(out["r0"] + np.array([X.dot(ref["lam"], (out["r1"][k], out["r2"][k])) for k in range(3)])).max() < 1e-8
    if not hermitian:                      # the left vector is not the right one
        l, r = (out["l1"][0], out["l2"][0]), (out["r1"][0], out["r2"][0])
        assert X.dot(l, r) / np.sqrt(X.dot(l, l) * X.dot(r, r)) < 0.999
    # the residuals under a FRESH sigma handle
    ctx = Context(no, nv)
    try:
        for name in LeftSigma.BLOCKS:
            ctx.set_V_block(name, np.ascontiguousarray(Vd[name]))
        sig = LeftSigma(ctx, fd, ctx.array(t2))
        for k in range(3):
            r, l = (out["r1"][k], out["r2"][k]), (out["l1"][k], out["l2"][k])
            a = [x.get() for x in sig.apply(ctx.array(r[0]), ctx.array(r[1]))]
            b = [x.get() for x in sig.apply_left(ctx.array(l[0]), ctx.array(l[1]))]
            w = out["e"][k]
            rr = np.sqrt(((a[0] - w * r[0]) ** 2).sum() + ((a[1] - w * r[1]) ** 2).sum()) / np.sqrt(X.dot(r, r))
            rl = np.sqrt(((b[0] - w * l[0]) ** 2).sum() + ((b[1] - w * l[1]) ** 2).sum()) / np.sqrt(X.dot(l, l))
            print("   root %d: fresh right residual %.2e (reported %.2e), left %.2e (reported %.2e)"
                  % (k, rr, out["right residual"][k], rl, out["left residual"][k]))
            assert rr < eps and rl < eps
        sig.close()
    finally:
        ctx.close()


# ---- 4. strengths and the normalisation -----------------------------------------------------------------------------------------------
def test_strengths_are_nonnegative_and_do_not_depend_on_the_scaling_4_12(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions, device_tdm1
    no, nv = 4, 12
    # (scale 0.005: at the default 0.02 the first-order doubles of 4 x 12 orbitals have norm 0.56 and the CCSD iteration
    # itself diverges; here |t2| = 0.17 and it converges in some 55 passes)
    f, V = R.random_problem(no, nv, seed=13, eight=True, scale=0.005)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    t2 = 0.5 * R.symd(t2)
    s = EOM_CCSD_Transitions(no, n_excit=3, r_epsilon=1e-9)
    out = quiet(s.solve, fd, Vd, t2, t1)
    assert out["converged"] and out["biorthogonality"] < 1e-9
    mu = np.stack([X.seeded_operator(no + nv, seed=30 + x) for x in range(3)])
    S = np.stack([s.strengths(mu[x]) for x in range(3)])
    print("S_k(mu_x):", S, "oscillator strengths:", s.oscillator_strengths(mu))
    assert S.min() > -1e-9                                          # hermitian: S_k = <0|O|k>^2
    assert np.allclose(s.oscillator_strengths(mu), (2.0 / 3.0) * out["e"] * S.sum(axis=0), rtol=0, atol=1e-14)
    # l_k / c_k and c_k r_k: the same strength (gammaL and gammaR are linear in their vector, r0 included)
    c = np.array([2.0, -0.5, 7.0])
    ctx = Context(no, nv)
    try:
        up = ctx.array
        gl, gr, _ = device_tdm1(ctx, up(t1), up(t2), up(out["lambda1"]), up(out["lambda2"]),
                                [up(out["l1"][k] / c[k]) for k in range(3)], [up(out["l2"][k] / c[k]) for k in range(3)],
                                [up(out["r1"][k] * c[k]) for k in range(3)], [up(out["r2"][k] * c[k]) for k in range(3)])
    finally:
        ctx.close()
    S2 = X.strengths(gl, gr, mu[0])
    print("rescaled:", np.abs(S2 - S[0]).max())
    assert np.abs(S2 - S[0]).max() < 1e-12 * max(1.0, np.abs(S[0]).max())
    # the normalisation itself: vectors handed back un-normalised give other numbers
    assert np.abs(X.strengths(gl * c[:, None, None], gr, mu[0]) - S[0]).max() > 1e-6 * np.abs(S[0]).max()


# ---- 5. the opt-in of CCSD.solve ---------------------------------------------------------------------------------------------------------
def test_ccsd_solve_ee_roots_4_12(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions
    no, nv = 4, 12
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    cc = CCSD(no, delta_e=1e-13)
    res = quiet(cc.solve, f, V, max_iter=300, ee_roots=2)
    for key in ("ee e", "ee tdm left", "ee tdm right", "ee residuals"):
        assert key in res
    assert "rdm1" not in res and "ee e" not in quiet(cc.solve, f, V, max_iter=300)
    Vb = oc.split_blocks(no, V)
    fd, Vd = oc.dressed_fock(no, f, res["t1"], Vb), oc.dressed_V(res["t1"], Vb)
    sep = quiet(EOM_CCSD_Transitions(no, n_excit=2).solve, fd, Vd, res["t2"], res["t1"])
    print("ee e", res["ee e"], "separate", sep["e"], "residuals", res["ee residuals"])
    assert np.abs(res["ee e"] - sep["e"]).max() < 1e-8
    sgn = np.sign(np.einsum("kpq,kpq->k", res["ee tdm left"], sep["tdm left"]))[:, None, None]      # (an eigenvector's sign is arbitrary)
    # (both runs stop at a relative residual of 1e-8, the gaps are of order 0.1: vectors and densities agree to ~1e-7)
    assert np.abs(res["ee tdm left"] - sgn * sep["tdm left"]).max() < 1e-6
    assert np.abs(res["ee tdm right"] - sgn * sep["tdm right"]).max() < 1e-6
    assert max(res["ee residuals"]["right"].max(), res["ee residuals"]["left"].max()) < 1e-8
    # together with the truncations and the density: Lambda once, densities of the correlated space
    res = quiet(cc.solve, f, V, max_iter=300, ee_roots=2, frozen_core=1, fno_nv=8, density=True)
    m = (no - 1) + 8
    assert res["ee tdm left"].shape == (2, m, m) and res["ee tdm right"].shape == (2, m, m) and res["rdm1"].shape == (m, m)
    assert cc.ee_solver.lambda_solver is None and cc.lambda_solver.converged          # (Lambda came from density=True)
    assert np.array_equal(cc.ee_solver.result["lambda1"], res["lambda1"])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.model import synthetic
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions
    E = _lib.PymesError
    no, nv = 4, 12
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    before = _live()
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, ee_roots=2)
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(no, shard_integrals=True).solve(f, V, ee_roots=2)
    with pytest.raises(E, match="too large for the LDS tile"):
        EOM_CCSD_Transitions(100).solve(np.zeros((101, 101)), {}, np.zeros((1, 1, 100, 100)), np.zeros((1, 100)))
    assert _live() == before
    B, eps = synthetic.factors(no, nv, seed=1)
    shard = DeviceIntegrals.from_factors(no, B, shard=(0, 2))
    try:
        held = _live()
        with pytest.raises(E, match="integral sharding"):
            quiet(CCSD(no).solve, np.diag(eps), shard, ee_roots=2)
        assert _live() == held
    finally:
        shard.ctx.close()
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        ctx = ints.ctx
        cc = CCSD(no)
        t1, t2 = np.zeros((nv, no)), np.zeros((nv, nv, no, no))
        dressed = quiet(cc.get_T1_dressed_V, t1, ints, EOM_CCSD_Transitions.BLOCKS)
        ctx.graph_begin()
        try:
            held = _live()
            with pytest.raises(E, match="recording a launch graph"):
                EOM_CCSD_Transitions(no).solve(f, dressed, t2, t1)
            assert _live() == held
        finally:
            ctx.graph_abort()
    finally:
        ints.ctx.close()
    # a complex-conjugate pair among the lowest roots (integrals with V_pqrs = V_qpsr only)
    no, nv = 2, 3
    f, V = R.random_problem(no, nv, seed=11, eight=False)
    t1, t2, fd, Vd, _ = R.converged_state(no, f, V, delta_e=1e-13)
    held = _live()
    with pytest.raises(E, match="complex Ritz value"):
        quiet(EOM_CCSD_Transitions(no, n_excit=3, r_epsilon=1e-8).solve, fd, Vd, 0.5 * R.symd(t2), t1)
    assert _live() == held
