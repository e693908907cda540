"""GPU: EOM-CCSD linear response functions (pymes_amd/solver/response.py; csrc/eom.cpp, response_vectors / response_dots /
response_update; include/pymes_amd.h, pymes_response_vectors).  The property vectors against their definitions and the written-out
numpy formulas, the adjoint identities on the device, the batched solver against the dense resolvent and the exact two-electron
value (tests/_response_reference.py), the solver's mechanics at (12,48), the opt-in of CCSD.solve, refusals."""
import contextlib
import ctypes as C
import gc
import io

import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from tests import _response_reference as P
from tests import _transition_reference as X

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    gc.collect()
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _device_vectors(ctx, t1, t2, lam, ops):
    from pymes_amd.solver.response import device_response_vectors
    up = ctx.array
    x1, x2, e1, e2, g0 = device_response_vectors(ctx, up(t1), up(t2), up(lam[0]), up(lam[1]), ops)
    return [a.get() for a in x1], [a.get() for a in x2], [a.get() for a in e1], [a.get() for a in e2], g0


# ---- 1. the property vectors -------------------------------------------------------------------------------------------------------------
# (6,17): o^2 <= 256 and v o <= 256, one trip of every loop; (17,3): the smallest o with o^2 > 256 (two trips over the tile, two of
# the oo part of g0); (2,260): the smallest nv > 256 (v o and v^2 past one trip in the singles block); k = 9 at (3,5): a second
# chunk of operators (eight accumulators per thread) with one operator in it
@pytest.mark.parametrize("no,nv,k", [(2, 3, 3), (3, 5, 3), (3, 5, 9), (6, 17, 3), (17, 3, 3), (2, 260, 3)])
def test_response_vectors_against_the_definitions(gpu_lib, no, nv, k):
    """xi, eta of k random non-symmetric operators: by definition at (2,3) and (3,5), against the written-out numpy formulas
    (themselves checked against the definitions to 1e-13 on the CPU) at the larger shapes; the tolerance of
    test_tdm1_against_the_definitions.  Two identical calls are bit-identical, a k = 3 call equals three k = 1 calls to 1e-13 of
    the largest element, xi2 and eta2 are exchange-symmetric to the bit."""
    from pymes_amd.device import Context
    t1, t2, lam, _, _ = X.density_inputs(no, nv, 9)
    ops = np.random.default_rng(40 + no).standard_normal((k, no + nv, no + nv))
    by_definition = (no, nv, k) in ((2, 3, 3), (3, 5, 3))
    ref = [((P.xi_definition(no, t1, t2, O), P.eta_definition(no, t1, t2, lam, O)) if by_definition else
            (P.xi_terms(no, t1, t2, O), P.eta_terms(no, t1, t2, lam, O))) for O in ops]
    ctx = Context(no, nv)
    try:
        got = _device_vectors(ctx, t1, t2, lam, ops)
        again = _device_vectors(ctx, t1, t2, lam, ops)
        ones = [_device_vectors(ctx, t1, t2, lam, ops[z:z + 1]) for z in range(3)]
    finally:
        ctx.close()
    for z in range(k):
        parts = (got[0][z], got[1][z], got[2][z], got[3][z])
        want = (ref[z][0][0], ref[z][0][1], ref[z][1][0], ref[z][1][1])
        errs = [np.abs(a - b).max() for a, b in zip(parts, want)]
        g0 = P.dot(lam, ref[z][0])
        print("(%d,%d) operator %d: max |xi1|, |xi2|, |eta1|, |eta2| errors %s  |g0 - <lambda, xi>| %.2e"
              % (no, nv, z, " ".join("%.2e" % e for e in errs), abs(got[4][z] - g0)))
        assert max(errs) < 1e-10 and abs(got[4][z] - g0) < 1e-10
        assert np.array_equal(parts[1], parts[1].transpose(1, 0, 3, 2)) and np.array_equal(parts[3], parts[3].transpose(1, 0, 3, 2))
    for part in range(4):
        for z in range(k):
            assert np.array_equal(got[part][z], again[part][z])
        for z in range(3):
            scale = np.abs(got[part][z]).max()
            assert np.abs(got[part][z] - ones[z][part][0]).max() <= 1e-13 * scale
    assert np.array_equal(got[4], again[4])
    assert np.abs(got[1][0] - got[1][1]).max() > 1e-3 and np.abs(got[3][0] - got[3][1]).max() > 1e-3


def test_response_vectors_with_a_full_pointer_table(gpu_lib):
    """k = 64 at (2,3): the whole by-value pointer table, eight full chunks of eight operators; k = 65: the Python side's second
    call with one operator.  Every operator against the definitions at the tolerance of
    test_response_vectors_against_the_definitions; operator 64 of the k = 65 call is, to the bit, a k = 1 call of its own; xi2 and
    eta2 are exchange-symmetric to the bit.  The 65 operators are seeded combinations of eight dense random ones: xi and eta are
    linear in O (test_definitions_are_linear_in_the_operator), so eight evaluations of the definitions give all 65 references."""
    from pymes_amd.device import Context
    from pymes_amd.solver.response import OPS_MAX
    no, nv = 2, 3
    assert OPS_MAX == 64
    t1, t2, lam, _, _ = X.density_inputs(no, nv, 9)
    rng = np.random.default_rng(64)
    basis, coef = rng.standard_normal((8, no + nv, no + nv)), rng.standard_normal((65, 8))
    ops = np.einsum("zb,bpq->zpq", coef, basis)
    defs = [P.xi_definition(no, t1, t2, O) + P.eta_definition(no, t1, t2, lam, O) for O in basis]
    mix = lambda z, part: sum(c * d[part] for c, d in zip(coef[z], defs))
    ref = [((mix(z, 0), mix(z, 1)), (mix(z, 2), mix(z, 3))) for z in range(65)]
    ctx = Context(no, nv)
    try:
        full = _device_vectors(ctx, t1, t2, lam, ops[:64])
        more = _device_vectors(ctx, t1, t2, lam, ops)
        last = _device_vectors(ctx, t1, t2, lam, ops[64:])
    finally:
        ctx.close()
    for k, got in ((64, full), (65, more)):
        worst = 0.0
        for z in range(k):
            parts = (got[0][z], got[1][z], got[2][z], got[3][z])
            want = (ref[z][0][0], ref[z][0][1], ref[z][1][0], ref[z][1][1])
            errs = [np.abs(a - b).max() for a, b in zip(parts, want)] + [abs(got[4][z] - P.dot(lam, ref[z][0]))]
            worst = max(worst, max(errs))
            assert max(errs) < 1e-10, (k, z, errs)
            assert np.array_equal(parts[1], parts[1].transpose(1, 0, 3, 2)) and np.array_equal(parts[3], parts[3].transpose(1, 0, 3, 2))
        print("k = %d: largest error of xi1, xi2, eta1, eta2, g0 over all operators %.2e" % (k, worst))
    for part in range(4):
        assert np.array_equal(more[part][64], last[part][0])
        for z in range(64):
            assert np.array_equal(more[part][z], full[part][z])
    assert more[4][64] == last[4][0] and np.array_equal(more[4][:64], full[4])


# ---- 2. the adjoint identities on the device ---------------------------------------------------------------------------------------------
def test_adjoint_identities_on_the_device_12_48(gpu_lib):
    """<eta(O), r> = sum gammaR(r) O and <l, xi(O)> = sum gammaL(l) O with the densities of ``device_tdm1``, for random
    exchange-symmetric vectors that solve nothing: within the bound of test_adjoint_identity_on_the_device_12_48."""
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_transitions import device_tdm1
    no, nv, k = 12, 48, 3
    t1, t2, lam, ls, rs = X.density_inputs(no, nv, 9, k)
    ops = np.random.default_rng(3).standard_normal((k, no + nv, no + nv))
    ctx = Context(no, nv)
    try:
        up = ctx.array
        gl, gr, _ = device_tdm1(ctx, up(t1), up(t2), up(lam[0]), up(lam[1]), [up(l[0]) for l in ls], [up(l[1]) for l in ls],
                                [up(r[0]) for r in rs], [up(r[1]) for r in rs])
        x1, x2, e1, e2, _ = _device_vectors(ctx, t1, t2, lam, ops)
    finally:
        ctx.close()
    for z in range(k):
        for v in range(k):
            a, b = P.dot((e1[z], e2[z]), rs[v]), (gr[v] * ops[z]).sum()
            c, d = P.dot(ls[v], (x1[z], x2[z])), (gl[v] * ops[z]).sum()
            print("operator %d vector %d: <eta, r> %.15e  gammaR.O %.15e (%.1e)   <l, xi> %.15e  gammaL.O %.15e (%.1e)"
                  % (z, v, a, b, abs(a - b) / abs(b), c, d, abs(c - d) / abs(d)))
            assert abs(a - b) <= 1e-11 * abs(b) and abs(c - d) <= 1e-11 * abs(d)


# ---- 3. / 4. the solver against the dense resolvent and the exact two-electron value ------------------------------------------------------
def _solve_three(ref, r_eps, **solver_options):
    """(values [3,m,m] at the three frequencies of the issue, results, solvers): z = 0 and 0.4 w1 in one real solve, 1.3 w1 + 0.05i
    in a complex one."""
    from pymes_amd.solver.response import EOM_CCSD_Response
    no = ref["t1"].shape[1]
    zs = P.frequencies(ref["w1"])
    outs, solvers, vals = [], [], []
    for omegas, gamma in (([zs[0], zs[1]], 0.0), ([zs[2].real], zs[2].imag)):
        s = EOM_CCSD_Response(no, r_epsilon=r_eps)
        s.history = 32                  # (full GCR at (2,3), dimension 27; the z inside the spectrum stalls a short window)
        for key, val in solver_options.items():
            setattr(s, key, val)
        out = quiet(s.solve, ref["fd"], ref["Vd"], ref["t2"], ref["t1"], ref["ops"], omegas, gamma=gamma, lam=ref.get("use lam"))
        outs.append(out)
        solvers.append(s)
        vals += list(out["response"])
    return zs, vals, outs, solvers


def _tolerance(dense, z, r_eps, X_, Y_):
    """10 r_epsilon sum |eta| |xi| |(z - A)^-1|_2 for the value <<X;Y>>_z: its two terms."""
    return 10.0 * r_eps * (P.norm(dense.eta[X_]) * P.norm(dense.xi[Y_]) * dense.resolvent_norm(z)
                           + P.norm(dense.eta[Y_]) * P.norm(dense.xi[X_]) * dense.resolvent_norm(-z))


@pytest.mark.parametrize("hermitian", [True, False], ids=["8-fold", "non-hermitian"])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_solver_against_the_dense_resolvent(gpu_lib, no, nv, seed, hermitian):
    """Two non-symmetric operators, z = 0, 0.4 w1, 1.3 w1 + 0.05i, r_epsilon = 1e-10, Lambda of the dense reference: every value
    of <<X;Y>>_z within 10 r_epsilon sum |eta| |xi| |(z - A)^-1|_2 of the dense resolvent; every system converged, every reported
    (fresh) residual at r_epsilon."""
    ref = dict(P.reference_problem(no, nv, seed, hermitian, 2))
    ref["use lam"] = ref["lam"]
    r_eps = 1e-10
    zs, vals, outs, solvers = _solve_three(ref, r_eps)
    dense = ref["dense"]
    for z, val in zip(zs, vals):
        want = dense.response(z)
        for X_ in range(2):
            for Y_ in range(2):
                tol = _tolerance(dense, z, r_eps, X_, Y_)
                err = abs(val[X_, Y_] - want[X_, Y_])
                print("(%d,%d) %s z = %s <<%d;%d>> = %s  dense %s  |difference| %.2e  tolerance %.2e"
                      % (no, nv, "8-fold" if hermitian else "non-hermitian", z, X_, Y_, val[X_, Y_], want[X_, Y_], err, tol))
                assert err <= tol
    for out, s in zip(outs, solvers):
        print("   sweeps %d, iterations %s, residuals %s" % (out["sweeps"], out["iterations"].ravel(), out["residuals"].ravel()))
        assert out["converged"] and out["converged systems"].all()
        assert out["residuals"].max() <= s.DRIFT * r_eps
        assert out["response"].dtype == (np.complex128 if out["gamma"] else np.float64)
        assert np.array_equal(out["polarizability"], -out["response"])


def test_two_electron_polarizability_against_fci(gpu_lib):
    """(no, nv) = (1, 4): the polarizability of a symmetric operator equals the exact singlet-state sum, at the tolerance of the
    dense comparison; Lambda is solved on the solver's own handle; the damped spectral density is positive."""
    ref = dict(P.reference_problem(1, 4, 3, True, 1, 0.05, True))
    r_eps = 1e-10
    zs, vals, outs, solvers = _solve_three(ref, r_eps, lambda_r_epsilon=1e-12)
    for z, val in zip(zs, vals):
        want = P.two_electron_polarizability(ref["f"], ref["V"], ref["ops"][0], z)
        tol = _tolerance(ref["dense"], z, r_eps, 0, 0)
        print("z = %s: polarizability %s  FCI %s  |difference| %.2e  tolerance %.2e" % (z, -val[0, 0], want, abs(-val[0, 0] - want), tol))
        assert abs(-val[0, 0] - want) <= tol
    assert all(out["converged"] for out in outs) and solvers[0].lambda_solver.converged
    assert np.abs(outs[0]["lambda2"] - ref["lam"][1]).max() < 1e-9
    assert solvers[1].spectral_density()[0] > 0.0 and solvers[0].spectral_density()[0] == 0.0
    assert np.allclose(solvers[1].isotropic(), -vals[2][0, 0])


# ---- 5. the solver's mechanics at (12,48) --------------------------------------------------------------------------------------------------
def test_batched_solver_12_48(gpu_lib):
    """Three operators, two frequencies below the HF gap, gamma = 0.05: twelve complex systems in one solve, on the converged CCSD
    state of the synthetic factors; Lambda is random (it enters eta alone).  Every reported residual is confirmed with a
    fresh handle; the batched solutions agree with per-system solves in the metric that needs no resolvent norm —
    |(z - A)(x_batched - x_single)| <= |res_batched| + |res_single| <= 2.02 r_epsilon |xi| — and in the values within
    10 r_epsilon sum |eta| |xi| rho, rho = 2 / min |z - d| (the resolvent norm of the diagonal, doubled for the off-diagonal
    part of these weakly correlated integrals); one apply, one dots and one update call per sweep (two synchronisations); allocations return
    to the baseline."""
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.model import synthetic
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    from pymes_amd.solver.response import EOM_CCSD_Response
    no, nv, m = 12, 48, 3
    n = no + nv
    B, eps = synthetic.factors(no, nv, seed=1)
    f = np.diag(eps)
    gap = float(eps[no] - eps[no - 1])
    _, _, lam, _, _ = X.density_inputs(no, nv, 9)
    ops = np.random.default_rng(100 * no + nv).standard_normal((m, n, n))
    omegas, gamma, r_eps = [0.1 * gap, 0.4 * gap], 0.05, 1e-8
    before = _live()
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        ctx = ints.ctx
        cc = CCSD(no, delta_e=1e-10)
        res = quiet(cc.solve, f, ints, device_amplitudes=True)
        t1, t2 = res["t1"], res["t2"]
        fd = cc.get_T1_dressed_fock(f, t1, ints)
        dressed = cc.get_T1_dressed_V(t1, ints, EOM_CCSD_Response.BLOCKS)
        s = EOM_CCSD_Response(no, r_epsilon=r_eps)
        s.keep_solutions = True
        out = quiet(s.solve, fd, dressed, t2, t1, ops, omegas, gamma=gamma, lam=lam)
        held = _live()                   # (after the first solve: the engine's arena has its size; six more solves must not add to it)
        sweeps = out["sweeps"]
        print("sweeps %d, calls %s, iterations %s" % (sweeps, s.calls, out["iterations"].ravel()))
        assert out["converged"] and s.calls == {"apply": sweeps + 1, "dots": sweeps, "update": sweeps}      # (+1: the certificate)
        assert out["response"].shape == (2, m, m) and out["response"].dtype == np.complex128
        singles = {}
        for w in range(2):
            for o in range(m):
                one = EOM_CCSD_Response(no, r_epsilon=r_eps)
                one.keep_solutions = True
                singles[(w, o)] = quiet(one.solve, fd, dressed, t2, t1, ops[o:o + 1], omegas[w:w + 1], gamma=gamma, lam=lam)
        assert _live() == held
        # fresh handle: residuals of the batched solutions, and (z - A) applied to the difference to the per-system ones
        sig = LeftSigma(ctx, fd, t2, True)
        d1, d2 = ctx.zeros((nv, no)), ctx.zeros((nv, nv, no, no))
        ctx.lib.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(np.ascontiguousarray(fd)), C.c_void_p(sig.T.ptr), 1,
                     C.c_void_p(d1.ptr), C.c_void_p(d2.ptr))
        diag = np.concatenate([d1.get().ravel(), d2.get().ravel()])

        def apply(x):
            parts = [[y.get() for y in sig.apply(ctx.array(np.ascontiguousarray(p(x[0]))), ctx.array(np.ascontiguousarray(p(x[1]))),
                                                 True)] for p in (np.real, np.imag)]
            return parts[0][0] + 1j * parts[1][0], parts[0][1] + 1j * parts[1][1]
        cnorm = lambda v: float(np.sqrt((np.abs(v[0]) ** 2).sum() + (np.abs(v[1]) ** 2).sum()))
        at = 0
        for w in range(2):
            for o in range(m):
                for sg, sign in enumerate((1.0, -1.0)):
                    z = sign * complex(omegas[w], gamma)
                    x, xs = out["x"][at], singles[(w, o)]["x"][sg]
                    ax = apply(x)
                    res = (out["xi"][o][0] - z * x[0] + ax[0], out["xi"][o][1] - z * x[1] + ax[1])
                    rel = cnorm(res) / P.norm(out["xi"][o])
                    dx = (x[0] - xs[0], x[1] - xs[1])
                    adx = apply(dx)
                    gap = cnorm((z * dx[0] - adx[0], z * dx[1] - adx[1])) / P.norm(out["xi"][o])
                    print("   system (w %d, operator %d, %+d z): fresh residual %.3e (reported %.3e)  |(z - A) dx| / |xi| %.2e"
                          % (w, o, int(sign), rel, out["residuals"][w, o, sg], gap))
                    assert rel <= s.DRIFT * r_eps and abs(rel - out["residuals"][w, o, sg]) <= 1e-3 * r_eps
                    assert gap <= 2.0 * s.DRIFT * r_eps
                    at += 1
                rho = [2.0 / np.abs(sign * complex(omegas[w], gamma) - diag).min() for sign in (1.0, -1.0)]
                tol = 10.0 * r_eps * P.norm(out["eta"][o]) * P.norm(out["xi"][o]) * (rho[0] + rho[1])
                diff = abs(out["response"][w, o, o] - singles[(w, o)]["response"][0, 0, 0])
                print("   <<%d;%d>> batched - single: %.2e (tolerance %.2e)" % (o, o, diff, tol))
                assert diff <= tol
        sig.close()
        del sig, d1, d2, dressed, res, t1, t2, cc
    finally:
        ints.ctx.close()
    assert _live() == before


# ---- 6. the opt-in of CCSD.solve and the refusals -----------------------------------------------------------------------------------------
def test_ccsd_solve_response_4_12(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 4, 12
    n = no + nv
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    ops = np.random.default_rng(8).standard_normal((2, n, n))
    ops = ops + ops.transpose(0, 2, 1)
    opt = dict(operators=ops, omegas=[0.0, 0.1], gamma=0.02)
    cc = CCSD(no, delta_e=1e-13)
    base = quiet(cc.solve, f, V, max_iter=300)
    res = quiet(cc.solve, f, V, max_iter=300, response=opt)
    assert set(res) - set(base) == {"response", "polarizability", "response converged", "lambda1", "lambda2"}
    assert res["response converged"] and res["response"].shape == (2, 2, 2) and res["response"].dtype == np.complex128
    assert np.array_equal(res["polarizability"], -res["response"])
    assert cc.response_solver.lambda_solver.converged                               # (Lambda was solved on the response handle)
    # a hermitian problem and symmetric operators: the polarizability tensor is symmetric, its damped spectral density positive
    assert np.abs(res["response"] - res["response"].transpose(0, 2, 1)).max() < 1e-6 * np.abs(res["response"]).max()
    assert (cc.response_solver.spectral_density()[1] > 0.0)
    # shared with density=True through one Lambda solve
    both = quiet(cc.solve, f, V, max_iter=300, response=opt, density=True)
    assert set(both) - set(base) == {"response", "polarizability", "response converged", "lambda1", "lambda2", "rdm1",
                                      "natural occupations"}
    assert cc.response_solver.lambda_solver is None and cc.lambda_solver.converged
    assert np.array_equal(cc.response_solver.result["lambda1"], both["lambda1"])
    assert np.abs(both["response"] - res["response"]).max() < 1e-6 * np.abs(res["response"]).max()
    # with the truncations: the operators are those of the correlated space
    fno = quiet(cc.solve, f, V, max_iter=300, response=opt, frozen_core=1, fno_nv=8)
    assert fno["response converged"] and fno["response"].shape == (2, 2, 2)
    assert cc.response_solver.result["xi"][0][0].shape == (8, no - 1)
    # real frequencies: a real tensor
    real = quiet(cc.solve, f, V, max_iter=300, response=dict(operators=ops, omegas=[0.0]))
    assert real["response"].dtype == np.float64 and real["response converged"]


def test_refusals_by_name(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.model import synthetic
    from pymes_amd.solver import response as M
    from pymes_amd.solver.ccsd import CCSD
    E = _lib.PymesError
    no, nv = 4, 12
    n = no + nv
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    ops = np.zeros((1, n, n))
    good = dict(operators=ops, omegas=[0.0])
    before = _live()
    # the option of CCSD.solve
    with pytest.raises(ValueError, match="response: .*DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, response=good)
    with pytest.raises(ValueError, match="response with shard_integrals=True"):
        CCSD(no, shard_integrals=True).solve(f, V, response=good)
    with pytest.raises(ValueError, match=r"operators must be \[m, n, n\]"):
        CCSD(no).solve(f, V, response=dict(good, operators=np.zeros((1, n, n - 1))))
    with pytest.raises(ValueError, match="operators must be float64"):
        CCSD(no).solve(f, V, response=dict(good, operators=np.zeros((1, n, n), dtype=np.complex128)))
    with pytest.raises(E, match="EOM_CCSD_Response: nocc = 100 is too large"):
        M.EOM_CCSD_Response(100).solve(np.zeros((101, 101)), {}, np.zeros((1, 1, 100, 100)), np.zeros((1, 100)),
                                       np.zeros((1, 101, 101)), [0.0])
    assert _live() == before
    B, eps = synthetic.factors(no, nv, seed=1)
    for kind, options, word in (("shard", dict(shard=(0, 2)), "integral sharding"), ("direct", dict(direct=True), "direct")):
        ints = DeviceIntegrals.from_factors(no, B, **options)
        try:
            held = _live()
            with pytest.raises((E, ValueError), match=word):
                quiet(CCSD(no).solve, np.diag(eps), ints, response=good)
            assert _live() == held
        finally:
            ints.ctx.close()
    # the entries
    t1, t2, lam, _, _ = X.density_inputs(no, nv, 9)
    ctx = Context(no, nv)
    try:
        up = ctx.array
        d = [up(t1), up(t2), up(lam[0]), up(lam[1])]
        out = tuple([ctx.zeros(shape)] for shape in ((nv, no), (nv, nv, no, no)) * 2)
        with pytest.raises(E, match="response_vectors: output aliases input"):
            M.device_response_vectors(ctx, *d, ops, out=(out[0], [d[1]], out[2], out[3]))
        with pytest.raises(E, match="response_vectors: two outputs are the same array"):
            M.device_response_vectors(ctx, *d, ops, out=(out[0], out[1], out[2], out[1]))
        skew = up(np.random.default_rng(2).standard_normal((nv, nv, no, no)))
        with pytest.raises(E, match="response_vectors: t2 does not have the exchange symmetry"):
            M.device_response_vectors(ctx, d[0], skew, d[2], d[3], ops, out=out)
        with pytest.raises(E, match="response_vectors: lambda2 does not have the exchange symmetry"):
            M.device_response_vectors(ctx, d[0], d[1], d[2], skew, ops, out=out)
        with pytest.raises(E, match="null"):
            ctx.lib.call("pymes_response_vectors", ctx.handle, *[C.c_void_p(x.ptr) for x in d], 1, None,
                         *[_lib.ptr_array([x[0].ptr]) for x in out], _lib.host_ptr(np.zeros(1)))
        if ctx.graphs_supported():
            ctx.graph_begin()
            try:
                with pytest.raises(E, match="response_vectors while a launch graph is being recorded"):
                    M.device_response_vectors(ctx, *d, ops, out=out)
                with pytest.raises(E, match="response_update while a launch graph is being recorded"):
                    ctx.lib.call("pymes_response_update", ctx.handle, 1, C.byref(_lib.ResponseSystem()), C.c_void_p(d[1].ptr), 0.0,
                                 64, 64 + (nv * no) ** 2, _lib.host_ptr(np.zeros(1)))
                with pytest.raises(E, match="response_dots while a launch graph is being recorded"):
                    ctx.lib.call("pymes_response_dots", ctx.handle, 1, C.byref(_lib.ResponseSystem()), 64, 64 + (nv * no) ** 2,
                                 _lib.host_ptr(np.zeros(_lib.RESPONSE_DOTS)))
            finally:
                ctx.graph_abort()
        with pytest.raises(E, match="response_update: null"):
            ctx.lib.call("pymes_response_update", ctx.handle, 1, None, C.c_void_p(d[1].ptr), 0.0, 64, 64 + (nv * no) ** 2,
                         _lib.host_ptr(np.zeros(1)))
    finally:
        ctx.close()
