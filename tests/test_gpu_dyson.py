"""GPU: left IP / EA-EOM-CCSD vectors, Dyson amplitudes and pole strengths (pymes_amd/solver/eom_dyson.py; csrc/eom.cpp,
IpEaSigma::apply_left, ipea_dyson; include/pymes_amd.h, pymes_ipea_sigma_apply_left / pymes_ipea_dyson).  The left apply against
the transposed dense operator, stacked against single, the amplitude kernel against the definition, the solver against the dense
biorthonormal eigenvectors (tests/_dyson_reference.py), the exact two-electron residues, the opt-in of CCSD.solve, sharding."""
import contextlib
import ctypes as C
import gc
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc, io_oracle as oio
from oracle.cases import random_case, synthetic_case
from oracle.io_oracle import synthetic_factors
from pymes_amd import _lib
from tests import _dyson_reference as D
from tests import _ipea_reference as R
from tests import _lambda_reference as LR

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KINDS = ("ip", "ea")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    gc.collect()
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _kind_id(kind):
    from pymes_amd.solver import eom_ip_ea as M
    return M.KIND_IP if kind == "ip" else M.KIND_EA


def _solver(kind, no, n_roots=3, **kw):
    from pymes_amd.solver.eom_dyson import EA_EOM_CCSD_Dyson, IP_EOM_CCSD_Dyson
    return (IP_EOM_CCSD_Dyson if kind == "ip" else EA_EOM_CCSD_Dyson)(no, n_roots=n_roots, **kw)


def _vectors(kind, no, nv, k, seed):
    rng = np.random.default_rng(seed)
    s1, s2 = R.shapes(kind, no, nv)
    return [rng.standard_normal(s1) for _ in range(k)], [rng.standard_normal(s2) for _ in range(k)]


def _sym_case(no, nv, seed):
    """The inputs of test_gpu_ip_ea's _check_sigma: integrals with V_pqrs = V_qpsr only, a non-symmetric Fock matrix,
    exchange-symmetric T2."""
    f, V, t1, t2 = random_case(no, nv, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return f + 0.03 * rng.standard_normal(f.shape), R.symmetrise(V), 0.1 * t1, t2


@contextlib.contextmanager
def _handle(kind, no, f, Vb, t2):
    """(ctx, IPEASigma) on a context that holds the blocks of the operator as they are."""
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_ip_ea import IPEASigma
    ctx = Context(no, f.shape[0] - no)
    try:
        for name in IPEASigma.BLOCKS[_kind_id(kind)]:
            ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        sig = IPEASigma(ctx, _kind_id(kind), f, ctx.array(t2))
        yield ctx, sig
        sig.close()
    finally:
        ctx.close()


def _get(pairs):
    return [(a.get(), b.get()) for a, b in pairs]


# ---- 1. the left apply against the transposed operator ------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5), (5, 19), (7, 33), (8, 40), (20, 10)])
@pytest.mark.parametrize("kind", KINDS)
def test_left_apply_against_the_transposed_operator(gpu_lib, kind, no, nv):
    """k = 3 stacked and each alone against dense(kind).T @ l — evaluated as the adjoint term tables, which tests/test_dyson.py
    pins against the transposed matrix (the matrix itself takes minutes beyond (3,5)) — with the bound of _check_sigma; at (8,40)
    the adjoint identity <l, H r> = <H^T l, r> on the device."""
    f, V, _, t2 = _sym_case(no, nv, seed=no + 3 * nv)
    Vb = oc.split_blocks(no, V)
    l1s, l2s = _vectors(kind, no, nv, 3, 5)
    H = R.dense(kind, no, f, Vb, t2) if no * nv <= 15 else None
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        up = lambda xs: [ctx.array(x) for x in xs]
        stacked = _get(sig.apply_left_many(up(l1s), up(l2s)))
        for z in range(3):
            a, b = D.left_sigma_terms(kind, no, f, Vb, t2, l1s[z], l2s[z])
            if H is not None:
                want = H.T @ D.flat((l1s[z], l2s[z]))
                assert np.abs(D.flat((a, b)) - want).max() <= 1e-12 * np.abs(want).max()
            scale = max(np.abs(a).max(), np.abs(b).max())
            one = _get(sig.apply_left_many(up(l1s[z:z + 1]), up(l2s[z:z + 1])))[0]
            for got in (stacked[z], one):
                err = max(np.abs(got[0] - a).max(), np.abs(got[1] - b).max())
                print(kind, no, nv, "vector", z, "max error / max |ref|", err / scale)
                assert err <= 1e-11 * scale, (kind, no, nv, z, err / scale)
        if (no, nv) == (8, 40):
            r1s, r2s = _vectors(kind, no, nv, 3, 6)
            sr = _get(sig.apply_many(up(r1s), up(r2s)))
            for z in range(3):
                a = D.dot((l1s[z], l2s[z]), sr[z])
                b = D.dot(stacked[z], (r1s[z], r2s[z]))
                print(kind, "vector %d: <l, H r> = %.15e  <H^T l, r> = %.15e  relative %.2e" % (z, a, b, abs(a - b) / abs(a)))
                assert abs(a - b) <= 1e-11 * abs(a)


# ---- 2. stacked against single -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(3, 5), (7, 33)])
@pytest.mark.parametrize("kind", KINDS)
def test_stacked_left_apply_equals_the_single_one(gpu_lib, kind, no, nv):
    f, V, _, t2 = _sym_case(no, nv, seed=no + 3 * nv)
    Vb = oc.split_blocks(no, V)
    l1s, l2s = _vectors(kind, no, nv, 3, 7)
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        d1, d2 = [ctx.array(x) for x in l1s], [ctx.array(x) for x in l2s]
        ctx.stats(reset=True)
        single = [_get(sig.apply_left_many(d1[z:z + 1], d2[z:z + 1]))[0] for z in range(3)]
        c1 = ctx.stats(reset=True)["gemm_calls"]
        stacked = _get(sig.apply_left_many(d1, d2))
        c3 = ctx.stats(reset=True)["gemm_calls"]
        again = _get(sig.apply_left_many(d1, d2))
        print(kind, "(%d,%d) GEMM calls: three k = 1 builds %d, one k = 3 build %d" % (no, nv, c1, c3))
        assert c3 < c1
        for z in range(3):
            scale = max(np.abs(single[z][0]).max(), np.abs(single[z][1]).max())
            dev = max(np.abs(single[z][0] - stacked[z][0]).max(), np.abs(single[z][1] - stacked[z][1]).max())
            print("   vector %d: max |stacked - single| / max |single| = %.2e" % (z, dev / scale))
            assert dev <= 1e-13 * scale
            assert np.array_equal(stacked[z][0], again[z][0]) and np.array_equal(stacked[z][1], again[z][1])


# ---- 3. the amplitude kernel against the definition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5), (5, 19), (20, 10)])
@pytest.mark.parametrize("kind", KINDS)
def test_dyson_against_the_definition(gpu_lib, kind, no, nv):
    """Random vectors that solve nothing, k = 3 and k = 1, against D2 evaluated with the oracles (2 n residual / sigma
    evaluations on the problem with the extra orbital; at (5,19) and (20,10) recorded in tests/golden by ``python -m
    tests._dyson_reference``); the bound of test_tdm1_against_the_definitions."""
    t1, t2, lam, ls, rs = D.definition_inputs(kind, no, nv)
    l1s, l2s, r1s, r2s = [x[0] for x in ls], [x[1] for x in ls], [x[0] for x in rs], [x[1] for x in rs]
    name, recorded = D.GOLDEN_DYSON
    if (no, nv) in recorded:
        gold = np.load(os.path.join(GOLD, name))
        ref_l, ref_r = gold["%s_%d_%d_left" % (kind, no, nv)], gold["%s_%d_%d_right" % (kind, no, nv)]
    else:
        ref_l, ref_r = D.dyson_definition(kind, no, t1, t2, lam, ls, rs)
    n = no + nv
    f, Vb = np.diag(np.arange(1.0, n + 1.0)), oc.split_blocks(no, np.zeros((n, n, n, n)))
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        up = ctx.array
        ups = lambda xs: [ctx.array(x) for x in xs]
        args = (up(t1), up(lam[0]), up(lam[1]))
        pl, pr = sig.dyson(*args, ups(l1s), ups(l2s), ups(r1s), ups(r2s))
        pl2, pr2 = sig.dyson(*args, ups(l1s), ups(l2s), ups(r1s), ups(r2s))
        pl1, pr1 = sig.dyson(*args, ups(l1s[1:2]), ups(l2s[1:2]), ups(r1s[1:2]), ups(r2s[1:2]))
    el, er = np.abs(pl - ref_l).max(), np.abs(pr - ref_r).max()
    e1 = max(np.abs(pl1[0] - ref_l[1]).max(), np.abs(pr1[0] - ref_r[1]).max())
    print(kind, no, nv, "max |psiL - definition| = %.2e  max |psiR - definition| = %.2e  k = 1: %.2e" % (el, er, e1))
    assert el < 1e-10 and er < 1e-10 and e1 < 1e-10
    assert np.array_equal(pl, pl2) and np.array_equal(pr, pr2)
    assert np.abs(pl[0] - pl[1]).max() > 1e-3 and np.abs(pr[0] - pr[1]).max() > 1e-3


# ---- 4. the solver against the dense biorthonormal eigenvectors ------------------------------------------------------------------------
@pytest.mark.parametrize("eight", [True, False], ids=["8-fold", "non-hermitian"])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
@pytest.mark.parametrize("kind", KINDS)
def test_solver_against_the_dense_reference(gpu_lib, kind, no, nv, seed, eight):
    nr = 3 if kind == "ea" or no >= 3 else 2                       # (IP at (2,3) has two singles)
    ref = D.reference_case(kind, no, nv, seed, eight, 4)
    assert ref["imag"] == 0.0                                      # the four lowest roots are real
    fd, Vd, t1, t2 = ref["fd"], ref["Vd"], ref["t1"], ref["t2"]
    eps = 1e-10
    s = _solver(kind, no, nr, r_epsilon=eps)
    out = quiet(s.solve, fd, Vd, t2, t1)
    dw = np.abs(out["e"] - ref["w"][:nr]).max()
    # sign-free: Z_k and P_k are products of one left and one right quantity of the same root
    Z, P = s.residues(), out["pole strengths"]
    Zr, Pr = D.residues(ref["psiL"][:nr], ref["psiR"][:nr]), D.pole_strengths(ref["psiL"][:nr], ref["psiR"][:nr])
    dz, dp = np.abs(Z - Zr).max(), np.abs(P - Pr).max()
    print("%s (%d,%d) %s: |w - dense| %.2e  |Z - dense| %.2e  |P - dense| %.2e  biorthogonality %.2e  passes %s  P %s"
          % (kind, no, nv, "8-fold" if eight else "non-hermitian", dw, dz, dp, out["biorthogonality"], out["iterations"], P))
    assert out["converged"]
    assert dw < 1e-9
    assert dz < 1e-7 and dp < 1e-7
    assert out["biorthogonality"] < 1e-9
    assert np.array_equal(P, (out["dyson left"] * out["dyson right"]).sum(axis=1))
    A = s.spectral_function(np.array([0.3, -0.7]), 0.05)
    assert np.abs(A - D.spectral_function(kind, out["e"], out["dyson left"], out["dyson right"], [0.3, -0.7], 0.05)).max() < 1e-13
    if eight:
        assert np.all(P > 0.0) and np.all(P <= 1.0)
    else:                                  # the left vector is not the right one
        l, r = (out["l1"][0], out["l2"][0]), (out["r1"][0], out["r2"][0])
        assert D.dot(l, r) / np.sqrt(D.dot(l, l) * D.dot(r, r)) < 0.999
    # the residuals under a FRESH sigma handle
    with _handle(kind, no, fd, Vd, t2) as (ctx, sig):
        for k in range(nr):
            r, l = (out["r1"][k], out["r2"][k]), (out["l1"][k], out["l2"][k])
            a = _get(sig.apply_many([ctx.array(r[0])], [ctx.array(r[1])]))[0]
            b = _get(sig.apply_left_many([ctx.array(l[0])], [ctx.array(l[1])]))[0]
            w = out["e"][k]
            rr = np.sqrt(((a[0] - w * r[0]) ** 2).sum() + ((a[1] - w * r[1]) ** 2).sum()) / np.sqrt(D.dot(r, r))
            rl = np.sqrt(((b[0] - w * l[0]) ** 2).sum() + ((b[1] - w * l[1]) ** 2).sum()) / np.sqrt(D.dot(l, l))
            print("   root %d: fresh right residual %.2e (reported %.2e), left %.2e (reported %.2e)"
                  % (k, rr, out["right residual"][k], rl, out["left residual"][k]))
            assert rr < eps and rl < eps


# ---- 5. two electrons: CCSD is exact ----------------------------------------------------------------------------------------------------------
def _check_two_electron(f, V, fd, Vd, t1, t2, nr):
    w, d = D.two_electron_dyson(f, V)
    s = _solver("ip", 1, nr, r_epsilon=1e-10)
    out = quiet(s.solve, fd, Vd, t2, t1)
    assert out["converged"]
    Z = s.residues()
    dz = max(np.abs(Z[k] - np.outer(d[k], d[k])).max() for k in range(nr))
    print("two electrons: |w - exact| %.2e  |Z - d d^T| %.2e  P %s" % (np.abs(out["e"] - w[:nr]).max(), dz, out["pole strengths"]))
    assert np.abs(out["e"] - w[:nr]).max() < 1e-8
    assert dz < 1e-8
    return out


def test_two_electron_residues_1_3(gpu_lib):
    c = D.reference_case("ip", 1, 3, 3, True, None, 0.05)
    out = _check_two_electron(c["f"], c["V"], c["fd"], c["Vd"], c["t1"], c["t2"], 1)
    assert abs(out["pole strengths"][0] - 0.97416896) < 1e-7


def test_two_electron_residues_h2_321g(gpu_lib):
    """FCIDUMP.H2.321g as test_two_electron_ip_spectrum builds it: CCSD on the device, then the exact residues."""
    from pymes_amd.integral.partition import part_2_body_int
    from pymes_amd.solver.ccsd import CCSD
    ne, n, ec, eps, h, V = oio.read_fcidump(os.path.join(GOLD, "fcidump", "FCIDUMP.H2.321g"), is_tc=False)
    no = ne // 2
    assert no == 1
    f = oio.fock_matrix(no, h, V)
    cc = CCSD(no, delta_e=1e-13)
    res = quiet(cc.solve, f, V, max_iter=200)
    Vb = part_2_body_int(no, V)
    fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], Vb)
    Vd = quiet(cc.get_T1_dressed_V, res["t1"], Vb)
    Vd = {k: (v if v is not None else Vb[k]) for k, v in Vd.items()}
    assert np.abs(h - (f - (2.0 * V[:, 0, :, 0] - V[:, 0, 0, :]))).max() < 1e-12
    _check_two_electron(f, V, fd, Vd, res["t1"], 0.5 * LR.symd(res["t2"]), 1)


# ---- 6. the opt-in of CCSD.solve and the refusals ---------------------------------------------------------------------------------------------
def test_ccsd_solve_dyson_4_12(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 4, 12
    f, V = LR.random_problem(no, nv, seed=13, eight=True, scale=0.005)
    # (a solver object per run: a second solve on the same object starts from the state the first one left in it)
    old = quiet(CCSD(no, delta_e=1e-13).solve, f, V, max_iter=300, ip_roots=2, ea_roots=2)
    cc = CCSD(no, delta_e=1e-13)
    res = quiet(cc.solve, f, V, max_iter=300, ip_roots=2, ea_roots=2, dyson=True)
    new = ("ip pole strengths", "ip dyson left", "ip dyson right", "ea pole strengths", "ea dyson left", "ea dyson right")
    assert set(res) - set(old) == set(new)
    for key in old:                                                 # every old key: the same bits
        assert np.array_equal(np.asarray(res[key]), np.asarray(old[key])), key
    assert cc.ea_dyson_solver.lambda_solver is None and cc.ip_dyson_solver.lambda_solver.converged      # (Lambda once)
    Vb = oc.split_blocks(no, V)
    fd, Vd = oc.dressed_fock(no, f, res["t1"], Vb), oc.dressed_V(res["t1"], Vb)
    Vd = {k: (v if v is not None else Vb[k]) for k, v in Vd.items()}
    for kind in KINDS:
        sep = quiet(_solver(kind, no, 2).solve, fd, Vd, res["t2"], res["t1"])
        P, Z = res[kind + " pole strengths"], D.residues(res[kind + " dyson left"], res[kind + " dyson right"])
        print(kind, "P", P, "separate", sep["pole strengths"], "roots", res[kind + " e"], sep["e"])
        assert res[kind + " dyson left"].shape == (2, no + nv)
        # (both runs stop at a relative residual of 1e-8, the gaps are of order 0.1: vectors and amplitudes agree to ~1e-7)
        assert np.abs(P - sep["pole strengths"]).max() < 1e-6
        assert np.abs(Z - D.residues(sep["dyson left"], sep["dyson right"])).max() < 1e-6
        assert np.all(P > 0.5) and np.all(P <= 1.0)
    # together with the truncations, (T) and the density (canonical orbitals: the synthetic case of the ee_roots test): Lambda
    # once, amplitudes of the correlated space
    f, V, _, _ = synthetic_case(no, nv, seed=3)
    res = quiet(cc.solve, f, V, max_iter=300, ip_roots=2, ea_roots=1, dyson=True, frozen_core=1, fno_nv=8, density=True,
                triples=True)
    assert "(t) e" in res
    m = (no - 1) + 8
    assert res["ip dyson left"].shape == (2, m) and res["ea dyson right"].shape == (1, m) and res["rdm1"].shape == (m, m)
    assert cc.ip_dyson_solver.lambda_solver is None and cc.lambda_solver.converged          # (Lambda came from density=True)
    assert np.array_equal(cc.ip_dyson_solver.result["lambda1"], res["lambda1"])


def test_refusals_by_name(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.ccsd import CCSD
    E = _lib.PymesError
    no, nv = 4, 12
    f, V = LR.random_problem(no, nv, seed=13, eight=True, scale=0.005)
    before = _live()
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, ip_roots=2, dyson=True)
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(no, shard_integrals=True).solve(f, V, ip_roots=2, dyson=True)
    with pytest.raises(ValueError, match="needs ip_roots"):
        CCSD(no).solve(f, V, dyson=True)
    assert _live() == before
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        ctx = ints.ctx
        t1, t2 = np.zeros((nv, no)), np.zeros((nv, nv, no, no))
        for kind in KINDS:
            s = _solver(kind, no)
            dressed = quiet(CCSD(no).get_T1_dressed_V, t1, ints, s.blocks(True))
            ctx.graph_begin()
            try:
                held, mem = _live(), ctx.mem_info()
                with pytest.raises(E, match="recording a launch graph"):
                    s.solve(f, dressed, t2, t1)
                assert _live() == held and ctx.mem_info() == mem
            finally:
                ctx.graph_abort()
    finally:
        ints.ctx.close()


# ---- 7. IP with lam= on an integral-sharded context -----------------------------------------------------------------------------------------
def test_ip_with_lambda_on_a_sharded_context_ea_refused(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 6, 24
    B, eps = synthetic_factors(no, nv, seed=5)
    f = np.diag(eps)
    full = DeviceIntegrals.from_factors(no, B)
    shard = DeviceIntegrals.from_factors(no, B, shard=(1, 2))
    try:
        cc = CCSD(no, delta_e=1e-12)
        res = quiet(cc.solve, f, full, max_iter=200, device_amplitudes=True)
        t1, t2 = res["t1"].get(), res["t2"].get()
        outs, lam = [], None
        for ints in (full, shard):
            s = _solver("ip", no, 2)
            fd = quiet(cc.get_T1_dressed_fock, f, t1, ints)
            dressed = quiet(cc.get_T1_dressed_V, t1, ints, s.blocks(lam is None))     # (sharded: never asks for abcd)
            out = quiet(s.solve, fd, dressed, ints.ctx.array(t2), t1, lam=lam)
            assert out["converged"]
            lam = (out["lambda1"], out["lambda2"])
            outs.append(out)
        a, b = outs
        print("IP pole strengths replicated / sharded", a["pole strengths"], b["pole strengths"])
        assert np.abs(a["e"] - b["e"]).max() < 1e-12
        assert np.abs(a["pole strengths"] - b["pole strengths"]).max() < 1e-12
        assert np.abs(D.residues(a["dyson left"], a["dyson right"]) - D.residues(b["dyson left"], b["dyson right"])).max() < 1e-12
        # without lam= on the sharded context, and EA at all: refused by the name of the mode, nothing allocated
        ctx = shard.ctx
        dressed = quiet(cc.get_T1_dressed_V, t1, shard, s.BLOCKS)
        t2d = ctx.array(t2)
        held, mem = _live(), ctx.mem_info()
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            quiet(_solver("ip", no, 2).solve, fd, dressed, t2d, t1)
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            quiet(_solver("ea", no, 2).solve, fd, dressed, t2d, t1, lam=lam)
        assert _live() == held and ctx.mem_info() == mem
    finally:
        full.ctx.close()
        shard.ctx.close()
