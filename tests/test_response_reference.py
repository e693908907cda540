"""CPU: the numpy reference of the EOM-CCSD linear response function (tests/_response_reference.py) — the written-out property
vectors against their definitions, the dense resolvent against the full sum over states and against the exact two-electron
value, the references of the solver's sweep (dots, fused update, the Orthomin loop built from them) against dense solves and a
case worked out by hand — and what of the device path needs no GPU: the declarations, the host side of the entries up to the kernels (host
simulator), the refusals of ``CCSD.solve(response=...)`` and ``UEG.density_operator``."""
import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.device import Context, PymesError
from tests import _response_reference as P
from tests import _transition_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pymes_response_vectors", "pymes_response_dots", "pymes_response_update")


@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_written_out_vectors_against_the_definitions(no, nv, seed):
    """xi(O) against the oracle's residuals with f = O, V = 0; eta(O) against gammaR's defining expression on every symmetric
    coordinate vector.  Random amplitudes and Lambda (nothing needs to solve anything), a non-symmetric operator."""
    t1, t2, lam, _, _ = T.density_inputs(no, nv, seed)
    O = np.random.default_rng(seed + 5).standard_normal((no + nv, no + nv))
    for name, ref, got in (("xi", P.xi_definition(no, t1, t2, O), P.xi_terms(no, t1, t2, O)),
                           ("eta", P.eta_definition(no, t1, t2, lam, O), P.eta_terms(no, t1, t2, lam, O))):
        for part in range(2):
            err = np.abs(ref[part] - got[part]).max()
            print("%s%d (%d,%d): %.2e" % (name, part + 1, no, nv, err))
            assert err < 1e-13
    assert np.array_equal(P.xi_terms(no, t1, t2, O)[1], P.xi_terms(no, t1, t2, O)[1].transpose(1, 0, 3, 2))


def test_definitions_are_linear_in_the_operator():
    """xi(O) and eta(O) by definition are linear in O, to rounding: a GPU test with 65 operators takes its references from the
    definitions of a few."""
    no, nv = 2, 3
    t1, t2, lam, _, _ = T.density_inputs(no, nv, 9)
    rng = np.random.default_rng(64)
    basis, coef = rng.standard_normal((3, no + nv, no + nv)), rng.standard_normal(3)
    both = lambda O: P.xi_definition(no, t1, t2, O) + P.eta_definition(no, t1, t2, lam, O)
    parts, whole = [both(O) for O in basis], both(np.einsum("b,bpq->pq", coef, basis))
    for k in range(4):
        mixed = sum(c * p[k] for c, p in zip(coef, parts))
        assert np.abs(mixed - whole[k]).max() < 1e-13 * max(1.0, np.abs(whole[k]).max())


@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_dense_resolvent_against_the_sum_over_all_states(no, nv, seed):
    """<eta(X), (z - A)^-1 xi(Y)> + <eta(Y), (-z - A)^-1 xi(X)> equals the sum over ALL states of the dense eigenproblem with the
    moments taken from the transition densities, at z = 0, 0.4 w1 and 1.3 w1 + 0.05i, for two non-symmetric operators."""
    ref = P.reference_problem(no, nv, seed, True, 2)
    dense = ref["dense"]
    states = dense.states()
    print("largest imaginary part among the eigenpairs: %.3e" % states[3])
    for z in P.frequencies(ref["w1"]):
        a, b = dense.response(z), dense.sum_over_states(z, states)
        assert np.abs(b.imag).max() <= 1e-12 * np.abs(b).max() or np.imag(z) != 0.0      # (complex pairs add up to a real sum)
        err = np.abs(a - b).max() / np.abs(b).max()
        print("(%d,%d) z = %s: relative difference %.2e, |(z - A)^-1| = %.1f" % (no, nv, z, err, dense.resolvent_norm(z)))
        assert err < 1e-10


def test_dense_resolvent_against_two_electron_fci():
    """(no, nv) = (1, 4): CCSD and its response function are exact for two electrons."""
    ref = P.reference_problem(1, 4, 3, True, 1, 0.05, True)
    for z in P.frequencies(ref["w1"]):
        got = -ref["dense"].response(z)[0, 0]
        want = P.two_electron_polarizability(ref["f"], ref["V"], ref["ops"][0], z)
        print("z = %s: polarizability %s, FCI %s" % (z, got, want))
        assert abs(got - want) < 1e-10 * max(1.0, abs(want))


# ---- the references of the solver's sweep, before a kernel is judged by them ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _orthomin_problem(no, nv, seed, hermitian):
    """(A, d, xi, w1): A in an orthonormalised symmetric basis (the construction of ``DenseResponse.resolvent_norm``), its
    diagonal, the xi of operator 0 in that basis."""
    ref = P.reference_problem(no, nv, seed, hermitian, 2)
    dense = ref["dense"]
    Q, _ = np.linalg.qr(dense.co.B)
    A = Q.T @ (dense.co.B @ np.linalg.solve(dense.G, dense.BA) @ np.linalg.solve(dense.G, dense.co.B.T @ Q))
    return A, np.diag(A).copy(), Q.T @ dense.co.full(*dense.xi[0]), ref["w1"]


@pytest.mark.parametrize("history", [1, 2, 12])
@pytest.mark.parametrize("hermitian", [True, False], ids=["8-fold", "non-hermitian"])
@pytest.mark.parametrize("no,nv,seed", [(2, 3, 11), (3, 5, 12)])
def test_orthomin_reference_against_the_dense_solve(no, nv, seed, hermitian, history):
    """The loop of ``EOM_CCSD_Response._sweep`` written with ``sweep_dots_reference`` and ``sweep_update_reference`` alone, at
    z = 0, +-0.4 w1 and 0.4 w1 + 0.05i: it converges within 200 sweeps, its fresh residual is at r_epsilon, x is the dense
    solution within 10 r_epsilon |xi| |(z - A)^-1|_2, and a window of 1 or 2 pairs slides (more sweeps than ``history``)."""
    A, d, xi, w1 = _orthomin_problem(no, nv, seed, hermitian)
    r_eps, floor, eye = 1e-10, 1e-3, np.eye(len(xi))
    for z in (0.0, 0.4 * w1, -0.4 * w1, 0.4 * w1 + 0.05j):
        x, sweeps, res = P.orthomin_reference(A, d, xi, z, history, floor, r_eps, 200)
        want = np.linalg.solve(z * eye - A, xi.astype(np.complex128))
        tol = 10.0 * r_eps * np.linalg.norm(xi) * np.linalg.norm(np.linalg.inv(z * eye - A), 2)
        err = np.linalg.norm(x - want)
        print("(%d,%d) %s history %d z = %s: %d sweeps, fresh residual %.2e, |x - dense| %.2e (tolerance %.2e)"
              % (no, nv, "8-fold" if hermitian else "non-hermitian", history, z, sweeps, res, err, tol))
        assert sweeps < 200 and res <= 1.01 * r_eps
        assert err <= tol
        assert np.imag(z) != 0.0 or np.abs(x.imag).max() == 0.0          # (a real system stays real)
        if history <= 2:
            assert sweeps > history


def test_sweep_references_on_a_hand_made_case():
    """Four active elements around a pad of NaN: the dots, the step and the floor against numbers worked out by hand."""
    nan = np.nan
    S = P.SweepSystem(x=np.array([1.0, nan, 0.0, 2.0, 1.0]), r=np.array([2.0, nan, 1.0, -1.0, 4.0]) + 0j,
                      p=np.array([1.0, nan, 2.0, 0.0, 1.0]) + 1j * np.array([0.0, nan, 1.0, 1.0, 0.0]),
                      ap=np.array([0.0, nan, 1.0, 1.0, 2.0]) + 0j, hp=[np.array([1.0, nan, 0.0, 0.0, 0.0]) + 0j],
                      hq=[np.array([0.0, nan, 1j, 0.0, 0.0])], g=[2.0j], alpha=0.5, z=2.0, inv=0.5)
    # q = 2 p - ap = [2, -, 3 + 2i, -1 + 2i, 0]
    row, mags = P.sweep_dots_reference(S, 1, 2)
    assert list(row[:6]) == [2.0, -3.0, 22.0, 0.0, 8.0, 0.0] and not row[6:].any()           # conj(i) (3 + 2i) = 2 - 3i
    # mag(q) = 2 mag(p) + mag(ap) = [2, -, 7, 3, 4]
    assert list(mags[:6]) == [7.0, 7.0, 4.0 + 49.0 + 9.0 + 16.0, 0.0, 4.0 + 7.0 + 3.0 + 16.0, 4.0 + 7.0 + 3.0 + 16.0] and not mags[6:].any()
    d = np.array([1.0, nan, 2.0, 2.0 + 0.25, 4.0])
    new, m, nrm, mnrm, floored = P.sweep_update_reference(S, d, 0.5, 1, 2)
    # ph = (p - 2i hp) / 2 = [0.5 - i, -, 1 + 0.5i, 0.5i, 0.5];  qh = (q - 2i hq) / 2 = [1, -, 2.5 + i, -0.5 + i, 0]
    assert np.array_equal(new["p"][[0, 2, 3, 4]], [0.5 - 1j, 1 + 0.5j, 0.5j, 0.5])
    assert np.array_equal(new["ap"][[0, 2, 3, 4]], [1.0, 2.5 + 1j, -0.5 + 1j, 0.0])
    assert np.array_equal(new["x"][[0, 2, 3, 4]], [1.25 - 0.5j, 0.5 + 0.25j, 2 + 0.25j, 1.25])
    assert np.array_equal(new["r"][[0, 2, 3, 4]], [1.5, -0.25 - 0.5j, -0.75 - 0.5j, 4.0])
    # z - d = [1, -, +0 -> 0.5, -0.25 -> -0.5, -2]
    assert list(floored) == [False, False, True, True, False]
    assert np.array_equal(new["pn"], [1.5, 0.0, -0.5 - 1j, 1.5 + 1j, -2.0]) and not np.signbit(new["pn"][1].real)
    assert nrm == 2.25 + 0.3125 + 0.8125 + 16.0
    # mag(qh) = ([2, -, 7, 3, 4] + 2 [0, -, 1, 0, 0]) / 2, mag(r) = [2, -, 1, 1, 4] + mag(qh) / 2
    assert np.array_equal(m["r"][[0, 2, 3, 4]], [2.5, 3.25, 1.75, 5.0]) and mnrm == 2.5 ** 2 + 3.25 ** 2 + 1.75 ** 2 + 25.0
    assert np.array_equal(m["pn"][[0, 2, 3, 4]], [2.5, 6.5, 3.5, 2.5])
    # no step: x and r as given, pn and |r|^2 of the r given
    S.p = S.ap = None
    with np.errstate(all="ignore"):
        new, m, nrm, _, floored = P.sweep_update_reference(S, d, 0.0, 1, 2)
    assert new["p"] is None and np.array_equal(new["r"][[0, 2, 3, 4]], [2.0, 1.0, -1.0, 4.0]) and nrm == 22.0
    assert np.array_equal(new["pn"][[0, 3, 4]], [2.0, 4.0, -2.0]) and not np.isfinite(new["pn"][2]) and not floored.any()


# ---- what needs no GPU of the device path ---------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and name in integration
    assert int(re.search(r"#define PYMES_RESPONSE_HIST (\d+)", header).group(1)) == _lib.RESPONSE_HIST
    # the structure of the systems, field by field as the header declares it
    body = re.search(r"typedef struct pymes_response_system \{(.*?)\} pymes_response_system;", header, re.S).group(1)
    declared = re.findall(r"\*?\s*(\w+)\[", body) + re.findall(r",\s*(inv)\b", body) + re.findall(r"int (nh)\b", body)
    assert [n for n, _ in _lib.ResponseSystem._fields_] == list(dict.fromkeys(declared))
    assert C.sizeof(_lib.ResponseSystem) == 8 * (10 + 6 * _lib.RESPONSE_HIST + 5) + 8
    for doc, word in (("README.md", "EOM_CCSD_Response"), ("DESIGN.md", "## 8h. EOM-CCSD linear response")):
        assert word in open(os.path.join(ROOT, doc)).read()


def _device_inputs(ctx, no, nv, seed=9):
    t1, t2, lam, _, _ = T.density_inputs(no, nv, seed)
    return [ctx.array(x) for x in (t1, t2, lam[0], lam[1])]


def test_the_host_side_runs_to_the_kernel_stubs_and_refuses_by_name(hostsim_lib):
    """On the host simulator the entries check their arguments, dress the operators and run the engine products; the kernels are
    the product library's."""
    from pymes_amd.solver import response as M
    from pymes_amd.solver.subspace import FlatLayout
    no, nv = 2, 3
    ctx = Context(no, nv, lib=hostsim_lib)
    try:
        t1, t2, l1, l2 = _device_inputs(ctx, no, nv)
        ops = np.random.default_rng(1).standard_normal((2, no + nv, no + nv))
        with pytest.raises(PymesError, match="response_singles: not available in this backend"):
            M.device_response_vectors(ctx, t1, t2, l1, l2, ops)
        outs = lambda: tuple([ctx.zeros(shape)] for shape in ((nv, no), (nv, nv, no, no)) * 2)
        out = outs()
        with pytest.raises(PymesError, match="response_vectors: output aliases input"):
            M.device_response_vectors(ctx, t1, t2, l1, l2, ops[:1], out=([t1],) + out[1:])
        with pytest.raises(PymesError, match="response_vectors: two outputs are the same array"):
            M.device_response_vectors(ctx, t1, t2, l1, l2, ops[:1], out=(out[0], out[1], out[0], out[3]))
        skew = ctx.array(np.random.default_rng(2).standard_normal((nv, nv, no, no)))
        with pytest.raises(PymesError, match="response_vectors: t2 does not have the exchange symmetry"):
            M.device_response_vectors(ctx, t1, skew, l1, l2, ops[:1], out=out)
        with pytest.raises(PymesError, match="response_vectors: lambda2 does not have the exchange symmetry"):
            M.device_response_vectors(ctx, t1, t2, l1, skew, ops[:1], out=out)
        with pytest.raises(PymesError, match="null pointer|null argument"):
            ctx.lib.call("pymes_response_vectors", ctx.handle, None, C.c_void_p(t2.ptr), C.c_void_p(l1.ptr), C.c_void_p(l2.ptr), 1,
                         _lib.host_ptr(ops[:1].copy()), *[_lib.ptr_array([x[0].ptr]) for x in out], _lib.host_ptr(np.zeros(1)))
        with pytest.raises(PymesError, match="1 <= k <= 64 operators"):
            ctx.lib.call("pymes_response_vectors", ctx.handle, *[C.c_void_p(x.ptr) for x in (t1, t2, l1, l2)], 65,
                         _lib.host_ptr(ops[:1].copy()), *[_lib.ptr_array([x[0].ptr]) for x in out], _lib.host_ptr(np.zeros(1)))
        # the sweep's two entries
        lay = FlatLayout(ctx, (nv, no), (nv, nv, no, no))
        vec = lambda: ctx.zeros((lay.nflat,))
        solver = M.EOM_CCSD_Response(no)
        sy = M._System(0, 0.3, False)
        sy.x, sy.r, sy.pn, sy.p, sy.ap = (vec(), None), (vec(), None), (vec(), None), (vec(), None), (vec(), None)
        sy.alpha, sy.inv, sy.g = 0j, 1.0, []
        d = vec()
        with pytest.raises(PymesError, match="response_update: not available in this backend"):
            solver._update(ctx, lay, d, [sy], False)
        with pytest.raises(PymesError, match="response_dots: not available in this backend"):
            solver._dots(ctx, lay, [sy])
        bad = FlatLayout(ctx, (nv, no), (nv, nv, no))
        with pytest.raises(PymesError, match="response_update: the flat layout does not match"):
            solver._update(ctx, bad, d, [sy], False)
        with pytest.raises(PymesError, match="response_dots: the flat layout does not match"):
            solver._dots(ctx, bad, [sy])
        half = M._System(0, 0.3, False)
        half.x, half.r, half.pn, half.p, half.ap = (vec(), vec()), (vec(), None), (vec(), None), None, None
        half.alpha, half.inv, half.g = 0j, 1.0, []
        with pytest.raises(PymesError, match="a system is real .* or complex"):
            solver._update(ctx, lay, d, [half], False)
    finally:
        ctx.close()


def test_ccsd_refuses_the_response_option_by_name_before_anything_is_uploaded():
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.lambda_ccsd import NOCC_MAX
    no, nv = 2, 3
    n = no + nv
    f, ops = np.diag(np.arange(n, dtype=np.float64)), np.zeros((1, n, n))
    good = dict(operators=ops, omegas=[0.0])
    no_upload = SimpleNamespace(direct=False)          # (not integrals: anything that tried to upload it would fail otherwise)
    with pytest.raises(ValueError, match="response: .*not defined for DCSD"):
        CCSD(no, is_dcsd=True).solve(f, no_upload, response=good)
    with pytest.raises(ValueError, match="response with shard_integrals=True"):
        CCSD(no, shard_integrals=True).solve(f, no_upload, response=good)
    with pytest.raises(ValueError, match="response with direct=True integrals"):
        CCSD(no).solve(f, SimpleNamespace(direct=True), response=good)
    with pytest.raises(ValueError, match=r"response: operators must be \[m, n, n\] with n = 5"):
        CCSD(no).solve(f, no_upload, response=dict(good, operators=np.zeros((1, n, n + 1))))
    with pytest.raises(ValueError, match="response: operators must be float64"):
        CCSD(no).solve(f, no_upload, response=dict(good, operators=np.zeros((1, n, n), dtype=np.complex128)))
    with pytest.raises(ValueError, match="response: operators must be float64"):
        CCSD(no).solve(f, no_upload, response=dict(good, operators=np.zeros((1, n, n), dtype=np.float32)))
    with pytest.raises(ValueError, match="response: expected dict"):
        CCSD(no).solve(f, no_upload, response=dict(operators=ops))
    with pytest.raises(ValueError, match="response: unknown option"):
        CCSD(no).solve(f, no_upload, response=dict(good, damping=0.1))
    big = NOCC_MAX + 1
    fb = np.diag(np.arange(big + 2, dtype=np.float64))
    with pytest.raises(PymesError, match="EOM_CCSD_Response: nocc = %d is too large" % big):
        CCSD(big).solve(fb, no_upload, response=dict(operators=np.zeros((1, big + 2, big + 2)), omegas=[0.0]))


def test_ueg_density_operator_against_the_basis_vectors():
    from pymes_amd.model.ueg import UEG
    ueg = UEG(14, 7, 7, 1.0)
    ueg.init_single_basis(3)
    k = np.array([ueg.basis_fns[2 * i].k for i in range(len(ueg.basis_fns) // 2)])
    for q in ([1, 0, 0], [0, -1, 1], [2, 0, 0], [0, 0, 0]):
        O = ueg.density_operator(q)
        assert O.shape == (len(k), len(k)) and O.dtype == np.float64
        for p in range(len(k)):
            for r in range(len(k)):
                assert O[p, r] == (1.0 if np.array_equal(k[p] - k[r], q) else 0.0)
        assert np.array_equal(ueg.density_operator([-x for x in q]), O.T)        # rho_-q is the transpose
    assert np.array_equal(ueg.density_operator([0, 0, 0]), np.eye(len(k)))
    assert ueg.density_operator([1, 0, 0]).sum() > 0
    with pytest.raises(ValueError, match="three integers"):
        ueg.density_operator([0.5, 0, 0])
    with pytest.raises(RuntimeError, match="init_single_basis"):
        UEG(14, 7, 7, 1.0).density_operator([1, 0, 0])
