"""GPU: the CCSD two-particle response density and two-body expectation values (pymes_amd/solver/lambda_ccsd.py, rdm2 /
expectation2; csrc/eom.cpp, lambda_rdm2 / lambda_rdm2_expectation; kernels_post.hip, rdm2_assemble / rdm2_contract).
Every block against the written-out reference (tests/_rdm2_reference.py, itself pinned against the definition on the CPU) and, at
(3,5), against the recorded definition; the device contraction against one evaluation of the Lagrangian; identical bits of
identical calls; CCSD.solve(rdm2=True) end to end; the refusals."""
import contextlib
import ctypes as C
import functools
import io

import numpy as np
import pytest

from oracle import cc_oracle as oc
from pymes_amd import _lib
from tests import _lambda_reference as LR
from tests import _rdm2_reference as R

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@functools.lru_cache(maxsize=None)
def _case(no, nv):
    """(inputs, reference blocks): the inputs of the golden file at (3,5), seeded ones elsewhere; they solve nothing."""
    inp = R.golden_rdm2()[2] if (no, nv) == R.GOLDEN_RDM2[1:3] else LR.density_inputs(no, nv, 100 * no + nv)
    ref = R.rdm2_terms(no, *inp)
    for x in ref.values():
        x.setflags(write=False)
    return inp, ref


def _solver(no, inp):
    """A Lambda_CCSD that holds the given (t2, lambda1, lambda2) as if it had solved for them: the density is a formula."""
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    s = Lambda_CCSD(no)
    _, s.t2, s.lambda1, s.lambda2 = inp
    return s


# ---- 1. every block, element by element --------------------------------------------------------------------------------------------
# (17,6): o^2 > 256, the second trip of the tile's block loop; (4,33): v^2 > 1024 and an odd v for the packed pairs; (1,4), (5,1):
# o (o - 1) / 2 = 0 and v (v - 1) / 2 = 0.  abcd is asked for everywhere but at (17,6), where its absence is asserted.
@pytest.mark.parametrize("no,nv", [(3, 5), (6, 17), (17, 6), (4, 33), (1, 4), (5, 1)])
def test_blocks_against_the_reference(gpu_lib, no, nv):
    from pymes_amd.solver.lambda_ccsd import RDM2_NAMES
    inp, ref = _case(no, nv)
    with_abcd = (no, nv) != (17, 6)
    got = _solver(no, inp).rdm2(inp[0], blocks=RDM2_NAMES if with_abcd else None)
    assert set(got) == (set(RDM2_NAMES) if with_abcd else set(RDM2_NAMES) - {"abcd"})
    worst = 0.0
    for nm, x in got.items():
        assert x.shape == ref[nm].shape and x.flags["C_CONTIGUOUS"]
        scale = np.abs(ref[nm]).max()
        err = np.abs(x - ref[nm]).max()
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (nm, err, scale)
    print(no, nv, "largest max |Gamma - reference| / max |reference| over the blocks = %.2e" % worst)
    if (no, nv) == R.GOLDEN_RDM2[1:3]:                        # ... and against the definition itself
        G = oc.split_blocks(no, R.golden_rdm2()[3])
        err = max(np.abs(got[nm] - G[nm]).max() / np.abs(G[nm]).max() for nm in got)
        print(no, nv, "against the recorded definition: %.2e" % err)
        assert err <= 1e-12
    assert np.abs(got["ijab"] - got["abij"].transpose(2, 3, 0, 1)).max() > 1e-3          # not hermitian, not symmetrised


# ---- 2. the device contraction ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator(no, nv):
    rng = np.random.default_rng(7)
    n = no + nv
    W = rng.standard_normal((n, n, n, n))
    W = W + W.transpose(1, 0, 3, 2)                           # W_pqrs = W_qpsr and nothing else
    O = rng.standard_normal((n, n))
    W.setflags(write=False)
    return W, O


def test_expectation2_against_the_lagrangian_6_17(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    no, nv = 6, 17
    inp, ref = _case(no, nv)
    W, O = _operator(no, nv)
    assert np.abs(W - W.transpose(2, 3, 0, 1)).max() > 1.0
    n = no + nv
    want = R.lagrangian(no, np.zeros((n, n)), W, *inp)
    Wb = oc.split_blocks(no, W)
    bound = 1e-12 * sum((np.abs(ref[nm]) * np.abs(Wb[nm])).sum() for nm in ref)
    s = _solver(no, inp)
    val = s.expectation2(W, t1=inp[0])
    print("sum Gamma W = %.15e  L(0, W) = %.15e  difference %.2e  bound %.2e" % (val, want, abs(val - want), bound))
    assert abs(val - want) <= bound
    # the other two forms of W hold the same numbers and go through the same device contraction: identical bits
    assert s.expectation2({nm: np.ascontiguousarray(x) for nm, x in Wb.items()}) == val
    ints = DeviceIntegrals.from_V_pqrs(no, W)
    try:
        assert s.expectation2(ints) == val
        assert s.expectation2(ints) == val                    # (and twice on the same context: the packed rows of W are cached)
    finally:
        ints.ctx.close()
    # with a one-body operator: + sum gamma O (the response density without the reference term)
    gamma = LR.density_terms(no, *inp)
    both = s.expectation2(W, O=O)
    assert abs(both - val - (gamma * O).sum()) <= 1e-12 * (np.abs(gamma) * np.abs(O)).sum() + 4e-16 * abs(val)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------------------
def test_identical_calls_give_identical_bits(gpu_lib):
    from pymes_amd.solver.lambda_ccsd import RDM2_NAMES
    no, nv = 6, 17
    inp, _ = _case(no, nv)
    W, _ = _operator(no, nv)
    s = _solver(no, inp)
    a, b = s.rdm2(inp[0], blocks=RDM2_NAMES), s.rdm2(inp[0], blocks=RDM2_NAMES)
    for nm in RDM2_NAMES:
        assert np.array_equal(a[nm], b[nm]), nm
    assert s.expectation2(W, t1=inp[0]) == s.expectation2(W, t1=inp[0])


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------------
DELTA_E, LAMBDA_R_EPSILON = 1e-12, 1e-8


@pytest.mark.parametrize("eight", [True, False], ids=["hermitian", "exchange-only"])
def test_ccsd_solve_rdm2_4_12(gpu_lib, eight):
    """"density e" = sum gamma f + sum Gamma V is the Lagrangian L(t, lambda) at the returned amplitudes.
    (a) L is linear in lambda, so density e = E(t) + <lambda, R(t)> EXACTLY, with E and R the oracle's energy and residuals at the
        returned (t1, t2): asserted to rounding, 1e-12 x the sum of |density| |integral|.
    (b) Against "ccsd e": with t* the exact solution and dt = t - t*, L(t, lambda) = E(t*) + <dL/dt, dt> + O(dt^2) and dL/dt is the
        Lambda residual, |dL/dt| <= lambda_r_epsilon, while "ccsd e" = E(t) is first order in dt: |E(t) - E(t*)| <= rho / (1 - rho)
        |dE| for an iteration that contracts by rho per pass, and the solve stops at |dE| <= delta_e.  Both solves here gain
        twelve digits in about thirty passes (rho ~ 0.4); rho <= 0.9 gives 10 delta_e.  |dt| <= 1e-3 is far more than a solve
        stopped at delta_e = 1e-12 leaves (dt ~ dE / |eta|).  Bound: 10 delta_e + 1e-3 lambda_r_epsilon = 2e-11."""
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 4, 12
    f, V = LR.random_problem(no, nv, seed=4, eight=eight, scale=0.005 if eight else 0.02)
    if not eight:
        assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-3
    # (a solver object per solve: its DIIS mixer keeps the history of the solve before)
    base = quiet(CCSD(no, delta_e=DELTA_E).solve, f, V, max_iter=300, density=True, lambda_r_epsilon=LAMBDA_R_EPSILON)
    cc = CCSD(no, delta_e=DELTA_E)
    res = quiet(cc.solve, f, V, max_iter=300, density=True, rdm2=True, lambda_r_epsilon=LAMBDA_R_EPSILON)
    assert cc.lambda_solver.converged
    assert set(res) == set(base) | {"rdm2 blocks", "density e"}
    for key, x in base.items():                               # the existing keys, bit for bit
        assert np.array_equal(np.asarray(x), np.asarray(res[key])), key
    if eight:                                                 # rdm2=True implies density=True
        only2 = quiet(CCSD(no, delta_e=DELTA_E).solve, f, V, max_iter=300, rdm2=True, lambda_r_epsilon=LAMBDA_R_EPSILON)
        assert set(only2) == set(res) and only2["density e"] == res["density e"]
    blocks = res["rdm2 blocks"]
    assert "abcd" not in blocks and len(blocks) == 15
    t1, t2, l1, l2 = res["t1"], res["t2"], res["lambda1"], res["lambda2"]
    ref = R.rdm2_terms(no, t1, t2, l1, l2)
    for nm, x in blocks.items():
        assert np.abs(x - ref[nm]).max() <= 1e-12 * np.abs(ref[nm]).max(), nm
    # (a)
    want = R.lagrangian(no, f, V, t1, t2, l1, l2)
    gamma = LR.density_terms(no, t1, t2, l1, l2)
    Vb = oc.split_blocks(no, V)
    rounding = 1e-12 * ((np.abs(gamma) * np.abs(f)).sum() + sum((np.abs(ref[nm]) * np.abs(Vb[nm])).sum() for nm in ref))
    print("density e %.15e  L by the oracle %.15e  difference %.2e  bound %.2e" % (res["density e"], want,
                                                                                  abs(res["density e"] - want), rounding))
    assert abs(res["density e"] - want) <= rounding
    # (b)
    bound = 10.0 * DELTA_E + 1e-3 * LAMBDA_R_EPSILON
    print("density e - ccsd e = %.2e  bound %.2e" % (res["density e"] - res["ccsd e"], bound))
    assert abs(res["density e"] - res["ccsd e"]) <= bound


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_context_usable(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.lambda_ccsd import NOCC_MAX, check_occupied, device_expectation2, device_rdm2
    E = _lib.PymesError
    no, nv = 3, 5
    inp, ref = _case(no, nv)
    f, V = LR.random_problem(no, nv, seed=1)
    with pytest.raises(ValueError, match="rdm2=True.*DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, rdm2=True)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, density=True, rdm2=True)
    with pytest.raises(E, match=r"rdm2: nocc = %d is too large for the LDS tile" % (NOCC_MAX + 1)):
        check_occupied(NOCC_MAX + 1, "rdm2")                  # (the message only: nothing is launched)
    s = _solver(no, inp)
    W, _ = _operator(no, nv)
    good = s.expectation2(W, t1=inp[0])
    with pytest.raises(E, match="W_pqrs = W_qpsr"):
        s.expectation2(W + 1e-6 * np.random.default_rng(0).standard_normal(W.shape))
    with pytest.raises(ValueError, match="unknown block"):
        s.rdm2(inp[0], blocks=("abji",))
    ctx = Context(no, nv)
    try:
        t1, t2, l1, l2 = (ctx.array(x) for x in inp)
        bad = ctx.array(inp[3] + 1e-3 * np.random.default_rng(1).standard_normal(inp[3].shape))
        held = device_rdm2(ctx, t1, t2, l1, l2)
        first = {nm: x.get() for nm, x in held.items()}
        with pytest.raises(E, match="rdm2: lambda2 does not have the exchange symmetry"):
            device_rdm2(ctx, t1, t2, l1, bad)
        with pytest.raises(E, match="rdm2: t2 does not have the exchange symmetry"):
            device_rdm2(ctx, t1, bad, l1, l2)
        with pytest.raises(E, match="rdm2: output aliases input"):
            device_rdm2(ctx, t1, t2, l1, l2, blocks=("abij",), out={"abij": l2})
        with pytest.raises(E, match="two outputs are the same array"):
            x = ctx.empty(ctx.block_shape("iajb"))
            device_rdm2(ctx, t1, t2, l1, l2, blocks=("iajb", "iabj"), out={"iajb": x, "iabj": x.reshape(*ctx.block_shape("iabj"))})
        ptrs = (C.c_void_p * 16)()
        ptrs[11] = x.ptr
        with pytest.raises(E, match="'aibc' is the image of 'iabc'"):
            ctx.lib.call("pymes_rdm2", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(l1.ptr),
                         C.c_void_p(l2.ptr), 1 << 11, ptrs)
        with pytest.raises(E, match="operator block .* is not set"):
            device_expectation2(ctx, t1, t2, l1, l2)
        ctx.graph_begin()
        try:
            with pytest.raises(E, match="rdm2 while a launch graph is being recorded"):
                device_rdm2(ctx, t1, t2, l1, l2, out=held)        # (outputs that exist: nothing is allocated while recording)
            with pytest.raises(E, match="rdm2_expectation while a launch graph is being recorded"):
                device_expectation2(ctx, t1, t2, l1, l2)
        finally:
            ctx.graph_abort()
        again = {nm: x.get() for nm, x in device_rdm2(ctx, t1, t2, l1, l2).items()}          # the context is still usable
        for nm in first:
            assert np.array_equal(first[nm], again[nm]), nm
            assert np.abs(first[nm] - ref[nm]).max() <= 1e-12 * np.abs(ref[nm]).max()
    finally:
        ctx.close()
    assert s.expectation2(W) == good
