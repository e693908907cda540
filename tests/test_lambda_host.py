"""CPU: the host side of the left sigma, the Lambda step and the one-particle density through the host simulator
(tests/hostsim): the C entries and their ctypes table, the refusals by name and their bookkeeping.  The two gfx950 kernels have
no CPU stand-in: the adjoint build runs its products here and refuses at the assembly, by name (the GPU tests cover the rest)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import cc_oracle as oc
from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _lambda_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pymes_eom_sigma_apply_left", "pymes_lambda_step", "pymes_rdm1")


def _live(lib):
    n = C.c_int64()
    lib.call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _case(no, nv, seed=3):
    rng = np.random.default_rng(seed)
    n = no + nv
    V = 0.1 * rng.standard_normal((n, n, n, n))
    V = V + V.transpose(1, 0, 3, 2)
    f = np.diag(np.concatenate([-1.0 - rng.random(no), 1.0 + rng.random(nv)])) + 0.05 * rng.standard_normal((n, n))
    t2 = 0.1 * R.symd(rng.standard_normal((nv, nv, no, no)))
    return f, oc.split_blocks(no, V), t2, rng.standard_normal((nv, no)), R.symd(rng.standard_normal((nv, nv, no, no)))


def _context(lib, no, nv, Vb, names):
    ctx = Context(no, nv, lib=lib)
    for name in names:
        ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
    return ctx


def test_entries_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and name in integration
    for doc, word in (("README.md", "Lambda_CCSD"), ("DESIGN.md", "## 8d. CCSD Lambda equations"),
                      ("INTEGRATION.md", "density=True")):
        assert word in open(os.path.join(ROOT, doc)).read()
    api = open(os.path.join(ROOT, "pymes_amd", "csrc", "device_api.h")).read()
    assert "void lambda_assemble(" in api and "void rdm1_assemble(" in api


def test_the_solver_reads_the_blocks_of_the_sigma_build():
    from pymes_amd.solver.eom_ccsd import _Sigma
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD, LeftSigma
    used = {nm for terms in (R.LEFT_SINGLES_TERMS, R.LEFT_DOUBLES_TERMS_P, R.LEFT_DOUBLES_TERMS_N) for row in terms
            for nm in row[2] if len(nm) == 4}
    assert used == set(_Sigma.BLOCKS) == set(Lambda_CCSD.BLOCKS) == set(LeftSigma.BLOCKS)


def test_the_kernel_stubs_refuse_by_name(hostsim_lib):
    from pymes_amd.solver.lambda_ccsd import LeftSigma, device_rdm1
    no, nv = 3, 4                                      # (the simulator has the fused pair kernels up to no = 3)
    f, Vb, t2, l1, l2 = _case(no, nv)
    before = _live(hostsim_lib)
    ctx = _context(hostsim_lib, no, nv, Vb, LeftSigma.BLOCKS)
    try:
        sig = LeftSigma(ctx, f, ctx.array(t2))
        a1, a2 = ctx.array(l1), ctx.array(l2)
        o1, o2, e1, e2 = ctx.empty(a1.shape), ctx.empty(a2.shape), ctx.empty(a1.shape), ctx.empty(a2.shape)
        eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
        with pytest.raises(_lib.PymesError, match="lambda_assemble: not available in this backend"):
            sig.apply_left_many([a1], [a2], out1=[o1], out2=[o2])
        with pytest.raises(_lib.PymesError, match="lambda_assemble: not available in this backend"):
            sig.lambda_step((a1, a2), eps_o, eps_v, 0.0, (o1, o2), (e1, e2))
        with pytest.raises(_lib.PymesError, match="lambda_assemble: not available in this backend"):
            sig.lambda_step(None, eps_o, eps_v, 0.0, (o1, o2), (e1, e2), start=True)
        with pytest.raises(_lib.PymesError, match="rdm1_assemble: not available in this backend"):
            device_rdm1(ctx, ctx.array(l1), ctx.array(t2), a1, a2)
        s1, s2 = [x.get() for x in sig.apply(a1, a2)]          # the right build on the same handle still runs
        assert np.abs(s2 - R.eo.sigma_doubles(no, f, Vb, l1, l2, t2)).max() < 1e-11 * np.abs(s2).max()
        sig.close()
        with pytest.raises(_lib.PymesError, match="destroyed"):
            sig.apply_left(a1, a2)
    finally:
        ctx.close()
    assert _live(hostsim_lib) == before


def test_refusals_name_their_reason_and_leave_nothing_behind(hostsim_lib):
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    E = _lib.PymesError
    no, nv = 2, 3
    f, Vb, t2, l1, l2 = _case(no, nv, seed=5)
    before = _live(hostsim_lib)
    ctx = _context(hostsim_lib, no, nv, Vb, [n for n in LeftSigma.BLOCKS if n != "iajb"])
    try:
        d2 = ctx.array(t2)
        held = _live(hostsim_lib)
        with pytest.raises(E, match="'iajb'"):
            LeftSigma(ctx, f, d2)
        ctx.trim()                       # (the hoist of the right build had begun: its buffers are in the context's pool)
        assert _live(hostsim_lib) == held
        ctx.set_V_block("iajb", np.ascontiguousarray(Vb["iajb"]))
        sig = LeftSigma(ctx, f, d2)
        a1, a2 = ctx.array(l1), ctx.array(l2)
        bad = ctx.array(l2 + 1e-3 * np.random.default_rng(1).standard_normal(l2.shape))
        o1, o2, e1, e2 = ctx.empty(a1.shape), ctx.empty(a2.shape), ctx.empty(a1.shape), ctx.empty(a2.shape)
        eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
        held = _live(hostsim_lib)
        with pytest.raises(E, match="apply_left: the left doubles do not have the exchange symmetry"):
            sig.apply_left_many([a1], [bad], out1=[o1], out2=[o2])
        with pytest.raises(E, match="lambda_step: lambda2 does not have the exchange symmetry"):
            sig.lambda_step((a1, bad), eps_o, eps_v, 0.0, (o1, o2), (e1, e2))
        with pytest.raises(E, match="output aliases input"):
            sig.apply_left_many([a1], [a2], out1=[a1], out2=[o2])
        with pytest.raises(E, match="error vector aliases"):
            sig.lambda_step((a1, a2), eps_o, eps_v, 0.0, (o1, o2), (o1, e2))
        with pytest.raises(E, match="null pointer: lam1"):
            ctx.lib.call("pymes_lambda_step", sig._h, None, None, _lib.host_ptr(eps_o), _lib.host_ptr(eps_v), 0.0, 1.0, 0, 0,
                         C.c_void_p(o1.ptr), C.c_void_p(o2.ptr), C.c_void_p(e1.ptr), C.c_void_p(e2.ptr),
                         _lib.host_ptr(np.zeros(1)))
        with pytest.raises(ValueError, match=r"\[no\] / \[nv\]"):
            sig.lambda_step((a1, a2), eps_v, eps_o, 0.0, (o1, o2), (e1, e2))
        assert _live(hostsim_lib) == held
        if ctx.graphs_supported():
            ctx.graph_begin()
            try:
                with pytest.raises(E, match="eom_sigma_apply_left while a launch graph is being recorded"):
                    sig.apply_left_many([a1], [a2], out1=[o1], out2=[o2])
                with pytest.raises(E, match="rdm1 while a launch graph is being recorded"):
                    from pymes_amd.solver.lambda_ccsd import device_rdm1
                    device_rdm1(ctx, a1, d2, a1, a2)
            finally:
                ctx.graph_abort()
            assert _live(hostsim_lib) == held
        sig.close()
    finally:
        ctx.close()
    assert _live(hostsim_lib) == before


def test_ccsd_solve_refuses_dcsd_and_sharded_integrals_before_any_work():
    from pymes_amd.solver.ccsd import CCSD
    f, V = R.random_problem(2, 3, seed=1)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(2, is_dcsd=True).solve(f, V, density=True)
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(2, shard_integrals=True).solve(f, V, density=True)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(2, is_dcsd=True).solve(f, V, density=True, frozen_core=1)
