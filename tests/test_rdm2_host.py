"""CPU: the host side of the two-particle density through the host simulator (tests/hostsim): the product sequence of lambda_rdm2
against the numpy reference for every block that needs no kernel, the C entries and their ctypes table, the refusals by name and
their bookkeeping.  The gfx950 kernels (rdm2_assemble for ijab, rdm2_contract for expectation2) have no CPU stand-in: the weak
definitions in the engine refuse by name, and the GPU tests cover them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _lambda_reference as LR
from tests import _rdm2_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pymes_rdm2", "pymes_rdm2_expectation")


def _live(lib):
    n = C.c_int64()
    lib.call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def test_entries_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and name in integration
    for doc, word in (("README.md", "expectation2"), ("DESIGN.md", "## 8g. The two-particle density"), ("INTEGRATION.md", "rdm2=True")):
        assert word in open(os.path.join(ROOT, doc)).read()
    api = open(os.path.join(ROOT, "pymes_amd", "csrc", "device_api.h")).read()
    for fn in ("void rdm2_assemble(", "void rdm2_contract(", "void rdm2_contract_packed(", "void rdm2_contract_finish("):
        assert fn in api
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    lambda_section = design.split("## 8d. ")[1].split("## 8e. ")[0]
    assert "wo-particle density" not in lambda_section.split("**Out of scope.**")[1]          # struck from that list


@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5), (1, 4), (5, 1)])
def test_product_sequence_against_the_reference(hostsim_lib, no, nv):
    from pymes_amd.solver.lambda_ccsd import RDM2_NAMES, RDM2_STORED, device_expectation2, device_rdm2
    inp = LR.density_inputs(no, nv, 5)
    ref = R.rdm2_terms(no, *inp)
    n = no + nv
    W = np.random.default_rng(1).standard_normal((n, n, n, n))
    W = W + W.transpose(1, 0, 3, 2)
    before = _live(hostsim_lib)
    ctx = Context(no, nv, lib=hostsim_lib)
    try:
        dev = [ctx.array(x) for x in inp]
        names = tuple(nm for nm in RDM2_NAMES if nm != "ijab")
        got = device_rdm2(ctx, *dev, blocks=names)
        assert tuple(got) == tuple(nm for nm in RDM2_STORED if nm != "ijab")       # the images come back as their stored blocks
        for nm, x in got.items():
            assert np.abs(x.get() - ref[nm]).max() <= 1e-13 * max(1.0, np.abs(ref[nm]).max()), nm
        assert "abcd" not in device_rdm2(ctx, *dev, blocks=[nm for nm in names if nm != "abcd"])
        with pytest.raises(_lib.PymesError, match="rdm2_assemble: not available in this backend"):
            device_rdm2(ctx, *dev, blocks=("ijab",))
        ctx.set_V_pqrs(W)
        with pytest.raises(_lib.PymesError, match="rdm2_contract: not available in this backend"):
            device_expectation2(ctx, *dev)
        del dev, got, x
    finally:
        ctx.close()
    assert _live(hostsim_lib) == before


def test_refusals_name_their_reason_and_leave_nothing_behind(hostsim_lib):
    from pymes_amd.solver.lambda_ccsd import device_expectation2, device_rdm2
    E = _lib.PymesError
    no, nv = 2, 3
    inp = LR.density_inputs(no, nv, 9)
    n = no + nv
    before = _live(hostsim_lib)
    ctx = Context(no, nv, lib=hostsim_lib)
    try:
        t1, t2, l1, l2 = (ctx.array(x) for x in inp)
        bad = ctx.array(inp[3] + 1e-3 * np.random.default_rng(1).standard_normal(inp[3].shape))
        names = ("klij", "ijka", "iajk", "iajb", "iabj", "iabc", "abij", "abic")       # (ijab needs the kernel)
        out = device_rdm2(ctx, t1, t2, l1, l2, blocks=names)
        first = {nm: x.get() for nm, x in out.items()}
        ctx.trim()
        held = _live(hostsim_lib)
        with pytest.raises(E, match="rdm2: lambda2 does not have the exchange symmetry"):
            device_rdm2(ctx, t1, t2, l1, bad, blocks=names, out=out)
        with pytest.raises(E, match="rdm2: t2 does not have the exchange symmetry"):
            device_rdm2(ctx, t1, bad, l1, l2, blocks=names, out=out)
        with pytest.raises(E, match="rdm2: output aliases input"):
            device_rdm2(ctx, t1, t2, l1, l2, blocks=("abij",), out={"abij": t2})
        ptrs = (C.c_void_p * 16)()
        ptrs[2] = out["ijka"].ptr
        args = [C.c_void_p(x.ptr) for x in (t1, t2, l1, l2)]
        with pytest.raises(E, match="'ijak' is the image of 'ijka'"):
            ctx.lib.call("pymes_rdm2", ctx.handle, *args, 1 << 2, ptrs)
        with pytest.raises(E, match="names no block"):
            ctx.lib.call("pymes_rdm2", ctx.handle, *args, 0, ptrs)
        with pytest.raises(E, match="null output for block 'klij'"):
            ctx.lib.call("pymes_rdm2", ctx.handle, *args, 1, ptrs)
        with pytest.raises(E, match="operator block 'klij' is not set"):
            device_expectation2(ctx, t1, t2, l1, l2)
        assert _live(hostsim_lib) == held                     # nothing was allocated for a refused call
        W = np.random.default_rng(3).standard_normal((n, n, n, n))
        ctx.set_V_pqrs(W)
        held = _live(hostsim_lib)                             # (the sixteen blocks of W)
        with pytest.raises(E, match="rdm2_expectation: the operator does not have the symmetry W_pqrs = W_qpsr"):
            device_expectation2(ctx, t1, t2, l1, l2)
        assert _live(hostsim_lib) == held                     # nothing was allocated for a refused call
        again = device_rdm2(ctx, t1, t2, l1, l2, blocks=names, out=out)
        for nm in first:
            assert np.array_equal(first[nm], again[nm].get())
        del t1, t2, l1, l2, bad, out, again, args
    finally:
        ctx.close()
    assert _live(hostsim_lib) == before
    shard = Context(no, nv, lib=hostsim_lib, shard=(0, 2))
    try:
        dev = [shard.array(x) for x in inp]
        got = device_rdm2(shard, *dev, blocks=("iajb", "iabc", "klij"))      # the density reads no integrals: a sharded context is served
        ref = R.rdm2_terms(no, *inp)
        assert all(np.abs(x.get() - ref[nm]).max() < 1e-13 for nm, x in got.items())
        with pytest.raises(E, match="rdm2_expectation: not available with integral sharding"):
            device_expectation2(shard, *dev)
        del dev, got
    finally:
        shard.close()


def test_ccsd_solve_refuses_dcsd_before_any_work():
    from pymes_amd.solver.ccsd import CCSD
    f, V = LR.random_problem(2, 3, seed=1)
    with pytest.raises(ValueError, match="rdm2=True.*DCSD"):
        CCSD(2, is_dcsd=True).solve(f, V, rdm2=True)
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(2, shard_integrals=True).solve(f, V, rdm2=True)


def test_python_refusals_without_a_device():
    from pymes_amd.solver.lambda_ccsd import NOCC_MAX, Lambda_CCSD, check_occupied
    with pytest.raises(_lib.PymesError, match="rdm2: nocc = %d is too large" % (NOCC_MAX + 1)):
        check_occupied(NOCC_MAX + 1, "rdm2")
    s = Lambda_CCSD(2)
    with pytest.raises(RuntimeError, match="rdm2: needs a finished solve"):
        s.rdm2(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="unknown block"):
        s.rdm2(np.zeros((3, 2)), blocks=("abcx",))
    with pytest.raises(RuntimeError, match="expectation2: pass t1"):
        s.expectation2(np.zeros((5, 5, 5, 5)))
