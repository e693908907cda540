"""CPU: the host side of IP- / EA-EOM-CCSD through the host simulator (tests/hostsim): the C entries and their ctypes table,
the hoist (contraction planner, scratch pool), the refusals by name and their bookkeeping.  The four gfx950 kernels have no CPU
stand-in: apply, diagonals and correction refuse in this backend, by name (the GPU tests cover them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import random_case
from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _ipea_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("prepare", "flags", "apply", "diagonals", "correction", "destroy")


def _live(lib):
    n = C.c_int64()
    lib.call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _case(no, nv, seed=3):
    f, V, _, t2 = random_case(no, nv, seed=seed)
    return f, R.symmetrise(V), t2


def _context(lib, no, nv, Vb, names):
    ctx = Context(no, nv, lib=lib)
    for name in names:
        ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
    return ctx


def test_entries_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    for e in ENTRIES:
        name = "pymes_ipea_sigma_" + e
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    assert "PYMES_IPEA_IP 0" in header and "PYMES_IPEA_EA 1" in header
    for doc, word in (("README.md", "IP_EOM_CCSD"), ("DESIGN.md", "## 8c. IP- and EA-EOM-CCSD"),
                      ("INTEGRATION.md", "pymes_ipea_sigma_prepare")):
        assert word in open(os.path.join(ROOT, doc)).read()


def test_block_lists_match_the_term_tables():
    from pymes_amd.solver.eom_ip_ea import EA_EOM_CCSD, IP_EOM_CCSD
    assert sorted(IP_EOM_CCSD.BLOCKS) == sorted(R.BLOCKS["ip"]) and sorted(EA_EOM_CCSD.BLOCKS) == sorted(R.BLOCKS["ea"])
    assert "abcd" not in IP_EOM_CCSD.BLOCKS


@pytest.mark.parametrize("kind", ["ip", "ea"])
def test_prepare_hoists_and_the_kernels_refuse_by_name(hostsim_lib, kind):
    from pymes_amd.solver import eom_ip_ea as M
    K = M.KIND_IP if kind == "ip" else M.KIND_EA
    no, nv = 3, 4
    f, V, t2 = _case(no, nv)
    Vb = oc.split_blocks(no, V)
    before = _live(hostsim_lib)
    ctx = _context(hostsim_lib, no, nv, Vb, M.IPEASigma.BLOCKS[K])
    try:
        sig = M.IPEASigma(ctx, K, f, ctx.array(t2))
        flags = C.c_int()
        ctx.lib.call("pymes_ipea_sigma_flags", sig._h, C.byref(flags))
        assert flags.value == K
        assert (sig.n1, sig.n2) == tuple(int(np.prod(s)) for s in R.shapes(kind, no, nv)) and sig.off2 % 32 == 0
        r1, r2 = ctx.zeros(sig.shape1), ctx.zeros(sig.shape2)
        with pytest.raises(_lib.PymesError, match="ipea_pack: not available in this backend"):
            sig.apply_many([r1], [r2])
        with pytest.raises(_lib.PymesError, match="ipea_diagonals: not available in this backend"):
            sig.diagonals()
        sig.close()
        with pytest.raises(_lib.PymesError, match="destroyed"):
            sig.apply_many([r1], [r2])
        sig = M.IPEASigma(ctx, K, f, ctx.array(t2))          # the second prepare finds the pooled buffers of the first
    finally:
        ctx.close()
    with pytest.raises(_lib.PymesError, match="destroyed"):
        sig.diagonals()
    sig.close()
    assert _live(hostsim_lib) == before


@pytest.mark.parametrize("kind", ["ip", "ea"])
def test_refusals_name_their_reason_and_leave_nothing_behind(hostsim_lib, kind):
    from pymes_amd.solver import eom_ip_ea as M
    K = M.KIND_IP if kind == "ip" else M.KIND_EA
    no, nv = 2, 3
    f, V, t2 = _case(no, nv, seed=5)
    Vb = oc.split_blocks(no, V)
    names = M.IPEASigma.BLOCKS[K]
    before = _live(hostsim_lib)
    ctx = _context(hostsim_lib, no, nv, Vb, [n for n in names if n != "iajb"])
    try:
        d2 = ctx.array(t2)
        held = _live(hostsim_lib)
        with pytest.raises(_lib.PymesError, match="'iajb'"):
            M.IPEASigma(ctx, K, f, d2)
        assert _live(hostsim_lib) == held
        rng = np.random.default_rng(1)
        ctx.set_V_block("iajb", np.ascontiguousarray(Vb["iajb"]))
        ctx.set_V_block("ijab", np.ascontiguousarray(Vb["ijab"] + 1e-3 * rng.standard_normal(Vb["ijab"].shape)))
        held = _live(hostsim_lib)
        with pytest.raises(_lib.PymesError, match="V_pqrs = V_qpsr"):
            M.IPEASigma(ctx, K, f, d2)
        ctx.set_V_block("ijab", np.ascontiguousarray(Vb["ijab"]))
        bad = ctx.array(t2 + 1e-3 * rng.standard_normal(t2.shape))
        held = _live(hostsim_lib)
        with pytest.raises(_lib.PymesError, match="T_abij = T_baji"):
            M.IPEASigma(ctx, K, f, bad)
        assert _live(hostsim_lib) == held
        h = C.c_void_p()
        with pytest.raises(_lib.PymesError, match="kind"):
            ctx.lib.call("pymes_ipea_sigma_prepare", ctx.handle, _lib.host_ptr(np.ascontiguousarray(f)), C.c_void_p(d2.ptr), 0, 7,
                         C.byref(h))
        with pytest.raises(ValueError, match=r"\[n, n\]"):
            M.IPEASigma(ctx, K, f[:-1, :-1], d2)
    finally:
        ctx.close()
    assert _live(hostsim_lib) == before


def test_ccsd_solve_refuses_dcsd_amplitudes():
    from pymes_amd.solver.ccsd import CCSD
    f, V, _ = _case(2, 3)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(2, is_dcsd=True).solve(f, V, ip_roots=1)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(2, is_dcsd=True).solve(f, V, ea_roots=2)
