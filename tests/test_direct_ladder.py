"""Factor-direct particle ladder (include/pymes_amd.h, pymes_set_integral_direct) on the host simulator, gemm row builder: a
context that holds the virtual-virtual factors and no V_abcd in any form gives the per-iteration energies of the stored
solve, builds every chunk of rows as the numpy packing does, holds exactly v^4 doubles less plus B_vv and its chunk buffers,
and refuses by name every path that needs the full, dressed or stored block."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from tests.test_shard_integrals import _energies, _pitch, pack_rows

SHAPES = ((5, 14), (4, 12), (3, 14), (3, 12))
CAP = 31          # rows per chunk: not a triangular number (edges inside an a-row); 78 = 31 + 31 + 16, 105 = 3 x 31 + 12


def _chunk_bytes(nv, cap=CAP):
    """The budget that gives `cap` rows per chunk with the gemm builder: a row of V^+ / V^- at the ladder pitches plus one
    plane V[a,b,:,:] each."""
    return cap * 8 * (_pitch(nv * (nv + 1) // 2) + _pitch(nv * (nv - 1) // 2) + nv * nv)


def _bvv_bytes(nv, naux):
    """B_vv [nv][naux up to 8][nv up to 64] (device_api.h, direct_rows_fused)."""
    return 8 * nv * ((naux + 7) // 8 * 8) * ((nv + 63) // 64 * 64)


@pytest.fixture
def sim(hostsim_lib, monkeypatch):
    monkeypatch.setattr(_lib, "_default", hostsim_lib)
    for name in ("PYMES_DIRECT_BUILDER", "PYMES_DIRECT_CHUNK_BYTES", "PYMES_LADDER_DRESS", "PYMES_FORCE_SHARDED"):
        monkeypatch.delenv(name, raising=False)
    return hostsim_lib


def _solve(kind, no, f, ints):
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd import CCSD
    if kind in ("ccsd", "dcsd"):
        s = CCSD(no, delta_e=1e-10, is_dcsd=kind == "dcsd")
    else:
        s = CCD(no, delta_e=1e-10, is_dcd=kind == "dcd")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        s.solve(f, ints)
    return _energies(buf.getvalue())


@pytest.mark.parametrize("no,nv", SHAPES)
def test_direct_energies_match_stored(sim, monkeypatch, no, nv):
    f, _, B, _ = synthetic_case(no, nv, seed=3, scale=0.3)
    monkeypatch.setenv("PYMES_DIRECT_CHUNK_BYTES", str(_chunk_bytes(nv)))
    for kind in ("ccsd", "dcsd", "ccd", "dcd"):
        stored = DeviceIntegrals.from_factors(no, B, lib=sim)
        direct = DeviceIntegrals.from_factors(no, B, direct=True, lib=sim)
        try:
            assert direct.direct and not stored.direct
            info = direct.ctx.direct_info()
            npp = nv * (nv + 1) // 2
            assert info["chunk_rows"] == CAP and -(-npp // CAP) >= 3 and npp % CAP != 0 and info["builder"] == "gemm"
            ref = _solve(kind, no, f, stored)
            got = _solve(kind, no, f, direct)
        finally:
            stored.ctx.close()
            direct.ctx.close()
        print(kind, no, nv, len(ref), float(np.abs(np.array(ref) - np.array(got)).max()))
        assert len(ref) == len(got) and len(ref) > 3, (kind, ref, got)
        assert np.abs(np.array(ref) - np.array(got)).max() < 1e-12, (kind, ref, got)


@pytest.mark.parametrize("no,nv", SHAPES)
def test_chunk_rows_match_numpy_packing_and_bytes(sim, no, nv):
    _, V, B, _ = synthetic_case(no, nv, seed=3, scale=0.3)
    n, naux, npp = no + nv, B.shape[0], nv * (nv + 1) // 2
    ints = DeviceIntegrals.from_factors(no, B, direct=_chunk_bytes(nv), lib=sim)      # (the budget as the argument)
    rep = Context(no, nv, lib=sim)
    try:
        ctx = ints.ctx
        assert ctx.direct_info()["chunk_rows"] == CAP
        worst = 0.0
        for c0 in range(0, npp, CAP):
            c1 = min(npp, c0 + CAP)
            P, M = ctx.direct_rows(c0, c1)
            Pr, Mr = pack_rows(V[no:, no:, no:, no:], c0, c1)
            worst = max(worst, float(np.abs(P - Pr).max()), float(np.abs(M - Mr).max(initial=0.0)))
        print("rows", no, nv, worst)
        assert worst < 1e-12
        with pytest.raises(_lib.PymesError, match="bad chunk"):
            ctx.direct_rows(0, CAP + 1)
        # integral bytes: the replicated count minus v^4 doubles plus B_vv and the chunk buffers, exactly
        rep.set_V_from_factors(B)
        assert rep.integral_bytes() == 8 * n ** 4
        assert ctx.integral_bytes() == rep.integral_bytes() - 8 * nv ** 4 + _bvv_bytes(nv, naux) + _chunk_bytes(nv)
        info = ctx.direct_info()
        assert (info["naux"], info["bvv_bytes"], info["chunk_buffer_bytes"]) == (naux, _bvv_bytes(nv, naux), _chunk_bytes(nv))
        # the other 15 blocks as the stored route forms them
        for name in ("ijab", "iabc", "aibc", "klij", "abij"):
            assert np.array_equal(ctx.V_block(name).get(), rep.V_block(name).get())
    finally:
        rep.close()
        ints.ctx.close()


def test_one_row_budget_and_default_budget(sim):
    """A budget below one row still holds one row per chunk; the default is 1 GiB, capped at all rows."""
    no, nv = 2, 6
    _, V, B, _ = synthetic_case(no, nv, seed=2, scale=0.3)
    ints = DeviceIntegrals.from_factors(no, B, direct=8, lib=sim)
    try:
        assert ints.ctx.direct_info()["chunk_rows"] == 1
        for r in (0, 2, 5, 20):           # (a == b rows: 0, 2, 5, 20)
            P, M = ints.ctx.direct_rows(r, r + 1)
            Pr, Mr = pack_rows(V[no:, no:, no:, no:], r, r + 1)
            assert np.abs(P - Pr).max() < 1e-12 and np.abs(M - Mr).max() < 1e-12 and not M.any()
    finally:
        ints.ctx.close()
    ints = DeviceIntegrals.from_factors(no, B, direct=True, lib=sim)
    try:
        assert ints.ctx.direct_info()["chunk_rows"] == nv * (nv + 1) // 2
    finally:
        ints.ctx.close()


def test_refusals(sim, monkeypatch):
    no, nv = 3, 7
    f, V, B, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    E = _lib.PymesError
    ctx = Context(no, nv, lib=sim, direct=True)
    for name, call in {"set_V_pqrs": lambda: ctx.set_V_pqrs(V),
                       "set_V_block": lambda: ctx.set_V_block("ijab", np.ascontiguousarray(V[:no, :no, no:, no:])),
                       "shard after direct": lambda: sim.call("pymes_set_integral_shard", ctx.handle, 0, 2),
                       "direct twice": lambda: sim.call("pymes_set_integral_direct", ctx.handle, 0),
                       "rows before the factors": lambda: ctx.direct_rows(0, 1)}.items():
        with pytest.raises(E, match="factor-direct"):
            call()
        assert name
    ctx.set_V_from_factors(B)
    ctx.set_orbital_energies(f.diagonal()[:no].copy(), f.diagonal()[no:].copy())
    t2, r2 = ctx.zeros((nv, nv, no, no)), ctx.zeros((nv, nv, no, no))
    t1 = ctx.zeros((nv, no))
    fd = ctx.array(f)
    npp = nv * (nv + 1) // 2
    L = ctx.zeros((npp, no * no))
    fh = np.ascontiguousarray(f)
    h = C.c_void_p()
    val = C.c_double()
    rep = Context(no, nv, lib=sim)
    rep.set_V_from_factors(B)
    dst = Context(no, nv - 1, lib=sim)
    ddst = Context(no, nv - 1, lib=sim, direct=True)
    Cm = np.ascontiguousarray(np.eye(nv)[:, :nv - 1])
    refused = {
        "block pointer": lambda: ctx.V_block("abcd"),
        "dressed block pointer": lambda: ctx.V_block("abcd", dressed=True),
        "ladder": lambda: ctx.ladder(t2, r2, 0, nv),
        "doubles_residual": lambda: ctx.doubles_residual(fd, t2, r2),
        "doubles_residual dressed": lambda: ctx.doubles_residual(fd, t2, r2, dressed=True, sym_ladder=True, sym_rings=True),
        "dress_abcd_rows": lambda: ctx.dress_abcd_rows(t1, 0, nv),
        "dress_V abcd": lambda: ctx.dress_V(t1, ("abcd",)),
        "ladder_sym dressed": lambda: ctx.ladder_sym(t2, L, 0, npp, dressed=True),
        "ladder_sym_multi": lambda: ctx.ladder_sym_multi([t2], ctx.zeros((1, npp, no * no))),
        "EE sigma": lambda: sim.call("pymes_eom_sigma_prepare", ctx.handle, _lib.host_ptr(fh), C.c_void_p(t2.ptr), 0, C.byref(h)),
        "EA sigma": lambda: sim.call("pymes_ipea_sigma_prepare", ctx.handle, _lib.host_ptr(fh), C.c_void_p(t2.ptr), 0, 1,
                                     C.byref(h)),
        "EOM diagonals": lambda: sim.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(fh), C.c_void_p(t2.ptr), 0,
                                          C.c_void_p(t1.ptr), C.c_void_p(r2.ptr)),
        "rdm2_expectation": lambda: sim.call("pymes_rdm2_expectation", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr),
                                             C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.byref(val)),
        "derive from direct": lambda: sim.call("pymes_derive_context", ctx.handle, dst.handle, 0, _lib.host_ptr(Cm), nv - 1),
        "derive into direct": lambda: sim.call("pymes_derive_context", rep.handle, ddst.handle, 0, _lib.host_ptr(Cm), nv - 1),
        "direct after set_V": lambda: sim.call("pymes_set_integral_direct", rep.handle, 0),
    }
    for name, call in refused.items():
        with pytest.raises(E, match=r"factor-direct|before any pymes_set_V"):
            call()
        assert name  # (the label names the case in a failure's traceback)
    for c in (rep, dst, ddst):
        c.close()
    # ... while the undressed pair-packed ladders (CCD / DCD, hole = 0/1/2) and the symmetric residual are served
    for hole in (0, 1, 2):
        ctx.ladder_sym(t2, L, 0, npp, hole_ladder=hole)
    ctx.doubles_residual(fd, t2, r2, sym_ladder=True, sym_rings=True)
    # the bra dressing of stored rows is no option of this mode
    monkeypatch.setenv("PYMES_LADDER_DRESS", "1")
    with pytest.raises(E, match="factor-direct"):
        ctx.ccsd_residuals(fd, t1, t2, ctx.zeros((nv, no)), r2)
    monkeypatch.delenv("PYMES_LADDER_DRESS")
    ctx.ccsd_residuals(fd, t1, t2, ctx.zeros((nv, no)), r2)
    ctx.close()
    # direct with integral sharding, either way round; the fused builder is the product library's; unknown builders
    with pytest.raises(E, match="integral sharding"):
        Context(no, nv, lib=sim, shard=(0, 2), direct=True)
    monkeypatch.setenv("PYMES_DIRECT_BUILDER", "fused")
    with pytest.raises(E, match="factor-direct mode is not available in this backend"):
        Context(no, nv, lib=sim, direct=True)
    monkeypatch.setenv("PYMES_DIRECT_BUILDER", "triton")
    with pytest.raises(E, match="gemm or fused"):
        Context(no, nv, lib=sim, direct=True)
    monkeypatch.setenv("PYMES_DIRECT_BUILDER", "gemm")
    Context(no, nv, lib=sim, direct=True).close()
    with pytest.raises(E, match="chunk_bytes"):
        Context(no, nv, lib=sim, direct=-5)
    with pytest.raises(E, match="not factor-direct"):
        Context(no, nv, lib=sim).direct_info()


def test_solver_refusals_before_upload(sim):
    """density / ee_roots / dyson / ea_roots / triples="lambda" on factor-direct integrals: refused by name before anything is
    uploaded or dressed; frozen natural orbitals are not derived from such a context."""
    from pymes_amd.solver import fno
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 2, 5
    f, _, B, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    ints = DeviceIntegrals.from_factors(no, B, direct=True, lib=sim)
    try:
        before = ints.ctx.integral_bytes()
        for kw in (dict(density=True), dict(rdm2=True), dict(ee_roots=1), dict(ip_roots=1, dyson=True), dict(ea_roots=1),
                   dict(triples="lambda"), dict(frozen_core=1)):
            with pytest.raises(ValueError, match="direct=True|factor-direct"):
                with contextlib.redirect_stdout(io.StringIO()):
                    CCSD(no).solve(f, ints, **kw)
        with pytest.raises(ValueError, match="factors"):
            fno.truncate(no, f, np.zeros((no + nv,) * 4), n_frozen=1, direct=True, lib=sim)
        assert ints.ctx.integral_bytes() == before
    finally:
        ints.ctx.close()
