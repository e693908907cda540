"""Factor-direct particle ladder (include/pymes_amd.h, pymes_set_integral_direct) on the host simulator, gemm row builder: a
context that holds the virtual-virtual factors and no V_abcd in any form gives the per-iteration energies of the stored
solve, builds every chunk of rows as the numpy packing does, holds exactly v^4 doubles less plus B_vv and its chunk buffers,
and refuses by name every path that needs the full, dressed or stored block."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd import dist as pdist
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from tests.test_shard_integrals import _energies, _pitch, pack_rows

SHAPES = ((5, 14), (4, 12), (3, 14), (3, 12))
CAP = 31          # rows per chunk: not a triangular number (edges inside an a-row); 78 = 31 + 31 + 16, 105 = 3 x 31 + 12


def _row_bytes(nv, builder="gemm"):
    """Chunk budget per row: V^+ / V^- at the ladder pitches, plus one plane V[a,b,:,:] for the gemm builder."""
    return 8 * (_pitch(nv * (nv + 1) // 2) + _pitch(nv * (nv - 1) // 2) + (nv * nv if builder == "gemm" else 0))


def _chunk_bytes(nv, cap=CAP):
    """The budget that gives `cap` rows per chunk with the gemm builder: a row of V^+ / V^- at the ladder pitches plus one
    plane V[a,b,:,:] each."""
    return cap * _row_bytes(nv, "gemm")


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


# (no, nv, seed): the shapes of test_sharded_residual_simulated_ranks (test_gpu_cc.py) and the degenerate pair shapes — no
# antisymmetric occupied pair (no = 1), no antisymmetric virtual pair and one row in all (nv = 1), three rows (nv = 2)
RANK_CASES = [(3, 5, 2), (6, 17, 3), (8, 24, 4), (1, 3, 21), (2, 1, 22), (3, 2, 23)]
RANK_WORLDS = (1, 2, 3, 8)        # 8: empty slabs at the small shapes
RANK_CAPS = (1, 7, None)          # rows per chunk (None: all rows); 7 divides no slab edge of these shapes


def direct_sharded_residual_check(lib, cases, worlds, caps, tol):
    """Simulated ranks on a factor-direct context: every rank's slab of the symmetry-reduced residual (T1 dressing on the
    amplitude side, the only form such a context serves) computed one after the other into shared buffers, then the replicated
    finish, against the oracle in numpy fp64 — for every chunk cap, so that chunks start at a rank's row0 and end inside its
    slab.  On the same context the CCD form: ladder_sym (hole = 0, 1, 2) over each rank's pair rows against the stored
    context's whole range and, for hole = 0, the plain einsum.  Returns the largest errors seen."""
    builder = os.environ.get("PYMES_DIRECT_BUILDER") or \
        ("fused" if lib.dll.pymes_backend().decode().startswith("hip") else "gemm")
    worst = {"residual": 0.0, "ladder vs stored": 0.0, "ladder vs einsum": 0.0}
    for no, nv, seed in cases:
        f, V, B, eps = synthetic_case(no, nv, seed, scale=0.3)
        rng = np.random.default_rng(seed)
        t1 = rng.standard_normal((nv, no)) * 0.1
        x = rng.standard_normal((nv, nv, no, no)) * 0.1
        t2 = 0.5 * (x + x.transpose(1, 0, 3, 2))
        Vb = oc.split_blocks(no, V)
        fd_ref = oc.dressed_fock(no, f, t1, Vb)
        Vd_ref = oc.dressed_V(t1, Vb)
        r2_ref = {dcd: oc.ccsd_doubles_residual(no, fd_ref, t2, Vd_ref, is_dcsd=dcd) for dcd in (False, True)}
        lad_ref = np.einsum("abcd,cdij->abij", Vb["abcd"], t2)
        ov, npp = no * nv, nv * (nv + 1) // 2
        stored = DeviceIntegrals.from_factors(no, B, lib=lib)
        try:
            c = stored.ctx
            lad_stored = []
            for hole in (0, 1, 2):
                L = c.ladder_sym(c.array(t2), c.zeros((npp, no * no)), 0, npp, hole_ladder=hole)
                lad_stored.append(c.ladder_sym_unpack(L, c.empty(t2.shape), beta=0.0).get())
        finally:
            stored.ctx.close()
        err = float(np.abs(lad_stored[0] - lad_ref).max())
        assert err < tol, ("stored ladder", no, nv, err)
        for cap in caps:
            rows = min(npp, cap or npp)
            ints = DeviceIntegrals.from_factors(no, B, direct=rows * _row_bytes(nv, builder), lib=lib)
            ctx = ints.ctx
            try:
                info = ctx.direct_info()
                assert info["builder"] == builder and info["chunk_rows"] == rows, (no, nv, cap, info)
                ctx.set_orbital_energies(eps[:no].copy(), eps[no:].copy())
                dT1, dT2, dF = ctx.array(t1), ctx.array(t2), ctx.array(fd_ref)
                for world in worlds:
                    pad = lambda n: pdist.padded_rows(n, world)
                    for dcd in (False, True):
                        ctx.dress_V(dT1, ["klij", "iajb", "iabj"])      # V_abij and V_abcd are never dressed in this mode
                        ETd, ETx, L = ctx.zeros((pad(ov), ov)), ctx.zeros((pad(ov), ov)), ctx.zeros((pad(npp), no * no))
                        QK = ctx.zeros((pad(ov), no * no))
                        for rank in range(world):
                            ctx.residual_slab(dF, dT2, ETd, ETx, L, rank, world, is_dcd=dcd, dressed=True, t1=dT1, QK=QK)
                        r2 = ctx.empty(t2.shape)
                        ctx.residual_finish(dF, dT2, ETd, ETx, L, r2, is_dcd=dcd, dressed=True, t1=dT1, QK=QK)
                        err = float(np.abs(r2.get() - r2_ref[dcd]).max())
                        worst["residual"] = max(worst["residual"], err)
                        assert err < tol, ("residual", builder, no, nv, cap, world, dcd, err)
                    for hole in (0, 1, 2):
                        L = ctx.zeros((npp, no * no))
                        for rank in range(world):
                            lo, hi = pdist.slab_rows(npp, rank, world)
                            ctx.ladder_sym(dT2, L, lo, hi, hole_ladder=hole)
                        got = ctx.ladder_sym_unpack(L, ctx.empty(t2.shape), beta=0.0).get()
                        err = float(np.abs(got - lad_stored[hole]).max())
                        worst["ladder vs stored"] = max(worst["ladder vs stored"], err)
                        assert err < tol, ("ladder_sym against stored", builder, no, nv, cap, world, hole, err)
                        if hole == 0:
                            err = float(np.abs(got - lad_ref).max())
                            worst["ladder vs einsum"] = max(worst["ladder vs einsum"], err)
                            assert err < tol, ("ladder_sym against einsum", builder, no, nv, cap, world, err)
            finally:
                ctx.close()
    print("direct simulated ranks,", builder, "builder: largest |error|", worst)
    return worst


@pytest.mark.parametrize("no,nv,seed", RANK_CASES)
def test_direct_sharded_residual_simulated_ranks(sim, no, nv, seed):
    """The host logic of the pair-sharded loop on a replicated factor-direct context (gemm builder): row slabs, chunk edges
    that start at a rank's row0, empty slabs."""
    direct_sharded_residual_check(sim, [(no, nv, seed)], RANK_WORLDS, RANK_CAPS, 1e-11)
