"""Integral sharding (include/pymes_amd.h, pymes_set_integral_shard) on the host simulator: a context that keeps only its
rank's rows of the pair-packed V_abcd gives the per-iteration energies of the replicated sharded solve, holds exactly
v^4 doubles less plus its rows, and refuses every path that needs the full or dressed block."""
import contextlib
import io
import os
import re
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pitch(n):
    return (n + 15) // 16 * 16


def _pair_chunk(nv, rank, world):
    npp = nv * (nv + 1) // 2
    c = -(-npp // world)
    lo = min(rank * c, npp)
    return lo, min(lo + c, npp)


def pack_rows(Vabcd, r0, r1):
    """numpy form of dev::ladder_pack_V for the pair rows [r0, r1) (device_api.h): Vp[P(c,d)] = V_abcd + V_abdc (c >= d),
    Vm[Q(c,d)] = V_abcd - V_abdc (c > d; zero rows for a == b)."""
    nv = Vabcd.shape[0]
    pairs = [(a, b) for a in range(nv) for b in range(a + 1)]
    lo = np.tril_indices(nv)
    slo = np.tril_indices(nv, -1)
    P = np.zeros((r1 - r0, nv * (nv + 1) // 2))
    M = np.zeros((r1 - r0, nv * (nv - 1) // 2))
    for r in range(r0, r1):
        a, b = pairs[r]
        X = Vabcd[a, b]
        P[r - r0] = (X + X.T)[lo]
        if a != b:
            M[r - r0] = (X - X.T)[slo]
    return P, M


def _energies(text):
    return [float(x) for x in re.findall(r"Correlation Energy = ([-0-9.eE+]+)", text)]


def _solve(kind, no, f, V, shard):
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd import CCSD
    if kind in ("ccsd", "dcsd"):
        s = CCSD(no, delta_e=1e-10, is_dcsd=kind == "dcsd", shard_integrals=shard)
    else:
        s = CCD(no, delta_e=1e-10, is_dcd=kind == "dcd", shard_integrals=shard)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        s.solve(f, V)
    # (the host simulator has the fused pair kernels up to no = 3: CCSD / DCSD above that take the sharded residual with
    # the replicated tail; CCD / DCD need the pair-sharded tail for their sharded path)
    assert s.pair_sharded == (no <= 3)
    return _energies(buf.getvalue())


def _worker(rank, world, port, libpath, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tests.conftest import hostsim_library
        lib = hostsim_library(libpath)
        _lib._default = lib
        res = {}
        for no, nv in ((5, 14), (4, 12), (3, 14), (3, 12)):
            f, V, _, _ = synthetic_case(no, nv, seed=3, scale=0.3)
            for kind in ("ccsd", "dcsd", "ccd", "dcd") if no <= 3 else ("ccsd", "dcsd"):
                rep = _solve(kind, no, f, V, False)
                sh = _solve(kind, no, f, V, True)
                res[(no, nv, kind)] = (rep, sh)
            # the stored rows against a numpy packing, staged in chunks that cut inside an a-row
            n = no + nv
            os.environ["PYMES_SHARD_STAGING_BYTES"] = str(8 * nv * nv * 5)
            try:
                ints = DeviceIntegrals.from_V_pqrs(no, V, shard=(rank, world), lib=lib)
            finally:
                del os.environ["PYMES_SHARD_STAGING_BYTES"]
            P, M, r0, r1 = ints.ctx.shard_rows()
            assert (r0, r1) == _pair_chunk(nv, rank, world)
            Pr, Mr = pack_rows(V[no:, no:, no:, no:], r0, r1)
            res[(no, nv, "rows")] = max(float(np.abs(P - Pr).max(initial=0.0)), float(np.abs(M - Mr).max(initial=0.0)))
            # integral bytes: the replicated count minus v^4 doubles plus the rank's rows
            rep = Context(no, nv, lib=lib)
            rep.set_V_pqrs(V)
            rows = r1 - r0
            want = rep.integral_bytes() - 8 * nv ** 4 + 8 * rows * (_pitch(nv * (nv + 1) // 2) + _pitch(nv * (nv - 1) // 2))
            res[(no, nv, "bytes")] = (ints.ctx.integral_bytes(), want)
            assert rep.integral_bytes() == 8 * n ** 4
            rep.close()
            ints.ctx.close()
        out[rank] = res
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_storage_matches_replicated(hostsim_lib, world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, hostsim_lib.path, out), nprocs=world, join=True)
    assert len(out) == world
    for rank in range(world):
        for key, val in out[rank].items():
            if key[2] == "rows":
                assert val < 1e-12, (rank, key, val)
            elif key[2] == "bytes":
                assert val[0] == val[1], (rank, key, val)
            else:
                rep, sh = val
                assert len(rep) == len(sh) and len(rep) > 3, (rank, key, rep, sh)
                assert np.abs(np.array(rep) - np.array(sh)).max() < 1e-12, (rank, key, rep, sh)


def _sharded_ctx(lib, no, nv, rank, world, seed=0):
    f, V, _, _ = synthetic_case(no, nv, seed=seed, scale=0.3)
    ctx = Context(no, nv, lib=lib, shard=(rank, world))
    ctx.set_V_pqrs(V)
    ctx.set_orbital_energies(f.diagonal()[:no].copy(), f.diagonal()[no:].copy())
    return ctx, f, V


def test_refusals(hostsim_lib):
    no, nv = 3, 7
    ctx, f, V = _sharded_ctx(hostsim_lib, no, nv, 1, 2)
    E = _lib.PymesError
    t2 = ctx.zeros((nv, nv, no, no))
    t1 = ctx.zeros((nv, no))
    fd = ctx.array(f)
    r2 = ctx.zeros((nv, nv, no, no))
    r1 = ctx.zeros((nv, no))
    npp = nv * (nv + 1) // 2
    L = ctx.zeros((npp, no * no))
    r0, r1_ = _pair_chunk(nv, 1, 2)
    rep = Context(no, nv, lib=hostsim_lib)
    rep.set_V_pqrs(V)
    refused = {
        "block pointer": lambda: ctx.V_block("abcd"),
        "dressed block pointer": lambda: ctx.V_block("abcd", dressed=True),
        "abcd from device": lambda: ctx.set_V_block("abcd", ctx.zeros((nv,) * 4)),
        "ladder": lambda: ctx.ladder(t2, r2, 0, nv),
        "doubles_residual": lambda: ctx.doubles_residual(fd, t2, r2),
        "doubles_residual sym": lambda: ctx.doubles_residual(fd, t2, r2, sym_ladder=True, sym_rings=True),
        "ccsd_residuals": lambda: ctx.ccsd_residuals(fd, t1, t2, r1, r2),
        "ccsd_iterate": lambda: ctx.ccsd_iterate(fd, t1, t2, ctx.zeros((nv, no)), ctx.zeros((nv, nv, no, no))),
        "dress_abcd_rows": lambda: ctx.dress_abcd_rows(t1, 0, nv),
        "dress_V abcd": lambda: ctx.dress_V(t1, ("abcd",)),
        "ladder_sym dressed": lambda: ctx.ladder_sym(t2, L, r0, r1_, dressed=True),
        "ladder_sym other rows": lambda: ctx.ladder_sym(t2, L, 0, r0),
        "ladder_sym all rows": lambda: ctx.ladder_sym(t2, L, 0, npp),
        "ladder_sym_multi": lambda: ctx.ladder_sym_multi([t2], ctx.zeros((1, npp, no * no))),
        "residual_slab other rank": lambda: ctx.residual_slab(fd, t2, ctx.zeros((no * nv, no * nv)), ctx.zeros((no * nv, no * nv)),
                                                              L, 0, 2),
        "residual_slab other world": lambda: ctx.residual_slab(fd, t2, ctx.zeros((no * nv, no * nv)), ctx.zeros((no * nv, no * nv)),
                                                               L, 1, 3),
        "shard after set_V": lambda: hostsim_lib.call("pymes_set_integral_shard", rep.handle, 0, 2),
    }
    for name, call in refused.items():
        with pytest.raises(E, match=r"integral shard|before any pymes_set_V"):
            call()
        assert name  # (the label names the case in a failure's traceback)
    rep.close()
    # the EOM sigma reads the whole V_abcd
    import ctypes as C
    h = C.c_void_p()
    fh = np.ascontiguousarray(f)
    with pytest.raises(E, match="integral sharding"):
        hostsim_lib.call("pymes_eom_sigma_prepare", ctx.handle, _lib.host_ptr(fh), C.c_void_p(t2.ptr), 0, C.byref(h))
    # ... while the rank's own rows serve the undressed ladder (CCD / DCD, hole = 0/1/2)
    for hole in (0, 1, 2):
        ctx.ladder_sym(t2, L, r0, r1_, hole_ladder=hole)
    ctx.close()
    # a replicated context has no rows to show; rank / world out of range
    rep = Context(no, nv, lib=hostsim_lib)
    with pytest.raises(E):
        rep.shard_rows()
    rep.close()
    for bad in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(E):
            Context(no, nv, lib=hostsim_lib, shard=bad)


def test_factors_kernel_absent_on_host_simulator(hostsim_lib):
    """The factor path needs the gfx950 kernel: the host simulator's weak stand-in refuses instead of computing anything."""
    no, nv = 2, 5
    _, _, B, _ = synthetic_case(no, nv, seed=1, scale=0.3)
    with pytest.raises(_lib.PymesError, match="not available in this backend"):
        DeviceIntegrals.from_factors(no, B, shard=(0, 2), lib=hostsim_lib)


def test_host_block_abcd_rows_and_bytes(hostsim_lib):
    """set_V_block('abcd') from the host fills the rows; the other blocks as ever; bytes counted without V_abcd."""
    no, nv = 2, 6
    _, V, _, _ = synthetic_case(no, nv, seed=2, scale=0.3)
    world = 3
    for rank in range(world):
        ctx = Context(no, nv, lib=hostsim_lib, shard=(rank, world))
        from pymes_amd.integral.partition import BLOCK_NAMES
        for name in BLOCK_NAMES:
            sl = tuple(slice(no, None) if ch in "abcd" else slice(0, no) for ch in name)
            ctx.set_V_block(name, np.ascontiguousarray(V[sl]))
        P, M, r0, r1 = ctx.shard_rows()
        Pr, Mr = pack_rows(V[no:, no:, no:, no:], r0, r1)
        assert np.array_equal(P, Pr) and np.array_equal(M, Mr)
        n = no + nv
        rows = r1 - r0
        assert ctx.integral_bytes() == 8 * (n ** 4 - nv ** 4) + 8 * rows * (_pitch(nv * (nv + 1) // 2) + _pitch(nv * (nv - 1) // 2))
        ctx.close()


def test_single_rank_path_refuses_shard_integrals(hostsim_lib, monkeypatch):
    from pymes_amd import dist as pdist
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd import CCSD
    monkeypatch.setattr(_lib, "_default", hostsim_lib)
    monkeypatch.delenv("PYMES_FORCE_SHARDED", raising=False)
    assert not pdist.sharded()
    no, nv = 2, 5
    f, V, _, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    for s in (CCSD(no, shard_integrals=True), CCD(no, shard_integrals=True)):
        with pytest.raises(ValueError, match="shard_integrals"):
            with contextlib.redirect_stdout(io.StringIO()):
                s.solve(f, V)
