"""GPU: the (T) correction (include/pymes_amd.h, pymes_ccsd_t; pymes_amd/solver/ccsd_t.py) against the numpy loop over the
unique triples (tests/_triples_reference.py): random amplitudes at tile-edge sizes, per-triple values across batch
boundaries, converged CCSD on FCIDUMP fixtures, CCD amplitudes of the 57-plane-wave electron gas (the test of the hole
term's integral), batch-size and rank-chunk reproducibility, the refusals, and a sharded-integral context."""
import contextlib
import ctypes as C
import io
import json
import os
import socket

import numpy as np
import pytest

from oracle.cases import synthetic_case
from oracle.io_oracle import synthetic_factors
from pymes_amd import _lib
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.solver import ccsd_t
from tests import _triples_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _rel(x, ref):
    return abs(x - ref) / max(abs(ref), 1e-300)


def _live():
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


@pytest.mark.parametrize("no,nv", [(2, 6), (4, 12), (5, 19), (7, 33), (8, 40), (5, 3), (6, 4), (20, 10)])
def test_random_amplitudes_against_oracle(gpu_lib, no, nv):
    f, V, B, eps = synthetic_case(no, nv, seed=no + nv)
    t1, t2 = R.random_amplitudes(no, nv, seed=3 * no + nv, amp=0.05)
    ref = R.energy(no, V, eps, t1, t2)
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        e = ccsd_t.get_triples_energy(no, f, ints, t1, t2)
        assert _rel(e, ref) < 1e-12, (e, ref)
        e0 = ccsd_t.get_triples_energy(no, f, ints, None, t2)
        ref0 = R.energy(no, V, eps, None, t2)
        assert _rel(e0, ref0) < 1e-12, (e0, ref0)
    finally:
        ints.ctx.close()


def test_per_triple_ranges_30_120(gpu_lib, monkeypatch):
    no, nv = 30, 120
    B, eps = synthetic_factors(no, nv, seed=4, scale=0.3)
    f = np.diag(eps)
    t1, t2 = R.random_amplitudes(no, nv, seed=9, amp=0.02)
    blk = R.blocks_from_factors(no, B)
    n = R.n_triples(no)
    monkeypatch.setenv("PYMES_TRIPLES_BATCH", "2")
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        # the start, a range over a batch boundary (batches begin at the range's start), the end
        for lo, hi in ((0, 3), (n // 2 - 1, n // 2 + 2), (n - 3, n)):
            e, vec = ccsd_t.get_triples_energy(no, f, ints, t1, t2, triple_range=(lo, hi), per_triple=True)
            ref = R.per_triple(no, None, eps, t1, t2, lo, hi, blk=blk)
            assert vec.shape == (hi - lo,)
            assert np.abs(vec - ref).max() <= 1e-12 * np.abs(ref).max(), (lo, hi, vec, ref)
            assert _rel(e, ref.sum()) < 1e-12
    finally:
        ints.ctx.close()


@pytest.mark.parametrize("tag", ["LiH.321g", "H2.ccpvdz", "syn_5_19"])
def test_converged_ccsd_fcidump(gpu_lib, tag, tmp_path):
    import gzip
    from pymes_amd.mean_field import hf
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.util import fcidump
    if tag.startswith("syn_"):
        path = str(tmp_path / "FCIDUMP.syn_5_19")
        with gzip.open(os.path.join(GOLD, "fcidump", "FCIDUMP.syn_5_19.gz"), "rb") as src, open(path, "wb") as dst:
            dst.write(src.read())
    else:
        path = os.path.join(GOLD, "fcidump", "FCIDUMP." + tag)
    ne, n, ec, eps, h, V = quiet(fcidump.read, path)
    no = ne // 2
    f = hf.construct_hf_matrix(no, h, V)
    # canonical orbitals: the HF matrix of these files is diagonal up to rounding
    f = np.diag(np.diag(f)) if np.abs(f - np.diag(np.diag(f))).max() < 1e-6 else f
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        s = CCSD(no, delta_e=1e-11)
        res = quiet(s.solve, f, ints, device_amplitudes=True, triples=True)
        t1, t2 = res["t1"], res["t2"]
        e_dev = ccsd_t.get_triples_energy(no, f, ints, t1, t2)
        assert e_dev == res["(t) e"]
        assert res["ccsd(t) e"] == res["ccsd e"] + res["(t) e"]
        ref = R.energy(no, V, np.diag(f), t1.get(), t2.get())
        if no == 1:
            assert abs(res["(t) e"]) <= 1e-14
        else:
            assert abs(ref) > 1e-7
            assert _rel(res["(t) e"], ref) < 1e-11, (res["(t) e"], ref)
    finally:
        ints.ctx.close()


def test_ueg_57_plane_waves_ccd_amplitudes(gpu_lib):
    """Plain Coulomb integrals of the electron gas (V_pqrs = V_qpsr = V_rspq, not V_psrq): the hole term must read <ij|am>."""
    from pymes_amd.mean_field import hf
    from pymes_amd.model.ueg import UEG
    from pymes_amd.solver import ccd
    ref = json.load(open(os.path.join(GOLD, "ueg.json")))["coulomb_N14_rs0.5_c5"]
    nel, rs = ref["nel"], ref["rs"]
    m = UEG(nel, nel // 2, nel // 2, rs)
    m.init_single_basis(ref["cutoff"])
    no, n_p = nel // 2, len(m.basis_fns) // 2
    assert n_p == 57
    kin = np.array([m.basis_fns[2 * i].kinetic for i in range(n_p)])
    V = quiet(m.eval_2b_integrals, sp=1)
    assert np.abs(V - V.transpose(2, 3, 0, 1)).max() < 1e-12
    assert np.abs(V - V.transpose(0, 3, 2, 1)).max() > 1e-3          # not 8-fold: <im|aj> != <ij|am>
    f = hf.construct_hf_matrix(no, np.diag(kin), V)
    rc = quiet(ccd.CCD(no, is_diis=True).solve, f, V, level_shift=-1., sp=0, max_iter=60)
    t2 = rc["t2 amp"]
    e = ccsd_t.get_triples_energy(no, f, V, None, t2)
    ref_e = R.energy(no, V, np.diag(f), None, t2)
    assert abs(ref_e) > 1e-6
    assert _rel(e, ref_e) < 1e-11, (e, ref_e)


def test_batch_size_and_rank_chunks(gpu_lib, monkeypatch):
    no, nv = 9, 40
    f, V, B, eps = synthetic_case(no, nv, seed=11)
    t1, t2 = R.random_amplitudes(no, nv, seed=12, amp=0.05)
    n = R.n_triples(no)
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        monkeypatch.delenv("PYMES_TRIPLES_BATCH", raising=False)
        e_def, v_def = ccsd_t.get_triples_energy(no, f, ints, t1, t2, per_triple=True)
        monkeypatch.setenv("PYMES_TRIPLES_BATCH", "1")
        e_one, v_one = ccsd_t.get_triples_energy(no, f, ints, t1, t2, per_triple=True)
        monkeypatch.setenv("PYMES_TRIPLES_BATCH", "7")
        e_sev, v_sev = ccsd_t.get_triples_energy(no, f, ints, t1, t2, per_triple=True)
        assert np.array_equal(v_def, v_one) and np.array_equal(v_def, v_sev)
        assert e_def == e_one == e_sev
        chunks = [ccsd_t.rank_range(no, r, 3) for r in range(3)]
        assert chunks[0][0] == 0 and chunks[-1][1] == n
        parts = [ccsd_t.get_triples_energy(no, f, ints, t1, t2, triple_range=c) for c in chunks]
        assert abs(sum(parts) - e_def) <= 1e-14 * abs(e_def)
    finally:
        ints.ctx.close()


def test_refusals_leave_no_allocation(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.util import fcidump
    E = _lib.PymesError
    before = _live()
    # transcorrelated integrals: no V_pqrs = V_rspq
    ne, n, ec, eps, h, V = quiet(fcidump.read, os.path.join(GOLD, "tc", "FCIDUMP.LiH.tc"), is_tc=True)
    no = ne // 2
    f = np.diag(np.arange(n, dtype=np.float64) - no + 0.5)
    t1, t2 = R.random_amplitudes(no, n - no, seed=1)
    with pytest.raises(E, match="Hermitian"):
        ccsd_t.get_triples_energy(no, f, V, t1, t2)
    # graph capture, a missing block
    no, nv = 3, 8
    f, V, B, eps = synthetic_case(no, nv, seed=2)
    t1, t2 = R.random_amplitudes(no, nv, seed=3)
    ctx = Context(no, nv)
    try:
        d1, d2 = ctx.array(t1), ctx.array(t2)
        for name in ("klij", "ijka", "ijak", "ijab", "iajk", "iajb", "iabj", "abij"):
            sl = tuple(slice(no, None) if ch in "abcd" else slice(0, no) for ch in name)
            ctx.set_V_block(name, np.ascontiguousarray(V[sl]))
        with pytest.raises(E, match="'iabc'"):
            ccsd_t.triples_energy(ctx, eps, d1, d2, 0, 4)
        ctx.set_V_pqrs(V)
        assert ctx.graphs_supported()
        ctx.graph_begin()
        try:
            with pytest.raises(E, match="launch graph"):
                ccsd_t.triples_energy(ctx, eps, d1, d2, 0, 4)
        finally:
            ctx.graph_abort()
        e, _ = ccsd_t.triples_energy(ctx, eps, d1, d2, 0, R.n_triples(no))
        assert _rel(e, R.energy(no, V, eps, t1, t2)) < 1e-12
        d1.free()
        d2.free()
    finally:
        ctx.close()
    assert _live() == before


def test_sharded_integrals_same_energy(gpu_lib):
    no, nv = 6, 24
    f, V, B, eps = synthetic_case(no, nv, seed=5)
    t1, t2 = R.random_amplitudes(no, nv, seed=6)
    full = DeviceIntegrals.from_factors(no, B)
    shard = DeviceIntegrals.from_factors(no, B, shard=(1, 2))
    try:
        # a dressing of the blocks on the same context does not touch what (T) reads
        quiet(shard.ctx.dress_V, shard.ctx.array(t1), ("iabc", "ijak", "ijab"))
        e_full = ccsd_t.get_triples_energy(no, f, full, t1, t2)
        e_shard = ccsd_t.get_triples_energy(no, f, shard, t1, t2)
        assert e_full == e_shard
        assert _rel(e_full, R.energy(no, V, eps, t1, t2)) < 1e-12
    finally:
        full.ctx.close()
        shard.ctx.close()


def _rank_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pymes_amd.solver.ccsd import CCSD
        no, nv = 5, 16
        f, V, B, eps = synthetic_case(no, nv, seed=21)
        t1, t2 = R.random_amplitudes(no, nv, seed=22)
        e = ccsd_t.get_triples_energy(no, f, V, t1, t2, device=0)
        r = quiet(CCSD(no, delta_e=1e-10, device=0).solve, f, V, triples=True)
        out[rank] = (e, float(r["ccsd e"]), float(r["(t) e"]))
    finally:
        dist.destroy_process_group()


def test_ranks_sum_their_chunks(gpu_lib):
    """Three ranks under torch.distributed (gloo, one GPU): each sums its chunk of the triples and one double is all-reduced;
    every rank returns the single-process energy, alone and inside CCSD.solve(triples=True)."""
    import torch.multiprocessing as mp
    from pymes_amd.solver.ccsd import CCSD
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = 3
    out = mp.Manager().dict()
    mp.spawn(_rank_worker, args=(world, port, out), nprocs=world, join=True)
    no, nv = 5, 16
    f, V, B, eps = synthetic_case(no, nv, seed=21)
    t1, t2 = R.random_amplitudes(no, nv, seed=22)
    e_one = ccsd_t.get_triples_energy(no, f, V, t1, t2)
    assert _rel(e_one, R.energy(no, V, eps, t1, t2)) < 1e-12
    r = quiet(CCSD(no, delta_e=1e-10).solve, f, V, triples=True)
    assert len(out) == world
    for rank in range(world):
        e, e_cc, e_t = out[rank]
        assert abs(e - e_one) <= 1e-14 * abs(e_one), (rank, e, e_one)
        assert abs(e_cc - r["ccsd e"]) < 1e-9, (rank, e_cc, r["ccsd e"])
        assert abs(e_t - r["(t) e"]) <= 1e-9 * abs(r["(t) e"]), (rank, e_t, r["(t) e"])
