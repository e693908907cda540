"""GPU: integral sharding (include/pymes_amd.h, pymes_set_integral_shard).  The rows of the pair-packed V_abcd built by the
factor kernel (dev::ladder_pack_V_factors) and by the bounded host upload (ladder_pack_V, nr == 0) against a numpy packing;
two ranks on one GPU with sharded storage against the replicated two-rank run and the reference's history; the integral
footprint of a stubbed rank at (50,200)."""
import contextlib
import io
import json
import os
import re
import socket

import numpy as np
import pytest

from oracle.cases import synthetic_case
from oracle.io_oracle import eri_from_factors, synthetic_factors
from pymes_amd.integral.device import DeviceIntegrals

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _pair_chunk(nv, rank, world):
    npp = nv * (nv + 1) // 2
    c = -(-npp // world)
    lo = min(rank * c, npp)
    return lo, min(lo + c, npp)


def _rows_from_factors(B, no, r0, r1):
    """numpy packing (device_api.h, ladder_pack_V) of the rows [r0, r1) of V_abcd = einsum('Qac,Qbd->abcd', B, B) over the
    virtual block, one (a, b) tile at a time."""
    Bv = B[:, no:, no:]
    nv = Bv.shape[1]
    lo, slo = np.tril_indices(nv), np.tril_indices(nv, -1)
    P = np.zeros((r1 - r0, nv * (nv + 1) // 2))
    M = np.zeros((r1 - r0, nv * (nv - 1) // 2))
    a = int((np.sqrt(8.0 * r0 + 1.0) - 1.0) / 2.0)
    while a * (a + 1) // 2 > r0:
        a -= 1
    while (a + 1) * (a + 2) // 2 <= r0:
        a += 1
    b = r0 - a * (a + 1) // 2
    for r in range(r0, r1):
        X = np.einsum("Qc,Qd->cd", Bv[:, a, :], Bv[:, b, :])
        P[r - r0] = (X + X.T)[lo]
        if a != b:
            M[r - r0] = (X - X.T)[slo]
        b += 1
        if b > a:
            a, b = a + 1, 0
    return P, M


def _rel(x, ref):
    return float(np.abs(x - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-300)


@pytest.mark.parametrize("source", ["factors", "host"])
def test_rows_match_numpy_packing_odd_shape(gpu_lib, source):
    """nv = 37, no = 5, naux = 23: rows of worlds 1, 2, 3 (chunk edges inside an a-row)."""
    no, nv, naux = 5, 37, 23
    n = no + nv
    rng = np.random.default_rng(7)
    B = rng.standard_normal((naux, n, n)) * 0.1
    B = 0.5 * (B + B.transpose(0, 2, 1))
    V = eri_from_factors(B) if source == "host" else None
    for world in (1, 2, 3):
        for rank in range(world):
            if source == "factors":
                ints = DeviceIntegrals.from_factors(no, B, shard=(rank, world), device=0)
            else:
                ints = DeviceIntegrals.from_V_pqrs(no, V, shard=(rank, world), device=0)
            try:
                P, M, r0, r1 = ints.ctx.shard_rows()
                assert (r0, r1) == _pair_chunk(nv, rank, world)
                Pr, Mr = _rows_from_factors(B, no, r0, r1)
                assert _rel(P, Pr) <= 1e-13 and _rel(M, Mr) <= 1e-13, (source, rank, world, _rel(P, Pr), _rel(M, Mr))
                if source == "factors":     # the other 15 blocks as set_V_from_factors forms them
                    Vijab = ints.ctx.V_block("ijab").get()
                    ref = np.einsum("Qia,Qjb->ijab", B[:, :no, no:], B[:, :no, no:])
                    assert _rel(Vijab, ref) <= 1e-13
            finally:
                ints.ctx.close()


def test_factor_rows_nv200_one_chunk(gpu_lib):
    """nv = 200: one rank's chunk (rank 3 of 8) from the factor kernel."""
    no, nv, naux = 2, 200, 40
    n = no + nv
    rng = np.random.default_rng(8)
    B = rng.standard_normal((naux, n, n)) * 0.05
    B = 0.5 * (B + B.transpose(0, 2, 1))
    ints = DeviceIntegrals.from_factors(no, B, shard=(3, 8), device=0)
    try:
        P, M, r0, r1 = ints.ctx.shard_rows()
        assert (r0, r1) == _pair_chunk(nv, 3, 8)
        Pr, Mr = _rows_from_factors(B, no, r0, r1)
        assert _rel(P, Pr) <= 1e-13 and _rel(M, Mr) <= 1e-13, (_rel(P, Pr), _rel(M, Mr))
    finally:
        ints.ctx.close()


def _energies(text):
    return [float(x) for x in re.findall(r"Correlation Energy = (-?[0-9.eE+-]+)", text)]


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pymes_amd.solver.ccd import CCD
        from pymes_amd.solver.ccsd import CCSD
        gold = json.load(open(os.path.join(GOLD, "solves.json")))["syn_20_80"]
        rec, de = gold["recipe"], gold["ccsd"]["delta_e"]
        no, nv = 20, 80
        f, V, B, eps = synthetic_case(no, nv, seed=rec["seed"], scale=rec["scale"], gap=rec["gap"])
        res = {}

        def run(kind, V_or_ints, shard):
            s = CCD(no, delta_e=de, device=0, shard_integrals=shard) if kind == "ccd" else \
                CCSD(no, delta_e=de, is_dcsd=kind == "dcsd", device=0, shard_integrals=shard)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                s.solve(f, V_or_ints)
            assert s.pair_sharded and s.hooked
            return _energies(buf.getvalue())

        for kind in ("ccsd", "dcsd", "ccd"):
            res[("replicated", kind)] = run(kind, V, False)
            res[("host", kind)] = run(kind, V, True)
            ints = DeviceIntegrals.from_factors(no, B, shard=(rank, world), device=0)
            try:
                res[("factors", kind)] = run(kind, ints, True)
                assert ints.ctx.integral_bytes() > 0
            finally:
                ints.ctx.close()
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_sharded_storage(gpu_lib):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    assert len(out) == 2
    gold = json.load(open(os.path.join(GOLD, "solves.json")))["syn_20_80"]["ccsd"]
    for rank in range(2):
        res = out[rank]
        for kind in ("ccsd", "dcsd", "ccd"):
            rep = np.array(res[("replicated", kind)])
            for source in ("host", "factors"):
                sh = np.array(res[(source, kind)])
                assert len(sh) == len(rep) > 3, (rank, kind, source)
                assert np.abs(sh - rep).max() < 1e-10, (rank, kind, source, np.abs(sh - rep).max())
        for source in ("host", "factors"):
            hist = np.array(res[(source, "ccsd")])
            assert len(hist) == gold["iterations"]
            assert np.abs(hist - np.array(gold["history"])).max() < 1e-9


def _stub_worker(_, out):
    """A fresh process: torch's HIP runtime is initialised before the library's (the stubbed path allocates its exchange
    buffers with torch), as bench.py does."""
    import torch
    torch.cuda.set_device(0)
    from pymes_amd import dist as pdist
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 50, 200
    B, eps = synthetic_factors(no, nv, seed=0)
    f = np.diag(eps)
    pdist.stub(0, 4)
    for shard in (False, True):
        ints = DeviceIntegrals.from_factors(no, B, shard=(0, 4) if shard else None, device=0)
        try:
            s = CCSD(no, delta_e=1e-10, device=0, shard_integrals=shard)
            with contextlib.redirect_stdout(io.StringIO()):
                s.solve(f, ints, max_iter=2)
            assert s.pair_sharded and s.iterations >= 1
            out[shard] = ints.ctx.integral_bytes()
        finally:
            ints.ctx.close()


def test_stub_rank_footprint_50_200(gpu_lib):
    """A stubbed rank 0 of 4 at (50,200) holds at least 0.7 x 12.8 GB fewer integral bytes than the replicated stubbed rank,
    and its compute path (energies meaningless under stubbed collectives) still runs."""
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_stub_worker, args=(out,), nprocs=1, join=True)
    assert out[False] - out[True] >= 0.7 * 8 * 200 ** 4, dict(out)
