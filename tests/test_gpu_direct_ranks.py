"""GPU: a replicated factor-direct context (include/pymes_amd.h, pymes_set_integral_direct) under the pair-sharded loop.  The
row builders called with a rank's slab start, chunk edges that start at row0 and not at 0, the chunk buffers rewritten between
the grouped products of the hooked whole steps, ranks with an empty slab: simulated ranks against the oracle residual, then
CCSD / DCSD / CCD solved by two ranks on the one GPU (gloo) and by the forced one-rank RCCL world, stored and direct."""
import contextlib
import io
import json
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BUILDERS = ("gemm", "fused")
CHUNK_ROWS = 50          # 210 pair rows at nv = 20: a slab of 105 is 50 + 50 + 5; 78 at nv = 12: a slab of 39 is one chunk
# (tag, kind, no, nv, builders; None: the context's own choice, the fused kernel)
SOLVES = (("syn_6_20", "ccsd", 6, 20, BUILDERS), ("syn_4_12", "dcsd", 4, 12, (None,)), ("syn_4_12", "ccd", 4, 12, (None,)))


@pytest.fixture
def clean_env(monkeypatch):
    for name in ("PYMES_DIRECT_BUILDER", "PYMES_DIRECT_CHUNK_BYTES", "PYMES_LADDER_DRESS", "PYMES_NO_GRAPH",
                 "PYMES_FORCE_SHARDED", "PYMES_OWNER_TILES", "PYMES_PY_SEQUENCED", "PYMES_ALLGATHER_CLONE"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("no,nv,seed", [(3, 5, 2), (6, 17, 3), (8, 24, 4), (1, 3, 21), (2, 1, 22), (3, 2, 23)])
def test_direct_sharded_residual_simulated_ranks(gpu_lib, clean_env, builder, no, nv, seed):
    """Worlds 1, 2, 3, 8 (empty slabs at the small shapes); chunks of 1, 7 and all rows (7 divides no slab edge).  1e-11
    absolute: the bound of the stored route at these shapes (test_gpu_cc.py)."""
    from tests.test_direct_ladder import RANK_CAPS, RANK_WORLDS, direct_sharded_residual_check
    clean_env.setenv("PYMES_DIRECT_BUILDER", builder)
    direct_sharded_residual_check(gpu_lib, [(no, nv, seed)], RANK_WORLDS, RANK_CAPS, 1e-11)


def _solve_all(sharded_calls=False, solves=SOLVES):
    """Inside a rank: every solve of `solves` on stored integrals from the factors and on factor-direct ones, per builder:
    {(kind, "stored" | builder): (energy, iterations, logged energies[, collective calls])}."""
    from oracle.cases import synthetic_case
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd import CCSD
    from tests.test_gpu_direct_ladder import _row_bytes
    from tests.test_gpu_shard_integrals import _energies
    res = {}
    for tag, kind, no, nv, builders in solves:
        f, V, B, eps = synthetic_case(no, nv, seed=0, scale=0.3)
        for mode in ("stored",) + tuple(builders):
            direct = None
            if mode != "stored":
                if mode is not None:
                    os.environ["PYMES_DIRECT_BUILDER"] = mode
                direct = CHUNK_ROWS * _row_bytes(nv, mode or "fused")
            ints = None
            try:
                ints = DeviceIntegrals.from_factors(no, B, direct=direct, device=0)
                assert bool(ints.direct) == (mode != "stored")
                if ints.direct:
                    info = ints.ctx.direct_info()
                    assert info["builder"] == (mode or "fused") and info["chunk_rows"] == min(CHUNK_ROWS, nv * (nv + 1) // 2)
                s = CCD(no, delta_e=1e-10, device=0) if kind == "ccd" else CCSD(no, delta_e=1e-10, is_dcsd=kind == "dcsd", device=0)
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    r = s.solve(f, ints)
                assert s.pair_sharded and s.hooked
                out = (float(r["ccd e" if kind == "ccd" else "ccsd e"]), int(s.iterations), tuple(_energies(buf.getvalue())))
                res[(kind, mode or "default")] = out + ((int(s.collective_calls),) if sharded_calls else ())
            finally:
                os.environ.pop("PYMES_DIRECT_BUILDER", None)
                if ints is not None:
                    ints.ctx.close()
    return res


def _check_solves(res, solves=SOLVES):
    gold = json.load(open(os.path.join(GOLD, "solves.json")))
    for tag, kind, no, nv, builders in solves:
        stored = res[(kind, "stored")]
        g = gold[tag][kind]
        for mode in ("stored",) + tuple(b or "default" for b in builders):
            got = res[(kind, mode)]
            assert abs(got[0] - g["e"]) < 1e-9 and got[1] == g["iterations"], (kind, mode, got[:2], g["e"], g["iterations"])
            assert len(got[2]) == len(stored[2]) > 3, (kind, mode)
            diff = float(np.abs(np.array(got[2]) - np.array(stored[2])).max())
            print(kind, (no, nv), mode, "max |direct - stored| over the logged energies:", diff)
            assert diff < 1e-10, (kind, mode, diff)


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["LOCAL_RANK"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out[rank] = _solve_all()
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_direct(gpu_lib, clean_env):
    """Two ranks share the one GPU (gloo staging): rank 1's slab starts at pair row 105 of 210, inside the a-row 13."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    assert len(out) == 2 and out[0] == out[1]                    # ranks agree bit for bit
    _check_solves(out[0])


def _worker_rccl(rank, port, out):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0", PYMES_FORCE_SHARDED="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        from pymes_amd import dist as pdist
        assert pdist.sharded()
        out[0] = _solve_all(sharded_calls=True, solves=SOLVES[:1])
    finally:
        dist.destroy_process_group()


def test_forced_one_rank_rccl_direct(gpu_lib, clean_env):
    """A world of one rank on an RCCL communicator (PYMES_FORCE_SHARDED=1): the hooked whole steps with device tensors, the
    chunk buffers rewritten between their grouped products."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker_rccl, args=(port, out), nprocs=1, join=True)
    _check_solves(out[0], SOLVES[:1])
    for key, (e, it, hist, calls) in out[0].items():
        assert calls >= 10 * it, (key, calls, it)                # ten collectives per residual build + finish
