"""GPU: the factor-direct particle ladder (include/pymes_amd.h, pymes_set_integral_direct).  The rows of the pair-packed V_abcd
from both row builders (batched products + ladder_pack_V; the fused kernel dev::direct_rows_fused) against a numpy packing;
CCSD / DCSD / CCD on a context without any V_abcd against the stored solve and the reference's history, chunked, with the
launch graph and without; the integral footprint at (50,200); (T), IP roots and frozen natural orbitals on such a context."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from oracle.cases import synthetic_case
from oracle.io_oracle import synthetic_factors
from pymes_amd.integral.device import DeviceIntegrals
from tests.test_gpu_shard_integrals import _energies, _rel, _rows_from_factors

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BUILDERS = ("gemm", "fused")


def _pitch(n):
    return (n + 15) // 16 * 16


def _row_bytes(nv, builder):
    """Chunk budget per row: V^+ / V^- at the ladder pitches, plus one plane V[a,b,:,:] for the gemm builder."""
    return 8 * (_pitch(nv * (nv + 1) // 2) + _pitch(nv * (nv - 1) // 2) + (nv * nv if builder == "gemm" else 0))


def _factors(no, nv, naux, seed, scale):
    n = no + nv
    B = np.random.default_rng(seed).standard_normal((naux, n, n)) * scale
    return 0.5 * (B + B.transpose(0, 2, 1))


@pytest.fixture
def clean_env(monkeypatch):
    for name in ("PYMES_DIRECT_BUILDER", "PYMES_DIRECT_CHUNK_BYTES", "PYMES_LADDER_DRESS", "PYMES_NO_GRAPH"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# (no, nv, naux, row ranges): every range starts and ends inside an a-row and holds rows with a == b (P(a,a) = a(a+3)/2: zero
# V^- rows); every row crosses the diagonal tiles (c >= d mask)
ROW_CASES = [
    (5, 37, 23, 7, 0.1, ((1, 40), (303, 391), (650, 700))),           # below one 64-wide tile; naux no multiple of 4 or of 8
    (3, 70, 50, 9, 0.1, ((4, 130), (2100, 2250), (2400, 2480))),      # crosses the first tile edge, ragged second tile
    (2, 200, 40, 8, 0.05, ((10007, 10400),)),                         # four tiles; one chunk in the middle of the range
    # loop edges of direct_rows_fused_kernel (no = 1): all rows in one chunk where there are at most 2200 of them
    (1, 1, 1, 11, 0.1, ((0, 1),)),                                    # one row, no antisymmetric pair: only P holds anything
    (1, 16, 5, 12, 0.1, ((0, 136),)),                                 # one stage (naux <= 8), one working wave
    (1, 32, 8, 13, 0.1, ((0, 528),)),                                 # naux without Q padding, nv on the quadrant edge
    (1, 33, 9, 14, 0.1, ((0, 561),)),                                 # two stages; a quadrant of one row and column
    (1, 64, 16, 15, 0.1, ((0, 2080),)),                               # xp == nv: no pad column
    (1, 65, 24, 16, 0.1, ((0, 2145),)),                               # a second tile of one column
    # three tiles, the last of one column (c = 128): across the a = 63 / 64 tile edge, inside the a-row 128 (rows 8256 ..
    # 8384), and up to the last row P(128,128) = 8384
    (1, 129, 17, 17, 0.1, ((2070, 2120), (8260, 8300), (8320, 8385))),
]
EDGE_ROW_CASES = ROW_CASES[3:]
NO_DIAGONAL_ROW = {(8260, 8300)}        # the one range that lies inside an a-row short of its a == b row


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("no,nv,naux,seed,scale,ranges", ROW_CASES)
def test_rows_match_numpy_packing(gpu_lib, clean_env, builder, no, nv, naux, seed, scale, ranges):
    B = _factors(no, nv, naux, seed, scale)
    cap = max(r1 - r0 for r0, r1 in ranges)
    clean_env.setenv("PYMES_DIRECT_BUILDER", builder)
    ints = DeviceIntegrals.from_factors(no, B, direct=cap * _row_bytes(nv, builder), device=0)
    try:
        info = ints.ctx.direct_info()
        assert info["builder"] == builder and info["chunk_rows"] == cap
        for r0, r1 in ranges:
            diag = [a * (a + 3) // 2 for a in range(nv) if r0 <= a * (a + 3) // 2 < r1]
            assert diag or (r0, r1) in NO_DIAGONAL_ROW, (r0, r1)
            P, M = ints.ctx.direct_rows(r0, r1)
            Pr, Mr = _rows_from_factors(B, no, r0, r1)
            print(builder, (no, nv, naux), (r0, r1), _rel(P, Pr), _rel(M, Mr))
            assert _rel(P, Pr) <= 1e-13 and _rel(M, Mr) <= 1e-13, (builder, r0, r1, _rel(P, Pr), _rel(M, Mr))
            assert not M[[d - r0 for d in diag]].any()
    finally:
        ints.ctx.close()


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("no,nv,naux,seed,scale,ranges", EDGE_ROW_CASES)
def test_single_rows_with_a_one_row_budget(gpu_lib, clean_env, builder, no, nv, naux, seed, scale, ranges):
    """The same shapes on a context whose budget holds one row (a grid of the tile pairs of one row): the first row, the
    last, an a == b row in between and its a > b neighbour."""
    B = _factors(no, nv, naux, seed, scale)
    npp, mid = nv * (nv + 1) // 2, (nv // 2) * (nv // 2 + 3) // 2
    clean_env.setenv("PYMES_DIRECT_BUILDER", builder)
    ints = DeviceIntegrals.from_factors(no, B, direct=8, device=0)
    try:
        info = ints.ctx.direct_info()
        assert info["builder"] == builder and info["chunk_rows"] == 1
        diag = {a * (a + 3) // 2 for a in range(nv)}
        assert {0, npp - 1, mid} <= diag
        for r in sorted({0, mid, min(mid + 1, npp - 1), npp - 1}):
            P, M = ints.ctx.direct_rows(r, r + 1)
            Pr, Mr = _rows_from_factors(B, no, r, r + 1)
            print(builder, (no, nv, naux), "row", r, _rel(P, Pr), _rel(M, Mr))
            assert _rel(P, Pr) <= 1e-13 and _rel(M, Mr) <= 1e-13, (builder, r, _rel(P, Pr), _rel(M, Mr))
            assert Pr.any() and (r in diag or nv < 2 or Mr.any())
            if r in diag:
                assert not M.any()
    finally:
        ints.ctx.close()


def _solve(kind, no, f, ints, de, **kw):
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd import CCSD
    s = CCD(no, delta_e=de, device=0) if kind == "ccd" else CCSD(no, delta_e=de, is_dcsd=kind == "dcsd", device=0)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = s.solve(f, ints, **kw)
    return _energies(buf.getvalue()), res


@pytest.fixture(scope="module")
def case_20_80():
    """(20,80) of tests/golden/solves.json and the stored solves of the three methods, computed once."""
    gold = json.load(open(os.path.join(GOLD, "solves.json")))["syn_20_80"]
    rec, de = gold["recipe"], gold["ccsd"]["delta_e"]
    no, nv = 20, 80
    f, _, B, _ = synthetic_case(no, nv, seed=rec["seed"], scale=rec["scale"], gap=rec["gap"])
    saved = {k: os.environ.pop(k, None) for k in ("PYMES_DIRECT_BUILDER", "PYMES_DIRECT_CHUNK_BYTES", "PYMES_NO_GRAPH")}
    stored = {}
    ints = DeviceIntegrals.from_factors(no, B, device=0)
    try:
        for kind in ("ccsd", "dcsd", "ccd"):
            stored[kind] = _solve(kind, no, f, ints, de)[0]
    finally:
        ints.ctx.close()
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return no, nv, f, B, de, stored, gold["ccsd"]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("builder", BUILDERS)
def test_solves_20_80_direct_against_stored(gpu_lib, clean_env, case_20_80, builder, graph):
    no, nv, f, B, de, stored, gold = case_20_80
    npp = nv * (nv + 1) // 2
    cap = 1000                                   # 3240 rows: chunks of 1000, 1000, 1000, 240, edges inside an a-row
    clean_env.setenv("PYMES_DIRECT_BUILDER", builder)
    clean_env.setenv("PYMES_DIRECT_CHUNK_BYTES", str(cap * _row_bytes(nv, builder)))
    if not graph:
        clean_env.setenv("PYMES_NO_GRAPH", "1")
    ints = DeviceIntegrals.from_factors(no, B, direct=True, device=0)
    try:
        info = ints.ctx.direct_info()
        assert info["builder"] == builder and info["chunk_rows"] == cap and -(-npp // cap) >= 3
        # (before the first solve adds its static packs: the 15 blocks, B_vv and the chunk buffers, nothing of size v^4)
        assert ints.ctx.integral_bytes() == 8 * ((no + nv) ** 4 - nv ** 4) + info["bvv_bytes"] + info["chunk_buffer_bytes"]
        assert info["chunk_buffer_bytes"] == cap * _row_bytes(nv, builder)
        for kind in ("ccsd", "dcsd", "ccd"):
            got = np.array(_solve(kind, no, f, ints, de)[0])
            ref = np.array(stored[kind])
            assert len(got) == len(ref) > 3, (kind, builder, graph)
            print(kind, builder, graph, float(np.abs(got - ref).max()))
            assert np.abs(got - ref).max() < 1e-10, (kind, builder, graph, np.abs(got - ref).max())
            if kind == "ccsd":
                assert len(got) == gold["iterations"]
                assert np.abs(got - np.array(gold["history"])).max() < 1e-9
    finally:
        ints.ctx.close()


@pytest.mark.parametrize("builder", BUILDERS)
def test_residuals_replayed_from_a_launch_graph(gpu_lib, clean_env, builder):
    """pymes_ccsd_residuals on a factor-direct context, recorded once and replayed: the chunk loop is a static sequence of
    launches, the replay gives the residuals of the eager pass."""
    no, nv = 6, 41
    f, _, B, _ = synthetic_case(no, nv, seed=5, scale=0.2)
    clean_env.setenv("PYMES_DIRECT_BUILDER", builder)
    ints = DeviceIntegrals.from_factors(no, B, direct=300 * _row_bytes(nv, builder), device=0)        # 861 rows: 300, 300, 261
    ctx = ints.ctx
    try:
        if not ctx.graphs_supported():
            pytest.fail("launch graphs are expected on the product library")
        ctx.set_orbital_energies(f.diagonal()[:no].copy(), f.diagonal()[no:].copy())
        rng = np.random.default_rng(1)
        t2h = rng.standard_normal((nv, nv, no, no)) * 0.05
        t2h = t2h + t2h.transpose(1, 0, 3, 2)
        t1, t2, fd = ctx.array(rng.standard_normal((nv, no)) * 0.05), ctx.array(t2h), ctx.array(f)
        r1, r2 = ctx.zeros((nv, no)), ctx.zeros((nv, nv, no, no))
        ctx.ccsd_residuals(fd, t1, t2, r1, r2)
        e1, e2 = r1.get(), r2.get()
        ctx.graph_begin()
        ctx.ccsd_residuals(fd, t1, t2, r1, r2)
        g = ctx.graph_end()
        for _ in range(2):
            r1.zero_()
            r2.zero_()
            ctx.graph_launch(g)
            assert np.array_equal(r1.get(), e1) and np.array_equal(r2.get(), e2)
        ctx.graph_destroy(g)
        # ... and they are the residuals of the stored route
        ref = DeviceIntegrals.from_factors(no, B, device=0)
        try:
            c = ref.ctx
            c.set_orbital_energies(f.diagonal()[:no].copy(), f.diagonal()[no:].copy())
            s1, s2 = c.zeros((nv, no)), c.zeros((nv, nv, no, no))
            c.ccsd_residuals(c.array(f), c.array(t1.get()), c.array(t2h), s1, s2)
            assert _rel(e1, s1.get()) <= 1e-12 and _rel(e2, s2.get()) <= 1e-12, (_rel(e1, s1.get()), _rel(e2, s2.get()))
        finally:
            ref.ctx.close()
    finally:
        ctx.close()


def _worker_50_200(_, out):
    """A fresh process: two CCSD iterations at (50,200), stored and factor-direct, their energies and integral bytes."""
    import torch
    torch.cuda.set_device(0)
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 50, 200
    B, eps = synthetic_factors(no, nv, seed=0)
    f = np.diag(eps)
    for direct in (False, True):
        ints = DeviceIntegrals.from_factors(no, B, direct=direct or None, device=0)
        try:
            s = CCSD(no, delta_e=1e-10, device=0)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                s.solve(f, ints, max_iter=2)
            out[direct] = (ints.ctx.integral_bytes(), _energies(buf.getvalue())[:2])
        finally:
            ints.ctx.close()


def test_footprint_and_energies_50_200(gpu_lib, clean_env):
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_worker_50_200, args=(out,), nprocs=1, join=True)
    (b_stored, e_stored), (b_direct, e_direct) = out[False], out[True]
    print("integral bytes stored / direct:", b_stored, b_direct, "energies:", e_stored, e_direct)
    assert b_stored - b_direct >= 8 * 200 ** 4, dict(out)
    assert len(e_stored) == len(e_direct) == 2
    assert np.abs(np.array(e_stored) - np.array(e_direct)).max() < 1e-10, dict(out)


def test_triples_ip_roots_and_fno_on_a_direct_context(gpu_lib, clean_env):
    """What reads no V_abcd works as on stored integrals: (T), the right IP vectors, and frozen natural orbitals / frozen core
    through fno.truncate(..., ("factors", B), direct=True)."""
    from pymes_amd.solver import fno
    no, nv = 6, 20
    f, _, B, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    clean_env.setenv("PYMES_DIRECT_CHUNK_BYTES", str(80 * _row_bytes(nv, "gemm")))             # 210 rows: 80, 80, 50
    res = {}
    for direct in (False, True):
        ints = DeviceIntegrals.from_factors(no, B, direct=direct or None, device=0)
        try:
            res[direct] = _solve("ccsd", no, f, ints, 1e-10, triples=True, ip_roots=2)[1]
        finally:
            ints.ctx.close()
        r = fno.truncate(no, f, ("factors", B), n_frozen=1, nv_keep=14, direct=direct or None, device=0)
        try:
            assert bool(r.ints.direct) == direct
            res[direct, "fno"] = _solve("ccsd", r.no, r.fock, r.ints, 1e-10, triples=True)[1]
        finally:
            r.close()
    for key in ("ccsd e", "(t) e"):
        assert abs(res[True][key] - res[False][key]) < 1e-10, (key, res[True][key], res[False][key])
        assert abs(res[True, "fno"][key] - res[False, "fno"][key]) < 1e-10, ("fno", key)
    assert np.abs(np.asarray(res[True]["ip e"]) - np.asarray(res[False]["ip e"])).max() < 1e-8
