"""GPU: frozen natural orbitals and frozen core (pymes_amd/solver/fno.py; include/pymes_amd.h, pymes_fno_density and
pymes_derive_context) against numpy restatements of the definitions (tests/_fno_reference.py) and against solves the
project already runs: the density kernel, the derived blocks, invariance under a full or rotated space, the truncated
CCSD(T) pipeline, frozen core, factor and host sources, two ranks, refusals and leaks."""
import contextlib
import ctypes as C
import gzip
import io
import os
import socket

import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.integral.partition import BLOCK_NAMES, part_2_body_int
from pymes_amd.solver import fno
from pymes_amd.solver.ccsd import CCSD
from tests import _fno_reference as ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _fcidump_5_19(tmp_path):
    from pymes_amd.mean_field import hf
    from pymes_amd.util import fcidump
    path = str(tmp_path / "FCIDUMP.syn_5_19")
    with gzip.open(os.path.join(GOLD, "fcidump", "FCIDUMP.syn_5_19.gz"), "rb") as src, open(path, "wb") as dst:
        dst.write(src.read())
    ne, n, ec, eps, h, V = quiet(fcidump.read, path)
    no = ne // 2
    f = hf.construct_hf_matrix(no, h, V)
    f = np.diag(np.diag(f))
    return no, f, np.ascontiguousarray(V)


def _case(name, tmp_path):
    if name == "fcidump_5_19":
        return _fcidump_5_19(tmp_path)
    f, V, _, _ = synthetic_case(8, 30, seed=11, scale=0.3)
    return 8, f, V


@pytest.mark.parametrize("name", ["fcidump_5_19", "random_8_30"])
@pytest.mark.parametrize("nf", [0, 1, 2])
def test_density_against_numpy(gpu_lib, name, nf, tmp_path):
    no, f, V = _case(name, tmp_path)
    D_ref, e_ref = ref.mp2_density(no, f, V, nf)
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        ints.ctx.set_orbital_energies(np.diag(f)[:no], np.diag(f)[no:])
        D, e = fno.density(ints.ctx, nf)
        D2, e2 = fno.density(ints.ctx, nf)
    finally:
        ints.ctx.close()
    assert np.abs(D - D_ref).max() <= 1e-12 * np.abs(D_ref).max()
    assert abs(e - e_ref) <= 1e-12 * abs(e_ref)
    assert np.array_equal(D, D2) and e == e2              # fixed summation order: bit-identical
    assert np.array_equal(D, D.T)


def test_derived_blocks_against_numpy(gpu_lib):
    no, nv, nf, k = 6, 21, 1, 13
    f, V, _, _ = synthetic_case(no, nv, seed=5, scale=0.3)
    Q, _ = np.linalg.qr(np.random.default_rng(7).standard_normal((nv, nv)))
    Cm = Q[:, :k]
    U = np.zeros((no + nv, no - nf + k))
    U[nf:no, :no - nf] = np.eye(no - nf)
    U[no:, no - nf:] = Cm
    want = part_2_body_int(no - nf, ref.transform(V, U))
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        new = fno.derive_context(ints, nf, Cm)
        try:
            for nm in BLOCK_NAMES:
                got = new.block(nm).get()
                assert np.abs(got - want[nm]).max() <= 1e-12 * np.abs(want[nm]).max(), nm
        finally:
            new.ctx.close()
    finally:
        ints.ctx.close()


def test_full_space_invariance(gpu_lib):
    no, nv = 5, 18
    f, V, B, _ = synthetic_case(no, nv, seed=3, scale=0.3)
    plain = quiet(CCSD(no, delta_e=1e-11).solve, f, V, triples=True)
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        full = quiet(CCSD(no, delta_e=1e-11).solve, f, ints, fno_nv=nv, triples=True)
    finally:
        ints.ctx.close()
    assert abs(full["ccsd e"] - plain["ccsd e"]) < 1e-9
    assert abs(full["(t) e"] - plain["(t) e"]) < 1e-9
    assert abs(full["fno dmp2 e"]) < 1e-12 and full["fno nv"] == nv
    r = fno.truncate(no, f, ("factors", B), nv_keep=nv)
    try:
        assert abs(r.de_mp2) < 1e-12
        fac = quiet(CCSD(r.no, delta_e=1e-11).solve, r.fock, r.ints, triples=True)
    finally:
        r.close()
    assert abs(fac["ccsd e"] - plain["ccsd e"]) < 1e-9
    assert abs(fac["(t) e"] - plain["(t) e"]) < 1e-9
    # a random rotation of the virtuals, no truncation: CCSD is invariant (the Fock matrix is no longer canonical: no (T))
    Q, _ = np.linalg.qr(np.random.default_rng(9).standard_normal((nv, nv)))
    src = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        rot = fno.derive_context(src, 0, Q)
    finally:
        src.ctx.close()
    g = f.copy()
    g[no:, no:] = Q.T @ f[no:, no:] @ Q
    try:
        er = quiet(CCSD(no, delta_e=1e-11).solve, g, rot)["ccsd e"]
    finally:
        rot.ctx.close()
    assert abs(er - plain["ccsd e"]) < 1e-9


def _host_pipeline(no, f, V, nf, k):
    U, occ, e_full, _ = ref.fno_space(no, f, V, nf, k)
    fn = U.T @ f @ U
    Vn = ref.transform(V, U)
    nn = no - nf
    res = quiet(CCSD(nn, delta_e=1e-11).solve, fn, Vn, triples=True)
    _, e_kept = ref.mp2_density(nn, fn, Vn, 0)
    return res, e_full - e_kept, occ


@pytest.mark.parametrize("cut", ["v-4", "v/2"])
def test_truncated_pipeline_against_host(gpu_lib, cut):
    no, nv, nf = 6, 24, 1
    f, V, _, _ = synthetic_case(no, nv, seed=21, scale=0.3)
    k = nv - 4 if cut == "v-4" else nv // 2
    want, dmp2, occ = _host_pipeline(no, f, V, nf, k)
    assert (occ[k - 1] - occ[k]) > 1e-6 * occ[0]                 # a gap at the cut: the kept space is well defined
    got = quiet(CCSD(no, delta_e=1e-11).solve, f, V, frozen_core=nf, fno_nv=k, triples=True)
    assert got["fno nv"] == k
    assert abs(got["ccsd e"] - want["ccsd e"]) < 1e-9
    assert abs(got["(t) e"] - want["(t) e"]) < 1e-9
    assert abs(got["fno dmp2 e"] - dmp2) < 1e-9
    assert dmp2 < 0.0 if k < nv else True


@pytest.mark.parametrize("k", [1, 2])
def test_frozen_core_matches_sliced_solve(gpu_lib, k):
    no, nv = 6, 20
    f, V, _, _ = synthetic_case(no, nv, seed=4, scale=0.3)
    want = quiet(CCSD(no - k, delta_e=1e-11).solve, f[k:, k:], np.ascontiguousarray(V[k:, k:, k:, k:]), triples=True)
    got = quiet(CCSD(no, delta_e=1e-11).solve, f, V, frozen_core=k, triples=True)
    assert abs(got["ccsd e"] - want["ccsd e"]) < 1e-10
    assert abs(got["(t) e"] - want["(t) e"]) < 1e-10
    assert got["fno dmp2 e"] == 0.0 and got["fno nv"] == nv
    assert got["t2"].shape == (nv, nv, no - k, no - k)


def test_factor_and_host_sources_agree(gpu_lib):
    no, nv = 6, 22
    f, V, B, _ = synthetic_case(no, nv, seed=8, scale=0.3)
    out = []
    for src in (V, ("factors", B)):
        r = fno.truncate(no, f, src, n_frozen=1, nv_keep=15)
        try:
            e = quiet(CCSD(r.no, delta_e=1e-11).solve, r.fock, r.ints, triples=True)
            out.append((e["ccsd e"], e["(t) e"], r.de_mp2))
        finally:
            r.close()
    assert np.abs(np.array(out[0]) - np.array(out[1])).max() < 1e-10


def test_occupation_threshold(gpu_lib):
    no, nv = 5, 18
    f, V, _, _ = synthetic_case(no, nv, seed=2, scale=0.3)
    r = fno.truncate(no, f, V, occ_threshold=1e-3)
    try:
        k = int(np.count_nonzero(r.occupations >= 1e-3))
        assert r.nv == k and r.C.shape == (nv, k) and r.fock.shape == (no + k, no + k)
        assert np.all(np.diff(r.eps_v) >= 0)
        assert np.abs(r.occupations.sum() - np.trace(ref.mp2_density(no, f, V)[0])) < 1e-10
    finally:
        r.close()


def test_refusals(gpu_lib):
    no, nv = 4, 12
    f, V, B, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    Vtc = V.copy()
    Vtc[no:, no:, :no, no:] += 1e-3 * np.random.default_rng(0).standard_normal((nv, nv, no, nv))
    with pytest.raises(Exception, match="Hermitian"):
        fno.truncate(no, f, Vtc, nv_keep=6)
    g = f.copy()
    g[0, 1] = g[1, 0] = 1e-3
    with pytest.raises(ValueError, match="canonical"):
        CCSD(no).solve(g, V, fno_nv=6)
    with pytest.raises(ValueError, match=r"n_frozen = 4 must lie in \[0, no\)"):
        CCSD(no).solve(f, V, frozen_core=no)
    for bad in (0, nv + 1):
        with pytest.raises(ValueError, match=r"nv_keep = %d must lie in \[1, nv\]" % bad):
            fno.truncate(no, f, ("factors", B), nv_keep=bad)
    sh = DeviceIntegrals.from_V_pqrs(no, V, shard=(0, 2))
    try:
        with pytest.raises(ValueError, match="sharded context"):
            fno.truncate(no, f, sh, nv_keep=6)
    finally:
        sh.ctx.close()


def test_no_leaks(gpu_lib):
    no, nv = 5, 16
    f, V, B, _ = synthetic_case(no, nv, seed=1, scale=0.3)
    n0 = _live()
    for src in (V, ("factors", B)):
        r = fno.truncate(no, f, src, n_frozen=1, nv_keep=10)
        r.close()
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    r = fno.truncate(no, f, ints, nv_keep=10)
    r.close()
    ints.ctx.close()
    assert _live() == n0


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        no, nv = 6, 20
        f, V, B, _ = synthetic_case(no, nv, seed=6, scale=0.3)
        r = quiet(CCSD(no, delta_e=1e-11, device=0).solve, f, V, frozen_core=1, fno_nv=14, triples=True)
        res["block"] = (float(r["ccsd e"]), float(r["(t) e"]), float(r["fno dmp2 e"]))
        t = fno.truncate(no, f, ("factors", B), n_frozen=1, nv_keep=14, shard=(rank, world))
        try:
            r = quiet(CCSD(t.no, delta_e=1e-11, device=0, shard_integrals=True).solve, t.fock, t.ints, triples=True)
            res["factors"] = (float(r["ccsd e"]), float(r["(t) e"]), float(t.de_mp2))
        finally:
            t.close()
        out[rank] = res
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu(gpu_lib):
    import torch.multiprocessing as mp
    no, nv = 6, 20
    f, V, B, _ = synthetic_case(no, nv, seed=6, scale=0.3)
    single = quiet(CCSD(no, delta_e=1e-11).solve, f, V, frozen_core=1, fno_nv=14, triples=True)
    want = np.array([single["ccsd e"], single["(t) e"], single["fno dmp2 e"]])
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    assert len(out) == 2 and out[0] == out[1]
    for key in ("block", "factors"):
        assert np.abs(np.array(out[0][key]) - want).max() < 1e-9, key


def fno_plan(noa, nv):
    """fno_plan of kernels_post.hip (64-wide tiles, 32-wide c chunks, about 1024 blocks): (nt, nchunk, kc_tot, want, nsplit)."""
    nt, nchunk = -(-nv // 64), -(-nv // 32)
    ntp, kc_tot = nt * (nt + 1) // 2, noa * noa * nchunk
    want = max(1, min(-(-1024 // ntp), kc_tot, 65535))
    kc_per = -(-kc_tot // want)
    return nt, nchunk, kc_tot, want, -(-kc_tot // kc_per)


# (no, n_frozen, nv): every nv of the list, active occupied 1, 3 and >= 12, with and without a frozen core
TILE_CASES = [(1, 0, 32), (13, 1, 32), (2, 1, 33), (3, 0, 63), (12, 0, 63), (5, 2, 64), (1, 0, 64), (12, 0, 65), (2, 1, 65),
              (4, 1, 96), (3, 0, 96), (1, 0, 128), (14, 2, 128), (3, 0, 129), (12, 0, 129), (2, 1, 200), (5, 2, 200),
              (13, 1, 200)]


def test_density_across_tiles(gpu_lib):
    """fno_density_kernel beyond one 64 x 64 tile: the off-diagonal tile pairs (unrank_pair), the (max, min) mirror of the finish
    kernel, the E_MP2 partials of row tiles > 0 and several 32-wide c chunks, on V_ijab = sum_Q B[Q,i,a] B[Q,j,b] built on the
    device, against the numpy statement of the definition."""
    plans = {c: fno_plan(c[0] - c[1], c[2]) for c in TILE_CASES}
    assert {nv for _, _, nv in TILE_CASES} == {32, 33, 63, 64, 65, 96, 128, 129, 200}
    assert {no - nf for no, nf, _ in TILE_CASES} >= {1, 3} and max(no - nf for no, nf, _ in TILE_CASES) >= 12
    assert any(p[2] < -(-1024 // (p[0] * (p[0] + 1) // 2)) for p in plans.values())      # kc_tot < the wanted split count
    assert max(p[4] for p in plans.values()) >= 100                                        # many splits
    for case in TILE_CASES:
        no, nf, nv = case
        nt = plans[case][0]
        rng = np.random.default_rng(no * 1000 + nv)
        B = rng.standard_normal((24, no, nv)) * 0.1
        eps_o = np.sort(rng.uniform(-2.0, -0.5, no))
        eps_v = np.sort(rng.uniform(0.3, 3.0, nv))
        ctx = Context(no, nv, lib=gpu_lib)
        try:
            Bd = ctx.array(B)
            Vd = ctx.contract("Qia,Qjb->ijab", Bd, Bd)
            ctx.set_orbital_energies(eps_o, eps_v)
            D, e = fno.density(ctx, nf, Vd)
            D2, e2 = fno.density(ctx, nf, Vd)
            Vijab = Vd.get()
        finally:
            ctx.close()
        D_ref, e_ref = ref.mp2_density_ijab(Vijab, eps_o, eps_v, nf)
        if nt >= 2:
            # a transposed tile store would show here: the block of the tile pair (1, 0), zero-padded to 64 x 64, is far from
            # its transpose (at nt = 1 the tile is symmetric and the mirror hides the transposition)
            h = min(64, nv - 64)
            M = np.zeros((64, 64))
            M[:h] = D_ref[64:64 + h, :64]
            assert np.abs(M - M.T)[:h].max() > 0.1 * np.abs(M).max(), case
        assert np.abs(D - D_ref).max() <= 1e-12 * np.abs(D_ref).max(), case
        assert abs(e - e_ref) <= 1e-12 * abs(e_ref), case
        assert np.array_equal(D, D2) and e == e2, case


def test_truncate_factors_multi_tile(gpu_lib):
    """fno.truncate on the production route (the ('factors', B) source, frozen core) with more than 64 kept virtuals, so that
    both density calls — full space and kept space — run on several tiles, against a numpy restatement from B alone."""
    from oracle.io_oracle import synthetic_factors
    no, nv, nf, k = 10, 150, 1, 80
    B, eps = synthetic_factors(no, nv, seed=12, scale=0.3)
    f = np.diag(eps)
    r = fno.truncate(no, f, ("factors", B), n_frozen=nf, nv_keep=k)
    try:
        got = (r.occupations.copy(), r.eps_v.copy(), r.C.copy(), r.de_mp2, r.e_mp2_full, r.nv, r.no)
    finally:
        r.close()
    Bov = B[:, :no, no:]
    D, e_full = ref.mp2_density_ijab(np.einsum("Qia,Qjb->ijab", Bov, Bov, optimize=True), eps[:no], eps[no:], nf)
    occ, vec = np.linalg.eigh(D)
    order = np.argsort(-occ, kind="stable")
    occ, N = occ[order], ref.sign_rule(vec[:, order])[:, :k]
    assert occ[k - 1] - occ[k] > 1e-3 * (occ[k - 1] - occ[-1])            # a gap at the cut: the kept space is well defined
    w, W = np.linalg.eigh(N.T @ f[no:, no:] @ N)
    Cm = ref.sign_rule(N @ W)
    Bn = np.einsum("Qia,ax->Qix", B[:, nf:no, no:], Cm, optimize=True)
    _, e_kept = ref.mp2_density_ijab(np.einsum("Qia,Qjb->ijab", Bn, Bn, optimize=True), eps[nf:no], w, 0)
    occ_g, eps_g, C_g, de_g, e_full_g, nv_g, no_g = got
    assert (nv_g, no_g) == (k, no - nf)
    assert np.abs(occ_g - occ).max() <= 1e-12 * occ[0]
    # (the kept space turns by |dD| / gap at the cut, about 1e-12 for a rounding-level dD, and the semicanonical rotation by
    # that times |f| / min spacing of eps')
    assert np.abs(eps_g - w).max() <= 1e-9 * np.abs(w).max()
    assert np.abs(C_g - Cm).max() < 1e-6
    assert abs(e_full_g - e_full) <= 1e-12 * abs(e_full)
    assert abs(de_g - (e_full - e_kept)) <= 1e-8 * abs(e_full)
    assert de_g < 0.0
