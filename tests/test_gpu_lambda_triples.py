"""GPU: Lambda-CCSD(T) (include/pymes_amd.h, pymes_ccsd_t_lambda; pymes_amd/solver/ccsd_t.py) against the numpy loop over the
unique triples (tests/_lambda_triples_reference.py): integrals without V_pqrs = V_rspq at tile-edge sizes, the Hermitian limit
against the device's own (T), per-triple values across batch boundaries with a second lane trip, batch-size and rank-chunk
reproducibility, a sharded-integral context, the transcorrelated electron gas end to end, CCSD.solve(triples="lambda") and the
refusals.

Every bound against the reference is relative to the ABS-SUM SCALE of the reference (sum m_ijk / 3 sum_abc |WR R(YL) / D|): the
terms of E_Lambda(T) for independent left and right amplitudes have both signs, so the energy itself can cancel.  1e-12 is the
bound the (T) tests assert on same-sign sums of the same products.

Observed E_Lambda(T) / E(T) of the two CCSD.solve fixtures: profiles/lambda_triples/INDEX.md."""
import contextlib
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.solver import ccsd_t
from tests import _lambda_triples_reference as LT
from tests import _triples_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _hermitian_limit(no, nv, seed):
    """(f, V, B, eps, t1, t2, lam1, lam2): Hermitian integrals with L = T, l1 = t1, where E_Lambda(T) = E(T)."""
    f, V, B, eps = synthetic_case(no, nv, seed=seed)
    t1, t2 = R.random_amplitudes(no, nv, seed=seed + 1, amp=0.05)
    lam1, lam2 = LT.library_normalisation(t1, t2)
    return f, V, B, eps, t1, t2, lam1, lam2


@pytest.mark.parametrize("no,nv", [(2, 6), (4, 12), (5, 19), (7, 33), (8, 40), (5, 3), (6, 4), (20, 10)])
def test_non_hermitian_against_reference(gpu_lib, no, nv):
    f, V, eps, T, lam1, lam2 = LT.problem(no, nv, seed=no + nv)
    assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-3         # left and right blocks exchanged: a different number
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        for l1, (ref, scale) in zip((lam1, None), LT.energy_with_and_without_lam1(no, V, eps, T, lam1, lam2)):
            e = ccsd_t.get_lambda_triples_energy(no, f, ints, T, l1, lam2)
            print(no, nv, "lam1" if l1 is not None else "no lam1", "e = %.15e ref = %.15e |e - ref| / scale = %.2e"
                  % (e, ref, abs(e - ref) / scale))
            assert abs(e - ref) <= 1e-12 * scale, (e, ref, scale)
    finally:
        ints.ctx.close()


@pytest.mark.parametrize("no,nv", [(5, 19), (8, 40)])
def test_hermitian_limit_equals_device_triples(gpu_lib, no, nv):
    f, V, B, eps, t1, t2, lam1, lam2 = _hermitian_limit(no, nv, seed=no + nv)
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        e_t = ccsd_t.get_triples_energy(no, f, ints, t1, t2)
        e_l = ccsd_t.get_lambda_triples_energy(no, f, ints, t2, lam1, lam2)
        print(no, nv, "E(T) = %.15e E_Lambda(T) = %.15e rel = %.2e" % (e_t, e_l, abs(e_l - e_t) / abs(e_t)))
        assert abs(e_l - e_t) <= 1e-12 * abs(e_t), (e_l, e_t)
    finally:
        ints.ctx.close()


def test_per_triple_ranges_second_lane_trip_6_70(gpu_lib, monkeypatch):
    """v = 70 > 64: a lane takes a second orbit; batches of two triples, ranges over batch boundaries."""
    no, nv = 6, 70
    f, V, eps, T, lam1, lam2 = LT.problem(no, nv, seed=8)
    n = R.n_triples(no)
    monkeypatch.setenv("PYMES_TRIPLES_BATCH", "2")
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        for lo, hi in ((0, 3), (n // 2 - 1, n // 2 + 2), (n - 3, n)):
            e, vec = ccsd_t.get_lambda_triples_energy(no, f, ints, T, lam1, lam2, triple_range=(lo, hi), per_triple=True)
            ref, scale = LT.per_triple(no, V, eps, T, lam1, lam2, lo, hi)
            assert vec.shape == (hi - lo,)
            print(lo, hi, "max |vec - ref| / max scale = %.2e" % (np.abs(vec - ref).max() / scale.max()))
            assert np.abs(vec - ref).max() <= 1e-12 * scale.max(), (lo, hi, vec, ref, scale)
            assert abs(e - ref.sum()) <= 1e-12 * scale.sum()
    finally:
        ints.ctx.close()


def test_batch_size_and_rank_chunks_9_40(gpu_lib, monkeypatch):
    no, nv = 9, 40
    f, V, eps, T, lam1, lam2 = LT.problem(no, nv, seed=11)
    n = R.n_triples(no)
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        d2, dl1, dl2 = ints.ctx.array(T), ints.ctx.array(lam1), ints.ctx.array(lam2)
        run = lambda **k: ccsd_t.get_lambda_triples_energy(no, f, ints, d2, dl1, dl2, **k)
        monkeypatch.delenv("PYMES_TRIPLES_BATCH", raising=False)
        e_def, v_def = run(per_triple=True)
        monkeypatch.setenv("PYMES_TRIPLES_BATCH", "1")
        e_one, v_one = run(per_triple=True)
        monkeypatch.setenv("PYMES_TRIPLES_BATCH", "7")
        e_sev, v_sev = run(per_triple=True)
        assert np.array_equal(v_def, v_one) and np.array_equal(v_def, v_sev)
        assert e_def == e_one == e_sev
        chunks = [ccsd_t.rank_range(no, r, 3) for r in range(3)]
        assert chunks[0][0] == 0 and chunks[-1][1] == n
        parts = [run(triple_range=c) for c in chunks]
        ref, scale = LT.per_triple(no, V, eps, T, lam1, lam2)
        assert np.abs(v_def - ref).max() <= 1e-12 * scale.max()
        assert abs(sum(parts) - e_def) <= 1e-14 * scale.sum(), (parts, e_def, scale.sum())
        for d in (d2, dl1, dl2):
            d.free()
    finally:
        ints.ctx.close()


def test_sharded_integrals_same_bits_6_24(gpu_lib):
    no, nv = 6, 24
    f, V, B, eps, t1, t2, lam1, lam2 = _hermitian_limit(no, nv, seed=5)
    full = DeviceIntegrals.from_factors(no, B)
    shard = DeviceIntegrals.from_factors(no, B, shard=(1, 2))
    try:
        # a dressing of the blocks on the same context does not touch what the call reads
        quiet(shard.ctx.dress_V, shard.ctx.array(t1), ("iabc", "ijak", "ijab"))
        e_full, v_full = ccsd_t.get_lambda_triples_energy(no, f, full, t2, lam1, lam2, per_triple=True)
        e_shard, v_shard = ccsd_t.get_lambda_triples_energy(no, f, shard, t2, lam1, lam2, per_triple=True)
        assert e_full == e_shard and np.array_equal(v_full, v_shard)
        ref = R.energy(no, V, eps, t1, t2)
        assert abs(e_full - ref) <= 1e-12 * abs(ref)
    finally:
        full.ctx.close()
        shard.ctx.close()


def test_transcorrelated_electron_gas_end_to_end(gpu_lib):
    """14 electrons in 19 plane waves (cutoff 2: the smallest basis with more than the 7 occupied plane waves), transcorrelated
    two-body integrals: CCD, then Lambda on the undressed blocks with t1 = 0, then Lambda-CCSD(T); (T) itself refuses them."""
    from pymes_amd.model.ueg import UEG
    from pymes_amd.solver import ccd
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    from tests.test_ueg import G, tc_problem
    ref = G["tc_N14_rs1.0_c2"]
    no, V, f, _, _, _, _, _ = tc_problem(UEG, ref["nel"], ref["rs"], 2, ref["k_cutoff"])
    n = V.shape[0]
    assert no == 7 and n == 19
    assert np.abs(f - np.diag(np.diag(f))).max() <= 1e-10
    assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-6 * np.abs(V).max()
    assert np.abs(V - V.transpose(1, 0, 3, 2)).max() <= 1e-12 * np.abs(V).max()
    t2 = quiet(ccd.CCD(no, delta_e=1e-10).solve, f, V)["t2 amp"]
    out = quiet(Lambda_CCSD(no).solve, f, oc.split_blocks(no, V), t2)
    assert out["converged"]
    lam1, lam2 = out["lambda1"], out["lambda2"]
    eps = np.diag(f).copy()
    for l1 in (None, lam1, np.zeros_like(lam1)):
        e = ccsd_t.get_lambda_triples_energy(no, f, V, t2, l1, lam2)
        e_ref, scale = LT.energy(no, V, eps, t2, l1, lam2)
        print("TC UEG (7,12): E_Lambda(T) = %.12e ref = %.12e |e - ref| / scale = %.2e" % (e, e_ref, abs(e - e_ref) / scale))
        assert abs(e_ref) > 1e-8
        assert abs(e - e_ref) <= 1e-11 * scale, (e, e_ref, scale)
    with pytest.raises(_lib.PymesError, match="Hermitian"):
        ccsd_t.get_triples_energy(no, f, V, None, t2)


def _fcidump_problem(tag, tmp_path):
    from pymes_amd.mean_field import hf
    from pymes_amd.util import fcidump
    if tag.startswith("syn_"):
        path = str(tmp_path / ("FCIDUMP." + tag))
        with gzip.open(os.path.join(GOLD, "fcidump", "FCIDUMP.%s.gz" % tag), "rb") as src, open(path, "wb") as dst:
            dst.write(src.read())
    else:
        path = os.path.join(GOLD, "fcidump", "FCIDUMP." + tag)
    ne, n, ec, eps, h, V = quiet(fcidump.read, path)
    no = ne // 2
    f = hf.construct_hf_matrix(no, h, V)
    # canonical orbitals: the HF matrix of these files is diagonal up to rounding
    f = np.diag(np.diag(f)) if np.abs(f - np.diag(np.diag(f))).max() < 1e-6 else f
    return no, f, V


@pytest.mark.parametrize("tag", ["LiH.321g", "syn_5_19"])
def test_ccsd_solve_triples_lambda(gpu_lib, tag, tmp_path, monkeypatch):
    from pymes_amd.solver import lambda_ccsd
    from pymes_amd.solver.ccsd import CCSD
    no, f, V = _fcidump_problem(tag, tmp_path)
    solves = []
    plain = lambda_ccsd.Lambda_CCSD.solve
    monkeypatch.setattr(lambda_ccsd.Lambda_CCSD, "solve", lambda self, *a, **k: (solves.append(1), plain(self, *a, **k))[1])
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        s = CCSD(no, delta_e=1e-11)
        res = quiet(s.solve, f, ints, triples="lambda", density=True)
        for key in ("lambda (t) e", "ccsd(t)_lambda e", "lambda1", "lambda2", "rdm1"):
            assert key in res, key
        assert "(t) e" not in res
        assert res["ccsd(t)_lambda e"] == res["ccsd e"] + res["lambda (t) e"]
        # with density=True Lambda is solved once: one call, one history
        assert len(solves) == 1
        assert len(s.lambda_solver.history) == s.lambda_solver.iterations and s.lambda_solver.converged
        e = ccsd_t.get_lambda_triples_energy(no, f, ints, res["t2"], res["lambda1"], res["lambda2"])
        assert e == res["lambda (t) e"]
        e_ref, scale = LT.energy(no, V, np.diag(f).copy(), res["t2"], res["lambda1"], res["lambda2"])
        assert abs(e - e_ref) <= 1e-11 * scale, (e, e_ref, scale)
        # without density=True: the same correction, no density
        res2 = quiet(CCSD(no, delta_e=1e-11).solve, f, ints, triples="lambda")
        assert "rdm1" not in res2 and "lambda2" in res2
        assert abs(res2["lambda (t) e"] - res["lambda (t) e"]) <= 1e-8 * abs(res["lambda (t) e"])
        rt = quiet(CCSD(no, delta_e=1e-11).solve, f, ints, triples=True)
        ratio = res["lambda (t) e"] / rt["(t) e"]
        print(tag, "lambda (t) e = %.12e (t) e = %.12e ratio = %.6f" % (res["lambda (t) e"], rt["(t) e"], ratio))
        if tag == "LiH.321g":       # a weakly correlated molecule: the two corrections are close
            assert 0.8 <= ratio <= 1.25, ratio
    finally:
        ints.ctx.close()


def test_ccsd_solve_triples_lambda_in_a_truncated_space(gpu_lib):
    """frozen_core / fno_nv: Lambda and Lambda-(T) are those of the correlated space, as for triples=True and density=True."""
    from pymes_amd.solver import fno
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 5, 19
    f, V, _, _ = synthetic_case(no, nv, seed=2)
    res = quiet(CCSD(no, delta_e=1e-11).solve, f, V, triples="lambda", frozen_core=1, fno_nv=12)
    assert res["fno nv"] == 12 and res["lambda2"].shape == (12, 12, no - 1, no - 1)
    assert res["ccsd(t)_lambda e"] == res["ccsd e"] + res["lambda (t) e"]
    r = quiet(fno.truncate, no, f, V, n_frozen=1, nv_keep=12)
    try:
        two = quiet(CCSD(r.no, delta_e=1e-11).solve, r.fock, r.ints, triples="lambda")
    finally:
        r.close()
    assert abs(res["lambda (t) e"]) > 1e-8
    assert abs(res["lambda (t) e"] - two["lambda (t) e"]) <= 1e-9 * abs(two["lambda (t) e"])


def test_refusals_leave_no_allocation(gpu_lib):
    from pymes_amd.device import Context
    from pymes_amd.solver.ccsd import CCSD
    E = _lib.PymesError
    before = _live()
    no, nv = 3, 8
    f, V, B, eps, t1, t2, lam1, lam2 = _hermitian_limit(no, nv, seed=2)
    # CCSD.solve: refused by name before anything is uploaded
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, triples="lambda")
    with pytest.raises(ValueError, match="shard_integrals"):
        CCSD(no, shard_integrals=True).solve(f, V, triples="lambda")
    with pytest.raises(ValueError, match="'perturbative'"):
        CCSD(no).solve(f, V, triples="perturbative")
    with pytest.raises(E, match="nocc = 89"):
        CCSD(89).solve(f, V, triples="lambda")
    assert _live() == before
    # non-canonical orbitals
    g = f.copy()
    g[0, no] = g[no, 0] = 1e-3
    with pytest.raises(ValueError, match="canonical"):
        ccsd_t.get_lambda_triples_energy(no, g, V, t2, lam1, lam2)
    with pytest.raises(ValueError, match="canonical"):
        CCSD(no).solve(g, V, triples="lambda")
    # integrals without V_pqrs = V_qpsr: the block pair is named
    X = V + 0.01 * np.random.default_rng(1).standard_normal(V.shape)
    with pytest.raises(E, match=r"V_pqrs = V_qpsr.*V_iabc"):
        ccsd_t.get_lambda_triples_energy(no, f, X, t2, lam1, lam2)
    assert _live() == before
    # a missing block, graph capture
    ctx = Context(no, nv)
    try:
        d2, dl1, dl2 = ctx.array(t2), ctx.array(lam1), ctx.array(lam2)
        for name in ("klij", "ijka", "ijak", "ijab", "iajk", "iajb", "iabj", "abij"):
            sl = tuple(slice(no, None) if ch in "abcd" else slice(0, no) for ch in name)
            ctx.set_V_block(name, np.ascontiguousarray(V[sl]))
        with pytest.raises(E, match="'iabc'"):
            ccsd_t.lambda_triples_energy(ctx, eps, d2, dl1, dl2, 0, 4)
        ctx.set_V_pqrs(V)
        assert ctx.graphs_supported()
        ctx.graph_begin()
        try:
            with pytest.raises(E, match="launch graph"):
                ccsd_t.lambda_triples_energy(ctx, eps, d2, dl1, dl2, 0, 4)
        finally:
            ctx.graph_abort()
        e, _ = ccsd_t.lambda_triples_energy(ctx, eps, d2, dl1, dl2, 0, R.n_triples(no))
        ref = R.energy(no, V, eps, t1, t2)
        assert abs(e - ref) <= 1e-12 * abs(ref)
        for d in (d2, dl1, dl2):
            d.free()
    finally:
        ctx.close()
    assert _live() == before
