"""CPU: the numpy restatement of the sector IP- / EA-EOM-CCD sigma (tests/_sector_ipea_reference.py) against the dense term
tables of tests/_ipea_reference.py -- the whole momentum block at 19 plane waves, seeded vectors where the dense matrix is too
large --, the tables of pymes_amd/solver/sectors.py (QuasiparticleTables), and the refusal of the host simulator, which has no
sector kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cc_oracle as oc
from pymes_amd.solver import sectors
from pymes_amd.solver.sectors import QuasiparticleTables, TriplesTables
from tests import _ipea_reference as ip
from tests import _sector_ipea_reference as sq
from tests import _sector_reference as sr
from tests.test_sector_lambda_reference import exchange_only, twist_problem
from tests.test_sector_reference import problem, symmetric_amplitudes

KINDS = ("ip", "ea")


def all_targets(tab, kind):
    return list(range(tab.no)) if kind == "ip" else list(range(tab.no, tab.n))


def some_targets(tt, kind):
    """The lowest and the highest admissible orbital, and the first one whose block has positions outside the space."""
    tab = tt.tables
    every = all_targets(tab, kind)
    picked = [every[0], every[-1]]
    holes = [p for p in every if not QuasiparticleTables(tt, kind, p).inside.all() and p not in picked]
    return picked + holes[:1] if holes else every[:3]


@functools.lru_cache(maxsize=None)
def host_case(label):
    """(tables, triples tables, dense V, orbital energies, sector families, implied-index lists)"""
    if label == "twist":
        tab, V, eps = twist_problem()
    else:
        nel, cutoff, mode = label
        if mode == "exchange":
            u, tab, V, _ = problem(nel, cutoff, "coulomb")
            V = exchange_only(V, 21)
        else:
            u, tab, V, _ = problem(nel, cutoff, mode)
        eps = sr.hf_orbital_energies(tab, sr.sector_integrals(tab, V), u.kinetic)
    tt = TriplesTables(tab)
    return tab, tt, V, eps, sr.sector_integrals(tab, V), sq.triples_lists(tt, V)


def block_of(tab, tt, V, ints, lists, qt):
    pq = qt.extra_pqrs()
    return sq.blocks(tab, tt, ints, lists, ladder=[(pq, V[pq[:, 0], pq[:, 1], pq[:, 2], pq[:, 3]])])


def dense_index(qt):
    """The elements of the dense [r1 | r2] vector that the block holds: the singles element, then the positions inside."""
    tab, no, nv = qt.tables, qt.tables.no, qt.tables.nv
    pos = np.flatnonzero(qt.inside)
    x, y, b = pos // no, pos % no, qt.b_of[pos].astype(np.int64)
    if qt.kind == "ip":
        return np.concatenate([[qt.target], no + (x * no + y) * nv + b]), pos
    return np.concatenate([[qt.target - no], nv + (x * nv + b) * no + y]), pos


@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("kind", KINDS)
def test_block_matrix_is_the_momentum_block_of_the_dense_operator(kind, mode):
    """N = 14 in 19 plane waves, every admissible target: the restatement on the unit vectors of the block against the
    momentum block of _ipea_reference.dense, to 1e-13 max|H| (the bound of test_residual_matches_the_dense_oracle); the dense
    matrix has exact zeros between different momenta; positions outside the space give zero rows and columns."""
    tab, tt, V, eps, ints, lists = host_case((14, 2, mode))
    no = tab.no
    T = 0.1 * symmetric_amplitudes(tab, 5)
    H = ip.dense(kind, no, np.diag(eps), oc.split_blocks(no, np.array(V)), tab.to_dense(T))
    scale, worst, seen = np.abs(H).max(), 0.0, np.zeros(H.shape[0], dtype=bool)
    for p in all_targets(tab, kind):
        qt = QuasiparticleTables(tt, kind, p)
        Hs = sq.matrix(qt, eps, block_of(tab, tt, V, ints, lists, qt), T)
        idx, pos = dense_index(qt)
        mine = np.concatenate([[0], 1 + pos])
        worst = max(worst, np.abs(Hs[np.ix_(mine, mine)] - H[np.ix_(idx, idx)]).max())
        rest = np.setdiff1d(np.arange(H.shape[0]), idx)
        assert np.count_nonzero(H[np.ix_(idx, rest)]) == 0 and np.count_nonzero(H[np.ix_(rest, idx)]) == 0
        outside = 1 + np.flatnonzero(~qt.inside)
        assert np.count_nonzero(Hs[outside]) == 0 and np.count_nonzero(Hs[:, outside]) == 0
        seen[idx] = True
    print(f"{kind} {mode}: max|restatement - dense| = {worst:.2e}, max|H| = {scale:.2e}")
    assert worst <= 1e-13 * scale
    assert seen[:no if kind == "ip" else tab.nv].all()


BIG = [(14, 3, "coulomb"), (14, 3, "tc"), (14, 5, "coulomb"), (14, 5, "tc"), (54, 5, "coulomb"), (14, 3, "exchange"),
       (14, 5, "exchange"), "twist"]


@pytest.mark.parametrize("label", BIG, ids=str)
def test_sigma_matches_the_dense_term_tables_on_seeded_vectors(label):
    """Where the dense matrix is too large: _ipea_reference.sigma_terms on seeded vectors of the block embedded into the
    dense shapes, three targets per kind, 1e-13 of the largest element.  "exchange" scales V element by element so that only
    V_pqrs = V_qpsr is left; the twisted basis has q without -q."""
    tab, tt, V, eps, ints, lists = host_case(label)
    no, nv = tab.no, tab.nv
    if label == "twist":
        assert (tab.neg < 0).any()
    T = 0.1 * symmetric_amplitudes(tab, 5)
    Vd, Td, f = oc.split_blocks(no, np.array(V)), tab.to_dense(T), np.diag(eps)
    rng = np.random.default_rng(9)
    for kind in KINDS:
        for p in some_targets(tt, kind):
            qt = QuasiparticleTables(tt, kind, p)
            r1 = rng.standard_normal(2)
            R = rng.standard_normal((2,) + qt.shape) * qt.inside.reshape(qt.shape)
            s1, S, leak = sq.sigma(qt, eps, block_of(tab, tt, V, ints, lists, qt), T, r1, R)
            assert leak == 0.0
            idx, pos = dense_index(qt)
            shape1, shape2 = ip.shapes(kind, no, nv)
            for z in range(2):
                flat = np.zeros(ip.dim(kind, no, nv))
                flat[idx] = np.concatenate([[r1[z]], R[z].reshape(-1)[pos]])
                n1 = int(np.prod(shape1))
                w1, w2 = ip.sigma_terms(kind, no, f, Vd, Td, flat[:n1].reshape(shape1), flat[n1:].reshape(shape2))
                want = np.concatenate([w1.ravel(), w2.ravel()])
                got = np.concatenate([[s1[z]], S[z].reshape(-1)[pos]])
                scale = np.abs(want).max()
                err = np.abs(got - want[idx]).max()
                want[idx] = 0.0
                print(f"{label} {kind} target {p} (dim {qt.dim}, extra {qt.extra_size}): |restatement - dense| = {err:.2e}, "
                      f"max|sigma| = {scale:.2e}, outside the block {np.abs(want).max():.1e}")
                assert err <= 1e-13 * scale
                assert np.count_nonzero(want) == 0                        # the dense sigma stays in the block, exactly
                assert np.count_nonzero(S[z].reshape(-1)[~qt.inside]) == 0


@pytest.mark.parametrize("label", [(14, 2, "coulomb"), (14, 5, "coulomb"), (54, 5, "coulomb"), "twist"], ids=str)
def test_tables_are_bijections_and_the_task_tables_are_checked(label):
    tab, tt = host_case(label)[:2]
    for kind in KINDS:
        for p in all_targets(tab, kind):
            qt = QuasiparticleTables(tt, kind, p)
            qt.check()
            inside = qt.inside
            assert qt.dim == 1 + inside.sum() and qt.shape == ((tab.no if kind == "ip" else tab.nv), tab.no)
            for m in (qt.ph, qt.ph_partner, qt.pair):
                assert m.min() >= -1 and m.max(initial=-1) < qt.count
                assert np.array_equal(np.sort(m[inside]), np.arange(qt.count)) and (m[~inside] == -1).all()
            assert np.array_equal(qt.partner[qt.partner[inside]], np.flatnonzero(inside))
            assert (qt.b_of[inside] >= 0).all() and (qt.b_of < tab.nv).all()
            # the implied orbital carries the momentum of the block
            x, y = np.divmod(np.flatnonzero(inside), tab.no)
            k, b = tab.k_int, tab.no + qt.b_of[inside]
            if kind == "ip":
                assert np.array_equal(k[b] - k[x] - k[y], np.broadcast_to(-k[p], (len(x), 3)))
            else:
                assert np.array_equal(k[tab.no + x] + k[b] - k[y], np.broadcast_to(k[p], (len(x), 3)))
            for nk in (1, 3, 17):
                for name, (tasks, la, lb, lc) in qt.tasks(nk).items():
                    sectors.check_tasks(tasks, la, lb, lc)
                    assert (tasks["n"] == nk).all()
            assert len(qt.extra_pqrs()) == qt.extra_size
            if kind == "ip":
                assert qt.extra_size == 0
    with pytest.raises(ValueError, match="is not an occupied orbital"):
        QuasiparticleTables(tt, "ip", tab.no)
    with pytest.raises(ValueError, match="is not a virtual orbital"):
        QuasiparticleTables(tt, "ea", 0)
    nsq = int(tab.offsets("ph", "ph")[-1])
    tr = sectors.square_transpose(tab)
    assert np.array_equal(np.sort(tr), np.arange(nsq)) and np.array_equal(tr[tr], np.arange(nsq))


def test_the_ea_ladder_needs_pair_momenta_outside_the_stored_sectors():
    """k_p + k_j with p virtual need not be a sum of two occupied momenta: those V_abcd blocks are the one family the
    sector integrals do not hold (SectorLadderIntegrals).  At 57 plane waves every EA target has some."""
    tab, tt = host_case((14, 5, "coulomb"))[:2]
    sizes = [QuasiparticleTables(tt, "ea", p).extra_size for p in all_targets(tab, "ea")]
    assert min(sizes) > 0
    qt = QuasiparticleTables(tt, "ea", tab.no)
    pq = qt.extra_pqrs()
    assert tab.conserving(pq).all() and (pq >= tab.no).all()
    k = tab.k_int
    stored = {tuple(v) for v in tab.P}
    assert all(tuple(k[a] + k[b]) not in stored for a, b in pq[:, :2])


def test_the_host_simulator_refuses_the_new_entries_by_name(hostsim_lib):
    from pymes_amd._lib import PymesError
    from pymes_amd.device import Context
    ctx = Context(1, 1, lib=hostsim_lib)
    try:
        x = ctx.zeros((4,))
        m = ctx.zeros((4,))
        p, pp = C.c_void_p(x.ptr), (C.c_void_p * 1)(x.ptr)
        box = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
        with pytest.raises(PymesError, match="sector_ipea_prepare: not available in this backend"):
            ctx.lib.call("pymes_sector_ipea_prepare", ctx.handle, 0, 0, 1, 1, p, p, box.ctypes.data_as(C.c_void_p), *[p] * 7, -1.0,
                         p, p, p)
        with pytest.raises(PymesError, match="sector_ipea_pack: not available in this backend"):
            ctx.lib.call("pymes_sector_ipea_pack", ctx.handle, 1, pp, 1, *[C.c_void_p(m.ptr)] * 3, p, p, p)
        with pytest.raises(PymesError, match="sector_ipea_assemble: not available in this backend"):
            ctx.lib.call("pymes_sector_ipea_assemble", ctx.handle, 1, pp, pp, pp, pp, 1, *[C.c_void_p(m.ptr)] * 3, p, p, p, 0.0,
                         p, p, p)
        with pytest.raises(PymesError, match="sector_ipea_correction: the flat layout"):
            out = np.zeros(2)
            ctx.lib.call("pymes_sector_ipea_correction", ctx.handle, 1, pp, pp, out.ctypes.data_as(C.c_void_p), p, 0.0, pp, 0, 0,
                         0, out.ctypes.data_as(C.c_void_p))
    finally:
        ctx.close()


def test_header_and_signatures_name_the_new_entries():
    import os
    from pymes_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pymes_amd.h")).read()
    for name in ("pymes_sector_ipea_prepare", "pymes_sector_ipea_pack", "pymes_sector_ipea_assemble",
                 "pymes_sector_ipea_correction"):
        assert name in _lib.SIGNATURES and ("int " + name + "(") in header
