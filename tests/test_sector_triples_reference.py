"""CPU: the implied-index tables of the momentum-blocked (T) (pymes_amd/solver/sectors.py, TriplesTables) and its numpy
restatement (tests/_sector_triples_reference.py) against tests/_triples_reference.per_triple on dense electron-gas integrals
of oracle.ueg_oracle, and on a k-list that is not inversion-symmetric."""
import functools
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.ueg_oracle import Ueg
from tests import _sector_reference as sr
from tests import _sector_triples_reference as tr
from tests import _triples_reference as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [(2, 1), (14, 2), (14, 3), (14, 5), (54, 5)]


@functools.lru_cache(maxsize=None)
def problem(nel, cutoff):
    """(no, tables, triples tables, dense Coulomb V, HF orbital energies, compact MP2 amplitudes)"""
    u = Ueg(nel, 1.0)
    u.init_basis(cutoff)
    V = u.two_body("coulomb")
    V.setflags(write=False)
    no = nel // 2
    tab, tt = tr.tables_for(u.k_int, no)
    ints = sr.sector_integrals(tab, V)
    eps = sr.hf_orbital_energies(tab, ints, u.kinetic)
    return no, tab, tt, V, eps, ints["abij"] / tab.denominators(eps)


def symmetric_amplitudes(tab, seed, amp=0.05):
    T = np.random.default_rng(seed).standard_normal(tab.nnz) * amp
    return 0.5 * (T + T[tab.pp_swap])


def compare(no, tab, tt, V, eps, T):
    """Worst per-triple difference of the restatement from the dense reference, and the reference values."""
    blk = tuple(np.ascontiguousarray(x) for x in R.blocks(no, V))        # the same blocks, contiguous: einsum runs twice as fast
    want = R.per_triple(no, V, eps, None, tab.to_dense(T), blk=blk)
    got, _ = tr.per_triple(tt, eps, *tr.triples_integrals(tt, V), tt.implied(T))
    return np.abs(got - want).max(), want, got


@pytest.mark.parametrize("nel,cutoff", CASES)
@pytest.mark.parametrize("amps", ["mp2", "random"])
def test_restatement_matches_the_dense_reference(nel, cutoff, amps):
    no, tab, tt, V, eps, mp2 = problem(nel, cutoff)
    T = mp2 if amps == "mp2" else symmetric_amplitudes(tab, 3)
    err, want, got = compare(no, tab, tt, V, eps, T)
    scale = np.abs(want).max()
    print(f"N={nel} cutoff={cutoff} {amps}: E(T) = {want.sum():.16e}, max|per triple| = {scale:.2e}, worst difference {err:.1e}")
    assert err <= 1e-13 * scale
    assert len(want) == R.n_triples(no)
    if (nel, cutoff) == (2, 1):
        assert len(want) == 1 and want[0] == 0.0 and got[0] == 0.0
    if (nel, cutoff) == (14, 2):                    # no virtual triple carries the momentum of these occupied triples
        assert np.count_nonzero(want == 0.0) == 62 and np.array_equal(want == 0.0, got == 0.0)
        if amps == "mp2":
            assert abs(want.sum() - -0.0026563666932396725) < 1e-15
    if (nel, cutoff) == (14, 3):
        assert np.count_nonzero(want == 0.0) == 0
        if amps == "mp2":
            assert abs(want.sum() - -0.013070069823249675) < 1e-15
    if (nel, cutoff) == (54, 5):
        assert tt.no == 27 and tt.nv == 30 and (tt.m_of >= 0).mean() > 0.15         # 18 % of the hole terms are live


def check_layouts(tab, tt, V, T):
    no, nv, k = tt.no, tt.nv, tab.k_int
    Vv, Vo = tr.triples_integrals(tt, V)
    Tc, Td = tt.implied(T), tab.to_dense(T)
    i, a, b = np.meshgrid(np.arange(no), np.arange(nv), np.arange(nv), indexing="ij")
    # Vv: the implied virtual by brute force over the orbitals
    target = k[no + a] + k[no + b] - k[i]
    hit = np.all(target[..., None, :] == k[no:], axis=-1)                 # [o,v,v,f]
    assert hit.sum(axis=-1).max() <= 1
    valid, f = hit.any(axis=-1), hit.argmax(axis=-1)
    assert np.array_equal(Vv != 0, valid & (V[i, no + f, no + a, no + b] != 0))
    assert np.array_equal(Vv[valid], V[i, no + f, no + a, no + b][valid]) and not Vv[~valid].any()
    # Vo, m_of and Tc
    i, j, a = np.meshgrid(np.arange(no), np.arange(no), np.arange(nv), indexing="ij")
    target = k[i] + k[j] - k[no + a]
    hit = np.all(target[..., None, :] == k, axis=-1)                      # [o,o,v,p]
    found, p = hit.any(axis=-1), hit.argmax(axis=-1)
    occ, vir = found & (p < no), found & (p >= no)
    assert np.array_equal(tt.m_of, np.where(occ, p, -1)) and tt.m_of.dtype == np.int32
    assert np.array_equal(Vo[occ], V[i, j, no + a, p][occ]) and not Vo[~occ].any()
    assert np.array_equal(Tc[vir], Td[a, np.maximum(p - no, 0), i, j][vir]) and not Tc[~vir].any()
    assert np.array_equal(np.signbit(Vv[~valid]), np.zeros((~valid).sum(), dtype=bool))       # +0.0, not -0.0
    # the lists: momentum-conserving where valid, and ranges concatenate to the whole
    for family in tt.FAMILIES:
        pqrs, ok = tt.list_pqrs(family)
        assert pqrs.dtype == np.int32 and len(pqrs) == tt.sizes[family]
        assert tab.conserving(pqrs[ok]).all()
        edges = [0, 1, 7, len(pqrs) // 3, len(pqrs) - 1, len(pqrs)]
        parts = [tt.list_pqrs(family, e0, e1) for e0, e1 in zip(edges[:-1], edges[1:])]
        assert np.array_equal(np.concatenate([q for q, _ in parts]), pqrs)
        assert np.array_equal(np.concatenate([m for _, m in parts]), ok)
    # the lookup grid
    assert tt.orb_of.dtype == np.int32 and tuple(tt.box[3:]) == tt.orb_of.shape
    assert np.array_equal(tt.lookup(k), np.arange(tab.n))
    assert np.count_nonzero(tt.orb_of >= 0) == tab.n
    outside = np.array([tt.lo - 1, tt.lo + tt.dims, tt.lo + [0, 0, tt.dims[2]], tt.lo - [0, 1, 0]])
    assert (tt.lookup(outside) == -1).all()                               # never wrapped into the box


@pytest.mark.parametrize("nel,cutoff", [(14, 2), (14, 3), (54, 5)])
def test_layouts_hold_the_dense_elements_and_exact_zeros(nel, cutoff):
    no, tab, tt, V, eps, mp2 = problem(nel, cutoff)
    check_layouts(tab, tt, V, symmetric_amplitudes(tab, 5))


def twisted_problem():
    """The 13 orbitals of the twisted basis plus one planted on the edge of the lookup box: not inversion-symmetric."""
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    k = np.concatenate((g["k"], [[2, -1, 0]])).astype(np.int64)
    no = 7
    tab, tt = tr.tables_for(k, no)
    V = tr.conserving_V(k, 17)
    rng = np.random.default_rng(19)
    eps = np.concatenate((np.sort(rng.random(no)) - 2.0, np.sort(rng.random(len(k) - no)) + 1.0))
    return no, tab, tt, V, eps


def test_twisted_k_list_with_an_orbital_on_the_edge_of_the_box():
    no, tab, tt, V, eps = twisted_problem()
    k = tab.k_int
    assert not np.array_equal(np.unique(k, axis=0), np.unique(-k, axis=0))
    assert tt.lo.tolist() == [-1, -1, -1] and tt.dims.tolist() == [4, 3, 3]
    # K - k_a - k_b leaves the box for some (a,b) of some triple, on either side
    kv, K = k[no:], k[6] + k[5] + k[2]
    rel = K - kv[:, None, :] - kv[None, :, :] - tt.lo
    assert (rel < 0).any() and (rel >= tt.dims).any()
    # a flattened lookup without per-axis checks would name an orbital for some of them
    flat = (rel[..., 0] * tt.dims[1] + rel[..., 1]) * tt.dims[2] + rel[..., 2]
    out = ~np.all((rel >= 0) & (rel < tt.dims), axis=-1)
    wrapped = out & (flat >= 0) & (flat < tt.orb_of.size)
    assert (tt.orb_of.reshape(-1)[flat[wrapped]] >= 0).any()
    assert np.abs(V - V.transpose(1, 0, 3, 2)).max() == 0 and np.abs(V - V.transpose(2, 3, 0, 1)).max() == 0
    assert tab.conserving(np.argwhere(V != 0)).all() and np.abs(V - V.transpose(0, 1, 3, 2)).max() > 0
    T = symmetric_amplitudes(tab, 23)
    check_layouts(tab, tt, V, T)
    err, want, got = compare(no, tab, tt, V, eps, T)
    print(f"twisted: E(T) = {want.sum():.16e}, max|per triple| = {np.abs(want).max():.2e}, worst difference {err:.1e}")
    assert np.count_nonzero(want) > 10 and err <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("no,nv,live", [(4, 7, 20), (8, 8, 100), (3, 1, 0)])
def test_line_lattice_orbital_counts_no_electron_gas_has(no, nv, live):
    """tests/_sector_lattices.line_lattice: the lists the GPU edge tests run on (tests/test_gpu_sector_edges.py), here against
    the dense reference.  nv = 1: check_layouts cuts every list at the fixed positions [0, 1, 7, ...], which a list of three
    elements does not have, so only the values are compared there (all of them an exact +0.0)."""
    from tests._sector_lattices import line_lattice
    k, _ = line_lattice(no, nv)
    tab, tt = tr.tables_for(k, no)
    assert (tt.no, tt.nv) == (no, nv) and tt.dims.tolist() == [no + nv, 1, 1]
    V = tr.conserving_V(k, 17)
    rng = np.random.default_rng(19)
    eps = np.concatenate((np.sort(rng.random(no)) - 2.0, np.sort(rng.random(nv)) + 1.0))
    T = symmetric_amplitudes(tab, 23)
    if nv > 1:
        check_layouts(tab, tt, V, T)
    err, want, got = compare(no, tab, tt, V, eps, T)
    scale = tr.per_triple(tt, eps, *tr.triples_integrals(tt, V), tt.implied(T))[1]
    print(f"line lattice ({no},{nv}): max|per triple| = {np.abs(want).max():.2e}, worst difference {err:.1e}, "
          f"{int((scale > 0).sum())} of {len(want)} triples live")
    assert len(want) == R.n_triples(no) and int((scale > 0).sum()) == live
    assert err <= 1e-13 * np.abs(want).max()
    if live == 0:
        assert np.array_equal(got.view(np.int64), np.zeros(len(got), dtype=np.int64))


def test_tables_refuse_what_they_cannot_hold():
    with pytest.raises(TypeError, match="a SectorTables is needed"):
        tr.TriplesTables(np.zeros((3, 3)))
    no, tab, tt, V, eps, mp2 = problem(14, 2)
    with pytest.raises(ValueError, match="a compact vector of 204 elements"):
        tt.implied(np.zeros(203))
    with pytest.raises(KeyError):
        tt.list_pqrs("abcd")


def test_mp2_amplitudes_of_the_oracle_are_the_compact_ones():
    """The amplitudes above are the dense MP2 amplitudes of the oracle, read on the support."""
    no, tab, tt, V, eps, mp2 = problem(14, 3)
    _, T = oc.mp2(eps[:no], eps[no:], V[:no, :no, no:, no:], V[no:, no:, :no, :no])
    assert np.abs(tab.compact(T) - mp2).max() < 1e-15


def test_host_simulator_has_no_triples_kernel(hostsim_lib):
    """The C entry runs to the kernel layer on the host engine, which answers by name."""
    import ctypes as C

    from pymes_amd import _lib
    from pymes_amd.device import Context
    from pymes_amd.solver.ueg_cc import triple_bytes, upload_raw
    no, tab, tt, V, eps, mp2 = problem(14, 2)
    ctx = Context(no, tt.nv, lib=hostsim_lib)
    try:
        Vv, Vo = (ctx.array(x) for x in tr.triples_integrals(tt, V))
        Tc, eps_dev, ws = ctx.array(tt.implied(mp2)), ctx.array(eps), ctx.empty((triple_bytes(tt.nv) // 8,))
        i32 = lambda x: upload_raw(ctx, np.append(x.astype(np.int32).reshape(-1), np.zeros(x.size % 2, dtype=np.int32)))
        k_dev, orb_dev, m_dev = i32(tab.k_int), i32(tt.orb_of), i32(tt.m_of)
        e = C.c_double()
        with pytest.raises(_lib.PymesError, match="sector_triples: not available in this backend"):
            ctx.lib.call("pymes_sector_triples", ctx.handle, no, tt.nv, C.c_void_p(eps_dev.ptr), C.c_void_p(k_dev.ptr),
                         C.c_void_p(orb_dev.ptr), tt.box.ctypes.data_as(C.c_void_p), C.c_void_p(m_dev.ptr), C.c_void_p(Tc.ptr),
                         C.c_void_p(Vv.ptr), C.c_void_p(Vo.ptr), 0, 84, C.c_void_p(ws.ptr), triple_bytes(tt.nv), None, C.byref(e))
    finally:
        ctx.close()
