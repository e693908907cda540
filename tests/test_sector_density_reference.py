"""CPU: the numpy restatement of the sector densities (tests/_sector_density_reference.py) against the definition
(L(eps, V) is linear, so every element of gamma and G is one evaluation of L), against the dense densities of
tests/_lambda_reference.py, tests/_rdm2_reference.py and ``lambda_ccsd.full_rdm2``, the identities of the transfer sums on every
basis, ``sectors.TransferBins``, and the refusals of the host simulator, which has no sector kernels."""
import os
import re

import numpy as np
import pytest

from pymes_amd.solver import lambda_ccsd, sectors
from pymes_amd.solver.sectors import BLOCKS
from tests import _lambda_reference as lref
from tests import _rdm2_reference as r2
from tests import _sector_density_reference as sd
from tests import _sector_reference as sr
from tests.test_sector_lambda_reference import exchange_only, small_problem, twist_problem
from tests.test_sector_reference import CASES, problem, symmetric_amplitudes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("pymes_sector_bin_sums", "pymes_sector_pair_transfer", "pymes_sector_gamma")


def seeded(tab, seed=3):
    return 0.1 * symmetric_amplitudes(tab, seed), symmetric_amplitudes(tab, seed + 1)


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("is_dcd", [False, True])
def test_every_element_is_the_derivative_of_the_lagrangian(hermitian, is_dcd):
    """G[element] = L(0, e_element) for every element of every family and gamma_p = L(e_p, 0), within 1e-13 x the sum of
    |terms| of that evaluation of L.  (The integrals of the problem do not enter: L is linear in them.)"""
    no, tab, tt, V, eps, ints = small_problem(5, hermitian)
    T, lam = seeded(tab)
    gamma, G = sd.density(tab, T, lam, is_dcd)
    unit, worst, count = sd.zero_integrals(tab), 0.0, 0
    for name in BLOCKS:
        assert len(G[name]) == len(unit[name])
        for e in range(len(unit[name])):
            unit[name][e] = 1.0
            want, scale = sd.lagrangian(tab, np.zeros(tab.n), unit, T, lam, is_dcd)
            unit[name][e] = 0.0
            assert abs(G[name][e] - want) <= 1e-13 * max(scale, 1e-300) + 1e-300, (name, e, G[name][e], want)
            worst, count = max(worst, abs(G[name][e] - want)), count + 1
        if not (is_dcd and name in ("klcd", "wx")):
            assert np.abs(G[name]).max() > 0, name
    for p in range(tab.n):
        e = np.zeros(tab.n)
        e[p] = 1.0
        want, scale = sd.lagrangian(tab, e, unit, T, lam, is_dcd)
        assert abs(gamma[p] - want) <= 1e-13 * max(scale, 1e-300) + 1e-300
    print(f"hermitian={hermitian} dcd={is_dcd}: {count} elements, largest |G - L(0, e)| = {worst:.2e}, tr gamma = {gamma.sum():.1e}")
    if is_dcd:
        assert not G["klcd"].any() and not G["wx"].any()
    # and for the integrals of the problem themselves
    want, scale = sd.lagrangian(tab, eps, ints, T, lam, is_dcd)
    assert abs(sd.expectation(tab, gamma, G, eps, ints) - want) <= 1e-13 * scale


@pytest.mark.parametrize("hermitian", [True, False])
def test_ccd_densities_match_the_dense_ones(hermitian):
    """gamma against ``lagrangian_density``, L(0, W) against ``_rdm2_reference.lagrangian`` for a seeded exchange-only W, and
    S(q) bin by bin against the binned ``full_rdm2`` of the dense blocks."""
    no, tab, tt, V, eps, ints = small_problem(5, hermitian)
    T, lam = seeded(tab)
    nv, n = tab.nv, tab.n
    Td, Ld, z1 = tab.to_dense(T), tab.to_dense(lam), np.zeros((nv, no))
    gamma, G = sd.density(tab, T, lam)
    dense = lref.lagrangian_density(no, z1, Td, z1, Ld)
    assert np.count_nonzero(dense - np.diag(dense.diagonal())) == 0
    assert np.abs(gamma - dense.diagonal()).max() <= 1e-13 * np.abs(dense).max()
    W = exchange_only(V, 77)
    want = r2.lagrangian(no, np.zeros((n, n)), W, z1, Td, z1, Ld)
    got = sd.expectation(tab, gamma, G, np.zeros(n), sr.sector_integrals(tab, W))
    print(f"hermitian={hermitian}: L(0, W) sector {got:.15e}, dense {want:.15e}")
    assert abs(got - want) <= 1e-12 * abs(want)
    # the structure factor: sum of the spin-summed two-particle density over the elements with k_r - k_p = q
    blocks = r2.rdm2_terms(no, z1, Td, z1, Ld)
    Dfull = lambda_ccsd.full_rdm2(no, np.diag(gamma), blocks)
    q, neg, zero = sd.transfer_bins(tab)
    index = {tuple(v): b for b, v in enumerate(q)}
    k = tab.k_int
    binned = np.zeros(len(q))
    for p, qq, r, s in np.argwhere(Dfull != 0.0):
        assert tuple(k[p] + k[qq]) == tuple(k[r] + k[s])
        binned[index[tuple(k[r] - k[p])]] += Dfull[p, qq, r, s]
    N = 2 * no
    S = sd.structure_factor(tab, gamma, sd.transfer_sums(tab, G, q), q, neg, zero)
    print("S(q) sector against 1 + binned full_rdm2 / N: largest difference %.2e, S in [%.4f, %.4f]"
          % (np.abs(S - 1.0 - binned / N).max(), S.min(), S.max()))
    assert np.abs(S - (1.0 + binned / N)).max() <= 1e-12 * np.abs(S).max()
    assert abs(S[zero] - N) <= 1e-12 * N


def identities(tab, label, uneven=False):
    for is_dcd in (False, True):
        T, lam = seeded(tab, 11)
        gamma, G = sd.density(tab, T, lam, is_dcd)
        q, neg, zero = sd.transfer_bins(tab)
        s = sd.transfer_sums(tab, G, q)
        scale = sum(np.abs(G[name]).sum() for name in BLOCKS)
        assert abs(gamma.sum()) <= 1e-13 * np.abs(gamma).sum()
        assert abs(s[zero] - gamma[:tab.no].sum()) <= 1e-13 * scale
        # integrals that depend on the transfer alone, v(q) = v(-q): sum_q v(q) s(q) = L(0, V_v)
        rng = np.random.default_rng(29)
        v = rng.standard_normal(len(q))
        v = 0.5 * (v + v[neg])
        index = {tuple(x): b for b, x in enumerate(q)}
        W = sd.zero_integrals(tab)
        for name in BLOCKS:
            pqrs = tab.block_pqrs(name)
            W[name] = v[[index[tuple(x)] for x in tab.k_int[pqrs[:, 2]] - tab.k_int[pqrs[:, 0]]]] if len(pqrs) else W[name]
        want, lscale = sd.lagrangian(tab, np.zeros(tab.n), W, T, lam, is_dcd)
        assert abs(v @ s - want) <= 1e-13 * max(lscale, np.abs(v) @ np.abs(s))
        s2 = 0.5 * (s + s[neg])
        assert np.array_equal(s2, s2[neg])
        odd = np.abs(s - s[neg]).max()
        print(f"{label} dcd={is_dcd}: s(0) = {s[zero]:.6e}, largest |s(q) - s(-q)| = {odd:.2e}, bins {len(q)}")
        if uneven:
            assert odd > 1e-3 * np.abs(s).max()


@pytest.mark.parametrize("nel,cutoff", sorted({case[:2] for case in CASES}))
def test_identities_of_the_transfer_sums(nel, cutoff):
    """tr gamma = 0, s(0) = sum_i gamma_i, sum_q v(q) s(q) = L(0, V_v), S2 even, on every basis of CASES (the identities do
    not read the integrals, so the Coulomb and the transcorrelated case of a basis are one case here)."""
    identities(problem(nel, cutoff, "coulomb")[1], f"N={nel} c={cutoff}")


def test_identities_on_the_twisted_basis():
    identities(twist_problem()[0], "twist")


def test_the_plain_transfer_sums_are_not_even():
    """On the eleven-orbital problem s(q) != s(-q): the product list treats the two electrons differently, and the published
    S2(q) = (s(q) + s(-q)) / 2 must keep its symmetrisation."""
    identities(small_problem(5, True)[1], "small", uneven=True)


def bins_check(tab):
    tb = sectors.TransferBins(tab)
    q, neg, zero = sd.transfer_bins(tab)
    assert np.array_equal(tb.q, q) and np.array_equal(tb.neg, neg) and tb.zero == zero
    assert np.array_equal(tb.q[tb.neg], -tb.q) and tb.nbins == len(q)
    assert "abcd" not in tb.csr and sorted(tb.csr) == sorted(nm for nm in BLOCKS if nm != "abcd")
    k = tab.k_int
    for name, (off, order) in tb.csr.items():
        pqrs = tab.block_pqrs(name)
        assert off.dtype == order.dtype == np.int64 and len(off) == tb.nbins + 1 and off[0] == 0 and off[-1] == len(pqrs)
        assert np.array_equal(np.sort(order), np.arange(len(pqrs)))                 # every element in exactly one list
        which = np.repeat(np.arange(tb.nbins), np.diff(off))
        assert np.array_equal(k[pqrs[order, 2]] - k[pqrs[order, 0]], tb.q[which])
    assert tb.oo_count.sum() == tab.no ** 2 and tb.oo_count[tb.zero] == tab.no
    assert len(tb.ip_orb) == tab.no * tab.n
    gamma = np.random.default_rng(2).standard_normal(tab.n)
    want = np.zeros(tb.nbins)
    for i in range(tab.no):
        for p in range(tab.n):
            want[tb.bin_of(k[i] - k[p])] -= gamma[p]
            want[tb.bin_of(k[p] - k[i])] -= gamma[p]
        for j in range(tab.no):
            want[tb.bin_of(k[j] - k[i])] -= 2.0
    assert np.abs(tb.reference_terms(gamma) - want).max() <= 1e-12 * np.abs(want).max()
    values, shell = tb.shells()
    assert values[0] == 0 and (np.diff(values) > 0).all() and np.array_equal(values[shell], (tb.q ** 2).sum(axis=1))
    assert tb.bin_of(np.array([99, 0, 0])) == -1
    vv, start, length, of_pair = tb.pair_rows()
    assert len(vv) == len(start) == len(length) == tab.n_vv.sum() and length.sum() == tab.nnz
    a, b, i, j = tab.abij()
    first = np.concatenate(([0], np.cumsum(length)))[:-1]
    assert np.array_equal(start, first) and (length > 0).all()
    assert np.array_equal(vv[:, 0], a[first]) and np.array_equal(vv[:, 1], b[first])
    assert np.array_equal(of_pair[vv[:, 0].astype(np.int64) * tab.nv + vv[:, 1]], np.arange(len(vv)))
    assert (of_pair >= 0).sum() == len(vv)


def test_transfer_bins():
    bins_check(problem(14, 2, "coulomb")[1])
    bins_check(small_problem(5, True)[1])
    tab = twist_problem()[0]
    assert (tab.neg < 0).any()
    bins_check(tab)
    with pytest.raises(TypeError, match="a SectorTables is needed"):
        sectors.TransferBins(None)


def test_header_and_signatures_name_the_new_entries():
    from pymes_amd import _lib
    text = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    declared = set(re.findall(r"\b(pymes_[a-zA-Z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES


def test_the_host_simulator_refuses_the_new_entries_by_name(hostsim_lib):
    import ctypes as C

    from pymes_amd._lib import PymesError
    from pymes_amd.device import Context
    ctx = Context(1, 1, lib=hostsim_lib)
    try:
        x = ctx.zeros((64,))
        box = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
        p = C.c_void_p(x.ptr)
        with pytest.raises(PymesError, match="sector_bin_sums: not available in this backend"):
            ctx.lib.call("pymes_sector_bin_sums", ctx.handle, p, 1, p, p, p, 1.0, 0.0)
        with pytest.raises(PymesError, match="sector_pair_transfer: not available in this backend"):
            ctx.lib.call("pymes_sector_pair_transfer", ctx.handle, p, 1, p, p, p, box.ctypes.data_as(C.c_void_p), 1, 1, 1, p, p, p,
                         p, p, p, 0)
        with pytest.raises(PymesError, match="sector_gamma: not available in this backend"):
            ctx.lib.call("pymes_sector_gamma", ctx.handle, p, p, 1, 1, p, p, p, p, p)
    finally:
        ctx.close()
