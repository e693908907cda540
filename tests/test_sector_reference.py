"""CPU: the momentum-sector tables (pymes_amd/solver/sectors.py) and the numpy restatement of the sector residual
(tests/_sector_reference.py) against oracle.cc_oracle on dense electron-gas integrals of oracle.ueg_oracle."""
import functools
import json
import os

import numpy as np
import pytest

from tests import _sector_reference as sr
from oracle import cc_oracle as oc
from oracle.ueg_oracle import Ueg
from pymes_amd.solver import sectors

GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = json.load(open(os.path.join(GOLD, "ueg.json")))
fast = functools.partial(np.einsum, optimize=True)


@functools.lru_cache(maxsize=None)
def problem(nel, cutoff, mode):
    """(model, tables, dense V, its sector blocks); mode "coulomb" or "tc" = only_2b + effect_2b with the recorded k_cutoff."""
    u = Ueg(nel, 1.0)
    u.init_basis(cutoff)
    if mode == "tc":
        u.k_cutoff = G[f"tc_N14_rs1.0_c{cutoff}"]["k_cutoff"]
        V = u.two_body("only_2b") + u.two_body("effect_2b")
    else:
        V = u.two_body("coulomb")
    V.setflags(write=False)
    tab = sr.tables_for(u.k_int, nel // 2)
    return u, tab, V, sr.sector_integrals(tab, V)


def symmetric_amplitudes(tab, seed):
    T = np.random.default_rng(seed).standard_normal(tab.nnz)
    return 0.5 * (T + T[tab.pp_swap])


CASES = [(2, 1, "coulomb"), (14, 2, "coulomb"), (14, 3, "coulomb"), (14, 5, "coulomb"), (54, 5, "coulomb"),
         (14, 2, "tc"), (14, 3, "tc"), (14, 5, "tc")]


@pytest.mark.parametrize("nel,cutoff,mode", CASES)
def test_residual_matches_the_dense_oracle(nel, cutoff, mode):
    u, tab, V, ints = problem(nel, cutoff, mode)
    no = nel // 2
    T = symmetric_amplitudes(tab, 7)
    eps = sr.hf_orbital_energies(tab, ints, u.kinetic)
    Td, B = tab.to_dense(T), oc.split_blocks(no, V)
    support = np.zeros(Td.shape, dtype=bool)
    support[tab.abij()] = True
    for is_dcd in (False, True):
        want = oc.doubles_residual(no, np.diag(eps), Td, B["klij"], B["ijab"], B["abij"], B["iajb"], B["iabj"], B["abcd"],
                                   is_dcd=is_dcd, ein=fast)
        got = sr.residual(tab, eps, T, ints, is_dcd=is_dcd)
        err = np.abs(tab.to_dense(got) - want).max()
        print(f"N={nel} cutoff={cutoff} {mode} dcd={is_dcd}: max|dR| = {err:.2e}, max|R| = {np.abs(want).max():.2e}")
        assert err <= 1e-13 * np.abs(want).max()
        assert np.count_nonzero(want[~support]) == 0        # exactly zero outside the support


def test_mp2_amplitudes_and_fock_live_on_the_support():
    u, tab, V, ints = problem(14, 3, "coulomb")
    no = 7
    f = np.diag(u.kinetic) + 2.0 * np.einsum("piqi->pq", V[:, :no, :, :no]) - np.einsum("piiq->pq", V[:, :no, :no, :])
    assert np.count_nonzero(f - np.diag(f.diagonal())) == 0
    eps = sr.hf_orbital_energies(tab, ints, u.kinetic)
    assert np.abs(eps - f.diagonal()).max() < 1e-13
    e, T = oc.mp2(eps[:no], eps[no:], V[:no, :no, no:, no:], V[no:, no:, :no, :no])
    vec = tab.compact(T)                                     # refuses weight outside the support
    assert np.abs(vec - ints["abij"] / tab.denominators(eps)).max() < 1e-15
    assert abs(sum(sr.energy(vec, ints)) - e) < 1e-13
    T[0, 0, 0, 1] = 1.0
    with pytest.raises(ValueError, match="weight outside the momentum-conserving support"):
        tab.compact(T)


@pytest.mark.parametrize("cutoff,n_pw,nnz,n_pp,n_ph", [(2, 19, 204, 25, 50), (3, 27, 380, 25, 74), (5, 57, 1238, 25, 122)])
def test_table_counts(cutoff, n_pw, nnz, n_pp, n_ph):
    u, tab, _, _ = problem(14, cutoff, "coulomb")
    assert (tab.n, tab.nnz, len(tab.P_keys), len(tab.q_keys)) == (n_pw, nnz, n_pp, n_ph)
    assert tab.nnz == tab.offsets("ph", "ph-")[-1] == len(tab.d_from_pp) == len(tab.c_from_pp)
    for perm in (tab.d_from_pp, tab.c_from_pp, tab.pp_to_d, tab.pp_to_c, tab.pp_to_dT, tab.pp_to_cT, tab.pp_swap, tab.d_partner):
        assert np.array_equal(np.sort(perm), np.arange(tab.nnz))
    assert np.array_equal(tab.pp_to_d[tab.d_from_pp], np.arange(tab.nnz))
    # the three layouts hold the same elements: a tagged dense array read through each of them
    T = np.arange(1.0, tab.nnz + 1)
    Td = tab.to_dense(T)
    sec, lr, lc = sectors._expand(tab.n_ph, tab.n_hp, 0, len(tab.q_keys))
    row, col = tab._pairs("ph", sec, lr), tab._pairs("ph-", sec, lc)
    assert np.array_equal(T[tab.d_from_pp], Td[row[:, 0], col[:, 0], row[:, 1], col[:, 1]])       # D^q[(a,i),(b,j)] = T_abij
    assert np.array_equal(T[tab.c_from_pp], Td[row[:, 0], col[:, 0], col[:, 1], row[:, 1]])       # C^q[(a,j),(b,i)] = T_abij
    assert np.count_nonzero(Td) == tab.nnz
    # every listed integral conserves the vector, and the lists are as long as the blocks
    for name in sectors.BLOCKS:
        pqrs = tab.block_pqrs(name)
        assert len(pqrs) == tab.block_offsets(name)[-1] and tab.conserving(pqrs).all()
        pieces = [tab.block_pqrs(name, s, s + 1) for s in range(tab.n_sectors(name))]
        assert np.array_equal(np.concatenate(pieces), pqrs)


def test_empty_sectors_are_kept():
    for nel, cutoff in ((14, 2), (54, 5)):
        tab = problem(nel, cutoff, "coulomb")[1]
        empty = np.flatnonzero(tab.n_vv == 0)
        assert len(empty) > 0 and (tab.n_oo[empty] > 0).all()
        assert (np.diff(tab.pp_off)[empty] == 0).all()


def test_twisted_basis():
    """k_shift = (0.1, 0.25, -0.05), cutoff 2 (tests/golden/ueg_twist.npz): the basis is not inversion-symmetric, some -q do
    not occur and their blocks are empty."""
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    no = int(g["nel"]) // 2
    tab = sr.tables_for(g["k"], no)
    assert (tab.neg < 0).any() and tab.nnz == tab.offsets("ph", "ph-")[-1] > 0
    assert np.array_equal(np.sort(tab.d_from_pp), np.arange(tab.nnz))
    V = g["coulomb"]
    idx = np.argwhere(V != 0)
    assert tab.conserving(idx).all()
    ints = sr.sector_integrals(tab, V)
    eps = sr.hf_orbital_energies(tab, ints, g["kinetic"])
    T = symmetric_amplitudes(tab, 3)
    B = oc.split_blocks(no, V)
    for is_dcd in (False, True):
        want = oc.doubles_residual(no, np.diag(eps), tab.to_dense(T), B["klij"], B["ijab"], B["abij"], B["iajb"], B["iabj"],
                                   B["abcd"], is_dcd=is_dcd, ein=fast)
        assert np.abs(tab.to_dense(sr.residual(tab, eps, T, ints, is_dcd=is_dcd)) - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("cutoff", [2, 3])
@pytest.mark.parametrize("is_dcd", [False, True])
def test_whole_solve_matches_the_oracle(cutoff, is_dcd):
    u, tab, V, ints = problem(14, cutoff, "coulomb")
    eps = sr.hf_orbital_energies(tab, ints, u.kinetic)
    ref = oc.ccd_solve(7, np.diag(eps), V, is_dcd=is_dcd, delta_e=1e-10, ein=fast)
    got = sr.solve(tab, eps, ints, is_dcd=is_dcd, delta_e=1e-10)
    want = np.array([h[0] for h in ref["history"]])
    assert len(got["history"]) == len(want) > 3
    assert np.abs(np.array(got["history"]) - want).max() < 1e-12
    assert np.abs(tab.to_dense(got["t2"]) - ref["t2"]).max() < 1e-11


def test_dense_builder_sets_non_conserving_elements_only_at_cutoff_4():
    """The reference's lookup range-checks only the flattened index (ueg.py:399-402): at N = 14, cutoff 4 the dense V holds 16
    elements that do not conserve momentum, none at cutoffs 2, 3 and 5.  The sector path does not reproduce them."""
    for cutoff, bad in ((2, 0), (3, 0), (4, 16), (5, 0)):
        u = Ueg(14, 1.0)
        u.init_basis(cutoff)
        V = problem(14, cutoff, "coulomb")[2] if cutoff != 4 else u.two_body("coulomb")
        tab = sr.tables_for(u.k_int, 7)
        assert np.count_nonzero(~tab.conserving(np.argwhere(V != 0))) == bad


def test_task_tables_chain_and_are_checked():
    tab = problem(14, 2, "coulomb")[1]
    t = tab.gemm_tasks(("vv", "vv", False), ("vv", "oo", False), ("vv", "oo", False), beta=1.0)
    assert len(t) == 25 and t.dtype.itemsize == 112 and (t["m"] == tab.n_vv).all() and (t["n"] == tab.n_oo).all()
    assert sectors.task_tiles(t) == t["tile0"][-1] + (-(-t["m"][-1] // sectors.TILE_M)) * (-(-t["n"][-1] // sectors.TILE_N))
    sectors.check_tasks(t, tab.offsets("vv", "vv")[-1], tab.nnz, tab.nnz)
    with pytest.raises(ValueError, match="past the end of operand A"):
        sectors.check_tasks(t, tab.offsets("vv", "vv")[-1] - 1, tab.nnz, tab.nnz)
    with pytest.raises(AssertionError, match="do not chain"):
        tab.gemm_tasks(("vv", "vv", False), ("oo", "oo", False), ("vv", "oo", False))


def test_entries_refuse_by_name_without_the_kernels(hostsim_lib):
    """The host simulator has no sector kernels: the engine's weak stand-ins refuse by name (there is no quiet fall-back), and
    the host-side checks of the C entries run before them."""
    import ctypes as C

    from pymes_amd._lib import PymesError
    from pymes_amd.device import Context
    from pymes_amd.solver.ueg_cc import SectorCCD, Tasks, gather, upload_raw
    ctx = Context(1, 1, lib=hostsim_lib)
    try:
        x = ctx.zeros((16,))
        table = Tasks(ctx, sectors.make_tasks([4], [4], [4], [0], [0], [0], [4], [4], [4]), 16, 16, 16)
        with pytest.raises(PymesError, match="sector_gemm: not available in this backend"):
            table.run(x, x, ctx.zeros((16,)))
        m = upload_raw(ctx, np.arange(16))
        m.count = 16
        with pytest.raises(PymesError, match="sector_gather: not available in this backend"):
            gather(ctx, ctx.zeros((16,)), x, m)
        with pytest.raises(PymesError, match="sector_update: not available in this backend"):
            SectorCCD._update(ctx, ctx.zeros((16,)), None, None, x, x, 0.0)
        with pytest.raises(PymesError, match="sector_xdiag: not available in this backend"):
            ctx.lib.call("pymes_sector_xdiag", ctx.handle, *[C.c_void_p(x.ptr)] * 5, 1.0, 1, 1, *[C.c_void_p(m.ptr)] * 4,
                         C.c_void_p(x.ptr))
        k = np.zeros((2, 3), dtype=np.int32)
        k[1, 0] = 1
        args = lambda imax, count: (ctx.handle, 2, 2, imax, 0, 1.0, 0.0, 1.0, 30, 0, None, k.ctypes.data_as(C.c_void_p), None,
                                    None, 0, C.c_void_p(m.ptr), count, C.c_void_p(x.ptr))
        with pytest.raises(PymesError, match="ueg_two_body_list: not available in this backend"):
            ctx.lib.call("pymes_ueg_eval_2b_list", *args(1, 4))
        with pytest.raises(PymesError, match="ueg: k outside the index map"):
            ctx.lib.call("pymes_ueg_eval_2b_list", *args(0, 4))
        with pytest.raises(PymesError, match="ueg: bad arguments"):
            ctx.lib.call("pymes_ueg_eval_2b_list", *args(1, -1))
    finally:
        ctx.close()
