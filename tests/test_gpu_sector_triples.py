"""GPU: the momentum-blocked (T) (pymes_amd/solver/ueg_cc.py, sector_triples_energy; csrc/kernels_sector.hip,
pymes_sector_triples): the kernels alone against the numpy restatement (tests/_sector_triples_reference.py), the
two integral families against the dense builder, whole solves against the dense CCD + (T) route, batching and determinism,
and the refusals."""
import contextlib
import ctypes as C
import io
import math
import os

import numpy as np
import pytest

from pymes_amd import _lib
from tests import _sector_triples_reference as tr
from tests import _triples_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from pymes_amd.device import Context
    c = Context(1, 1, lib=gpu_lib)
    yield c
    c.close()


def model(nel, cutoff, rs=1.0, k_shift=None, k_cutoff=None):
    from pymes_amd.model.ueg import UEG
    m = UEG(nel, nel // 2, nel // 2, rs)
    m.init_single_basis(cutoff, **({"k_shift": list(k_shift)} if k_shift is not None else {}))
    m.k_cutoff, m.gamma = k_cutoff, None
    return m


def twisted_model():
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    return model(int(g["nel"]), int(g["cutoff"]), float(g["rs"]), k_shift=g["k_shift"], k_cutoff=float(g["k_cutoff"]))


def twisted_k():
    """The 13 twisted orbitals and one planted on the edge of the lookup box (tests/test_sector_triples_reference.py)."""
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    return np.concatenate((g["k"], [[2, -1, 0]])).astype(np.int64), 7


# ---- the kernels alone ---------------------------------------------------------------------------------------------
def run_kernel(ctx, tt, eps, Tc, Vv, Vo, lo, hi, triples_in_ws=None):
    """pymes_sector_triples on uploaded operands: (sum, per-triple values)."""
    from pymes_amd.solver.ueg_cc import SectorTriplesIntegrals, triple_bytes
    holder = SectorTriplesIntegrals(ctx, tt)
    holder.Vv.set(Vv)
    holder.Vo.set(Vo)
    k_dev, orb_dev, m_dev, _ = holder.device_tables()
    ws_bytes = triple_bytes(tt.nv) * (triples_in_ws or max(hi - lo, 1))
    ws = ctx.array(np.full(ws_bytes // 8, np.nan))                # nothing relies on what the workspace held
    out, e = ctx.array(np.full(max(hi - lo, 1), np.nan)), C.c_double()
    eps_dev, tc_dev = ctx.array(eps), ctx.array(Tc)
    ctx.lib.call("pymes_sector_triples", ctx.handle, tt.no, tt.nv, C.c_void_p(eps_dev.ptr), C.c_void_p(k_dev.ptr),
                 C.c_void_p(orb_dev.ptr), tt.box.ctypes.data_as(C.c_void_p), C.c_void_p(m_dev.ptr), C.c_void_p(tc_dev.ptr),
                 C.c_void_p(holder.Vv.ptr), C.c_void_p(holder.Vo.ptr), lo, hi, C.c_void_p(ws.ptr), ws_bytes, C.c_void_p(out.ptr),
                 C.byref(e))
    return e.value, out.get()[:hi - lo]


def random_operands(tt, seed):
    """Seeded random Vv / Vo / Tc on their supports (exact zeros elsewhere) and orbital energies with a gap."""
    rng = np.random.default_rng(seed)
    Vv = np.zeros(tt.sizes["vv"])
    Vv[tt.list_pqrs("vv")[1]] = rng.standard_normal(int(tt.list_pqrs("vv")[1].sum()))
    Vo = np.where(tt.m_of >= 0, rng.standard_normal(tt.m_of.shape), 0.0)
    Tc = np.where(tt.b_of >= 0, rng.standard_normal(tt.b_of.shape) * 0.1, 0.0)
    eps = np.concatenate((np.sort(rng.random(tt.no)) - 2.0, np.sort(rng.random(tt.nv)) + 1.0))
    return eps, Tc, Vv.reshape(tt.no, tt.nv, tt.nv), Vo


def support(case):
    if case == "twist":
        return tr.tables_for(*twisted_k())
    m = model(*case)
    return tr.tables_for(m.sector_tables().k_int, case[0] // 2)


@pytest.mark.parametrize("case", [(14, 2), (14, 5), (54, 5), (14, 8), "twist"], ids=str)
def test_kernel_matches_the_numpy_restatement(ctx, case):
    """(14,8): v = 86, past two 32-wide tiles with a ragged third; (54,5): o = 27, 18 % of the hole terms live;
    (14,2): 62 triples without any virtual triple; twist: vectors that leave the lookup box."""
    tab, tt = support(case)
    eps, Tc, Vv, Vo = random_operands(tt, 31)
    n = R.n_triples(tt.no)
    want, scale = tr.per_triple(tt, eps, Vv, Vo, Tc)
    e, got = run_kernel(ctx, tt, eps, Tc, Vv, Vo, 0, n)
    live = scale > 0
    ratio = (np.abs(got - want)[live] / scale[live]).max() if live.any() else 0.0
    print(f"{case}: v = {tt.nv}, {n} triples, {int((~live).sum())} vanish, worst |d| / sum|terms| = {ratio:.2e}")
    assert (np.abs(got - want) <= 1e-12 * scale).all()
    assert np.array_equal(got[~live], np.zeros((~live).sum())) and not np.signbit(got[~live]).any()
    assert e == tr.ordered_sum(got)                             # the values in triple order, every add's error carried along
    assert abs(e - math.fsum(got)) <= 2.0 ** -52 * abs(e)
    if case == (14, 2):
        assert (~live).sum() == 62
    if case == (14, 8):
        assert tt.nv == 86


# ---- the integral families against the dense builder ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["coulomb", "only_2b", "effect_2b", "twist"])
def test_integrals_match_the_dense_builder_to_the_bit(ctx, case):
    m = twisted_model() if case == "twist" else model(14, 2, k_cutoff=1.0)
    runs = {"coulomb": [(None, {})], "only_2b": [(m.trunc, dict(is_only_2b=True))],
            "effect_2b": [(m.trunc, dict(is_effect_2b=True))],
            "twist": [(None, {}), (m.trunc, dict(is_only_2b=True)), (m.trunc, dict(is_effect_2b=True))]}[case]
    tab = m.sector_tables()
    assert tab.n == (13 if case == "twist" else 19)
    for correlator, flags in runs:
        tints = quiet(m.eval_2b_triples, tab, correlator=correlator, ctx=ctx, **flags)
        V = quiet(m.eval_2b_integrals, correlator=correlator, sp=0, on_device=True, ctx=ctx, **flags).get()
        tt = tints.tables
        for got, want, family in zip((tints.Vv.get(), tints.Vo.get()), tr.triples_integrals(tt, V), tt.FAMILIES):
            valid = tt.list_pqrs(family)[1].reshape(got.shape)
            assert np.array_equal(got[valid].view(np.int64), want[valid].view(np.int64)), (case, family)
            assert np.array_equal(got[~valid].view(np.int64), np.zeros((~valid).sum(), dtype=np.int64))      # exact +0.0
            assert np.count_nonzero(got) > 0 and (~valid).any()


def test_integrals_are_placed_chunk_by_chunk(ctx, monkeypatch):
    """A chunk of 1000 list positions: Vv (7 * 12 * 12 = 1008) ends in a chunk of 8."""
    from pymes_amd.model.ueg import UEG
    m = model(14, 2)
    tab = m.sector_tables()
    whole = quiet(m.eval_2b_triples, tab, ctx=ctx)
    monkeypatch.setattr(UEG, "SECTOR_CHUNK", 1000)
    pieces = quiet(m.eval_2b_triples, tab, ctx=ctx)
    for a, b in ((whole.Vv, pieces.Vv), (whole.Vo, pieces.Vo)):
        assert np.array_equal(a.get().view(np.int64), b.get().view(np.int64))


# ---- whole solves against the dense route --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def coulomb(ctx):
    cache = {}

    def get(nel, cutoff):
        if (nel, cutoff) not in cache:
            m = model(nel, cutoff)
            tab = m.sector_tables()
            ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
            kin = np.array([b.kinetic for b in m.basis_fns[::2]])
            cache[nel, cutoff] = (m, tab, ints, ints.hf_orbital_energies(kin), quiet(m.eval_2b_triples, tab, ctx=ctx))
        return cache[nel, cutoff]
    return get


@pytest.fixture(scope="module")
def dense_V():
    last = {}

    def get(m, key):
        if key not in last:
            last.clear()                        # one dense array at a time: 0.6 GB at 93 plane waves
            last[key] = quiet(m.eval_2b_integrals)
        return last[key]
    return get


@pytest.mark.parametrize("is_dcd", [False, True], ids=["ccd", "dcd"])
@pytest.mark.parametrize("nel,cutoff", [(14, 2), (14, 5), (54, 5), (14, 8)])
def test_solve_with_triples_matches_the_dense_route(ctx, coulomb, dense_V, nel, cutoff, is_dcd):
    """SectorCCD.solve(triples=) against CCD.solve + get_triples_energy, |d E(T)| <= 1e-11 max |per-triple value|.

    Both loops are converged as far as doubles go (delta_e = 1e-14, 38 to 52 passes): the bound is 61 units in the last place
    of E(T) at (54,5), where E(T) is a thousand times its largest term, and two loops stopped at 1e-10 still differ by
    1e-15 in their amplitudes (the DIIS steps amplify the last bits of the residuals), which alone moves E(T) by 2.4e-16
    there.  Converged, the amplitudes agree to 7e-18 and the exactly rounded sums of the two per-triple arrays to 2e-18.
    Measured on an MI355X (2026-10-20), |d E(T)| of the bound: (14,2) 0 / 2.2e-19 (CCD / DCD) of 1.1e-15; (14,5) 0 / 1.4e-17 of
    5.2e-15; (14,8) 3.5e-18 / 0 of 6.0e-15; (54,5) 9.7e-17 / 1.7e-17 of 1.06e-16 / 1.09e-16.  The per-triple values agree to
    7e-21 at (54,5); the 9.7e-17 are the dense route's own sum of 3 654 values, 9.5e-17 off the exactly rounded sum of its
    per-triple array (the sector sum carries the error of every add along and equals the exactly rounded sum)."""
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ccsd_t import get_triples_energy
    from pymes_amd.solver.ueg_cc import SectorCCD, sector_triples_energy
    m, tab, ints, eps, tints = coulomb(nel, cutoff)
    no = nel // 2
    V = dense_V(m, (nel, cutoff))
    got = quiet(SectorCCD(no, delta_e=1e-14, is_dcd=is_dcd).solve, eps, ints, triples=tints, max_iter=100)
    dense = quiet(CCD(no, delta_e=1e-14, is_dcd=is_dcd).solve, np.diag(eps), V, max_iter=100)
    e_t, pt = get_triples_energy(no, np.diag(eps), V, None, dense["t2 amp"], per_triple=True)
    e_s, ps = sector_triples_energy(eps, ints, tints, got["t2 amp"], per_triple=True)
    e_k, pk = sector_triples_energy(eps, ints, tints, dense["t2 amp"], per_triple=True)      # the kernels alone: same amplitudes
    scale = np.abs(pt).max()
    print(f"N={nel} cutoff={cutoff} dcd={is_dcd}: E(T) sector {got['(t) e']:.15e} dense {e_t:.15e}, |d| = "
          f"{abs(got['(t) e'] - e_t):.2e}, worst per triple {np.abs(ps - pt).max():.2e}, max|per triple| = {scale:.2e}; "
          f"on the dense amplitudes |d| = {abs(e_k - e_t):.2e}, per triple {np.abs(pk - pt).max():.2e}; "
          f"against the exactly rounded sums of the per-triple values: sector {e_s - math.fsum(ps):.2e}, dense "
          f"{e_t - math.fsum(pt):.2e}, between the two exact sums {math.fsum(ps) - math.fsum(pt):.2e}")
    assert np.abs(ps - pt).max() <= 1e-11 * scale
    assert np.abs(pk - pt).max() <= 1e-11 * scale and abs(e_k - e_t) <= 1e-11 * scale
    assert e_s == got["(t) e"] and got["ccd(t) e"] == got["ccd e"] + got["(t) e"]
    assert sorted(got) == sorted(list(dense) + ["(t) e", "ccd(t) e"])
    assert sorted(quiet(SectorCCD(no, is_dcd=is_dcd).solve, eps, ints, max_iter=1)) == sorted(dense)      # unchanged without
    assert abs(got["(t) e"] - e_t) <= 1e-11 * scale


# ---- determinism and batching --------------------------------------------------------------------------------------
def test_values_do_not_depend_on_batches_ranges_or_repetition(ctx, coulomb):
    from pymes_amd.solver.ueg_cc import sector_triples_energy, triple_bytes
    m, tab, ints, eps, tints = coulomb(54, 5)
    T = np.random.default_rng(41).standard_normal(tab.nnz) * 0.05
    T = 0.5 * (T + T[tab.pp_swap])
    n, each = R.n_triples(27), triple_bytes(tab.nv)
    bits = lambda x: x.view(np.int64)
    e0, p0 = sector_triples_energy(eps, ints, tints, T, per_triple=True)
    e1, p1 = sector_triples_energy(eps, ints, tints, T, per_triple=True)
    assert e0 == e1 and np.array_equal(bits(p0), bits(p1)) and len(p0) == n
    for k in (1, 5, n):                        # 5: a batch boundary inside a run of equal i; 0 bytes: still one triple
        ek, pk = sector_triples_energy(eps, ints, tints, T, per_triple=True, workspace_bytes=k * each if k > 1 else 0)
        assert ek == e0 and np.array_equal(bits(pk), bits(p0)), k
    edges = [0, 1, 17, 1000, n - 1, n]
    parts = [sector_triples_energy(eps, ints, tints, T, triple_range=r, per_triple=True, workspace_bytes=7 * each)
             for r in zip(edges[:-1], edges[1:])]
    assert np.array_equal(bits(np.concatenate([p for _, p in parts])), bits(p0))
    # (two sequential sums of n terms in different groupings: each within (n - 1) 2^-53 sum |terms| of the exact sum)
    assert abs(sum(e for e, _ in parts) - e0) <= 2 * n * 2.0 ** -53 * np.abs(p0).sum()
    assert sector_triples_energy(eps, ints, tints, T, triple_range=(5, 5)) == 0.0


def test_workspace_default_comes_from_the_environment(ctx, coulomb, monkeypatch):
    from pymes_amd.solver import ueg_cc
    m, tab, ints, eps, tints = coulomb(14, 2)
    T = np.zeros(tab.nnz)
    assert (ueg_cc.TRIPLES_WS_ENV, ueg_cc.TRIPLES_WS_DEFAULT) == ("PYMES_SECTOR_TRIPLES_BYTES", 1 << 30)
    monkeypatch.setenv(ueg_cc.TRIPLES_WS_ENV, "not a number")
    with pytest.raises(ValueError):
        ueg_cc.sector_triples_energy(eps, ints, tints, T)
    monkeypatch.setenv(ueg_cc.TRIPLES_WS_ENV, str(3 * ueg_cc.triple_bytes(tab.nv)))
    assert ueg_cc.sector_triples_energy(eps, ints, tints, T) == 0.0


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals(ctx, coulomb):
    from pymes_amd.solver.ueg_cc import SectorCCD, sector_triples_energy, triple_bytes
    m, tab, ints, eps, tints = coulomb(14, 2)
    T = np.zeros(tab.nnz)
    # transcorrelated integrals: before anything iterates
    mt = model(14, 2, k_cutoff=1.0)
    v2 = quiet(mt.eval_2b_sectors, tab, correlator=mt.trunc, is_only_2b=True, ctx=ctx)
    tc = v2 + quiet(mt.eval_2b_sectors, tab, correlator=mt.trunc, is_effect_2b=True, ctx=ctx)
    for call in (lambda: sector_triples_energy(eps, tc, tints, T),
                 lambda: quiet(SectorCCD(7).solve, eps, tc, triples=tints, max_iter=0)):
        with pytest.raises(ValueError, match=r"not defined for transcorrelated integrals, and Lambda-\(T\) does not exist on "
                                             "sectors yet"):
            call()
    other = quiet(model(14, 3).eval_2b_triples, model(14, 3).sector_tables(), ctx=ctx)
    with pytest.raises(ValueError, match="the triples integrals belong to other tables or another context"):
        sector_triples_energy(eps, ints, other, T)
    with pytest.raises(ValueError, match="the tables do not belong to this basis"):
        m.eval_2b_triples(model(14, 3).sector_tables(), ctx=ctx)
    with pytest.raises(TypeError, match="must be SectorTriplesIntegrals"):
        sector_triples_energy(eps, ints, ints, T)
    with pytest.raises(ValueError, match="the Fock matrix must be diagonal"):
        sector_triples_energy(np.diag(eps) + 1e-3, ints, tints, T)
    with pytest.raises(ValueError, match="not exchange-symmetric"):
        sector_triples_energy(eps, ints, tints, np.random.default_rng(0).standard_normal(tab.nnz))
    with pytest.raises(ValueError, match=r"triple range \[3, 85\) outside \[0, 84\]"):
        sector_triples_energy(eps, ints, tints, T, triple_range=(3, 85))
    k_dev, orb_dev, m_dev, _ = tints.device_tables()
    ws, e, eps_dev = ctx.empty((triple_bytes(tab.nv) // 8,)), C.c_double(), ctx.array(eps)

    def raw(ws_bytes, lo=0, hi=84):
        ctx.lib.call("pymes_sector_triples", ctx.handle, 7, 12, C.c_void_p(eps_dev.ptr), C.c_void_p(k_dev.ptr),
                     C.c_void_p(orb_dev.ptr), tints.tables.box.ctypes.data_as(C.c_void_p), C.c_void_p(m_dev.ptr),
                     C.c_void_p(tints.Vo.ptr), C.c_void_p(tints.Vv.ptr), C.c_void_p(tints.Vo.ptr), lo, hi, C.c_void_p(ws.ptr),
                     ws_bytes, None, C.byref(e))
    with pytest.raises(_lib.PymesError, match="sector_triples: the workspace does not hold one triple"):
        raw(triple_bytes(tab.nv) - 8)
    with pytest.raises(_lib.PymesError, match=r"sector_triples: triple range \[0, 85\) outside"):
        raw(triple_bytes(tab.nv), 0, 85)
    ctx.graph_begin()
    try:
        with pytest.raises(RuntimeError, match="sector_triples_energy: the context is recording a launch graph"):
            sector_triples_energy(eps, ints, tints, T)
        with pytest.raises(RuntimeError, match="eval_2b_triples: the context is recording a launch graph"):
            m.eval_2b_triples(tab, ctx=ctx)
        with pytest.raises(_lib.PymesError, match="sector_triples while a launch graph is being recorded"):
            raw(triple_bytes(tab.nv))
    finally:
        ctx.graph_abort()
    assert sector_triples_energy(eps, ints, tints, T) == 0.0           # the context is usable afterwards
