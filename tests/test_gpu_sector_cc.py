"""GPU: the momentum-sector CCD / DCD path (pymes_amd/solver/ueg_cc.py, sectors.py; csrc/kernels_sector.hip and the list
form of the electron-gas integrals in csrc/kernels_integrals.hip): the ragged batched product alone against numpy, the
integral list against the dense builder, the sector residual against the dense residual, whole solves against the recorded
energies and the dense ``CCD`` class, and the refusals."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.solver import sectors
from tests import _sector_reference as sr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = json.load(open(os.path.join(GOLD, "ueg.json")))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from pymes_amd.device import Context
    c = Context(1, 1, lib=gpu_lib)
    yield c
    c.close()


# ---- pymes_sector_gemm alone ---------------------------------------------------------------------------------------
def ragged_case(seed, nblocks, hi=130, small_n=False, forced=None):
    """Seeded task table over NaN-padded arenas (operand blocks separated by NaN gaps, leading dimensions above the row
    lengths) and what numpy makes of it.  ``forced``: the (m, n, k) tuples of sizes the first blocks take."""
    rng = np.random.default_rng(seed)
    m, n, k = (rng.integers(1, hi + 1, nblocks) for _ in range(3))
    if small_n:
        n = rng.integers(1, 8, nblocks)
    if forced is None:
        forced = ((0, 1, 64, 65, 128, 129, 130), (1, 0, 16, 17, 1, 33, 130), (7, 5, 0, 1, 33, 130, 31))
    for arr, forced in zip((m, n, k), forced):
        arr[:min(nblocks, len(forced))] = forced[:nblocks]      # 0-sized blocks, n = 1, k no multiple of 4, tile edges
    ta, tb = rng.integers(0, 2, nblocks).astype(bool), rng.integers(0, 2, nblocks).astype(bool)
    beta = rng.integers(0, 2, nblocks).astype(float)
    alpha = rng.choice([1.0, -1.0, 0.5], nblocks)
    pad = lambda: rng.integers(0, 4, nblocks)
    ar, ac = np.where(ta, k, m), np.where(ta, m, k)
    br, bc = np.where(tb, n, k), np.where(tb, k, n)
    lda, ldb, ldc = ac + pad(), bc + pad(), n + pad()

    def place(rows, ld):
        size = rows * ld + rng.integers(1, 6, nblocks)          # at least one NaN between two blocks
        off = np.concatenate(([3], 3 + np.cumsum(size)))
        return off[:-1], int(off[-1])
    (a, len_a), (b, len_b), (c, len_c) = place(ar, lda), place(br, ldb), place(m, ldc)
    A, B, Cm = (np.full(n_, np.nan) for n_ in (len_a, len_b, len_c))
    want, written = None, np.zeros(len_c, dtype=bool)
    for t in range(nblocks):
        for arena, off, rows, cols, ld in ((A, a, ar, ac, lda), (B, b, br, bc, ldb)):
            blk = rng.standard_normal((rows[t], cols[t]))
            idx = off[t] + np.arange(rows[t])[:, None] * ld[t] + np.arange(cols[t])[None, :]
            arena[idx] = blk
        idx = c[t] + np.arange(m[t])[:, None] * ldc[t] + np.arange(n[t])[None, :]
        if beta[t]:
            Cm[idx] = rng.standard_normal((m[t], n[t]))
        written[idx] = True
    want = Cm.copy()
    bound = np.zeros(len_c)
    for t in range(nblocks):
        blk = lambda arena, off, rows, cols, ld: arena[off[t] + np.arange(rows[t])[:, None] * ld[t] + np.arange(cols[t])[None, :]]
        Ab, Bb = blk(A, a, ar, ac, lda), blk(B, b, br, bc, ldb)
        Ab, Bb = (Ab.T if ta[t] else Ab), (Bb.T if tb[t] else Bb)
        idx = c[t] + np.arange(m[t])[:, None] * ldc[t] + np.arange(n[t])[None, :]
        prod = alpha[t] * (Ab @ Bb)
        want[idx] = prod + (beta[t] * Cm[idx] if beta[t] else 0.0)
        if Ab.size and Bb.size:
            bound[idx] = 1e-13 * k[t] * np.abs(Ab).max() * np.abs(Bb).max()
    tasks = sectors.make_tasks(m, n, k, a, b, c, lda, ldb, ldc, alpha, beta, trans_a=ta, trans_b=tb)
    return tasks, A, B, Cm, want, written, bound


@pytest.mark.parametrize("seed,nblocks,small_n", [(0, 1, False), (1, 7, False), (2, 60, False), (3, 300, False), (4, 300, True)])
def test_sector_gemm_against_numpy(ctx, seed, nblocks, small_n):
    from pymes_amd.solver.ueg_cc import Tasks
    tasks, A, B, Cm, want, written, bound = ragged_case(seed, nblocks, small_n=small_n)
    table = Tasks(ctx, tasks, len(A), len(B), len(Cm))
    dA, dB = ctx.array(A), ctx.array(B)
    outs = []
    for _ in range(2):
        dC = ctx.array(Cm)
        table.run(dA, dB, dC)
        outs.append(dC.get())
    got = outs[0]
    assert np.array_equal(np.isnan(got), ~written)                   # nothing outside the declared output blocks is touched,
    untouched = ~written
    assert np.array_equal(got[untouched].view(np.int64), Cm[untouched].view(np.int64))       # ... bit for bit
    err = np.abs(got[written] - want[written])
    print(f"{nblocks} blocks: max error {err.max() if err.size else 0.0:.2e}, {table.tiles} tiles")
    assert (err <= bound[written]).all()
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))       # identical calls give identical bits


def test_sector_gemm_refuses_a_table_that_leaves_its_arena(ctx):
    from pymes_amd.solver.ueg_cc import Tasks
    tasks = sectors.make_tasks([4], [4], [4], [0], [0], [0], [4], [4], [4])
    with pytest.raises(ValueError, match="past the end of operand C"):
        Tasks(ctx, tasks, 16, 16, 15)
    table = Tasks(ctx, tasks, 16, 16, 16)
    with pytest.raises(ValueError, match="shorter than the task table was checked for"):
        table.run(ctx.zeros((16,)), ctx.zeros((16,)), ctx.zeros((15,)))
    with pytest.raises(_lib.PymesError, match="sector_gemm: null argument"):
        ctx.lib.call("pymes_sector_gemm", ctx.handle, C.c_void_p(table.dev.ptr), 1, 1, None, None, None)


def test_sector_gather_and_update_against_numpy(ctx):
    from pymes_amd.solver.ueg_cc import SectorCCD, gather, upload_raw
    rng = np.random.default_rng(5)
    n, ns = 70001, 4097                       # more than one pass of the grid-stride loop
    src, src2, dst = rng.standard_normal(ns), rng.standard_normal(ns), rng.standard_normal(n)
    m1, m2 = rng.integers(0, ns, n), rng.integers(0, ns, n)
    d1, d2 = upload_raw(ctx, m1), upload_raw(ctx, m2)
    d1.count = d2.count = n
    out = ctx.array(np.full(n, np.nan))
    gather(ctx, out, ctx.array(src), d1, 2.0, ctx.array(src2), d2, -1.0)
    assert np.array_equal(out.get(), 2.0 * src[m1] - src2[m2])            # 2 D - C: one rounding either way
    out = ctx.array(dst)
    gather(ctx, out, ctx.array(src), d1, beta=1.0)
    assert np.abs(out.get() - (dst + src[m1])).max() < 1e-15
    r, den, t = rng.standard_normal(n), -1.0 - rng.random(n), rng.standard_normal(n)
    tn, dt = ctx.empty((n,)), ctx.empty((n,))
    SectorCCD._update(ctx, tn, dt, ctx.array(t), ctx.array(r), ctx.array(den), -0.25)
    assert np.array_equal(dt.get(), r / (den - 0.25)) and np.array_equal(tn.get(), t + r / (den - 0.25))
    SectorCCD._update(ctx, tn, None, None, ctx.array(r), ctx.array(den), 0.0)
    assert np.array_equal(tn.get(), r / den)


# ---- pymes_ueg_eval_2b_list against the dense builder ---------------------------------------------------------------
def model(nel, cutoff, rs=1.0, k_shift=None, k_cutoff=None, gamma=None):
    from pymes_amd.model.ueg import UEG
    m = UEG(nel, nel // 2, nel // 2, rs)
    m.init_single_basis(cutoff, **({"k_shift": list(k_shift)} if k_shift is not None else {}))
    m.k_cutoff, m.gamma = k_cutoff, gamma
    return m


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_list_against_dense(ctx, m, correlator, flags):
    tab = m.sector_tables()
    ints = quiet(m.eval_2b_sectors, tab, correlator=correlator, ctx=ctx, **flags)
    V = quiet(m.eval_2b_integrals, correlator=correlator, sp=0, on_device=True, ctx=ctx, **flags).get()
    worst, nonzero = 0.0, 0
    for name in ints.NAMES:
        idx = tab.block_pqrs(name)
        want, got = V[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]], ints[name].get()
        nonzero += np.count_nonzero(want)
        assert np.array_equal(want == 0, got == 0)
        worst = max(worst, float(ulps(got, want).max()) if len(want) else 0.0)
    assert nonzero > tab.nnz
    # everything the dense array holds outside the lists' support is what the sector path never stores: nothing conserving
    # is lost (the blocks of the lists cover klij, ijab, abij, iajb, iabj, abcd where momentum is conserved)
    assert tab.conserving(np.argwhere(V != 0)).all()
    return worst


@pytest.mark.parametrize("case", ["coulomb", "only_2b", "effect_2b", "rpa", "yukawa", "table", "twist"])
def test_integral_list_matches_the_dense_builder(ctx, case):
    """Equal to the bit: both kernels inline the same per-element function (ueg_element of kernels_integrals.hip) on the same
    prepared u_mat / E[p,r] tables, and the symmetrisation of is_effect_2b, 0.5 a + 0.5 b, is exact scaling and one rounding
    whether it is formed in the list kernel or by the two permute passes of the dense builder."""
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    m = model(14, 2, k_cutoff=1.0) if case != "twist" else \
        model(int(g["nel"]), int(g["cutoff"]), float(g["rs"]), k_shift=g["k_shift"], k_cutoff=float(g["k_cutoff"]))
    assert len(m.basis_fns) // 2 == (13 if case == "twist" else 19)
    runs = {"coulomb": [(None, {})], "only_2b": [(m.trunc, dict(is_only_2b=True))],
            "effect_2b": [(m.trunc, dict(is_effect_2b=True))], "rpa": [(m.trunc, dict(is_rpa_approx=True))],
            "yukawa": [(m.yukawa, dict(is_only_2b=True)), (m.yukawa, dict(is_effect_2b=True))],
            "table": [(lambda k2: m.trunc(k2), dict(is_only_2b=True)), (lambda k2: m.trunc(k2), dict(is_effect_2b=True))],
            "twist": [(None, {}), (m.trunc, dict(is_only_2b=True)), (m.trunc, dict(is_effect_2b=True))]}[case]
    for correlator, flags in runs:
        worst = check_list_against_dense(ctx, m, correlator, flags)
        print(f"{case} {sorted(flags)}: largest difference {worst:.2f} ulp")
        assert worst == 0.0


# ---- the sector residual against the dense one ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def coulomb(ctx):
    cache = {}

    def get(nel, cutoff):
        if (nel, cutoff) not in cache:
            m = model(nel, cutoff)
            tab = m.sector_tables()
            ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
            kin = np.array([b.kinetic for b in m.basis_fns[::2]])
            cache[nel, cutoff] = (m, tab, ints, ints.hf_orbital_energies(kin))
        return cache[nel, cutoff]
    return get


@pytest.mark.parametrize("nel,cutoff", [(14, 2), (14, 5), (54, 5), (14, 8)])
def test_residual_matches_the_dense_path(ctx, coulomb, nel, cutoff):
    """(14,2): empty sectors; (54,5): no = 27 above most block sizes, empty sectors; (14,8): 93 plane waves, |VV_P| up to 86,
    past one 64-row tile."""
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ueg_cc import SectorCCD
    m, tab, ints, eps = coulomb(nel, cutoff)
    no = nel // 2
    if (nel, cutoff) == (14, 8):
        assert tab.n == 93 and tab.n_vv.max() > 64
    if nel == 54 or cutoff == 2:
        assert (tab.n_vv == 0).any()
    rng = np.random.default_rng(11)
    T = rng.standard_normal(tab.nnz)
    T = 0.5 * (T + T[tab.pp_swap])
    V = quiet(m.eval_2b_integrals)
    from oracle import cc_oracle as oc
    B = {nm: np.ascontiguousarray(oc.split_blocks(no, V)[nm]) for nm in ("klij", "ijab", "abij", "iajb", "iabj", "abcd")}
    Td = tab.to_dense(T)
    for is_dcd in (False, True):
        want = CCD(no, is_dcd=is_dcd).get_residual(np.diag(eps), Td, B["klij"], B["ijab"], B["abij"], B["iajb"], B["iabj"],
                                                   B["abcd"])
        got = SectorCCD(no, is_dcd=is_dcd).get_residual(eps, ints, T)
        err, scale = np.abs(tab.to_dense(got) - want).max(), np.abs(want).max()
        host = sr.residual(tab, eps, T, {nm: ints[nm].get() for nm in ints.NAMES}, is_dcd=is_dcd)
        print(f"N={nel} cutoff={cutoff} dcd={is_dcd}: |sector - dense| = {err:.2e}, |sector - numpy| = "
              f"{np.abs(got - host).max():.2e}, max|R| = {scale:.2e}")
        assert err <= 1e-11 * scale
        assert np.abs(got - host).max() <= 1e-11 * scale


# ---- whole solves --------------------------------------------------------------------------------------------------
def tc_sector_problem(ctx, cutoff):
    """The calling sequence of tests/test_ueg.py::tc_problem on sectors: the Fock matrix from the only_2b integrals plus
    the doubly contracted 3-body term, the Hamiltonian only_2b + effect_2b."""
    ref = G[f"tc_N14_rs1.0_c{cutoff}"]
    m = model(ref["nel"], cutoff, ref["rs"], k_cutoff=ref["k_cutoff"])
    tab = m.sector_tables()
    v2 = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_only_2b=True, ctx=ctx)
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    eps = v2.hf_orbital_energies(kin) + quiet(m.double_contractions_in_3_body)
    return ref, eps, v2 + quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_effect_2b=True, ctx=ctx)


@pytest.mark.parametrize("cutoff", [2, 3, 5])
def test_transcorrelated_solves(ctx, cutoff):
    from pymes_amd.model.ueg import UEG
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ueg_cc import SectorCCD
    from tests.test_ueg import tc_problem
    ref, eps, ints = tc_sector_problem(ctx, cutoff)
    no, V, f = tc_problem(UEG, ref["nel"], ref["rs"], cutoff, ref["k_cutoff"])[:3]
    assert np.abs(f.diagonal() - eps).max() < 1e-12
    for key, is_dcd in (("ccd", False), ("dcd", True)):
        if key not in ref["energies"]:
            continue
        got = quiet(SectorCCD(no, delta_e=1e-10, is_dcd=is_dcd).solve, eps, ints)
        dense = quiet(CCD(no, delta_e=1e-10, is_dcd=is_dcd).solve, f, V)
        print(f"c{cutoff} {key}: sector {got['ccd e']:.12f}, dense {dense['ccd e']:.12f}, recorded {ref['energies'][key]:.12f}")
        assert abs(got["ccd e"] - ref["energies"][key]) < 1e-8
        assert abs(got["ccd e"] - dense["ccd e"]) < 1e-10
        assert np.abs(got["t2 amp"].to_dense() - dense["t2 amp"]).max() < 1e-8
        assert sorted(got) == sorted(dense)


def test_coulomb_57_plane_waves_level_shift_and_warm_start(ctx):
    from pymes_amd.mean_field import hf
    from pymes_amd.solver.ccd import CCD
    from pymes_amd.solver.ueg_cc import SectorCCD
    ref = G["coulomb_N14_rs0.5_c5"]
    m = model(ref["nel"], ref["cutoff"], ref["rs"])
    no, tab = ref["nel"] // 2, m.sector_tables()
    assert tab.n == ref["n_pw"]
    ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    eps = ints.hf_orbital_energies(kin)
    V = quiet(m.eval_2b_integrals, sp=1)
    f = hf.construct_hf_matrix(no, np.diag(kin), V)
    assert np.abs(f.diagonal() - eps).max() < 1e-12 and np.count_nonzero(f - np.diag(f.diagonal())) == 0
    rc = quiet(SectorCCD(no).solve, eps, ints, level_shift=-1., max_iter=60)
    rd = quiet(SectorCCD(no, is_dcd=True).solve, eps, ints, level_shift=-1., max_iter=60, amps=rc["t2 amp"])
    assert abs(rc["ccd e"] - ref["energies"]["ccd"]) < 1e-8
    assert abs(rd["ccd e"] - ref["energies"]["dcd_from_ccd_amps"]) < 1e-8
    dc = quiet(CCD(no).solve, f, V, level_shift=-1., sp=0, max_iter=60)
    amps = dc["t2 amp"].copy()
    dd = quiet(CCD(no, is_dcd=True).solve, f, V, level_shift=-1., sp=0, max_iter=60, amps=amps)
    print(f"ccd: sector {rc['ccd e']:.12f} dense {dc['ccd e']:.12f}; dcd: sector {rd['ccd e']:.12f} dense {dd['ccd e']:.12f}")
    assert abs(rc["ccd e"] - dc["ccd e"]) < 1e-10 and abs(rd["ccd e"] - dd["ccd e"]) < 1e-10
    # a dense warm start is accepted too
    rd2 = quiet(SectorCCD(no, is_dcd=True).solve, eps, ints, level_shift=-1., max_iter=60, amps=rc["t2 amp"].to_dense())
    assert abs(rd2["ccd e"] - rd["ccd e"]) < 1e-12


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals(ctx, coulomb):
    from pymes_amd.solver.ueg_cc import SectorAmplitudes, SectorCCD
    m, tab, ints, eps = coulomb(14, 2)
    for flag in ("is_dr_ccd", "is_bruekner"):
        with pytest.raises(NotImplementedError, match="dr-CCD and Brueckner energies"):
            SectorCCD(7, **{flag: True})
    with pytest.raises(TypeError, match="ints must be SectorIntegrals"):
        SectorCCD(7).solve(eps, np.zeros((19,) * 4))
    with pytest.raises(ValueError, match="do not match the solver"):
        SectorCCD(6).solve(eps, ints)
    with pytest.raises(ValueError, match="do not match the solver"):
        SectorCCD(7).solve(eps[:-1], ints)
    with pytest.raises(ValueError, match="the Fock matrix must be diagonal"):
        SectorCCD(7).solve(np.diag(eps) + 1e-3, ints)
    other = model(14, 3).sector_tables()
    with pytest.raises(ValueError, match="the tables do not belong to this basis"):
        m.eval_2b_sectors(other, ctx=ctx)
    with pytest.raises(ValueError, match="the tables of the amplitudes do not match the integrals"):
        quiet(SectorCCD(7).solve, eps, ints, amps=SectorAmplitudes(other, np.zeros(other.nnz)))
    dense = np.zeros((12, 12, 7, 7))
    dense[0, 0, 0, 1] = 1.0
    with pytest.raises(ValueError, match="amps has weight outside the momentum-conserving support"):
        quiet(SectorCCD(7).solve, eps, ints, amps=dense)
    skew = np.random.default_rng(0).standard_normal(tab.nnz)
    with pytest.raises(ValueError, match="the amplitudes are not exchange-symmetric"):
        quiet(SectorCCD(7).solve, eps, ints, amps=skew)
    lopsided = ints * 1.0
    w1 = lopsided["w1"].get()
    w1[0] += 1.0
    lopsided["w1"].set(w1)
    with pytest.raises(ValueError, match="not symmetric under the exchange of the two electrons"):
        SectorCCD(7).solve(eps, lopsided)
    with pytest.raises(ValueError, match="same tables and context"):
        ints + 1.0
    ctx.graph_begin()
    try:
        with pytest.raises(RuntimeError, match="SectorCCD.solve: the context is recording a launch graph"):
            SectorCCD(7).solve(eps, ints)
        with pytest.raises(RuntimeError, match="eval_2b_sectors: the context is recording a launch graph"):
            m.eval_2b_sectors(tab, ctx=ctx)
        with pytest.raises(_lib.PymesError, match="ueg_eval_2b_list while a launch graph is being recorded"):
            ctx.lib.call("pymes_ueg_eval_2b_list", ctx.handle, 19, 14, 3, 0, 1.0, 0.0, 1.0, 30, 0, None, None, None, None, 0,
                         None, 0, None)
    finally:
        ctx.graph_abort()
    # the context is usable afterwards
    assert abs(quiet(SectorCCD(7, delta_e=1e-9).solve, eps, ints)["ccd e"]) > 0.0
