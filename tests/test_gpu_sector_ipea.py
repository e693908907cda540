"""GPU: the sector IP- / EA-EOM-CCD (pymes_amd/solver/ueg_eom.py; csrc/kernels_sector.hip, pymes_sector_ipea_*): the
sigma of stacked vectors and the diagonals against the numpy restatement (tests/_sector_ipea_reference.py) on the host copies
of the device's own integrals, whole solves against numpy.linalg.eig of the restatement's block matrix and against the dense
IP_EOM_CCSD / EA_EOM_CCSD, SectorCCD.solve(quasiparticles=...), and the refusals."""
import ctypes as C

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.solver.sectors import QuasiparticleTables, TriplesTables
from tests import _sector_ipea_reference as sq
from tests.test_gpu_sector_cc import model, quiet, tc_sector_problem
from tests.test_gpu_sector_lambda import host, symmetric
from tests.test_gpu_sector_triples import twisted_model
from tests.test_sector_ipea_reference import all_targets, some_targets

pytestmark = pytest.mark.gpu
KINDS = ("ip", "ea")


def record(line):
    """The observed differences: `pytest -s` prints them, and profiles/sector_ipea/gpu_test_errors.txt keeps one such run."""
    print(line)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from pymes_amd.device import Context
    c = Context(1, 1, lib=gpu_lib)
    yield c
    c.close()


def families(m, fn, mode, *args, **kw):
    """One integral object of the Coulomb or of the transcorrelated (only_2b + effect_2b) Hamiltonian."""
    if mode == "coulomb":
        return quiet(fn, *args, **kw)
    return quiet(fn, *args, correlator=m.trunc, is_only_2b=True, **kw) + quiet(fn, *args, correlator=m.trunc, is_effect_2b=True, **kw)


@pytest.fixture(scope="module")
def hamiltonians(ctx):
    """(model, tables, triples tables, integrals, two-sided triples integrals, orbital energies, host copies) per case and mode,
    built once."""
    cache = {}

    def get(case, mode):
        if (case, mode) not in cache:
            m = twisted_model() if case == "twist" else model(*case, k_cutoff=1.0)
            tab = m.sector_tables()
            tt = TriplesTables(tab)
            kin = np.array([b.kinetic for b in m.basis_fns[::2]])
            ints = families(m, m.eval_2b_sectors, mode, tab, ctx=ctx)
            tints = families(m, m.eval_2b_triples, mode, tt, ctx=ctx, both_sides=True)
            lists = {nm: getattr(tints, nm).get() for nm in tints.SIDES}
            cache[case, mode] = (m, tab, tt, ints, tints, ints.hf_orbital_energies(kin), host(ints), lists)
        return cache[case, mode]
    return get


def ladders_for(ctx, m, tt, mode, targets):
    return families(m, m.eval_2b_ladder, mode, tt, targets, ctx=ctx)


def reference_blocks(tab, tt, hi, lists, ladders, targets):
    ladder = None
    if ladders is not None:
        ladder = [(ladders.qtabs[p].extra_pqrs(), ladders.arenas[p].get()[:ladders.qtabs[p].extra_size]) for p in targets]
    return sq.blocks(tab, tt, hi, lists, ladder=ladder)


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# ---- sigma and diagonals against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("case", [(14, 2), (14, 5), (54, 5), "twist"], ids=str)
def test_sigma_matches_the_numpy_restatement(ctx, hamiltonians, case, mode, kind):
    """Stacks of 1, 3 and 17 vectors (the 16-wide N tile of the products is crossed) for the lowest and the highest admissible
    target and one whose block has positions outside the space: 1e-11 max|sigma| against the restatement (the bound of
    test_lambda_residual_matches_the_numpy_restatement), an exact +0.0 outside the space, identical applies bit-equal, stacked
    against single within 1e-13 max|sigma|.  (14,2) has empty sectors, (54,5) an IP vector of 729 elements and (14,5)
    an EA vector of 350: past one 256-lane block; the twisted basis has q without -q; "tc" is not Hermitian."""
    from pymes_amd.solver.ueg_eom import SectorIPEASigma
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians(case, mode)
    T = symmetric(tab, 11, 0.1)
    targets = some_targets(tt, kind)
    ladders = ladders_for(ctx, m, tt, mode, targets) if kind == "ea" else None
    blk = reference_blocks(tab, tt, hi, lists, ladders, targets)
    sig = SectorIPEASigma(kind, eps, ints, tints, T, ladders=ladders)
    rng = np.random.default_rng(3)
    try:
        for p in targets:
            qt = sig.tables_of(p)
            mask = qt.inside.reshape(qt.shape)
            r1, R = rng.standard_normal(17), rng.standard_normal((17,) + qt.shape) * mask
            want1, want, leak = sq.sigma(qt, eps, blk, T, r1, R)
            assert leak == 0.0
            scale = max(np.abs(want).max(), np.abs(want1).max())
            got1, got = sig.get_sigma(p, r1, R)
            again1, again = sig.get_sigma(p, r1, R)
            err = max(np.abs(got - want).max(), np.abs(got1 - want1).max())
            three1, three = sig.get_sigma(p, r1[:3], R[:3])
            one1, one = sig.get_sigma(p, r1[1], R[1])
            stack = max(np.abs(three - got[:3]).max(), np.abs(three1 - got1[:3]).max(), np.abs(one - got[1]).max(),
                        abs(one1 - got1[1]))
            record(f"sigma {case} {mode} {kind} target {p} (dim {qt.dim}, extra {qt.extra_size}): |device - numpy| = {err:.2e}, "
                   f"stacked against single {stack:.2e}, max|sigma| = {scale:.2e}")
            assert err <= 1e-11 * scale
            assert stack <= 1e-13 * scale
            assert np.array_equal(bits(got), bits(again)) and np.array_equal(bits(got1), bits(again1))
            outside = got[:, ~mask]
            assert np.array_equal(bits(outside), np.zeros(outside.shape, dtype=np.int64))         # +0.0, not -0.0
    finally:
        sig.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [(14, 2), (14, 5), (54, 5), "twist"], ids=str)
def test_diagonals_element_by_element(ctx, hamiltonians, case, kind):
    """d1, every element of d2 and every L_oo, L_vv against numpy (tests/_sector_ipea_reference.diagonals, which finds the
    implied virtual by comparing momenta, not through the tables): within 4 ulp, not bit-equal, and the ulp is that of the sum
    of the magnitudes of the terms that enter the element.  Why not bit-equal: L is eps plus up to o v products, which the
    device adds one after the other with an fma and numpy in pairs.  Why the magnitudes: eps of either sign and signed
    products cancel in L, and three L cancel in d2 (it vanishes at a Fermi-surface degeneracy), so an ulp of the element
    itself bounds nothing; the rounding errors of a sum scale with the sum of |terms|.  The observed differences are printed in
    both units.  Positions outside the space hold QuasiparticleTables.OUTSIDE to the bit; the pad between r1 and R is zero."""
    from pymes_amd.solver.ueg_eom import SectorIPEASigma
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians(case, "tc")
    T = symmetric(tab, 11, 0.1)
    sig = SectorIPEASigma(kind, eps, ints, tints, T)
    try:
        for p in some_targets(tt, kind):
            qt, lay, d = sig.tables_of(p), sig.layout(p), sig.diagonals(p)
            d1, d2, L = lay.part1(d).get()[0], lay.part2(d).get(), sig.L_host
            want1, want2, wantL, m1, m2, mL = sq.diagonals(qt, eps, hi, T)
            inside = qt.inside.reshape(qt.shape)
            assert np.array_equal(inside, want2 != qt.OUTSIDE)
            assert np.array_equal(bits(d2[~inside]), bits(np.full((~inside).sum(), qt.OUTSIDE)))
            e2, eL = np.abs(d2 - want2)[inside], np.abs(L - wantL)
            own = max((e2 / np.spacing(np.abs(want2[inside]))).max(initial=0.0), (eL / np.spacing(np.abs(wantL))).max())
            terms = max((e2 / np.spacing(m2[inside])).max(initial=0.0), (eL / np.spacing(mL)).max(), abs(d1 - want1) / np.spacing(m1))
            record(f"diagonals {case} {kind} target {p}: max|device - numpy| = {max(e2.max(initial=0.0), eL.max()):.2e}, that is "
                   f"{terms:.2f} ulp of the sum of |terms| and {own:.1f} ulp of the element itself")
            assert abs(d1 - want1) <= 4 * np.spacing(m1)
            assert (e2 <= 4 * np.spacing(m2[inside])).all()
            assert (eL <= 4 * np.spacing(mL)).all()
            assert np.all(np.isfinite(d2)) and np.all(d2 != 0.0)
            assert np.array_equal(d.get()[1:lay.off2], np.zeros(lay.off2 - 1))
    finally:
        sig.close()


@pytest.mark.parametrize("kind", KINDS)
def test_more_vectors_than_one_launch_takes(ctx, hamiltonians, kind):
    """33 stacked vectors are worked off in groups of 32 and 1: every sigma against an apply of its own, within 1e-13
    max|sigma|, and the outputs land at their own places."""
    from pymes_amd.solver.ueg_eom import MAX_STACK, SectorIPEASigma
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians((14, 5), "tc")
    p = some_targets(tt, kind)[-1]
    ladders = ladders_for(ctx, m, tt, "tc", [p]) if kind == "ea" else None
    sig = SectorIPEASigma(kind, eps, ints, tints, symmetric(tab, 11, 0.1), ladders=ladders)
    try:
        qt, k = sig.tables_of(p), MAX_STACK + 1
        rng = np.random.default_rng(8)
        r1, R = rng.standard_normal(k), rng.standard_normal((k,) + qt.shape) * qt.inside.reshape(qt.shape)
        got1, got = sig.get_sigma(p, r1, R)
        worst, scale = 0.0, np.abs(got).max()
        for z in range(k):
            one1, one = sig.get_sigma(p, r1[z], R[z])
            worst = max(worst, np.abs(one - got[z]).max(), abs(one1 - got1[z]))
        record(f"stack of {k} {kind} target {p} (dim {qt.dim}): stacked against single {worst:.2e}, max|sigma| = {scale:.2e}")
        assert scale > 0 and worst <= 1e-13 * scale
    finally:
        sig.close()


# ---- whole solves -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def converged(ctx):
    """(model, tables, triples tables, eps, ints, tints, amplitudes, host copies) of a converged SectorCCD solve, once."""
    from pymes_amd.solver.ueg_cc import SectorCCD
    cache = {}

    def get(cutoff, mode):
        if (cutoff, mode) not in cache:
            if mode == "tc":
                ref, eps, ints = tc_sector_problem(ctx, cutoff)
                m = model(ref["nel"], cutoff, ref["rs"], k_cutoff=ref["k_cutoff"])
            else:
                m = model(14, cutoff)
                ints = quiet(m.eval_2b_sectors, m.sector_tables(), ctx=ctx)
                eps = ints.hf_orbital_energies(np.array([b.kinetic for b in m.basis_fns[::2]]))
            tab = ints.tables
            tt = TriplesTables(tab)
            tints = families(m, m.eval_2b_triples, mode, tt, ctx=ctx, both_sides=True)
            amps = quiet(SectorCCD(tab.no, delta_e=1e-11).solve, eps, ints)["t2 amp"]
            lists = {nm: getattr(tints, nm).get() for nm in tints.SIDES}
            cache[cutoff, mode] = (m, tab, tt, eps, ints, tints, amps, host(ints), lists)
        return cache[cutoff, mode]
    return get


def block_spectrum(qt, eps, blk, T):
    """(eigenvalues, right eigenvectors, condition number of the eigenvector matrix, which eigenvalues the singles unit vector
    reaches) of the block on the positions inside the space."""
    H = sq.matrix(qt, eps, blk, T)
    keep = np.concatenate([[0], 1 + np.flatnonzero(qt.inside)])
    w, vr = np.linalg.eig(H[np.ix_(keep, keep)])
    reach = np.abs(np.linalg.inv(vr)[:, 0]) > 1e-8
    return w, vr, float(np.linalg.cond(vr)), reach


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["coulomb", "tc"])
@pytest.mark.parametrize("cutoff", [2, 3])
def test_solves_against_the_spectrum_of_the_restatement(ctx, converged, cutoff, mode, kind):
    """n_roots = 1: the root is the lowest eigenvalue of the block that the singles unit vector reaches (left eigenvector
    component above 1e-8), i.e. the lowest root of the Krylov space of the start vector.  n_roots = 3: every root has
    |s - w r| / |r| < r_epsilon under a fresh sigma of the restatement and lies within kappa |s - w r| / |r| of an eigenvalue of the
    block (Bauer-Fike, kappa the condition number of the block's eigenvector matrix); the roots ascend.  Which three roots they
    are is not asserted: symmetry-decoupled and degenerate satellites make that ill-defined."""
    from pymes_amd.solver.ueg_eom import SectorEA_EOM_CCD, SectorIP_EOM_CCD
    m, tab, tt, eps, ints, tints, amps, hi, lists = converged(cutoff, mode)
    cls = SectorIP_EOM_CCD if kind == "ip" else SectorEA_EOM_CCD
    T = amps.get()
    targets = some_targets(tt, kind)
    ladders = ladders_for(ctx, m, tt, mode, targets) if kind == "ea" else None
    blk = reference_blocks(tab, tt, hi, lists, ladders, targets)
    one = quiet(cls(tab.no, n_roots=1, r_epsilon=1e-8).solve, eps, ints, tints, amps, targets, ladders=ladders)
    eps_r = 1e-6
    for n, p in enumerate(targets):
        qt = QuasiparticleTables(tt, kind, p)
        w, vr, kappa, reach = block_spectrum(qt, eps, blk, T)
        want = w.real[reach].min()
        got, res = one[kind + " e"][n, 0], one["residuals"][n, 0]
        record(f"solve c{cutoff} {mode} {kind} target {p} (dim {qt.dim}): root {got:.10f}, eig {want:.10f}, diff {abs(got - want):.2e}, "
               f"residual {res:.1e}, kappa {kappa:.2f}, reachable {int(reach.sum())}, passes {one['passes'][n]}, "
               f"singles weight {one['singles weight'][n, 0]:.4f}")
        assert one["converged"][n]
        assert abs(got - want) <= kappa * max(res, 1e-13) * max(1.0, abs(want)) + 1e-12
        if qt.dim < 3:
            continue
        three = quiet(cls(tab.no, n_roots=3, r_epsilon=eps_r).solve, eps, ints, tints, amps, [p], ladders=ladders, keep_vectors=True)
        e = three[kind + " e"][0]
        assert np.all(np.diff(e) >= 0)
        for root, (r1, R) in enumerate(three[kind + " vectors"][0]):
            s1, S, _ = sq.sigma(qt, eps, blk, T, r1, R[None])
            nrm = np.sqrt(r1[0] ** 2 + (R ** 2).sum())
            res = np.sqrt((s1[0] - e[root] * r1[0]) ** 2 + ((S[0] - e[root] * R) ** 2).sum()) / nrm
            near = np.abs(w - e[root]).min()
            record(f"  three roots: root {root} {e[root]:.10f}, fresh residual {res:.2e}, nearest eigenvalue at {near:.2e}, "
                   f"bound {kappa * res:.2e}")
            assert res < eps_r
            assert near <= kappa * res + 1e-12


def dense_route(m, ctx, eps, amps, tab, mode, cls_name, n_roots=1):
    """Root 0 (and its residual) of the dense IP_EOM_CCSD / EA_EOM_CCSD on the dense integrals and the dense amplitudes."""
    from oracle import cc_oracle as oc
    from pymes_amd.solver import eom_ip_ea
    dense = lambda **flags: quiet(m.eval_2b_integrals, sp=0, on_device=True, ctx=ctx, **flags).get()
    if mode == "tc":
        V = dense(correlator=m.trunc, is_only_2b=True) + dense(correlator=m.trunc, is_effect_2b=True)
    else:
        V = dense()
    solver = getattr(eom_ip_ea, cls_name)(tab.no, n_roots=n_roots)
    e = quiet(solver.solve, np.diag(eps), oc.split_blocks(tab.no, 0.5 * (V + V.transpose(1, 0, 3, 2))), amps.to_dense())
    return float(e[0]), float(solver.residual_norms[0])


@pytest.mark.parametrize("mode", ["coulomb", "tc"])
def test_whole_route_against_the_dense_library(ctx, converged, mode):
    """(14,3): the lowest "ip e" over all occupied targets and the lowest "ea e" over all virtual targets against root 0 of
    IP_EOM_CCSD / EA_EOM_CCSD on the dense integrals and to_dense() amplitudes, within the sum of the two Bauer-Fike bounds
    (kappa of the winning block times the two residuals), and "qp gap" likewise."""
    from pymes_amd.solver.ueg_eom import sector_quasiparticles
    m, tab, tt, eps, ints, tints, amps, hi, lists = converged(3, mode)
    ip_t, ea_t = all_targets(tab, "ip"), all_targets(tab, "ea")
    ladders = ladders_for(ctx, m, tt, mode, ea_t)
    res = quiet(sector_quasiparticles, tab.no, eps, ints, amps, tints=tints, ip=ip_t, ea=ea_t, ladders=ladders, r_epsilon=1e-8)
    total, gap = 0.0, 0.0
    for kind, targets, name in (("ip", ip_t, "IP_EOM_CCSD"), ("ea", ea_t, "EA_EOM_CCSD")):
        e = res[kind + " e"][:, 0]
        win = targets[int(np.argmin(e))]
        blk = reference_blocks(tab, tt, hi, lists, ladders if kind == "ea" else None, [win])
        kappa = block_spectrum(QuasiparticleTables(tt, kind, win), eps, blk, amps.get())[2]
        dense, dres = dense_route(m, ctx, eps, amps, tab, mode, name)
        bound = kappa * (1e-8 + dres) * max(1.0, abs(dense)) + 1e-12
        total += bound
        record(f"route c3 {mode} {kind}: sector {e.min():.10f} (target {win}), dense {dense:.10f}, diff {abs(e.min() - dense):.2e}, "
               f"bound {bound:.2e} (kappa {kappa:.2f}, dense residual {dres:.1e})")
        assert abs(e.min() - dense) <= bound
        gap += dense
    record(f"route c3 {mode}: qp gap {res['qp gap']:.10f}, dense {gap:.10f}")
    assert abs(res["qp gap"] - gap) <= total
    assert res["qp gap"] == res["ip e"].min() + res["ea e"].min()


def test_solve_with_quasiparticles_and_lambda_triples_on_the_same_integrals(ctx, converged):
    """SectorCCD.solve(quasiparticles=...) together with lambda_triples= on the same tints: the keys are there and the values
    are those of the stand-alone solvers on the amplitudes it returns, to the bit."""
    from pymes_amd.solver.ueg_cc import SectorCCD, SectorEA_EOM_CCD, SectorIP_EOM_CCD
    m, tab, tt, eps, ints, tints, _, _, _ = converged(2, "tc")
    ip_t, ea_t = [0, tab.no - 1], [tab.no, tab.n - 1]
    ladders = ladders_for(ctx, m, tt, "tc", ea_t)
    out = quiet(SectorCCD(tab.no, delta_e=1e-9).solve, eps, ints, lambda_triples=tints,
                quasiparticles=dict(tints=tints, ip=ip_t, ea=ea_t, n_roots=2, ladders=ladders))
    for key in ("ip e", "ea e", "ip singles weight", "ea singles weight", "qp gap", "lambda (t) e", "ccd(t)_lambda e"):
        assert key in out
    assert out["ip e"].shape == (2, 2) and out["ea e"].shape == (2, 2)
    alone_ip = quiet(SectorIP_EOM_CCD(tab.no, n_roots=2).solve, eps, ints, tints, out["t2 amp"], ip_t)
    alone_ea = quiet(SectorEA_EOM_CCD(tab.no, n_roots=2).solve, eps, ints, tints, out["t2 amp"], ea_t, ladders=ladders)
    assert np.array_equal(bits(out["ip e"]), bits(alone_ip["ip e"])) and np.array_equal(bits(out["ea e"]), bits(alone_ea["ea e"]))
    assert np.array_equal(bits(out["ip singles weight"]), bits(alone_ip["singles weight"]))
    assert out["qp gap"] == out["ip e"].min() + out["ea e"].min()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ctx, hamiltonians):
    from pymes_amd.device import Context
    from pymes_amd.solver.ueg_eom import SectorEA_EOM_CCD, SectorIP_EOM_CCD, SectorIPEASigma
    m, tab, tt, ints, tints, eps, hi, lists = hamiltonians((14, 2), "tc")
    T, skew = symmetric(tab, 1, 0.1), np.random.default_rng(0).standard_normal(tab.nnz)
    one_sided = quiet(m.eval_2b_triples, tt, ctx=ctx)
    with pytest.raises(ValueError, match="SectorIPEASigma: the triples integrals lack the right-hand families"):
        SectorIPEASigma("ip", eps, ints, one_sided, T)
    other = model(14, 3)
    foreign = quiet(other.eval_2b_triples, other.sector_tables(), ctx=ctx, both_sides=True)
    with pytest.raises(ValueError, match="belong to other tables or another context"):
        SectorIPEASigma("ip", eps, ints, foreign, T)
    ctx2 = Context(1, 1, lib=ctx.lib)
    try:
        elsewhere = quiet(m.eval_2b_triples, tt, ctx=ctx2, both_sides=True)
        with pytest.raises(ValueError, match="belong to other tables or another context"):
            SectorIPEASigma("ea", eps, ints, elsewhere, T)
    finally:
        ctx2.close()
    with pytest.raises(TypeError, match="SectorIPEASigma: ints must be SectorIntegrals"):
        SectorIPEASigma("ip", eps, np.zeros((19,) * 4), tints, T)
    with pytest.raises(ValueError, match="kind must be 'ip' or 'ea'"):
        SectorIPEASigma("ee", eps, ints, tints, T)
    with pytest.raises(ValueError, match="SectorIPEASigma: the Fock matrix must be diagonal"):
        SectorIPEASigma("ip", np.diag(eps) + 1e-3, ints, tints, T)
    with pytest.raises(ValueError, match="SectorIPEASigma: the amplitudes are not exchange-symmetric"):
        SectorIPEASigma("ip", eps, ints, tints, skew)
    dense = np.zeros((tab.nv, tab.nv, tab.no, tab.no))
    dense[0, 0, 0, 1] = 1.0
    with pytest.raises(ValueError, match="weight outside the momentum-conserving support"):
        SectorIPEASigma("ea", eps, ints, tints, dense)
    lopsided = ints * 1.0
    w1 = lopsided["w1"].get()
    w1[0] += 1.0
    lopsided["w1"].set(w1)
    with pytest.raises(ValueError, match="SectorIPEASigma: the integrals are not symmetric under the exchange"):
        SectorIPEASigma("ip", eps, lopsided, tints, T)
    with pytest.raises(ValueError, match="SectorIP_EOM_CCD.solve: the tables of the integrals"):
        SectorIP_EOM_CCD(6).solve(eps, ints, tints, T, [0])
    with pytest.raises(ValueError, match="the IP target 7 is not an occupied orbital"):
        SectorIP_EOM_CCD(7).solve(eps, ints, tints, T, [7])
    with pytest.raises(ValueError, match="the EA target 6 is not a virtual orbital"):
        SectorEA_EOM_CCD(7).solve(eps, ints, tints, T, [6])
    dim = QuasiparticleTables(tt, "ea", 7).dim
    with pytest.raises(ValueError, match="n_roots = %d exceeds the dimension %d of the block of target 7" % (dim + 1, dim)):
        SectorEA_EOM_CCD(7, n_roots=dim + 1).solve(eps, ints, tints, T, [7])
    m5, tab5, tt5, ints5, tints5, eps5, _, _ = hamiltonians((14, 5), "coulomb")
    with pytest.raises(ValueError, match="reads V_abcd at pair momenta.*eval_2b_ladder"):
        SectorEA_EOM_CCD(7).solve(eps5, ints5, tints5, symmetric(tab5, 1, 0.1), [7])
    sig = SectorIPEASigma("ip", eps, ints, tints, T)
    x = ctx.zeros((64,))
    p, pp = C.c_void_p(x.ptr), (C.c_void_p * 1)(x.ptr)
    with pytest.raises(_lib.PymesError, match="sector_ipea_pack: 1 <= k <= 32 vectors per call"):
        ctx.lib.call("pymes_sector_ipea_pack", ctx.handle, 33, pp, 1, p, p, p, p, p, p)
    ctx.graph_begin()
    try:
        with pytest.raises(RuntimeError, match="SectorIPEASigma: the context is recording a launch graph"):
            SectorIPEASigma("ip", eps, ints, tints, T)
        with pytest.raises(RuntimeError, match="the context is recording a launch graph"):
            sig.get_sigma(0, 1.0, np.zeros((7, 7)))
        with pytest.raises(_lib.PymesError, match="sector_ipea_pack while a launch graph is being recorded"):
            ctx.lib.call("pymes_sector_ipea_pack", ctx.handle, 1, pp, 1, p, p, p, p, p, p)
        with pytest.raises(_lib.PymesError, match="sector_ipea_assemble while a launch graph is being recorded"):
            ctx.lib.call("pymes_sector_ipea_assemble", ctx.handle, 1, pp, pp, pp, pp, 1, p, p, p, p, p, p, 0.0, p, p, p)
        with pytest.raises(_lib.PymesError, match="sector_ipea_prepare while a launch graph is being recorded"):
            ctx.lib.call("pymes_sector_ipea_prepare", ctx.handle, 0, 0, 1, 1, p, p, tt.box.ctypes.data_as(C.c_void_p), *[p] * 7,
                         -1.0, p, p, p)
        with pytest.raises(_lib.PymesError, match="sector_ipea_correction while a launch graph is being recorded"):
            out = np.zeros(2)
            ctx.lib.call("pymes_sector_ipea_correction", ctx.handle, 1, pp, pp, out.ctypes.data_as(C.c_void_p), p, 0.0, pp, 1, 32,
                         64, out.ctypes.data_as(C.c_void_p))
    finally:
        ctx.graph_abort()
        sig.close()
