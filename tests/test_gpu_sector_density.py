"""GPU: the sector densities (pymes_amd/solver/ueg_cc.py, SectorDensity; csrc/kernels_sector.hip, pymes_sector_bin_sums,
pymes_sector_pair_transfer, pymes_sector_gamma): gamma and every stored family of the density arena against the
numpy restatement (tests/_sector_density_reference.py), the two transfer-sum kernels alone, expectation values against the
dense Lagrangian and against the transfer sums, whole solves with ``density=True``, a Hellmann-Feynman derivative for DCD,
and the refusals.  The amplitudes and lambda are seeded and exchange-symmetric wherever nothing has to be solved."""
import ctypes as C

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.solver.sectors import BLOCKS
from tests import _rdm2_reference as r2
from tests import _sector_density_reference as sd
from tests.test_gpu_sector_cc import G, model, quiet, tc_sector_problem
from tests.test_gpu_sector_lambda import ctx, hamiltonians, host, symmetric      # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

CASES = [(14, 2), (14, 5), (54, 5), "twist"]
EPS = 2.0 ** -53


def record(line):
    """The observed differences: `pytest -s` prints them, and profiles/sector_density/gpu_test_errors.txt keeps one such run."""
    print(line)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def seeded(tab):
    return symmetric(tab, 11, 0.1), symmetric(tab, 12)


def density_of(ints, eps, tab, is_dcd):
    from pymes_amd.solver.ueg_cc import sector_density
    T, lam = seeded(tab)
    return sector_density(eps, ints, T, lam, is_dcd=is_dcd), T, lam


# ---- gamma and the density arena against the numpy restatement ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coulomb", "tc"])
@pytest.mark.parametrize("is_dcd", [False, True], ids=["ccd", "dcd"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_density_matches_the_numpy_restatement(ctx, hamiltonians, case, is_dcd, kind):
    """1e-11 max|.| per family, the bound of the sector products against their restatements (tests/test_gpu_sector_cc.py,
    tests/test_gpu_sector_lambda.py); identical calls give identical bits.  (14,2) and (54,5) have empty sectors, the twisted
    basis has q without -q.  The densities do not read the integrals: the two kinds differ in the context they come with."""
    tab, ints, eps = hamiltonians(case, kind)
    dens, T, lam = density_of(ints, eps, tab, is_dcd)
    again = density_of(ints, eps, tab, is_dcd)[0]
    gamma, Gref = sd.density(tab, T, lam, is_dcd)
    got = dens.gamma.get()
    err = np.abs(got - gamma).max()
    record(f"density {case} {kind} dcd={is_dcd}: gamma |device - numpy| = {err:.2e} of {np.abs(gamma).max():.2e}, tr = {got.sum():.1e}")
    assert err <= 1e-11 * np.abs(gamma).max()
    assert np.array_equal(bits(got), bits(again.gamma.get()))
    assert dens.FAMILIES == tuple(nm for nm in BLOCKS if nm != "abcd")
    for name in dens.FAMILIES:
        x, want = dens[name].get(), Gref[name]
        assert x.shape == want.shape
        if not len(want):
            continue
        err, scale = np.abs(x - want).max(), np.abs(want).max()
        record(f"density {case} {kind} dcd={is_dcd}: G_{name} |device - numpy| = {err:.2e}, max|G| = {scale:.2e}, {len(want)} elements")
        assert err <= 1e-11 * scale
        assert scale > 0 or (is_dcd and name in ("klcd", "wx"))
        assert np.array_equal(bits(x), bits(again[name].get()))
    n_k = dens.momentum_distribution()
    assert np.array_equal(n_k[:tab.no], got[:tab.no] + 2.0) and np.array_equal(n_k[tab.no:], got[tab.no:])
    assert abs(n_k.sum() - 2 * tab.no) <= 1e-13 * np.abs(n_k).sum()


# ---- pymes_sector_bin_sums alone ---------------------------------------------------------------------------------------------
def run_bin_sums(ctx, off, order, src, alpha=1.0, beta=0.0, start=None):
    from pymes_amd.solver.ueg_cc import upload_raw
    nb = len(off) - 1
    out = ctx.array(np.full(nb, np.nan) if start is None else start)
    o, l, s = upload_raw(ctx, np.ascontiguousarray(off, dtype=np.int64)), upload_raw(ctx, np.ascontiguousarray(order, dtype=np.int64)), \
        ctx.array(src)
    ctx.lib.call("pymes_sector_bin_sums", ctx.handle, C.c_void_p(out.ptr), nb, C.c_void_p(o.ptr), C.c_void_p(l.ptr),
                 C.c_void_p(s.ptr), float(alpha), float(beta))
    return out.get()


def check_bin_sums(ctx, off, order, src, label):
    nb = len(off) - 1
    want = np.array([src[order[off[b]:off[b + 1]]].sum() for b in range(nb)])
    scale = np.array([np.abs(src[order[off[b]:off[b + 1]]]).sum() for b in range(nb)])
    length = np.diff(off)
    got = run_bin_sums(ctx, off, order, src)                        # beta = 0: the NaN in `out` must not be read
    assert np.array_equal(bits(got), bits(run_bin_sums(ctx, off, order, src)))
    worst = np.abs(got - want) / np.maximum(length * EPS * scale, 1e-300)
    record(f"bin_sums {label}: {nb} bins, lengths {length.min()}..{length.max()}, worst |d| / (len 2^-53 sum|x|) = "
           f"{worst[length > 0].max():.2e}")
    assert (np.abs(got - want) <= length * EPS * scale).all()
    assert (bits(got[length == 0]) == 0).all()                      # an empty bin: +0.0
    start = np.random.default_rng(5).standard_normal(nb)
    acc = run_bin_sums(ctx, off, order, src, alpha=-0.5, beta=2.0, start=start)
    assert (np.abs(acc - (2.0 * start - 0.5 * want)) <= (length + 2) * EPS * (0.5 * scale + 2.0 * np.abs(start))).all()


def test_bin_sums_on_synthetic_lists(ctx):
    """Empty bins, a one-element bin, the two sides of the wavefront / workgroup threshold (256, 257), a bin of several
    workgroup passes, a bin count that is no multiple of the four bins of a workgroup; the source is NaN wherever no list
    points."""
    rng = np.random.default_rng(17)
    length = np.array([0, 1, 63, 64, 65, 0, 256, 257, 0, 5000, 1025, 2, 0])
    off = np.concatenate(([0], np.cumsum(length)))
    src = np.full(2 * off[-1] + 3, np.nan)
    order = rng.permutation(off[-1]) * 2 + 1                        # every second slot, in a seeded order
    src[order] = rng.standard_normal(off[-1])
    check_bin_sums(ctx, off, order, src, "synthetic")


def test_bin_sums_on_the_lists_of_a_basis(ctx, hamiltonians):
    """Every stored family at (54,5) against numpy; the q = 0 bin of wa is longer than one workgroup pass."""
    from pymes_amd.solver.sectors import TransferBins
    tab = hamiltonians((54, 5), "coulomb")[0]
    tb = TransferBins(tab)
    rng = np.random.default_rng(23)
    for name in TransferBins.STORED:
        off, order = tb.csr[name]
        if name == "wa":
            assert off[tb.zero + 1] - off[tb.zero] > 256
        check_bin_sums(ctx, off, order, rng.standard_normal(len(order)), name)


# ---- pymes_sector_pair_transfer alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
def test_pair_transfer_matches_the_binned_ladder_density(ctx, hamiltonians, case):
    """Against numpy's lam^P (T^P)^T summed by bin, within 1e-13 x the sum of |terms| of the bin; a bin that no virtual pair
    reaches is an exact +0.0; identical bits for two grid shapes and a repetition.  (54,5): more rows than one pass of
    the 256 threads of a workgroup, fewer workgroups than bins at max_groups = 7."""
    tab, ints, eps = hamiltonians(case, "coulomb")
    dens, T, lam = density_of(ints, eps, tab, False)
    q, neg, zero = sd.transfer_bins(tab)
    assert np.array_equal(q, dens.bins().q)
    Gref = sd.density(tab, T, lam)[1]
    Gabs = sd.density(tab, np.abs(T), np.abs(lam))[1]
    want = sd.transfer_sums(tab, Gref, q, families=("abcd",))
    scale = sd.transfer_sums(tab, Gabs, q, families=("abcd",))
    nan = lambda: ctx.array(np.full(len(q), np.nan))
    got = dens.pair_transfer(nan()).get()
    few, again = dens.pair_transfer(nan(), max_groups=7).get(), dens.pair_transfer(nan()).get()
    reached = scale > 0
    record(f"pair_transfer {case}: {len(q)} bins, {int(reached.sum())} reached, {tab.n_vv.sum()} rows, worst |d| / sum|terms| = "
           f"{(np.abs(got - want)[reached] / scale[reached]).max():.2e}")
    assert reached.any() and ((~reached).any() or case == (14, 5))        # (at (14,5) every bin is reached)
    assert (np.abs(got - want) <= 1e-13 * scale).all()
    assert (bits(got[~reached]) == 0).all()
    assert np.array_equal(bits(got), bits(few)) and np.array_equal(bits(got), bits(again))


# ---- expectation values ---------------------------------------------------------------------------------------------------------
def dense_operator(tab, W):
    """[n,n,n,n] from the families of a host dictionary, each element with its exchange partner W_qpsr."""
    out = np.zeros((tab.n,) * 4)
    for name in BLOCKS:
        p, q, r, s = tab.block_pqrs(name).T
        out[p, q, r, s] = W[name]
        out[q, p, s, r] = W[name]
    return out


@pytest.mark.parametrize("kind", ["coulomb", "tc"])
@pytest.mark.parametrize("cutoff", [2, 3])
def test_expectation_matches_the_dense_lagrangian(ctx, hamiltonians, cutoff, kind):
    """19 and 27 plane waves, CCD: L(eps_W, W) of the device against tests/_rdm2_reference.lagrangian (the oracle's energy and
    residuals on dense arrays) for the operator assembled from the sector families, within 1e-12 x the sum of |terms| of the
    restatement."""
    tab, ints, eps = hamiltonians((14, cutoff), kind)
    dens, T, lam = density_of(ints, eps, tab, False)
    W = host(ints)
    kin = np.random.default_rng(3).standard_normal(tab.n)
    eps_w = ints.hf_orbital_energies(kin)
    no, nv = tab.no, tab.nv
    z1 = np.zeros((nv, no))
    want = r2.lagrangian(no, np.diag(eps_w), dense_operator(tab, W), z1, tab.to_dense(T), z1, tab.to_dense(lam))
    got = dens.expectation(ints, one_body=kin)
    gamma, Gref = sd.density(tab, T, lam)
    scale = float(np.abs(gamma) @ np.abs(eps_w) + sum(np.abs(Gref[nm]) @ np.abs(W[nm]) for nm in BLOCKS))
    record(f"expectation c{cutoff} {kind}: device {got:.15e}, dense {want:.15e}, |d| = {abs(got - want):.2e}, sum|terms| {scale:.2e}")
    assert abs(got - want) <= 1e-12 * scale
    assert got == dens.expectation(ints, one_body=kin)
    bare = dens.expectation(ints, one_body=kin, mean_field=False)
    assert abs((got - bare) - float(gamma @ (eps_w - kin))) <= 1e-12 * scale


@pytest.mark.parametrize("is_dcd", [False, True], ids=["ccd", "dcd"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_transfer_sums_give_the_coulomb_expectation(ctx, hamiltonians, case, is_dcd):
    """The Coulomb integrals depend on the transfer alone, V_pqrs = v(k_r - k_p), so sum_q v(q) s(q) = L(0, V): the two bin
    kernels against the dots and the ladder product, also where nothing dense exists.  Within 1e-12 x the sum of |terms|:
    both sides add the same products, in trees of at most ~20 levels behind runs of at most a few thousand ascending adds.
    And s(0) = sum_i gamma_i, S2 even to the bit, S(0) = N."""
    tab, ints, eps = hamiltonians(case, "coulomb")
    dens, T, lam = density_of(ints, eps, tab, is_dcd)
    tb = dens.bins()
    W = host(ints)
    v, seen = np.zeros(tb.nbins), np.zeros(tb.nbins, dtype=bool)
    for name in BLOCKS:
        pqrs = tab.block_pqrs(name)
        b = tb.bin_of(tab.k_int[pqrs[:, 2]] - tab.k_int[pqrs[:, 0]])
        assert (b >= 0).all()
        v[b], seen[b] = W[name], True
        assert np.abs(W[name] - v[b]).max(initial=0.0) <= 1e-12 * np.abs(v).max()       # one value per bin
    assert np.abs(v - v[tb.neg])[seen & seen[tb.neg]].max() <= 1e-12 * np.abs(v).max()
    s, q = dens.transfer_sums(symmetrize=False)
    s2 = dens.transfer_sums()[0]
    want = dens.expectation(ints, mean_field=False)
    gamma, Gref = sd.density(tab, T, lam, is_dcd)
    scale = float(sum(np.abs(Gref[nm]) @ np.abs(W[nm]) for nm in BLOCKS))
    gscale = float(sum(np.abs(Gref[nm]).sum() for nm in BLOCKS))
    record(f"transfer {case} dcd={is_dcd}: sum v s = {v @ s:.15e}, L(0, V) = {want:.15e}, |d| = {abs(v @ s - want):.2e}, "
           f"sum|terms| {scale:.2e}; s(0) - sum_i gamma_i = {s[tb.zero] - gamma[:tab.no].sum():.2e}; "
           f"largest |s(q) - s(-q)| = {np.abs(s - s[tb.neg]).max():.2e}")
    assert abs(v @ s - want) <= 1e-12 * scale and abs(v @ s2 - want) <= 1e-12 * scale
    assert abs(s[tb.zero] - gamma[:tab.no].sum()) <= 1e-12 * gscale
    assert np.abs(s - sd.transfer_sums(tab, Gref, q)).max() <= 1e-11 * gscale
    assert np.array_equal(bits(s2), bits(s2[tb.neg]))
    S, qs = dens.structure_factor()
    assert np.array_equal(qs, tb.q) and np.array_equal(bits(S), bits(S[tb.neg])) and S[tb.zero] == 2 * tab.no
    want_S = sd.structure_factor(tab, gamma, sd.transfer_sums(tab, Gref, q), *sd.transfer_bins(tab))
    assert np.abs(S - want_S).max() <= 1e-11 * gscale / (2 * tab.no)
    avg, q2 = dens.structure_factor(shells=True)
    assert q2[0] == 0 and avg[0] == S[tb.zero] and len(avg) == len(q2) == len(np.unique((tb.q ** 2).sum(axis=1)))


# ---- whole solves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_dcd", [False, True], ids=["ccd", "dcd"])
def test_solve_with_densities(ctx, is_dcd):
    """N = 14, 27 plane waves, transcorrelated.  "density e" = L(eps, ints) = E(T) + <lam, R(T)> for the T and lam of the
    result, and "ccd e" = E(T): the two differ by <lam, R(T)>, at most |lam| |R(T)| (2-norms; R measured by
    ``get_residual``, lam as returned -- its own residual enters only the distance of either number from the converged
    energy), plus the rounding of L, 1e-12 x the sum of |terms| of the restatement."""
    from pymes_amd.solver.ueg_cc import SectorCCD, SectorDensity
    ref, eps, ints = tc_sector_problem(ctx, 3)
    tab, no = ints.tables, ints.tables.no
    plain = quiet(SectorCCD(no, delta_e=1e-12, is_dcd=is_dcd).solve, eps, ints, max_iter=100)
    got = quiet(SectorCCD(no, delta_e=1e-12, is_dcd=is_dcd).solve, eps, ints, max_iter=100, density=True,
                lambda_threshold=1e-10)
    assert sorted(got) == sorted(list(plain) + ["lambda2", "lambda residual", "density", "n(k)", "density e",
                                                "structure factor", "structure factor q"])
    assert got["ccd e"] == plain["ccd e"] and isinstance(got["density"], SectorDensity)
    T, lam = got["t2 amp"].get(), got["lambda2"].get()
    r = float(np.linalg.norm(SectorCCD(no, is_dcd=is_dcd).get_residual(eps, ints, T)))
    W = host(ints)
    gamma, Gref = sd.density(tab, T, lam, is_dcd)
    scale = float(np.abs(gamma) @ np.abs(eps) + sum(np.abs(Gref[nm]) @ np.abs(W[nm]) for nm in BLOCKS))
    bound = float(np.linalg.norm(lam)) * r + 1e-12 * scale
    diff = abs(got["density e"] - got["ccd e"])
    n_k, S, q = got["n(k)"], got["structure factor"], got["structure factor q"]
    tb = got["density"].bins()
    record(f"solve dcd={is_dcd}: ccd e {got['ccd e']:.12f}, density e {got['density e']:.12f}, |d| = {diff:.2e} (bound {bound:.2e}: "
           f"|lam| {np.linalg.norm(lam):.2e}, |R| {r:.1e}, |G| {got['lambda residual']:.1e}); tr n(k) - N = {n_k.sum() - 2 * no:.1e}; "
           f"n(k) at the Fermi surface {n_k[no - 1]:.6f} | {n_k[no]:.6f}; S on the first shells "
           + " ".join("%.6f" % x for x in got["density"].structure_factor(shells=True)[0][:4]))
    assert got["lambda residual"] <= 1e-10
    assert diff <= bound
    assert abs(n_k.sum() - 2 * no) <= 1e-13 * np.abs(n_k).sum()
    assert np.array_equal(q, tb.q) and np.array_equal(bits(S), bits(S[tb.neg]))


def test_hellmann_feynman_for_dcd(ctx):
    """DCD has no dense density to compare with.  ints(s) = only_2b + s effect_2b at N = 14, cutoff 3, eps held fixed:
    dE/ds at s = 1 is L(0, effect_2b) = expectation(effect_2b, mean_field=False) (the orbital energies do not move with s,
    so f_HF[effect_2b] stays out), against the Richardson-extrapolated central differences of
    tests/test_gpu_sector_lambda.py::test_lambda_gives_the_derivative_of_the_energy: h = 0.2, tolerance ten times the
    difference of the (h, 2h) and the (2h, 4h) extrapolation."""
    from pymes_amd.solver.ueg_cc import SectorCCD, SectorLambda, sector_density
    ref = G["tc_N14_rs1.0_c3"]
    m = model(ref["nel"], 3, ref["rs"], k_cutoff=ref["k_cutoff"])
    tab = m.sector_tables()
    v2 = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_only_2b=True, ctx=ctx)
    eff = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_effect_2b=True, ctx=ctx)
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    eps = v2.hf_orbital_energies(kin) + quiet(m.double_contractions_in_3_body)
    no, h = tab.no, 0.2

    def energy(s):
        return quiet(SectorCCD(no, delta_e=1e-14, is_dcd=True).solve, eps, v2 + s * eff, max_iter=150)
    T = energy(1.0)["t2 amp"]
    lam = quiet(SectorLambda(no, 1e-12, is_dcd=True).solve, eps, v2 + eff, T, max_iter=200)
    assert lam["converged"]
    dens = sector_density(eps, v2 + eff, T, lam["lambda2"], is_dcd=True)
    analytic = dens.expectation(eff, mean_field=False)
    D = {k: (energy(1.0 + k * h)["ccd e"] - energy(1.0 - k * h)["ccd e"]) / (2.0 * k * h) for k in (1, 2, 4)}
    r1, r2_ = (4.0 * D[1] - D[2]) / 3.0, (4.0 * D[2] - D[4]) / 3.0
    tol = 10.0 * abs(r1 - r2_)
    record(f"hellmann-feynman dcd: expectation(effect_2b) {analytic:.12e}, Richardson (h,2h) {r1:.12e}, (2h,4h) {r2_:.12e}, "
           f"|analytic - (h,2h)| = {abs(analytic - r1):.2e}, tolerance {tol:.2e}")
    assert abs(analytic - r1) <= tol


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, hamiltonians):
    from pymes_amd.device import Context
    from pymes_amd.solver.ueg_cc import sector_density
    tab, ints, eps = hamiltonians((14, 2), "coulomb")
    other_tab, other, _ = hamiltonians((14, 5), "coulomb")
    T, lam = seeded(tab)
    with pytest.raises(TypeError, match="sector_density: ints must be SectorIntegrals"):
        sector_density(eps, host(ints), T, lam)
    with pytest.raises(ValueError, match="the tables of the amplitudes do not match the integrals"):
        sector_density(eps, ints, symmetric(other_tab, 1), lam)
    dense = tab.to_dense(T)
    dense[0, 0, 0, 1] = 1.0
    with pytest.raises(ValueError, match="weight outside the momentum-conserving support"):
        sector_density(eps, ints, dense, lam)
    skew = np.random.default_rng(1).standard_normal(tab.nnz)
    with pytest.raises(ValueError, match="sector_density: the amplitudes are not exchange-symmetric"):
        sector_density(eps, ints, skew, lam)
    with pytest.raises(ValueError, match="sector_density: lambda is not exchange-symmetric"):
        sector_density(eps, ints, T, skew)
    f = np.diag(eps)
    f[0, 1] = 1e-3
    with pytest.raises(ValueError, match="sector_density: the Fock matrix must be diagonal"):
        sector_density(f, ints, T, lam)
    with pytest.raises(ValueError, match="sector_density: 3 orbital energies for"):
        sector_density(eps[:3], ints, T, lam)
    dens = sector_density(np.diag(eps), ints, T, lam)
    with pytest.raises(TypeError, match="SectorDensity.expectation: W must be SectorIntegrals"):
        dens.expectation(host(ints))
    with pytest.raises(ValueError, match="SectorDensity.expectation: W belongs to other tables or another context"):
        dens.expectation(other)
    c2 = Context(1, 1, lib=ctx.lib)
    try:
        from pymes_amd.solver.ueg_cc import SectorIntegrals
        with pytest.raises(ValueError, match="W belongs to other tables or another context"):
            dens.expectation(SectorIntegrals(c2, tab))
    finally:
        c2.close()
    bad = ints * 1.0
    w1 = bad["w1"].get()
    w1[0] += 1.0
    bad["w1"].set(w1)
    with pytest.raises(ValueError, match=r"W is not symmetric under the exchange of the two electrons \(W_pqrs = W_qpsr\)"):
        dens.expectation(bad)
    with pytest.raises(ValueError, match="one number per orbital is needed"):
        dens.expectation(ints, one_body=np.zeros(3))
    ctx.graph_begin()
    try:
        with pytest.raises(RuntimeError, match="sector_density: the context is recording a launch graph"):
            sector_density(eps, ints, T, lam)
        with pytest.raises(RuntimeError, match="SectorDensity.transfer_sums: the context is recording a launch graph"):
            dens.transfer_sums()
    finally:
        ctx.graph_abort()
    assert dens.expectation(ints) != 0.0                                          # the context is usable afterwards
    x = ctx.zeros((8,))
    p = C.c_void_p(x.ptr)
    with pytest.raises(_lib.PymesError, match="sector_bin_sums: null argument"):
        ctx.lib.call("pymes_sector_bin_sums", ctx.handle, p, 1, None, p, p, 1.0, 0.0)
    with pytest.raises(_lib.PymesError, match="sector_pair_transfer: bad orbital counts"):
        ctx.lib.call("pymes_sector_pair_transfer", ctx.handle, p, 1, p, p, p, p, 0, 1, 1, p, p, p, p, p, p, 0)
    with pytest.raises(_lib.PymesError, match="sector_gamma: null argument"):
        ctx.lib.call("pymes_sector_gamma", ctx.handle, p, p, 1, 1, p, p, p, None, p)
