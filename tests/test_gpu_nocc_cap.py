"""GPU: the kernels that stage one nocc x (nocc + 1) tile of doubles in LDS, up to the cap on nocc and past it
(include/pymes_amd.h, PYMES_NOCC_MAX_FUSED = 90 / PYMES_NOCC_MAX_LAMBDA = 88; csrc/kernels.hip: t2_layouts (both template
forms), t2_layouts_sym, residual_assemble, residual_assemble_pairs, cc_update_sym, lincomb_sym; csrc/kernels_post.hip: lambda_assemble).  The sibling
modules stop at nocc = 32 (test_gpu_sym_tail.py), 23 for Lambda and 40 for IP / EA (test_gpu_loop_edges.py); whole solves reach 50.

Shapes (no, nv), nvirt tiny so that every array is at most 9 x 8100 doubles:
  (64,2)  LDS pitch 65, exactly 16 trips of the 256-thread tile loops, even nocc (16-byte forms)
  (65,3)  a ragged 17th trip, odd nocc (scalar forms), three b per a
  (78,2)  the first tile above 48 KB
  (88,2)  the last nocc the Lambda assembly admits
  (89,2)  odd, below the cap, the first nocc the Lambda assembly refuses
  (90,3)  the cap: 65 520 B of dynamic LDS (65 552 B with the 32 static bytes of the phase union kernel)
  (90,1)  the cap with one diagonal pair only

1. every entry point at every shape, as a launch (``forced``) and as a recorded phase task (default switches, checked through
   ``phase_stats``), against numpy;  2. the boundary: the predicates and the refusals by name, without a leaked allocation;
3. the engine at (90,2) — fused — and (91,2) — permutes, ladder_sym_unpack, assembly in separate passes — against the oracles,
   phases on and off, with the branch that ran asserted.  Integrals come from eight density-fitting factors.
3b. the sigma build's other branches on the same two contexts (tests/_eom_branch_cases.py): a symmetric vector — at 91 the packed
   build that is not fused —, a handle over an unsymmetric T2 (t_sym = hole_sym = 0) with a symmetric and a general vector, two
   symmetric vectors at 91 (vector by vector); the left build on an unsymmetric T2 at (88,2), the last nocc it admits."""
import contextlib
import functools
import os
import re
import tempfile

import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle import eom_oracle as eo
from oracle import slab_oracle as so
from oracle.cases import synthetic_factors
from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _eom_branch_cases as BC
from tests import test_gpu_loop_edges as LE
from tests import test_gpu_sym_tail as ST
from tests.test_gpu_sym_tail import env, forced, grid_energies, sym4
from tests.test_gpu_transitions import _live

pytestmark = pytest.mark.gpu
SHAPES = [(64, 2), (65, 3), (78, 2), (88, 2), (89, 2), (90, 3), (90, 1)]
LAMBDA_SHAPES = [(64, 2), (65, 3), (88, 2)]
ROUTES = ["launch", "task"]
EPS = 2.0 ** -53
E = _lib.PymesError
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pymes_amd.h")


def limit(name):
    return int(re.search(r"#define %s (\d+)" % name, open(HEADER).read()).group(1))


def tasks(ctx):
    """The default switches: phases on, calls below 60 us are recorded as tasks of a phase."""
    return env(ctx, PYMES_PHASE=None, PYMES_PHASE_MAX_US=None, PYMES_SYM_TAIL=None)


class route:
    """``with route(ctx, how):`` — "launch": nothing is small enough to be a task; "task": the default switches, and the block
    must have recorded at least one task (it would otherwise have turned into the launch route unnoticed)."""

    def __init__(self, ctx, how):
        self.ctx, self.how = ctx, how
        self.cm = forced(ctx) if how == "launch" else tasks(ctx)

    def __enter__(self):
        self.cm.__enter__()
        self.before = self.ctx.phase_stats()["tasks"]
        return self

    def __exit__(self, *exc):
        recorded = self.ctx.phase_stats()["tasks"] - self.before
        self.cm.__exit__(*exc)
        if exc[0] is None:
            assert (recorded > 0) == (self.how == "task"), (self.how, recorded)
        return False


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def case(request, gpu_lib):
    no, nv = request.param
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=1 << 24)
    assert ctx.sym_tail() and ctx.pairs_supported()
    yield ctx, no, nv
    ctx.close()


def unrank(P):
    a = int((np.sqrt(8.0 * P + 1.0) - 1.0) / 2.0)
    while a * (a + 1) // 2 > P:
        a -= 1
    while (a + 1) * (a + 2) // 2 <= P:
        a += 1
    return a, P - a * (a + 1) // 2


def chunk_of(nv, rank, world):
    """(first pair, one past the last pair, rows of a rank's compact buffer): Engine::pair_chunk."""
    npp = nv * (nv + 1) // 2
    c = -(-npp // world)
    r0 = min(rank * c, npp)
    return r0, min(r0 + c, npp), c


# ---- 1a. the pair layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ROUTES)
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "sym"])
@pytest.mark.parametrize("with_td", [True, False], ids=["Td", "noTd"])
def test_pair_layouts(case, how, sym, with_td):
    """Td / Tx are copies: bit for bit; Ttd = 2 x - y is one rounding of an exact product, the same in numpy: bit for bit
    (the rule of test_gpu_sym_tail.test_layouts_bitwise).  The plain entry gets an array WITHOUT the exchange symmetry."""
    ctx, no, nv = case
    rng = np.random.default_rng(1000 * no + 10 * nv + sym)
    T = sym4(rng, no, nv) if sym else rng.standard_normal((nv, nv, no, no))
    ov = no * nv
    nan = lambda: ctx.array(np.full((ov, ov), np.nan))
    Xd, Xx, Xt = (nan() if with_td else None), nan(), nan()
    with route(ctx, how):
        ctx.pair_layouts(ctx.array(T), Xx, Xt, Xd, sym=sym)
        got = (Xd.get() if with_td else None), Xx.get(), Xt.get()
    Td = T.transpose(0, 2, 1, 3).reshape(ov, ov)
    if with_td:
        assert np.array_equal(got[0], Td)
    assert np.array_equal(got[1], T.transpose(0, 3, 1, 2).reshape(ov, ov))
    assert np.array_equal(got[2], 2.0 * Td - T.transpose(1, 2, 0, 3).reshape(ov, ov))


# ---- 1b. the symmetrised assembly ----------------------------------------------------------------------------------------------------------
def assemble_reference(no, nv, N, D, X, V, L, N_terms=None):
    """The sum of csrc/kernels.hip's comment on residual_assemble in extended precision, and the sum of the magnitudes of its
    terms: S_ij = N_ab[i][j] + N_ba[j][i] + D[(a,i),(b,j)] + D[(b,j),(a,i)] + X[(a,j),(b,i)] + X[(b,i),(a,j)],
    R_ab = V_ab + unpack(L)_ab + S.  L[P(a,b)] holds o (o + 1) / 2 symmetric entries [P(max, min)] and, behind them,
    o (o - 1) / 2 antisymmetric ones that enter with the sign of i - j for a > b (the pair (b,a) sees them at (j,i)) and are
    skipped for a == b and i == j.  ``N_terms``: what stands for N_ab[i][j] + N_ba[j][i], term by term (the pair-sharded tail)."""
    ld = np.longdouble
    D4, X4 = D.reshape(nv, no, nv, no), X.reshape(nv, no, nv, no)
    terms = list(N_terms) if N_terms is not None else [N, N.transpose(1, 0, 3, 2)]
    terms += [D4.transpose(0, 2, 1, 3), D4.transpose(2, 0, 3, 1), X4.transpose(0, 2, 3, 1), X4.transpose(2, 0, 1, 3)]
    if V is not None:
        terms.append(V)
    if L is not None:
        opp = no * (no + 1) // 2
        i, j = np.indices((no, no))
        ih, il = np.maximum(i, j), np.minimum(i, j)
        Ls, La = np.zeros((nv, nv, no, no)), np.zeros((nv, nv, no, no))
        for a in range(nv):
            for b in range(a + 1):
                row = L[a * (a + 1) // 2 + b]
                Ls[a, b] = Ls[b, a] = row[ih * (ih + 1) // 2 + il]
                if a != b:
                    anti = np.where(i != j, row[opp + np.where(i != j, ih * (ih - 1) // 2 + il, 0)], 0.0)
                    La[a, b] = np.sign(i - j) * anti
                    La[b, a] = -np.sign(i - j) * anti
        terms += [Ls, La]
    ref, mag = np.zeros((nv, nv, no, no), dtype=ld), np.zeros((nv, nv, no, no), dtype=ld)
    for t in terms:
        ref += t.astype(ld)
        mag += np.abs(t).astype(ld)
    return ref, mag


@pytest.mark.parametrize("how", ROUTES)
@pytest.mark.parametrize("with_vl", [True, False], ids=["V+L", "bare"])
def test_symmetrised_assemble(case, how, with_vl):
    """At most 9 terms per element, added in double precision in some order: |error| <= 9 * 2^-53 * sum |terms| against the
    sum in extended precision (whose own rounding is 2^-11 of that)."""
    ctx, no, nv = case
    rng = np.random.default_rng(2000 * no + 10 * nv + with_vl)
    ov, npp = no * nv, nv * (nv + 1) // 2
    N, D, X = rng.standard_normal((nv, nv, no, no)), rng.standard_normal((ov, ov)), rng.standard_normal((ov, ov))
    V = rng.standard_normal((nv, nv, no, no)) if with_vl else None
    L = rng.standard_normal((npp, no * no)) if with_vl else None
    out = ctx.array(np.full(N.shape, np.nan))
    dev = lambda x: None if x is None else ctx.array(x)
    with route(ctx, how):
        ctx.symmetrised_assemble(ctx.array(N), ctx.array(D), ctx.array(X), out, V=dev(V), L=dev(L))
        got = out.get()
    ref, mag = assemble_reference(no, nv, N, D, X, V, L)
    err = np.abs(got.astype(np.longdouble) - ref)
    print("assemble", (no, nv), how, with_vl, "max error / bound", float((err / (9 * EPS * mag)).max()))
    assert np.all(np.isfinite(got))
    assert np.all(err <= 9 * EPS * mag)


# ---- 1c. the read-once amplitude tail: the checks of test_gpu_sym_tail.py at these shapes ------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True])
def test_update_bitwise(case, inplace):
    ST.test_update_bitwise(case, inplace)


def test_update_arbitrary_energies(case):
    ST.test_update_arbitrary_energies(case)


@pytest.mark.parametrize("m", [1, 6])
def test_lincomb_bitwise(case, m):
    ST.test_lincomb_bitwise(case, m)


def test_layouts_bitwise(case):
    ST.test_layouts_bitwise(case)


@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("with_t1", [False, True])
def test_dots(case, m, with_t1):
    ST.test_dots(case, m, with_t1)


def set_ijab_block(ctx, no, nv, seed):
    """The block the energy pass reads, alone, with V_ijab == V_jiba bit for bit."""
    x = np.random.default_rng(seed).standard_normal((no, no, nv, nv)) * 0.1
    Vijab = np.ascontiguousarray(x + x.transpose(1, 0, 3, 2))
    ctx.set_V_block("ijab", Vijab)
    return Vijab


@pytest.mark.parametrize("with_t1", [False, True])
@pytest.mark.parametrize("with_dt2", [False, True])
def test_energy_norms(case, with_t1, with_dt2):
    ST.check_energy_norms(case, with_t1, with_dt2, set_V=set_ijab_block)


def test_guard_never_inferred_from_the_shape(case):
    ST.test_guard_never_inferred_from_the_shape(case)


def test_tail_as_tasks(case):
    """The declaring calls under the default switches: every call is small at these sizes, so it is recorded as a task and keeps
    the full-read form — the bits of the launched read-once forms (grid energies, see grid_energies)."""
    ctx, no, nv = case
    rng = np.random.default_rng(3000 * no + nv)
    eo_, ev_ = grid_energies(rng, no, nv)
    ctx.set_orbital_energies(eo_, ev_)
    Vijab = set_ijab_block(ctx, no, nv, 31 * no + nv)
    R, T = sym4(rng, no, nv), sym4(rng, no, nv)
    X, c = [sym4(rng, no, nv) for _ in range(6)], rng.standard_normal(6)

    def run():
        dO, dD, mix = ctx.empty(T.shape), ctx.empty(T.shape), ctx.empty(T.shape)
        ctx.cc_update_to(dO, dD, ctx.array(T), ctx.array(R), level_shift=0.25, delta=0.75, sym=True)
        ctx.lincomb(mix, [ctx.array(x) for x in X], c, sym=True)
        d = ctx.dots([dO, dD], [dD, dD], sym=[True, True])
        return dO.get(), dD.get(), mix.get(), d, np.array(ctx.energy_norms(None, None, dO, dD, sym=True))
    with route(ctx, "task"):
        as_task = run()
    with forced(ctx):                    # (the second stage of the overlaps is a task whenever phases are on: ``route`` would object)
        launched = run()
    for a, b in zip(as_task[:3], launched[:3]):
        assert np.array_equal(a, b)
    t_new, d_new = launched[0], launched[1]
    bound = 2 * T.size * EPS * np.array([np.abs(t_new * d_new).sum(), (d_new * d_new).sum()])
    assert np.all(np.abs(as_task[3] - launched[3]) <= bound)
    # the energy pass (no T1) over the updated amplitudes: both routes against numpy, the bound of test_gpu_sym_tail.test_energy_norms
    Edir, Eex = Vijab.transpose(2, 3, 0, 1), Vijab.transpose(3, 2, 0, 1)
    ref = np.array([0.0, 2.0 * (t_new * Edir).sum(), -(t_new * Eex).sum(), (t_new * t_new).sum(), (d_new * d_new).sum(), 0.0])
    ebound = 2 * T.size * EPS * np.array([0.0, 2.0 * np.abs(t_new * Edir).sum(), np.abs(t_new * Eex).sum(), (t_new * t_new).sum(),
                                          (d_new * d_new).sum(), 0.0])
    for got in (as_task[4], launched[4]):
        assert np.all(np.abs(got - ref) <= ebound)


# ---- 1d. the pair-sharded tail on compact tiles -----------------------------------------------------------------------------------------------
def compact(X, no, nv, rank, world):
    """Xc[P - r0][2][o*o] of a rank (csrc/kernels.hip): tile 0 = X[a,b], tile 1 = X[b,a], zero for a == b; rows past the rank's
    last pair stay as they are (NaN here)."""
    r0, r1, c = chunk_of(nv, rank, world)
    out = np.full((c, 2, no * no), np.nan, dtype=X.dtype)
    for P in range(r0, r1):
        a, b = unrank(P)
        out[P - r0, 0] = X[a, b].ravel()
        out[P - r0, 1] = X[b, a].ravel() if a != b else 0.0
    return out


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_pairs_pack_update_energy_unpack(case, rank, world):
    """pairs_pack, cc_update_pairs, energy_norms_pairs and pairs_unpack of one rank against numpy on its pairs.  Copies: bit for
    bit.  The update on grid energies (every denominator exact): dt bit for bit as r * (1 / d); t + delta dt may or may not be
    contracted into one fused operation: two roundings of at most 2^-53 (|t| + |delta dt|) apart.  The sums: 2 n 2^-53 sum |x y|
    (test_gpu_sym_tail.test_energy_norms)."""
    ctx, no, nv = case
    rng = np.random.default_rng(4000 * no + 10 * nv + world)
    r0, r1, c = chunk_of(nv, rank, world)
    eo_, ev_ = grid_energies(rng, no, nv)
    ctx.set_orbital_energies(eo_, ev_)
    Vijab = set_ijab_block(ctx, no, nv, 29 * no + nv)
    T, R = rng.standard_normal((nv, nv, no, no)), rng.standard_normal((nv, nv, no, no))      # no symmetry: tile 1 is its own data
    f, t1 = rng.standard_normal((no + nv, no + nv)), rng.standard_normal((nv, no))
    nan = lambda: ctx.array(np.full((c, 2, no * no), np.nan))
    tc, rc, dtc = nan(), nan(), nan()
    ctx.pairs_pack(ctx.array(T), tc, rank, world)
    ctx.pairs_pack(ctx.array(R), rc, rank, world)
    Tc, Rc = compact(T, no, nv, rank, world), compact(R, no, nv, rank, world)
    assert np.array_equal(tc.get(), Tc, equal_nan=True) and np.array_equal(rc.get(), Rc, equal_nan=True)
    # the update
    shift, delta = 0.25, 0.75
    ctx.cc_update_pairs(tc, dtc, rc, shift, delta, rank, world)
    Dt, Tn = np.full(Tc.shape, np.nan), np.full(Tc.shape, np.nan)
    for P in range(r0, r1):
        a, b = unrank(P)
        d = (eo_[:, None] + eo_[None, :] - (ev_[a] + ev_[b]) + shift).ravel()
        Dt[P - r0] = Rc[P - r0] * (1.0 / d)[None, :]
        Tn[P - r0] = Tc[P - r0] + delta * Dt[P - r0]
    got_dt, got_t = dtc.get(), tc.get()
    assert np.array_equal(got_dt, Dt, equal_nan=True)
    live = np.isfinite(Tn)
    assert np.array_equal(np.isfinite(got_t), live)
    assert np.all(np.abs(got_t[live] - Tn[live]) <= 2 * EPS * (np.abs(Tc[live]) + np.abs(delta * Dt[live])))
    # the energy pass of this rank over (t, dt) as they are now
    for with_t1 in (False, True):
        got = ctx.energy_norms_pairs(ctx.array(f) if with_t1 else None, ctx.array(t1) if with_t1 else None, tc, dtc, rank, world)
        ref, mag = np.zeros(6), np.zeros(6)
        for P in range(r0, r1):
            a, b = unrank(P)
            for half, (x, y) in enumerate(((a, b), (b, a))[:1 if a == b else 2]):
                t, dt = got_t[P - r0, half].reshape(no, no), got_dt[P - r0, half].reshape(no, no)
                tau = t + (np.outer(t1[x], t1[y]) if with_t1 else 0.0)
                ed, ex = Vijab[:, :, x, y], Vijab[:, :, y, x]
                ref[1:5] += [2.0 * (tau * ed).sum(), -(tau * ex).sum(), (t * t).sum(), (dt * dt).sum()]
                mag[1:5] += [2.0 * np.abs(tau * ed).sum(), np.abs(tau * ex).sum(), (t * t).sum(), (dt * dt).sum()]
        if with_t1 and rank == 0:                              # the T1 sums enter on rank 0
            ref[[0, 5]] = [2.0 * (f[:no, no:].T * t1).sum(), (t1 * t1).sum()]
            mag[[0, 5]] = [2.0 * np.abs(f[:no, no:].T * t1).sum(), (t1 * t1).sum()]
        bound = 2 * max(1, r1 - r0) * 2 * no * no * EPS * mag
        bound[[0, 5]] = 2 * t1.size * EPS * mag[[0, 5]]
        print("pairs energy", (no, nv), (rank, world), with_t1, np.abs(got - ref), bound)
        assert np.all(np.abs(got - ref) <= bound)
    # every rank's chunk back into a full array: this rank's updated tiles, the other ranks' tiles as packed from T
    parts = np.concatenate([got_t if w == rank else compact(T, no, nv, w, world) for w in range(world)])
    full = ctx.array(np.full(T.shape, np.nan))
    ctx.pairs_unpack(ctx.array(np.nan_to_num(parts, nan=-7.0)), full, world)      # (the rows past a rank's last pair are never read)
    back = full.get()
    want = T.copy()
    for P in range(r0, r1):
        a, b = unrank(P)
        want[a, b] = got_t[P - r0, 0].reshape(no, no)
        if a != b:
            want[b, a] = got_t[P - r0, 1].reshape(no, no)
    assert np.array_equal(back, want)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_residual_assemble_pairs(case, rank, world):
    """residual_assemble_pairs through residual_finish_pairs with X_ac handed in (``Xvv=``) and no T1: the only integral read is
    the block V_abij, ETd / ETx / L are whatever the caller says (random here), and what stands for N_ab + N_ba^T is
    N'_ab[i][j] = sum_c X_ac T_cbij + X_bc T_caji, formed by the engine for the rows a of the rank's pairs.  Per element that is
    V, two ladder entries, four pair-matrix entries and 2 nv products: n = 7 + 2 nv terms (9, 11, 13 for nv = 1, 2, 3), each
    product rounded once at most and n - 1 additions, so |error| <= n * 2^-53 * sum |terms| against the sum in extended
    precision — the rule of test_symmetrised_assemble.  T carries no exchange symmetry; rows of the compact buffer past the
    rank's last pair stay untouched, tile 1 of a diagonal pair is zero."""
    ctx, no, nv = case
    rng = np.random.default_rng(5000 * no + 10 * nv + world)
    ov, npp, n = no * nv, nv * (nv + 1) // 2, no + nv
    r0, r1, c = chunk_of(nv, rank, world)
    T, V = rng.standard_normal((nv, nv, no, no)), rng.standard_normal((nv, nv, no, no))
    D, X, L = rng.standard_normal((ov, ov)), rng.standard_normal((ov, ov)), rng.standard_normal((npp, no * no))
    Xvv = rng.standard_normal((nv, nv))
    ctx.set_V_block("abij", V)
    Rc = ctx.array(np.full((c, 2, no * no), np.nan))
    ctx.residual_finish_pairs(ctx.array(rng.standard_normal((n, n))), ctx.array(T), ctx.array(D), ctx.array(X), ctx.array(L), Rc,
                              rank, world, Xvv=ctx.array(Xvv))
    got = Rc.get()
    ld = np.longdouble
    N_terms = []
    for cc in range(nv):
        t = Xvv[:, cc].astype(ld)[:, None, None, None] * T[cc].astype(ld)[None, :, :, :]        # X_ac T_cbij
        N_terms += [t, t.transpose(1, 0, 3, 2)]                                                 # ... and X_bc T_caji
    ref, mag = assemble_reference(no, nv, None, D, X, V, L, N_terms=N_terms)
    want, wmag = compact(ref, no, nv, rank, world), compact(mag, no, nv, rank, world)
    live = np.isfinite(want.astype(np.float64))
    assert np.array_equal(np.isfinite(got), live)
    if r1 > r0:
        nterms = 7 + 2 * nv
        err = np.abs(got[live].astype(ld) - want[live])
        print("pairs assemble", (no, nv), (rank, world), "max error / bound", float((err / np.maximum(nterms * EPS * wmag[live], 1e-300)).max()))
        assert np.all(err <= nterms * EPS * wmag[live])
        for P in range(r0, r1):
            if unrank(P)[0] == unrank(P)[1]:
                assert np.all(got[P - r0, 1] == 0.0)


# ---- 1e. the Lambda assembly: the route of test_gpu_loop_edges.py ---------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", LAMBDA_SHAPES)
def test_lambda_left_apply(gpu_lib, no, nv):
    before = _live()
    LE.test_lambda_left_apply_past_one_trip(gpu_lib, no, nv, False)
    assert _live() == before


@pytest.mark.parametrize("no,nv", LAMBDA_SHAPES)
def test_lambda_step(gpu_lib, no, nv):
    """The update branch and the lambda_norm result."""
    LE.test_lambda_step_past_one_trip(gpu_lib, no, nv)


# ---- 2. the boundary ---------------------------------------------------------------------------------------------------------------------
def test_limits_are_stated_once():
    cap, lam, bra = limit("PYMES_NOCC_MAX_FUSED"), limit("PYMES_NOCC_MAX_LAMBDA"), limit("PYMES_NOCC_MAX_BRA_DRESS")
    assert 8 * cap * (cap + 1) <= 65536 < 8 * (cap + 1) * (cap + 2)
    assert 8 * (lam * (lam + 1) + 256) <= 65536 < 8 * ((lam + 1) * (lam + 2) + 256)
    assert (cap, lam, bra) == (90, 88, 80)
    from pymes_amd.solver import lambda_ccsd
    assert lambda_ccsd.NOCC_MAX == lam


def test_bra_dressing_refuses_past_its_limit(gpu_lib):
    """The library's own decision against the header's PYMES_NOCC_MAX_BRA_DRESS (the fused and Lambda limits are met through the
    library in the tests around this one): refused by name at the limit + 1, before an operand is looked at."""
    bra = limit("PYMES_NOCC_MAX_BRA_DRESS")
    ctx = Context(bra + 1, 1, lib=gpu_lib, workspace_bytes=1 << 24)
    try:
        x, t1 = ctx.zeros((16, 16)), ctx.zeros((1, bra + 1))
        with pytest.raises(E, match="ladder_dress: nocc outside 1..%d" % bra):
            ctx.ladder_dress(x, x, t1, x, 16, 0, 1)
    finally:
        ctx.close()


def test_predicates_at_the_cap(gpu_lib):
    cap = limit("PYMES_NOCC_MAX_FUSED")
    for no, want in ((cap, True), (cap + 1, False)):
        ctx = Context(no, 1, lib=gpu_lib, workspace_bytes=1 << 24)
        try:
            assert ctx.sym_tail() == want and ctx.pairs_supported() == want
        finally:
            ctx.close()


@pytest.mark.parametrize("how", ROUTES)
def test_fused_entries_refuse_by_name_past_the_cap(gpu_lib, how):
    no, nv = limit("PYMES_NOCC_MAX_FUSED") + 1, 1
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=1 << 24)
    try:
        ov, npp, o2 = no * nv, nv * (nv + 1) // 2, no * no
        T, A, B_ = ctx.zeros((nv, nv, no, no)), ctx.zeros((ov, ov)), ctx.zeros((ov, ov))
        L, Rc, f, out = ctx.zeros((npp, o2)), ctx.zeros((npp, 2, o2)), ctx.zeros((no + nv, no + nv)), ctx.zeros((nv, nv, no, no))
        held = _live()
        with (forced(ctx) if how == "launch" else tasks(ctx)):
            for sym in (False, True):
                with pytest.raises(E, match="pair_layouts: nocc too large for the LDS tile"):
                    ctx.pair_layouts(T, A, B_, sym=sym)
            with pytest.raises(E, match="symmetrised_assemble: nocc too large for the LDS tile"):
                ctx.symmetrised_assemble(T, A, B_, out)
            with pytest.raises(E, match="residual_finish_pairs: nocc too large for the fused assembly"):
                ctx.residual_finish_pairs(f, T, A, B_, L, Rc, 0, 1)
        assert _live() == held
    finally:
        ctx.close()


@pytest.mark.parametrize("no", [89, 90])
def test_lambda_assemble_refuses_by_name(gpu_lib, no):
    """The library, on a handle whose sigma build is hoisted (zero integrals): both entries of the left assembly refuse at their
    head — nothing allocated, nothing left behind — and the right build on the same handle still runs."""
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    nv = 1
    assert no > limit("PYMES_NOCC_MAX_LAMBDA")
    ctx = Context(no, nv, lib=gpu_lib)
    try:
        for name in LeftSigma.BLOCKS:
            ctx.set_V_block(name, np.zeros(ctx.block_shape(name)))
        f = np.diag(np.concatenate([-1.0 - np.arange(no) / no, [1.0]]))
        sig = LeftSigma(ctx, f, ctx.zeros((nv, nv, no, no)))
        assert sig.fused_ok
        l1, l2 = ctx.zeros((nv, no)), ctx.zeros((nv, nv, no, no))
        o1, o2, e1, e2 = ctx.empty(l1.shape), ctx.empty(l2.shape), ctx.empty(l1.shape), ctx.empty(l2.shape)
        eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
        held = _live()
        with pytest.raises(E, match="lambda_assemble: nocc = %d is too large for the LDS tile" % no):
            sig.apply_left_many([l1], [l2], out1=[o1], out2=[o2])
        with pytest.raises(E, match="lambda_assemble: nocc = %d is too large for the LDS tile" % no):
            sig.lambda_step((l1, l2), eps_o, eps_v, 0.0, (o1, o2), (e1, e2), sym=True)
        with pytest.raises(E, match="lambda_assemble: nocc = %d is too large for the LDS tile" % no):
            sig.lambda_step(None, eps_o, eps_v, 0.0, (o1, o2), (e1, e2), start=True)
        assert _live() == held
        s1, s2 = sig.apply(l1, l2)
        assert np.all(s1.get() == 0.0) and np.all(s2.get() == 0.0)
        sig.close()
    finally:
        ctx.close()


def test_left_solvers_refuse_before_they_allocate(gpu_lib):
    """A Lambda or left-vector solve at nocc = 89: refused by the driver before a context, a handle or a vector exists — the
    integrals are never looked at (an empty dictionary), the allocation count does not move."""
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    no = 89
    f, t2, t1 = np.zeros((no + 1, no + 1)), np.zeros((1, 1, no, no)), np.zeros((1, no))
    before = _live()
    with pytest.raises(E, match="Lambda_CCSD: nocc = 89 is too large for the LDS tile"):
        Lambda_CCSD(no).solve(f, {}, t2)
    with pytest.raises(E, match="Lambda_CCSD: nocc = 89 is too large for the LDS tile"):
        Lambda_CCSD(no).apply_left(f, {}, t2, t1, t2)
    with pytest.raises(E, match="EOM_CCSD_Transitions: nocc = 89 is too large for the LDS tile"):
        EOM_CCSD_Transitions(no).solve(f, {}, t2, t1)
    with pytest.raises(E, match="Lambda_CCSD: nocc = 89 is too large for the LDS tile"):
        CCSD(no).solve(f, None, density=True)
    from pymes_amd.solver.eom_dyson import EA_EOM_CCSD_Dyson, IP_EOM_CCSD_Dyson
    for cls in (IP_EOM_CCSD_Dyson, EA_EOM_CCSD_Dyson):          # (no ``lam``: the Lambda equations would be solved inside)
        with pytest.raises(E, match="nocc = 89 is too large for the LDS tile"):
            cls(no, n_roots=1).solve(f, {}, t2, t1)
    assert _live() == before


# ---- 3. the engine on both sides of the cap, against the oracles ---------------------------------------------------------------------------
NAUX = 8
TOL = 1e-12          # test_gpu_cc.py: R1 at TOL, R2 at 10 TOL, of max(1, max |reference|) (test_pair_packed_ladder's scaling)
PHASES = [None, "0"]
PHASE_IDS = ["phases", "PYMES_PHASE=0"]


@functools.lru_cache(maxsize=None)
def engine_inputs(no, nv):
    """Factors (the host never holds more than the blocks the oracles read), a non-diagonal Fock matrix, non-zero T1,
    exchange-symmetric T2, a trial vector whose doubles have NO exchange symmetry; the oracles' R1, R2 and sigma, once."""
    B, eps = synthetic_factors(no, nv, seed=no, scale=0.3, gap=3.0)
    B = np.ascontiguousarray(B[:NAUX])
    rng = np.random.default_rng(5 * no + nv)
    n = no + nv
    f = np.diag(eps) + 0.02 * rng.standard_normal((n, n))
    t1 = 0.05 * rng.standard_normal((nv, no))
    x = 0.05 * rng.standard_normal((nv, nv, no, no))
    t2 = np.ascontiguousarray(0.5 * (x + x.transpose(1, 0, 3, 2)))
    u1, u2 = rng.standard_normal((nv, no)), rng.standard_normal((nv, nv, no, no))
    fd = oc.dressed_fock(no, f, t1, so.fock_blocks(no, B))
    r1 = oc.singles_residual(no, fd, t1, t2, so.singles_blocks(no, B))
    r2 = so.residual_slab(no, fd, t1, t2, B, 0, nv)
    Vu = so.FactorBlocks(no, B)
    from pymes_amd.solver.eom_ccsd import _Sigma
    Vb = {k: Vu(k) for k in _Sigma.BLOCKS}
    s1, s2 = eo.sigma_singles(no, f, Vb, u1, u2, t2), eo.sigma_doubles(no, f, Vb, u1, u2, t2)
    return dict(B=B, f=f, t1=t1, t2=t2, u1=u1, u2=u2, fd=fd, r1=r1, r2=r2, s1=s1, s2=s2)


@pytest.fixture(scope="module")
def engines(gpu_lib):
    """One context per side of the cap with the integrals built on the device from the factors; ``cache`` keeps what a pass
    gave, so that the tests of the results and those of the branch share one run."""
    made = {}

    def get(no):
        if no not in made:
            ctx = Context(no, 2, lib=gpu_lib)
            ctx.set_V_from_factors(engine_inputs(no, 2)["B"])
            made[no] = ctx
        return made[no]
    get.cache = {}
    yield get
    for ctx in made.values():
        ctx.close()


def close_to(got, ref, tol, scaled=False):
    """Absolute, as test_gpu_cc.py asserts its residuals (the references here are O(1): max |R1| = 0.8, |R2| = 1.5, |sigma2| =
    27); ``scaled``: of max(1, max |reference|), the rule of test_gpu_big.py for the pair-sharded tail."""
    err, scale = np.abs(got - ref).max(), (max(1.0, np.abs(ref).max()) if scaled else 1.0)
    print("   max error %.2e, bound %.2e, max |reference| %.2e" % (err, tol * scale, np.abs(ref).max()))
    return err <= tol * scale


@contextlib.contextmanager
def task_kinds(ctx, phase, into):
    """With phases on: PYMES_PHASE_LOG for the block, and the kinds of the tasks it recorded — the names in the library's
    "[phase]   L<level> kind:blocks:cost ..." lines on stderr — added to the set ``into``.  What ran, told by the launcher itself:
    "layouts" is t2_layouts, "assemble" residual_assemble, "perm" / "permT" a permute, "unpackL" ladder_sym_unpack."""
    if phase is not None:
        yield
        return
    with tempfile.TemporaryFile() as tmp, env(ctx, PYMES_PHASE_LOG="1"):
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            yield
            ctx.sync()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    into.update(re.findall(r" ([A-Za-z0-9]+):\d+:[0-9.]+", text))


def fused_by_the_log(kinds):
    """True: both fused kernels were recorded; False: neither of them, permutes instead."""
    if {"layouts", "assemble"} <= kinds:
        return True
    assert not ({"layouts", "assemble"} & kinds) and ({"perm", "permT"} & kinds), kinds
    return False


def cc_pass(engines, no, phase):
    """(R1, R2, permutation passes, phase tasks recorded) of one whole-step residual pass (CCSD, T1 != 0), once per switch.  The
    pass that is counted is the second one under the switch: the first builds what a context builds once (packed blocks and
    other statics, some of them with permutes), on whichever context happens to be new."""
    key = ("cc", no, phase)
    if key not in engines.cache:
        nv = 2
        ctx, c = engines(no), engine_inputs(no, nv)
        with env(ctx, PYMES_PHASE=phase, PYMES_PHASE_MAX_US=None):
            r1, r2 = ctx.array(np.full((nv, no), np.nan)), ctx.array(np.full((nv, nv, no, no), np.nan))
            f, t1, t2 = ctx.array(c["f"]), ctx.array(c["t1"]), ctx.array(c["t2"])
            ctx.ccsd_residuals(f, t1, t2, r1, r2)
            r1.set(np.full((nv, no), np.nan))
            r2.set(np.full((nv, nv, no, no), np.nan))
            before = ctx.phase_stats()["tasks"]
            ctx.stats(reset=True)
            kinds = set()
            with task_kinds(ctx, phase, kinds):
                ctx.ccsd_residuals(f, t1, t2, r1, r2)
            permutes = ctx.stats(reset=True)["permute_calls"]
            recorded = ctx.phase_stats()["tasks"] - before
            engines.cache[key] = (r1.get(), r2.get(), permutes, recorded, kinds)
    return engines.cache[key]


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
@pytest.mark.parametrize("no", [90, 91])
def test_ccsd_residuals_both_sides(engines, no, phase):
    c = engine_inputs(no, 2)
    g1, g2, _, recorded, _ = cc_pass(engines, no, phase)
    assert engines(no).pairs_supported() == (no == 90)
    assert (recorded > 0) == (phase is None)
    assert close_to(g1, c["r1"], TOL)
    assert close_to(g2, c["r2"], 10 * TOL)


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
def test_ccsd_residuals_branch(engines, phase):
    """Which branch ran: Engine::pair_layouts_of and Engine::residual_finish count ONE pass each when fused; past the cap the
    layouts are three or four permutes and the assembly six or more.  Everything else in the pass is the same code at 90 and 91
    (both are above the 80 of the bra dressing): at least seven passes more.  With phases on the launcher's own log names
    the tasks: t2_layouts and residual_assemble at 90, neither of them and permutes at 91."""
    a, b = cc_pass(engines, 90, phase), cc_pass(engines, 91, phase)
    print("   permutation passes: %d at 90, %d at 91; task kinds %s | %s" % (a[2], b[2], sorted(a[4]), sorted(b[4])))
    assert b[2] >= a[2] + 7
    if phase is None:
        assert fused_by_the_log(a[4]) and not fused_by_the_log(b[4])
        assert "unpackL" in b[4] and "unpackL" not in a[4]


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_pair_sharded_assembly_at_the_cap(engines, rank, world):
    """residual_assemble_pairs (through residual_finish_pairs, after the slab of the same amplitudes) on a rank's pairs against
    the oracle's rows, at the bound test_gpu_big.py asks of this path."""
    no, nv = 90, 2
    ctx, c = engines(no), engine_inputs(no, nv)
    ov, npp, o2 = no * nv, nv * (nv + 1) // 2, no * no
    r0, r1, ch = chunk_of(nv, rank, world)
    dT1, dT2 = ctx.array(c["t1"]), ctx.array(c["t2"])
    fd = ctx.empty(c["f"].shape)
    ctx.dress_fock(ctx.array(c["f"]), dT1, fd)
    ctx.dress_V(dT1, ("klij", "iajb", "iabj"))
    pad = -(-ov // world) * world
    ETd, ETx, L, QK = ctx.zeros((pad, ov)), ctx.zeros((pad, ov)), ctx.zeros((world * ch, o2)), ctx.zeros((pad, o2))
    for r in range(world):
        ctx.residual_slab(fd, dT2, ETd, ETx, L, r, world, dressed=True, t1=dT1, QK=QK)
    Rc = ctx.array(np.full((ch, 2, o2), np.nan))
    ctx.residual_finish_pairs(fd, dT2, ETd, ETx, L, Rc, rank, world, dT1, QK, dressed=True)
    got = Rc.get()
    want = compact(c["r2"], no, nv, rank, world)
    live = np.isfinite(want)
    assert r1 > r0 and np.array_equal(np.isfinite(got), live)
    assert close_to(got[live], want[live], 1e-11, scaled=True)


def eom_pass(engines, no, phase):
    """(sigma1, sigma2, permutation passes, tasks recorded, the handle's fused flag) of one right sigma build for a trial vector
    whose doubles have no exchange symmetry; past the cap the left build on the same handle must refuse by name."""
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    key = ("eom", no, phase)
    if key not in engines.cache:
        ctx, c = engines(no), engine_inputs(no, 2)
        with env(ctx, PYMES_PHASE=phase, PYMES_PHASE_MAX_US=None):
            sig = LeftSigma(ctx, c["f"], ctx.array(c["t2"]))
            try:
                u1, u2, l2 = ctx.array(c["u1"]), ctx.array(c["u2"]), ctx.array(c["t2"])
                before = ctx.phase_stats()["tasks"]
                ctx.stats(reset=True)
                kinds = set()
                with task_kinds(ctx, phase, kinds):
                    s1, s2 = [x.get() for x in sig.apply(u1, u2)]
                permutes = ctx.stats(reset=True)["permute_calls"]
                recorded = ctx.phase_stats()["tasks"] - before
                if no > 90:
                    held = _live()
                    with pytest.raises(E, match="apply_left: nocc too large for the fused pair kernels"):
                        sig.apply_left(u1, l2, True)
                    assert _live() == held
                engines.cache[key] = (s1, s2, permutes, recorded, sig.fused_ok, kinds)
            finally:
                sig.close()
    return engines.cache[key]


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
@pytest.mark.parametrize("no", [90, 91])
def test_eom_sigma_both_sides(engines, no, phase):
    """Against oracle/eom_oracle.py at the bounds of the residual test above."""
    c = engine_inputs(no, 2)
    s1, s2, _, recorded, fused, _ = eom_pass(engines, no, phase)
    assert fused == (no == 90)
    assert (recorded > 0) == (phase is None)
    assert close_to(s1, c["s1"], TOL)
    assert close_to(s2, c["s2"], 10 * TOL)


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
def test_eom_sigma_branch(engines, phase):
    """The handle says which branch it takes (pymes_eom_sigma_flags: the flag every fork of the build reads), and with phases on
    the launcher's log says what ran: t2_layouts and residual_assemble tasks at 90, neither and permutes at 91.  The count of
    permutation passes says nothing here: the fused build counts its stacked layouts and its assembly, the unfused one its
    permutes, and the two totals differ by one in either direction (printed)."""
    a, b = eom_pass(engines, 90, phase), eom_pass(engines, 91, phase)
    print("   permutation passes: %d at 90, %d at 91; task kinds %s | %s" % (a[2], b[2], sorted(a[5]), sorted(b[5])))
    assert a[4] and not b[4]
    if phase is None:
        assert fused_by_the_log(a[5]) and not fused_by_the_log(b[5])


# ---- 3b. the other branches of the sigma build on both sides of the cap (tests/_eom_branch_cases.py; the lattice at small shapes:
# tests/test_gpu_eom_branches.py).  eom_pass above runs a general vector on the all-symmetric handle only ---------------------------------
@functools.lru_cache(maxsize=None)
def branch_inputs(no):
    """On the problem of ``engine_inputs(no, 2)``: two trial vectors WITH the exchange symmetry, T2 plus noise without it (a
    handle with t_sym = hole_sym = 0 on the shared integrals), and the oracle's sigma for (amplitudes, vector) in
    ("T", "sym0"), ("T", "sym1"), ("Tn", "sym0"), ("Tn", "gen") — "gen" is the general vector of engine_inputs —, once."""
    from pymes_amd.solver.eom_ccsd import _Sigma
    nv = 2
    c = engine_inputs(no, nv)
    rng = np.random.default_rng(11 * no + nv)
    vec = {"gen": (c["u1"], c["u2"])}
    for z in range(2):
        vec["sym%d" % z] = (rng.standard_normal((nv, no)), 0.5 * sym4(rng, no, nv))       # (the size of the general one)
    amp = {"T": c["t2"], "Tn": np.ascontiguousarray(c["t2"] + 0.02 * rng.standard_normal(c["t2"].shape))}
    Vu = so.FactorBlocks(no, c["B"])
    Vb = {k: Vu(k) for k in _Sigma.BLOCKS}
    flags = {k: BC.expected_flags(no, Vb, t) for k, t in amp.items()}
    assert flags == {"T": (True, True, True), "Tn": (True, False, False)}
    sigma = {}
    for a, v in (("T", "sym0"), ("T", "sym1"), ("Tn", "sym0"), ("Tn", "gen")):
        u1, u2 = vec[v]
        sigma[a, v] = (eo.sigma_singles(no, c["f"], Vb, u1, u2, amp[a]), eo.sigma_doubles(no, c["f"], Vb, u1, u2, amp[a]))
    return dict(vec=vec, amp=amp, flags=flags, sigma=sigma)


def branch_pass(engines, no, phase, amps, names):
    """One ``apply_many`` of the named vectors (symmetry detected on the device) on a handle over the named amplitudes, into
    NaN-filled arrays: ([(sigma1, sigma2)], the same vectors built one by one, the handle's flags, tasks recorded, task kinds);
    past the cap, and at the cap (above PYMES_NOCC_MAX_LAMBDA), the left build on the handle must refuse by name."""
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    key = ("branch", no, phase, amps, names)
    if key not in engines.cache:
        ctx, c, b = engines(no), engine_inputs(no, 2), branch_inputs(no)
        nv = 2
        with env(ctx, PYMES_PHASE=phase, PYMES_PHASE_MAX_US=None):
            sig = LeftSigma(ctx, c["f"], ctx.array(b["amp"][amps]))
            try:
                d1, d2 = [ctx.array(b["vec"][n][0]) for n in names], [ctx.array(b["vec"][n][1]) for n in names]
                o1 = [ctx.array(np.full((nv, no), np.nan)) for _ in names]
                o2 = [ctx.array(np.full((nv, nv, no, no), np.nan)) for _ in names]
                before = ctx.phase_stats()["tasks"]
                kinds = set()
                with task_kinds(ctx, phase, kinds):
                    sig.apply_many(d1, d2, out1=o1, out2=o2)
                    got = [(x.get(), y.get()) for x, y in zip(o1, o2)]
                recorded = ctx.phase_stats()["tasks"] - before
                single = [tuple(x.get() for x in sig.apply(d1[z], d2[z])) for z in range(len(names))]
                l2 = ctx.array(b["vec"]["sym0"][1])
                held = _live()
                refusal = ("apply_left: nocc too large for the fused pair kernels" if no > limit("PYMES_NOCC_MAX_FUSED") else
                           "lambda_assemble: nocc = %d is too large for the LDS tile" % no)
                with pytest.raises(E, match=refusal):          # (into arrays of the caller: nothing is allocated on the way in)
                    sig.apply_left_many([d1[0]], [l2], syms=[True], out1=[o1[0]], out2=[o2[0]])
                assert _live() == held
                engines.cache[key] = (got, single, BC.handle_flags(sig) + (sig.fused_ok, sig.many_ok), recorded, kinds)
            finally:
                sig.close()
    return engines.cache[key]


BRANCH_CASES = [("T", ("sym0",)), ("Tn", ("sym0",)), ("Tn", ("gen",))]
BRANCH_IDS = ["T-sym", "Tn-sym", "Tn-general"]


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
@pytest.mark.parametrize("amps,names", BRANCH_CASES, ids=BRANCH_IDS)
@pytest.mark.parametrize("no", [90, 91])
def test_eom_sigma_branches_both_sides(engines, no, amps, names, phase):
    """A trial vector WITH the exchange symmetry on the all-symmetric handle — at 91 the packed build that is not fused: a scaled
    copy of Dx, the symmetrisation by permutes, the packed terms, ladder_sym_unpack —, and a symmetric and a general vector on
    a handle over an unsymmetric T2 (t_sym = hole_sym = 0: the T . B5 term inside the symmetrisation, Bn without the held-back u1
    term), against oracle/eom_oracle.py at the bounds of test_eom_sigma_both_sides, with the flags of the handle asserted."""
    b = branch_inputs(no)
    got, _, flags, recorded, kinds = branch_pass(engines, no, phase, amps, names)
    fused = no == 90
    assert flags == b["flags"][amps] + (fused, fused and amps == "T")
    assert (recorded > 0) == (phase is None)
    print("branch (%d,2) amplitudes %s vector %s %s: flags %s" % (no, amps, names[0], "phases" if phase is None else "PYMES_PHASE=0", flags))
    for n, (s1, s2) in zip(names, got):
        assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
        assert close_to(s1, b["sigma"][amps, n][0], TOL)
        assert close_to(s2, b["sigma"][amps, n][1], 10 * TOL)
    if phase is None:
        assert fused_by_the_log(kinds) == fused
        if names == ("sym0",) and amps == "T":              # the packed rows are unpacked by a kernel of their own past the cap only
            assert ("unpackL" in kinds) == (not fused)


@pytest.mark.parametrize("phase", PHASES, ids=PHASE_IDS)
def test_eom_sigma_two_symmetric_vectors_past_the_cap(engines, phase):
    """k = 2 symmetric vectors at 91: many_ok is false, so the batch goes vector by vector — each result in its own array,
    equal to the build of that vector alone (the same kernels in the same order: printed whether to the bit), at the oracle."""
    no, names = 91, ("sym0", "sym1")
    b = branch_inputs(no)
    got, single, flags, _, _ = branch_pass(engines, no, phase, "T", names)
    assert flags == (True, True, True, False, False)
    print("branch (91,2) k = 2 symmetric vectors %s" % ("phases" if phase is None else "PYMES_PHASE=0"))
    for n, (s1, s2), (t1_, t2_) in zip(names, got, single):
        assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
        assert close_to(s1, b["sigma"]["T", n][0], TOL)
        assert close_to(s2, b["sigma"]["T", n][1], 10 * TOL)
        print("   batch == single to the bit:", np.array_equal(s1, t1_) and np.array_equal(s2, t2_))
        assert close_to(s1, t1_, TOL) and close_to(s2, t2_, 10 * TOL)
    assert np.abs(got[0][1] - got[1][1]).max() > 1e-3


def test_left_build_on_unsymmetric_T_at_the_lambda_cap(gpu_lib):
    """The left build admits nocc <= PYMES_NOCC_MAX_LAMBDA = 88 < 90 (refused by name at 89 and 90: branch_pass above and
    test_lambda_assemble_refuses_by_name), so its run on a handle with t_sym = hole_sym = 0 is at (88,2): k = 2, stacked and
    one by one, against tests/_lambda_reference.left_sigma at the bound of tests/test_gpu_lambda.py."""
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    no, nv = limit("PYMES_NOCC_MAX_LAMBDA"), 2
    f, Vb, t2, l1, l2, _ = LE._apply_case(no, nv, False)
    rng = np.random.default_rng(88)
    case = BC.Case(no, nv, 0, ("t2",), problem=(f, Vb, np.ascontiguousarray(t2 + 0.02 * rng.standard_normal(t2.shape))))
    assert case.flags == (True, False, False)
    before = _live()
    ctx = Context(no, nv, lib=gpu_lib)
    try:
        case.upload(ctx, LeftSigma.BLOCKS)
        sig = LeftSigma(ctx, f, ctx.array(case.t2))
        assert BC.handle_flags(sig) == case.flags and sig.fused_ok
        l1s, l2s = [l1, rng.standard_normal(l1.shape)], [l2, sym4(rng, no, nv)]
        assert BC.check_left(ctx, sig, case, l1s, l2s, None, BC.LEFT_TOL, label="(88,2) t2") <= BC.LEFT_TOL
        sig.close()
    finally:
        ctx.close()
    assert _live() == before
