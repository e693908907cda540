"""GPU: the amplitude tail on exchange-symmetric amplitudes (include/pymes_amd.h, pymes_sym_tail) — the forms of the update,
the DIIS overlaps and extrapolation, the energy pass and the residual's pair layouts that read each exchange pair of tiles
once — against their full-read forms (PYMES_SYM_TAIL=0, the same process) and against numpy.

The new forms are launches for calls too large to be a task of a phase; a smaller call keeps the full-read form (with
phases on or off), and at these sizes every call is that small.  ``forced`` therefore arms the phase machinery with
PYMES_PHASE_MAX_US=0 (nothing is small).

Shapes (no, nv): (1,2) and (6,1) the smallest / a diagonal pair only; (2,3) even nocc (16-byte loads); (3,4), (5,3) odd nocc
(scalar loads); (16,5), (17,4) o^2 = 256 and 289 against the 256-thread block loop; (24,3), (32,2) the 16-byte form past one
trip of that loop: o^2 / 2 = 288 and 512 double2 per tile, at no = 24 the (i, j) digits advance by (21, 4) per trip and carry on
the second one, at no = 32 by (16, 0) without a carry."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from oracle.cases import synthetic_factors
from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.mixer.diis import DIIS
from pymes_amd.solver import ccd, ccsd

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2), (2, 3), (3, 4), (5, 3), (16, 5), (17, 4), (24, 3), (32, 2), (6, 1)]
GOLD = os.path.join(os.path.dirname(__file__), "golden")
EPS = 2.0 ** -53


@contextlib.contextmanager
def env(ctx, **kv):
    """Set / unset environment switches; the phase switches are read when the machinery is re-armed (phase_enable(-1))."""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    ctx.phase_enable(-1)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.phase_enable(-1)


def forced(ctx):
    return env(ctx, PYMES_PHASE_MAX_US="0", PYMES_SYM_TAIL=None)


def full_read(ctx):
    return env(ctx, PYMES_PHASE_MAX_US="0", PYMES_SYM_TAIL="0")


def sym4(rng, no, nv):
    """Random [v,v,o,o] array with X[a,b,i,j] == X[b,a,j,i] bit for bit (x + y == y + x in floating point)."""
    x = rng.standard_normal((nv, nv, no, no))
    return np.ascontiguousarray(x + x.transpose(1, 0, 3, 2))


def tr(x):
    return x.transpose(1, 0, 3, 2)


def grid_energies(rng, no, nv):
    """Orbital energies on a 1/64 grid: every partial sum of eo_i + eo_j - ev_a - ev_b + shift (shift on the grid too) is
    exact, so the denominator does not depend on the order in which a and b enter it.  The full-read update evaluates it per
    element in index order; with arbitrary energies its tile (b,a) can differ from the transpose of its tile (a,b) in the
    last bits (test_update_arbitrary_energies) — the grid separates what the new kernel moves from that rounding."""
    eo = np.sort(-1.0 - rng.integers(0, 64, no) / 64.0)
    ev = np.sort(1.0 + rng.integers(0, 64, nv) / 64.0)
    return eo, ev


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def case(request, gpu_lib):
    no, nv = request.param
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=1 << 24)
    assert ctx.sym_tail(), "the build must have the read-once forms and the tile must fit"
    yield ctx, no, nv
    ctx.close()


@pytest.mark.parametrize("inplace", [False, True])
def test_update_bitwise(case, inplace):
    ctx, no, nv = case
    rng = np.random.default_rng(100 * no + nv)
    eo, ev = grid_energies(rng, no, nv)
    ctx.set_orbital_energies(eo, ev)
    R, T = sym4(rng, no, nv), sym4(rng, no, nv)

    def run(sym):
        dT, dR, dD = ctx.array(T), ctx.array(R), ctx.empty(T.shape)
        if inplace:
            ctx.cc_update(dT, dD, dR, level_shift=0.25, delta=0.75, sym=sym)
            return dT.get(), dD.get()
        dO = ctx.empty(T.shape)
        ctx.cc_update_to(dO, dD, dT, dR, level_shift=0.25, delta=0.75, sym=sym)
        assert np.array_equal(dT.get(), T)
        return dO.get(), dD.get()
    with forced(ctx):
        t_new, d_new = run(True)
    with full_read(ctx):
        t_old, d_old = run(True)            # the declaration without the forms: the parent's kernel
        t_plain, d_plain = run(False)
    assert np.array_equal(t_old, t_plain) and np.array_equal(d_old, d_plain)
    assert np.array_equal(t_new, t_old) and np.array_equal(d_new, d_old)
    assert np.array_equal(t_new, tr(t_new)) and np.array_equal(d_new, tr(d_new))
    D = eo[None, None, :, None] + eo[None, None, None, :] - ev[:, None, None, None] - ev[None, :, None, None]
    assert np.array_equal(d_new, R * (1.0 / (D + 0.25)))


def test_update_arbitrary_energies(case):
    """Arbitrary orbital energies: tiles a >= b equal the full-read form bit for bit, the output is exchange-symmetric bit
    for bit, and the tiles a < b differ from the full-read form by no more than the rounding of the denominator allows.
    Energies in [-2,-1] and [1,2], no shift: |D| >= 4, partial sums <= 8 in magnitude, so two orders of summation differ by
    <= 4 roundings of 8 * 2^-53, i.e. 2^-50 relative to D; two more roundings each (reciprocal, product) give 2^-49 with room."""
    ctx, no, nv = case
    rng = np.random.default_rng(7 * no + nv)
    eo, ev = np.sort(-1 - rng.random(no)), np.sort(1 + rng.random(nv))
    ctx.set_orbital_energies(eo, ev)
    R, T = sym4(rng, no, nv), sym4(rng, no, nv)

    def run():
        dO, dD = ctx.empty(T.shape), ctx.empty(T.shape)
        ctx.cc_update_to(dO, dD, ctx.array(T), ctx.array(R), sym=True)
        return dO.get(), dD.get()
    with forced(ctx):
        t_new, d_new = run()
    with full_read(ctx):
        t_old, d_old = run()
    lower = np.tril(np.ones((nv, nv), dtype=bool))[:, :, None, None] & np.ones((1, 1, no, no), dtype=bool)
    assert np.array_equal(t_new[lower], t_old[lower]) and np.array_equal(d_new[lower], d_old[lower])
    assert np.array_equal(t_new, tr(t_new)) and np.array_equal(d_new, tr(d_new))
    assert np.all(np.abs(d_new - d_old) <= 2.0 ** -49 * np.abs(d_old))
    assert np.all(np.abs(t_new - t_old) <= 2.0 ** -49 * (np.abs(T) + np.abs(d_old)))


@pytest.mark.parametrize("m", [1, 6])
def test_lincomb_bitwise(case, m):
    ctx, no, nv = case
    rng = np.random.default_rng(13 * no + nv + m)
    X = [sym4(rng, no, nv) for _ in range(m)]
    c = rng.standard_normal(m)
    xs = [ctx.array(x) for x in X]

    def run(sym):
        out = ctx.empty(X[0].shape)
        ctx.lincomb(out, xs, c, sym=sym)
        return out.get()
    with forced(ctx):
        new = run(True)
    with full_read(ctx):
        old, plain = run(True), run(False)
    assert np.array_equal(old, plain)
    assert np.array_equal(new, old)
    assert np.array_equal(new, tr(new))
    for x, d in zip(X, xs):
        assert np.array_equal(d.get(), x)             # out aliases no input: the inputs are untouched


def test_layouts_bitwise(case):
    ctx, no, nv = case
    rng = np.random.default_rng(17 * no + nv)
    T = sym4(rng, no, nv)
    dT, ov = ctx.array(T), no * nv

    def run(sym, with_td):
        Xd, Xx, Xt = ctx.empty((ov, ov)) if with_td else None, ctx.empty((ov, ov)), ctx.empty((ov, ov))
        ctx.pair_layouts(dT, Xx, Xt, Xd, sym=sym)
        return (Xd.get() if with_td else None), Xx.get(), Xt.get()
    for with_td in (True, False):
        with forced(ctx):
            new = run(True, with_td)
        with full_read(ctx):
            old = run(False, with_td)
        for a, b in zip(new, old):
            assert (a is None and b is None) or np.array_equal(a, b)
    Td = T.transpose(0, 2, 1, 3).reshape(ov, ov)
    assert np.array_equal(new[1], T.transpose(0, 3, 1, 2).reshape(ov, ov))
    assert np.array_equal(new[2], 2.0 * Td - T.transpose(1, 2, 0, 3).reshape(ov, ov))
    assert np.array_equal(new[2], new[2].T)           # Tt_d[(a,i),(b,j)] == Tt_d[(b,j),(a,i)]: the transpose of the array


@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("with_t1", [False, True])
def test_dots(case, m, with_t1):
    """<e_i, e_new> over the history, T2-sized pairs declared symmetric, T1-sized pairs of the same call plain.  Both forms
    sum the same n products in another order: |difference| <= 2 n 2^-53 sum |x_i y_i| against numpy and against each other."""
    ctx, no, nv = case
    rng = np.random.default_rng(19 * no + nv + m)
    E2 = [sym4(rng, no, nv) for _ in range(m)]
    new2 = sym4(rng, no, nv)
    E1 = [rng.standard_normal((nv, no)) for _ in range(m)] if with_t1 else []
    new1 = rng.standard_normal((nv, no))
    xs = [ctx.array(x) for x in E1 + E2]
    ys = [ctx.array(new1)] * len(E1) + [ctx.array(new2)] * m
    flags = [False] * len(E1) + [True] * m
    ref = np.array([np.dot(x.ravel(), new1.ravel()) for x in E1] + [np.dot(x.ravel(), new2.ravel()) for x in E2])
    bound = np.array([2 * x.size * EPS * np.abs(x * new1).sum() for x in E1] +
                     [2 * x.size * EPS * np.abs(x * new2).sum() for x in E2])
    with forced(ctx):
        new = ctx.dots(xs, ys, sym=flags)
    with full_read(ctx):
        old, plain = ctx.dots(xs, ys, sym=flags), ctx.dots(xs, ys)
    print("dots", (no, nv), m, with_t1, np.abs(new - ref).max(), np.abs(new - old).max(), bound.min())
    assert np.array_equal(old, plain)
    assert np.all(np.abs(new - ref) <= bound) and np.all(np.abs(new - old) <= bound)
    if with_t1:
        assert np.array_equal(new[:m], old[:m])       # the T1 pairs keep the plain form


def _bitsym_V(no, nv, seed):
    rng = np.random.default_rng(seed)
    n = no + nv
    V = rng.standard_normal((n, n, n, n)) * 0.1
    return np.ascontiguousarray(V + V.transpose(1, 0, 3, 2))


def set_whole_V(ctx, no, nv, seed):
    """All of a random V_pqrs == V_qpsr (bit for bit) on the context; returns its block V_ijab [o,o,v,v]."""
    V = _bitsym_V(no, nv, seed)
    ctx.set_V_pqrs(V)
    return V[:no, :no, no:, no:]


@pytest.mark.parametrize("with_t1", [False, True])
@pytest.mark.parametrize("with_dt2", [False, True])
def test_energy_norms(case, with_t1, with_dt2):
    check_energy_norms(case, with_t1, with_dt2)


def check_energy_norms(case, with_t1, with_dt2, set_V=set_whole_V):
    """``set_V(ctx, no, nv, seed)`` puts the integrals on the context and returns V_ijab (tests/test_gpu_nocc_cap.py uploads
    that block alone: (no + nv)^4 doubles are 0.6 GB at no = 90)."""
    ctx, no, nv = case
    rng = np.random.default_rng(23 * no + nv)
    n = no + nv
    Vijab = set_V(ctx, no, nv, 29 * no + nv)
    f = rng.standard_normal((n, n))
    t1 = rng.standard_normal((nv, no))
    T, dT = sym4(rng, no, nv), sym4(rng, no, nv)
    args = (ctx.array(f) if with_t1 else None, ctx.array(t1) if with_t1 else None, ctx.array(T),
            ctx.array(dT) if with_dt2 else None)
    with forced(ctx):
        new = np.array(ctx.energy_norms(*args, sym=True))
    with full_read(ctx):
        old, plain = np.array(ctx.energy_norms(*args, sym=True)), np.array(ctx.energy_norms(*args))
    assert np.array_equal(old, plain)
    Edir = Vijab.transpose(2, 3, 0, 1)
    Eex = Vijab.transpose(3, 2, 0, 1)
    tau = T + (np.einsum("ai,bj->abij", t1, t1) if with_t1 else 0.0)
    ref = np.array([2.0 * (f[:no, no:].T * t1).sum() if with_t1 else 0.0, 2.0 * (tau * Edir).sum(), -(tau * Eex).sum(),
                    (T * T).sum(), (dT * dT).sum() if with_dt2 else 0.0, (t1 * t1).sum() if with_t1 else 0.0])
    cnt = T.size
    # (tau itself carries one rounding per element: one more n-independent unit on the two energy sums)
    bound = 2 * cnt * EPS * np.array([0.0, 2.0 * np.abs(tau * Edir).sum(), np.abs(tau * Eex).sum(), (T * T).sum(),
                                      (dT * dT).sum() if with_dt2 else 0.0, 0.0])
    bound[[0, 5]] = 2 * t1.size * EPS * np.array([2.0 * np.abs(f[:no, no:].T * t1).sum(), (t1 * t1).sum()]) if with_t1 else 0.0
    print("energy", (no, nv), with_t1, with_dt2, np.abs(new - ref), np.abs(new - old), bound)
    assert np.all(np.abs(new - ref) <= bound) and np.all(np.abs(new - old) <= bound)
    assert new[0] == old[0] and new[5] == old[5]          # the T1 sums are the same code


def test_guard_never_inferred_from_the_shape(case):
    """Vectors WITHOUT the symmetry: the plain calls, and the declaring calls under PYMES_SYM_TAIL=0, give the plain results
    (numpy); the declaring calls with the forms on read the tiles a >= b only — which also shows that the forms ran."""
    ctx, no, nv = case
    rng = np.random.default_rng(31 * no + nv)
    X, Y = rng.standard_normal((nv, nv, no, no)), rng.standard_normal((nv, nv, no, no))
    dX, dY = ctx.array(X), ctx.array(Y)
    ref = float(np.dot(X.ravel(), Y.ravel()))
    tol = 2 * X.size * EPS * np.abs(X * Y).sum()
    out = ctx.empty(X.shape)
    with forced(ctx):
        assert abs(ctx.dots([dX], [dY])[0] - ref) <= tol                       # no declaration
        ctx.lincomb(out, [dX, dY], [0.5, -2.0])
        assert np.array_equal(out.get(), X * 0.5 + Y * -2.0)
        half = ctx.dots([dX], [dY], sym=[True])[0]
        ctx.lincomb(out, [dX, dY], [0.5, -2.0], sym=True)
        got = out.get()
    with full_read(ctx):
        assert abs(ctx.dots([dX], [dY], sym=[True])[0] - ref) <= tol           # declared, forms off
        ctx.lincomb(out, [dX, dY], [0.5, -2.0], sym=True)
        assert np.array_equal(out.get(), X * 0.5 + Y * -2.0)
    low = np.tril(np.ones((nv, nv)), -1)[:, :, None, None]
    dia = np.eye(nv)[:, :, None, None]
    assert abs(half - (2.0 * (X * Y * low).sum() + (X * Y * dia).sum())) <= 2 * tol + 2 * X.size * EPS * abs(half)
    plain = X * 0.5 + Y * -2.0
    for a in range(nv):
        for b in range(a + 1):           # tile (a, b <= a) as the plain form computes it, tile (b,a) its transpose
            assert np.array_equal(got[a, b], plain[a, b]) and np.array_equal(got[b, a], got[a, b].T if a != b else plain[a, a])
    if nv > 1:
        assert not np.array_equal(got, plain)


@pytest.mark.parametrize("m", [1, 6])
@pytest.mark.parametrize("native", [True, False])
def test_mixer_with_declaration(case, m, native):
    """DIIS.mix over a history of m (T1, T2) pairs, T2 declared symmetric (pymes_diis_mix_sym; dots + lincomb with the
    flags): the extrapolated T2 is exchange-symmetric bit for bit and equals the full-read mixer's to the accuracy the
    overlaps allow (their differences enter the coefficients through a small linear solve: compared at 1e-9 of the scale,
    far above the reductions' reordering and far below any error of substance)."""
    ctx, no, nv = case
    rng = np.random.default_rng(37 * no + nv + m)
    hist = [([rng.standard_normal((nv, no)), sym4(rng, no, nv)], [rng.standard_normal((nv, no)), sym4(rng, no, nv)])
            for _ in range(m)]

    def run(sym):
        mixer = DIIS(dim_space=8)
        for err, amp in hist:
            with contextlib.redirect_stdout(io.StringIO()):
                res = mixer.mix([ctx.array(e) for e in err], [ctx.array(a) for a in amp], native=native, sym=sym)
        return [r.get() for r in res]
    with forced(ctx):
        new = run((1,))
    with full_read(ctx):
        old = run((1,))
    assert np.array_equal(new[1], tr(new[1]))
    scale = max(1.0, np.abs(old[1]).max())
    assert np.abs(new[0] - old[0]).max() <= 1e-9 * scale and np.abs(new[1] - old[1]).max() <= 1e-9 * scale


def _golden_solve(gpu_lib, monkeypatch, kind):
    ref = json.load(open(os.path.join(GOLD, "solves.json")))["syn_20_80"]
    rec, ref = ref["recipe"], ref[kind]
    no, nv = 20, 80
    B, eps = synthetic_factors(no, nv, rec["seed"], rec["scale"], rec["gap"])
    monkeypatch.setattr(_lib, "_default", gpu_lib)
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        assert ints.ctx.sym_tail()
        with forced(ints.ctx), contextlib.redirect_stdout(io.StringIO()):
            if kind in ("ccsd", "dcsd"):
                s = ccsd.CCSD(no, delta_e=ref["delta_e"], is_dcsd=kind == "dcsd")
                e = s.solve(np.diag(eps), ints)["ccsd e"]
            else:
                s = ccd.CCD(no, delta_e=ref["delta_e"], is_dcd=kind == "dcd")
                e = s.solve(np.diag(eps), ints)["ccd e"]
    finally:
        ints.ctx.close()
    print(kind, "e", repr(e), "golden", repr(ref["e"]), "diff", e - ref["e"], "iterations", s.iterations)
    assert s.iterations == ref["iterations"]
    assert abs(e - ref["e"]) <= ref["delta_e"]


def test_golden_ccsd_20_80(gpu_lib, monkeypatch):
    """tests/golden/solves.json["syn_20_80"]["ccsd"] with the read-once tail forced (launches instead of phase tasks): the
    energy within the file's own tolerance (its delta_e), in the same 9 iterations."""
    _golden_solve(gpu_lib, monkeypatch, "ccsd")


def test_golden_dcsd_20_80(gpu_lib, monkeypatch):
    _golden_solve(gpu_lib, monkeypatch, "dcsd")


def test_golden_ccd_20_80(gpu_lib, monkeypatch):
    _golden_solve(gpu_lib, monkeypatch, "ccd")
