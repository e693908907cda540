"""GPU: the two kernels of the response solver's sweep and their shared second stage (csrc/kernels_post.hip: response_dots_kernel,
response_update_kernel, response_final_kernel; the C entries pymes_response_dots / pymes_response_update of include/pymes_amd.h)
called directly through ``_lib.ResponseSystem`` on a bare context and compared with the numpy references of the same operations
(tests/_response_reference.py: ``sweep_dots_reference``, ``sweep_update_reference``, proved on the CPU in
tests/test_response_reference.py).  The solver itself hides a wrong kernel — it converges more slowly or reports a break-down,
and measures every residual afresh — so nothing here goes through its stopping rule except test_solver_with_a_sliding_window.

  layouts     any off2 >= n1 with len = off2 + n1^2 is legal: an empty pad, a pad inside block 0, one that runs into block 1, a
              block that is all pad, a ragged last block, and 259 / 260 blocks of 2048 elements (the second trip of the final
              reduction's loop over the block partials), once almost all pad and once all data
  systems     real and complex in one call, nh = 0 ... 32 in one call, the start of a solve (p null, with and without nh)
  read-back   the pinned ring (up to 128 doubles) and the copy beyond it, for both entries; 4096 systems in one call
  the floor   z - d = +0, +-floor / 2, +-2 floor, real and complex, and floor = 0
  every call  each active element of x, r, p, ap, pn within (4 nh + 16) 2^-53 of its expression's magnitude — the forward bound
              of a chain of at most 4 nh + 16 roundings per component (q = z p - ap: 3; each stored direction: a product of 2 and a
              subtraction; the scale; alpha qh: 2, its subtraction; z - d; r conj(z - d): 2 more; |z - d|^2: 4; the division);
              pn = +0 in the pad; no NaN from the NaN pads; d and the stored directions untouched; each sum within 1e-13 of its
              magnitude sum from the exactly rounded sum (the bound of test_eom_correction_against_numpy for the same two-stage
              sum); the unused part of a row of dots zero; identical calls identical to the bit; a system in a batch identical to
              the bit to the same system alone
  in sequence eight sweeps of ``_sweep``'s own aliasing (p, ap become the next stored pair, pn the next p, a window of three) in
              lock-step with the reference, which is applied to the device's own state before every call
  the solver  history = 1 and 2 against the dense resolvent, with more sweeps than the window holds
  refusals    by name, leaving the allocations and the context as they were"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.solver.response import _pair
from tests import _response_reference as P
from tests.test_gpu_response import _live, _tolerance, quiet

pytestmark = pytest.mark.gpu
WS = 1 << 27                # bytes of workspace for a bare context: its default grows with o v^3
U = 2.0 ** -53
SUM_TOL = 1e-13
FLOOR = 1e-3
VECTORS = ("x", "r", "p", "ap", "pn")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (no, nv, n1, off2, len, blocks of the kernels' chunk)
SMALL = (3, 5, 15, 32, 257, 1)
RAGGED = (4, 16, 64, 64, 4160, 3)
PAD_IN_0 = (5, 13, 65, 96, 4321, 3)
PAD_INTO_1 = (5, 13, 65, 2100, 6325, 4)
PAD_BLOCK = (5, 13, 65, 4200, 8425, 5)
TRIP_PAD = (3, 5, 15, 530000, 530225, 259)
TRIP_DATA = (27, 27, 729, 736, 532177, 260)
LAYOUTS = [SMALL, RAGGED, PAD_IN_0, PAD_INTO_1, PAD_BLOCK, TRIP_PAD, TRIP_DATA]
ids = lambda lays: ["%d-%d-off%d" % (l[0], l[1], l[3]) for l in lays]


class Layout:
    def __init__(self, no, nv, n1, off2, length, blocks):
        src = open(os.path.join(ROOT, "pymes_amd", "csrc", "kernels_post.hip")).read()
        a, b = re.search(r"constexpr long kRespElems = (\d+) \* (\d+);", src).groups()
        chunk = int(a) * int(b)
        assert chunk == 2048
        assert n1 == no * nv and off2 >= n1 and length == off2 + n1 * n1 and blocks == -(-length // chunk)
        assert (blocks > 256) == (length > 524288)
        self.no, self.nv, self.n1, self.off2, self.nflat, self.blocks = no, nv, n1, off2, length, blocks
        self.act = P.active_mask(length, n1, off2)
        self.pad = ~self.act


# ---- host systems, their device copies, the two calls ------------------------------------------------------------------------------------
def _normal(rng, lay, cplx):
    """A seeded standard-normal flat vector, NaN in the pad."""
    v = rng.standard_normal(lay.nflat) + (1j * rng.standard_normal(lay.nflat) if cplx else 0.0)
    v[lay.pad] = complex(np.nan, np.nan) if cplx else np.nan
    return v


def _scalar(rng, cplx, lo=None, hi=None):
    """A coefficient of order 1 (``lo`` given: of modulus in [lo, hi]), real with either sign or complex."""
    v = complex(rng.standard_normal(), rng.standard_normal()) if cplx else complex(rng.standard_normal())
    return v if lo is None else v / abs(v) * rng.uniform(lo, hi)


def _system(rng, lay, cplx, nh, step=True):
    S = P.SweepSystem(x=_normal(rng, lay, cplx), r=_normal(rng, lay, cplx), p=_normal(rng, lay, cplx) if step else None,
                      ap=_normal(rng, lay, cplx) if step else None,
                      hp=[_normal(rng, lay, cplx) for _ in range(nh if step else 0)],
                      hq=[_normal(rng, lay, cplx) for _ in range(nh if step else 0)],
                      g=[_scalar(rng, cplx) for _ in range(nh if step else 0)], alpha=_scalar(rng, cplx),
                      z=_scalar(rng, cplx, 0.5, 3.0), inv=rng.uniform(0.5, 2.0))
    S.cplx, S.struct_nh = cplx, nh
    return S


def _upload(ctx, v, cplx):
    """A host vector as the (real, imaginary) pair of device vectors the entries take (imaginary None: a real system)."""
    if v is None:
        return None
    v = np.asarray(v)
    return ctx.array(np.ascontiguousarray(v.real)), ctx.array(np.ascontiguousarray(v.imag)) if cplx else None


class DeviceSystem:
    """The device vectors of one host system, freshly uploaded; pn all NaN: every element must be written."""

    def __init__(self, ctx, lay, S, shared=None):
        self.S = S
        nan = np.full(lay.nflat, np.nan)
        self.v = dict(shared.v) if shared else {k: _upload(ctx, getattr(S, k), S.cplx) for k in ("x", "r", "p", "ap")}
        if not shared:
            self.v["pn"] = _upload(ctx, nan + (1j * nan if S.cplx else 0.0), S.cplx)
        self.hp = shared.hp if shared else [_upload(ctx, v, S.cplx) for v in S.hp]
        self.hq = shared.hq if shared else [_upload(ctx, v, S.cplx) for v in S.hq]

    def describe(self, s):
        S = self.S
        for k in VECTORS:
            _pair(getattr(s, k), self.v[k])
        s.nh = S.struct_nh
        for j in range(S.nh):
            _pair(s.hp[j], self.hp[j])
            _pair(s.hq[j], self.hq[j])
            s.g[j][0], s.g[j][1] = S.g[j].real, S.g[j].imag
        s.alpha[0], s.alpha[1] = S.alpha.real, S.alpha.imag
        s.z[0], s.z[1] = S.z.real, S.z.imag
        s.inv = S.inv

    def download(self):
        """Every vector as its (real, imaginary) pair of host arrays, as the device holds them."""
        get = lambda pair: None if pair is None else (pair[0].get(), pair[1].get() if pair[1] is not None else None)
        out = {k: get(self.v[k]) for k in VECTORS}
        out["hp"], out["hq"] = [get(v) for v in self.hp], [get(v) for v in self.hq]
        return out


def _structs(devs):
    arr = (_lib.ResponseSystem * len(devs))()
    for s, dev in zip(arr, devs):
        dev.describe(s)
    return arr


def _call_dots(ctx, lay, arr, n=None):
    n = len(arr) if n is None else n
    out = np.full((max(n, 1), _lib.RESPONSE_DOTS), np.nan)
    ctx.lib.call("pymes_response_dots", ctx.handle, n, C.byref(arr), lay.off2, lay.nflat, _lib.host_ptr(out))
    return out


def _call_update(ctx, lay, arr, d, floor, n=None):
    n = len(arr) if n is None else n
    out = np.full(max(n, 1), np.nan)
    ctx.lib.call("pymes_response_update", ctx.handle, n, C.byref(arr), C.c_void_p(d.ptr), floor, lay.off2, lay.nflat,
                 _lib.host_ptr(out))
    return out


def _cx(pair):
    return None if pair is None else pair[0] + (1j * pair[1] if pair[1] is not None else 0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    """Two downloads (nested pairs, lists, dictionaries of arrays) hold the same bits."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(_bits(a), _bits(b))


def _run(ctx, lay, systems, d, floor):
    """The systems freshly uploaded; the dots of all of them from ONE call (where they have a direction), then the update of all
    of them in ONE call.  Returns (rows or None, |r|^2, the downloads, d as the device holds it afterwards)."""
    devs = [DeviceSystem(ctx, lay, S) for S in systems]
    dd = ctx.array(d)
    arr = _structs(devs)
    rows = _call_dots(ctx, lay, arr) if systems[0].p is not None else None
    nrm = _call_update(ctx, lay, arr, dd, floor)
    return rows, nrm, [dev.download() for dev in devs], dd.get()


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------
class Worst:
    """The largest element error / bound and sum error / magnitude of a case, printed for profiles/response."""

    def __init__(self):
        self.element, self.sum = 0.0, 0.0

    def elements(self, got, ref, magnitude, act, bound, what):
        got, ref = np.asarray(got)[act], np.asarray(ref)[act]
        assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), what
        assert np.isfinite(ref.real).all() and np.isfinite(ref.imag).all(), what
        lim = bound * U * magnitude[act]
        for part in (np.real, np.imag):
            err = np.abs(part(got) - part(ref))
            bad = err > lim
            assert not bad.any(), (what, int(np.argmax(bad)), float(err[bad][0]), float(lim[bad][0]))
            if (lim > 0.0).any():
                self.element = max(self.element, float((err[lim > 0.0] / lim[lim > 0.0]).max()))

    def sums(self, got, ref, magnitude, what):
        got, ref, magnitude = np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(magnitude)
        assert np.isfinite(got).all(), what
        err = np.abs(got - ref)
        assert np.all(err <= SUM_TOL * magnitude), (what, got, ref, magnitude)
        if (magnitude > 0.0).any():
            self.sum = max(self.sum, float((err[magnitude > 0.0] / magnitude[magnitude > 0.0]).max()))


def _compare(lay, S, d, floor, row, nrm, got, worst, what, before=None):
    """One system of one pair of calls against the references (``before``: the system as the device held it, else S itself)."""
    B = before or S
    if row is not None:
        ref_row, mags = P.sweep_dots_reference(B, lay.n1, lay.off2)
        worst.sums(row, ref_row, mags, what + " dots")
        assert not row[2 * (S.nh + 2):].any() and row[2 * S.nh + 1] == 0.0, what
    new, mags, ref_nrm, mag_nrm, floored = P.sweep_update_reference(B, d, floor, lay.n1, lay.off2)
    bound = 4 * S.nh + 16
    for k in VECTORS:
        if new[k] is None:
            assert got[k] is None
            continue
        assert (got[k][1] is not None) == S.cplx
        worst.elements(_cx(got[k]), new[k], mags[k], lay.act, bound, "%s %s" % (what, k))
    for part in got["pn"][:2 if S.cplx else 1]:
        assert np.all(part[lay.pad] == 0.0) and not np.signbit(part[lay.pad]).any(), what + ": the pad of pn"
    worst.sums(nrm, ref_nrm, mag_nrm, what + " |r|^2")
    if B.p is None:                                   # no step: x and r are as they were, to the bit
        for k in ("x", "r"):
            assert _same(_cx(got[k])[lay.act], np.asarray(getattr(B, k))[lay.act] + (0j if S.cplx else 0.0)), "%s: %s changed" % (what, k)
    for name in ("hp", "hq"):
        assert _same([(np.asarray(v).real, np.asarray(v).imag) if S.cplx else (np.asarray(v).real, None) for v in getattr(S, name)],
                     got[name]), "%s: %s changed" % (what, name)
    return floored


def _check(ctx, lay, systems, d, floor, what, alone=True):
    """The whole set of assertions of the module's docstring for one batch of systems.  Returns the references' floored masks."""
    worst = Worst()
    rows, nrm, got, d_after = _run(ctx, lay, systems, d, floor)
    assert _same(d, d_after), what + ": d changed"
    floored = [_compare(lay, S, d, floor, None if rows is None else rows[s], nrm[s], got[s], worst, "%s system %d" % (what, s))
               for s, S in enumerate(systems)]
    again = _run(ctx, lay, systems, d, floor)
    assert _same(rows, again[0]) and _same(nrm, again[1]) and _same(got, again[2]), what + ": two identical calls differ"
    del again
    for s, S in enumerate(systems if alone else []):
        one = _run(ctx, lay, [S], d, floor)
        assert _same(None if rows is None else rows[s:s + 1], one[0]) and _same(nrm[s:s + 1], one[1]) and _same(got[s], one[2][0]), \
            "%s: system %d alone differs from the batch" % (what, s)
    print("SWEEP %-34s len %6d  %4d systems  element error / bound %.3f  sum error / magnitude %.2e"
          % (what, lay.nflat, len(systems), worst.element, worst.sum))
    return floored


def _context(lay, gpu_lib):
    from pymes_amd.device import Context
    return Context(lay.no, lay.nv, lib=gpu_lib, workspace_bytes=WS)


def _diagonal(rng, lay):
    d = rng.standard_normal(lay.nflat)
    d[lay.pad] = np.nan
    return d


# ---- 1. the cases of every layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=ids(LAYOUTS))
def test_real_and_complex_in_one_call(gpu_lib, layout):
    """One real system without stored directions and one complex system with three, in ONE call of each entry."""
    lay = Layout(*layout)
    rng = np.random.default_rng(100 + lay.nflat)
    ctx = _context(lay, gpu_lib)
    try:
        systems = [_system(rng, lay, False, 0), _system(rng, lay, True, 3)]
        _check(ctx, lay, systems, _diagonal(rng, lay), FLOOR, "real nh 0 + complex nh 3")
    finally:
        ctx.close()


FOUR = [RAGGED, PAD_IN_0, PAD_INTO_1, PAD_BLOCK, TRIP_PAD, TRIP_DATA]


@pytest.mark.parametrize("layout", FOUR, ids=ids(FOUR))
def test_systems_that_differ_in_nh(gpu_lib, layout):
    """Complex systems with nh = 0, 1, 12 and 32 in one call (the whole table of stored directions, on more than one block); at
    the two layouts of 259 / 260 blocks nh = 0 and 2, which keeps the upload near 100 MB."""
    lay = Layout(*layout)
    rng = np.random.default_rng(200 + lay.nflat)
    ctx = _context(lay, gpu_lib)
    try:
        nhs = (0, 2) if lay.blocks > 256 else (0, 1, 12, 32)
        systems = [_system(rng, lay, True, nh) for nh in nhs]
        _check(ctx, lay, systems, _diagonal(rng, lay), FLOOR, "complex nh " + " ".join(map(str, nhs)))
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids(LAYOUTS))
def test_start_of_a_solve(gpu_lib, layout):
    """The update with p null: pn and |r|^2 of the r given, x and r as they were.  Once with nh = 0 and once with nh = 5 and null
    stored directions, which the entry accepts: it looks at them only when there is a step."""
    lay = Layout(*layout)
    rng = np.random.default_rng(300 + lay.nflat)
    ctx = _context(lay, gpu_lib)
    try:
        for nh in (0, 5):
            systems = [_system(rng, lay, False, nh, step=False), _system(rng, lay, True, nh, step=False)]
            assert all(S.struct_nh == nh and S.nh == 0 and S.p is None for S in systems)
            _check(ctx, lay, systems, _diagonal(rng, lay), FLOOR, "p null, nh %d" % nh)
    finally:
        ctx.close()


# ---- 2. the two routes of the read-back ------------------------------------------------------------------------------------------------------
def test_read_back_through_the_ring_and_beyond(gpu_lib):
    """Dots are 68 doubles per system (n = 1: the ring, n = 2: the copy); the update returns one (n = 128: the ring, n = 129: the
    copy).  Then 4096 systems, the most a call takes, that share one read-only p, ap, r and two stored directions and differ in z
    and nh."""
    lay = Layout(*SMALL)
    rng = np.random.default_rng(400)
    ctx = _context(lay, gpu_lib)
    try:
        d = _diagonal(rng, lay)
        for n in (1, 2):
            _check(ctx, lay, [_system(rng, lay, True, 2) for _ in range(n)], d, FLOOR, "dots and update, n = %d" % n)
        for n in (128, 129):
            systems = [_system(rng, lay, False, 0, step=False) for _ in range(n)]
            _check(ctx, lay, systems, d, FLOOR, "update, p null, n = %d" % n, alone=False)
        first = _system(rng, lay, True, 2)
        systems = []
        for s in range(4096):
            S = P.SweepSystem(x=first.x, r=first.r, p=first.p, ap=first.ap, hp=first.hp[:s % 3], hq=first.hq[:s % 3],
                              g=first.g[:s % 3], z=_scalar(rng, True, 0.5, 3.0))
            S.cplx, S.struct_nh = True, s % 3
            systems.append(S)
        shared = DeviceSystem(ctx, lay, first)
        worst = Worst()
        runs = []
        for _ in range(2):
            arr = _structs([DeviceSystem(ctx, lay, S, shared=shared) for S in systems])
            runs.append(_call_dots(ctx, lay, arr))
        assert _same(runs[0], runs[1])
        for s, S in enumerate(systems):
            ref_row, mags = P.sweep_dots_reference(S, lay.n1, lay.off2)
            worst.sums(runs[0][s], ref_row, mags, "system %d of 4096" % s)
            assert not runs[0][s][2 * (S.nh + 2):].any() and runs[0][s][2 * S.nh + 1] == 0.0
        for s in (0, 1, 2, 4095):
            assert _same(runs[0][s:s + 1], _call_dots(ctx, lay, _structs([DeviceSystem(ctx, lay, systems[s], shared=shared)])))
        print("SWEEP %-34s len %6d  %4d systems  sum error / magnitude %.2e" % ("dots, shared vectors", lay.nflat, 4096, worst.sum))
    finally:
        ctx.close()


# ---- 3. the floor of the preconditioner --------------------------------------------------------------------------------------------------------
def test_preconditioner_floor(gpu_lib):
    """z - d = +0, +-floor / 2 (floored, the sign of Re(z - d) kept, +floor at zero) and +-2 floor (not floored) at chosen active
    elements of the first, the second and the last block, everything else at |z - d| >= 0.5; a real system, a complex one with
    Im z = floor / 4 (floored where |Re| <= floor / 2) and one with Im z = 2 floor (never floored).  Every |z - d| is <= 0.6
    floor or >= 2 floor, so no rounding of x^2 + y^2 can move an element across the threshold.  Then floor = 0: nothing floored."""
    lay = Layout(*PAD_IN_0)
    rng = np.random.default_rng(500)
    z0 = 1.5
    spots = np.array([0, 1, 2, 3, 4, 63, 64, 96, 97, 98, 2046, 2047, 2048, 2049, 2050, 4316, 4317, 4318, 4319, 4320])
    assert lay.act[spots].all()
    targets = np.resize([0.0, 0.5 * FLOOR, -0.5 * FLOOR, 2.0 * FLOOR, -2.0 * FLOOR], len(spots))
    d = z0 + np.where(rng.random(lay.nflat) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, lay.nflat)
    d[spots] = z0 - targets
    d[lay.pad] = np.nan
    low = np.zeros(lay.nflat, dtype=bool)
    low[spots] = np.abs(targets) <= 0.5 * FLOOR
    ctx = _context(lay, gpu_lib)
    try:
        systems = [_system(rng, lay, False, 2), _system(rng, lay, True, 2), _system(rng, lay, True, 2)]
        for S, im in zip(systems, (0.0, 0.25 * FLOOR, 2.0 * FLOOR)):
            S.z = complex(z0, im)
        w = np.abs(systems[1].z - d[lay.act])
        assert np.all((w <= 0.6 * FLOOR) | (w >= 2.0 * FLOOR)) and (z0 - d[spots[0]]) == 0.0 and not np.signbit(z0 - d[spots[0]])
        floored = _check(ctx, lay, systems, d, FLOOR, "floor 1e-3")
        assert np.array_equal(floored[0], low) and np.array_equal(floored[1], low) and not floored[2].any() and low.sum() == 12
        d[spots[targets == 0.0]] = z0 - 0.5 * FLOOR
        floored = _check(ctx, lay, systems, d, 0.0, "floor 0")
        assert not any(f.any() for f in floored)
    finally:
        ctx.close()


# ---- 4. the solver's own aliasing, in lock-step with the reference -----------------------------------------------------------------------------
def test_eight_sweeps_in_lock_step(gpu_lib):
    """``_sweep``'s sequence with history = 3 on a real and a complex system against a host dense A = diag(d) + 0.05 N: each sweep
    downloads p, uploads A p as ap, calls the dots, forms the coefficients as ``_sweep`` does and calls the update; the update's p
    and ap become the newest stored pair, pn the next p, the window drops its oldest pair.  Before every call the reference is
    applied to the device's own downloaded state, so nothing accumulates and the bounds of a single call hold."""
    lay = Layout(*SMALL)
    rng = np.random.default_rng(600)
    na = int(lay.act.sum())
    d = np.full(lay.nflat, np.nan)
    d[lay.act] = rng.uniform(1.0, 3.0, na)
    A = np.diag(d[lay.act]) + 0.05 * rng.standard_normal((na, na))
    history, worst = 3, Worst()
    ctx = _context(lay, gpu_lib)
    try:
        dd = ctx.array(d)
        systems = []
        for cplx, z in ((False, 0.5), (True, 0.5 + 0.05j)):
            S = _system(rng, lay, cplx, 0, step=False)
            S.z, S.alpha, S.inv = complex(z), 0j, 1.0
            S.x[lay.act] = 0.0
            if cplx:
                S.r[lay.act] = S.r.real[lay.act]                  # (a real right-hand side, as xi is)
            systems.append(S)
        devs = [DeviceSystem(ctx, lay, S) for S in systems]
        nrm = _call_update(ctx, lay, _structs(devs), dd, FLOOR)
        for s, (S, dev) in enumerate(zip(systems, devs)):
            _compare(lay, S, d, FLOOR, None, nrm[s], dev.download(), worst, "start, system %d" % s)
        norm0 = last = np.sqrt(nrm)
        for sweep in range(8):
            for S, dev in zip(systems, devs):
                dev.v["p"], dev.v["pn"] = dev.v["pn"], None
                p = _cx((dev.v["p"][0].get(), dev.v["p"][1].get() if S.cplx else None))
                ap = np.full(lay.nflat, complex(np.nan, np.nan) if S.cplx else np.nan)
                ap[lay.act] = A @ p[lay.act]
                dev.v["ap"] = _upload(ctx, ap, S.cplx)
                nan = np.full(lay.nflat, np.nan)
                dev.v["pn"] = _upload(ctx, nan + (1j * nan if S.cplx else 0.0), S.cplx)
                S.struct_nh = len(dev.hp)
                S.hp, S.hq, S.g = [None] * S.struct_nh, [None] * S.struct_nh, [0j] * S.struct_nh
            rows = _call_dots(ctx, lay, _structs(devs))
            for S, row in zip(systems, rows):
                nh = S.nh
                g = row[0:2 * nh:2] + 1j * row[1:2 * nh:2]
                qq, qr = row[2 * nh], complex(row[2 * nh + 2], row[2 * nh + 3])
                left = qq - float((np.abs(g) ** 2).sum())
                assert np.isfinite(left) and left > 1e-12 * qq
                S.g, S.inv = list(g), 1.0 / np.sqrt(left)
                S.alpha = qr * S.inv
                assert S.cplx or not np.any(g.imag) and S.alpha.imag == 0.0
            before = []
            for S, dev in zip(systems, devs):             # the device's own state, which the references are applied to
                got = dev.download()
                before.append(P.SweepSystem(x=_cx(got["x"]), r=_cx(got["r"]), p=_cx(got["p"]), ap=_cx(got["ap"]),
                                            hp=[_cx(v) for v in got["hp"]], hq=[_cx(v) for v in got["hq"]], g=S.g, alpha=S.alpha,
                                            z=S.z, inv=S.inv))
                S.hp, S.hq = before[-1].hp, before[-1].hq       # (for the check that the update leaves them alone)
            nrm = _call_update(ctx, lay, _structs(devs), dd, FLOOR)
            for s, (S, dev) in enumerate(zip(systems, devs)):
                _compare(lay, S, d, FLOOR, rows[s], nrm[s], dev.download(), worst, "sweep %d, system %d" % (sweep, s), before[s])
                dev.hp.append(dev.v["p"])
                dev.hq.append(dev.v["ap"])
                if len(dev.hp) > history:
                    dev.hp.pop(0)
                    dev.hq.pop(0)
                dev.v["p"] = dev.v["ap"] = None
                assert len(dev.hp) == min(sweep + 1, history)
            print("   sweep %d: |r| / |xi| = %s" % (sweep + 1, np.sqrt(nrm) / norm0))
            assert np.all(np.sqrt(nrm) <= last * (1.0 + 1e-12))       # (r loses its component along a unit vector qh)
            last = np.sqrt(nrm)
        print("SWEEP %-34s len %6d  %4d systems  element error / bound %.3f  sum error / magnitude %.2e"
              % ("8 sweeps in lock-step, history 3", lay.nflat, 2, worst.element, worst.sum))
    finally:
        ctx.close()


# ---- 5. the sliding window through the solver ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [1, 2])
@pytest.mark.parametrize("hermitian", [True, False], ids=["8-fold", "non-hermitian"])
def test_solver_with_a_sliding_window(gpu_lib, hermitian, history):
    """(3,5), r_epsilon = 1e-10, Lambda of the dense reference, a window of one or two pairs: a real solve at z = 0 and 0.4 w1 and
    a complex one at 0.4 w1 + 0.05i.  Every value within the tolerance of test_solver_against_the_dense_resolvent, every system
    converged, and every system needed more sweeps than the window holds: the window slid."""
    from pymes_amd.solver.response import EOM_CCSD_Response
    ref = P.reference_problem(3, 5, 12, hermitian, 2)
    dense, w1, r_eps = ref["dense"], ref["w1"], 1e-10
    for omegas, gamma in (([0.0, 0.4 * w1], 0.0), ([0.4 * w1], 0.05)):
        s = EOM_CCSD_Response(3, r_epsilon=r_eps)
        s.history = history
        out = quiet(s.solve, ref["fd"], ref["Vd"], ref["t2"], ref["t1"], ref["ops"], omegas, gamma=gamma, lam=ref["lam"])
        print("SWEEP solver %s history %d gamma %.2f: sweeps %d, iterations %s, residuals %s"
              % ("8-fold" if hermitian else "non-hermitian", history, gamma, out["sweeps"], out["iterations"].ravel(),
                 out["residuals"].ravel()))
        for w, val in zip(omegas, out["response"]):
            z = complex(w, gamma) if gamma else w
            want = dense.response(z)
            for X_ in range(2):
                for Y_ in range(2):
                    assert abs(val[X_, Y_] - want[X_, Y_]) <= _tolerance(dense, z, r_eps, X_, Y_)
        assert out["converged"] and out["converged systems"].all() and out["residuals"].max() <= s.DRIFT * r_eps
        assert out["iterations"].min() > history


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_sweep_refusals_by_name(gpu_lib):
    """Each refusal leaves the library's allocations where they were and the context usable: the good call gives the same bits
    afterwards."""
    from pymes_amd.device import Context
    E = _lib.PymesError
    no, nv = 4, 12
    lay = Layout(no, nv, 48, 64, 64 + 48 * 48, 2)
    rng = np.random.default_rng(700)
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=WS)
    try:
        d = ctx.array(_diagonal(rng, lay))
        real, cplx = DeviceSystem(ctx, lay, _system(rng, lay, False, 1)), DeviceSystem(ctx, lay, _system(rng, lay, True, 1))
        start = DeviceSystem(ctx, lay, _system(rng, lay, False, 0, step=False))
        good = lambda: _call_dots(ctx, lay, _structs([real, cplx]))
        want = good()
        _call_update(ctx, lay, _structs([start]), d, FLOOR)
        many = (_lib.ResponseSystem * 4097)()
        for s in many:
            real.describe(s)
        held = _live()

        def refused(word, entries, change=None, n=None, off2=lay.off2, length=lay.nflat, floor=FLOOR, dev=real):
            for entry in entries:
                arr = many if n is not None else _structs([dev, cplx])
                if change:
                    change(arr[0])
                with pytest.raises(E, match=word):
                    if entry == "dots":
                        ctx.lib.call("pymes_response_dots", ctx.handle, len(arr) if n is None else n, C.byref(arr), off2, length,
                                     _lib.host_ptr(np.zeros((len(arr), _lib.RESPONSE_DOTS))))
                    else:
                        ctx.lib.call("pymes_response_update", ctx.handle, len(arr) if n is None else n, C.byref(arr),
                                     C.c_void_p(d.ptr), floor, off2, length, _lib.host_ptr(np.zeros(len(arr))))
                assert _live() == held and _same(good(), want), (word, entry)

        def field(name, index, value):
            def change(s):
                getattr(s, name)[index] = value
            return change

        def set_nh(value):
            def change(s):
                s.nh = value
            return change

        def hist(name, value):
            def change(s):
                getattr(s, name)[0][0] = value
            return change

        def coefficient(s):
            s.g[0][1] = 0.25
        both = ("dots", "update")
        refused("response_\\w+: the flat layout does not match", both, length=lay.nflat + 1)
        refused("response_\\w+: the flat layout does not match", both, off2=47, length=47 + 48 * 48)
        refused("1 <= n <= 4096 systems per call", both, n=0)
        refused("1 <= n <= 4096 systems per call", both, n=4097)
        refused("0 <= nh <= 32 stored directions", both, set_nh(33))
        refused("0 <= nh <= 32 stored directions", both, set_nh(-1))
        refused("a system is real .* or complex", ("update",), field("r", 1, cplx.v["r"][1].ptr))
        refused("a system is real .* or complex", both, field("z", 1, 0.125))
        refused("a real system with a complex coefficient", both, coefficient)
        refused("null stored direction", both, hist("hp", None))
        refused("response_dots: null vector", ("dots",), dev=start)
        refused("the floor must not be negative", ("update",), floor=-1.0)
        refused("the floor must not be negative", ("update",), floor=float("nan"))
    finally:
        ctx.close()
