"""The small algebra of one DIIS step on the device (pymes_diis_step: diis_step_kernel in kernels.hip) in every branch —
the Gauss-Jordan fast path, the inverse reached through the cyclic Jacobi fallback, the pseudo-inverse of a dependent
history and the refusal of non-finite overlaps — against the host step (pymes_diis_solve, csrc/diis_small.h) and the numpy
statement of diis.py:56-95 (the mixer's own ``_update_L`` / ``_solve``), with L prescribed through the 96-double state.
Each case's regime is checked in numpy before anything runs, with a margin of two from the thresholds |lambda| < 1e-12
and n max|L^-1| < 0.5e12.  The overlaps are exact: the x arrays are unit vectors."""
import contextlib
import io

import numpy as np
import pytest

from pymes_amd import _lib
from pymes_amd.device import Context
from pymes_amd.mixer.diis import DIIS
from tests.test_host_round2 import (check_device_resident_diis_gives_the_same_solve,
                                    check_mixer_near_singular_and_non_finite_subspace)

NL = 16          # length of the x / y / amplitude arrays


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def regimes(m):
    """(a) well conditioned, (b) inverse through the Jacobi fallback (a near-dependent pair: max|L^-1| ~ 1 / (2 lambda), so
    n max|L^-1| >= 1e12 with lambda >= 3e-12 needs n >= 7), (c) an exactly dependent pair, (d) NaN / +inf overlaps."""
    out = ["a"] + (["b"] if m >= 6 else []) + (["c"] if m >= 2 else []) + ["nan", "inf"]
    return out


def numpy_L(old, ov_types, m, was_full):
    """diis.py:56-80: the overlaps summed over the types in the reference's order, L built from the stored one."""
    ref = DIIS()
    ref.L = old.copy()
    ov = np.zeros(m)
    for part in ov_types:
        ov += part
    ref._update_L(ov, was_full)
    return ref


def design(m, was_full, regime, rng):
    """The new L's Gram block G (m x m) with the full-subspace quirk applied: row / column m-2 of G is not carried over."""
    E = rng.standard_normal((m, 12)) / np.sqrt(12)
    if regime == "b":
        # E[0], E[1] = p +- (s/2) d with d orthogonal to p and to every other row: (1, -1, 0, ..., 0) / sqrt(2) is an
        # eigenvector of L with lambda = s^2 / 2 = 3.3e-12 that sums to zero, so it does not enter c = -L^-1[:, n-1]
        Q, _ = np.linalg.qr(np.concatenate([E[1:], rng.standard_normal((1, 12))]).T)
        s = np.sqrt(2 * 3.3e-12)
        E[0], E[1] = E[1] + 0.5 * s * Q[:, -1], E[1] - 0.5 * s * Q[:, -1]
    G = E @ E.T
    if regime == "c":
        i, j = (0, m - 1) if not (was_full and m >= 4) else (0, 1)
        G[j, :] = G[i, :]
        G[:, j] = G[:, i]
        G[j, j] = G[i, i]
        if was_full and m in (2, 3):          # the quirk zeroes row m-2: the dependent rows must agree there too
            G[m - 2, m - 1] = G[m - 1, m - 2] = 0.0
            if m == 2:
                G[:] = 0.0
    if was_full and m >= 2:
        keep = G[m - 2, m - 1]
        G[m - 2, :] = G[:, m - 2] = 0.0
        G[m - 2, m - 1] = G[m - 1, m - 2] = keep
    return G


def inputs(m, ntypes, was_full, regime, rng):
    """(stored L, per-type overlaps [ntypes, m], (t, i) of the pair with a non-finite overlap or None) giving the designed
    L."""
    G = design(m, was_full, regime, rng)
    n = m + 1
    if was_full:                    # stored: m + 1 vectors' L; rows 0 and m-1 of it are dropped (the quirk), junk there
        old = np.zeros((n, n))
        J = rng.standard_normal((n, n))
        old[:] = J + J.T
        old[1:m - 1, 1:m - 1] = G[:m - 2, :m - 2]
    else:
        old = np.zeros((m, m))
        old[:m - 1, :m - 1] = G[:m - 1, :m - 1]
    old[-1, :-1] = old[:-1, -1] = -1.0
    old[-1, -1] = 0.0
    ov = G[:, m - 1].copy()
    ov_types = np.empty((ntypes, m))
    ov_types[0] = ov if ntypes == 1 else 0.3 * ov
    if ntypes == 2:
        ov_types[1] = ov - ov_types[0]
    odd = None                      # the pair with a non-finite overlap: every other overlap stays finite
    if regime == "nan":             # <NaN e_i, y> = NaN
        odd = (ntypes - 1, m // 2)
        ov_types[odd] = np.nan
    elif regime == "inf":           # <1e200 e_i, y> with y_i = 1e200 overflows to +inf
        odd = (0, m - 1)
        ov_types[odd] = np.inf
    return old, ov_types, odd


def numpy_regime(L):
    """(min |lambda|, n max|L^-1|) of the built L."""
    lam = np.abs(np.linalg.eigvalsh(L)).min()
    try:
        return lam, L.shape[0] * np.abs(np.linalg.inv(L)).max()
    except np.linalg.LinAlgError:          # exactly singular
        return lam, np.inf


def check_diis_step(lib):
    """m = 1..8, one and two amplitude types (npairs up to 16), with and without the full-subspace quirk.  The Jacobi fallback
    decides the branch; in case (b) the coefficients themselves then come from the LU solve of diis_small::finish, so the
    rotations are seen through the decision there and through the eigenvectors of the pseudo-inverse in case (c).  An
    infinite overlap must be refused like a NaN: the sweeps leave it on the diagonal, and before the fix the pseudo-inverse
    dropped it as an ordinary eigenvalue and returned zero coefficients."""
    rng = np.random.default_rng(2024)
    ctx = Context(2, 3, lib=lib)
    try:
        units = [ctx.array(np.eye(NL)[i]) for i in range(8)]
        amps = [ctx.array(rng.standard_normal(NL)) for _ in range(8)]
        amps_h = [a.get() for a in amps]
        seen = set()
        for m in range(1, 9):
            for ntypes in (1, 2):
                for was_full in (0, 1):
                    for regime in regimes(m):
                        key = (m, ntypes, was_full, regime)
                        n = m + 1
                        old, ov_types, odd = inputs(m, ntypes, was_full, regime, rng)
                        ref = numpy_L(old, ov_types, m, was_full)
                        L = ref.L
                        # the regime in numpy on the host, before anything runs, with a margin of two from both thresholds
                        if regime in ("a", "b", "c"):
                            lam_min, bound = numpy_regime(L)
                            if regime == "a":
                                assert lam_min >= 2e-12 and bound <= 0.25e12, (key, lam_min, bound)
                            elif regime == "b":
                                assert lam_min >= 3e-12 and bound >= 1e12, (key, lam_min, bound)
                            else:
                                assert lam_min <= 0.5e-12, (key, lam_min)
                            c_np = quiet(ref._solve_on_this_thread)
                        else:
                            assert not np.all(np.isfinite(L))
                        # the state: the stored L (pitch 9) and a step count
                        state = np.zeros(96)
                        state[0] = old.shape[0]
                        pad = np.zeros((9, 9))
                        pad[:old.shape[0], :old.shape[0]] = old
                        state[1:82] = pad.ravel()
                        state[92] = 5.0
                        # host: diis_small::step
                        host = state.copy()
                        lib.call("pymes_diis_solve", _lib.host_ptr(host),
                                 _lib.host_ptr(np.ascontiguousarray(ov_types.ravel())), ntypes, m, was_full)
                        # device: overlaps <x, y> with x a unit vector, the step, and the extrapolation reading the state
                        xs, ys = [], []
                        for t in range(ntypes):
                            y = rng.standard_normal(NL)
                            y[:m] = ov_types[t]
                            if odd is not None and odd[0] == t:
                                y[odd[1]] = 1e200 if regime == "inf" else 1.0
                            yd = ctx.array(y)
                            for i in range(m):
                                if odd == (t, i):
                                    x = np.zeros(NL)
                                    x[i] = 1e200 if regime == "inf" else np.nan
                                    xs.append(ctx.array(x))
                                else:
                                    xs.append(units[i])
                                ys.append(yd)
                        st = ctx.array(state)
                        ctx.diis_step(st, xs, ys, ntypes, m, was_full)
                        out = ctx.lincomb_dev(ctx.empty((NL,)), amps[:m], st.ptr + 8 * 82)
                        dev, got = st.get(), out.get()
                        for S in (host, dev):
                            assert S[0] == n and S[92] == 6.0, key
                            Ls = S[1:82].reshape(9, 9)
                            assert np.all(Ls[n:, :] == 0.0) and np.all(Ls[:, n:] == 0.0), key
                            # bit-identical L: the same additions in the same order in all three
                            assert np.array_equal(np.isnan(Ls[:n, :n]), np.isnan(L)), key
                            fin = ~np.isnan(L)
                            assert np.array_equal(Ls[:n, :n][fin].view(np.int64), L[fin].view(np.int64)), key
                            c = S[82:82 + n]
                            assert np.all(S[82 + n:91] == 0.0), key
                            if regime in ("a", "b"):
                                assert S[91] == 0.0, (key, S[91])
                                err = c - c_np
                                if regime == "b":
                                    # along the near-null eigenvector u the solve is determined only to eps / lambda (3e-5,
                                    # whichever solver); everything orthogonal to it to the usual 1e-9
                                    u = np.zeros(n)
                                    u[:2] = (1.0, -1.0)
                                    u /= np.sqrt(2.0)
                                    assert abs(u @ err) < 1e-3, (key, c, c_np)
                                    err = err - (u @ err) * u
                                assert np.abs(err).max() <= 1e-9 * np.abs(c_np).max(), (key, c, c_np)
                            elif regime == "c":
                                assert S[91] == 1.0, (key, S[91])
                                assert np.allclose(c, c_np, rtol=1e-9, atol=1e-11), (key, c, c_np)
                            else:
                                assert S[91] == 2.0, (key, S[91])
                                assert np.array_equal(c, np.eye(n)[n - 2]), (key, c)     # the newest vector alone
                        if regime in ("nan", "inf"):
                            assert np.array_equal(got, amps_h[m - 1]), key               # finite: the newest amplitudes
                        else:
                            c = dev[82:82 + m]
                            want = sum(c[k] * amps_h[k] for k in range(m))
                            assert np.abs(got - want).max() <= 1e-14 * np.abs(c).sum() * np.abs(amps_h).max(), key
                        seen.add(key)
        for full in (0, 1):                          # npairs = 16 in every branch
            assert {(8, 2, full, r) for r in ("a", "b", "c", "nan", "inf")} <= seen
    finally:
        ctx.close()


def test_diis_step_host_logic(hostsim_lib):
    check_diis_step(hostsim_lib)


@pytest.mark.gpu
def test_diis_step_gpu(gpu_lib):
    check_diis_step(gpu_lib)


@pytest.mark.gpu
def test_mixer_near_singular_and_non_finite_subspace_gpu(gpu_lib):
    check_mixer_near_singular_and_non_finite_subspace(gpu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["ccsd", "ccd"])
def test_device_resident_diis_gives_the_same_solve_gpu(gpu_lib, monkeypatch, solver):
    check_device_resident_diis_gives_the_same_solve(gpu_lib, monkeypatch, solver)
