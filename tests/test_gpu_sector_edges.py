"""GPU: the kernels of the momentum-sector path (csrc/kernels_sector.hip) at tile edges, past one trip of their loops and at their
caps.  The sibling modules (test_gpu_sector_cc / _triples / _lambda / _density / _gf) meet them at electron-gas shapes only: nv in
{6, 12, 30, 50, 86}, no in {7, 27}, Krylov steps j <= 100.  SectorTables / TriplesTables and the numpy restatements take any list
of distinct integer vectors, so here the same references (tests/_sector_triples_reference.py, _sector_lambda_reference.py,
_sector_gf_reference.cgs2_step, numpy products, math.fsum) are met on the synthetic list of tests/_sector_lattices.line_lattice
and on synthetic row and task tables, at the smallest shapes that cross each boundary:

  (T), Lambda-(T)   line_lattice(no, nv): the lookup box is degenerate on two axes and K - k_a - k_b leaves it on both sides
    (3,1), (3,2)      nv below the 8 rows of a thread column (every row ty + 8 q of most threads outside); nv = 1: no live triple
    (4,7), (8,8)      nv = 7 < 8 and nv = 8: the last thread row inside / the first q = 1 row outside
    (8,31) ... (8,65) nv = 31, 32, 33, 64, 65: one tile less one, exactly one, one past; two tiles exactly, one past
    (2,513)           17 x 17 = 289 tiles: the second trip of ``for (q0 = 0; q0 < ntiles; q0 += 256)`` in sector_triples_sum_kernel
    (73,4)            67 525 triples: ``nb = min(fit, 65535)`` binds, a second batch of 1 990 starts after a full grid; a range
                      that starts at 65 000 straddles the boundary
  arnoldi_step      len 1000, j = 255 / 256 / 257 / 511: the second trip of ``for (i = tid; i <= j; i += 256)`` in arn_reduce_rows,
                      the h1[] copy and the hess[] column store; hs[] up to its cap; 32 grid rows of the dots kernel
    len 4099, j = 511 the same with 17 chunks
    len 2; 64, 65     the smallest vector; one row of lanes exactly and one past
    len 256, 512      no ragged last chunk
    len 70001         274 small chunks: the second trip of ``for (c = tid; c < nch; c += 256)`` in arn_block_total
    len 262143/262144 1024 small chunks with a last one ragged by one / the switch: exactly 256 large chunks
    len 262144, j = 256   the large chunk past one trip of the row loops (a Householder basis; a QR of that size is too slow)
    len 1000, j = 300 breakdown past one trip: status 301
  xdiag, gamma      synthetic direct layouts, rows of 0 ... 70 elements between NaN gaps, (no, nv) =
    (1,1)             one row, one block of each kernel
    (3,61), (3,62)    no + nv = 64: exactly one 64-thread block of sector_xdiag_kernel / sector_gamma_kernel, and one past
    (17,16)           272 rows: a second 256-row block of sector_rowsum_kernel / sector_rowscale_kernel
    (40,90)           3 600 rows, three blocks of 64 orbitals
  sector_gemm       m in {31, 32, 33, 64}, n in {15, 16, 17, 32}, k in {63, 64, 65, 127, 128, 129, 192}: at k = 64, 128, 192 the
                      prefetch test ``k0 + 64 < t.k`` turns false exactly at a panel boundary

The error bounds of the triples and the Arnoldi step are the project's (1e-12 sum|terms|; 1e-13 |w|, subspace.ORTH_TOL, 1e-14); those
of the row kernels are derived in their test (number of roundings x 2^-53 x sum of magnitudes) against exact references.

Not covered: j = 511 with the large chunk (a basis of 1 GB); the far sides of the refusals ``nv > 2^20`` and ``ntiles > 2^31``
(operands of terabytes); the IP / EA prepare kernel on synthetic lists (its restatement needs the ladder families, which only the
electron-gas builder makes).  ``pytest -s`` prints one line per case with the observed errors in units of their bounds;
profiles/sector_edges/gpu_test_errors.txt keeps one such run."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from pymes_amd.solver import subspace
from tests import _sector_gf_reference as gf
from tests import _sector_lambda_reference as sl
from tests import _sector_triples_reference as tr
from tests import _triples_reference as R
from tests._sector_lattices import line_lattice
from tests.test_gpu_sector_cc import ragged_case
from tests.test_gpu_sector_gf import run_step, untouched
from tests.test_gpu_sector_ipea import bits
from tests.test_gpu_sector_lambda import run_lambda_kernel, two_sided_operands
from tests.test_gpu_sector_triples import random_operands, run_kernel

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
KERNELS = ("t", "lambda")


def record(line):
    """The observed differences: `pytest -s` prints them, and profiles/sector_edges/gpu_test_errors.txt keeps one such run."""
    print(line)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from pymes_amd.device import Context
    c = Context(1, 1, lib=gpu_lib)
    yield c
    c.close()


# ---- 1. (T) and Lambda-(T) on the line lattice --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(no, nv):
    return tr.tables_for(*line_lattice(no, nv))


@functools.lru_cache(maxsize=None)
def triples_case(which, no, nv, begin=0):
    """(triples tables, operands in the order of the run function, numpy's values and sums of |terms| of the triples from
    ``begin`` on), computed once and read-only."""
    tt = lattice(no, nv)[1]
    if which == "t":
        ops = random_operands(tt, 31)
        eps, Tc, Vv, Vo = ops
        want, scale = tr.per_triple(tt, eps, Vv, Vo, Tc, begin)
    else:
        ops = two_sided_operands(tt)
        eps, Tc, Lc, VvR, VoR, VvL, VoL = ops
        want, scale = sl.per_triple(tt, eps, VvR, VoR, VvL, VoL, Tc, Lc, begin)
    for x in ops + (want, scale):
        x.setflags(write=False)
    return tt, ops, want, scale


def run(ctx, which, tt, ops, lo, hi, triples_in_ws=None):
    """(sum, per-triple values) of pymes_sector_triples / pymes_sector_triples_lambda over [lo, hi)."""
    call = run_kernel if which == "t" else run_lambda_kernel
    return call(ctx, tt, *ops, lo, hi, triples_in_ws=triples_in_ws)


def check_values(label, e, got, want, scale):
    """The assertions of test_kernel_matches_the_numpy_restatement and its two-slab twin; returns the live triples."""
    live = scale > 0
    ratio = (np.abs(got - want)[live] / scale[live]).max() if live.any() else 0.0
    record(f"{label}: {len(got)} triples, {int(live.sum())} live, worst |d| / sum|terms| = {ratio:.2e} = {ratio / 1e-12:.2e} of the bound")
    assert (np.abs(got - want) <= 1e-12 * scale).all()
    assert np.array_equal(bits(got[~live]), np.zeros(int((~live).sum()), dtype=np.int64))           # an exact +0.0
    if e is not None:
        assert e == tr.ordered_sum(got)
    return live


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("no,nv,live", [(3, 1, 0), (3, 2, 2), (4, 7, 20), (8, 8, 100), (8, 31, 120), (8, 32, 120), (8, 33, 120),
                                        (8, 64, 120), (8, 65, 120)])
@pytest.mark.parametrize("which", KERNELS)
def test_triples_kernels_on_the_line_lattice(ctx, which, no, nv, live):
    tt, ops, want, scale = triples_case(which, no, nv)
    assert (tt.no, tt.nv) == (no, nv) and tt.box.tolist() == [0, 0, 0, no + nv, 1, 1]
    n = R.n_triples(no)
    first = run(ctx, which, tt, ops, 0, n)
    assert len(want) == n and len(first[1]) == n
    assert int(check_values(f"triples {which} ({no},{nv})", *first, want, scale).sum()) == live
    assert same_bits(first, run(ctx, which, tt, ops, 0, n))
    if no == 8 and nv > 8:
        assert 0.035 < (tt.m_of >= 0).mean() < 0.09                  # 4 to 8 % of the hole terms are live
    if live == 0:
        assert first[0] == 0.0 and not math.copysign(1.0, first[0]) < 0


@pytest.mark.parametrize("which", KERNELS)
def test_triples_sum_kernel_past_256_tiles(ctx, which):
    """(2,513): 289 partials per triple.  One triple per batch moves every slab, partial and value to the front of the workspace."""
    tt, ops, want, scale = triples_case(which, 2, 513)
    assert (-(-tt.nv // 32)) ** 2 == 289
    first = run(ctx, which, tt, ops, 0, 4)
    assert int(check_values(f"triples {which} (2,513)", *first, want, scale).sum()) == 4
    assert same_bits(first, run(ctx, which, tt, ops, 0, 4))
    assert same_bits(first, run(ctx, which, tt, ops, 0, 4, triples_in_ws=1))


@pytest.fixture(scope="module")
def full_grid(ctx):
    """The whole range of (73,4) with workspace for every triple, once per kernel: two batches, 65 535 and 1 990 triples."""
    cache = {}

    def get(which):
        if which not in cache:
            tt, ops = triples_case(which, 73, 4, 63000)[:2]
            cache[which] = run(ctx, which, tt, ops, 0, R.n_triples(73))
            cache[which][1].setflags(write=False)
        return cache[which]
    return get


@pytest.mark.parametrize("which", KERNELS)
def test_triples_second_batch_after_a_full_grid(ctx, full_grid, which):
    """(73,4): numpy on [63 000, 67 525) (the whole range would take it 8 s), a device run in batches of 4 096 on all of it."""
    lo, n = 63000, 67525
    tt, ops, want, scale = triples_case(which, 73, 4, lo)
    assert R.n_triples(73) == n and n > 65535
    e, got = full_grid(which)
    live = check_values(f"triples {which} (73,4) [{lo}, {n})", None, got[lo:], want, scale)
    assert int(live[65535 - lo:].sum()) >= 100                       # the second batch has something to get wrong
    record(f"triples {which} (73,4): {int(live[65535 - lo:].sum())} live triples at t >= 65535, {np.count_nonzero(got)} values of "
           f"the whole range are not zero")
    assert np.count_nonzero(got) <= 3602                             # no more than there are live triples (numpy, whole range)
    assert e == tr.ordered_sum(got)
    assert same_bits((e, got), run(ctx, which, tt, ops, 0, n, triples_in_ws=4096))


@pytest.mark.parametrize("which", KERNELS)
def test_triples_range_that_straddles_the_full_grid(ctx, full_grid, which):
    """t_begin = 65 000 > 0 with workspace for the whole range: one batch that the boundary 65 535 lies inside of."""
    lo, n = 65000, 67525
    tt, ops = triples_case(which, 73, 4, 63000)[:2]
    e, got = run(ctx, which, tt, ops, lo, n)
    whole = full_grid(which)[1]
    assert np.array_equal(bits(got), bits(whole[lo:])) and np.count_nonzero(got) > 100
    assert e == tr.ordered_sum(got)


# ---- 2. pymes_sector_arnoldi_step ---------------------------------------------------------------------------------------------------
def check_step(ctx, V, w, variants=True):
    """One step on the orthonormal rows V and w against gf.cgs2_step, with the assertions and bounds of
    test_gpu_sector_gf.test_step_against_numpy_cgs2; ``variants``: a repeat, and another pitch, ldh and row count."""
    j, length = V.shape[0] - 1, V.shape[1]
    pitch = -(-length // 32) * 32 + 32
    col, nrm, v = gf.cgs2_step(V, w)
    got, hess, flag = run_step(ctx, V, w, pitch, j + 2)
    wn = np.linalg.norm(w)
    new = got[j + 1, :length]
    e_col = max(np.abs(hess[:j + 1, j] - col).max(), abs(hess[j + 1, j] - nrm))
    e_orth, e_norm = np.abs(V @ new).max(), abs(np.linalg.norm(new) - 1.0)
    record(f"step len {length} j {j}: |column - numpy| / |w| = {e_col / wn:.2e} = {e_col / wn / 1e-13:.2e} of the bound, max|V v| = "
           f"{e_orth:.2e} = {e_orth / subspace.ORTH_TOL:.2e} of the bound, ||v| - 1| = {e_norm:.2e} = {e_norm / 1e-14:.2e} of the bound, "
           f"|v - numpy| = {np.abs(new - v).max():.2e}")
    assert np.all(np.isfinite(new)) and np.all(np.isfinite(hess[:, j]))
    assert e_col <= 1e-13 * wn
    assert e_orth <= subspace.ORTH_TOL
    assert e_norm <= 1e-14
    assert flag == 0
    assert untouched(got, V, w, j, length)
    assert np.isnan(hess[:, :j]).all()                                    # the other columns are not written
    if not variants:
        return
    again, hess2, _ = run_step(ctx, V, w, pitch, j + 2)
    wide, hess3, _ = run_step(ctx, V, w, pitch + 64, j + 5, extra_ldh=3)
    assert untouched(wide, V, w, j, length)
    assert np.isnan(hess3[:, :j]).all() and np.isnan(hess3[:, j + 1:]).all()
    for other, h in ((again, hess2), (wide, hess3)):
        assert np.array_equal(bits(other[j + 1, :length]), bits(new))
        assert np.array_equal(bits(h[:, j]), bits(hess[:, j]))


STEPS = [(1000, 255), (1000, 256), (1000, 257), (1000, 511), (4099, 511), (2, 0), (64, 0), (64, 33), (65, 0), (65, 33), (256, 1),
         (256, 100), (512, 1), (512, 100), (70001, 0), (70001, 33), (262143, 1), (262144, 1)]


@pytest.mark.parametrize("length,j", [(n, j) for n, j in STEPS if j + 2 <= n])     # a basis holds at most len orthonormal rows
def test_step_past_one_trip_and_at_chunk_edges(ctx, length, j):
    """Bases from numpy's QR of seeded matrices, as in test_gpu_sector_gf."""
    rng = np.random.default_rng(1000 * length + j)
    V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((length, j + 1)))[0].T)
    check_step(ctx, V, rng.standard_normal(length) * 3.0)


def test_step_large_chunk_past_one_trip(ctx):
    """len = 262 144 (256 chunks of 1024), j = 256: the first 257 rows of the Householder reflector 1 - 2 u u^T, orthonormal to
    rounding.  One run: the basis is 0.54 GB."""
    length, j = 262144, 256
    rng = np.random.default_rng(length + j)
    u = rng.standard_normal(length)
    u /= np.linalg.norm(u)
    V = np.multiply.outer(-2.0 * u[:j + 1], u)
    V[np.arange(j + 1), np.arange(j + 1)] += 1.0
    assert np.abs(V @ V.T - np.eye(j + 1)).max() <= 1e-14
    check_step(ctx, V, rng.standard_normal(length) * 3.0, variants=False)


def test_step_breakdown_past_one_trip(ctx):
    """len 1000, j = 300, w in the span of the rows: the assertions of test_gpu_sector_gf.test_step_breakdown."""
    length, j = 1000, 300
    rng = np.random.default_rng(7 + length + j)
    pitch = -(-length // 32) * 32 + 32
    V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((length, j + 1)))[0].T)
    w = V.T @ rng.standard_normal(j + 1)
    got, hess, flag = run_step(ctx, V, w, pitch, j + 2)
    assert bits(hess[j + 1:j + 2, j])[0] == 0
    assert np.array_equal(bits(got[j + 1, :length]), np.zeros(length, dtype=np.int64))               # +0.0, not -0.0
    assert flag == j + 1 == 301
    e_col = np.abs(hess[:j + 1, j] - V @ w).max() / np.linalg.norm(w)
    record(f"breakdown len {length} j {j}: |column - numpy| / |w| = {e_col:.2e} = {e_col / 1e-13:.2e} of the bound")
    assert e_col <= 1e-13
    assert untouched(got, V, w, j, length)
    assert np.isnan(hess[:, :j]).all()
    assert run_step(ctx, V, w, pitch, j + 2, status=3)[2] == 3
    assert run_step(ctx, V, rng.standard_normal(length), pitch, j + 2, status=3)[2] == 3
    zero = run_step(ctx, V, np.zeros(length), pitch, j + 2)                                          # H v = 0: nothing new either
    assert zero[2] == j + 1 and bits(zero[1][j + 1:j + 2, j])[0] == 0
    assert np.array_equal(bits(zero[0][j + 1, :length]), np.zeros(length, dtype=np.int64))


# ---- 3. the row kernels alone: pymes_sector_xdiag, pymes_sector_gamma -----------------------------------------------------------------
ROW_SHAPES = [(1, 1), (3, 61), (3, 62), (17, 16), (40, 90)]


def two_product(x, y):
    """(p, e) with p + e = x y exactly (Veltkamp's split and Dekker's product; nothing here comes near over- or underflow)."""
    def split(a):
        c = 134217729.0 * a
        hi = c - (c - a)
        return hi, a - hi
    p = x * y
    (xh, xl), (yh, yl) = split(x), split(y)
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


class DirectLayout:
    """A synthetic direct layout: no nv rows of seeded lengths 0 ... 70 (a 70, a 1 and a 0 among them where there are three
    rows), one to five NaN in front of, between and behind the rows; row_of a seeded permutation of a no + i, ai_of its inverse."""

    def __init__(self, ctx, no, nv, seed):
        from pymes_amd.solver.ueg_cc import upload_raw
        rng = np.random.default_rng(seed)
        self.no, self.nv, self.rows = no, nv, no * nv
        self.len = rng.integers(0, 71, self.rows)
        where = rng.permutation(self.rows)[:3]
        self.len[where] = (70, 1, 0)[:len(where)]
        gap = rng.integers(1, 6, self.rows + 1)
        self.start = gap[0] + np.concatenate(([0], np.cumsum(self.len + gap[1:])))[:-1]
        self.size = int(gap[0] + (self.len + gap[1:]).sum())
        self.row_of = rng.permutation(self.rows)
        self.ai_of = np.argsort(self.row_of)
        assert np.array_equal(self.row_of[self.ai_of], np.arange(self.rows))
        self.row = np.repeat(np.arange(self.rows), self.len)                       # the row of every valid element, row after row
        self.idx = self.start[self.row] + np.arange(len(self.row)) - np.repeat(np.cumsum(self.len) - self.len, self.len)
        self.gaps = np.ones(self.size, dtype=bool)
        self.gaps[self.idx] = False
        assert self.gaps.sum() == gap.sum() and (np.diff(self.start) > self.len[:-1]).all()
        self.rng = rng
        self.dev = [upload_raw(ctx, np.ascontiguousarray(x, dtype=np.int64)) for x in (self.start, self.len, self.row_of, self.ai_of)]

    def arena(self):
        x = np.full(self.size, np.nan)
        x[self.idx] = self.rng.standard_normal(len(self.idx))
        return x

    def check_row_sums(self, label, s, x, y):
        """s[g] = fma(x_c, y_c, .) in ascending c: len[g] roundings, |s - sum| <= len 2^-53 sum|x y| for every len (Jeannerod and
        Rump's bound of a recursive dot product has no higher-order term); the exact sum from the exact products by math.fsum,
        the device's value inside it, so that the reference adds no rounding of its own.  A row without elements: +0.0."""
        worst = 0.0
        for g in range(self.rows):
            at = slice(self.start[g], self.start[g] + self.len[g])
            p, e = two_product(x[at], y[at])
            err, bound = abs(math.fsum([*p, *e, -s[g]])), self.len[g] * EPS * math.fsum(np.abs(p))
            assert err <= bound, (g, self.len[g], err, bound)
            if self.len[g] == 0:
                assert bits(s[g:g + 1])[0] == 0
            worst = max(worst, err / bound if bound else 0.0)
        record(f"{label}: {self.rows} row sums, lengths {self.len.min()}..{self.len.max()}, worst |d| / (len 2^-53 sum|x y|) = {worst:.2e}")

    def check_orbital_sums(self, label, got, s, eps, w, sign_oo, sign_vv):
        """got[i] = eps[i] + sign_oo w sum_a s[row(a,i)], got[no + a] = eps[no + a] + sign_vv w sum_i s[row(a,i)] from the
        device's own s: the terms added one after the other (terms - 1 roundings), times w (exact: w is a power of two), plus eps
        (one rounding, or none where eps = 0), i.e. a recursive sum of terms + 1 numbers; (terms + 2) 2^-53 (|eps| + |w| sum|s|)
        bounds it with room for a compiler that fuses nothing.  The reference: math.fsum with the device's value inside."""
        no, nv = self.no, self.nv
        sr = s[self.row_of].reshape(nv, no)                                         # sr[a,i] = s[row(a,i)]
        worst = 0.0
        for p in range(no + nv):
            terms, sign = (sr[:, p], sign_oo) if p < no else (sr[p - no, :], sign_vv)
            err = abs(math.fsum([eps[p], *(sign * w * terms), -got[p]]))
            bound = (len(terms) + 2) * EPS * (abs(eps[p]) + w * math.fsum(np.abs(terms)))
            assert err <= bound, (p, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
        record(f"{label}: {no} + {nv} orbital sums, worst |d| / ((terms + 2) 2^-53 (|eps| + |w| sum|s|)) = {worst:.2e}")


@pytest.fixture(scope="module")
def layouts(ctx):
    """(layout, four arenas on it) per shape, made once: Tt, W1, D, Ex of the xdiag test; the first two are x, y of gamma."""
    cache = {}

    def get(no, nv):
        if (no, nv) not in cache:
            lay = DirectLayout(ctx, no, nv, 1000 * no + nv)
            cache[no, nv] = (lay, [lay.arena() for _ in range(4)])
        return cache[no, nv]
    return get


@pytest.mark.parametrize("w", [0.5, 1.0])
@pytest.mark.parametrize("no,nv", ROW_SHAPES)
def test_xdiag_against_exact_sums(ctx, layouts, no, nv, w):
    """pymes_sector_xdiag on a synthetic layout.  The row sums s and x are read back from the workspace (rows doubles, then
    no + nv), so each of the three kernels is held against the exact result of its own inputs:
      s    DirectLayout.check_row_sums
      x    DirectLayout.check_orbital_sums, x_oo = eps + w sum_a s, x_vv = eps - w sum_i s
      Ex   Ex0 + f D with f = x_vv[a] - x_oo[i] rounded (one rounding, the same in numpy) and one fma (one rounding): within
           2 2^-53 (|Ex0| + |f D|) of the exact Ex0 + f D, taken from the exact product and an exact sum
    Everything between the rows and behind the workspace keeps its NaN; identical calls give identical bits."""
    lay, (Tt, W1, D, Ex0) = layouts(no, nv)
    rows, n = lay.rows, no + nv
    eps = np.random.default_rng(no + nv).standard_normal(n)
    dev = [ctx.array(x) for x in (Tt, W1, D, eps)]
    outs = []
    for _ in range(2):
        Ex, ws = ctx.array(Ex0), ctx.array(np.full(rows + n + 5, np.nan))
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(dev[0].ptr), C.c_void_p(dev[1].ptr), C.c_void_p(dev[2].ptr),
                     C.c_void_p(Ex.ptr), C.c_void_p(dev[3].ptr), w, no, nv, *[C.c_void_p(x.ptr) for x in lay.dev], C.c_void_p(ws.ptr))
        outs.append((Ex.get(), ws.get()))
    got, ws = outs[0]
    s, x = ws[:rows], ws[rows:rows + n]
    label = f"xdiag ({no},{nv}) w = {w}"
    assert np.isnan(ws[rows + n:]).all() and np.all(np.isfinite(ws[:rows + n]))
    lay.check_row_sums(label, s, Tt, W1)
    lay.check_orbital_sums(label, x, s, eps, w, 1.0, -1.0)
    ai = lay.ai_of[lay.row]
    f = x[no + ai // no] - x[ai % no]
    p, e = two_product(f, D[lay.idx])
    total = p + Ex0[lay.idx]                                             # (total, rest): the exact p + Ex0 (Knuth's two-sum)
    back = total - p
    rest = (p - (total - back)) + (Ex0[lay.idx] - back)
    err, bound = np.abs((total - got[lay.idx]) + (rest + e)), 2 * EPS * (np.abs(Ex0[lay.idx]) + np.abs(p))
    record(f"{label}: {len(lay.idx)} elements of Ex, worst |d| / (2 2^-53 (|Ex0| + |f D|)) = {(err / bound).max():.2e}")
    assert (err <= bound).all()
    assert np.array_equal(bits(got[lay.gaps]), bits(Ex0[lay.gaps])) and np.isnan(got[lay.gaps]).all()
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("no,nv", ROW_SHAPES)
def test_gamma_against_exact_sums(ctx, layouts, no, nv):
    """pymes_sector_gamma: rho[g] = sum_c x[g,c] y[g,c] (read back from the workspace), gamma[no + a] = sum_i rho[row(a,i)],
    gamma[i] = -sum_a rho[row(a,i)], with the bounds of the xdiag test (eps = 0, w = 1)."""
    lay, (x, y, _, _) = layouts(no, nv)
    rows, n = lay.rows, no + nv
    dx, dy = ctx.array(x), ctx.array(y)
    outs = []
    for _ in range(2):
        gamma, ws = ctx.array(np.full(n + 3, np.nan)), ctx.array(np.full(rows + 5, np.nan))
        ctx.lib.call("pymes_sector_gamma", ctx.handle, C.c_void_p(dx.ptr), C.c_void_p(dy.ptr), no, nv,
                     *[C.c_void_p(t.ptr) for t in lay.dev[:3]], C.c_void_p(gamma.ptr), C.c_void_p(ws.ptr))
        outs.append((gamma.get(), ws.get()))
    gamma, ws = outs[0]
    assert np.isnan(gamma[n:]).all() and np.isnan(ws[rows:]).all() and np.all(np.isfinite(gamma[:n]))
    lay.check_row_sums(f"gamma ({no},{nv})", ws[:rows], x, y)
    lay.check_orbital_sums(f"gamma ({no},{nv})", gamma[:n], ws[:rows], np.zeros(n), 1.0, -1.0, 1.0)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(bits(a), bits(b))


# ---- 4. sector_gemm at panel boundaries -----------------------------------------------------------------------------------------------
def test_sector_gemm_at_panel_boundaries(ctx):
    """Every (m, n, k) of {31, 32, 33, 64} x {15, 16, 17, 32} x {63, 64, 65, 127, 128, 129, 192} once, and every (m, n) four more
    times at k = 64 and at k = 128, so that the seeded transposes and beta values of ragged_case cover all eight combinations
    there (asserted on the table); the assertions of test_gpu_sector_cc.test_sector_gemm_against_numpy."""
    from pymes_amd.solver.sectors import TRANS_A, TRANS_B
    from pymes_amd.solver.ueg_cc import Tasks
    ms, ns, ks = (31, 32, 33, 64), (15, 16, 17, 32), (63, 64, 65, 127, 128, 129, 192)
    sizes = [(m, n, k) for m in ms for n in ns for k in ks] + [(m, n, k) for k in (64, 128) for m in ms for n in ns] * 4
    tasks, A, B, Cm, want, written, bound = ragged_case(5, len(sizes), forced=tuple(zip(*sizes)))
    assert np.array_equal(np.stack([tasks[nm] for nm in "mnk"], axis=1), np.array(sizes))
    for k in (64, 128):
        t = tasks[tasks["k"] == k]
        seen = set(zip((t["flags"] & TRANS_A != 0).tolist(), (t["flags"] & TRANS_B != 0).tolist(), (t["beta"] != 0).tolist()))
        assert len(seen) == 8, (k, sorted(seen))
    table = Tasks(ctx, tasks, len(A), len(B), len(Cm))
    dA, dB = ctx.array(A), ctx.array(B)
    outs = []
    for _ in range(2):
        dC = ctx.array(Cm)
        table.run(dA, dB, dC)
        outs.append(dC.get())
    got = outs[0]
    assert np.array_equal(np.isnan(got), ~written)                   # nothing outside the declared output blocks is touched,
    assert np.array_equal(bits(got[~written]), bits(Cm[~written]))   # ... bit for bit
    err = np.abs(got[written] - want[written])
    record(f"gemm {len(sizes)} blocks, {table.tiles} tiles: worst error / bound = {(err / bound[written]).max():.2e}")
    assert (err <= bound[written]).all()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))              # identical calls give identical bits
