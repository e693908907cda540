"""The shared block Davidson and orthonormalisers (pymes_amd/solver/subspace.py) on the host simulator, with a dense numpy matrix
as the operator: no GPU and no sigma kernel (the IP / EA and left builds are refusing stubs in the simulator, so the drivers that
run this loop are tested on the GPU only)."""
import functools

import numpy as np
import pytest

from pymes_amd.device import Context, PymesError
from pymes_amd.solver import subspace as S

N1, N2 = 6, 90                       # singles, doubles: off2 = 32, nflat = 122, m = 96 active elements
M = N1 + N2
SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _problem(seed):
    """(A, d, eigenvalues ascending): a diagonally dominant non-symmetric matrix with a real, well separated spectrum."""
    rng = np.random.default_rng(seed)
    d = rng.permutation(np.arange(1., M + 1.))
    A = np.diag(d) + 0.002 * rng.uniform(-1, 1, (M, M))
    lam = np.linalg.eigvals(A)
    assert np.abs(lam.imag).max() == 0
    lam = np.sort(lam.real)
    assert np.diff(lam).min() > 0.5
    for x in (A, d, lam):
        x.setflags(write=False)
    return A, d, lam


class _Dense:
    """The callbacks of ``block_davidson`` for a dense matrix on the active elements of the flat layout."""

    def __init__(self, ctx, A, d):
        self.ctx, self.A = ctx, A
        self.lay = S.FlatLayout(ctx, (N1,), (N2,))
        assert (self.lay.off2, self.lay.nflat) == (32, 122)
        self.d = self.flat(d)
        self.applied = 0

    def active(self, vec):
        x = vec.get()
        return np.concatenate([x[:N1], x[self.lay.off2:]])

    def pad(self, vec):
        return vec.get()[N1:self.lay.off2]

    def flat(self, a):
        """A flat device vector with active elements ``a`` and a zero pad."""
        out = self.lay.padded()
        self.lay.part1(out).set(np.ascontiguousarray(a[:N1]))
        self.lay.part2(out).set(np.ascontiguousarray(a[N1:]))
        return out

    def apply_flat(self, vecs):
        self.applied += len(vecs)
        return [self.flat(self.A @ self.active(u)) for u in vecs]

    def correction(self, ss, rs, w, d, shift, qs):
        res, nrm, dd = np.zeros(len(rs)), np.zeros(len(rs)), self.active(d)
        for n, (s, r, q) in enumerate(zip(ss, rs, qs)):
            sa, ra = self.active(s), self.active(r)
            z = sa - w[n] * ra
            q.copy_from(self.flat(z / (w[n] - dd + shift)))
            res[n], nrm[n] = z @ z, ra @ ra
        return res, nrm

    def start(self, d, k):
        """Unit vectors on the k smallest diagonal elements."""
        return [self.flat(np.eye(M)[p]) for p in np.argsort(d, kind="stable")[:k]]

    def run(self, start, **kw):
        kw = dict(dict(max_dim=24, max_iter=30, r_epsilon=1e-10), **kw)
        return S.block_davidson(self.ctx, self.lay, self.apply_flat, self.correction, self.d, start, 3, **kw)


@pytest.fixture
def ctx(hostsim_lib):
    c = Context(2, 3, lib=hostsim_lib)
    yield c
    c.close()


def test_flat_layout(ctx):
    lay = S.FlatLayout(ctx, (3, 2), (3, 3, 2, 2))
    assert (lay.n1, lay.n2, lay.off2, lay.nflat) == (6, 36, 32, 68)
    u = lay.unit(4)
    want = np.zeros(68)
    want[4] = 1.0
    assert np.array_equal(u.get(), want)
    assert lay.part1(u).get().shape == (3, 2) and lay.part1(u).get()[2, 0] == 1.0 and lay.part2(u).get().shape == (3, 3, 2, 2)
    v = ctx.array(np.arange(1., 69.))
    assert lay.zero_pad(v) is v
    got = v.get()
    assert np.array_equal(got[6:32], np.zeros(26)) and np.array_equal(got[:6], np.arange(1., 7.)) and got[32] == 33.0
    assert np.array_equal(lay.padded().get()[6:32], np.zeros(26)) and lay.empty().shape == (68,)
    # no pad at all: nothing is touched
    full = S.FlatLayout(ctx, (32,), (4,))
    assert (full.off2, full.nflat) == (32, 36)
    w = ctx.array(np.arange(1., 37.))
    assert np.array_equal(full.zero_pad(w).get(), np.arange(1., 37.))


@pytest.mark.parametrize("seed", SEEDS)
def test_lowest_roots_collapse_and_targets(ctx, seed):
    A, d, lam = _problem(seed)
    # 1. the three lowest roots
    op = _Dense(ctx, A, d)
    out = op.run(op.start(d, 3))
    assert out.converged and out.passes < 30 and len(out.history) == out.passes
    assert np.abs(out.theta - lam[:3]).max() < 1e-9 and np.array_equal(out.w, out.theta)
    assert np.array_equal(out.history[-1], out.theta) and np.all(out.rel < 1e-10)
    for x in out.rz + out.sz:
        assert np.array_equal(op.pad(x), np.zeros(26))
    assert op.applied <= 3 * out.passes               # sigma for the new vectors only
    assert out.max_basis == op.applied <= 24
    # 2. the same with a collapse: the basis never holds more than max_dim vectors
    small = _Dense(ctx, A, d)
    col = small.run(small.start(d, 3), max_dim=6)
    assert col.converged and col.passes < 30 and col.max_basis <= 6 and small.applied > 6
    assert np.abs(col.theta - lam[:3]).max() < 1e-9
    # 3. the left problem from the right vectors: the Ritz pair nearest each target, residuals at the target
    left = _Dense(ctx, A.T, d)
    lo = left.run([op.lay.empty().copy_from(x) for x in out.rz], targets=out.theta)
    assert lo.converged and lo.passes < 30
    assert np.array_equal(lo.w, out.theta)
    for n in range(3):
        l = left.active(lo.rz[n])
        assert np.linalg.norm(A.T @ l - lo.w[n] * l) / np.linalg.norm(l) < 1e-9


def test_refuse_complex(ctx):
    A, d, _ = _problem(1)
    A = A.copy()
    p, q = np.argsort(d)[:2]                           # a rotation block on the two lowest diagonal positions: 1 +- 5i
    A[np.ix_([p, q], [p, q])] = [[1., 5.], [-5., 1.]]
    dd = np.array(A.diagonal())
    op = _Dense(ctx, A, dd)
    # (the real parts of a conjugate pair of Ritz vectors coincide: their second correction is dropped)
    kw = dict(max_iter=6, on_null=S.DROP_NULL)
    with pytest.raises(PymesError, match=r"test: root [01] of the right problem has a complex Ritz value"):
        op.run(op.start(dd, 3), refuse_complex="test: root %d of the right problem", **kw)
    out = op.run(op.start(dd, 3), **kw)
    # (the pair's plane is in the span from the first pass: its residual stays, and the search ends when root 2 is done)
    assert 3 <= out.passes == len(out.history) <= 6 and not out.converged
    assert out.rel[2] < 1e-10 and np.all(out.rel[:2] > 1.0)


def test_null_vector_policy(ctx):
    lay = S.FlatLayout(ctx, (3, 2), (3, 3, 2, 2))
    rng = np.random.default_rng(5)

    def vectors(k):
        out = []
        for _ in range(k):
            v = lay.padded()
            r2 = rng.standard_normal(lay.shape2)
            lay.part1(v).set(rng.standard_normal(lay.shape1))
            lay.part2(v).set(r2 + r2.transpose(1, 0, 3, 2))
            out.append(v)
        return out
    us = S.orthonormalise_block(ctx, lay, [], vectors(2))
    ys = vectors(2)
    ys.append(lay.empty().copy_from(ys[0]))            # a duplicate: nothing new in the third direction
    before = [y.get() for y in ys]
    dropped = S.orthonormalise_block(ctx, lay, us, ys, on_null=S.DROP_NULL)
    assert len(dropped) == 2
    assert np.abs(ctx.gram(us + dropped, us + dropped) - np.eye(4)).max() <= S.ORTH_TOL
    replaced = S.orthonormalise_block(ctx, lay, us, ys, on_null=S.REPLACE_NULL)
    assert len(replaced) == 3
    assert np.abs(ctx.gram(us + replaced, us + replaced) - np.eye(5)).max() <= S.ORTH_TOL
    r2 = lay.part2(replaced[2]).get()
    assert np.abs(r2 - r2.transpose(1, 0, 3, 2)).max() < 1e-14          # the replacement is exchange-symmetric
    assert np.array_equal(replaced[2].get()[6:32], np.zeros(26))
    for y, b in zip(ys, before):                       # the inputs are left as they were
        assert np.array_equal(y.get(), b)
    for policy in (S.DROP_NULL, S.REPLACE_NULL):
        with pytest.raises(np.linalg.LinAlgError, match="linearly dependent Ritz vectors"):
            S.orthonormalise_block(ctx, lay, [], ys, shadows=vectors(3), on_null=policy)
