"""GPU: the post-CCSD assembly kernels past one trip of their block loops (csrc/kernels_post.hip: ipea_correction / _final,
ipea_diagonals, ipea_pack / _assemble / _unpack, ipea_dyson, lambda_assemble, rdm1_assemble, tdm1_assemble).  Each of them runs one
block per virtual pair, row or root and strides ``for (e = threadIdx.x; e < extent; e += 256)`` over o^2, nv, no nv or a chunk of
4096 elements, often with an LDS tile or row between two such loops; the sibling modules compare them with numpy where every such
loop makes exactly one trip.  Here the same numpy references (tests/_lambda_reference.py, _transition_reference.py,
_dyson_reference.py, _ipea_reference.py) are met at the smallest shapes that cross each boundary:

  Davidson correction   two and 257 blocks of 4096 elements (the second stage's loop over the block partials makes a second trip),
                        a ragged last block, the pad [n1, off2) of the flat vector filled with NaN, 17 roots (two launches)
  IP / EA sigma, left   EA has S = no along w: a second tile of 32 w from no = 33; k = 16 fills the by-value pointer table
  Dyson amplitudes      the LDS row [no] of EA longer than a wave and a w tile
  Lambda assembly       o^2 > 256 from no = 17 (289; 529 at no = 23: three trips), o^2 = 256 exactly at no = 16, the update branch,
                        the ladder halves of k = 3 vectors side by side (row pitches other than the defaults), a single virtual
  densities             n1 = no nv = 297 and 514 (the block sum of <lambda, r>), nv = 257 (the loops over b), no = 33

Not covered: nv > 256 in ipea_dyson (the second trip of its loops over the virtuals).  The sigma handle it runs on hoists o v^3
intermediates and needs the o v^3 / v^4 blocks of the operator, several hundred MB at nv = 257 for one loop trip."""
import functools
import math

import numpy as np
import pytest

from oracle import cc_oracle as oc
from tests import _dyson_reference as D
from tests import _ipea_reference as IR
from tests import _lambda_reference as LR
from tests import _transition_reference as X
from tests.test_gpu_dyson import _get, _handle
from tests.test_gpu_ip_ea import _check_sigma, _solver, _sym_case
from tests.test_gpu_ip_ea import _vectors as _ipea_vectors
from tests.test_gpu_lambda import _apply_case, quiet
from tests.test_gpu_lambda import _vectors as _left_vectors

pytestmark = pytest.mark.gpu
KINDS = ("ip", "ea")
SMALL_WS = 1 << 27          # bytes of workspace for a bare context: its default grows with o v^3


# ---- 1. the Davidson correction against numpy ---------------------------------------------------------------------------------------
def _correction_inputs(lay, n, seed):
    """n flat vectors s, r, one flat d, roots w of both signs with |w - d + shift| >= 0.5, the pad [n1, off2) NaN everywhere."""
    rng = np.random.default_rng(seed)
    s, r = rng.standard_normal((n, lay.nflat)), rng.standard_normal((n, lay.nflat))
    d = rng.uniform(-1.0, 1.0, lay.nflat)
    w = rng.uniform(2.0, 4.0, n) * np.where(np.arange(n) % 2, -1.0, 1.0)
    for x in (s, r):
        x[:, lay.n1:lay.off2] = np.nan
    d[lay.n1:lay.off2] = np.nan
    return s, r, d, w


def _check_correction(ctx, lay, call, n, seed, shift=0.125):
    """``call(ss, rs, w, d, shift, qs)`` on device vectors against numpy: the pad of q, every element, both sums, the bits."""
    s, r, d, w = _correction_inputs(lay, n, seed)
    act = np.ones(lay.nflat, dtype=bool)
    act[lay.n1:lay.off2] = False
    assert np.abs(w[:, None] - d[None, act] + shift).min() >= 0.5
    ss, rs, dd = [ctx.array(x) for x in s], [ctx.array(x) for x in r], ctx.array(d)
    runs = []
    for _ in range(2):
        qs = [ctx.array(np.full(lay.nflat, np.nan)) for _ in range(n)]          # every element must be written
        res, nrm = call(ss, rs, w, dd, shift, qs)
        runs.append((np.array([q.get() for q in qs]), res, nrm))
    q, res, nrm = runs[0]
    assert res.shape == (n,) and nrm.shape == (n,)
    worst = [0.0, 0.0, 0.0]
    for z in range(n):
        assert np.all(q[z, lay.n1:lay.off2] == 0.0) and not np.signbit(q[z, lay.n1:lay.off2]).any()
        sa, ra, den = s[z, act], r[z, act], w[z] - d[act] + shift
        x = sa - w[z] * ra
        # one subtraction, one product-difference that the compiler may fuse, one division
        bound = 2.0 ** -50 * (np.abs(sa) + np.abs(w[z] * ra)) / np.abs(den)
        err = np.abs(q[z, act] - x / den)
        assert np.all(err <= bound), (z, int(np.argmax(err - bound)), float((err / bound).max()))
        ref_res, ref_nrm = math.fsum(x * x), math.fsum(ra * ra)
        worst = [max(worst[0], float((err / bound).max())), max(worst[1], abs(res[z] - ref_res) / ref_res),
                 max(worst[2], abs(nrm[z] - ref_nrm) / ref_nrm)]
        assert abs(res[z] - ref_res) <= 1e-13 * ref_res, (z, res[z], ref_res)
        assert abs(nrm[z] - ref_nrm) <= 1e-13 * ref_nrm, (z, nrm[z], ref_nrm)
    print("len %d, n %d: max element error / bound %.2e, residual sum %.2e, norm sum %.2e (relative)" % ((lay.nflat, n) + tuple(worst)))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("no,nv,n,n1,off2,nflat", [(3, 5, 1, 15, 32, 257), (3, 5, 3, 15, 32, 257), (4, 16, 17, 64, 64, 4160),
                                                   (5, 13, 16, 65, 96, 4321), (32, 32, 2, 1024, 1024, 1049600)])
def test_eom_correction_against_numpy(gpu_lib, no, nv, n, n1, off2, nflat):
    from pymes_amd.device import Context
    from pymes_amd.solver import subspace
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=SMALL_WS)
    try:
        lay = subspace.FlatLayout(ctx, (nv, no), (nv, nv, no, no))
        assert (lay.n1, lay.off2, lay.nflat) == (n1, off2, nflat)
        call = lambda *a: subspace.correction(ctx.lib, "pymes_eom_correction", ctx.handle, lay, *a)
        _check_correction(ctx, lay, call, n, seed=1000 * no + nv + n)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _ipea_case(no, nv):
    """(f, blocks, t2) of test_gpu_ip_ea's _sym_case: no hermiticity."""
    f, V, _, t2 = _sym_case(no, nv, seed=no + 3 * nv)
    return f, oc.split_blocks(no, V), t2


@pytest.mark.parametrize("kind", KINDS)
def test_ipea_correction_and_diagonals_8_40(gpu_lib, kind):
    """The handle's own correction entry (IP: one block with a pad; EA: n2 = 12800, four blocks) and its diagonals."""
    no, nv = 8, 40
    f, Vb, t2 = _ipea_case(no, nv)
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        assert sig.nflat == (2592 if kind == "ip" else 12864)
        _check_correction(ctx, sig.layout, sig.correction, 3, seed=7 + (kind == "ea"))
        _check_diagonals(kind, no, f, Vb, t2, sig)


# ---- 2. the IP / EA diagonals --------------------------------------------------------------------------------------------------------
def _check_diagonals(kind, no, f, Vb, t2, sig):
    d = sig.diagonals()
    d1, d2 = sig.part1(d).get(), sig.part2(d).get()
    r1, r2 = IR.diagonals(kind, no, f, Vb, t2)
    tol = 1e-12 * max(1.0, np.abs(r1).max(), np.abs(r2).max())
    e1, e2 = np.abs(d1 - r1).max(), np.abs(d2 - r2).max()
    print(kind, sig.no, sig.nv, "diagonals: max error %.2e %.2e (bound %.2e)" % (e1, e2, tol))
    assert d1.shape == r1.shape and d2.shape == r2.shape
    assert e1 <= tol and e2 <= tol
    assert np.all(d.get()[sig.n1:sig.off2] == 0.0)


@pytest.mark.parametrize("no,nv", [(33, 3), (3, 33)])
@pytest.mark.parametrize("kind", KINDS)
def test_ipea_diagonals_against_the_reference(gpu_lib, kind, no, nv):
    f, Vb, t2 = _ipea_case(no, nv)
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        _check_diagonals(kind, no, f, Vb, t2, sig)


# ---- 3. IP / EA sigma, right and left, where EA's w extent exceeds one tile of 32 --------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(33, 3), (40, 2)])
@pytest.mark.parametrize("kind", KINDS)
def test_ipea_sigma_right_and_left_second_w_tile(gpu_lib, kind, no, nv):
    f, Vb, t2 = _ipea_case(no, nv)
    assert np.abs(Vb["ijab"] - Vb["ijab"].transpose(1, 0, 3, 2)).max() < 1e-14
    s = _solver(kind, no)
    _check_sigma(kind, no, f, Vb, t2, lambda a, b: quiet(s.apply, f, Vb, t2, a, b), seed=5)
    l1s, l2s = _ipea_vectors(kind, no, nv, 3, 5)
    stacked = quiet(s.apply_left, f, Vb, t2, l1s, l2s)
    for z in range(3):
        a, b = D.left_sigma_terms(kind, no, f, Vb, t2, l1s[z], l2s[z])
        scale = max(np.abs(a).max(), np.abs(b).max())
        one = quiet(s.apply_left, f, Vb, t2, l1s[z], l2s[z])
        for got in (stacked[z], one):
            err = max(np.abs(got[0] - a).max(), np.abs(got[1] - b).max())
            print(kind, no, nv, "left vector", z, "max error / max |ref|", err / scale)
            assert err <= 1e-11 * scale, (kind, no, nv, z, err / scale)


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("kind", KINDS)
def test_ipea_sixteen_stacked_vectors_33_3(gpu_lib, kind, side):
    """k = 16, the most one call takes (the by-value pointer table of the pack / assemble / unpack kernels holds 16), vector by
    vector against the k = 1 build on the same handle: the stacked-against-single bound of the sibling tests."""
    no, nv = 33, 3
    f, Vb, t2 = _ipea_case(no, nv)
    x1s, x2s = _ipea_vectors(kind, no, nv, 16, 8)
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        apply = sig.apply_many if side == "right" else sig.apply_left_many
        d1, d2 = [ctx.array(x) for x in x1s], [ctx.array(x) for x in x2s]
        stacked = _get(apply(d1, d2))
        single = [_get(apply(d1[z:z + 1], d2[z:z + 1]))[0] for z in range(16)]
    worst = 0.0
    for z in range(16):
        scale = max(np.abs(single[z][0]).max(), np.abs(single[z][1]).max())
        dev = max(np.abs(single[z][0] - stacked[z][0]).max(), np.abs(single[z][1] - stacked[z][1]).max())
        worst = max(worst, dev / scale)
        assert dev <= 1e-13 * scale, (kind, side, z, dev / scale)
    assert max(np.abs(single[0][1] - single[15][1]).max(), np.abs(stacked[0][1] - stacked[15][1]).max()) > 1e-3
    print(kind, side, "k = 16: max |stacked - single| / max |single| = %.2e" % worst)


# ---- 4. Dyson amplitudes: the LDS row of EA longer than a wave ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_dyson_against_the_terms_33_3(gpu_lib, kind):
    no, nv = 33, 3
    t1, t2, lam, ls, rs = D.definition_inputs(kind, no, nv)
    l1s, l2s, r1s, r2s = [x[0] for x in ls], [x[1] for x in ls], [x[0] for x in rs], [x[1] for x in rs]
    ref = [D.dyson_terms(kind, no, t1, t2, lam[0], lam[1], ls[z], rs[z]) for z in range(3)]
    ref_l, ref_r = np.array([x[0] for x in ref]), np.array([x[1] for x in ref])
    n = no + nv
    f, Vb = np.diag(np.arange(1.0, n + 1.0)), oc.split_blocks(no, np.zeros((n, n, n, n)))
    with _handle(kind, no, f, Vb, t2) as (ctx, sig):
        up = ctx.array
        ups = lambda xs: [ctx.array(x) for x in xs]
        args = (up(t1), up(lam[0]), up(lam[1]))
        pl, pr = sig.dyson(*args, ups(l1s), ups(l2s), ups(r1s), ups(r2s))
        pl2, pr2 = sig.dyson(*args, ups(l1s), ups(l2s), ups(r1s), ups(r2s))
        pl1, pr1 = sig.dyson(*args, ups(l1s[1:2]), ups(l2s[1:2]), ups(r1s[1:2]), ups(r2s[1:2]))
    el, er = np.abs(pl - ref_l).max(), np.abs(pr - ref_r).max()
    e1 = max(np.abs(pl1[0] - ref_l[1]).max(), np.abs(pr1[0] - ref_r[1]).max())
    print(kind, no, nv, "max |psiL - terms| = %.2e  max |psiR - terms| = %.2e  k = 1: %.2e" % (el, er, e1))
    assert el < 1e-10 and er < 1e-10 and e1 < 1e-10
    assert np.array_equal(pl, pl2) and np.array_equal(pr, pr2)
    assert np.abs(pl[0] - pl[1]).max() > 1e-3 and np.abs(pr[0] - pr[1]).max() > 1e-3


# ---- 5. the Lambda assembly -----------------------------------------------------------------------------------------------------------------
LEFT_CASES = [(16, 3, False), (17, 3, False), (17, 3, True), (23, 2, False), (17, 1, False)]
LEFT_IDS = ["%dx%d-%s" % (o, v, "hermitian" if h else "exchange-only") for o, v, h in LEFT_CASES]


@pytest.mark.parametrize("no,nv,hermitian", LEFT_CASES, ids=LEFT_IDS)
def test_lambda_left_apply_past_one_trip(gpu_lib, no, nv, hermitian):
    """o^2 = 256 (the last shape of one trip), 289 and 529; at (17,1) there is no strictly-lower virtual pair, so the
    antisymmetric half of the packed ladder has no rows."""
    from pymes_amd.solver.lambda_ccsd import Lambda_CCSD
    f, Vb, t2, l1, l2, (r1, r2) = _apply_case(no, nv, hermitian)
    o1, o2 = quiet(Lambda_CCSD(no).apply_left, f, Vb, t2, l1, l2)
    scale = max(np.abs(r1).max(), np.abs(r2).max())
    err = max(np.abs(o1 - r1).max(), np.abs(o2 - r2).max())
    print(no, nv, "hermitian" if hermitian else "exchange-only", "max error / max |ref| = %.2e" % (err / scale))
    assert err <= 1e-10 * scale
    assert np.array_equal(o2, o2.transpose(1, 0, 3, 2))


def _left_handle(no, nv, hermitian):
    """(ctx, LeftSigma, the case) on a context that holds the blocks of _apply_case as they are; the caller closes the context."""
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import LeftSigma
    case = _apply_case(no, nv, hermitian)
    ctx = Context(no, nv)
    try:
        for name in LeftSigma.BLOCKS:
            ctx.set_V_block(name, np.ascontiguousarray(case[1][name]))
        return ctx, LeftSigma(ctx, case[0], ctx.array(case[2])), case
    except Exception:
        ctx.close()
        raise


@pytest.mark.parametrize("no,nv,hermitian", LEFT_CASES[1:4], ids=LEFT_IDS[1:4])
def test_lambda_stacked_left_apply_past_one_trip(gpu_lib, no, nv, hermitian):
    """k = 3: the ladder halves of the three vectors lie side by side, so the assembly reads them with row pitches other than
    o^2 and o (o - 1) / 2; each vector against its k = 1 build (the bound of test_gpu_transitions) and against the reference."""
    ls = [_left_vectors(no, nv, 20 + z) for z in range(3)]
    ctx, sig, (f, Vb, t2, _, _, _) = _left_handle(no, nv, hermitian)
    try:
        d1, d2 = [ctx.array(l[0]) for l in ls], [ctx.array(l[1]) for l in ls]
        single = [[x.get() for x in sig.apply_left(d1[z], d2[z])] for z in range(3)]
        stacked = [[x.get() for x in pair] for pair in sig.apply_left_many(d1, d2)]
        sig.close()
    finally:
        ctx.close()
    for z in range(3):
        r1, r2 = LR.left_sigma(no, f, Vb, ls[z][0], ls[z][1], t2)
        scale = max(np.abs(r1).max(), np.abs(r2).max())
        dev = max(np.abs(single[z][0] - stacked[z][0]).max(), np.abs(single[z][1] - stacked[z][1]).max())
        err = max(np.abs(stacked[z][0] - r1).max(), np.abs(stacked[z][1] - r2).max())
        print(no, nv, "vector %d: |stacked - single| / scale = %.2e  |stacked - reference| / scale = %.2e" % (z, dev / scale, err / scale))
        assert dev <= 1e-13 * scale
        assert err <= 1e-10 * scale
        assert np.array_equal(stacked[z][1], stacked[z][1].transpose(1, 0, 3, 2))


@pytest.mark.parametrize("no,nv", [(17, 3), (23, 2)])
def test_lambda_step_past_one_trip(gpu_lib, no, nv):
    """One step against its definition — res = eta + A^T lam (eta alone at the start), out = lam - res / d, err = -err_scale res / d,
    the returned norm |res| — with the denominators and bounds of test_gpu_lambda.test_handle_refusals_and_allocations."""
    ctx, sig, (f, Vb, t2, l1, l2, (s1, s2)) = _left_handle(no, nv, False)
    try:
        eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
        shift = 0.25
        d1 = eps_v[:, None] - eps_o[None, :] - shift
        d2 = (eps_v[:, None, None, None] + eps_v[None, :, None, None] - eps_o[None, None, :, None] - eps_o[None, None, None, :]
              - shift)
        n1, n2 = LR.eta(no, f, Vb)
        a1, a2 = ctx.array(l1), ctx.array(l2)
        for start, es in ((False, 1.0), (False, 1.0e5), (True, 1.0)):
            r1, r2 = (n1, n2) if start else (n1 + s1, n2 + s2)
            b1, b2 = (np.zeros_like(l1), np.zeros_like(l2)) if start else (l1, l2)
            o1, o2 = ctx.array(np.full(l1.shape, np.nan)), ctx.array(np.full(l2.shape, np.nan))
            e1, e2 = ctx.array(np.full(l1.shape, np.nan)), ctx.array(np.full(l2.shape, np.nan))
            norm = sig.lambda_step(None if start else (a1, a2), eps_o, eps_v, shift, (o1, o2), (e1, e2), start=start, err_scale=es)
            scale = max(np.abs(r1).max(), np.abs(r2).max())
            got = [x.get() for x in (o1, o2, e1, e2)]
            for x in got:
                assert np.all(np.isfinite(x))                # every element is overwritten
            en = abs(norm - np.sqrt((r1 ** 2).sum() + (r2 ** 2).sum()))
            eo = max(np.abs(got[0] - (b1 - r1 / d1)).max(), np.abs(got[1] - (b2 - r2 / d2)).max())
            ee = max(np.abs(got[2] + es * r1 / d1).max(), np.abs(got[3] + es * r2 / d2).max())
            print(no, nv, "start" if start else "step", "err_scale %g: norm %.2e  out %.2e  err %.2e  (scale %.2e)" % (es, en, eo, ee, scale))
            assert en < 1e-10 * scale
            assert eo < 1e-10 * scale
            assert ee < es * 1e-10 * scale
        sig.close()
    finally:
        ctx.close()


# ---- 6. the density and the transition densities ---------------------------------------------------------------------------------------------
DENSITY_SHAPES = [(17, 3), (33, 9), (2, 257)]


@functools.lru_cache(maxsize=None)
def _density_case(no, nv):
    """(inputs, gamma, gammaL, gammaR) by the term tables, once per shape."""
    inp = X.density_inputs(no, nv, 9, k=3)
    t1, t2, lam, ls, rs = inp
    gl, gr = X.transition_density_terms(no, t1, t2, lam, ls, rs)
    return inp, LR.density_terms(no, t1, t2, lam[0], lam[1]), gl, gr


@pytest.mark.parametrize("no,nv", DENSITY_SHAPES)
def test_rdm1_past_one_trip(gpu_lib, no, nv):
    from pymes_amd.device import Context
    from pymes_amd.solver.lambda_ccsd import device_rdm1
    (t1, t2, lam, _, _), ref0, _, _ = _density_case(no, nv)
    ref = ref0.copy()
    ref[np.arange(no), np.arange(no)] += 2.0
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=SMALL_WS)
    try:
        args = (ctx.array(t1), ctx.array(t2), ctx.array(lam[0]), ctx.array(lam[1]))
        g = device_rdm1(ctx, *args)
        g2 = device_rdm1(ctx, *args)
        g0 = device_rdm1(ctx, *args, ref=0.0)
    finally:
        ctx.close()
    err, err0 = np.abs(g - ref).max(), np.abs(g0 - ref0).max()
    print(no, nv, "max |gamma - terms| = %.2e (ref = 0: %.2e)  trace - 2 no = %.2e" % (err, err0, np.trace(g) - 2 * no))
    assert err <= 1e-10 * max(1.0, np.abs(ref).max()) and err0 <= 1e-10 * max(1.0, np.abs(ref0).max())
    assert abs(np.trace(g) - 2 * no) < 1e-12 * no
    assert np.array_equal(g, g2)


@pytest.mark.parametrize("no,nv", DENSITY_SHAPES)
def test_tdm1_past_one_trip(gpu_lib, no, nv):
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_transitions import device_tdm1
    (t1, t2, lam, ls, rs), _, ref_l, ref_r = _density_case(no, nv)
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=SMALL_WS)
    try:
        up = ctx.array
        head = (up(t1), up(t2), up(lam[0]), up(lam[1]))
        vecs = lambda sl: ([up(l[0]) for l in ls[sl]], [up(l[1]) for l in ls[sl]], [up(r[0]) for r in rs[sl]], [up(r[1]) for r in rs[sl]])
        gl, gr, r0 = device_tdm1(ctx, *head, *vecs(slice(0, 3)))
        gl2, gr2, r02 = device_tdm1(ctx, *head, *vecs(slice(0, 3)))
        one = device_tdm1(ctx, *head, *vecs(slice(1, 2))) if (no, nv) == (33, 9) else None
    finally:
        ctx.close()
    dots = np.array([X.dot(lam, r) for r in rs])
    el, er = np.abs(gl - ref_l).max(), np.abs(gr - ref_r).max()
    e0 = np.abs(r0 + dots) / np.maximum(1.0, np.abs(dots))
    print(no, nv, "max |gammaL - terms| = %.2e  max |gammaR - terms| = %.2e  max |r0 + <lambda, r>| = %.2e" % (el, er, e0.max()))
    assert el <= 1e-10 * max(1.0, np.abs(ref_l).max()) and er <= 1e-10 * max(1.0, np.abs(ref_r).max())
    assert np.all(e0 <= 1e-12)
    assert np.array_equal(gl, gl2) and np.array_equal(gr, gr2) and np.array_equal(r0, r02)
    assert np.abs(gl[0] - gl[1]).max() > 1e-3 and np.abs(gr[0] - gr[1]).max() > 1e-3
    if one is not None:                                         # k = 1: row 1 of the k = 3 reference
        assert one[0].shape == (1, no + nv, no + nv)
        assert np.abs(one[0][0] - ref_l[1]).max() <= 1e-10 * max(1.0, np.abs(ref_l[1]).max())
        assert np.abs(one[1][0] - ref_r[1]).max() <= 1e-10 * max(1.0, np.abs(ref_r[1]).max())
        assert abs(one[2][0] + dots[1]) <= 1e-12 * max(1.0, abs(dots[1]))
