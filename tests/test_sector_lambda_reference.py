"""CPU: the numpy restatement of the momentum-sector Lambda equations and of the two-slab Lambda-(T)
(tests/_sector_lambda_reference.py) against finite differences of tests/_sector_reference.residual, against the dense
Lambda of tests/_lambda_reference.py and against tests/_lambda_triples_reference.py; the new table arguments of
pymes_amd/solver/sectors.py; the refusal of the host simulator, which has no sector kernels."""
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc
from pymes_amd.solver import sectors
from tests import _lambda_reference as lref
from tests import _lambda_triples_reference as ltr
from tests import _sector_lambda_reference as sl
from tests import _sector_reference as sr
from tests import _sector_triples_reference as tr
from tests.test_sector_reference import CASES, GOLD, problem, symmetric_amplitudes


def exchange_only(V, seed, amount=0.3):
    """V scaled element by element with a seeded factor that keeps V_pqrs = V_qpsr and nothing else: as conserving as V,
    not Hermitian."""
    A = np.random.default_rng(seed).standard_normal(V.shape)
    W = V * (1.0 + amount * A)
    return 0.5 * (W + W.transpose(1, 0, 3, 2))              # to the bit: a sum of two terms commutes


def twist_problem():
    g = np.load(os.path.join(GOLD, "ueg_twist.npz"))
    tab = sr.tables_for(g["k"], int(g["nel"]) // 2)
    V = g["coulomb"]
    return tab, V, sr.hf_orbital_energies(tab, sr.sector_integrals(tab, V), g["kinetic"])


def adjoint_check(tab, eps, V, label):
    for name, W in (("hermitian", V), ("exchange only", exchange_only(V, 21))):
        ints = sr.sector_integrals(tab, W)
        if name == "exchange only":
            assert np.abs(W - W.transpose(2, 3, 0, 1)).max() > 1e-3 * np.abs(W).max()
            assert np.array_equal(W, W.transpose(1, 0, 3, 2))
        for is_dcd in (False, True):
            T, u, w = 0.1 * symmetric_amplitudes(tab, 3), symmetric_amplitudes(tab, 4), symmetric_amplitudes(tab, 5)
            Ju = 0.5 * (sr.residual(tab, eps, T + u, ints, is_dcd) - sr.residual(tab, eps, T - u, ints, is_dcd))
            jt = sl.jt_apply(tab, eps, T, ints, w, is_dcd)
            lhs, rhs = float(w @ Ju), float(jt @ u)
            bound = 1e-13 * (np.abs(w) @ np.abs(Ju) + np.abs(jt) @ np.abs(u))
            plain = sl.jt_plain(tab, eps, T, ints, w, is_dcd)
            print(f"{label} {name} dcd={is_dcd}: <w,Ju> = {lhs:.15e}, <J^T w,u> = {rhs:.15e}, diff {abs(lhs - rhs):.2e}, "
                  f"bound {bound:.2e}; plain adjoint asymmetry {np.abs(plain - plain[tab.pp_swap]).max():.2e}")
            assert abs(lhs - rhs) <= bound
            assert abs(lhs - float(plain @ u)) <= bound                 # the projection changes nothing on symmetric u
            assert np.array_equal(jt, jt[tab.pp_swap])                   # exchange-symmetric, to the bit
            assert np.abs(jt).max() > 0


@pytest.mark.parametrize("nel,cutoff,mode", CASES)
def test_adjoint_identity(nel, cutoff, mode):
    """<w, J u> = <J^T w, u> with J u = [R(T + u) - R(T - u)] / 2 (exact for a quadratic R, up to rounding)."""
    u, tab, V, ints = problem(nel, cutoff, mode)
    adjoint_check(tab, sr.hf_orbital_energies(tab, ints, u.kinetic), V, f"N={nel} c={cutoff} {mode}")


def test_adjoint_identity_on_the_twisted_basis():
    tab, V, eps = twist_problem()
    assert (tab.neg < 0).any()
    adjoint_check(tab, eps, V, "twist")


def test_adjoint_task_tables_chain():
    """``trans_a`` of gemm_tasks: the default leaves a table unchanged to the byte, the adjoint shapes chain, and every table
    of the Lambda residual stays inside its operands (twisted basis: blocks without a -q included)."""
    for tab in (problem(14, 2, "coulomb")[1], twist_problem()[0]):
        F, S, Fn, Sn = ("ph", "ph-", False), ("ph", "ph", False), ("ph", "ph-", True), ("ph", "ph", True)
        vo, oo, ov, vv = ("vv", "oo", False), ("oo", "oo", False), ("oo", "vv", False), ("vv", "vv", False)
        size = lambda op: tab.offsets(*op[:2])[-1]
        t0 = tab.gemm_tasks(vv, vo, vo, beta=1.0)
        assert t0.tobytes() == tab.gemm_tasks(vv, vo, vo, beta=1.0, trans_a=False).tobytes()
        assert not (t0["flags"] & sectors.TRANS_A).any()
        for a, b, c, kw in ((vv, vo, vo, dict(trans_a=True)), (vo, vo, oo, dict(trans_a=True)), (ov, oo, vo, dict(trans_a=True)),
                            (vo, oo, vo, dict(trans_b=True)), (Fn, Fn, S, dict(trans_a=True)), (F, Sn, F, dict(trans_b=True)),
                            (Fn, Sn, F, dict(trans_a=True)), (S, F, F, dict(trans_a=True)), (F, Sn, F, {}),
                            (F, F, S, dict(trans_b=True)), (S, Fn, F, dict(trans_b=True))):
            t = tab.gemm_tasks(a, b, c, **kw)
            sectors.check_tasks(t, size(a), size(b), size(c))
            assert ((t["flags"] & sectors.TRANS_A) != 0).all() == bool(kw.get("trans_a"))
        t = tab.gemm_tasks(vo, vo, oo, trans_a=True)
        assert (t["m"] == tab.n_oo).all() and (t["k"] == tab.n_vv).all() and (t["lda"] == tab.n_oo).all()
        with pytest.raises(AssertionError, match="do not chain"):
            tab.gemm_tasks(vv, oo, vo, trans_a=True)


# ---- a small conserving problem with a gap: eleven vectors that are not inversion-symmetric, three of them occupied ------
K_SMALL = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, 1, 0], [2, 0, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1],
                    [-1, 1, 0]])


def small_problem(seed, hermitian):
    no, n = 3, len(K_SMALL)
    tab, tt = tr.tables_for(K_SMALL, no)
    V = tr.conserving_V(K_SMALL, seed, scale=0.08)
    if not hermitian:
        V = exchange_only(V, seed + 1)
    eps = ltr.gapped_eps(no, n - no, seed + 2)
    return no, tab, tt, V, eps, sr.sector_integrals(tab, V)


def converged_T(tab, eps, ints, is_dcd=False):
    T = ints["abij"] / tab.denominators(eps)
    inv, mixer = 1.0 / tab.denominators(eps), oc.Diis(6)
    for _ in range(200):
        r = sr.residual(tab, eps, T, ints, is_dcd)
        if np.linalg.norm(r) < 1e-13:
            break
        T = mixer.mix([r * inv], [T + r * inv])[0]
    assert np.linalg.norm(r) < 1e-12
    return T


@pytest.mark.parametrize("hermitian", [True, False])
def test_ccd_lambda_matches_the_dense_lambda(hermitian):
    """For CCD amplitudes the densified sector Lambda is the lambda2 of the dense library's convention at t1 = 0, and
    lambda1 vanishes by momentum conservation."""
    no, tab, tt, V, eps, ints = small_problem(5, hermitian)
    T = converged_T(tab, eps, ints)
    lam, norm = sl.solve_lambda(tab, eps, T, ints, tol=1e-13)
    assert norm <= 1e-13
    nv = tab.nv
    Vd = oc.dressed_V(np.zeros((nv, no)), oc.split_blocks(no, V))
    l1, l2 = lref.solve_lambda(no, np.diag(eps), Vd, tab.to_dense(T))
    err = np.abs(tab.to_dense(lam) - l2).max()
    print(f"hermitian={hermitian}: |lambda2 sector - dense| = {err:.2e}, max|lambda2| = {np.abs(l2).max():.2e}, "
          f"max|lambda1| = {np.abs(l1).max():.2e}, |G| = {norm:.1e}")
    assert np.abs(l1).max() <= 1e-12 * np.abs(l2).max()
    assert err <= 1e-10 * np.abs(l2).max()
    assert np.abs(lam - lam[tab.pp_swap]).max() <= 1e-14 * np.abs(lam).max()


def test_two_slab_triples_match_the_dense_lambda_triples():
    """Per triple within 1e-12 x the abs-sum scale of the dense reference, on a non-Hermitian conserving V."""
    no, tab, tt, V, eps, ints = small_problem(9, hermitian=False)
    T, lam = 0.3 * symmetric_amplitudes(tab, 1), 0.3 * symmetric_amplitudes(tab, 2)
    want, scale = ltr.per_triple(no, V, eps, tab.to_dense(T), None, tab.to_dense(lam))
    VvL, VoL = tr.triples_integrals(tt, V)
    VvR, VoR = sl.right_integrals(tt, V)
    assert np.abs(VvR - VvL).max() > 0 and np.abs(VoR - VoL).max() > 0
    got, own = sl.per_triple(tt, eps, VvR, VoR, VvL, VoL, tt.implied(T), tt.implied(sl.left_amplitudes(tab, lam)))
    live = scale > 0
    worst = np.abs(got - want)[live] / scale[live]
    print(f"{len(want)} triples: largest |d| / scale {worst.max():.2e}; sum {got.sum():.12e} against {want.sum():.12e}")
    assert np.count_nonzero(want) > len(want) // 2
    assert (np.abs(got - want) <= 1e-12 * scale).all()
    # the restatement's own scale takes the six products of R by their absolute values one by one: never below the dense one
    assert (own >= scale * (1.0 - 1e-9)).all()


def test_two_slabs_with_hermitian_integrals_give_the_triples_energy():
    """V_pqrs = V_rspq and lambda2 = 2 T - T^x (so L = T): the (T) of tests/_sector_triples_reference.per_triple."""
    no, tab, tt, V, eps, ints = small_problem(13, hermitian=True)
    T = 0.3 * symmetric_amplitudes(tab, 1)
    a, b, i, j = tab.abij()
    lam = 2.0 * T - T[tab._pp_index(b, a, i, j)]
    assert np.abs(sl.left_amplitudes(tab, lam) - T).max() <= 4 * np.finfo(float).eps * np.abs(T).max()
    Vv, Vo = tr.triples_integrals(tt, V)
    VvR, VoR = sl.right_integrals(tt, V)
    assert np.array_equal(VvR, Vv) and np.array_equal(VoR, Vo)
    want, scale = tr.per_triple(tt, eps, Vv, Vo, tt.implied(T))
    got, _ = sl.per_triple(tt, eps, VvR, VoR, Vv, Vo, tt.implied(T), tt.implied(sl.left_amplitudes(tab, lam)))
    assert np.count_nonzero(want) > 0 and (np.abs(got - want) <= 1e-12 * scale).all()


def test_right_hand_list_families():
    tab, tt = tr.tables_for(K_SMALL, 3)
    assert tt.FAMILIES == ("vv", "vo") and tt.RIGHT_FAMILIES == ("vv_r", "vo_r") and sorted(tt.sizes) == ["vo", "vv"]
    for fam in tt.FAMILIES:
        left, ok = tt.list_pqrs(fam)
        right, ok_r = tt.list_pqrs(fam + "_r")
        assert np.array_equal(ok, ok_r) and np.array_equal(right, left[:, [2, 3, 0, 1]]) and right.dtype == np.int32
        assert tab.conserving(right[ok]).all()
        part, okp = tt.list_pqrs(fam + "_r", 5, 17)
        assert np.array_equal(part, right[5:17]) and np.array_equal(okp, ok[5:17])
    with pytest.raises(KeyError):
        tt.list_pqrs("ov_r")


def test_the_host_simulator_refuses_the_lambda_triples_by_name(hostsim_lib):
    import ctypes as C

    from pymes_amd._lib import PymesError
    from pymes_amd.device import Context
    ctx = Context(1, 1, lib=hostsim_lib)
    try:
        x = ctx.zeros((64,))
        box = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
        p = C.c_void_p(x.ptr)
        e = C.c_double()
        with pytest.raises(PymesError, match="sector_triples_lambda: not available in this backend"):
            ctx.lib.call("pymes_sector_triples_lambda", ctx.handle, 1, 1, p, p, p, box.ctypes.data_as(C.c_void_p), p, p, p, p, p,
                         p, p, 0, 1, p, 512, None, C.byref(e))
    finally:
        ctx.close()
