"""GPU: IP- and EA-EOM-CCSD (pymes_amd/solver/eom_ip_ea.py; csrc/eom.cpp, IpEaSigma; include/pymes_amd.h, pymes_ipea_sigma_*).
The sigma builds against the numpy definition (tests/_ipea_reference.py) and against the device EE build on the embedded
problem, the closed-form limits end to end, the Davidson driver against dense diagonalisation, transcorrelated integrals,
integral sharding, FNO truncation, housekeeping."""
import contextlib
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest

from oracle import cc_oracle as oc, io_oracle as oio
from oracle.cases import random_case, synthetic_case
from oracle.io_oracle import synthetic_factors
from pymes_amd import _lib
from tests import _ipea_reference as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KINDS = ("ip", "ea")


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _live():
    n = C.c_int64()
    _lib.default_library().call("pymes_live_allocations", C.byref(n))
    return int(n.value)


def _solver(kind, no, n_roots=3):
    from pymes_amd.solver.eom_ip_ea import EA_EOM_CCSD, IP_EOM_CCSD
    return (IP_EOM_CCSD if kind == "ip" else EA_EOM_CCSD)(no, n_roots=n_roots)


def _kind_id(kind):
    from pymes_amd.solver import eom_ip_ea as M
    return M.KIND_IP if kind == "ip" else M.KIND_EA


def _vectors(kind, no, nv, k, seed):
    rng = np.random.default_rng(seed)
    s1, s2 = R.shapes(kind, no, nv)
    return [rng.standard_normal(s1) for _ in range(k)], [rng.standard_normal(s2) for _ in range(k)]


def _check_sigma(kind, no, f, Vd, t2, apply, seed, bound=1e-11):
    """`apply(r1s, r2s)` for k = 3 stacked vectors and for each alone against the term tables of the reference."""
    nv = f.shape[0] - no
    r1s, r2s = _vectors(kind, no, nv, 3, seed)
    stacked = apply(r1s, r2s)
    for z in range(3):
        a, b = R.sigma_terms(kind, no, f, Vd, t2, r1s[z], r2s[z])
        scale = max(np.abs(a).max(), np.abs(b).max())
        one = apply(r1s[z:z + 1], r2s[z:z + 1])[0]
        for got in (stacked[z], one):
            err = max(np.abs(got[0] - a).max(), np.abs(got[1] - b).max())
            print(kind, no, nv, "vector", z, "max error / max |ref|", err / scale)
            assert err <= bound * scale, (kind, no, nv, z, err / scale)
        # stacked against single: the products run with N = 3 P against N = P columns, and the GEMM's plan (tile shape,
        # split-K) depends on N, so the summation order may differ: not bit for bit, bounded instead
        dev = max(np.abs(stacked[z][0] - one[0]).max(), np.abs(stacked[z][1] - one[1]).max())
        print(kind, no, nv, "vector", z, "stacked - single / max |ref|", dev / scale)
        assert dev <= 1e-13 * scale


def _sym_case(no, nv, seed):
    """Integrals with V_pqrs = V_qpsr only, a non-symmetric Fock matrix, exchange-symmetric T2, a small T1."""
    f, V, t1, t2 = random_case(no, nv, seed=seed)
    rng = np.random.default_rng(seed + 1)
    return f + 0.03 * rng.standard_normal(f.shape), R.symmetrise(V), 0.1 * t1, t2


# ---- 1. sigma against the definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv", [(2, 3), (3, 5), (5, 19), (8, 40), (7, 33), (20, 10)])
@pytest.mark.parametrize("kind", KINDS)
def test_sigma_against_the_definition(gpu_lib, kind, no, nv):
    from pymes_amd.integral.device import DeviceIntegrals, DressedDeviceIntegrals
    from pymes_amd.solver.ccsd import CCSD
    f, V, t1, t2 = _sym_case(no, nv, seed=no + 3 * nv)
    assert np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-3             # no hermiticity
    Vb = oc.split_blocks(no, V)
    s = _solver(kind, no)
    # host-dictionary form, blocks read as set (dressed = 0)
    _check_sigma(kind, no, f, Vb, t2, lambda a, b: quiet(s.apply, f, Vb, t2, a, b), seed=5)
    # device form, the context's T1-dressed blocks (dressed = 1)
    Vd = oc.dressed_V(t1, Vb)
    Vd = {k: (v if v is not None else Vb[k]) for k, v in Vd.items()}
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        dressed = CCSD(no).get_T1_dressed_V(t1, ints, s.BLOCKS)
        assert isinstance(dressed, DressedDeviceIntegrals)
        t2d = ints.ctx.array(t2)
        _check_sigma(kind, no, f, Vd, t2, lambda a, b: quiet(s.apply, f, dressed, t2d, a, b), seed=6)
    finally:
        ints.ctx.close()


# ---- 2. sigma against the device EE build on the embedded problem, at a size numpy cannot reach ----------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sigma_against_the_device_ee_build_30_120(gpu_lib, kind):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.eom_ccsd import _Sigma
    from pymes_amd.solver.eom_ip_ea import IPEASigma
    no, nv, eps_x = 30, 120, (0.37 if kind == "ip" else -0.41)
    n = no + nv
    B, eps = synthetic_factors(no, nv, seed=3)
    rng = np.random.default_rng(11)
    f = np.diag(eps) + 0.01 * rng.standard_normal((n, n))
    t2 = 0.02 * rng.standard_normal((nv, nv, no, no))
    t2 = t2 + t2.transpose(1, 0, 3, 2)
    r1s, r2s = _vectors(kind, no, nv, 2, seed=12)
    # the new build on the (30,120) context
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        c = ints.ctx
        sig = IPEASigma(c, _kind_id(kind), f, c.array(t2))
        got = [(a.get(), b.get()) for a, b in sig.apply_many([c.array(x) for x in r1s], [c.array(x) for x in r2s])]
        sig.close()
    finally:
        ints.ctx.close()
    # the embedded context: one all-zero orbital more in the factors (the 121st virtual / an occupied in front)
    idx = np.arange(n) + (1 if kind == "ea" else 0)
    x = 0 if kind == "ea" else n
    Bx = np.zeros((B.shape[0], n + 1, n + 1))
    Bx[np.ix_(np.arange(B.shape[0]), idx, idx)] = B
    fx = np.zeros((n + 1, n + 1))
    fx[np.ix_(idx, idx)] = f
    fx[x, x] = eps_x
    nox, nvx = (no, nv + 1) if kind == "ip" else (no + 1, nv)
    T = np.zeros((nvx, nvx, nox, nox))
    u1s, u2s = [], []
    if kind == "ip":
        T[:nv, :nv] = t2
        for r1, r2 in zip(r1s, r2s):
            u1, u2 = np.zeros((nvx, nox)), np.zeros((nvx, nvx, nox, nox))
            u1[nv] = r1
            u2[nv, :nv] = r2.transpose(2, 0, 1)
            u2[:nv, nv] = r2.transpose(2, 1, 0)
            u1s.append(u1), u2s.append(u2)
    else:
        T[:, :, 1:, 1:] = t2
        for r1, r2 in zip(r1s, r2s):
            u1, u2 = np.zeros((nvx, nox)), np.zeros((nvx, nvx, nox, nox))
            u1[:, 0] = r1
            u2[:, :, 0, 1:] = r2
            u2[:, :, 1:, 0] = r2.transpose(1, 0, 2)
            u1s.append(u1), u2s.append(u2)
    ints = DeviceIntegrals.from_factors(nox, Bx)
    try:
        c = ints.ctx
        ee = _Sigma(c, fx, c.array(T))
        out = [(a.get(), b.get()) for a, b in ee.apply_many([c.array(u) for u in u1s], [c.array(u) for u in u2s])]
        ee.close()
    finally:
        ints.ctx.close()
    for z, (s1, s2) in enumerate(out):
        if kind == "ip":
            ref1, ref2 = s1[nv] - eps_x * r1s[z], s2[nv, :nv].transpose(1, 2, 0) - eps_x * r2s[z]
            leak = max(np.abs(s1[:nv]).max(), np.abs(s2[:nv, :nv]).max())
        else:
            ref1, ref2 = s1[:, 0] + eps_x * r1s[z], s2[:, :, 0, 1:] + eps_x * r2s[z]
            leak = max(np.abs(s1[:, 1:]).max(), np.abs(s2[:, :, 1:, 1:]).max())
        scale = max(np.abs(ref1).max(), np.abs(ref2).max())
        err = max(np.abs(got[z][0] - ref1).max(), np.abs(got[z][1] - ref2).max())
        print(kind, "vector", z, "max error / max |ref|", err / scale, "leak", leak / scale)
        assert leak <= 1e-10 * scale
        assert err <= 1e-10 * scale


# ---- 3. closed-form limits end to end --------------------------------------------------------------------------------------------
def _ccsd_dressed(no, f, V, delta_e=1e-12):
    """CCSD on the GPU, then the dressed Fock matrix and dictionary of dressed blocks (host forms)."""
    from pymes_amd.integral.partition import part_2_body_int
    from pymes_amd.solver.ccsd import CCSD
    cc = CCSD(no, delta_e=delta_e)
    res = quiet(cc.solve, f, V, max_iter=200)
    Vb = part_2_body_int(no, V)
    fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], Vb)
    Vd = quiet(cc.get_T1_dressed_V, res["t1"], Vb)
    Vd = {k: (v if v is not None else Vb[k]) for k, v in Vd.items()}
    return res, fd, Vd


def _dense_by_apply(kind, no, fd, Vd, t2):
    nv = fd.shape[0] - no
    s1, s2 = R.shapes(kind, no, nv)
    n1, n = int(np.prod(s1)), R.dim(kind, no, nv)
    eye = np.eye(n)
    out = quiet(_solver(kind, no).apply, fd, Vd, t2, [eye[c, :n1].reshape(s1) for c in range(n)],
                [eye[c, n1:].reshape(s2) for c in range(n)])
    return np.array([np.concatenate([a.ravel(), b.ravel()]) for a, b in out]).T


def _fcidump(tag, tmp_path=None, is_tc=False):
    path = os.path.join(GOLD, "tc" if is_tc else "fcidump", "FCIDUMP." + tag)
    if not os.path.exists(path):
        with gzip.open(path + ".gz", "rb") as src, open(str(tmp_path / ("FCIDUMP." + tag)), "wb") as dst:
            dst.write(src.read())
        path = str(tmp_path / ("FCIDUMP." + tag))
    ne, n, ec, eps, h, V = oio.read_fcidump(path, is_tc=is_tc)
    return ne // 2, h, V


@pytest.mark.parametrize("tag", ["H2.ccpvdz", "H2.321g", "H2.sto6g"])
def test_two_electron_ip_spectrum(gpu_lib, tag):
    no, h, V = _fcidump(tag)
    assert no == 1
    f = oio.fock_matrix(no, h, V)
    res, fd, Vd = _ccsd_dressed(no, f, V)
    w = np.linalg.eigvals(_dense_by_apply("ip", no, fd, Vd, res["t2"]))
    exact = np.sort(np.linalg.eigvalsh(h)) - (R.hf_energy(no, h, f) + res["ccsd e"])
    dev = np.abs(np.sort(w.real) - exact).max()
    print(tag, "IP spectrum, max deviation", dev, "max |imag|", np.abs(w.imag).max())
    assert len(w) == h.shape[0] and np.abs(w.imag).max() < 1e-9 and dev < 1e-9


def _two_hole_case(name):
    if name == "H2.sto6g":
        no, h, V = _fcidump(name)
        return no, h, V, oio.fock_matrix(no, h, V)
    no = int(name)
    f, V, _, _ = synthetic_case(no, 1, seed=no - 2, scale=0.6)
    return no, R.fock_and_core(no, f, V)[0], V, f


@pytest.mark.parametrize("name", ["H2.sto6g", "5", "7"])
def test_two_hole_ea_spectrum(gpu_lib, name):
    no, h, V, f = _two_hole_case(name)
    assert f.shape[0] == no + 1
    f_full = R.fock_and_core(no, f, V)[1]
    res, fd, Vd = _ccsd_dressed(no, f, V)
    w = np.linalg.eigvals(_dense_by_apply("ea", no, fd, Vd, res["t2"]))
    exact = np.sort(R.full_energy(h, f_full) - np.linalg.eigvalsh(f_full)) - (R.hf_energy(no, h, f) + res["ccsd e"])
    dev = np.abs(np.sort(w.real) - exact).max()
    print(name, "EA spectrum, max deviation", dev, "max |imag|", np.abs(w.imag).max())
    assert len(w) == no + 1 and np.abs(w.imag).max() < 1e-9 and dev < 1e-9


# ---- 4. Davidson against dense diagonalisation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("no,nv,seed", [(4, 10, 1), (6, 14, 2)])
@pytest.mark.parametrize("kind", KINDS)
def test_davidson_against_dense(gpu_lib, kind, no, nv, seed):
    f, V, _, _ = synthetic_case(no, nv, seed=seed)
    r, fd_ref, Vd_ref = R.converged_case(no, f, V, delta_e=1e-13)
    w = np.linalg.eigvals(R.dense(kind, no, fd_ref, Vd_ref, r["t2"]))
    w = w[np.argsort(w.real)][:4]
    assert np.abs(w.imag).max() == 0.0 and np.diff(w.real).min() > 1e-3, w      # on the numpy reference alone
    res, fd, Vd = _ccsd_dressed(no, f, V)
    s = _solver(kind, no, n_roots=3)
    e = quiet(s.solve, fd, Vd, res["t2"])
    print(kind, no, nv, "roots", e, "dense", w.real[:3], "passes", s.iterations, "residuals", s.residual_norms,
          "singles weight", s.singles_weight)
    assert s.converged and s.iterations <= s.max_iter
    assert np.abs(e - w.real[:3]).max() < 1e-8
    assert np.all(np.diff(e) > 0.0)
    assert np.all(s.residual_norms < s.r_epsilon) and np.all(s.singles_weight > 0.9)
    assert len(s.history) == s.iterations and s.r_singles[0].shape == R.shapes(kind, no, nv)[0]


def _certify(sig, r1s, r2s, e):
    """|sigma(r_n) - e_n r_n| / |r_n| from a FRESH apply on the returned vectors, by gram products."""
    c = sig.ctx
    out = sig.apply_many(r1s, r2s)
    rel = []
    for n, (s1, s2) in enumerate(out):
        num = den = 0.0
        for s, r in ((s1, r1s[n]), (s2, r2s[n])):
            z = c.empty(r.shape)
            c.lincomb_multi([z], [s, r], np.array([[1.0], [-e[n]]]))
            num += c.gram([z], [z])[0, 0]
            den += c.gram([r], [r])[0, 0]
        rel.append(float(np.sqrt(num / den)))
    return rel


def _device_chain(kind, no, f, V, n_roots):
    """DeviceIntegrals -> CCSD with device amplitudes -> the dressed hand-over -> solve -> certificate."""
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.eom_ip_ea import IPEASigma
    ints = DeviceIntegrals.from_V_pqrs(no, V)
    try:
        cc = CCSD(no, delta_e=1e-12)
        res = quiet(cc.solve, f, ints, max_iter=200, device_amplitudes=True)
        fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], ints)
        s = _solver(kind, no, n_roots=n_roots)
        dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, s.BLOCKS)
        e = quiet(s.solve, fd, dressed, res["t2"])
        assert s.r_doubles[0].ctx is ints.ctx                              # the vectors stay in HBM
        sig = IPEASigma(ints.ctx, _kind_id(kind), fd, res["t2"], dressed=True)
        rel = _certify(sig, s.r_singles, s.r_doubles, e)
        sig.close()
        return e, rel, s
    finally:
        ints.ctx.close()


@pytest.mark.parametrize("tag", ["LiH.321g", "syn_5_19"])
@pytest.mark.parametrize("kind", KINDS)
def test_roots_certified_by_a_fresh_apply(gpu_lib, tmp_path, kind, tag):
    no, h, V = _fcidump(tag, tmp_path)
    f = oio.fock_matrix(no, h, V)
    e, rel, s = _device_chain(kind, no, f, V, n_roots=min(3, no))
    print(tag, kind, "roots", e, "certificate", rel, "passes", s.iterations)
    assert s.converged and max(rel) < 1e-6, rel
    assert np.all(np.diff(e) >= 0.0)
    if kind == "ip":
        assert e[0] > 0.0


# ---- 5. transcorrelated integrals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_transcorrelated(gpu_lib, kind):
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_ip_ea import IPEASigma
    no, h, V = _fcidump("LiH.tc", is_tc=True)
    nv = h.shape[0] - no
    assert np.abs(V - V.transpose(1, 0, 3, 2)).max() < 1e-14 and np.abs(V - V.transpose(2, 3, 0, 1)).max() > 1e-6
    f = oio.fock_matrix(no, h, V)
    r, fd, Vd = R.converged_case(no, f, V, delta_e=1e-12)
    s = _solver(kind, no)
    _check_sigma(kind, no, fd, Vd, r["t2"], lambda a, b: quiet(s.apply, fd, Vd, r["t2"], a, b), seed=9)
    # the operator is not symmetric: only roots below the first complex pair or near-degeneracy (gap < 1e-3) are asked for
    w = np.linalg.eigvals(R.dense(kind, no, fd, Vd, r["t2"]))
    w = w[np.argsort(w.real)]
    good, most = 0, min(3, R.shapes(kind, no, nv)[0][0], len(w) - 1)
    while good < most and w[good].imag == 0.0 and w[good + 1].imag == 0.0 and w[good + 1].real - w[good].real > 1e-3:
        good += 1
    print(kind, "dense spectrum (lowest)", w[:4], "roots asked for:", good)
    if good:
        s = _solver(kind, no, n_roots=good)
        e = quiet(s.solve, fd, Vd, r["t2"])
        c = Context(no, nv)
        try:
            for name in s.BLOCKS:
                c.set_V_block(name, np.ascontiguousarray(Vd[name]))
            sig = IPEASigma(c, _kind_id(kind), fd, c.array(r["t2"]))
            rel = _certify(sig, [c.array(x) for x in s.r_singles], [c.array(x) for x in s.r_doubles], e)
            sig.close()
        finally:
            c.close()
        print(kind, "roots", e, "certificate", rel)
        assert s.converged and max(rel) < 1e-6
        # every root is an eigenvalue of the dense operator.  (Not necessarily its `good` lowest: a Davidson run that starts
        # from singles cannot reach a root whose eigenvector has no singles component at all — here the second IP root, a
        # pure 2h1p state with singles weight 6e-34 in the numpy reference.)
        assert max(np.abs(w - x).min() for x in e) < 1e-8 and abs(e[0] - w[0].real) < 1e-8
    else:
        print(kind, "no root qualifies: the sigma check alone stands")
    # integrals without V_pqrs = V_qpsr are refused, by the name of the symmetry
    rng = np.random.default_rng(3)
    bad = {k: v + 1e-3 * rng.standard_normal(v.shape) for k, v in Vd.items()}
    before = _live()
    with pytest.raises(_lib.PymesError, match="V_pqrs = V_qpsr"):
        quiet(s.apply, fd, bad, r["t2"], *[x[0] for x in _vectors(kind, no, nv, 1, 1)])
    t_bad = r["t2"] + 1e-3 * rng.standard_normal(r["t2"].shape)
    with pytest.raises(_lib.PymesError, match="T_abij = T_baji"):
        quiet(s.apply, fd, Vd, t_bad, *[x[0] for x in _vectors(kind, no, nv, 1, 1)])
    assert _live() == before


# ---- 6. sharding and truncation --------------------------------------------------------------------------------------------------
def test_ip_on_a_sharded_context_ea_refused(gpu_lib):
    from pymes_amd.integral.device import DeviceIntegrals
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 6, 24
    B, eps = synthetic_factors(no, nv, seed=5)
    f = np.diag(eps)
    full = DeviceIntegrals.from_factors(no, B)
    shard = DeviceIntegrals.from_factors(no, B, shard=(1, 2))
    try:
        cc = CCSD(no, delta_e=1e-12)
        res = quiet(cc.solve, f, full, max_iter=200, device_amplitudes=True)
        t1, t2 = res["t1"].get(), res["t2"].get()
        roots = []
        for ints in (full, shard):
            s = _solver("ip", no)
            fd = quiet(cc.get_T1_dressed_fock, f, t1, ints)
            dressed = quiet(cc.get_T1_dressed_V, t1, ints, s.BLOCKS)          # never asks a sharded context for abcd
            roots.append(quiet(s.solve, fd, dressed, ints.ctx.array(t2)))
            assert s.converged
        print("IP roots replicated / sharded", roots)
        assert np.abs(roots[0] - roots[1]).max() < 1e-12
        # EA on the sharded context: refused by the name of the mode before anything is dressed (dressing abic or abcd would
        # need the whole V_abcd) — by the solver and by the engine
        from pymes_amd.solver.eom_ip_ea import IPEASigma
        ea = _solver("ea", no)
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            quiet(ea.solve, fd, dressed, shard.ctx.array(t2))
        with pytest.raises(_lib.PymesError, match="integral sharding"):
            IPEASigma(shard.ctx, _kind_id("ea"), fd, shard.ctx.array(t2), dressed=True)
    finally:
        full.ctx.close()
        shard.ctx.close()


def test_ccsd_solve_ip_ea_roots_and_fno(gpu_lib):
    from pymes_amd.solver.ccsd import CCSD
    no, nv = 5, 12
    f, V, _, _ = synthetic_case(no, nv, seed=4)
    cc = CCSD(no, delta_e=1e-12)
    tight = dict(max_iter=200, ip_roots=2, ea_roots=2, ip_ea_r_epsilon=1e-9)     # (for the comparison of two solves at 1e-8)
    plain = quiet(cc.solve, f, V, max_iter=200, ip_roots=2, ea_roots=2)
    assert len(plain["ip e"]) == 2 and len(plain["ea e"]) == 2
    assert plain["qp gap"] == plain["ip e"][0] + plain["ea e"][0]
    assert cc.ip_solver.converged and cc.ea_solver.converged
    only_ip = quiet(cc.solve, f, V, max_iter=200, ip_roots=1)
    assert "ea e" not in only_ip and "qp gap" not in only_ip and "ip e" in only_ip
    # (one root against the first of two: two Davidson runs, each stopped at a relative residual of 1e-6)
    assert abs(only_ip["ip e"][0] - plain["ip e"][0]) < 1e-6 * abs(plain["ip e"][0])
    assert "ip e" not in quiet(cc.solve, f, V, max_iter=200)
    # a truncation that keeps fewer virtuals returns the keys of the correlated space
    cut = quiet(cc.solve, f, V, max_iter=200, ip_roots=2, ea_roots=2, fno_nv=8)
    assert cut["fno nv"] == 8 and len(cut["ip e"]) == 2 and cut["qp gap"] == cut["ip e"][0] + cut["ea e"][0]
    # fno_nv = nv is a rotation of the virtuals: the spectrum is invariant
    ref = quiet(cc.solve, f, V, **tight)
    assert cc.ip_solver.r_epsilon == 1e-9 and np.all(cc.ip_solver.residual_norms < 1e-9)
    assert np.abs(ref["ip e"] - plain["ip e"]).max() < 1e-6 and np.abs(ref["ea e"] - plain["ea e"]).max() < 1e-6
    rot = quiet(cc.solve, f, V, fno_nv=nv, **tight)
    print("ip", ref["ip e"], rot["ip e"], "ea", ref["ea e"], rot["ea e"])
    assert rot["fno nv"] == nv
    assert np.abs(rot["ip e"] - ref["ip e"]).max() < 1e-8 and np.abs(rot["ea e"] - ref["ea e"]).max() < 1e-8
    assert abs(rot["qp gap"] - ref["qp gap"]) < 2e-8
    # with (T) and a frozen core in the same call
    both = quiet(cc.solve, f, V, max_iter=200, triples=True, frozen_core=1, ip_roots=1, ea_roots=1)
    assert "(t) e" in both and len(both["ip e"]) == 1 and both["qp gap"] == both["ip e"][0] + both["ea e"][0]
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(no, is_dcsd=True).solve(f, V, ip_roots=1)


# ---- 7. housekeeping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_handle_lifetime(gpu_lib, kind):
    from pymes_amd.device import Context
    from pymes_amd.solver.eom_ip_ea import IPEASigma
    E = _lib.PymesError
    no, nv = 3, 8
    f, V, t1, t2 = _sym_case(no, nv, seed=2)
    Vb = oc.split_blocks(no, V)
    s = _solver(kind, no)
    before = _live()
    ctx = Context(no, nv)
    try:
        d2 = ctx.array(t2)
        missing = "iabc"
        for name in s.BLOCKS:
            if name != missing:
                ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        with_blocks = _live()
        with pytest.raises(E, match="'iabc'"):
            IPEASigma(ctx, _kind_id(kind), f, d2)
        assert _live() == with_blocks
        ctx.set_V_block(missing, np.ascontiguousarray(Vb[missing]))
        assert ctx.graphs_supported()
        ctx.graph_begin()
        try:
            held = _live()
            with pytest.raises(E, match="launch graph"):
                IPEASigma(ctx, _kind_id(kind), f, d2)
            assert _live() == held
        finally:
            ctx.graph_abort()
        sig = IPEASigma(ctx, _kind_id(kind), f, d2)
        r1s, r2s = _vectors(kind, no, nv, 1, 4)
        a1, a2 = ctx.array(r1s[0]), ctx.array(r2s[0])
        o1, o2 = ctx.empty(a1.shape), ctx.empty(a2.shape)
        first = [x.get() for x in sig.apply_many([a1], [a2])[0]]
        ctx.graph_begin()
        try:
            held = _live()
            with pytest.raises(E, match="launch graph"):
                sig.apply_many([a1], [a2], out1=[o1], out2=[o2])
            assert _live() == held
        finally:
            ctx.graph_abort()
        again = [x.get() for x in sig.apply_many([a1], [a2])[0]]
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        sig.close()
        with pytest.raises(E, match="destroyed"):                       # a handle does not outlive a close() ...
            sig.apply_many([a1], [a2])
        sig = IPEASigma(ctx, _kind_id(kind), f, d2)
    finally:
        ctx.close()
    with pytest.raises(E, match="destroyed"):                           # ... nor its context
        sig.apply_many([a1], [a2])
    sig.close()
    assert _live() == before
    with pytest.raises(KeyError, match="iabc"):                         # the host-dictionary form names the block too
        quiet(s.solve, f, {k: v for k, v in Vb.items() if k != "iabc"}, t2)
    assert _live() == before


@pytest.mark.parametrize("kind", KINDS)
def test_two_identical_solves_return_identical_bits(gpu_lib, kind):
    no, nv = 4, 10
    f, V, _, _ = synthetic_case(no, nv, seed=1)
    r, fd, Vd = R.converged_case(no, f, V, delta_e=1e-12)
    runs = []
    for _ in range(2):
        s = _solver(kind, no)
        e = quiet(s.solve, fd, Vd, r["t2"])
        runs.append((e, s.residual_norms, s.r_singles, s.r_doubles, np.array(s.history)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][4], runs[1][4])
    for a, b in zip(runs[0][2] + runs[0][3], runs[1][2] + runs[1][3]):
        assert np.array_equal(a, b)
