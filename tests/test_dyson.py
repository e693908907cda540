"""CPU: the numpy reference of the left IP / EA vectors and the Dyson amplitudes (tests/_dyson_reference.py, the GPU tests'
oracle): the written-out terms against the definition, the sum rules, the exact two-electron residues, the adjoint tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg

from oracle import cc_oracle as oc
from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _dyson_reference as D
from tests import _ipea_reference as IR
from tests import _lambda_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ip", "ea")
SHAPES = ((2, 3), (3, 5))


def random_inputs(kind, no, nv, seed, k=2):
    """(t1, t2, (lam1, lam2), ls, rs): random, exchange-symmetric T2 and Lambda2; they solve nothing."""
    rng = np.random.default_rng(seed)
    t1, t2, l1, l2 = LR.density_inputs(no, nv, seed)
    s1, s2 = IR.shapes(kind, no, nv)
    vec = lambda: (rng.standard_normal(s1), rng.standard_normal(s2))
    return t1, t2, (l1, l2), [vec() for _ in range(k)], [vec() for _ in range(k)]


@pytest.mark.parametrize("no,nv", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_terms_against_the_definition(kind, no, nv):
    t1, t2, lam, ls, rs = random_inputs(kind, no, nv, 31 + no)
    pl, pr = D.dyson_definition(kind, no, t1, t2, lam, ls, rs)
    for z in range(len(ls)):
        tl, tr = D.dyson_terms(kind, no, t1, t2, lam[0], lam[1], ls[z], rs[z])
        assert np.abs(tl - pl[z]).max() < 1e-12
        assert np.abs(tr - pr[z]).max() < 1e-12
    assert np.abs(pl).max() > 1e-2 and np.abs(pr).max() > 1e-2


@pytest.mark.parametrize("no,nv", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_b_vectors_are_the_unit_singles_and_the_amplitudes(kind, no, nv):
    t1, t2, lam, _, _ = random_inputs(kind, no, nv, 5)
    B, _ = D.dyson_matrices(kind, no, t1, t2, lam[0], lam[1])
    n1 = no if kind == "ip" else nv
    own = slice(0, no) if kind == "ip" else slice(no, no + nv)
    assert np.array_equal(B[:n1, own], np.eye(n1)) and not B[n1:, own].any()
    for p in range(nv if kind == "ip" else no):
        if kind == "ip":
            want = np.concatenate([t1[p], t2[p].transpose(1, 2, 0).ravel()])
            got = B[:, no + p]
        else:
            want = -np.concatenate([t1[:, p], t2[:, :, p, :].ravel()])
            got = B[:, p]
        assert np.abs(got - want).max() < 1e-15


@pytest.mark.parametrize("no,nv", ((2, 3), (3, 4), (3, 5)))
@pytest.mark.parametrize("kind", KINDS)
def test_sum_rule(kind, no, nv):
    t1, t2, lam, _, _ = random_inputs(kind, no, nv, 17)
    B, E = D.dyson_matrices(kind, no, t1, t2, lam[0], lam[1])
    assert np.abs(E.T @ B - D.sum_rule(kind, no, t1, t2, lam[0], lam[1])).max() < 1e-12


def test_koopmans_limit():
    """Without T and Lambda every unit single has amplitude one on its own orbital and nothing else."""
    for kind in KINDS:
        no, nv = 2, 3
        z1, z2 = np.zeros((nv, no)), np.zeros((nv, nv, no, no))
        B, E = D.dyson_matrices(kind, no, z1, z2, z1, z2)
        assert np.array_equal(B, E)
        n1 = no if kind == "ip" else nv
        assert np.abs(B.T @ B - np.diag(([1.0] * no + [0.0] * nv) if kind == "ip" else ([0.0] * no + [1.0] * nv))).max() == 0.0
        assert B[:n1].sum() == n1


@pytest.mark.parametrize("no,nv", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_tables_against_the_transposed_matrix(kind, no, nv):
    f, V = LR.random_problem(no, nv, 7 + nv, eight=False)
    _, fd, Vd = IR.converged_case(no, f, V, delta_e=1e-12)
    t2 = LR.density_inputs(no, nv, 3)[1]
    H = IR.dense(kind, no, fd, Vd, t2)
    rng = np.random.default_rng(9)
    l = D.split(kind, no, nv, rng.standard_normal(H.shape[0]))
    got = D.flat(D.left_sigma_terms(kind, no, fd, Vd, t2, *l))
    want = H.T @ D.flat(l)
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(H - H.T).max() > 1e-3


def test_two_electron_residues():
    """Two electrons: CCSD is exact, so the IP poles are eps_k(h) - E0 and the residue matrices d d^T with d = C0 phi_k."""
    c = D.reference_case("ip", 1, 3, 3, True, None, 0.05)
    w, d = D.two_electron_dyson(c["f"], c["V"])
    assert c["imag"] == 0.0
    assert np.abs(c["w"][:3] - w[:3]).max() < 1e-10
    Z = D.residues(c["psiL"], c["psiR"])
    for k in range(3):
        assert np.abs(Z[k] - np.outer(d[k], d[k])).max() < 1e-10
    P = D.pole_strengths(c["psiL"], c["psiR"])
    assert np.abs(P[:3] - np.array([0.97416896, 0.00559696, 0.01051013])).max() < 1e-8


@pytest.mark.parametrize("eight", (True, False))
@pytest.mark.parametrize("kind", KINDS)
def test_dense_spectrum_sums_to_the_sum_rule(kind, eight):
    """sum_k Z_k over the complete spectrum (complex-conjugate pairs of the non-hermitian problems included: the plain,
    unconjugated product pairs l_k with r_k) is E^T B."""
    no, nv = 2, 3
    c = D.reference_case(kind, no, nv, 11, eight, 2)
    H = IR.dense(kind, no, c["fd"], c["Vd"], c["t2"])
    w, vl, vr = scipy.linalg.eig(H, left=True)
    L = np.conj(vl)
    L = L @ np.linalg.inv(L.T @ vr).T
    B, E = D.dyson_matrices(kind, no, c["t1"], c["t2"], *c["lam"])
    Z = np.einsum("ck,cq,dk,dp->qp", vr, E, L, B)
    want = D.sum_rule(kind, no, c["t1"], c["t2"], *c["lam"])
    assert np.abs(Z - want).max() < 1e-6
    assert abs(np.trace(Z) - (no if kind == "ip" else nv)) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_spectral_function_integrates_to_the_residues(kind):
    c = D.reference_case(kind, 2, 3, 11, True, 2)
    assert c["imag"] == 0.0
    om = np.linspace(-60.0, 60.0, 240001)
    A = D.spectral_function(kind, c["w"], c["psiL"], c["psiR"], om, 0.01)
    assert np.abs(A.sum(axis=0) * (om[1] - om[0]) - D.residues(c["psiL"], c["psiR"]).sum(axis=0)).max() < 1e-3
    P = D.pole_strengths(c["psiL"], c["psiR"])
    assert np.all(P > 0.0) and np.all(P <= 1.0)


# ---- the library's side, without a GPU -------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    for name in ("pymes_ipea_sigma_apply_left", "pymes_ipea_dyson"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES
    for doc, word in (("README.md", "IP_EOM_CCSD_Dyson"), ("DESIGN.md", "## 8f."), ("INTEGRATION.md", "pymes_ipea_dyson")):
        assert word in open(os.path.join(ROOT, doc)).read()


def test_solver_refusals_need_no_context():
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.eom_dyson import EA_EOM_CCSD_Dyson, IP_EOM_CCSD_Dyson

    class Ctx:
        shard, recording = (0, 2), False
    with pytest.raises(_lib.PymesError, match="EA-EOM-CCSD Dyson: not available with integral sharding"):
        EA_EOM_CCSD_Dyson(2).check_context(Ctx, True)
    with pytest.raises(_lib.PymesError, match="pass lam="):
        IP_EOM_CCSD_Dyson(2).check_context(Ctx, False)
    IP_EOM_CCSD_Dyson(2).check_context(Ctx, True)
    Ctx.shard, Ctx.recording = None, True
    with pytest.raises(_lib.PymesError, match="recording a launch graph"):
        IP_EOM_CCSD_Dyson(2).check_context(Ctx, True)
    assert "abcd" not in IP_EOM_CCSD_Dyson.blocks(False) and "abcd" in IP_EOM_CCSD_Dyson.blocks(True)
    assert set(EA_EOM_CCSD_Dyson.blocks(True)) == set(IP_EOM_CCSD_Dyson.blocks(True))
    f = np.zeros((5, 5))
    with pytest.raises(ValueError, match="dyson=True needs ip_roots"):
        CCSD(2).solve(f, None, dyson=True)
    with pytest.raises(ValueError, match="DCSD"):
        CCSD(2, is_dcsd=True).solve(f, None, ip_roots=1, dyson=True)
    with pytest.raises(RuntimeError, match="finished solve"):
        IP_EOM_CCSD_Dyson(2).residues()


@pytest.mark.parametrize("kind", KINDS)
def test_new_kernels_refuse_by_name_in_the_host_backend(hostsim_lib, kind):
    """The CPU stand-in links unchanged: the engine's weak defaults of the new kernels throw by name, and nothing stays
    allocated behind a refused call."""
    from pymes_amd.solver import eom_ip_ea as M
    K = M.KIND_IP if kind == "ip" else M.KIND_EA
    no, nv = 3, 4
    f, V = LR.random_problem(no, nv, 5, eight=False)
    Vb = oc.split_blocks(no, V)
    t1, t2, l1, l2 = LR.density_inputs(no, nv, 2)
    ctx = Context(no, nv, lib=hostsim_lib)
    try:
        for name in M.IPEASigma.BLOCKS[K]:
            ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        sig = M.IPEASigma(ctx, K, f, ctx.array(t2))
        x1, x2 = ctx.zeros(sig.shape1), ctx.zeros(sig.shape2)
        args = (ctx.array(t1), ctx.array(l1), ctx.array(l2), [x1], [x2], [x1], [x2])
        n = C.c_int64()
        live = lambda: (hostsim_lib.call("pymes_live_allocations", C.byref(n)), int(n.value))[1]
        held = live()
        with pytest.raises(_lib.PymesError, match="ipea_pack: not available in this backend"):
            sig.apply_left_many([x1], [x2])
        with pytest.raises(_lib.PymesError, match="ipea_pack: not available in this backend"):
            sig.dyson(*args)
        with pytest.raises(_lib.PymesError, match="output aliases input"):
            sig.apply_left_many([x1], [x2], out1=[x1], out2=[x2])
        ctx.lib.call("pymes_scratch_trim", ctx.handle)
        assert live() <= held + 2          # (the two outputs of the first refused call)
        sig.close()
    finally:
        ctx.close()
