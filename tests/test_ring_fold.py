"""Ring fold of the symmetry-reduced doubles residual (cc.cpp, residual_slab / residual_finish): the one-index terms
X_ac T_cbij and -X_ki T_abkj (ccd.py:231-232) enter through the operands of the two ring applications instead of through two
streaming products.  The identity in numpy, then the engine on the CPU stand-in for the kernels with the fold on and off
(PYMES_RING_FOLD), where the two forms differ by summation order only."""
import numpy as np
import pytest

from oracle import cc_oracle as oc
from oracle.cases import random_case
from pymes_amd import _lib
from pymes_amd.device import Context

TOL = 1e-11          # relative to max |R|: what tests/test_gpu_big.py asks of the same path against the oracle


@pytest.fixture()
def sim(hostsim_lib, monkeypatch):
    """Route the package's default library to the host simulator for this test only."""
    monkeypatch.setattr(_lib, "_default", hostsim_lib)
    return hostsim_lib


def fold_matrix(Xvv, Xoo):
    """Dx[(c,k),(b,j)] = X_bc d_kj - d_cb X_kj as an (ov) x (ov) pair matrix."""
    v, o = Xvv.shape[0], Xoo.shape[0]
    D = np.zeros((v, o, v, o))
    for k in range(o):
        D[:, k, :, k] += Xvv.T
    for c in range(v):
        D[c, :, c, :] -= Xoo
    return D.reshape(o * v, o * v)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("o,v,seed", [(3, 5, 1), (4, 7, 2), (1, 3, 3), (5, 2, 4)])
def test_fold_identity(o, v, seed, paired):
    """Placing ET_d = Tt_d M / 2 + ET_x / 2 and ET_x = Tx N1 as the assembly does, M -> M + Dx / 2 and N1 -> N1 + Dx / 2 add
    exactly X_ac T_cbij + X_bc T_acij - X_ki T_abkj - X_kj T_abik; in the paired form (M_h = M / 2 stored, the assembly adds
    ET_x / 2 in the direct placement itself) the same is Dx / 4 into M_h.  Arbitrary operands, non-symmetric X."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((v, v, o, o))
    T = T + T.transpose(1, 0, 3, 2)
    Xvv, Xoo = rng.standard_normal((v, v)), rng.standard_normal((o, o))
    ov = o * v
    Tx = T.transpose(0, 3, 1, 2).reshape(ov, ov)                                 # Tx[(a,j),(b,i)] = T_abij
    Ttd = (2 * T - T.transpose(1, 0, 2, 3)).transpose(0, 2, 1, 3).reshape(ov, ov)
    want = (np.einsum("ac,cbij->abij", Xvv, T) + np.einsum("bc,acij->abij", Xvv, T)
            - np.einsum("ki,abkj->abij", Xoo, T) - np.einsum("kj,abik->abij", Xoo, T))
    D = fold_matrix(Xvv, Xoo)

    def assemble(M, N1):
        ETx = Tx @ N1
        if paired:                       # M is M_h; ring_xd_ = 1/2
            ETd, xd = Ttd @ M, 0.5
        else:
            ETd, xd = 0.5 * Ttd @ M + 0.5 * ETx, 0.0
        E, X = ETd.reshape(v, o, v, o), ETx.reshape(v, o, v, o)
        R = E.transpose(0, 2, 1, 3) + E.transpose(2, 0, 3, 1) + X.transpose(0, 2, 3, 1) + X.transpose(2, 0, 1, 3)
        return R + xd * (X.transpose(0, 2, 1, 3) + X.transpose(2, 0, 3, 1))

    M0, N0 = rng.standard_normal((ov, ov)), rng.standard_normal((ov, ov))
    got = assemble(M0 + (0.25 if paired else 0.5) * D, N0 + 0.5 * D) - assemble(M0, N0)
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()


def _case(lib, no, nv, seed):
    f, V, t1, t2 = random_case(no, nv, seed, symmetric=True)
    V = V + 0.05 * np.random.default_rng(seed).standard_normal(V.shape)        # V_pqrs = V_qpsr only
    V = 0.5 * (V + V.transpose(1, 0, 3, 2))
    ctx = Context(no, nv, lib=lib)
    ctx.set_V_pqrs(V)
    ctx.set_orbital_energies(-1.0 - np.arange(no, dtype=float), 1.0 + np.arange(nv, dtype=float))
    return ctx, f, V, t1, t2


def _slab_finish(ctx, dF, dT2, dcd, dT1, second_t2=None):
    """One-rank slab + finish as the C API exposes them; dT1 given: amplitude-side mode (what CCSD.iterate runs)."""
    no, nv = ctx.no, ctx.nv
    ov, npp = no * nv, nv * (nv + 1) // 2
    ETd, ETx, L = ctx.zeros((ov, ov)), ctx.zeros((ov, ov)), ctx.zeros((npp, no * no))
    kw = dict(is_dcd=dcd, dressed=dT1 is not None)
    if dT1 is not None:
        kw.update(t1=dT1, QK=ctx.zeros((ov, no * no)))
    ctx.residual_slab(dF, dT2, ETd, ETx, L, 0, 1, **kw)
    r2 = ctx.empty(dT2.shape)
    ctx.residual_finish(dF, dT2 if second_t2 is None else second_t2, ETd, ETx, L, r2, **kw)
    return r2.get(), (ETd, ETx, L, kw)


# nocc = 3: the simulator's fused pair kernels (one-pass layouts and assembly); nocc = 4: the permutation sequences
@pytest.mark.parametrize("no,nv,seed", [(3, 5, 2), (2, 3, 1), (4, 5, 7)])
def test_fold_on_equals_fold_off(sim, monkeypatch, no, nv, seed):
    """R2 of slab + finish with the fold on and off, and both against the oracle: CCSD with T1 != 0 (amplitude-side
    dressing), DCSD, and the undressed form that the T1 = 0 step runs (Exn then holds nothing at all)."""
    ctx, f, V, t1, t2 = _case(sim, no, nv, seed)
    Vb = oc.split_blocks(no, V)
    fd_ref, Vd_ref = oc.dressed_fock(no, f, t1, Vb), oc.dressed_V(t1, Vb)
    dT1, dT2 = ctx.array(t1), ctx.array(t2)
    for dcd in (False, True):
        for with_t1 in (True, False):
            if with_t1:
                dF = ctx.array(fd_ref)                  # the dressed Fock matrix is not symmetric: X_ki != X_ik
                ctx.dress_V(dT1, ["klij", "iajb", "iabj"])
                ref = oc.ccsd_doubles_residual(no, fd_ref, t2, Vd_ref, is_dcsd=dcd)
            else:
                dF = ctx.array(f)
                ref = oc.ccsd_doubles_residual(no, f, t2, Vb, is_dcsd=dcd)
            out = {}
            for fold in ("0", "1"):
                monkeypatch.setenv("PYMES_RING_FOLD", fold)
                out[fold], _ = _slab_finish(ctx, dF, dT2, dcd, dT1 if with_t1 else None)
            scale = max(1.0, np.abs(ref).max())
            d_fold, d_on, d_off = (np.abs(out["1"] - out["0"]).max(), np.abs(out["1"] - ref).max(),
                                   np.abs(out["0"] - ref).max())
            print(f"({no},{nv}) dcd={dcd} t1={with_t1}: on-off {d_fold:.2e} on-ref {d_on:.2e} off-ref {d_off:.2e} scale {scale:.2e}")
            assert d_fold < TOL * scale, (dcd, with_t1)
            assert d_on < TOL * scale and d_off < TOL * scale, (dcd, with_t1)
    ctx.close()


@pytest.mark.parametrize("no,nv,seed", [(3, 5, 4), (4, 5, 5)])
def test_whole_step_fold_on_equals_fold_off(sim, monkeypatch, no, nv, seed):
    """pymes_ccsd_residuals (what the loop calls): R1 and R2 with the fold on and off, with T1 and as the T1 = 0 step."""
    ctx, f, V, t1, t2 = _case(sim, no, nv, seed)
    dF, dT2 = ctx.array(f), ctx.array(t2)
    for dcd in (False, True):
        for t1_zero in (False, True):
            dT1 = ctx.array(np.zeros_like(t1) if t1_zero else t1)
            out = {}
            for fold in ("0", "1"):
                monkeypatch.setenv("PYMES_RING_FOLD", fold)
                r1, r2 = ctx.empty(t1.shape), ctx.empty(t2.shape)
                ctx.ccsd_residuals(dF, dT1, dT2, r1, r2, is_dcd=dcd, t1_zero=t1_zero)
                out[fold] = (r1.get(), r2.get())
            for a, b in zip(out["0"], out["1"]):
                assert np.abs(a - b).max() < TOL * max(1.0, np.abs(a).max()), (dcd, t1_zero)
    ctx.close()


@pytest.mark.parametrize("no,nv,seed", [(3, 5, 6), (4, 5, 8)])
def test_stale_fold_tag(sim, monkeypatch, no, nv, seed):
    """residual_finish on ANOTHER t2 than the folded slab before it must form X_ac T itself; a second finish of the folded
    slab itself must not."""
    ctx, f, V, t1, t2 = _case(sim, no, nv, seed)
    Vb = oc.split_blocks(no, V)
    dF, dT1 = ctx.array(oc.dressed_fock(no, f, t1, Vb)), ctx.array(t1)
    ctx.dress_V(dT1, ["klij", "iajb", "iabj"])
    t2b = 0.7 * t2 + 0.05 * np.sin(np.arange(t2.size)).reshape(t2.shape)
    t2b = 0.5 * (t2b + t2b.transpose(1, 0, 3, 2))
    dA, dB = ctx.array(t2), ctx.array(t2b)
    for dcd in (False, True):
        monkeypatch.setenv("PYMES_RING_FOLD", "0")
        ref_b, (ETd, ETx, L, kw) = _slab_finish(ctx, dF, dB, dcd, dT1)         # unfolded slab of t2b, kept
        ref_a, _ = _slab_finish(ctx, dF, dA, dcd, dT1)
        monkeypatch.setenv("PYMES_RING_FOLD", "1")
        got_a, (ETdA, ETxA, LA, kwA) = _slab_finish(ctx, dF, dA, dcd, dT1)     # folded slab of t2: the tag names dA
        assert np.abs(got_a - ref_a).max() < TOL * max(1.0, np.abs(ref_a).max())
        r2 = ctx.empty(t2.shape)
        ctx.residual_finish(dF, dB, ETd, ETx, L, r2, **kw)                     # the unfolded slab of another t2
        assert np.abs(r2.get() - ref_b).max() < TOL * max(1.0, np.abs(ref_b).max()), dcd
        ctx.residual_finish(dF, dA, ETdA, ETxA, LA, r2, **kwA)                 # the folded slab once more
        assert np.abs(r2.get() - ref_a).max() < TOL * max(1.0, np.abs(ref_a).max()), dcd
    ctx.close()


def test_pair_sharded_tail_after_a_folded_slab(sim, monkeypatch):
    """World 1 without slab_prepare: the slab is folded, so the pair-sharded tail must not add X_ac T either."""
    no, nv = 3, 5
    ctx, f, V, t1, t2 = _case(sim, no, nv, 9)
    Vb = oc.split_blocks(no, V)
    dF, dT1, dT2 = ctx.array(oc.dressed_fock(no, f, t1, Vb)), ctx.array(t1), ctx.array(t2)
    ctx.dress_V(dT1, ["klij", "iajb", "iabj"])
    npp = nv * (nv + 1) // 2
    for dcd in (False, True):
        out = {}
        for fold in ("0", "1"):
            monkeypatch.setenv("PYMES_RING_FOLD", fold)
            ref, (ETd, ETx, L, kw) = _slab_finish(ctx, dF, dT2, dcd, dT1)
            ctx.residual_slab(dF, dT2, ETd, ETx, L, 0, 1, **kw)
            Rall = ctx.zeros((npp, 2, no * no))
            ctx.residual_finish_pairs(dF, dT2, ETd, ETx, L, Rall, 0, 1, kw["t1"], kw["QK"], is_dcd=dcd, dressed=True)
            full = ctx.pairs_unpack(Rall, ctx.zeros(t2.shape), 1).get()
            assert np.abs(full - ref).max() < TOL * max(1.0, np.abs(ref).max()), (dcd, fold)
            out[fold] = full
        assert np.abs(out["0"] - out["1"]).max() < TOL * max(1.0, np.abs(out["0"]).max())
    ctx.close()


def test_switch_is_read(sim, monkeypatch):
    """Not a comparison of two identical runs: with the fold, slab + finish through the C API issue three products fewer
    (Td X_ki, X_ac T, and the S_ac sum that a finish without PYMES_REUSE_LAYOUTS forms for X_ac) and move fewer bytes in
    explicit copies (no Td layout, no private Tt_d in the finish)."""
    no, nv = 3, 5
    ctx, f, V, t1, t2 = _case(sim, no, nv, 10)
    Vb = oc.split_blocks(no, V)
    dF, dT1, dT2 = ctx.array(oc.dressed_fock(no, f, t1, Vb)), ctx.array(t1), ctx.array(t2)
    ctx.dress_V(dT1, ["klij", "iajb", "iabj"])
    got = {}
    for fold in ("0", "1"):
        monkeypatch.setenv("PYMES_RING_FOLD", fold)
        ctx.stats(reset=True)
        _slab_finish(ctx, dF, dT2, False, dT1)
        got[fold] = ctx.stats()
    assert got["0"]["gemm_calls"] - got["1"]["gemm_calls"] == 3
    assert got["1"]["permute_bytes"] < got["0"]["permute_bytes"]
    ctx.close()


@pytest.mark.parametrize("no,nv,seed", [(3, 5, 12), (4, 5, 13)])
def test_fold_tag_names_the_slab_not_only_t2(sim, monkeypatch, no, nv, seed):
    """The tag is the pair (t2, ETd) of the last slab call that built or could have built rings: a finish of the SAME t2 on an
    unfolded ETd kept from before forms X_ac T itself, and a later slab call of a rank without columns (it writes nothing,
    but what the caller then finishes came from elsewhere, here copied into the very buffers the tag named) clears the tag."""
    ctx, f, V, t1, t2 = _case(sim, no, nv, seed)
    Vb = oc.split_blocks(no, V)
    dF, dT1, dT2 = ctx.array(oc.dressed_fock(no, f, t1, Vb)), ctx.array(t1), ctx.array(t2)
    ctx.dress_V(dT1, ["klij", "iajb", "iabj"])
    ov = no * nv
    for dcd in (False, True):
        monkeypatch.setenv("PYMES_RING_FOLD", "0")
        ref, (ETd0, ETx0, L0, kw0) = _slab_finish(ctx, dF, dT2, dcd, dT1)       # unfolded slab, kept
        monkeypatch.setenv("PYMES_RING_FOLD", "1")
        got, (ETd1, ETx1, L1, kw1) = _slab_finish(ctx, dF, dT2, dcd, dT1)       # folded slab of the same t2 in other buffers
        scale = max(1.0, np.abs(ref).max())
        assert np.abs(got - ref).max() < TOL * scale
        r2 = ctx.empty(t2.shape)
        ctx.residual_finish(dF, dT2, ETd0, ETx0, L0, r2, **kw0)                 # same t2, the unfolded slab
        assert np.abs(r2.get() - ref).max() < TOL * scale, dcd
        # rank ov of world ov + 1 has no columns and no ladder rows to speak of: the call returns early, the tag is gone
        world = ov + 1
        pad = -(-ov // world) * world
        ctx.residual_slab(dF, dT2, ctx.zeros((pad, ov)), ctx.zeros((pad, ov)), None, world - 1, world, **kw1)
        ETd1.set(ETd0.get())                                                    # the folded slab's buffers, refilled with
        ETx1.set(ETx0.get())                                                    # rows that do not carry the terms
        ctx.residual_finish(dF, dT2, ETd1, ETx1, L1, r2, **kw1)
        assert np.abs(r2.get() - ref).max() < TOL * scale, dcd
    ctx.close()
