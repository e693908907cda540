"""GPU: the ring fold of the doubles residual (cc.cpp, residual_slab / residual_finish; tests/test_ring_fold.py has the
identity and the host logic) on the HIP kernels: the strided accumulations of the sparse pair matrix into the ring operands,
the products that follow, and the assembly that starts from an Exn without X_ac T — fold on against fold off
(PYMES_RING_FOLD), which differ by summation order only."""
import numpy as np
import pytest

from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.model import synthetic

pytestmark = pytest.mark.gpu
TOL = 1e-11          # relative to max |R| (tests/test_gpu_big.py asks the same of this path against the oracle)


# (20,80): 169 tiles per ring product, the paired form (M_h, Dx / 4);  (30,120): 841 tiles, the unpaired form (Dx / 2)
@pytest.mark.parametrize("no,nv", [(20, 80), (30, 120)])
def test_fold_on_equals_fold_off(gpu_lib, monkeypatch, no, nv):
    B, eps = synthetic.factors(no, nv, seed=0)
    rng = np.random.default_rng(17)
    n = no + nv
    f = np.diag(eps) + 0.02 * rng.standard_normal((n, n))              # not symmetric: X_ki != X_ik, X_ac != X_ca
    t1 = 0.02 * rng.standard_normal((nv, no))
    t2 = 0.05 * rng.standard_normal((nv, nv, no, no))
    t2 = 0.5 * (t2 + t2.transpose(1, 0, 3, 2))
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
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
                    r1.free()
                    r2.free()
                for name, a, b in zip(("R1", "R2"), out["0"], out["1"]):
                    d, scale = np.abs(a - b).max(), max(1.0, np.abs(a).max())
                    print(f"({no},{nv}) dcd={dcd} t1_zero={t1_zero} {name}: |on - off| = {d:.3e}, max |R| = {np.abs(a).max():.3e}")
                    assert d < TOL * scale, (name, dcd, t1_zero)
                # the fold must have changed something to compare: X_ac T and X_ki T are far above the tolerance
                assert np.abs(out["0"][1]).max() > 1e-3
                dT1.free()
    finally:
        ctx.close()


def test_slab_and_finish_one_by_one(gpu_lib, monkeypatch):
    """The two halves through the C API without PYMES_REUSE_LAYOUTS, and a finish on another t2 after a folded slab."""
    no, nv = 20, 80
    B, eps = synthetic.factors(no, nv, seed=1)
    rng = np.random.default_rng(5)
    n, ov, npp = no + nv, no * nv, nv * (nv + 1) // 2
    f = np.diag(eps) + 0.02 * rng.standard_normal((n, n))
    sym = lambda t: 0.5 * (t + t.transpose(1, 0, 3, 2))
    t2a, t2b = sym(0.05 * rng.standard_normal((nv, nv, no, no))), sym(0.05 * rng.standard_normal((nv, nv, no, no)))
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
        dF, dA, dB = ctx.array(f), ctx.array(t2a), ctx.array(t2b)

        def slab(dT2):
            ETd, ETx, L = ctx.empty((ov, ov)), ctx.empty((ov, ov)), ctx.empty((npp, no * no))
            ctx.residual_slab(dF, dT2, ETd, ETx, L, 0, 1)
            return ETd, ETx, L

        def finish(dT2, bufs):
            return ctx.residual_finish(dF, dT2, *bufs, ctx.empty(t2a.shape)).get()
        monkeypatch.setenv("PYMES_RING_FOLD", "0")
        bufs_b = slab(dB)
        ref_b = finish(dB, bufs_b)
        ref_a = finish(dA, slab(dA))
        monkeypatch.setenv("PYMES_RING_FOLD", "1")
        bufs_a = slab(dA)                                    # folded: the tag names dA
        got_b = finish(dB, bufs_b)                           # the unfolded slab of another t2: X_ac T formed here
        got_a = finish(dA, bufs_a)
        for got, ref in ((got_a, ref_a), (got_b, ref_b)):
            d = np.abs(got - ref).max()
            print(f"|on - off| = {d:.3e}, max |R| = {np.abs(ref).max():.3e}")
            assert d < TOL * max(1.0, np.abs(ref).max())
    finally:
        ctx.close()
