"""The CCSD two-particle density on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device amplitudes, then on the
integrals' context the time of the density blocks without abcd (pymes_rdm2), of the same with the dense abcd block (the
difference is the abcd build), of the two-body expectation value against the resident integrals (pymes_rdm2_expectation: the
blocks, their contraction and the pair-packed abcd part) and, as the yardstick, of one Lambda left apply on a sigma handle of
the same context.  The density is a formula in (t1, t2, lambda1, lambda2): the left vectors are random exchange-symmetric ones.
Times are host wall clock around a device synchronisation, best of --repeat; the executed GEMM flops come from pymes_stats.
Usage: python tools/probe_rdm2.py [--sizes 30x120,50x200] [--out profiles/rdm2/probe_rdm2.txt]"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.model import synthetic  # noqa: E402
from pymes_amd.solver.ccsd import CCSD  # noqa: E402
from pymes_amd.solver.lambda_ccsd import (RDM2_STORED, Lambda_CCSD, LeftSigma, device_expectation2,  # noqa: E402
                                          device_rdm2)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def best_of(ctx, fn, repeat):
    best = None
    for _ in range(repeat):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def probe(no, nv, repeat, emit):
    B, eps = synthetic.factors(no, nv, seed=0)
    f = np.diag(eps)
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
        cc = CCSD(no, delta_e=1e-8)
        res = quiet(cc.solve, f, ints, device_amplitudes=True)
        emit("(%d,%d): E_CCSD = %.10f" % (no, nv, res["ccsd e"]))
        t1, t2 = res["t1"], res["t2"]
        rng = np.random.default_rng(1)
        u2 = 0.05 * rng.standard_normal((nv, nv, no, no))
        a1, a2 = ctx.array(0.1 * rng.standard_normal((nv, no))), ctx.array(u2 + u2.transpose(1, 0, 3, 2))
        del u2
        times = {}

        def timed(name, fn):
            fn()                                                       # (warm: pooled temporaries, cached plans and packs)
            ctx.stats(reset=True)
            fn()
            st = ctx.stats(reset=True)
            times[name] = best_of(ctx, fn, repeat)
            emit("  %s: %.3f ms, %.3e GEMM flops in %d products (%.1f TF/s), %d explicit copies moving %.2f GB" % (
                name, 1e3 * times[name], st["gemm_flops"], st["gemm_calls"], st["gemm_flops"] / times[name] / 1e12,
                st["permute_calls"], st["permute_bytes"] / 1e9))

        names = tuple(nm for nm in RDM2_STORED if nm != "abcd")
        out = {nm: ctx.empty(ctx.block_shape(nm)) for nm in names}
        timed("rdm2 without abcd", lambda: device_rdm2(ctx, t1, t2, a1, a2, blocks=names, out=out))
        out["abcd"] = ctx.empty(ctx.block_shape("abcd"))
        timed("rdm2 with the dense abcd", lambda: device_rdm2(ctx, t1, t2, a1, a2, blocks=RDM2_STORED, out=out))
        emit("  the abcd build (difference): %.3f ms" % (1e3 * (times["rdm2 with the dense abcd"] - times["rdm2 without abcd"])))
        for arr in out.values():
            arr.free()
        out.clear()
        ctx.trim()
        val = [0.0]

        def expect():
            val[0] = device_expectation2(ctx, t1, t2, a1, a2)
        timed("expectation2 against the resident integrals", expect)
        emit("  sum Gamma V = %.12e" % val[0])
        ctx.trim()
        fd = quiet(cc.get_T1_dressed_fock, f, t1, ints)
        dressed = quiet(cc.get_T1_dressed_V, t1, ints, Lambda_CCSD.BLOCKS)
        sig = LeftSigma(ctx, fd, t2, dressed=True)
        o1, o2 = ctx.empty(a1.shape), ctx.empty(a2.shape)
        timed("one Lambda left apply", lambda: sig.apply_left_many([a1], [a2], [True], out1=[o1], out2=[o2]))
        sig.close()
        left = times["one Lambda left apply"]
        emit("  in left applies: rdm2 without abcd %.2f, expectation2 %.2f" % (
            times["rdm2 without abcd"] / left, times["expectation2 against the resident integrals"] / left))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120,50x200")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="profiles/rdm2/probe_rdm2.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_rdm2: synthetic.factors(seed=0), CCSD delta_e = 1e-8, random exchange-symmetric left vectors")
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.repeat, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
