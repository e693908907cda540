"""CCSD Lambda equations on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device amplitudes, then on ONE handle
of the sigma build the time of prepare (the hoist), of one right apply and of one left apply (same vector, same process, so
the ratio is that of one visit to one device), of a full Lambda solve and of the density.  Times are host wall clock around a
device synchronisation, best of --repeat; the executed GEMM flops of each apply come from pymes_stats.
Usage: python tools/probe_lambda.py [--sizes 30x120,50x200] [--out profiles/lambda/probe_lambda.txt]"""
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
from pymes_amd.solver.lambda_ccsd import Lambda_CCSD, LeftSigma  # noqa: E402


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
        fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], ints)
        dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, Lambda_CCSD.BLOCKS)
        emit("(%d,%d): E_CCSD = %.10f" % (no, nv, res["ccsd e"]))
        ctx.sync()
        t0 = time.perf_counter()
        sig = LeftSigma(ctx, fd, res["t2"], dressed=True)
        ctx.sync()
        emit("  prepare %.4f s" % (time.perf_counter() - t0))
        rng = np.random.default_rng(1)
        u2 = rng.standard_normal((nv, nv, no, no))
        a1, a2 = ctx.array(rng.standard_normal((nv, no))), ctx.array(u2 + u2.transpose(1, 0, 3, 2))
        o1, o2 = ctx.empty(a1.shape), ctx.empty(a2.shape)
        times = {}
        for name, fn in (("right", lambda: sig.apply_many([a1], [a2], [True], out1=[o1], out2=[o2])),
                         ("left", lambda: sig.apply_left_many([a1], [a2], [True], out1=[o1], out2=[o2]))):
            fn()                                                   # (warm: pooled temporaries, cached plans, the ladder test)
            ctx.stats(reset=True)
            fn()
            st = ctx.stats(reset=True)
            times[name] = best_of(ctx, fn, repeat)
            emit("  %s apply: %.3f ms, %.3e GEMM flops in %d products (%.1f TF/s), %d explicit copies moving %.2f GB" % (
                name, 1e3 * times[name], st["gemm_flops"], st["gemm_calls"], st["gemm_flops"] / times[name] / 1e12,
                st["permute_calls"], st["permute_bytes"] / 1e9))
        emit("  left / right = %.3f" % (times["left"] / times["right"]))
        sig.close()
        ctx.trim()
        s = Lambda_CCSD(no)
        ctx.sync()
        t0 = time.perf_counter()
        out = quiet(s.solve, fd, dressed, res["t2"], eps=(eps[:no].copy(), eps[no:].copy()))
        ctx.sync()
        emit("  Lambda solve: %.3f s, %d iterations, converged %s, |eta + A^T lambda| = %.2e" % (
            time.perf_counter() - t0, out["iterations"], out["converged"], out["residual norm"]))
        ctx.sync()
        t0 = time.perf_counter()
        g = s.rdm1(res["t1"], ctx=ctx)
        emit("  density: %.4f s (with the upload of lambda), trace - 2 no = %.2e, largest natural occupation of a virtual %.5f" % (
            time.perf_counter() - t0, np.trace(g) - 2 * no, np.linalg.eigvalsh(0.5 * (g + g.T))[::-1][no]))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120,50x200")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="profiles/lambda/probe_lambda.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_lambda: synthetic.factors(seed=0), CCSD delta_e = 1e-8, lambda r_epsilon = 1e-8")
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.repeat, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
