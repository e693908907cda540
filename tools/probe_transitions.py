"""Left EOM-CCSD vectors and transition densities on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device
amplitudes, then on ONE handle of the sigma build a stacked left apply of k = 3 vectors against three k = 1 calls (same vectors,
same handle, same process, so the ratio is that of one visit to one device), then the whole transition solve (right vectors,
Lambda, left vectors) and the density call alone.  Times are host wall clock around a device synchronisation, best of --repeat;
GEMM launches and explicit copies come from pymes_stats.
Usage: python tools/probe_transitions.py [--sizes 30x120] [--out profiles/transitions/probe_transitions.txt]"""
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
from pymes_amd.solver.eom_transitions import EOM_CCSD_Transitions, device_tdm1  # noqa: E402
from pymes_amd.solver.lambda_ccsd import LeftSigma  # noqa: E402


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


def probe(no, nv, repeat, k, r_epsilon, emit):
    B, eps = synthetic.factors(no, nv, seed=0)
    f = np.diag(eps)
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
        cc = CCSD(no, delta_e=1e-8)
        res = quiet(cc.solve, f, ints, device_amplitudes=True)
        fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], ints)
        dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, EOM_CCSD_Transitions.BLOCKS)
        emit("(%d,%d): E_CCSD = %.10f" % (no, nv, res["ccsd e"]))
        sig = LeftSigma(ctx, fd, res["t2"], dressed=True)
        rng = np.random.default_rng(1)
        a1, a2 = [], []
        for _ in range(k):
            u2 = rng.standard_normal((nv, nv, no, no))
            a1.append(ctx.array(rng.standard_normal((nv, no))))
            a2.append(ctx.array(u2 + u2.transpose(1, 0, 3, 2)))
        o1, o2 = [ctx.empty(x.shape) for x in a1], [ctx.empty(x.shape) for x in a2]

        def looped():
            for z in range(k):
                sig.apply_left_many([a1[z]], [a2[z]], [True], out1=[o1[z]], out2=[o2[z]])

        def stacked():
            sig.apply_left_many(a1, a2, [True] * k, out1=o1, out2=o2)
        times = {}
        for name, fn in (("looped", looped), ("stacked", stacked)):
            fn()                                                   # (warm: pooled temporaries, cached plans, the packed V+ / V-)
            ctx.stats(reset=True)
            fn()
            st = ctx.stats(reset=True)
            times[name] = best_of(ctx, fn, repeat)
            emit("  left apply, k = %d %s: %.3f ms, %.3e GEMM flops in %d products (%.1f TF/s), %d explicit copies moving %.2f GB" % (
                k, name, 1e3 * times[name], st["gemm_flops"], st["gemm_calls"], st["gemm_flops"] / times[name] / 1e12,
                st["permute_calls"], st["permute_bytes"] / 1e9))
        emit("  stacked / looped = %.3f" % (times["stacked"] / times["looped"]))
        sig.close()
        del a1, a2, o1, o2
        ctx.trim()
        s = EOM_CCSD_Transitions(no, n_excit=k, r_epsilon=r_epsilon)
        ctx.sync()
        t0 = time.perf_counter()
        out = quiet(s.solve, fd, dressed, res["t2"], res["t1"], eps=(eps[:no].copy(), eps[no:].copy()))
        ctx.sync()
        emit("  transition solve (right, Lambda, left, densities): %.3f s, passes %s, Lambda iterations %d, converged %s" % (
            time.perf_counter() - t0, out["iterations"], s.lambda_solver.iterations, out["converged"]))
        emit("  w = %s" % np.array2string(out["e"], precision=8))
        emit("  right residuals %s  left residuals %s  biorthogonality %.2e" % (
            np.array2string(out["right residual"], precision=2), np.array2string(out["left residual"], precision=2),
            out["biorthogonality"]))
        up = ctx.array
        args = (up(res["t1"].get()), res["t2"], up(out["lambda1"]), up(out["lambda2"]), [up(x) for x in out["l1"]],
                [up(x) for x in out["l2"]], [up(x) for x in out["r1"]], [up(x) for x in out["r2"]])
        device_tdm1(ctx, *args)
        emit("  densities of %d roots (pymes_tdm1, with the read-back of 2 k n^2 numbers): %.3f ms" % (
            k, 1e3 * best_of(ctx, lambda: device_tdm1(ctx, *args), repeat)))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--roots", type=int, default=3)
    ap.add_argument("--r-epsilon", type=float, default=1e-6)
    ap.add_argument("--out", default="profiles/transitions/probe_transitions.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_transitions: synthetic.factors(seed=0), CCSD delta_e = 1e-8, r_epsilon = %g, %d roots" % (a.r_epsilon, a.roots))
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.repeat, a.roots, a.r_epsilon, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
