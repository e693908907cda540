"""Left IP / EA-EOM-CCSD vectors and Dyson amplitudes on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device
amplitudes, then per kind on ONE handle of the sigma build: prepare, a stacked right apply of k = 3 vectors, a stacked left apply
of the same vectors, three k = 1 left applies (same handle, same process, so the ratios are those of one visit to one device), the
whole solve (right vectors, Lambda for the first kind only, left vectors, amplitudes) and the amplitude call alone.  The left apply
runs the right apply's products with one operand exchanged, so the right apply next to it is what it is compared with.  Times are
host wall clock around a device synchronisation, best of --repeat; GEMM launches and explicit copies come from pymes_stats.
Usage: python tools/probe_dyson.py [--sizes 30x120] [--out profiles/dyson/probe_dyson.txt]"""
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
from pymes_amd.solver.eom_dyson import EA_EOM_CCSD_Dyson, IP_EOM_CCSD_Dyson  # noqa: E402
from pymes_amd.solver.eom_ip_ea import IPEASigma  # noqa: E402


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
        emit("(%d,%d): E_CCSD = %.10f" % (no, nv, res["ccsd e"]))
        lam = None
        for cls in (IP_EOM_CCSD_Dyson, EA_EOM_CCSD_Dyson):
            s = cls(no, n_roots=k, r_epsilon=r_epsilon)
            dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, s.blocks(lam is None))
            ctx.sync()
            t0 = time.perf_counter()
            sig = IPEASigma(ctx, s.KIND, fd, res["t2"], dressed=True)
            ctx.sync()
            emit(" %s: prepare %.3f ms" % (s.NAME, 1e3 * (time.perf_counter() - t0)))
            rng = np.random.default_rng(1)
            a1 = [ctx.array(rng.standard_normal(sig.shape1)) for _ in range(k)]
            a2 = [ctx.array(rng.standard_normal(sig.shape2)) for _ in range(k)]
            o1, o2 = [ctx.empty(x.shape) for x in a1], [ctx.empty(x.shape) for x in a2]

            def looped():
                for z in range(k):
                    sig.apply_left_many([a1[z]], [a2[z]], out1=[o1[z]], out2=[o2[z]])
            times = {}
            for name, fn in (("right apply, stacked", lambda: sig.apply_many(a1, a2, out1=o1, out2=o2)),
                             ("left apply, stacked", lambda: sig.apply_left_many(a1, a2, out1=o1, out2=o2)),
                             ("left apply, looped", looped)):
                fn()                                                   # (warm: pooled temporaries, cached plans)
                ctx.stats(reset=True)
                fn()
                st = ctx.stats(reset=True)
                times[name] = best_of(ctx, fn, repeat)
                emit("  %s, k = %d: %.3f ms, %.3e GEMM flops in %d products (%.1f TF/s), %d explicit copies moving %.3f GB" % (
                    name, k, 1e3 * times[name], st["gemm_flops"], st["gemm_calls"], st["gemm_flops"] / times[name] / 1e12,
                    st["permute_calls"], st["permute_bytes"] / 1e9))
            emit("  left stacked / right stacked = %.3f,  left stacked / left looped = %.3f" % (
                times["left apply, stacked"] / times["right apply, stacked"],
                times["left apply, stacked"] / times["left apply, looped"]))
            sig.close()
            del a1, a2, o1, o2
            ctx.trim()
            ctx.sync()
            t0 = time.perf_counter()
            out = quiet(s.solve, fd, dressed, res["t2"], res["t1"], lam=lam, eps=(eps[:no].copy(), eps[no:].copy()))
            ctx.sync()
            emit("  solve (right%s, left, amplitudes): %.3f s, passes %s, converged %s" % (
                ", Lambda (%d iterations)" % s.lambda_solver.iterations if lam is None else "", time.perf_counter() - t0,
                out["iterations"], out["converged"]))
            lam = (out["lambda1"], out["lambda2"])
            emit("  w = %s  pole strengths = %s" % (np.array2string(out["e"], precision=8),
                                                    np.array2string(out["pole strengths"], precision=6)))
            emit("  right residuals %s  left residuals %s  biorthogonality %.2e" % (
                np.array2string(out["right residual"], precision=2), np.array2string(out["left residual"], precision=2),
                out["biorthogonality"]))
            sig = IPEASigma(ctx, s.KIND, fd, res["t2"], dressed=True)
            up = ctx.array
            args = (up(res["t1"].get()), up(lam[0]), up(lam[1]), [up(x) for x in out["l1"]], [up(x) for x in out["l2"]],
                    [up(x) for x in out["r1"]], [up(x) for x in out["r2"]])
            sig.dyson(*args)
            emit("  amplitudes of %d roots (pymes_ipea_dyson, with the read-back of 2 k n numbers): %.3f ms" % (
                k, 1e3 * best_of(ctx, lambda: sig.dyson(*args), repeat)))
            sig.close()
            del args
            ctx.trim()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--roots", type=int, default=3)
    ap.add_argument("--r-epsilon", type=float, default=1e-6)
    ap.add_argument("--out", default="profiles/dyson/probe_dyson.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_dyson: synthetic.factors(seed=0), CCSD delta_e = 1e-8, r_epsilon = %g, %d roots" % (a.r_epsilon, a.roots))
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.repeat, a.roots, a.r_epsilon, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
