"""IP- and EA-EOM-CCSD on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device amplitudes, then for each
operator the time of prepare (the hoist), of one apply at k = 1 and k = n_roots, and of a three-root solve.  Each apply is
printed next to its own floor: the executed GEMM flops (pymes_stats) over the rate an (ov)^3 ring-shaped product reaches in
the same process, and for EA at k = 1 the bytes of V_abcd over the traffic rate of pymes_copy measured in the same run.
Times are host wall clock around a device synchronisation, best of --repeat.
Usage: python tools/probe_ip_ea.py [--sizes 30x120,50x200] [--roots 3] [--out profiles/ipea/probe_ip_ea.txt]"""
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
from pymes_amd.solver.eom_ip_ea import EA_EOM_CCSD, IP_EOM_CCSD, IPEASigma  # noqa: E402


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


def yardsticks(ctx, no, nv, repeat):
    """(flop/s of an (ov)^3 product, bytes/s of traffic of pymes_copy) in this process."""
    ov = no * nv
    a, b = ctx.zeros((ov, ov)), ctx.zeros((ov, ov))
    c = ctx.empty((ov, ov))
    t = best_of(ctx, lambda: ctx.contract("xk,ky->xy", a, b, out=c), repeat + 1)
    tc = best_of(ctx, lambda: c.copy_from(a), repeat + 1)
    return 2.0 * ov ** 3 / t, 2.0 * 8.0 * ov * ov / tc


def probe(no, nv, roots, repeat, emit):
    B, eps = synthetic.factors(no, nv, seed=0)
    f = np.diag(eps)
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
        cc = CCSD(no, delta_e=1e-8)
        res = quiet(cc.solve, f, ints, device_amplitudes=True)
        fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], ints)
        dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, sorted(set(IP_EOM_CCSD.BLOCKS) | set(EA_EOM_CCSD.BLOCKS)))
        gemm_rate, copy_rate = yardsticks(ctx, no, nv, repeat)
        emit("(%d,%d): E_CCSD = %.10f; ring-shaped GEMM %.1f TF/s, pymes_copy %.2f TB/s of traffic" % (
            no, nv, res["ccsd e"], gemm_rate / 1e12, copy_rate / 1e12))
        for cls in (IP_EOM_CCSD, EA_EOM_CCSD):
            ctx.sync()
            t0 = time.perf_counter()
            sig = IPEASigma(ctx, cls.KIND, fd, res["t2"], dressed=True)
            ctx.sync()
            t_prep = time.perf_counter() - t0
            emit("  %s prepare %.4f s" % (cls.NAME, t_prep))
            for k in sorted({1, roots}):
                vecs = [ctx.zeros((sig.nflat,)) for _ in range(k)]
                rng = np.random.default_rng(k)
                for v in vecs:
                    sig.part1(v).set(rng.standard_normal(sig.shape1))
                    sig.part2(v).set(rng.standard_normal(sig.shape2))
                outs = [ctx.zeros((sig.nflat,)) for _ in range(k)]
                args = ([sig.part1(v) for v in vecs], [sig.part2(v) for v in vecs])
                kw = dict(out1=[sig.part1(w) for w in outs], out2=[sig.part2(w) for w in outs])
                sig.apply_many(*args, **kw)                            # (warm: pooled temporaries, cached plans)
                ctx.stats(reset=True)
                sig.apply_many(*args, **kw)
                st = ctx.stats(reset=True)
                t = best_of(ctx, lambda: sig.apply_many(*args, **kw), repeat)
                line = "  %s apply k = %d: %.3f ms, %.3e GEMM flops in %d products (%.1f TF/s), floor %.3f ms at the GEMM rate" % (
                    cls.NAME, k, 1e3 * t, st["gemm_flops"], st["gemm_calls"], st["gemm_flops"] / t / 1e12,
                    1e3 * st["gemm_flops"] / gemm_rate)
                if cls is EA_EOM_CCSD and k == 1:
                    line += "; V_abcd %.2f GB, floor %.3f ms at the copy rate" % (8e-9 * nv ** 4, 1e3 * 8.0 * nv ** 4 / copy_rate)
                line += "; %d explicit copies moving %.2f GB" % (st["permute_calls"], st["permute_bytes"] / 1e9)
                emit(line)
            sig.close()
            ctx.trim()
            s = cls(no, n_roots=roots)
            ctx.sync()
            t0 = time.perf_counter()
            e = quiet(s.solve, fd, dressed, res["t2"])
            ctx.sync()
            emit("  %s solve, %d roots: %.3f s, %d passes, converged %s, roots %s, residuals %s, singles weight %s" % (
                cls.NAME, roots, time.perf_counter() - t0, s.iterations, s.converged, np.array2string(e, precision=8),
                np.array2string(s.residual_norms, precision=1), np.array2string(s.singles_weight, precision=3)))
            ctx.trim()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120,50x200")
    ap.add_argument("--roots", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="profiles/ipea/probe_ip_ea.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_ip_ea: synthetic.factors(seed=0), CCSD delta_e = 1e-8, r_epsilon = 1e-6")
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.roots, a.repeat, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
