"""Wall time of Lambda-CCSD(T) (pymes_ccsd_t_lambda) next to (T) (pymes_ccsd_t), in one process on the same triple ranges:
synthetic factors, random amplitudes and a random Lambda.  Two ranges of n1 and n2 triples from the middle of the list are
timed for each; the slope is the cost per triple, the intercept what a call does once (checks, permuted amplitudes, and for
Lambda-(T) the two o v^3 copies of V_abic), and intercept + slope * N_triples the extrapolation to all triples.  A second pass
with the GEMM event timers on (pymes_prof_*) splits the per-triple cost of that pass into the matrix-core products and the rest
(the energy kernel, launch gaps); a kernel trace is the finer instrument (profiles/lambda_triples).  Usage: python tools/probe_lambda_triples.py [--sizes 30x120,50x200] [--n1 1000] [--n2 4000] [--batch N]
[--methods t,lambda]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.io_oracle import synthetic_factors  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.solver import ccsd_t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120,50x200")
    ap.add_argument("--n1", type=int, default=1000)
    ap.add_argument("--n2", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=0, help="PYMES_TRIPLES_BATCH (0: the library's defaults)")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--methods", default="t,lambda", help="t, lambda or both (one alone: for a kernel trace of that call)")
    a = ap.parse_args()
    if a.batch:
        os.environ["PYMES_TRIPLES_BATCH"] = str(a.batch)
    print("%9s %10s %8s %12s %11s %13s %10s %10s" % ("(o,v)", "method", "triples", "ms / triple", "once (s)", "all triples (s)",
                                                     "products", "rest"))
    for spec in a.sizes.split(","):
        no, nv = (int(x) for x in spec.split("x"))
        B, eps = synthetic_factors(no, nv, seed=0, scale=0.3)
        rng = np.random.default_rng(1)

        def sym(x):
            return 0.5 * (x + x.transpose(1, 0, 3, 2))
        ints = DeviceIntegrals.from_factors(no, B)
        ctx = ints.ctx
        d1 = ctx.array(rng.standard_normal((nv, no)) * 0.02)
        d2 = ctx.array(sym(rng.standard_normal((nv, nv, no, no)) * 0.02))
        l1 = ctx.array(rng.standard_normal((nv, no)) * 0.04)
        l2 = ctx.array(sym(rng.standard_normal((nv, nv, no, no)) * 0.04))
        f = np.diag(eps)
        n = ccsd_t.n_triples(no)
        n1, n2 = min(a.n1, n // 4), min(a.n2, n // 2)
        lo = n // 2
        calls = {"(T)": lambda hi: ccsd_t.get_triples_energy(no, f, ints, d1, d2, triple_range=(lo, hi)),
                 "Lambda-(T)": lambda hi: ccsd_t.get_lambda_triples_energy(no, f, ints, d2, l1, l2, triple_range=(lo, hi))}
        calls = {name: call for name, call in calls.items() if ("lambda" if "Lambda" in name else "t") in a.methods.split(",")}
        for call in calls.values():
            call(lo + 8)                                  # warm-up: code objects, the allocator
        counts = (n1, n2)
        wall = {name: [None, None] for name in calls}
        for _ in range(a.repeat):                         # the two methods alternate: a drift of the clocks hits both
            for z, cnt in enumerate(counts):
                for name, call in calls.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    call(lo + cnt)
                    dt = time.perf_counter() - t0
                    wall[name][z] = dt if wall[name][z] is None else min(wall[name][z], dt)
        total = {}
        for name, call in calls.items():
            # the event pass: its own wall time is the base of the shares (the event pairs slow the host down)
            pwall, gemm = [], []
            ctx.prof_enable(True)
            for cnt in counts:
                ctx.prof_reset()
                ctx.sync()
                t0 = time.perf_counter()
                call(lo + cnt)
                pwall.append(time.perf_counter() - t0)
                gemm.append(ctx.prof_query(0)["ms"] * 1e-3)
            ctx.prof_enable(False)
            slope = (wall[name][1] - wall[name][0]) / (n2 - n1)
            once = wall[name][0] - slope * n1
            share = (gemm[1] - gemm[0]) / (pwall[1] - pwall[0])
            total[name] = once + slope * n
            print("%9s %10s %8d %12.4f %11.3f %13.2f %9.1f%% %9.1f%%" % ("(%d,%d)" % (no, nv), name, n, 1e3 * slope, once,
                                                                       total[name], 100.0 * share, 100.0 * (1.0 - share)),
                  flush=True)
        if len(total) == 2:
            print("%9s Lambda-(T) / (T), all triples: %.3f" % ("(%d,%d)" % (no, nv), total["Lambda-(T)"] / total["(T)"]),
                  flush=True)
        for d in (d1, d2, l1, l2):
            d.free()
        ctx.close()


if __name__ == "__main__":
    main()
