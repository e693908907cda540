"""Wall time of the (T) correction (pymes_ccsd_t) on synthetic factors with random amplitudes: seconds, executed flops
N_triples * 12 v^3 (v + o) (six particle products of 2 v^4 and six hole products of 2 o v^3 per triple), TF/s and the share of
the 78.6-TF fp64 MFMA peak of the MI355X.  Usage: python tools/probe_triples.py [--sizes 20x80,30x120,50x200] [--batch N]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.io_oracle import synthetic_factors  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.solver import ccsd_t  # noqa: E402

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20x80,30x120,50x200")
    ap.add_argument("--batch", type=int, default=0, help="PYMES_TRIPLES_BATCH (0: the library's default)")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    if a.batch:
        os.environ["PYMES_TRIPLES_BATCH"] = str(a.batch)
    print("%8s %10s %10s %12s %8s %7s %22s" % ("(o,v)", "triples", "seconds", "flops", "TF/s", "peak", "E(T)"))
    for spec in a.sizes.split(","):
        no, nv = (int(x) for x in spec.split("x"))
        B, eps = synthetic_factors(no, nv, seed=0, scale=0.3)
        rng = np.random.default_rng(1)
        t1 = rng.standard_normal((nv, no)) * 0.02
        t2 = rng.standard_normal((nv, nv, no, no)) * 0.02
        t2 = 0.5 * (t2 + t2.transpose(1, 0, 3, 2))
        ints = DeviceIntegrals.from_factors(no, B)
        ctx = ints.ctx
        d1, d2 = ctx.array(t1), ctx.array(t2)
        del t2
        n = ccsd_t.n_triples(no)
        flops = n * 12.0 * nv ** 3 * (nv + no)
        best, e = None, None
        for _ in range(a.repeat):
            ctx.sync()
            t0 = time.perf_counter()
            e = ccsd_t.get_triples_energy(no, np.diag(eps), ints, d1, d2)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        print("%8s %10d %10.3f %12.4e %8.2f %6.1f%% %22.14e" % ("(%d,%d)" % (no, nv), n, best, flops, flops / best / 1e12,
                                                              100.0 * flops / best / PEAK, e), flush=True)
        d1.free()
        d2.free()
        ctx.close()


if __name__ == "__main__":
    main()
