"""Frozen natural orbitals on the synthetic factors (pymes_amd/model/synthetic.py): the full-space CCSD(T) against
fno_nv = 140 and 100 through the factor path (fno.truncate(..., ("factors", B))), with the preparation time, the CCSD
time per iteration, the (T) time and the energy differences against the full space.  ``--density-only``: just the MP2
density kernel (pymes_fno_density on a V_ijab formed from the factors), timed over --repeat calls, for a kernel trace.
Usage: python tools/probe_fno.py [--size 50x200] [--keep 140,100] [--out profiles/fno/probe_fno.txt]"""
import argparse
import contextlib
import io
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymes_amd.device import Context  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.model import synthetic  # noqa: E402
from pymes_amd.solver import fno  # noqa: E402
from pymes_amd.solver.ccsd import CCSD  # noqa: E402

PEAK = 78.6e12


def solve(no, f, ints):
    """(result, iterations, CCSD seconds, (T) seconds) from the solver's own log lines."""
    s = CCSD(no, delta_e=1e-8)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        r = s.solve(f, ints, triples=True)
    out = log.getvalue()
    def seconds(pattern):
        m = re.search(pattern, out)
        return float(m.group(1)) if m else float("nan")
    t_cc = seconds(r"([\d.]+) seconds spent on ccsd")
    t_t = seconds(r"\(T\) correction = \S+ \(([\d.]+) seconds\)")
    return r, s.iterations, t_cc, t_t


def density_only(no, nv, B, eps, repeat):
    ctx = Context(no, nv)
    try:
        ctx.set_orbital_energies(eps[:no], eps[no:])
        Bov = ctx.array(B[:, :no, no:])
        V = ctx.contract("Qia,Qjb->ijab", Bov, Bov)
        best = None
        for _ in range(repeat):
            ctx.sync()
            t0 = time.perf_counter()
            fno.density(ctx, 0, V)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        flops = 2.0 * no * no * nv ** 3
        print("density (%d,%d): %.3f ms per call (host wall, incl. the symmetry check and the copy of D), %.3e flops "
              "(2 o^2 v^3), %.2f TF/s" % (no, nv, 1e3 * best, flops, flops / best / 1e12))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="50x200")
    ap.add_argument("--keep", default="140,100")
    ap.add_argument("--out", default="profiles/fno/probe_fno.txt")
    ap.add_argument("--density-only", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    no, nv = (int(x) for x in a.size.split("x"))
    B, eps = synthetic.factors(no, nv, seed=0)
    if a.density_only:
        density_only(no, nv, B, eps, a.repeat)
        return
    f = np.diag(eps)
    lines = ["probe_fno (%d,%d), synthetic.factors(seed=0), delta_e = 1e-8; times in seconds" % (no, nv),
             "%6s %9s %9s %9s %6s %9s %20s %12s %12s %12s %12s" % ("nv'", "prep", "ccsd", "ccsd/it", "iter", "(T)",
                                                                   "ccsd(t)+dmp2", "d ccsd", "d (t)", "dmp2",
                                                                   "d total")]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for line in lines:
        print(line)
    ints = DeviceIntegrals.from_factors(no, B)
    try:
        full, it, t_cc, t_t = solve(no, f, ints)
    finally:
        ints.ctx.close()
    e_full = full["ccsd(t) e"]
    emit("%6d %9s %9.3f %9.4f %6d %9.3f %20.12f %12s %12s %12s %12s" % (nv, "-", t_cc, t_cc / max(it, 1), it, t_t, e_full,
                                                                      "0", "0", "0", "0"))
    for k in (int(x) for x in a.keep.split(",")):
        t0 = time.perf_counter()
        r = fno.truncate(no, f, ("factors", B), nv_keep=k)
        prep = time.perf_counter() - t0
        try:
            res, it, t_cc, t_t = solve(r.no, r.fock, r.ints)
        finally:
            r.close()
        tot = res["ccsd(t) e"] + r.de_mp2
        emit("%6d %9.3f %9.3f %9.4f %6d %9s %20.12f %12.3e %12.3e %12.3e %12.3e" % (
            k, prep, t_cc, t_cc / max(it, 1), it, t_t, tot, res["ccsd e"] - full["ccsd e"],
            res["(t) e"] - full["(t) e"], r.de_mp2, tot - e_full))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
