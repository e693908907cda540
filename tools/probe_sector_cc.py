#!/usr/bin/env python3
"""GPU probe of the momentum-sector CCD / DCD path (pymes_amd/solver/ueg_cc.py).  Prints JSON lines and writes
profiles/sector/probe_sector_cc.txt:
  small   ms per DCD iteration of the sector path next to the dense ``CCD`` class at N = 14, cutoff 5 and 8 (57 and 93 plane
          waves): two solves that cannot converge (delta_e = 0) with different iteration caps, the difference divided;
  big     a basis the dense path cannot hold (N = 14, --cutoff 60: about 1 950 plane waves): the integral build time, the
          bytes held, ms per DCD iteration, the ladder launch alone (host-timed with a synchronisation, --reps times) as bytes
          of V_abcd per second against the 6.3 TB/s this project uses for HBM, and the library calls per iteration.
    python3 tools/probe_sector_cc.py [--part small,big] [--cutoff 60] [--nel 14] [--iters 10] [--reps 5]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from pymes_amd.device import Context  # noqa: E402
from pymes_amd.model.ueg import UEG  # noqa: E402
from pymes_amd.solver.ccd import CCD  # noqa: E402
from pymes_amd.solver.ueg_cc import SectorCCD  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def per_iteration(solve, iters):
    """ms per iteration: (time of 2 + iters passes) - (time of 2 passes), after one untimed solve."""
    def run(cap):
        t0 = time.perf_counter()
        quiet(solve, cap)
        return time.perf_counter() - t0
    run(1)
    short, long_ = min(run(1) for _ in range(3)), min(run(1 + iters) for _ in range(3))
    return 1e3 * (long_ - short) / iters


def sector_problem(ctx, nel, cutoff):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    t0 = time.perf_counter()
    tab = m.sector_tables()
    t_tab = time.perf_counter() - t0
    t0 = time.perf_counter()
    ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
    ctx.sync()
    t_int = time.perf_counter() - t0
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    return m, tab, ints, ints.hf_orbital_energies(kin), kin, t_tab, t_int


def part_small(ctx, iters):
    out = []
    for cutoff in (5, 8):
        m, tab, ints, eps, kin, _, _ = sector_problem(ctx, 14, cutoff)
        sector = per_iteration(lambda cap: SectorCCD(7, is_dcd=True, delta_e=0.0).solve(eps, ints, max_iter=cap), iters)
        V = quiet(m.eval_2b_integrals)
        f = np.diag(eps)
        dense = per_iteration(lambda cap: CCD(7, is_dcd=True, delta_e=0.0).solve(f, V, max_iter=cap), iters)
        out.append({"part": "small", "nel": 14, "cutoff": cutoff, "plane_waves": tab.n, "nnz": tab.nnz,
                    "sector_ms_per_iteration": round(sector, 4), "dense_ms_per_iteration": round(dense, 4),
                    "note": "dense figure includes nothing but the loop: both solves upload the same integrals"})
    return out


def part_big(ctx, nel, cutoff, iters, reps):
    m, tab, ints, eps, kin, t_tab, t_int = sector_problem(ctx, nel, cutoff)
    no = nel // 2
    calls = {"n": 0}
    lib_call = ctx.lib.call

    def counting(name, *a):
        calls["n"] += 1
        return lib_call(name, *a)
    solve = lambda cap: SectorCCD(no, is_dcd=True, delta_e=0.0).solve(eps, ints, max_iter=cap)
    ms = per_iteration(solve, iters)
    ctx.lib.call = counting
    try:
        calls["n"] = 0
        quiet(solve, 1)
        two = calls["n"]
        calls["n"] = 0
        quiet(solve, 1 + iters)
        per_iter_calls = (calls["n"] - two) / iters
    finally:
        del ctx.lib.call
    # the ladder launch alone
    dt = ints.device_tables()
    T, R = ctx.array(np.random.default_rng(0).standard_normal(tab.nnz)), ctx.zeros((tab.nnz,))
    dt.ladder.run(ints["abcd"], T, R)
    ctx.sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dt.ladder.run(ints["abcd"], T, R)
        ctx.sync()
        times.append(time.perf_counter() - t0)
    abcd_bytes = 8 * ints.sizes["abcd"]
    rate = abcd_bytes / statistics.median(times)
    converged = SectorCCD(no, is_dcd=True, delta_e=1e-7)
    e = quiet(converged.solve, eps, ints)
    return [{"part": "big", "nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "nnz": tab.nnz,
             "dense_T2_elements": tab.nv ** 2 * no ** 2, "dense_V_bytes": 8 * tab.n ** 4, "pp_sectors": len(tab.P_keys),
             "ph_sectors": len(tab.q_keys), "max_vv": int(tab.n_vv.max()), "tables_s": round(t_tab, 3),
             "integral_build_s": round(t_int, 3), "integral_bytes": ints.nbytes, "abcd_bytes": abcd_bytes,
             "ms_per_iteration": round(ms, 3), "library_calls_per_iteration": per_iter_calls,
             "ladder_ms": round(1e3 * statistics.median(times), 4), "ladder_tiles": dt.ladder.tiles,
             "ladder_bytes_per_s": rate, "ladder_fraction_of_hbm": round(rate / HBM_BYTES_PER_S, 4),
             "dcd_energy": e["ccd e"], "dcd_iterations": converged.iterations}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="small,big")
    ap.add_argument("--nel", type=int, default=14)
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector", "probe_sector_cc.txt"))
    args = ap.parse_args()
    ctx = Context(1, 1, device=0)
    lines = []
    try:
        if "small" in args.part:
            lines += part_small(ctx, args.iters)
        if "big" in args.part:
            lines += part_big(ctx, args.nel, args.cutoff, args.iters, args.reps)
    finally:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            for ln in lines:
                print(json.dumps(ln))
                fh.write(json.dumps(ln) + "\n")
        ctx.close()


if __name__ == "__main__":
    main()
