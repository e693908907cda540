#!/usr/bin/env python3
"""GPU probe of the sector densities (pymes_amd/solver/ueg_cc.py, SectorDensity).  Prints JSON lines and appends
them to profiles/sector_density/probe_sector_density.txt, one line per --nel at --cutoff (default 60: 1 935 plane waves), all
from one run with Coulomb integrals, converged DCD amplitudes and their Lambda:
  build        ms per density build (gamma and every stored family of G) next to ms per Lambda iteration of the same run
               (the difference of a long and a short solve after a warm-up solve, smallest of three, as
               tools/probe_sector_lambda.py windows it); the build is the median of --reps windows of back-to-back builds
               that fill 0.3 s with one synchronisation at the end;
  expectation  ms per expectation(ints) (the dots, the ladder launch, the download of W's w1 block for the symmetry check and
               of its Fock lists) next to ms per amplitude iteration;
  transfer     the two S(q) kernels on their own, windows of the same kind: pymes_sector_bin_sums over all stored families
               (one launch each) with the bytes it must move (8 B of source and 8 B of index per element, 8 B per bin and
               family), and pymes_sector_pair_transfer with the bytes it cannot avoid (both compact vectors once, the row tables
               once) -- it re-reads them for every bin through the caches, so its fraction of HBM says how far a
               lookup-bound kernel is from a streaming one, not how well it streams; both at the 6.3 TB/s this project uses;
  values       n(k) on the two sides of the Fermi surface, S(q) on the smallest shells, "density e" next to the DCD energy.
All times are host clocks around work that ends in a synchronisation: launch and synchronisation overhead is inside.
    python3 tools/probe_sector_density.py [--nel 14,54] [--cutoff 60] [--iters 50] [--reps 3]"""
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
from pymes_amd.solver.ueg_cc import SectorCCD, SectorLambda, sector_density  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
WINDOW_S = 0.3


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def per_iteration(solve, iters):
    """ms per iteration: (time of 1 + iters passes) - (time of 1 pass), after one untimed solve; smallest of three each."""
    def run(cap):
        t0 = time.perf_counter()
        quiet(solve, cap)
        return time.perf_counter() - t0
    run(1)
    short, long_ = min(run(1) for _ in range(3)), min(run(1 + iters) for _ in range(3))
    return 1e3 * (long_ - short) / iters


def windows(f, ctx, reps):
    """(ms per call: median of `reps` windows, calls per window, all windows)."""
    def window(n):
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        ctx.sync()
        return (time.perf_counter() - t0) / n
    f()
    ctx.sync()
    inner = max(1, int(np.ceil(WINDOW_S / window(1))))
    ts = [1e3 * window(inner) for _ in range(reps)]
    return round(statistics.median(ts), 4), inner, [round(t, 4) for t in ts]


def run(ctx, nel, cutoff, iters, reps):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    tab = m.sector_tables()
    no = tab.no
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    out = {"nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "no": no, "nv": tab.nv, "nnz": tab.nnz}
    ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
    eps = ints.hf_orbital_energies(kin)
    solver = SectorCCD(no, is_dcd=True, delta_e=1e-9)
    res = quiet(solver.solve, eps, ints, max_iter=100)
    T = res["t2 amp"]
    left = quiet(SectorLambda(no, 1e-8, is_dcd=True).solve, eps, ints, T)
    lam = left["lambda2"]
    amp_ms = per_iteration(lambda cap: SectorCCD(no, is_dcd=True, delta_e=0.0).solve(eps, ints, max_iter=cap), iters)
    lam_ms = per_iteration(lambda cap: SectorLambda(no, 0.0, is_dcd=True).solve(eps, ints, T, max_iter=cap), iters)
    t0 = time.perf_counter()
    dens = sector_density(eps, ints, T, lam, is_dcd=True)
    ctx.sync()
    first = time.perf_counter() - t0
    b_ms, b_n, b_all = windows(lambda: sector_density(eps, ints, T, lam, is_dcd=True), ctx, reps)
    out["build"] = {"density_build_ms": b_ms, "builds_per_window": b_n, "density_build_ms_all": b_all,
                    "first_build_s_with_task_tables": round(first, 3), "lambda_ms_per_iteration": round(lam_ms, 4),
                    "ratio_to_lambda_iteration": round(b_ms / lam_ms, 3), "stored_density_bytes": 8 * dens.arena.size,
                    "note": "each build also uploads T and lambda and checks their symmetry on the host"}
    value = {}

    def expect():
        value["e"] = dens.expectation(ints, one_body=kin)
    e_ms, e_n, e_all = windows(expect, ctx, reps)
    out["expectation"] = {"expectation_ms": e_ms, "calls_per_window": e_n, "expectation_ms_all": e_all,
                          "amplitude_ms_per_iteration": round(amp_ms, 4), "ratio_to_amplitude_iteration": round(e_ms / amp_ms, 3)}
    t0 = time.perf_counter()
    tb = dens.bins()
    dens._bin_tables()
    ctx.sync()
    t_bins = time.perf_counter() - t0
    stored, pair = ctx.empty((tb.nbins,)), ctx.empty((tb.nbins,))
    s_ms, s_n, s_all = windows(lambda: dens.stored_transfer(stored), ctx, reps)
    p_ms, p_n, p_all = windows(lambda: dens.pair_transfer(pair), ctx, reps)
    elements = int(sum(dens.sizes[nm] for nm in dens.FAMILIES))
    s_bytes = 16 * elements + 8 * tb.nbins * len(dens.FAMILIES)
    rows = int(tab.n_vv.sum())
    p_bytes = 16 * tab.nnz + rows * (8 + 8 + 8) + 8 * tab.nv * tab.nv + 8 * tb.nbins
    out["transfer"] = {"bins": tb.nbins, "bins_and_lists_host_s": round(t_bins, 3),
                       "bin_sums_ms": s_ms, "bin_sums_launches": len(dens.FAMILIES), "bin_sums_elements": elements,
                       "bin_sums_bytes": s_bytes, "bin_sums_fraction_of_hbm": round(s_bytes / (1e-3 * s_ms) / HBM_BYTES_PER_S, 4),
                       "bin_sums_ms_all": s_all, "bin_sums_calls_per_window": s_n,
                       "pair_transfer_ms": p_ms, "pair_rows": rows, "pair_transfer_lookups": tb.nbins * rows,
                       "pair_transfer_compulsory_bytes": p_bytes,
                       "pair_transfer_fraction_of_hbm": round(p_bytes / (1e-3 * p_ms) / HBM_BYTES_PER_S, 6),
                       "pair_transfer_ms_all": p_all, "pair_transfer_calls_per_window": p_n}
    n_k = dens.momentum_distribution()
    S, q2 = dens.structure_factor(shells=True)
    order = np.argsort(kin, kind="stable")
    out["values"] = {"dcd_energy": res["ccd e"], "dcd_iterations": solver.iterations, "lambda_residual": left["lambda residual"],
                     "density_e": dens.lagrangian(eps, ints), "expectation_ints_kinetic": value["e"],
                     "trace_n_k_minus_N": float(n_k.sum() - nel),
                     "n_k_below_fermi": [round(float(x), 8) for x in n_k[order[max(no - 3, 0):no]]],
                     "n_k_above_fermi": [round(float(x), 8) for x in n_k[order[no:no + 3]]],
                     "shell_q2": [int(x) for x in q2[:6]], "S_on_shells": [round(float(x), 8) for x in S[:6]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_density", "probe_sector_density.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for nel in (int(x) for x in args.nel.split(",")):
        ctx = Context(1, 1, device=0)
        try:
            line = json.dumps(run(ctx, nel, args.cutoff, args.iters, args.reps))
        finally:
            ctx.close()
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
