#!/usr/bin/env python3
"""GPU probe of the direct particle ladder of the sector path (``UEG.eval_2b_sectors(..., ladder="direct")``).
Prints JSON lines and appends them to profiles/sector_direct/probe_sector_direct.txt.  Every time is a host clock around
synchronised work, the median of three windows after one untimed pass.

  pair    N = 14 and N = 54 at --cutoff (60: 1 935 plane waves), stored against direct: ``eval_2b_sectors``; the ladder launch
          alone (--reps launches per window); ms per DCD iteration (two solves that cannot converge, with different iteration
          caps, the difference divided); integrals plus a converged DCD solve (delta_e 1e-7), end to end; device bytes
  big     N = 54 at --big-cutoff (150: 7 809 plane waves) with the direct ladder, Coulomb and transcorrelated
          (only_2b + effect_2b, trunc with k_cutoff 1): ms per DCD iteration, the ladder launch, the DCD energy, device bytes next
          to the bytes a stored abcd block would take (arithmetic from the tables)
    python3 tools/probe_sector_direct.py [--part pair,big] [--nel 14,54] [--cutoff 60] [--big-cutoff 150] [--iters 5] [--reps 5]"""
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
from pymes_amd.solver.ueg_cc import SectorCCD  # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def windows(ctx, work, n=3, warm=True):
    """Median seconds of n windows of ``work()``, each closed by a synchronisation."""
    if warm:
        work()
        ctx.sync()
    times = []
    for _ in range(n):
        ctx.sync()
        t0 = time.perf_counter()
        work()
        ctx.sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def per_iteration(ctx, solve, iters):
    """ms per iteration: (median time of 1 + iters passes) - (median time of 1 pass), divided."""
    short = windows(ctx, lambda: quiet(solve, 1))
    long_ = windows(ctx, lambda: quiet(solve, 1 + iters), warm=False)
    return 1e3 * (long_ - short) / iters


def basis(nel, cutoff, k_cutoff=None):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    m.k_cutoff, m.gamma = k_cutoff, None
    return m, np.array([b.kinetic for b in m.basis_fns[::2]])


def ladder_ms(ctx, ints, reps):
    tab, dt = ints.tables, ints.device_tables()
    T, R = ctx.array(np.random.default_rng(0).standard_normal(tab.nnz)), ctx.zeros((tab.nnz,))

    def work():
        for _ in range(reps):
            ints.ladder(dt.ladder, T, R)
    return 1e3 * windows(ctx, work) / reps


def part_pair(ctx, nel, cutoff, iters, reps):
    m, kin = basis(nel, cutoff)
    tab = m.sector_tables()
    no = nel // 2
    out = {"part": "pair", "nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "nnz": tab.nnz, "max_vv": int(tab.n_vv.max()),
           "max_oo": int(tab.n_oo.max()), "abcd_elements": int(tab.block_offsets("abcd")[-1])}
    energies = {}
    for ladder in ("stored", "direct"):
        held = {}

        def build():
            held.clear()                         # (the previous window's integrals go back to the context first)
            held["ints"] = quiet(m.eval_2b_sectors, tab, ctx=ctx, ladder=ladder)
        out[ladder + "_eval_2b_sectors_s"] = round(windows(ctx, build, warm=False), 4)
        ints = held["ints"]
        eps = ints.hf_orbital_energies(kin)
        out[ladder + "_device_bytes"] = ints.nbytes
        out[ladder + "_ladder_ms"] = round(ladder_ms(ctx, ints, reps), 4)
        out[ladder + "_dcd_ms_per_iteration"] = round(
            per_iteration(ctx, lambda cap: SectorCCD(no, is_dcd=True, delta_e=0.0).solve(eps, ints, max_iter=cap), iters), 4)
        solver = SectorCCD(no, is_dcd=True, delta_e=1e-7)
        res = {}

        def solve():
            res["e"] = quiet(solver.solve, eps, ints)["ccd e"]
        out[ladder + "_converged_dcd_solve_s"] = round(windows(ctx, solve), 4)
        out[ladder + "_dcd_iterations"], energies[ladder] = solver.iterations, res["e"]
        out[ladder + "_end_to_end_s"] = round(out[ladder + "_eval_2b_sectors_s"] + out[ladder + "_converged_dcd_solve_s"], 4)
        held.clear()
        del ints
    out["dcd_energy"], out["energies_equal"] = energies["stored"], energies["stored"] == energies["direct"]
    out["ladder_direct_over_stored"] = round(out["direct_ladder_ms"] / out["stored_ladder_ms"], 3)
    out["end_to_end_direct_over_stored"] = round(out["direct_end_to_end_s"] / out["stored_end_to_end_s"], 4)
    return out


def part_big(ctx, nel, cutoff, iters, reps):
    lines = []
    m, kin = basis(nel, cutoff, k_cutoff=1.0)
    t0 = time.perf_counter()
    tab = m.sector_tables()
    t_tab = time.perf_counter() - t0
    no = nel // 2
    for kind in ("coulomb", "transcorrelated"):
        t0 = time.perf_counter()
        if kind == "coulomb":
            ints = quiet(m.eval_2b_sectors, tab, ctx=ctx, ladder="direct")
            eps = ints.hf_orbital_energies(kin)
        else:
            v2 = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_only_2b=True, ctx=ctx, ladder="direct")
            eps = v2.hf_orbital_energies(kin) + quiet(m.double_contractions_in_3_body)
            ints = v2 + quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_effect_2b=True, ctx=ctx, ladder="direct")
            del v2
        ctx.sync()
        t_int = time.perf_counter() - t0
        ms = per_iteration(ctx, lambda cap: SectorCCD(no, is_dcd=True, delta_e=0.0).solve(eps, ints, max_iter=cap), iters)
        solver = SectorCCD(no, is_dcd=True, delta_e=1e-7)
        t0 = time.perf_counter()
        e = quiet(solver.solve, eps, ints)["ccd e"]
        ctx.sync()
        t_solve = time.perf_counter() - t0
        lines.append({"part": "big", "kind": kind, "nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "nnz": tab.nnz,
                      "max_vv": int(tab.n_vv.max()), "tables_s": round(t_tab, 2), "integrals_s": round(t_int, 2),
                      "device_bytes": ints.nbytes, "term_bytes": ints.nbytes - 8 * ints.total,
                      "stored_abcd_bytes_would_be": 8 * int(tab.block_offsets("abcd")[-1]),
                      "ladder_ms": round(ladder_ms(ctx, ints, reps), 3), "dcd_ms_per_iteration": round(ms, 3),
                      "dcd_energy": e, "dcd_iterations": solver.iterations, "converged_dcd_solve_s": round(t_solve, 3)})
        del ints
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="pair,big")
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--big-cutoff", type=int, default=150)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_direct", "probe_sector_direct.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(line):
        text = json.dumps(line, default=lambda x: x.item())         # (numpy scalars)
        print(text, flush=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    ctx = Context(1, 1, device=0)
    try:
        if "pair" in args.part:
            for nel in (int(x) for x in args.nel.split(",")):
                emit(part_pair(ctx, nel, args.cutoff, args.iters, args.reps))
        if "big" in args.part:
            for line in part_big(ctx, 54, args.big_cutoff, args.iters, args.reps):
                emit(line)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
